"""The certified bf16 shortlist search on the device (include/ffrnet.h: ffr_coarse_pack, ffr_search_topk_coarse;
ffrnet_amd.search.Gallery(coarse=True)).

The oracle is the exact search, Engine.search: every comparison is torch.equal on scores and indices, no tolerance.  Equality
alone would pass if every probe fell back to the exact search, so the certified share is asserted where the CPU model of
tests/search_coarse_ref.py says what it must be."""
import ctypes as C

import pytest
import torch

import ffrnet_amd
import search_coarse_ref as ref
from ffrnet_amd import native
from ffrnet_amd.search import COARSE_EPS, Gallery, shortlist_size

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


def cpu_rows(n, seed):
    return torch.randn((n, 512), generator=torch.Generator().manual_seed(seed))


def rand_rows(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn((n, 512), device='cuda', generator=g)


def corr_rows(n, seed, base_seed=77):
    """Strongly correlated rows, base + 0.05 * noise: every cosine between two of them is within 2 * COARSE_EPS of every
    other, the case a shortlist cannot separate."""
    return rand_rows(1, base_seed) + 0.05 * rand_rows(n, seed)


def cpu_corr(n, seed, base_seed=77):
    return cpu_rows(1, base_seed) + 0.05 * cpu_rows(n, seed)


@pytest.fixture(scope='module')
def real_rows(state_dicts):
    """f_new (masked-probe side) and f (enrolment side) of 512 synthetic images: 1024 real embeddings, [f_new ..., f ...] --
    the recipe of tests/test_gpu_search.py."""
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    outs = []
    for s in range(2):
        x = ffrnet_amd.synth.synth_images(256, seed=900 + s).cuda()
        f_new, f = e.embed(x)
        outs += [f_new, f]
    torch.cuda.synchronize()
    e.close()
    return torch.cat(outs[0::2] + outs[1::2], 0)


def real_family(real_rows, Q, G):
    """Masked-side probes against the enrolments, then the masked side, then all of it again: row j of the gallery is row
    j % 1024 of [f ..., f_new ...].  Up to 1536 rows that is the gallery of tests/test_gpu_search.py; beyond, the 1024
    embeddings repeat, so at G = 65537 every row has 64 exact copies (more than any k'), spread over every chunk, and every
    probe is itself enrolled 64 times: exact score ties across the shortlist edge, the chunk-list merge and the live-count
    exact pass, on real embedding geometry."""
    q = real_rows[(37 * torch.arange(Q, device='cuda')) % 512]
    pool = torch.cat((real_rows[512:], real_rows[:512]), 0)
    return q, pool[torch.arange(G, device='cuda') % 1024]


def coarse_gallery(eng, g):
    gal = Gallery(eng, coarse=True)
    gal.add(g)
    return gal


def check_equal(eng, gal, q, k, **kw):
    """gal.search == Engine.search over the same rows -> the certified flags [Q] (bool, on the host)."""
    s, i = gal.search(q, k, **kw)
    es, ei = eng.search(q, gal.embeddings, k, gallery_norms=gal.norms, **kw)
    torch.cuda.synchronize()
    assert s.shape == es.shape and torch.equal(s, es) and torch.equal(i, ei)
    cert = gal.last_certified
    assert cert.shape == (q.size(0),) and cert.dtype == torch.int32 and bool(((cert == 0) | (cert == 1)).all())
    return cert.bool().cpu()


CASES = [(1, 1000, 1), (31, 1000, 10), (33, 65537, 10), (32, 65537, 64), (257, 4096, 10), (32, 10, 10), (31, 1, 1),
         (5, 200, 65), (4, 0, 10)]


@pytest.mark.parametrize('data', ['rand', 'real', 'corr'])
@pytest.mark.parametrize('Q,G,k', CASES)
def test_equals_the_exact_search(eng, real_rows, Q, G, k, data):
    """The nine cases on Gaussian rows, on the real_rows recipe (real_family) and, beside them, on base + 0.05 * noise."""
    if data == 'real':
        q, g = real_family(real_rows, Q, G)
    else:
        rows = rand_rows if data == 'rand' else corr_rows
        q, g = rows(Q, 11 * Q + k), rows(G, 7 * G + 1)
    gal = coarse_gallery(eng, g)
    cert = check_equal(eng, gal, q, k)
    kp = shortlist_size(k)
    if k > 64 or G == 0:
        assert not bool(cert.any())              # the exact search alone
    elif G <= kp:
        assert bool(cert.all())                  # the shortlist is the gallery
    elif kp < 128:
        # A certificate says that every row outside the k' of the shortlist scores strictly below the k-th, so a probe with
        # more than k' rows at or above its k-th exact score cannot hold one.  The exact top 128 counts up to 128 of them.
        es, _ = eng.search(q, g, 128, gallery_norms=gal.norms)
        must_fall_back = ((es >= es[:, k - 1:k]).sum(1) > kp).cpu()
        print('%s: certified %d, more than k\' = %d rows tie or beat the k-th for %d, of %d probes'
              % (data, int(cert.sum()), kp, int(must_fall_back.sum()), Q))
        assert not bool((cert & must_fall_back).any())
        if data == 'real' and G == 65537:
            # every probe is enrolled 64 times > k' = 32, and nothing beats the cosine of a row with itself by more than
            # the 1e-6 of the fp32 score: short of 10 other embeddings within 2e-6 of parallel to a probe, its 64 copies
            # reach the top 10.  Asked of one probe only, so that the exact pass over live probes certainly ran here.
            assert bool(must_fall_back.any())


def test_exact_score_does_not_depend_on_the_place_in_a_tile(eng):
    """The exact score of one (q, g) pair has the same bits at each of the 128 places of a step's tile, in every chunk: what
    the re-score of a shortlist relies on when it scores a row elsewhere than the search did, and what include/ffrnet.h
    promises of sharding.  |q||g| runs from 1e-4 to 1e-1 here, where the 1e-8 of the denominator is many units in the last
    place of the product, so a denominator rounded once in some places and twice in others shows."""
    x = cpu_rows(1, 91)
    x = 0.1 * x / x.norm()
    scale = torch.logspace(-3, 0, 33)[:, None]
    q = ((x + 0.01 * cpu_rows(33, 92) / 22.6) * scale / 0.1).cuda()
    s0, i0 = eng.search(q, x.expand(128, 512).contiguous().cuda(), 128)
    assert torch.equal(i0, torch.arange(128, device='cuda').expand(33, 128)) and torch.equal(s0, s0[:, :1].expand(33, 128))
    g = 0.1 * cpu_rows(70000, 93) / 22.6                 # cosines of about 0.05 with the probes, against 0.99 of the copies
    where = 11 + 517 * torch.arange(128)                 # 517 = 5 mod 128: every place of a tile once, rows up to 65670
    g[where] = x
    s, i = eng.search(q, g.cuda(), 128)
    assert torch.equal(i.cpu(), where.expand(33, 128)) and torch.equal(s, s0)


@pytest.fixture(scope='module')
def cpu_gallery():
    return cpu_rows(65537, 101)


@pytest.mark.parametrize('Q,k,seed', [(33, 10, 102), (32, 64, 103)])
def test_gaussian_rows_certify(eng, cpu_gallery, Q, k, seed):
    """Rows drawn on the CPU from fixed seeds: the CPU model, with eps widened by 3e-4, needs at most 21 of 32 (k = 10)
    and 107 of 128 (k = 64) shortlist slots on these very rows, so every probe certifies in the model; the device, whose coarse scores differ from
    the model's only in the rounding of the accumulation, must certify >= 90 %."""
    q = cpu_rows(Q, seed)
    cert = check_equal(eng, coarse_gallery(eng, cpu_gallery.cuda()), q.cuda(), k)
    print('certified %d of %d' % (int(cert.sum()), Q))
    assert int(cert.sum()) >= 0.9 * Q


def test_correlated_rows_do_not_certify_and_mixed_batches_split(eng):
    g, q = corr_rows(65537, 5), corr_rows(33, 6)
    assert not bool(check_equal(eng, coarse_gallery(eng, g), q, 10).any())
    # both kinds in one gallery and one batch: the Gaussian probes certify, the correlated ones do not (the CPU model on
    # these rows: at most 18 of 32 slots for the first 16 probes, 3001 for the others)
    g = torch.cat((cpu_rows(20000, 111), cpu_corr(3000, 7)), 0).cuda()
    q = torch.cat((cpu_rows(16, 112), cpu_corr(16, 8)), 0).cuda()
    gal = coarse_gallery(eng, g)
    cert = check_equal(eng, gal, q, 10)
    assert bool(cert[:16].all()) and not bool(cert[16:].any()), cert.tolist()
    s, i = gal.search(q, 10)
    for r in range(32):
        sr, ir = gal.search(q[r:r + 1], 10)
        assert torch.equal(sr[0], s[r]) and torch.equal(ir[0], i[r]) and bool(gal.last_certified[0]) == bool(cert[r]), r


def test_ties_across_the_shortlist_edge(eng):
    g = rand_rows(3000, 5)
    copies = torch.randperm(3000, generator=torch.Generator().manual_seed(9))[:40].sort().values
    g[copies.cuda()] = g[900].clone()
    q = g[900:901] * 0.5 + rand_rows(1, 6) * 1e-3
    # 40 equal rows > k' = 32: the shortlist cannot hold them all, c_k' ties s_k up to rounding, no certificate
    gal = coarse_gallery(eng, g)
    cert = check_equal(eng, gal, q, 2)
    s, i = gal.search(q, 2)
    assert not bool(cert.any()) and i[0].tolist() == copies[:2].tolist() and s[0, 0] == s[0, 1]
    # 4 copies, k = 10: certified, the copies first, by ascending index with equal scores
    g = cpu_rows(3000, 5).cuda()
    for dst in (17, 2500, 40):
        g[dst] = g[900]
    q = g[900:901] * 0.5 + rand_rows(1, 6) * 1e-3
    gal = coarse_gallery(eng, g)
    cert = check_equal(eng, gal, q, 10)
    s, i = gal.search(q, 10)
    assert bool(cert.all()) and i[0, :4].tolist() == [17, 40, 900, 2500] and torch.equal(s[0, :4], s[0, :1].expand(4))


def test_worst_case_rounding(eng):
    """Rows whose every element rounds up by nearly the whole unit round-off (search_coarse_ref.midpoint_row, shuffled and
    rescaled), against an all-ones probe: the coarse scores of these rows err by 0.93 u, all the same way."""
    gen = torch.Generator().manual_seed(21)
    mid = torch.stack([ref.midpoint_row()[torch.randperm(512, generator=gen)] * (0.5 + i) for i in range(8)])
    g = cpu_rows(3000, 22)
    where = torch.tensor([5, 130, 131, 999, 1500, 2047, 2048, 2999])
    g[where] = mid
    q = torch.cat((torch.ones((1, 512)), 3.0 * torch.ones((1, 512)), cpu_rows(3, 23)), 0)
    err = (ref.coarse_scores(q[:1], mid).double() - ref.exact_scores(q[:1], mid).double()).abs().max().item()
    print('model: largest |coarse - exact| on the midpoint rows = %.6f = %.3f u (eps = %.6f)' % (err, err * 256, COARSE_EPS))
    assert 0.9 * 2.0 ** -8 <= err <= COARSE_EPS
    gal = coarse_gallery(eng, g.cuda())
    for k in (1, 2, 8, 10, 64):
        cert = check_equal(eng, gal, q.cuda(), k)
        print('k = %d: certified %s' % (k, cert.int().tolist()))
    s, i = gal.search(q.cuda(), 8)
    assert torch.equal(i[0].sort().values.cpu(), where) and torch.equal(i[1].sort().values.cpu(), where)


def test_unsafe_norms(eng):
    g = rand_rows(500, 31)
    g[7] *= 1e-30                     # every square underflows: norm 0 over a row that is not zero
    g[9] = 0.0
    q = torch.cat((rand_rows(4, 32), g[7:8] * 1e30 * 1e30), 0)     # the probe of row 7, its norm overflows
    gal = coarse_gallery(eng, g)
    assert int(gal.flag.item()) == 1
    assert not bool(check_equal(eng, gal, q, 10).any())
    g2 = rand_rows(500, 31)
    g2[11] *= 1e-20                   # norm 2.3e-19 < 2^-60
    gal2 = coarse_gallery(eng, g2)
    assert int(gal2.flag.item()) == 1 and not bool(check_equal(eng, gal2, q[:4], 10).any())
    # a zero row is safe: the gallery certifies, an unsafe probe alone does not
    g3 = rand_rows(500, 31)
    g3[9] = 0.0
    gal3 = coarse_gallery(eng, g3)
    assert int(gal3.flag.item()) == 0
    big = torch.cat((rand_rows(4, 32), rand_rows(1, 33) * 1e30, rand_rows(1, 34) * 1e-30, torch.zeros((1, 512), device='cuda')), 0)
    cert = check_equal(eng, gal3, big, 10)
    assert cert.tolist() == [True] * 4 + [False] * 3
    # the flag is sticky: a later unsafe row switches the certificates off for good
    gal3.add(g2[11:12])
    gal3.add(rand_rows(5, 35))
    assert int(gal3.flag.item()) == 1 and not bool(check_equal(eng, gal3, big[:4], 10).any())


def test_growth_in_pieces(eng):
    g = rand_rows(3561, 41)
    q = rand_rows(9, 42)
    gal = Gallery(eng, coarse=True)
    first = 0
    for n in (60, 1, 2000, 1500):               # 1024 -> 2061 -> 4122 rows of capacity: two reallocations
        assert gal.add(g[first:first + n]) == first
        first += n
        assert len(gal) == first and torch.equal(gal.embeddings, g[:first])
        check_equal(eng, gal, q, 10)
    whole = torch.empty((3561, 512), device='cuda', dtype=torch.int16)
    flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    eng.coarse_pack(g, eng.row_norms(g), whole, flag)
    assert torch.equal(gal.plane, whole) and int(flag.item()) == 0 and int(gal.flag.item()) == 0
    # the plane is the bf16 of the normalised rows, to the last bit of a correctly rounded division or one step beside it
    want = (g / eng.row_norms(g)[:, None]).to(torch.bfloat16).view(torch.int16)
    assert int((whole.int() - want.int()).abs().max()) <= 1 and float((whole != want).float().mean()) < 1e-3


def test_shards_and_leave_one_out(eng):
    q, g = rand_rows(33, 51), rand_rows(65537, 52)
    one = coarse_gallery(eng, g)
    plain = Gallery(eng)
    plain.add(g)
    for k in (10, 64):
        bounds = [0, k // 2, 30000, g.size(0)]
        ss, ii = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            s, i = coarse_gallery(eng, g[lo:hi]).search(q, k, index_base=lo)
            ss.append(s)
            ii.append(i)
        ms, mi = eng.topk_merge(torch.stack(ss), torch.stack(ii))
        s, i = one.search(q, k)
        es, ei = plain.search(q, k)
        assert torch.equal(ms, s) and torch.equal(mi, i) and torch.equal(s, es) and torch.equal(i, ei), k
    me = torch.tensor([5, 17, 60, 65536], device='cuda')
    ls, li = one.search(g[me], 10, self_index=me)
    es, ei = plain.search(g[me], 10, self_index=me)
    assert torch.equal(ls, es) and torch.equal(li, ei) and not bool((li == me[:, None]).any())
    ls, li = one.search(g[me], 10, self_index=me, index_base=1000)
    es, ei = plain.search(g[me], 10, self_index=me, index_base=1000)
    assert torch.equal(ls, es) and torch.equal(li, ei)


def test_beyond_one_chunk(eng):
    """G = 2^20 + 129 rows (2.1 GB of rows, 1.07 GB of plane): 64-bit row bases in the pass and in the gathering re-score."""
    G, Q, k = (1 << 20) + 129, 8, 10
    gal = Gallery(eng, capacity=G, coarse=True)
    step = 1 << 18
    for lo in range(0, G, step):
        gal.add(rand_rows(min(step, G - lo), 1000 + lo))
    g = gal.embeddings
    planted = [3, (1 << 20) - 1, G - 1]
    q = torch.cat((g[planted] + 0.01 * rand_rows(3, 41), rand_rows(5, 42)), 0)
    cert = check_equal(eng, gal, q, k)
    s, i = gal.search(q, k)
    assert i[:3, 0].tolist() == planted
    print('certified %d of %d' % (int(cert.sum()), Q))


def test_deterministic_and_batch_independent(eng):
    q = torch.cat((cpu_rows(241, 61), cpu_corr(16, 62)), 0).cuda()
    gal = coarse_gallery(eng, torch.cat((cpu_rows(20000, 63), cpu_corr(2000, 64)), 0).cuda())
    for k in (10, 64):
        s1, i1 = gal.search(q, k)
        c1 = gal.last_certified
        s2, i2 = gal.search(q, k)
        assert torch.equal(s1, s2) and torch.equal(i1, i2) and torch.equal(c1, gal.last_certified)
        assert int(c1[:241].sum()) >= 217 and int(c1[241:].sum()) == 0      # as the CPU model has it: all, and none
        for r in range(257):
            sr, ir = gal.search(q[r:r + 1], k)
            assert torch.equal(sr[0], s1[r]) and torch.equal(ir[0], i1[r]) and torch.equal(gal.last_certified[0], c1[r]), r
    check_equal(eng, gal, q, 10)


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_arguments(eng):
    q, g = rand_rows(4, 71), rand_rows(100, 72)
    n = eng.row_norms(g)
    plane = torch.empty((100, 512), device='cuda', dtype=torch.int16)
    flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    cert = torch.empty((4,), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    pack_ok = (P(g), P(n), 100, 512, P(plane), P(flag), st)
    assert _rc(eng, 'ffr_coarse_pack', *pack_ok) == 0
    names = ['rows', 'norms', 'n', 'dim', 'plane', 'flag', 'st']

    def pack(**kw):
        a = list(pack_ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return _rc(eng, 'ffr_coarse_pack', *a)

    assert pack(dim=256) == -6
    for bad in (dict(rows=null), dict(norms=null), dict(plane=null), dict(flag=null), dict(n=0),
                dict(plane=C.c_void_p(plane.data_ptr() + 2)), dict(rows=C.c_void_p(g.data_ptr() + 4))):
        assert pack(**bad) == -1, bad
    ok = (P(q), 4, P(g), P(n), P(plane), P(flag), 100, 512, 10, 0, P(s), P(i), P(cert), st)
    snames = ['q', 'Q', 'g', 'n', 'plane', 'flag', 'G', 'dim', 'k', 'base', 's', 'i', 'cert', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[snames.index(key)] = v
        return _rc(eng, 'ffr_search_topk_coarse', *a)

    assert call() == 0 and call(cert=null) == 0
    assert call(dim=256) == -6
    for bad in (dict(k=0), dict(k=129), dict(Q=0), dict(G=-1), dict(q=null), dict(g=null), dict(n=null), dict(plane=null),
                dict(flag=null), dict(s=null), dict(i=null), dict(plane=C.c_void_p(plane.data_ptr() + 2)),
                dict(g=C.c_void_p(g.data_ptr() + 4))):
        assert call(**bad) == -1, bad
    assert call(G=0, g=null, n=null, plane=null, flag=null) == 0          # the null rule of the gallery at G = 0
    torch.cuda.synchronize()
    assert bool((i[:4].view(-1)[:40] == -1).all())
    # G = 3 < k = 10: the 3 rows, then 7 (-inf, -1); certified, the shortlist is the gallery
    gal = coarse_gallery(eng, g[:3])
    s3, i3 = gal.search(q, 10)
    assert torch.equal(torch.sort(i3[:, :3], 1).values, torch.arange(3, device='cuda').expand(4, 3))
    assert torch.all(i3[:, 3:] == -1) and torch.all(s3[:, 3:] == float('-inf')) and bool(gal.last_certified.all())
    with pytest.raises(RuntimeError):
        gal.search(q, 129)
    with pytest.raises(RuntimeError):
        eng.search_coarse(q, g, plane.float(), flag, 10)
    with pytest.raises(RuntimeError):
        eng.search_coarse(q, g, plane[:50], flag, 10)
    with pytest.raises(RuntimeError):
        eng.search_coarse(q.cpu(), g, plane, flag, 10)
    assert Gallery(eng).coarse is False and not hasattr(Gallery(eng), '_plane')


def test_profile_counts_coarse_search_under_score(eng):
    q = rand_rows(40, 81)
    gal = coarse_gallery(eng, rand_rows(5000, 82))
    gal.search(q, 10)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    gal.search(q, 10)
    st = eng.profile_read()
    eng.profile_enable(False)
    assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * 40 * 5000 * 512 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
