"""1:N identification on the device (include/ffrnet.h: ffr_row_norms, ffr_search_topk, ffr_topk_merge; ffrnet_amd.search).

The oracle is torch float64 on the device: cos = q.g / (|q| |g| + 1e-8).  fp32 MFMA errs by ~1.5e-7 * sum|a*b|, so a
returned score must be within TOL = 1e-6 of its float64 cosine, and no row left out may score more than 2 * TOL above the
k-th returned one."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import ffrnet_amd
from ffrnet_amd import native
from ffrnet_amd.search import Gallery, drop_self

pytestmark = pytest.mark.gpu

TOL = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def real_rows(state_dicts):
    """f_new (masked-probe side) and f (enrolment side) of 512 synthetic images: 1024 real embeddings."""
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
    return torch.cat(outs[0::2] + outs[1::2], 0)          # [f_new ..., f ...]


def rand_rows(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn((n, 512), device='cuda', generator=g)


def cos64(q, g):
    q64, g64 = q.double(), g.double()
    return (q64 @ g64.T) / (q64.norm(dim=1)[:, None] * g64.norm(dim=1)[None, :] + 1e-8)


def check_ranking(q, g, k, s, i):
    Q, G = q.size(0), g.size(0)
    kk = min(k, G)
    assert s.shape == (Q, k) and i.shape == (Q, k) and s.dtype == torch.float32 and i.dtype == torch.int64
    if kk < k:
        assert torch.all(i[:, kk:] == -1) and torch.all(torch.isinf(s[:, kk:]) & (s[:, kk:] < 0))
    s, i = s[:, :kk], i[:, :kk]
    assert int(i.min()) >= 0 and int(i.max()) < G
    # distinct indices, descending score, ties by ascending index
    si = torch.sort(i, 1).values
    assert torch.all(si[:, 1:] != si[:, :-1])
    if kk > 1:
        ds = s[:, :-1] - s[:, 1:]
        assert torch.all(ds >= 0)
        assert torch.all((ds > 0) | (i[:, :-1] < i[:, 1:]))
    ref = cos64(q, g)
    err = (s.double() - ref.gather(1, i)).abs().max().item()
    assert err <= TOL, err
    left = ref.clone()
    left.scatter_(1, i, float('-inf'))
    worst = (left.max(1).values - s[:, -1].double()).max().item()
    assert worst <= 2 * TOL, worst


CASES = [  # (Q, G, k, data)
    (1, 1000, 1, 'rand'), (31, 1000, 10, 'rand'), (32, 65537, 128, 'rand'), (33, 65537, 10, 'rand'),
    (257, 1000, 128, 'rand'), (1, 1 << 20, 10, 'rand'), (257, 1 << 20, 10, 'rand'), (33, 1 << 20, 128, 'rand'),
    (32, 10, 10, 'rand'), (257, 128, 128, 'rand'), (31, 1, 1, 'rand'),
    (1, 1000, 10, 'real'), (31, 1000, 128, 'real'), (257, 1000, 1, 'real'), (33, 10, 10, 'real'), (32, 128, 128, 'real'),
]


@pytest.mark.parametrize('Q,G,k,data', CASES)
def test_search_ranking_matches_float64(eng, real_rows, Q, G, k, data):
    if data == 'rand':
        q, g = rand_rows(Q, 11 * Q + k), rand_rows(G, 7 * G + 1)
    else:
        q = real_rows[(37 * torch.arange(Q, device='cuda')) % 512]              # masked-side probes (f_new)
        g = real_rows[512 + (torch.arange(G, device='cuda') % 512)]            # mask-free enrolments (f), repeated
        if G > 512:
            g = torch.cat((g[:512], real_rows[:G - 512]), 0)
    s, i = eng.search(q, g, k)
    torch.cuda.synchronize()
    check_ranking(q, g, k, s, i)


def test_ties_zero_rows_and_cosine_scores(eng):
    g = rand_rows(3000, 5)
    g[100] = 0.0
    for dst in (17, 2500, 40):                    # copies of row 900: identical scores, returned by ascending index
        g[dst] = g[900]
    q = torch.cat((g[900:901] * 0.5 + rand_rows(1, 6) * 1e-3, rand_rows(4, 7)), 0)
    s, i = eng.search(q, g, 10)
    torch.cuda.synchronize()
    assert i[0, :4].tolist() == [17, 40, 900, 2500]
    assert torch.equal(s[0, :4], s[0, :1].expand(4))
    check_ranking(q, g, 10, s, i)
    # a zero gallery row scores exactly 0: every probe, k = G
    s, i = eng.search(q, g[:200], 128)
    s2, i2 = eng.search(q, g[95:105], 10, index_base=95)
    z = (i2 == 100)
    assert int(z.sum()) == q.size(0) and torch.all(s2[z] == 0.0)
    # the scores agree with ffr_cosine_scores on the same pairs
    for r in range(q.size(0)):
        cs = eng.cosine_scores(q[r:r + 1].expand(128, 512).contiguous(), g[i[r]])
        assert (cs - s[r]).abs().max().item() <= TOL


def test_deterministic_and_batch_independent(eng):
    q, g = rand_rows(257, 21), rand_rows(65537, 22)
    norms = eng.row_norms(g)
    for k in (10, 128):
        s1, i1 = eng.search(q, g, k, gallery_norms=norms)
        s2, i2 = eng.search(q, g, k, gallery_norms=norms)
        assert torch.equal(s1, s2) and torch.equal(i1, i2)
        for r in range(257):
            sr, ir = eng.search(q[r:r + 1], g, k, gallery_norms=norms)
            assert torch.equal(sr[0], s1[r]) and torch.equal(ir[0], i1[r]), r


def test_shard_merge_equals_single_search(eng):
    q, g = rand_rows(33, 31), rand_rows(65537, 32)
    for k in (10, 128):
        bounds = [0, k // 2, 30000, g.size(0)]           # three uneven contiguous shards, the first smaller than k
        ss, ii = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            s, i = eng.search(q, g[lo:hi], k, index_base=lo)
            ss.append(s)
            ii.append(i)
        ms, mi = eng.topk_merge(torch.stack(ss), torch.stack(ii))
        s, i = eng.search(q, g, k)
        assert torch.equal(ms, s) and torch.equal(mi, i), k
        # an empty shard and the bases of a second gallery block merge the same way
        es, ei = eng.search(q, g[:0], k, index_base=123)
        assert torch.all(ei == -1) and torch.all(torch.isinf(es))
        ms2, mi2 = eng.topk_merge(torch.stack(ss + [es]), torch.stack(ii + [ei]))
        assert torch.equal(ms2, s) and torch.equal(mi2, i)


def test_gallery_beyond_2gib(eng):
    """G = 1 200 001 rows = 2.46 GB: 64-bit chunk bases (run once)."""
    G, Q, k = 1200001, 8, 10
    g = torch.empty((G, 512), device='cuda')
    step = 200000
    for lo in range(0, G, step):
        g[lo:lo + step] = rand_rows(min(step, G - lo), 1000 + lo)
    q = torch.cat((g[[3, 700000, G - 1]] + 0.01 * rand_rows(3, 41), rand_rows(5, 42)), 0)
    s, i = eng.search(q, g, k)
    torch.cuda.synchronize()
    assert i[0, 0].item() == 3 and i[1, 0].item() == 700000 and i[2, 0].item() == G - 1
    q64 = q.double()
    qn = q64.norm(dim=1)
    best = torch.full((Q,), float('-inf'), device='cuda', dtype=torch.float64)
    got = torch.zeros((Q, k), device='cuda', dtype=torch.float64)
    for lo in range(0, G, step):
        g64 = g[lo:lo + step].double()
        c = (q64 @ g64.T) / (qn[:, None] * g64.norm(dim=1)[None, :] + 1e-8)
        inside = (i >= lo) & (i < lo + g64.size(0))
        got[inside] = c.gather(1, (i - lo).clamp(0, g64.size(0) - 1))[inside]
        mask = torch.zeros_like(c, dtype=torch.bool)
        for r in range(Q):
            sel = i[r][inside[r]] - lo
            mask[r, sel] = True
        best = torch.maximum(best, c.masked_fill(mask, float('-inf')).max(1).values)
        del g64, c, mask
    assert (got - s.double()).abs().max().item() <= TOL
    assert (best - s[:, -1].double()).max().item() <= 2 * TOL


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_arguments(eng):
    q, g = rand_rows(4, 51), rand_rows(100, 52)
    n = eng.row_norms(g)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    P = native._ptr
    st = eng._stream()
    ok = (P(q), 4, P(g), P(n), 100, 512, 10, 0, P(s), P(i), st)

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[['q', 'Q', 'g', 'n', 'G', 'dim', 'k', 'base', 's', 'i', 'st'].index(key)] = v
        return _rc(eng, 'ffr_search_topk', *a)

    assert call() == 0
    assert call(dim=256) == -6
    assert _rc(eng, 'ffr_row_norms', P(g), 100, 256, P(n), st) == -6
    for bad in (dict(k=0), dict(k=129), dict(Q=0), dict(G=-1), dict(q=C.c_void_p(0)), dict(g=C.c_void_p(0)),
                dict(n=C.c_void_p(0)), dict(s=C.c_void_p(0)), dict(i=C.c_void_p(0))):
        assert call(**bad) == -1, bad
    assert _rc(eng, 'ffr_topk_merge', P(s), P(i), 0, 4, 10, P(s), P(i), st) == -1
    assert _rc(eng, 'ffr_topk_merge', P(s), P(i), 1, 4, 129, P(s), P(i), st) == -1
    # G = 3 < k = 10: the 3 rows, then 7 (-inf, -1)
    s3, i3 = eng.search(q, g[:3], 10)
    assert torch.equal(torch.sort(i3[:, :3], 1).values, torch.arange(3, device='cuda').expand(4, 3))
    assert torch.all(i3[:, 3:] == -1) and torch.all(s3[:, 3:] == float('-inf'))
    with pytest.raises(RuntimeError):
        eng.search(q, g, 129)
    # a tensor on another device is rejected by the binding
    with pytest.raises(RuntimeError):
        eng.search(q.cpu(), g, 10)
    with pytest.raises(RuntimeError):
        eng.search(q, g, 10, gallery_norms=n.cpu())
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            eng.search(q.to('cuda:1'), g, 10)
    # leave-one-out never returns the probe's own row
    gal = Gallery(eng)
    assert gal.add(g[:60]) == 0 and gal.add(g[60:]) == 60 and len(gal) == 100
    assert torch.equal(gal.norms, n)
    me = torch.tensor([5, 17, 60, 99], device='cuda')
    ls, li = gal.search(g[me], 10, self_index=me)
    assert li.shape == (4, 10) and not torch.any(li == me[:, None])
    fs, fi = gal.search(g[me], 11)
    assert torch.all(fi[:, 0] == me)                   # the probe itself would have been first
    assert torch.equal(li, fi[:, 1:]) and torch.equal(ls, fs[:, 1:])
    ds, di = drop_self(fs, fi, me)
    assert torch.equal(di, li)


def test_profile_counts_search_under_score(eng):
    q, g = rand_rows(40, 61), rand_rows(5000, 62)
    n = eng.row_norms(g)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    eng.search(q, g, 10, gallery_norms=n)
    st = eng.profile_read()
    eng.profile_enable(False)
    assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * 40 * 5000 * 512 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0


def test_sharded_search_two_ranks_on_one_gpu():
    """tools/search_two_ranks_one_gpu.py: two gloo ranks on cuda:0, each with a contiguous shard; every rank's
    search_sharded result equals the single-process search bitwise."""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'search_two_ranks_one_gpu.py')], cwd=ROOT,
                             capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail('two-rank search timed out: %s' % ((e.stderr or b'')[-2000:],))
    assert out.returncode == 0 and 'OK' in out.stdout, (out.stdout[-1000:], out.stderr[-2000:])
