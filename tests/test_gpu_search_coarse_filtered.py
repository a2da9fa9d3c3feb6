"""The certified bf16 shortlist under a per-probe filter, on the device (include/ffrnet.h: ffr_search_topk_coarse_filtered;
Engine.search_coarse_filtered; ffrnet_amd.search.Gallery.shortlist_filtered).

The oracle is the exact filtered search, Engine.search_filtered: every comparison is torch.equal on scores, indices and
subjects, no tolerance; on the small shape also against the numpy restatement of tests/search_filtered_ref.py.  Equality
alone would pass if every probe fell back to the exact search, so the certified flags are asserted where the definition or
the CPU model of tests/search_coarse_filtered_ref.py says what they must be."""
import ctypes as C

import numpy as np
import pytest
import torch

import ffrnet_amd
import search_coarse_filtered_ref as ref
import search_filtered_ref as fref
import test_gpu_search_subjects as base
from ffrnet_amd import native
from ffrnet_amd.search import Gallery, search_sharded_filtered, shortlist_size

pytestmark = pytest.mark.gpu

FULL, B31 = 0xFFFFFFFF, 0x80000000
MASKS8 = [1, 2, 0, FULL, B31, 3, 1 << 5, B31 | 1]          # 8 distinct masks in one batch, a mask-0 probe among them
TAG_KINDS = ('all', 'half', 'one', 'zero', 'bit31')


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


rand_rows = base.rand_rows
same = base.same


def cpu_rows(n, seed):
    return torch.randn((n, 512), generator=torch.Generator().manual_seed(seed))


def corr_rows(n, seed, base_seed=77):
    """base + 0.05 * noise: every cosine between two of them is within 2 * COARSE_EPS of every other"""
    return rand_rows(1, base_seed) + 0.05 * rand_rows(n, seed)


def planted_rows(Q, G, seed, per=8, noise=0.7):
    """a centre per person, rows = centre[g % nsub] + noise * randn, probes of Q people"""
    nsub = max(1, (G + per - 1) // per)
    cent = rand_rows(nsub, seed)
    g = cent[torch.arange(G, device='cuda') % nsub] + noise * rand_rows(G, seed + 1)
    return cent[(37 * torch.arange(Q, device='cuda')) % nsub] + noise * rand_rows(Q, seed + 2), g


def spread_subjects(G, per=8):
    return (torch.arange(G, device='cuda') % max(1, (G + per - 1) // per)).to(torch.int32)


def dev(words):
    """int64 words in [0, 2^32) (tensor, array or list) -> the int32 device tensor the library reads"""
    return native.tag_words(torch.as_tensor(np.asarray(words, dtype=np.int64)), 'words', 'cuda')


def tags_of(kind, G, seed):
    """tag[G] int64 on the host: the kinds of tests/search_coarse_filtered_ref.py, and 'zero': one bit of 32 with a quarter of
    the rows at tag 0"""
    if kind != 'zero':
        return ref.tag_patterns(G, kind, seed)
    t = ref.tag_patterns(G, 'one', seed)
    t[torch.rand((G,), generator=torch.Generator().manual_seed(seed + 1)) < 0.25] = 0
    return t


def masks_of(Q):
    return torch.tensor([MASKS8[r % 8] for r in range(Q)], dtype=torch.int64)


class Packed(object):
    """rows with their norms, plane and flag"""

    def __init__(self, eng, g):
        self.g = g.contiguous()
        G = g.size(0)
        self.norms = eng.row_norms(self.g) if G else torch.empty((0,), device='cuda')
        self.plane = torch.empty((G, 512), device='cuda', dtype=torch.int16)
        self.flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
        eng.coarse_pack(self.g, self.norms, self.plane, self.flag)


def check(eng, p, q, mask, tags, k, subj=None, distinct=False, index_base=0):
    """Engine.search_coarse_filtered == Engine.search_filtered, every plane -> the certified flags [Q] (bool, on the host)"""
    got = eng.search_coarse_filtered(q, mask, p.g, p.plane, p.flag, tags, k, gallery_norms=p.norms, index_base=index_base,
                                     subjects=subj, distinct=distinct, return_certified=True)
    want = eng.search_filtered(q, mask, p.g, tags, k, gallery_norms=p.norms, index_base=index_base, subjects=subj, distinct=distinct)
    torch.cuda.synchronize()
    assert len(got) == len(want) + 1 == (3 if subj is None else 4)
    assert same(got[:-1], want), (k, distinct, index_base)
    cert = got[-1]
    assert cert.shape == (q.size(0),) and cert.dtype == torch.int32 and bool(((cert == 0) | (cert == 1)).all())
    return cert.bool().cpu()


def n_admissible(tags, mask, subj=None):
    """[Q] on the host: the rows each probe may see"""
    return torch.tensor([int(ref.admissible(tags, m, None if subj is None else subj.cpu()).sum()) for m in mask])


CASES = [(1, 1000, 1), (31, 1000, 10), (33, 65537, 10), (32, 65537, 32), (257, 4096, 10), (32, 10, 10), (31, 1, 1),
         (5, 200, 64), (5, 200, 65), (5, 200, 33)]


@pytest.mark.parametrize('data', ['rand', 'corr', 'planted'])
@pytest.mark.parametrize('Q,G,k', CASES)
def test_equals_the_exact_filtered_search(eng, Q, G, k, data):
    """The seven shapes and the k limits (64 rows and 32 identities are served, 65 and 33 are not) on Gaussian, correlated and
    planted rows; without subjects, with them and with a seeded 10 % of them removed; rows and identities; five tag kinds;
    eight masks per batch, mask 0 among them; with and without an index base."""
    if data == 'planted':
        q, g = planted_rows(Q, G, 13 * Q + k)
    else:
        rows = rand_rows if data == 'rand' else corr_rows
        q, g = rows(Q, 11 * Q + k), rows(G, 7 * G + 1)
    p = Packed(eng, g)
    subj = spread_subjects(G)
    gone = subj.clone()
    gone[torch.isin(subj, base_ids(subj, 0.1, G + k).cuda().to(torch.int32))] = -1
    mask = masks_of(Q)
    md = dev(mask)
    for j, kind in enumerate(TAG_KINDS):
        tags = tags_of(kind, G, 100 * k + j)
        td = dev(tags)
        for s_, distinct in ((None, False), (subj, False), (subj, True), (gone, False), (gone, True)):
            if distinct and k > 64:
                continue                                         # identity mode serves k <= 64 in either entry
            ib = (1 << 33) + 5 if (j + int(distinct)) % 2 else 0
            cert = check(eng, p, q, md, td, k, s_, distinct, index_base=ib)
            kp = shortlist_size(k, distinct)
            if kp is None:
                assert not bool(cert.any()), (kind, distinct)    # the exact filtered search alone
                continue
            assert bool(cert[mask == 0].all())                   # an empty shortlist: certified padding
            short = n_admissible(tags, mask, s_) < kp
            assert bool(cert[short].all()), (kind, distinct)     # the shortlist is every admissible row
            if G <= kp:
                assert bool(cert.all())
            if data == 'corr' and kind == 'all' and G > kp and kp < 128:
                assert not bool(cert[(mask != 0) & ~short].any())  # a shortlist that cannot separate


def base_ids(subj, frac, seed):
    """a seeded share of the subject ids (at least one)"""
    ids = torch.unique(subj[subj >= 0]).cpu()
    n = max(1, int(round(frac * ids.numel())))
    return ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))[:n]]


def test_small_shape_equals_the_numpy_restatement(eng):
    """(31, 1000): the score matrix from 128-row shards of the exact search, the lists from tests/search_filtered_ref.py"""
    d = base.Data(eng, rand_rows(31, 501), rand_rows(1000, 601))
    p = Packed(eng, d.g)
    mask = masks_of(31)
    subj = base.layout('removed', 1000)
    for j, kind in enumerate(TAG_KINDS):
        tags = tags_of(kind, 1000, 40 + j)
        for s_, distinct, k in ((None, False, 10), (subj, False, 64), (subj, True, 10), (subj, True, 32)):
            got = eng.search_coarse_filtered(d.q, dev(mask), p.g, p.plane, p.flag, dev(tags), k, gallery_norms=p.norms,
                                             subjects=None if s_ is None else torch.from_numpy(s_).cuda(), distinct=distinct)
            want = fref.search_ref(d.S, tags.numpy(), mask.numpy(), k, s_, int(distinct), order=d.order)
            assert same(got, tuple(torch.from_numpy(x).cuda() for x in want[:len(got)])), (kind, k, distinct)


@pytest.mark.parametrize('kind,seed', ref.CERTIFYING)
def test_certifying_inputs_certify(eng, kind, seed):
    """The nine inputs whose margin tests/test_host_search_coarse_filtered.py checks on the CPU (slack > 2^-11, where the
    accumulation order of the matrix core is allowed 2^-13): the device certifies 33 of 33."""
    q, g, tags, mask = ref.certifying_inputs(kind, seed)
    p = Packed(eng, g.cuda())
    for k in ref.CERTIFYING_K:
        cert = check(eng, p, q.cuda(), dev(mask), dev(tags), k)
        print('%s k = %d: certified %d of 33' % (kind, k, int(cert.sum())))
        assert bool(cert.all()), (kind, k)


def test_fewer_admissible_rows_than_the_shortlist_and_than_k(eng):
    """G = 4096 under one bit of 32: about 128 admissible rows.  At k = 64 (k' = 128) a probe with fewer than 128 has a short
    list and is certified, correlated rows or not; fewer admissible rows than k: certified padding."""
    q, g = corr_rows(33, 1), corr_rows(4096, 2)
    p = Packed(eng, g)
    tags = ref.tag_patterns(4096, 'one', 3)
    mask = torch.tensor([1 << (r % 32) for r in range(33)], dtype=torch.int64)
    n_adm = n_admissible(tags, mask)
    assert bool((n_adm < 128).any()) and bool((n_adm > 64).all())
    cert = check(eng, p, q, dev(mask), dev(tags), 64)
    assert bool(cert[n_adm < 128].all())
    assert not bool(check(eng, p, q, dev(mask), dev(tags), 10).any())          # k' = 32: full lists that cannot separate
    few = torch.zeros((4096,), dtype=torch.int64)
    few[::1000] = 4
    few[7] = 8
    mask = torch.tensor([4, 8, 12, 0, 4] * 6 + [8, 4, 12], dtype=torch.int64)
    subj = spread_subjects(4096)
    for s_, distinct in ((None, False), (subj, False), (subj, True)):
        for k in (1, 10, 64) if not distinct else (1, 10, 32):
            assert bool(check(eng, p, q, dev(mask), dev(few), k, s_, distinct).all())
    s, i = eng.search_coarse_filtered(q, dev(mask), p.g, p.plane, p.flag, dev(few), 10, gallery_norms=p.norms)
    assert bool((i[0, 5:] == -1).all()) and bool((i[0, :5] % 1000 == 0).all()) and i[1].tolist() == [7] + [-1] * 9
    assert bool((i[3] == -1).all()) and bool(torch.isinf(s[3]).all()) and int((i[2] >= 0).sum()) == 6


def copies_gallery(n_copies, seed):
    """3000 Gaussian rows on the host, n_copies of them (sorted, the first is the source) exact duplicates of one row, and a
    probe next to that row"""
    g = cpu_rows(3000, seed)
    copies = torch.randperm(3000, generator=torch.Generator().manual_seed(seed + 1))[:n_copies].sort().values
    g[copies] = g[int(copies[0])].clone()
    return g, copies, g[int(copies[0]):int(copies[0]) + 1] * 0.5 + 1e-3 * cpu_rows(1, seed + 2)


def test_mixed_batch_keeps_each_probes_mask(eng):
    """The mask gather.  40 exact duplicates of one row carry bit 1 alone, every other row bit 0 alone.  The probe next to
    that row under a mask with bit 1 meets 40 tied rows, more than k' = 32: no certificate.  Under mask 1 the duplicates are
    invisible and it certifies (the model says so, slack > 2^-11).  Both kinds at scattered places of one batch, Gaussian
    probes between them: every row is the one-probe call with its own mask."""
    g, copies, near = copies_gallery(40, 5)
    tags = torch.ones((3000,), dtype=torch.int64)
    tags[copies] = 2
    mask = torch.tensor([1, 3, 1, 2, 2, 1, 3, 0, 1, 1, 3, 2, 1, 3, 3, 1, 2, 1, 1], dtype=torch.int64)
    q = near.repeat(19, 1) + 1e-4 * cpu_rows(19, 8)
    q[[5, 12]] = cpu_rows(2, 9)                                   # Gaussian probes, whatever they do
    model = ref.search(q, g, tags, mask, 2)
    sees = (mask & 2) != 0
    sees[[5, 12]] = False
    plain = ~sees
    plain[[5, 12]] = False
    assert not bool(model[3][sees].any()) and bool(model[3][plain].all()) and float(model[4][plain].min()) > 2.0 ** -11
    p = Packed(eng, g.cuda())
    qd, md, td = q.cuda(), dev(mask), dev(tags)
    cert = check(eng, p, qd, md, td, 2)
    assert not bool(cert[sees].any()) and bool(cert[plain].all()) and int(sees.sum()) == 9 and int(plain.sum()) == 8
    whole = eng.search_coarse_filtered(qd, md, p.g, p.plane, p.flag, td, 2, gallery_norms=p.norms, return_certified=True)
    for r in range(19):
        one = eng.search_coarse_filtered(qd[r:r + 1], md[r:r + 1], p.g, p.plane, p.flag, td, 2, gallery_norms=p.norms,
                                         return_certified=True)
        assert all(torch.equal(a[0], b[r]) for a, b in zip(one, whole)), r
    s, i = whole[:2]
    assert i[1].tolist() == copies[:2].tolist() and i[3].tolist() == copies[:2].tolist() and s[1, 0] == s[1, 1]
    assert not bool(torch.isin(i[0], copies.cuda()).any()) and bool((i[7] == -1).all())
    # with subjects, the gathered probes go through the filtered subject kernels with their own masks
    subj = (torch.arange(3000) % 500).to(torch.int32).cuda()
    for distinct in (False, True):
        cert = check(eng, p, qd, md, td, 2, subj, distinct)
        assert bool(cert[mask == 0].all()) and (distinct or not bool(cert[sees].any()))     # k' = 64 holds all 40 duplicates


def test_ties_across_the_shortlist_edge(eng):
    """More tied admissible rows than k' = 32: not certified, the exact answer.  The same rows inadmissible by their tag:
    certified."""
    g, copies, near = copies_gallery(40, 15)
    q = torch.cat((near, cpu_rows(3, 18)), 0)
    tags = torch.full((3000,), 5, dtype=torch.int64)
    mask = torch.tensor([1, 1, 4, 5], dtype=torch.int64)
    p = Packed(eng, g.cuda())
    for k in (2, 16):
        assert not bool(ref.search(q, g, tags, mask, k)[3][0])
        cert = check(eng, p, q.cuda(), dev(mask), dev(tags), k)
        assert not bool(cert[0])
    s, i = eng.search_coarse_filtered(q.cuda(), dev(mask), p.g, p.plane, p.flag, dev(tags), 2, gallery_norms=p.norms)
    assert i[0].tolist() == copies[:2].tolist() and s[0, 0] == s[0, 1]
    tags[copies[1:]] = 2                                          # 39 of the 40 leave probe 0's sight
    for k in (2, 16):
        model = ref.search(q, g, tags, mask, k)
        assert bool(model[3].all()) and float(model[4].min()) > 2.0 ** -11
        assert bool(check(eng, p, q.cuda(), dev(mask), dev(tags), k).all())
    s, i = eng.search_coarse_filtered(q.cuda(), dev(mask), p.g, p.plane, p.flag, dev(tags), 2, gallery_norms=p.norms)
    assert int(i[0, 0]) == int(copies[0]) and s[0, 1] < s[0, 0] and int(i[0, 1]) not in copies.tolist()


def test_one_person_with_more_admissible_rows_than_the_shortlist(eng):
    """200 near-copies of probe 0 under one subject: the shortlist (k' = 64) holds that subject alone, no certificate, the
    right answer.  All but two of them inadmissible: certified.  The model says the same of both."""
    g = cpu_rows(3000, 41)
    q = cpu_rows(2, 42)
    g[:200] = q[0] + 0.01 * cpu_rows(200, 43)
    subject = torch.arange(3000) + 10
    subject[:200] = 3
    tags = torch.ones((3000,), dtype=torch.int64)
    mask = torch.tensor([1, 1], dtype=torch.int64)
    p = Packed(eng, g.cuda())
    sd = subject.to(torch.int32).cuda()
    assert ref.search(q, g, tags, mask, 5, subject, True)[3].tolist() == [False, True]
    assert check(eng, p, q.cuda(), dev(mask), dev(tags), 5, sd, True).tolist() == [False, True]
    s, i, u = eng.search_coarse_filtered(q.cuda(), dev(mask), p.g, p.plane, p.flag, dev(tags), 5, gallery_norms=p.norms,
                                         subjects=sd, distinct=True)
    assert int(u[0, 0]) == 3 and int((u[0] == 3).sum()) == 1 and int(i[0, 0]) < 200
    check(eng, p, q.cuda(), dev(mask), dev(tags), 5, sd, False)
    tags[2:200] = 2
    model = ref.search(q, g, tags, mask, 5, subject, True)
    assert model[3].tolist() == [True, True] and float(model[4].min()) > 2.0 ** -11
    assert check(eng, p, q.cuda(), dev(mask), dev(tags), 5, sd, True).tolist() == [True, True]
    s, i, u = eng.search_coarse_filtered(q.cuda(), dev(mask), p.g, p.plane, p.flag, dev(tags), 5, gallery_norms=p.norms,
                                         subjects=sd, distinct=True)
    assert int(u[0, 0]) == 3 and int((u[0] == 3).sum()) == 1 and int(i[0, 0]) < 2


def test_unsafe_norms_and_a_set_flag(eng):
    subj = spread_subjects(500)
    tags = dev(tags_of('half', 500, 30))
    g = rand_rows(500, 31)
    g[7] *= 1e-30                     # every square underflows: norm 0 over a row that is not zero
    g[9] = 0.0
    q = torch.cat((rand_rows(4, 32), g[7:8] * 1e30 * 1e30), 0)     # the probe of row 7, its norm overflows
    mask = dev([1, 2, 3, 1, 3])
    p = Packed(eng, g)
    assert int(p.flag.item()) == 1
    for s_, distinct in ((None, False), (subj, False), (subj, True)):
        assert not bool(check(eng, p, q, mask, tags, 10, s_, distinct).any())
    # a zero row is safe: the gallery certifies, an unsafe probe alone does not
    g3 = rand_rows(500, 31)
    g3[9] = 0.0
    p3 = Packed(eng, g3)
    assert int(p3.flag.item()) == 0
    big = torch.cat((rand_rows(4, 32), rand_rows(1, 33) * 1e30, rand_rows(1, 34) * 1e-30, torch.zeros((1, 512), device='cuda')), 0)
    m7 = dev([1, 2, 3, 1, 3, 3, 3])
    for s_, distinct in ((None, False), (subj, False), (subj, True)):
        assert check(eng, p3, big, m7, tags, 10, s_, distinct).tolist() == [True] * 4 + [False] * 3
    # the flag does not look at the filter: set by hand, nothing is certified, mask 0 included
    p3.flag.fill_(1)
    assert not bool(check(eng, p3, big[:4], dev([1, 0, 3, 2]), tags, 10).any())


def test_deterministic_and_batch_independent(eng):
    """24 Gaussian probes and 16 correlated ones in one batch over Gaussian and correlated rows, eight masks: two runs are
    equal, and row r is the one-probe call with mask[r], results and certified flag."""
    q = torch.cat((cpu_rows(24, 61), cpu_rows(1, 77) + 0.05 * cpu_rows(16, 62)), 0).cuda()
    g = torch.cat((cpu_rows(6000, 63), cpu_rows(1, 77) + 0.05 * cpu_rows(2000, 64)), 0).cuda()
    p = Packed(eng, g)
    tags = dev(tags_of('zero', 8000, 65) | 1)
    mask = dev(masks_of(40))
    subj = spread_subjects(8000)
    subj[::13] = -1
    for s_, distinct in ((None, False), (subj, False), (subj, True)):
        def run(rows):
            return eng.search_coarse_filtered(q[rows], mask[rows], p.g, p.plane, p.flag, tags, 10, gallery_norms=p.norms,
                                              subjects=s_, distinct=distinct, return_certified=True)
        first, again = run(slice(0, 40)), run(slice(0, 40))
        assert same(first, again)
        assert 0 < int(first[-1].sum()) < 40                      # both ways occur
        for r in range(40):
            assert all(torch.equal(a[0], b[r]) for a, b in zip(run(slice(r, r + 1)), first)), (distinct, r)
        check(eng, p, q, mask, tags, 10, s_, distinct)


def test_shards_merge_to_one_call(eng):
    q, g = planted_rows(33, 65537, 71)
    p = Packed(eng, g)
    subj = spread_subjects(65537)
    subj[torch.isin(subj, base_ids(subj, 0.1, 72).cuda().to(torch.int32))] = -1
    tags, mask = dev(tags_of('zero', 65537, 73)), dev(masks_of(33))
    for s_, k, distinct in ((None, 10, False), (None, 64, False), (subj, 10, False), (subj, 10, True), (subj, 32, True)):
        bounds = [0, k // 2, 30000, 65537]
        parts = [eng.search_coarse_filtered(q, mask, g[lo:hi], p.plane[lo:hi], p.flag, tags[lo:hi], k, gallery_norms=p.norms[lo:hi],
                                            index_base=lo, subjects=None if s_ is None else s_[lo:hi], distinct=distinct)
                 for lo, hi in zip(bounds[:-1], bounds[1:])]
        stacked = [torch.stack([x[j] for x in parts]) for j in range(len(parts[0]))]
        merged = eng.topk_merge(*stacked) if s_ is None else eng.topk_merge_subjects(*stacked, distinct=distinct)
        whole = eng.search_coarse_filtered(q, mask, g, p.plane, p.flag, tags, k, gallery_norms=p.norms, subjects=s_, distinct=distinct)
        exact = eng.search_filtered(q, mask, g, tags, k, gallery_norms=p.norms, subjects=s_, distinct=distinct)
        assert same(merged, whole) and same(whole, exact), (k, distinct)


def test_gallery_opt_in(eng):
    """Off (the default): a masked search on a gallery with a plane takes the exact entry, last_certified is None.  On: the same
    results, last_certified set -- leave-one-out, search_subjects(mask=), and add / set_tags / remove / compact, then search."""
    q, g = planted_rows(33, 3561, 81)
    subj = spread_subjects(3561)
    tags = dev(tags_of('half', 3561, 82) | (tags_of('one', 3561, 83) << 2 & FULL))
    mask = dev(masks_of(33))
    gal = Gallery(eng, subjects=True)
    gal.build_tags()
    gal.add(g[:2000], subj[:2000], tags=tags[:2000])
    gal.build_plane()
    assert gal.shortlist_filtered is False

    def both(fn):
        """fn() with the route off and on -> the certified flags of the second"""
        gal.shortlist_filtered = False
        gal.last_certified = 'untouched'
        off = fn()
        assert gal.last_certified is None
        gal.shortlist_filtered = True
        on = fn()
        cert = gal.last_certified
        gal.shortlist_filtered = False
        assert same(on, off) and cert is not None and cert.dtype == torch.int32
        return cert

    cert = both(lambda: gal.search_subjects(q, 10, mask=mask))
    assert cert.shape == (33,) and bool(cert[2].item()) and 0 < int(cert.sum())
    both(lambda: gal.search(q, 10, mask=mask))
    both(lambda: gal.search(q, 10, mask=3, index_base=1 << 33))
    me = torch.tensor([5, 17, 60, 1999], device='cuda')
    cert = both(lambda: gal.search(g[me], 10, self_index=me, mask=dev([1, 3, FULL, B31 | 2])))
    assert cert.shape == (4,)
    gal.shortlist_filtered = True
    ls, li = gal.search(g[me], 10, self_index=me, mask=FULL)
    assert not bool((li == me[:, None]).any())
    # add / set_tags / remove / compact, then search: the plane, the tags and the subjects move together
    gal.add(g[2000:], subj[2000:], tags=tags[2000:])
    gal.set_tags([3, 700, 3000], B31 | 1)
    gal.set_subject_tags([int(subj[9])], 2)
    both(lambda: gal.search_subjects(q, 10, mask=mask))
    gal.remove(base_ids(subj, 0.2, 84))
    both(lambda: gal.search_subjects(q, 32, mask=mask))
    both(lambda: gal.search(q, 64, mask=mask))
    gal.shortlist_filtered = True
    before = gal.search_subjects(q, 10, mask=mask)
    old_to_new = gal.compact()
    after = gal.search_subjects(q, 10, mask=mask)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    assert torch.equal(after[2], torch.where(before[2] >= 0, old_to_new[before[2].clamp(min=0)], before[2]))
    both(lambda: gal.search_subjects(q, 10, mask=mask))
    gal.shortlist_filtered = True
    assert same(search_sharded_filtered(gal, q, 10, mask, distinct=True), gal.search_subjects(q, 10, mask=mask))
    # without a mask the attribute changes nothing; without a plane it changes nothing either
    s, u, i = gal.search_subjects(q, 10)
    assert same((s, i, u), eng.search_subjects(q, gal.embeddings, gal.subjects, 10, gallery_norms=gal.norms))
    plain = Gallery(eng)
    plain.build_tags()
    plain.add(g, tags=tags)
    plain.shortlist_filtered = True
    exact = eng.search_filtered(q, mask, g, tags, 10)
    assert same(plain.search(q, 10, mask=mask), exact) and plain.last_certified is None
    plain.build_plane()
    assert same(plain.search(q, 10, mask=mask), exact) and plain.last_certified is not None


def test_arguments(eng):
    q, g = rand_rows(4, 91), rand_rows(100, 92)
    p = Packed(eng, g)
    sub = torch.arange(101, device='cuda', dtype=torch.int32)
    tag = torch.full((101,), 3, device='cuda', dtype=torch.int32)
    m = torch.full((5,), 1, device='cuda', dtype=torch.int32)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    u = torch.empty((4, 129), device='cuda', dtype=torch.int32)
    cert = torch.ones((4,), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    ok = (P(q), P(m), 4, P(p.g), P(p.norms), P(p.plane), P(p.flag), P(tag), P(sub), 100, 512, 10, 0, 1, P(s), P(i), P(u), P(cert), st)
    names = ['q', 'm', 'Q', 'g', 'n', 'plane', 'flag', 'tag', 'sub', 'G', 'dim', 'k', 'base', 'distinct', 's', 'i', 'u', 'cert', 'st']
    who = b'ffr_search_topk_coarse_filtered'

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_search_topk_coarse_filtered(eng._h, *a)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    assert call() == 0 and call(distinct=0) == 0 and call(cert=null) == 0 and call(sub=null, u=null, distinct=0) == 0
    assert call(dim=256) == -6 and who in eng.lib.ffr_last_error(eng._h)
    for bad in (  # what ffr_search_topk_filtered rejects
                dict(m=null), dict(tag=null), dict(m=off(m, 2)), dict(tag=off(tag, 2)), dict(m=off(m, 1)), dict(sub=null, u=null),
                dict(u=null), dict(sub=null), dict(k=0), dict(k=129, distinct=0), dict(Q=0), dict(G=-1), dict(q=null), dict(g=null),
                dict(n=null), dict(s=null), dict(i=null), dict(sub=off(sub, 2)), dict(distinct=2), dict(distinct=-1), dict(k=65),
                dict(k=128), dict(q=off(q, 4)), dict(g=off(p.g, 8)),
                # what the coarse entries reject
                dict(plane=null), dict(flag=null), dict(plane=off(p.plane, 2))):
        assert call(**bad) == -1, bad
        assert who in eng.lib.ffr_last_error(eng._h), bad
    assert call(m=off(m, 4), tag=off(tag, 4), sub=off(sub, 4)) == 0      # 4-byte alignment is all the words need
    # the k rules: the exact filtered search alone, certified zeroed
    for kw in (dict(k=33), dict(k=64), dict(k=65, distinct=0), dict(k=128, distinct=0), dict(k=65, distinct=0, sub=null, u=null)):
        cert.fill_(1)
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        assert cert.tolist() == [0] * 4, kw
    assert call(k=32) == 0 and call(k=64, distinct=0) == 0
    torch.cuda.synchronize()
    assert cert.tolist() == [1] * 4                                   # G = 100 <= k' = 128
    # G = 0: all padding, nothing certified, NULL gallery pointers allowed
    s.fill_(0), i.fill_(0), u.fill_(0), cert.fill_(1)
    gone = dict(G=0, g=null, n=null, plane=null, flag=null, tag=null, sub=null)
    assert call(**gone) == 0 and call(cert=null, **gone) == 0
    torch.cuda.synchronize()
    assert cert.tolist() == [0] * 4
    assert torch.all(i.reshape(-1)[:40] == -1) and torch.all(u.reshape(-1)[:40] == -1) and torch.all(s.reshape(-1)[:40] == float('-inf'))
    assert call(u=null, distinct=0, **gone) == 0 and call(u=null, distinct=1, **gone) == -1 and call(**dict(gone, m=null)) == -1
    u.fill_(7)
    assert call(sub=null, u=null, distinct=0) == 0                    # without subjects top_subject is not touched
    torch.cuda.synchronize()
    assert torch.all(u == 7)
    # the binding
    tag, sub, m = tag[:100], sub[:100], m[:4]
    out = eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 10)
    assert len(out) == 2 and out[0].shape == (4, 10) and out[1].dtype == torch.int64
    assert len(eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 10, return_certified=True)) == 3
    a = eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 10, subjects=sub, distinct=True, return_certified=True)
    assert len(a) == 4 and a[2].dtype == torch.int32 and a[3].dtype == torch.int32
    assert same(a, eng.search_coarse_filtered(q, 1, g, p.plane, p.flag, tag.to(torch.int64), 10, subjects=sub.to(torch.int64),
                                              distinct=True, return_certified=True))
    es, ei = eng.search_coarse_filtered(q, m, g[:0], p.plane[:0], p.flag, tag[:0], 5)
    assert torch.all(ei == -1) and torch.all(es == float('-inf'))
    for bad in (lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 10, distinct=True),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 65, subjects=sub, distinct=True),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 129),
                lambda: eng.search_coarse_filtered(q, m[:3], g, p.plane, p.flag, tag, 10),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag[:99], 10),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane[:50], p.flag, tag, 10),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane.float(), p.flag, tag, 10),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag.to(torch.int64), tag, 10),
                lambda: eng.search_coarse_filtered(q, -1, g, p.plane, p.flag, tag, 10),
                lambda: eng.search_coarse_filtered(q, m, g, p.plane, p.flag, tag, 10, subjects=sub[:99]),
                lambda: eng.search_coarse_filtered(q.cpu(), m, g, p.plane, p.flag, tag, 10)):
        with pytest.raises(RuntimeError):
            bad()


def test_profile_counts_one_launch_under_score(eng):
    Q, G = 40, 5000
    q, p = rand_rows(Q, 101), Packed(eng, rand_rows(5000, 102))
    sub = (torch.arange(G, device='cuda') // 8).to(torch.int32)
    tag, m = dev(tags_of('one', G, 103)), dev(masks_of(Q))
    torch.cuda.synchronize()

    def profiled(fn):
        fn()
        torch.cuda.synchronize()
        eng.profile_enable(True)
        eng.profile_read()
        fn()
        st = eng.profile_read()
        eng.profile_enable(False)
        assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * Q * G * 512 and st['score']['ms'] > 0
        assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
        return st['score']['bytes']
    for distinct in (True, False):
        got = profiled(lambda: eng.search_coarse_filtered(q, m, p.g, p.plane, p.flag, tag, 10, gallery_norms=p.norms, subjects=sub,
                                                          distinct=distinct))
        assert got == profiled(lambda: eng.search_coarse_subjects(q, p.g, p.plane, p.flag, sub, 10, gallery_norms=p.norms,
                                                                  distinct=distinct)) + 4.0 * G + 4.0 * Q
    got = profiled(lambda: eng.search_coarse_filtered(q, m, p.g, p.plane, p.flag, tag, 10, gallery_norms=p.norms))
    assert got == profiled(lambda: eng.search_coarse(q, p.g, p.plane, p.flag, 10, gallery_norms=p.norms)) + 4.0 * G + 4.0 * Q


def test_beyond_one_chunk(eng):
    """G = 2^20 + 129 rows, probes planted at rows 3, 2^20 - 1 and G - 1: the smallest shape at which the 64-bit chunk base of
    the tag plane (tag + c0) in the pass over the bf16 plane can go wrong."""
    G, k = (1 << 20) + 129, 10
    gal = Gallery(eng, capacity=G, subjects=True)
    gal.build_tags()
    step = 1 << 18
    for lo in range(0, G, step):
        n = min(step, G - lo)
        rows = torch.arange(lo, lo + n, device='cuda')
        gal.add(rand_rows(n, 1000 + lo), (rows % 131072).to(torch.int32), tags=(1 + (rows >> 20)).to(torch.int32))
    gal.build_plane()                              # tag 1 in the first chunk, 2 in the second
    gal.remove([5])
    g = gal.embeddings
    planted = [3, (1 << 20) - 1, G - 1]
    q = torch.cat((g[planted] + 0.01 * rand_rows(3, 41), g[planted] + 0.01 * rand_rows(3, 43), rand_rows(2, 42)), 0)
    mask = dev([3, 3, 3, 2, 2, 1, 1, 2])
    p = Packed.__new__(Packed)
    p.g, p.norms, p.plane, p.flag = g, gal.norms, gal.plane, gal.flag
    for distinct in (True, False):
        cert = check(eng, p, q, mask, gal.tags, k, gal.subjects, distinct)
        print('distinct=%s: certified %d of 8' % (distinct, int(cert.sum())))
    gal.shortlist_filtered = True
    s, u, i = gal.search_subjects(q, k, mask=mask)
    assert i[:3, 0].tolist() == planted and bool((i[5] < 1 << 20).all()) and bool((i[3] >= 1 << 20).all()) and bool((i[6] < 1 << 20).all())
    assert int(i[4, 0]) != (1 << 20) - 1 and bool((i[7] >= 1 << 20).all()) and int((i[7] >= 0).sum()) == 10
