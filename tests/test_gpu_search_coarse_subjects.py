"""The certified bf16 shortlist over a subject-labelled gallery, on the device (include/ffrnet.h:
ffr_search_topk_coarse_subjects; ffrnet_amd.search.Gallery(subjects=True).build_plane()).

The oracle is the exact subject search, Engine.search_subjects: every comparison is torch.equal on scores, indices and
subjects, no tolerance.  Equality alone would pass if every probe fell back to the exact search, so the certified share is
asserted where the CPU model of tests/search_coarse_subjects_ref.py says what it must be."""
import ctypes as C

import pytest
import torch

import ffrnet_amd
import search_coarse_ref as cref
import search_coarse_subjects_ref as ref
from ffrnet_amd import native
from ffrnet_amd.search import Gallery, shortlist_size

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
    """base + 0.05 * noise: every cosine between two of them is within 2 * COARSE_EPS of every other"""
    return rand_rows(1, base_seed) + 0.05 * rand_rows(n, seed)


def cpu_corr(n, seed, base_seed=77):
    return cpu_rows(1, base_seed) + 0.05 * cpu_rows(n, seed)


def spread_subjects(G, per=8):
    """subject[g] = g % ceil(G / per), int32 on the device: a person's rows spread over the gallery"""
    return (torch.arange(G, device='cuda') % max(1, (G + per - 1) // per)).to(torch.int32)


def planted_rows(Q, G, seed, per=8, noise=0.7):
    """The planted recipe on the device: a centre per person, rows = centre[g % nsub] + noise * randn, probes of Q people"""
    nsub = max(1, (G + per - 1) // per)
    cent = rand_rows(nsub, seed)
    g = cent[torch.arange(G, device='cuda') % nsub] + noise * rand_rows(G, seed + 1)
    return cent[(37 * torch.arange(Q, device='cuda')) % nsub] + noise * rand_rows(Q, seed + 2), g


def subject_gallery(eng, g, subj, gone=None):
    """A gallery with subjects that got its plane afterwards, `gone` withdrawn"""
    gal = Gallery(eng, subjects=True)
    gal.add(g, subj)
    gal.build_plane()
    if gone is not None and len(gone):
        gal.remove(gone)
    return gal


def some_subjects(subj, frac, seed):
    """a seeded share of the subject ids (at least one)"""
    ids = torch.unique(subj[subj >= 0]).cpu()
    n = max(1, int(round(frac * ids.numel())))
    return ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))[:n]]


def check_equal(eng, gal, q, k, distinct, **kw):
    """The gallery's search == Engine.search_subjects over the same rows -> the certified flags [Q] (bool, on the host)."""
    if distinct:
        s, u, i = gal.search_subjects(q, k, **kw)
    else:
        s, i = gal.search(q, k, **kw)
    es, ei, eu = eng.search_subjects(q, gal.embeddings, gal.subjects, k, gallery_norms=gal.norms, distinct=distinct, **kw)
    torch.cuda.synchronize()
    assert s.shape == es.shape and torch.equal(s, es) and torch.equal(i, ei)
    if distinct:
        assert u.dtype == torch.int32 and torch.equal(u, eu)
    cert = gal.last_certified
    assert cert.shape == (q.size(0),) and cert.dtype == torch.int32 and bool(((cert == 0) | (cert == 1)).all())
    return cert.bool().cpu()


def check_raw(eng, gal, q, k, distinct, index_base=0):
    """Engine.search_coarse_subjects == Engine.search_subjects, the subject plane included, in either mode"""
    got = eng.search_coarse_subjects(q, gal.embeddings, gal.plane, gal.flag, gal.subjects, k, gallery_norms=gal.norms,
                                     index_base=index_base, distinct=distinct, return_certified=True)
    want = eng.search_subjects(q, gal.embeddings, gal.subjects, k, gallery_norms=gal.norms, index_base=index_base,
                               distinct=distinct)
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return got[3].bool().cpu()


CASES = [(1, 1000, 1), (31, 1000, 10), (33, 65537, 10), (32, 65537, 32), (257, 4096, 10), (32, 10, 10), (31, 1, 1),
         (5, 200, 33), (5, 200, 65), (4, 0, 10)]


@pytest.mark.parametrize('data', ['rand', 'corr', 'planted'])
@pytest.mark.parametrize('Q,G,k', CASES)
def test_equals_the_exact_subject_search(eng, Q, G, k, data):
    """The ten shapes on Gaussian, correlated and planted rows, identities and rows, nothing removed and a seeded 10 % of the
    subjects removed."""
    if data == 'planted':
        q, g = planted_rows(Q, G, 13 * Q + k)
    else:
        rows = rand_rows if data == 'rand' else corr_rows
        q, g = rows(Q, 11 * Q + k), rows(G, 7 * G + 1)
    subj = spread_subjects(G)
    for removed in (False, True):
        gal = subject_gallery(eng, g, subj, some_subjects(subj, 0.1, G + k) if removed and G else None)
        n_live = int((gal.subjects >= 0).sum())
        for distinct in (True, False):
            if distinct and k > 64:
                with pytest.raises(RuntimeError):
                    gal.search_subjects(q, k)
                continue
            cert = check_raw(eng, gal, q, k, distinct)
            assert torch.equal(cert, check_equal(eng, gal, q, k, distinct))
            kp = shortlist_size(k, distinct)
            print('%s removed=%s distinct=%s: certified %d of %d' % (data, removed, distinct, int(cert.sum()), Q))
            if kp is None or G == 0:
                assert not bool(cert.any())              # the exact search alone
            elif n_live < kp or G <= kp:
                assert bool(cert.all())                  # the shortlist is the live gallery
            elif kp < 128:
                # A certificate says that every live row outside the k' of the shortlist scores strictly below the k-th listed
                # score, so a probe with more than k' live rows at or above it cannot hold one (a list with fewer than k
                # entries counts every live row).  The exact top 128 live rows count up to 128 of them.
                s = eng.search_subjects(q, g, gal.subjects, k, gallery_norms=gal.norms, distinct=distinct)[0]
                es, ei, _ = eng.search_subjects(q, g, gal.subjects, 128, gallery_norms=gal.norms, distinct=False)
                must_fall_back = (((es >= s[:, k - 1:k]) & (ei >= 0)).sum(1) > kp).cpu()
                assert not bool((cert & must_fall_back).any())
                if data == 'corr':
                    assert not bool(cert.any())


@pytest.mark.parametrize('G,per,noise', [(65537, 8, 1.0), (65537, 8, 0.5), (20000, 4, 0.7)])
def test_planted_identities_certify(eng, G, per, noise):
    """The planted shapes of tests/test_host_search_coarse_subjects.py, the very rows: the CPU model, with eps widened by
    3e-4, certifies every one of the 33 probes at (k = 10, identities) and at (k = 32, identities); the device, whose coarse
    scores differ from the model's only in the rounding of the accumulation, must certify >= 90 %."""
    rows, subject, cent = ref.planted(G, per, noise, 5)
    q, _ = ref.planted_probes(cent, 33, noise, 9)
    gal = subject_gallery(eng, rows.cuda(), subject.cuda())
    for k in (10, 32):
        cert = check_equal(eng, gal, q.cuda(), k, True)
        print('k = %d: certified %d of 33' % (k, int(cert.sum())))
        assert int(cert.sum()) >= 0.9 * 33
        check_equal(eng, gal, q.cuda(), k, False)


def test_one_person_with_more_rows_than_the_shortlist(eng):
    """200 near-copies of probe 0 under one subject: the shortlist (k' = 64) holds that subject alone, fewer than k = 5
    identities in a full list, no certificate; the answer is still the exact one.  The Gaussian probe beside it certifies."""
    g = cpu_rows(3000, 41)
    q = cpu_rows(2, 42)
    g[:200] = q[0] + 0.01 * cpu_rows(200, 43)
    subject = torch.arange(3000) + 10
    subject[:200] = 3
    assert ref.search(q, g, subject, 5, True)[3].tolist() == [False, True]        # the model
    gal = subject_gallery(eng, g.cuda(), subject.cuda())
    cert = check_equal(eng, gal, q.cuda(), 5, True)
    assert cert.tolist() == [False, True]
    s, u, i = gal.search_subjects(q.cuda(), 5)
    assert int(u[0, 0]) == 3 and int((u[0] == 3).sum()) == 1 and int(i[0, 0]) < 200
    # as rows the 200 copies are the answer, and a list of 32 that holds the 5 best of them is not proven to: no row is withdrawn
    check_equal(eng, gal, q.cuda(), 5, False)


def test_removal(eng):
    rows, subject, cent = ref.planted(4096, 8, 0.7, 51)
    q, pick = ref.planted_probes(cent, 16, 0.7, 52)
    gal = subject_gallery(eng, rows.cuda(), subject.cuda())
    qd = q.cuda()
    s, u, i = gal.search_subjects(qd, 10)
    assert u[:, 0].cpu().tolist() == pick.tolist()
    # the subject that leads for probe 0 is withdrawn: neither mode returns it, and the probes still certify (the model, with
    # eps widened by 3e-4, certifies all 16 on these rows)
    gone = int(u[0, 0])
    subject2 = subject.clone()
    subject2[subject == gone] = -1
    for distinct in (True, False):
        assert bool(ref.search(q, rows, subject2, 10, distinct, eps=cref.COARSE_EPS + 3e-4)[3].all())
    assert gal.remove([gone]) == int((subject == gone).sum())
    cert = check_equal(eng, gal, qd, 10, True)
    s2, u2, i2 = gal.search_subjects(qd, 10)
    assert bool(cert.all()) and not bool((u2 == gone).any()) and int(u2[0, 0]) == int(u[0, 1])
    cert = check_equal(eng, gal, qd, 10, False)
    rs, ri = gal.search(qd, 10)
    assert bool(cert.all()) and not bool((gal.subjects[ri] < 0).any()) and not bool((subject.cuda()[ri] == gone).any())
    # 20 live rows of 1000, correlated (no score separates them): the shortlist is the live gallery, every probe is certified,
    # and the padding is exact
    g = corr_rows(1000, 53)
    qc = corr_rows(5, 54)
    subj = torch.full((1000,), -1, device='cuda', dtype=torch.int32)
    subj[::50] = (torch.arange(20, device='cuda') % 7).to(torch.int32)
    gal = Gallery(eng, subjects=True)
    gal.add(g, torch.arange(1000, device='cuda') % 7)
    gal.build_plane()
    gal.subjects[:] = subj
    for k, distinct in ((10, True), (10, False), (32, False)):
        assert bool(check_equal(eng, gal, qc, k, distinct).all())
    s, u, i = gal.search_subjects(qc, 10)
    assert bool((u[:, 7:] == -1).all()) and bool((i[:, 7:] == -1).all()) and bool(torch.isinf(s[:, 7:]).all()) and bool((u[:, :7] >= 0).all())
    rs, ri = gal.search(qc, 32)
    assert bool((ri[:, 20:] == -1).all()) and bool((ri[:, :20] % 50 == 0).all())
    # every row removed: all padding
    gal.subjects[:] = -1
    for distinct in (True, False):
        check_equal(eng, gal, qc, 10, distinct)
    s, u, i = gal.search_subjects(qc, 10)
    assert bool((u == -1).all()) and bool((i == -1).all()) and bool(torch.isinf(s).all())


@pytest.mark.parametrize('nsub', [40, 2])
def test_ties_across_the_shortlist_edge(eng, nsub):
    """40 equal rows over 40 subjects, and over 2: more ties than k' = 32 hold, fewer than k' = 64."""
    g = rand_rows(3000, 5)
    copies = torch.randperm(3000, generator=torch.Generator().manual_seed(9))[:40].sort().values
    src = int(copies[0])                                   # the first of them is the row the others copy: 40 equal rows
    g[copies.cuda()] = g[src].clone()
    subj = (100 + torch.arange(3000)).to(torch.int32)
    subj[copies] = (torch.arange(40) % nsub).to(torch.int32)
    q = torch.cat((g[src:src + 1] * 0.5 + rand_rows(1, 6) * 1e-3, rand_rows(3, 7)), 0)
    gal = subject_gallery(eng, g, subj.cuda())
    # rows, k = 2, k' = 32 < 40 ties: c_k' ties s_k up to rounding, no certificate for the probe of the copies
    cert = check_equal(eng, gal, q, 2, False)
    s, i = gal.search(q, 2)
    assert not bool(cert[0]) and i[0].tolist() == copies[:2].tolist() and s[0, 0] == s[0, 1]
    cert = check_equal(eng, gal, q, 16, False)
    assert not bool(cert[0])
    # k' = 64 > 40 ties: rows at k = 32, identities at k = 2 and 16
    cert = check_equal(eng, gal, q, 32, False)
    s, i = gal.search(q, 32)
    assert i[0].tolist() == copies[:32].tolist()
    print('%d subjects, rows k = 32: certified %s' % (nsub, cert.tolist()))
    for k in (2, 16):
        cert = check_equal(eng, gal, q, k, True)
        s, u, i = gal.search_subjects(q, k)
        n = min(k, nsub)
        assert i[0, :n].tolist() == copies[:n].tolist() and u[0, :n].tolist() == list(range(n))
        assert torch.equal(s[0, :n], s[0, :1].expand(n)) and (n == k or s[0, n] < s[0, 0])
        print('%d subjects, identities k = %d: certified %s' % (nsub, k, cert.tolist()))
    # one more copy than a shortlist of 64 holds, each its own subject: no certificate for identities either
    g2 = g.clone()
    more = torch.randperm(3000, generator=torch.Generator().manual_seed(10))[:70]
    g2[more.cuda()] = g[src].clone()
    gal2 = subject_gallery(eng, g2, (100 + torch.arange(3000)).to(torch.int32).cuda())
    assert not bool(check_equal(eng, gal2, q, 2, True)[0]) and not bool(check_equal(eng, gal2, q, 32, False)[0])


def test_unsafe_norms(eng):
    subj = spread_subjects(500)
    g = rand_rows(500, 31)
    g[7] *= 1e-30                     # every square underflows: norm 0 over a row that is not zero
    g[9] = 0.0
    q = torch.cat((rand_rows(4, 32), g[7:8] * 1e30 * 1e30), 0)     # the probe of row 7, its norm overflows
    gal = subject_gallery(eng, g, subj)
    assert int(gal.flag.item()) == 1
    for distinct in (True, False):
        assert not bool(check_equal(eng, gal, q, 10, distinct).any())
    g2 = rand_rows(500, 31)
    g2[11] *= 1e-20                   # norm 2.3e-19 < 2^-60
    gal2 = subject_gallery(eng, g2, subj)
    assert int(gal2.flag.item()) == 1 and not bool(check_equal(eng, gal2, q[:4], 10, True).any())
    # the flag does not look at the mask: the unsafe row withdrawn, it stays set
    gal2.remove([int(subj[11])])
    assert int(gal2.flag.item()) == 1 and not bool(check_equal(eng, gal2, q[:4], 10, True).any())
    # a zero row is safe: the gallery certifies, an unsafe probe alone does not
    g3 = rand_rows(500, 31)
    g3[9] = 0.0
    gal3 = subject_gallery(eng, g3, subj)
    assert int(gal3.flag.item()) == 0
    big = torch.cat((rand_rows(4, 32), rand_rows(1, 33) * 1e30, rand_rows(1, 34) * 1e-30, torch.zeros((1, 512), device='cuda')), 0)
    for distinct in (True, False):
        assert check_equal(eng, gal3, big, 10, distinct).tolist() == [True] * 4 + [False] * 3
    # the flag is sticky: a later unsafe row switches the certificates off for good, compact() included
    gal3.add(g2[11:12], torch.tensor([900], device='cuda'))
    gal3.add(rand_rows(5, 35), torch.arange(901, 906, device='cuda'))
    assert int(gal3.flag.item()) == 1 and not bool(check_equal(eng, gal3, big[:4], 10, True).any())
    gal3.remove([900])
    gal3.compact()
    assert int(gal3.flag.item()) == 1 and not bool(check_equal(eng, gal3, big[:4], 10, False).any())


def test_deterministic_and_batch_independent(eng):
    """241 Gaussian probes, which certify, and 16 correlated ones, which do not, in one batch: row r of the 257-probe call is
    the 1-probe call, results and certified flag."""
    q = torch.cat((cpu_rows(241, 61), cpu_corr(16, 62)), 0).cuda()
    g = torch.cat((cpu_rows(20000, 63), cpu_corr(2000, 64)), 0).cuda()
    subj = spread_subjects(22000)
    gal = subject_gallery(eng, g, subj, some_subjects(subj, 0.1, 65))
    for k, distinct in ((10, True), (10, False)):
        first = gal.search_subjects(q, k) if distinct else gal.search(q, k)
        c1 = gal.last_certified
        again = gal.search_subjects(q, k) if distinct else gal.search(q, k)
        assert all(torch.equal(a, b) for a, b in zip(first, again)) and torch.equal(c1, gal.last_certified)
        assert int(c1[:241].sum()) >= 217 and int(c1[241:].sum()) == 0
        for r in range(257):
            one = gal.search_subjects(q[r:r + 1], k) if distinct else gal.search(q[r:r + 1], k)
            assert all(torch.equal(a[0], b[r]) for a, b in zip(one, first)) and torch.equal(gal.last_certified[0], c1[r]), r
        check_equal(eng, gal, q, k, distinct)


def test_shards_and_leave_one_out(eng):
    q, g = planted_rows(33, 65537, 71)
    subj = spread_subjects(65537)
    gone = some_subjects(subj, 0.1, 72)
    one = subject_gallery(eng, g, subj, gone)
    live = one.subjects
    for k, distinct in ((10, True), (32, True), (10, False), (64, False)):
        bounds = [0, k // 2, 30000, 65537]
        parts = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            shard = subject_gallery(eng, g[lo:hi], subj[lo:hi], gone)
            parts.append(eng.search_coarse_subjects(q, shard.embeddings, shard.plane, shard.flag, shard.subjects, k,
                                                    gallery_norms=shard.norms, index_base=lo, distinct=distinct))
        merged = eng.topk_merge_subjects(*[torch.stack([p[j] for p in parts]) for j in range(3)], distinct=distinct)
        whole = eng.search_coarse_subjects(q, g, one.plane, one.flag, live, k, gallery_norms=one.norms, distinct=distinct)
        exact = eng.search_subjects(q, g, live, k, gallery_norms=one.norms, distinct=distinct)
        for a, b, c in zip(merged, whole, exact):
            assert torch.equal(a, b) and torch.equal(b, c), (k, distinct)
    # leave-one-out under the mask, with and without an index base
    me = torch.tensor([5, 17, 60, 65536], device='cuda')
    me = me[live[me] >= 0]
    assert me.numel() >= 2
    plain = Gallery(eng, subjects=True)
    plain.add(g, subj)
    plain.remove(gone)
    for base in (0, 1000):
        ls, li = one.search(g[me], 10, self_index=me, index_base=base)
        es, ei = plain.search(g[me], 10, self_index=me, index_base=base)
        assert torch.equal(ls, es) and torch.equal(li, ei) and not bool((li == me[:, None] + base).any())
    assert one.last_certified is not None and plain.last_certified is None


def test_gallery_build_plane_add_and_compact(eng):
    g = rand_rows(3561, 81)
    subj = spread_subjects(3561)
    q = rand_rows(9, 82)
    gal = Gallery(eng, subjects=True)
    first = 0
    for n in (60, 1, 2000):                     # grown in pieces, no plane yet
        assert gal.add(g[first:first + n], subj[first:first + n]) == first
        first += n
    assert gal.coarse is False and not hasattr(gal, '_plane') and gal.last_certified is None
    gal.search_subjects(q, 10)
    assert gal.last_certified is None
    gal.build_plane()
    whole = torch.empty((3561, 512), device='cuda', dtype=torch.int16)
    flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    eng.coarse_pack(g, eng.row_norms(g), whole, flag)
    assert gal.coarse is True and torch.equal(gal.plane, whole[:2061]) and int(gal.flag.item()) == 0
    plane_was = gal._plane
    gal.build_plane()                           # twice: nothing happens
    assert gal._plane is plane_was and torch.equal(gal.plane, whole[:2061])
    assert gal.add(g[2061:], subj[2061:]) == 2061           # add() after it packs what it appends (and reallocates here)
    assert torch.equal(gal.plane, whole) and torch.equal(gal.embeddings, g) and int(gal.flag.item()) == 0
    for distinct in (True, False):
        check_equal(eng, gal, q, 10, distinct)
    # compact(): every score bit stays, and the plane is the re-packed plane of the kept rows
    gone = some_subjects(subj, 0.2, 83)
    gal.remove(gone)
    s2, u2, i2 = gal.search_subjects(q, 10)
    rs2, ri2 = gal.search(q, 10)
    old_to_new = gal.compact()
    keep = ~torch.isin(subj, gone.cuda().to(torch.int32))
    assert len(gal) == int(keep.sum()) and torch.equal(gal.embeddings, g[keep]) and torch.equal(gal.subjects, subj[keep])
    packed = torch.empty((len(gal), 512), device='cuda', dtype=torch.int16)
    eng.coarse_pack(gal.embeddings, gal.norms, packed, flag)
    assert torch.equal(gal.plane, packed) and torch.equal(gal.plane, whole[keep])
    s3, u3, i3 = gal.search_subjects(q, 10)
    assert torch.equal(s3, s2) and torch.equal(u3, u2) and torch.equal(i3, old_to_new[i2])
    rs3, ri3 = gal.search(q, 10)
    assert torch.equal(rs3, rs2) and torch.equal(ri3, old_to_new[ri2])
    for distinct in (True, False):
        check_equal(eng, gal, q, 10, distinct)
    # a gallery without subjects switches the pass on the same way
    plain = Gallery(eng)
    plain.add(g)
    plain.build_plane()
    s, i = plain.search(q, 10)
    es, ei = eng.search(q, g, 10)
    assert torch.equal(plain.plane, whole) and torch.equal(s, es) and torch.equal(i, ei) and plain.last_certified is not None
    # the constructor combination still raises, and says where to go
    with pytest.raises(RuntimeError, match='shortlist does not know subjects') as e:
        Gallery(eng, coarse=True, subjects=True)
    assert 'build_plane()' in str(e.value)


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_arguments(eng):
    q, g = rand_rows(4, 91), rand_rows(100, 92)
    n = eng.row_norms(g)
    plane = torch.empty((100, 512), device='cuda', dtype=torch.int16)
    flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    eng.coarse_pack(g, n, plane, flag)
    sub = torch.arange(101, device='cuda', dtype=torch.int32)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    u = torch.empty((4, 129), device='cuda', dtype=torch.int32)
    cert = torch.ones((4,), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    ok = (P(q), 4, P(g), P(n), P(plane), P(flag), P(sub), 100, 512, 10, 0, 1, P(s), P(i), P(u), P(cert), st)
    names = ['q', 'Q', 'g', 'n', 'plane', 'flag', 'sub', 'G', 'dim', 'k', 'base', 'distinct', 's', 'i', 'u', 'cert', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return _rc(eng, 'ffr_search_topk_coarse_subjects', *a)

    assert call() == 0 and call(distinct=0) == 0 and call(cert=null) == 0 and call(cert=null, distinct=0) == 0
    assert call(dim=256) == -6
    for bad in (dict(k=0), dict(k=129, distinct=0), dict(Q=0), dict(G=-1), dict(q=null), dict(g=null), dict(n=null),
                dict(plane=null), dict(flag=null), dict(sub=null), dict(s=null), dict(i=null), dict(u=null),
                dict(plane=C.c_void_p(plane.data_ptr() + 2)), dict(g=C.c_void_p(g.data_ptr() + 4)),
                dict(q=C.c_void_p(q.data_ptr() + 4)), dict(sub=C.c_void_p(sub.data_ptr() + 2)), dict(distinct=2),
                dict(distinct=-1), dict(k=65), dict(k=128)):
        assert call(**bad) == -1, bad
    assert call(sub=C.c_void_p(sub.data_ptr() + 4)) == 0            # 4-byte alignment is all the subjects need
    # the k rules: the exact search alone, certified zeroed
    for kw in (dict(k=33), dict(k=64), dict(k=65, distinct=0), dict(k=128, distinct=0)):
        cert.fill_(1)
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        assert cert.tolist() == [0] * 4, kw
    assert call(k=32) == 0 and call(k=64, distinct=0) == 0
    torch.cuda.synchronize()
    assert cert.tolist() == [1] * 4                                  # G = 100 <= k' = 128
    cert.fill_(1)
    assert call(G=0, g=null, n=null, plane=null, flag=null, sub=null) == 0          # the null rule of the gallery at G = 0
    assert call(G=0, g=null, n=null, plane=null, flag=null, sub=null, cert=null) == 0
    torch.cuda.synchronize()
    assert cert.tolist() == [0] * 4
    assert bool((i.view(-1)[:40] == -1).all()) and bool((u.view(-1)[:40] == -1).all()) and bool(torch.isinf(s.view(-1)[:40]).all())
    # the binding: k, devices, dtypes and shapes
    sub = sub[:100]
    out = eng.search_coarse_subjects(q, g, plane, flag, sub, 10)
    assert len(out) == 3 and out[0].shape == (4, 10) and out[2].dtype == torch.int32
    assert len(eng.search_coarse_subjects(q, g, plane, flag, sub, 10, return_certified=True)) == 4
    b = eng.search_coarse_subjects(q, g, plane, flag, sub.to(torch.int64), 10)
    assert all(torch.equal(x, y) for x, y in zip(out, b))
    es = eng.search_coarse_subjects(q, g[:0], plane[:0], flag, sub[:0], 5)
    assert bool((es[1] == -1).all()) and bool((es[2] == -1).all())
    for bad in (lambda: eng.search_coarse_subjects(q, g, plane, flag, sub, 65),
                lambda: eng.search_coarse_subjects(q, g, plane, flag, sub, 129, distinct=False),
                lambda: eng.search_coarse_subjects(q, g, plane.float(), flag, sub, 10),
                lambda: eng.search_coarse_subjects(q, g, plane[:50], flag, sub, 10),
                lambda: eng.search_coarse_subjects(q, g, plane, flag, sub[:99], 10),
                lambda: eng.search_coarse_subjects(q, g, plane, flag, sub.float(), 10),
                lambda: eng.search_coarse_subjects(q, g, plane, flag, sub.cpu(), 10),
                lambda: eng.search_coarse_subjects(q.cpu(), g, plane, flag, sub, 10),
                lambda: eng.search_coarse_subjects(q, g, plane, flag.to(torch.int64), sub, 10)):
        with pytest.raises(RuntimeError):
            bad()


def test_profile_counts_one_launch_under_score(eng):
    q, g = rand_rows(40, 101), rand_rows(5000, 102)
    gal = subject_gallery(eng, g, spread_subjects(5000), [3, 4])
    for distinct in (True, False):
        gal.search_subjects(q, 10) if distinct else gal.search(q, 10)
        torch.cuda.synchronize()
        eng.profile_enable(True)
        eng.profile_read()
        gal.search_subjects(q, 10) if distinct else gal.search(q, 10)
        st = eng.profile_read()
        eng.profile_enable(False)
        assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * 40 * 5000 * 512 and st['score']['ms'] > 0
        assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0


def test_beyond_one_chunk(eng):
    """G = 2^20 + 129 rows, subjects g % 131072, probes planted at rows 3, 2^20 - 1 and G - 1: the smallest shape at which
    the 64-bit chunk base of the subject plane (subject + c0) in the coarse pass can go wrong."""
    G, k = (1 << 20) + 129, 10
    gal = Gallery(eng, capacity=G, subjects=True)
    step = 1 << 18
    for lo in range(0, G, step):
        n = min(step, G - lo)
        gal.add(rand_rows(n, 1000 + lo), (torch.arange(lo, lo + n, device='cuda') % 131072).to(torch.int32))
    gal.build_plane()
    gal.remove([5, 131070])                       # rows 5, 131077, ..., 2^20 + 5 and 131070, ..., 2^20 - 2: the mask in both chunks
    g = gal.embeddings
    planted = [3, (1 << 20) - 1, G - 1]
    q = torch.cat((g[planted] + 0.01 * rand_rows(3, 41), g[(1 << 20) - 2:(1 << 20) - 1] + 0.01 * rand_rows(1, 43), rand_rows(4, 42)), 0)
    for distinct in (True, False):
        cert = check_equal(eng, gal, q, k, distinct)
        print('distinct=%s: certified %d of 8' % (distinct, int(cert.sum())))
    s, u, i = gal.search_subjects(q, k)
    assert i[:3, 0].tolist() == planted and u[:3, 0].tolist() == [p % 131072 for p in planted]
    assert int(i[3, 0]) != (1 << 20) - 2 and not bool((u == 131070).any()) and not bool((u == 5).any())
