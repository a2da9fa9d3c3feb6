"""Removal from a single-link clustering on the device (include/ffrnet.h: ffr_cluster_remove; Engine.cluster_remove,
cluster.remove, cluster.Incremental.remove, cluster.removal_changes).

The contract under test: the labels after a removal EQUAL the clustering of the surviving rows alone -- torch.equal with
Engine.cluster over the compacted rows, and equal to both forms of the float64 oracle of tests/cluster_remove_ref.py
wherever no float64 score lies within 1e-3 of the threshold (the library's fp32 score is within 1e-6 of the float64 cosine,
tests/test_gpu_search.py; every such test asserts that margin first).  Where there is no margin (thresholds taken from the
scores themselves) the reference is Engine.cluster over the compacted rows, bit for bit: the walk over the listed rows must
compute the bits of the triangle, also for a pair it meets with the roles exchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_density_ref as dref
import cluster_ref
import cluster_remove_ref as rref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
_DATA = {}


def bridged(N):
    """(emb float32 numpy, float64 scores, oracle rep of all rows, info) of planted_bridged(N), computed once, read-only."""
    if N not in _DATA:
        emb, truth, info = dref.planted_bridged(N)
        S = cluster_ref.cosine64(emb)
        rep = cluster_ref.union_find(N, cluster_ref.upper_edges(S, THR))
        for a in (emb, S, rep):
            a.setflags(write=False)
        _DATA[N] = (emb, S, rep, info, cluster_ref.margin(S, THR))
    return _DATA[N][:4]


def margin(N):
    bridged(N)
    return _DATA[N][4]


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def synth_rows(state_dicts):
    """f_new of 128 synthetic images: embeddings of the real network, strongly correlated."""
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    f_new, _ = e.embed(ffrnet_amd.synth.synth_images(128, seed=77).cuda(), want_f=False)
    torch.cuda.synchronize()
    e.close()
    return f_new


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared arrays are read-only


def arange(lo, hi):
    return torch.arange(lo, hi, device='cuda', dtype=torch.int64)


def compact_labels(rep, keep):
    """device labels in the old numbering, device bool keep -> the survivors' labels in compact numbering"""
    old_to_new = torch.full((keep.numel(),), -1, device='cuda', dtype=torch.int64)
    old_to_new[keep] = arange(0, int(keep.sum()))
    return old_to_new[rep[keep]]


def pattern_rows(name, N, rep, info):
    if name == 'every_rep':
        return np.unique(rep[np.bincount(rep, minlength=N)[rep] > 1]).tolist()
    return {'nothing': [], 'everything': list(range(N)), 'bridge': [info['bridge'][0]], 'chain_mid': [info['chain'][2]],
            'chain_end': [info['chain'][0]], 'zero': [info['zero']], 'first': [0], 'last': [N - 1],
            'every_second': list(range(0, N, 2))}[name]


PATTERNS = ['nothing', 'everything', 'bridge', 'chain_mid', 'chain_end', 'zero', 'first', 'last', 'every_rep', 'every_second']


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('N', [20, 33, 129, 168, 1000, 4129])
def test_removal_equals_clustering_the_rest(eng, N, pattern):
    emb, S, rep_all, info = bridged(N)
    assert margin(N) > MARGIN
    d = dev(emb)
    rep_in = eng.cluster(d, THR)
    assert np.array_equal(rep_in.cpu().numpy(), rep_all)
    keep_np = rref.keep_without(N, pattern_rows(pattern, N, rep_all, info))
    keep = dev(keep_np)
    got = eng.cluster_remove(d, THR, rep_in, keep)
    assert got.dtype == torch.int64 and got.shape == (N,)
    g = got.cpu().numpy()
    aff = rref.affected(rep_all, keep_np)
    print('N %d %s: %d removed, m = %d' % (N, pattern, int((~keep_np).sum()), int(aff.sum())))
    assert np.all(g[~keep_np] == -1)
    assert np.array_equal(g[keep_np & ~aff], rep_all[keep_np & ~aff])                   # untouched clusters keep their label
    assert torch.equal(compact_labels(got, keep), eng.cluster(d[keep].contiguous(), THR))
    assert np.array_equal(g, rref.remove_from_scores(S, THR, rep_all, keep_np))
    assert np.array_equal(g, rref.survivors_only(S, THR, keep_np))
    chain, both = info['chain'], info['ident'][0] + info['ident'][1]
    if pattern == 'nothing':
        assert torch.equal(got, rep_in) and not aff.any()
    if pattern == 'everything':
        assert np.all(g == -1)
    if pattern == 'bridge':
        assert aff.sum() == 11 and len(set(rep_all[both].tolist())) == 1 and len(set(g[both].tolist())) == 2
    if pattern == 'chain_mid':
        assert aff.sum() == 5 and g[chain[0]] == g[chain[1]] != g[chain[3]] == g[chain[4]] == g[chain[5]]
    if pattern == 'chain_end':
        assert aff.sum() == 5 and len(set(g[chain[1:]].tolist())) == 1
    if pattern == 'zero':
        assert not aff.any() and np.array_equal(g[keep_np], rep_all[keep_np])
    if pattern == 'every_rep':
        assert aff.any() and np.all(g[aff] > rep_all[aff])                             # every affected label rises
        if N in (168, 1000, 4129):
            assert int(aff.sum()) == {168: 126, 1000: 751, 4129: 3097}[N]
    # the functional form: compact Clusters and the index maps
    c, old_to_new, kept = fc.remove(eng, d, THR, rep_in, keep=keep)
    assert torch.equal(c.rep, compact_labels(got, keep)) and torch.equal(kept, torch.nonzero(keep).reshape(-1))
    assert torch.equal(old_to_new[kept], arange(0, kept.numel())) and bool((old_to_new[~keep] == -1).all())


@pytest.mark.parametrize('m', [1, 2, 31, 32, 33, 127, 128, 129, 511, 512, 513])
def test_list_boundaries(eng, m):
    # hit clusters chosen so that exactly m rows are listed: tile (32), step (128) and multi-step edges in list positions
    N = 1000 if m <= 129 else 4129
    emb, S, rep_all, info = bridged(N)
    assert margin(N) > MARGIN
    rows = rref.pick_clusters_for(rep_all, m)
    assert rows is not None
    keep_np = rref.keep_without(N, rows)
    assert int(rref.affected(rep_all, keep_np).sum()) == m                   # the count the device reaches, from the oracle
    d, keep = dev(emb), dev(keep_np)
    got = eng.cluster_remove(d, THR, dev(rep_all), keep)
    assert np.array_equal(got.cpu().numpy(), rref.remove_from_scores(S, THR, rep_all, keep_np))
    assert np.array_equal(got.cpu().numpy(), rref.survivors_only(S, THR, keep_np))
    assert torch.equal(compact_labels(got, keep), eng.cluster(d[keep].contiguous(), THR))


def test_one_dense_cluster(eng):
    g = torch.Generator(device='cuda')
    g.manual_seed(11)
    centre = torch.nn.functional.normalize(torch.randn((1, 512), device='cuda', generator=g), dim=1)
    rows = (centre + 0.02 * torch.randn((300, 512), device='cuda', generator=g)).contiguous()
    rep_in = eng.cluster(rows, THR)
    assert bool((rep_in == 0).all())                        # every pair is an edge (cosine about 0.83)
    for gone in (0, 150):
        keep = torch.ones(300, device='cuda', dtype=torch.bool)
        keep[gone] = False
        a = eng.cluster_remove(rows, THR, rep_in, keep)
        b = eng.cluster_remove(rows, THR, rep_in, keep)
        want = torch.full((300,), 1 if gone == 0 else 0, device='cuda', dtype=torch.int64)
        want[gone] = -1
        assert torch.equal(a, want) and torch.equal(a, b)   # m = 299: one cluster, every union meets one root
        buf = rep_in.clone()
        out = eng.cluster_remove(rows, THR, buf, keep, out=buf)
        assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
        # straight through the C ABI with rep == rep_in
        buf = rep_in.clone()
        P = native._ptr
        assert eng.lib.ffr_cluster_remove(eng._h, P(rows), C.c_void_p(0), 300, 512, THR, P(buf), C.c_void_p(0), P(keep), P(buf),
                                          eng._stream()) == 0
        assert torch.equal(buf, want)


def test_no_margin_equals_the_triangle_bitwise(eng, synth_rows):
    emb = synth_rows
    n = emb.size(0)
    s, i = eng.search(emb, emb, n)
    S = torch.full((n, n), float('nan'), device='cuda').scatter_(1, i, s)
    assert not torch.isnan(S).any()
    ranked = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    # each threshold IS one of the scores, so the strict > is exercised on equal bits
    picks = [ranked[(ranked.numel() - 1) // 2].item()] + [ranked[int(q * (ranked.numel() - 1))].item()
                                                         for q in (0.9, 0.97, 0.99, 0.997, 0.9995)]
    seen, listed = set(), 0
    for thr in picks:
        full = eng.cluster(emb, thr)
        seen.add(int(full.unique().numel()))
        for rows in ([0], [n - 1], list(range(0, n, 5)), list(range(64, 96)), full.unique().tolist()):
            keep = torch.ones(n, device='cuda', dtype=torch.bool)
            keep[rows] = False
            got = eng.cluster_remove(emb, thr, full, keep)
            listed += int(rref.affected(full.cpu().numpy(), keep.cpu().numpy()).sum())
            assert bool((got[~keep] == -1).all())
            assert torch.equal(compact_labels(got, keep), eng.cluster(emb[keep].contiguous(), thr)), (thr, rows[:4])
    assert len(seen) > 1 and listed > 0                     # not one blob at every threshold, and pairs were scored


def test_must_links(eng):
    eye = torch.eye(512, device='cuda')
    # a, b, c orthogonal (no scored edge), one track: tied through c, which leaves
    rows = eye[:3].contiguous()
    tied = eng.cluster_extend(rows, THR, torch.tensor([0, 0, 0], device='cuda'), 0)
    assert tied.tolist() == [0, 0, 0]
    keep = torch.tensor([True, True, False], device='cuda')
    assert eng.cluster_remove(rows, THR, tied, keep, prior=torch.tensor([0, 0, 2], device='cuda')).tolist() == [0, 0, -1]
    assert eng.cluster_remove(rows, THR, tied, keep).tolist() == [0, 1, -1]
    # the first row of the group leaves: the others hang under the first survivor
    keep = torch.tensor([False, True, True], device='cuda')
    assert eng.cluster_remove(rows, THR, tied, keep, prior=torch.tensor([0, 1, 1], device='cuda')).tolist() == [-1, 1, 1]
    assert eng.cluster_remove(rows, THR, tied, keep).tolist() == [-1, 1, 2]
    # a link plus a scored edge among the survivors: x ~ y by score (equal rows), y ~ z by the track, w leaves
    rows = eye[[5, 0, 0, 1, 2]].contiguous()                # w, x, y, z, and one row of another cluster
    rep_in = torch.tensor([0, 0, 0, 0, 4], device='cuda')
    keep = torch.tensor([False, True, True, True, True], device='cuda')
    assert eng.cluster_remove(rows, THR, rep_in, keep, prior=torch.tensor([0, 1, 2, 2, 4], device='cuda')).tolist() == [-1, 1, 1, 1, 4]
    assert eng.cluster_remove(rows, THR, rep_in, keep).tolist() == [-1, 1, 1, 3, 4]
    # a link to an unaffected or a removed row is no link
    assert eng.cluster_remove(rows, THR, rep_in, keep, prior=torch.tensor([0, 0, 2, 0, 3], device='cuda'),
                              validate=False).tolist() == [-1, 1, 1, 3, 4]
    # through Incremental: equal to cluster.extend from scratch over the survivors with their labels
    emb, S, rep_all, info = bridged(168)
    d = dev(emb)
    track = torch.arange(168, device='cuda') // 3           # tracks of three consecutive rows, across identities
    inc = fc.Incremental(eng, THR)
    inc.add(d[:99], must_link=track[:99])                   # the batches end with a track: add() ties within a batch
    inc.add(d[99:], must_link=track[99:])
    gone = list(range(0, 168, 3)) + [info['bridge'][0], 167]
    old_to_new = inc.remove(gone)
    kept = torch.nonzero(old_to_new >= 0).reshape(-1)
    want = fc.extend(eng, d[kept].contiguous(), THR, arange(0, 0), must_link=track[kept])
    assert torch.equal(inc.rep, want.rep) and torch.equal(inc.embeddings, d[kept])
    c, o2, k2 = fc.remove(eng, d, THR, fc.extend(eng, d, THR, arange(0, 0), must_link=track), rows=gone, must_link=track)
    assert torch.equal(c.rep, want.rep) and torch.equal(o2, old_to_new) and torch.equal(k2, kept)


def test_stream_add_remove_add_remove(eng):
    emb, S, rep_all, info = bridged(1000)
    assert margin(1000) > MARGIN
    d = dev(emb)
    inc = fc.Incremental(eng, THR)
    ids = arange(0, 0)                                      # the side table a caller keeps: which row of d each row held is

    def check():
        held = d[ids].contiguous()
        once = fc.cluster(eng, held, THR)
        assert len(inc) == ids.numel() and torch.equal(inc.embeddings, held) and torch.equal(inc.norms, eng.row_norms(held))
        assert torch.equal(inc.rep, once.rep) and torch.equal(inc.templates(), fc.templates(eng, held, once))
        sub = ids.cpu().numpy()
        assert np.array_equal(inc.rep.cpu().numpy(), cluster_ref.union_find(sub.size, cluster_ref.upper_edges(S[np.ix_(sub, sub)], THR)))

    def renumber(old_to_new):
        out = torch.empty((int((old_to_new >= 0).sum()),), device='cuda', dtype=torch.int64)
        out[old_to_new[old_to_new >= 0]] = ids[old_to_new >= 0]
        return out

    assert inc.add(d[:600]) == 0
    ids = arange(0, 600)
    check()
    before = inc.rep.clone()
    m1 = inc.remove(arange(0, 200))                         # the oldest rows expire
    ids = renumber(m1)
    assert torch.equal(ids, arange(200, 600))
    check()
    assert inc.add(d[600:]) == 400
    ids = torch.cat((ids, arange(600, 1000)))
    check()
    rng = np.random.default_rng(3)
    gone = rng.choice(800, 100, replace=False)
    m2 = inc.remove(gone)
    ids = renumber(m2)
    check()
    # the maps compose: row r of the first 600 is now at m2[m1[r]] where it survived both
    comp = torch.where(m1 >= 0, m2[m1.clamp(min=0)], torch.full_like(m1, -1))
    alive = comp >= 0
    assert torch.equal(ids[comp[alive]], arange(0, 600)[alive])
    assert int(alive.sum()) == 400 - int((gone < 400).sum())
    # removal_changes on the labels before compaction names the clusters to recompute
    keep = torch.ones(600, device='cuda', dtype=torch.bool)
    keep[:200] = False
    after = eng.cluster_remove(d[:600], THR, before, keep)
    touched, now = fc.removal_changes(before, after)
    assert torch.equal(touched, torch.unique(before[:200]))
    assert torch.equal(now, torch.unique(after[keep & torch.isin(before, touched)]))
    assert bool((after[keep & ~torch.isin(before, touched)] == before[keep & ~torch.isin(before, touched)]).all())


def test_any_input_is_defined(eng):
    N = 168
    emb, S, rep_all, info = bridged(N)
    assert margin(N) > MARGIN
    d = dev(emb)
    rng = np.random.default_rng(17)
    big = np.iinfo(np.int64)
    P = native._ptr
    for trial in range(4):
        rep_in = rep_all.copy()
        prior = np.arange(N, dtype=np.int64)
        for arr in (rep_in, prior):
            where = rng.choice(N, 60, replace=False)
            arr[where[:12]] = rng.integers(-5, N + 5, 12)                           # around the range, forward entries too
            arr[where[12:20]] = [big.min, big.max, -1, N, N + 1, 1 << 31, 1 << 32, -(1 << 31)]
            arr[where[20:40]] = np.minimum(where[20:40] + rng.integers(1, 9, 20), N + 3)        # rep_in[x] > x
            arr[where[40:]] = (rng.random(20) * where[40:]).astype(np.int64)        # in range, but wrong
        keep_np = rng.integers(0, 256, N).astype(np.uint8)
        keep_np[rng.random(N) < 0.3] = 0
        rep = torch.full((N,), -7, device='cuda', dtype=torch.int64)
        d_rep_in, d_prior, d_keep = dev(rep_in), dev(prior), dev(keep_np)
        rc = eng.lib.ffr_cluster_remove(eng._h, P(d), C.c_void_p(0), N, 512, THR, P(d_rep_in), P(d_prior), P(d_keep), P(rep),
                                        eng._stream())
        assert rc == 0
        g = rep.cpu().numpy()
        assert np.all((g >= -1) & (g < N))
        assert np.array_equal(g, rref.remove_from_scores(S, THR, rep_in, keep_np, prior)), trial
        no_prior = eng.cluster_remove(d, THR, dev(rep_in), dev(keep_np), validate=False)
        assert np.array_equal(no_prior.cpu().numpy(), rref.remove_from_scores(S, THR, rep_in, keep_np)), trial
    # the binding refuses out-of-contract entries before any launch
    keep = torch.ones(N, device='cuda', dtype=torch.bool)
    for i, v in ((2, 5), (0, -1), (N - 1, N), (N - 1, 1 << 40)):
        bad = dev(rep_all)
        bad[i] = v
        with pytest.raises(RuntimeError):
            eng.cluster_remove(d, THR, bad, keep)
        with pytest.raises(RuntimeError):
            eng.cluster_remove(d, THR, dev(rep_all), keep, prior=bad)


def test_deterministic_and_shares_the_scratch():
    e = ffrnet_amd.Engine(0)
    small, Ss, rep_s, info_s = bridged(168)
    big, Sb, rep_b, info_b = bridged(1000)
    ds, db = dev(small), dev(big)
    ks, kb = dev(rref.keep_without(168, range(0, 168, 2))), dev(rref.keep_without(1000, range(0, 1000, 2)))
    e.cluster(ds, THR)
    r1 = e.cluster_remove(ds, THR, dev(rep_s), ks)
    g1 = e.generation()
    r2 = e.cluster_remove(ds, THR, dev(rep_s), ks)
    assert torch.equal(r1, r2) and e.generation() == g1                  # the scratch is reused
    rb = e.cluster_remove(db, THR, dev(rep_b), kb)
    assert e.generation() != g1                                           # a larger N grows it: captured graphs re-capture
    assert np.array_equal(rb.cpu().numpy(), rref.survivors_only(Sb, THR, rref.keep_without(1000, range(0, 1000, 2))))
    g2 = e.generation()
    # the calls alternate on one handle at different N
    assert np.array_equal(e.cluster(ds, THR).cpu().numpy(), rep_s)
    assert torch.equal(e.cluster_remove(db, THR, dev(rep_b), kb), rb)
    assert np.array_equal(e.cluster_extend(db, THR, dev(rep_b), 1000).cpu().numpy(), rep_b)
    assert torch.equal(e.cluster_remove(ds, THR, dev(rep_s), ks), r1)
    assert e.generation() == g2
    e.close()


def test_arguments(eng):
    g = torch.Generator(device='cuda')
    g.manual_seed(51)
    emb = torch.randn((100, 512), device='cuda', generator=g)
    norms = eng.row_norms(emb)
    rep_in, prior = arange(0, 100), arange(0, 100)
    keep = torch.ones(100, device='cuda', dtype=torch.uint8)
    keep[::3] = 0
    rep = torch.full((100,), -7, device='cuda', dtype=torch.int64)
    P = native._ptr
    null = C.c_void_p(0)
    ok = (P(emb), P(norms), 100, 512, 0.5, P(rep_in), P(prior), P(keep), P(rep), eng._stream())
    names = ['emb', 'norms', 'N', 'dim', 'thr', 'rep_in', 'prior', 'keep', 'rep', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_cluster_remove(eng._h, *a)

    def message():
        return (eng.lib.ffr_last_error(eng._h) or b'').decode()

    assert call(dim=256) == -6 and '512' in message()
    for bad in (dict(N=-1), dict(N=1 << 31), dict(thr=float('nan')), dict(rep=null), dict(emb=null), dict(rep_in=null),
                dict(keep=null), dict(emb=C.c_void_p(emb.data_ptr() + 4)), dict(rep_in=C.c_void_p(rep_in.data_ptr() + 4)),
                dict(prior=C.c_void_p(prior.data_ptr() + 4)), dict(rep=C.c_void_p(rep.data_ptr() + 4)),
                dict(norms=C.c_void_p(norms.data_ptr() + 2))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_remove' in message(), bad
    torch.cuda.synchronize()
    assert bool((rep == -7).all())                          # refused before any launch: nothing was written
    assert call(N=0) == 0 and call(N=0, emb=null, rep=null, rep_in=null, keep=null, prior=null) == 0
    torch.cuda.synchronize()
    assert bool((rep == -7).all())
    assert call() == 0 and call(norms=null) == 0 and call(prior=null) == 0
    want = arange(0, 100)
    want[::3] = -1
    assert torch.equal(rep, want)                           # random rows: every row its own cluster
    # the binding: wrong device, shape, dtype
    kb = keep != 0
    for args, kw in (((emb.cpu(), 0.5, rep_in, kb), {}), ((emb[:, :256].contiguous(), 0.5, rep_in, kb), {}),
                     ((emb, 0.5, rep_in[:50], kb), {}), ((emb, 0.5, rep_in.int(), kb), {}), ((emb, 0.5, rep_in.cpu(), kb), {}),
                     ((emb, 0.5, rep_in, kb[:50]), {}), ((emb, 0.5, rep_in, kb.cpu()), {}), ((emb, 0.5, rep_in, kb.float()), {}),
                     ((emb, 0.5, rep_in, kb), dict(prior=prior[:50])), ((emb, 0.5, rep_in, kb), dict(norms=norms[:50])),
                     ((emb, float('nan'), rep_in, kb), {}),
                     ((emb, 0.5, rep_in, kb), dict(out=torch.empty((50,), device='cuda', dtype=torch.int64)))):
        with pytest.raises(RuntimeError):
            eng.cluster_remove(*args, **kw)
    none = eng.cluster_remove(emb[:0], 0.5, rep_in[:0], kb[:0])
    assert none.shape == (0,) and none.dtype == torch.int64


def test_profile_counts_one_score_launch_without_flops(eng):
    emb, S, rep_all, info = bridged(168)
    d, rep_in, keep = dev(emb), dev(rep_all), dev(rref.keep_without(168, [info['bridge'][0]]))
    eng.cluster_remove(d, THR, rep_in, keep)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    eng.cluster_remove(d, THR, rep_in, keep)
    st = eng.profile_read()
    eng.profile_enable(False)
    # the pair count is on the device only: the record carries 0 flops, and the time
    assert st['score']['launches'] == 1 and st['score']['flops'] == 0.0 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
