"""Incremental clustering on the device (include/ffrnet.h: ffr_cluster_extend; Engine.cluster_extend, cluster.extend,
cluster.Incremental).

The contract under test: a clustering extended by new rows EQUALS the clustering of all rows at once -- torch.equal with
Engine.cluster over everything, and equal to the float64 oracle of tests/cluster_extend_ref.py wherever no float64 score
lies within 1e-3 of the threshold (the library's fp32 score is within 1e-6 of the float64 cosine, tests/test_gpu_search.py;
every such test asserts that margin first).  Where there is no margin (thresholds taken from the scores themselves) the
reference is Engine.cluster itself, bit for bit: the rectangle must compute the bits of the triangle."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_extend_ref as xref
import cluster_ref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
_PLANTED = {}


def planted(N):
    """(emb float32 numpy, oracle rep of all rows, float64 scores) of the shared recipe at N rows, computed once."""
    if N not in _PLANTED:
        emb = cluster_ref.planted(N)[0]
        rep, S = cluster_ref.cluster_oracle(emb, THR)
        for a in (emb, rep, S):
            a.setflags(write=False)
        _PLANTED[N] = (emb, rep, S)
    return _PLANTED[N]


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


def rand_rows(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn((n, 512), device='cuda', generator=g)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared arrays are read-only


def arange(lo, hi):
    return torch.arange(lo, hi, device='cuda', dtype=torch.int64)


def flat_prior(rep_old, N):
    return torch.cat((rep_old, arange(rep_old.numel(), N)))


# the old/new boundary on, just before and just after a tile (32) and a step (128); one new row, one old row, no new rows;
# at 4129 chunks of several steps.  MERGES: splits at which a new row joins two clusters that are separate among the old rows
SPLITS = [(1, 0), (1, 1), (2, 1), (33, 32), (129, 128)] + [(168, k) for k in (0, 1, 84, 96, 100, 167, 168)] \
    + [(1000, k) for k in (31, 32, 33, 127, 128, 129, 999)] + [(4129, k) for k in (1000, 2064, 4096, 4128)]
MERGES = {(168, 84), (168, 96), (168, 100), (4129, 1000), (4129, 2064)}


@pytest.mark.parametrize('N,n_old', SPLITS)
def test_extension_equals_the_full_clustering(eng, N, n_old):
    emb, want, S = planted(N)
    assert cluster_ref.margin(S, THR) > MARGIN
    d = dev(emb)
    rep_old = eng.cluster(d[:n_old], THR)
    old_want = cluster_ref.union_find(n_old, cluster_ref.upper_edges(S[:n_old, :n_old], THR))
    assert np.array_equal(rep_old.cpu().numpy(), old_want)
    rep_new = eng.cluster_extend(d, THR, flat_prior(rep_old, N), n_old)
    assert rep_new.dtype == torch.int64 and rep_new.shape == (N,)
    assert torch.equal(rep_new, eng.cluster(d, THR))
    got = rep_new.cpu().numpy()
    assert np.array_equal(got, xref.extend_from_scores(S, THR, flat_prior(rep_old, N).cpu().numpy(), n_old))
    assert np.array_equal(got, want)
    assert np.all(got[:n_old] <= old_want)
    merged = int((want[:n_old] != old_want).sum())
    print('N %d n_old %d: %d old rows change their label' % (N, n_old, merged))
    if (N, n_old) in MERGES:
        assert merged > 0                                                 # old rows are flattened again


def test_three_batches_through_incremental(eng):
    emb, want, S = planted(168)
    assert cluster_ref.margin(S, THR) > MARGIN
    d = dev(emb)
    inc = fc.Incremental(eng, THR)
    assert [inc.add(d[:50]), inc.add(d[50:100]), inc.add(d[100:])] == [0, 50, 100] and len(inc) == 168
    once = fc.cluster(eng, d, THR)
    assert torch.equal(inc.rep, once.rep) and np.array_equal(inc.rep.cpu().numpy(), want)
    c = inc.clusters
    assert c.n_clusters == once.n_clusters == 43 and torch.equal(c.cluster_id, once.cluster_id) and torch.equal(c.sizes, once.sizes)
    assert torch.equal(inc.embeddings, d) and torch.equal(inc.norms, eng.row_norms(d))
    assert torch.equal(inc.templates(), fc.templates(eng, d, once))
    # the functional form, from a Clusters and from a rep
    head = fc.cluster(eng, d[:100], THR)
    assert torch.equal(fc.extend(eng, d, THR, head).rep, once.rep)
    assert torch.equal(fc.extend(eng, d, THR, head.rep, norms=eng.row_norms(d)).rep, once.rep)
    stale, now = fc.changes(head.rep, once.rep)
    assert torch.equal(now, once.rep[stale]) and bool((now < stale).all())
    assert stale.numel() == int(((head.rep == arange(0, 100)) & (once.rep[:100] != arange(0, 100))).sum())


def test_no_margin_rectangle_equals_triangle_bitwise(eng, synth_rows):
    emb = synth_rows
    n = emb.size(0)
    s, i = eng.search(emb, emb, n)
    S = torch.full((n, n), float('nan'), device='cuda').scatter_(1, i, s)
    assert not torch.isnan(S).any()
    ranked = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    # each threshold IS one of the scores, so the strict > is exercised on equal bits
    picks = [ranked[(ranked.numel() - 1) // 2].item()] + [ranked[int(q * (ranked.numel() - 1))].item()
                                                         for q in (0.9, 0.97, 0.99, 0.997, 0.9995)]
    Sn = S.cpu().numpy()
    seen = set()
    for thr in picks:
        full = eng.cluster(emb, thr)
        seen.add(int(full.unique().numel()))
        for n_old in (64, 96):
            prior = flat_prior(eng.cluster(emb[:n_old], thr), n)
            got = eng.cluster_extend(emb, thr, prior, n_old)
            assert torch.equal(got, full), (thr, n_old)
            assert np.array_equal(got.cpu().numpy(), xref.extend_from_scores(Sn, np.float32(thr), prior.cpu().numpy(), n_old))
    assert len(seen) > 1                                                  # the thresholds do not all give one blob


def test_must_links(eng):
    eye = torch.eye(512, device='cuda')
    # 257 orthonormal rows tied in threes, nothing old: no score is an edge, the labels are the ties
    rows = eye[:257].contiguous()
    prior = arange(0, 257) // 3 * 3
    assert torch.equal(eng.cluster_extend(rows, THR, prior, 0), prior)
    assert torch.equal(eng.cluster_extend(rows, THR, prior, 200), prior)
    # a link plus a scored edge: a ~ b by prior, b ~ c by score (equal rows), d alone
    rows = eye[[0, 1, 1, 2]].contiguous()
    prior = torch.tensor([0, 0, 2, 3], device='cuda')
    for n_old in (0, 1, 2):
        assert eng.cluster_extend(rows, THR, prior, n_old).tolist() == [0, 0, 0, 3], n_old
    for n_old in (3, 4):                                                  # c is old: (b, c) is not scored
        assert eng.cluster_extend(rows, THR, prior, n_old).tolist() == [0, 0, 2, 3], n_old
    # the link the other way round: b ~ c by prior, a ~ b by score
    rows = eye[[1, 1, 2, 3]].contiguous()
    assert eng.cluster_extend(rows, THR, torch.tensor([0, 1, 1, 3], device='cuda'), 1).tolist() == [0, 0, 0, 3]
    # a chain prior: legal, walked hop by hop
    rows = eye[:5].contiguous()
    chain = torch.tensor([0, 0, 1, 2, 3], device='cuda')
    for n_old in (0, 3, 5):
        assert eng.cluster_extend(rows, THR, chain, n_old).tolist() == [0] * 5, n_old
    # track ids through the helpers
    c = fc.extend(eng, eye[:6].contiguous(), THR, arange(0, 2), must_link=[9, 4, 9, 4])
    assert c.rep.tolist() == [0, 1, 2, 3, 2, 3] and c.n_clusters == 4


def test_seed_reads_a_forward_entry_as_the_row_itself(eng):
    # prior[i] = j with i < j < N and prior[j] = j: in bounds and acyclic even for a seed without its guard, which would join
    # i to j; the contract says row i starts alone.  Straight through the C ABI: nothing validates in front of the kernel
    rows = torch.eye(512, device='cuda')[:40].contiguous()
    prior = arange(0, 40)
    prior[2], prior[7], prior[33] = 5, 39, 34
    rep = torch.full((40,), -1, device='cuda', dtype=torch.int64)
    P = native._ptr
    for n_old in (0, 20, 40):
        rep.fill_(-1)
        rc = eng.lib.ffr_cluster_extend(eng._h, P(rows), C.c_void_p(0), n_old, 40, 512, THR, P(prior), P(rep), eng._stream())
        assert rc == 0
        assert torch.equal(rep, arange(0, 40)), n_old
    assert torch.equal(eng.cluster_extend(rows, THR, prior, 20, validate=False), arange(0, 40))
    # the binding refuses out-of-contract entries before any launch
    for i, v in ((2, 5), (0, -1), (39, 40), (39, 1 << 40), (5, -(1 << 40))):
        bad = arange(0, 40)
        bad[i] = v
        with pytest.raises(RuntimeError):
            eng.cluster_extend(rows, THR, bad, 20)


def test_in_place_no_new_rows_and_empty(eng):
    emb, want, S = planted(168)
    d = dev(emb)
    prior = flat_prior(eng.cluster(d[:84], THR), 168)
    keep = prior.clone()
    out = eng.cluster_extend(d, THR, prior, 84, out=prior)
    assert out.data_ptr() == prior.data_ptr() and np.array_equal(prior.cpu().numpy(), want)
    # straight through the C ABI with rep == prior
    buf = keep.clone()
    P = native._ptr
    assert eng.lib.ffr_cluster_extend(eng._h, P(d), C.c_void_p(0), 84, 168, 512, THR, P(buf), P(buf), eng._stream()) == 0
    assert np.array_equal(buf.cpu().numpy(), want)
    # N_old = N scores nothing: equal rows stay apart, the prior comes back flattened
    same = rand_rows(1, 5).expand(7, 512).contiguous()
    deep = torch.tensor([0, 0, 1, 2, 4, 4, 5], device='cuda')
    assert eng.cluster_extend(same, THR, deep, 7).tolist() == [0, 0, 0, 0, 4, 4, 4]
    assert eng.cluster_extend(same, THR, deep, 6).tolist() == [0] * 7
    assert torch.equal(eng.cluster_extend(d, THR, dev(want), 168), dev(want))
    # N = 0
    none = eng.cluster_extend(d[:0], THR, arange(0, 0), 0)
    assert none.shape == (0,) and none.dtype == torch.int64
    assert fc.extend(eng, d[:0], THR, arange(0, 0)).n_clusters == 0
    inc = fc.Incremental(eng, THR)
    assert inc.add(d[:0]) == 0 and len(inc) == 0 and inc.templates().shape == (0, 512)


def test_worst_contention(eng):
    same = rand_rows(1, 5).expand(257, 512).contiguous()
    prior = flat_prior(torch.zeros(128, device='cuda', dtype=torch.int64), 257)
    assert torch.all(eng.cluster_extend(same, THR, prior, 128) == 0)     # every edge hits one root
    basis = torch.zeros((257, 512), device='cuda')
    basis[torch.arange(257), torch.arange(257) % 3] = 1.0
    rep = eng.cluster_extend(basis, THR, flat_prior(arange(0, 129) % 3, 257), 129)
    assert torch.equal(rep, arange(0, 257) % 3)


def test_deterministic_and_shares_the_scratch_with_cluster():
    e = ffrnet_amd.Engine(0)
    small, want_small, _ = planted(168)
    big, want_big, _ = planted(1000)
    ds, db = dev(small), dev(big)
    prior = flat_prior(e.cluster(ds[:84], THR), 168)
    r1 = e.cluster_extend(ds, THR, prior, 84)
    g1 = e.generation()
    r2 = e.cluster_extend(ds, THR, prior, 84)
    assert torch.equal(r1, r2) and e.generation() == g1                  # the scratch is reused
    assert np.array_equal(r1.cpu().numpy(), want_small)
    # the extension grows the scratch: captured graphs must re-capture
    pb = flat_prior(dev(cluster_ref.union_find(500, cluster_ref.upper_edges(planted(1000)[2][:500, :500], THR))), 1000)
    rb = e.cluster_extend(db, THR, pb, 500)
    assert e.generation() != g1 and np.array_equal(rb.cpu().numpy(), want_big)
    g2 = e.generation()
    # the two calls alternate on one handle at different N
    assert np.array_equal(e.cluster(ds, THR).cpu().numpy(), want_small)
    assert torch.equal(e.cluster_extend(db, THR, pb, 500), rb)
    assert np.array_equal(e.cluster(db, THR).cpu().numpy(), want_big)
    assert torch.equal(e.cluster_extend(ds, THR, prior, 84), r1)
    assert e.generation() == g2
    e.close()


def test_arguments(eng):
    emb = rand_rows(100, 51)
    norms = eng.row_norms(emb)
    prior = arange(0, 100)
    rep = torch.empty((100,), device='cuda', dtype=torch.int64)
    P = native._ptr
    null = C.c_void_p(0)
    ok = (P(emb), P(norms), 60, 100, 512, 0.5, P(prior), P(rep), eng._stream())
    names = ['emb', 'norms', 'N_old', 'N', 'dim', 'thr', 'prior', 'rep', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_cluster_extend(eng._h, *a)

    def message():
        return (eng.lib.ffr_last_error(eng._h) or b'').decode()

    assert call() == 0
    assert call(norms=null) == 0
    assert call(dim=256) == -6 and '512' in message()
    for bad in (dict(N=-1, N_old=0), dict(N=1 << 31), dict(thr=float('nan')), dict(rep=null), dict(emb=null),
                dict(emb=C.c_void_p(emb.data_ptr() + 4)), dict(N_old=-1), dict(N_old=101), dict(prior=null),
                dict(prior=C.c_void_p(prior.data_ptr() + 4))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_extend' in message(), bad
    assert call(N=0, N_old=0) == 0 and call(N=0, N_old=0, emb=null, rep=null, prior=null) == 0
    assert call(N=0, N_old=1) == -1
    # the binding: wrong device, wrong shape, wrong dtype, n_old out of range
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb.cpu(), 0.5, prior, 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb[:, :256].contiguous(), 0.5, prior, 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior[:50], 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior.int(), 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior.cpu(), 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior, 101)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior, -1)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior, 60, norms=norms[:50])
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, float('nan'), prior, 60)
    with pytest.raises(RuntimeError):
        eng.cluster_extend(emb, 0.5, prior, 60, out=torch.empty((50,), device='cuda', dtype=torch.int64))


@pytest.mark.parametrize('n_old', [0, 100, 299, 300])
def test_profile_counts_one_score_launch(eng, n_old):
    emb = rand_rows(300, 61)
    prior = flat_prior(eng.cluster(emb[:n_old], THR), 300)
    eng.cluster_extend(emb, THR, prior, n_old)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    eng.cluster_extend(emb, THR, prior, n_old)
    st = eng.profile_read()
    eng.profile_enable(False)
    n_new = 300 - n_old
    assert st['score']['launches'] == 1 and st['score']['flops'] == 512.0 * (2 * n_old * n_new + n_new * (n_new - 1))
    assert st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
