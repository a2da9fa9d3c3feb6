"""Clustering on the device (include/ffrnet.h: ffr_cluster_threshold, ffr_cluster_templates; ffrnet_amd.cluster).

The oracle is tests/cluster_ref.py: float64 cosine, the edges of the upper triangle, a sequential union-find.  The
library's fp32 score is within 1e-6 of the float64 cosine (tests/test_gpu_search.py), so wherever no float64 score lies
within 1e-3 of the threshold both must find the same edges and the labels must be EQUAL; every such test asserts that
margin first.  Where there is no margin (thresholds taken from the scores themselves) the oracle's union-find runs on the
edges of the scores ffr_search_topk returns, which the clustering promises to reproduce bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_ref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native
from ffrnet_amd.search import Gallery, identification_rates

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
_PLANTED = {}


def planted(N):
    """(emb float32 numpy, truth, info, oracle rep, float64 scores) of the shared recipe at N rows, computed once."""
    if N not in _PLANTED:
        emb, truth, info = cluster_ref.planted(N)
        rep, S = cluster_ref.cluster_oracle(emb, THR)
        for a in (emb, truth, rep, S):
            a.setflags(write=False)
        _PLANTED[N] = (emb, truth, info, rep, S)
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


def search_matrix(eng, emb):
    """S[i, j] = the score ffr_search_topk gives for probe i and gallery row j, all N <= 128 of them."""
    n = emb.size(0)
    s, i = eng.search(emb, emb, n)
    S = torch.full((n, n), float('nan'), device='cuda')
    S.scatter_(1, i, s)
    assert not torch.isnan(S).any()
    return S


def test_planted_clusters_exact(eng):
    emb, truth, info, want, S = planted(168)
    assert cluster_ref.margin(S, THR) > MARGIN
    rep = eng.cluster(dev(emb), THR)
    assert rep.dtype == torch.int64 and rep.shape == (168,)
    got = rep.cpu().numpy()
    assert np.array_equal(got, want)
    z = info['zero']
    assert got[z] == z and (got == z).sum() == 1                       # the zero row is a singleton
    assert len(set(got[info['chain']].tolist())) == 1                   # the chain needs more than one hop
    assert len(np.unique(got)) == 43
    # norms handed in or computed in the call: the same labels
    assert torch.equal(eng.cluster(dev(emb), THR, norms=eng.row_norms(dev(emb))), rep)


# 4129 = 4096 + 33: up to 1000 rows a chunk is one 128-row step; at 4129 a chunk has several, so blocks start at a later
# step of their chunk and the prefetch crosses a step boundary inside it; the last tile holds one probe
@pytest.mark.parametrize('N', [1, 2, 31, 32, 33, 127, 128, 129, 257, 1000, 4129])
def test_tile_and_step_boundaries(eng, N):
    emb, truth, info, want, S = planted(N)
    assert cluster_ref.margin(S, THR) > MARGIN
    got = eng.cluster(dev(emb), THR).cpu().numpy()
    assert np.array_equal(got, want)


def test_no_margin_agrees_with_search_scores(eng, synth_rows):
    emb = synth_rows
    S = search_matrix(eng, emb)
    off = S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]
    Sn = S.cpu().numpy()
    # the median of the issue, and scores from the sparse end, where single edges decide the components; each threshold IS
    # one of the scores, so the strict > is exercised on equal bits
    ranked = torch.sort(off).values
    picks = [ranked[(ranked.numel() - 1) // 2].item()] + [ranked[int(q * (ranked.numel() - 1))].item()
                                                         for q in (0.9, 0.97, 0.99, 0.997, 0.9995)]
    seen = set()
    for thr in picks:
        want = cluster_ref.union_find(128, cluster_ref.upper_edges(Sn, np.float32(thr)))
        got = eng.cluster(emb, thr).cpu().numpy()
        assert np.array_equal(got, want), thr
        seen.add(len(np.unique(want)))
    assert len(seen) > 1                                                  # the thresholds do not all give one blob


def test_worst_contention(eng):
    same = rand_rows(1, 5).expand(257, 512).contiguous()
    assert torch.all(eng.cluster(same, THR) == 0)                         # every edge hits one root
    basis = torch.zeros((257, 512), device='cuda')
    basis[torch.arange(257), torch.arange(257) % 3] = 1.0
    rep = eng.cluster(basis, THR)
    assert torch.equal(rep, torch.arange(257, device='cuda') % 3)


def test_threshold_is_strict(eng):
    a, b = rand_rows(1, 6)[0], rand_rows(1, 7)[0]
    a = a / a.norm()
    b = b - (b @ a) * a
    b = b / b.norm()
    emb = torch.stack((a, b, a)).contiguous()
    s02 = search_matrix(eng, emb)[0, 2].item()                           # the fp32 score of the equal rows, about 1
    assert abs(s02 - 1.0) < 1e-6
    assert eng.cluster(emb, s02).tolist() == [0, 1, 2]                   # s is not > s
    below = float(np.nextafter(np.float32(s02), np.float32(-1.0)))
    assert eng.cluster(emb, below).tolist() == [0, 1, 0]


def test_deterministic_and_independent_of_scratch_growth():
    e = ffrnet_amd.Engine(0)
    emb = dev(planted(168)[0])
    r1 = e.cluster(emb, THR)
    g1 = e.generation()
    r2 = e.cluster(emb, THR)
    assert torch.equal(r1, r2) and e.generation() == g1                  # the scratch is reused
    big = e.cluster(dev(planted(1000)[0]), THR)
    assert e.generation() != g1                                           # it grew: captured graphs must re-capture
    assert np.array_equal(big.cpu().numpy(), planted(1000)[3])
    g2 = e.generation()
    assert torch.equal(e.cluster(emb, THR), r1) and e.generation() == g2
    e.close()


def template_tolerance(emb, rep):
    """Per component, from the inputs alone (float64).  u_r = x_r / |x_r|, s = sum of the m rows of a cluster, A = sum |u_r|
    per component.  Sequential fp32 summation errs by at most e = (m - 1) 2^-24 A per component (recursive summation,
    first order).  t = s / |s|: an error e of s moves t by at most e / |s| + |t| |e|_2 / |s| per component.  The roundings of
    the terms themselves (norm, division) and of the final normalisation are relative to each term: 4 ulp (2^-23) of
    A / |s|, which for a singleton is 4 ulp of the component itself."""
    x = np.asarray(emb, dtype=np.float64)
    n = np.sqrt((x * x).sum(1))
    u = np.divide(x, n[:, None], out=np.zeros_like(x), where=n[:, None] > 0)
    tol = []
    for r in np.unique(rep):
        rows = u[rep == r]
        m = rows.shape[0]
        A = np.abs(rows).sum(0)
        s = rows.sum(0)
        sn = np.sqrt((s * s).sum())
        if sn == 0:
            tol.append(np.zeros(512))
            continue
        e = (m - 1) * 2.0 ** -24 * A
        tol.append(e / sn + np.abs(s / sn) * np.sqrt((e * e).sum()) / sn + 4 * 2.0 ** -23 * A / sn)
    return np.stack(tol)


def test_templates_match_float64(eng):
    emb, truth, info, rep, S = planted(168)
    d = dev(emb)
    c = fc.cluster(eng, d, THR)
    assert np.array_equal(c.rep.cpu().numpy(), rep) and c.n_clusters == 43
    t = fc.templates(eng, d, c)
    assert t.shape == (43, 512) and t.dtype == torch.float32
    want = cluster_ref.templates64(emb, rep)
    err = np.abs(t.cpu().numpy().astype(np.float64) - want)
    tol = template_tolerance(emb, rep)
    worst = float((err - tol).max())
    print('templates: max |err| %.3e, max (err - tol) %.3e, max err / tol %.3f' % (err.max(), worst, (err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol)
    cid = c.cluster_id.cpu().numpy()
    sizes = c.sizes.cpu().numpy()
    assert sizes.sum() == 168 and np.array_equal(sizes, np.bincount(cid))
    # a singleton's template is its own normalised row; the zero row's is zero
    single = [r for r in range(168) if sizes[cid[r]] == 1 and r != info['zero']]
    assert single
    for r in single:
        x = emb[r].astype(np.float64)
        assert np.all(np.abs(t[cid[r]].cpu().numpy() - x / np.linalg.norm(x)) <= 4 * 2.0 ** -23 * np.abs(x / np.linalg.norm(x)))
    assert not t[cid[info['zero']]].any()
    # unit rows, bitwise repeatable, the same with the norms handed in
    nz = torch.ones(43, dtype=torch.bool)
    nz[cid[info['zero']]] = False
    assert (t[nz.cuda()].double().norm(dim=1) - 1).abs().max().item() < 1e-6
    assert torch.equal(fc.templates(eng, d, c), t)
    assert torch.equal(fc.templates(eng, d, c, norms=eng.row_norms(d)), t)
    # the plain call checks its index tensors
    order, offsets = fc.member_order(c)
    assert torch.equal(eng.cluster_templates(d, order, offsets), t)
    with pytest.raises(RuntimeError):
        eng.cluster_templates(d, order + 1, offsets)
    with pytest.raises(RuntimeError):
        eng.cluster_templates(d, order, offsets.flip(0))


def test_end_to_end_enrolment(eng):
    emb, truth, info, rep, S = planted(168)
    d = dev(emb)
    c = fc.cluster(eng, d, THR)
    gal = Gallery(eng)
    assert gal.add(fc.templates(eng, d, c)) == 0 and len(gal) == c.n_clusters
    # Gallery row r is cluster id r.  Every member of a compact cluster finds its cluster's template first.  The chain is
    # one cluster only by single link: it spans 184 degrees, its end points are orthogonal to its own template, so its
    # probe is the member nearest the float64 template.  The zero row scores 0 against everything and is no probe.
    t64 = cluster_ref.templates64(emb, rep)
    cid = c.cluster_id.cpu().numpy()
    chain = info['chain']
    mid = chain[int(np.argmax(emb[chain].astype(np.float64) @ t64[cid[chain[0]]]))]      # chain points are unit vectors
    compact = [r for r in range(168) if r != info['zero'] and r not in chain]
    s, i = gal.search(d[compact], 1)
    assert torch.equal(i[:, 0], c.cluster_id[compact])
    assert s.min().item() > 0.8
    # one member of each cluster as probe: rank-1 identification over the templates is perfect
    probes = sorted([int(np.nonzero(rep == r)[0][0]) for r in np.unique(rep) if r not in (info['zero'], rep[mid])] + [mid])
    assert len(probes) == c.n_clusters - 1
    s, i = gal.search(d[probes], 1)
    assert torch.equal(i[:, 0], c.cluster_id[probes])
    rates = identification_rates(i, dev(truth)[probes], dev(truth)[c.rep.unique()], ranks=(1,))
    assert rates[1] == 1.0
    assert fc.pairwise_scores(c.cluster_id, dev(truth)) == (1.0, 1.0, 1.0)
    assert fc.pairwise_scores(c.rep, dev(truth)) == (1.0, 1.0, 1.0)


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_arguments(eng):
    emb = rand_rows(100, 51)
    norms = eng.row_norms(emb)
    rep = torch.empty((100,), device='cuda', dtype=torch.int64)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    ok = (P(emb), P(norms), 100, 512, 0.5, P(rep), st)

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[['emb', 'norms', 'N', 'dim', 'thr', 'rep', 'st'].index(key)] = v
        return _rc(eng, 'ffr_cluster_threshold', *a)

    def message():
        return (eng.lib.ffr_last_error(eng._h) or b'').decode()

    assert call() == 0
    assert call(norms=null) == 0
    assert call(dim=256) == -6 and '512' in message()
    for bad in (dict(N=-1), dict(N=1 << 31), dict(thr=float('nan')), dict(rep=null), dict(emb=null),
                dict(emb=C.c_void_p(emb.data_ptr() + 4))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_threshold' in message(), bad
    assert call(N=0) == 0 and call(N=0, emb=null, rep=null) == 0
    # templates: the same conventions
    order = torch.arange(100, device='cuda')
    offsets = torch.arange(101, device='cuda')
    out = torch.empty((100, 512), device='cuda')
    okt = (P(emb), P(norms), P(order), P(offsets), 100, 512, P(out), st)

    def callt(**kw):
        a = list(okt)
        for key, v in kw.items():
            a[['emb', 'norms', 'order', 'offsets', 'C', 'dim', 'out', 'st'].index(key)] = v
        return _rc(eng, 'ffr_cluster_templates', *a)

    assert callt() == 0 and callt(norms=null) == 0
    assert callt(dim=256) == -6
    for bad in (dict(C=-1), dict(order=null), dict(offsets=null), dict(out=null), dict(emb=null),
                dict(emb=C.c_void_p(emb.data_ptr() + 4))):
        assert callt(**bad) == -1, bad
        assert 'ffr_cluster_templates' in message(), bad
    assert callt(C=0) == 0
    # the binding: wrong device, wrong shape, an empty collection
    with pytest.raises(RuntimeError):
        eng.cluster(emb.cpu(), 0.5)
    with pytest.raises(RuntimeError):
        eng.cluster(emb[:, :256].contiguous(), 0.5)
    with pytest.raises(RuntimeError):
        eng.cluster(emb, 0.5, norms=norms[:50])
    with pytest.raises(RuntimeError):
        eng.cluster(emb, float('nan'))
    none = fc.cluster(eng, emb[:0], 0.5)
    assert none.n_clusters == 0 and none.rep.numel() == 0 and fc.templates(eng, emb[:0], none).shape == (0, 512)


def test_profile_counts_clustering_under_score(eng):
    emb = rand_rows(300, 61)
    eng.cluster(emb, THR)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    eng.cluster(emb, THR)
    st = eng.profile_read()
    eng.profile_enable(False)
    assert st['score']['launches'] == 1 and st['score']['flops'] == 300.0 * 299 * 512 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
