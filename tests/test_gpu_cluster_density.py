"""Density-gated clustering on the device (include/ffrnet.h: ffr_cluster_density; ffrnet_amd.cluster.density).

The oracle is tests/cluster_density_ref.py.  As in test_gpu_cluster.py: the library's fp32 score is within 1e-6 of the
float64 cosine, so wherever no float64 score lies within 1e-3 of the threshold both find the same edges, and where in
addition no border row has two core neighbours the labels, kinds and degrees must be EQUAL to the float64 oracle's; every
such test asserts the margin first.  Where there is no margin, or where equal scores decide a border row, the oracle runs
on the scores ffr_search_topk returns, which the clustering promises to reproduce bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_density_ref as dref
import cluster_ref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native
from ffrnet_amd.search import Gallery

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
_BRIDGED, _ORACLE = {}, {}


def bridged(N):
    """(emb float32 numpy, truth, info, float64 scores) of planted_bridged(N), computed once."""
    if N not in _BRIDGED:
        emb, truth, info = dref.planted_bridged(N)
        S = cluster_ref.cosine64(emb)
        for a in (emb, truth, S):
            a.setflags(write=False)
        _BRIDGED[N] = (emb, truth, info, S)
    return _BRIDGED[N]


def bridged_oracle(N, m):
    if (N, m) not in _ORACLE:
        out = dref.density_oracle(bridged(N)[3], THR, m)
        for a in out:
            a.setflags(write=False)
        _ORACLE[(N, m)] = out
    return _ORACLE[(N, m)]


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def synth_rows(state_dicts):
    """f_new of 128 synthetic images: embeddings of the real network, strongly correlated (the recipe of test_gpu_cluster.py)."""
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    f_new, _ = e.embed(ffrnet_amd.synth.synth_images(128, seed=77).cuda(), want_f=False)
    torch.cuda.synchronize()
    e.close()
    return f_new


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


def run(eng, emb, thr, m, **kw):
    rep, kind, degree = eng.cluster_density(emb, thr, m, return_degree=True, **kw)
    assert rep.dtype == torch.int64 and kind.dtype == torch.uint8 and degree.dtype == torch.int32
    assert rep.shape == kind.shape == degree.shape == (emb.size(0),)
    return rep.cpu().numpy(), kind.cpu().numpy(), degree.cpu().numpy()


def assert_equal(got, want, what=None):
    for name, g, w in zip(('rep', 'kind', 'degree'), got, want):
        assert np.array_equal(g, w), (name, what, np.nonzero(g != w)[0][:8].tolist())


# 4129 = 4096 + 33: up to 1000 rows a chunk is one 128-row step; at 4129 a chunk has several (test_gpu_cluster.py)
@pytest.mark.parametrize('N', [20, 31, 32, 33, 127, 128, 129, 257, 1000, 4129])
def test_with_margin_equals_float64_oracle(eng, N):
    emb, truth, info, S = bridged(N)
    assert cluster_ref.margin(S, THR) > MARGIN
    d = dev(emb)
    for m in (3, 4, 5):
        want = bridged_oracle(N, m)
        # no border row with two core neighbours within 1e-3 of each other: the float64 ranking is the fp32 ranking
        for x in np.nonzero(want[1] == 1)[0]:
            sc = np.sort(S[x][(S[x] > THR) & (want[1] == 2)])[::-1]
            assert sc.size >= 1 and (sc.size == 1 or sc[0] - sc[1] > MARGIN), (N, m, x)
        got = run(eng, d, THR, m)
        assert_equal(got, want, (N, m))
        assert np.array_equal(got[0][got[0]], got[0])
        assert set(got[1].tolist()) == {0, 1, 2}


def test_bridge_separates_what_single_link_merges(eng):
    emb, truth, info, S = bridged(168)
    assert cluster_ref.margin(S, THR) > MARGIN
    d = dev(emb)
    A, B = info['ident']
    single = eng.cluster(d, THR).cpu().numpy()
    assert len(set(single[A + B].tolist())) == 1
    rep, kind, degree = run(eng, d, THR, 4)
    assert_equal((rep, kind, degree), bridged_oracle(168, 4))
    assert len(set(rep[A].tolist())) == 1 and len(set(rep[B].tolist())) == 1 and rep[A[0]] != rep[B[0]]
    assert np.bincount(kind).tolist() == [46, 2, 120] and (kind[info['bridge']] == 1).all()
    # norms handed in or computed in the call: the same results
    again = run(eng, d, THR, 4, norms=eng.row_norms(d))
    assert_equal(again, (rep, kind, degree))
    r2, k2 = eng.cluster_density(d, THR, 4)                              # without the degrees
    assert np.array_equal(r2.cpu().numpy(), rep) and np.array_equal(k2.cpu().numpy(), kind)


def test_min_rows_1_and_2_equal_single_link(eng, synth_rows):
    sets = [(dev(cluster_ref.planted(168)[0]), [THR]), (dev(bridged(1000)[0]), [THR])]
    S = search_matrix(eng, synth_rows)
    off = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    sets.append((synth_rows, [off[int(q * (off.numel() - 1))].item() for q in (0.5, 0.97, 0.997)]))
    for emb, thrs in sets:
        sizes = set()
        for thr in thrs:
            want = eng.cluster(emb, thr)
            rep, kind, degree = eng.cluster_density(emb, thr, 1, return_degree=True)
            assert torch.equal(rep, want) and bool((kind == 2).all())
            rep2, kind2, degree2 = eng.cluster_density(emb, thr, 2, return_degree=True)
            assert torch.equal(rep2, want) and torch.equal(degree2, degree)
            assert torch.equal(kind2, torch.where(degree > 0, 2, 0).to(torch.uint8))
            sizes.add((len(torch.unique(want)), int((degree > 0).sum())))
        assert any(1 < c < emb.size(0) and 0 < d < emb.size(0) for c, d in sizes), sizes     # not one blob, not all alone


def test_no_margin_agrees_with_search_scores(eng, synth_rows):
    emb = synth_rows
    S = search_matrix(eng, emb)
    off = S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]
    Sn = S.cpu().numpy()
    # each threshold IS one of the scores, so the strict > is exercised on equal bits
    ranked = torch.sort(off).values
    picks = [ranked[(ranked.numel() - 1) // 2].item()] + [ranked[int(q * (ranked.numel() - 1))].item()
                                                         for q in (0.9, 0.97, 0.99, 0.997, 0.9995)]
    seen, kinds = set(), set()
    for thr in picks:
        for m in (3, 6, 12):
            want = dref.density_oracle(Sn, np.float32(thr), m)
            got = run(eng, emb, thr, m)
            assert_equal(got, want, (thr, m))
            seen.add(len(np.unique(want[0])))
            kinds |= set(want[1].tolist())
    assert len(seen) > 1 and kinds == {0, 1, 2}                          # the cases do not all give one blob


def unit(*pairs):
    """A row with small integer entries: unit(coordinate, value, ...).  Dots and squared norms of such rows are exact."""
    x = np.zeros(512, dtype=np.float32)
    for k, v in zip(pairs[::2], pairs[1::2]):
        x[k] = v
    return x


def border_case(which):
    """-> (rows [128,512], threshold, min_rows, named rows).  Cluster A: a_k = e0 + 2 e_k, k = 2..5, cluster B: b_k = e1 +
    2 e_k, k = 12..15: within a cluster every pair scores 1/5, across 0.  min_rows = 4: the 8 rows are core once they have
    their 3 fellows.  Fillers e_100+i score 0 with everything."""
    rows = [unit(100 + i, 1) for i in range(128)]
    A = [unit(0, 1, k, 2) for k in (2, 3, 4, 5)]
    B = [unit(1, 1, k, 2) for k in (12, 13, 14, 15)]
    named = {}
    if which == 'tie':            # x = e2 + e12: 2 / (sqrt 2 sqrt 5) with a_2 and with b_12, the same bits
        place = dict(A=[40, 41, 42, 43], B=[4, 5, 6, 7], x=127)          # B holds the smaller core row: x goes to B
        x = unit(2, 1, 12, 1)
    elif which == 'tie_mirrored':
        place = dict(A=[4, 5, 6, 7], B=[100, 101, 102, 103], x=64)
        x = unit(2, 1, 12, 1)
    elif which == 'gap':          # x = e2 + 2 e12: 2/5 with a_2, 4/5 with b_12 (the larger index)
        place = dict(A=[4, 5, 6, 7], B=[100, 101, 102, 103], x=50)
        x = unit(2, 1, 12, 2)
    elif which == 'row0':         # the border row is row 0, every core row of its cluster is larger
        place = dict(A=[33, 70, 71, 99], B=[10, 11, 12, 13], x=0)
        x = unit(2, 1)
    elif which == 'noise_pair':   # y1 = e20, y2 = e20 + e21: adjacent to each other and to nothing else
        place = dict(A=[4, 5, 6, 7], B=[100, 101, 102, 103], x=50)
        x = unit(20, 1)
        rows[90] = unit(20, 1, 21, 1)
        named['y2'] = 90
    for r, v in zip(place['A'] + place['B'], A + B):
        rows[r] = v
    rows[place['x']] = x
    named.update(place)
    return np.stack(rows), 0.1, 4, named


@pytest.mark.parametrize('which', ['tie', 'tie_mirrored', 'gap', 'row0', 'noise_pair'])
def test_border_rule_on_exact_arithmetic(eng, which):
    rows, thr, m, at = border_case(which)
    d = dev(rows)
    S = search_matrix(eng, d)
    Sn = S.cpu().numpy()
    want = dref.density_oracle(Sn, np.float32(thr), m)
    got = run(eng, d, thr, m)
    assert_equal(got, want, which)
    rep, kind, degree = got
    A, B, x = at['A'], at['B'], at['x']
    assert (kind[A + B] == 2).all() and len(set(rep[A].tolist())) == 1 and len(set(rep[B].tolist())) == 1 and rep[A[0]] != rep[B[0]]
    if which in ('tie', 'tie_mirrored'):
        sa, sb = Sn[min(x, A[0]), max(x, A[0])], Sn[min(x, B[0]), max(x, B[0])]
        assert sa == sb and sa > thr                                     # bitwise equal scores decide nothing
        winner = A if A[0] < B[0] else B
        assert kind[x] == 1 and degree[x] == 2 and rep[x] == rep[winner[0]]
    elif which == 'gap':
        assert Sn[x, B[0]] > Sn[A[0], x] > thr and B[0] > A[0]
        assert kind[x] == 1 and rep[x] == rep[B[0]]
    elif which == 'row0':
        assert kind[0] == 1 and (rep[A] == 0).all() and rep[0] == 0 and np.array_equal(rep[rep], rep)
    else:
        y2 = at['y2']
        assert Sn[x, y2] > thr and degree[x] == 1 and degree[y2] == 1
        assert kind[x] == 0 and kind[y2] == 0 and rep[x] == x and rep[y2] == y2
    # the same rows in other orders: whichever block meets an edge first, the oracle's answer
    rng = np.random.default_rng(3)
    for _ in range(3):
        p = rng.permutation(128)
        dp = dev(rows[p])
        assert_equal(run(eng, dp, thr, m), dref.density_oracle(search_matrix(eng, dp).cpu().numpy(), np.float32(thr), m), which)


def test_contention_and_determinism():
    e = ffrnet_amd.Engine(0)
    g = torch.Generator(device='cuda')
    g.manual_seed(5)
    same = torch.randn((1, 512), device='cuda', generator=g).expand(257, 512).contiguous()
    rep, kind, degree = e.cluster_density(same, THR, 200, return_degree=True)
    assert bool((rep == 0).all()) and bool((kind == 2).all()) and bool((degree == 256).all())
    basis = torch.zeros((257, 512), device='cuda')
    basis[torch.arange(257), torch.arange(257) % 3] = 1.0
    rep, kind, degree = e.cluster_density(basis, THR, 80, return_degree=True)
    assert torch.equal(rep, torch.arange(257, device='cuda') % 3) and bool((kind == 2).all())
    assert torch.equal(degree, torch.tensor([85, 85, 84], device='cuda', dtype=torch.int32)[torch.arange(257, device='cuda') % 3])
    rep, kind = e.cluster_density(basis, THR, 87)                        # 86 rows are one short: nobody is core
    assert torch.equal(rep, torch.arange(257, device='cuda')) and not bool(kind.any())
    # two calls are bitwise equal; a larger call in between grows the scratch and changes nothing
    emb = dev(bridged(168)[0])
    r1 = e.cluster_density(emb, THR, 4, return_degree=True)
    g1 = e.generation()
    r2 = e.cluster_density(emb, THR, 4, return_degree=True)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2)) and e.generation() == g1
    big = e.cluster_density(dev(bridged(1000)[0]), THR, 4, return_degree=True)
    assert e.generation() != g1
    assert_equal([t.cpu().numpy() for t in big], bridged_oracle(1000, 4))
    g2 = e.generation()
    r3 = e.cluster_density(emb, THR, 4, return_degree=True)
    assert all(torch.equal(a, b) for a, b in zip(r1, r3)) and e.generation() == g2
    assert torch.equal(e.cluster(emb, THR), torch.from_numpy(cluster_ref.cluster_oracle(bridged(168)[0], THR)[0]).cuda())
    e.close()


def test_arguments(eng):
    g = torch.Generator(device='cuda')
    g.manual_seed(51)
    emb = torch.randn((100, 512), device='cuda', generator=g)
    norms = eng.row_norms(emb)
    rep = torch.empty((100,), device='cuda', dtype=torch.int64)
    kind = torch.empty((100,), device='cuda', dtype=torch.uint8)
    degree = torch.empty((100,), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    names = ['emb', 'norms', 'N', 'dim', 'thr', 'min_rows', 'rep', 'kind', 'degree', 'st']
    ok = (P(emb), P(norms), 100, 512, 0.5, 3, P(rep), P(kind), P(degree), st)

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_cluster_density(eng._h, *a)

    def message():
        return (eng.lib.ffr_last_error(eng._h) or b'').decode()

    assert call() == 0
    assert call(norms=null) == 0
    assert call(degree=null) == 0                                         # the degrees are optional
    assert call(dim=256) == -6 and '512' in message()
    for bad in (dict(N=-1), dict(N=1 << 31), dict(thr=float('nan')), dict(min_rows=0), dict(min_rows=-3), dict(rep=null),
                dict(kind=null), dict(emb=null), dict(emb=C.c_void_p(emb.data_ptr() + 4)), dict(rep=C.c_void_p(rep.data_ptr() + 4)),
                dict(degree=C.c_void_p(degree.data_ptr() + 2))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_density' in message(), bad
    assert call(N=0) == 0 and call(N=0, emb=null, rep=null, kind=null, degree=null) == 0
    assert call(N=0, min_rows=0) == -1
    # the binding: wrong device, wrong shape, norms of another length, bad min_rows, an empty collection, one row
    with pytest.raises(RuntimeError):
        eng.cluster_density(emb.cpu(), 0.5, 3)
    with pytest.raises(RuntimeError):
        eng.cluster_density(emb[:, :256].contiguous(), 0.5, 3)
    with pytest.raises(RuntimeError):
        eng.cluster_density(emb, 0.5, 3, norms=norms[:50])
    with pytest.raises(RuntimeError):
        eng.cluster_density(emb, float('nan'), 3)
    with pytest.raises(RuntimeError):
        eng.cluster_density(emb, 0.5, 0)
    none = fc.density(eng, emb[:0], 0.5, 3)
    assert none.n_clusters == 0 and none.rep.numel() == 0 and none.has_core.numel() == 0
    assert fc.templates(eng, emb[:0], none).shape == (0, 512)
    one = eng.cluster_density(emb[:1], 0.5, 1, return_degree=True)
    assert [t.tolist() for t in one] == [[0], [2], [0]]
    assert [t.tolist() for t in eng.cluster_density(emb[:1], 0.5, 2)] == [[0], [0]]


def test_profile_counts_two_walks_under_score(eng):
    g = torch.Generator(device='cuda')
    g.manual_seed(61)
    emb = torch.randn((300, 512), device='cuda', generator=g)
    eng.cluster_density(emb, THR, 4)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    eng.cluster_density(emb, THR, 4)
    st = eng.profile_read()
    eng.profile_enable(False)
    assert st['score']['launches'] == 1 and st['score']['flops'] == 2 * 300.0 * 299 * 512 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0


def test_end_to_end_enrolment(eng):
    emb, truth, info, S = bridged(168)
    d = dev(emb)
    c = fc.density(eng, d, THR, 4)
    want = bridged_oracle(168, 4)
    assert np.array_equal(c.rep.cpu().numpy(), want[0]) and np.array_equal(c.kind.cpu().numpy(), want[1])
    n_core_clusters = len(np.unique(want[0][want[1] == 2]))
    assert int(c.has_core.sum()) == n_core_clusters and c.n_clusters == n_core_clusters + int((want[1] == 0).sum())
    t = fc.templates(eng, d, c)
    assert t.shape == (c.n_clusters, 512)
    gal = Gallery(eng)
    assert gal.add(t[c.has_core]) == 0 and len(gal) == n_core_clusters     # exactly the clusters with a core
    gallery_row = torch.cumsum(c.has_core.to(torch.int64), 0) - 1           # cluster id -> its row in the gallery
    core = torch.nonzero(c.kind == 2).reshape(-1)
    s, i = gal.search(d[core], 1)
    assert torch.equal(i[:, 0], gallery_row[c.cluster_id[core]])
    assert s.min().item() > 0.8
    # the two bridged identities are two gallery rows, and neither template is a mixture of the two
    A, B = info['ident']
    ga, gb = int(gallery_row[c.cluster_id[A[0]]]), int(gallery_row[c.cluster_id[B[0]]])
    assert ga != gb
    single = fc.cluster(eng, d, THR)
    assert int(single.cluster_id[A[0]]) == int(single.cluster_id[B[0]])
