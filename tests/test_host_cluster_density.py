"""CPU checks of the density-gated clustering's host side: the oracle of tests/cluster_density_ref.py against an
independently written brute force, its agreement with single link at min_rows 1 and 2, the planted data's margin and kind
counts, DensityClusters on CPU tensors, and the C symbol."""
import collections
import ctypes

import numpy as np
import torch

import cluster_density_ref as dref
import cluster_ref
from ffrnet_amd import cluster as fc
from ffrnet_amd import native

NS = [20, 31, 32, 33, 127, 128, 129, 168, 257, 1000, 4129]


def brute_force(S, threshold, min_rows):
    """Written without the oracle's helpers: adjacency matrix, BFS over core-core adjacency, border assignment."""
    n = S.shape[0]
    adj = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for j in range(i + 1, n):
            if S[i, j] > threshold:
                adj[i, j] = adj[j, i] = True
    degree = adj.sum(1)
    core = [bool(degree[i] + 1 >= min_rows) for i in range(n)]
    label = [-1] * n
    for s in range(n):
        if not core[s] or label[s] >= 0:
            continue
        label[s] = s
        queue = collections.deque([s])
        while queue:
            x = queue.popleft()
            for y in range(n):
                if adj[x, y] and core[y] and label[y] < 0:
                    label[y] = s
                    queue.append(y)
    kind = [2 if c else 0 for c in core]
    for x in range(n):
        if core[x]:
            continue
        best = None
        for c in range(n):                                     # ascending: a later equal score does not replace
            if adj[x, c] and core[c]:
                sc = S[min(x, c), max(x, c)]
                if best is None or sc > best[0]:
                    best = (sc, c)
        if best is None:
            label[x] = n + x                                   # noise: a label nobody else has
        else:
            label[x] = label[best[1]]
            kind[x] = 1
    rep = [min(y for y in range(n) if label[y] == label[x]) for x in range(n)]
    return np.array(rep, dtype=np.int64), np.array(kind, dtype=np.uint8), degree.astype(np.int32)


def test_oracle_matches_bruteforce_on_small_graphs():
    rng = np.random.default_rng(5)
    kinds = set()
    for case in range(60):
        n = int(rng.integers(1, 24))
        # few distinct values: ties between the candidates of a border row are common
        S = rng.integers(0, 6, size=(n, n)).astype(np.float32) / 5
        thr = np.float32(rng.choice([0.2, 0.4, 0.6]))
        for m in (1, 2, 3, 4, 6):
            got, want = dref.density_oracle(S, thr, m), brute_force(S, thr, m)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (case, m)
            rep, kind, _ = got
            assert np.array_equal(rep[rep], rep)
            kinds |= set(kind.tolist())
    assert kinds == {0, 1, 2}
    # by hand: cores 1..4 and 6..9 (two 4-cliques); row 0 ties between core 1 and core 6 -> the smaller; row 5 scores 0.6
    # with core 4 and 0.8 with core 9 -> the higher; row 10 is alone
    n = 11
    S = np.zeros((n, n), dtype=np.float32)
    for q in ((1, 2, 3, 4), (6, 7, 8, 9)):
        for a in q:
            for b in q:
                if a < b:
                    S[a, b] = 0.9
    S[0, 1] = S[0, 6] = 0.7
    S[4, 5] = 0.6
    S[5, 9] = 0.8
    rep, kind, degree = dref.density_oracle(S, 0.5, 4)
    assert rep.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 10]  # border rows 0 and 5 carry the smallest index of their clusters
    assert kind.tolist() == [1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 0] and degree.tolist() == [2, 4, 3, 3, 4, 2, 4, 3, 3, 4, 0]
    # two non-core rows adjacent only to each other are noise, each on its own
    S = np.zeros((4, 4), dtype=np.float32)
    S[0, 1] = 0.9
    rep, kind, _ = dref.density_oracle(S, 0.5, 3)
    assert rep.tolist() == [0, 1, 2, 3] and not kind.any()


def test_min_rows_1_and_2_are_single_link():
    rng = np.random.default_rng(6)
    for case in range(40):
        n = int(rng.integers(1, 40))
        S = rng.random((n, n))
        thr = rng.choice([0.5, 0.8, 0.95])
        want = cluster_ref.union_find(n, cluster_ref.upper_edges(S, thr))
        for m in (1, 2):
            rep, kind, degree = dref.density_oracle(S, thr, m)
            assert np.array_equal(rep, want)
            assert np.array_equal(kind, np.where((degree > 0) | (m == 1), 2, 0))


def _expected_cores(N, m):
    """Core rows of planted_bridged(N) at min_rows = m in 4, 5, from the recipe alone: a compact identity of s rows is a
    clique, core iff s >= m; the two bridged identities (4 members, degree 4; an outlier, degree 5) are core; chain,
    bridge and zero rows are not."""
    n_centre = N - 12 - 7
    sizes, c = [], 0
    while sum(sizes) < n_centre:
        sizes.append(min(1 + c % 7, n_centre - sum(sizes)))
        c += 1
    return sum(s for s in sizes if s >= m) + 10


def test_planted_bridged_margin_and_kinds():
    for N in NS:
        emb, truth, info = dref.planted_bridged(N)
        assert emb.shape == (N, 512) and emb.dtype == np.float32 and truth.shape == (N,)
        S = cluster_ref.cosine64(emb)
        assert cluster_ref.margin(S, 0.5) > 0.19, N            # the nearest score: cos(2 theta) = 0.28 and its noisy kin
        A, B = info['ident']
        single = cluster_ref.union_find(N, cluster_ref.upper_edges(S, 0.5))
        assert len(set(single[A + B + info['bridge']].tolist())) == 1       # single link merges the two identities
        for m in (4, 5):
            rep, kind, degree = dref.density_oracle(S, 0.5, m)
            assert len(set(rep[A].tolist())) == 1 and len(set(rep[B].tolist())) == 1 and rep[A[0]] != rep[B[0]]
            assert (kind[A + B] == 2).all()
            for b in info['bridge']:
                nb = np.nonzero((S[b] > 0.5) & (np.arange(N) != b))[0]
                assert kind[b] == 1 and degree[b] == 2 and (kind[nb] == 2).sum() == 1     # no near-tie decides anything
            assert rep[info['bridge'][0]] != rep[info['bridge'][1]]
            counts = np.bincount(kind, minlength=3)
            assert counts[2] == _expected_cores(N, m) and counts[1] == 2 and counts[0] == N - counts[2] - 2
            assert counts.min() > 0
        # min_rows = 3: the chain's interior turns core, its ends are border rows
        rep, kind, degree = dref.density_oracle(S, 0.5, 3)
        chain = info['chain']
        assert kind[chain].tolist() == [1, 2, 2, 2, 2, 1] and len(set(rep[chain].tolist())) == 1
        assert (kind[info['bridge']] == 2).all() and rep[A[0]] == rep[B[0]]                # at 3 the bridge rows link
    emb, truth, info = dref.planted_bridged(168)
    rep, kind, _ = dref.density_oracle(cluster_ref.cosine64(emb), 0.5, 4)
    assert np.bincount(kind).tolist() == [46, 2, 120]
    again = dref.planted_bridged(168)
    assert np.array_equal(again[0], emb) and np.array_equal(again[1], truth)


def test_density_clusters_on_cpu_tensors():
    # clusters {0 (border), 2, 5 (core)}, {1, 4 (core)}, noise 3 and 6
    rep = torch.tensor([0, 1, 0, 3, 1, 0, 6], dtype=torch.int64)
    kind = torch.tensor([1, 2, 2, 0, 2, 2, 0], dtype=torch.uint8)
    c = fc.density_ids(rep, kind)
    assert isinstance(c, fc.DensityClusters) and c._fields == ('rep', 'cluster_id', 'n_clusters', 'sizes', 'kind', 'has_core')
    assert c.n_clusters == 4 and c.cluster_id.tolist() == [0, 1, 0, 2, 1, 0, 3] and c.sizes.tolist() == [3, 2, 1, 1]
    assert c.has_core.dtype == torch.bool and c.has_core.tolist() == [True, True, False, False]
    assert torch.equal(c.rep, rep) and torch.equal(c.kind, kind)
    order, offsets = fc.member_order(c)                                     # accepted unchanged
    assert order.tolist() == [0, 2, 5, 1, 4, 3, 6] and offsets.tolist() == [0, 3, 5, 6, 7]
    empty = fc.density_ids(torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.uint8))
    assert empty.n_clusters == 0 and empty.has_core.numel() == 0
    import ffrnet_amd
    assert ffrnet_amd.DensityClusters is fc.DensityClusters and callable(fc.density)


def test_symbol_is_bound_and_exported():
    rows = {name: (res, args) for name, res, args in native.SYMBOLS}
    res, args = rows['ffr_cluster_density']
    assert res is ctypes.c_int and len(args) == 11
    assert args[3] is ctypes.c_longlong and args[4] is ctypes.c_int and args[5] is ctypes.c_float and args[6] is ctypes.c_int
    lib = ctypes.CDLL(native.lib_path())                                    # loads without a GPU
    assert lib.ffr_cluster_density is not None
    assert hasattr(native.Engine, 'cluster_density')
