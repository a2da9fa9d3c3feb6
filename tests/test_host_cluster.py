"""CPU checks of the clustering's host side: the oracle of tests/cluster_ref.py against brute-force transitive closure,
ffrnet_amd.cluster.pairwise_scores against hand-computed values, and the dense-id helper.  (The C symbols are held to the
header with every other row of native.SYMBOLS: test_host_logic.py.)"""
import numpy as np
import torch

import cluster_ref
from ffrnet_amd import cluster as fc


def test_oracle_union_find_matches_bruteforce_closure():
    graphs = [
        # a chain given back to front, a triangle, an isolated row
        (8, [(5, 6), (4, 5), (3, 4), (0, 2), (1, 2), (0, 1)], [0, 0, 0, 3, 3, 3, 3, 7]),
        # two stars that one late edge merges: the root of the merged component is its smallest row
        (7, [(3, 6), (3, 5), (1, 4), (1, 2), (2, 6)], [0, 1, 1, 1, 1, 1, 1]),
        # no edges; then everything through row 5
        (6, [], [0, 1, 2, 3, 4, 5]),
    ]
    for n, edges, want in graphs:
        got = cluster_ref.union_find(n, np.array(edges, dtype=np.int64).reshape(-1, 2))
        assert got.tolist() == want
        assert cluster_ref.closure_bruteforce(n, edges).tolist() == want
    n, edges = 6, [(i, 5) for i in range(5)]
    assert cluster_ref.union_find(n, edges).tolist() == [0] * 6 == cluster_ref.closure_bruteforce(n, edges).tolist()
    # from scores: the strict > and the upper triangle
    S = np.array([[1.0, 0.5, 0.1], [0.9, 1.0, 0.6], [0.9, 0.9, 1.0]])
    assert cluster_ref.upper_edges(S, 0.5).tolist() == [[1, 2]]           # 0.5 is not > 0.5; the lower triangle is ignored
    assert cluster_ref.union_find(3, cluster_ref.upper_edges(S, 0.5)).tolist() == [0, 1, 1]
    # the planted recipe: 168 rows, 41 centres + the chain + the zero row
    emb, truth, info = cluster_ref.planted(168)
    assert emb.shape == (168, 512) and emb.dtype == np.float32 and len(np.unique(truth)) == 43
    assert not emb[info['zero']].any() and len(info['chain']) == 6
    rep, S = cluster_ref.cluster_oracle(emb, 0.5)
    assert rep.tolist() == cluster_ref.closure_bruteforce(168, cluster_ref.upper_edges(S, 0.5)).tolist()
    assert cluster_ref.margin(S, 0.5) > 0.2
    assert fc.pairwise_scores(rep, truth) == (1.0, 1.0, 1.0)
    chain = info['chain']
    assert len(set(rep[chain].tolist())) == 1
    for a in range(6):
        for b in range(a + 2, 6):
            assert S[chain[a], chain[b]] < 0.3                             # only consecutive links are edges


def test_pairwise_scores_match_hand_counts():
    # truth {0,1,2} {3,4} {5}: 3 + 1 = 4 pairs; pred {0,1} {2,3,4} {5}: 1 + 3 = 4 pairs; together in both: (0,1), (3,4)
    p, r, f = fc.pairwise_scores([0, 0, 1, 1, 1, 2], [7, 7, 7, 9, 9, 4])
    assert (p, r, f) == (0.5, 0.5, 0.5)
    # everything in one predicted cluster: 15 pairs, 4 of them true
    p, r, f = fc.pairwise_scores(torch.zeros(6, dtype=torch.int64), torch.tensor([7, 7, 7, 9, 9, 4]))
    assert p == 4 / 15 and r == 1.0 and f == 2 * (4 / 15) / (4 / 15 + 1)
    # all singletons predicted: no predicted pair
    p, r, f = fc.pairwise_scores([0, 1, 2, 3], [0, 0, 1, 1])
    assert p == 1.0 and r == 0.0 and f == 0.0
    # label values do not matter, only the partition
    assert fc.pairwise_scores([5, 5, 9], [1, 1, 0]) == (1.0, 1.0, 1.0)
    assert fc.pairwise_scores([], []) == (1.0, 1.0, 1.0)


def test_dense_ids_on_cpu_tensors():
    rep = torch.tensor([0, 1, 0, 3, 1, 0, 6], dtype=torch.int64)
    c = fc.dense_ids(rep)
    assert isinstance(c, fc.Clusters) and c.n_clusters == 4
    assert c.cluster_id.tolist() == [0, 1, 0, 2, 1, 0, 3] and c.sizes.tolist() == [3, 2, 1, 1]
    assert torch.equal(c.rep, rep)
    order, offsets = fc.member_order(c)
    assert order.tolist() == [0, 2, 5, 1, 4, 3, 6] and offsets.tolist() == [0, 3, 5, 6, 7]
    empty = fc.dense_ids(torch.empty(0, dtype=torch.int64))
    assert empty.n_clusters == 0 and fc.member_order(empty)[1].tolist() == [0]
    import ffrnet_amd
    assert ffrnet_amd.cluster is fc and ffrnet_amd.Clusters is fc.Clusters
