"""CPU oracle of the removal from a single-link clustering (include/ffrnet.h: ffr_cluster_remove), from a float64 (or any)
score matrix of which only the upper triangle is read, built on the union-find of tests/cluster_ref.py.

remove_from_scores is the definition of the header, for any rep_in, prior and keep; survivors_only is the other side of
contract (a): the clustering of the surviving rows alone, mapped back to the old numbering."""
import numpy as np

import cluster_ref


def guard(rep_in):
    """g(x) = rep_in[x] where 0 <= rep_in[x] <= x, else x."""
    rep_in = np.asarray(rep_in, dtype=np.int64).reshape(-1)
    x = np.arange(rep_in.size, dtype=np.int64)
    return np.where((rep_in >= 0) & (rep_in <= x), rep_in, x)


def affected(rep_in, keep):
    """-> bool[N]: the surviving rows whose label g(x) is hit (some removed row d has g(d) equal to it)."""
    g = guard(rep_in)
    keep = np.asarray(keep).reshape(-1) != 0
    hit = np.zeros(g.size, dtype=bool)
    hit[g[~keep]] = True
    return keep & hit[g]


def remove_from_scores(S, threshold, rep_in, keep, prior=None):
    """rep[N] int64 of the definition: -1 for a removed row, g(x) for an unaffected survivor, and for the affected survivors
    the smallest row of their component under the edges a < b, S[a,b] > threshold, and the links x - prior[x] (0 <= prior[x]
    <= x), both between affected survivors only."""
    S = np.asarray(S)
    n = S.shape[0]
    g = guard(rep_in)
    keep = np.asarray(keep).reshape(-1) != 0
    aff = affected(rep_in, keep)
    edges = cluster_ref.upper_edges(S, threshold)
    edges = edges[aff[edges[:, 0]] & aff[edges[:, 1]]]
    if prior is not None:
        prior = np.asarray(prior, dtype=np.int64).reshape(-1)
        x = np.arange(n, dtype=np.int64)
        ok = (prior >= 0) & (prior <= x)
        ok[ok] &= aff[prior[ok]]
        ok &= aff
        edges = np.concatenate((edges.reshape(-1, 2), np.stack((prior[ok], x[ok]), 1)))
    joined = cluster_ref.union_find(n, edges)
    return np.where(~keep, -1, np.where(aff, joined, g)).astype(np.int64)


def survivors_only(S, threshold, keep):
    """The clustering of the surviving rows alone, union_find over S[keep][:, keep], in the OLD numbering: rep[N] int64 with
    -1 for a removed row."""
    S = np.asarray(S)
    keep = np.asarray(keep).reshape(-1) != 0
    kept = np.nonzero(keep)[0]
    sub = cluster_ref.union_find(kept.size, cluster_ref.upper_edges(S[np.ix_(kept, kept)], threshold))
    out = np.full(S.shape[0], -1, dtype=np.int64)
    out[kept] = kept[sub]
    return out


def compact(rep, keep):
    """Labels in the old numbering (-1 for removed rows) -> the survivors' labels in compact numbering."""
    keep = np.asarray(keep).reshape(-1) != 0
    old_to_new = np.full(keep.size, -1, dtype=np.int64)
    old_to_new[keep] = np.arange(int(keep.sum()), dtype=np.int64)
    return old_to_new[np.asarray(rep)[keep]]


def keep_without(n, rows):
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(rows, dtype=np.int64).reshape(-1)] = False
    return keep


def pick_clusters_for(rep, m):
    """Rows to remove -- one row (the representative) of each chosen multi-row cluster -- so that exactly m rows are affected:
    greedily by cluster size, largest first.  -> rows, or None when the sizes do not add up."""
    reps, sizes = np.unique(rep, return_counts=True)
    order = np.argsort(-sizes, kind='stable')
    rows, left = [], m
    for k in order.tolist():
        s = int(sizes[k]) - 1                       # survivors of the cluster once its representative is gone
        if 1 <= s <= left:
            rows.append(int(reps[k]))
            left -= s
        if left == 0:
            return np.array(rows, dtype=np.int64)
    return None
