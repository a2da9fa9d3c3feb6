"""CPU oracle of the density-gated clustering (include/ffrnet.h: ffr_cluster_density) and the planted data its tests share.

density_oracle works on a score matrix of which only the upper triangle is read, so it serves both the float64 cosine
(where the data keeps every score away from the threshold) and the fp32 scores of the search (where it does not)."""
import numpy as np

import cluster_ref

DIM = cluster_ref.DIM


def density_oracle(S, threshold, min_rows):
    """S[N,N] (upper triangle read), threshold, min_rows >= 1 -> (rep[N] int64, kind[N] uint8, degree[N] int32).
    Edges i < j iff S[i,j] > threshold; core iff degree + 1 >= min_rows; clusters = components of the core-core edges; a
    non-core row goes to the core neighbour with the highest score (as the dtype of S compares), then the smallest index;
    rep = the smallest member of the cluster, border rows included."""
    S = np.asarray(S)
    n = S.shape[0]
    edges = cluster_ref.upper_edges(S, threshold)
    degree = np.bincount(edges.reshape(-1), minlength=n).astype(np.int32)
    core = degree.astype(np.int64) + 1 >= min_rows
    root = cluster_ref.union_find(n, edges[core[edges[:, 0]] & core[edges[:, 1]]])
    kind = np.where(core, 2, 0).astype(np.uint8)
    cand = {}                                                  # non-core row -> [(-score, core row)]
    for i, j in edges.tolist():
        if core[i] != core[j]:
            c, x = (i, j) if core[i] else (j, i)
            cand.setdefault(x, []).append((-S[i, j], c))
    for x, lst in cand.items():
        root[x] = root[min(lst)[1]]
        kind[x] = 1
    rep = np.empty(n, dtype=np.int64)
    for r in np.unique(root):
        members = np.nonzero(root == r)[0]
        rep[members] = members[0]
    return rep, kind, degree


def planted_bridged(N, seed=20261020):
    """cluster_ref.planted(N - 12) plus 12 rows in a random plane (a, v), theta = arccos 0.8, then a permutation; N >= 20.
    Two identities of 4 members each, at plane angles 0 and 5 theta, a member being (centre + 0.02 randn) * uniform(0.5, 2);
    one outlier member of each at theta and at 4 theta; two bridge rows at 2 theta and 3 theta.  Consecutive angles score
    0.8, everything further apart in the plane at most 0.28: single link joins the two identities through outlier - bridge -
    bridge - outlier; at min_rows 4 and 5 the members and outliers are core, the bridge rows border rows with exactly one
    core neighbour each, and the identities stay apart.
    -> (emb[N,512] float32, truth[N] int64, info: ident = (rows of identity A, rows of B), members and outlier of each;
    bridge = the two bridge rows; chain, zero as cluster_ref.planted).  The bridge rows carry labels of their own."""
    assert N >= 20
    base, truth, binfo = cluster_ref.planted(N - 12, seed)
    rng = np.random.default_rng(seed + 1)
    a = rng.standard_normal(DIM)
    a /= np.linalg.norm(a)
    v = rng.standard_normal(DIM)
    v -= (v @ a) * a
    v /= np.linalg.norm(v)
    theta = np.arccos(0.8)

    def at(k):
        return np.cos(k * theta) * a + np.sin(k * theta) * v

    t0 = int(truth.max()) + 1
    rows, lab = [], []
    for k, t in ((0, t0), (5, t0 + 1)):
        for _ in range(4):
            rows.append((at(k) + 0.02 * rng.standard_normal(DIM)) * rng.uniform(0.5, 2.0))
            lab.append(t)
    for k, t in ((1, t0), (4, t0 + 1), (2, t0 + 2), (3, t0 + 3)):
        rows.append(at(k))
        lab.append(t)
    emb = np.concatenate((base.astype(np.float64), np.stack(rows)))
    truth = np.concatenate((truth, np.array(lab, dtype=np.int64)))
    perm = rng.permutation(N)
    inv = np.argsort(perm)                     # inv[position before the permutation] = row after it
    n0 = N - 12
    info = dict(ident=(sorted(inv[[n0, n0 + 1, n0 + 2, n0 + 3, n0 + 8]].tolist()),
                       sorted(inv[[n0 + 4, n0 + 5, n0 + 6, n0 + 7, n0 + 9]].tolist())),
                bridge=inv[[n0 + 10, n0 + 11]].tolist(),
                chain=[int(inv[r]) for r in binfo['chain']],
                zero=None if binfo['zero'] is None else int(inv[binfo['zero']]))
    return emb[perm].astype(np.float32), truth[perm], info
