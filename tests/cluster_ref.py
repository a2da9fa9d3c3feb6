"""CPU oracle of the clustering (include/ffrnet.h: ffr_cluster_threshold): float64 cosine with the +1e-8 of the library's
score, the edge set of the upper triangle, and a plain union-find that returns the smallest row index per component.
Also the planted data the tests share: well separated identities, a chain that only transitive closure connects, and a
zero row."""
import numpy as np

DIM = 512


def cosine64(emb):
    """emb[N,512] (any float dtype) -> S[N,N] float64, S[i,j] = x_i.x_j / (|x_i| |x_j| + 1e-8)."""
    x = np.asarray(emb, dtype=np.float64)
    n = np.sqrt((x * x).sum(1))
    return (x @ x.T) / (n[:, None] * n[None, :] + 1e-8)


def upper_edges(S, threshold):
    """The pairs i < j with S[i,j] > threshold (strict), as an [E,2] array."""
    i, j = np.nonzero(np.triu(np.asarray(S) > threshold, 1))
    return np.stack((i, j), 1)


def union_find(n, edges):
    """Plain sequential union-find -> rep[n] int64, rep[i] = the smallest index of i's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def closure_bruteforce(n, edges):
    """Transitive closure by Warshall on the boolean adjacency -> rep[i] = the smallest index reachable from i."""
    reach = np.eye(n, dtype=bool)
    for a, b in edges:
        reach[a, b] = reach[b, a] = True
    for k in range(n):
        reach |= reach[:, k:k + 1] & reach[k:k + 1, :]
    return np.array([int(np.nonzero(reach[i])[0][0]) for i in range(n)], dtype=np.int64)


def cluster_oracle(emb, threshold):
    """-> (rep[N], S[N,N]): the components of the float64 scores' upper-triangle edges."""
    S = cosine64(emb)
    return union_find(S.shape[0], upper_edges(S, threshold)), S


def margin(S, threshold):
    """The distance of the nearest off-diagonal score to the threshold (inf for N < 2)."""
    iu = np.triu_indices(S.shape[0], 1)
    return float(np.abs(S[iu] - threshold).min()) if iu[0].size else float('inf')


def planted(N, seed=20261018):
    """N rows (float32) and their true labels: unit centres c = 0, 1, ... with 1 + c % 7 members each, a member being
    (centre + 0.02 randn) * uniform(0.5, 2); for N >= 8 also a 6-point chain in a random plane with consecutive cosine
    0.8 (one identity, connected only through its 5 consecutive links) and one all-zero row; then a random permutation.
    N = 168 gives 41 centres.  -> (emb[N,512] float32, truth[N] int64, info: rows of the chain and of the zero row)."""
    rng = np.random.default_rng(seed)
    special = 7 if N >= 8 else 0
    rows, truth = [], []
    c = 0
    while len(rows) < N - special:
        centre = rng.standard_normal(DIM)
        centre /= np.linalg.norm(centre)
        for _ in range(min(1 + c % 7, N - special - len(rows))):
            rows.append((centre + 0.02 * rng.standard_normal(DIM)) * rng.uniform(0.5, 2.0))
            truth.append(c)
        c += 1
    if special:
        u = rng.standard_normal(DIM)
        u /= np.linalg.norm(u)
        v = rng.standard_normal(DIM)
        v -= (v @ u) * u
        v /= np.linalg.norm(v)
        theta = np.arccos(0.8)
        for k in range(6):
            rows.append(np.cos(k * theta) * u + np.sin(k * theta) * v)
            truth.append(c)
        rows.append(np.zeros(DIM))
        truth.append(c + 1)
    perm = rng.permutation(N)
    emb = np.stack(rows)[perm].astype(np.float32)
    truth = np.array(truth, dtype=np.int64)[perm]
    inv = np.argsort(perm)                     # inv[original position] = row after the permutation
    info = dict(chain=inv[N - 7:N - 1].tolist(), zero=int(inv[N - 1])) if special else dict(chain=[], zero=None)
    return emb, truth, info


def templates64(emb, rep):
    """float64 templates of the clusters of rep, in order of representative: normalised sum of the normalised rows."""
    x = np.asarray(emb, dtype=np.float64)
    n = np.sqrt((x * x).sum(1))
    unit = np.divide(x, n[:, None], out=np.zeros_like(x), where=n[:, None] > 0)
    out = []
    for r in np.unique(rep):
        t = unit[rep == r].sum(0)
        tn = np.sqrt((t * t).sum())
        out.append(t / tn if tn > 0 else t)
    return np.stack(out)
