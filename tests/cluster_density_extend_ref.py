"""CPU oracle of the extension of a density-gated clustering (include/ffrnet.h: ffr_cluster_density_extend) and the
constructed cases its tests share.

extend_from_scores follows the passes of the device code one after the other, sequentially, on a score matrix of which only
the upper triangle is read: seed from the state, degrees over the pairs with a new row, the promoted list, the gated join
over those pairs, the old-old edges at a promoted row, labels.  It never clusters all rows at once: that it equals
cluster_density_ref.density_oracle is what tests/test_host_cluster_density_extend.py checks.

The state is (rep[n] int64, degree[n] int32, (score[n], row[n])): the key of a border row as the score it chose by and the
core row it chose, row = -1 (and score = -inf) where there is none, i.e. for core and noise rows."""
import numpy as np

import cluster_ref


def empty_state(dtype=np.float64):
    return (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), (np.zeros(0, dtype=dtype), np.zeros(0, dtype=np.int64)))


def extend_from_scores(S, threshold, min_rows, n_old, state):
    """S[N,N] (upper triangle read), the state of the rows [0, n_old) -> (rep[N] int64, kind[N] uint8, degree[N] int32,
    (score[N], row[N]), m): the clustering and the state of all N rows, and the number of promoted rows."""
    S = np.asarray(S)
    n, need = S.shape[0], min_rows - 1
    rep0, deg0, (bs0, br0) = state
    assert len(rep0) == len(deg0) == len(bs0) == len(br0) == n_old <= n
    degree = np.zeros(n, dtype=np.int64)
    degree[:n_old] = deg0
    bscore = np.full(n, -np.inf, dtype=S.dtype)
    brow = np.full(n, -1, dtype=np.int64)
    was_core = np.zeros(n, dtype=bool)
    was_core[:n_old] = degree[:n_old] >= need

    # seed: an old core row under the smallest old core row of its rep; the keys of the old non-core rows
    parent = list(range(n))
    coremin = {}
    for x in range(n_old):
        if was_core[x]:
            coremin[int(rep0[x])] = min(coremin.get(int(rep0[x]), x), x)
        elif br0[x] >= 0:
            bscore[x], brow[x] = bs0[x], br0[x]
    for x in range(n_old):
        if was_core[x]:
            parent[x] = coremin[int(rep0[x])]

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def unite(a, b):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)

    def offer(x, c, s):
        """the highest score wins, then the smallest core row"""
        if brow[x] < 0 or s > bscore[x] or (s == bscore[x] and c < brow[x]):
            bscore[x], brow[x] = s, c

    # degrees over the pairs with a new row
    edges = cluster_ref.upper_edges(S, threshold)
    fresh, stale = edges[edges[:, 1] >= n_old], edges[edges[:, 1] < n_old]
    degree += np.bincount(fresh.reshape(-1), minlength=n)
    core = degree >= need

    # the promoted rows; their keys are void
    promoted = np.zeros(n, dtype=bool)
    promoted[:n_old] = ~was_core[:n_old] & core[:n_old]
    bscore[promoted], brow[promoted] = -np.inf, -1

    def treat(i, j):
        if core[i] and core[j]:
            unite(i, j)
        elif core[i] != core[j]:
            c, x = (i, j) if core[i] else (j, i)
            offer(x, c, S[i, j])

    # the gated join over the pairs with a new row, then the old-old edges with a promoted end
    for i, j in fresh.tolist():
        treat(i, j)
    for i, j in stale.tolist():
        if promoted[i] or promoted[j]:
            treat(i, j)

    # labels
    root = np.arange(n)
    kind = np.zeros(n, dtype=np.uint8)
    for x in range(n):
        if core[x]:
            root[x], kind[x] = find(x), 2
        elif brow[x] >= 0:
            root[x], kind[x] = find(int(brow[x])), 1
    rep = np.empty(n, dtype=np.int64)
    for r in np.unique(root):
        members = np.nonzero(root == r)[0]
        rep[members] = members[0]
    return rep, kind, degree.astype(np.int32), (bscore, brow), int(promoted.sum())


def state_of(result):
    """The state part (rep, degree, key) of what extend_from_scores returned."""
    return result[0], result[2], result[3]


def in_batches(S, threshold, min_rows, cuts):
    """extend_from_scores batch after batch: cuts = ascending row counts, the last one N -> the list of the results."""
    S = np.asarray(S)
    out, state, n_old = [], empty_state(S.dtype), 0
    for n in cuts:
        out.append(extend_from_scores(S[:n, :n], threshold, min_rows, n_old, state))
        state, n_old = state_of(out[-1]), n
    return out


def ordered_bits(score):
    """fp32 scores -> uint32 in the order of the values, as the device forms the high word of a key"""
    u = np.asarray(score, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u ^ np.uint64(0x80000000))


def keys(best):
    """(score, row) -> the int64 the binding holds: ordered score bits << 32 | 0xFFFFFFFF - row, 0 where row < 0."""
    score, row = best
    has = np.asarray(row) >= 0
    k = (ordered_bits(np.where(has, score, 0)) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.where(has, row, 0).astype(np.uint64))
    return np.where(has, k, np.uint64(0)).astype(np.uint64).view(np.int64)


def transitions(kind_before, kind_after):
    """{(kind before, kind after): count} over the rows both labelings hold, the changed ones only."""
    out = {}
    for a, b in zip(np.asarray(kind_before).tolist(), np.asarray(kind_after)[:len(kind_before)].tolist()):
        if a != b:
            out[(a, b)] = out.get((a, b), 0) + 1
    return out


# ---- constructed integer rows: every dot and squared norm is exact ----------------------------------------------------

def unit(*pairs):
    """A row with small integer entries: unit(coordinate, value, ...)."""
    x = np.zeros(512, dtype=np.float32)
    for k, v in zip(pairs[::2], pairs[1::2]):
        x[k] = v
    return x


def constructed(which):
    """-> (rows [128,512], threshold, min_rows, n_old or the list of them, named rows).  Cluster A: a_k = e0 + 2 e_k, k =
    2..5, cluster B: b_k = e1 + 2 e_k, k = 12..15 (named A and B in the order of k): within a cluster every pair scores 1/5,
    across 0; min_rows = 4: a row of A or B is core once it has its 3 fellows.  Fillers e_100+i score 0 with everything.
      switch        A old and complete; b_12, b_13 old, b_14, b_15 new.  x = e2 + 2 e12 at row 0: 2/5 with a_2, 4/5 with b_12.
                    Before, x is a border row of A and A's rep is 0.  The new rows promote b_12, which offers 4/5 through the
                    promoted pass: x goes to B, B's rep is 0, A's rep rises to its own smallest row.
      tie_promoted  x = e2 + e12 scores the same bits with a_2 and b_12.  a_2 is in the persisted key; b_12 is old, at a
                    SMALLER row than a_2, and promoted by the new b_14, b_15: its offer comes from the promoted pass and wins.
      tie_new       the same x; B is new altogether, so b_12 offers from the gated join at a LARGER row: the persisted key stays.
      noise_pair    y1 = e20 and y2 = e20 + e21 are adjacent to each other and to nothing else: noise at every split."""
    rows = [unit(100 + i, 1) for i in range(128)]
    A = [unit(0, 1, k, 2) for k in (2, 3, 4, 5)]
    B = [unit(1, 1, k, 2) for k in (12, 13, 14, 15)]
    named = {}
    if which == 'switch':
        place, x, n_old = dict(A=[4, 5, 6, 7], B=[10, 11, 100, 101], x=0), unit(2, 1, 12, 2), 64
    elif which == 'tie_promoted':
        place, x, n_old = dict(A=[4, 5, 6, 7], B=[3, 8, 100, 101], x=50), unit(2, 1, 12, 1), 64
    elif which == 'tie_new':
        place, x, n_old = dict(A=[4, 5, 6, 7], B=[100, 101, 102, 103], x=50), unit(2, 1, 12, 1), 64
    elif which == 'noise_pair':
        place, x, n_old = dict(A=[4, 5, 6, 7], B=[100, 101, 102, 103], x=50), unit(20, 1), [0, 6, 51, 64, 90, 91, 102, 127, 128]
        rows[90] = unit(20, 1, 21, 1)
        named['y2'] = 90
    for r, v in zip(place['A'] + place['B'], A + B):
        rows[r] = v
    rows[place['x']] = x
    named.update(place)
    return np.stack(rows), 0.1, 4, n_old, named
