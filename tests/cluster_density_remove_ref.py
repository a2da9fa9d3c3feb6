"""CPU oracle of the removal from a density-gated clustering (include/ffrnet.h: ffr_cluster_density_remove) and the
constructed cases its tests share.

remove_from_scores follows the six passes of the device code one after the other, sequentially, on a score matrix of which
only the upper triangle is read: degrees fall, status, seed, re-join, keys, finish.  It never clusters the survivors at
once: that it equals survivors_only (cluster_density_ref.density_oracle over the compacted rows, mapped back) is what
tests/test_host_cluster_density_remove.py checks.

The state is that of cluster_density_extend_ref: (rep[n] int64, degree[n] int32, (score[n], row[n])), row = -1 and score =
-inf where a row has no key.  Everything is in the numbering BEFORE the removal; a removed row carries rep -1, kind 0,
degree 0 and no key."""
import numpy as np

import cluster_density_extend_ref as xref
import cluster_density_ref
import cluster_ref
from cluster_remove_ref import guard, keep_without  # noqa: F401  (keep_without: for the tests)


def remove_from_scores(S, threshold, min_rows, state, keep):
    """-> (rep[N] int64, kind[N] uint8, degree[N] int32, (score[N], row[N]), (r, m, q)): the clustering and the state of
    the survivors, and the lengths of the three lists (removed rows, still-core rows of hit labels, rows that choose again)."""
    S = np.asarray(S)
    n, need = S.shape[0], min_rows - 1
    rep0, deg0, (bs0, br0) = state
    assert len(rep0) == len(deg0) == len(bs0) == len(br0) == n
    keep = np.asarray(keep).reshape(-1) != 0
    g = guard(rep0)
    deg0 = np.maximum(np.asarray(deg0, dtype=np.int64), 0)
    was_core = deg0 >= need
    edges = cluster_ref.upper_edges(S, threshold)
    ei, ej = edges[:, 0], edges[:, 1]

    # 1. degrees fall: every edge between a removed and a surviving row takes one from the survivor
    degree = np.where(keep, deg0, 0)
    for d, x in ((ei, ej), (ej, ei)):
        sel = ~keep[d] & keep[x]
        np.subtract.at(degree, x[sel], 1)
    degree = np.maximum(degree, 0)

    # 2. status
    core = keep & (degree >= need)
    lost = was_core & ~core
    hit = np.zeros(n, dtype=bool)
    hit[g[lost]] = True

    # 3. seed
    parent = list(range(n))
    rejoin = core & hit[g]
    coremin = {}
    for x in np.nonzero(core & ~hit[g])[0].tolist():
        coremin.setdefault(int(g[x]), x)                   # ascending x: the first is the smallest
    for x in np.nonzero(core & ~hit[g])[0].tolist():
        parent[x] = coremin[int(g[x])]

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    # 4. re-join: the pairs of L
    for i, j in edges[rejoin[ei] & rejoin[ej]].tolist():
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)

    # 5. keys
    bscore = np.full(n, -np.inf, dtype=S.dtype)
    brow = np.full(n, -1, dtype=np.int64)
    rekey = np.zeros(n, dtype=bool)
    for y in np.nonzero(keep & ~core)[0].tolist():
        c = int(br0[y])
        holds = 0 <= c < n and keep[c] and core[c]
        if was_core[y] or (c >= 0 and not holds):
            rekey[y] = True
        elif holds:
            bscore[y], brow[y] = bs0[y], c
    for c, y in ((ei, ej), (ej, ei)):
        sel = core[c] & rekey[y]
        for cc, yy, s in zip(c[sel].tolist(), y[sel].tolist(), S[ei[sel], ej[sel]].tolist()):
            if brow[yy] < 0 or s > bscore[yy] or (s == bscore[yy] and cc < brow[yy]):
                bscore[yy], brow[yy] = s, cc

    # 6. finish, over the survivors
    root = np.arange(n)
    kind = np.zeros(n, dtype=np.uint8)
    for x in np.nonzero(keep)[0].tolist():
        if core[x]:
            root[x], kind[x] = find(x), 2
        elif brow[x] >= 0:
            root[x], kind[x] = find(int(brow[x])), 1
    rep = np.full(n, -1, dtype=np.int64)
    kept = np.nonzero(keep)[0]
    for r in np.unique(root[kept]):
        members = kept[root[kept] == r]
        rep[members] = members[0]
    return rep, kind, degree.astype(np.int32), (bscore, brow), (int((~keep).sum()), int(rejoin.sum()), int(rekey.sum()))


def survivors_only(S, threshold, min_rows, keep):
    """The clustering of the surviving rows alone and the state a call from scratch leaves over them, in the OLD numbering
    -> (rep, kind, degree, (score, row)) as remove_from_scores returns them."""
    S = np.asarray(S)
    n = S.shape[0]
    keep = np.asarray(keep).reshape(-1) != 0
    kept = np.nonzero(keep)[0]
    sub = S[np.ix_(kept, kept)]
    rep_s, kind_s, deg_s = cluster_density_ref.density_oracle(sub, threshold, min_rows)
    scratch = xref.extend_from_scores(sub, threshold, min_rows, 0, xref.empty_state(S.dtype))
    assert (scratch[0] == rep_s).all() and (scratch[1] == kind_s).all() and (scratch[2] == deg_s).all()
    bs_s, br_s = scratch[3]
    rep = np.full(n, -1, dtype=np.int64)
    kind = np.zeros(n, dtype=np.uint8)
    degree = np.zeros(n, dtype=np.int32)
    bscore = np.full(n, -np.inf, dtype=S.dtype)
    brow = np.full(n, -1, dtype=np.int64)
    if kept.size:
        rep[kept], kind[kept], degree[kept], bscore[kept] = kept[rep_s], kind_s, deg_s, bs_s
        brow[kept] = np.where(br_s >= 0, kept[np.maximum(br_s, 0)], -1)
    return rep, kind, degree, (bscore, brow)


def full_state(S, threshold, min_rows):
    """The state a call from scratch leaves over all rows of S -> (rep, degree, (score, row))."""
    S = np.asarray(S)
    return xref.state_of(xref.extend_from_scores(S, threshold, min_rows, 0, xref.empty_state(S.dtype)))


def same(a, b):
    """Do two results (rep, kind, degree, (score, row), ...) agree in all four parts?"""
    return bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3][1] == b[3][1]).all()
                and (a[3][0] == b[3][0]).all())


def compact_state(result, keep):
    """A result in the old numbering -> (rep, kind, degree, (score, row)) of the survivors in compact numbering."""
    keep = np.asarray(keep).reshape(-1) != 0
    o2n = np.full(keep.size, -1, dtype=np.int64)
    o2n[keep] = np.arange(int(keep.sum()), dtype=np.int64)
    rep, kind, degree, (bs, br) = result[:4]
    br = br[keep]
    return o2n[rep[keep]], kind[keep], degree[keep], (bs[keep], np.where(br >= 0, o2n[np.maximum(br, 0)], -1))


def patterns(S, threshold, info, seed, n_random=3):
    """The named removal patterns of cluster_density_ref.planted_bridged (an identity member, its outlier: the row of the
    identity next to a bridge row, a bridge row, every second row, row 0, nothing, everything) and seeded random ones of up
    to N / 2 rows -> [(name, keep[N])]."""
    n = S.shape[0]
    rng = np.random.default_rng(seed)
    near = [x for x in info['ident'][0] if max(S[min(x, b), max(x, b)] for b in info['bridge']) > threshold]
    assert len(near) == 1
    member = [x for x in info['ident'][0] if x != near[0]][:1]
    out = [('member', keep_without(n, member)), ('outlier', keep_without(n, near)), ('bridge', keep_without(n, info['bridge'][:1])),
           ('every_second', np.arange(n) % 2 == 0), ('row0', keep_without(n, [0])), ('nothing', np.ones(n, dtype=bool)),
           ('everything', np.zeros(n, dtype=bool))]
    for k in range(n_random):
        out.append(('random%d' % k, keep_without(n, rng.choice(n, size=int(rng.integers(1, n // 2 + 1)), replace=False))))
    return out


# ---- constructed integer rows: every dot and squared norm is exact ----------------------------------------------------

unit = xref.unit


def group(base, ks):
    """Rows e_base + 2 e_k: any two of them score 1/5, and 0 with the rows of a group on other coordinates."""
    return [unit(base, 1, k, 2) for k in ks]


def constructed(which):
    """-> (rows [128,512], threshold, min_rows, the rows to remove, named rows).  min_rows = 5: a row is core with 4
    neighbours.  Fillers e_300+i score 0 with everything.  A group is group(base, ks) above.
      switch     A of 6 rows, B of 5.  x = 2 e_k(a0) + e_k(b0) at row 0 scores 4/5 with a0 and 2/5 with b0: a border row of
                 A, and A's rep is 0.  a0 is removed: A is hit but stays whole (5 rows), x moves to b0 in the unhit B, B's rep
                 becomes 0 and A's rises to its own smallest row.  r = 1, m = 5, q = 1.
      tie        the same with a third group C of 5 and x = 2 e_k(a0) + e_k(b0) + e_k(c0): b0 and c0 offer the same bits, and c0
                 sits at the smaller row: x goes to C.
      to_noise   D of exactly 5 rows, y a border row of d0 alone.  d1 and d2 are removed: every row of D is demoted, nothing
                 is core, y and the rest of D are noise.  r = 2, m = 0, q = 4: the three demoted rows and y.
      split      E and F of 5 rows each, z scores 2/sqrt(35) with e0 and e1, 4/sqrt(35) with f0 and 1/sqrt(7) with the pendant
                 row w: degree 4, core, and the one link between E and F.  w is removed: z is demoted, the cluster splits into
                 E and F, and z attaches to f0, the better side.  r = 1, m = 10, q = 1.
      no_cascade H of 4 rows; v scores with h0, h1, h2 and the pendant p: degree 4, core; h0, h1, h2 have 3 fellows and v:
                 degree 4, core through v alone; h3 is a border row.  p is removed: v is demoted, but it still counts in the
                 degrees of h0, h1, h2, which stay core; v becomes a border row of h0 (equal scores: the smallest row).
                 r = 1, m = 3, q = 1.
      rep_rises  I of 5 rows and u, a border row of i0 at row 0, the smallest member.  u is removed: it was not core, so no
                 label is hit, m = q = 0, and the rep of I rises to its own smallest row."""
    rows = [unit(300 + i, 1) for i in range(128)]
    named, remove = {}, []

    def put(name, at, vecs):
        for r, v in zip(at, vecs):
            rows[r] = v
        named[name] = list(at)

    if which in ('switch', 'tie'):
        put('A', [4, 5, 6, 7, 8, 9], group(0, (10, 11, 12, 13, 14, 15)))
        put('B', [40, 41, 42, 43, 44], group(1, (20, 21, 22, 23, 24)))
        x = unit(10, 2, 20, 1)
        if which == 'tie':
            put('C', [30, 31, 32, 33, 34], group(2, (50, 51, 52, 53, 54)))
            x = unit(10, 2, 20, 1, 50, 1)
        put('x', [0], [x])
        remove = [4]
    elif which == 'to_noise':
        put('D', [3, 4, 5, 6, 7], group(0, (10, 11, 12, 13, 14)))
        put('y', [20], [unit(10, 1, 60, 2)])
        remove = [4, 5]
    elif which == 'split':
        put('E', [3, 4, 5, 6, 7], group(0, (10, 11, 12, 13, 14)))
        put('F', [13, 14, 15, 16, 17], group(1, (20, 21, 22, 23, 24)))
        put('z', [50], [unit(10, 1, 11, 1, 20, 2, 70, 1)])
        put('w', [60], [unit(70, 1)])
        remove = [60]
    elif which == 'no_cascade':
        put('H', [3, 4, 5, 6], group(0, (10, 11, 12, 13)))
        put('v', [50], [unit(10, 1, 11, 1, 12, 1, 70, 1)])
        put('p', [60], [unit(70, 1)])
        remove = [60]
    elif which == 'rep_rises':
        put('I', [3, 4, 5, 6, 7], group(0, (10, 11, 12, 13, 14)))
        put('u', [0], [unit(10, 1, 60, 2)])
        remove = [0]
    else:
        raise KeyError(which)
    return np.stack(rows), 0.1, 5, remove, named


CONSTRUCTED = ('switch', 'tie', 'to_noise', 'split', 'no_cascade', 'rep_rises')
