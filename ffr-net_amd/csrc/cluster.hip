// cluster.hip -- group N unlabelled 512-d embeddings into identities on the device (include/ffrnet.h:
// ffr_cluster_threshold / ffr_cluster_extend / ffr_cluster_remove / ffr_cluster_density / ffr_cluster_density_extend /
// ffr_cluster_density_remove / ffr_cluster_templates): single-link clustering at one cosine threshold, or gated by density
// over the same edges (core rows link, border rows attach, noise stays alone), either of them extended batch by batch where
// the collection grows and with rows taken out again, then one template row per cluster.  The N x N score matrix never leaves the
// chip; the output is one label per row.
//
// Edge rule: rows i < j are joined iff s(probe = i, gallery row = j) > threshold (strict, as eval_acc compares), with
// s = dot / (|i| |j| + 1e-8) in exactly the fp32 arithmetic of k_search_topk (search.hip): the score of (i, j) is
// bit-for-bit the score ffr_search_topk returns for probe i and gallery row j.  The diagonal and i > j are never evaluated.
//
// k_cluster_init     parent[x] = x.
// k_cluster_seed     ffr_cluster_extend's start: parent[x] = prior[x] where 0 <= prior[x] <= x, else x.  The only place
//                    where caller data reaches parent[]; see "Seeded start" below.
// k_cluster_walk     the hot path: the self-join of the [N][512] array with itself, one body (block map, early return,
//                    step0, probe fill, norm prefetch, K loop, scores, edge mask) with the epilogue as a parameter.
//                    <RANGE, EdgesUnite> is the join of single link, described first; EdgesDegree and EdgesGated are the
//                    two passes of ffr_cluster_density, see "Density" below.
//  - K loop: the 32 x 128 cosine tile of cosine_tile.h, the one k_search_topk instantiates: the bitwise identity of the edge
//    scores with the scores of ffr_search_topk is structural.
//  - Triangle: a block is (chunk of rows, tile of 32 probes), logical id as in the search.  A block whose chunk ends at
//    or before its tile's first probe has no pair i < j and exits at once; the others start at the first 128-row step
//    that can hold a row greater than the tile's smallest probe.  The grid is the chunks x tiles rectangle (cluster_plan
//    sizes the chunks so that the blocks with work, about half of it, fill the CUs several times over: their work is uneven
//    along the diagonal); the idle half costs one early return each.  Known cost (EXPERIMENTS.md): an XCD takes a
//    contiguous run of tiles, so the XCD with the long rows of the triangle finishes last.
//  - Row range: k_cluster_walk<true, .> (ffr_cluster_extend) lays the chunks over the rows [first, N) only and the tiles over
//    all probes [0, N): the pairs i < j with j >= first, i.e. the first x (N - first) rectangle plus the triangle among
//    the new rows.  Chunk bases, the early return, step0 and the edge test work on absolute row numbers; with first = 0
//    they are those of k_cluster_walk<false, .>, the instantiation ffr_cluster_threshold launches, which is compiled with the
//    constant 0.  All tiles of one chunk of new rows are neighbours in the XCD-contiguous block map, and the old rows are
//    read once per chunk into LDS as probes.  Over the old rows no block is idle and none sits on the diagonal.
//  - Epilogue (EdgesUnite): no list, no LDS merge.  Lane (n, h) holds the 16 scores of probe q0 + n; every (i, j) with
//    i < j, j inside the chunk and score > threshold is united in a lock-free union-find over parent[N] (int32, the
//    handle's scratch):
//      find   walk parent[] to a root r (parent[r] == r);
//      unite  roots equal -> done (tested with loads only: inside a formed cluster almost every edge is redundant, and
//             loads are cheap where atomics are not); else atomicCAS(&parent[big], big, small), agent scope, which hooks
//             the LARGER root under the SMALLER; on failure continue from the value the CAS returned.
//    Two properties make this safe on a shared machine:
//      (1) parent[x] <= x at every instant: parent[x] starts at x and is only ever replaced, by a successful CAS from x,
//          with a smaller index.  So every walk strictly descends and ends within N hops whatever the other waves do, and
//          every failed CAS hands back a value below `big`, so the larger of the two roots of a unite strictly decreases
//          from one attempt to the next: no loop can spin, there is no lock and no wait on another wave.
//      (2) only a root is ever hooked, under a smaller member of the other tree, so a component keeps exactly one root, and
//          that root is its smallest row index (a row can only point to smaller rows; the smallest points to itself).
//          The flattened result is therefore independent of the order in which the edges arrive.
//    parent[] is read with relaxed agent-scope atomic loads: a plain load may be served from a stale line of another XCD's
//    L2 or this CU's L1; a stale value is still a valid (older) ancestor, but the loads that decide "already one root" and
//    the CAS must see the memory the atomics of the other XCDs work on.  Vector atomics only.
//    No path compression: a walk is bounded by the component's size, and the clusters of a face collection are small.
//    Seeded start: properties (1) and (2) ask of the START only that parent[] is a forest with parent[x] <= x.  The seed
//    writes prior[x] only where 0 <= prior[x] <= x and x otherwise, so (1) holds at the first instant whatever the caller
//    passed (a cycle in parent[] would be a hang, an index outside [0, N) a fault), and afterwards by the same argument: a
//    CAS replaces parent[x] only from x, by something smaller.  In such a forest every walk descends to a row that points
//    to itself, so the root of a tree is its smallest member, as (2) needs; from there on only roots are hooked, under
//    smaller members of other trees, and every tree keeps one root, its smallest row.  The components at the end are those
//    of (links x - prior[x]) + (scored edges), and the flattened result is their smallest row whatever the order.  A deep
//    prior (prior[x] = x - 1) is legal and walked hop by hop: callers pass flattened labels.
//  - Density (ffr_cluster_density): k_density_init (parent[x] = x, degree[x] = 0, best[x] = 0), then two walks of the
//    triangle with the same body, so both see the edge mask single link sees, then three N-sized kernels.
//      EdgesDegree  degree[x] += edges at x.  The probe side is summed in a register and added once per block; the row side
//                   per step: a wave ballot of bit r of the mask, the popcount of each 32-lane half (the 32 probes against
//                   one row), one vector atomic of up to 32 counts per wave.  Integer adds commute.
//      EdgesGated   core(x) = degree[x] + 1 >= min_rows, read once per block for the probe and ahead of the K loop for the
//                   lane's 16 rows.  Both ends core: uf_unite, as above.  One end core: a 64-bit atomic max of
//                   (ordered score bits << 32 | 0xFFFFFFFF - core row) into best[non-core row]: the highest score wins,
//                   then the smallest core row, whatever the order.  Neither: nothing.
//      k_density_root / k_density_min / k_density_label: root[i] = find(i) for a core row, find(the core row of best[i]) for
//                   a border row, i for noise; minrow[root[i]] = min over the members (atomicMin; only a border row can be
//                   smaller than the root, the smallest core row); rep[i] = minrow[root[i]], kind[i], degree[i].
//    The safety argument carries over unchanged: nothing here waits on another wave.  Only core rows enter the
//    union-find, through the same uf_unite, so every parent[] walk (also the finds of k_density_root, which run after the
//    join in stream order) keeps parent[x] <= x and descends.  The degree adds, the 64-bit max and the min are single
//    no-return vector atomics at agent scope without a retry loop; there is no scalar memory write anywhere.  Every index
//    is a row the edge mask admitted (< N) or a prefetch clamped to the chunk's last row; the core row read back from
//    best[] was written as a row < N, and best[] is zeroed first (a real key is never 0: its low word is >= 2^31).
//  - Density, extended (ffr_cluster_density_extend): the rows [0, n_old) carry the state (rep, degree, best) of an earlier
//    call at the same threshold and min_rows; the result and the state left behind are those of ffr_cluster_density over
//    all N rows.  need = min_rows - 1.  Degrees only grow, so a core row stays core and the old core components persist;
//    among the old rows only the PROMOTED ones (degree_old < need <= degree) change status; and an old non-core row's key is
//    a maximum over its core neighbours, a set that only grows: new key = max(old key, offers of the newly core neighbours).
//      k_dext_init / k_dext_coremin / k_dext_parent   the seed: parent[x] = the smallest old core row with x's rep for an
//                   old core row, x for every other row; degree and best of the new rows 0; deg0[] = the old degrees.
//      k_cluster_walk<true, EdgesDegree>   adds the edges with a new end into degree[]: the instantiation is new, the body not.
//      k_dext_promoted_list   P[0 .. m) = the promoted rows, m in device memory; any order: what follows is unions and maxima.
//      k_cluster_walk<true, EdgesGated>    the gated join over the pairs with a new end, on the final core flags.
//      k_list_walk<WalkPromoted>   the old-old edges with an end in P: both ends are now core -> uf_unite; the other end y is not ->
//                   p is offered to best[y].  Old-old edges with no end in P need nothing: core-core ones are in the seed,
//                   core - non-core ones in the persisted key.  An edge between two promoted rows is met twice; a union and
//                   a maximum are idempotent.
//      k_density_root / k_density_min / k_density_label   as above.  best[] of core rows was zeroed on the way (old core
//                   rows in the seed, promoted rows where they are listed, new rows start at 0 and a core row gets no
//                   offer), so the state after an extension is bit for bit the state a call from scratch leaves.
//    Transposed pairs: k_list_walk<WalkPromoted> scores (y, p), y > p, as probe y against row p, where ffr_cluster_density scores
//    probe p against row y.  The bits are the same: a dot is the same 8 chains over the same k in the same order, each term
//    the product of the two rows' k-th components (an fp32 product commutes, and the MFMA adds its two products of a step in
//    k order whichever operand they came in); the chain sum is a fixed tree; the denominator fmaf(qn, gn, 1e-8) commutes in
//    qn, gn.  tests/test_gpu_cluster_density_extend.py holds this on the device (the score matrix equals its transpose).
//    Seeded start (extends the paragraph above): caller data reaches parent[] only in the seed.  rep[x] is used only where
//    0 <= rep[x] <= x, as an index into coremin[N]; coremin[r] is DX_NONE or the minimum of rows x < n_old that took part
//    with rep[x] = r, and an old core row reads the cell it took part in itself: 0 <= parent[x] <= x, and parent[parent[x]]
//    = parent[x] (the minimum is a core row of the same rep): a forest of depth 1 whatever was passed.  A rep outside [0, x]
//    leaves x alone; a negative degree is read as 0; a key whose decoded row is >= n_old, or is no old core row, is read as 0,
//    so k_density_root only ever follows a key to a core row of [0, N), a row of the union-find.  The walk over P is
//    "List walk" below; its own part: an edge is a uf_unite between two core rows, or the same single 64-bit max into
//    best[y] of an old non-core row y < n_old, with a promoted row p < n_old in the key: a core row of [0, N), as
//    k_density_root needs.
//  - Density, removal (ffr_cluster_density_remove): keep[x] = 0 takes row x out of a density-gated clustering whose state (rep,
//    degree, best) the caller holds for all N rows; nothing moves.  need = min_rows - 1, g(x) as in "Removal" below, was_core(x)
//    = degree_in[x] >= need.  The result and the state left behind are those of ffr_cluster_density over the survivors.
//      k_drem_init / k_drem_removed_list   counts, hit[] and coremin[] cleared, deg0[] = the old degrees, a removed row's degree
//                   0; R[0 .. r) = the removed rows.
//      k_list_walk<WalkFall>   all rows as probes against R: degree[x] -= 1 for a surviving x per removed neighbour.  Integer
//                   adds commute.  Degrees count all neighbours, core or not, so a demotion takes nothing from anyone: no cascade.
//      k_drem_status   core(x) = survivor with degree[x] >= need, a subset of the old core rows (degrees only fell).  LOST =
//                   was core, now removed or demoted; hit[g(x)] = 1 for a lost x.  Removing a border or a noise row hits nothing.
//      k_drem_seed_lists / k_dext_parent   a core row of a hit label goes into L[0 .. m) with parent[x] = x; a core row of an
//                   unhit label hangs under the smallest core row with its rep (the coremin seed of the extension; in an unhit
//                   cluster every core row survived and stayed core, so its core component is the old one); every other row
//                   starts alone.  best[] of core and removed rows is zeroed.  A non-core survivor keeps its key iff the key's
//                   core row survives and is still core; else -- every demoted row, every border row whose chosen core row was
//                   lost -- it goes into Q[0 .. q) with key 0.  A noise row that was not core stays noise and is not listed.
//      k_list_walk<WalkRemove>   the pairs of L by list position, every edge a uf_unite: all listed rows are core.
//      k_list_walk<WalkRekey>    all rows as probes against Q: a surviving core probe c adjacent to a listed y offers
//                   best_key(score, c) to best[y], the 64-bit max of the gated join.
//      k_density_root / k_density_min / k_density_label   as above; a removed row is alone in root[] (nothing points at it, it is
//                   smaller than no root) and is labelled rep -1, kind 0; its degree and key are 0 already.
//    Equality: compacting the survivors is a monotone renumbering, so "the smallest row" (roots, rep, the tie-break of a key)
//    and "the smaller index is the probe" carry over.  Degrees: the old degree minus the edges to removed rows is the degree
//    among the survivors.  Core components: the edges among still-core rows of unhit labels are exactly the old ones, kept by
//    the seed; a hit label's still-core rows are joined again over all their pairs, and no edge runs between core rows of two
//    old clusters.  Keys: a kept key is the maximum over a set of offers that shrank but still holds its maximum; a key looked
//    for again is the maximum over all surviving core neighbours, as from scratch; a demoted row had key 0 and is in Q.  The
//    walks score (probe, listed row) in either role; the bits are those of the triangle by "Transposed pairs" above.
//    Safety: caller data reaches an index only through g(x) in [0, x] (hit[], coremin[]) and through best_core(key), which is
//    used only after c < N is tested; a key is kept only if it names a surviving core row of [0, N), so k_density_root follows
//    a key only to a row of the union-find.  A negative degree reads as 0, on entry and after the fall.  parent[x] is x, or
//    coremin[rep[x]] <= x, the minimum x took part in itself (depth 1), so every walk descends.  The three lists are filled by
//    one fetch-add per wave without a retry loop (wave_list_push), each row at most once per list, so their counts are <= N;
//    the walks read them as min(*count, N), fixed at entry ("List walk" below).  The fall and the offers are single no-return
//    vector atomics; nothing waits on another wave.  An empty R (nothing removed) or Q is one early return per block.
//  - Removal (ffr_cluster_remove; single link only): keep[x] = 0 takes row x out; nothing moves, labels stay in the caller's
//    numbering.  g(x) = rep_in[x] where 0 <= rep_in[x] <= x, else x.  A cluster that loses no row had no edge to any other
//    cluster and removing rows adds none: it keeps its label.  A cluster that loses a row (its label is HIT) may fall apart:
//    its survivors, the AFFECTED rows, are joined again among themselves, and only their pairs are scored.
//      k_remove_init / k_remove_mark   hit[] = 0, m = 0; glabel[x] = g(x), hit[g(d)] = 1 for every removed d.
//      k_remove_list   rep[x] = -1 for a removed row, g(x) for an unaffected survivor; the affected survivors go into
//                   list[0 .. m), m in device memory, in any order, with parent[x] = prior[x] where prior is given,
//                   0 <= prior[x] <= x and prior[x] is an affected survivor too (a must-link that outlives the removal), else x.
//      k_list_walk<WalkRemove>   the self-join of the listed rows, pairs taken by list position a < b; probes and rows are
//                   both gathered through the list; uf_unite on row numbers.
//      k_remove_flatten   rep[x] = find(x) for the listed rows.
//    Equality with ffr_cluster_threshold over the survivors: compacting the survivors is a monotone renumbering, so "the
//    smallest row" and "the smaller index is the probe" carry over.  The union-find works on row numbers, so its root is the
//    component's smallest row whatever the list's order.  The list is NOT ascending, so a pair (x, y), x < y, may be scored
//    as probe y against row x: the transposed score has the same bits, by the argument of "Transposed pairs" above, which
//    tests/test_gpu_cluster_density_extend.py holds on the device; the edge set is therefore that of the ascending order, and
//    the components of an edge set do not depend on the order the edges are met in.
//    Safety: caller data (rep_in, prior, keep) reaches an index only through g(x) and the prior guard, both in [0, x], so
//    hit[], glabel[] and keep[] are read inside [0, N).  parent[x] <= x after the seed whatever was passed: it is x, or a
//    prior[x] in [0, x] that is itself listed, and so has its own parent set in the same launch; rows off the list never
//    enter the union-find.  From there (1) and (2) hold as before: a CAS replaces parent[x] only from x by something smaller.
//    The slot reservation of k_remove_list is one fetch-add per wave without a retry loop; the flatten reads m once and
//    clamps it to N as the walk does ("List walk" below).  m = 0 (nothing removed, or only whole clusters) scores nothing.
//  - List walk (k_list_walk<P>; P = WalkPromoted: the old rows [0, n_old) as probes against the promoted rows P, every pair
//    but (p, p); P = WalkFall, WalkRekey: the same orientation, all N rows against the lists of the density removal;
//    P = WalkRemove: the listed rows against themselves, the pairs of list positions a < b).  One body: work
//    items of (tile of 32 probes, span of 128-row steps of the list) under a fixed grid, the listed rows gathered through
//    CosineStreamT<GatherRows> (and, as probes, cosine_fill_probes_gather), the tile, chain sum and score of k_cluster_walk.
//    m: the list's length lives in device memory (the host never learns it); every block reads it once and reads it as at
//    most `bound`, the number of rows that can be listed (n_old, N), so every loop is bounded by a value fixed at entry,
//    whatever the cell holds.  Slots: list[] is written only by the kernel that builds it (k_dext_promoted_list,
//    k_remove_list, k_drem_removed_list, k_drem_seed_lists), earlier in stream order; a row is listed once, by its own thread, so m <= bound, the slots [0, m) are
//    all written and none past them is.  Rows: every slot holds the listing thread's own row, < bound <= N, and a probe is
//    either such a row or a position below n_old <= N: every index into emb, norm, degree, best and parent is < N.  Pads:
//    the walk reads list[] only at positions below m; the probes of a tile past its end are zeros, the slots of a span
//    past its end repeat its last listed row, in bounds, and the edge test masks both (n < nq, slot < ns): never an edge.
//    No wave waits on another: the barriers sit in the item loop, whose trip count and first `continue` depend on m, the
//    grid and the block index alone (uniform in a block); a wave with no live slot in a span skips the K loop after the
//    barriers; the edges are uf_unite, one no-return 64-bit max or one no-return integer add; vector atomics only.
// k_cluster_flatten  rep[i] = find(i) as int64, after the join in stream order.
// k_cluster_templates  one template per cluster: t = sum_r x_r / |x_r| over the cluster's rows in ascending row index
//                (order[] = rows sorted by cluster then index, offsets[C + 1]), then t / |t|.  One wave per cluster, lane
//                l owns components 8l .. 8l + 7; the sum over the rows is sequential fp32 per component: deterministic,
//                no atomics.  A zero row contributes zero, an all-zero sum stays zero.  Without norms[] the wave computes
//                |x_r| with the summation order of k_row_norms (bitwise the same value).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cosine_tile.h"
#include "device_util.h"
#include "ffr_kernels.h"

namespace ffr {

namespace {

__device__ __forceinline__ int uf_load(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x: the walk strictly descends
__device__ __forceinline__ int uf_find(const int* parent, int x) {
    for (;;) {
        const int p = uf_load(parent, x);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const int big = max(ra, rb), small = min(ra, rb);
        int expected = big;
        if (__hip_atomic_compare_exchange_strong(parent + big, &expected, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // big was hooked by another wave meanwhile: expected = parent[big] < big
        ra = uf_find(parent, expected);
        rb = uf_find(parent, small);
    }
}

__global__ __launch_bounds__(256) void k_cluster_init(int* __restrict__ parent, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n) parent[x] = x;
}

// whatever prior[] holds, parent[x] <= x afterwards (the invariant every walk relies on) and no index leaves [0, n)
__global__ __launch_bounds__(256) void k_cluster_seed(int* __restrict__ parent, const int64_t* __restrict__ prior, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int64_t p = prior[x];
    parent[x] = (0 <= p && p <= (int64_t)x) ? (int)p : x;
}

__global__ __launch_bounds__(256) void k_cluster_flatten(const int* __restrict__ parent, int n, int64_t* __restrict__ rep) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n) rep[x] = uf_find(parent, x);
}

struct JoinArgs {
    const float* emb;         // [N][512]
    const float* norm;        // [N]
    int* parent;              // [N]
    long long N;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), a multiple of CT_STEP, <= CT_MAX_CHUNK
    float threshold;
    int nchunks, ntiles;
    long long first;          // RANGE: the chunks cover the rows [first, N)
    // ffr_cluster_density and ffr_cluster_density_extend only
    int* degree;              // [N]
    unsigned long long* best; // [N]
    int min_rows;
};

// What a lane does with the edges of one step (EdgesUnite, EdgesDegree, EdgesGated below):
//   E(a, irow, live)   once per block; irow = the lane's probe row, live = it exists
//   rows_ahead(...)    ahead of the K loop, where gn[] is fetched: per-row data of the 16 rows the lane scores
//   step(...)          after the scores: mask has bit r set iff (irow, row of accumulator element r) is an edge.  Called by
//                      all 64 lanes of every wave in every step (the step loop is uniform in a block): wave ballots are legal
//   done(irow)         after the last step
// Single link: every edge is united.
struct EdgesUnite {
    int* parent;
    __device__ __forceinline__ EdgesUnite(const JoinArgs& a, int, bool) : parent(a.parent) {}
    __device__ __forceinline__ void rows_ahead(long long, int, int, int, int) {}
    __device__ __forceinline__ void step(unsigned mask, const f32x16&, float, const float (&)[16], int irow, long long j0, int w,
                                         int h, int) {
        while (mask) {
            const int r = __builtin_ctz(mask);
            mask &= mask - 1;
            const int jrow = (int)(j0 + cosine_lane_row(w, r, h));      // < N < 2^31
            uf_unite(parent, irow, jrow);
        }
    }
    __device__ __forceinline__ void done(int) {}
};

__device__ __forceinline__ void degree_add(int* p, int v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Degree pass: degree[x] += the edges at x.  Integer adds commute: any grouping gives the same sums.  Probe side: the
// lane's edges of all steps are counted in a register and added once per block.  Row side: the 32 lanes of half h hold the
// 32 probes against the same row of accumulator element r, so the popcount of that half of a wave ballot of bit r is the
// row's count in this step; lane (n = r, h) keeps it, and one vector atomic per wave and step adds the up to 32 counts.
struct EdgesDegree {
    int* degree;
    int mine;
    __device__ __forceinline__ EdgesDegree(const JoinArgs& a, int, bool) : degree(a.degree), mine(0) {}
    __device__ __forceinline__ void rows_ahead(long long, int, int, int, int) {}
    __device__ __forceinline__ void step(unsigned mask, const f32x16&, float, const float (&)[16], int, long long j0, int w, int h,
                                         int n) {
        mine += __builtin_popcount(mask);
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long b = __ballot((mask >> r) & 1u);
            const int c = __builtin_popcount(h ? (unsigned)(b >> 32) : (unsigned)b);
            if (n == r) cnt = c;
        }
        // cnt > 0 only for n < 16 and a row inside the chunk (the edge mask tests it)
        if (cnt) degree_add(degree + (j0 + cosine_lane_row(w, n & 15, h)), cnt);
    }
    __device__ __forceinline__ void done(int irow) {
        if (mine) degree_add(degree + irow, mine);          // mine > 0 needs an edge, and an edge a live probe
    }
};

// fp32 bits -> uint32 in the order of the values (-0 below +0; no NaN arrives: an edge has score > threshold)
__device__ __forceinline__ unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// The key by which a non-core row chooses among the core rows offered to it: the highest score wins a 64-bit maximum, among
// equal scores the smallest core row.  A real key is never 0: its low word is >= 2^31.
__device__ __forceinline__ unsigned long long best_key(float score, int core) {
    return ((unsigned long long)ordered_bits(score) << 32) | (0xFFFFFFFFu - (unsigned)core);
}
__device__ __forceinline__ unsigned best_core(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)key; }

// Gated join, after the degree pass in stream order.  core(x) = degree[x] + 1 >= min_rows.  An edge between two core rows
// is united as in single link (only core rows ever enter the union-find); an edge between a core row c and a non-core row
// x offers c to x: best[x] = max(best[x], (ordered score << 32) | (0xFFFFFFFF - c)), one 64-bit vector atomic max at agent
// scope, no loop.  The maximum of a set does not depend on the order of its elements: the winner is the highest score,
// among equal scores the smallest core row.  best[] starts at 0, and a real key is never 0 (its low word is >= 2^31).
struct EdgesGated {
    int* parent;
    const int* degree;
    unsigned long long* best;
    int need;                 // min_rows - 1 >= 0
    bool pcore;               // the lane's probe row is core
    unsigned cmask;           // bit r: the row of accumulator element r is core
    __device__ __forceinline__ EdgesGated(const JoinArgs& a, int irow, bool live)
        : parent(a.parent), degree(a.degree), best(a.best), need(a.min_rows - 1), cmask(0) {
        pcore = live && degree[irow] >= need;
    }
    __device__ __forceinline__ void rows_ahead(long long c0, int sbase, int w, int h, int rows) {
        const int* __restrict__ dch = degree + c0;
        cmask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (dch[(unsigned)min(acc_row(sbase + w * 32, r) + 4 * h, rows - 1)] >= need) cmask |= 1u << r;
    }
    __device__ __forceinline__ void step(unsigned mask, const f32x16& acc, float qn, const float (&gn)[16], int irow, long long j0,
                                         int w, int h, int) {
        unsigned both = pcore ? mask & cmask : 0u;
        const unsigned one = mask & (pcore ? ~cmask : cmask);
        if (one) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!((one >> r) & 1u)) continue;
                const int jrow = (int)(j0 + cosine_lane_row(w, r, h));
                const int core = pcore ? irow : jrow, other = pcore ? jrow : irow;
                // best_key(score, core), spelled out: through the helper the register allocation of the walk moves
                const unsigned long long key =
                    ((unsigned long long)ordered_bits(cosine_score(acc[r], qn, gn[r])) << 32) | (0xFFFFFFFFu - (unsigned)core);
                __hip_atomic_fetch_max(best + other, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        while (both) {
            const int r = __builtin_ctz(both);
            both &= both - 1;
            uf_unite(parent, irow, (int)(j0 + cosine_lane_row(w, r, h)));
        }
    }
    __device__ __forceinline__ void done(int) {}
};

// The walk over the pairs i < j, one body for every pass: RANGE = false: the chunks cover all rows (first is not read);
// E: what happens to the edges.  The scores and the edge mask are the same code for every E, so the passes of
// ffr_cluster_density see exactly the edge set of ffr_cluster_threshold.
template <bool RANGE, class E>
__global__ __launch_bounds__(256, 1) void k_cluster_walk(const JoinArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 qf[CT_NG * 64];    // probe fragments [64][64]

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    int chunk, tile;
    cosine_block(a.ntiles, chunk, tile);
    const long long c0 = (RANGE ? a.first : 0) + (long long)chunk * a.chunk_rows;
    const long long rem = a.N - c0;
    const int rows = (int)(rem < a.chunk_rows ? rem : a.chunk_rows);    // >= 1
    const int q0 = tile * CT_QT;
    if (c0 + rows <= (long long)q0 + 1) return;        // no row of this chunk is greater than the tile's smallest probe
    const int nq = min(CT_QT, (int)(a.N - q0));
    // the first step that can hold row q0 + 1
    const int step0 = (long long)q0 + 1 > c0 ? (int)(((long long)q0 + 1 - c0) / CT_STEP) : 0;

    cosine_fill_probes(qf, a.emb, q0, nq, tid);
    const float qn_lane = n < nq ? a.norm[q0 + n] : 0.f;
    const int irow = q0 + n;                            // this lane's probe row (an edge needs n < nq)
    E edges(a, irow, n < nq);

    const float* __restrict__ nch = a.norm + c0;
    CosineStream gs(a.emb + (size_t)c0 * CT_DIM, lane);
    gs.prime(min(step0 * CT_STEP + w * 32 + n, rows - 1));
    __syncthreads();

    const int nsteps = (rows + CT_STEP - 1) / CT_STEP;
    for (int step = step0; step < nsteps; ++step) {
        const int sbase = step * CT_STEP;
        const int next = min(gs.row + CT_STEP, rows - 1);
        // gallery norms of the 16 rows this lane scores, fetched ahead of the K loop
        float gn[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) gn[r] = nch[(unsigned)min(acc_row(sbase + w * 32, r) + 4 * h, rows - 1)];
        edges.rows_ahead(c0, sbase, w, h, rows);
        f32x16 acc8[CT_NACC];
        gs.tile(acc8, qf, next);
        const f32x16 acc = COSINE_CHAIN_SUM(acc8);

        // scores, edge test (i < j inside the chunk, score > threshold); the epilogue gets the edges
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = cosine_lane_row(w, r, h);
            const float sc = cosine_score(acc[r], qn_lane, gn[r]);
            if (n < nq && sbase + lr < rows && c0 + sbase + lr > (long long)irow && sc > a.threshold) mask |= 1u << r;
        }
        edges.step(mask, acc, qn_lane, gn, irow, c0 + sbase, w, h, n);
    }
    edges.done(irow);
}

// root[i]: the union-find root of the cluster i belongs to.  A core row: its own; a border row (best[i] != 0): that of the
// core row its key names; a noise row: itself (it never entered the union-find, and no row points at it).  minrow starts
// at the row itself: a root is a member of its cluster.
__global__ __launch_bounds__(256) void k_density_root(const int* __restrict__ parent, const int* __restrict__ degree,
                                                      const unsigned long long* __restrict__ best, int min_rows, int n,
                                                      int* __restrict__ root, int* __restrict__ minrow) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    int r = x;
    if (degree[x] >= min_rows - 1) r = uf_find(parent, x);
    else if (best[x]) r = uf_find(parent, (int)best_core(best[x]));     // a core row of [0, n)
    root[x] = r;
    minrow[x] = x;
}

// the smallest member per cluster; a root is the smallest CORE row, so only a border row can lower it
__global__ __launch_bounds__(256) void k_density_min(const int* __restrict__ root, int n, int* __restrict__ minrow) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n && x < root[x]) __hip_atomic_fetch_min(minrow + root[x], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// keep: null, or the rows that are still there
__global__ __launch_bounds__(256) void k_density_label(const int* __restrict__ root, const int* __restrict__ minrow,
                                                       const int* __restrict__ degree, const unsigned long long* __restrict__ best,
                                                       int min_rows, int n, const uint8_t* __restrict__ keep,
                                                       int64_t* __restrict__ rep, uint8_t* __restrict__ kind,
                                                       int32_t* __restrict__ degree_out) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    if (keep && !keep[x]) {              // ffr_cluster_density_remove: a removed row (its degree and best are 0 already)
        rep[x] = -1;
        kind[x] = 0;
        return;
    }
    const int d = degree[x];
    rep[x] = minrow[root[x]];
    kind[x] = d >= min_rows - 1 ? 2 : best[x] ? 1 : 0;
    if (degree_out) degree_out[x] = d;
}

// ---- ffr_cluster_density_extend: see "Density, extended" in the header ----

constexpr int DX_NONE = 0x7FFFFFFF;       // coremin[]: no core row carries this rep

__device__ __forceinline__ bool dx_rep_ok(int64_t r, int x) { return 0 <= r && r <= (int64_t)x; }

// Seed 1 of 3.  New rows: alone, degree and best 0.  Old rows: the degree read as >= 0, written back and kept in deg0[]
// (the promoted list needs the old value after the walk has added to degree[]).  coremin[] and the counter of P start empty.
__global__ __launch_bounds__(256) void k_dext_init(int* __restrict__ parent, int* __restrict__ degree,
                                                   unsigned long long* __restrict__ best, int* __restrict__ deg0,
                                                   int* __restrict__ coremin, int* __restrict__ pcount, int n_old, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x == 0) *pcount = 0;
    if (x >= n) return;
    coremin[x] = DX_NONE;
    if (x >= n_old) {
        parent[x] = x;
        degree[x] = 0;
        best[x] = 0;
        return;
    }
    const int d = max(degree[x], 0);
    degree[x] = d;
    deg0[x] = d;
}

// Seed 2 of 3, old rows.  A core row: best read as 0, and coremin[rep[x]] = min over the core rows x that carry this rep
// (a rep outside [0, x] names nothing).  A non-core row: a key whose core row is not an old core row is read as 0.
__global__ __launch_bounds__(256) void k_dext_coremin(const int64_t* __restrict__ rep, const int* __restrict__ deg0,
                                                      unsigned long long* __restrict__ best, int* __restrict__ coremin, int need,
                                                      int n_old) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_old) return;
    if (deg0[x] >= need) {
        best[x] = 0;
        const int64_t r = rep[x];
        if (dx_rep_ok(r, x)) __hip_atomic_fetch_min(coremin + r, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const unsigned long long key = best[x];
        const unsigned c = best_core(key);
        if (key && (c >= (unsigned)n_old || deg0[c] < need)) best[x] = 0;
    }
}

// Seed 3 of 3, old rows: an old core row hangs under the smallest old core row of its rep (itself at the least: it took
// part in the minimum, so 0 <= coremin[rep[x]] <= x); every other row starts alone.  The removal seeds through the same
// kernel: deg0 = the degrees after the fall, and only a surviving row (keep) whose label is not hit took part in coremin[].
__global__ __launch_bounds__(256) void k_dext_parent(const int64_t* __restrict__ rep, const int* __restrict__ deg0,
                                                     const int* __restrict__ coremin, const uint8_t* __restrict__ keep,
                                                     const int* __restrict__ hit, int* __restrict__ parent, int need, int n_old) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_old) return;
    const int64_t r = rep[x];
    const bool seeded = deg0[x] >= need && dx_rep_ok(r, x) && (!keep || (keep[x] && !hit[r]));
    parent[x] = seeded ? coremin[r] : x;
}

// P[0 .. m) = the old rows the new rows made core, in any order; their keys are void from here on.  m <= n_old: a row
// enters once.
__global__ __launch_bounds__(256) void k_dext_promoted_list(const int* __restrict__ deg0, const int* __restrict__ degree,
                                                            unsigned long long* __restrict__ best, int* __restrict__ plist,
                                                            int* __restrict__ pcount, int need, int n_old) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_old || deg0[x] >= need || degree[x] < need) return;
    best[x] = 0;
    plist[__hip_atomic_fetch_add(pcount, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = x;
}

// list[slot] = x for the lanes with `listed`, the slots taken from *count: one fetch-add per wave reserves the wave's slots,
// no retry loop; the order of the list is whatever the waves' atomics make it.  Called by all 64 lanes of the wave.  A row
// is listed once per list, by its own thread, so every slot is below the number of rows.
__device__ __forceinline__ void wave_list_push(bool listed, int x, int* __restrict__ list, int* __restrict__ count) {
    const unsigned long long b = __ballot(listed);
    if (!b) return;
    const int lane = threadIdx.x & 63, leader = __builtin_ctzll(b);
    int base = 0;
    if (lane == leader) base = __hip_atomic_fetch_add(count, __builtin_popcountll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader);
    if (listed) list[base + __builtin_popcountll(b & ((1ull << lane) - 1))] = x;
}

// ---- ffr_cluster_remove: see "Removal" in the header ----

// g(x): the label row x came with, under the guard of the seed (an entry outside [0, x] is read as x)
__device__ __forceinline__ int rm_label(const int64_t* rep_in, int x) {
    const int64_t r = rep_in[x];
    return dx_rep_ok(r, x) ? (int)r : x;
}

__global__ __launch_bounds__(256) void k_remove_init(int* __restrict__ hit, int* __restrict__ mcount, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x == 0) *mcount = 0;
    if (x < n) hit[x] = 0;
}

// glabel[x] = g(x), kept so that nothing reads rep_in after this kernel (rep may be rep_in); hit[g(d)] = 1 for a removed d:
// every writer of a cell stores the same 1
__global__ __launch_bounds__(256) void k_remove_mark(const int64_t* __restrict__ rep_in, const uint8_t* __restrict__ keep,
                                                     int* __restrict__ glabel, int* __restrict__ hit, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int g = rm_label(rep_in, x);
    glabel[x] = g;
    if (!keep[x]) hit[g] = 1;
}

// Removed rows and unaffected survivors get their label here.  An affected survivor is listed and seeded: parent[x] =
// prior[x] where that is a row of [0, x] that is itself an affected survivor (it is then listed by its own thread), else x.
__global__ __launch_bounds__(256) void k_remove_list(const int* __restrict__ glabel, const int* __restrict__ hit,
                                                     const uint8_t* __restrict__ keep, const int64_t* __restrict__ prior,
                                                     int* __restrict__ parent, int* __restrict__ list, int* __restrict__ mcount,
                                                     int64_t* __restrict__ rep, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    bool listed = false;
    int p = x;
    if (x < n) {
        if (!keep[x]) {
            rep[x] = -1;
        } else if (!hit[glabel[x]]) {
            rep[x] = glabel[x];
        } else {
            listed = true;
            if (prior) {
                const int64_t q = prior[x];
                if (dx_rep_ok(q, x) && keep[q] && hit[glabel[q]]) p = (int)q;
            }
        }
    }
    if (listed) parent[x] = p;
    wave_list_push(listed, x, list, mcount);                 // slot < m <= n: a row is listed once
}

// ---- ffr_cluster_density_remove: see "Density, removal" in the header ----

constexpr int DR_REMOVED = 0, DR_REJOIN = 1, DR_REKEY = 2;       // counts[]: the lengths r, m, q of the lists R, L, Q

// The three lists start empty, no label is hit, no rep has a core minimum.  deg0[] keeps the old degrees, read as >= 0 (the
// status needs them after the walk has taken from degree[]); a removed row's degree is 0 from here on.
__global__ __launch_bounds__(256) void k_drem_init(const uint8_t* __restrict__ keep, int* __restrict__ degree,
                                                   int* __restrict__ deg0, int* __restrict__ coremin, int* __restrict__ hit,
                                                   int* __restrict__ counts, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < 3) counts[x] = 0;
    if (x >= n) return;
    coremin[x] = DX_NONE;
    hit[x] = 0;
    const int d = max(degree[x], 0);
    deg0[x] = d;
    degree[x] = keep[x] ? d : 0;
}

// R[0 .. r) = the removed rows, in any order: what follows is integer adds
__global__ __launch_bounds__(256) void k_drem_removed_list(const uint8_t* __restrict__ keep, int* __restrict__ rlist,
                                                           int* __restrict__ counts, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    wave_list_push(x < n && !keep[x], x, rlist, counts + DR_REMOVED);
}

// After the fall.  A wrong state can take a degree below 0: it is read as 0, as on entry.  LOST = a row that was core and
// is no more, removed or demoted: its label is hit (every writer of a cell stores the same 1).
__global__ __launch_bounds__(256) void k_drem_status(const int64_t* __restrict__ rep_in, const uint8_t* __restrict__ keep,
                                                     const int* __restrict__ deg0, int* __restrict__ degree,
                                                     int* __restrict__ hit, int need, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int d = max(degree[x], 0);
    degree[x] = d;
    if (deg0[x] >= need && !(keep[x] && d >= need)) hit[rm_label(rep_in, x)] = 1;
}

// Seed 1 of 2 and the keys, on the final degrees and hit flags.  A removed row: key 0.  A core row: key 0; where its label
// is hit it goes into L (its parent stays x: k_dext_parent), else it takes part in the core minimum of its rep, as in
// k_dext_coremin.  A non-core survivor keeps its key iff that names a row of [0, n) that survives and is core; it goes
// into Q, key 0, if its key is void or if it was core itself (a demoted row never had a key).  A row with no key that was
// not core is noise and stays noise: its core neighbours can only have become fewer.
__global__ __launch_bounds__(256) void k_drem_seed_lists(const int64_t* __restrict__ rep_in, const uint8_t* __restrict__ keep,
                                                         const int* __restrict__ deg0, const int* __restrict__ degree,
                                                         const int* __restrict__ hit, unsigned long long* __restrict__ best,
                                                         int* __restrict__ coremin, int* __restrict__ llist,
                                                         int* __restrict__ qlist, int* __restrict__ counts, int need, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    bool rejoin = false, rekey = false;
    if (x < n) {
        if (!keep[x]) {
            best[x] = 0;
        } else if (degree[x] >= need) {
            best[x] = 0;
            const int64_t r = rep_in[x];
            if (hit[rm_label(rep_in, x)]) rejoin = true;
            else if (dx_rep_ok(r, x)) __hip_atomic_fetch_min(coremin + r, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned long long key = best[x];
            const unsigned c = best_core(key);
            const bool holds = key && c < (unsigned)n && keep[c] && degree[c] >= need;
            rekey = deg0[x] >= need || (key && !holds);
            if (rekey) best[x] = 0;
        }
    }
    wave_list_push(rejoin, x, llist, counts + DR_REJOIN);
    wave_list_push(rekey, x, qlist, counts + DR_REKEY);
}

// ---- k_list_walk: see "List walk" in the header ----

constexpr int RM_SPAN_STEPS = 8;          // 128-slot steps an item of the removal streams per probe fill, at most

struct ListArgs {
    const float* emb;         // [N][512]
    const float* norm;        // [N]
    int* parent;              // [N]
    const int* list;          // the first *count entries are set, each a row < bound
    const int* count;
    int bound;                // *count is read as at most this: N (the removals), n_old (promoted pass)
    float threshold;
    // the promoted pass and the two walks of the density removal only
    int* degree;              // [N]; final but for the fall, which takes from it
    unsigned long long* best; // [N]
    int need;
    const uint8_t* keep;      // [N], the density removal only
};

// What differs between the two walks over a list; the item loop is k_list_walk's.
//   SPAN_STEPS     the most 128-slot steps an item spans: prow / pnorm hold that many
//   BLOCKS_PER_CU  the kernel's launch bound
//   TRIANGLE       pairs go by list position a < b: items below the diagonal are skipped, the others start at step0
//   probes(a, m)   how many probe positions there are; probe_row(a, pos) the row at one (pos below that count);
//                  fill(qf, a, q0, nq, tid) the fragments of the probes at the positions q0 .. q0 + nq
//   pair(...)      does (probe at position apos, listed row at position bpos) count?
//   P(a, irow, live) per-probe state, once per item; edge(a, irow, jrow, sc) what an edge does
// Promoted pass (ffr_cluster_density_extend): the probes are the old rows [0, n_old) themselves and every pair but (p, p)
// counts.  The listed row is always core, so an edge is a unite when the probe is core and an offer of the listed row to
// best[probe] when it is not.  One step per item: two blocks share a CU.
struct ProbesAreRows {           // the orientation: the probes are the rows [0, bound) themselves, every pair but (p, p) counts
    static constexpr bool TRIANGLE = false;
    static __device__ __forceinline__ int probes(const ListArgs& a, int) { return a.bound; }
    static __device__ __forceinline__ int probe_row(const ListArgs&, int pos) { return pos; }
    static __device__ __forceinline__ void fill(f32x4* qf, const ListArgs& a, int q0, int nq, int tid) {
        cosine_fill_probes(qf, a.emb, q0, nq, tid);
    }
    static __device__ __forceinline__ bool pair(int, int, int irow, int jrow) { return jrow != irow; }
};
struct WalkPromoted : ProbesAreRows {
    static constexpr int SPAN_STEPS = 1, BLOCKS_PER_CU = 2;
    bool pcore;
    __device__ __forceinline__ WalkPromoted(const ListArgs& a, int irow, bool live) : pcore(live && a.degree[irow] >= a.need) {}
    __device__ __forceinline__ void edge(const ListArgs& a, int irow, int jrow, float sc) const {
        if (pcore) uf_unite(a.parent, irow, jrow);
        else __hip_atomic_fetch_max(a.best + irow, best_key(sc, jrow), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// Removal (ffr_cluster_remove): the self-join of the listed rows, probe list[a] against row list[b] for the positions
// a < b; every edge is a unite on the rows' own numbers.  A probe fill (64 KiB into LDS) is shared by up to 1024 rows and the
// prefetch ring runs across the steps.
struct WalkRemove {
    static constexpr int SPAN_STEPS = RM_SPAN_STEPS, BLOCKS_PER_CU = 1;
    static constexpr bool TRIANGLE = true;
    __device__ __forceinline__ WalkRemove(const ListArgs&, int, bool) {}
    static __device__ __forceinline__ int probes(const ListArgs&, int m) { return m; }
    static __device__ __forceinline__ int probe_row(const ListArgs& a, int pos) { return a.list[pos]; }
    static __device__ __forceinline__ void fill(f32x4* qf, const ListArgs& a, int q0, int nq, int tid) {
        cosine_fill_probes_gather(qf, a.emb, a.list + q0, nq, tid);
    }
    static __device__ __forceinline__ bool pair(int apos, int bpos, int, int) { return bpos > apos; }
    __device__ __forceinline__ void edge(const ListArgs& a, int irow, int jrow, float) const { uf_unite(a.parent, irow, jrow); }
};

// The two walks of ffr_cluster_density_remove, in the orientation of the promoted pass: all N rows are probes, the listed
// rows come from R (the removed rows) and Q (the rows that choose again).  SPAN_STEPS and BLOCKS_PER_CU: EXPERIMENTS.md.
// Degrees fall: a surviving probe adjacent to a listed removed row loses that edge.  Integer adds commute; a removed probe
// is masked (its degree is 0 already).
struct WalkFall : ProbesAreRows {
    static constexpr int SPAN_STEPS = RM_SPAN_STEPS, BLOCKS_PER_CU = 1;
    bool alive;
    __device__ __forceinline__ WalkFall(const ListArgs& a, int irow, bool live) : alive(live && a.keep[irow]) {}
    __device__ __forceinline__ void edge(const ListArgs& a, int irow, int, float) const {
        if (alive) degree_add(a.degree + irow, -1);
    }
};

// Keys again: a surviving core probe is offered to the listed row, which is a non-core survivor whose key was zeroed: the
// one 64-bit max of the gated join, so the highest score wins, then the smallest core row, whatever the order.
struct WalkRekey : ProbesAreRows {
    static constexpr int SPAN_STEPS = RM_SPAN_STEPS, BLOCKS_PER_CU = 1;
    bool pcore;
    __device__ __forceinline__ WalkRekey(const ListArgs& a, int irow, bool live)
        : pcore(live && a.keep[irow] && a.degree[irow] >= a.need) {}
    __device__ __forceinline__ void edge(const ListArgs& a, int irow, int jrow, float sc) const {
        if (pcore) __hip_atomic_fetch_max(a.best + jrow, best_key(sc, irow), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// Probes against the rows of a list.  A work item is (tile of 32 probe positions, span of `spi` steps of 128 list positions);
// a fixed grid loops over the items, m read once from device memory (uniform in the block: the barriers and the first
// `continue` are legal; the second one is per wave, after the item's barriers), so an empty list is one early return per
// block.  spi is sized from m so that there are about 4 items per block, up to P::SPAN_STEPS.  The span's rows and their
// norms are staged in LDS once per item; slots past the span's end repeat its last listed row, in bounds, and are masked
// out.  The rows are gathered through CosineStreamT<GatherRows>; the tile, the chain sum and cosine_score are those of
// k_cluster_walk.
template <class P>
__global__ __launch_bounds__(256, P::BLOCKS_PER_CU) void k_list_walk(const ListArgs a) {
    constexpr int SPAN = P::SPAN_STEPS * CT_STEP;
    __shared__ __attribute__((aligned(16))) f32x4 qf[CT_NG * 64];
    __shared__ int prow[SPAN];
    __shared__ float pnorm[SPAN];

    const int m = min(*a.count, a.bound);
    if (m < (P::TRIANGLE ? 2 : 1)) return;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = P::probes(a, m);
    const int ntiles = (np + CT_QT - 1) / CT_QT, nst = (m + CT_STEP - 1) / CT_STEP;
    const long long fit = (long long)ntiles * nst / (4LL * gridDim.x);
    const int spi = (int)max(1LL, min((long long)P::SPAN_STEPS, fit));
    const int ngroups = (nst + spi - 1) / spi, span = spi * CT_STEP;
    const long long items = (long long)ntiles * ngroups;

    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int tile = (int)(it / ngroups), group = (int)(it - (long long)tile * ngroups);
        const int q0 = tile * CT_QT, nq = min(CT_QT, np - q0);             // >= 1
        const int s0 = group * span, ns = min(span, m - s0);               // >= 1
        if (P::TRIANGLE && s0 + ns <= q0 + 1) continue;     // no position of this span is above the tile's first
        const int step0 = P::TRIANGLE && q0 + 1 > s0 ? (q0 + 1 - s0) / CT_STEP : 0;
        __syncthreads();                                    // the previous item's reads of qf, prow, pnorm are over
        P::fill(qf, a, q0, nq, tid);
        for (int e = tid; e < span; e += 256) {
            const int p = a.list[s0 + min(e, ns - 1)];
            prow[e] = p;
            pnorm[e] = a.norm[p];
        }
        __syncthreads();

        const bool live = n < nq;
        const int apos = q0 + n;                            // the lane's probe position
        const int irow = live ? P::probe_row(a, apos) : 0;
        const float qn = live ? a.norm[irow] : 0.f;
        const P walk(a, irow, live);

        // the steps in which this wave has a slot below ns (wave-uniform: only a span's last step can lack one)
        const int nsteps = (ns - w * 32 + CT_STEP - 1) / CT_STEP;          // nsteps * CT_STEP <= span
        if (step0 >= nsteps) continue;
        CosineStreamT<GatherRows> gs(a.emb, lane);
        gs.prime(prow[min(step0 * CT_STEP + w * 32 + n, ns - 1)]);
        for (int step = step0; step < nsteps; ++step) {
            const int sbase = step * CT_STEP;
            f32x16 acc8[CT_NACC];
            gs.tile(acc8, qf, prow[min(sbase + CT_STEP + w * 32 + n, ns - 1)]);
            const f32x16 acc = COSINE_CHAIN_SUM(acc8);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = sbase + cosine_lane_row(w, r, h);           // < span
                const int jrow = prow[lr];
                const float sc = cosine_score(acc[r], qn, pnorm[lr]);
                if (live && lr < ns && P::pair(apos, s0 + lr, irow, jrow) && sc > a.threshold) walk.edge(a, irow, jrow, sc);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_remove_flatten(const int* __restrict__ parent, const int* __restrict__ list,
                                                        const int* __restrict__ mcount, int n, int64_t* __restrict__ rep) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= min(*mcount, n)) return;
    const int x = list[s];
    rep[x] = uf_find(parent, x);
}

// parent[x] = x, degree[x] = 0, best[x] = 0
__global__ __launch_bounds__(256) void k_density_init(int* __restrict__ parent, int* __restrict__ degree,
                                                      unsigned long long* __restrict__ best, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    parent[x] = x;
    degree[x] = 0;
    best[x] = 0;
}

struct TemplateArgs {
    const float* emb;         // [.][512]
    const float* norm;        // [.] or null
    const int64_t* order;     // rows sorted by cluster, then index
    const int64_t* offsets;   // [C + 1]
    float* out;               // [C][512]
    long long C;
};

__global__ __launch_bounds__(256) void k_cluster_templates(const TemplateArgs a) {
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= a.C) return;
    const long long lo = a.offsets[c], hi = a.offsets[c + 1];
    f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
    for (long long e = lo; e < hi; ++e) {
        const float* p = a.emb + (size_t)a.order[e] * CT_DIM;
        float nr;
        if (a.norm) {
            nr = a.norm[a.order[e]];
        } else {                         // |x_r| in the summation order of k_row_norms
            float aa = 0.f;
            for (int k = lane; k < CT_DIM; k += 64) {
                const float v = p[k];
                aa += v * v;
            }
            nr = sqrtf(wave_sum(aa));
        }
        if (!(nr > 0.f)) continue;       // a zero row contributes zero
        const f32x4 x0 = *(const f32x4*)(p + 8 * lane), x1 = *(const f32x4*)(p + 8 * lane + 4);
        t0 += x0 / nr;
        t1 += x1 / nr;
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) ss += t0[k] * t0[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) ss += t1[k] * t1[k];
    const float tn = sqrtf(wave_sum(ss));
    if (tn > 0.f) {
        t0 /= tn;
        t1 /= tn;
    }
    float* o = a.out + (size_t)c * CT_DIM + 8 * lane;
    *(f32x4*)o = t0;
    *(f32x4*)(o + 4) = t1;
}

}  // namespace

// The search balances a rectangle; here only the blocks on and above the diagonal work, about half of chunks x tiles, and
// the ones on the diagonal less than the others: aim at 4 working blocks per CU so that the uneven ones even out.
void cluster_plan(long long N, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    *ntiles = (int)((N + CT_QT - 1) / CT_QT);
    cosine_chunks(*ntiles, N, 8, num_cus, nchunks, chunk_rows);
}

// The chunks cover the N - N_old new rows only, the tiles every probe.  Of the chunks x tiles rectangle the share
// 1 - N_new / 2N has work (all of it over the old rows, half of it over the new rows' own triangle): the same aim of 4
// working blocks per CU gives 8 N / (2 N - N_new) blocks per CU, 8 at N_old = 0 (cluster_plan) and 4 for a small batch.
void cluster_extend_plan(long long N_old, long long N, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    const long long n_new = N - N_old;
    *ntiles = (int)((N + CT_QT - 1) / CT_QT);
    const long long per_cu = N > 0 ? (8 * N + 2 * N - n_new - 1) / (2 * N - n_new) : 8;
    cosine_chunks(*ntiles, n_new, per_cu, num_cus, nchunks, chunk_rows);
}

// 256-thread blocks throughout.  The arguments are converted to the kernel's parameter types here, so a call site passes
// its pointers as they are.
template <class... KA, class... A>
static hipError_t launch(void (*kernel)(KA...), unsigned grid, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, static_cast<KA>(args)...);
    return hipGetLastError();
}
#define LAUNCH(...)                                                          \
    do {                                                                     \
        if (hipError_t e_ = launch(__VA_ARGS__); e_ != hipSuccess) return e_; \
    } while (0)

static unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

// prior = null: ffr_cluster_threshold (N_old = 0), the walk compiled with the constant 0
hipError_t launch_cluster_extend(const float* emb, const float* norms, long long N_old, long long N, float threshold, int ntiles,
                                 int nchunks, long long chunk_rows, const int64_t* prior, int* parent, int64_t* rep,
                                 hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (prior) LAUNCH(k_cluster_seed, blocks_of(N), stream, parent, prior, (int)N);
    else LAUNCH(k_cluster_init, blocks_of(N), stream, parent, (int)N);
    if (N > 1 && N_old < N) {
        const JoinArgs a{emb, norms, parent, N, chunk_rows, threshold, nchunks, ntiles, N_old, nullptr, nullptr, 0};
        const unsigned grid = (unsigned)((long long)nchunks * ntiles);
        if (prior) LAUNCH(k_cluster_walk<true, EdgesUnite>, grid, stream, a);
        else LAUNCH(k_cluster_walk<false, EdgesUnite>, grid, stream, a);
    }
    LAUNCH(k_cluster_flatten, blocks_of(N), stream, parent, (int)N, rep);
    return hipSuccess;
}

// root, min, label: the end of the three density launchers; keep: the removal's, else null
static hipError_t density_finish(long long N, int min_rows, const int* parent, const int* degree, const unsigned long long* best,
                                 const uint8_t* keep, int* root, int* minrow, int64_t* rep, uint8_t* kind, int32_t* degree_out,
                                 hipStream_t stream) {
    LAUNCH(k_density_root, blocks_of(N), stream, parent, degree, best, min_rows, (int)N, root, minrow);
    LAUNCH(k_density_min, blocks_of(N), stream, root, (int)N, minrow);
    LAUNCH(k_density_label, blocks_of(N), stream, root, minrow, degree, best, min_rows, (int)N, keep, rep, kind, degree_out);
    return hipSuccess;
}

hipError_t launch_cluster_density(const float* emb, const float* norms, long long N, float threshold, int min_rows, int ntiles,
                                  int nchunks, long long chunk_rows, int* parent, int* degree, int* root, int* minrow,
                                  unsigned long long* best, int64_t* rep, uint8_t* kind, int32_t* degree_out, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    LAUNCH(k_density_init, blocks_of(N), stream, parent, degree, best, (int)N);
    if (N > 1) {
        const JoinArgs a{emb, norms, parent, N, chunk_rows, threshold, nchunks, ntiles, 0, degree, best, min_rows};
        const unsigned grid = (unsigned)((long long)nchunks * ntiles);
        LAUNCH(k_cluster_walk<false, EdgesDegree>, grid, stream, a);
        LAUNCH(k_cluster_walk<false, EdgesGated>, grid, stream, a);
    }
    return density_finish(N, min_rows, parent, degree, best, nullptr, root, minrow, rep, kind, degree_out, stream);
}

// the blocks loop over the items, which are counted on the device; two blocks of 64 KiB LDS fit a CU
int cluster_list_grid(long long rows, int num_cus) {
    const long long tiles = (rows + CT_QT - 1) / CT_QT, most = tiles * ((rows + CT_STEP - 1) / CT_STEP);
    return (int)std::max(1LL, std::min(most, 2LL * num_cus));
}

hipError_t launch_cluster_density_extend(const float* emb, const float* norms, long long N_old, long long N, float threshold,
                                         int min_rows, int ntiles, int nchunks, long long chunk_rows, int promoted_grid, int* parent,
                                         int* deg0, int* coremin, int* root, int* minrow, int* plist, int* pcount, int64_t* rep,
                                         uint8_t* kind, int32_t* degree, unsigned long long* best, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    const unsigned nbo = blocks_of(N_old);
    const int need = min_rows - 1;
    LAUNCH(k_dext_init, blocks_of(N), stream, parent, degree, best, deg0, coremin, pcount, (int)N_old, (int)N);
    if (N_old > 0) {
        LAUNCH(k_dext_coremin, nbo, stream, rep, deg0, best, coremin, need, (int)N_old);
        LAUNCH(k_dext_parent, nbo, stream, rep, deg0, coremin, nullptr, nullptr, parent, need, (int)N_old);
    }
    if (N > 1 && N_old < N) {
        const JoinArgs a{emb, norms, parent, N, chunk_rows, threshold, nchunks, ntiles, N_old, degree, best, min_rows};
        const unsigned grid = (unsigned)((long long)nchunks * ntiles);
        LAUNCH(k_cluster_walk<true, EdgesDegree>, grid, stream, a);
        if (N_old > 0) LAUNCH(k_dext_promoted_list, nbo, stream, deg0, degree, best, plist, pcount, need, (int)N_old);
        LAUNCH(k_cluster_walk<true, EdgesGated>, grid, stream, a);
        if (N_old > 1) {
            const ListArgs p{emb, norms, parent, plist, pcount, (int)N_old, threshold, degree, best, need};
            LAUNCH(k_list_walk<WalkPromoted>, (unsigned)promoted_grid, stream, p);
        }
    }
    return density_finish(N, min_rows, parent, degree, best, nullptr, root, minrow, rep, kind, nullptr, stream);
}

hipError_t launch_cluster_remove(const float* emb, const float* norms, long long N, float threshold, int walk_grid,
                                 const int64_t* rep_in, const int64_t* prior, const uint8_t* keep, int* parent, int* glabel, int* hit,
                                 int* list, int* mcount, int64_t* rep, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    LAUNCH(k_remove_init, blocks_of(N), stream, hit, mcount, (int)N);
    LAUNCH(k_remove_mark, blocks_of(N), stream, rep_in, keep, glabel, hit, (int)N);
    LAUNCH(k_remove_list, blocks_of(N), stream, glabel, hit, keep, prior, parent, list, mcount, rep, (int)N);
    if (N > 1) {
        const ListArgs a{emb, norms, parent, list, mcount, (int)N, threshold, nullptr, nullptr, 0};
        LAUNCH(k_list_walk<WalkRemove>, (unsigned)walk_grid, stream, a);
    }
    LAUNCH(k_remove_flatten, blocks_of(N), stream, parent, list, mcount, (int)N, rep);
    return hipSuccess;
}

hipError_t launch_cluster_density_remove(const float* emb, const float* norms, long long N, float threshold, int min_rows,
                                         int walk_grid, const uint8_t* keep, int* parent, int* deg0, int* coremin, int* hit,
                                         int* root, int* minrow, int* rlist, int* llist, int* qlist, int* counts, int64_t* rep,
                                         uint8_t* kind, int32_t* degree, unsigned long long* best, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    const unsigned nb = blocks_of(N), grid = (unsigned)walk_grid;
    const int need = min_rows - 1, n = (int)N;
    LAUNCH(k_drem_init, nb, stream, keep, degree, deg0, coremin, hit, counts, n);
    LAUNCH(k_drem_removed_list, nb, stream, keep, rlist, counts, n);
    if (N > 1) {
        const ListArgs fall{emb, norms, nullptr, rlist, counts + DR_REMOVED, n, threshold, degree, nullptr, need, keep};
        LAUNCH(k_list_walk<WalkFall>, grid, stream, fall);
    }
    LAUNCH(k_drem_status, nb, stream, rep, keep, deg0, degree, hit, need, n);
    LAUNCH(k_drem_seed_lists, nb, stream, rep, keep, deg0, degree, hit, best, coremin, llist, qlist, counts, need, n);
    LAUNCH(k_dext_parent, nb, stream, rep, degree, coremin, keep, hit, parent, need, n);
    if (N > 1) {
        const ListArgs rejoin{emb, norms, parent, llist, counts + DR_REJOIN, n, threshold, nullptr, nullptr, 0, nullptr};
        LAUNCH(k_list_walk<WalkRemove>, grid, stream, rejoin);
        const ListArgs rekey{emb, norms, nullptr, qlist, counts + DR_REKEY, n, threshold, degree, best, need, keep};
        LAUNCH(k_list_walk<WalkRekey>, grid, stream, rekey);
    }
    return density_finish(N, min_rows, parent, degree, best, keep, root, minrow, rep, kind, nullptr, stream);
}

hipError_t launch_cluster_templates(const float* emb, const float* norms, const int64_t* order, const int64_t* offsets,
                                    long long C, float* templates, hipStream_t stream) {
    if (C <= 0) return hipSuccess;
    return launch(k_cluster_templates, (unsigned)((C + 3) / 4), stream, TemplateArgs{emb, norms, order, offsets, templates, C});
}

}  // namespace ffr
