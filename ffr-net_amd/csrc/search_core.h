// search_core.h -- the block of a top-k search over one chunk of the gallery, shared by k_search_topk (search.hip, the
// exact fp32 tile of cosine_tile.h) and k_search_coarse (search_coarse.hip, the bf16 tile of coarse_tile.h).  The two
// differ in the tile alone.  A block (4 waves) holds a tile of 32 probes in LDS and walks one contiguous chunk of the
// gallery, 128 rows per step (32 per wave):
//  - K loop: the 32 x 128 tile of scores.  Every (q, g) score is the same arithmetic wherever it sits in a tile, a block
//    or a shard: results are bitwise independent of Q, of the chunking and of the sharding.
//  - Epilogue, outside the K loop: lane (n, h) holds the 16 scores of probe n against gallery rows (r&3) + 8(r>>2) + 4h;
//    each is compared with the probe's current k-th score (LDS).  Rows of a step have larger indices than every listed
//    row, so a row enters iff its score is strictly greater (or the list is not full yet).  Survivors go to a per
//    (probe, wave) LDS slot array; once the lists fill, most steps have none and skip the merge (one __syncthreads_or).
//  - Merge (rare): the new list is the rank scatter of list + candidates -- rank = number of elements that beat it under
//    the total order -- into the second LDS list buffer.  The top k of a set under a total order is unique, so the list
//    is the same whatever order the candidates arrive in: no atomics, no ordering between waves needed.
//  - Each block writes one sorted list per (chunk, probe); k_topk_merge (search.hip) folds the chunk lists.
//  - Addressing: a block's chunk is a 64-bit base pointer plus 32-bit element offsets inside it (<= 2^20 rows =
//    2^29 elements per chunk), so galleries beyond 2 GiB / 4 GiB work; rows past the chunk's end are clamped to its last
//    row (in bounds) and never become candidates.
//  - Grid: chunks x probe tiles >= the CU count (also at Q = 1: 256 chunks of a 2^20-row gallery); block b runs on XCD
//    b % 8, and the bijective remap gives each XCD a contiguous run of logical blocks, chunk-major, so the probe tiles
//    of one chunk share that XCD's L2 and the chunk comes from HBM about once.
//  - Live count: with a device pointer in SearchArgs::live, the probes [*live, Q) are not searched; blocks whose probe
//    tile lies past the count leave at once.  A null pointer searches all Q.
//  - Subjects (k_search_subjects, search.hip; include/ffrnet.h, ffr_search_topk_subjects): a compile-time policy.  SR_ROWS is
//    the block above.  SR_LIVE reads subject[G] beside the norms and adds `subject >= 0` to the candidate test: removed rows
//    never enter, the merge is the same, and the subject of a listed row is read again at write-out.  SR_DISTINCT lists
//    subjects, not rows: candidates and list entries carry their subject in LDS, and the merge is the rank scatter over the
//    elements that no other element of their own subject beats, so the list stays subject-unique and still does not depend
//    on the order of arrival (no atomics here either).  The policy goes with either tile, and the chunk's subjects, like its
//    norms, are a 64-bit base (subject + c0) plus 32-bit offsets.  The threshold argument holds: with k subjects listed, a row at or below the k-th score loses
//    to k listed entries on score or index, or to its own subject's entry.
//  - Filter (k_search_filtered, search.hip; include/ffrnet.h, ffr_search_topk_filtered; k_search_coarse_filtered and
//    k_search_coarse_filtered_live, search_coarse.hip; ffr_search_topk_coarse_filtered): a second compile-time policy, TAG,
//    that goes with each of the three above and with either tile.  The candidate test so far depends on the row alone; TAG adds a term that depends
//    on the probe too: `(tag[g] & qmask[q]) != 0`.  Lane (n, h) keeps its probe's mask word in a register beside qn_lane (0
//    for a probe past Q, which takes nothing anyway), and the 16 tag words of the rows it scores are read beside their norms
//    and subjects, a 64-bit base (tag + c0) plus the same clamped 32-bit offsets.  Nothing else changes and no LDS is added:
//    the list is the top k of a set under a total order, so it does not matter which rows were candidates before, and the
//    threshold argument holds per probe with "rows" read as "rows admissible for this probe".  The K loop still scores every
//    row: a step none of whose rows is admissible costs what any step costs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coarse_tile.h"
#include "cosine_tile.h"
#include "device_util.h"
#include "ffr_kernels.h"

namespace ffr {

constexpr int SR_CAND = 32;               // candidate slots per (probe, wave) and step
constexpr int SR_MAX_K = 128;             // rows listed per probe (SR_ROWS, SR_LIVE)
constexpr int SR_MAX_K_DISTINCT = 64;     // subjects listed per probe (SR_DISTINCT): see sr_lds_bytes
constexpr int SR_NO_VICTIM = 255;         // SR_DISTINCT: a candidate that replaces no listed row (list positions are < 64)

enum { SR_ROWS = 0, SR_LIVE = 1, SR_DISTINCT = 2 };     // the subject policy of a search block

// SearchArgs: ffr_kernels.h, where the host units fill it

// The tile a search block scores with: the exact fp32 one of cosine_tile.h, or the bf16 one of coarse_tile.h
template <bool COARSE> struct SearchTile;
template <> struct SearchTile<false> {
    typedef CosineStream Stream;
    static __device__ __forceinline__ const float* chunk(const SearchArgs& a, long long c0) { return a.gallery + (size_t)c0 * CT_DIM; }
};
template <> struct SearchTile<true> {
    typedef CoarseStream Stream;
    static __device__ __forceinline__ const uint16_t* chunk(const SearchArgs& a, long long c0) { return a.plane + (size_t)c0 * CT_DIM; }
};

// LDS: probe fragments [64][64] f32x4 (coarse: two planes [32][64] of 8 bf16, the same 64 KB) |
// candidates cs[32][4][32] f32, cr[32][4][32] u8, cn[32][4] | thr[32], nl[32] | two lists [32][k] of (score, chunk row)
constexpr size_t SR_OFF_CS = (size_t)CT_NG * 64 * 16;
constexpr size_t SR_OFF_CR = SR_OFF_CS + CT_QT * CT_WAVES * SR_CAND * 4;
constexpr size_t SR_OFF_CN = SR_OFF_CR + CT_QT * CT_WAVES * SR_CAND;
constexpr size_t SR_OFF_THR = SR_OFF_CN + CT_QT * CT_WAVES * 4;
constexpr size_t SR_OFF_NL = SR_OFF_THR + CT_QT * 4;
constexpr size_t SR_OFF_LIST = SR_OFF_NL + CT_QT * 4;
// SR_DISTINCT adds, behind the lists: candidate subjects cu[32][4][32] i32 | two lists [32][k] of subjects | the candidates'
// victims cv[32][4][32] u8.  One block per CU has 160 KiB: 71 424 + 512 k without subjects (136 960 at k = 128),
// 91 904 + 768 k with them -- 141 056 at k = 64, and 190 208 at k = 128, which does not fit: SR_DISTINCT serves
// k <= SR_MAX_K_DISTINCT.
__host__ __device__ constexpr size_t sr_lds_bytes(int k, bool distinct = false) {
    return SR_OFF_LIST + 2 * (size_t)CT_QT * k * 8 +
           (distinct ? (size_t)CT_QT * CT_WAVES * SR_CAND * 5 + 2 * (size_t)CT_QT * k * 4 : 0);
}
static_assert(sr_lds_bytes(SR_MAX_K) <= 160 * 1024 && sr_lds_bytes(SR_MAX_K_DISTINCT, true) <= 160 * 1024 &&
              sr_lds_bytes(SR_MAX_K, true) > 160 * 1024, "LDS of one search block");

// One block of a search: k_search_topk (search.hip) is the exact instantiation, k_search_coarse (search_coarse.hip) the
// bf16 one, k_search_subjects (search.hip) the exact one with a subject policy, k_search_coarse_live (search_coarse.hip) the
// bf16 one under the removal mask.  They differ in the tile and in what the policy adds; the threshold test, the survivor
// slots and the rank-scatter merge are this text.  OUT_U = false: the lists go out without their subject plane (out_u is not
// touched and may be null) -- a shortlist of rows, whose reader looks subject[row] up again.  TAG: k_search_filtered
// (search.hip), the candidate test under the per-probe filter of SearchArgs::tag and qmask; with the bf16 tile,
// k_search_coarse_filtered (SR_ROWS) and k_search_coarse_filtered_live (SR_LIVE), both without the subject plane
// (search_coarse.hip): the shortlist of the rows admissible for each probe.
template <bool COARSE, int SUBJ = SR_ROWS, bool OUT_U = SUBJ != SR_ROWS, bool TAG = false>
__device__ __forceinline__ void search_block(const SearchArgs& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    f32x4* qf = (f32x4*)sm;
    float* cs = (float*)(sm + SR_OFF_CS);
    unsigned char* cr = sm + SR_OFF_CR;
    int* cn = (int*)(sm + SR_OFF_CN);
    float* thr = (float*)(sm + SR_OFF_THR);
    int* nl = (int*)(sm + SR_OFF_NL);
    float* ls0 = (float*)(sm + SR_OFF_LIST);              // list buffer b: scores at ls0 + b*QT*k, rows at li0 + b*QT*k
    int* li0 = (int*)(ls0 + 2 * CT_QT * a.k);
    int *cu = nullptr, *lu0 = nullptr;                    // SR_DISTINCT: candidate subjects, the lists' subjects, victims
    unsigned char* cv = nullptr;
    if constexpr (SUBJ == SR_DISTINCT) {
        cu = (int*)(sm + sr_lds_bytes(a.k));
        lu0 = cu + CT_QT * CT_WAVES * SR_CAND;
        cv = (unsigned char*)(lu0 + 2 * CT_QT * a.k);
    }

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k;

    int chunk, tile;
    cosine_block(a.ntiles, chunk, tile);
    const int Q = a.live ? min(*a.live, a.Q) : a.Q;
    if (tile * CT_QT >= Q) return;
    const long long c0 = (long long)chunk * a.chunk_rows;
    const long long rem = a.G - c0;
    const int rows = (int)(rem < a.chunk_rows ? rem : a.chunk_rows);    // >= 1
    const int q0 = tile * CT_QT;
    const int nq = min(CT_QT, Q - q0);

    if constexpr (COARSE) coarse_fill_probes((u32x4*)sm, a.query, a.qnorm, q0, nq, tid);
    else cosine_fill_probes(qf, a.query, q0, nq, tid);
    if (tid < CT_QT) {
        thr[tid] = tid < nq ? -INFINITY : INFINITY;    // probes past Q never take a candidate
        nl[tid] = 0;
    }
    const float qn_lane = n < nq ? a.qnorm[q0 + n] : 0.f;
    uint32_t qm_lane = 0;                       // TAG: the mask word of probe n
    if constexpr (TAG) qm_lane = n < nq ? a.qmask[q0 + n] : 0u;

    const float* __restrict__ nch = a.gnorm + c0;
    const int32_t* __restrict__ sch = SUBJ != SR_ROWS ? a.subject + c0 : nullptr;
    const uint32_t* __restrict__ tch = TAG ? a.tag + c0 : nullptr;
    typename SearchTile<COARSE>::Stream gs(SearchTile<COARSE>::chunk(a, c0), lane);
    gs.prime(min(w * 32 + n, rows - 1));
    __syncthreads();

    int cur = 0;
    const int nsteps = (rows + CT_STEP - 1) / CT_STEP;
    for (int step = 0; step < nsteps; ++step) {
        const int sbase = step * CT_STEP;
        const int next = min(gs.row + CT_STEP, rows - 1);
        // gallery norms of the 16 rows this lane scores, fetched ahead of the K loop
        float gn[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) gn[r] = nch[(unsigned)min(acc_row(sbase + w * 32, r) + 4 * h, rows - 1)];
        int gu[SUBJ != SR_ROWS ? 16 : 1];        // and their subjects
        if constexpr (SUBJ != SR_ROWS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) gu[r] = sch[(unsigned)min(acc_row(sbase + w * 32, r) + 4 * h, rows - 1)];
        }
        uint32_t gt[TAG ? 16 : 1];               // and their tag words
        if constexpr (TAG) {
#pragma unroll
            for (int r = 0; r < 16; ++r) gt[r] = tch[(unsigned)min(acc_row(sbase + w * 32, r) + 4 * h, rows - 1)];
        }
        f32x16 acc;
        if constexpr (COARSE) {
            acc = gs.tile((const u32x4*)sm, next);
        } else {
            f32x16 acc8[CT_NACC];
            gs.tile(acc8, qf, next);
            acc = COSINE_CHAIN_SUM(acc8);
        }

        // epilogue: scores, threshold test, survivors to this wave's slots of probe n
        const float t = thr[n];
        float sc[16];
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = COARSE ? coarse_score(acc[r], qn_lane, gn[r]) : cosine_score(acc[r], qn_lane, gn[r]);
            bool in = sbase + cosine_lane_row(w, r, h) < rows;
            if constexpr (SUBJ != SR_ROWS) in = in && gu[r] >= 0;
            if constexpr (TAG) in = in && (gt[r] & qm_lane) != 0;
            if (in && sc[r] > t) mask |= 1u << r;
        }
        const int cnt = __builtin_popcount(mask);
        const int cnt0 = __shfl(cnt, n);         // the h = 0 lane of probe n goes first
        int slot = h ? cnt0 : 0;
        float* csq = cs + (n * CT_WAVES + w) * SR_CAND;
        unsigned char* crq = cr + (n * CT_WAVES + w) * SR_CAND;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mask & (1u << r)) {
                csq[slot] = sc[r];
                crq[slot] = (unsigned char)cosine_lane_row(w, r, h);
                if constexpr (SUBJ == SR_DISTINCT) cu[(n * CT_WAVES + w) * SR_CAND + slot] = gu[r];
                ++slot;
            }
        if (h) cn[n * CT_WAVES + w] = cnt0 + cnt;
        if (!__syncthreads_or(cnt)) continue;

        // merge: rank scatter of list (cur) + candidates into list (cur ^ 1); 8 threads per probe
        if constexpr (SUBJ == SR_DISTINCT) {
            // The list holds a subject once, and its rows have smaller indices than every candidate.  A candidate is dead when a
            // listed row of its subject scores as much, or another candidate of its subject beats it; the best candidate of a
            // listed subject that scores more than the listed row kills that row (its victim).  The new list is the rank scatter
            // of what is alive: rank = the rank of the row-mode merge less the dead rows in front.
            const int q = tid >> 3, sub = tid & 7;
            const int nL = nl[q];
            int cw[CT_WAVES], m = 0;
#pragma unroll
            for (int v = 0; v < CT_WAVES; ++v) { cw[v] = cn[q * CT_WAVES + v]; m += cw[v]; }
            const float* Ls = ls0 + (size_t)(cur * CT_QT + q) * k;
            const int* Li = li0 + (size_t)(cur * CT_QT + q) * k;
            int* Lu = lu0 + (size_t)(cur * CT_QT + q) * k;
            float* Ns = ls0 + (size_t)((cur ^ 1) * CT_QT + q) * k;
            int* Ni = li0 + (size_t)((cur ^ 1) * CT_QT + q) * k;
            int* Nu = lu0 + (size_t)((cur ^ 1) * CT_QT + q) * k;
            const float* csb = cs + q * CT_WAVES * SR_CAND;
            const unsigned char* crb = cr + q * CT_WAVES * SR_CAND;
            int* cub = cu + q * CT_WAVES * SR_CAND;
            unsigned char* cvb = cv + q * CT_WAVES * SR_CAND;
            // pass 1, candidates (x = sub + 8 i, i < 16): dead or alive, and the victim; written once every thread has looked
            unsigned dead = 0;
            int alive = 0, nvic = 0;
            for (int x = sub, i = 0; x < m; x += 8, ++i) {
                int c = x, v = 0;
                while (c >= cw[v]) { c -= cw[v]; ++v; }
                const float s = csb[v * SR_CAND + c];
                const int lr = crb[v * SR_CAND + c], u = cub[v * SR_CAND + c];
                bool d = false;
                int victim = SR_NO_VICTIM;
                // without a branch in the body, so that the reads of several rounds are in flight together: one wave per SIMD
                // hides no LDS latency, and a merge costs what its dependent reads cost
#pragma unroll 8
                for (int j = 0; j < nL; ++j) {
                    const bool mine = Lu[j] == u, ge = Ls[j] >= s;
                    d |= mine & ge;
                    victim = (mine & !ge) ? j : victim;
                }
                for (int v2 = 0; v2 < CT_WAVES; ++v2)
#pragma unroll 4
                    for (int c2 = 0; c2 < cw[v2]; ++c2) {
                        const float s2 = csb[v2 * SR_CAND + c2];
                        const bool mine = cub[v2 * SR_CAND + c2] == u;
                        d |= mine & ((s2 > s) | ((s2 == s) & ((int)crb[v2 * SR_CAND + c2] < lr)));
                    }
                dead |= (unsigned)d << i;
                cvb[v * SR_CAND + c] = (unsigned char)(d ? SR_NO_VICTIM : victim);     // nobody reads cv in this pass
                alive += !d && victim == SR_NO_VICTIM;                                  // alive with a victim: one in, one out
                nvic += !d && victim != SR_NO_VICTIM;
            }
            nvic += __shfl_xor(nvic, 1);                  // victims of this probe: none, most of the time
            nvic += __shfl_xor(nvic, 2);
            nvic += __shfl_xor(nvic, 4);
            __syncthreads();
            for (int x = sub, i = 0; x < m; x += 8, ++i) {
                int c = x, v = 0;
                while (c >= cw[v]) { c -= cw[v]; ++v; }
                if (dead & (1u << i)) {                   // a dead candidate beats nothing from here on
                    cub[v * SR_CAND + c] = -1;
                    cs[q * CT_WAVES * SR_CAND + v * SR_CAND + c] = -INFINITY;
                } else if (cvb[v * SR_CAND + c] != SR_NO_VICTIM) Lu[cvb[v * SR_CAND + c]] = -1;
            }
            __syncthreads();
            // pass 2: the rank scatter of what is alive
            for (int e = sub; e < nL + m; e += 8) {
                float s;
                int ri, u, rank, lr = 0;
                if (e < nL) {
                    u = Lu[e];
                    if (u < 0) continue;
                    s = Ls[e]; ri = Li[e];
                    rank = e;
                } else {
                    int c = e - nL, v = 0;
                    while (c >= cw[v]) { c -= cw[v]; ++v; }
                    u = cub[v * SR_CAND + c];
                    if (u < 0) continue;
                    s = csb[v * SR_CAND + c];
                    lr = crb[v * SR_CAND + c];
                    ri = sbase + lr;
                    int lo = 0, hi = nL;    // listed rows with a score >= s beat it (smaller index): binary search
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (Ls[mid] >= s) lo = mid + 1; else hi = mid;
                    }
                    rank = lo;
                }
                const int before = rank;    // the listed rows in front, dead ones included
                if (e < nL) lr = -1;        // a listed row loses no tie to a candidate
                for (int v2 = 0; v2 < CT_WAVES; ++v2)
#pragma unroll 4
                    for (int c2 = 0; c2 < cw[v2]; ++c2) {
                        const float s2 = csb[v2 * SR_CAND + c2];
                        rank += (s2 > s) | ((s2 == s) & ((int)crb[v2 * SR_CAND + c2] < lr));
                    }
                if (nvic)
                    for (int v2 = 0; v2 < CT_WAVES; ++v2)
                        for (int c2 = 0; c2 < cw[v2]; ++c2) rank -= (int)cvb[v2 * SR_CAND + c2] < before;
                if (rank < k) { Ns[rank] = s; Ni[rank] = ri; Nu[rank] = u; }
            }
            alive += __shfl_xor(alive, 1);
            alive += __shfl_xor(alive, 2);
            alive += __shfl_xor(alive, 4);
            __syncthreads();
            if (sub == 0) {
                const int nn = min(k, nL + alive);
                nl[q] = nn;
                if (q < nq && nn == k) thr[q] = Ns[k - 1];
            }
            cur ^= 1;
            __syncthreads();
        } else {
            const int q = tid >> 3, sub = tid & 7;
            const int nL = nl[q];
            int cw[CT_WAVES], m = 0;
#pragma unroll
            for (int v = 0; v < CT_WAVES; ++v) { cw[v] = cn[q * CT_WAVES + v]; m += cw[v]; }
            const float* Ls = ls0 + (size_t)(cur * CT_QT + q) * k;
            const int* Li = li0 + (size_t)(cur * CT_QT + q) * k;
            float* Ns = ls0 + (size_t)((cur ^ 1) * CT_QT + q) * k;
            int* Ni = li0 + (size_t)((cur ^ 1) * CT_QT + q) * k;
            const float* csb = cs + q * CT_WAVES * SR_CAND;
            const unsigned char* crb = cr + q * CT_WAVES * SR_CAND;
            for (int e = sub; e < nL + m; e += 8) {
                float s;
                int ri, rank;
                if (e < nL) {               // a listed row: beaten only by candidates with a strictly greater score
                    s = Ls[e];
                    ri = Li[e];
                    rank = e;
                    for (int v = 0; v < CT_WAVES; ++v)
                        for (int c = 0; c < cw[v]; ++c) rank += csb[v * SR_CAND + c] > s;
                } else {
                    int c = e - nL, v = 0;
                    while (c >= cw[v]) { c -= cw[v]; ++v; }
                    s = csb[v * SR_CAND + c];
                    const int lr = crb[v * SR_CAND + c];
                    ri = sbase + lr;
                    int lo = 0, hi = nL;    // listed rows with a score >= s beat it (smaller index): binary search
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (Ls[mid] >= s) lo = mid + 1; else hi = mid;
                    }
                    rank = lo;
                    for (int v2 = 0; v2 < CT_WAVES; ++v2)
                        for (int c2 = 0; c2 < cw[v2]; ++c2) {
                            const float s2 = csb[v2 * SR_CAND + c2];
                            rank += s2 > s || (s2 == s && (int)crb[v2 * SR_CAND + c2] < lr);
                        }
                }
                if (rank < k) { Ns[rank] = s; Ni[rank] = ri; }
            }
            __syncthreads();
            if (sub == 0) {
                const int nn = min(k, nL + m);
                nl[q] = nn;
                if (q < nq && nn == k) thr[q] = Ns[k - 1];
            }
            cur ^= 1;
            __syncthreads();
        }
    }

    // one sorted list per (chunk, probe); empty slots are (-inf, -1), and -1 for the subject
    const float* Ls = ls0 + (size_t)cur * CT_QT * k;
    const int* Li = li0 + (size_t)cur * CT_QT * k;
    const long long ib = a.index_base + c0;
    for (int e = tid; e < nq * k; e += 256) {
        const int q = e / k, p = e - q * k;
        const bool ok = p < nl[q];
        const size_t o = ((size_t)chunk * a.Q + q0 + q) * k + p;
        a.out_s[o] = ok ? Ls[q * k + p] : -INFINITY;
        a.out_i[o] = ok ? ib + Li[q * k + p] : (int64_t)-1;
        if constexpr (OUT_U && SUBJ == SR_LIVE) a.out_u[o] = ok ? sch[(unsigned)Li[q * k + p]] : -1;
        if constexpr (OUT_U && SUBJ == SR_DISTINCT) a.out_u[o] = ok ? lu0[(size_t)cur * CT_QT * k + q * k + p] : -1;
    }
}

}  // namespace ffr
