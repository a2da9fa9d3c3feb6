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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coarse_tile.h"
#include "cosine_tile.h"
#include "device_util.h"

namespace ffr {

constexpr int SR_CAND = 32;               // candidate slots per (probe, wave) and step

struct SearchArgs {
    const float* query;       // [Q][512]
    const float* qnorm;       // [Q]
    const float* gallery;     // [G][512] (the exact tile)
    const uint16_t* plane;    // [G][512] bf16 of the normalised rows (the coarse tile)
    const float* gnorm;       // [G]
    long long G;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), <= CT_MAX_CHUNK
    long long index_base;
    float* out_s;             // [S][Q][k]
    int64_t* out_i;
    const int* live;          // device, or null: the probes [*live, Q) are not searched (their tiles leave at once)
    int Q, k, nchunks, ntiles;
};

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
__host__ __device__ constexpr size_t sr_lds_bytes(int k) { return SR_OFF_LIST + 2 * (size_t)CT_QT * k * 8; }

// One block of a search: k_search_topk (search.hip) is the exact instantiation, k_search_coarse (search_coarse.hip) the
// bf16 one.  They differ in the tile alone; the threshold test, the survivor slots and the rank-scatter merge are this text.
template <bool COARSE>
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

    const float* __restrict__ nch = a.gnorm + c0;
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
            if (sbase + cosine_lane_row(w, r, h) < rows && sc[r] > t) mask |= 1u << r;
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
                ++slot;
            }
        if (h) cn[n * CT_WAVES + w] = cnt0 + cnt;
        if (!__syncthreads_or(cnt)) continue;

        // merge: rank scatter of list (cur) + candidates into list (cur ^ 1); 8 threads per probe
        {
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

    // one sorted list per (chunk, probe); empty slots are (-inf, -1)
    const float* Ls = ls0 + (size_t)cur * CT_QT * k;
    const int* Li = li0 + (size_t)cur * CT_QT * k;
    const long long ib = a.index_base + c0;
    for (int e = tid; e < nq * k; e += 256) {
        const int q = e / k, p = e - q * k;
        const bool ok = p < nl[q];
        const size_t o = ((size_t)chunk * a.Q + q0 + q) * k + p;
        a.out_s[o] = ok ? Ls[q * k + p] : -INFINITY;
        a.out_i[o] = ok ? ib + Li[q * k + p] : (int64_t)-1;
    }
}

}  // namespace ffr
