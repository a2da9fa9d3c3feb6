// search.hip -- 1:N identification: exact cosine top-k of Q probes over a gallery of G enrolled 512-d embeddings
// (include/ffrnet.h, ffr_row_norms / ffr_search_topk / ffr_topk_merge).  Score = lfw/lfw_eval.py:246:
// dot(q, g) / (|q| |g| + 1e-8), the formula of k_cosine; order = descending score, ties by ascending index.
//
// k_row_norms    |x| of [n][512] rows, one wave per row, the lane-strided sum of squares of k_cosine.
// k_search_topk  the hot path.  A block (4 waves) holds a tile of 32 probes in LDS and walks one contiguous chunk of the
//                gallery, 128 rows per step (32 per wave):
//  - K loop: the 32 x 128 cosine tile of cosine_tile.h.  Every (q, g) score is the same fp32 arithmetic wherever it sits in a
//    tile, a block or a shard: results are bitwise independent of Q, of the chunking and of the sharding.
//  - Epilogue, outside the K loop: lane (n, h) holds the 16 scores of probe n against gallery rows (r&3) + 8(r>>2) + 4h;
//    each is compared with the probe's current k-th score (LDS).  Rows of a step have larger indices than every listed
//    row, so a row enters iff its score is strictly greater (or the list is not full yet).  Survivors go to a per
//    (probe, wave) LDS slot array; once the lists fill, most steps have none and skip the merge (one __syncthreads_or).
//  - Merge (rare): the new list is the rank scatter of list + candidates -- rank = number of elements that beat it under
//    the total order -- into the second LDS list buffer.  The top k of a set under a total order is unique, so the list
//    is the same whatever order the candidates arrive in: no atomics, no ordering between waves needed.
//  - Each block writes one sorted list per (chunk, probe); k_topk_merge folds the chunk lists.
//  - Addressing: a block's chunk is a 64-bit base pointer plus 32-bit element offsets inside it (<= 2^20 rows =
//    2^29 floats per chunk), so galleries beyond 2 GiB / 4 GiB work; rows past the chunk's end are clamped to its last
//    row (in bounds) and never become candidates.
//  - Grid: chunks x probe tiles >= the CU count (also at Q = 1: 256 chunks of a 2^20-row gallery); block b runs on XCD
//    b % 8, and the bijective remap gives each XCD a contiguous run of logical blocks, chunk-major, so the probe tiles
//    of one chunk share that XCD's L2 and the chunk comes from HBM about once.
// k_topk_merge   S sorted lists per probe -> one: one wave per probe, a k-step tournament over the list heads (wave
//                argmax with the total order, lane as the last tie-break); the lists are staged in LDS when they fit.
//                Slots with index < 0 are padding (-inf, -1) and sort after every real entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>

#include "cosine_tile.h"
#include "device_util.h"
#include "ffr_kernels.h"

namespace ffr {

namespace {

constexpr int SR_CAND = 32;               // candidate slots per (probe, wave) and step
constexpr int MG_LDS_CAP = 64 * 1024;

__global__ __launch_bounds__(256) void k_row_norms(const float* __restrict__ x, long long n, float* __restrict__ norms) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = x + row * CT_DIM;
    float aa = 0.f;
    for (int c = lane; c < CT_DIM; c += 64) {
        const float v = p[c];
        aa += v * v;
    }
    aa = wave_sum(aa);
    if (lane == 0) norms[row] = sqrtf(aa);
}

struct SearchArgs {
    const float* query;       // [Q][512]
    const float* qnorm;       // [Q]
    const float* gallery;     // [G][512]
    const float* gnorm;       // [G]
    long long G;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), <= CT_MAX_CHUNK
    long long index_base;
    float* out_s;             // [S][Q][k]
    int64_t* out_i;
    int Q, k, nchunks, ntiles;
};

// LDS: probe fragments [64][64] f32x4 | candidates cs[32][4][32] f32, cr[32][4][32] u8, cn[32][4] | thr[32], nl[32] |
// two lists [32][k] of (score, chunk row)
constexpr size_t SR_OFF_CS = (size_t)CT_NG * 64 * 16;
constexpr size_t SR_OFF_CR = SR_OFF_CS + CT_QT * CT_WAVES * SR_CAND * 4;
constexpr size_t SR_OFF_CN = SR_OFF_CR + CT_QT * CT_WAVES * SR_CAND;
constexpr size_t SR_OFF_THR = SR_OFF_CN + CT_QT * CT_WAVES * 4;
constexpr size_t SR_OFF_NL = SR_OFF_THR + CT_QT * 4;
constexpr size_t SR_OFF_LIST = SR_OFF_NL + CT_QT * 4;
__host__ __device__ constexpr size_t sr_lds_bytes(int k) { return SR_OFF_LIST + 2 * (size_t)CT_QT * k * 8; }

__global__ __launch_bounds__(256, 1) void k_search_topk(const SearchArgs a) {
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
    const long long c0 = (long long)chunk * a.chunk_rows;
    const long long rem = a.G - c0;
    const int rows = (int)(rem < a.chunk_rows ? rem : a.chunk_rows);    // >= 1
    const int q0 = tile * CT_QT;
    const int nq = min(CT_QT, a.Q - q0);

    cosine_fill_probes(qf, a.query, q0, nq, tid);
    if (tid < CT_QT) {
        thr[tid] = tid < nq ? -INFINITY : INFINITY;    // probes past Q never take a candidate
        nl[tid] = 0;
    }
    const float qn_lane = n < nq ? a.qnorm[q0 + n] : 0.f;

    const float* __restrict__ nch = a.gnorm + c0;
    CosineStream gs(a.gallery + (size_t)c0 * CT_DIM, lane);
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
        f32x16 acc8[CT_NACC];
        gs.tile(acc8, qf, next);
        const f32x16 acc = COSINE_CHAIN_SUM(acc8);

        // epilogue: scores, threshold test, survivors to this wave's slots of probe n
        const float t = thr[n];
        float sc[16];
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = cosine_score(acc[r], qn_lane, gn[r]);
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

// (score, index) keys of the merge: padding (index < 0) sorts after everything
__device__ __forceinline__ bool mg_beats(float s1, long long i1, int l1, float s2, long long i2, int l2) {
    if (s1 != s2) return s1 > s2;
    if (i1 != i2) return i1 < i2;
    return l1 < l2;
}

__global__ __launch_bounds__(64) void k_topk_merge(const float* __restrict__ score, const int64_t* __restrict__ index, int S,
                                                   int Q, int k, int staged, float* __restrict__ out_s,
                                                   int64_t* __restrict__ out_i) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int q = blockIdx.x, lane = threadIdx.x;
    int* hp = (int*)sm;                                   // head position of each list
    const float* ps;
    const int64_t* pi;
    long long stride;                                     // elements between two lists
    if (staged) {
        int64_t* si = (int64_t*)(sm + (((size_t)S * 4 + 15) & ~(size_t)15));
        float* ss = (float*)(si + (size_t)S * k);
        for (int e = lane; e < S * k; e += 64) {
            const int l = e / k, p = e - l * k;
            const size_t o = ((size_t)l * Q + q) * k + p;
            ss[e] = score[o];
            si[e] = index[o];
        }
        ps = ss; pi = si; stride = k;
    } else {
        ps = score + (size_t)q * k; pi = index + (size_t)q * k; stride = (long long)Q * k;
    }
    for (int l = lane; l < S; l += 64) hp[l] = 0;
    __syncthreads();
    auto head = [&](int l, float& s, long long& i) {
        const int p = hp[l];
        if (p >= k) { s = -INFINITY; i = LLONG_MAX; return; }
        s = ps[l * stride + p];
        i = pi[l * stride + p];
        if (i < 0) { s = -INFINITY; i = LLONG_MAX; }
    };
    auto lane_best = [&](float& bs, long long& bi, int& bl) {
        bs = -INFINITY; bi = LLONG_MAX; bl = INT_MAX;
        for (int l = lane; l < S; l += 64) {
            float s; long long i;
            head(l, s, i);
            if (mg_beats(s, i, l, bs, bi, bl)) { bs = s; bi = i; bl = l; }
        }
    };
    float bs; long long bi; int bl;
    lane_best(bs, bi, bl);
    for (int p = 0; p < k; ++p) {
        float ws = bs; long long wi = bi; int wl = bl;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float s2 = __shfl_xor(ws, o);
            const long long i2 = __shfl_xor(wi, o);
            const int l2 = __shfl_xor(wl, o);
            if (mg_beats(s2, i2, l2, ws, wi, wl)) { ws = s2; wi = i2; wl = l2; }
        }
        const bool pad = wi == LLONG_MAX;
        if (lane == 0) {
            out_s[(size_t)q * k + p] = pad ? -INFINITY : ws;
            out_i[(size_t)q * k + p] = pad ? (int64_t)-1 : (int64_t)wi;
        }
        if (pad) {                                        // every list is exhausted: the rest is padding
            for (int r = p + 1 + lane; r < k; r += 64) { out_s[(size_t)q * k + r] = -INFINITY; out_i[(size_t)q * k + r] = -1; }
            break;
        }
        if (wl < S && (wl & 63) == lane) {                // the lane that owns the winning list advances it
            hp[wl] += 1;
            lane_best(bs, bi, bl);
        }
    }
}

}  // namespace

long long search_max_chunk_rows() { return CT_MAX_CHUNK; }

hipError_t launch_row_norms(const float* x, long long n, float* norms, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, x, n, norms);
    return hipGetLastError();
}

void search_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    *ntiles = (Q + CT_QT - 1) / CT_QT;
    cosine_chunks(*ntiles, G, 1, num_cus, nchunks, chunk_rows);      // chunks x tiles fill the CUs, also at Q = 1
}

hipError_t launch_search_topk(const float* query, const float* qnorm, int Q, const float* gallery, const float* gnorm,
                              long long G, int k, long long index_base, int ntiles, int nchunks, long long chunk_rows,
                              float* out_s, int64_t* out_i, hipStream_t stream) {
    SearchArgs a{query, qnorm, gallery, gnorm, G, chunk_rows, index_base, out_s, out_i, Q, k, nchunks, ntiles};
    const size_t lds = sr_lds_bytes(k);
    hipError_t e = hipFuncSetAttribute((const void*)k_search_topk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_search_topk, dim3((unsigned)(nchunks * ntiles)), dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const float* score, const int64_t* index, int S, int Q, int k, float* out_s, int64_t* out_i,
                             hipStream_t stream) {
    const size_t head = ((size_t)S * 4 + 15) & ~(size_t)15;
    const size_t full = head + (size_t)S * k * 12;
    const int staged = S > 0 && full <= (size_t)MG_LDS_CAP;
    const size_t lds = staged ? full : head;
    hipError_t e = hipFuncSetAttribute((const void*)k_topk_merge, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MG_LDS_CAP);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)Q), dim3(64), lds, stream, score, index, S, Q, k, staged, out_s, out_i);
    return hipGetLastError();
}

}  // namespace ffr
