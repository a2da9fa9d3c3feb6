// search.hip -- 1:N identification: exact cosine top-k of Q probes over a gallery of G enrolled 512-d embeddings
// (include/ffrnet.h, ffr_row_norms / ffr_search_topk / ffr_topk_merge).  Score = lfw/lfw_eval.py:246:
// dot(q, g) / (|q| |g| + 1e-8), the formula of k_cosine; order = descending score, ties by ascending index.
//
// k_row_norms    |x| of [n][512] rows, one wave per row, the lane-strided sum of squares of k_cosine.
// k_search_topk  the hot path.  A block (4 waves) holds a tile of 32 probes in LDS and walks one contiguous chunk of the
//                gallery, 128 rows per step (32 per wave):
//  - K loop: a wave computes the 32 x 32 tile D[g][q] = sum_k G[g][k] Q[q][k] with v_mfma_f32_32x32x2_f32, operands
//    straight from global memory / LDS without a repack.  Lane (n = l & 31, h = l >> 5) does ONE 16-byte load of
//    g[n][8j + 4h .. 8j + 4h + 3] per group j (64 groups over K = 512) and uses element i as its k-value in the i-th of
//    four MFMAs; the probe operand comes from LDS in the same permutation (fragment order [j][lane], written once per
//    block).  Group j accumulates into chain j % 8 (8 accumulators: 64 k-values per fp32 chain instead of 512, which
//    keeps strongly correlated embeddings within 1e-6 of the float64 cosine), and the chains are added in a fixed tree.
//    So every (q, g) score is the same fp32 arithmetic wherever it sits in a tile, a block or a shard: results are
//    bitwise independent of Q, of the chunking and of the sharding.  32 groups (128 VGPRs) of the gallery
//    operand are in flight ahead of the MFMAs, across the tile boundary: one wave per SIMD keeps the pipe fed.
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

#include "ffr_kernels.h"

namespace ffr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SR_DIM = 512;
constexpr int SR_QT = 32;                 // probes per block
constexpr int SR_WAVES = 4;
constexpr int SR_STEP = 32 * SR_WAVES;    // gallery rows per block step
constexpr int SR_NG = SR_DIM / 8;         // 16-byte groups per lane and row half: 64
constexpr int SR_PF = 16;                 // groups of the gallery operand in flight (4 k cycles of MFMA ahead)
constexpr int SR_CAND = 32;               // candidate slots per (probe, wave) and step
constexpr int SR_NACC = 8;                // accumulators per tile: group j feeds chain j % 8 (64 k-values per chain)
constexpr long long SR_MAX_CHUNK = 1 << 20;   // rows: 2^29 floats, a 32-bit element offset
constexpr int MG_LDS_CAP = 64 * 1024;

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_row_norms(const float* __restrict__ x, long long n, float* __restrict__ norms) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = x + row * SR_DIM;
    float aa = 0.f;
    for (int c = lane; c < SR_DIM; c += 64) {
        const float v = p[c];
        aa += v * v;
    }
    aa = wave_sum64(aa);
    if (lane == 0) norms[row] = sqrtf(aa);
}

struct SearchArgs {
    const float* query;       // [Q][512]
    const float* qnorm;       // [Q]
    const float* gallery;     // [G][512]
    const float* gnorm;       // [G]
    long long G;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), <= SR_MAX_CHUNK
    long long index_base;
    float* out_s;             // [S][Q][k]
    int64_t* out_i;
    int Q, k, nchunks, ntiles;
};

// LDS: probe fragments [64][64] f32x4 | candidates cs[32][4][32] f32, cr[32][4][32] u8, cn[32][4] | thr[32], nl[32] |
// two lists [32][k] of (score, chunk row)
constexpr size_t SR_OFF_CS = (size_t)SR_NG * 64 * 16;
constexpr size_t SR_OFF_CR = SR_OFF_CS + SR_QT * SR_WAVES * SR_CAND * 4;
constexpr size_t SR_OFF_CN = SR_OFF_CR + SR_QT * SR_WAVES * SR_CAND;
constexpr size_t SR_OFF_THR = SR_OFF_CN + SR_QT * SR_WAVES * 4;
constexpr size_t SR_OFF_NL = SR_OFF_THR + SR_QT * 4;
constexpr size_t SR_OFF_LIST = SR_OFF_NL + SR_QT * 4;
__host__ __device__ constexpr size_t sr_lds_bytes(int k) { return SR_OFF_LIST + 2 * (size_t)SR_QT * k * 8; }

__global__ __launch_bounds__(256, 1) void k_search_topk(const SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    f32x4* qf = (f32x4*)sm;
    float* cs = (float*)(sm + SR_OFF_CS);
    unsigned char* cr = sm + SR_OFF_CR;
    int* cn = (int*)(sm + SR_OFF_CN);
    float* thr = (float*)(sm + SR_OFF_THR);
    int* nl = (int*)(sm + SR_OFF_NL);
    float* ls0 = (float*)(sm + SR_OFF_LIST);              // list buffer b: scores at ls0 + b*QT*k, rows at li0 + b*QT*k
    int* li0 = (int*)(ls0 + 2 * SR_QT * a.k);

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k;

    // XCD-grouped logical block id (bijective for any grid): the probe tiles of one chunk run on one XCD
    const int nb = gridDim.x, b = blockIdx.x, xcd = b & 7, loc = b >> 3, qq = nb >> 3, rr = nb & 7;
    const int lid = xcd < rr ? xcd * (qq + 1) + loc : rr * (qq + 1) + (xcd - rr) * qq + loc;
    const int chunk = lid / a.ntiles, tile = lid - chunk * a.ntiles;
    const long long c0 = (long long)chunk * a.chunk_rows;
    const long long rem = a.G - c0;
    const int rows = (int)(rem < a.chunk_rows ? rem : a.chunk_rows);    // >= 1
    const int q0 = tile * SR_QT;
    const int nq = min(SR_QT, a.Q - q0);

    // probe tile in fragment order: qf[j*64 + l] = q[q0 + (l&31)][8j + 4(l>>5) .. +3]
    for (int e = tid; e < SR_NG * 64; e += 256) {
        const int j = e >> 6, l = e & 63, qn = l & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qn < nq) v = *(const f32x4*)(a.query + (size_t)(q0 + qn) * SR_DIM + 8 * j + 4 * (l >> 5));
        qf[e] = v;
    }
    if (tid < SR_QT) {
        thr[tid] = tid < nq ? -INFINITY : INFINITY;    // probes past Q never take a candidate
        nl[tid] = 0;
    }
    const float qn_lane = n < nq ? a.qnorm[q0 + n] : 0.f;

    // 64-bit chunk base, 32-bit element offsets inside it
    const float* __restrict__ gch = a.gallery + (size_t)c0 * SR_DIM;
    const float* __restrict__ nch = a.gnorm + c0;
    const unsigned lane_off = 4u * h;
    int row = min(w * 32 + n, rows - 1);
    f32x4 pf[SR_PF];
#pragma unroll
    for (int u = 0; u < SR_PF; ++u) pf[u] = *(const f32x4*)(gch + ((unsigned)row * SR_DIM + 8u * u + lane_off));
    __syncthreads();

    int cur = 0;
    const int nsteps = (rows + SR_STEP - 1) / SR_STEP;
    for (int step = 0; step < nsteps; ++step) {
        const int sbase = step * SR_STEP;
        const int next = min(row + SR_STEP, rows - 1);
        // gallery norms of the 16 rows this lane scores, fetched ahead of the K loop
        float gn[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gr = min(sbase + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, rows - 1);
            gn[r] = nch[(unsigned)gr];
        }
        f32x16 acc8[SR_NACC];
#pragma unroll
        for (int u = 0; u < SR_NACC; ++u) acc8[u] = f32x16{};
        f32x4 bq = qf[lane];
#pragma unroll
        for (int j = 0; j < SR_NG; ++j) {
            const f32x4 av = pf[j % SR_PF];
            const int jn = j + SR_PF;          // refill the slot: this tile's group jn, or the next tile's group jn - 64
            if (jn < SR_NG) pf[j % SR_PF] = *(const f32x4*)(gch + ((unsigned)row * SR_DIM + 8u * jn + lane_off));
            else pf[j % SR_PF] = *(const f32x4*)(gch + ((unsigned)next * SR_DIM + 8u * (jn - SR_NG) + lane_off));
            const f32x4 bv = bq;
            if (j + 1 < SR_NG) bq = qf[(j + 1) * 64 + lane];
            f32x16& acc = acc8[j % SR_NACC];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);     // keep each refill SR_PF groups ahead of its use (hipcc sinks it otherwise)
        }
        row = next;
        // the 8 partial chains in a fixed tree
        const f32x16 acc = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));

        // epilogue: scores, threshold test, survivors to this wave's slots of probe n
        const float t = thr[n];
        float sc[16];
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;        // row within the step
            sc[r] = acc[r] / (qn_lane * gn[r] + 1e-8f);
            if (sbase + lr < rows && sc[r] > t) mask |= 1u << r;
        }
        const int cnt = __builtin_popcount(mask);
        const int cnt0 = __shfl(cnt, n);         // the h = 0 lane of probe n goes first
        int slot = h ? cnt0 : 0;
        float* csq = cs + (n * SR_WAVES + w) * SR_CAND;
        unsigned char* crq = cr + (n * SR_WAVES + w) * SR_CAND;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mask & (1u << r)) {
                csq[slot] = sc[r];
                crq[slot] = (unsigned char)(w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
                ++slot;
            }
        if (h) cn[n * SR_WAVES + w] = cnt0 + cnt;
        if (!__syncthreads_or(cnt)) continue;

        // merge: rank scatter of list (cur) + candidates into list (cur ^ 1); 8 threads per probe
        {
            const int q = tid >> 3, sub = tid & 7;
            const int nL = nl[q];
            int cw[SR_WAVES], m = 0;
#pragma unroll
            for (int v = 0; v < SR_WAVES; ++v) { cw[v] = cn[q * SR_WAVES + v]; m += cw[v]; }
            const float* Ls = ls0 + (size_t)(cur * SR_QT + q) * k;
            const int* Li = li0 + (size_t)(cur * SR_QT + q) * k;
            float* Ns = ls0 + (size_t)((cur ^ 1) * SR_QT + q) * k;
            int* Ni = li0 + (size_t)((cur ^ 1) * SR_QT + q) * k;
            const float* csb = cs + q * SR_WAVES * SR_CAND;
            const unsigned char* crb = cr + q * SR_WAVES * SR_CAND;
            for (int e = sub; e < nL + m; e += 8) {
                float s;
                int ri, rank;
                if (e < nL) {               // a listed row: beaten only by candidates with a strictly greater score
                    s = Ls[e];
                    ri = Li[e];
                    rank = e;
                    for (int v = 0; v < SR_WAVES; ++v)
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
                    for (int v2 = 0; v2 < SR_WAVES; ++v2)
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
    const float* Ls = ls0 + (size_t)cur * SR_QT * k;
    const int* Li = li0 + (size_t)cur * SR_QT * k;
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

long long search_max_chunk_rows() { return SR_MAX_CHUNK; }

hipError_t launch_row_norms(const float* x, long long n, float* norms, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, x, n, norms);
    return hipGetLastError();
}

void search_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    const int T = (Q + SR_QT - 1) / SR_QT;
    long long S = (num_cus + T - 1) / T;                             // chunks x tiles fill the CUs, also at Q = 1
    S = std::max(S, (G + SR_MAX_CHUNK - 1) / SR_MAX_CHUNK);
    S = std::max(1LL, std::min(S, (G + SR_STEP - 1) / SR_STEP));       // at least one step of rows per chunk
    long long cr = (G + S - 1) / S;
    cr = std::min(SR_MAX_CHUNK, (cr + SR_STEP - 1) / SR_STEP * SR_STEP);
    *ntiles = T;
    *nchunks = (int)((G + cr - 1) / cr);
    *chunk_rows = cr;
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
