// search.hip -- 1:N identification: exact cosine top-k of Q probes over a gallery of G enrolled 512-d embeddings
// (include/ffrnet.h, ffr_row_norms / ffr_search_topk / ffr_topk_merge).  Score = lfw/lfw_eval.py:246:
// dot(q, g) / (|q| |g| + 1e-8), the formula of k_cosine; order = descending score, ties by ascending index.
//
// k_row_norms    |x| of [n][512] rows, one wave per row, the lane-strided sum of squares of k_cosine.
// k_search_topk  the hot path: the exact instantiation of the search block of search_core.h, which describes it (the
//                bf16 instantiation is k_search_coarse, search_coarse.hip).
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
#include "search_core.h"

namespace ffr {

namespace {

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

__global__ __launch_bounds__(256, 1) void k_search_topk(const SearchArgs a) { search_block<false>(a); }

// (score, index) keys of the merge: padding (index < 0) sorts after everything
__device__ __forceinline__ bool mg_beats(float s1, long long i1, int l1, float s2, long long i2, int l2) {
    if (s1 != s2) return s1 > s2;
    if (i1 != i2) return i1 < i2;
    return l1 < l2;
}

__global__ __launch_bounds__(64) void k_topk_merge(const float* __restrict__ score, const int64_t* __restrict__ index, int S,
                                                   int Q, int k, int staged, float* __restrict__ out_s,
                                                   int64_t* __restrict__ out_i, const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (live && q >= *live) return;                       // a probe that was not searched: no lists, nothing to write
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
                              float* out_s, int64_t* out_i, hipStream_t stream, const int* live) {
    SearchArgs a{query, qnorm, gallery, nullptr, gnorm, G, chunk_rows, index_base, out_s, out_i, live, Q, k, nchunks, ntiles};
    const size_t lds = sr_lds_bytes(k);
    hipError_t e = hipFuncSetAttribute((const void*)k_search_topk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_search_topk, dim3((unsigned)(nchunks * ntiles)), dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const float* score, const int64_t* index, int S, int Q, int k, float* out_s, int64_t* out_i,
                             hipStream_t stream, const int* live) {
    const size_t head = ((size_t)S * 4 + 15) & ~(size_t)15;
    const size_t full = head + (size_t)S * k * 12;
    const int staged = S > 0 && full <= (size_t)MG_LDS_CAP;
    const size_t lds = staged ? full : head;
    hipError_t e = hipFuncSetAttribute((const void*)k_topk_merge, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MG_LDS_CAP);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)Q), dim3(64), lds, stream, score, index, S, Q, k, staged, out_s, out_i, live);
    return hipGetLastError();
}

}  // namespace ffr
