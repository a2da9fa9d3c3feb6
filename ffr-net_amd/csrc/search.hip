// search.hip -- 1:N identification: exact cosine top-k of Q probes over a gallery of G enrolled 512-d embeddings
// (include/ffrnet.h, ffr_row_norms / ffr_search_topk / ffr_topk_merge).  Score = lfw/lfw_eval.py:246:
// dot(q, g) / (|q| |g| + 1e-8), the formula of k_cosine; order = descending score, ties by ascending index.
//
// k_row_norms    |x| of [n][512] rows, one wave per row, the lane-strided sum of squares of k_cosine.
// k_search_topk  the hot path: the exact instantiation of the search block of search_core.h, which describes it (the
//                bf16 instantiation is k_search_coarse, search_coarse.hip).
// k_search_subjects  the same block with a subject policy (ffr_search_topk_subjects): SR_LIVE ranks the rows that were not
//                removed, SR_DISTINCT ranks subjects, each by its best row.
// k_search_filtered  the same block, with each of the three policies, under a per-probe filter (ffr_search_topk_filtered): a
//                row is a candidate of a probe iff its tag word and the probe's mask word share a bit.
// k_topk_merge   S sorted lists per probe -> one: one wave per probe, a k-step tournament over the list heads (wave
//                argmax with the total order, lane as the last tie-break); the lists are staged in LDS when they fit.
//                Slots with index < 0 are padding (-inf, -1) and sort after every real entry.
// k_topk_merge_subjects  the same tournament with a subject per entry; in identity mode a winner whose subject was emitted
//                before is dropped (lane p keeps the p-th emitted subject: one wave-wide compare), until k subjects are out.
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
template <int SUBJ> __global__ __launch_bounds__(256, 1) void k_search_subjects(const SearchArgs a) { search_block<false, SUBJ>(a); }
template <int SUBJ> __global__ __launch_bounds__(256, 1) void k_search_filtered(const SearchArgs a) {
    search_block<false, SUBJ, SUBJ != SR_ROWS, true>(a);
}

// (score, index) keys of the merge: padding (index < 0) sorts after everything
__device__ __forceinline__ bool mg_beats(float s1, long long i1, int l1, float s2, long long i2, int l2) {
    if (s1 != s2) return s1 > s2;
    if (i1 != i2) return i1 < i2;
    return l1 < l2;
}

// The merge of one probe's lists by one wave.  SUBJ: entries carry a subject (staged entries are 16 bytes, not 12), and with
// `distinct` a popped winner is dropped when its subject is out already (k <= 64: lane p holds the p-th emitted subject).
template <bool SUBJ>
__device__ __forceinline__ void topk_merge_wave(const float* __restrict__ score, const int64_t* __restrict__ index,
                                                const int32_t* __restrict__ subject, int S, int Q, int k, int staged, int distinct,
                                                float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                int32_t* __restrict__ out_u, const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (live && q >= *live) return;                       // a probe that was not searched: no lists, nothing to write
    int* hp = (int*)sm;                                   // head position of each list
    const float* ps;
    const int64_t* pi;
    const int32_t* pu = nullptr;
    long long stride;                                     // elements between two lists
    if (staged) {
        int64_t* si = (int64_t*)(sm + (((size_t)S * 4 + 15) & ~(size_t)15));
        float* ss = (float*)(si + (size_t)S * k);
        int32_t* su = (int32_t*)(ss + (size_t)S * k);
        for (int e = lane; e < S * k; e += 64) {
            const int l = e / k, p = e - l * k;
            const size_t o = ((size_t)l * Q + q) * k + p;
            ss[e] = score[o];
            si[e] = index[o];
            if constexpr (SUBJ) su[e] = subject[o];
        }
        ps = ss; pi = si; stride = k;
        if constexpr (SUBJ) pu = su;
    } else {
        ps = score + (size_t)q * k; pi = index + (size_t)q * k; stride = (long long)Q * k;
        if constexpr (SUBJ) pu = subject + (size_t)q * k;
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
    int p = 0, mine = -1;                                 // p entries are out; mine: the subject entry `lane` went out with
    while (p < k) {
        float ws = bs; long long wi = bi; int wl = bl;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float s2 = __shfl_xor(ws, o);
            const long long i2 = __shfl_xor(wi, o);
            const int l2 = __shfl_xor(wl, o);
            if (mg_beats(s2, i2, l2, ws, wi, wl)) { ws = s2; wi = i2; wl = l2; }
        }
        if (wi == LLONG_MAX) break;                       // every list is exhausted: the rest is padding
        bool out = true;
        int wu = 0;
        if constexpr (SUBJ) {
            wu = pu[wl * stride + hp[wl]];
            if (distinct) out = !__any(lane < p && mine == wu);
        }
        if (out) {
            if (lane == 0) {
                out_s[(size_t)q * k + p] = ws;
                out_i[(size_t)q * k + p] = (int64_t)wi;
                if constexpr (SUBJ) out_u[(size_t)q * k + p] = wu;
            }
            if (lane == p) mine = wu;
            ++p;
        }
        if ((wl & 63) == lane) {                          // the lane that owns the winning list advances it
            hp[wl] += 1;
            lane_best(bs, bi, bl);
        }
    }
    for (int r = p + lane; r < k; r += 64) {
        out_s[(size_t)q * k + r] = -INFINITY;
        out_i[(size_t)q * k + r] = -1;
        if constexpr (SUBJ) out_u[(size_t)q * k + r] = -1;
    }
}

__global__ __launch_bounds__(64) void k_topk_merge(const float* __restrict__ score, const int64_t* __restrict__ index, int S,
                                                   int Q, int k, int staged, float* __restrict__ out_s,
                                                   int64_t* __restrict__ out_i, const int* __restrict__ live) {
    topk_merge_wave<false>(score, index, nullptr, S, Q, k, staged, 0, out_s, out_i, nullptr, live);
}

__global__ __launch_bounds__(64) void k_topk_merge_subjects(const float* __restrict__ score, const int64_t* __restrict__ index,
                                                            const int32_t* __restrict__ subject, int S, int Q, int k, int staged,
                                                            int distinct, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                            int32_t* __restrict__ out_u, const int* __restrict__ live) {
    topk_merge_wave<true>(score, index, subject, S, Q, k, staged, distinct, out_s, out_i, out_u, live);
}

}  // namespace

long long search_max_chunk_rows() { return CT_MAX_CHUNK; }
int search_max_k_distinct() { return SR_MAX_K_DISTINCT; }

hipError_t launch_row_norms(const float* x, long long n, float* norms, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, x, n, norms);
    return hipGetLastError();
}

void search_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    *ntiles = (Q + CT_QT - 1) / CT_QT;
    cosine_chunks(*ntiles, G, 1, num_cus, nchunks, chunk_rows);      // chunks x tiles fill the CUs, also at Q = 1
}

// One launch for every instantiation of the search block, in the order of SearchKernel; the LDS follows (k, distinct)
hipError_t launch_search(const SearchArgs& a, SearchKernel kernel, hipStream_t stream) {
    const void* const fn[] = {(const void*)k_search_topk, (const void*)k_search_subjects<SR_LIVE>,
                              (const void*)k_search_subjects<SR_DISTINCT>, search_coarse_kernel(false), search_coarse_kernel(true),
                              (const void*)k_search_filtered<SR_ROWS>, (const void*)k_search_filtered<SR_LIVE>,
                              (const void*)k_search_filtered<SR_DISTINCT>, search_coarse_kernel(false, true),
                              search_coarse_kernel(true, true)};
    const size_t lds = sr_lds_bytes(a.k, kernel == SEARCH_DISTINCT || kernel == SEARCH_FILTERED_DISTINCT);
    hipError_t e = hipFuncSetAttribute(fn[kernel], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<SearchArgs*>(&a)};
    return hipLaunchKernel(fn[kernel], dim3((unsigned)(a.nchunks * a.ntiles)), dim3(256), args, lds, stream);
}

// LDS of a merge: head positions [S], then the staged entries (12 bytes each, 16 with a subject) when they fit under MG_LDS_CAP
hipError_t launch_topk_merge(const float* score, const int64_t* index, const int32_t* subject, int S, int Q, int k, int distinct,
                             float* out_s, int64_t* out_i, int32_t* out_u, hipStream_t stream, const int* live) {
    const size_t head = ((size_t)S * 4 + 15) & ~(size_t)15;
    const size_t full = head + (size_t)S * k * (out_u ? 16 : 12);
    const int staged = S > 0 && full <= (size_t)MG_LDS_CAP;
    const size_t lds = staged ? full : head;
    const void* fn = out_u ? (const void*)k_topk_merge_subjects : (const void*)k_topk_merge;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MG_LDS_CAP);
    if (e != hipSuccess) return e;
    if (out_u)          // the two kernels differ in their arguments, not in their grid
        hipLaunchKernelGGL(k_topk_merge_subjects, dim3((unsigned)Q), dim3(64), lds, stream, score, index, subject, S, Q, k, staged,
                           distinct, out_s, out_i, out_u, live);
    else hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)Q), dim3(64), lds, stream, score, index, S, Q, k, staged, out_s, out_i, live);
    return hipGetLastError();
}

}  // namespace ffr
