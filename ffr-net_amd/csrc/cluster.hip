// cluster.hip -- group N unlabelled 512-d embeddings into identities on the device (include/ffrnet.h:
// ffr_cluster_threshold / ffr_cluster_templates): single-link clustering at one cosine threshold, then one template row
// per cluster.  The N x N score matrix never leaves the chip; the output is one label per row.
//
// Edge rule: rows i < j are joined iff s(probe = i, gallery row = j) > threshold (strict, as eval_acc compares), with
// s = dot / (|i| |j| + 1e-8) in exactly the fp32 arithmetic of k_search_topk (search.hip): the score of (i, j) is
// bit-for-bit the score ffr_search_topk returns for probe i and gallery row j.  The diagonal and i > j are never evaluated.
//
// k_cluster_init     parent[x] = x.
// k_cluster_join     the hot path: the self-join of the [N][512] array with itself.
//  - K loop: the K loop of k_search_topk, copied unchanged (32 probes x 128 rows per block step, v_mfma_f32_32x32x2_f32,
//    operands in the same lane permutation, 8 accumulator chains added in the same fixed tree, acc / (qn*gn + 1e-8f)).
//    Keep the two loops textually identical: the tests compare the edge set with the scores of ffr_search_topk bitwise.
//  - Triangle: a block is (chunk of rows, tile of 32 probes), logical id as in the search.  A block whose chunk ends at
//    or before its tile's first probe has no pair i < j and exits at once; the others start at the first 128-row step
//    that can hold a row greater than the tile's smallest probe.  The grid is the chunks x tiles rectangle (cluster_plan
//    sizes the chunks so that the blocks with work, about half of it, fill the CUs several times over: their work is uneven
//    along the diagonal); the idle half costs one early return each.  Known cost (EXPERIMENTS.md): an XCD takes a
//    contiguous run of tiles, so the XCD with the long rows of the triangle finishes last.
//  - Epilogue: no list, no LDS merge.  Lane (n, h) holds the 16 scores of probe q0 + n; every (i, j) with i < j, j inside
//    the chunk and score > threshold is united in a lock-free union-find over parent[N] (int32, the handle's scratch):
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
// k_cluster_flatten  rep[i] = find(i) as int64, after the join in stream order.
// k_cluster_templates  one template per cluster: t = sum_r x_r / |x_r| over the cluster's rows in ascending row index
//                (order[] = rows sorted by cluster then index, offsets[C + 1]), then t / |t|.  One wave per cluster, lane
//                l owns components 8l .. 8l + 7; the sum over the rows is sequential fp32 per component: deterministic,
//                no atomics.  A zero row contributes zero, an all-zero sum stays zero.  Without norms[] the wave computes
//                |x_r| with the summation order of k_row_norms (bitwise the same value).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ffr_kernels.h"

namespace ffr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// the tile constants of search.hip
constexpr int CL_DIM = 512;
constexpr int CL_QT = 32;                 // probes per block
constexpr int CL_WAVES = 4;
constexpr int CL_STEP = 32 * CL_WAVES;    // rows per block step
constexpr int CL_NG = CL_DIM / 8;         // 16-byte groups per lane and row half: 64
constexpr int CL_PF = 16;                 // groups of the row operand in flight
constexpr int CL_NACC = 8;                // accumulators per tile: group j feeds chain j % 8
constexpr long long CL_MAX_CHUNK = 1 << 20;   // rows: 2^29 floats, a 32-bit element offset

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

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

__global__ __launch_bounds__(256) void k_cluster_flatten(const int* __restrict__ parent, int n, int64_t* __restrict__ rep) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n) rep[x] = uf_find(parent, x);
}

struct JoinArgs {
    const float* emb;         // [N][512]
    const float* norm;        // [N]
    int* parent;              // [N]
    long long N;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), a multiple of CL_STEP, <= CL_MAX_CHUNK
    float threshold;
    int nchunks, ntiles;
};

__global__ __launch_bounds__(256, 1) void k_cluster_join(const JoinArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 qf[CL_NG * 64];    // probe fragments [64][64]

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // XCD-grouped logical block id (bijective for any grid), chunk-major: as k_search_topk
    const int nb = gridDim.x, b = blockIdx.x, xcd = b & 7, loc = b >> 3, qq = nb >> 3, rr = nb & 7;
    const int lid = xcd < rr ? xcd * (qq + 1) + loc : rr * (qq + 1) + (xcd - rr) * qq + loc;
    const int chunk = lid / a.ntiles, tile = lid - chunk * a.ntiles;
    const long long c0 = (long long)chunk * a.chunk_rows;
    const long long rem = a.N - c0;
    const int rows = (int)(rem < a.chunk_rows ? rem : a.chunk_rows);    // >= 1
    const int q0 = tile * CL_QT;
    if (c0 + rows <= (long long)q0 + 1) return;        // no row of this chunk is greater than the tile's smallest probe
    const int nq = min(CL_QT, (int)(a.N - q0));
    // the first step that can hold row q0 + 1
    const int step0 = (long long)q0 + 1 > c0 ? (int)(((long long)q0 + 1 - c0) / CL_STEP) : 0;

    // probe tile in fragment order: qf[j*64 + l] = q[q0 + (l&31)][8j + 4(l>>5) .. +3]
    for (int e = tid; e < CL_NG * 64; e += 256) {
        const int j = e >> 6, l = e & 63, qn = l & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qn < nq) v = *(const f32x4*)(a.emb + (size_t)(q0 + qn) * CL_DIM + 8 * j + 4 * (l >> 5));
        qf[e] = v;
    }
    const float qn_lane = n < nq ? a.norm[q0 + n] : 0.f;
    const int irow = q0 + n;                            // this lane's probe row (an edge needs n < nq)

    // 64-bit chunk base, 32-bit element offsets inside it
    const float* __restrict__ gch = a.emb + (size_t)c0 * CL_DIM;
    const float* __restrict__ nch = a.norm + c0;
    const unsigned lane_off = 4u * h;
    int row = min(step0 * CL_STEP + w * 32 + n, rows - 1);
    f32x4 pf[CL_PF];
#pragma unroll
    for (int u = 0; u < CL_PF; ++u) pf[u] = *(const f32x4*)(gch + ((unsigned)row * CL_DIM + 8u * u + lane_off));
    __syncthreads();

    const int nsteps = (rows + CL_STEP - 1) / CL_STEP;
    for (int step = step0; step < nsteps; ++step) {
        const int sbase = step * CL_STEP;
        const int next = min(row + CL_STEP, rows - 1);
        // norms of the 16 rows this lane scores, fetched ahead of the K loop
        float gn[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gr = min(sbase + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, rows - 1);
            gn[r] = nch[(unsigned)gr];
        }
        f32x16 acc8[CL_NACC];
#pragma unroll
        for (int u = 0; u < CL_NACC; ++u) acc8[u] = f32x16{};
        f32x4 bq = qf[lane];
#pragma unroll
        for (int j = 0; j < CL_NG; ++j) {
            const f32x4 av = pf[j % CL_PF];
            const int jn = j + CL_PF;          // refill the slot: this tile's group jn, or the next tile's group jn - 64
            if (jn < CL_NG) pf[j % CL_PF] = *(const f32x4*)(gch + ((unsigned)row * CL_DIM + 8u * jn + lane_off));
            else pf[j % CL_PF] = *(const f32x4*)(gch + ((unsigned)next * CL_DIM + 8u * (jn - CL_NG) + lane_off));
            const f32x4 bv = bq;
            if (j + 1 < CL_NG) bq = qf[(j + 1) * 64 + lane];
            f32x16& acc = acc8[j % CL_NACC];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);     // keep each refill CL_PF groups ahead of its use (hipcc sinks it otherwise)
        }
        row = next;
        // the 8 partial chains in a fixed tree
        const f32x16 acc = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));

        // epilogue: scores, edge test (i < j inside the chunk, score > threshold), union
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;        // row within the step
            const float sc = acc[r] / (qn_lane * gn[r] + 1e-8f);
            if (n < nq && sbase + lr < rows && c0 + sbase + lr > (long long)irow && sc > a.threshold) mask |= 1u << r;
        }
        while (mask) {
            const int r = __builtin_ctz(mask);
            mask &= mask - 1;
            const int jrow = (int)(c0 + sbase + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);      // < N < 2^31
            uf_unite(a.parent, irow, jrow);
        }
    }
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
        const float* p = a.emb + (size_t)a.order[e] * CL_DIM;
        float nr;
        if (a.norm) {
            nr = a.norm[a.order[e]];
        } else {                         // |x_r| in the summation order of k_row_norms
            float aa = 0.f;
            for (int k = lane; k < CL_DIM; k += 64) {
                const float v = p[k];
                aa += v * v;
            }
            nr = sqrtf(wave_sum64(aa));
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
    const float tn = sqrtf(wave_sum64(ss));
    if (tn > 0.f) {
        t0 /= tn;
        t1 /= tn;
    }
    float* o = a.out + (size_t)c * CL_DIM + 8 * lane;
    *(f32x4*)o = t0;
    *(f32x4*)(o + 4) = t1;
}

}  // namespace

// The search balances a rectangle; here only the blocks on and above the diagonal work, about half of chunks x tiles, and
// the ones on the diagonal less than the others: aim at 4 working blocks per CU so that the uneven ones even out.
void cluster_plan(long long N, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    const long long T = (N + CL_QT - 1) / CL_QT;
    long long S = (8LL * num_cus + T - 1) / T;
    S = std::max(S, (N + CL_MAX_CHUNK - 1) / CL_MAX_CHUNK);
    S = std::max(1LL, std::min(S, (N + CL_STEP - 1) / CL_STEP));       // at least one step of rows per chunk
    long long cr = (N + S - 1) / S;
    cr = std::min(CL_MAX_CHUNK, (cr + CL_STEP - 1) / CL_STEP * CL_STEP);
    *ntiles = (int)T;
    *nchunks = (int)((N + cr - 1) / cr);
    *chunk_rows = cr;
}

hipError_t launch_cluster_threshold(const float* emb, const float* norms, long long N, float threshold, int ntiles, int nchunks,
                                    long long chunk_rows, int* parent, int64_t* rep, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    const unsigned nb = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(k_cluster_init, dim3(nb), dim3(256), 0, stream, parent, (int)N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (N > 1) {
        JoinArgs a{emb, norms, parent, N, chunk_rows, threshold, nchunks, ntiles};
        hipLaunchKernelGGL(k_cluster_join, dim3((unsigned)((long long)nchunks * ntiles)), dim3(256), 0, stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_cluster_flatten, dim3(nb), dim3(256), 0, stream, (const int*)parent, (int)N, rep);
    return hipGetLastError();
}

hipError_t launch_cluster_templates(const float* emb, const float* norms, const int64_t* order, const int64_t* offsets,
                                    long long C, float* templates, hipStream_t stream) {
    if (C <= 0) return hipSuccess;
    TemplateArgs a{emb, norms, order, offsets, templates, C};
    hipLaunchKernelGGL(k_cluster_templates, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ffr
