// coarse_tile.h -- the bf16 form of the 32 probes x 128 rows tile of cosine_tile.h, for the shortlist pass of
// search_coarse.hip: the rules of the coarse search (bound, shortlist size, safe norms), the probe planes, the per-lane plane
// stream with its K loop and the coarse score.
//
// K loop: a wave computes the 32 x 32 tile D[g][q] = sum_k G^[g][k] (Qhi[q][k] + Qlo[q][k]) with v_mfma_f32_32x32x16_bf16.
// Lane (n = l & 31, h = l >> 5) does ONE 16-byte load of the 8 bf16 g^[n][16j + 8h .. 16j + 8h + 7] per group j (32 groups
// over K = 512) and feeds it to two MFMAs, against the hi and the lo plane of the probes, which come from LDS in the same
// permutation (fragment order [plane][j][lane], written once per block).  Both operands arrive as bf16: no conversion in
// the loop.  One accumulator: a single chain of this instruction issues back to back.  The whole next row (32 groups) is in
// flight ahead of the MFMAs -- a bf16 tile lasts an eighth of the fp32 one, so the 16 groups of cosine_tile.h would cover
// a quarter of the memory latency they cover there.  A load instruction takes 32 bytes of each of a wave's 32 rows, a
// quarter of a 128-byte line, and with a row per lane in flight (128 KB per CU) a line does not stay in the 32 KB vector
// cache from one group to the next; the four loads that share a line are therefore issued back to back rather than one per
// group (measured: 3-4 % of the pass; the pass stays bound by this access pattern, EXPERIMENTS.md).
#pragma once
#include <stdint.h>

#include "cosine_tile.h"
#include "ffrnet.h"

namespace ffr {

constexpr float COARSE_EPS = FFR_COARSE_EPS;                 // |coarse - exact score| <= COARSE_EPS (search_coarse.hip)
constexpr int COARSE_MAX_K = 64;                             // the pass serves k <= 64; above, the exact search runs alone
constexpr int COARSE_MAX_SHORT = 128;
// rows the pass lists per probe for a top-k
__host__ __device__ constexpr int coarse_shortlist(int k) { return 2 * k > COARSE_MAX_SHORT ? COARSE_MAX_SHORT : 2 * k < 32 ? 32 : 2 * k; }
// Identities (ffr_search_topk_coarse_subjects, distinct = 1): a person's rows crowd the head of a shortlist of rows, so the
// list is min(128, max(4k, 64)) rows long and the pass serves k <= 32
constexpr int COARSE_MAX_K_DISTINCT = 32;
__host__ __device__ constexpr int coarse_shortlist_distinct(int k) { return 4 * k > COARSE_MAX_SHORT ? COARSE_MAX_SHORT : 4 * k < 64 ? 64 : 4 * k; }
// a norm the bound holds for: zero (over a row of zeros: coarse_any_nonzero8), or within [2^-60, 2^60] (outside, the sum of
// squares under- or overflows)
__host__ __device__ __forceinline__ bool coarse_safe_norm(float nrm) { return nrm == 0.f || (nrm >= 0x1p-60f && nrm <= 0x1p60f); }
__device__ __forceinline__ bool coarse_any_nonzero8(const float* p) {
    const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
    return v0.x != 0.f || v0.y != 0.f || v0.z != 0.f || v0.w != 0.f || v1.x != 0.f || v1.y != 0.f || v1.z != 0.f || v1.w != 0.f;
}

constexpr int CO_NG = CT_DIM / 16;        // 16-byte groups of 8 bf16 per lane and row half: 32

// bf16(x / nrm) of 8 consecutive elements, and (lo != null) the bf16 of what that rounding left; a zero (or NaN) norm gives zeros
__device__ __forceinline__ u32x4 coarse_round8(const float* p, float nrm, u32x4* lo) {
    u32x4 hi = {0u, 0u, 0u, 0u};
    if (lo) *lo = hi;
    if (!(nrm > 0.f)) return hi;
    const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
    float x[8] = {v0.x / nrm, v0.y / nrm, v0.z / nrm, v0.w / nrm, v1.x / nrm, v1.y / nrm, v1.z / nrm, v1.w / nrm};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = split_bf16_first(x[2 * i], x[2 * i + 1]);      // x becomes the residual
        if (lo) (*lo)[i] = cvt_pk_bf16(x[2 * i], x[2 * i + 1]);
    }
    return hi;
}

// probe tile in fragment order, two planes: qf[(plane * 32 + j) * 64 + l] = 8 bf16 of q^[q0 + (l&31)][16j + 8(l>>5) .. +7],
// q^ = q / |q| = hi + lo; zeros for the probes past nq
__device__ __forceinline__ void coarse_fill_probes(u32x4* qf, const float* q, const float* qnorm, int q0, int nq, int tid) {
    for (int e = tid; e < CO_NG * 64; e += 256) {
        const int j = e >> 6, l = e & 63, qn = l & 31;
        u32x4 hi = {0u, 0u, 0u, 0u}, lo = hi;
        if (qn < nq) hi = coarse_round8(q + (size_t)(q0 + qn) * CT_DIM + 16 * j + 8 * (l >> 5), qnorm[q0 + qn], &lo);
        qf[e] = hi;
        qf[CO_NG * 64 + e] = lo;
    }
}

// c = (sum q^ g^) * |q||g| / (|q||g| + 1e-8): the factor (<= 1) of the exact score's denominator, from the same fp32 norms
__device__ __forceinline__ float coarse_score(float acc, float qn, float gn) {
#pragma clang fp contract(off)             // one arithmetic wherever the row sits in a tile
    const float p = qn * gn;
    return acc * (p / (p + 1e-8f));
}

// A lane's stream through one chunk of the plane: a 64-bit chunk base plus 32-bit element offsets inside it (<= 2^20 rows =
// 2^29 bf16 per chunk), one row in flight.
struct CoarseStream {
    const uint16_t* __restrict__ base;
    unsigned lane_off;
    int lane, row;
    u32x4 pf[CO_NG];

    __device__ __forceinline__ CoarseStream(const uint16_t* chunk_base, int lane_) : base(chunk_base), lane_off(8u * (lane_ >> 5)), lane(lane_) {}

    __device__ __forceinline__ u32x4 group(int r, int j) const { return *(const u32x4*)(base + ((unsigned)r * CT_DIM + 16u * j + lane_off)); }

    // row r (in bounds of the chunk)
    __device__ __forceinline__ void prime(int r) {
        row = r;
#pragma unroll
        for (int u = 0; u < CO_NG; ++u) pf[u] = group(row, u);
    }

    // the 32 x 32 coarse dots of the current row against the probe planes qf; the ring refills with row `next`, which becomes
    // the current row
    __device__ __forceinline__ f32x16 tile(const u32x4* qf, int next) {
        f32x16 acc = {};
#pragma unroll
        for (int j = 0; j < CO_NG; ++j) {
            const bf16x8 av = __builtin_bit_cast(bf16x8, pf[j]);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, qf[j * 64 + lane]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, qf[(CO_NG + j) * 64 + lane]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bl, acc, 0, 0, 0);
            if ((j & 3) == 3) {                // refill a whole 128-byte line of the row (4 groups) at once, see above
#pragma unroll
                for (int u = j - 3; u <= j; ++u) pf[u] = group(next, u);
            }
            FFR_PIN;                           // keep each refill a row ahead of its use
        }
        row = next;
        return acc;
    }
};

}  // namespace ffr
