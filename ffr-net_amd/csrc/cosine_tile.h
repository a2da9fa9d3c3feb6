// cosine_tile.h -- the 32 probes x 128 rows cosine tile of k_search_topk (search.hip) and k_cluster_walk (cluster.hip): the
// block map, the probe fragments, the per-lane gallery stream with its K loop, the accumulator row map and the score
// formula.  Both kernels instantiate this one definition, so the score of a (probe, row) pair is the same fp32 arithmetic in
// either of them by construction.
//
// K loop: a wave computes the 32 x 32 tile D[g][q] = sum_k G[g][k] Q[q][k] with v_mfma_f32_32x32x2_f32, operands straight from
// global memory / LDS without a repack.  Lane (n = l & 31, h = l >> 5) does ONE 16-byte load of g[n][8j + 4h .. 8j + 4h + 3]
// per group j (64 groups over K = 512) and uses element i as its k-value in the i-th of four MFMAs; the probe operand comes
// from LDS in the same permutation (fragment order [j][lane], written once per block).  Group j accumulates into chain j % 8
// (8 accumulators: 64 k-values per fp32 chain instead of 512, which keeps strongly correlated embeddings within 1e-6 of the
// float64 cosine), and the chains are added in a fixed tree.  16 groups of the gallery operand are in flight ahead of the
// MFMAs, across the tile boundary: one wave per SIMD keeps the pipe fed.
#pragma once
#include <algorithm>

#include "device_util.h"

namespace ffr {

constexpr int CT_DIM = 512;
constexpr int CT_QT = 32;                 // probes per block
constexpr int CT_WAVES = 4;
constexpr int CT_STEP = 32 * CT_WAVES;    // gallery rows per block step
constexpr int CT_NG = CT_DIM / 8;         // 16-byte groups per lane and row half: 64
constexpr int CT_PF = 16;                 // groups of the gallery operand in flight (4 k cycles of MFMA ahead)
constexpr int CT_NACC = 8;                // accumulators per tile: group j feeds chain j % 8 (64 k-values per chain)
constexpr long long CT_MAX_CHUNK = 1 << 20;   // rows: 2^29 floats, a 32-bit element offset

// Chunking of `rows` gallery rows under T probe tiles: chunks x tiles reach blocks_per_cu * num_cus blocks where the rows
// allow it; a chunk is a whole number of steps, at least one, and at most CT_MAX_CHUNK rows.
inline void cosine_chunks(long long T, long long rows, long long blocks_per_cu, int num_cus, int* nchunks, long long* chunk_rows) {
    long long S = (blocks_per_cu * num_cus + T - 1) / T;
    S = std::max(S, (rows + CT_MAX_CHUNK - 1) / CT_MAX_CHUNK);
    S = std::max(1LL, std::min(S, (rows + CT_STEP - 1) / CT_STEP));
    long long cr = (rows + S - 1) / S;
    cr = std::min(CT_MAX_CHUNK, (cr + CT_STEP - 1) / CT_STEP * CT_STEP);
    *nchunks = (int)((rows + cr - 1) / cr);
    *chunk_rows = cr;
}

// XCD-grouped logical block id (bijective for any grid), chunk-major: block b runs on XCD b % 8, and the remap gives each XCD a
// contiguous run of logical blocks, so the probe tiles of one chunk share that XCD's L2
__device__ __forceinline__ void cosine_block(int ntiles, int& chunk, int& tile) {
    const int nb = gridDim.x, b = blockIdx.x, xcd = b & 7, loc = b >> 3, qq = nb >> 3, rr = nb & 7;
    const int lid = xcd < rr ? xcd * (qq + 1) + loc : rr * (qq + 1) + (xcd - rr) * qq + loc;
    chunk = lid / ntiles;
    tile = lid - chunk * ntiles;
}

// probe tile in fragment order: qf[j*64 + l] = q[q0 + (l&31)][8j + 4(l>>5) .. +3], zeros for the probes past nq
__device__ __forceinline__ void cosine_fill_probes(f32x4* qf, const float* q, int q0, int nq, int tid) {
    for (int e = tid; e < CT_NG * 64; e += 256) {
        const int j = e >> 6, l = e & 63, qn = l & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qn < nq) v = *(const f32x4*)(q + (size_t)(q0 + qn) * CT_DIM + 8 * j + 4 * (l >> 5));
        qf[e] = v;
    }
}

// the gathered form: probe qn is the row rows[qn] of q (the caller keeps rows[0 .. nq) inside q); the same fragment order
__device__ __forceinline__ void cosine_fill_probes_gather(f32x4* qf, const float* q, const int* rows, int nq, int tid) {
    for (int e = tid; e < CT_NG * 64; e += 256) {
        const int j = e >> 6, l = e & 63, qn = l & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qn < nq) v = *(const f32x4*)(q + (size_t)rows[qn] * CT_DIM + 8 * j + 4 * (l >> 5));
        qf[e] = v;
    }
}

// row within a block step of accumulator element r of wave w, lane half h
__device__ __forceinline__ int cosine_lane_row(int w, int r, int h) { return acc_row(w * 32, r) + 4 * h; }

// The denominator is one fused multiply-add, spelled out: left to the compiler's contraction, k_search_topk fused it for 14 of
// a lane's 16 scores and not for the other 2, so a pair's last bit depended on where its row sat in a tile (and a kernel that
// places rows elsewhere, k_search_rescore, could not reproduce it).
__device__ __forceinline__ float cosine_score(float acc, float qn, float gn) { return acc / __builtin_fmaf(qn, gn, 1e-8f); }

// The 8 partial chains of a tile, added in a fixed tree.  A macro, expanded in kernel scope: as a function (even a forced
// inline one) the sum is vectorised differently and the register allocation of both kernels moves.
#define COSINE_CHAIN_SUM(a) ((((a)[0] + (a)[1]) + ((a)[2] + (a)[3])) + (((a)[4] + (a)[5]) + ((a)[6] + (a)[7])))

// Where the 16-byte group j of a lane's row lies.  ChunkRows: a row of one chunk of the gallery, a 64-bit chunk base plus
// 32-bit element offsets inside it (<= 2^20 rows = 2^29 floats per chunk).  GatherRows: any row of the gallery, named by its
// 64-bit index (the shortlist of search_coarse.hip spans the whole gallery).
struct ChunkRows {
    typedef int Row;
    const float* __restrict__ base;
    unsigned lane_off;
    __device__ __forceinline__ f32x4 group(int r, int j) const { return *(const f32x4*)(base + ((unsigned)r * CT_DIM + 8u * j + lane_off)); }
};
struct GatherRows {
    typedef long long Row;
    const float* __restrict__ base;
    unsigned lane_off;
    __device__ __forceinline__ f32x4 group(long long r, int j) const { return *(const f32x4*)(base + (size_t)r * CT_DIM + (8u * j + lane_off)); }
};

// A lane's stream through the rows its address rule names, CT_PF groups in flight.
template <class Addr>
struct CosineStreamT {
    Addr addr;
    int lane;
    typename Addr::Row row;
    f32x4 pf[CT_PF];

    __device__ __forceinline__ CosineStreamT(const float* base, int lane_) : addr{base, 4u * (lane_ >> 5)}, lane(lane_) {}

    __device__ __forceinline__ f32x4 group(typename Addr::Row r, int j) const { return addr.group(r, j); }

    // the first CT_PF groups of row r (in bounds)
    __device__ __forceinline__ void prime(typename Addr::Row r) {
        row = r;
#pragma unroll
        for (int u = 0; u < CT_PF; ++u) pf[u] = group(row, u);
    }

    // acc8 = the 8 chains of the 32 x 32 dots of the current row against the probe fragments qf (their sum:
    // COSINE_CHAIN_SUM); the ring refills with the rest of this row, then with the first groups of row `next`, which becomes
    // the current row
    __device__ __forceinline__ void tile(f32x16 (&acc8)[CT_NACC], const f32x4* qf, typename Addr::Row next) {
#pragma unroll
        for (int u = 0; u < CT_NACC; ++u) acc8[u] = f32x16{};
        f32x4 bq = qf[lane];
#pragma unroll
        for (int j = 0; j < CT_NG; ++j) {
            const f32x4 av = pf[j % CT_PF];
            const int jn = j + CT_PF;          // refill the slot: this tile's group jn, or the next tile's group jn - 64
            pf[j % CT_PF] = jn < CT_NG ? group(row, jn) : group(next, jn - CT_NG);
            const f32x4 bv = bq;
            if (j + 1 < CT_NG) bq = qf[(j + 1) * 64 + lane];
            f32x16& acc = acc8[j % CT_NACC];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            FFR_PIN;                           // keep each refill CT_PF groups ahead of its use (hipcc sinks it otherwise)
        }
        row = next;
    }
};
typedef CosineStreamT<ChunkRows> CosineStream;

}  // namespace ffr
