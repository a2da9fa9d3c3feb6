// The fp32 operand path of the GEMM family, one definition of what the fp32 form of k_igemm (igemm.hip) and k_gemm_stream
// (gemm_stream.hip) have in common: a K-tile of 32 floats per row is fetched by 16-byte LDS-DMA pieces into the stage
// [BM rows of A, then BN rows of B][32], lane-linear for the DMA, with the 16-B chunk index XOR-swizzled by (row >> 1) & 7 on
// the SOURCE side and on the ds_read_b128 side (bank-conflict free fragment reads); one ds_read_b128 per operand row feeds
// the 4 v_mfma_f32_32x32x2_f32 of an 8-k chunk (lanes 0-31 hold k..k+3, lanes 32-63 k+4..k+7).  The kernels own their
// pointers, their stage ring and what happens between K-tiles; igemm.hip's header describes the convolution around it.
// Everything is __forceinline__ and takes its arrays by reference.
#pragma once
#include "device_util.h"

namespace ffr {

// The thread id through an opaque asm.  The kernels re-derive every lane value from it per segment / per tile: otherwise
// hipcc hoists every lane-dependent address out of that loop and keeps ~100 extra VGPRs alive across the MFMA loop
// (k_igemm 128x64: 196 instead of ~100 registers -> 2 blocks/CU).
__device__ __forceinline__ int opaque_tid() {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return tid;
}

// The lane map of wave (wm, wn) of a WARPS_M x WARPS_N grid over a BM x BN tile.  Staging: this lane fetches the logical
// chunk lch of row srow + 32 d of piece d.  Fragments: row frow of the wave's 32-row blocks, k half fh; fragA / fragB = float
// offset of its first A / B row in a stage, pc[q] = swizzled float offset of chunk q (of 4) in a row.
template <int BM, int WM, int WN>
__device__ __forceinline__ void igemm_lane_map(int tid, int wm, int wn, int& srow, int& lch, int& frow, int& fh, int (&pc)[4], int& fragA,
                                               int& fragB) {
    const int lane = tid & 63;
    srow = tid >> 3;                                 // 0..31
    lch = (tid & 7) ^ ((srow >> 1) & 7);
    frow = lane & 31;
    fh = lane >> 5;
    const int fswz = (lane >> 1) & 7;
#pragma unroll
    for (int q = 0; q < 4; ++q) pc[q] = ((2 * q + fh) ^ fswz) * 4;
    fragA = (wm * WM + frow) * 32;
    fragB = (BM + wn * WN + frow) * 32;
}

// LDS-DMA piece d of a K-tile: 16 B per lane, 8 rows x 128 B per wave, into the stage rows [32 d, 32 d + 32) (A pieces first:
// BM = 32 A_PT, so the B piece i is piece A_PT + i); src, this lane's source of the piece, moves on one K-tile
__device__ __forceinline__ void igemm_dma_piece(float* stage, int wave, int d, const float*& src) {
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(stage + (32 * d + 8 * wave) * 32), 16, 0, 0);
    src += 32;
}

// fragment read r of a chunk: rows of A then rows of B, 16 B per lane (4 k values)
template <int TM, int TN>
__device__ __forceinline__ void igemm_read_piece(f32x4 (&af)[TM], f32x4 (&bf)[TN], const float* stage, int fragA, int fragB, int pcv, int r) {
    if (r < TM) af[r] = *reinterpret_cast<const f32x4*>(stage + fragA + r * 32 * 32 + pcv);
    else bf[r - TM] = *reinterpret_cast<const f32x4*>(stage + fragB + (r - TM) * 32 * 32 + pcv);
}

// One K-tile of a wave's TM x TN blocks of 32 x 32: four 8-k chunks from `stage`, fragments double-buffered in af / bf (slot
// 0 holds chunk 0 on entry).  Every MFMA gap (64 cycles on the SIMD's matrix pipe) carries at most ONE filler -- a fragment
// ds_read_b128 for the next chunk or one LDS-DMA piece of the next K-tile -- and the order is pinned (sched_barrier): an
// LDS-DMA costs its wave ~60 issue cycles, so 4-8 of them back to back starve the matrix pipe (measured: -10 % at 8
// blocks/CU, more in the 1-block/CU tail).  The barrier that publishes the next K-tile (in stage_n) sits in front of the LAST
// chunk, so its first fragments are read under that chunk's MFMAs.  LAST: nothing follows, no DMA, no barrier, no read-ahead.
// dma(d) issues piece d (of ND) of the next K-tile; after_chunk1() runs once all of them are out.
template <int TM, int TN, int ND, bool LAST, typename Dma, typename After>
__device__ __forceinline__ void igemm_ktile(f32x16 (&acc)[TM][TN], f32x4 (&af)[2][TM], f32x4 (&bf)[2][TN], const float* stage,
                                            const float* stage_n, int fragA, int fragB, const int (&pc)[4], Dma&& dma, After&& after_chunk1) {
    constexpr int NQ = TM * TN * 4;          // MFMAs per 8-k chunk
    constexpr int NR = TM + TN;              // fragment reads per chunk
    constexpr int NDH = (ND + 1) / 2;        // DMA pieces issued in the gaps of chunk 0 and of chunk 1
    static_assert(NR + NDH <= NQ, "fillers must fit the MFMA gaps of a chunk");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q == 3 && !LAST) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            FFR_PIN;
        }
#pragma unroll
        for (int g = 0; g < NQ; ++g) {
            const int e = g / (TM * TN), i = (g / TN) % TM, j = g % TN;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q & 1][i][e], bf[q & 1][j][e], acc[i][j], 0, 0, 0);
            if (g < NR) {
                if (q < 3) igemm_read_piece(af[(q + 1) & 1], bf[(q + 1) & 1], stage, fragA, fragB, pc[q + 1], g);
                else if (!LAST) igemm_read_piece(af[0], bf[0], stage_n, fragA, fragB, pc[0], g);
            } else if (!LAST && q < 2 && (g - NR) < NDH && q * NDH + (g - NR) < ND) {
                dma(q * NDH + (g - NR));
            }
            FFR_PIN;
        }
        if (q == 1 && !LAST) after_chunk1();
    }
}

}  // namespace ffr
