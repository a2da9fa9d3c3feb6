// The V-fed fused Winograd convolution, one definition of every piece that k_wino_fused (wino_fused.hip, F(4x4) tiles) and
// k_wino_fused_mixed (wino_mixed.hip, tiles of 4 and 3 outputs per dimension) have in common, and of what the producers of
// their fragment image V share.  A block is 32 tiles x 32 NT channels; wave w owns S consecutive xi (S = 9 for the
// 36 xi of F(4x4); 8 / 8 / 7 for the mixed types), XP = 4 S xi per K chunk with the padded ones zero.  wino_fused.hip's header
// describes the operand order and the work split; DESIGN.md 3.1 the design.
// Everything is __forceinline__ and takes the accumulators by reference: the kernels sit at 256 VGPRs + 256 AGPRs.
#pragma once
#include "conv_tail.h"
#include "device_util.h"
#include "ffr_kernels.h"
#include "wino_math.h"

namespace ffr {

// ---- input side: the fragment image V [tile group][K chunk][XP][64 pieces][4] -----------------------------------------
// xi 0 of (tile group mb, K chunk kc) for the piece (k half hf, tile tl): the lane of the fused kernels that reads it
template <int XP>
__device__ __forceinline__ float* wino_frag_ptr(float* V, size_t mb, int nkc, int kc, int hf, int tl) {
    return V + ((mb * nkc + kc) * XP) * 256 + (hf * 32 + tl) * 4;
}
// V rows beyond T are zero for every producer (the GEMM computes them and drops the results)
template <int XP>
__device__ __forceinline__ void wino_frag_zero(float* vout) {
#pragma unroll
    for (int e = 0; e < XP; ++e) *reinterpret_cast<f32x4*>(vout + e * 256) = (f32x4){0.f, 0.f, 0.f, 0.f};
}
// B_r^T d B_c of the AR x AC patch d (four channels, loaded by the caller) into the fragments at vout: columns in place, then
// row by row straight into the fragment image; the padded xi (their weights are zero as well) are written as zeros.
// The combine kernels (patch from their LDS image) call this.  k_wino_in_c and k_wino_in_mixed (patch from global memory) keep
// their own loop, which transforms a column while the next one loads: hipcc contracts a * b + c into fma per basic block, so
// the same B^T d B between other loads rounds differently (k_wino_in_mixed: 506 packed fmas instead of 516), and
// every byte of V is held to what these kernels have always written.
template <int AR, int AC>
__device__ __forceinline__ void wino_patch_to_frags(f32x4 (&d)[AR][AC], float* vout) {
    constexpr int X = AR * AC, XP = (X + 3) / 4 * 4;
#pragma unroll
    for (int j = 0; j < AC; ++j) {
        f32x4 col[AR], v[AR];
#pragma unroll
        for (int i = 0; i < AR; ++i) col[i] = d[i][j];
        btv<AR>(col, v);
#pragma unroll
        for (int i = 0; i < AR; ++i) d[i][j] = v[i];
    }
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        f32x4 v[AC];
        btv<AC>(d[i], v);
#pragma unroll
        for (int j = 0; j < AC; ++j) *reinterpret_cast<f32x4*>(vout + (i * AC + j) * 256) = v[j];
    }
#pragma unroll
    for (int e = X; e < XP; ++e) *reinterpret_cast<f32x4*>(vout + e * 256) = (f32x4){0.f, 0.f, 0.f, 0.f};
}
// phase 1 of the combine kernels: x = res * scale[n] + shortcut for the npx pixels of the block's images (first image
// n_first, HW pixels each) and the 32 channels from cb on, to `out` and to s_x [pixel][32]; 8 lanes per pixel line
__device__ __forceinline__ void combine_to_lds(const float* __restrict__ res, const float* __restrict__ scale, const float* __restrict__ sh,
                                               float* __restrict__ out, float* s_x, int n_first, int npx, int HW, int C, int cb) {
    const int tid = threadIdx.x, q4 = (tid & 7) * 4;
    for (int p = tid >> 3; p < npx; p += 32) {
        const int il = p / HW;
        const size_t off = ((size_t)n_first * HW + p) * C + cb + q4;
        const f32x4 sv = scale ? *reinterpret_cast<const f32x4*>(scale + (size_t)(n_first + il) * C + cb + q4) : (f32x4){1.f, 1.f, 1.f, 1.f};
        const f32x4 x = *reinterpret_cast<const f32x4*>(res + off) * sv + *reinterpret_cast<const f32x4*>(sh + off);
        *reinterpret_cast<f32x4*>(out + off) = x;
        *reinterpret_cast<f32x4*>(s_x + p * 32 + q4) = x;
    }
}

// ---- LDS of a fused block ----------------------------------------------------------------------------------------------
constexpr int WF_EPI_FLOATS = 36 * 32 * 32;  // the epilogue's E[xi][tile][32 channels] (147,456 B); the V-fed K loop uses no LDS
// behind it (never aliased; the epilogue's first barrier publishes them): s_bias [9][64], the border-class biases of the block's
// channel group, and s_tile [32][8]: 0 origin pixel of the tile's outputs, 1 valid rows | cols << 8 (0: tile beyond T), 2 / 3
// border rows / columns, 4.. the kernel's own
template <int NT>
__device__ __forceinline__ void wf_fill_bias(float* s_bias, const float* bias, int border_bias, int cout_pad, int n0) {
    for (int i = threadIdx.x; i < (border_bias ? 9 : 1) * 64; i += 256)
        if ((i & 63) < 32 * NT) s_bias[i] = bias[(size_t)(i >> 6) * cout_pad + n0 + (i & 63)];
}
// the record of the MR x MC tile of image n whose outputs start at (r0, c0); valid = false: a tile beyond T
__device__ __forceinline__ void wf_tile_record(int* rec, bool valid, int n, int r0, int c0, int MR, int MC, int H, int W) {
    int pix0 = 0, vrc = 0, br = 0, bc = 0;
    if (valid) {
        pix0 = (n * H + r0) * W + c0;
        const int vr = H - r0 < MR ? H - r0 : MR, vc = W - c0 < MC ? W - c0 : MC;
        vrc = vr | (vc << 8);
        // row i of the tile is the map's top row iff r0 == 0 && i == 0; its bottom row iff i == H - 1 - r0
        br = (r0 == 0 ? 1 : 0) | ((H - 1 - r0) & 0xff) << 8;
        bc = (c0 == 0 ? 1 : 0) | ((W - 1 - c0) & 0xff) << 8;
    }
    rec[0] = pix0; rec[1] = vrc; rec[2] = br; rec[3] = bc;
}

// ---- the accumulators ----------------------------------------------------------------------------------------------------
// 2 S accumulator tiles of 32x32: 18 = 288 registers for S = 9, but a wave addresses 256 AGPRs + 256 VGPRs and hipcc keeps
// every builtin MFMA accumulator in AGPRs (a 17th tile is copied in and out around each of its MFMAs, with the full MFMA
// latency exposed): xi 0..7 of the wave use the builtin (16 tiles, all 256 AGPRs), xi 8 the VGPR form of the same
// instruction through inline asm (accv, 32 VGPRs)
template <int NT>
__device__ __forceinline__ void wf_zero_acc(f32x16 (&acc)[8][NT], f32x16 (&accv)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            accv[nt][r] = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j][nt][r] = 0.f;
        }
}

// ---- the V-fed K loop ----------------------------------------------------------------------------------------------------
// M[xi] += V[xi] U[xi]^T over the nkc K chunks for the S xi of this wave; V = fragment image of tile group mb (XP xi per chunk),
// U [cout_pad/64][K chunk][XP][2 halves][64 lanes][4] of channel group nb (32 NT channels).  st1 (trace build): the shader clock
// between prologue and loop.
// Both streams are read through buffer resources: the per-lane part of the address (lane * 16 bytes) sits in one VGPR,
// everything else -- tile group, wave, xi, K chunk -- in the SCALAR offset, which SALU instructions and immediates
// advance.  (Per-lane 64-bit pointers cost 16 v_add_co / v_addc pairs per K chunk, and every VALU instruction delays
// the next MFMA by its issue time: round 4, measured on k_wino_fused_q first.)
template <int S, int NT>
__device__ __forceinline__ void wf_vfed_gemm(const float* V, const float* U, int mb, int nb, int nkc, int cout_pad, int wave, int lane,
                                             f32x16 (&acc)[8][NT], f32x16 (&accv)[NT], const unsigned long long* trace, unsigned long long& st1) {
    constexpr unsigned XP = 4 * S;
    // (V can exceed 4 GB -- 7.4 GB for the 112x112 layer at 1024 images -- so its resource starts at this block's tile group:
    // 36 KB per K chunk, at most 6.9 MB)
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(V + (size_t)mb * nkc * XP * 256), 0, (unsigned)nkc * XP * 1024u, 0x00020000);
    const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc((void*)U, 0, (unsigned)((size_t)cout_pad * nkc * 8 * XP * 4), 0x00020000);
    const unsigned lane16 = (unsigned)lane * 16u;
    unsigned vp = (unsigned)(S * wave) * 1024u;                                 // scalar byte offsets of this wave's xi 0 in the current K chunk
    unsigned up = NT == 2 ? (unsigned)(nb * nkc * XP + S * wave) * 2048u
                          : (unsigned)((nb >> 1) * nkc * XP + S * wave) * 2048u + (unsigned)(nb & 1) * 1024u;
    auto ldfrag = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned so) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, so, 0));
    };
    // fragment registers: slot j holds (V, U lo, U hi) of xi j for the K chunk that consumes it next
    f32x4 fv[S], fu[S][NT];
    auto load = [&](int j, int part, unsigned v, unsigned u) {
        if (part == 0) fv[j] = ldfrag(vrs, v + j * 1024u);
        else fu[j][part - 1] = ldfrag(urs, u + j * 2048u + (part - 1) * 1024u);
    };
    // ---- prologue: xi 0..S-2 of K chunk 0 in flight (the last follows in step 0) ----
#pragma unroll
    for (int j = 0; j < S - 1; ++j) {
#pragma unroll
        for (int part = 0; part <= NT; ++part) load(j, part, vp, up);
        FFR_PIN;            // in THIS order: vmcnt counts loads in issue order, and the loop's waits are derived from it
    }
    FFR_PIN;
    if (FFR_TRACE_ON(trace)) st1 = __builtin_amdgcn_s_memtime();

    // one K chunk: S steps (xi) of 8 MFMAs; every step reloads the slot the previous step consumed, S - 1 steps ahead of
    // its next use.  vp/up point at the chunk being multiplied.  LAST: no chunk follows.
    auto chunk = [&]<bool LAST>() {
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const f32x4 av = fv[j], b0 = fu[j][0], b1 = fu[j][NT - 1];
#pragma unroll
            for (int g = 0; g < 4 * NT; ++g) {
                const int e = g / NT, nt = g % NT;
                if (j < 8) acc[j][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(nt ? b1[e] : b0[e], av[e], acc[j][nt], 0, 0, 0);
                else asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(accv[nt]) : "v"(nt ? b1[e] : b0[e]), "v"(av[e]));
                // the step's three loads go out back to back in ONE MFMA gap: an MFMA whose gap carries vector-memory
                // instructions issues ~8 cycles late plus ~14 per load (measured: 5.30k cycles per K chunk with one load in
                // each of three gaps, 5.15k with three loads in one gap, 4.70k without loads)
                if (g == 1) {
#pragma unroll
                    for (int part = 0; part <= NT; ++part) {
                        if (j == 0) load(S - 1, part, vp, up);                                          // the last xi of this chunk
                        else if (!LAST) load(j - 1, part, vp + XP * 1024u, up + XP * 2048u);           // xi j-1 of the next chunk
                    }
                }
                FFR_PIN;
            }
        }
    };
#pragma unroll 1
    for (int kc = 0; kc + 1 < nkc; ++kc) {
        chunk.template operator()<false>();
        vp += XP * 1024u;
        up += XP * 2048u;
    }
    chunk.template operator()<true>();
}

// ---- epilogue ------------------------------------------------------------------------------------------------------------
// The products of the block go through LDS in NT passes of 32 channels; a thread then owns (tile, 4 channels).
// Accumulators of 32-channel half nt -> E[xi][tile][32], the first X of the wave's xi S wave .. S wave + S - 1.  The MFMAs run
// with A = U, B = V: a lane holds tile lane & 31 and, in registers 4q..4q+3, the FOUR CONSECUTIVE channels 8q + 4 (lane >> 5) +
// 0..3 -> one 16-byte LDS write (36 per pass instead of 144 dword writes); the 16-byte chunk index is XOR-ed with the tile so
// that 8 lanes (8 tiles, one chunk) hit 8 different bank columns; wf_staged applies the same XOR
template <int S, int X, int NT>
__device__ __forceinline__ void wf_stage_acc(float* smem, int wave, int lane, int nt, const f32x16 (&acc)[8][NT], const f32x16 (&accv)[NT]) {
    const int rowl = lane & 31, hsel = lane >> 5;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const int e = S * wave + j;
        if (X == 4 * S || e < X) {
            const f32x16& t16 = j < 8 ? acc[j < 8 ? j : 0][nt] : accv[nt];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(smem + (e * 32 + rowl) * 32 + (((2 * q + hsel) ^ (rowl & 7)) * 4)) =
                    (f32x4){t16[4 * q], t16[4 * q + 1], t16[4 * q + 2], t16[4 * q + 3]};
        }
    }
}
// the staged products of (tile tl, channel quad cq): xi at [xi * 256]
__device__ __forceinline__ const f32x4* wf_staged(const float* smem, int tl, int cq) {
    return reinterpret_cast<const f32x4*>(smem + tl * 32 + 4 * (cq ^ (tl & 7)));
}
// offsets into s_bias of the border classes of a tile's M rows (stride 3 * 64) or columns (64) from the record's br / bc:
// class 0 = first row of the map, 2 = last, 1 = interior
template <int M>
__device__ __forceinline__ void wf_border_offsets(int b, int stride, int (&o)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) o[i] = ((i == 0 && (b & 1)) ? 0 : (i == (b >> 8) ? 2 : 1)) * stride;
}
// (the pointwise part of the epilogue is conv_tail.h's, in the form PRELU_MINMAX)

}  // namespace ffr
