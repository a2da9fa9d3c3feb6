// The F(4x4,3x3) and F(3x3,3x3) transforms shared by the Winograd kernels (winograd.hip, wino_fused.hip, wino_mixed.hip).
#pragma once
#include "device_util.h"

namespace ffr {

// v = B^T d for any vector width, 12 operations (shared sub-expressions of the F(4x4,3x3) input transform)
template <typename V>
__device__ __forceinline__ void bt6t(const V d[6], V v[6]) {
    const V p = d[4] - 4.f * d[2], q = d[3] - 4.f * d[1];
    const V t0 = d[4] - d[2], t1 = d[3] - d[1];
    v[0] = 4.f * d[0] + (d[4] - 5.f * d[2]);
    v[1] = p + q;
    v[2] = p - q;
    v[3] = t0 + 2.f * t1;
    v[4] = t0 - 2.f * t1;
    v[5] = 4.f * d[1] + (d[5] - 5.f * d[3]);
}

// v = B^T d as the stand-alone transform kernels always computed it.  NOT bt6t with V = f32x4: the sub-expression order
// differs, so the two round differently and both stay.
__device__ __forceinline__ void bt6v(const f32x4 d[6], f32x4 v[6]) {
    v[0] = 4.f * d[0] - 5.f * d[2] + d[4];
    v[1] = -4.f * (d[1] + d[2]) + d[3] + d[4];
    v[2] = 4.f * (d[1] - d[2]) - d[3] + d[4];
    v[3] = 2.f * (d[3] - d[1]) - d[2] + d[4];
    v[4] = 2.f * (d[1] - d[3]) - d[2] + d[4];
    v[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}

// y = A^T m for any vector width (float, f32x2, f32x4)
template <typename V>
__device__ __forceinline__ void at6t(const V m[6], V y[4]) {
    const V s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    y[0] = m[0] + s12 + s34;
    y[1] = d12 + 2.f * d34;
    y[2] = s12 + 4.f * s34;
    y[3] = d12 + 8.f * d34 + m[5];
}

// v = B^T d for F(3,3): 5 points {0, 1, -1, 2, inf}
__device__ __forceinline__ void bt5v(const f32x4 d[5], f32x4 v[5]) {
    v[0] = 2.f * d[0] - d[1] - 2.f * d[2] + d[3];
    v[1] = -2.f * d[1] - d[2] + d[3];
    v[2] = 2.f * d[1] - 3.f * d[2] + d[3];
    v[3] = d[3] - d[1];
    v[4] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
}
// y = A^T m for F(3,3)
__device__ __forceinline__ void at5q(const f32x4 m[5], f32x4 y[3]) {
    const f32x4 s12 = m[1] + m[2], d12 = m[1] - m[2];
    y[0] = m[0] + s12 + m[3];
    y[1] = d12 + 2.f * m[3];
    y[2] = s12 + 4.f * m[3] + m[4];
}
// by the number of interpolation points of a dimension: 6 = 4 outputs, 5 = 3 outputs
template <int A> __device__ __forceinline__ void btv(const f32x4* d, f32x4* v) { if constexpr (A == 6) bt6v(d, v); else bt5v(d, v); }
template <int A> __device__ __forceinline__ void atq(const f32x4* m, f32x4* y) { if constexpr (A == 6) at6t(m, y); else at5q(m, y); }

// ---- the F(4x4,3x3) tile walk -----------------------------------------------------------------------------------------
// tile t < 2^31 of a map of th x tw tiles per image -> image n, tile row ty, tile column tx, in 32-bit arithmetic (a 64-bit
// division is ~100 instructions)
__device__ __forceinline__ void wino_tile_of(unsigned t, int th, int tw, int* n, int* ty, int* tx) {
    const unsigned tpi = (unsigned)(tw * th);
    const unsigned nn = t / tpi, tr = t - nn * tpi;
    const unsigned y = tr / (unsigned)tw;
    *n = (int)nn; *ty = (int)y; *tx = (int)(tr - y * (unsigned)tw);
}
// The 6x6 patch whose top-left pixel is (h0, w0) of the image src [H][W][pitch], four channels, gathered column by column
// with B^T applied to every column: tmp[i][j] = (B^T d)[i][j].  PAD_MODE 0: zeros outside the map, 1: reflection.  A column
// is transformed while the next one loads (see wino_fused_core.h on why the patch loops are not wino_patch_to_frags).
// The reflection is written out, not reflect_index_clamped (device_util.h): through the call the reflect instances of k_wino_in
// and k_wino_in_c lose 4 and 2 VGPRs and their fp sequence is reordered.
template <int PAD_MODE>
__device__ __forceinline__ void wino_gather_bt_cols(const float* src, int H, int W, int pitch, int h0, int w0, f32x4 (&tmp)[6][6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        f32x4 d[6], v[6];
        int wi = w0 + j;
        bool okw = true;
        if (PAD_MODE == 1) wi = wi < 0 ? -wi : (wi >= W ? 2 * W - 2 - wi : wi);
        else okw = (unsigned)wi < (unsigned)W;
        if (PAD_MODE == 1 && wi < 0) wi = 0;      // tiles hanging over the right/bottom edge (outputs dropped)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            int hi = h0 + i;
            bool ok = okw;
            if (PAD_MODE == 1) { hi = hi < 0 ? -hi : (hi >= H ? 2 * H - 2 - hi : hi); if (hi < 0) hi = 0; }
            else ok = ok && ((unsigned)hi < (unsigned)H);
            d[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (ok) d[i] = *reinterpret_cast<const f32x4*>(src + ((size_t)hi * W + wi) * pitch);
        }
        bt6v(d, v);
#pragma unroll
        for (int i = 0; i < 6; ++i) tmp[i][j] = v[i];
    }
}
// (The A^T column pass over a tile's 36 products stays a loop of its own in k_wino_out, k_wino_out_in and k_wino_fused: as one
// shared function it reorders the fp sequence of k_wino_out_in and makes k_wino_fused's 32 x 64 forms spill 20 bytes.)

}  // namespace ffr
