// The pointwise tail of a convolution (ConvTail, ffr_kernels.h), one definition for the five kernels a convolution ends in:
// add the bias of the pixel's border class, PReLU, add the residual, sigmoid under flags bit 0; the caller stores the value
// and adds it into its tile sum.  Everything is __forceinline__: the fused kernels sit at 256 VGPRs + 256 AGPRs.
#pragma once
#include "device_util.h"

namespace ffr {

// PReLU has two spellings, equal except for the sign of a zero and for NaN; every kernel keeps the one it has always had
// (its bits, and its epilogue's instruction count, depend on it):
//   PRELU_SELECT  k_igemm, k_wino_out, k_wino_out_in: compare and select
//   PRELU_MINMAX  k_wino_fused, k_wino_fused_mixed: max / min / fma, no compare through VCC (their epilogues are issue-bound)
enum PreluForm { PRELU_SELECT, PRELU_MINMAX };
__device__ __forceinline__ float prelu_select(float v, float s) { return v >= 0.f ? v : v * s; }
__device__ __forceinline__ float prelu_minmax(float v, float s) { return fmaxf(v, 0.f) + s * fminf(v, 0.f); }
template <PreluForm F>
__device__ __forceinline__ float prelu(float v, float s) { return F == PRELU_SELECT ? prelu_select(v, s) : prelu_minmax(v, s); }

__device__ __forceinline__ float tail_sigmoid(float v) { return 1.0f / (1.0f + __expf(-v)); }

// the slopes of the channels c .. c + 3; no slopes: 1, PReLU is the identity
__device__ __forceinline__ f32x4 tail_slope4(const float* slope, int c) {
    f32x4 s = {1.f, 1.f, 1.f, 1.f};
    if (slope) s = *reinterpret_cast<const f32x4*>(slope + c);
    return s;
}
// border class of output row or column o of n (3x3, stride 1, pad 1): 0 first, 2 last, 1 interior; a pixel's class is
// 3 * (row class) + (column class).  (k_igemm's s_cls is defined by tap bounds for any stride and pad and stays its own.)
__device__ __forceinline__ int border_class(int o, int n) { return o == 0 ? 0 : (o == n - 1 ? 2 : 1); }

// The tail of one output pixel, four channels, in its two halves.  tail_act4: bias and PReLU (all that k_wino_out_in, the
// activation between conv1 and conv2, applies; k_wino_out applies it once in front of its vector / scalar branch) ...
template <PreluForm F>
__device__ __forceinline__ f32x4 tail_act4(f32x4 v, const f32x4& bias, const f32x4& slope) {
    v += bias;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = prelu<F>(v[c], slope[c]);
    return v;
}
// ... tail_end4: residual (resid() is evaluated only if has_res) and sigmoid
template <typename R>
__device__ __forceinline__ f32x4 tail_end4(f32x4 v, bool has_res, R&& resid, int flags) {
    if (has_res) v += resid();
    if (flags & 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = tail_sigmoid(v[c]);
    }
    return v;
}
template <PreluForm F, typename R>
__device__ __forceinline__ f32x4 tail4(const f32x4& v, const f32x4& bias, const f32x4& slope, bool has_res, R&& resid, int flags) {
    return tail_end4(tail_act4<F>(v, bias, slope), has_res, resid, flags);
}
// one output pixel, one channel, after the PReLU: the three scalar-store loops (odd pitches, channel counts that end inside a
// quad).  The residual is a callable as in tail_end4: taken as an address-or-null, k_wino_fused and k_wino_out grow by 250-550
// instructions and k_igemm's fp sequence is reordered.
template <typename R>
__device__ __forceinline__ float tail_end1(float v, bool has_res, R&& resid, int flags) {
    if (has_res) v += resid();
    if (flags & 1) v = tail_sigmoid(v);
    return v;
}
// the sum of a tile's stored outputs (ConvTail::tile_sums), tile_sums [slot][cout_pad]
__device__ __forceinline__ void tail_store_tile_sum(float* tile_sums, long long slot, int cout_pad, int c, const f32x4& psum) {
    *reinterpret_cast<f32x4*>(tile_sums + (size_t)slot * cout_pad + c) = psum;
}

}  // namespace ffr
