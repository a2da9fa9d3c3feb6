// The device vocabulary every kernel translation unit shares: vector types, address-space casts, the scheduling pin, the
// 64-lane sum, the 32x32 accumulator row map and the bf16 pieces of the split-operand forms.  One definition each.
#pragma once
#include <hip/hip_runtime.h>

namespace ffr {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
// nothing is scheduled across this point
#define FFR_PIN __builtin_amdgcn_sched_barrier(0)

// sum over the 64 lanes of a wave (xor shuffles: every lane gets the same bits)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// row of element r (0..15) of a 32x32 MFMA accumulator whose tile starts at row0, in the lanes 0-31; the lanes 32-63 hold
// row + 4.  The one part of this header that host code uses too (the packer lays a bias out in accumulator order).
__host__ __device__ __forceinline__ constexpr int acc_row(int row0, int r) { return row0 + (r & 3) + 8 * (r >> 2); }

// index i in [-(n - 1), 2n - 2] of a reflect-padded dimension of n >= 2 (torch 'reflect': the edge is not repeated) -> [0, n)
__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// ... for any i <= 3n - 2 too: the Winograd tiles that hang over the right / bottom edge read row 0 there (their outputs are dropped)
__device__ __forceinline__ int reflect_index_clamped(int i, int n) {
    const int r = reflect_index(i, n);
    return r < 0 ? 0 : r;
}

// two bf16 (round to nearest even) of two floats in one register: lo in bits 0-15
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// The 3-way bf16 split of a pair of fp32 values, a = a1 + a2 + a3 (the split-operand forms of k_igemm and k_wino_fused), in
// the two halves their K loops schedule as separate fillers.
// First half: plane 0 of the pair (returned); lo, hi become the residuals.
__device__ __forceinline__ unsigned split_bf16_first(float& lo, float& hi) {
    const unsigned w = cvt_pk_bf16(lo, hi);
    lo -= __builtin_bit_cast(float, w << 16);          // exact: the residual of a rounding to 8 bits fits fp32
    hi -= __builtin_bit_cast(float, w & 0xffff0000u);
    return w;
}
// Second half, on the residuals of the first: plane 1 (x) and plane 2 (y), the rounded second residual.
__device__ __forceinline__ u32x2 split_bf16_second(float lo, float hi) {
    const unsigned w = split_bf16_first(lo, hi);
    return u32x2{w, cvt_pk_bf16(lo, hi)};
}

}  // namespace ffr
