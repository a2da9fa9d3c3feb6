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

}  // namespace ffr
