// align.hip -- face alignment on the device: five (K) landmarks per face -> similarity transform -> aligned uint8 crop
// (include/ffrnet.h, ffr_align_transforms / ffr_align_warp / ffr_embed_aligned).  Replaces the host path of the
// reference, lfw/gen_lfw112x96.py:6-17 (align) with lfw/matlab_cp2tform.py:223-432 (findNonreflectiveSimilarity,
// findSimilarity) in front of cv2.warpAffine.
//
// k_align_tfm   one thread per face, fp64.  The reference solves the least squares of the map template -> landmarks
//               (crop -> frame) and hands cv2 its inverse; the warp needs dst -> src, which is that solution itself, so no
//               matrix is inverted for the result.  With p = r - mean(r) (template), q = s - mean(s) (landmarks),
//               den = sum |p|^2:  a = sum(p . q) / den,  b = sum(p x q) / den,  A1 = [a -b tx; b a ty],
//               t = mean(s) - L mean(r).  The reflective candidate A2 is the same fit with r.x negated and the first
//               column of the result negated.  Each candidate's inverse maps the landmarks into the crop; the L2 norm
//               of the residual against the template decides, the non-reflective one winning when norm1 <= norm2
//               (matlab_cp2tform.py:421-432).  A candidate whose linear part is exactly singular has no inverse and an
//               infinite norm.  valid = 0 and A = 0 when den == 0, when both candidates are singular (all landmarks
//               equal) or when anything is not finite -- the cases in which the reference raises.  With a frame_index
//               (ffr_embed_aligned) a face whose frame is outside [0,F) is invalid as well.
//               The reference's `xyR = xy` (matlab_cp2tform.py:407) is an alias, so it takes both norms against the mirrored
//               template.  With n = a^2 + b^2 of each candidate, both its comparison and the one above reduce to
//               n1 >= n2 whenever sum |q|^2 > 2 den (a1 a2 + b1 b2), which holds for landmarks that a similarity nearly
//               relates: all 256 cases of golden G13 agree (near-ties are not in it); on 3000 random point sets that no
//               similarity relates the two part in 2 % of the draws, exactly those where the inequality fails.
// k_align_warp  the crop by an exact integer bilinear rule in cv2's manner (1/32-pixel sampling grid, constant-0 border);
//               NOT claimed equal to cv2.warpAffine, whose fixed-point coordinate walk differs:
//                 sx = (A0 x + A1 y) + A2,  sy = (A3 x + A4 y) + A5     fp64, in this order, no contraction, clamped
//                                                                        to +-2^20 (fmin(fmax()): a NaN goes to -2^20)
//                 fx = (int)floor(sx * 32 + 0.5),  ix = fx >> 5,  ax = fx & 31   (the same for y)
//                 v  = (sum of w p over the 4 taps + 512) >> 10  per channel, w = (32-ax)(32-ay), ax(32-ay),
//                      (32-ax)ay, ax ay; a tap outside [0,W) x [0,H) contributes 0, decided per tap.
//               A face with valid == 0 or a frame_index outside [0,F) gets zeros.
//  - Grid (face, band of rows); a block is (out_w / 4) x rows threads, lanes along x, so at small rotations neighbouring
//    lanes read neighbouring source bytes; the six coefficients, the frame base and the face's flags are block-uniform.
//  - A thread makes 4 adjacent pixels = 12 bytes and writes them as three dword vector stores (out_w % 4 == 0 and a
//    4-byte aligned crop keep every store aligned).
//  - Taps are byte loads at coordinates clamped into the frame, with the weight of an outside tap set to 0: every address
//    is in bounds whatever A holds.  Frame bases are 64-bit, offsets inside a frame 32-bit (host check: pitch*H < 2^31).
//  - No LDS: the kernel is a gather with 9.6 MB of output at 256 faces (measured: profiles/align_bench.json).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "device_util.h"
#include "ffr_kernels.h"

namespace ffr {

namespace {

constexpr int AL_MAX_K = 16;

// residual norm of landmarks mapped back by the inverse of L = [a -b; b a] against the points (sgn * p.x, p.y)
__device__ __forceinline__ double tfm_resid(const float* s, const float* r, int K, double msx, double msy, double mrx,
                                            double mry, double a, double b, double sgn) {
    const double n = a * a + b * b;
    if (!(n > 0.0)) return INFINITY;
    double acc = 0.0;
    for (int i = 0; i < K; ++i) {
        const double qx = (double)s[2 * i] - msx, qy = (double)s[2 * i + 1] - msy;
        const double px = sgn * ((double)r[2 * i] - mrx), py = (double)r[2 * i + 1] - mry;
        const double ex = (a * qx + b * qy) / n - px, ey = (a * qy - b * qx) / n - py;
        acc += ex * ex + ey * ey;
    }
    return sqrt(acc);
}

__global__ __launch_bounds__(64) void k_align_tfm(const float* __restrict__ lm, const float* __restrict__ tmpl, int N, int K,
                                                  const int* __restrict__ frame_index, int F, double* __restrict__ A,
                                                  uint8_t* __restrict__ valid) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float* s = lm + (size_t)n * K * 2;
    double msx = 0.0, msy = 0.0, mrx = 0.0, mry = 0.0;
    for (int i = 0; i < K; ++i) {
        msx += (double)s[2 * i]; msy += (double)s[2 * i + 1];
        mrx += (double)tmpl[2 * i]; mry += (double)tmpl[2 * i + 1];
    }
    msx /= K; msy /= K; mrx /= K; mry /= K;
    double den = 0.0, dot = 0.0, crs = 0.0, dot2 = 0.0, crs2 = 0.0;
    for (int i = 0; i < K; ++i) {
        const double qx = (double)s[2 * i] - msx, qy = (double)s[2 * i + 1] - msy;
        const double px = (double)tmpl[2 * i] - mrx, py = (double)tmpl[2 * i + 1] - mry;
        den += px * px + py * py;
        dot += px * qx + py * qy;   crs += px * qy - py * qx;
        dot2 += py * qy - px * qx;  crs2 += -px * qy - py * qx;      // the same with p.x negated
    }
    const double a1 = dot / den, b1 = crs / den, a2 = dot2 / den, b2 = crs2 / den;
    const double n1 = tfm_resid(s, tmpl, K, msx, msy, mrx, mry, a1, b1, 1.0);
    const double n2 = tfm_resid(s, tmpl, K, msx, msy, mrx, mry, a2, b2, -1.0);
    double o[6];
    if (n1 <= n2) {
        o[0] = a1; o[1] = -b1; o[2] = msx - (a1 * mrx - b1 * mry);
        o[3] = b1; o[4] = a1;  o[5] = msy - (b1 * mrx + a1 * mry);
    } else {
        o[0] = -a2; o[1] = -b2; o[2] = msx - (-a2 * mrx - b2 * mry);
        o[3] = -b2; o[4] = a2;  o[5] = msy - (-b2 * mrx + a2 * mry);
    }
    bool ok = den > 0.0 && (isfinite(n1) || isfinite(n2));
    if (frame_index) ok = ok && frame_index[n] >= 0 && frame_index[n] < F;
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(o[k]);
    for (int k = 0; k < 6; ++k) A[(size_t)n * 6 + k] = ok ? o[k] : 0.0;
    valid[n] = ok ? 1 : 0;
}

// source coordinate of an output pixel on the 1/32 grid
__device__ __forceinline__ int warp_coord(double c0, double c1, double c2, double x, double y) {
#pragma clang fp contract(off)
    double v = (c0 * x + c1 * y) + c2;
    v = fmin(fmax(v, -1048576.0), 1048576.0);
    return (int)floor(v * 32.0 + 0.5);
}

__global__ __launch_bounds__(256) void k_align_warp(const uint8_t* __restrict__ frames, int F, int H, int W, int pitch,
                                                    const int* __restrict__ frame_index, const double* __restrict__ A,
                                                    const uint8_t* __restrict__ valid, int oh, int ow,
                                                    uint8_t* __restrict__ crop) {
    const int face = blockIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int x0 = threadIdx.x * 4;
    if (y >= oh) return;
    uint32_t* out = reinterpret_cast<uint32_t*>(crop + (((size_t)face * oh + y) * ow + x0) * 3);
    const int fi = frame_index[face];
    const bool live = (valid == nullptr || valid[face] != 0) && fi >= 0 && fi < F;
    if (!live) {
        out[0] = 0u; out[1] = 0u; out[2] = 0u;
        return;
    }
    const double* Af = A + (size_t)face * 6;
    const double c0 = Af[0], c1 = Af[1], c2 = Af[2], c3 = Af[3], c4 = Af[4], c5 = Af[5];
    const uint8_t* src = frames + (size_t)fi * ((size_t)pitch * (size_t)H);
    uint32_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int fx = warp_coord(c0, c1, c2, (double)(x0 + j), (double)y);
        const int fy = warp_coord(c3, c4, c5, (double)(x0 + j), (double)y);
        const int ix = fx >> 5, ax = fx & 31, iy = fy >> 5, ay = fy & 31;
        const bool inx0 = (unsigned)ix < (unsigned)W, inx1 = (unsigned)(ix + 1) < (unsigned)W;
        const bool iny0 = (unsigned)iy < (unsigned)H, iny1 = (unsigned)(iy + 1) < (unsigned)H;
        const uint32_t w00 = inx0 && iny0 ? (uint32_t)((32 - ax) * (32 - ay)) : 0u;
        const uint32_t w01 = inx1 && iny0 ? (uint32_t)(ax * (32 - ay)) : 0u;
        const uint32_t w10 = inx0 && iny1 ? (uint32_t)((32 - ax) * ay) : 0u;
        const uint32_t w11 = inx1 && iny1 ? (uint32_t)(ax * ay) : 0u;
        const int xa = min(max(ix, 0), W - 1) * 3, xb = min(max(ix + 1, 0), W - 1) * 3;
        const int ya = min(max(iy, 0), H - 1) * pitch, yb = min(max(iy + 1, 0), H - 1) * pitch;
        const uint8_t *p00 = src + (ya + xa), *p01 = src + (ya + xb), *p10 = src + (yb + xa), *p11 = src + (yb + xb);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            px[3 * j + c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 512u) >> 10;
    }
    out[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    out[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    out[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
}

}  // namespace

hipError_t launch_align_tfm(const float* landmarks, const float* tmpl, int N, int K, const int* frame_index, int F, double* A,
                            uint8_t* valid, hipStream_t stream) {
    if (N <= 0 || K < 2 || K > AL_MAX_K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_tfm, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, landmarks, tmpl, N, K,
                       frame_index, F, A, valid);
    return hipGetLastError();
}

hipError_t launch_align_warp(const uint8_t* frames, int F, int H, int W, int pitch, const int* frame_index, const double* A,
                             const uint8_t* valid, int N, int oh, int ow, uint8_t* crop, hipStream_t stream) {
    if (N <= 0 || oh < 1 || oh > 256 || ow < 4 || ow > 256 || (ow & 3) || F < 1 || H < 1 || W < 1 || pitch < 3 * W ||
        (long long)pitch * H >= (1ll << 31) || ((uintptr_t)crop & 3))
        return hipErrorInvalidValue;
    const int tx = ow / 4;
    int ty = 256 / tx < oh ? 256 / tx : oh;
    for (int d = ty; 2 * d > ty; --d)             // a row count that divides out_h leaves no idle rows in the last band
        if (oh % d == 0) { ty = d; break; }
    hipLaunchKernelGGL(k_align_warp, dim3((unsigned)N, (unsigned)((oh + ty - 1) / ty)), dim3(tx, ty), 0, stream, frames, F, H,
                       W, pitch, frame_index, A, valid, oh, ow, crop);
    return hipGetLastError();
}

}  // namespace ffr
