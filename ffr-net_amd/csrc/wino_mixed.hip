// Winograd convolution on maps whose side is not a multiple of 4, tiled EXACTLY with tiles of 4 and 3 outputs per dimension
// (14 = 4 + 4 + 3 + 3, 7 = 4 + 3) instead of padding to whole F(4x4) tiles (reference convolutions: the 3x3 / stride 1 / zero-padded
// convolutions of stage 3, pretrain/model_ir_se50.py:67,69).
//
// Four tile types (MR x MC outputs): F(4x4,3x3) with 6 x 6 = 36 xi, F(4x3) and F(3x4) with 30, F(3x3) with 5 x 5 = 25
// (interpolation points {0, 1, -1, 2, inf} for the 3-output dimension).  A 14x14 image is 4 tiles of each type = 484 xi-tiles
// instead of the 576 of 16 padded F(4x4) tiles.  A block stays what it is in k_wino_fused<0, 2> -- 32 tiles (of ONE type) x 64
// channels, every xi, wave w owning S consecutive xi -- with S = 9 / 8 / 8 / 7 slots per wave (30 and 25 xi are padded to 32 and
// 28 with zero weights), so a block of type (3,3) takes 7/9 of the K-loop time of a type (4,4) block.  All four types run in ONE
// launch, blocks ordered by type: with two blocks per CU (batch 256: 128 blocks per type on 256 CUs) the CUs that ran (4,3) take
// (3,4) and those that ran (4,4) take (3,3): 16 slots per CU where 16 padded F(4x4) tiles per image cost 18 (EXPERIMENTS.md, round 4).
//
//   k_wino_in_mixed    : X[N,H,W,pitch] --B_r^T d B_c--> V_type in the fragment order the GEMM streams, one region per type
//   k_wino_fused_mixed : per block M[xi] = V[xi] U[xi]^T on the fp32 matrix cores, A_r^T M A_c + bias (border class) + PReLU
//                        (+ residual, sigmoid, SE tile sums) -> out
// Both are the F(4x4) kernels of wino_fused.hip with other constants: the pieces they share are in wino_fused_core.h, the 5-point
// transforms beside the 6-point ones in wino_math.h.  Here: tile -> origin, the type dispatch, A_r^T M A_c and the full-tile stores.
#include "device_util.h"
#include "ffr_kernels.h"
#include "wino_fused_core.h"
#include "wino_math.h"

namespace ffr {

// tile t of type (MR, MC) -> image, origin of its outputs
template <int MR, int MC>
__device__ __forceinline__ void mixed_tile(const WinoMixedGeom& g, long long t, int* n, int* q, int* r0, int* c0) {
    const int nr = MR == 4 ? g.n4 : g.n3, nc = MC == 4 ? g.n4 : g.n3;
    const unsigned tpi = (unsigned)(nr * nc);           // t < 2^31 (checked by the launchers): 32-bit division
    *n = (int)((unsigned)t / tpi);
    *q = (int)((unsigned)t - (unsigned)*n * tpi);
    const int ai = *q / nc, bi = *q - ai * nc;
    *r0 = MR == 4 ? g.o4[ai] : g.o3[ai];
    *c0 = MC == 4 ? g.o4[bi] : g.o3[bi];
}

// ---- input transform ------------------------------------------------------------------------------------------
// grid (sum of the types' tile groups, cin_pad / 32); wave w of a block = K chunk 4 blockIdx.y + w; lane = (tile, k half)
template <int MR, int MC>
__device__ __forceinline__ void in_mixed_body(const WinoInMixedArgs& a, int tau, int mb) {
    constexpr int AR = MR + 2, AC = MC + 2, X = AR * AC, XP = (X + 3) / 4 * 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kc = blockIdx.y * 4 + wave;
    const int tl = lane >> 1, hh = lane & 1;
    const long long t = (long long)mb * 32 + tl;
    float* vout = wino_frag_ptr<XP>(a.V[tau], mb, a.nkc, kc, hh, tl);
    if (t >= a.T[tau]) { wino_frag_zero<XP>(vout); return; }
    int n, q, r0, c0;
    mixed_tile<MR, MC>(a.g, t, &n, &q, &r0, &c0);
    const float* xn = a.x + (size_t)n * a.H * a.W * a.pitch + kc * 8 + hh * 4;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 tmp[AR][AC];
#pragma unroll
    for (int j = 0; j < AC; ++j) {
        f32x4 d[AR], v[AR];
        const int wi = c0 - 1 + j;
        const bool okw = (unsigned)wi < (unsigned)a.W;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int hi = r0 - 1 + i;
            d[i] = zero4;
            if (okw && (unsigned)hi < (unsigned)a.H) d[i] = *reinterpret_cast<const f32x4*>(xn + ((size_t)hi * a.W + wi) * a.pitch);
        }
        btv<AR>(d, v);
#pragma unroll
        for (int i = 0; i < AR; ++i) tmp[i][j] = v[i];
    }
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        f32x4 v[AC];
        btv<AC>(tmp[i], v);
#pragma unroll
        for (int j = 0; j < AC; ++j) *reinterpret_cast<f32x4*>(vout + (i * AC + j) * 256) = v[j];
    }
#pragma unroll
    for (int e = X; e < XP; ++e) *reinterpret_cast<f32x4*>(vout + e * 256) = zero4;      // the padded xi (their weights are zero as well)
}

__global__ __launch_bounds__(256) void k_wino_in_mixed(const WinoInMixedArgs a) {
    const int b = blockIdx.x;
    const int tau = b >= a.goff[2] ? (b >= a.goff[3] ? 3 : 2) : (b >= a.goff[1] ? 1 : 0);
    const int mb = b - a.goff[tau];
    switch (tau) {
        case 0: in_mixed_body<4, 4>(a, 0, mb); break;
        case 1: in_mixed_body<4, 3>(a, 1, mb); break;
        case 2: in_mixed_body<3, 4>(a, 2, mb); break;
        default: in_mixed_body<3, 3>(a, 3, mb); break;
    }
}

// ---- bottleneck combine + input transform of the next conv1 (the mixed-tile form of k_combine_in_c) ---------------------
// x = res * scale[n] + shortcut (pretrain/model_ir_se50.py:73-76) is written as the next unit's shortcut (NHWC `out`) and,
// transformed, as the V of the next unit's conv1.  A block owns 2 images x 32 channels of a 14x14 map: it reads res and the
// shortcut once with full 128-byte lines, writes `out` the same way and keeps x in LDS (50 KB); then WAVE w transforms the 8
// tiles of type w (2 images x 4 tiles) -- no divergence inside a wave, four code paths per block.
// grid (ceil(N / 2), C / 32).
constexpr int CIM_PX = 2 * 14 * 14;
template <int MR, int MC>
__device__ __forceinline__ void combine_mixed_tiles(const WinoInMixedArgs& a, const float* s_x, int n_first, int n_imgs) {
    constexpr int AR = MR + 2, AC = MC + 2, XP = (AR * AC + 3) / 4 * 4, TAU = 2 * (MR == 3) + (MC == 3);
    const int lane = threadIdx.x & 63;
    const int tile = lane >> 3, quad = lane & 7;            // 8 tiles (2 images x 4 of this type), 4-channel quad of the block's 32
    const int il = tile >> 2, q = tile & 3;
    const int kc = blockIdx.y * 4 + (quad >> 1), hf = quad & 1;
    const int t = (n_first + il) * 4 + q;                   // tile index within the type: 4 tiles per image
    float* vout = wino_frag_ptr<XP>(a.V[TAU], t >> 5, a.nkc, kc, hf, t & 31);
    if (blockIdx.x == gridDim.x - 1) {
        // the rows of the last 32-tile group behind this block's two images: zero, as k_wino_in_mixed leaves them
        const int t_end = (int)((a.T[TAU] + 31) / 32) * 32;
        for (int tz = (n_first + 2) * 4 + tile; tz < t_end; tz += 8) wino_frag_zero<XP>(wino_frag_ptr<XP>(a.V[TAU], tz >> 5, a.nkc, kc, hf, tz & 31));
    }
    if (il >= n_imgs) { wino_frag_zero<XP>(vout); return; }
    const int ai = q >> 1, bi = q & 1;
    const int r0 = MR == 4 ? a.g.o4[ai] : a.g.o3[ai], c0 = MC == 4 ? a.g.o4[bi] : a.g.o3[bi];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float* xb = s_x + il * (14 * 14) * 32 + quad * 4;
    f32x4 d[AR][AC];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        const int hi = r0 - 1 + i;
        const bool okh = (unsigned)hi < 14u;
#pragma unroll
        for (int j = 0; j < AC; ++j) {
            const int wi = c0 - 1 + j;
            d[i][j] = zero4;
            if (okh && (unsigned)wi < 14u) d[i][j] = *reinterpret_cast<const f32x4*>(xb + (hi * 14 + wi) * 32);
        }
    }
    wino_patch_to_frags<AR, AC>(d, vout);
}

__global__ __launch_bounds__(256) void k_combine_in_mixed(const float* __restrict__ res, const float* __restrict__ scale,
                                                         const float* __restrict__ sh, float* __restrict__ out,
                                                         const WinoInMixedArgs a, int C) {
    __shared__ __attribute__((aligned(16))) float s_x[CIM_PX * 32];
    const int wave = threadIdx.x >> 6;
    const int n_first = blockIdx.x * 2;
    const int n_imgs = a.N - n_first < 2 ? a.N - n_first : 2;
    combine_to_lds(res, scale, sh, out, s_x, n_first, n_imgs * 14 * 14, 14 * 14, C, blockIdx.y * 32);      // phase 1
    __syncthreads();
    switch (wave) {         // phase 2: one tile type per wave
        case 0: combine_mixed_tiles<4, 4>(a, s_x, n_first, n_imgs); break;
        case 1: combine_mixed_tiles<4, 3>(a, s_x, n_first, n_imgs); break;
        case 2: combine_mixed_tiles<3, 4>(a, s_x, n_first, n_imgs); break;
        default: combine_mixed_tiles<3, 3>(a, s_x, n_first, n_imgs); break;
    }
}

// ---- weights of the tile types (4,3), (3,4), (3,3): U = G_r g G_c^T from the packed direct weights, on the device ----------
// (round 5: these three sets -- 24-48 MB per layer, 0.7 GB per handle -- were packed by the host at load time whether or not a
// batch that uses them ever arrived; now the engine derives them from W[cout_pad][9][cin_pad] (BatchNorm already folded) the
// first time a launch is eligible: pack.cpp, prepare_mixed_weights.)  One thread per (output channel, input channel); fp64
// arithmetic, rounded once.  Output in fragment order [cout_pad/64][K chunk][XP][128 pieces][4]; padded xi stay zero (memset).
__global__ __launch_bounds__(256) void k_wino_weights_mixed(const float* __restrict__ w, float* __restrict__ um, int cout_pad, int cin_pad,
                                                           int mr, int mc, int xp) {
    const double G4[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                             {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    const double G3[5][3] = {{0.5, 0, 0}, {-0.5, -0.5, -0.5}, {-1.0 / 6, 1.0 / 6, -1.0 / 6}, {1.0 / 6, 1.0 / 3, 2.0 / 3}, {0, 0, 1}};
    const int ci = blockIdx.x * 256 + threadIdx.x, co = blockIdx.y;
    if (ci >= cin_pad) return;
    double g[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = (double)w[((size_t)co * 9 + t) * cin_pad + ci];
    const int ar = mr + 2, ac = mc + 2, nkc = cin_pad / 8;
    const int nb = co >> 6, nl = co & 63;
    const int kc = ci >> 3, hf = (ci & 7) >> 2, e4 = ci & 3;
    const int piece = (nl >> 5) * 64 + hf * 32 + (nl & 31);
    float* dst = um + (((size_t)nb * nkc + kc) * xp * 128 + piece) * 4 + e4;
    for (int i = 0; i < ar; ++i) {
        const double* gr = mr == 4 ? G4[i] : G3[i];
        double tmp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) tmp[c] = gr[0] * g[0 * 3 + c] + gr[1] * g[1 * 3 + c] + gr[2] * g[2 * 3 + c];
        for (int j = 0; j < ac; ++j) {
            const double* gc = mc == 4 ? G4[j] : G3[j];
            dst[(size_t)(i * ac + j) * 512] = (float)(tmp[0] * gc[0] + tmp[1] * gc[1] + tmp[2] * gc[2]);
        }
    }
}

// ---- geometry / sizes (host) -------------------------------------------------------------------------------------
bool wino_mixed_geom(int H, int W, WinoMixedGeom* g) {
    if (H != W) return false;
    if (H == 14) { *g = WinoMixedGeom{2, {0, 4}, 2, {8, 11}}; return true; }
    if (H == 7) { *g = WinoMixedGeom{1, {0, 0}, 1, {4, 0}}; return true; }
    return false;
}

static const int MIXED_MR[4] = {4, 4, 3, 3}, MIXED_MC[4] = {4, 3, 4, 3};
int wino_mixed_xp(int tau) { return ((MIXED_MR[tau] + 2) * (MIXED_MC[tau] + 2) + 3) / 4 * 4; }
int wino_mixed_x(int tau) { return (MIXED_MR[tau] + 2) * (MIXED_MC[tau] + 2); }

// tiles and 32-tile groups per type; floats of the four V regions together
void wino_mixed_counts(const WinoMixedGeom& g, int N, long long T[4], int groups[4]) {
    for (int tau = 0; tau < 4; ++tau) {
        const int nr = MIXED_MR[tau] == 4 ? g.n4 : g.n3, nc = MIXED_MC[tau] == 4 ? g.n4 : g.n3;
        T[tau] = (long long)N * nr * nc;
        groups[tau] = (int)((T[tau] + 31) / 32);
    }
}
size_t wino_mixed_v_floats(const WinoMixedGeom& g, int N, int cin_pad, size_t off[4]) {
    long long T[4]; int groups[4];
    wino_mixed_counts(g, N, T, groups);
    size_t tot = 0;
    for (int tau = 0; tau < 4; ++tau) {
        if (off) off[tau] = tot;
        tot += (size_t)groups[tau] * 32 * wino_mixed_xp(tau) * cin_pad;
    }
    return tot;
}

hipError_t launch_wino_in_mixed(const float* x, float* V, int N, int H, int W, int pitch, int cin_pad, hipStream_t stream) {
    WinoInMixedArgs a{};
    if (cin_pad % 32 || !wino_mixed_geom(H, W, &a.g)) return hipErrorInvalidValue;
    a.x = x; a.N = N; a.H = H; a.W = W; a.pitch = pitch; a.nkc = cin_pad / 8;
    size_t off[4];
    wino_mixed_v_floats(a.g, N, cin_pad, off);
    int groups[4];
    wino_mixed_counts(a.g, N, a.T, groups);
    int tot = 0;
    for (int tau = 0; tau < 4; ++tau) { a.V[tau] = V + off[tau]; a.goff[tau] = tot; tot += groups[tau]; }
    hipLaunchKernelGGL(k_wino_in_mixed, dim3(tot, cin_pad / 32), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// res * scale + shortcut -> out (NHWC, C channels) and its mixed-tile transform V (the layout launch_wino_in_mixed writes); 14x14 only
hipError_t launch_combine_in_mixed(const float* res, const float* scale, const float* sh, float* out, float* V, int N, int H, int W,
                                   int C, hipStream_t stream) {
    WinoInMixedArgs a{};
    if (H != 14 || W != 14 || C % 32 || !wino_mixed_geom(H, W, &a.g)) return hipErrorInvalidValue;
    a.x = nullptr; a.N = N; a.H = H; a.W = W; a.pitch = C; a.nkc = C / 8;
    size_t off[4];
    wino_mixed_v_floats(a.g, N, C, off);
    int groups[4];
    wino_mixed_counts(a.g, N, a.T, groups);
    for (int tau = 0; tau < 4; ++tau) a.V[tau] = V + off[tau];
    hipLaunchKernelGGL(k_combine_in_mixed, dim3((N + 1) / 2, C / 32), dim3(256), 0, stream, res, scale, sh, out, a, C);
    return hipGetLastError();
}

// ---- the fused GEMM + output transform -----------------------------------------------------------------------------
constexpr int WM_LDS_BYTES = (WF_EPI_FLOATS + 9 * 64 + 32 * 8) * 4;      // E + bias table + tile table

template <int MR, int MC>
__device__ __forceinline__ void fused_mixed_body(const WinoMixedArgs& a, int tau, int mb, int nb, float* smem) {
    constexpr int AR = MR + 2, AC = MC + 2, X = AR * AC, S = (X + 3) / 4, XP = 4 * S, NT = 2;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tid = threadIdx.x;
    const ConvTail& e = a.tail;
    const int nkc = a.nkc;
    const int n0 = nb * 64;
    unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, sr0 = 0;      // trace build (option wf_trace): shader-clock stamps of the phases
    if (FFR_TRACE_ON(a.trace)) { st0 = __builtin_amdgcn_s_memtime(); sr0 = __builtin_amdgcn_s_memrealtime(); }
    float* const s_bias = smem + WF_EPI_FLOATS;
    int* const s_tile = reinterpret_cast<int*>(s_bias + 9 * 64);     // [4]: tile-sum slot
    wf_fill_bias<NT>(s_bias, e.bias, e.border_bias, e.cout_pad, n0);
    if (tid < 32) {
        const long long t = (long long)mb * 32 + tid;
        const bool valid = t < a.T[tau];
        int n = 0, q = 0, r0 = 0, c0 = 0;
        if (valid) mixed_tile<MR, MC>(a.g, t, &n, &q, &r0, &c0);
        wf_tile_record(s_tile + tid * 8, valid, n, r0, c0, MR, MC, a.H, a.W);
        // tile-sum slot: image n owns tpi_total consecutive slots, the tile types in the order (4,4), (4,3), (3,4), (3,3) (tpi_off),
        // the tiles of a type in raster order of that type's own grid (q).  plan_conv sends only whole channel quads here
        // (cout_store % 4 == 0), so a quad is stored and summed entirely or not at all (its sums are 0): ConvTail::tile_sums
        s_tile[tid * 8 + 4] = valid ? n * a.tpi_total + a.tpi_off[tau] + q : 0;
    }
    f32x16 acc[8][NT], accv[NT];
    wf_zero_acc<NT>(acc, accv);
    wf_vfed_gemm<S, NT>(a.V[tau], a.U[tau], mb, nb, nkc, e.cout_pad, wave, lane, acc, accv, a.trace, st1);
    if (FFR_TRACE_ON(a.trace)) st2 = __builtin_amdgcn_s_memtime();

    // ---- epilogue: two passes of 32 channels through E[xi][tile][32] in LDS (as k_wino_fused), transforms per tile type ----
    if (S == 9) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    const int cq = lane & 7;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        wf_stage_acc<S, X, NT>(smem, wave, lane, nt, acc, accv);
        __syncthreads();
        const int tl = (lane >> 3) + 8 * wave;
        if (s_tile[tl * 8 + 1] != 0) {                                  // else: tile beyond T
            const int pix0 = s_tile[tl * 8 + 0];
            const f32x4* ev = wf_staged(smem, tl, cq);
            f32x4 tmp[MR][AC];
#pragma unroll
            for (int j = 0; j < AC; ++j) {
                f32x4 mc[AR], yc[MR];
#pragma unroll
                for (int i = 0; i < AR; ++i) mc[i] = ev[(i * AC + j) * 256];
                atq<AR>(mc, yc);
#pragma unroll
                for (int i = 0; i < MR; ++i) tmp[i][j] = yc[i];
            }
            const int cl = nt * 32 + 4 * cq;
            const int cg = n0 + cl;
            const f32x4 slope = tail_slope4(e.slope, cg);
            int rc[MR], cc[MC];
            if (e.border_bias) {
                wf_border_offsets(s_tile[tl * 8 + 2], 3 * 64, rc);
                wf_border_offsets(s_tile[tl * 8 + 3], 64, cc);
            } else {
#pragma unroll
                for (int i = 0; i < MR; ++i) rc[i] = 0;
#pragma unroll
                for (int i = 0; i < MC; ++i) cc[i] = 0;
            }
            f32x4 psum = {0.f, 0.f, 0.f, 0.f};
            if (cg + 3 < e.cout_store) {
                float* const ob = e.out + (size_t)pix0 * e.out_pitch + e.out_coff + cg;
                const float* const rb = e.resid ? e.resid + (size_t)pix0 * e.res_pitch + cg : nullptr;
#pragma unroll
                for (int i = 0; i < MR; ++i) {
                    f32x4 yr[MC];
                    atq<AC>(tmp[i], yr);
#pragma unroll
                    for (int jj = 0; jj < MC; ++jj) {
                        const f32x4 v = tail4<PRELU_MINMAX>(yr[jj], *reinterpret_cast<const f32x4*>(s_bias + rc[i] + cc[jj] + cl), slope, rb != nullptr,
                                                            [&] { return *reinterpret_cast<const f32x4*>(rb + (size_t)(i * a.W + jj) * e.res_pitch); }, e.flags);
                        *reinterpret_cast<f32x4*>(ob + (size_t)(i * a.W + jj) * e.out_pitch) = v;
                        psum += v;
                    }
                }
            }
            if (e.tile_sums) tail_store_tile_sum(e.tile_sums, s_tile[tl * 8 + 4], e.cout_pad, cg, psum);
        }
        __syncthreads();
        if (FFR_TRACE_ON(a.trace) && nt == 0) st3 = __builtin_amdgcn_s_memtime();
    }
    if (FFR_TRACE_ON(a.trace) && threadIdx.x == 0) {
        unsigned long long* tr = a.trace + (size_t)blockIdx.x * 12;
        unsigned xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        tr[0] = st0; tr[1] = st1; tr[2] = st2; tr[3] = st3; tr[4] = __builtin_amdgcn_s_memtime();
        tr[5] = sr0; tr[6] = __builtin_amdgcn_s_memrealtime();
        tr[7] = ((unsigned long long)(xcc & 0xf) << 8) | ((hwid >> 8) & 0xff);     // XCD | (SE, SH, CU): one key per CU
        tr[8] = (unsigned long long)tau; tr[9] = 1;
    }
}

__global__ __launch_bounds__(256, 1) void k_wino_fused_mixed(const WinoMixedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // The XCDs specialise in PAIRS of tile types.  Blocks b and b + 8 share an XCD (round-robin dispatch); XCDs 0-3 run
    // (4,4) in the first half of the grid and (3,3) in the second, XCDs 4-7 run (4,3) then (3,4): every CU pairs a long block
    // with a short one (9 + 7 = 8 + 8 slots), and an XCD's L2 streams TWO weight sets per launch instead of four (268 -> 134 MB of
    // the 405 MB a 256 -> 256 launch fetched with the types in four consecutive ranges, where every XCD read all four sets once:
    // EXPERIMENTS.md, round 5).  Inside a type: tile groups round-robin over the four XCDs of its pair, the channel groups of a
    // tile group next to each other on one XCD (V from that L2).
    const int half = blockIdx.x >= a.half_blocks;       // half_blocks is a multiple of 8
    const int bl = blockIdx.x - (half ? a.half_blocks : 0);
    const int xcd = bl & 7, idx = bl >> 3;
    const int tau = xcd < 4 ? (half ? 3 : 0) : (half ? 2 : 1);
    const int nb = idx % a.nbn, mb = (idx / a.nbn) * 4 + (xcd & 3);
    if (mb >= a.mbn[tau]) return;
    switch (tau) {
        case 0: fused_mixed_body<4, 4>(a, 0, mb, nb, smem); break;
        case 1: fused_mixed_body<4, 3>(a, 1, mb, nb, smem); break;
        case 2: fused_mixed_body<3, 4>(a, 2, mb, nb, smem); break;
        default: fused_mixed_body<3, 3>(a, 3, mb, nb, smem); break;
    }
}

hipError_t wino_mixed_init() {
    return hipFuncSetAttribute((const void*)k_wino_fused_mixed, hipFuncAttributeMaxDynamicSharedMemorySize, WM_LDS_BYTES);
}

// a.V[0] = base of the four V regions (laid out by wino_mixed_v_floats), a.U[tau] set by the caller
hipError_t launch_wino_fused_mixed(WinoMixedArgs a, hipStream_t stream) {
    const ConvTail& e = a.tail;
    if (e.cout_pad % 64 || a.nkc < 2 || !wino_mixed_geom(a.H, a.W, &a.g)) return hipErrorInvalidValue;
    if (((e.out_pitch | e.out_coff | e.res_pitch | e.cout_store) & 3) != 0) return hipErrorInvalidValue;
    size_t off[4];
    wino_mixed_v_floats(a.g, a.N, a.nkc * 8, off);
    wino_mixed_counts(a.g, a.N, a.T, a.mbn);
    a.nbn = e.cout_pad / 64;
    const float* vbase = a.V[0];
    int tpi = 0;
    for (int tau = 0; tau < 4; ++tau) {
        a.V[tau] = vbase + off[tau];
        const int nr = MIXED_MR[tau] == 4 ? a.g.n4 : a.g.n3, nc = MIXED_MC[tau] == 4 ? a.g.n4 : a.g.n3;
        a.tpi_off[tau] = tpi;
        tpi += nr * nc;
    }
    a.tpi_total = tpi;
    const int tot = wino_mixed_blocks_launched(a.N, a.H, a.W, e.cout_pad);
    a.half_blocks = tot / 2;
    hipLaunchKernelGGL(k_wino_fused_mixed, dim3(tot), dim3(256), WM_LDS_BYTES, stream, a);
    return hipGetLastError();
}

// grid size of launch_wino_fused_mixed: two halves of 8 * ceil(groups / 4) * nbn blocks (every type has the same number of tile
// groups on a square map, n4 * n3 tiles per image each way; a pair of types shares the four XCDs of its quad)
int wino_mixed_blocks_launched(int N, int H, int W, int cout_pad) {
    WinoMixedGeom g;
    if (!wino_mixed_geom(H, W, &g)) return 0;
    long long T[4]; int groups[4];
    wino_mixed_counts(g, N, T, groups);
    int gmax = 0;
    for (int tau = 0; tau < 4; ++tau) gmax = groups[tau] > gmax ? groups[tau] : gmax;
    return 2 * ((gmax + 3) / 4 * 8 * (cout_pad / 64));
}

size_t wino_mixed_u_floats(int tau, int cout_pad, int cin_pad) { return (size_t)(cout_pad / 64) * (cin_pad / 8) * wino_mixed_xp(tau) * 512; }

// um (wino_mixed_u_floats(tau, ..) floats, device) <- the weights of tile type tau in [1, 3] from the packed direct weights w
hipError_t launch_wino_weights_mixed(const float* w, float* um, int cout_pad, int cin_pad, int tau, hipStream_t stream) {
    if (tau < 1 || tau > 3 || cout_pad % 64 || cin_pad % 32) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(um, 0, wino_mixed_u_floats(tau, cout_pad, cin_pad) * sizeof(float), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_wino_weights_mixed, dim3((cin_pad + 255) / 256, cout_pad), dim3(256), 0, stream, w, um, cout_pad, cin_pad,
                       MIXED_MR[tau], MIXED_MC[tau], wino_mixed_xp(tau));
    return hipGetLastError();
}

int wino_mixed_blocks(int N, int H, int W, int cout_pad) {
    WinoMixedGeom g;
    if (!wino_mixed_geom(H, W, &g)) return 0;
    long long T[4]; int groups[4];
    wino_mixed_counts(g, N, T, groups);
    int tot = 0;
    for (int tau = 0; tau < 4; ++tau) tot += groups[tau] * (cout_pad / 64);
    return tot;
}

}  // namespace ffr
