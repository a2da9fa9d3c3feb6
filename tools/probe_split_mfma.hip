// Probe (gfx950): fp32 products on the bf16 matrix cores through 3-way split operands.
//
//   hipcc --offload-arch=gfx950 -O3 tools/probe_split_mfma.hip -o build/probe_split_mfma && build/probe_split_mfma
//
// An fp32 value is split a = a1 + a2 + a3 with a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2) (round to nearest
// even: |a2| <= 2^-9 |a|, |a3| <= 2^-18 |a|); a*b is the sum of the products ai*bj, each exact in fp32, accumulated by
// v_mfma_f32_32x32x16_bf16.  Products kept: 6 (i + j <= 4), 8 (+ a2*b3, a3*b2) or 9.
//
//  (a) accuracy: C[32][32] = A[32][4608] * B[4608][32] per wave, against float64 on the host, beside the same product on
//      v_mfma_f32_32x32x2_f32.  Data: N(0,1); and N(0,1) with a per-k scale 10^U(-1.5, 1.5) on each operand (channel scales
//      over three decades, as the 'trained' weight family of synth.py has them).  Error: max |c - ref| / max |ref|, and the
//      same against sum |a||b| (the bound of SURVEY / cdna notes for the fp32 MFMA chain).
//      The small products go FIRST within a k-step (ascending magnitude), as k_igemm's split form issues them.
//  (b) rate: the product loop of one 64x64 wave tile per K = 16 step, operands in registers, one wave per SIMD, 512 blocks:
//      32 x 32x32x2 (fp32)  against  4 tiles x {6, 8, 9} x 32x32x16 bf16 with the split of the 16 A values per lane (the B
//      planes come pre-split) beside them; also without the split VALU.  Reported: cycles per step, the in-kernel shader
//      clock (d s_memtime / d s_memrealtime x 100 MHz) and fp32-equivalent TFLOP/s by wall.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
#define PIN __builtin_amdgcn_sched_barrier(0)

struct Planes { bf16x8 p[3]; };

__device__ __forceinline__ Planes split3(const float* v) {
    Planes o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h1 = (__bf16)v[e];
        const float r1 = v[e] - (float)h1;
        const __bf16 h2 = (__bf16)r1;
        const float r2 = r1 - (float)h2;
        o.p[0][e] = h1; o.p[1][e] = h2; o.p[2][e] = (__bf16)r2;
    }
    return o;
}

// product list, small terms first: (i, j) plane indices of A and B
template <int NP> struct Prod;
template <> struct Prod<6> { static constexpr int n = 6; static constexpr int ij[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}}; };
template <> struct Prod<8> { static constexpr int n = 8; static constexpr int ij[8][2] = {{2, 1}, {1, 2}, {2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}}; };
template <> struct Prod<9> { static constexpr int n = 9; static constexpr int ij[9][2] = {{2, 2}, {2, 1}, {1, 2}, {2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}}; };

// ---- (a) accuracy: one wave per block, block b multiplies problem b ---------------------------------------------------
// A [nprob][32][K], Bt [nprob][32][K] (column-major B), C [nprob][32][32] (row-major)
template <int NP>
__global__ __launch_bounds__(64) void k_dot(const float* __restrict__ A, const float* __restrict__ Bt, float* __restrict__ C, int K) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const float* a = A + ((size_t)blockIdx.x * 32 + r) * K;
    const float* b = Bt + ((size_t)blockIdx.x * 32 + r) * K;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if constexpr (NP == 0) {
        for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k + h], b[k + h], acc, 0, 0, 0);
    } else {
        for (int k = 0; k < K; k += 16) {
            const Planes pa = split3(a + k + 8 * h), pb = split3(b + k + 8 * h);
#pragma unroll
            for (int q = 0; q < Prod<NP>::n; ++q)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa.p[Prod<NP>::ij[q][0]], pb.p[Prod<NP>::ij[q][1]], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) C[((size_t)blockIdx.x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
}

// ---- (b) rate ----------------------------------------------------------------------------------------------------------
// NP 0: fp32 MFMAs; else NP bf16 products per tile.  VALU: split the A values of every step in registers
template <int NP, bool VALU>
__global__ __launch_bounds__(256, 1) void k_rate(const float* __restrict__ src, int steps, unsigned long long* __restrict__ stamps,
                                                 float* __restrict__ sink) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float av[2][8], bv[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { av[i][e] = src[(i * 8 + e) * 256 + threadIdx.x]; bv[i][e] = src[(16 + i * 8 + e) * 256 + threadIdx.x]; }
    Planes pb[2] = {split3(bv[0]), split3(bv[1])}, pa[2] = {split3(av[0]), split3(av[1])};
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    unsigned long long t0 = 0, r0 = 0;
    if (lane == 0) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        if constexpr (NP == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
        } else {
            if constexpr (VALU) {
                // the values change every step as far as the compiler can tell: the split is redone, as after a ds_read
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(av[i][e]));
                    pa[i] = split3(av[i]);
                }
            }
#pragma unroll
            for (int q = 0; q < Prod<NP>::n; ++q)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[i].p[Prod<NP>::ij[q][0]], pb[j].p[Prod<NP>::ij[q][1]], acc[i][j], 0, 0, 0);
        }
    }
    asm volatile("s_nop 7\ns_nop 7" ::: "memory");
    if (lane == 0) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        unsigned long long* st = stamps + (size_t)(blockIdx.x * 4 + wave) * 4;
        st[0] = t0; st[1] = t1; st[2] = r0; st[3] = r1;
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) sum += acc[i][j][r];
    sink[blockIdx.x * 256 + threadIdx.x] = sum;
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

struct RateArm { const char* name; void (*fn)(const float*, int, unsigned long long*, float*); };

int main(int argc, char** argv) {
    const double seconds = argc > 1 ? atof(argv[1]) : 1.5;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    printf("# %s, %d CUs\n", prop.gcnArchName, prop.multiProcessorCount);

    // ---- (a) ----
    const int K = 4608, NPROB = 64;
    std::mt19937_64 rng(20240611);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(-1.5, 1.5);
    float *dA, *dB, *dC;
    CK(hipMalloc(&dA, (size_t)NPROB * 32 * K * 4)); CK(hipMalloc(&dB, (size_t)NPROB * 32 * K * 4)); CK(hipMalloc(&dC, (size_t)NPROB * 1024 * 4));
    for (int fam = 0; fam < 2; ++fam) {
        std::vector<float> A((size_t)NPROB * 32 * K), B(A.size());
        for (int p = 0; p < NPROB; ++p) {
            std::vector<double> sa(K, 1.0), sb(K, 1.0);
            if (fam == 1) for (int k = 0; k < K; ++k) { sa[k] = std::pow(10.0, ud(rng)); sb[k] = std::pow(10.0, ud(rng)); }
            for (int r = 0; r < 32; ++r)
                for (int k = 0; k < K; ++k) {
                    A[((size_t)p * 32 + r) * K + k] = (float)(nd(rng) * sa[k]);
                    B[((size_t)p * 32 + r) * K + k] = (float)(nd(rng) * sb[k]);
                }
        }
        std::vector<double> ref((size_t)NPROB * 1024), mag(ref.size());
        for (int p = 0; p < NPROB; ++p)
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    double s = 0, m = 0;
                    const float* a = &A[((size_t)p * 32 + i) * K];
                    const float* b = &B[((size_t)p * 32 + j) * K];
                    for (int k = 0; k < K; ++k) { const double t = (double)a[k] * (double)b[k]; s += t; m += std::fabs(t); }
                    ref[(size_t)p * 1024 + i * 32 + j] = s; mag[(size_t)p * 1024 + i * 32 + j] = m;
                }
        CK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
        const char* names[4] = {"fp32 32x32x2      ", "split, 6 products ", "split, 8 products ", "split, 9 products "};
        for (int arm = 0; arm < 4; ++arm) {
            if (arm == 0) hipLaunchKernelGGL(k_dot<0>, dim3(NPROB), dim3(64), 0, 0, dA, dB, dC, K);
            if (arm == 1) hipLaunchKernelGGL(k_dot<6>, dim3(NPROB), dim3(64), 0, 0, dA, dB, dC, K);
            if (arm == 2) hipLaunchKernelGGL(k_dot<8>, dim3(NPROB), dim3(64), 0, 0, dA, dB, dC, K);
            if (arm == 3) hipLaunchKernelGGL(k_dot<9>, dim3(NPROB), dim3(64), 0, 0, dA, dB, dC, K);
            CK(hipDeviceSynchronize());
            std::vector<float> Cc((size_t)NPROB * 1024);
            CK(hipMemcpy(Cc.data(), dC, Cc.size() * 4, hipMemcpyDeviceToHost));
            // per problem: max-abs error over max-abs reference; over all: the worst and the median problem, the mean signed
            // error over sum|a||b| (a bias shows truncation in the matrix core's adder) and the worst |err| / sum|a||b|
            std::vector<double> rel;
            double worst_mag = 0, bias = 0;
            for (int p = 0; p < NPROB; ++p) {
                double me = 0, mr = 0;
                for (int i = 0; i < 1024; ++i) {
                    const size_t o = (size_t)p * 1024 + i;
                    const double e = (double)Cc[o] - ref[o];
                    me = std::max(me, std::fabs(e)); mr = std::max(mr, std::fabs(ref[o]));
                    worst_mag = std::max(worst_mag, std::fabs(e) / mag[o]); bias += e / mag[o];
                }
                rel.push_back(me / mr);
            }
            printf("accuracy  K %d  %s  %s  max-abs-err / max-abs-ref: worst %.3e median %.3e | |err| / sum|a||b|: worst %.3e, mean signed %.3e\n",
                   K, fam ? "per-k scales 10^U(-1.5,1.5)" : "N(0,1)                     ", names[arm], *std::max_element(rel.begin(), rel.end()),
                   median(rel), worst_mag, bias / (NPROB * 1024.0));
        }
    }

    // ---- (b) ----
    const int blocks = 2 * prop.multiProcessorCount, steps = 4000;
    float *src, *sink; unsigned long long* stamps;
    CK(hipMalloc(&src, 32 * 256 * 4)); CK(hipMalloc(&sink, (size_t)blocks * 256 * 4)); CK(hipMalloc(&stamps, (size_t)blocks * 128));
    {
        std::vector<float> h(32 * 256);
        for (auto& x : h) x = (float)nd(rng);
        CK(hipMemcpy(src, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    const RateArm arms[] = {
        {"fp32: 32 x 32x32x2 per step           ", k_rate<0, false>},
        {"split 6: 24 x 32x32x16 bf16, no VALU  ", k_rate<6, false>},
        {"split 6: 24 x 32x32x16 bf16 + A split ", k_rate<6, true>},
        {"split 8: 32 x 32x32x16 bf16 + A split ", k_rate<8, true>},
        {"split 9: 36 x 32x32x16 bf16 + A split ", k_rate<9, true>},
    };
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("# rate: %d blocks x 4 waves, %d K = 16 steps of a 64x64 wave tile (131072 fp32-equivalent FLOP per step and wave), %.1f s per arm\n", blocks, steps, seconds);
    for (int rep = 0; rep < 2; ++rep)
        for (const RateArm& a : arms) {
            for (int i = 0; i < 20; ++i) hipLaunchKernelGGL(a.fn, dim3(blocks), dim3(256), 0, 0, src, steps, stamps, sink);
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(a.fn, dim3(blocks), dim3(256), 0, 0, src, steps, stamps, sink);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float one; CK(hipEventElapsedTime(&one, e0, e1));
            const int n = std::max(10, (int)(seconds * 1e3 / one));
            CK(hipEventRecord(e0));
            for (int i = 0; i < n; ++i) hipLaunchKernelGGL(a.fn, dim3(blocks), dim3(256), 0, 0, src, steps, stamps, sink);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            std::vector<unsigned long long> st((size_t)blocks * 16);
            CK(hipMemcpy(st.data(), stamps, st.size() * 8, hipMemcpyDeviceToHost));
            std::vector<double> cyc, mhz;
            for (int b = 0; b < blocks * 4; ++b) {
                const unsigned long long* q = &st[(size_t)b * 4];
                const double dc = (double)(q[1] - q[0]), dr = (double)(q[3] - q[2]);
                cyc.push_back(dc / steps); mhz.push_back(dr > 0 ? dc / dr * 100.0 : 0.0);
            }
            const double flop = 131072.0 * 4 * steps * blocks * (double)n;
            printf("rate  rep %d  %s  %7.1f cycles/step  clock %5.0f MHz  %7.2f fp32-equivalent TFLOP/s by wall  (%d launches of %.0f us)\n", rep, a.name,
                   median(cyc), median(mhz), flop / (ms * 1e-3) * 1e-12, n, ms * 1e3 / n);
            fflush(stdout);
        }
    return 0;
}
