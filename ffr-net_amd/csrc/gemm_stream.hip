// Batched plain fp32-MFMA GEMM with a CONTINUOUS K-tile stream across output tiles:
//     C[b][m][n] = sum_k A[b][m][k] * W[b][n][k]          (the 36 GEMMs of a Winograd F(4x4,3x3) conv)
//
// Same operand staging and MFMA schedule as the fp32 form of k_igemm, from the same definitions (igemm_core.h describes
// them).  What differs: these GEMMs have short K (4..48 K-tiles), so a per-tile prologue (first DMA round trip) and an
// LDS-staged epilogue cost as much as the multiply (measured: 2x the loop time at K = 256).  Here a persistent block owns
// a contiguous range of whole tiles and never stops the stream: the first K-tile of the next tile is fetched and its
// fragments are read under the last K-tile of the current one, and a finished accumulator tile is copied out of the
// accumulation registers and stored straight from registers (128-byte pieces) while the next tile multiplies.  No bias /
// activation: plain store.
#include "ffr_kernels.h"
#include "igemm_core.h"

namespace ffr {

template <int BM, int BN, int WARPS_M, int WARPS_N>
__global__ __launch_bounds__(256, 163840 / igemm_lds_bytes(BM, BN, false))      // the fp32 k_igemm's residency: what plan_gemm_stream counts on
void k_gemm_stream(const GemmStreamArgs a) {
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_PT = BM / 32, B_PT = BN / 32;
    constexpr int STAGE_FLOATS = igemm_stage_floats(BM, BN, false);
    constexpr int NR = TM + TN, ND = A_PT + B_PT;
    static_assert(WARPS_M * WARPS_N == 4, "layout");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WARPS_N, wn = wave % WARPS_N;
    // lane-derived values are re-derived per tile from an opaque copy of the thread id
    int srow, lch, frow, fh, fragA, fragB, pc[4];
    auto lane_values = [&]() { igemm_lane_map<BM, WM, WN>(opaque_tid(), wm, wn, srow, lch, frow, fh, pc, fragA, fragB); };
    lane_values();

    const long long T = (long long)a.nbatch * a.mtiles * a.ntiles;
    int t = (int)((long long)blockIdx.x * T / gridDim.x);
    const int t_end = (int)((long long)(blockIdx.x + 1) * T / gridDim.x);
    if (t >= t_end) return;
    const int nkt = a.K / 32;

    const float* a_ptr[A_PT];
    const float* b_ptr[B_PT];
    float* orow = nullptr;      // this lane's first output element of the tile being staged
    int mrow0 = 0;              // its row index (for the M edge)
    auto tile_ptrs = [&](int tile) {
        const int tpb = a.mtiles * a.ntiles;
        const int batch = tile / tpb;
        const int tb = tile - batch * tpb;
        const int nt = tb % a.ntiles, mt = tb / a.ntiles;
        const int m0 = mt * BM, n0 = nt * BN;
        const float* Ab = a.A + (long long)batch * a.M * a.K;
        const float* Wb = a.W + (long long)batch * a.Npad * a.K;
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            int m = m0 + srow + 32 * i;
            if (m >= a.M) m = 0;
            a_ptr[i] = Ab + (size_t)m * a.K + lch * 4;
        }
#pragma unroll
        for (int i = 0; i < B_PT; ++i) b_ptr[i] = Wb + (size_t)(n0 + srow + 32 * i) * a.K + lch * 4;
        mrow0 = m0 + wm * WM + 4 * fh;
        orow = a.C + (long long)batch * a.M * a.Npad + (size_t)mrow0 * a.Npad + n0 + wn * WN + frow;
    };
    auto dma_piece = [&](int buf, int d) {
        igemm_dma_piece(smem + buf * STAGE_FLOATS, wave, d, d < A_PT ? a_ptr[d] : b_ptr[d - A_PT]);
    };

    f32x16 acc[TM][TN];
    f32x4 af[2][TM], bf[2][TN];
    // one K-tile; LAST = nothing follows in this block's stream
    auto ktile = [&]<bool LAST>(int cur) {
        igemm_ktile<TM, TN, ND, LAST>(acc, af, bf, smem + cur * STAGE_FLOATS, smem + (cur ^ 1) * STAGE_FLOATS, fragA, fragB, pc,
                                      [&](int d) { dma_piece(cur ^ 1, d); }, [] {});
    };

    // ---- start of the stream -----------------------------------------------------------
    tile_ptrs(t);
#pragma unroll
    for (int d = 0; d < ND; ++d) dma_piece(0, d);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) igemm_read_piece(af[0], bf[0], smem, fragA, fragB, pc[0], r);
    FFR_PIN;
    int s = 0;                                    // K-tiles streamed so far (stage parity)
#pragma unroll 1
    for (; t < t_end; ++t) {
        lane_values();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        float* const orow_cur = orow;
        const int mrow_cur = mrow0;
        const bool last_tile = (t + 1 == t_end);
#pragma unroll 1
        for (int kt = 0; kt + 1 < nkt; ++kt, ++s) ktile.template operator()<false>(s & 1);
        // last K-tile of this tile: its DMA pieces already fetch the FIRST K-tile of the next tile
        if (!last_tile) {
            tile_ptrs(t + 1);
            ktile.template operator()<false>(s & 1);
            ++s;
        } else {
            ktile.template operator()<true>(s & 1);
        }
        // finished tile: registers -> memory, 128-byte pieces (lanes 0-31 one row, lanes 32-63 the row + 4)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mlr = acc_row(i * 32, r);
                if (mrow_cur + mlr < a.M) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        orow_cur[(size_t)mlr * a.Npad + j * 32] = acc[i][j][r];
                    }
                }
            }
    }
}

static size_t gs_lds_bytes(int bm, int bn) { return (size_t)2 * igemm_stage_floats(bm, bn, false) * 4; }

// tile index -> instantiation (the fp32 wave grid of the tile table); null: not a tile of this kernel
static const void* gemm_stream_kernel(int tile) {
    return igemm_tile_dispatch(tile, [](auto t) -> const void* {
        constexpr IgemmTile T = IGEMM_TILES[t];
        if constexpr (t == IGEMM_TILE_128x128 || t == IGEMM_TILE_128x64) return (const void*)k_gemm_stream<T.bm, T.bn, T.wm, T.wn>;
        else return nullptr;
    });
}

hipError_t gemm_stream_init() {
    for (int tile = IGEMM_TILE_128x128; tile <= IGEMM_TILE_128x64; ++tile) {
        const hipError_t e = hipFuncSetAttribute(gemm_stream_kernel(tile), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)gs_lds_bytes(IGEMM_TILES[tile].bm, IGEMM_TILES[tile].bn));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// tile: IGEMM_TILE_128x128 or IGEMM_TILE_128x64
hipError_t launch_gemm_stream(GemmStreamArgs a, int tile, int nblocks, hipStream_t stream) {
    int bm, bn;
    igemm_tile_shape(tile, &bm, &bn);
    const void* kernel = gemm_stream_kernel(tile);
    if (!kernel || a.Npad % bn || a.K % 32 || nblocks <= 0) return hipErrorInvalidValue;
    a.mtiles = (a.M + bm - 1) / bm;
    a.ntiles = a.Npad / bn;
    void* args[] = {&a};
    return hipLaunchKernel(kernel, dim3(nblocks), dim3(256), args, gs_lds_bytes(bm, bn), stream);
}

}  // namespace ffr
