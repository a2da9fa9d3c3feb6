// fp32-MFMA implicit-GEMM convolution for gfx950 (MI355X), NHWC activations.
//
// Replaces every torch Conv2d / Linear GEMM on the FFR-Net hot path
// (reference pretrain/model_ir_se50.py:63,67,69,124 and models/recnet.py:65,82).
//
//   C[m][n] = sum_k A[m][k] * Wp[n][k]      m = (img,ho,wo)   n = cout   k = (r,s,ci)
//
// * A is never materialised: each 16-byte piece of an A-tile row is fetched straight
//   from the NHWC activation by an LDS-DMA load (global_load_lds_dwordx4) whose
//   per-lane SOURCE address does the im2col gather; zero padding reads a zero page,
//   reflect padding mirrors the index.  Weights are pre-packed [cout][r][s][ci], so
//   A- and B-tile rows are both 128-byte runs of k and share one staging path.
// * K-tile = 32 floats (one tap, 32 channels) on v_mfma_f32_32x32x2_f32 (exact fp32, 256 FLOP/clk/CU).  The swizzled
//   LDS image, the fragment reads and the K-tile schedule are igemm_core.h's, shared with k_gemm_stream.
// * 2-stage LDS ring, one barrier per K-tile: the DMA of tile t+1 is in flight while
//   tile t is multiplied.
// * Split-operand form (template parameter SPLIT, launches with IgemmArgs::w3): the same fp32 product
//   as six exact bf16 x bf16 products per term on v_mfma_f32_32x32x16_bf16 -- see the comment at k_igemm.
// * Epilogue in registers: bias (optionally one of 9 border classes, for the BN that
//   precedes a zero-padded conv), PReLU, residual add, sigmoid; NHWC store with pitch /
//   channel offset so concatenations are just addressing.
#include "conv_tail.h"
#include "ffr_kernels.h"
#include "igemm_core.h"

#include <utility>

namespace ffr {

// SPLIT (split-operand form): the same fp32 product on v_mfma_f32_32x32x16_bf16.  Every fp32 value is the sum
// of three bf16 pieces (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)); the six products ai*bj with i + j <= 4, each
// exact in fp32, are accumulated in fp32 by the matrix core.  A stays fp32 in LDS and is split in registers after the
// fragment read; B arrives as three bf16 planes a.w3 (split once from the weights), each [cout_pad][KK] bf16: per K-tile and
// row 3 x 64 B instead of 128 B, staged by the same LDS-DMA into three [BN][32] bf16 images whose 16-B chunk index is
// XOR-swizzled with (row >> 2) & 3.  Units, fix-up, epilogue and the C layout are those of the fp32 form (both MFMA shapes
// have the same 32x32 accumulator layout).
template <int BM, int BN, int WARPS_M, int WARPS_N, int PAD_MODE, bool SPLIT = false>
__global__ __launch_bounds__(256) void k_igemm(const IgemmArgs a) {
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_PT = BM / 32;                      // A staging rows per thread = A pieces per K-tile
    constexpr int B_PT = SPLIT ? 3 * (BN / 64) : BN / 32;      // B pieces per K-tile (split: 64 rows of one plane per piece)
    constexpr int STAGE_FLOATS = igemm_stage_floats(BM, BN, SPLIT);
    static_assert(WARPS_M * WARPS_N == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* s_cls = reinterpret_cast<int*>(smem + igemm_cls_offset(BM, BN, SPLIT));     // [BM] border class per row, [BM] = ticket
    float* s_bias = smem + igemm_bias_offset(BM, BN, SPLIT);                        // [9][BN] border-class biases of this tile

    const ConvTail& e = a.tail;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WARPS_N, wn = wave % WARPS_N;
    const int HoWo = a.Ho * a.Wo;

    // ---- stream-K: this persistent block owns the contiguous range [u, uend) of the
    // launch's (tile, K-tile) units; every block gets the same amount of MFMA work,
    // whatever the tile count is modulo the 256 CUs ----------------------------------------
    const long long U = (long long)a.nbatch * a.mtiles * a.ntiles * a.nkt;
    const long long G = U / a.granule;      // granule = 1, or nkt when tiles are not cut (tiny K)
    long long u = (long long)blockIdx.x * G / gridDim.x * a.granule;
    const long long uend = (long long)(blockIdx.x + 1) * G / gridDim.x * a.granule;
    unsigned long long tr_acc[6] = {0, 0, 0, 0, 0, 0}, tr_seg = 0, tr_t = 0, tr_rt0 = 0;   // trace build (option igemm_trace) only
    if (FFR_TRACE_ON(a.trace)) tr_rt0 = __builtin_amdgcn_s_memrealtime();
    while (u < uend) {
    const int tile_id = (int)(u / a.nkt);
    const int kb = (int)(u - (long long)tile_id * a.nkt);
    const int nk = (uend - u < (long long)(a.nkt - kb)) ? (int)(uend - u) : a.nkt - kb;
    u += nk;
    // batched launches (Winograd: 36 GEMMs that differ in A, W and C base) put the batch outermost
    const int tpb = a.mtiles * a.ntiles;
    const int batch = tile_id / tpb;
    const int tile_b = tile_id - batch * tpb;
    const int nt = tile_b % a.ntiles, mt = tile_b / a.ntiles;
    const float* const xb = a.x + (long long)batch * a.x_bstride;
    const float* const wb = a.w + (long long)batch * a.w_bstride;
    float* const ob = e.out + (long long)batch * a.out_bstride;
    const int m0 = mt * BM, n0 = nt * BN;
    __syncthreads();        // LDS (stages, s_cls) of the previous segment is free
    // Outside the MFMA loop this wave competes for issue slots with the co-resident block's wave,
    // which is streaming MFMAs and wins the age-based arbitration: the setup / epilogue VALU and
    // memory instructions went out at ~1 per MFMA (64 cycles).  Priority 2 for these phases.
    __builtin_amdgcn_s_setprio(2);
    // every lane value of the segment, the epilogue's addresses included, derives from this opaque copy (igemm_core.h)
    const int tid = opaque_tid();
    if (FFR_TRACE_ON(a.trace)) { tr_t = __builtin_amdgcn_s_memtime(); ++tr_seg; }
    const int lane = tid & 63;
    int srow, lch, frow, fh, fragA, fragB, pc[4];
    igemm_lane_map<BM, WM, WN>(tid, wm, wn, srow, lch, frow, fh, pc, fragA, fragB);

    // ---- per-thread staging rows -------------------------------------------------
    int a_pix[A_PT], a_h0[A_PT], a_w0[A_PT];                // pixel base of the image, top-left tap coordinates
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
        int m = m0 + srow + 32 * i;
        if (m >= a.M) m = 0;                                // rows past M compute garbage, never stored
        if (a.H == 1 && a.N == 1) {                         // plain GEMM rows (FC, Winograd GEMMs): no division
            a_pix[i] = 0;
            a_h0[i] = -a.pad;
            a_w0[i] = m * a.stride - a.pad;
        } else {
            const int n = m / HoWo;
            const int rem = m - n * HoWo;
            const int ho = rem / a.Wo;
            const int wo = rem - ho * a.Wo;
            a_pix[i] = n * a.H * a.W;
            a_h0[i] = ho * a.stride - a.pad;
            a_w0[i] = wo * a.stride - a.pad;
        }
    }
    if (e.border_bias && tid < BM) {
        int m = m0 + tid;
        if (m >= a.M) m = 0;
        const int n = m / HoWo;
        const int rem = m - n * HoWo;
        const int ho = rem / a.Wo;
        const int wo = rem - ho * a.Wo;
        const int h0 = ho * a.stride - a.pad, w0 = wo * a.stride - a.pad;
        const int rc = (h0 < 0) ? 0 : ((h0 + a.R - 1 >= a.H) ? 2 : 1);
        const int cc = (w0 < 0) ? 0 : ((w0 + a.S - 1 >= a.W) ? 2 : 1);
        s_cls[tid] = rc * 3 + cc;
    }
    if (e.border_bias) {
        for (int idx = tid; idx < 9 * BN; idx += 256) s_bias[idx] = e.bias[(idx / BN) * e.cout_pad + n0 + (idx % BN)];
    }

    // ---- tap state at the first K-tile of this segment -----------------------------------
    const int kbase0 = kb * 32;
    int tap = kbase0 / a.cin_pad;
    int c0 = kbase0 - tap * a.cin_pad;
    int tr = tap / a.S, ts = tap - tr * a.S;

    // current source pointer of every staged row (advances 32 floats per K-tile; the
    // A pointers are re-derived when the tap changes)
    const float* a_ptr[A_PT];
    const float* b_ptr[B_PT];        // split form: pointers into the bf16 planes
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
        if constexpr (SPLIT) {
            const int brow = tid >> 2, bch = (tid & 3) ^ ((brow >> 2) & 3);
            const int plane = i / (BN / 64), piece = i % (BN / 64);
            b_ptr[i] = reinterpret_cast<const float*>(a.w3 + (size_t)plane * a.w3_pstride + (size_t)(n0 + brow + 64 * piece) * a.KK + kbase0 + bch * 8);
        } else {
            b_ptr[i] = wb + (size_t)(n0 + srow + 32 * i) * a.KK + kbase0 + lch * 4;
        }
    }

    auto set_tap = [&]() {
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            int hi = a_h0[i] + tr, wi = a_w0[i] + ts;
            bool ok = true;
            if (PAD_MODE == 1) {
                hi = reflect_index(hi, a.H);
                wi = reflect_index(wi, a.W);
            } else {
                ok = ((unsigned)hi < (unsigned)a.H) && ((unsigned)wi < (unsigned)a.W);
            }
            const float* src = xb + (size_t)(a_pix[i] + hi * a.W + wi) * a.in_pitch;
            a_ptr[i] = (ok ? src : a.zero) + c0 + lch * 4;   // the zero page is >= cin_pad floats long
        }
    };
    set_tap();

    // one 16-B-per-lane LDS-DMA piece (8 rows x 128 B per wave) of the next K-tile
    auto dma_piece = [&](int buf, int d) {
        float* sA = smem + buf * STAGE_FLOATS;
        if (d < A_PT) igemm_dma_piece(sA, wave, d, a_ptr[d]);
        else if constexpr (!SPLIT) igemm_dma_piece(sA, wave, d, b_ptr[d - A_PT]);
        else {                          // 16 rows x 64 B per wave; 32 bf16 = 16 floats per K-tile
            const int i = d - A_PT;
            __builtin_amdgcn_global_load_lds(GLB_PTR(b_ptr[i]), LDS_PTR(sA + BM * 32 + (i / (BN / 64)) * BN * 16 + (64 * (i % (BN / 64)) + 16 * wave) * 16), 16, 0, 0);
            b_ptr[i] += 16;
        }
    };
    // after all pieces of a K-tile are issued: move to the next tap when the channel run ends
    auto advance_tile = [&]() {
        c0 += 32;
        if (c0 == a.cin_pad) {
            c0 = 0;
            if (++ts == a.S) { ts = 0; ++tr; }
            set_tap();
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    constexpr int ND = A_PT + B_PT;          // DMA pieces per K-tile
    if constexpr (SPLIT) {
        // K-tile = two K = 16 steps.  Per step and 32x32 tile six bf16 MFMAs (small products first); the fillers of a step, in
        // this order, spread evenly over its MFMA gaps and pinned: the fragment reads of the NEXT step (A: two fp32
        // ds_read_b128 per 32 rows, B: one per plane and 32 columns), in step 1 the LDS-DMA pieces of the K-tile after the
        // next, then the split of the next step's A values in registers (per pair of values two units: 5 and 6 vector
        // instructions).  A K-tile lasts ~1.5 k cycles here, a quarter of the fp32 form's: a DMA issued in step 0 for the
        // barrier in front of step 1 (the fp32 form's distance) would have ~0.3 us to arrive.  The stage of tile t is free
        // once that barrier has passed (step 1 reads tile t + 1), so tile t + 2 is requested right behind it and has a whole
        // K-tile of time.
        // Vector instructions do not overlap with MFMAs on this chip (profiles/r05_probe_mfma_valu_coissue.txt): the split
        // is paid in full, which is why a wave takes ALL columns of its rows (WARPS_N = 1 where BN allows): no A value is
        // split twice.
        constexpr int NPROD = 6;
        constexpr int PA[NPROD] = {2, 0, 1, 1, 0, 0}, PB[NPROD] = {0, 2, 1, 0, 1, 0};
        constexpr int NQ = TM * TN * NPROD;      // MFMAs per step
        constexpr int NR = 2 * TM + 3 * TN;      // fragment reads per step
        constexpr int NU = TM * 8;               // split units per step
        f32x4 araw[TM][2];
        u32x4 pa[2][TM][3];
        f32x4 pb[2][TN][3];
        const int fswz = (lane >> 1) & 7, bswz = (lane >> 2) & 3;     // chunk swizzle of the fp32 A rows, of the bf16 B rows
        int pcA[2][2], pcB[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            pcA[st][0] = ((4 * st + 2 * fh) ^ fswz) * 4;
            pcA[st][1] = ((4 * st + 2 * fh + 1) ^ fswz) * 4;
            pcB[st] = ((2 * st + fh) ^ bswz) * 4;
        }
        const int fragB3 = BM * 32 + (wn * WN + frow) * 16;
        auto read_piece = [&](int slot, const float* stage, int st, int r) __attribute__((always_inline)) {
            if (r < 2 * TM) araw[r / 2][r % 2] = *reinterpret_cast<const f32x4*>(stage + fragA + (r / 2) * 32 * 32 + pcA[st][r % 2]);
            else {
                const int j = (r - 2 * TM) / 3, p = (r - 2 * TM) % 3;
                pb[slot][j][p] = *reinterpret_cast<const f32x4*>(stage + fragB3 + p * BN * 16 + j * 32 * 16 + pcB[st]);
            }
        };
        // unit u of the split of araw into pa[slot]: row block u / 8, pair (u / 2) % 4, first / second half
        auto split_unit = [&](int slot, int u) __attribute__((always_inline)) {
            const int i = u / 8, e2 = (u / 2) % 4, v = e2 / 2, e = 2 * (e2 % 2);
            float lo = araw[i][v][e], hi = araw[i][v][e + 1];
            if (u % 2) { const u32x2 p = split_bf16_second(lo, hi); pa[slot][i][1][e2] = p.x; pa[slot][i][2][e2] = p.y; }
            else { pa[slot][i][0][e2] = split_bf16_first(lo, hi); araw[i][v][e] = lo; araw[i][v][e + 1] = hi; }
        };
        // Step ST of a K-tile is spelled out at compile time, gap by gap (a `#pragma unroll` nest over steps, gaps and fillers
        // exceeds the unroller's size limit for the 128x128 tile before it folds, and the fragment arrays then live in scratch).
        // filler FI of the step: a fragment read, an LDS-DMA piece or a split unit
        auto filler = [&]<int ST, bool LAST, int FI>(int cur, bool more) __attribute__((always_inline)) {
            constexpr int NDS = (ST == 1 && !LAST) ? ND : 0;
            if constexpr (FI < NR) read_piece(ST ^ 1, smem + (ST == 0 ? cur : cur ^ 1) * STAGE_FLOATS, ST ^ 1, FI);
            else if constexpr (FI < NR + NDS) { if (more) dma_piece(cur, FI - NR); }
            else split_unit(ST ^ 1, FI - NR - NDS);
        };
        // gap G: one MFMA and the fillers f with f * NQ / F == G
        auto gap = [&]<int ST, bool LAST, int G>(int cur, bool more) __attribute__((always_inline)) {
            constexpr int NDS = (ST == 1 && !LAST) ? ND : 0;
            constexpr int F = (ST == 0 || !LAST) ? NR + NDS + NU : 0;       // LAST: step 1 has no next step to prepare
            constexpr int q = G / (TM * TN), i = (G / TN) % TM, j = G % TN;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[ST][i][PA[q]]),
                                                               __builtin_bit_cast(bf16x8, pb[ST][j][PB[q]]), acc[i][j], 0, 0, 0);
            constexpr int F0 = (G * F + NQ - 1) / NQ, F1 = ((G + 1) * F + NQ - 1) / NQ;
            [&]<int... K>(std::integer_sequence<int, K...>) __attribute__((always_inline)) {
                (filler.template operator()<ST, LAST, F0 + K>(cur, more), ...);
            }(std::make_integer_sequence<int, F1 - F0>{});
            FFR_PIN;
        };
        auto step = [&]<int ST, bool LAST, int... G>(int cur, bool more, std::integer_sequence<int, G...>) __attribute__((always_inline)) {
            if (ST == 1 && !LAST) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                FFR_PIN;
            }
            (gap.template operator()<ST, LAST, G>(cur, more), ...);
            if (ST == 1 && !LAST && more) { advance_tile(); FFR_PIN; }
        };
        // tile t in stage cur = t & 1; more: tile t + 2 exists
        auto tile_body = [&]<bool LAST>(int cur, bool more) __attribute__((always_inline)) {
            step.template operator()<0, LAST>(cur, more, std::make_integer_sequence<int, NQ>{});
            step.template operator()<1, LAST>(cur, more, std::make_integer_sequence<int, NQ>{});
        };
        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[0] += t - tr_t; tr_t = t; }
        // prologue: tiles 0 and 1 -> stages 0 and 1; wait for tile 0 only; its first fragments -> slot 0
#pragma unroll
        for (int d = 0; d < ND; ++d) dma_piece(0, d);
        advance_tile();
        if (nk > 1) {
#pragma unroll
            for (int d = 0; d < ND; ++d) dma_piece(1, d);
            advance_tile();
            static_assert(ND < 16, "vmcnt immediate");
            __builtin_amdgcn_s_waitcnt(0x0F70 | ND);        // vmcnt(ND): the ND pieces of tile 1 may still be in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int r = 0; r < NR; ++r) read_piece(0, smem, 0, r);
#pragma unroll
        for (int u = 0; u < NU; ++u) split_unit(0, u);
        FFR_PIN;
        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[1] += t - tr_t; tr_t = t; }
        __builtin_amdgcn_s_setprio(0);
#pragma unroll 1
        for (int it = 0; it + 1 < nk; ++it) tile_body.template operator()<false>(it & 1, it + 2 < nk);
        tile_body.template operator()<true>((nk - 1) & 1, false);
        __builtin_amdgcn_s_setprio(2);
        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[2] += t - tr_t; tr_t = t; }
    } else {
        constexpr int NR = TM + TN;              // fragment reads per chunk
        f32x4 af[2][TM], bf[2][TN];
        // one K-tile from stage cur (igemm_core.h); once the pieces of the next one are out, the sources move on
        auto tile_body = [&]<bool LAST>(int cur) {
            igemm_ktile<TM, TN, ND, LAST>(acc, af, bf, smem + cur * STAGE_FLOATS, smem + (cur ^ 1) * STAGE_FLOATS, fragA, fragB, pc,
                                          [&](int d) { dma_piece(cur ^ 1, d); }, [&] { advance_tile(); FFR_PIN; });
        };

        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[0] += t - tr_t; tr_t = t; }
        // prologue: tile 0 -> stage 0, its first fragments -> slot 0
#pragma unroll
        for (int d = 0; d < ND; ++d) dma_piece(0, d);
        advance_tile();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; ++r) igemm_read_piece(af[0], bf[0], smem, fragA, fragB, pc[0], r);
        FFR_PIN;
        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[1] += t - tr_t; tr_t = t; }
        __builtin_amdgcn_s_setprio(0);
#pragma unroll 1
        for (int it = 0; it + 1 < nk; ++it) tile_body.template operator()<false>(it & 1);
        tile_body.template operator()<true>((nk - 1) & 1);
        __builtin_amdgcn_s_setprio(2);
        if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[2] += t - tr_t; tr_t = t; }
    }

    // ---- epilogue: accumulators -> LDS (C tile, row stride BN+4) -> whole rows, 16 B per lane ----
    // (register-layout stores are 128-B pieces, one instruction per accumulator register: 64
    //  store instructions per wave for a 64x64 wave tile took as long as 10-20 K-tiles)
    constexpr int LDC = BN + 4;
    constexpr int NQ4 = BN / 4;            // float4 columns per row
    constexpr int RPP = 256 / NQ4;         // rows per pass of the 256 threads
    float* sC = smem;
    __syncthreads();                       // every wave is done reading the stage buffers
    if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[4] += t - tr_t; }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ml = acc_row(wm * WM + i * 32, r) + 4 * fh;
#pragma unroll
            for (int j = 0; j < TN; ++j) sC[ml * LDC + wn * WN + j * 32 + frow] = acc[i][j][r];
        }
    __syncthreads();
    if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[5] += t - tr_t; }
    const int erow = tid / NQ4, ecol = (tid - erow * NQ4) * 4;
    bool finish = true;                    // this block applies the epilogue and stores the tile
    if (nk != a.nkt) {
        // Partial K range (stream-K cut).  Every contributor stores its raw sums to its slab
        // (slot 0: segment does not start at k = 0, slot 1: it does) with write-through stores,
        // drains them and draws a ticket; the block that draws the last ticket adds
        // the slabs in block order (bitwise reproducible) and finishes the tile.  Nobody waits.
        const long long tb = (long long)tile_id * a.nkt;
        const int P = gridDim.x;
        const int b_lo = (int)(((tb + 1) * P - 1) / G), b_hi = (int)(((tb + a.nkt) * P - 1) / G);
        float* dst = a.partial + ((size_t)blockIdx.x * 2 + (kb != 0 ? 0 : 1)) * (BM * BN);
#pragma unroll 4
        for (int p = 0; p < BM / RPP; ++p) {
            const int ml = p * RPP + erow;
            // write-through (sc1) stores: the slab is in memory once vmcnt drains, so no agent-scope
            // release (L2 write-back of 64 KB of fresh lines: tens of us per cut) is needed
            const f32x4 val = *reinterpret_cast<const f32x4*>(sC + ml * LDC + ecol);
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst + ml * BN + ecol), "v"(val) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave drains before the barrier
        __syncthreads();
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(a.tickets + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == b_hi - b_lo) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(a.tickets + tile_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            }
            s_cls[BM] = old;
        }
        __syncthreads();
        finish = s_cls[BM] == b_hi - b_lo;
        if (finish) {
#pragma unroll 1
            for (int p = 0; p < BM / RPP; ++p) {
                const int ml = p * RPP + erow;
                f32x4 sum = {0.f, 0.f, 0.f, 0.f};
                // eight slabs in flight at a time, added in block order (a tile of the FC is cut into 32 segments: one load per
                // add left the last arriver waiting a memory latency 128 times, half of that launch's 123 us)
                for (int bb = b_lo; bb <= b_hi; bb += 8) {
                    f32x4 v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int bk = bb + k;
                        v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        if (bk <= b_hi) {
                            if (bk == (int)blockIdx.x) {
                                v[k] = *reinterpret_cast<const f32x4*>(sC + ml * LDC + ecol);
                            } else {
                                const int slot = ((long long)bk * G / P * a.granule > tb) ? 0 : 1;
                                v[k] = *reinterpret_cast<const f32x4*>(a.partial + ((size_t)bk * 2 + slot) * (BM * BN) + ml * BN + ecol);
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (bb + k <= b_hi) sum += v[k];
                }
                *reinterpret_cast<f32x4*>(sC + ml * LDC + ecol) = sum;   // same thread re-reads it below
            }
        }
    }
    if (finish) {
        const int n = n0 + ecol;
        // (the one sigmoid conv of the network, 49 channels, takes the generic path)
        const bool vec = ((e.out_pitch | e.out_coff | e.res_pitch) & 3) == 0 && n + 4 <= e.cout_store && !(e.flags & 1);
        const f32x4 slope4 = tail_slope4(e.slope, n);
        const f32x4 bias0 = *reinterpret_cast<const f32x4*>(e.bias + n);
        // No global LOAD may sit between the stores of this loop: vmcnt retires in order, so the
        // wait in front of a load's first use also drains every older store (a full HBM write
        // latency per pass: 37k of the 42k epilogue cycles measured).  Border-class biases come
        // from LDS; residual rows are fetched one batch AHEAD of the batch being stored.
        constexpr int NP = BM / RPP;
        constexpr int BATCH = NP < 4 ? NP : 4;
        auto finish_tile = [&]<bool BORDER, bool RESID>() {
            f32x4 rs[BATCH], rn[BATCH];
            // row pointers advance by RPP rows per pass (no 64-bit multiply per store)
            const int mrow = m0 + erow;
            float* optr = ob + (size_t)mrow * e.out_pitch + e.out_coff + n;
            const size_t ostep = (size_t)RPP * e.out_pitch;
            const float* rptr = RESID ? e.resid + (size_t)mrow * e.res_pitch + n : nullptr;
            const size_t rstep = (size_t)RPP * e.res_pitch;
            auto load_resid = [&](f32x4* dstv, int p0) {
#pragma unroll
                for (int k = 0; k < BATCH; ++k) {
                    dstv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (mrow + (p0 + k) * RPP < a.M) dstv[k] = *reinterpret_cast<const f32x4*>(rptr + (size_t)(p0 + k) * rstep);
                }
            };
            if (RESID) load_resid(rs, 0);
#pragma unroll
            for (int p0 = 0; p0 < NP; p0 += BATCH) {
                if (RESID && p0 + BATCH < NP) load_resid(rn, p0 + BATCH);
#pragma unroll
                for (int k = 0; k < BATCH; ++k) {
                    const int ml = (p0 + k) * RPP + erow;
                    // tail_act4's arithmetic, written out: through the call, or through prelu<> alone, the fp and MFMA sequence of
                    // all 16 instantiations comes out in another order
                    f32x4 v = *reinterpret_cast<const f32x4*>(sC + ml * LDC + ecol);
                    if (BORDER) v += *reinterpret_cast<const f32x4*>(s_bias + s_cls[ml] * BN + ecol);
                    else v += bias0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = v[c] >= 0.f ? v[c] : v[c] * slope4[c];
                    if (RESID) v += rs[k];
                    if (m0 + ml < a.M) *reinterpret_cast<f32x4*>(optr) = v;
                    optr += ostep;
                }
                if (RESID) {
#pragma unroll
                    for (int k = 0; k < BATCH; ++k) rs[k] = rn[k];
                }
            }
        };
        if (vec) {
            if (e.border_bias) {
                if (e.resid) finish_tile.template operator()<true, true>();
                else finish_tile.template operator()<true, false>();
            } else {
                if (e.resid) finish_tile.template operator()<false, true>();
                else finish_tile.template operator()<false, false>();
            }
        } else {
            // generic slow path: channel slices that are not 16-B aligned / ragged cout / sigmoid
#pragma unroll 1
            for (int p = 0; p < NP; ++p) {
                const int ml = p * RPP + erow;
                const int m = m0 + ml;
                if (m >= a.M) continue;
                f32x4 v = *reinterpret_cast<const f32x4*>(sC + ml * LDC + ecol);
                v += e.border_bias ? *reinterpret_cast<const f32x4*>(s_bias + s_cls[ml] * BN + ecol) : bias0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (n + c < e.cout_store) {
                        float x = prelu<PRELU_SELECT>(v[c], slope4[c]);
                        x = tail_end1(x, e.resid != nullptr, [&] { return e.resid[(size_t)m * e.res_pitch + n + c]; }, e.flags);
                        ob[(size_t)m * e.out_pitch + e.out_coff + n + c] = x;
                    }
                }
            }
        }
    }
    if (FFR_TRACE_ON(a.trace)) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr_acc[3] += t - tr_t; tr_t = t; }
    }   // stream-K segment loop
    if (FFR_TRACE_ON(a.trace) && threadIdx.x == 0) {
        unsigned long long* t = a.trace + (size_t)blockIdx.x * 8;
        t[0] = tr_acc[0]; t[1] = tr_acc[1]; t[2] = tr_acc[2]; t[3] = tr_acc[3]; t[4] = tr_seg;
        t[5] = tr_rt0; t[6] = __builtin_amdgcn_s_memrealtime(); t[7] = (tr_acc[4] << 32) | (tr_acc[5] & 0xffffffffull);
    }
}

// tile index -> instantiation of (pad mode, form), with the form's wave grid of the tile table; null: no such tile
static const void* igemm_kernel(int tile, int pad_mode, bool split) {
    return igemm_tile_dispatch(tile, [&](auto t) -> const void* {
        constexpr IgemmTile T = IGEMM_TILES[t];
        if (split) return pad_mode == 1 ? (const void*)k_igemm<T.bm, T.bn, T.wm_split, T.wn_split, 1, true> : (const void*)k_igemm<T.bm, T.bn, T.wm_split, T.wn_split, 0, true>;
        return pad_mode == 1 ? (const void*)k_igemm<T.bm, T.bn, T.wm, T.wn, 1, false> : (const void*)k_igemm<T.bm, T.bn, T.wm, T.wn, 0, false>;
    });
}

hipError_t igemm_init() {
    for (int i = 0; i < IGEMM_NTILES * 4; ++i) {       // every tile x pad mode x form
        const int tile = 1 + i / 4, split = i & 1;
        const hipError_t e = hipFuncSetAttribute(igemm_kernel(tile, (i >> 1) & 1, split), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 igemm_lds_bytes(IGEMM_TILES[tile].bm, IGEMM_TILES[tile].bn, split));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_igemm(const IgemmArgs& a, int tile, int nblocks, hipStream_t stream) {
    const bool split = a.w3 != nullptr;
    const void* kernel = igemm_kernel(tile, a.pad_mode, split);
    if (!kernel || nblocks <= 0) return hipErrorInvalidValue;
    if (split && a.nbatch != 1) return hipErrorInvalidValue;      // the planes have no batch stride
    void* args[] = {const_cast<IgemmArgs*>(&a)};
    return hipLaunchKernel(kernel, dim3((unsigned)nblocks, 1, 1), dim3(256), args,
                           igemm_lds_bytes(IGEMM_TILES[tile].bm, IGEMM_TILES[tile].bn, split), stream);
}

// planes[p][i] = piece p of w[i] (bf16, round to nearest even), p = 0..2: the device-side split of raw fp32 weights
// (ffr_op_conv's test flag; the loaders split on the host from the double-precision fold)
__global__ void k_split_weights(const float* __restrict__ w, unsigned short* __restrict__ planes, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float r = w[i];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const unsigned short h = (unsigned short)(cvt_pk_bf16(r, 0.f) & 0xffffu);
            planes[(size_t)p * n + i] = h;
            r -= __builtin_bit_cast(float, (unsigned)h << 16);
        }
    }
}

hipError_t launch_split_weights(const float* w, unsigned short* planes, size_t n, hipStream_t stream) {
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_split_weights, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, w, planes, n);
    return hipGetLastError();
}

}  // namespace ffr
