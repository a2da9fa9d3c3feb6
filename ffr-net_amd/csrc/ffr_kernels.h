// Internal launcher declarations shared by the kernel translation units and the
// engine.  Everything here is fp32, NHWC ("pixel-major, channel-minor") unless a
// name says nchw.  Launchers only enqueue work on `stream`; they return hipError_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// Diagnostics (per-block clock stamps) exist only in a -DFFR_TRACE build (tools/trace_build.py); the shipped library
// compiles them out.
#ifdef FFR_TRACE
#define FFR_TRACE_ON(p) ((p) != nullptr)
#else
#define FFR_TRACE_ON(p) false
#endif

namespace ffr {

// ---- what a convolution stores: the epilogue of every convolution kernel -----------
// out[m][out_coff + c] = tail(acc[m][c]) for the pixels m = (img, ho, wo) and the channels c < cout_store, with
//   tail(v) = sigmoid?( PReLU(v + bias[class(m)][c], slope[c]) + resid[m][c] )       (device side: conv_tail.h)
struct ConvTail {
    const float* bias;    // [n_cls][cout_pad]: the 9 border classes (3 * row class + column class) iff border_bias, else 1
    const float* slope;   // [cout_pad] PReLU slopes, or null: no activation
    const float* resid;   // [M][res_pitch], added after the activation, or null
    float* out;           // [M][out_pitch]; channel c goes to column out_coff + c (concatenations are just addressing)
    // Winograd kernels only (k_igemm does not read it), or null: per-tile sums of the stored outputs [T][cout_pad], the SE
    // squeeze partials.  One rule for every kernel and every store path (vector or scalar stores, any pitch, cout_store <
    // cout_pad): entry (tile, channel) is the sum of exactly the values this call stored to `out` for that channel over the
    // tile's pixels inside the map; a channel that is not stored gets 0.
    float* tile_sums;
    int cout_pad;         // channels computed: the row length of bias, slope and tile_sums
    int cout_store;       // channels stored, <= cout_pad: the others are computed and dropped
    int out_pitch, out_coff, res_pitch;
    int border_bias;
    int flags;            // bit 0: sigmoid at the end
};

// ---- implicit-GEMM convolution (igemm.hip) -----------------------------------------
// out[m][n] = tail( sum_k A[m][k] * Wp[n][k] ),  m = (img, ho, wo), k = (r, s, ci)
struct IgemmArgs {
    const float* x;       // [N,H,W,in_pitch]
    const float* w;       // [cout_pad][KK] packed, KK = R*S*cin_pad
    ConvTail tail;
    const float* zero;    // >= 128 B of zeros (source of zero-padded taps)
    float* partial;       // stream-K slabs [nblocks][2][BM*BN]
    int* tickets;         // stream-K arrival counters, one per tile, zero between launches
    unsigned long long* trace;   // diagnostic (-DFFR_TRACE build, option "igemm_trace"): 8 words per block, or null
    int N, H, W, Ho, Wo, in_pitch, cin_pad, R, S, stride, pad, pad_mode;
    int M, KK, nkt, granule;
    int nbatch;                              // >= 1: independent GEMMs in one launch (tile id = batch-major)
    long long x_bstride, w_bstride, out_bstride;   // element strides between batches
    int mtiles, ntiles;
    // split-operand form (igemm.hip): three bf16 planes of w, plane p at w3 + p * w3_pstride, each [cout_pad][KK];
    // non-null selects the form (nbatch must be 1)
    const unsigned short* w3;
    long long w3_pstride;
};
enum { IGEMM_TILE_128x128 = 1, IGEMM_TILE_128x64 = 2, IGEMM_TILE_64x64 = 3, IGEMM_TILE_256x64 = 4,
       IGEMM_NTILES = 4 };
// The one table of tile facts: shape and the grid of the block's 4 waves (rows x columns) in the fp32 form and in the split
// form, where a wave owns all columns of its rows when the tile allows it (no A value is split twice).  Entry 0: no tile.
struct IgemmTile { int bm, bn, wm, wn, wm_split, wn_split; };
constexpr IgemmTile IGEMM_TILES[IGEMM_NTILES + 1] = {
    {0, 0, 0, 0, 0, 0}, {128, 128, 2, 2, 4, 1}, {128, 64, 2, 2, 4, 1}, {64, 64, 2, 2, 2, 2}, {256, 64, 4, 1, 4, 1}};
// calls f with the tile index as a compile-time constant (IGEMM_TILES[t] picks the template arguments); no tile: a null result
template <typename F>
inline auto igemm_tile_dispatch(int tile, F&& f) -> decltype(f(std::integral_constant<int, IGEMM_TILE_128x128>{})) {
    switch (tile) {
        case IGEMM_TILE_128x128: return f(std::integral_constant<int, IGEMM_TILE_128x128>{});
        case IGEMM_TILE_128x64: return f(std::integral_constant<int, IGEMM_TILE_128x64>{});
        case IGEMM_TILE_64x64: return f(std::integral_constant<int, IGEMM_TILE_64x64>{});
        case IGEMM_TILE_256x64: return f(std::integral_constant<int, IGEMM_TILE_256x64>{});
        default: return {};
    }
}
inline void igemm_tile_shape(int tile, int* bm, int* bn) {
    const IgemmTile& t = IGEMM_TILES[tile >= 1 && tile <= IGEMM_NTILES ? tile : 0];
    *bm = t.bm; *bn = t.bn;
}
// Dynamic LDS of a k_igemm block, in floats from its start.  One stage of the 2-stage ring: a K-tile of BM rows of A and BN of B,
// 32 fp32 each; split form: B as three bf16 planes, 3 x 16 floats per row (k_gemm_stream's stage is the fp32 one).  The
// epilogue's C tile [BM][BN + 4] lies over the ring; behind both s_cls, [BM] border class per row and [BM] = ticket (4 ints
// keep the alignment), then s_bias [9][BN], the border-class biases of the tile.
constexpr int igemm_stage_floats(int bm, int bn, bool split) { return split ? bm * 32 + bn * 48 : (bm + bn) * 32; }
constexpr int igemm_cls_offset(int bm, int bn, bool split) {
    return 2 * igemm_stage_floats(bm, bn, split) > bm * (bn + 4) ? 2 * igemm_stage_floats(bm, bn, split) : bm * (bn + 4);
}
constexpr int igemm_bias_offset(int bm, int bn, bool split) { return igemm_cls_offset(bm, bn, split) + bm + 4; }
constexpr int igemm_lds_bytes(int bm, int bn, bool split) { return (igemm_bias_offset(bm, bn, split) + 9 * bn) * 4; }
// blocks of 256 threads one CU holds: k_igemm is LDS-limited, 160 KiB per CU
constexpr int igemm_resident_blocks(int tile, bool split = false) {
    return tile >= 1 && tile <= IGEMM_NTILES ? 163840 / igemm_lds_bytes(IGEMM_TILES[tile].bm, IGEMM_TILES[tile].bn, split) : 0;
}
// the planners (plan.cpp) are tuned to these: a stage change that alters a residency has to be a decision, not a side effect
static_assert(igemm_resident_blocks(IGEMM_TILE_128x128) == 2 && igemm_resident_blocks(IGEMM_TILE_128x128, true) == 1 &&
              igemm_resident_blocks(IGEMM_TILE_128x64) == 3 && igemm_resident_blocks(IGEMM_TILE_128x64, true) == 2 &&
              igemm_resident_blocks(IGEMM_TILE_64x64) == 4 && igemm_resident_blocks(IGEMM_TILE_64x64, true) == 3 &&
              igemm_resident_blocks(IGEMM_TILE_256x64) == 1 && igemm_resident_blocks(IGEMM_TILE_256x64, true) == 1, "residency");
hipError_t igemm_init();   // raises the dynamic-LDS limit of the instantiations
// planes[p][i], p = 0..2: the bf16 pieces of w[i] (round to nearest even; w[i] = their sum up to 2^-26 |w[i]|)
hipError_t launch_split_weights(const float* w, unsigned short* planes, size_t n, hipStream_t stream);
// persistent stream-K launch over `nblocks` blocks; tiles that are cut are finished inside
// the launch by the last contributor (a.partial / a.tickets)
hipError_t launch_igemm(const IgemmArgs& a, int tile, int nblocks, hipStream_t stream);

// ---- batched plain GEMM with a continuous K-tile stream (gemm_stream.hip) -------------------
// C[b][m][n] = sum_k A[b][m][k] * W[b][n][k];  A [nbatch][M][K], W [nbatch][Npad][K], C [nbatch][M][Npad]
struct GemmStreamArgs {
    const float* A; const float* W; float* C;
    int M, K, Npad, nbatch;
    int mtiles, ntiles;      // filled by the launcher
};
hipError_t gemm_stream_init();
hipError_t launch_gemm_stream(GemmStreamArgs a, int tile, int nblocks, hipStream_t stream);

// ---- Winograd F(4x4,3x3) transforms (winograd.hip) ----------------------------------------
// V[36][T][cin_pad] = B^T d B of every 6x6 patch (T = N*ceil(H/4)*ceil(W/4)); pad 1, stride 1
hipError_t launch_wino_in(const float* x, float* V, int N, int H, int W, int pitch, int cin_pad, int pad_mode,
                          hipStream_t stream);
// U[36][out_pad][in_pad] = G g G^T of W[out_pad][9][in_pad] (device-side; the training step re-derives it per step)
hipError_t launch_wino_weights(const float* W, float* U, int out_pad, int in_pad, hipStream_t stream, int chunked = 0);
// weight gradient in the Winograd domain: dM[36][T][Cp] = A dy A^T per 4x4 output tile; grad[o][9][i] (+)= G^T dU G
hipError_t launch_wino_dout(const float* dy, float* dM, int N, int H, int W, int Cp, hipStream_t stream);
hipError_t launch_wino_dweights(const float* dU, float* grad, int out_pad, int in_pad, int accumulate, hipStream_t stream);
// conv1 -> conv2 inside one bottleneck on maps of at most 4x4 tiles: V2 = B^T PReLU(A^T M1 A + bias) B per image, the
// activation stays in LDS
struct WinoOutInArgs {
    const float* M; const float* bias; const float* slope; float* V;
    int H, W, C, th, tw, border_bias;
    long long T;
};
bool wino_out_in_supported(int H, int W, int C);
hipError_t launch_wino_out_in(const float* M, const float* bias, const float* slope, float* V, int N, int H, int W, int C,
                              int border_bias, hipStream_t stream);
// out = tail(A^T M A) of M [36][T][tail.cout_pad]
struct WinoOutArgs {
    const float* M;
    ConvTail tail;
    int N, H, W, th, tw;        // th, tw and T: filled by the launcher
    long long T;
};
hipError_t launch_wino_out(const float* M, const ConvTail& tail, int N, int H, int W, hipStream_t stream);

// ---- Winograd conv with GEMM and output transform in one kernel (wino_fused.hip) -----------------------------
// Vc [mbn][nkc][36][64 pieces][4]: the input transform of 32-tile groups in 8-channel K chunks (piece order: see
// wino_fused.hip); Uc [cout_pad/64][nkc][36][128 pieces][4]: G g G^T in the same chunk order (host packer)
hipError_t launch_wino_in_chunked(const float* x, float* Vc, int N, int H, int W, int pitch, int cin_pad, int pad_mode,
                                  hipStream_t stream);
struct WinoFusedArgs {
    const float* Vc; const float* Uc;       // Vc == null: the kernel transforms x itself (phased mode)
    const float* x;                         // phased mode: input [N,H,W,in_pitch] ...
    unsigned x_bytes;                       // ... and its size in bytes (<= 1 GiB; out-of-range reads return zeros)
    int in_pitch, pad_mode;
    ConvTail tail;
    int N, H, W, nkc;                       // nkc = cin_pad / 8
    int half_n;                             // 1: blocks of 32 tiles x 32 channels (k_wino_fused<., 1>) instead of 32 x 64
    int th, tw, mbn, nbn;                   // filled by the launcher
    long long T;
    unsigned long long* trace;              // diagnostics (-DFFR_TRACE build, option "wf_trace"): 10 words per wave, or null
    // split-operand form (wino_fused.hip): G g G^T as three bf16 planes in the order
    // [cout_pad/64][cin_pad/16][36][2 halves][3 planes][64 lanes][8 bf16]; non-null selects the form (Vc null, half_n 0)
    const unsigned short* U3;
};
inline size_t wino_split_u_elems(int cout_pad, int cin_pad) { return (size_t)(cout_pad / 64) * (cin_pad / 16) * 36 * 2 * 3 * 64 * 8; }
bool combine_in_c_supported(int H, int W, int C);
hipError_t launch_combine_in_c(const float* res, const float* scale, const float* sh, float* out, float* Vc, int N, int H,
                               int W, int C, hipStream_t stream);
int wino_fused_blocks(const WinoFusedArgs& a);
hipError_t wino_fused_init();
hipError_t launch_wino_fused(WinoFusedArgs a, hipStream_t stream);
inline size_t wino_chunked_floats(long long T, int cin_pad) { return (size_t)((T + 31) / 32) * 32 * 36 * cin_pad; }

// ---- wino_mixed.hip: exact tilings with tiles of 4 and 3 outputs per dimension (14 = 4+4+3+3, 7 = 4+3) ------------
// tile type tau = 2 * (MR == 3) + (MC == 3): (4,4), (4,3), (3,4), (3,3) with 36 / 30 / 30 / 25 xi, padded to 36 / 32 / 32 / 28
struct WinoMixedGeom { int n4, o4[2], n3, o3[2]; };      // per dimension: origins of the 4-output and of the 3-output segments
struct WinoInMixedArgs {
    const float* x; float* V[4];
    int N, H, W, pitch, nkc;
    WinoMixedGeom g;
    int goff[4];                            // first tile group (= block column) of each type
    long long T[4];
};
struct WinoMixedArgs {
    const float* V[4];                      // in: V[0] = base of the four regions (wino_mixed_v_floats); the launcher fills the rest
    const float* U[4];                      // weights per type in fragment order [cout_pad/64][K chunk][XP][128 pieces][4]
    ConvTail tail;
    int N, H, W, nkc;
    WinoMixedGeom g;                        // filled by the launcher, as everything below
    int mbn[4], half_blocks, nbn, tpi_off[4], tpi_total;       // half_blocks: the grid's first half, (4,4) | (4,3); the second runs (3,3) | (3,4)
    long long T[4];
    unsigned long long* trace;              // diagnostics (-DFFR_TRACE build, option "wf_trace"): 12 words per block, or null
};
bool wino_mixed_geom(int H, int W, WinoMixedGeom* g);
int wino_mixed_x(int tau);
int wino_mixed_xp(int tau);
size_t wino_mixed_v_floats(const WinoMixedGeom& g, int N, int cin_pad, size_t off[4]);
int wino_mixed_blocks(int N, int H, int W, int cout_pad);
size_t wino_mixed_u_floats(int tau, int cout_pad, int cin_pad);
int wino_mixed_blocks_launched(int N, int H, int W, int cout_pad);
hipError_t launch_wino_weights_mixed(const float* w, float* um, int cout_pad, int cin_pad, int tau, hipStream_t stream);
hipError_t wino_mixed_init();
hipError_t launch_wino_in_mixed(const float* x, float* V, int N, int H, int W, int pitch, int cin_pad, hipStream_t stream);
hipError_t launch_wino_fused_mixed(WinoMixedArgs a, hipStream_t stream);
hipError_t launch_combine_in_mixed(const float* res, const float* scale, const float* sh, float* out, float* V, int N, int H, int W,
                                   int C, hipStream_t stream);

// ---- measurement: what the fp32 matrix cores deliver on THIS device (probe.hip) ------------------------
// `blocks` x 256 threads, each wave issues iters x 16 independent-accumulator v_mfma_f32_32x32x2_f32 on random
// register operands; stamps[block*4 + {0,1,2,3}] = s_memtime begin/end, s_memrealtime begin/end of wave 0
hipError_t launch_mfma_probe(int iters, int blocks, unsigned long long* stamps, float* sink, hipStream_t stream);

// ---- trunk elementwise (elementwise.hip) -------------------------------------------
// stem: x_nchw[N,3,H,W] -> out[N,H,W,64] = PReLU(conv3x3(x)*bnscale + bias); w [27][64] folded
// input: x_nchw fp32, OR (xu8 != null) uint8 [N,H,W,3] RGB images preprocessed on the fly
// (BGR swap, h-flip where flip[n mod n_split] != 0, /255, (x-0.5)/0.5)
// With a second buffer (x2, or xu8b on the uint8 path) images [n_split, N) are read from it, 0 < n_split < N.
hipError_t launch_stem(const float* x_nchw, const unsigned char* xu8, const unsigned char* flip, const float* w27x64,
                       const float* bias, const float* slope, float* out, int N, int H, int W, hipStream_t stream,
                       const float* x2 = nullptr, int n_split = 0, const unsigned char* xu8b = nullptr);
// SE: scale[n][c] = sigmoid(fc2(relu(fc1(mean_hw res[n]))))   fc1 [C/16][C], fc2 [C][C/16]
// part: scratch [N][se_slices(N,HW)][C] floats (<= N*32*512)
int se_slices(int N, int HW);
hipError_t launch_se(const float* res, int N, int HW, int C, const float* fc1, const float* fc2,
                     float* scale, float* part, hipStream_t stream);
hipError_t launch_se_fc(const float* part, int N, int S, int HW, int C, const float* fc1, const float* fc2, float* scale,
                        hipStream_t stream);
// out[n,ho,wo,c] = res*scale[n,c] + (sc ? sc[n,ho,wo,c] : x[n,ho*stride,wo*stride,c])
hipError_t launch_combine(const float* res, const float* scale, const float* sc, const float* x,
                          float* out, int N, int Ho, int Wo, int C, int stride, hipStream_t stream);
// y[m][c] = x[m][c]*s[c] + t[c]    (Backbone.bn on the trunk output)
hipError_t launch_affine(const float* x, const float* s, const float* t, float* y, int M, int C,
                         hipStream_t stream);
// f[n][:] = l2norm( sum_splits partial[s][n][:] + bias )   (C = 512)
hipError_t launch_head_finish(const float* partial, int splits, int N, int C, const float* bias,
                              float* f, hipStream_t stream);
// layout: [N,P,C](pitch) <-> [N,C,P]
hipError_t launch_nhwc_to_nchw(const float* in, int in_pitch, float* out, int N, int P, int C,
                               hipStream_t stream);
hipError_t launch_nchw_to_nhwc(const float* in, float* out, int out_pitch, int N, int P, int C,
                               hipStream_t stream);
// copy rows [M][C] into channel slice [coff, coff+C) of a [M][pitch] buffer
hipError_t launch_copy_slice(const float* in, float* out, int M, int C, int pitch, int coff,
                             hipStream_t stream);
hipError_t launch_cosine(const float* a, const float* b, int n, int dim, float* score,
                         hipStream_t stream);
// calibration distance: out[0] = max|a - b|, out[1] = max|b| over rows x cols (pitched rows; a NaN difference counts as
// +inf); part: absdiff_scratch_floats() floats of scratch.  Two launches, deterministic
int absdiff_scratch_floats();
hipError_t launch_absdiff_max(const float* a, int a_pitch, const float* b, int b_pitch, int rows, int cols, float* part,
                              float* out, hipStream_t stream);

// ---- 1:N identification (search.hip) -------------------------------------------------
// norms[r] = |x[r]| of [n][512] rows (the sum of squares of k_cosine)
hipError_t launch_row_norms(const float* x, long long n, float* norms, hipStream_t stream);
// chunking of a search: probe tiles x gallery chunks (chunk_rows <= search_max_chunk_rows()); G >= 1
long long search_max_chunk_rows();
void search_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows);
// The arguments of one search block (search_core.h, which describes it).  The exact tile reads `gallery`, the coarse tile
// `plane`; rows 16-byte aligned, dim 512.  The lists of the probes that `live` leaves out are left as they are
struct SearchArgs {
    const float* query;       // [Q][512]
    const float* qnorm;       // [Q]
    const float* gallery;     // [G][512] (the exact tile)
    const uint16_t* plane;    // [G][512] bf16 of the normalised rows (the coarse tile)
    const float* gnorm;       // [G]
    long long G;
    long long chunk_rows;     // rows per chunk (the last one may be shorter), <= CT_MAX_CHUNK
    long long index_base;
    float* out_s;             // [S][Q][k]
    int64_t* out_i;
    const int* live;          // device, or null: the probes [*live, Q) are not searched (their tiles leave at once)
    int Q, k, nchunks, ntiles;
    const int32_t* subject;   // [G], < 0 = a removed row (SR_LIVE, SR_DISTINCT)
    int32_t* out_u;           // [S][Q][k] (SR_LIVE, SR_DISTINCT; not touched, may be null, where OUT_U is false)
    const uint32_t* tag;      // [G] one word per row (TAG): row g is a candidate of probe q iff (tag[g] & qmask[q]) != 0
    const uint32_t* qmask;    // [Q] one word per probe (TAG)
};
// The instantiations search_block<COARSE, SUBJ, OUT_U, TAG> has, by kernel: the exact tile with the policy SR_ROWS (k_search_topk),
// SR_LIVE and SR_DISTINCT (k_search_subjects: subject[G], < 0 = a removed row, never listed, and a third plane out_u of
// subjects; SR_DISTINCT lists subjects, each by its best row, k <= search_max_k_distinct()); the coarse tile with SR_ROWS
// (k_search_coarse) and, under the removal mask, SR_LIVE without the subject plane (k_search_coarse_live); the exact
// tile with each of the three policies under the per-probe filter of tag and qmask (k_search_filtered); and the coarse tile
// with SR_ROWS and SR_LIVE under that filter, without the subject plane (k_search_coarse_filtered, k_search_coarse_filtered_live).
// New kernels go at the end: the values are the positions in the table of launch_search
enum SearchKernel {
    SEARCH_ROWS, SEARCH_LIVE, SEARCH_DISTINCT, SEARCH_COARSE, SEARCH_COARSE_LIVE,
    SEARCH_FILTERED_ROWS, SEARCH_FILTERED_LIVE, SEARCH_FILTERED_DISTINCT,
    SEARCH_COARSE_FILTERED, SEARCH_COARSE_FILTERED_LIVE
};
int search_max_k_distinct();
// top-k lists [nchunks][Q][k] of every gallery chunk (one launch of nchunks x ntiles blocks); k <= 128.  The coarse kernels
// list by coarse score, index = gallery row: index_base 0, no live count, k = the shortlist's length
hipError_t launch_search(const SearchArgs& a, SearchKernel kernel, hipStream_t stream);
// S sorted lists [S][Q][k] -> [Q][k] (descending score, ties by ascending index; index < 0 = padding); S <= 4096; live as
// above.  out_u (or null: subject and distinct are not read): the lists carry a third plane of subjects; distinct: a winner
// whose subject is out already is dropped, k <= search_max_k_distinct().  S = 0: k slots of padding per probe
hipError_t launch_topk_merge(const float* score, const int64_t* index, const int32_t* subject, int S, int Q, int k, int distinct,
                             float* out_s, int64_t* out_i, int32_t* out_u, hipStream_t stream, const int* live = nullptr);

// ---- certified bf16 shortlist search (search_coarse.hip) ------------------------------
// rows the coarse pass lists per probe for a top-k (k <= coarse_max_k()), and the largest k it serves; distinct: for a list
// of subjects (ffr_search_topk_coarse_subjects)
int coarse_shortlist_size(int k, int distinct = 0);
int coarse_max_k(int distinct = 0);
// chunking of the exact pass over the probes that were not certified: as search_plan, with chunks fine enough that a few live
// probes still reach every CU
void coarse_fallback_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows);
// plane[r] = bf16(rows[r] / norms[r]) of [n][512] rows; *flag |= 1 when a norm is unsafe (not zero and outside [2^-60, 2^60])
hipError_t launch_coarse_pack(const float* rows, const float* norms, long long n, uint16_t* plane, int* flag, hipStream_t stream);
// k_search_coarse (live: k_search_coarse_live; filtered: k_search_coarse_filtered and k_search_coarse_filtered_live), for the
// table of launch_search: shortlists [nchunks][Q][kp] of every plane chunk, merged by launch_topk_merge
const void* search_coarse_kernel(bool live, bool filtered = false);
// exact scores of the shortlists sl[Q][kp], the certificate, the certified probes' top-k -> top[Q][k]; the others' ids ->
// ulist[0 .. *ucount) (ucount zero before the launch); certified[Q] (0 / 1) may be null.  subject[G] (or null): shortlists of
// live rows; top_u[Q][k] gets the subjects, and with distinct the lists hold subjects, each by its best row.  filtered: the
// shortlists came from k_search_coarse_filtered(_live); a list shorter than kp is then every row its probe may see, as it
// is under removals
hipError_t launch_search_rescore(const float* query, const float* qnorm, int Q, const float* gallery, const float* gnorm,
                                 const float* sl_s, const int64_t* sl_i, const int* plane_flag, long long G, int k, int kp,
                                 long long index_base, float* top_s, int64_t* top_i, int* certified, int* ulist, int* ucount,
                                 hipStream_t stream, const int32_t* subject = nullptr, int distinct = 0, int32_t* top_u = nullptr,
                                 bool filtered = false);
// uq[i] = query[ulist[i]], uqn[i] = qnorm[ulist[i]] for i < *ucount (grid sized for Q); with qmask (or null) also
// uqm[i] = qmask[ulist[i]], the mask words of a filtered search
hipError_t launch_probe_gather(const float* query, const float* qnorm, const int* ulist, const int* ucount, int Q, float* uq,
                               float* uqn, hipStream_t stream, const uint32_t* qmask = nullptr, uint32_t* uqm = nullptr);
// top[ulist[i]] = fb[i] for i < *ucount: the lists [k] of the exact pass back to their probes (fb_u -> top_u: their subject
// plane, or null)
hipError_t launch_topk_scatter(const float* fb_s, const int64_t* fb_i, const int* ulist, const int* ucount, int Q, int k,
                               float* top_s, int64_t* top_i, hipStream_t stream, const int32_t* fb_u = nullptr,
                               int32_t* top_u = nullptr);

// ---- clustering (cluster.hip) ----------------------------------------------------------
// chunking of the self-join: probe tiles x row chunks, sized for the blocks on and above the diagonal; N >= 1
void cluster_plan(long long N, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows);
// chunking of the row-range join: the N - N_old new rows in chunks under ceil(N / 32) probe tiles; 0 <= N_old <= N, N >= 1
void cluster_extend_plan(long long N_old, long long N, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows);
// rep[i] = smallest row of i's component under the links i - prior[i] and the edges s(i, j) > threshold, i < j, j >= N_old
// (seed, row-range join, flatten); an entry of prior outside [0, i] counts as i; rep may be prior.  prior = null with
// N_old = 0 and cluster_plan's chunking: no links, every pair i < j (init, join, flatten).  parent: N ints of scratch;
// norms = launch_row_norms(emb); N < 2^31, nchunks * ntiles < 2^31, rows 16-byte aligned
hipError_t launch_cluster_extend(const float* emb, const float* norms, long long N_old, long long N, float threshold, int ntiles,
                                 int nchunks, long long chunk_rows, const int64_t* prior, int* parent, int64_t* rep,
                                 hipStream_t stream);
// density-gated clustering over the edges of launch_cluster_extend (init, degree walk, gated walk, root, min, label):
// degree[i] = edges at i; core iff degree + 1 >= min_rows; rep[i] = smallest row of i's cluster (core components + the
// border rows attached by best score, then smallest core row); kind 2 / 1 / 0 = core / border / noise.  Scratch: parent,
// degree, root, minrow N ints each, best N 8-byte words; degree_out may be null; the plan is cluster_plan's
hipError_t launch_cluster_density(const float* emb, const float* norms, long long N, float threshold, int min_rows, int ntiles,
                                  int nchunks, long long chunk_rows, int* parent, int* degree, int* root, int* minrow,
                                  unsigned long long* best, int64_t* rep, uint8_t* kind, int32_t* degree_out, hipStream_t stream);
// blocks of a walk over a list of at most `rows` rows (the promoted pass of launch_cluster_density_extend, rows = N_old;
// the walks of launch_cluster_remove and launch_cluster_density_remove, rows = N): a fixed grid, the work is counted on the device
int cluster_list_grid(long long rows, int num_cus);
// launch_cluster_density over all N rows, from the state (rep, degree, best) of the first N_old: seed, degree walk and gated
// walk over the pairs with a new row (the plan is cluster_extend_plan's), the old rows they made core listed in plist[*pcount],
// the old-old edges at those, then root, min, label.  rep, degree, best [N] in and out (the caller's), kind [N] out.
// Scratch: parent, deg0, coremin, root, minrow N ints each, plist N_old ints, pcount one int
hipError_t launch_cluster_density_extend(const float* emb, const float* norms, long long N_old, long long N, float threshold,
                                         int min_rows, int ntiles, int nchunks, long long chunk_rows, int promoted_grid, int* parent,
                                         int* deg0, int* coremin, int* root, int* minrow, int* plist, int* pcount, int64_t* rep,
                                         uint8_t* kind, int32_t* degree, unsigned long long* best, hipStream_t stream);
// rows with keep[x] = 0 leave a single-link clustering rep_in (mark, list, walk over the pairs of the listed rows, flatten):
// rep[x] = -1 for a removed row, the guarded rep_in[x] where x's cluster lost no row, else the smallest row of x's component
// among the survivors of the clusters that lost one, under the edges s > threshold and the links x - prior[x] between two
// such rows; prior may be null, rep may be rep_in.  Scratch: parent, glabel, hit, list N ints each, mcount one int
hipError_t launch_cluster_remove(const float* emb, const float* norms, long long N, float threshold, int walk_grid,
                                 const int64_t* rep_in, const int64_t* prior, const uint8_t* keep, int* parent, int* glabel, int* hit,
                                 int* list, int* mcount, int64_t* rep, hipStream_t stream);
// rows with keep[x] = 0 leave a density-gated clustering whose state (rep, degree, best) the caller holds for all N rows:
// init, the removed rows listed in rlist, the walk that takes their edges from degree[], status (hit labels), seed and the
// lists llist (still-core rows of hit labels) and qlist (non-core survivors that choose again), the pair walk over llist,
// the walk that offers the core rows to qlist, then root, min, label.  rep, degree, best [N] in and out, kind [N] out; a
// removed row gets -1 / 0 / 0 / 0.  Scratch: parent, deg0, coremin, hit, root, minrow, rlist, llist, qlist N ints each,
// counts 3 ints; walk_grid = cluster_list_grid(N)
hipError_t launch_cluster_density_remove(const float* emb, const float* norms, long long N, float threshold, int min_rows,
                                         int walk_grid, const uint8_t* keep, int* parent, int* deg0, int* coremin, int* hit,
                                         int* root, int* minrow, int* rlist, int* llist, int* qlist, int* counts, int64_t* rep,
                                         uint8_t* kind, int32_t* degree, unsigned long long* best, hipStream_t stream);
// templates[c] = normalised sum of the normalised rows order[offsets[c] .. offsets[c+1]); norms may be null
hipError_t launch_cluster_templates(const float* emb, const float* norms, const int64_t* order, const int64_t* offsets,
                                    long long C, float* templates, hipStream_t stream);

// ---- face alignment (align.hip) --------------------------------------------------------
// landmarks[N][K][2], tmpl[K][2] fp32 -> A[N][6] fp64 (row-major 2x3, crop -> frame), valid[N]; 2 <= K <= 16; with a
// frame_index[N] (may be null) a face whose frame is outside [0,F) is invalid too
hipError_t launch_align_tfm(const float* landmarks, const float* tmpl, int N, int K, const int* frame_index, int F, double* A,
                            uint8_t* valid, hipStream_t stream);
// frames[F][H][W][3] uint8 (row pitch in bytes, pitch*H < 2^31) -> crop[N][oh][ow][3]; valid may be null; ow % 4 == 0,
// oh, ow <= 256, crop 4-byte aligned
hipError_t launch_align_warp(const uint8_t* frames, int F, int H, int W, int pitch, const int* frame_index, const double* A,
                             const uint8_t* valid, int N, int oh, int ow, uint8_t* crop, hipStream_t stream);

// LFW fold protocol on device; scratch = 400*32 ints, best_thr/test_acc = nf doubles (device)
hipError_t launch_fold_protocol(const float* score, const int* label, int n, int nf, int* scratch, double* best_thr,
                                double* test_acc, hipStream_t stream);

// ---- RecNet operators (recnet_ops.hip) ---------------------------------------------
// ss_space of models/recnet.py:226-236 for X[N,49,512]; writes bufS[n,j,512+i] = ss[i][j],
// zeros in channels [561,576), optional dense copy ss_out[N,49,49]
hipError_t launch_selfsim_space(const float* X, float* bufS, int pitchS, float* ss_out, int N,
                                hipStream_t stream);
struct ChannelPathWeights {   // device pointers, see pack.cpp ffr_load_recnet()
    const float* w1a;   // [32][49]   Conv4Channel.0.weight[:, :49]
    const float* w1b;   // [32][512]  Conv4Channel.0.weight[:, 49:]
    const float* b1;    // [32]
    const float* a1;    // [512] PReLU slopes (per row c)
    const float* A2;    // [32][32]  = W3*W2      (Conv4Channel.3 o Conv4Channel.2)
    const float* d2;    // [32]
    const float* a4;    // [512]
    const float* A3;    // [32][32]  = W6*W5
    const float* d3;    // [32]
    const float* a7;    // [512]
    const float* w8;    // [512][32] Conv4Channel.8.weight
    const float* b8;    // [512]
    const float* w8a;   // [16][64][16]  w8 in MFMA A-operand order: [c' tile][lane][k-step] = w8[32t + (lane&31)][2ks + (lane>>5)]
    const float* b8a;   // [16][2][16]   b8 in accumulator order: [c' tile][lane>>5][reg] = b8[32t + (r&3) + 8(r>>2) + 4h]
};
// feat_channel_raw[c][p] = sum_c' sigmoid(Conv4Channel(..))[c][c'] X[c'][p]; written to
// bufF[n,p,512+c] and W-flipped to bufF[n,flip(p),c]  (bufF pitch 1024)
// dbg_ss / dbg_M (parity tests, optional): ss_channel and M_channel [512][512] of image 0, which the path never stores
hipError_t launch_channel_path(const float* X, const ChannelPathWeights& w, float* bufF, int pitchF, int N, hipStream_t stream,
                               float* dbg_ss, float* dbg_M, int dbg_n /* the image dbg_ss / dbg_M are stored for */,
                               int row_blocks /* 1 | 2 | 4 blocks per image: plan_channel_rows */,
                               unsigned long long* trace = nullptr /* -DFFR_TRACE: 8 words per block */);
// feat_space: out[n,j,c] = sum_i ms[n,j,i] * X[n,i,c]   (ms pitch = ms_pitch, out pitch/coff)
hipError_t launch_space_apply(const float* X, const float* ms, int ms_pitch, float* out, int out_pitch,
                              int out_coff, int N, hipStream_t stream);
// f_new[n][c] = mean_p feat[n,p,c]
hipError_t launch_avgpool49(const float* feat, float* f_new, int N, int C, hipStream_t stream);

}  // namespace ffr
