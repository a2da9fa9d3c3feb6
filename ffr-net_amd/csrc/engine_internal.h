// Types and helpers shared by the host translation units of libffrnet_hip.so: plan.cpp (convolution planner), conv.cpp
// (launchers), pack.cpp (weight packer, ffr_load_*), forward.cpp (workspace and forward pipelines), engine.cpp (the rest of
// the C ABI) and train_layer.cpp / train_graph.cpp / train_params.cpp (the RecNet training step; their own types are in
// train_internal.h).  Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/ffrnet.h"
#include "../../include/ffrnet_train.h"
#include "ffr_kernels.h"

namespace ffr_eng {

using namespace ffr;

struct TrainState;   // train_internal.h

struct ConvW {
    int cin = 0, cin_pad = 0, cout = 0, cout_pad = 0, R = 1, S = 1, stride = 1, pad = 0, pad_mode = 0, border = 0;
    float* w = nullptr;
    float* bias = nullptr;
    float* slope = nullptr;
    float* wu = nullptr;     // Winograd F(4,3) weights [36][cout_pad][cin_pad] (G g G^T, BN folded) or null
    float* wum[4] = {nullptr, nullptr, nullptr, nullptr};   // mixed tile sizes (wino_mixed.hip): weights of the tile types (4,3), (3,4), (3,3) in fragment
                             // order at [1..3] ([0] = wuc); derived on the device from `w` the first time a launch of this layer is eligible
                             // (pack.cpp, ensure_mixed_weights), null before
    bool wum_gave_up = false;   // the device could not hold this layer's extra sets: it stays on padded F(4x4) tiles (never retried)
    unsigned short* w3 = nullptr;   // `w` as three bf16 planes [3][cout_pad][KK] for k_igemm's split-operand form (layers that always run
                             // direct, and the FC; split from the double-precision fold at load time), or null: the fp32 form
    unsigned short* wu3 = nullptr;  // G g G^T as three bf16 planes in the order of k_wino_fused's split-operand form (ffr_kernels.h: WinoFusedArgs::U3;
                             // layers with cin_pad <= wf_phased_maxk, split from the double-precision fold at load time), or null
    float* wuc = nullptr;    // the same in the K-chunk order k_wino_fused streams ([cout_pad/64][cin_pad/8][36][128][4]) or null
    // per-layer arithmetic plan (ffr_layer_set_arith / ffr_calibrate): a layer with wu pinned to direct runs exactly
    // what it runs under option wino = 0.  ffr_load_* reset it (pack_conv).
    bool direct = false;
    double sensitivity = -1.0;   // last ffr_calibrate: end-to-end difference with only this layer on Winograd (-1: none)
};

struct Block {
    int cin = 0, depth = 0, stride = 1;
    bool has_sc = false;
    ConvW c1, c2, sc;
    float* fc1 = nullptr;
    float* fc2 = nullptr;
};

// Experiment knobs (ffr_set_option).  Defaults are the measured best; nothing is read from the
// environment.
struct Options {
    int wino = 1;                 // 0: every 3x3 convolution of the inference path runs as a direct implicit GEMM
    int wino_mincin = 64;         // smallest padded input-channel count packed for Winograd (takes effect at load time)
    int wino_fused = 1;           // 0: Winograd convolutions run as transform kernels around the batched GEMM
    int wf_phased_maxk = 128;     // largest padded cin for which k_wino_fused transforms its own input
    long long wf_minblocks = 200; // fewest block tiles for which the fused kernel is used
    int se_maxtiles = 256;        // most 4x4 tiles per image for which the SE squeeze comes from the fused kernel's tile sums (0: own pass)
    int wf_tailsplit = 1;         // 1: images that do not fill whole rounds of block tiles run on the second stream
    int gemm_stream = 1;          // 0: the 36 Winograd GEMMs go through k_igemm (batched) instead of k_gemm_stream
    int sk_minunits = 18;         // smallest number of K-tiles a stream-K block may own
    int wf_mixed = 1;             // 1: 14x14 maps are tiled 4+4+3+3 (k_wino_fused_mixed) when the launch gives every CU two blocks or more
    int channel_rows = 0;         // k_channel_path: blocks per image (1, 2, 4); 0 = from the batch and the CU count (round 5)
    int igemm_split = 1;          // 1: direct convolutions whose weights were split at load time run k_igemm's split-operand form (bf16 matrix cores)
    int wf_split = 1;             // 1: fused Winograd launches that transform their own input run the split-operand K loop where the layer has the planes
    int combine_v = 1;            // 1: a bottleneck's combine also writes V for the next conv1 when that runs k_wino_fused from V
    int wf_trace = 0, igemm_trace = 0;   // -DFFR_TRACE builds only: per-launch phase stamps on stderr (synchronises)
    // Retired in round 6, their A/B settled (EXPERIMENTS.md): wino_112, wf_halfblocks, wf_mapv, wf_mapx, wf_maph, wm_xcdpairs,
    // wino_slice_mb, gs_tile, wino_oi, se_fuse, igemm_tile64 -- the code keeps the measured-best setting of each (of the block
    // maps wf_mapv, wf_mapx, wf_maph and wm_xcdpairs only that one: the maps that lost are gone from the kernels).
};

struct DevBuf { char* p = nullptr; size_t bytes = 0; };

struct ProfRec {
    hipEvent_t e0, e1;
    int kc;
    double flops, bytes, fexec, fuse;
    bool side;          // enqueued on the handle's second stream: runs beside a launch of the main stream
};

}  // namespace ffr_eng

struct ffr_handle {
    int device = 0;
    int num_cus = 256;       // multiProcessorCount of the device
    hipStream_t side = nullptr;          // second stream: the few images split off a fused Winograd launch run beside it
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    float* zero = nullptr;   // 128 KiB zero page (source of zero-padded taps, >= any cin_pad)
    // weights
    std::vector<void*> enc_allocs, rec_allocs;
    bool enc_loaded = false, rec_loaded = false;
    size_t enc_weight_bytes = 0, rec_weight_bytes = 0;      // device bytes of the packed weights (ffr_memory_stats)
    size_t mixed_weight_bytes = 0;                          // of them: the lazily derived weight sets of the exact 14x14 tiling
    double enc_load_s = 0.0, rec_load_s = 0.0, mixed_pack_s = 0.0;   // wall seconds of the last ffr_load_* / of all lazy packs
    size_t split_weight_bytes = 0;                          // of enc_weight_bytes: the bf16 planes of k_igemm's split-operand form
    size_t wf_split_weight_bytes = 0;                       // of enc_weight_bytes: the bf16 planes of k_wino_fused's split-operand form
    long long wf_split_launches = 0;                        // k_wino_fused launches in the split-operand form since ffr_create
    bool mixed_gave_up_logged = false, split_gave_up_logged = false;
    int mixed_ready_n = 0, mixed_ready_h = 0, mixed_ready_w = 0;     // prepare_mixed_weights ran for batches up to n of h x w (a shortcut only:
                                                                     // readiness itself is per layer, ConvW::wum / wum_gave_up)
    float *stem_w = nullptr, *stem_b = nullptr, *stem_s = nullptr;
    std::vector<ffr_eng::Block> blocks;      // 24 / 49 / 50 bottlenecks: Backbone(50 | 100 | 152), with or without SE
    float *bn_s = nullptr, *bn_t = nullptr;
    ffr_eng::ConvW fc;
    ffr_eng::ConvW sp[9], fm[3], mg[3];
    ffr::ChannelPathWeights cw{};
    // grow-only device buffers (grow(), forward.cpp): the workspace arena, the stream-K arrival counters (int, zero between
    // launches), and the scratch of ffr_search_topk (probe norms + per-chunk top-k lists), of ffr_cluster_threshold /
    // ffr_cluster_extend (row norms [N] + union-find parent [N]) and of ffr_embed_aligned (transforms, valid flags, crops)
    ffr_eng::DevBuf arena, tickets, search, cluster, align;
    ffr_eng::Options opt;
    // profiling
    bool prof = false;
    std::vector<ffr_eng::ProfRec> prof_log;
    std::vector<hipEvent_t> ev_pool;
    // RecNet training state (train_params.cpp), or null
    ffr_eng::TrainState* train = nullptr;
    // weight-gradient launch plans of the most recent backward (ffr_train_wgrad_plan)
    std::vector<ffr_wgrad_launch> wgrad_log;
    // plan record of the convolution launchers (ffr_conv_plan_record / ffr_conv_plan_read): filled by run_conv's launchers while on
    bool conv_rec = false;
    std::vector<ffr_conv_launch> conv_log;
    // bumped whenever device memory a caller may have captured (hipGraph) moves: every allocation of grow(), weight
    // reload, ffr_train_init
    unsigned long long generation = 1;
};

namespace ffr_eng {

int fail(ffr_handle* h, int code, const char* fmt, ...);

#define HIPCK(h, expr)                                                                          \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(h, FFR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define RC(expr)                  \
    do {                          \
        int _rc = (expr);         \
        if (_rc != FFR_OK) return _rc; \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Every C entry point runs on its handle's device and leaves the calling thread's current device as it found it
// (a process may hold several handles / torch may have another device current).
struct DeviceScope {
    int prev = -1;
    bool switched = false, ok = true;
    explicit DeviceScope(int dev) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; switched = ok && prev >= 0; }
    }
    ~DeviceScope() { if (switched) hipSetDevice(prev); }
};
#define FFR_DEVICE_SCOPE(h) ffr_eng::DeviceScope _dev_scope((h) ? (h)->device : -1)

// ---- profiling scope: hipEvents on the launch stream around one launch -----------------
struct Scope {
    ffr_handle* h;
    hipStream_t st;
    ProfRec r;
    bool on;
    // fexec: FLOPs the launch executes (default: flops); fuse: the part of them that is not padding (default: flops)
    Scope(ffr_handle* h_, hipStream_t st_, int kc, double flops, double bytes, double fexec = -1.0, double fuse = -1.0)
        : h(h_), st(st_), on(h_->prof) {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!h->ev_pool.empty()) { e = h->ev_pool.back(); h->ev_pool.pop_back(); }
            else hipEventCreate(&e);
            return e;
        };
        r.e0 = get(); r.e1 = get(); r.kc = kc; r.flops = flops; r.bytes = bytes; r.fexec = fexec < 0 ? flops : fexec; r.fuse = fuse < 0 ? flops : fuse;
        r.side = h->side && st == h->side;
        hipEventRecord(r.e0, st);
    }
    ~Scope() {
        if (!on) return;
        hipEventRecord(r.e1, st);
        h->prof_log.push_back(r);
    }
};

struct SD {
    std::map<std::string, const ffr_tensor_desc*> m;
    ffr_handle* h;
    int rc = FFR_OK;
    const float* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = m.find(name);
        if (it == m.end()) { rc = fail(h, FFR_ERR_KEY, "state_dict entry '%s' is missing", name.c_str()); return nullptr; }
        const ffr_tensor_desc* d = it->second;
        bool ok = d->data && d->ndim == (int)shape.size();
        int i = 0;
        for (int64_t s : shape) { if (ok && d->shape[i] != s) ok = false; ++i; }
        if (!ok) { rc = fail(h, FFR_ERR_KEY, "state_dict entry '%s' has an unexpected shape", name.c_str()); return nullptr; }
        return d->data;
    }
};

// pack.cpp
struct BNFold { std::vector<double> s, t; };
bool bn_fold(SD& sd, const std::string& p, int C, BNFold& o);
int upload(ffr_handle* h, std::vector<void*>& owner, const std::vector<float>& v, float** out);
int pack_conv(ffr_handle* h, std::vector<void*>& owner, const float* W, int cout, int cin, int R, int S,
              const BNFold* in_bn, const BNFold* out_bn, const float* slope, int stride, int pad, int pad_mode, ConvW* L);
void split_bf16x3(double w, unsigned short out[3]);       // p1 = bf16(w), p2 = bf16(w - p1), p3 = bf16(w - p1 - p2), round to nearest even
void pack_wino_split(const double* ud, int cout_pad, int cin_pad, unsigned short* pl);
void free_list(std::vector<void*>& v);
int ensure_mixed_weights(ffr_handle* h, ConvW& L, std::vector<void*>& owner, bool strict);
int prepare_mixed_weights(ffr_handle* h, int N, int H, int W, size_t wino_cap);
struct RecLayer { const char* prefix; int cin, cout; };
extern const RecLayer REC_LAYERS[15];       // RecNet's ConvLayers: h->sp[0..8], h->fm[0..2], h->mg[0..2]
inline ConvW& rec_conv(ffr_handle* h, int i) { return i < 9 ? h->sp[i] : i < 12 ? h->fm[i - 9] : h->mg[i - 12]; }

// What a caller asks of a convolution's arithmetic; the values are those of use_wino in ffr_op_conv3x3.  Auto: the planner
// decides (option wino, the layer's plan, wino_fused_form, the tail split).  Fused / FusedHalf: k_wino_fused with 32 x 64 /
// 32 x 32 blocks.  Unfused: transform kernels + batched GEMM.  Mixed: the exact 4+4+3+3 tiling of a 14x14 map.
// FusedSplit: Fused with the in-kernel transform and the split-operand K loop (refused where the layer or the launch cannot).
enum class ConvForce { Auto = -1, Direct = 0, Fused = 1, Unfused = 2, FusedHalf = 3, Mixed = 4, FusedSplit = 5 };

struct ConvCall {
    const float* x; int N, H, W, in_pitch;
    const float* resid; int res_pitch;
    float* out; int out_pitch, out_coff, cout_store;
    int flags; int tile;
    float* partial; size_t partial_cap;   // floats
    int* tickets; size_t tickets_cap;
    float* winoV; float* winoM; size_t wino_cap;   // Winograd scratch (floats each), or null
    ConvForce force = ConvForce::Auto;
    int wino_stage = 0;                            // 0 whole conv; 1 stop after the GEMM (M stays in winoM); 2 V is ready in winoV
    bool v_mixed = false;                          // with wino_stage 2: V is in the four-region layout of wino_mixed.hip (k_combine_in_mixed wrote it)
    bool v_chunked = false;                        // with wino_stage 2: V is in the K-chunked fragment order of k_wino_fused (ConvPlan::takes_v)
    float* tile_sums = nullptr;                    // Winograd paths only: the rule is ConvTail::tile_sums' (ffr_kernels.h)
};

// One planned k_igemm launch (plan_gemm_launch): tile config, persistent blocks, K-tiles a block owns at least, the tile grid, its
// (tile, K-tile) units, whether a tile is cut, and which piece of the call's stream-K scratch does not hold it (null: it fits)
struct GemmPlan { int tile, nblocks, granule, mtiles, ntiles; long long units; bool cut; const char* nomem; };

// One entry of a convolution's plan: what the plan record shows of it, and what its launcher needs that is a decision rather
// than a tensor.  k_gemm_stream's tile and blocks and the fused kernels' form and block tiles are in rec; the Winograd paths are
// only chosen when the scratch holds them, so only a k_igemm entry can fail to fit (gemm.nomem).
struct ConvLaunch {
    ffr_conv_launch rec{};
    GemmPlan gemm{};                // k_igemm entries
    int n0 = 0;                     // the entry covers the images [n0, n0 + rec.images) of the call (n0 > 0: the rest of a tail split)
};

// Which kernels one convolution launches and how (plan_conv; run_conv executes the entries)
struct ConvPlan {
    enum Path { Direct, Mixed, Fused, Unfused } path = Direct;
    bool half_n = false;            // Fused: blocks of 32 tiles x 32 channels (else 32 x 64)
    bool phased = false;            // Fused: the kernel transforms its own input, V never exists in memory
    bool split = false;             // Fused + phased: the K loop runs on the bf16 matrix cores from the layer's three planes (ConvW::wu3)
    int n_main = 0;                 // Fused: the first n_main images run fused and the rest Unfused (0: no split)
    hipStream_t side = nullptr;     // ... the rest is enqueued first, on this stream (null: after the main part on the launch stream)
    bool takes_v = false;           // the whole conv runs fused from a V in k_wino_fused's order (a combine may write it)
    const char* refused = nullptr;  // the call cannot run as asked: why (run_conv fails with FFR_ERR_STATE)
    // the launches, in launch order: one, or for a tail split its header (FFR_CP_TAIL_SPLIT, no launch), the part enqueued first
    // and the other part (none when refused)
    int n_launch = 0;
    ConvLaunch launch[3];
};

// Does layer L run Winograd when the caller leaves the choice to the planner (ConvForce::Auto)?  Option wino and the layer's plan.
inline bool layer_wino(const ffr_handle* h, const ConvW& L) { return h->opt.wino != 0 && !L.direct; }
// plan.cpp
ConvForce wino_fused_form(const ffr_handle* h, int cin_pad, int cout_pad, long long T, double x_bytes, ConvForce ask);
bool wino_mixed_eligible(const ffr_handle* h, const ConvW& L, int N, int H, int W, int in_pitch, size_t wino_cap, ConvForce force);
ConvPlan plan_conv(const ffr_handle* h, const ConvW& L, const ConvCall& c);
ConvCall conv_part(const ConvW& L, const ConvCall& c, int n0, int n);
void plan_igemm(long long M, int cout_pad, int nkt, int nbatch, int force_tile, int min_units, int* tile, int* nblocks, int* granule,
                bool split = false);
int plan_channel_rows(int N, int num_cus, int forced);
ConvLaunch plan_gemm_launch(const ffr_handle* h, const ConvCall& c, int path, int images, long long M, int cout_pad, int nkt, int nbatch,
                            bool split);
// conv.cpp
int run_conv(ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvPlan& p, hipStream_t st);      // executes the ready plan p of call c
int run_conv(ffr_handle* h, const ConvW& L, const ConvCall& c, hipStream_t st);                         // plans, then executes

// Hands out 256-byte aligned pieces of one buffer; on a null base it only measures (off = the bytes the pieces need)
struct Arena {
    char* base; size_t off = 0;
    explicit Arena(char* b) : base(b) {}
    template <class T = float> T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

struct Work {
    // encoder
    float *bufA, *bufB, *t1, *res, *sc, *scale, *se_part, *trunk_bn;
    // shared
    float* partial; size_t partial_cap;
    int* tickets; size_t tickets_cap;
    float *winoV, *winoM; size_t wino_cap;
    // recnet
    float *X, *bufS, *bufF, *bufM, *s256a, *s256b, *s256c, *ms, *m512a, *m512b, *m512c, *dbg;
    size_t total;
};

// forward.cpp
Work layout(const Options& opt, char* base, int N, int H, int W);
inline ConvCall conv_call(const Work& w, ConvForce force = ConvForce::Auto) {     // a call with the scratch of w; the rest to fill in
    ConvCall c{};
    c.partial = w.partial; c.partial_cap = w.partial_cap; c.tickets = w.tickets; c.tickets_cap = w.tickets_cap;
    c.winoV = w.winoV; c.winoM = w.winoM; c.wino_cap = w.wino_cap; c.force = force;
    return c;
}
// The one place a DevBuf is allocated: enough already -> nothing; else synchronise, free, hipMalloc (and zero fill), and
// ++generation -- a graph captured around an earlier call points at the old buffer.  FFR_ERR_NOMEM names `what`.
int grow(ffr_handle* h, DevBuf& b, size_t need_bytes, const char* what, bool zeroed = false);
int ensure_arena(ffr_handle* h, int N, int H, int W, Work* w);
int ensure_arena_encoder(ffr_handle* h, int N, int H, int W, Work* w);     // + the exact-tiling weight sets an encoder forward of this size uses
// uint8 HWC RGB input of the stem; with img2, images [n_split, N) come from img2 and flip[] has one flag per pair
struct U8In { const unsigned char* img; const unsigned char* flip; const unsigned char* img2 = nullptr; };
int run_trunk(ffr_handle* h, const Work& w, const float* x_nchw, int N, int H, int W, int n_blocks, hipStream_t st,
              float** out_ptr, int* oh, int* ow, int* oc, const U8In* u8 = nullptr, const float* x2 = nullptr, int n_split = 0);
int run_encoder(ffr_handle* h, const Work& w, const float* x, int N, int H, int W, float* featmap_nhwc, float* f,
                hipStream_t st, const U8In* u8 = nullptr, const float* x2 = nullptr, int n_split = 0);
struct RecDebug { float *ss_space, *M_space, *feat_space, *feat_channel_raw, *feat_channel, *ss_channel0, *M_channel0; int image = 0; };   // ss_channel0 / M_channel0: of image `image`
int conv_rec(ffr_handle* h, const Work& w, const ConvW& L, const float* x, int in_pitch, const float* resid,
             int res_pitch, float* out, int out_pitch, int out_coff, int flags, int N, hipStream_t st);
int run_recnet(ffr_handle* h, const Work& w, int N, float* f_new, const RecDebug* dbg, hipStream_t st);
int check_fwd(ffr_handle* h, bool need_enc, bool need_rec, int N);
// conv.cpp: plain GEMMs through k_igemm (the training step)
int gemm_rows(ffr_handle* h, const Work& w, const float* A, int a_pitch, int K_pad, const float* W, const float* bias,
              int N_pad, float* out, int out_pitch, long long rows, const float* resid, int res_pitch, int flags,
              hipStream_t st);
int gemm_batched(ffr_handle* h, const Work& w, const float* A, long long a_bstride, int K_pad, const float* W,
                 long long w_bstride, int N_pad, float* out, int out_pitch, long long out_bstride, int M, int nbatch,
                 hipStream_t st);
// train_params.cpp
void train_free(ffr_handle* h);

}  // namespace ffr_eng
