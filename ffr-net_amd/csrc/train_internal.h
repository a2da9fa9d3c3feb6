// RecNet training step, host side: the types of its three units and the few functions that
// cross them.  train_layer.cpp: the ConvLayer and Linear operators; train_graph.cpp: the network (contexts, scratch, forward,
// backward, losses); train_params.cpp: the parameter store.  Included by those three only.
#pragma once
#include "engine_internal.h"
#include "train_kernels.h"

// One launch of the training step under a profiling scope of its kernel class (ffr_profile_*; bench.py --workload train
// itemises the step with them).  Costs nothing when profiling is off; `st` is the launch stream of the calling function.
#define TLAUNCH(kc, call) do { Scope _ps(h, st, kc, 0.0, 0.0); HIPCK(h, call); } while (0)

namespace ffr_eng {

const int N_CLASSES = 10575, CLS_PAD = 10624;
const float COSFACE_S = 30.0f, COSFACE_M = 0.40f;

// ---- the ConvLayer and Linear operators (train_layer.cpp) -------------------------------------------------------------
// One ConvLayer (reflect-pad -> conv3x3 no bias -> BatchNorm2d -> PReLU) in training form.
// Weights stay in the kernel layout [cout_pad][9][cin_pad] (no BN fold: the statistics are the batch's).
struct TLayer {
    std::string name = "op";                       // state_dict prefix (the weight-gradient plan record)
    int cin = 0, cin_pad = 0, cout = 0, cout_pad = 0;
    int dgrad_width = 0;                           // input channels whose data gradient the backward produces (0: none)
    float *w = nullptr, *gamma = nullptr, *beta = nullptr, *slope = nullptr;      // parameters
    float *gw = nullptr, *ggamma = nullptr, *gbeta = nullptr, *gslope = nullptr;  // gradients
    float *rmean = nullptr, *rvar = nullptr;                                      // running statistics
};

struct Lin {
    std::string name;                       // state_dict prefix (the weight-gradient plan record)
    int in = 0, out = 0, in_pad = 0, out_pad = 0;
    float *w = nullptr, *b = nullptr, *gw = nullptr, *gb = nullptr;
};

// what one forward call keeps of a layer for its backward
struct TSaved {
    const float* x = nullptr; int x_pitch = 0;     // the layer's input
    float* y = nullptr;                            // raw convolution output [rows][cout_pad]
    BnBuffers bn{};
};

// What one ConvLayer backward needs of the scratch, in floats: layer_scratch() is the single definition
struct LayerScratch {
    size_t part = 0;                         // BatchNorm slice partials (doubles)
    size_t wd = 0, dxp = 0, dy = 0;          // data-gradient weights; 9x9 padded data gradient; gradient wrt the raw convolution output
    size_t U = 0, canvas = 0;                // Winograd weights (re-derived per use); dy in a zero-bordered 8x8 map (Winograd data gradient)
    size_t edgeA = 0, edgeW = 0, edgeO = 0;  // bottom-row / right-column GEMMs: gathered operands, weights, outputs [2][imgs*9][need_pad]
};
LayerScratch layer_scratch(int cin_pad, int cout_pad, int dgrad_width, int imgs);
void grow_to(LayerScratch& a, const LayerScratch& b);       // a = max(a, b), buffer by buffer

// Capacity of the split-K slabs of the weight gradient, in floats.  An INPUT of the weight-gradient plan, not a derived size:
// launch_wgrad and launch_wgrad_batched lower `splits` and the tail split until the slabs fit, so another capacity is another
// plan record (profiles/wgrad_plan.txt) and another summation order.
const size_t NET_SLAB_FLOATS = (size_t)4 * 512 * 9 * 1536;                                  // the network
inline size_t op_slab_floats(const TLayer& L) { return (size_t)16 * L.cout_pad * 9 * L.cin_pad; }   // ffr_op_convlayer_train

struct TScratch {
    double* part = nullptr;
    float *wd = nullptr, *dxp = nullptr, *dy = nullptr, *U = nullptr, *canvas = nullptr, *edgeA = nullptr, *edgeW = nullptr, *edgeO = nullptr;
    LayerScratch cap;                                // their capacities
    float* slabs = nullptr; size_t slab_floats = 0;  // split-K slabs of the weight gradient
    bool wino = true;   // ffr_train_option("winograd")
    int fused = 1;      // ffr_train_option("fused"): 1 = Winograd launches that fill the chip run k_wino_fused on the live weights, 2 = all of them (tests), 0 = none
    bool fold = true;                              // ffr_train_option("fold_channel")
};
void carve_scratch(Arena& a, const LayerScratch& cap, size_t slab_floats, TScratch& s);
void carve_bn(Arena& a, int G, int Cp, BnBuffers& b);

// channels [coff, ..) of NHWC rows of `pitch` floats
struct Slice { float* p = nullptr; int pitch = 0, coff = 0; };
struct CSlice { const float* p = nullptr; int pitch = 0, coff = 0; };
// y = conv(reflect_pad(x)); batch statistics; out = PReLU(BN(y)) (+ resid) (sigmoid when flags & 1)
struct LayerFwd { const TLayer& L; TSaved& sv; CSlice x, resid; Slice out; int flags = 0; };
// da: gradient wrt the layer's PReLU output.  Produces the parameter gradients and, when dx.p is not null,
// dx[row][dx.coff + c] = (data gradient of the first L.dgrad_width input channels) (+ add)
struct LayerBwd { const TLayer& L; const TSaved& sv; CSlice da; Slice dx; CSlice add; int accumulate = 1; };
int layer_forward(ffr_handle* h, const Work& w, TScratch& s, int G, int N, const LayerFwd& f, hipStream_t st);
int layer_backward(ffr_handle* h, const Work& w, TScratch& s, int G, int N, const LayerBwd& b, hipStream_t st);

// Operands of a weight-gradient GEMM in its two forms: taps 1, grad[cout_pad][cin_pad] (+)= dy^T x over plain rows (a Linear);
// taps 9, grad[cout_pad][9][cin_pad] (+)= dy^T gather(x) over the taps of reflect-padded 7x7 maps.  run_wgrad: scope + launch + plan record
WgradArgs wgrad_args(ffr_handle* h, CSlice dy, int cout_pad, CSlice x, int cin_pad, long long rows, int taps);
int run_wgrad(ffr_handle* h, TScratch& s, const std::string& name, const WgradArgs& a, float* grad, int accumulate, int nbatch,
              double useful_flops, hipStream_t st);

// ---- the network (train_graph.cpp) -------------------------------------------------------------------------------------
// activations one forward call keeps for its backward
struct Ctx {
    int G = 0, N = 0;
    void* mem = nullptr;
    float *X, *bufS, *bufF, *bufM, *ms, *featnew;
    TSaved sp[9], fm[3], mg[3];
    float* out_sp[9]; float* out_fm[2]; float* out_mg[2];
    float *Xt, *Xht, *cat, *h1pre, *h1, *t2, *h2pre, *h2, *t5, *h3pre, *h3, *Mc, *raw;
    float *fnew, *fn, *fnorm, *cosv, *wn, *wnorm;
    int* label;
    bool valid = false, folded = false;
};
void free_graph(TrainState* t);      // contexts and scratch

// ---- the parameter store (train_params.cpp) ----------------------------------------------------------------------------
enum SegKind { SEG_CONV, SEG_VEC, SEG_LIN };
struct Seg {
    std::string key;
    SegKind kind;
    size_t off = 0, n_native = 0, n_natural = 0;
    int d0 = 0, d1 = 0, p0 = 0, p1 = 0;     // natural dims (cout,cin | n,1 | out,in) and their padded sizes
    int colperm = 0;                        // Linear(561,32): native columns = [ss_channel (512) | X (49) | pad]
    size_t native_index(size_t i) const {
        if (kind == SEG_VEC) return i;
        if (kind == SEG_CONV) {
            const size_t t = i % 9, ci = (i / 9) % d1, co = i / 9 / d1;
            return (co * 9 + t) * p1 + ci;
        }
        const size_t in = i % d1, o = i / d1;
        const size_t col = colperm ? (in < 49 ? 512 + in : in - 49) : in;
        return o * p1 + col;
    }
};

struct TrainState {
    std::vector<void*> allocs;
    std::vector<Seg> segs;
    std::map<std::string, int> seg_of;
    std::map<std::string, std::pair<float*, int>> running_of;     // key -> (device ptr, n)
    size_t n_flat = 0;
    float *P = nullptr, *Gr = nullptr, *M1 = nullptr, *M2 = nullptr, *running = nullptr;
    long long nbt = 0;             // BatchNorm updates since ffr_train_init (num_batches_tracked increments)
    TLayer sp[9], fm[3], mg[3];
    Lin lin[6];
    float *a[3] = {nullptr, nullptr, nullptr}, *ga[3] = {nullptr, nullptr, nullptr};
    float *clsW = nullptr, *gclsW = nullptr;
    int adam_step = 0;
    Ctx ctx[2];
    // backward scratch, sized for `scratch_imgs`
    int scratch_imgs = 0;
    void* scratch_mem = nullptr;
    TScratch sc;
    float *dFeatNew, *d512a, *d512b, *dBufM, *extM, *dF, *d256a, *d256b, *d256c, *dms;
    float *dRawt, *dMc, *dt, *d32a, *d32b, *rowdot, *dcos, *dfn, *df, *dwn, *wnT, *wT;
    // native loss items (ffr_train_losses)
    float *lYht, *lYh, *df_ext, *loss_out;
    float *foldA[2], *foldd[2], *gfoldA, *gfoldd;     // Conv4Channel pairs folded to 32x32 (+ their gradients)
    double *p_sss, *p_ssc, *p_vec, *p_ce;
    int* hit;
    // dcos / df_ext / extM hold the loss gradients of the forward in this slot (-1: of none).  Set by train_losses; reset by whatever
    // overwrites them: any backward, a new forward into that slot, a reallocation of the scratch
    int loss_grads_slot = -1;
    bool fold_ready = false;       // foldA / foldd hold the products of the live weights (a folded forward since the scratch was allocated)
    // gradient buckets of the data-parallel exchange: contiguous ranges of the flat buffer in the order the backward
    // finishes them (classifier, Conv4Merge, ChannelFlipMerge, Conv4Channel, Conv4Space); one event per bucket
    static const int NBUCKET = 5;
    size_t bucket_off[NBUCKET + 1] = {0, 0, 0, 0, 0, 0};     // ascending offsets: sp | fm | mg | channel | classifier | end
    hipEvent_t bucket_ev[NBUCKET] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

inline TLayer& train_layer(TrainState* t, int i) { return i < 9 ? t->sp[i] : i < 12 ? t->fm[i - 9] : t->mg[i - 12]; }   // as REC_LAYERS[i]
int lin_backward(ffr_handle* h, TrainState* t, const Work& w, const Lin& ln, CSlice dy, CSlice x, long long rows, Slice dx, hipStream_t st);
int get_train(ffr_handle* h, TrainState** t);      // the handle's training state on the handle's device, or why not
int dev_alloc(ffr_handle* h, std::vector<void*>& owner, size_t floats, float** out);

}  // namespace ffr_eng
