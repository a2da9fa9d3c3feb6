// RecNet training step -- the ConvLayer and Linear operators, forward and backward, the weight-gradient plan record and the
// rule that sizes a ConvLayer backward's scratch.  Reference behaviour restated (paths relative to the reference repository):
//   ConvLayer / ResidualBlock in train() mode   models/recnet.py:52-85,202-218 (BatchNorm2d batch statistics)
#include "train_internal.h"

namespace ffr_eng {

namespace {

const float BN_MOMENTUM = 0.1f, BN_EPS_F = 1e-5f;

const struct { const char* name; size_t LayerScratch::*n; } SCRATCH_BUFS[] = {
    {"part", &LayerScratch::part}, {"wd", &LayerScratch::wd}, {"dxp", &LayerScratch::dxp}, {"dy", &LayerScratch::dy},
    {"U", &LayerScratch::U}, {"canvas", &LayerScratch::canvas}, {"edgeA", &LayerScratch::edgeA}, {"edgeW", &LayerScratch::edgeW},
    {"edgeO", &LayerScratch::edgeO}};

// a shortfall is an error naming the buffer, never another path
int check_scratch(ffr_handle* h, const TScratch& s, const TLayer& L, int imgs) {
    const LayerScratch need = layer_scratch(L.cin_pad, L.cout_pad, L.dgrad_width, imgs);
    for (const auto& b : SCRATCH_BUFS)
        if (need.*b.n > s.cap.*b.n) return fail(h, FFR_ERR_NOMEM, "training scratch (%s) too small: %zu < %zu", b.name, s.cap.*b.n, need.*b.n);
    return FFR_OK;
}

// Winograd F(4x4,3x3) as the inference path: U = G g G^T from the live weights cw.w into the U scratch, emitted in
// the order k_wino_fused streams when the launch of T tiles can run fused (the kernel of the inference path: GEMMs + output
// transform in one launch).  The planner's form of the fused kernel (option "fused" 1; 2: always fused, 0: never), never
// Auto: the training step splits off no tail.
int wino_prepare(ffr_handle* h, TScratch& s, ConvW& cw, ConvCall& c, long long T, double x_bytes, hipStream_t st) {
    c.force = s.fused ? wino_fused_form(h, cw.cin_pad, cw.cout_pad, T, x_bytes, s.fused == 2 ? ConvForce::Fused : ConvForce::Auto)
                      : ConvForce::Unfused;
    const bool fused = c.force != ConvForce::Unfused;
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_wino_weights(cw.w, s.U, cw.cout_pad, cw.cin_pad, st, fused ? 1 : 0));
    cw.wu = s.U;
    if (fused) cw.wuc = s.U;
    return FFR_OK;
}

}  // namespace

// The single definition of what the backward of a ConvLayer (cin_pad -> cout_pad, data gradient of the first dgrad_width
// input channels) takes on `imgs` 7x7 maps.  ffr_op_convlayer_train allocates it, ensure_scratch its maximum over the network's
// layers, layer_forward / layer_backward check their scratch against it.
LayerScratch layer_scratch(int cin_pad, int cout_pad, int dgrad_width, int imgs_i) {
    const size_t imgs = imgs_i, need_pad = round_up(dgrad_width, 64);
    LayerScratch n;
    // bn_part_doubles(G, N * 49, cout_pad) for every G * N = imgs: a group of N images is cut into at most (N + 1) / 2 <= N slices
    n.part = imgs * 3 * cout_pad;
    n.dy = imgs * 49 * cout_pad;
    // forward and weight gradient [36][cout_pad][cin_pad], data gradient [36][need_pad][cout_pad]
    n.U = (size_t)36 * cout_pad * std::max((size_t)cin_pad, need_pad);
    if (!dgrad_width) return n;
    n.wd = need_pad * 9 * cout_pad; n.dxp = imgs * 81 * need_pad; n.canvas = imgs * 64 * cout_pad;
    n.edgeA = imgs * 18 * 3 * cout_pad; n.edgeW = 2 * need_pad * 3 * cout_pad; n.edgeO = imgs * 18 * need_pad;
    return n;
}

void grow_to(LayerScratch& a, const LayerScratch& b) {
    for (const auto& f : SCRATCH_BUFS) a.*f.n = std::max(a.*f.n, b.*f.n);
}

void carve_scratch(Arena& a, const LayerScratch& cap, size_t slab_floats, TScratch& s) {
    s.cap = cap; s.slab_floats = slab_floats;
    s.part = (double*)a.take(cap.part * 2);
    s.wd = a.take(cap.wd); s.dxp = a.take(cap.dxp); s.dy = a.take(cap.dy); s.slabs = a.take(slab_floats); s.U = a.take(cap.U);
    s.canvas = a.take(cap.canvas); s.edgeA = a.take(cap.edgeA); s.edgeW = a.take(cap.edgeW); s.edgeO = a.take(cap.edgeO);
}

void carve_bn(Arena& a, int G, int Cp, BnBuffers& b) {
    const size_t gc = (size_t)G * Cp;
    float* p = a.take(6 * gc);
    float** f[6] = {&b.mean, &b.invstd, &b.scale, &b.shift, &b.c1, &b.c2};
    for (int i = 0; i < 6; ++i) *f[i] = p ? p + i * gc : nullptr;
}

WgradArgs wgrad_args(ffr_handle* h, CSlice dy, int cout_pad, CSlice x, int cin_pad, long long rows, int taps) {
    WgradArgs a{};
    a.dy = dy.p; a.x = x.p; a.zero = h->zero; a.rows = (int)rows; a.x_pitch = x.pitch; a.dy_pitch = dy.pitch;
    a.cin_pad = cin_pad; a.cout_pad = cout_pad; a.taps = taps;
    a.H = a.W = taps == 9 ? 7 : 1; a.pad_mode = taps == 9 ? 1 : 0;
    return a;
}

// One weight-gradient GEMM: profiling scope, launch (nbatch 0: launch_wgrad into grad; else launch_wgrad_batched of nbatch
// consecutive problems of a.rows rows, which never accumulates) and its entry in the plan record (ffr_train_wgrad_plan: the
// launcher's arguments as it ran them).  useful_flops: those of the layer's gradient without any padding.
int run_wgrad(ffr_handle* h, TScratch& s, const std::string& name, const WgradArgs& a, float* grad, int accumulate, int nbatch,
              double useful_flops, hipStream_t st) {
    const double nb = nbatch ? nbatch : 1;
    Scope sc(h, st, FFR_KC_WGRAD, useful_flops, 4.0 * nb * a.rows * (a.cout_pad + a.cin_pad),
             2.0 * nb * a.rows * a.taps * a.cout_pad * a.cin_pad, nbatch ? useful_flops / 4.0 : -1.0);
    WgradArgs pl{};
    if (nbatch) HIPCK(h, launch_wgrad_batched(a, grad, nbatch, (long long)a.rows * a.dy_pitch, (long long)a.rows * a.x_pitch, s.slabs, s.slab_floats, st, &pl));
    else HIPCK(h, launch_wgrad(a, grad, accumulate, s.slabs, s.slab_floats, st, &pl));
    ffr_wgrad_launch r{};
    snprintf(r.name, sizeof r.name, "%s", name.c_str());
    r.path = nbatch ? 2 : a.taps == 9 ? 0 : 1;
    r.rows = pl.rows; r.cout_pad = pl.cout_pad; r.Ng = pl.Ng; r.nbatch = pl.nbatch; r.nkt = pl.nkt; r.splits = pl.splits; r.kt_per_split = pl.kt_per_split;
    r.full_tiles = pl.full_tiles; r.tail_splits = pl.tail_splits; r.tail_kt = pl.tail_kt; r.accumulate = nbatch ? 0 : accumulate;
    h->wgrad_log.push_back(r);
    return FFR_OK;
}

int layer_forward(ffr_handle* h, const Work& w, TScratch& s, int G, int N, const LayerFwd& f, hipStream_t st) {
    const TLayer& L = f.L; TSaved& sv = f.sv;
    RC(check_scratch(h, s, L, G * N));
    sv.x = f.x.p; sv.x_pitch = f.x.pitch;
    ConvW cw;
    cw.cin = L.cin; cw.cin_pad = L.cin_pad; cw.cout = L.cout; cw.cout_pad = L.cout_pad; cw.R = 3; cw.S = 3; cw.stride = 1;
    cw.pad = 1; cw.pad_mode = 1; cw.border = 0; cw.w = L.w; cw.bias = h->zero; cw.slope = nullptr; cw.wu = nullptr;
    ConvCall c = conv_call(w, ConvForce::Direct);
    if (s.wino && L.cin_pad >= 128) RC(wino_prepare(h, s, cw, c, (long long)G * N * 4, 4.0 * G * N * 49 * sv.x_pitch, st));
    c.x = sv.x; c.N = G * N; c.H = 7; c.W = 7; c.in_pitch = sv.x_pitch;
    c.out = sv.y; c.out_pitch = L.cout_pad; c.out_coff = 0; c.cout_store = L.cout_pad;
    RC(run_conv(h, cw, c, st));     // the raw convolution output, for the batch statistics
    TLAUNCH(FFR_KC_TRAIN_BN, launch_bn_stats(sv.y, L.cout_pad, G, N * 49, L.gamma, L.beta, L.rmean, L.rvar, BN_MOMENTUM, BN_EPS_F, sv.bn, s.part, st));
    TLAUNCH(FFR_KC_TRAIN_BN, launch_bn_apply(sv.y, L.cout_pad, G, N * 49, sv.bn, L.slope, f.resid.p, f.resid.pitch, f.out.p, f.out.pitch,
                                             f.out.coff, f.flags, st));
    return FFR_OK;
}

int layer_backward(ffr_handle* h, const Work& w, TScratch& s, int G, int N, const LayerBwd& b, hipStream_t st) {
    const TLayer& L = b.L; const TSaved& sv = b.sv;
    const int imgs = G * N, rows = imgs * 49;
    RC(check_scratch(h, s, L, imgs));
    TLAUNCH(FFR_KC_TRAIN_BN, launch_bn_bwd(b.da.p, b.da.pitch, b.da.coff, sv.y, L.cout_pad, G, N * 49, sv.bn, L.slope, L.ggamma, L.gbeta,
                                           L.gslope, b.accumulate, s.dy, s.part, st));
    const long long T = (long long)imgs * 4;          // 2x2 tiles of 4x4 outputs per 7x7 map
    const double useful = 2.0 * rows * 9.0 * L.cout * L.cin;
    // the arena is sized by the forward pipelines, not here: its capacity stays a condition of the path
    if (s.wino && L.cin_pad >= 128 && w.winoV && (size_t)36 * T * L.cin_pad <= w.wino_cap && (size_t)36 * T * L.cout_pad <= w.wino_cap) {
        // weight gradient in the Winograd domain: dU[xi] = dM[xi]^T V[xi] (36 TN GEMMs over the tiles), dW += G^T dU G
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_wino_in(sv.x, w.winoV, imgs, 7, 7, sv.x_pitch, L.cin_pad, 1, st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_wino_dout(s.dy, w.winoM, imgs, 7, 7, L.cout_pad, st));
        // dU in the U scratch (free until the data gradient re-derives its weights), split-K slabs in s.slabs
        RC(run_wgrad(h, s, L.name, wgrad_args(h, {w.winoM, L.cout_pad}, L.cout_pad, {w.winoV, L.cin_pad}, L.cin_pad, T, 1), s.U, 0, 36, useful, st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_wino_dweights(s.U, L.gw, L.cout_pad, L.cin_pad, b.accumulate, st));
    } else {
        RC(run_wgrad(h, s, L.name, wgrad_args(h, {s.dy, L.cout_pad}, L.cout_pad, {sv.x, sv.x_pitch}, L.cin_pad, rows, 9), L.gw, b.accumulate, 0, useful, st));
    }
    if (!b.dx.p) return FFR_OK;
    const int need_pad = round_up(L.dgrad_width, 64), cfold = round_up(L.dgrad_width, 4);
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_pack_dgrad(L.w, L.cout_pad, L.cin_pad, s.wd, need_pad, st));
    ConvW cw;
    cw.cin = L.cout_pad; cw.cin_pad = L.cout_pad; cw.cout = need_pad; cw.cout_pad = need_pad; cw.R = 3; cw.S = 3;
    cw.stride = 1; cw.pad = 2; cw.pad_mode = 0; cw.border = 0; cw.w = s.wd; cw.bias = h->zero; cw.slope = nullptr; cw.wu = nullptr;
    ConvCall c = conv_call(w, ConvForce::Direct);
    c.x = s.dy; c.N = imgs; c.H = 7; c.W = 7; c.in_pitch = L.cout_pad;
    c.out = s.dxp; c.out_pitch = need_pad; c.out_coff = 0; c.cout_store = need_pad;
    if (!(s.wino && L.cout_pad >= 128)) {
        RC(run_conv(h, cw, c, st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_fold_reflect(s.dxp, need_pad, imgs, cfold, b.add.p, b.add.pitch, b.add.coff, b.dx.p, b.dx.pitch, b.dx.coff, st));
        return FFR_OK;
    }
    // The 9x9 padded gradient in three pieces: rows/columns 0..7 as the 'same' F(4x4,3x3) convolution of dy embedded at
    // (1,1) of an 8x8 map (2x2 tiles instead of the 3x3 a 9x9 output would need), row 8 and column 8 (only the last
    // weight row / column reaches them) as two GEMMs with K = 3*cout.
    RC(wino_prepare(h, s, cw, c, T, 4.0 * imgs * 64 * L.cout_pad, st));
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_embed_8x8(s.dy, s.canvas, imgs, L.cout_pad, st));
    cw.pad = 1;
    c.x = s.canvas; c.H = 8; c.W = 8;
    RC(run_conv(h, cw, c, st));
    const long long e_stride = (long long)imgs * 9 * 3 * L.cout_pad, w_stride = (long long)need_pad * 3 * L.cout_pad, o_stride = (long long)imgs * 9 * need_pad;
    float *Eb = s.edgeA, *Er = s.edgeA + e_stride, *Wb = s.edgeW, *Wr = s.edgeW + w_stride, *Ob = s.edgeO, *Or = s.edgeO + o_stride;
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_dgrad_edges(s.dy, Eb, Er, imgs, L.cout_pad, st));
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_pack_dgrad_edges(L.w, L.cout_pad, L.cin_pad, Wb, Wr, need_pad, st));
    // row 8 and column 8 as ONE batched launch of two GEMMs (each fills 144 .. 288 of the chip's 768 tile slots by itself; the
    // column GEMM runs with imgs * 9 rows like the row GEMM -- its last imgs rows read scratch and land in rows nobody reads)
    RC(gemm_batched(h, w, Eb, e_stride, 3 * L.cout_pad, Wb, w_stride, need_pad, Ob, need_pad, o_stride, imgs * 9, 2, st));
    TLAUNCH(FFR_KC_TRAIN_XFORM, launch_fold_reflect3(s.dxp, Ob, Or, need_pad, imgs, cfold, b.add.p, b.add.pitch, b.add.coff, b.dx.p, b.dx.pitch,
                                                  b.dx.coff, st));
    return FFR_OK;
}

int lin_backward(ffr_handle* h, TrainState* t, const Work& w, const Lin& ln, CSlice dy, CSlice x, long long rows, Slice dx, hipStream_t st) {
    RC(run_wgrad(h, t->sc, ln.name, wgrad_args(h, dy, ln.out_pad, x, ln.in_pad, rows, 1), ln.gw, 1, 0, 2.0 * rows * ln.out * ln.in, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_colsum(dy.p, dy.pitch, (int)rows, ln.out_pad, ln.gb, 1, t->sc.part, st));
    if (dx.p) {
        // dx[rows][in] = dy[rows][out] * W  -> the kernel wants W^T as [in rounded to 64][K], K = out (32 or 512)
        const int n_pad = round_up(ln.in_pad, 64);
        const int kb = ln.out <= 32 ? 32 : ln.out_pad;
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_transpose_pad(ln.w, kb, ln.in_pad, ln.in_pad, t->wT, n_pad, kb, st));
        RC(gemm_rows(h, w, dy.p, dy.pitch, kb, t->wT, nullptr, n_pad, dx.p, dx.pitch, rows, nullptr, 0, 0, st));
    }
    return FFR_OK;
}

}  // namespace ffr_eng

using namespace ffr_eng;

// raw [cout][cin][3][3] -> kernel layout [cout_pad][9][cin_pad]
static std::vector<float> pack3x3(const float* W, int cout, int cin, int cout_pad, int cin_pad) {
    std::vector<float> p((size_t)cout_pad * 9 * cin_pad, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) p[((size_t)co * 9 + t) * cin_pad + ci] = W[((size_t)co * cin + ci) * 9 + t];
    return p;
}

// Test hook: one ConvLayer in train() mode, forward and backward, on caller-provided NHWC buffers.
extern "C" int ffr_op_convlayer_train(ffr_handle* h, const float* x_nhwc, int G, int N, int cin, int cout, const float* w_host,
                                      const float* gamma_host, const float* beta_host, const float* slope_host,
                                      const float* da_nhwc, float* out_nhwc, float* dx_nhwc, float* dw_packed, float* dvec,
                                      float* stats, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    if (!x_nhwc || !w_host || !gamma_host || !beta_host || !slope_host || !da_nhwc || !out_nhwc || G <= 0 || N <= 0)
        return fail(h, FFR_ERR_ARG, "ffr_op_convlayer_train: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, G * N, 112, 112, &w));
    std::vector<void*> own;
    struct Guard { std::vector<void*>& v; ~Guard() { hipDeviceSynchronize(); free_list(v); } } guard{own};
    TLayer L;
    L.cin = cin; L.cout = cout; L.cin_pad = round_up(cin, 32); L.cout_pad = round_up(cout, 64); L.dgrad_width = cin;
    const int rows = G * N * 49;
    std::vector<float> wp = pack3x3(w_host, cout, cin, L.cout_pad, L.cin_pad);
    std::vector<float> vec((size_t)3 * L.cout_pad, 0.f);
    for (int c = 0; c < cout; ++c) { vec[c] = gamma_host[c]; vec[L.cout_pad + c] = beta_host[c]; vec[2 * L.cout_pad + c] = slope_host[c]; }
    float* pv;
    RC(upload(h, own, wp, &L.w));
    RC(upload(h, own, vec, &pv));
    L.gamma = pv; L.beta = pv + L.cout_pad; L.slope = pv + 2 * L.cout_pad;
    // the gradients, the raw convolution output, the BatchNorm buffers and the backward scratch in one allocation
    float* gv;
    TSaved sv;
    TScratch s;
    if (h->train) { s.wino = h->train->sc.wino; s.fused = h->train->sc.fused; }     // ffr_train_option, when a training state exists
    const LayerScratch cap = layer_scratch(L.cin_pad, L.cout_pad, L.dgrad_width, G * N);
    auto carve = [&](char* base) -> size_t {
        Arena a(base);
        L.gw = a.take(wp.size()); gv = a.take((size_t)5 * L.cout_pad); sv.y = a.take((size_t)rows * L.cout_pad);
        carve_bn(a, G, L.cout_pad, sv.bn);
        carve_scratch(a, cap, op_slab_floats(L), s);
        return a.off;
    };
    float* mem;
    RC(dev_alloc(h, own, carve(nullptr) / 4, &mem));
    carve((char*)mem);
    L.ggamma = gv; L.gbeta = gv + L.cout_pad; L.gslope = gv + 2 * L.cout_pad; L.rmean = gv + 3 * L.cout_pad; L.rvar = gv + 4 * L.cout_pad;
    HIPCK(h, hipMemsetAsync(gv, 0, (size_t)5 * L.cout_pad * 4, st));
    HIPCK(h, hipMemsetAsync(s.edgeA, 0, cap.edgeA * sizeof(float), st));      // the unwritten tail rows of Er: see ensure_scratch
    h->wgrad_log.clear();
    RC(layer_forward(h, w, s, G, N, {L, sv, {x_nhwc, L.cin_pad}, {}, {out_nhwc, L.cout_pad}}, st));
    RC(layer_backward(h, w, s, G, N, {L, sv, {da_nhwc, L.cout_pad}, {dx_nhwc, L.cin_pad}, {}, 0}, st));
    if (dw_packed) HIPCK(h, hipMemcpyAsync(dw_packed, L.gw, wp.size() * 4, hipMemcpyDeviceToDevice, st));
    if (dvec) HIPCK(h, hipMemcpyAsync(dvec, gv, (size_t)5 * L.cout_pad * 4, hipMemcpyDeviceToDevice, st));
    if (stats) HIPCK(h, hipMemcpyAsync(stats, sv.bn.mean, (size_t)2 * G * L.cout_pad * 4, hipMemcpyDeviceToDevice, st));
    HIPCK(h, hipStreamSynchronize(st));
    return FFR_OK;
}
