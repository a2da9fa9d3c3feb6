// RecNet training step -- the network: contexts (what a forward keeps), the backward scratch, train-mode forward, the four
// loss items, backward, and the entry points that run them.  Reference behaviour restated (paths relative to the reference):
//   RecNet.forward(input, label) models/recnet.py:398-429; AddMarginProduct (CosFace head) :238-270; the loss items models/trainer.py:154-178
#include "train_internal.h"

namespace ffr_eng {

namespace {

void free_ctx(Ctx& c) {
    if (c.mem) hipFree(c.mem);
    c = Ctx();
}

int ensure_ctx(ffr_handle* h, TrainState* t, Ctx& c, int G, int N) {
    if (c.mem && c.G == G && c.N == N) return FFR_OK;
    hipDeviceSynchronize();
    free_ctx(c);
    const size_t imgs = (size_t)G * N, rows = imgs * 49, crow = imgs * 512;
    auto carve = [&](char* base) -> size_t {
        Arena a(base);
        c.X = a.take(rows * 512 + 64 * 512);
        c.bufS = a.take(rows * 576); c.bufF = a.take(rows * 1024); c.bufM = a.take(rows * 1536);
        c.ms = a.take(rows * 64); c.featnew = a.take(rows * 512);
        auto layer = [&](const TLayer& L, TSaved& sv) { sv.y = a.take(rows * L.cout_pad); carve_bn(a, G, L.cout_pad, sv.bn); };
        for (int i = 0; i < 9; ++i) { layer(t->sp[i], c.sp[i]); c.out_sp[i] = a.take(rows * t->sp[i].cout_pad); }
        for (int i = 0; i < 3; ++i) layer(t->fm[i], c.fm[i]);
        for (int i = 0; i < 3; ++i) layer(t->mg[i], c.mg[i]);
        for (int i = 0; i < 2; ++i) { c.out_fm[i] = a.take(rows * 512); c.out_mg[i] = a.take(rows * 512); }
        c.Xt = a.take(crow * 64); c.Xht = a.take(crow * 64); c.cat = a.take(crow * 576);
        c.h1pre = a.take(crow * 64); c.h1 = a.take(crow * 64); c.t2 = a.take(crow * 512);
        c.h2pre = a.take(crow * 64); c.h2 = a.take(crow * 64); c.t5 = a.take(crow * 512);
        c.h3pre = a.take(crow * 64); c.h3 = a.take(crow * 64); c.Mc = a.take(crow * 512); c.raw = a.take(crow * 64);
        c.fnew = a.take(imgs * 512); c.fn = a.take(imgs * 512); c.fnorm = a.take(imgs + 64);
        c.cosv = a.take(imgs * CLS_PAD); c.wn = a.take((size_t)CLS_PAD * 512); c.wnorm = a.take(CLS_PAD);
        c.label = (int*)a.take(imgs + 64);
        return a.off;
    };
    const size_t need = carve(nullptr);
    if (hipMalloc(&c.mem, need) != hipSuccess) { c.mem = nullptr; return fail(h, FFR_ERR_NOMEM, "hipMalloc of %zu training-context bytes failed", need); }
    carve((char*)c.mem);
    HIPCK(h, hipMemset(c.mem, 0, need));
    c.G = G; c.N = N;
    return FFR_OK;
}

int ensure_scratch(ffr_handle* h, TrainState* t, int imgs_i) {
    if (t->scratch_mem && t->scratch_imgs >= imgs_i) return FFR_OK;
    hipDeviceSynchronize();
    if (t->scratch_mem) hipFree(t->scratch_mem);
    t->scratch_mem = nullptr;
    t->loss_grads_slot = -1;      // what lived in the old scratch is gone: the loss gradients and the folded Conv4Channel products
    t->fold_ready = false;
    const size_t imgs = imgs_i, rows = imgs * 49, crow = imgs * 512;
    // the ConvLayer buffers: the largest need of any of the 15 layers; the slice partials also serve launch_colsum (512 slices x 512 columns)
    LayerScratch cap;
    cap.part = (size_t)512 * 512;
    for (int i = 0; i < 15; ++i) { const TLayer& L = train_layer(t, i); grow_to(cap, layer_scratch(L.cin_pad, L.cout_pad, L.dgrad_width, imgs_i)); }
    auto carve = [&](char* base) -> size_t {
        Arena a(base);
        carve_scratch(a, cap, NET_SLAB_FLOATS, t->sc);
        t->dFeatNew = a.take(rows * 512); t->d512a = a.take(rows * 512); t->d512b = a.take(rows * 512);
        t->dBufM = a.take(rows * 1024); t->extM = a.take(rows * 1024); t->dF = a.take(rows * 1024);
        t->d256a = a.take(rows * 256); t->d256b = a.take(rows * 256); t->d256c = a.take(rows * 256); t->dms = a.take(rows * 64);
        t->dRawt = a.take(crow * 64); t->dMc = a.take(crow * 512); t->dt = a.take(crow * 512);
        t->d32a = a.take(crow * 64); t->d32b = a.take(crow * 64); t->rowdot = a.take(crow);
        t->dcos = a.take(imgs * CLS_PAD); t->dfn = a.take(imgs * 512); t->df = a.take(imgs * 512);
        t->dwn = a.take((size_t)CLS_PAD * 512); t->wnT = a.take((size_t)512 * CLS_PAD); t->wT = a.take((size_t)512 * 576);
        for (int q = 0; q < 2; ++q) { t->foldA[q] = a.take(64 * 32); t->foldd[q] = a.take(64); }
        t->gfoldA = a.take(64 * 32); t->gfoldd = a.take(64);
        t->lYht = a.take(crow * 64); t->lYh = a.take(imgs * 64 * 512); t->df_ext = a.take(imgs * 512); t->loss_out = a.take(64);
        t->p_sss = (double*)a.take(imgs * 2 + 64); t->p_ssc = (double*)a.take(imgs * 64 * 2 + 64);
        t->p_vec = (double*)a.take(imgs * 4 + 64); t->p_ce = (double*)a.take(imgs * 2 + 64); t->hit = (int*)a.take(imgs + 64);
        return a.off;
    };
    const size_t need = carve(nullptr);
    if (hipMalloc(&t->scratch_mem, need) != hipSuccess) { t->scratch_mem = nullptr; return fail(h, FFR_ERR_NOMEM, "hipMalloc of %zu training-scratch bytes failed", need); }
    carve((char*)t->scratch_mem);
    // zeroed once, all of it: the merged edge GEMM of layer_backward runs the column-8 problem with imgs * 9 rows, and the last imgs rows of
    // its operand Er are never written by launch_dgrad_edges (their results land in rows nobody reads; run_gemm never mixes rows) -- they
    // hold initialised, finite values from here on
    HIPCK(h, hipMemset(t->scratch_mem, 0, need));
    t->scratch_imgs = imgs_i;
    return FFR_OK;
}

// What every entry point that works on a context slot starts with: the training state, the slot, the workspace arena and the
// backward scratch for the slot's images.  args_ok: the entry point's own argument checks; imgs 0: the slot must hold a recorded
// forward, whose size it is; encoder: the arena also serves an encoder forward
struct Slot { TrainState* t; Ctx* c; Work w; hipStream_t st; };
int enter_slot(ffr_handle* h, const char* who, int slot, bool args_ok, int imgs, bool encoder, void* stream, Slot* s) {
    RC(get_train(h, &s->t));
    if (slot < 0 || slot > 1 || !args_ok) return fail(h, FFR_ERR_ARG, "%s: bad arguments", who);
    s->c = &s->t->ctx[slot];
    s->st = (hipStream_t)stream;
    if (!imgs) {
        if (!s->c->valid) return fail(h, FFR_ERR_STATE, "%s: no forward recorded in slot %d", who, slot);
        imgs = s->c->G * s->c->N;
    }
    RC(encoder ? ensure_arena_encoder(h, imgs, 112, 112, &s->w) : ensure_arena(h, imgs, 112, 112, &s->w));
    return ensure_scratch(h, s->t, imgs);
}

// ---- forward -----------------------------------------------------------------------------------------
int train_forward(ffr_handle* h, TrainState* t, Ctx& c, const Work& w, hipStream_t st) {
    const int G = c.G, N = c.N, imgs = G * N, rows = imgs * 49;
    const long long crow = (long long)imgs * 512;
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_copy_slice(c.X, c.bufS, rows, 512, 576, 0, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_copy_slice(c.X, c.bufM, rows, 512, 1536, 1024, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_selfsim_space(c.X, c.bufS, 576, nullptr, imgs, st));
    t->nbt += G;      // num_batches_tracked: every BatchNorm of the net sees G batches per call
    auto L = [&](const LayerFwd& f) { return layer_forward(h, w, t->sc, G, N, f, st); };
    const TLayer *sp = t->sp, *fm = t->fm, *mg = t->mg;
    float *const *osp = c.out_sp, *const *ofm = c.out_fm, *const *omg = c.out_mg;
    // Conv4Space (recnet.py:362-371) -> M_space (pitch-64 rows, sigmoid)
    RC(L({.L = sp[0], .sv = c.sp[0], .x = {c.bufS, 576}, .out = {osp[0], 256}}));
    RC(L({.L = sp[1], .sv = c.sp[1], .x = {osp[0], 256}, .out = {osp[1], 256}}));
    RC(L({.L = sp[2], .sv = c.sp[2], .x = {osp[1], 256}, .resid = {osp[0], 256}, .out = {osp[2], 256}}));
    RC(L({.L = sp[3], .sv = c.sp[3], .x = {osp[2], 256}, .out = {osp[3], 128}}));
    RC(L({.L = sp[4], .sv = c.sp[4], .x = {osp[3], 128}, .out = {osp[4], 128}}));
    RC(L({.L = sp[5], .sv = c.sp[5], .x = {osp[4], 128}, .resid = {osp[3], 128}, .out = {osp[5], 128}}));
    RC(L({.L = sp[6], .sv = c.sp[6], .x = {osp[5], 128}, .out = {osp[6], 64}}));
    RC(L({.L = sp[7], .sv = c.sp[7], .x = {osp[6], 64}, .out = {osp[7], 64}}));
    RC(L({.L = sp[8], .sv = c.sp[8], .x = {osp[7], 64}, .resid = {osp[6], 64}, .out = {c.ms, 64}, .flags = 1}));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_space_apply(c.X, c.ms, 64, c.bufM, 1536, 0, imgs, st));
    // Conv4Channel (recnet.py:372-386) on channelF_cat = [ss_channel | X^T] as six GEMMs
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_ch_prep(c.X, c.Xt, c.Xht, c.cat, imgs, st));
    RC(gemm_batched(h, w, c.Xht, 512 * 64, 64, c.Xht, 512 * 64, 512, c.cat, 576, (long long)512 * 576, 512, imgs, st));
    const Lin* ln = t->lin;
    RC(gemm_rows(h, w, c.cat, 576, 576, ln[0].w, ln[0].b, 64, c.h1pre, 64, crow, nullptr, 0, 0, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows(c.h1pre, c.h1, 64, 64, t->a[0], crow, st));
    c.folded = t->sc.fold;
    if (c.folded) {
        // Linear(32,512) -> Linear(512,32) pairs as their 32x32 product (exact algebra, as the inference kernel does)
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_ch_fold(ln[2].w, ln[2].b, ln[1].w, ln[1].b, t->foldA[0], t->foldd[0], st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_ch_fold(ln[4].w, ln[4].b, ln[3].w, ln[3].b, t->foldA[1], t->foldd[1], st));
        t->fold_ready = true;
        RC(gemm_rows(h, w, c.h1, 64, 32, t->foldA[0], t->foldd[0], 64, c.h2pre, 64, crow, nullptr, 0, 0, st));
    } else {
        RC(gemm_rows(h, w, c.h1, 64, 32, ln[1].w, ln[1].b, 512, c.t2, 512, crow, nullptr, 0, 0, st));
        RC(gemm_rows(h, w, c.t2, 512, 512, ln[2].w, ln[2].b, 64, c.h2pre, 64, crow, nullptr, 0, 0, st));
    }
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows(c.h2pre, c.h2, 64, 64, t->a[1], crow, st));
    if (c.folded) {
        RC(gemm_rows(h, w, c.h2, 64, 32, t->foldA[1], t->foldd[1], 64, c.h3pre, 64, crow, nullptr, 0, 0, st));
    } else {
        RC(gemm_rows(h, w, c.h2, 64, 32, ln[3].w, ln[3].b, 512, c.t5, 512, crow, nullptr, 0, 0, st));
        RC(gemm_rows(h, w, c.t5, 512, 512, ln[4].w, ln[4].b, 64, c.h3pre, 64, crow, nullptr, 0, 0, st));
    }
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows(c.h3pre, c.h3, 64, 64, t->a[2], crow, st));
    RC(gemm_rows(h, w, c.h3, 64, 32, ln[5].w, ln[5].b, 512, c.Mc, 512, crow, nullptr, 0, 1 /*sigmoid*/, st));
    // feat_channel_raw = M_channel @ X (recnet.py:410), flip + cat (:416-417)
    RC(gemm_batched(h, w, c.Mc, (long long)512 * 512, 512, c.X, 49 * 512, 64, c.raw, 64, 512 * 64, 512, imgs, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_raw_to_cat(c.raw, c.bufF, imgs, st));
    // ChannelFlipMerge -> bufM[:, 512:1024]; Conv4Merge -> feat_new
    RC(L({.L = fm[0], .sv = c.fm[0], .x = {c.bufF, 1024}, .out = {ofm[0], 512}}));
    RC(L({.L = fm[1], .sv = c.fm[1], .x = {ofm[0], 512}, .out = {ofm[1], 512}}));
    RC(L({.L = fm[2], .sv = c.fm[2], .x = {ofm[1], 512}, .resid = {ofm[0], 512}, .out = {c.bufM, 1536, 512}}));
    RC(L({.L = mg[0], .sv = c.mg[0], .x = {c.bufM, 1536}, .out = {omg[0], 512}}));
    RC(L({.L = mg[1], .sv = c.mg[1], .x = {omg[0], 512}, .out = {omg[1], 512}}));
    RC(L({.L = mg[2], .sv = c.mg[2], .x = {omg[1], 512}, .resid = {omg[0], 512}, .out = {c.featnew, 512}}));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_avgpool49(c.featnew, c.fnew, imgs, 512, st));
    // CosFace head (recnet.py:254-270)
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_row_normalize(c.fnew, 512, c.fn, c.fnorm, imgs, st));
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_row_normalize(t->clsW, 512, c.wn, c.wnorm, N_CLASSES, st));
    RC(gemm_rows(h, w, c.fn, 512, 512, c.wn, nullptr, CLS_PAD, c.cosv, CLS_PAD, imgs, nullptr, 0, 0, st));
    c.valid = true;
    return FFR_OK;
}

// ---- backward ----------------------------------------------------------------------------------------
// gradients wrt the outputs of a forward (null: none)
struct OutGrads {
    const float *f_new = nullptr, *pred_loss = nullptr, *pred_label = nullptr, *M_space = nullptr, *M_channel = nullptr,
                *feat_space = nullptr, *feat_channel = nullptr;
    bool in_scratch = false;     // instead: train_losses left them in the scratch (dcos, df_ext, extM)
};

int train_backward(ffr_handle* h, TrainState* t, Ctx& c, const Work& w, const OutGrads& og, hipStream_t st) {
    t->loss_grads_slot = -1;      // every backward spends or overwrites dcos / df_ext / extM
    const int G = c.G, N = c.N, imgs = G * N, rows = imgs * 49;
    const long long crow = (long long)imgs * 512;
    TScratch& s = t->sc;
    h->wgrad_log.clear();
    auto LB = [&](const LayerBwd& b) { return layer_backward(h, w, s, G, N, b, st); };
    const TLayer *sp = t->sp, *fm = t->fm, *mg = t->mg;
    // ---- CosFace head and f_new ----------------------------------------------------------------
    const float* df = og.in_scratch ? t->df_ext : og.f_new;
    if (og.in_scratch || og.pred_loss || og.pred_label) {
        if (!og.in_scratch) TLAUNCH(FFR_KC_TRAIN_LOSS, launch_cosface_dcos(og.pred_loss, og.pred_label, t->dcos, CLS_PAD, imgs, N_CLASSES, COSFACE_S, st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_transpose_pad(c.wn, CLS_PAD, 512, 512, t->wnT, 512, CLS_PAD, st));
        RC(gemm_rows(h, w, t->dcos, CLS_PAD, CLS_PAD, t->wnT, nullptr, 512, t->dfn, 512, imgs, nullptr, 0, 0, st));
        RC(run_wgrad(h, s, "classifier", wgrad_args(h, {t->dcos, CLS_PAD}, CLS_PAD, {c.fn, 512}, 512, imgs, 1), t->dwn, 0, 0, 2.0 * imgs * 512.0 * N_CLASSES, st));
        TLAUNCH(FFR_KC_TRAIN_LOSS, launch_normalize_bwd(t->dwn, 512, c.wn, c.wnorm, nullptr, t->gclsW, 512, 1, N_CLASSES, st));
        TLAUNCH(FFR_KC_TRAIN_LOSS, launch_normalize_bwd(t->dfn, 512, c.fn, c.fnorm, df, t->df, 512, 0, imgs, st));
        df = t->df;
    }
    HIPCK(h, hipEventRecord(t->bucket_ev[4], st));          // classifier.weight gradient is final
    if (df) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_avgpool_bwd(df, nullptr, t->dFeatNew, imgs, 512, st));
    else HIPCK(h, hipMemsetAsync(t->dFeatNew, 0, (size_t)rows * 512 * 4, st));
    if (!og.in_scratch) {
        // external gradients wrt feat_space / feat_channel (NCHW) -> extM [rows][1024]
        if (og.feat_space) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_nchw_to_nhwc(og.feat_space, t->extM, 1024, imgs, 49, 512, st));
        else TLAUNCH(FFR_KC_TRAIN_ELEM, launch_fill(t->extM, 0.f, (size_t)rows * 1024, st));
        if (og.feat_channel) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_nchw_to_nhwc(og.feat_channel, t->extM + 512, 1024, imgs, 49, 512, st));
        else if (og.feat_space) HIPCK(h, hipMemset2DAsync(t->extM + 512, 1024 * 4, 0, 512 * 4, rows, st));      // zero the second half only
    }
    // ---- Conv4Merge ------------------------------------------------------------------------------
    RC(LB({.L = mg[2], .sv = c.mg[2], .da = {t->dFeatNew, 512}, .dx = {t->d512a, 512}}));
    RC(LB({.L = mg[1], .sv = c.mg[1], .da = {t->d512a, 512}, .dx = {t->d512b, 512}, .add = {t->dFeatNew, 512}}));
    RC(LB({.L = mg[0], .sv = c.mg[0], .da = {t->d512b, 512}, .dx = {t->dBufM, 1024}, .add = {t->extM, 1024}}));
    HIPCK(h, hipEventRecord(t->bucket_ev[2], st));          // Conv4Merge gradients are final
    // ---- ChannelFlipMerge ------------------------------------------------------------------------
    RC(LB({.L = fm[2], .sv = c.fm[2], .da = {t->dBufM, 1024, 512}, .dx = {t->d512a, 512}}));
    RC(LB({.L = fm[1], .sv = c.fm[1], .da = {t->d512a, 512}, .dx = {t->d512b, 512}, .add = {t->dBufM, 1024, 512}}));
    RC(LB({.L = fm[0], .sv = c.fm[0], .da = {t->d512b, 512}, .dx = {t->dF, 1024}}));
    HIPCK(h, hipEventRecord(t->bucket_ev[1], st));          // ChannelFlipMerge
    // ---- M_channel: feat_channel_raw = M_channel @ X -------------------------------------------
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_cat_to_draw(t->dF, t->dRawt, imgs, st));
    RC(gemm_batched(h, w, t->dRawt, 512 * 64, 64, c.Xt, 512 * 64, 512, t->dMc, 512, (long long)512 * 512, 512, imgs, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_sigmoid_bwd_ext(t->dMc, og.M_channel, c.Mc, (size_t)crow * 512, st));
    // ---- Conv4Channel, last linear first -------------------------------------------------------
    const Lin* ln = t->lin;
    RC(lin_backward(h, t, w, ln[5], {t->dMc, 512}, {c.h3, 64}, crow, {t->d32a, 64}, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows_bwd(t->d32a, c.h3pre, 64, 64, t->a[2], crow, t->rowdot, t->ga[2], 1, st));
    // a folded pair: gradient of the 32x32 product, then its adjoint onto the two linears
    auto pair_backward = [&](int q, const Lin& lb, const Lin& la, const float* dy, const float* x, float* dx) -> int {
        Lin f;
        f.name = "Conv4Channel.fold" + std::to_string(q);
        f.in = 32; f.out = 32; f.in_pad = 32; f.out_pad = 64; f.w = t->foldA[q]; f.b = t->foldd[q]; f.gw = t->gfoldA; f.gb = t->gfoldd;
        HIPCK(h, hipMemsetAsync(t->gfoldA, 0, 64 * 32 * sizeof(float), st));
        HIPCK(h, hipMemsetAsync(t->gfoldd, 0, 64 * sizeof(float), st));
        RC(lin_backward(h, t, w, f, {dy, 64}, {x, 64}, crow, {dx, 64}, st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_ch_unfold(t->gfoldA, t->gfoldd, lb.w, la.w, la.b, lb.gw, lb.gb, la.gw, la.gb, st));
        return FFR_OK;
    };
    if (c.folded && !t->fold_ready) {
        // the scratch was reallocated since the folded forward (a larger forward in the other slot): the products again, from the live weights
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_ch_fold(ln[2].w, ln[2].b, ln[1].w, ln[1].b, t->foldA[0], t->foldd[0], st));
        TLAUNCH(FFR_KC_TRAIN_XFORM, launch_ch_fold(ln[4].w, ln[4].b, ln[3].w, ln[3].b, t->foldA[1], t->foldd[1], st));
        t->fold_ready = true;
    }
    if (c.folded) RC(pair_backward(1, ln[4], ln[3], t->d32a, c.h2, t->d32b));
    else {
        RC(lin_backward(h, t, w, ln[4], {t->d32a, 64}, {c.t5, 512}, crow, {t->dt, 512}, st));
        RC(lin_backward(h, t, w, ln[3], {t->dt, 512}, {c.h2, 64}, crow, {t->d32b, 64}, st));
    }
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows_bwd(t->d32b, c.h2pre, 64, 64, t->a[1], crow, t->rowdot, t->ga[1], 1, st));
    if (c.folded) RC(pair_backward(0, ln[2], ln[1], t->d32b, c.h1, t->d32a));
    else {
        RC(lin_backward(h, t, w, ln[2], {t->d32b, 64}, {c.t2, 512}, crow, {t->dt, 512}, st));
        RC(lin_backward(h, t, w, ln[1], {t->dt, 512}, {c.h1, 64}, crow, {t->d32a, 64}, st));
    }
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_prelu_rows_bwd(t->d32a, c.h1pre, 64, 64, t->a[0], crow, t->rowdot, t->ga[0], 1, st));
    RC(lin_backward(h, t, w, ln[0], {t->d32a, 64}, {c.cat, 576}, crow, {}, st));
    HIPCK(h, hipEventRecord(t->bucket_ev[3], st));          // Conv4Channel (linears, biases, PReLU slopes)
    // ---- M_space: feat_space = X_flat @ M_space ------------------------------------------------
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_space_apply_bwd(t->dBufM, 1024, 0, c.X, t->dms, imgs, st));
    if (og.M_space) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_mspace_grad_in(og.M_space, t->dms, imgs, st));
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_sigmoid_bwd(t->dms, 64, c.ms, 64, rows, 64, st));
    // ---- Conv4Space ------------------------------------------------------------------------------
    RC(LB({.L = sp[8], .sv = c.sp[8], .da = {t->dms, 64}, .dx = {t->d256a, 64}}));
    RC(LB({.L = sp[7], .sv = c.sp[7], .da = {t->d256a, 64}, .dx = {t->d256b, 64}, .add = {t->dms, 64}}));
    RC(LB({.L = sp[6], .sv = c.sp[6], .da = {t->d256b, 64}, .dx = {t->d256c, 128}}));
    RC(LB({.L = sp[5], .sv = c.sp[5], .da = {t->d256c, 128}, .dx = {t->d256a, 128}}));
    RC(LB({.L = sp[4], .sv = c.sp[4], .da = {t->d256a, 128}, .dx = {t->d256b, 128}, .add = {t->d256c, 128}}));
    RC(LB({.L = sp[3], .sv = c.sp[3], .da = {t->d256b, 128}, .dx = {t->d256c, 256}}));
    RC(LB({.L = sp[2], .sv = c.sp[2], .da = {t->d256c, 256}, .dx = {t->d256a, 256}}));
    RC(LB({.L = sp[1], .sv = c.sp[1], .da = {t->d256a, 256}, .dx = {t->d256b, 256}, .add = {t->d256c, 256}}));
    RC(LB({.L = sp[0], .sv = c.sp[0], .da = {t->d256b, 256}}));
    HIPCK(h, hipEventRecord(t->bucket_ev[0], st));          // Conv4Space: the whole flat gradient buffer is final
    return FFR_OK;
}

// ---- the four loss items (models/trainer.py:154-178) and their gradients wrt the outputs of `c` (G == 2) ----------
int train_losses(ffr_handle* h, TrainState* t, Ctx& c, const Work& w, const float* f_enc, const double lw[4], hipStream_t st) {
    t->loss_grads_slot = -1;      // overwritten from here on
    if (c.G != 2) return fail(h, FFR_ERR_ARG, "the loss items need the clean and the occluded half in one forward (G = 2)");
    const int N = c.N, imgs = 2 * N;
    LossCoef k;
    k.w_ss_space = (float)(lw[0] / (4.0 * N * 49.0 * 49.0));
    k.w_ss_channel = (float)(lw[0] / (4.0 * N * 512.0 * 512.0));
    k.w_triplet = (float)(lw[1] / N);
    k.w_identity = (float)(lw[2] / (2.0 * N * 512.0));
    k.w_ce_non = (float)(lw[3] / ((1e-8 + lw[3]) * N));
    k.w_ce_ocl = (float)(lw[3] / N);
    // ss_channel term on feat_channel (bufM[:, 512:1024]): Gram, difference to the target (ss_channel of the clean
    // feature map = the first 512 columns of channelF_cat), gradient back through the Gram and the normalisation
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_loss_ch_prep(c.bufM, 1536, 512, t->lYht, t->lYh, t->rowdot, imgs, st));
    RC(gemm_batched(h, w, t->lYht, 512 * 64, 64, t->lYht, 512 * 64, 512, t->dMc, 512, (long long)512 * 512, 512, imgs, st));
    int n_ssc = 0;
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_ssc_loss_grad(t->dMc, c.cat, imgs, N, k.w_ss_channel, t->p_ssc, &n_ssc, st));
    RC(gemm_batched(h, w, t->dMc, (long long)512 * 512, 512, t->lYh, 64 * 512, 64, t->dRawt, 64, 512 * 64, 512, imgs, st));
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_loss_ch_finish(t->dRawt, t->lYht, t->rowdot, t->extM, 1024, 512, imgs, st));
    // ss_space term on feat_space (bufM[:, 0:512])
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_ss_space_loss(c.bufM, 1536, 0, c.bufS, imgs, N, k.w_ss_space, t->p_sss, t->extM, 1024, 0, st));
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_vec_losses(c.fnew, f_enc, N, 2.0f * k.w_identity, k.w_triplet, 0.1f, t->df_ext, t->p_vec, st));
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_ce_loss(c.cosv, CLS_PAD, c.label, N, N_CLASSES, COSFACE_S, COSFACE_M, k.w_ce_non, k.w_ce_ocl, t->dcos,
                            t->p_ce, t->hit, st));
    LossParts lp{t->p_sss, t->p_ssc, t->p_vec, t->p_ce, t->hit, n_ssc};
    TLAUNCH(FFR_KC_TRAIN_LOSS, launch_loss_finish(lp, N, k, t->loss_out, st));
    t->loss_grads_slot = (int)(&c - t->ctx);
    return FFR_OK;
}

// the backward of the gradients train_losses left in the scratch; the slot's forward is spent
int backward_of_losses(ffr_handle* h, Slot& s) {
    OutGrads og; og.in_scratch = true;
    RC(train_backward(h, s.t, *s.c, s.w, og, s.st));
    s.c->valid = false;
    return FFR_OK;
}

}  // namespace

void free_graph(TrainState* t) {
    for (auto& c : t->ctx) free_ctx(c);
    if (t->scratch_mem) hipFree(t->scratch_mem);
    t->scratch_mem = nullptr;
}

}  // namespace ffr_eng

using namespace ffr_eng;

extern "C" {

int ffr_train_forward(ffr_handle* h, int slot, const float* featmap_nchw, const int32_t* label, int G, int N,
                      float* f_new, float* pred_loss, float* pred_label, float* M_space, float* M_channel,
                      float* feat_space, float* feat_channel, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const int imgs = G * N;
    Slot s;
    RC(enter_slot(h, "ffr_train_forward", slot, featmap_nchw && G > 0 && N > 0 && (label || !(pred_loss || pred_label)), imgs, false, stream, &s));
    TrainState* t = s.t; Ctx& c = *s.c; hipStream_t st = s.st;
    RC(ensure_ctx(h, t, c, G, N));
    if (t->loss_grads_slot == slot) t->loss_grads_slot = -1;      // they belonged to the forward this one replaces
    TLAUNCH(FFR_KC_TRAIN_ELEM, launch_nchw_to_nhwc(featmap_nchw, c.X, 512, imgs, 49, 512, st));
    if (label) HIPCK(h, hipMemcpyAsync(c.label, label, (size_t)imgs * 4, hipMemcpyDeviceToDevice, st));
    RC(train_forward(h, t, c, s.w, st));
    if (f_new) HIPCK(h, hipMemcpyAsync(f_new, c.fnew, (size_t)imgs * 512 * 4, hipMemcpyDeviceToDevice, st));
    if (pred_loss || pred_label)
        TLAUNCH(FFR_KC_TRAIN_LOSS, launch_cosface_out(c.cosv, CLS_PAD, c.label, pred_loss, pred_label, imgs, N_CLASSES, COSFACE_S, COSFACE_M, st));
    if (M_space) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_mspace_out(c.ms, M_space, imgs, st));
    if (M_channel) HIPCK(h, hipMemcpyAsync(M_channel, c.Mc, (size_t)imgs * 512 * 512 * 4, hipMemcpyDeviceToDevice, st));
    if (feat_space) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_nhwc_to_nchw(c.bufM, 1536, feat_space, imgs, 49, 512, st));
    if (feat_channel) TLAUNCH(FFR_KC_TRAIN_ELEM, launch_nhwc_to_nchw(c.bufM + 512, 1536, feat_channel, imgs, 49, 512, st));
    return FFR_OK;
}

int ffr_train_backward(ffr_handle* h, int slot, const float* d_f_new, const float* d_pred_loss, const float* d_pred_label,
                       const float* d_M_space, const float* d_M_channel, const float* d_feat_space,
                       const float* d_feat_channel, void* stream) {
    FFR_DEVICE_SCOPE(h);
    Slot s;
    RC(enter_slot(h, "ffr_train_backward", slot, true, 0, false, stream, &s));
    const OutGrads og{d_f_new, d_pred_loss, d_pred_label, d_M_space, d_M_channel, d_feat_space, d_feat_channel};
    RC(train_backward(h, s.t, *s.c, s.w, og, s.st));
    s.c->valid = false;
    return FFR_OK;
}

int ffr_train_losses(ffr_handle* h, int slot, const float* f_enc, const double* loss_weight, float* out5, void* stream) {
    FFR_DEVICE_SCOPE(h);
    Slot s;
    RC(enter_slot(h, "ffr_train_losses", slot, f_enc && loss_weight, 0, false, stream, &s));
    RC(train_losses(h, s.t, *s.c, s.w, f_enc, loss_weight, s.st));
    if (out5) HIPCK(h, hipMemcpyAsync(out5, s.t->loss_out, 5 * sizeof(float), hipMemcpyDeviceToDevice, s.st));
    return FFR_OK;
}

int ffr_train_backward_losses(ffr_handle* h, int slot, void* stream) {
    FFR_DEVICE_SCOPE(h);
    Slot s;
    RC(enter_slot(h, "ffr_train_backward_losses", slot, true, 0, false, stream, &s));
    if (s.t->loss_grads_slot != slot)
        return fail(h, FFR_ERR_STATE, "ffr_train_backward_losses: slot %d holds no loss gradients (ffr_train_losses on this slot must be the last call "
                                      "that used the backward scratch)", slot);
    return backward_of_losses(h, s);
}

// One iteration up to the gradients (train.py:46-54 without the optimiser step): encoder on both halves (frozen, eval),
// RecNet train-mode forward, the four loss items, zero_grad, backward.  The caller averages the flat gradient buffer
// over the ranks (if any) and calls ffr_train_adam_step.
// The images are fp32 NCHW (img_non / img_ocl) or, with u8 (img = clean, img2 = occluded), uint8 HWC RGB.
static int train_iteration(ffr_handle* h, const float* img_non, const float* img_ocl, const U8In* u8, const int32_t* label,
                           int N, const double* loss_weight, float* out5, void* stream, const char* who) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, false, N));
    const int imgs = 2 * N;
    Slot s;
    RC(enter_slot(h, who, 0, (u8 ? u8->img && u8->img2 : img_non && img_ocl) && label && loss_weight, imgs, true, stream, &s));   // the frozen encoder runs on both image sets
    TrainState* t = s.t; Ctx& c = *s.c; hipStream_t st = s.st;
    RC(ensure_ctx(h, t, c, 2, N));
    // the encoder writes the NHWC feature maps straight into the context (no NCHW round trip); f -> dfn/df scratch rows
    float* f_enc = t->d512a;    // [2N][512]; this scratch is free until the backward starts
    // both halves in one pass of 2N images: the stem reads the second half from img_ocl (u8->img2)
    RC(run_encoder(h, s.w, img_non, imgs, 112, 112, c.X, f_enc, st, u8, img_ocl, N));
    HIPCK(h, hipMemcpyAsync(c.label, label, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    HIPCK(h, hipMemcpyAsync(c.label + N, label, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    RC(train_forward(h, t, c, s.w, st));
    RC(train_losses(h, t, c, s.w, f_enc, loss_weight, st));
    if (out5) HIPCK(h, hipMemcpyAsync(out5, t->loss_out, 5 * sizeof(float), hipMemcpyDeviceToDevice, st));
    { Scope _ps(h, st, FFR_KC_TRAIN_OPTIM, 0.0, 4.0 * t->n_flat); HIPCK(h, hipMemsetAsync(t->Gr, 0, t->n_flat * 4, st)); }
    return backward_of_losses(h, s);
}

int ffr_train_iteration(ffr_handle* h, const float* img_non, const float* img_ocl, const int32_t* label, int N,
                        const double* loss_weight, float* out5, void* stream) {
    return train_iteration(h, img_non, img_ocl, nullptr, label, N, loss_weight, out5, stream, "ffr_train_iteration");
}

int ffr_train_iteration_u8(ffr_handle* h, const uint8_t* img_non, const uint8_t* img_ocl, const uint8_t* pair_flip,
                           const int32_t* label, int N, const double* loss_weight, float* out5, void* stream) {
    const U8In u8{img_non, pair_flip, img_ocl};
    return train_iteration(h, nullptr, nullptr, &u8, label, N, loss_weight, out5, stream, "ffr_train_iteration_u8");
}

// Test hook: copy a named intermediate of context `slot` (or of the backward scratch) to the host.
int ffr_train_debug_copy(ffr_handle* h, int slot, const char* name, float* host_out, size_t n) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (slot < 0 || slot > 1 || !name || !host_out) return fail(h, FFR_ERR_ARG, "ffr_train_debug_copy: bad arguments");
    Ctx& c = t->ctx[slot];
    if (!c.mem) return fail(h, FFR_ERR_STATE, "no forward in slot %d", slot);
    const std::string k = name;
    const struct { const char* name; const float* p; } named[] = {
        {"cat", c.cat}, {"h1pre", c.h1pre}, {"h1", c.h1}, {"t2", c.t2}, {"h2pre", c.h2pre}, {"h3pre", c.h3pre}, {"Mc", c.Mc},
        {"raw", c.raw}, {"X", c.X}, {"Xht", c.Xht}, {"d32a", t->d32a}, {"d32b", t->d32b}, {"dMc", t->dMc}, {"dt", t->dt},
        {"dBufM", t->dBufM}, {"dF", t->dF}, {"dms", t->dms}, {"df_ext", t->df_ext}, {"dcos", t->dcos}, {"extM", t->extM}};
    const float* src = nullptr;
    for (const auto& e : named) if (k == e.name) src = e.p;
    // "y.sp3" / "scale.fm0" / "shift.mg2": raw convolution output [rows][cout_pad] and the batch-norm scale / shift [G][cout_pad] of
    // ConvLayer i of Conv4Space (sp 0..8), ChannelFlipMerge (fm 0..2), Conv4Merge (mg 0..2): the PReLU pre-activation is
    // y * scale + shift -- the tests read its SIGN pattern (which side of the kink every element fell on)
    const size_t dot = k.find('.');
    if (dot != std::string::npos && k.size() == dot + 4) {
        const std::string what = k.substr(0, dot), set = k.substr(dot + 1, 2);
        const int i = k[dot + 3] - '0';
        const TSaved* sv = set == "sp" && i >= 0 && i < 9 ? &c.sp[i] : set == "fm" && i >= 0 && i < 3 ? &c.fm[i] :
                           set == "mg" && i >= 0 && i < 3 ? &c.mg[i] : nullptr;
        if (sv) src = what == "y" ? sv->y : what == "scale" ? sv->bn.scale : what == "shift" ? sv->bn.shift : nullptr;
    }
    if (!src) return fail(h, FFR_ERR_KEY, "no intermediate named '%s'", name);
    HIPCK(h, hipDeviceSynchronize());
    HIPCK(h, hipMemcpy(host_out, src, n * 4, hipMemcpyDeviceToHost));
    return FFR_OK;
}

int ffr_train_wgrad_plan(ffr_handle* h, ffr_wgrad_launch* out, int max, int* n) {
    if (!h || !n || max < 0 || (max > 0 && !out)) return fail(h, FFR_ERR_ARG, "ffr_train_wgrad_plan: bad arguments");
    *n = (int)h->wgrad_log.size();
    for (int i = 0; i < *n && i < max; ++i) out[i] = h->wgrad_log[i];
    return FFR_OK;
}

int ffr_train_option(ffr_handle* h, const char* name, int value) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (!name) return fail(h, FFR_ERR_ARG, "ffr_train_option: null name");
    if (std::string(name) == "winograd") { t->sc.wino = value != 0; return FFR_OK; }
    if (std::string(name) == "fused") { t->sc.fused = value < 0 ? 0 : (value > 2 ? 2 : value); return FFR_OK; }
    if (std::string(name) == "fold_channel") { t->sc.fold = value != 0; return FFR_OK; }
    if (std::string(name) == "adam_step" && value < 0) return fail(h, FFR_ERR_ARG, "ffr_train_option: adam_step must be >= 0");
    if (std::string(name) == "adam_step") { t->adam_step = value; return FFR_OK; }      // resume: Adam's bias correction continues from the saved step count
    return fail(h, FFR_ERR_KEY, "ffr_train_option: unknown option '%s'", name);
}

}  // extern "C"
