// libffrnet_hip.so: the forward pipelines -- the workspace layout, the encoder (stem, bottlenecks, head) and RecNet as
// sequences of launches on the caller's stream.  Host code only.
//
// Reference behaviour restated here (paths relative to the reference repository):
//   Backbone.forward            pretrain/model_ir_se50.py:136-141
//   bottleneck_IR_SE / SEModule pretrain/model_ir_se50.py:18-36,56-76
//   RecNet.forward (label=None) models/recnet.py:398-426
#include "engine_internal.h"

namespace ffr_eng {

// ---- workspace ---------------------------------------------------------------------------

Work layout(const Options& opt, char* base, int N, int H, int W) {
    Arena a(base);
    Work w{};
    const size_t S0 = (size_t)N * H * W * 64;
    const size_t hw16 = (size_t)(H / 16) * (W / 16);
    w.bufA = a.take(S0);
    w.bufB = a.take(S0 / 4);
    w.t1 = a.take(S0);
    w.res = a.take(S0 / 4);
    w.sc = a.take(S0 / 8);
    w.scale = a.take((size_t)N * 512);
    w.se_part = a.take((size_t)N * 32 * 512);
    w.trunk_bn = a.take((size_t)N * hw16 * 512);
    w.partial_cap = (size_t)1024 * 2 * 128 * 128 / 2 + 4096;   // 64 MiB: nblocks * 2 slabs of one tile (fp32)
    w.partial = a.take(w.partial_cap);
    // Winograd scratch: the largest V / M (36 * tiles * channels) over the layers that may use it
    {
        auto tiles = [&](int div) { return (size_t)N * ((H / div + 3) / 4) * ((W / div + 3) / 4); };
        size_t cap = 36 * tiles(2) * 128;                                   // 56x56, 64 -> 128 channels
        if (36 * tiles(1) * 64 > cap) cap = 36 * tiles(1) * 64;   // 112x112, 64 -> 64 (first bottleneck)
        if (36 * tiles(4) * 256 > cap) cap = 36 * tiles(4) * 256;           // 28x28, 128 -> 256
        if (36 * tiles(8) * 512 > cap) cap = 36 * tiles(8) * 512;           // 14x14, 256 -> 512
        if (36 * tiles(16) * 1536 > cap) cap = 36 * tiles(16) * 1536;       // 7x7, RecNet 1536 -> 512
        if (36 * (size_t)N * 9 * 1024 > cap) cap = 36 * (size_t)N * 9 * 1024;  // 9x9 data gradient of the training step, 1024 channels
        cap += (size_t)36 * 32 * 1536;                                      // k_wino_fused rounds the tile count up to 32
        w.wino_cap = cap;
        w.winoV = a.take(cap);
        w.winoM = a.take(cap);
    }
    const size_t P = (size_t)N * 49;
    w.X = a.take(P * 512);
    w.bufS = a.take(P * 576);
    w.bufF = a.take(P * 1024);
    w.bufM = a.take(P * 1536);
    w.s256a = a.take(P * 256);
    w.s256b = a.take(P * 256);
    w.s256c = a.take(P * 256);
    w.ms = a.take(P * 64);
    w.m512a = a.take(P * 512);
    w.m512b = a.take(P * 512);
    w.m512c = a.take(P * 512);
    w.dbg = a.take(P * 512);
    w.total = a.off;
    return w;
}

int grow(ffr_handle* h, DevBuf& b, size_t need_bytes, const char* what, bool zeroed) {
    if (need_bytes <= b.bytes) return FFR_OK;
    ++h->generation;          // also when the allocation below fails: the old buffer is gone by then
    if (b.p) { hipDeviceSynchronize(); hipFree(b.p); b = DevBuf(); }
    void* p = nullptr;
    if (hipMalloc(&p, need_bytes) != hipSuccess) return fail(h, FFR_ERR_NOMEM, "hipMalloc of %zu %s bytes failed", need_bytes, what);
    if (zeroed && hipMemset(p, 0, need_bytes) != hipSuccess) { hipFree(p); return fail(h, FFR_ERR_HIP, "hipMemset failed"); }
    b.p = (char*)p;
    b.bytes = need_bytes;
    return FFR_OK;
}

int ensure_arena(ffr_handle* h, int N, int H, int W, Work* w) {
    RC(grow(h, h->arena, layout(h->opt, nullptr, N, H, W).total, "workspace"));
    RC(grow(h, h->tickets, ((size_t)N * H * W / 64 + 4096) * sizeof(int), "ticket", true));
    *w = layout(h->opt, h->arena.p, N, H, W);
    w->tickets = (int*)h->tickets.p;
    w->tickets_cap = h->tickets.bytes / sizeof(int);
    return FFR_OK;
}

// ensure_arena for the calls that run the encoder on N images of H x W: also derives the exact-tiling weight sets those launches use
int ensure_arena_encoder(ffr_handle* h, int N, int H, int W, Work* w) {
    RC(ensure_arena(h, N, H, W, w));
    return prepare_mixed_weights(h, N, H, W, w->wino_cap);
}

// ---- encoder ---------------------------------------------------------------------------
// Runs stem + n_blocks bottlenecks; *out_ptr = NHWC result, *oh/*ow/*oc its geometry.

int run_trunk(ffr_handle* h, const Work& w, const float* x_nchw, int N, int H, int W, int n_blocks, hipStream_t st,
              float** out_ptr, int* oh, int* ow, int* oc, const U8In* u8, const float* x2, int n_split) {
    {
        Scope s(h, st, FFR_KC_STEM, 2.0 * N * H * W * 64 * 27, 4.0 * N * H * W * (3 + 64));
        HIPCK(h, launch_stem(x_nchw, u8 ? u8->img : nullptr, u8 ? u8->flip : nullptr, h->stem_w, h->stem_b, h->stem_s,
                             w.bufA, N, H, W, st, x2, n_split, u8 ? u8->img2 : nullptr));
    }
    float* cur = w.bufA;
    float* nxt = w.bufB;
    int ch = H, cw = W, cc = 64;
    auto conv1_call = [&](const Block& b, const float* x, int hh, int ww) {
        ConvCall c = conv_call(w);
        c.x = x; c.N = N; c.H = hh; c.W = ww; c.in_pitch = b.cin;
        c.out = w.t1; c.out_pitch = b.depth; c.cout_store = b.depth;
        return c;
    };
    // the plan record: one entry per glue launch, with the values the launch below it gets (include/ffrnet.h)
    auto note = [&](int path, int rows, int tiles, int stride = 0, bool conv_sc = false, bool scaled = false) {
        ffr_conv_launch r{};
        r.path = path; r.images = N; r.rows = rows; r.tiles = tiles;
        r.stride = stride; r.conv_shortcut = conv_sc; r.se_scale = scaled;
        h->conv_log.push_back(r);
    };
    bool v_ready = false, v_mixed = false;  // winoV holds the transform of `cur` in the order k_wino_fused (/ k_wino_fused_mixed) streams
    for (int i = 0; i < n_blocks; ++i) {
        const Block& b = h->blocks[i];
        const int ho = ch / b.stride, wo = cw / b.stride;
        ConvCall c1 = conv1_call(b, cur, ch, cw);
        // conv1 -> conv2 without the activation round trip when both run as Winograd on a map of <= 4x4 tiles
        const long long Tt = (long long)N * ((ch + 3) / 4) * ((cw + 3) / 4);
        if (!h->opt.wino_fused && b.stride == 1 && b.c1.wu && b.c2.wu && !b.c1.direct && !b.c2.direct && b.c1.cout_pad == b.c2.cin_pad &&
            b.c2.pad_mode == 0 && wino_out_in_supported(ch, cw, b.c1.cout_pad) && (size_t)36 * Tt * b.c1.cout_pad <= w.wino_cap &&
            (size_t)36 * Tt * b.c1.cin_pad <= w.wino_cap && (size_t)36 * Tt * b.c2.cout_pad <= w.wino_cap)
            c1.wino_stage = 1;
        if (v_ready) { c1.wino_stage = 2; c1.v_chunked = !v_mixed; c1.v_mixed = v_mixed; }
        const ConvPlan p1 = plan_conv(h, b.c1, c1);
        const bool chained = c1.wino_stage == 1 && p1.path == ConvPlan::Unfused;
        RC(run_conv(h, b.c1, c1, p1, st));
        if (chained) {
            Scope s(h, st, FFR_KC_WINO, 0, 4.0 * 72.0 * Tt * b.c1.cout_pad);
            if (h->conv_rec) note(FFR_CP_WINO_OUT_IN, (int)Tt, ((ch + 3) / 4) * ((cw + 3) / 4));
            HIPCK(h, launch_wino_out_in(w.winoM, b.c1.bias, b.c1.slope, w.winoV, N, ch, cw, b.c1.cout_pad, b.c1.border, st));
        }
        ConvCall c2 = conv_call(w);
        c2.x = w.t1; c2.N = N; c2.H = ch; c2.W = cw; c2.in_pitch = b.depth;
        c2.out = w.res; c2.out_pitch = b.depth; c2.cout_store = b.depth;
        if (chained) c2.wino_stage = 2;
        // SE squeeze: the Winograd output transform of conv2 leaves one partial sum per 4x4 tile in se_part
        // ([N][tiles][C], the layout k_se_fc reads); the direct path (stride 2, 64 channels) pools separately
        const int tiles = ((ho + 3) / 4) * ((wo + 3) / 4);
        if (b.fc1 && b.stride == 1 && tiles <= h->opt.se_maxtiles && (size_t)tiles * b.depth <= (size_t)32 * 512 && b.c2.cout_pad == b.depth)
            c2.tile_sums = w.se_part;
        const ConvPlan p2 = plan_conv(h, b.c2, c2);
        const bool pooled = c2.tile_sums && p2.path != ConvPlan::Direct;
        RC(run_conv(h, b.c2, c2, p2, st));
        const float* se_scale = nullptr;          // bottleneck_IR (mode 'ir'): no SEModule, the combine is res + shortcut
        if (b.fc1) {
            const double e = (double)N * ho * wo * b.depth;
            Scope s(h, st, FFR_KC_SE, e + 4.0 * N * b.depth * (b.depth / 16), 4.0 * e);
            if (pooled) {
                if (h->conv_rec) note(FFR_CP_SE_TILES, ho * wo, tiles);
                HIPCK(h, launch_se_fc(w.se_part, N, tiles, ho * wo, b.depth, b.fc1, b.fc2, w.scale, st));
            } else {
                if (h->conv_rec) note(FFR_CP_SE_POOL, ho * wo, se_slices(N, ho * wo));
                HIPCK(h, launch_se(w.res, N, ho * wo, b.depth, b.fc1, b.fc2, w.scale, w.se_part, st));
            }
            se_scale = w.scale;
        }
        const float* scp = nullptr;
        if (b.has_sc) {
            ConvCall cs = conv_call(w);
            cs.x = cur; cs.N = N; cs.H = ch; cs.W = cw; cs.in_pitch = b.cin;
            cs.out = w.sc; cs.out_pitch = b.depth; cs.cout_store = b.depth;
            RC(run_conv(h, b.sc, cs, st));
            scp = w.sc;
        }
        // the next unit's conv1 reads this unit's output through its Winograd transform: when that conv runs k_wino_fused
        // from V (cin >= 256: stage 3 and 4), the combine writes V itself and the separate transform pass is skipped
        ConvPlan next;
        if (h->opt.combine_v && i + 1 < n_blocks && (scp || b.stride == 1))
            next = plan_conv(h, h->blocks[i + 1].c1, conv1_call(h->blocks[i + 1], nxt, ho, wo));
        v_mixed = next.path == ConvPlan::Mixed && b.depth % 32 == 0;
        v_ready = v_mixed || (next.takes_v && combine_in_c_supported(ho, wo, b.depth));
        const double e = (double)N * ho * wo * b.depth;
        if (v_mixed) {
            WinoMixedGeom mg;
            wino_mixed_geom(ho, wo, &mg);
            Scope s(h, st, FFR_KC_COMBINE, 2.0 * e, 4.0 * (3.0 * e + (double)wino_mixed_v_floats(mg, N, b.depth, nullptr)));
            if (h->conv_rec) note(FFR_CP_COMBINE_IN_MIXED, ho * wo, tiles, b.stride, scp != nullptr, se_scale != nullptr);
            HIPCK(h, launch_combine_in_mixed(w.res, se_scale, scp ? scp : cur, nxt, w.winoV, N, ho, wo, b.depth, st));
        } else if (v_ready) {
            Scope s(h, st, FFR_KC_COMBINE, 2.0 * e, 4.0 * (3.0 * e + 36.0 * N * ((ho + 3) / 4) * ((wo + 3) / 4) * b.depth));
            if (h->conv_rec) note(FFR_CP_COMBINE_IN_C, ho * wo, tiles, b.stride, scp != nullptr, se_scale != nullptr);
            HIPCK(h, launch_combine_in_c(w.res, se_scale, scp ? scp : cur, nxt, w.winoV, N, ho, wo, b.depth, st));
        } else {
            Scope s(h, st, FFR_KC_COMBINE, 2.0 * e, 12.0 * e);
            if (h->conv_rec) note(FFR_CP_COMBINE, ho * wo, tiles, b.stride, scp != nullptr, se_scale != nullptr);
            HIPCK(h, launch_combine(w.res, se_scale, scp, cur, nxt, N, ho, wo, b.depth, b.stride, st));
        }
        float* t = cur; cur = nxt; nxt = t;
        ch = ho; cw = wo; cc = b.depth;
    }
    *out_ptr = cur; *oh = ch; *ow = cw; *oc = cc;
    return FFR_OK;
}

// trunk -> featmap (NHWC in w.X / w.trunk_bn) and f
int run_encoder(ffr_handle* h, const Work& w, const float* x, int N, int H, int W, float* featmap_nhwc, float* f,
                hipStream_t st, const U8In* u8, const float* x2, int n_split) {
    float* t; int oh, ow, oc;
    RC(run_trunk(h, w, x, N, H, W, (int)h->blocks.size(), st, &t, &oh, &ow, &oc, u8, x2, n_split));
    const int P = oh * ow;
    if (featmap_nhwc) {
        Scope s(h, st, FFR_KC_HEAD, 2.0 * N * P * 512, 8.0 * N * P * 512);
        HIPCK(h, launch_affine(t, h->bn_s, h->bn_t, featmap_nhwc, N * P, 512, st));
    }
    if (f) {
        if (P != 49) return fail(h, FFR_ERR_UNSUPPORTED, "output_layer needs a 7x7 trunk map (112x112 input)");
        ConvCall c = conv_call(w);
        c.x = t; c.N = N; c.H = 1; c.W = 1; c.in_pitch = 25088;
        c.out = w.scale; c.out_pitch = 512; c.cout_store = 512;     // SE scale buffer is free here
        RC(run_conv(h, h->fc, c, st));
        Scope s(h, st, FFR_KC_HEAD, 3.0 * N * 512, 8.0 * N * 512);
        HIPCK(h, launch_head_finish(w.scale, 1, N, 512, nullptr, f, st));
    }
    return FFR_OK;
}

// ---- recnet ----------------------------------------------------------------------------

int conv_rec(ffr_handle* h, const Work& w, const ConvW& L, const float* x, int in_pitch, const float* resid,
             int res_pitch, float* out, int out_pitch, int out_coff, int flags, int N, hipStream_t st) {
    ConvCall c = conv_call(w);
    c.x = x; c.N = N; c.H = 7; c.W = 7; c.in_pitch = in_pitch; c.resid = resid; c.res_pitch = res_pitch;
    c.out = out; c.out_pitch = out_pitch; c.out_coff = out_coff; c.cout_store = L.cout_pad; c.flags = flags;
    return run_conv(h, L, c, st);
}

#ifdef FFR_TRACE
// k_channel_path with per-block phase stamps (option wf_trace): the launch, a stream sync, a summary on stderr
static int trace_channel_path(ffr_handle* h, const Work& w, int N, int rb, hipStream_t st) {
    unsigned long long* dbuf = nullptr;
    HIPCK(h, hipMalloc((void**)&dbuf, (size_t)N * 4 * 8 * sizeof(unsigned long long)));
    HIPCK(h, hipMemsetAsync(dbuf, 0, (size_t)N * 4 * 8 * sizeof(unsigned long long), st));
    HIPCK(h, launch_channel_path(w.X, h->cw, w.bufF, 1024, N, st, nullptr, nullptr, 0, rb, dbuf));
    HIPCK(h, hipStreamSynchronize(st));
    std::vector<unsigned long long> tr((size_t)N * 4 * 8);
    HIPCK(h, hipMemcpy(tr.data(), dbuf, tr.size() * 8, hipMemcpyDeviceToHost));
    HIPCK(h, hipFree(dbuf));
    double ph[6] = {0, 0, 0, 0, 0, 0}; int cnt = 0;
    for (int b = 0; b < N * rb; ++b) {
        const unsigned long long* q = &tr[(size_t)b * 8];
        if (!q[6]) continue;
        for (int i = 0; i < 6; ++i) ph[i] += (double)(q[i + 1] - q[i]);
        ++cnt;
    }
    fprintf(stderr, "[wf trace] k_channel_path, %d images x %d row blocks: per block (wave 0) transpose+norms %.0f | G on MFMA %.0f | first linear %.0f | "
                    "two 32x32 affines %.0f | sigmoid(W8 h) @ X on MFMA %.0f | stores %.0f cyc\n", N, rb, ph[0] / cnt, ph[1] / cnt, ph[2] / cnt, ph[3] / cnt,
            ph[4] / cnt, ph[5] / cnt);
    return FFR_OK;
}
#endif

// X (w.X, [N,49,512]) must be filled.  Produces feat_new NHWC in w.m512c and f_new.
int run_recnet(ffr_handle* h, const Work& w, int N, float* f_new, const RecDebug* dbg, hipStream_t st) {
    const int M = N * 49;
    {
        Scope s(h, st, FFR_KC_LAYOUT, 0, 16.0 * M * 512);
        HIPCK(h, launch_copy_slice(w.X, w.bufS, M, 512, 576, 0, st));
        HIPCK(h, launch_copy_slice(w.X, w.bufM, M, 512, 1536, 1024, st));
    }
    {
        Scope s(h, st, FFR_KC_SELFSIM, 2.0 * N * 49 * 49 * 512, 4.0 * N * (49 * 512 + 49 * 49));
        HIPCK(h, launch_selfsim_space(w.X, w.bufS, 576, dbg ? dbg->ss_space : nullptr, N, st));
    }
    {
        // ss_channel Gram + Conv4Channel (6 linears) + M_channel @ X, algorithmic (unfused) count
        const double fl = 2.0 * N * (512.0 * 512 * 49 + 512.0 * (561 * 32 + 5 * 32 * 512) + 512.0 * 512 * 49);
        Scope s(h, st, FFR_KC_CHANNEL, fl, 4.0 * N * (49 * 512 * 3));
        const int rb = plan_channel_rows(N, h->num_cus, h->opt.channel_rows);
        if (!rb) return fail(h, FFR_ERR_ARG, "channel_rows is 0 (auto), 1, 2 or 4");
        if (h->conv_rec) {      // the plan record: which instantiation of k_channel_path this launch is
            ffr_conv_launch r{};
            r.path = FFR_CP_CHANNEL; r.images = N; r.rows = 512 / rb; r.nblocks = N * rb;
            h->conv_log.push_back(r);
        }
#ifdef FFR_TRACE
        if (h->opt.wf_trace) RC(trace_channel_path(h, w, N, rb, st));
        else
#endif
        HIPCK(h, launch_channel_path(w.X, h->cw, w.bufF, 1024, N, st, dbg ? dbg->ss_channel0 : nullptr, dbg ? dbg->M_channel0 : nullptr,
                                     dbg ? dbg->image : 0, rb));
    }
    // Conv4Space (recnet.py:362-371)
    RC(conv_rec(h, w, h->sp[0], w.bufS, 576, nullptr, 0, w.s256a, 256, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[1], w.s256a, 256, nullptr, 0, w.s256b, 256, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[2], w.s256b, 256, w.s256a, 256, w.s256c, 256, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[3], w.s256c, 256, nullptr, 0, w.s256a, 128, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[4], w.s256a, 128, nullptr, 0, w.s256b, 128, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[5], w.s256b, 128, w.s256a, 128, w.s256c, 128, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[6], w.s256c, 128, nullptr, 0, w.s256a, 64, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[7], w.s256a, 64, nullptr, 0, w.s256b, 64, 0, 0, N, st));
    RC(conv_rec(h, w, h->sp[8], w.s256b, 64, w.s256a, 64, w.ms, 64, 0, 1 /*sigmoid*/, N, st));
    {
        Scope s(h, st, FFR_KC_SPACE, 2.0 * N * 512 * 49 * 49, 4.0 * N * (2 * 49 * 512 + 49 * 49));
        HIPCK(h, launch_space_apply(w.X, w.ms, 64, w.bufM, 1536, 0, N, st));
    }
    // ChannelFlipMerge (recnet.py:387-390,416-418) -> bufM channels [512,1024)
    RC(conv_rec(h, w, h->fm[0], w.bufF, 1024, nullptr, 0, w.m512a, 512, 0, 0, N, st));
    RC(conv_rec(h, w, h->fm[1], w.m512a, 512, nullptr, 0, w.m512b, 512, 0, 0, N, st));
    RC(conv_rec(h, w, h->fm[2], w.m512b, 512, w.m512a, 512, w.bufM, 1536, 512, 0, N, st));
    // Conv4Merge (recnet.py:391-394,420-421)
    RC(conv_rec(h, w, h->mg[0], w.bufM, 1536, nullptr, 0, w.m512a, 512, 0, 0, N, st));
    RC(conv_rec(h, w, h->mg[1], w.m512a, 512, nullptr, 0, w.m512b, 512, 0, 0, N, st));
    RC(conv_rec(h, w, h->mg[2], w.m512b, 512, w.m512a, 512, w.m512c, 512, 0, 0, N, st));
    if (f_new) {
        Scope s(h, st, FFR_KC_HEAD, (double)N * 49 * 512, 4.0 * N * 50 * 512);
        HIPCK(h, launch_avgpool49(w.m512c, f_new, N, 512, st));
    }
    if (dbg) {
        Scope s(h, st, FFR_KC_LAYOUT, 0, 0);
        if (dbg->M_space) {   // M_space[n][i][j] = ms[n][j][i]: "NCHW" with C = 49 of a pitch-64 buffer
            // transpose kernel works on 64-channel groups: use dbg scratch [N,64,49] then compact on host side
            HIPCK(h, launch_nhwc_to_nchw(w.ms, 64, w.dbg, N, 49, 64, st));
            for (int n = 0; n < N; ++n)
                HIPCK(h, hipMemcpyAsync(dbg->M_space + (size_t)n * 2401, w.dbg + (size_t)n * 64 * 49,
                                        2401 * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        if (dbg->feat_space) HIPCK(h, launch_nhwc_to_nchw(w.bufM, 1536, dbg->feat_space, N, 49, 512, st));
        if (dbg->feat_channel_raw) HIPCK(h, launch_nhwc_to_nchw(w.bufF + 512, 1024, dbg->feat_channel_raw, N, 49, 512, st));
        if (dbg->feat_channel) HIPCK(h, launch_nhwc_to_nchw(w.bufM + 512, 1536, dbg->feat_channel, N, 49, 512, st));
    }
    return FFR_OK;
}

int check_fwd(ffr_handle* h, bool need_enc, bool need_rec, int N) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    if (N <= 0) return fail(h, FFR_ERR_ARG, "N must be positive");
    if (need_enc && !h->enc_loaded) return fail(h, FFR_ERR_STATE, "encoder weights are not loaded");
    if (need_rec && !h->rec_loaded) return fail(h, FFR_ERR_STATE, "recnet weights are not loaded");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return fail(h, FFR_ERR_HIP, "hipGetDevice failed");
    if (cur != h->device) return fail(h, FFR_ERR_HIP, "current device %d != handle device %d (entry point without FFR_DEVICE_SCOPE?)", cur, h->device);
    return FFR_OK;
}

}  // namespace ffr_eng
