// libffrnet_hip.so: the convolution launchers -- run_conv executes the entries of a plan (plan_conv, plan.cpp) and decides
// nothing itself: the direct implicit GEMM, the Winograd paths (fused, exact 14x14 tiling, transform kernels + batched GEMM)
// and the tail split; the plain GEMMs of the training step; the -DFFR_TRACE launch diagnostics.  Host code only.
#include "engine_internal.h"

namespace ffr_eng {

#ifdef FFR_TRACE
// ---- diagnostics (options igemm_trace / wf_trace): the launch with in-kernel clock stamps, a stream sync, a summary on stderr
// k_igemm: per-block clock sums
static int trace_igemm(ffr_handle* h, IgemmArgs& a, const ConvLaunch& e, hipStream_t st) {
    const int tile = e.gemm.tile, nblocks = e.gemm.nblocks;
    const long long units = e.gemm.units;
    unsigned long long* dbuf = nullptr;
    HIPCK(h, hipMalloc((void**)&dbuf, (size_t)nblocks * 8 * sizeof(unsigned long long)));
    a.trace = dbuf;
    HIPCK(h, launch_igemm(a, tile, nblocks, st));
    HIPCK(h, hipStreamSynchronize(st));
    std::vector<unsigned long long> t((size_t)nblocks * 8);
    HIPCK(h, hipMemcpy(t.data(), dbuf, t.size() * 8, hipMemcpyDeviceToHost));
    HIPCK(h, hipFree(dbuf));
    a.trace = nullptr;
    double acc[4] = {0, 0, 0, 0}, segs = 0, e1 = 0, e2 = 0, ghz = 0;
    unsigned long long r0 = ~0ull, r1 = 0, smax = 0;
    for (int b = 0; b < nblocks; ++b) {
        const unsigned long long* q = &t[(size_t)b * 8];
        for (int k = 0; k < 4; ++k) acc[k] += (double)q[k];
        segs += (double)q[4];
        ghz += (double)(q[0] + q[1] + q[2] + q[3]) / ((double)(q[6] - q[5]) * 10.0);
        e1 += (double)(q[7] >> 32); e2 += (double)(q[7] & 0xffffffffull);
        if (q[5] < r0) r0 = q[5];
        if (q[5] > smax) smax = q[5];
        if (q[6] > r1) r1 = q[6];
    }
    fprintf(stderr, "[igemm trace] tile %d blocks %d units %lld nkt %d segs/blk %.2f | per segment: setup %.0f prologue %.0f "
                    "loop %.0f (%.0f per K-tile) epilogue %.0f (first barrier at %.0f, C in LDS at %.0f) cyc | span %.1f us, starts within %.1f us, shader clock %.2f GHz\n",
            tile, nblocks, units, a.nkt, segs / nblocks, acc[0] / segs, acc[1] / segs, acc[2] / segs,
            acc[2] / ((double)units), acc[3] / segs, e1 / segs, e2 / segs, (double)(r1 - r0) / 100.0, (double)(smax - r0) / 100.0, ghz / nblocks);
    return FFR_OK;
}

// k_wino_fused_mixed: per-block phase stamps and which CU ran which tile types
static int trace_wino_mixed(ffr_handle* h, WinoMixedArgs& f, const ConvW& L, const ConvCall& c, hipStream_t st) {
    const int nbm = wino_mixed_blocks_launched(c.N, c.H, c.W, L.cout_pad);
    unsigned long long* dbuf = nullptr;
    HIPCK(h, hipMalloc((void**)&dbuf, (size_t)nbm * 12 * sizeof(unsigned long long)));
    HIPCK(h, hipMemsetAsync(dbuf, 0, (size_t)nbm * 12 * sizeof(unsigned long long), st));
    f.trace = dbuf;
    hipEvent_t e0, e1;
    HIPCK(h, hipEventCreate(&e0)); HIPCK(h, hipEventCreate(&e1));
    HIPCK(h, hipEventRecord(e0, st));
    HIPCK(h, launch_wino_fused_mixed(f, st));
    HIPCK(h, hipEventRecord(e1, st));
    HIPCK(h, hipStreamSynchronize(st));
    float ev_ms = 0.f;
    HIPCK(h, hipEventElapsedTime(&ev_ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    std::vector<unsigned long long> tr((size_t)nbm * 12);
    HIPCK(h, hipMemcpy(tr.data(), dbuf, tr.size() * 8, hipMemcpyDeviceToHost));
    HIPCK(h, hipFree(dbuf));
    double pro[4] = {0, 0, 0, 0}, loop[4] = {0, 0, 0, 0}, ep1[4] = {0, 0, 0, 0}, ep2[4] = {0, 0, 0, 0}, clk[4] = {0, 0, 0, 0};
    int cnt[4] = {0, 0, 0, 0};
    unsigned long long r_first = ~0ull, r_last = 0;
    struct Run { unsigned long long start, end; int tau; };
    std::map<unsigned long long, std::vector<Run>> per_cu;
    for (int b = 0; b < nbm; ++b) {
        const unsigned long long* q = &tr[(size_t)b * 12];
        if (!q[9]) continue;
        const int tau = (int)q[8];
        pro[tau] += (double)(q[1] - q[0]); loop[tau] += (double)(q[2] - q[1]); ep1[tau] += (double)(q[3] - q[2]); ep2[tau] += (double)(q[4] - q[3]);
        clk[tau] += (double)(q[4] - q[0]) / (double)(q[6] - q[5]) * 0.1;       // shader cycles per 10 ns tick -> GHz
        ++cnt[tau];
        if (q[5] < r_first) r_first = q[5];
        if (q[6] > r_last) r_last = q[6];
        per_cu[q[7]].push_back(Run{q[5], q[6], tau});
    }
    static const char* tname[4] = {"(4,4)", "(4,3)", "(3,4)", "(3,3)"};
    fprintf(stderr, "[wf trace] mixed %dx%d cin %d cout %d, %d images: hipEvent %.1f us, first block start to last block end %.1f us\n",
            c.H, c.W, L.cin_pad, L.cout_pad, c.N, ev_ms * 1e3, (double)(r_last - r_first) / 100.0);
    for (int tau = 0; tau < 4; ++tau) {
        if (!cnt[tau]) continue;
        const int S = wino_mixed_xp(tau) / 4;
        fprintf(stderr, "[wf trace]   type %s: %d blocks of %d slots | per block (wave 0): prologue %.0f loop %.0f (%.0f per K chunk, floor %d) "
                        "epilogue %.0f + %.0f = block %.0f cyc at %.2f GHz = %.1f us\n", tname[tau], cnt[tau], S, pro[tau] / cnt[tau], loop[tau] / cnt[tau],
                loop[tau] / cnt[tau] / f.nkc, S * 8 * 64, ep1[tau] / cnt[tau], ep2[tau] / cnt[tau],
                (pro[tau] + loop[tau] + ep1[tau] + ep2[tau]) / cnt[tau], clk[tau] / cnt[tau],
                (pro[tau] + loop[tau] + ep1[tau] + ep2[tau]) / cnt[tau] / (clk[tau] / cnt[tau]) * 1e-3);
    }
    // which block types did each CU run, in order; how long was it busy, how long idle between / after its blocks
    std::map<std::string, int> hist;
    double busy = 0, gap = 0, tail = 0, lead = 0;
    for (auto& kv : per_cu) {
        auto& v = kv.second;
        std::sort(v.begin(), v.end(), [](const Run& x, const Run& y) { return x.start < y.start; });
        std::string key;
        for (size_t i = 0; i < v.size(); ++i) {
            key += tname[v[i].tau];
            busy += (double)(v[i].end - v[i].start);
            if (i) gap += (double)(v[i].start - v[i - 1].end);
        }
        lead += (double)(v.front().start - r_first);
        tail += (double)(r_last - v.back().end);
        ++hist[key];
    }
    const double ncu = (double)per_cu.size();
    fprintf(stderr, "[wf trace]   %d CUs ran blocks; per CU: busy %.1f us, idle before its first block %.1f, between blocks %.1f, after its last block %.1f us | sequences:",
            (int)per_cu.size(), busy / ncu / 100.0, lead / ncu / 100.0, gap / ncu / 100.0, tail / ncu / 100.0);
    for (auto& kv : hist) fprintf(stderr, "  %s x %d", kv.first.c_str(), kv.second);
    fprintf(stderr, "\n");
    return FFR_OK;
}

// k_wino_fused: per-block phase stamps
static int trace_wino_fused(ffr_handle* h, WinoFusedArgs& f, const ConvW& L, const ConvCall& c, const ConvLaunch& e, hipStream_t st) {
    const ffr_conv_launch& p = e.rec;
    const int nb = wino_fused_blocks(f);
    unsigned long long* dbuf = nullptr;
    HIPCK(h, hipMalloc((void**)&dbuf, (size_t)nb * 40 * sizeof(unsigned long long)));
    HIPCK(h, hipMemsetAsync(dbuf, 0, (size_t)nb * 40 * sizeof(unsigned long long), st));
    f.trace = dbuf;
    HIPCK(h, launch_wino_fused(f, st));
    HIPCK(h, hipStreamSynchronize(st));
    std::vector<unsigned long long> tr((size_t)nb * 40);
    HIPCK(h, hipMemcpy(tr.data(), dbuf, tr.size() * 8, hipMemcpyDeviceToHost));
    HIPCK(h, hipFree(dbuf));
    double pro = 0, loop = 0, epi = 0, ep[5] = {0, 0, 0, 0, 0}; int cnt = 0;
    unsigned long long r0 = ~0ull, r1 = 0;
    for (int b = 0; b < nb; ++b) {
        const unsigned long long* q = &tr[(size_t)b * 40];
        if (!q[3]) continue;
        ep[0] += (double)(q[6] - q[2]); ep[1] += (double)(q[7] - q[6]); ep[2] += (double)(q[8] - q[7]);
        ep[3] += (double)(q[9] - q[8]); ep[4] += (double)(q[3] - q[9]);
        pro += (double)(q[1] - q[0]); loop += (double)(q[2] - q[1]); epi += (double)(q[3] - q[2]); ++cnt;
        if (q[4] > r1) r1 = q[4];
        if (q[4] < r0) r0 = q[4];
    }
    if (p.phased) {    // the kernel reports per phase: input transform, wait at the barrier behind it
        const int cpp = 4, nph = f.nkc / cpp;                      // K chunks per phase, phases
        fprintf(stderr, "[wf trace] %dx%d cin %d cout %d (input transform in the kernel, %d-channel blocks%s): %d live blocks of %d | per block (wave 0): "
                        "prologue %.0f loop %.0f = %d phases x (transform %.0f + barrier %.0f + %d K chunks of %.0f) epilogue %.0f cyc | "
                        "block ends spread over %.1f us\n", c.H, c.W, L.cin_pad, L.cout_pad, p.half_n ? 32 : 64, p.split ? ", split-operand K loop" : "", cnt, nb,
                pro / cnt, loop / cnt, nph, ep[0] / cnt, ep[1] / cnt, cpp, (loop / cnt / nph - ep[0] / cnt - ep[1] / cnt) / cpp, epi / cnt,
                (double)(r1 - r0) / 100.0);
    }
    else
        fprintf(stderr, "[wf trace] %dx%d cin %d cout %d: %d live blocks of %d | per block (wave 0): prologue %.0f loop %.0f (%.0f per K chunk) "
                        "epilogue %.0f cyc (to LDS %.0f, transform+store %.0f, barrier+to LDS %.0f, transform+store %.0f, end %.0f) | block ends spread over %.1f us\n",
                c.H, c.W, L.cin_pad, L.cout_pad, cnt, nb, pro / cnt, loop / cnt, loop / cnt / f.nkc, epi / cnt, ep[0] / cnt, ep[1] / cnt,
                ep[2] / cnt, ep[3] / cnt, ep[4] / cnt, (double)(r1 - r0) / 100.0);
    return FFR_OK;
}
#endif

// what the convolution L stores for call c: the epilogue of whichever kernel it ends in
static ConvTail conv_tail(const ConvW& L, const ConvCall& c) {
    return ConvTail{L.bias, L.slope, c.resid, c.out, c.tile_sums, L.cout_pad, c.cout_store, c.out_pitch, c.out_coff, c.res_pitch, L.border, c.flags};
}

// the plan record: the entry a launcher is about to execute
static void record(ffr_handle* h, const ConvLaunch& e) {
    if (h->conv_rec) h->conv_log.push_back(e.rec);
}

// launches the planned k_igemm entry e: the (possibly batched) implicit GEMM described by `a` (M, nkt, tail.cout_pad, nbatch set)
static int run_gemm(ffr_handle* h, IgemmArgs& a, const ConvCall& c, const ConvLaunch& e, double flops, double bytes, hipStream_t st,
                    double fuse = -1.0) {
    const GemmPlan& g = e.gemm;
    const int cout_pad = a.tail.cout_pad;
    if (c.tile) {     // a forced tile whose width does not divide cout_pad would launch zero column tiles and leave `out` unwritten
        int fbm, fbn;
        igemm_tile_shape(c.tile, &fbm, &fbn);
        if (cout_pad % fbn) return fail(h, FFR_ERR_ARG, "conv: forced tile %d (%d x %d) does not divide cout_pad %d", c.tile, fbm, fbn, cout_pad);
    }
    if (g.nomem) return fail(h, FFR_ERR_NOMEM, "%s", g.nomem);
    int bm, bn;
    igemm_tile_shape(g.tile, &bm, &bn);
    a.granule = g.granule; a.mtiles = g.mtiles; a.ntiles = g.ntiles;
    a.partial = c.partial;
    a.tickets = c.tickets;
    record(h, e);
#ifdef FFR_TRACE
    if (h->opt.igemm_trace) return trace_igemm(h, a, e, st);
#endif
    const double fexec = 2.0 * a.nbatch * (double)a.mtiles * bm * (double)cout_pad * a.KK;
    Scope s(h, st, FFR_KC_CONV_IGEMM, flops, bytes, fexec, fuse);
    HIPCK(h, launch_igemm(a, g.tile, g.nblocks, st));
    return FFR_OK;
}

// exact tiling 4+4+3+3 of a 14x14 map (wino_mixed.hip): one transform launch and one fused launch for all four tile types
static int conv_mixed(ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvLaunch& e, double flops, double bytes, hipStream_t st) {
    WinoMixedGeom g;
    wino_mixed_geom(c.H, c.W, &g);
    if (c.wino_stage == 0) {
        Scope s(h, st, FFR_KC_WINO, 0, 4.0 * ((double)c.N * c.H * c.W * L.cin + (double)wino_mixed_v_floats(g, c.N, L.cin_pad, nullptr)));
        HIPCK(h, launch_wino_in_mixed(c.x, c.winoV, c.N, c.H, c.W, c.in_pitch, L.cin_pad, st));
    }
    WinoMixedArgs f{};
    f.V[0] = c.winoV;
    for (int tau = 0; tau < 4; ++tau) f.U[tau] = L.wum[tau];
    f.tail = conv_tail(L, c);
    f.N = c.N; f.H = c.H; f.W = c.W; f.nkc = L.cin_pad / 8;
    double fexec = 0.0, fuse = 0.0;
    for (int tau = 0; tau < 4; ++tau) {
        const int nr = tau >= 2 ? g.n3 : g.n4, nc = (tau & 1) ? g.n3 : g.n4;
        const double Tt = (double)c.N * nr * nc;
        fexec += 2.0 * wino_mixed_xp(tau) * std::ceil(Tt / 32.0) * 32.0 * L.cout_pad * L.cin_pad;
        fuse += 2.0 * wino_mixed_x(tau) * Tt * L.cout * L.cin;
    }
    record(h, e);
#ifdef FFR_TRACE
    if (h->opt.wf_trace) return trace_wino_mixed(h, f, L, c, st);
#endif
    Scope s(h, st, FFR_KC_WINO_FUSED, flops, bytes, fexec, fuse);
    HIPCK(h, launch_wino_fused_mixed(f, st));
    return FFR_OK;
}

// Winograd F(4x4,3x3), GEMM + output transform in one kernel (wino_fused.hip): M never exists in memory
static int conv_fused(ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvLaunch& e, double flops, double bytes, hipStream_t st) {
    const ffr_conv_launch& p = e.rec;
    const long long T = (long long)c.N * ((c.H + 3) / 4) * ((c.W + 3) / 4);
    if (!p.phased && c.wino_stage == 0) {
        Scope s(h, st, FFR_KC_WINO, 0, 4.0 * ((double)c.N * c.H * c.W * L.cin + 36.0 * T * L.cin_pad));
        HIPCK(h, launch_wino_in_chunked(c.x, c.winoV, c.N, c.H, c.W, c.in_pitch, L.cin_pad, L.pad_mode, st));
    }
    WinoFusedArgs f{};
    f.Vc = p.phased ? nullptr : c.winoV; f.x = c.x; f.in_pitch = c.in_pitch; f.pad_mode = L.pad_mode;
    f.x_bytes = p.phased ? (unsigned)(4.0 * c.N * c.H * c.W * c.in_pitch) : 0u;
    f.half_n = p.half_n;
    f.U3 = p.split ? L.wu3 : nullptr;
    f.Uc = L.wuc; f.tail = conv_tail(L, c);
    f.N = c.N; f.H = c.H; f.W = c.W; f.nkc = L.cin_pad / 8;
    const double fexec = 2.0 * 36.0 * (double)((T + 31) / 32 * 32) * (double)L.cout_pad * L.cin_pad;
    record(h, e);
#ifdef FFR_TRACE
    if (h->opt.wf_trace) return trace_wino_fused(h, f, L, c, e, st);
#endif
    Scope s(h, st, FFR_KC_WINO_FUSED, flops, bytes, fexec, flops / 4.0);      // flops_executed stays the fp32-equivalent count in the split form
    HIPCK(h, launch_wino_fused(f, st));
    if (p.split) ++h->wf_split_launches;
    return FFR_OK;
}

// nbatch independent GEMMs out[b][M][out_pitch] = A[b][M][K_pad] * W[b][N_pad][K_pad]^T through k_igemm, with the stream-K
// scratch of c; flops, bytes and fuse are the caller's figures for the profiling scope (run_gemm).  planned: the entry of a
// convolution's plan this launch executes, or null: a GEMM of its own, planned here
static int igemm_batched(ffr_handle* h, const ConvCall& c, const ConvLaunch* planned, const float* A, long long a_bstride, int K_pad,
                         const float* W, long long w_bstride, int N_pad, float* out, int out_pitch, long long out_bstride, int M, int nbatch,
                         double flops, double bytes, double fuse, hipStream_t st) {
    IgemmArgs g{};
    g.x = A; g.w = W; g.zero = h->zero;
    g.tail = ConvTail{h->zero, nullptr, nullptr, out, nullptr, N_pad, N_pad, out_pitch, 0, 0, 0, 0};      // the neutral tail: + 0, all N_pad columns
    g.N = 1; g.H = 1; g.W = M; g.Ho = 1; g.Wo = M;
    g.in_pitch = K_pad; g.cin_pad = K_pad; g.R = 1; g.S = 1; g.stride = 1; g.pad = 0; g.pad_mode = 0;
    g.M = M; g.KK = K_pad; g.nkt = K_pad / 32;
    g.nbatch = nbatch; g.x_bstride = a_bstride; g.w_bstride = w_bstride; g.out_bstride = out_bstride;
    return run_gemm(h, g, c, planned ? *planned : plan_gemm_launch(h, c, FFR_CP_DIRECT, 1, M, N_pad, g.nkt, nbatch, false), flops, bytes, st, fuse);
}

// Winograd F(4x4,3x3): input transform -> 36 batched GEMMs [T x cin] * [cin x cout] -> output transform
static int conv_unfused(ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvLaunch& e, long long M, double flops, double bytes,
                        hipStream_t st) {
    const long long T = (long long)c.N * ((c.H + 3) / 4) * ((c.W + 3) / 4);
    if (c.wino_stage != 2) {
        Scope s(h, st, FFR_KC_WINO, 0, 4.0 * ((double)c.N * c.H * c.W * L.cin + 36.0 * T * L.cin_pad));
        HIPCK(h, launch_wino_in(c.x, c.winoV, c.N, c.H, c.W, c.in_pitch, L.cin_pad, L.pad_mode, st));
    }
    // the roofline numerator of the GEMM stays the DIRECT convolution's algorithmic FLOPs
    if (e.rec.path == FFR_CP_UNFUSED_STREAM) {
        // 36 GEMMs in one persistent launch with a continuous K-tile stream
        GemmStreamArgs g{};
        g.A = c.winoV; g.W = L.wu; g.C = c.winoM; g.M = (int)T; g.K = L.cin_pad; g.Npad = L.cout_pad; g.nbatch = 36;
        int bm, bn;
        igemm_tile_shape(e.rec.tile, &bm, &bn);
        const double fexec = 2.0 * 36.0 * (double)((T + bm - 1) / bm) * bm * (double)L.cout_pad * L.cin_pad;
        record(h, e);
        Scope s(h, st, FFR_KC_CONV_IGEMM, flops, bytes, fexec, flops / 4.0);
        HIPCK(h, launch_gemm_stream(g, e.rec.tile, e.rec.nblocks, st));
    } else {
        RC(igemm_batched(h, c, &e, c.winoV, T * L.cin_pad, L.cin_pad, L.wu, (long long)L.cout_pad * L.cin_pad, L.cout_pad, c.winoM, L.cout_pad,
                         T * L.cout_pad, (int)T, 36, flops, bytes, flops / 4.0, st));
    }
    if (c.wino_stage == 1) return FFR_OK;        // the caller transforms M itself (k_wino_out_in)
    Scope s(h, st, FFR_KC_WINO, 0, 4.0 * (36.0 * T * L.cout_pad + (double)M * L.cout));
    HIPCK(h, launch_wino_out(c.winoM, conv_tail(L, c), c.N, c.H, c.W, st));
    return FFR_OK;
}

// Executes one launching entry e of a plan on the images of call c that it covers, on stream st
static int run_launch(ffr_handle* h, const ConvW& L, const ConvCall& whole, const ConvLaunch& e, hipStream_t st) {
    const ConvCall c = conv_part(L, whole, e.n0, e.rec.images);
    const int Ho = (c.H + 2 * L.pad - L.R) / L.stride + 1, Wo = (c.W + 2 * L.pad - L.S) / L.stride + 1;
    const long long M = (long long)c.N * Ho * Wo;
    const double flops = 2.0 * M * L.cout * (double)L.R * L.S * L.cin;
    const double bytes = 4.0 * ((double)c.N * c.H * c.W * L.cin + (double)M * L.cout + (double)L.cout * L.R * L.S * L.cin);
    if (e.rec.path == FFR_CP_MIXED) return conv_mixed(h, L, c, e, flops, bytes, st);
    if (e.rec.path == FFR_CP_FUSED) return conv_fused(h, L, c, e, flops, bytes, st);
    if (e.rec.path != FFR_CP_DIRECT) return conv_unfused(h, L, c, e, M, flops, bytes, st);
    IgemmArgs a{};
    a.x = c.x; a.w = L.w; a.tail = conv_tail(L, c); a.zero = h->zero;
    a.N = c.N; a.H = c.H; a.W = c.W; a.Ho = Ho; a.Wo = Wo;
    a.in_pitch = c.in_pitch; a.cin_pad = L.cin_pad; a.R = L.R; a.S = L.S; a.stride = L.stride; a.pad = L.pad; a.pad_mode = L.pad_mode;
    a.M = (int)M; a.KK = L.R * L.S * L.cin_pad; a.nkt = a.KK / 32; a.nbatch = 1;
    // split-operand form (plan.cpp, conv_launch).  flops_executed of the launch stays the fp32-equivalent count (run_gemm)
    if (e.rec.split) { a.w3 = L.w3; a.w3_pstride = (long long)L.cout_pad * a.KK; }
    return run_gemm(h, a, c, e, flops, bytes, st);
}

// Runs the convolution L on call c as its plan p = plan_conv(h, L, c) says: every entry of p, in order
int run_conv(ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvPlan& p, hipStream_t st) {
    const long long M = (long long)c.N * ((c.H + 2 * L.pad - L.R) / L.stride + 1) * ((c.W + 2 * L.pad - L.S) / L.stride + 1);
    if (M <= 0 || M > 0x7fffffffLL) return fail(h, FFR_ERR_ARG, "conv: bad M");
    if (L.pad_mode == 1 && (c.H < 2 || c.W < 2)) return fail(h, FFR_ERR_UNSUPPORTED, "reflect pad needs H,W >= 2");
    if (L.border && (c.H < 2 || c.W < 2)) return fail(h, FFR_ERR_UNSUPPORTED, "border-class bias needs H,W >= 2");
    if (h->conv_rec) {      // a replayed capture would launch without recording
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCK(h, hipStreamIsCapturing(st, &cs));
        if (cs != hipStreamCaptureStatusNone) return fail(h, FFR_ERR_STATE, "conv: the plan record is on and the stream is capturing");
    }
    if (p.refused) return fail(h, FFR_ERR_STATE, "%s", p.refused);
    if (p.n_launch == 1) return run_launch(h, L, c, p.launch[0], st);
    // tail split: the header, then its two parts; with p.side the first of them (the few images behind n_main) runs on that
    // stream beside the second
    record(h, p.launch[0]);
    if (p.side) {
        HIPCK(h, hipEventRecord(h->ev_fork, st));
        HIPCK(h, hipStreamWaitEvent(p.side, h->ev_fork, 0));
    }
    RC(run_launch(h, L, c, p.launch[1], p.side ? p.side : st));
    if (p.side) HIPCK(h, hipEventRecord(h->ev_join, p.side));
    RC(run_launch(h, L, c, p.launch[2], st));
    if (p.side) HIPCK(h, hipStreamWaitEvent(st, h->ev_join, 0));
    return FFR_OK;
}

int run_conv(ffr_handle* h, const ConvW& L, const ConvCall& c, hipStream_t st) {
    return run_conv(h, L, c, plan_conv(h, L, c), st);
}

// ---- plain GEMMs through the implicit-GEMM kernel (the training step) -------------------------------------
// out[rows][N_pad] = A[rows][K_pad] * W[N_pad][K_pad]^T + bias (+ resid) (sigmoid when flags & 1)
int gemm_rows(ffr_handle* h, const Work& w, const float* A, int a_pitch, int K_pad, const float* W, const float* bias,
              int N_pad, float* out, int out_pitch, long long rows, const float* resid, int res_pitch, int flags,
              hipStream_t st) {
    ConvW cw;
    cw.cin = K_pad; cw.cin_pad = K_pad; cw.cout = N_pad; cw.cout_pad = N_pad; cw.R = 1; cw.S = 1; cw.stride = 1; cw.pad = 0;
    cw.pad_mode = 0; cw.border = 0; cw.w = const_cast<float*>(W); cw.bias = bias ? const_cast<float*>(bias) : h->zero;
    cw.slope = nullptr; cw.wu = nullptr;
    ConvCall c = conv_call(w, ConvForce::Direct);
    c.x = A; c.N = 1; c.H = 1; c.W = (int)rows; c.in_pitch = a_pitch; c.resid = resid; c.res_pitch = res_pitch;
    c.out = out; c.out_pitch = out_pitch; c.out_coff = 0; c.cout_store = N_pad; c.flags = flags;
    return run_conv(h, cw, c, st);
}

// nbatch independent GEMMs out[b][M][out_pitch] = A[b][M][K_pad] * W[b][N_pad][K_pad]^T
int gemm_batched(ffr_handle* h, const Work& w, const float* A, long long a_bstride, int K_pad, const float* W,
                 long long w_bstride, int N_pad, float* out, int out_pitch, long long out_bstride, int M, int nbatch,
                 hipStream_t st) {
    const double fl = 2.0 * nbatch * (double)M * N_pad * K_pad;
    return igemm_batched(h, conv_call(w, ConvForce::Direct), nullptr, A, a_bstride, K_pad, W, w_bstride, N_pad, out, out_pitch, out_bstride, M,
                         nbatch, fl, 4.0 * nbatch * ((double)M * K_pad + (double)N_pad * K_pad + (double)M * N_pad), fl, st);
}

}  // namespace ffr_eng
