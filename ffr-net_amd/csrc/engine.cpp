// libffrnet_hip.so: C ABI (include/ffrnet.h) of the MI355X-native FFR-Net embedding path -- handles, forwards, scoring,
// the per-layer arithmetic plan and its calibration, options, probe, profiling, operator test hooks.  The planner is in
// plan.cpp, the launchers in conv.cpp, the weight packer in pack.cpp, the pipelines in forward.cpp, the kernels in *.hip.
//
// Reference behaviour restated here (paths relative to the reference repository):
//   calculate_distance cosine   lfw/lfw_eval.py:246,248
#include "engine_internal.h"

using namespace ffr;
using namespace ffr_eng;

namespace ffr_eng {

std::string g_err = "";

int fail(ffr_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_err = buf;
    return code;
}

struct PlanLayer { ConvW* L; std::string name; int net; };

// The Winograd-eligible convolutions of the loaded nets (those the handle packed wu for), in ffr_layer_get order.
std::vector<PlanLayer> plan_layers(const ffr_handle* hc) {
    ffr_handle* h = const_cast<ffr_handle*>(hc);
    std::vector<PlanLayer> v;
    if (h->enc_loaded)
        for (size_t i = 0; i < h->blocks.size(); ++i) {
            Block& b = h->blocks[i];
            const std::string p = "body." + std::to_string(i) + ".res_layer.";
            if (b.c1.wu) v.push_back({&b.c1, p + "1", 0});
            if (b.c2.wu) v.push_back({&b.c2, p + "3", 0});
        }
    if (h->rec_loaded)
        for (int i = 0; i < 15; ++i)
            if (rec_conv(h, i).wu) v.push_back({&rec_conv(h, i), std::string(REC_LAYERS[i].prefix) + ".conv2d", 1});
    return v;
}

// A plan change invalidates captured graphs, and the exact-tiling weight sets of a layer that returns to Winograd may not
// exist yet: the next encoder call walks the layers again (prepare_mixed_weights).
void plan_changed(ffr_handle* h) { ++h->generation; h->mixed_ready_n = 0; }
}  // namespace ffr_eng

// ---- pieces the entry points share --------------------------------------------------------------------------------------
static int check_hw(ffr_handle* h, int H, int W) {
    if (H < 32 || W < 32 || (H & 15) || (W & 15)) return fail(h, FFR_ERR_ARG, "H and W must be multiples of 16, >= 32");
    return FFR_OK;
}

static int check_dim(ffr_handle* h, const char* who, int dim) {
    if (dim != 512) return fail(h, FFR_ERR_UNSUPPORTED, "%s: dim must be 512, got %d", who, dim);
    return FFR_OK;
}

static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// A scratch laid out the way layout() lays out the workspace: `lay` takes its pieces from a measuring Arena, the buffer grows
// to that size, and `lay` runs again on the buffer
template <class F> static int carve(ffr_handle* h, DevBuf& b, const char* what, F lay) {
    Arena measure(nullptr);
    lay(measure);
    RC(grow(h, b, measure.off, what));
    Arena a(b.p);
    lay(a);
    return FFR_OK;
}

// featmap [N,512,7,7] -> w.X, where run_recnet reads it
static int featmap_to_x(ffr_handle* h, const Work& w, const float* featmap_nchw, int N, hipStream_t st) {
    HIPCK(h, launch_nchw_to_nhwc(featmap_nchw, w.X, 512, N, 49, 512, st));
    return FFR_OK;
}

// The tail of ffr_embed, ffr_embed_u8 and ffr_embed_aligned: workspace, encoder into w.X, RecNet
static int embed_tail(ffr_handle* h, const float* x, const U8In* u8, int N, float* f_new, float* f, hipStream_t st) {
    Work w;
    RC(ensure_arena_encoder(h, N, 112, 112, &w));
    RC(run_encoder(h, w, x, N, 112, 112, w.X, f, st, u8));
    return run_recnet(h, w, N, f_new, nullptr, st);
}

// =========================================================================================
extern "C" {

const char* ffr_version(void) { return "ffrnet-hip 0.1 (gfx950)"; }

const char* ffr_last_error(const ffr_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int ffr_create(ffr_handle** out, int device) {
    if (!out) return fail(nullptr, FFR_ERR_ARG, "ffr_create: out is null");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, FFR_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= count) return fail(nullptr, FFR_ERR_ARG, "device %d out of range (%d devices)", device, count);
    DeviceScope scope(device);
    if (!scope.ok) return fail(nullptr, FFR_ERR_HIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, FFR_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, FFR_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    ffr_handle* h = new ffr_handle();
    h->device = device;
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    void* z = nullptr;
    if (hipMalloc(&z, 131072) != hipSuccess) { delete h; return fail(nullptr, FFR_ERR_NOMEM, "hipMalloc failed"); }
    hipMemset(z, 0, 131072);
    h->zero = (float*)z;
    hipError_t e = igemm_init();
    if (e == hipSuccess) e = gemm_stream_init();
    if (e == hipSuccess) e = wino_fused_init();
    if (e == hipSuccess) e = wino_mixed_init();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (h->ev_fork) hipEventDestroy(h->ev_fork);
        if (h->ev_join) hipEventDestroy(h->ev_join);
        if (h->side) hipStreamDestroy(h->side);
        hipFree(z); delete h;
        return fail(nullptr, FFR_ERR_HIP, "ffr_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return FFR_OK;
}

void ffr_destroy(ffr_handle* h) {
    if (!h) return;
    FFR_DEVICE_SCOPE(h);
    hipDeviceSynchronize();
    train_free(h);
    free_list(h->enc_allocs);
    free_list(h->rec_allocs);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->side) hipStreamDestroy(h->side);
    for (DevBuf* b : {&h->arena, &h->tickets, &h->search, &h->cluster, &h->align}) if (b->p) hipFree(b->p);
    if (h->zero) hipFree(h->zero);
    for (auto& r : h->prof_log) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (auto e : h->ev_pool) hipEventDestroy(e);
    delete h;
}

int ffr_memory_stats(const ffr_handle* h, ffr_mem_stats* out) {
    if (!h || !out) return fail(nullptr, FFR_ERR_ARG, "ffr_memory_stats: null argument");
    out->encoder_weight_bytes = h->enc_weight_bytes;
    out->recnet_weight_bytes = h->rec_weight_bytes;
    out->mixed_tile_weight_bytes = h->mixed_weight_bytes;
    out->workspace_bytes = h->arena.bytes;
    out->encoder_load_seconds = h->enc_load_s;
    out->recnet_load_seconds = h->rec_load_s;
    out->mixed_tile_pack_seconds = h->mixed_pack_s;
    out->split_weight_bytes = h->split_weight_bytes;
    out->wf_split_weight_bytes = h->wf_split_weight_bytes;
    out->wf_split_launches = h->wf_split_launches;
    return FFR_OK;
}

int ffr_split_planes_host(const double* w, long long n, unsigned short* planes) {
    if (!w || !planes || n < 0) return FFR_ERR_ARG;
    for (long long i = 0; i < n; ++i) {
        unsigned short q[3];
        split_bf16x3(w[i], q);
        for (int p = 0; p < 3; ++p) planes[(size_t)p * n + i] = q[p];
    }
    return FFR_OK;
}

size_t ffr_workspace_bytes(const ffr_handle* h, int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return layout(h ? h->opt : Options(), nullptr, N, H, W).total;
}

int ffr_reserve(ffr_handle* h, int N, int H, int W) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, N));
    Work w;
    return ensure_arena_encoder(h, N, H, W, &w);
}

// ffr_encoder_forward and its uint8 twin: the input is x (fp32 NCHW) or u8 (uint8 HWC RGB)
static int encoder_forward(ffr_handle* h, const float* x, const U8In* u8, int N, int H, int W, float* featmap_nchw, float* f,
                           void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, false, N));
    if (u8 ? !u8->img : !x) return fail(h, FFR_ERR_ARG, u8 ? "img is null" : "x is null");
    RC(check_hw(h, H, W));
    if (f && (H != 112 || W != 112)) return fail(h, FFR_ERR_UNSUPPORTED, "f needs a 112x112 input (Linear(512*7*7,512))");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena_encoder(h, N, H, W, &w));
    RC(run_encoder(h, w, x, N, H, W, featmap_nchw ? w.trunk_bn : nullptr, f, st, u8));
    if (featmap_nchw) {
        Scope s(h, st, FFR_KC_LAYOUT, 0, 8.0 * N * (H / 16) * (W / 16) * 512);
        HIPCK(h, launch_nhwc_to_nchw(w.trunk_bn, 512, featmap_nchw, N, (H / 16) * (W / 16), 512, st));
    }
    return FFR_OK;
}

int ffr_encoder_forward(ffr_handle* h, const float* x, int N, int H, int W, float* featmap_nchw, float* f, void* stream) {
    return encoder_forward(h, x, nullptr, N, H, W, featmap_nchw, f, stream);
}

int ffr_encoder_forward_u8(ffr_handle* h, const uint8_t* img_hwc_rgb, const uint8_t* flip, int N, int H, int W,
                           float* featmap_nchw, float* f, void* stream) {
    const U8In u8{img_hwc_rgb, flip};
    return encoder_forward(h, nullptr, &u8, N, H, W, featmap_nchw, f, stream);
}

int ffr_recnet_forward(ffr_handle* h, const float* featmap_nchw, int N, float* f_new, float* feat_new_nchw, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, true, N));
    if (!featmap_nchw) return fail(h, FFR_ERR_ARG, "featmap is null");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, N, 112, 112, &w));
    {
        Scope s(h, st, FFR_KC_LAYOUT, 0, 8.0 * N * 49 * 512);
        RC(featmap_to_x(h, w, featmap_nchw, N, st));
    }
    RC(run_recnet(h, w, N, f_new, nullptr, st));
    if (feat_new_nchw) {
        Scope s(h, st, FFR_KC_LAYOUT, 0, 8.0 * N * 49 * 512);
        HIPCK(h, launch_nhwc_to_nchw(w.m512c, 512, feat_new_nchw, N, 49, 512, st));
    }
    return FFR_OK;
}

int ffr_embed(ffr_handle* h, const float* x, int N, float* f_new, float* f, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, true, N));
    if (!x || !f_new) return fail(h, FFR_ERR_ARG, "x / f_new is null");
    return embed_tail(h, x, nullptr, N, f_new, f, (hipStream_t)stream);
}

int ffr_embed_u8(ffr_handle* h, const uint8_t* img_hwc_rgb, const uint8_t* flip, int N, float* f_new, float* f,
                 void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, true, N));
    if (!img_hwc_rgb || !f_new) return fail(h, FFR_ERR_ARG, "img / f_new is null");
    const U8In u8{img_hwc_rgb, flip};
    return embed_tail(h, nullptr, &u8, N, f_new, f, (hipStream_t)stream);
}

int ffr_cosine_scores(ffr_handle* h, const float* a, const float* b, int n, int dim, float* score, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, n));
    if (!a || !b || !score || dim <= 0) return fail(h, FFR_ERR_ARG, "ffr_cosine_scores: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Scope s(h, st, FFR_KC_SCORE, 6.0 * n * dim, 8.0 * n * dim);
    HIPCK(h, launch_cosine(a, b, n, dim, score, st));
    return FFR_OK;
}

int ffr_lfw_fold_accuracy(ffr_handle* h, const float* score, const int32_t* label, int n, int n_folds, double* best_thr,
                          double* test_acc, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, n));
    if (!score || !label || !best_thr || !test_acc || n_folds < 1 || n_folds > 32 || n < n_folds)
        return fail(h, FFR_ERR_ARG, "ffr_lfw_fold_accuracy: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, 8, 112, 112, &w));
    Scope s(h, st, FFR_KC_SCORE, 400.0 * n, 8.0 * 400 * n);
    HIPCK(h, launch_fold_protocol(score, (const int*)label, n, n_folds, (int*)w.partial, best_thr, test_acc, st));
    return FFR_OK;
}

unsigned long long ffr_generation(const ffr_handle* h) { return h ? h->generation : 0; }

// ---- 1:N identification (search.hip) ---------------------------------------------------------------------------------
int ffr_row_norms(ffr_handle* h, const float* x, long long n, int dim, float* norms, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    RC(check_dim(h, "ffr_row_norms", dim));
    if (!x || !norms || n < 1) return fail(h, FFR_ERR_ARG, "ffr_row_norms: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Scope s(h, st, FFR_KC_SCORE, 2.0 * n * dim, 4.0 * n * (dim + 1));
    HIPCK(h, launch_row_norms(x, n, norms, st));
    return FFR_OK;
}

// What the search and merge entries share.  Lists [..][Q][k] of scores and indices; u: their subject plane, null in an entry
// without subjects -- what tells the two kinds of entry apart from here on (12 or 16 bytes per slot)
struct TopLists { float* s = nullptr; int64_t* i = nullptr; int32_t* u = nullptr; };
// The per-probe filter of ffr_search_topk_filtered and ffr_search_topk_coarse_filtered: tag[G] and qmask[Q]; both null in every
// other entry -- what tells the filtered searches apart from here on (qmask is never null in them, tag only at G = 0)
struct SearchFilter { const uint32_t* tag = nullptr; const uint32_t* qmask = nullptr; };

static bool misaligned4(const void* p) { return ((uintptr_t)p & 3) != 0; }

static int check_distinct(ffr_handle* h, const char* who, int distinct, int k) {
    if (distinct != 0 && distinct != 1) return fail(h, FFR_ERR_ARG, "%s: distinct must be 0 or 1, got %d", who, distinct);
    if (distinct && k > search_max_k_distinct())
        return fail(h, FFR_ERR_ARG, "%s: identity mode serves k <= %d, got %d", who, search_max_k_distinct(), k);
    return FFR_OK;
}

// The checks of the six search entries, in the order every entry makes them: handle, dim, null pointers and ranges (at
// G = 0 the gallery side may be null), distinct and the k of identity mode, 16-byte rows, 4-byte subjects, 4-byte tags and
// masks.  coarse: the entry takes plane and plane_flag; subj: it takes subject and top.u (an entry without passes distinct = 0,
// or is refused); flt (or null): it takes tag and qmask.  `who` names it in messages.
static int search_pre(ffr_handle* h, const char* who, bool coarse, const float* query, int Q, const float* gallery,
                      const float* gallery_norms, const uint16_t* plane, const int* plane_flag, const int32_t* subject, long long G,
                      int dim, int k, int distinct, const TopLists& top, bool subj, const SearchFilter* flt = nullptr) {
    RC(check_fwd(h, false, false, 1));
    RC(check_dim(h, who, dim));
    const bool gallery_side = gallery && gallery_norms && (!coarse || (plane && plane_flag)) && (!subj || subject) && (!flt || flt->tag);
    if (!query || !top.s || !top.i || (subj && !top.u) || (flt && !flt->qmask) || Q < 1 || k < 1 || k > 128 || G < 0 ||
        (G > 0 && !gallery_side))
        return fail(h, FFR_ERR_ARG, "%s: bad arguments (Q >= 1, 1 <= k <= 128, G >= 0, non-null pointers)", who);
    RC(check_distinct(h, who, distinct, k));
    if (distinct && !subj) return fail(h, FFR_ERR_ARG, "%s: distinct = 1 needs gallery_subject and top_subject", who);
    if (misaligned16(query) || (G > 0 && (misaligned16(gallery) || misaligned16(plane))))
        return fail(h, FFR_ERR_ARG, "%s: %s rows must be 16-byte aligned", who, coarse ? "query, gallery and plane" : "query and gallery");
    if (G > 0 && misaligned4(subject)) return fail(h, FFR_ERR_ARG, "%s: gallery_subject must be 4-byte aligned", who);
    if (flt && (misaligned4(flt->qmask) || (G > 0 && misaligned4(flt->tag))))
        return fail(h, FFR_ERR_ARG, "%s: gallery_tag and query_mask must be 4-byte aligned", who);
    return FFR_OK;
}

// An exact pass into given lists: the search of the plan (T, S, chunk_rows) and, when S > 1, the merge of its chunk lists
// part[S][Q][k].  subject (or null) and distinct: the policy.  live (device, or null): only the probes [0, *live) are searched.
// flt: the per-probe filter, with which the same policy runs in its filtered kernel; the merge is the same, the lists hold
// admissible rows only
static int exact_pass(ffr_handle* h, const float* query, const float* qnorm, int Q, const float* gallery, const float* gallery_norms,
                      const int32_t* subject, long long G, int k, long long index_base, int distinct, int T, int S,
                      long long chunk_rows, const TopLists& dst, const TopLists& part, const int* live, hipStream_t st,
                      const SearchFilter& flt = {}) {
    const TopLists& out = S > 1 ? part : dst;
    const SearchArgs a{query, qnorm, gallery, nullptr, gallery_norms, G, chunk_rows, index_base, out.s, out.i, live, Q, k, S, T,
                       subject, out.u, flt.tag, flt.qmask};
    const SearchKernel policy = !subject ? SEARCH_ROWS : distinct ? SEARCH_DISTINCT : SEARCH_LIVE;
    static_assert(SEARCH_FILTERED_LIVE - SEARCH_FILTERED_ROWS == SEARCH_LIVE - SEARCH_ROWS &&
                  SEARCH_FILTERED_DISTINCT - SEARCH_FILTERED_ROWS == SEARCH_DISTINCT - SEARCH_ROWS,
                  "the filtered kernels come in the order of the policies");
    HIPCK(h, launch_search(a, flt.qmask ? (SearchKernel)(SEARCH_FILTERED_ROWS + policy) : policy, st));
    if (S > 1) HIPCK(h, launch_topk_merge(part.s, part.i, part.u, S, Q, k, distinct, dst.s, dst.i, dst.u, st, live));
    return FFR_OK;
}

// The exact search of checked arguments: ffr_search_topk, ffr_search_topk_subjects (top.u), ffr_search_topk_filtered (flt), and
// the coarse entries where their pass does not serve
static int exact_search(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                        const int32_t* subject, long long G, int dim, int k, long long index_base, int distinct, const TopLists& top,
                        hipStream_t st, const SearchFilter& flt = {}) {
    const double slot = top.u ? 16.0 : 12.0;
    if (G == 0) {                 // k slots of padding per probe: the merge of no list
        Scope s(h, st, FFR_KC_SCORE, 0.0, slot * Q * k);
        HIPCK(h, launch_topk_merge(nullptr, nullptr, nullptr, 0, Q, k, distinct, top.s, top.i, top.u, st));
        return FFR_OK;
    }
    int T = 0, S = 0;
    long long chunk_rows = 0;
    search_plan(Q, G, h->num_cus, &T, &S, &chunk_rows);
    // scratch: probe norms [Q], then the chunk lists [S][Q][k] (scores, indices, with subjects a third plane) when there is
    // more than one chunk
    float* qnorm = nullptr;
    TopLists part;
    RC(carve(h, h->search, "search", [&](Arena& a) {
        qnorm = a.take(Q);
        if (S > 1) {
            part.s = a.take((size_t)S * Q * k); part.i = a.take<int64_t>((size_t)S * Q * k);
            if (top.u) part.u = a.take<int32_t>((size_t)S * Q * k);
        }
    }));
    Scope s(h, st, FFR_KC_SCORE, 2.0 * Q * (double)G * dim,
            4.0 * (double)G * (dim + (top.u ? 2 : 1)) + 4.0 * Q * dim + slot * Q * k + (flt.qmask ? 4.0 * (double)G + 4.0 * Q : 0.0));
    HIPCK(h, launch_row_norms(query, Q, qnorm, st));
    return exact_pass(h, query, qnorm, Q, gallery, gallery_norms, subject, G, k, index_base, distinct, T, S, chunk_rows, top, part,
                      nullptr, st, flt);
}

int ffr_search_topk(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms, long long G,
                    int dim, int k, long long index_base, float* top_score, int64_t* top_index, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, nullptr};
    RC(search_pre(h, "ffr_search_topk", false, query, Q, gallery, gallery_norms, nullptr, nullptr, nullptr, G, dim, k, 0, top, false));
    return exact_search(h, query, Q, gallery, gallery_norms, nullptr, G, dim, k, index_base, 0, top, (hipStream_t)stream);
}

int ffr_search_topk_subjects(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                             const int32_t* gallery_subject, long long G, int dim, int k, long long index_base, int distinct,
                             float* top_score, int64_t* top_index, int32_t* top_subject, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, top_subject};
    RC(search_pre(h, "ffr_search_topk_subjects", false, query, Q, gallery, gallery_norms, nullptr, nullptr, gallery_subject, G, dim, k,
                  distinct, top, true));
    return exact_search(h, query, Q, gallery, gallery_norms, gallery_subject, G, dim, k, index_base, distinct, top, (hipStream_t)stream);
}

// The subject search under a per-probe filter.  It takes subjects or not: with either of gallery_subject and top_subject it is
// checked as the subject entry is (both are needed; at G = 0 the gallery side may be null), without them as the plain one
int ffr_search_topk_filtered(ffr_handle* h, const float* query, const uint32_t* query_mask, int Q, const float* gallery,
                             const float* gallery_norms, const uint32_t* gallery_tag, const int32_t* gallery_subject, long long G,
                             int dim, int k, long long index_base, int distinct, float* top_score, int64_t* top_index,
                             int32_t* top_subject, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, top_subject};
    const SearchFilter flt{gallery_tag, query_mask};
    const bool subj = gallery_subject || top_subject;
    RC(search_pre(h, "ffr_search_topk_filtered", false, query, Q, gallery, gallery_norms, nullptr, nullptr, gallery_subject, G, dim, k,
                  distinct, top, subj, &flt));
    return exact_search(h, query, Q, gallery, gallery_norms, gallery_subject, G, dim, k, index_base, distinct, top, (hipStream_t)stream,
                        flt);
}

// The body of ffr_topk_merge and of ffr_topk_merge_subjects (subj: the lists carry subjects)
static int merge_entry(ffr_handle* h, const char* who, bool subj, const float* score, const int64_t* index, const int32_t* subject,
                       int S, int Q, int k, int distinct, const TopLists& out, hipStream_t st) {
    RC(check_fwd(h, false, false, 1));
    if (!score || !index || !out.s || !out.i || (subj && (!subject || !out.u)) || S < 1 || S > 4096 || Q < 1 || k < 1 || k > 128)
        return fail(h, FFR_ERR_ARG, "%s: bad arguments (1 <= S <= 4096, Q >= 1, 1 <= k <= 128, non-null pointers)", who);
    RC(check_distinct(h, who, distinct, k));
    const double slot = subj ? 16.0 : 12.0;
    Scope s(h, st, FFR_KC_SCORE, 0.0, slot * (double)S * Q * k + slot * Q * k);
    HIPCK(h, launch_topk_merge(score, index, subject, S, Q, k, distinct, out.s, out.i, out.u, st));
    return FFR_OK;
}

int ffr_topk_merge(ffr_handle* h, const float* score, const int64_t* index, int S, int Q, int k, float* out_score,
                   int64_t* out_index, void* stream) {
    FFR_DEVICE_SCOPE(h);
    return merge_entry(h, "ffr_topk_merge", false, score, index, nullptr, S, Q, k, 0, {out_score, out_index, nullptr}, (hipStream_t)stream);
}

int ffr_topk_merge_subjects(ffr_handle* h, const float* score, const int64_t* index, const int32_t* subject, int S, int Q,
                            int k, int distinct, float* out_score, int64_t* out_index, int32_t* out_subject, void* stream) {
    FFR_DEVICE_SCOPE(h);
    return merge_entry(h, "ffr_topk_merge_subjects", true, score, index, subject, S, Q, k, distinct,
                       {out_score, out_index, out_subject}, (hipStream_t)stream);
}

// ---- certified bf16 shortlist search (search_coarse.hip) -----------------------------------------------------------------
int ffr_coarse_pack(ffr_handle* h, const float* rows, const float* norms, long long n, int dim, uint16_t* plane, int* plane_flag,
                    void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    RC(check_dim(h, "ffr_coarse_pack", dim));
    if (!rows || !norms || !plane || !plane_flag || n < 1) return fail(h, FFR_ERR_ARG, "ffr_coarse_pack: bad arguments (n >= 1, non-null pointers)");
    if (misaligned16(rows) || misaligned16(plane)) return fail(h, FFR_ERR_ARG, "ffr_coarse_pack: rows and plane must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Scope s(h, st, FFR_KC_SCORE, 1.0 * n * dim, 6.0 * n * dim + 4.0 * n);
    HIPCK(h, launch_coarse_pack(rows, norms, n, plane, plane_flag, st));
    return FFR_OK;
}

// The shortlist search of checked arguments: ffr_search_topk_coarse (subject = null), ffr_search_topk_coarse_subjects,
// whose pass skips the removed rows, whose lists carry a subject plane and whose exact pass is the subject search, and
// ffr_search_topk_coarse_filtered (flt), whose pass also skips the rows inadmissible for the probe and whose exact pass is the
// filtered search, every gathered probe under its own mask
static int coarse_search(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                         const uint16_t* gallery_plane, const int* plane_flag, const int32_t* subject, long long G, int dim, int k,
                         long long index_base, int distinct, const TopLists& top, int* certified, hipStream_t st,
                         const SearchFilter& flt = {}) {
    if (G == 0 || k > coarse_max_k(distinct)) {  // nothing to shortlist, or a k the pass does not serve (64 rows, 32 identities):
        if (certified) HIPCK(h, hipMemsetAsync(certified, 0, sizeof(int) * (size_t)Q, st));      // the exact search alone
        return exact_search(h, query, Q, gallery, gallery_norms, subject, G, dim, k, index_base, distinct, top, st, flt);
    }
    const int kp = coarse_shortlist_size(k, distinct);
    int T = 0, S = 0, Tf = 0, Sf = 0;
    long long chunk_rows = 0, chunk_f = 0;
    search_plan(Q, G, h->num_cus, &T, &S, &chunk_rows);
    coarse_fallback_plan(Q, G, h->num_cus, &Tf, &Sf, &chunk_f);
    // scratch: probe norms [Q]; shortlists [Q][kp]; the uncertified probes' ids [Q], count, rows [Q][512], norms [Q] and exact
    // lists [Q][k]; the chunk lists of the coarse pass [S][Q][kp] and then of the exact pass [Sf][Q][k], in the same space;
    // with subjects, a third plane for the exact lists and their chunk lists; with a filter, the uncertified probes' masks [Q]
    const size_t part_n = std::max(S > 1 ? (size_t)S * Q * kp : 0, Sf > 1 ? (size_t)Sf * Q * k : 0);
    float *qnorm = nullptr, *uq = nullptr, *uqn = nullptr;
    TopLists sl, fb, part;
    int *ulist = nullptr, *ucount = nullptr;
    uint32_t* uqm = nullptr;
    RC(carve(h, h->search, "search", [&](Arena& a) {
        qnorm = a.take(Q);
        sl.s = a.take((size_t)Q * kp); sl.i = a.take<int64_t>((size_t)Q * kp);
        ulist = a.take<int>(Q); ucount = a.take<int>(1);
        uq = a.take((size_t)Q * dim); uqn = a.take(Q);
        fb.s = a.take((size_t)Q * k); fb.i = a.take<int64_t>((size_t)Q * k);
        if (part_n) { part.s = a.take(part_n); part.i = a.take<int64_t>(part_n); }
        if (subject) {
            fb.u = a.take<int32_t>((size_t)Q * k);
            if (Sf > 1) part.u = a.take<int32_t>((size_t)Sf * Q * k);
        }
        if (flt.qmask) uqm = a.take<uint32_t>(Q);
    }));
    Scope s(h, st, FFR_KC_SCORE, 2.0 * Q * (double)G * dim,
            2.0 * (double)G * (dim + 2) + 4.0 * Q * dim + 12.0 * Q * (k + kp) + (subject ? 4.0 * (double)G + 4.0 * Q * k : 0.0) +
                (flt.qmask ? 4.0 * (double)G + 4.0 * Q : 0.0));
    HIPCK(h, launch_row_norms(query, Q, qnorm, st));
    HIPCK(h, hipMemsetAsync(ucount, 0, sizeof(int), st));
    // the coarse pass: shortlists by coarse score, index = gallery row (no base), every probe, without a subject plane
    const TopLists& cl = S > 1 ? part : sl;
    const SearchArgs ca{query, qnorm, nullptr, gallery_plane, gallery_norms, G, chunk_rows, 0, cl.s, cl.i, nullptr, Q, kp, S, T,
                        subject, nullptr, flt.tag, flt.qmask};
    static_assert(SEARCH_COARSE_LIVE - SEARCH_COARSE == 1 && SEARCH_COARSE_FILTERED_LIVE - SEARCH_COARSE_FILTERED == 1,
                  "the live kernel follows the plain one");
    HIPCK(h, launch_search(ca, (SearchKernel)((flt.qmask ? SEARCH_COARSE_FILTERED : SEARCH_COARSE) + (subject ? 1 : 0)), st));
    if (S > 1) HIPCK(h, launch_topk_merge(part.s, part.i, nullptr, S, Q, kp, 0, sl.s, sl.i, nullptr, st));
    HIPCK(h, launch_search_rescore(query, qnorm, Q, gallery, gallery_norms, sl.s, sl.i, plane_flag, G, k, kp, index_base, top.s, top.i,
                                   certified, ulist, ucount, st, subject, distinct, top.u, flt.qmask != nullptr));
    // the exact search of the probes that were not certified, sized for Q: tiles past the device count leave at once
    HIPCK(h, launch_probe_gather(query, qnorm, ulist, ucount, Q, uq, uqn, st, flt.qmask, uqm));
    RC(exact_pass(h, uq, uqn, Q, gallery, gallery_norms, subject, G, k, index_base, distinct, Tf, Sf, chunk_f, fb, part, ucount, st,
                  SearchFilter{flt.tag, uqm}));
    HIPCK(h, launch_topk_scatter(fb.s, fb.i, ulist, ucount, Q, k, top.s, top.i, st, fb.u, top.u));
    return FFR_OK;
}

int ffr_search_topk_coarse(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                           const uint16_t* gallery_plane, const int* plane_flag, long long G, int dim, int k, long long index_base,
                           float* top_score, int64_t* top_index, int* certified, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, nullptr};
    RC(search_pre(h, "ffr_search_topk_coarse", true, query, Q, gallery, gallery_norms, gallery_plane, plane_flag, nullptr, G, dim, k, 0,
                  top, false));
    return coarse_search(h, query, Q, gallery, gallery_norms, gallery_plane, plane_flag, nullptr, G, dim, k, index_base, 0, top,
                         certified, (hipStream_t)stream);
}

int ffr_search_topk_coarse_subjects(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                                    const uint16_t* gallery_plane, const int* plane_flag, const int32_t* gallery_subject, long long G,
                                    int dim, int k, long long index_base, int distinct, float* top_score, int64_t* top_index,
                                    int32_t* top_subject, int* certified, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, top_subject};
    RC(search_pre(h, "ffr_search_topk_coarse_subjects", true, query, Q, gallery, gallery_norms, gallery_plane, plane_flag,
                  gallery_subject, G, dim, k, distinct, top, true));
    return coarse_search(h, query, Q, gallery, gallery_norms, gallery_plane, plane_flag, gallery_subject, G, dim, k, index_base, distinct,
                         top, certified, (hipStream_t)stream);
}

// The filtered search through the shortlist: checked as ffr_search_topk_filtered and as the coarse entries are
int ffr_search_topk_coarse_filtered(ffr_handle* h, const float* query, const uint32_t* query_mask, int Q, const float* gallery,
                                    const float* gallery_norms, const uint16_t* gallery_plane, const int* plane_flag,
                                    const uint32_t* gallery_tag, const int32_t* gallery_subject, long long G, int dim, int k,
                                    long long index_base, int distinct, float* top_score, int64_t* top_index, int32_t* top_subject,
                                    int* certified, void* stream) {
    FFR_DEVICE_SCOPE(h);
    const TopLists top{top_score, top_index, top_subject};
    const SearchFilter flt{gallery_tag, query_mask};
    const bool subj = gallery_subject || top_subject;
    RC(search_pre(h, "ffr_search_topk_coarse_filtered", true, query, Q, gallery, gallery_norms, gallery_plane, plane_flag,
                  gallery_subject, G, dim, k, distinct, top, subj, &flt));
    return coarse_search(h, query, Q, gallery, gallery_norms, gallery_plane, plane_flag, gallery_subject, G, dim, k, index_base, distinct,
                         top, certified, (hipStream_t)stream, flt);
}

// ---- clustering (cluster.hip) ----------------------------------------------------------------------------------------
// What the six clustering entries check and plan alike.  The pairs an entry walks with k_cluster_walk:
enum ClusterPairs {
    PAIRS_NONE,     // none (the removals walk lists)
    PAIRS_ALL,      // every pair i < j: cluster_plan
    PAIRS_NEW       // the pairs with a row >= N_old: N_old is an argument, cluster_extend_plan
};
struct ClusterAligned { const void* p; unsigned mask; };     // the address must be a multiple of mask + 1; null passes
struct ClusterPre {
    bool empty = false;       // N = 0: the entry returns FFR_OK
    bool scores = false;      // are there pairs to score?  If not, no norms are needed
    long long n_new = 0;
    int T = 0, S = 0;         // the plan of the walk (PAIRS_NONE: unset)
    long long chunk_rows = 0;
};

// The checks in the order every entry makes them: handle, dim, N, N_old, threshold, min_rows (null: the entry has none),
// then for N > 0 the null pointers (`missing`; the message lists `missing_names`), the alignment (emb 16, norms 4 and
// `aligned`; the message gives `aligned_names`), the plan and the grid limit.  `who` names the entry in messages.
static int cluster_pre(ffr_handle* h, const char* who, ClusterPairs pairs, const float* emb, const float* norms, long long N_old,
                       long long N, int dim, float threshold, const int* min_rows, bool missing, const char* missing_names,
                       std::initializer_list<ClusterAligned> aligned, const char* aligned_names, ClusterPre* p) {
    RC(check_fwd(h, false, false, 1));
    RC(check_dim(h, who, dim));
    if (N < 0 || N >= (1ll << 31)) return fail(h, FFR_ERR_ARG, "%s: N must be in [0, 2^31), got %lld", who, N);
    if (pairs == PAIRS_NEW && (N_old < 0 || N_old > N))
        return fail(h, FFR_ERR_ARG, "%s: N_old must be in [0, N = %lld], got %lld", who, N, N_old);
    if (threshold != threshold) return fail(h, FFR_ERR_ARG, "%s: the threshold is NaN", who);
    if (min_rows && *min_rows < 1) return fail(h, FFR_ERR_ARG, "%s: min_rows must be >= 1, got %d", who, *min_rows);
    p->empty = N == 0;
    if (p->empty) return FFR_OK;
    if (!emb || missing) return fail(h, FFR_ERR_ARG, "%s: %s is null", who, missing_names);
    bool off = misaligned16(emb) || ((uintptr_t)norms & 3);
    for (const ClusterAligned& a : aligned) off = off || ((uintptr_t)a.p & a.mask);
    if (off) return fail(h, FFR_ERR_ARG, "%s: emb rows must be 16-byte aligned (%s)", who, aligned_names);
    p->n_new = N - N_old;
    p->scores = pairs == PAIRS_ALL || (N > 1 && p->n_new > 0);
    if (pairs == PAIRS_ALL) cluster_plan(N, h->num_cus, &p->T, &p->S, &p->chunk_rows);
    else if (pairs == PAIRS_NEW && p->scores) cluster_extend_plan(N_old, N, h->num_cus, &p->T, &p->S, &p->chunk_rows);
    if ((long long)p->T * p->S >= (1ll << 31)) {
        if (pairs == PAIRS_NEW)
            return fail(h, FFR_ERR_UNSUPPORTED, "%s: N = %lld with %lld new rows needs %lld blocks, over the grid limit", who, N, p->n_new,
                        (long long)p->T * p->S);
        return fail(h, FFR_ERR_UNSUPPORTED, "%s: N = %lld needs %lld blocks, over the grid limit", who, N, (long long)p->T * p->S);
    }
    return FFR_OK;
}

// our own norms (scratch of the entry's carve) where the caller passed none and pairs are scored
static int cluster_norms(ffr_handle* h, const ClusterPre& p, const float* emb, long long N, float* own_norms, hipStream_t st,
                         const float** norms) {
    if (*norms || !p.scores) return FFR_OK;
    HIPCK(h, launch_row_norms(emb, N, own_norms, st));
    *norms = own_norms;
    return FFR_OK;
}

// The body of ffr_cluster_threshold (ext = false: no prior, N_old = 0) and of ffr_cluster_extend; `who` names the entry in messages
static int cluster_rows(ffr_handle* h, const char* who, bool ext, const float* emb, const float* norms, long long N_old,
                        long long N, int dim, float threshold, const int64_t* prior, int64_t* rep, void* stream) {
    FFR_DEVICE_SCOPE(h);
    ClusterPre p;
    RC(cluster_pre(h, who, ext ? PAIRS_NEW : PAIRS_ALL, emb, norms, N_old, N, dim, threshold, nullptr, !rep || (ext && !prior),
                   ext ? "emb / prior / rep" : "emb / rep", {{rep, 7}, {prior, 7}}, ext ? "prior and rep 8, norms 4" : "rep 8, norms 4", &p));
    if (p.empty) return FFR_OK;
    hipStream_t st = (hipStream_t)stream;
    // scratch: row norms [N] (used when the caller passes none), then parent [N]
    float* own_norms = nullptr;
    int* parent = nullptr;
    RC(carve(h, h->cluster, "clustering", [&](Arena& a) { own_norms = a.take(N); parent = a.take<int>(N); }));
    const double n_new = (double)p.n_new;
    const double pairs = ext ? 2.0 * (double)N_old * n_new + n_new * (n_new - 1) : (double)N * (double)(N - 1);
    Scope s(h, st, FFR_KC_SCORE, dim * pairs, 2.0 * (double)N * (dim + 1) + (ext ? 24.0 : 16.0) * N);
    RC(cluster_norms(h, p, emb, N, own_norms, st, &norms));
    HIPCK(h, launch_cluster_extend(emb, norms, N_old, N, threshold, p.T, p.S, p.chunk_rows, prior, parent, rep, st));
    return FFR_OK;
}

int ffr_cluster_threshold(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                          int64_t* rep, void* stream) {
    return cluster_rows(h, "ffr_cluster_threshold", false, emb, norms, 0, N, dim, threshold, nullptr, rep, stream);
}

int ffr_cluster_extend(ffr_handle* h, const float* emb, const float* norms, long long N_old, long long N, int dim,
                       float threshold, const int64_t* prior, int64_t* rep, void* stream) {
    return cluster_rows(h, "ffr_cluster_extend", true, emb, norms, N_old, N, dim, threshold, prior, rep, stream);
}

int ffr_cluster_remove(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                       const int64_t* rep_in, const int64_t* prior, const uint8_t* keep, int64_t* rep, void* stream) {
    FFR_DEVICE_SCOPE(h);
    ClusterPre p;
    RC(cluster_pre(h, "ffr_cluster_remove", PAIRS_NONE, emb, norms, 0, N, dim, threshold, nullptr, !rep || !rep_in || !keep,
                   "emb / rep_in / keep / rep", {{rep, 7}, {rep_in, 7}, {prior, 7}}, "rep_in, prior and rep 8, norms 4", &p));
    if (p.empty) return FFR_OK;
    hipStream_t st = (hipStream_t)stream;
    // scratch: row norms [N] (used when the caller passes none), parent, the guarded labels, the hit flags and the list of
    // affected survivors [N] ints each, and the list's count
    float* own_norms = nullptr;
    int *parent = nullptr, *glabel = nullptr, *hit = nullptr, *list = nullptr, *mcount = nullptr;
    RC(carve(h, h->cluster, "clustering", [&](Arena& a) {
        own_norms = a.take(N); parent = a.take<int>(N); glabel = a.take<int>(N); hit = a.take<int>(N); list = a.take<int>(N);
        mcount = a.take<int>(1);
    }));
    // the pairs scored, m (m - 1) for m affected survivors, are counted on the device only: 0 flops are recorded; bytes: the
    // labels in and out, keep, and the N-sized scratch written and read
    Scope s(h, st, FFR_KC_SCORE, 0.0, (prior ? 57.0 : 49.0) * (double)N);
    RC(cluster_norms(h, p, emb, N, own_norms, st, &norms));
    HIPCK(h, launch_cluster_remove(emb, norms, N, threshold, cluster_list_grid(N, h->num_cus), rep_in, prior, keep, parent, glabel,
                                   hit, list, mcount, rep, st));
    return FFR_OK;
}

int ffr_cluster_density(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold, int min_rows,
                        int64_t* rep, uint8_t* kind, int32_t* degree, void* stream) {
    FFR_DEVICE_SCOPE(h);
    ClusterPre p;
    RC(cluster_pre(h, "ffr_cluster_density", PAIRS_ALL, emb, norms, 0, N, dim, threshold, &min_rows, !rep || !kind, "emb / rep / kind",
                   {{rep, 7}, {degree, 3}}, "rep 8, degree and norms 4", &p));
    if (p.empty) return FFR_OK;
    hipStream_t st = (hipStream_t)stream;
    // scratch: row norms [N] (used when the caller passes none), parent, degree, root, minrow [N] ints, best [N] 8-byte words
    float* own_norms = nullptr;
    int *parent = nullptr, *deg = nullptr, *root = nullptr, *minrow = nullptr;
    unsigned long long* best = nullptr;
    RC(carve(h, h->cluster, "clustering", [&](Arena& a) {
        own_norms = a.take(N); parent = a.take<int>(N); deg = a.take<int>(N); root = a.take<int>(N); minrow = a.take<int>(N);
        best = a.take<unsigned long long>(N);
    }));
    // the triangle is walked twice: degrees, then the gated join; bytes: the rows twice, 24 of scratch per row written and
    // read, rep, kind and degree
    Scope s(h, st, FFR_KC_SCORE, 2.0 * dim * (double)N * (double)(N - 1), 4.0 * (double)N * (dim + 1) + (degree ? 61.0 : 57.0) * N);
    RC(cluster_norms(h, p, emb, N, own_norms, st, &norms));
    HIPCK(h, launch_cluster_density(emb, norms, N, threshold, min_rows, p.T, p.S, p.chunk_rows, parent, deg, root, minrow, best, rep,
                                    kind, degree, st));
    return FFR_OK;
}

int ffr_cluster_density_extend(ffr_handle* h, const float* emb, const float* norms, long long N_old, long long N, int dim,
                               float threshold, int min_rows, int64_t* rep, uint8_t* kind, int32_t* degree,
                               unsigned long long* best, void* stream) {
    FFR_DEVICE_SCOPE(h);
    ClusterPre p;
    RC(cluster_pre(h, "ffr_cluster_density_extend", PAIRS_NEW, emb, norms, N_old, N, dim, threshold, &min_rows,
                   !rep || !kind || !degree || !best, "emb / rep / kind / degree / best", {{rep, 7}, {best, 7}, {degree, 3}},
                   "rep and best 8, degree and norms 4", &p));
    if (p.empty) return FFR_OK;
    hipStream_t st = (hipStream_t)stream;
    // scratch: row norms [N] (used when the caller passes none), parent, the old degrees, the per-rep core minimum, root,
    // minrow [N] ints, the promoted rows [N_old] and their count; degree and best are the caller's state
    float* own_norms = nullptr;
    int *parent = nullptr, *deg0 = nullptr, *coremin = nullptr, *root = nullptr, *minrow = nullptr, *plist = nullptr, *pcount = nullptr;
    RC(carve(h, h->cluster, "clustering", [&](Arena& a) {
        own_norms = a.take(N); parent = a.take<int>(N); deg0 = a.take<int>(N); coremin = a.take<int>(N); root = a.take<int>(N);
        minrow = a.take<int>(N); plist = a.take<int>(N_old + 1); pcount = a.take<int>(1);
    }));
    // both range walks, plus the promoted pass at its upper bound m = N_old (m is known on the device only)
    const double n_new = (double)p.n_new;
    const double pairs = p.scores ? 2.0 * (2.0 * (double)N_old * n_new + n_new * (n_new - 1)) + 2.0 * (double)N_old * (double)N_old : 0.0;
    Scope s(h, st, FFR_KC_SCORE, dim * pairs, 4.0 * (double)N * (dim + 1) + 64.0 * N);
    RC(cluster_norms(h, p, emb, N, own_norms, st, &norms));
    HIPCK(h, launch_cluster_density_extend(emb, norms, N_old, N, threshold, min_rows, p.T, p.S, p.chunk_rows,
                                           cluster_list_grid(N_old, h->num_cus), parent, deg0, coremin, root, minrow, plist, pcount,
                                           rep, kind, degree, best, st));
    return FFR_OK;
}

int ffr_cluster_density_remove(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                               int min_rows, const uint8_t* keep, int64_t* rep, uint8_t* kind, int32_t* degree,
                               unsigned long long* best, void* stream) {
    FFR_DEVICE_SCOPE(h);
    ClusterPre p;
    RC(cluster_pre(h, "ffr_cluster_density_remove", PAIRS_NONE, emb, norms, 0, N, dim, threshold, &min_rows,
                   !keep || !rep || !kind || !degree || !best, "emb / keep / rep / kind / degree / best",
                   {{rep, 7}, {best, 7}, {degree, 3}}, "rep and best 8, degree and norms 4", &p));
    if (p.empty) return FFR_OK;
    hipStream_t st = (hipStream_t)stream;
    // scratch: row norms [N] (used when the caller passes none), parent, the old degrees, the per-rep core minimum, the hit
    // flags, root, minrow and the three lists [N] ints each, and the lists' counts; degree and best are the caller's state
    float* own_norms = nullptr;
    int *parent = nullptr, *deg0 = nullptr, *coremin = nullptr, *hit = nullptr, *root = nullptr, *minrow = nullptr, *rlist = nullptr,
        *llist = nullptr, *qlist = nullptr, *counts = nullptr;
    RC(carve(h, h->cluster, "clustering", [&](Arena& a) {
        own_norms = a.take(N); parent = a.take<int>(N); deg0 = a.take<int>(N); coremin = a.take<int>(N); hit = a.take<int>(N);
        root = a.take<int>(N); minrow = a.take<int>(N); rlist = a.take<int>(N); llist = a.take<int>(N); qlist = a.take<int>(N);
        counts = a.take<int>(3);
    }));
    // the pairs scored, (r + q) N + m (m - 1) / 2, are counted on the device only: 0 flops are recorded; bytes: the state in
    // and out, keep, kind, and the N-sized scratch written and read
    Scope s(h, st, FFR_KC_SCORE, 0.0, 114.0 * (double)N);
    RC(cluster_norms(h, p, emb, N, own_norms, st, &norms));
    HIPCK(h, launch_cluster_density_remove(emb, norms, N, threshold, min_rows, cluster_list_grid(N, h->num_cus), keep, parent, deg0,
                                           coremin, hit, root, minrow, rlist, llist, qlist, counts, rep, kind, degree, best, st));
    return FFR_OK;
}

int ffr_cluster_templates(ffr_handle* h, const float* emb, const float* norms, const int64_t* order, const int64_t* offsets,
                          long long C, int dim, float* templates, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    RC(check_dim(h, "ffr_cluster_templates", dim));
    if (C < 0 || C >= (1ll << 31)) return fail(h, FFR_ERR_ARG, "ffr_cluster_templates: C must be in [0, 2^31), got %lld", C);
    if (C == 0) return FFR_OK;
    if (!emb || !order || !offsets || !templates) return fail(h, FFR_ERR_ARG, "ffr_cluster_templates: a null pointer");
    if (misaligned16(emb) || misaligned16(templates) || ((uintptr_t)order & 7) || ((uintptr_t)offsets & 7) || ((uintptr_t)norms & 3))
        return fail(h, FFR_ERR_ARG, "ffr_cluster_templates: emb and templates rows must be 16-byte aligned (order, offsets 8, norms 4)");
    hipStream_t st = (hipStream_t)stream;
    Scope s(h, st, FFR_KC_SCORE, 0.0, 4.0 * (double)C * dim);
    HIPCK(h, launch_cluster_templates(emb, norms, order, offsets, C, templates, st));
    return FFR_OK;
}

// ---- face alignment (align.hip) --------------------------------------------------------------------------------------
static int align_tfm_check(ffr_handle* h, const float* landmarks, const float* tmpl, int K) {
    if (!landmarks || !tmpl || K < 2 || K > 16)
        return fail(h, FFR_ERR_ARG, "alignment transforms: bad arguments (non-null landmarks and template, 2 <= K <= 16)");
    return FFR_OK;
}

static int align_warp_check(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch,
                            const int32_t* frame_index, int oh, int ow) {
    if (!frames || !frame_index || F < 1 || H < 1 || W < 1)
        return fail(h, FFR_ERR_ARG, "alignment warp: bad arguments (non-null frames and frame_index, F, H, W >= 1)");
    if (oh < 1 || oh > 256 || ow < 1 || ow > 256 || (ow & 3))
        return fail(h, FFR_ERR_ARG, "alignment warp: out_h and out_w must be in 1..256 and out_w a multiple of 4, got %d x %d", oh, ow);
    if (pitch < 3ll * W) return fail(h, FFR_ERR_ARG, "alignment warp: pitch_bytes %lld < 3 * W = %d", pitch, 3 * W);
    if (pitch * H >= (1ll << 31))
        return fail(h, FFR_ERR_ARG, "alignment warp: a frame of %lld bytes is over the 2 GiB offset limit", pitch * H);
    return FFR_OK;
}

static int align_tfm(ffr_handle* h, const float* landmarks, const float* tmpl, int N, int K, const int32_t* frame_index, int F,
                     double* A, uint8_t* valid, hipStream_t st) {
    Scope s(h, st, FFR_KC_LAYOUT, 40.0 * N * K, 8.0 * N * K + 49.0 * N);
    HIPCK(h, launch_align_tfm(landmarks, tmpl, N, K, (const int*)frame_index, F, A, valid, st));
    return FFR_OK;
}

static int align_warp(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch, const int32_t* frame_index,
                      const double* A, const uint8_t* valid, int N, int oh, int ow, uint8_t* crop, hipStream_t st) {
    Scope s(h, st, FFR_KC_LAYOUT, 0, 15.0 * N * oh * ow);      // 4 taps read + 1 byte written per output byte
    HIPCK(h, launch_align_warp(frames, F, H, W, (int)pitch, (const int*)frame_index, A, valid, N, oh, ow, crop, st));
    return FFR_OK;
}

int ffr_align_transforms(ffr_handle* h, const float* landmarks, const float* tmpl, int N, int K, double* A, uint8_t* valid,
                         void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, N));
    RC(align_tfm_check(h, landmarks, tmpl, K));
    if (!A || !valid) return fail(h, FFR_ERR_ARG, "ffr_align_transforms: A / valid is null");
    return align_tfm(h, landmarks, tmpl, N, K, nullptr, 0, A, valid, (hipStream_t)stream);
}

int ffr_align_warp(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch_bytes, const int32_t* frame_index,
                   const double* A, const uint8_t* valid, int N, int out_h, int out_w, uint8_t* crop, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, N));
    RC(align_warp_check(h, frames, F, H, W, pitch_bytes, frame_index, out_h, out_w));
    if (!A || !crop) return fail(h, FFR_ERR_ARG, "ffr_align_warp: A / crop is null");
    if ((uintptr_t)crop & 3) return fail(h, FFR_ERR_ARG, "ffr_align_warp: crop must be 4-byte aligned");
    return align_warp(h, frames, F, H, W, pitch_bytes, frame_index, A, valid, N, out_h, out_w, crop, (hipStream_t)stream);
}

int ffr_embed_aligned(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch_bytes,
                      const int32_t* frame_index, const float* landmarks, const float* tmpl, int K, const uint8_t* flip, int N,
                      float* f_new, float* f, uint8_t* valid, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, true, N));
    if (!f_new) return fail(h, FFR_ERR_ARG, "f_new is null");
    RC(align_tfm_check(h, landmarks, tmpl, K));
    RC(align_warp_check(h, frames, F, H, W, pitch_bytes, frame_index, 112, 112));
    hipStream_t st = (hipStream_t)stream;
    // scratch: transforms [N][6] fp64, valid [N], crops [N][112][112][3]
    double* A = nullptr;
    uint8_t *v = nullptr, *crop = nullptr;
    RC(carve(h, h->align, "alignment", [&](Arena& a) {
        A = a.take<double>((size_t)N * 6);
        v = a.take<uint8_t>(N);
        crop = a.take<uint8_t>((size_t)N * 112 * 112 * 3);
    }));
    RC(align_tfm(h, landmarks, tmpl, N, K, frame_index, F, A, v, st));
    RC(align_warp(h, frames, F, H, W, pitch_bytes, frame_index, A, v, N, 112, 112, crop, st));
    if (valid) HIPCK(h, hipMemcpyAsync(valid, v, (size_t)N, hipMemcpyDeviceToDevice, st));
    const U8In u8{crop, flip};
    return embed_tail(h, nullptr, &u8, N, f_new, f, st);
}

// ---- per-layer arithmetic plan --------------------------------------------------------------------------------------
int ffr_layer_count(const ffr_handle* h, int* n) {
    if (!h || !n) return fail(const_cast<ffr_handle*>(h), FFR_ERR_ARG, "ffr_layer_count: null argument");
    *n = (int)plan_layers(h).size();
    return FFR_OK;
}

int ffr_layer_get(const ffr_handle* h, int i, ffr_layer_info* out) {
    if (!h || !out) return fail(const_cast<ffr_handle*>(h), FFR_ERR_ARG, "ffr_layer_get: null argument");
    const std::vector<PlanLayer> v = plan_layers(h);
    if (i < 0 || i >= (int)v.size()) return fail(const_cast<ffr_handle*>(h), FFR_ERR_ARG, "ffr_layer_get: index %d outside [0, %d)", i, (int)v.size());
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", v[i].name.c_str());
    out->net = v[i].net;
    out->arith = v[i].L->direct ? FFR_ARITH_DIRECT : FFR_ARITH_WINOGRAD;
    out->sensitivity = v[i].L->sensitivity;
    return FFR_OK;
}

int ffr_layer_set_arith(ffr_handle* h, int i, int arith) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    if (arith != FFR_ARITH_DIRECT && arith != FFR_ARITH_WINOGRAD) return fail(h, FFR_ERR_ARG, "ffr_layer_set_arith: arith %d is neither 0 (direct) nor 1 (Winograd)", arith);
    const std::vector<PlanLayer> v = plan_layers(h);
    if (i < 0 || i >= (int)v.size()) return fail(h, FFR_ERR_ARG, "ffr_layer_set_arith: index %d outside [0, %d)", i, (int)v.size());
    const bool direct = arith == FFR_ARITH_DIRECT;
    if (v[i].L->direct != direct) { v[i].L->direct = direct; plan_changed(h); }
    return FFR_OK;
}

int ffr_calibrate(ffr_handle* h, const float* x, const float* featmap, int N, int H, int W, double tol, double* achieved,
                  void* stream) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    hipStream_t st = (hipStream_t)stream;
    {   // first, before anything is enqueued: a calibration synchronises, which a capture cannot hold
        FFR_DEVICE_SCOPE(h);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCK(h, hipStreamIsCapturing(st, &cs));
        if (cs != hipStreamCaptureStatusNone) return fail(h, FFR_ERR_ARG, "ffr_calibrate: the stream is capturing (the call synchronises)");
    }
    if (!(tol > 0.0)) return fail(h, FFR_ERR_ARG, "ffr_calibrate: tol must be > 0 (got %g)", tol);
    if ((x != nullptr) == (featmap != nullptr)) return fail(h, FFR_ERR_ARG, "ffr_calibrate: pass images (x) or a featmap, exactly one of them");
    const bool enc = x != nullptr;
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, enc, !enc, N));
    if (enc) RC(check_hw(h, H, W));
    if (!enc && (H != 7 || W != 7)) return fail(h, FFR_ERR_ARG, "ffr_calibrate: a featmap is [N,512,7,7] (H = W = 7)");
    const bool is112 = enc && H == 112 && W == 112;
    const bool rec = !enc || (h->rec_loaded && is112);
    const int P = enc ? (H / 16) * (W / 16) : 49;

    // candidates: the layers this forward runs; the plan of the others stays as it is
    std::vector<ConvW*> cand;
    for (const PlanLayer& pl : plan_layers(h))
        if ((pl.net == 0 && enc) || (pl.net == 1 && rec)) cand.push_back(pl.L);
    const int L = (int)cand.size();
    struct Saved {      // the plan and the profiling switch come back on every path; device buffers are released
        ffr_handle* h; std::vector<std::pair<ConvW*, bool>> plan; bool prof; void* buf = nullptr; bool keep = false;
        ~Saved() {
            if (buf) { hipDeviceSynchronize(); hipFree(buf); }
            h->prof = prof;
            if (!keep) for (auto& p : plan) p.first->direct = p.second;
        }
    } sv{h, {}, h->prof};
    for (ConvW* c : cand) sv.plan.push_back({c, c->direct});
    h->prof = false;          // calibration forwards are not part of any measurement

    // every candidate on Winograd while the workspace is prepared: the exact-tiling weight sets of all eligible layers are
    // derived now (synchronous, once), so that no forward below needs them derived
    for (ConvW* c : cand) c->direct = false;
    h->mixed_ready_n = 0;
    Work w;
    if (enc) RC(ensure_arena_encoder(h, N, H, W, &w));
    else RC(ensure_arena(h, N, 112, 112, &w));

    // outputs: 0 f, 1 featmap, 2 f_new, 3 feat_new (NHWC rows of 512); where the current forward leaves them / the anchor copy
    const bool have[4] = {is112, enc, rec, rec};
    const size_t rows[4] = {(size_t)N, (size_t)N * P, (size_t)N, (size_t)N * 49};
    float* featmap_nhwc = rec ? w.X : w.trunk_bn;
    const int max_trials = 2 * L + 4;
    const size_t scratch = (size_t)absdiff_scratch_floats();
    size_t floats = scratch + (size_t)max_trials * 4 * 2 + 2 * (size_t)N * 512;        // scratch, table, f / f_new of the forward
    size_t off_anchor[4];
    for (int t = 0; t < 4; ++t) { off_anchor[t] = floats; floats += have[t] ? rows[t] * 512 : 0; }
    HIPCK(h, hipMalloc(&sv.buf, floats * sizeof(float)));
    float* base = (float*)sv.buf;
    float* part = base;
    float* table = base + scratch;
    float* f_cur = table + (size_t)max_trials * 8;
    float* fnew_cur = f_cur + (size_t)N * 512;
    const float* cur[4] = {f_cur, featmap_nhwc, fnew_cur, w.m512c};
    float* anchor[4];
    for (int t = 0; t < 4; ++t) anchor[t] = base + off_anchor[t];
    HIPCK(h, hipMemsetAsync(table, 0, (size_t)max_trials * 8 * sizeof(float), st));

    auto forward = [&]() -> int {
        if (enc) RC(run_encoder(h, w, x, N, H, W, featmap_nhwc, is112 ? f_cur : nullptr, st));
        else RC(featmap_to_x(h, w, featmap, N, st));
        if (rec) RC(run_recnet(h, w, N, fnew_cur, nullptr, st));
        return FFR_OK;
    };
    auto compare = [&](int slot) -> int {
        for (int t = 0; t < 4; ++t)
            if (have[t]) HIPCK(h, launch_absdiff_max(cur[t], 512, anchor[t], 512, (int)rows[t], 512, part, table + ((size_t)slot * 4 + t) * 2, st));
        return FFR_OK;
    };
    std::vector<float> host((size_t)max_trials * 8);
    auto read = [&]() -> int {          // the phase's one copy to the host
        HIPCK(h, hipMemcpyAsync(host.data(), table, host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCK(h, hipStreamSynchronize(st));
        return FFR_OK;
    };
    // inf / inf (an anchor that holds an infinity) is NaN, which std::max below would drop: it counts as +inf, as in k_absdiff_max
    auto rel = [&](int slot, int t) {
        const float* q = &host[((size_t)slot * 4 + t) * 2];
        const double r = q[1] > 0.f ? (double)q[0] / q[1] : (double)q[0];
        return r != r ? (double)INFINITY : r;
    };
    auto err = [&](int slot) { double e = 0.0; for (int t = 0; t < 4; ++t) if (have[t]) e = std::max(e, rel(slot, t)); return e; };
    auto set_plan = [&](const std::vector<char>& wino) { for (int k = 0; k < L; ++k) cand[k]->direct = !wino[k]; };

    // phase 1: anchor (all direct), slot 0 = all Winograd, slot 1 + k = only layer k on Winograd
    set_plan(std::vector<char>(L, 0));
    RC(forward());
    for (int t = 0; t < 4; ++t)
        if (have[t]) HIPCK(h, hipMemcpyAsync(anchor[t], cur[t], rows[t] * 512 * sizeof(float), hipMemcpyDeviceToDevice, st));
    set_plan(std::vector<char>(L, 1));
    RC(forward()); RC(compare(0));
    for (int k = 0; k < L; ++k) {
        std::vector<char> one(L, 0);
        one[k] = 1;
        set_plan(one);
        RC(forward()); RC(compare(1 + k));
    }
    RC(read());
    const double half = 0.5 * tol;
    for (int k = 0; k < L; ++k) cand[k]->sensitivity = err(1 + k);
    std::vector<int> order(L);
    for (int k = 0; k < L; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand[a]->sensitivity < cand[b]->sensitivity; });
    auto prefix_plan = [&](int p) { std::vector<char> v(L, 0); for (int i = 0; i < p; ++i) v[order[i]] = 1; return v; };

    // phase 2: the passing prefixes of the sensitivity order (p = L is slot 0 above; p = 0 is the anchor itself)
    std::vector<int> passing;           // prefix lengths <= tol / 2, longest first
    if (err(0) <= half) passing.push_back(L);
    else if (L > 1) {
        for (int p = 1; p < L; ++p) { set_plan(prefix_plan(p)); RC(forward()); RC(compare(p)); }
        RC(read());
        // Only prefixes whose every shorter prefix passes too.  The error is not monotone in the prefix length (one more layer on
        // Winograd can cancel part of the others' error on THESE images), and a longer prefix that passes by such a cancellation
        // does not hold on other images: on the trained-like family the longest passing prefix left held-out images at 3.1 x the
        // calibration error, above tol.
        int pmax = 0;
        while (pmax + 1 < L && err(pmax + 1) <= half) ++pmax;
        for (int p = pmax; p >= 1; --p) passing.push_back(p);
    }
    passing.push_back(0);

    // phase 3: verify the chosen plan with one more forward; should it fail, the next shorter passing prefix is verified
    for (int p : passing) {
        set_plan(prefix_plan(p));
        RC(forward()); RC(compare(0));
        RC(read());
        if (err(0) <= half || p == 0) break;
    }
    if (achieved) for (int t = 0; t < 4; ++t) achieved[t] = have[t] ? rel(0, t) : -1.0;
    sv.keep = true;
    bool changed = false;
    for (auto& pr : sv.plan) changed |= pr.first->direct != pr.second;
    if (changed) plan_changed(h);
    else h->mixed_ready_n = 0;
    return FFR_OK;
}

namespace {
struct OptEntry { const char* name; int ffr_eng::Options::*i; long long ffr_eng::Options::*l; long long lo, hi; };
const OptEntry OPTIONS[] = {
    {"wino", &Options::wino, nullptr, 0, 1}, {"wino_mincin", &Options::wino_mincin, nullptr, 0, 1 << 20},
    {"wino_fused", &Options::wino_fused, nullptr, 0, 1},
    {"wf_phased_maxk", &Options::wf_phased_maxk, nullptr, 0, 1 << 20}, {"wf_minblocks", nullptr, &Options::wf_minblocks, 0, 1LL << 40},
    {"se_maxtiles", &Options::se_maxtiles, nullptr, 0, 1 << 20}, {"wf_tailsplit", &Options::wf_tailsplit, nullptr, 0, 1},
    {"gemm_stream", &Options::gemm_stream, nullptr, 0, 1}, {"sk_minunits", &Options::sk_minunits, nullptr, 1, 1 << 20},
    {"combine_v", &Options::combine_v, nullptr, 0, 1}, {"wf_split", &Options::wf_split, nullptr, 0, 1}, {"wf_mixed", &Options::wf_mixed, nullptr, 0, 1},
    {"channel_rows", &Options::channel_rows, nullptr, 0, 4}, {"igemm_split", &Options::igemm_split, nullptr, 0, 1},
    {"wf_trace", &Options::wf_trace, nullptr, 0, 1}, {"igemm_trace", &Options::igemm_trace, nullptr, 0, 1},
};
long long option_value(const Options& o, const OptEntry& e) { return e.i ? (long long)(o.*(e.i)) : o.*(e.l); }
const OptEntry* find_option(const char* name) {
    if (name) for (const OptEntry& e : OPTIONS) if (!strcmp(e.name, name)) return &e;
    return nullptr;
}
}  // namespace

int ffr_set_option(ffr_handle* h, const char* name, long long value) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    const OptEntry* e = find_option(name);
    if (!e) return fail(h, FFR_ERR_ARG, "ffr_set_option: unknown option '%s'", name ? name : "(null)");
    if (value < e->lo || value > e->hi) return fail(h, FFR_ERR_ARG, "ffr_set_option: %s = %lld is outside [%lld, %lld]", name, value, e->lo, e->hi);
    if (e->i == &Options::channel_rows && value == 3) return fail(h, FFR_ERR_ARG, "ffr_set_option: channel_rows is 0 (auto), 1, 2 or 4");
#ifndef FFR_TRACE
    if ((e->i == &Options::wf_trace || e->i == &Options::igemm_trace) && value)
        return fail(h, FFR_ERR_UNSUPPORTED, "ffr_set_option: %s needs a -DFFR_TRACE build of the library (tools/trace_build.py)", name);
#endif
    // every knob changes which kernels a forward launches or which scratch buffers they use: a hipGraph captured
    // before the change replays the OLD sequence, so a changed value invalidates captures (GraphedEmbed re-captures
    // when ffr_generation moves)
    if (option_value(h->opt, *e) != value) ++h->generation;
    if (e->i) h->opt.*(e->i) = (int)value; else h->opt.*(e->l) = value;
    return FFR_OK;
}

int ffr_get_option(const ffr_handle* h, const char* name, long long* value) {
    if (!h || !value) return fail(nullptr, FFR_ERR_ARG, "ffr_get_option: bad arguments");
    const OptEntry* e = find_option(name);
    if (!e) return fail(const_cast<ffr_handle*>(h), FFR_ERR_ARG, "ffr_get_option: unknown option '%s'", name ? name : "(null)");
    *value = option_value(h->opt, *e);
    return FFR_OK;
}

int ffr_probe_mfma_peak(ffr_handle* h, int iters, double* tflops, double* clock_ghz, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    if (iters <= 0 || !tflops) return fail(h, FFR_ERR_ARG, "ffr_probe_mfma_peak: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = h->num_cus * 2;             // 2 blocks of 4 waves per CU
    struct Res {                                   // released on every path
        unsigned long long* stamps = nullptr; float* sink = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Res() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); if (stamps) hipFree(stamps); if (sink) hipFree(sink); }
    } r;
    HIPCK(h, hipMalloc((void**)&r.stamps, (size_t)blocks * 4 * sizeof(unsigned long long)));
    HIPCK(h, hipMalloc((void**)&r.sink, (size_t)blocks * 256 * sizeof(float)));
    HIPCK(h, hipEventCreate(&r.e0)); HIPCK(h, hipEventCreate(&r.e1));
    for (int rep = 0; rep < 3; ++rep) HIPCK(h, launch_mfma_probe(iters, blocks, r.stamps, r.sink, st));   // warm the clock
    HIPCK(h, hipEventRecord(r.e0, st));
    HIPCK(h, launch_mfma_probe(iters, blocks, r.stamps, r.sink, st));
    HIPCK(h, hipEventRecord(r.e1, st));
    HIPCK(h, hipEventSynchronize(r.e1));
    float ms = 0.f;
    HIPCK(h, hipEventElapsedTime(&ms, r.e0, r.e1));
    std::vector<unsigned long long> sv((size_t)blocks * 4);
    HIPCK(h, hipMemcpy(sv.data(), r.stamps, sv.size() * 8, hipMemcpyDeviceToHost));
    // shader clock = s_memtime ticks per s_memrealtime tick, the latter taken as the constant 100 MHz reference counter of gfx9
    // (consistent with the hipEvent rate of the same launch: 152 TFLOP/s measured, 2.384 GHz x 65,536 FLOP/clk = 156)
    double ghz = 0;
    for (int b = 0; b < blocks; ++b) ghz += (double)(sv[b * 4 + 1] - sv[b * 4 + 0]) / ((double)(sv[b * 4 + 3] - sv[b * 4 + 2]) * 10.0);
    // 4 waves x 16 MFMAs of 32x32x2 (4096 FLOP each) per iteration and block
    *tflops = (double)blocks * 4.0 * iters * 16.0 * 4096.0 / ((double)ms * 1e-3) / 1e12;
    if (clock_ghz) *clock_ghz = ghz / blocks;
    return FFR_OK;
}

int ffr_profile_enable(ffr_handle* h, int on) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    h->prof = on != 0;
    return FFR_OK;
}

int ffr_profile_read(ffr_handle* h, ffr_kclass_stat* out) {
    if (!h || !out) return fail(h, FFR_ERR_ARG, "ffr_profile_read: bad arguments");
    for (int i = 0; i < FFR_KC_COUNT; ++i) out[i] = ffr_kclass_stat{0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (auto& r : h->prof_log) {
        HIPCK(h, hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIPCK(h, hipEventElapsedTime(&ms, r.e0, r.e1));
        out[r.kc].launches += 1;
        // second-stream work (the few images split off a fused Winograd launch) overlaps a main-stream launch whose time is
        // already counted: neither its time nor its work enters the per-class figures, so every TFLOP/s and TB/s derived
        // from them divides work by the time that work took
        if (!r.side) {
            out[r.kc].ms += ms;
            out[r.kc].flops += r.flops;
            out[r.kc].bytes += r.bytes;
            out[r.kc].flops_executed += r.fexec;
            out[r.kc].flops_useful += r.fuse;
        }
        h->ev_pool.push_back(r.e0);
        h->ev_pool.push_back(r.e1);
    }
    h->prof_log.clear();
    return FFR_OK;
}

int ffr_op_conv(ffr_handle* h, const ffr_conv_desc* d, void* stream) {
    if (!d) return fail(h, FFR_ERR_ARG, "desc is null");
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, d->N));
    if (!d->x || !d->w || !d->bias || !d->out) return fail(h, FFR_ERR_ARG, "ffr_op_conv: null tensor");
    if (d->cin_pad % 32 || d->cout_pad % 64 || d->cin_pad <= 0) return fail(h, FFR_ERR_ARG, "ffr_op_conv: bad padding");
    Work w;
    RC(ensure_arena(h, d->N > 8 ? d->N : 8, 112, 112, &w));
    ConvW L;
    L.cin = L.cin_pad = d->cin_pad; L.cout = d->cout_store; L.cout_pad = d->cout_pad; L.R = d->R; L.S = d->S;
    L.stride = d->stride; L.pad = d->pad; L.pad_mode = d->pad_mode; L.border = d->border_bias;
    L.w = (float*)d->w; L.bias = (float*)d->bias; L.slope = (float*)d->slope;
    // flags bit1 (tests): the split-operand form of k_igemm on a device-side split of d->w (synchronises; not for captures)
    struct Planes { void* p = nullptr; ~Planes() { if (p) hipFree(p); } } planes;
    if (d->flags & 2) {
        if (!h->opt.igemm_split) return fail(h, FFR_ERR_STATE, "ffr_op_conv: flags bit1 asks for the split form, but option igemm_split is 0");
        const size_t nw = (size_t)d->cout_pad * d->R * d->S * d->cin_pad;
        HIPCK(h, hipMalloc(&planes.p, nw * 3 * sizeof(unsigned short)));
        HIPCK(h, launch_split_weights(d->w, (unsigned short*)planes.p, nw, (hipStream_t)stream));
        L.w3 = (unsigned short*)planes.p;
    }
    ConvCall c = conv_call(w);
    c.x = d->x; c.N = d->N; c.H = d->H; c.W = d->W; c.in_pitch = d->in_pitch; c.resid = d->resid; c.res_pitch = d->res_pitch;
    c.out = d->out; c.out_pitch = d->out_pitch; c.out_coff = d->out_coff; c.cout_store = d->cout_store; c.flags = d->flags & 1;
    c.tile = d->tile;
    const int rc = run_conv(h, L, c, (hipStream_t)stream);
    if (planes.p) hipStreamSynchronize((hipStream_t)stream);       // the planes are released on return
    return rc;
}

int ffr_op_conv3x3(ffr_handle* h, const float* x, int N, int H, int W, int cin, const float* w_host,
                   const float* bias_host, const float* slope_host, int cout, int pad_mode, int use_wino,
                   const float* resid, float* out, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, N));
    if (!x || !w_host || !bias_host || !out || cin % 32 || cout % 4 || cin <= 0 || cout <= 0)
        return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3: bad arguments (cin %% 32, cout %% 4)");
    if (use_wino < 0 || use_wino > 5) return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3: use_wino must be 0..5");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, N > 8 ? N : 8, 112, 112, &w));
    std::vector<void*> own;
    BNFold ob;
    ob.s.assign(cout, 1.0);
    ob.t.assign(bias_host, bias_host + cout);
    ConvW L;
    int rc = pack_conv(h, own, w_host, cout, cin, 3, 3, nullptr, &ob, slope_host, 1, 1, pad_mode, &L);
    if (rc == FFR_OK && use_wino && !L.wu) rc = fail(h, FFR_ERR_UNSUPPORTED, "layer not eligible for the Winograd path (cin < FFR_WINO_MINCIN)");
    if (rc == FFR_OK && use_wino == 5 && !L.wu3)
        rc = fail(h, FFR_ERR_UNSUPPORTED, "the split-operand fused form needs cin <= wf_phased_maxk (%d) and room for its weight planes", h->opt.wf_phased_maxk);
    if (rc == FFR_OK && use_wino == 4) {
        if (!wino_mixed_eligible(h, L, N, H, W, cin, w.wino_cap, ConvForce::Mixed)) rc = fail(h, FFR_ERR_UNSUPPORTED, "layer / map not eligible for the mixed-tile path");
        else rc = ensure_mixed_weights(h, L, own, true);
    }
    if (rc == FFR_OK) {
        ConvCall c = conv_call(w, (ConvForce)use_wino);
        c.x = x; c.N = N; c.H = H; c.W = W; c.in_pitch = cin; c.resid = resid; c.res_pitch = cout;
        c.out = out; c.out_pitch = cout; c.out_coff = 0; c.cout_store = cout;
        // a Winograd form whose scratch the workspace does not hold comes back direct from the planner: an error here, before any launch
        const ConvPlan p = plan_conv(h, L, c);
        if (use_wino && !p.refused && p.path == ConvPlan::Direct) rc = fail(h, FFR_ERR_NOMEM, "Winograd scratch too small for this test shape");
        else rc = run_conv(h, L, c, p, st);
    }
    hipStreamSynchronize(st);      // the packed weights die with this call
    free_list(own);
    return rc;
}

int ffr_op_conv3x3_ex(ffr_handle* h, const ffr_conv3x3_desc* d, void* stream) {
    if (!d) return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3_ex: desc is null");
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, d->N));
    const int cin = d->cin, cout = d->cout;
    if (!d->x || !d->w_host || !d->bias_host || !d->out || cin <= 0 || cin % 32 || cout <= 0 || d->H <= 0 || d->W <= 0 || d->N > 700)
        return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3_ex: bad arguments (null tensor, cin %% 32, N <= 700)");
    if (d->use_wino < -1 || d->use_wino > 5) return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3_ex: use_wino must be -1..5");
    if (!d->in_scale_host != !d->in_shift_host || (d->in_scale_host && d->pad_mode != 0))
        return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3_ex: in_scale and in_shift come together, with zero padding");
    const int in_pitch = d->in_pitch ? d->in_pitch : cin, out_pitch = d->out_pitch ? d->out_pitch : cout;
    const int res_pitch = d->res_pitch ? d->res_pitch : cout, cout_store = d->cout_store ? d->cout_store : cout;
    if (in_pitch < cin || in_pitch % 4 || cout_store < 1 || cout_store > cout || d->out_coff < 0 || d->out_coff + cout_store > out_pitch ||
        (d->resid && res_pitch < cout_store) || (d->pad_mode != 0 && d->pad_mode != 1))
        return fail(h, FFR_ERR_ARG, "ffr_op_conv3x3_ex: bad pitches (in_pitch >= cin and %% 4, out_coff + cout_store <= out_pitch, res_pitch >= cout_store)");
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, d->N > 8 ? d->N : 8, 112, 112, &w));
    std::vector<void*> own;
    BNFold ob, ib;
    ob.s.assign(cout, 1.0);
    ob.t.assign(d->bias_host, d->bias_host + cout);
    if (d->in_scale_host) { ib.s.assign(d->in_scale_host, d->in_scale_host + cin); ib.t.assign(d->in_shift_host, d->in_shift_host + cin); }
    ConvW L;
    const ConvForce force = (ConvForce)d->use_wino;
    int rc = pack_conv(h, own, d->w_host, cout, cin, 3, 3, d->in_scale_host ? &ib : nullptr, &ob, d->slope_host, 1, 1, d->pad_mode, &L);
    if (rc == FFR_OK && force != ConvForce::Direct && !L.wu) rc = fail(h, FFR_ERR_UNSUPPORTED, "layer not eligible for the Winograd path (cin < FFR_WINO_MINCIN)");
    if (rc == FFR_OK && force == ConvForce::FusedSplit && !L.wu3)
        rc = fail(h, FFR_ERR_UNSUPPORTED, "the split-operand fused form needs cin <= wf_phased_maxk (%d) and room for its weight planes", h->opt.wf_phased_maxk);
    if (rc == FFR_OK && force == ConvForce::Mixed) {
        if (((out_pitch | d->out_coff | res_pitch | cout_store) & 3) != 0) rc = fail(h, FFR_ERR_UNSUPPORTED, "the mixed-tile path stores whole channel quads: out_pitch, out_coff, res_pitch and cout_store must be multiples of 4");
        else if (!wino_mixed_eligible(h, L, d->N, d->H, d->W, in_pitch, w.wino_cap, ConvForce::Mixed)) rc = fail(h, FFR_ERR_UNSUPPORTED, "layer / map not eligible for the mixed-tile path");
        else rc = ensure_mixed_weights(h, L, own, true);
    }
    if (rc == FFR_OK) {
        ConvCall c = conv_call(w, force);
        c.x = d->x; c.N = d->N; c.H = d->H; c.W = d->W; c.in_pitch = in_pitch; c.resid = d->resid; c.res_pitch = res_pitch;
        c.out = d->out; c.out_pitch = out_pitch; c.out_coff = d->out_coff; c.cout_store = cout_store; c.flags = d->flags & 1;
        c.tile_sums = d->tile_sums;
        // the form that was asked for runs, or the call fails: the planner's fall-backs (a scratch that is too small sends a
        // Winograd convolution to the direct kernel) are the product's, not this hook's
        const ConvPlan p = plan_conv(h, L, c);
        const ConvPlan::Path want = force == ConvForce::Direct ? ConvPlan::Direct : force == ConvForce::Mixed ? ConvPlan::Mixed
                                  : force == ConvForce::Unfused ? ConvPlan::Unfused : ConvPlan::Fused;
        if (p.refused) rc = fail(h, FFR_ERR_STATE, "%s", p.refused);
        else if (force == ConvForce::Auto ? p.path == ConvPlan::Direct : p.path != want)
            rc = fail(h, FFR_ERR_UNSUPPORTED, "ffr_op_conv3x3_ex: the planner cannot run this descriptor in the form asked for (Winograd scratch too small for the shape?)");
        else if (c.tile_sums && p.path == ConvPlan::Direct) rc = fail(h, FFR_ERR_UNSUPPORTED, "tile_sums come from the Winograd paths only");
        else rc = run_conv(h, L, c, p, st);
    }
    hipStreamSynchronize(st);      // the packed weights die with this call
    if (h->side) hipStreamSynchronize(h->side);
    free_list(own);
    return rc;
}

int ffr_conv_plan_record(ffr_handle* h, int on) {
    if (!h) return fail(nullptr, FFR_ERR_ARG, "null handle");
    h->conv_rec = on != 0;
    if (on) h->conv_log.clear();
    return FFR_OK;
}

int ffr_conv_plan_read(ffr_handle* h, ffr_conv_launch* out, int cap, int* n) {
    if (!h || !n || cap < 0 || (cap > 0 && !out)) return fail(h, FFR_ERR_ARG, "ffr_conv_plan_read: bad arguments");
    *n = (int)h->conv_log.size();
    for (int i = 0; i < *n && i < cap; ++i) out[i] = h->conv_log[i];
    return FFR_OK;
}

int ffr_plan_igemm_host(long long M, int cout_pad, int nkt, int nbatch, int force_tile, int min_units, int split, int count,
                        int* tile, int* nblocks, int* granule) {
    if (M < 1 || cout_pad < 64 || cout_pad % 64 || nkt < 1 || nbatch < 1 || min_units < 1 || count < 1 || !tile || !nblocks || !granule ||
        force_tile < 0 || force_tile > IGEMM_NTILES)
        return FFR_ERR_ARG;
    if (force_tile) {
        int bm, bn;
        igemm_tile_shape(force_tile, &bm, &bn);
        if (cout_pad % bn) return FFR_ERR_ARG;
    }
    for (int i = 0; i < count; ++i) plan_igemm(M + i, cout_pad, nkt, nbatch, force_tile, min_units, &tile[i], &nblocks[i], &granule[i], split != 0);
    return FFR_OK;
}

int ffr_plan_conv_host(int cin, int cout, int R, int stride, int pad, int pad_mode, int has_wino, int has_wu3, int has_w3,
                       int has_mixed, int N, int H, int W, int in_pitch, int out_pitch, int out_coff, int cout_store,
                       int res_pitch, int num_cus, int force, long long* out) {
    if (cin < 1 || cout < 1 || R < 1 || stride < 1 || pad < 0 || N < 1 || H < 1 || W < 1 || num_cus < 1 || force < -1 || force > 5 || !out)
        return FFR_ERR_ARG;
    static float mark[16];          // presence flags: the planner compares and tests the weight pointers, it never reads through them
    ffr_handle fh;
    fh.num_cus = num_cus;
    fh.side = (hipStream_t)(void*)&mark[15];
    ConvW L;
    L.cin = cin; L.cin_pad = round_up(cin, 32); L.cout = cout; L.cout_pad = round_up(cout, 64);
    L.R = R; L.S = R; L.stride = stride; L.pad = pad; L.pad_mode = pad_mode;
    L.w = &mark[0];
    if (has_wino) { L.wu = &mark[1]; L.wuc = &mark[2]; }
    if (has_wu3) L.wu3 = (unsigned short*)&mark[3];
    if (has_w3) L.w3 = (unsigned short*)&mark[4];
    if (has_mixed) { L.wum[0] = L.wuc; L.wum[1] = &mark[5]; L.wum[2] = &mark[6]; L.wum[3] = &mark[7]; }
    const int Na = N > 8 ? N : 8;
    Work w = layout(fh.opt, nullptr, Na, 112, 112);
    w.tickets_cap = (size_t)Na * 112 * 112 / 64 + 4096;
    w.winoV = &mark[8]; w.winoM = &mark[9];
    ConvCall c = conv_call(w, (ConvForce)force);
    c.N = N; c.H = H; c.W = W; c.in_pitch = in_pitch ? in_pitch : L.cin_pad; c.out_pitch = out_pitch ? out_pitch : L.cout_pad;
    c.out_coff = out_coff; c.cout_store = cout_store ? cout_store : cout; c.res_pitch = res_pitch ? res_pitch : L.cout_pad;
    for (int i = 0; i < 24; ++i) out[i] = 0;
    const ConvPlan p = plan_conv(&fh, L, c);
    out[0] = p.path == ConvPlan::Direct ? 0 : p.path == ConvPlan::Mixed ? 1 : p.path == ConvPlan::Fused ? 2 : 3;
    out[1] = p.half_n; out[2] = p.phased; out[3] = p.split; out[4] = p.n_main; out[5] = p.side != nullptr; out[6] = p.takes_v;
    out[7] = p.refused != nullptr;
    out[8] = ((H + 3) / 4) * ((W + 3) / 4);
    // the plan's launching entries (a tail split's header is skipped): kind, fits, tile, nblocks, and for k_igemm granule, cut
    for (int i = p.n_launch == 3 ? 1 : 0; i < p.n_launch; ++i) {
        const ConvLaunch& e = p.launch[i];
        const ffr_conv_launch& r = e.rec;
        const bool igemm = r.path == FFR_CP_DIRECT || r.path == FFR_CP_UNFUSED_IGEMM;
        long long* o = out + (e.n0 ? 15 : 9);
        o[0] = igemm ? 1 : r.path == FFR_CP_FUSED ? 2 : r.path == FFR_CP_UNFUSED_STREAM ? 3 : 4;
        o[1] = e.gemm.nomem ? 0 : 1; o[2] = r.tile; o[3] = r.nblocks;
        if (igemm) { o[4] = r.granule; o[5] = r.cut; }
    }
    return FFR_OK;
}

int ffr_plan_channel_rows_host(int N, int num_cus, int forced, int* row_blocks) {
    if (N < 1 || num_cus < 1 || !row_blocks) return FFR_ERR_ARG;
    const int rb = plan_channel_rows(N, num_cus, forced);
    if (!rb) return FFR_ERR_ARG;
    *row_blocks = rb;
    return FFR_OK;
}

int ffr_encoder_trunk_nhwc(ffr_handle* h, const float* x, int N, int H, int W, int n_blocks, float* out, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, true, false, N));
    if (!x || !out || n_blocks < 0 || n_blocks > (int)h->blocks.size()) return fail(h, FFR_ERR_ARG, "ffr_encoder_trunk_nhwc: bad arguments");
    RC(check_hw(h, H, W));
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena_encoder(h, N, H, W, &w));
    float* t; int oh, ow, oc;
    RC(run_trunk(h, w, x, N, H, W, n_blocks, st, &t, &oh, &ow, &oc));
    HIPCK(h, hipMemcpyAsync(out, t, (size_t)N * oh * ow * oc * sizeof(float), hipMemcpyDeviceToDevice, st));
    return FFR_OK;
}

int ffr_recnet_debug(ffr_handle* h, const float* featmap_nchw, int N, float* ss_space, float* M_space, float* feat_space,
                     float* feat_channel_raw, float* feat_channel, float* ss_channel0, float* M_channel0, int image, void* stream) {
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, true, N));
    if (!featmap_nchw) return fail(h, FFR_ERR_ARG, "featmap is null");
    if (image < 0 || image >= N) return fail(h, FFR_ERR_ARG, "ffr_recnet_debug: image %d is outside [0, %d)", image, N);
    hipStream_t st = (hipStream_t)stream;
    Work w;
    RC(ensure_arena(h, N, 112, 112, &w));
    RC(featmap_to_x(h, w, featmap_nchw, N, st));
    RecDebug d{ss_space, M_space, feat_space, feat_channel_raw, feat_channel, ss_channel0, M_channel0, image};
    return run_recnet(h, w, N, nullptr, &d, st);
}

}  // extern "C"
