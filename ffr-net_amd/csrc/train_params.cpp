// RecNet training step -- the parameter store: one flat buffer each for the parameters, their gradients and Adam's two
// moments in the kernel layouts, the state_dict view of them, the gradient buckets, the optimiser.
//   clip_grad_value_(1.0) + Adam                models/trainer.py:115-121,182-187
#include "train_internal.h"

namespace ffr_eng {

namespace {

const int LIN_IDX[6] = {0, 2, 3, 5, 6, 8};
const int LIN_IN[6] = {561, 32, 512, 32, 512, 32}, LIN_OUT[6] = {32, 512, 32, 512, 32, 512};
const int ACT_IDX[3] = {1, 4, 7};

size_t add_seg(TrainState* t, const std::string& key, SegKind kind, int d0, int d1, int p0, int p1, int colperm = 0) {
    Seg s;
    s.key = key; s.kind = kind; s.d0 = d0; s.d1 = d1; s.p0 = p0; s.p1 = p1; s.colperm = colperm;
    s.n_natural = kind == SEG_CONV ? (size_t)d0 * d1 * 9 : (size_t)d0 * d1;
    s.n_native = kind == SEG_CONV ? (size_t)p0 * 9 * p1 : (size_t)p0 * p1;
    s.off = t->n_flat;
    t->n_flat += (s.n_native + 63) / 64 * 64;
    t->seg_of[key] = (int)t->segs.size();
    t->segs.push_back(s);
    return s.off;
}

// One state_dict entry of buffer `which` (0 parameters, 1 gradients, 2 / 3 Adam's moments; 4, where `running` allows it, the
// BatchNorm running statistics): seg null for a running statistic.  n: the caller's element count, checked unless null.
struct ParamRef { const Seg* seg = nullptr; float* base = nullptr; size_t n = 0; };
int find_param(ffr_handle* h, TrainState* t, const char* who, int which, const char* key, const size_t* n, bool running, ParamRef* r) {
    if (running && which == 4) {
        auto it = t->running_of.find(key);
        if (it == t->running_of.end()) return fail(h, FFR_ERR_KEY, "no running statistic '%s'", key);
        r->base = it->second.first; r->n = it->second.second;
    } else {
        auto it = t->seg_of.find(key);
        if (it == t->seg_of.end()) return fail(h, FFR_ERR_KEY, "no parameter '%s'", key);
        r->seg = &t->segs[it->second]; r->n = r->seg->n_natural;
    }
    if (n && *n != r->n) return fail(h, FFR_ERR_ARG, "'%s' has %zu elements, not %zu", key, r->n, *n);
    if (!r->seg) return FFR_OK;
    float* const bufs[4] = {t->P, t->Gr, t->M1, t->M2};
    if (which < 0 || which > 3) return fail(h, FFR_ERR_ARG, "%s: which must be 0..%d", who, running ? 4 : 3);
    r->base = bufs[which] + r->seg->off;
    return FFR_OK;
}

}  // namespace

int dev_alloc(ffr_handle* h, std::vector<void*>& owner, size_t floats, float** out) {
    void* p = nullptr;
    if (hipMalloc(&p, floats ? floats * 4 : 256) != hipSuccess) return fail(h, FFR_ERR_NOMEM, "hipMalloc of %zu bytes failed", floats * 4);
    owner.push_back(p);
    *out = (float*)p;
    return FFR_OK;
}

int get_train(ffr_handle* h, TrainState** t) {
    RC(check_fwd(h, false, false, 1));      // the handle, on its device
    if (!h->train) return fail(h, FFR_ERR_STATE, "ffr_train_init has not been called");
    *t = h->train;
    return FFR_OK;
}

void train_free(ffr_handle* h) {
    if (!h || !h->train) return;
    hipDeviceSynchronize();
    free_graph(h->train);
    for (auto& e : h->train->bucket_ev) if (e) hipEventDestroy(e);
    free_list(h->train->allocs);
    delete h->train;
    h->train = nullptr;
}

}  // namespace ffr_eng

using namespace ffr_eng;

extern "C" {

int ffr_train_init(ffr_handle* h, const ffr_tensor_desc* td, int n) {
    if (!h || !td || n <= 0) return fail(h, FFR_ERR_ARG, "ffr_train_init: bad arguments");
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    train_free(h);
    ++h->generation;
    TrainState* t = new TrainState();
    h->train = t;
    SD sd; sd.h = h;
    for (int i = 0; i < n; ++i) if (td[i].name) sd.m[td[i].name] = &td[i];
    // ---- layout of the flat parameter buffer --------------------------------------------------
    size_t running_floats = 0;
    for (int i = 0; i < 15; ++i) {
        if (i == 0 || i == 9 || i == 12) t->bucket_off[i / 6] = t->n_flat;      // Conv4Space | ChannelFlipMerge | Conv4Merge
        TLayer& L = train_layer(t, i);
        const std::string p = L.name = REC_LAYERS[i].prefix;
        L.cin = REC_LAYERS[i].cin; L.cout = REC_LAYERS[i].cout; L.cin_pad = round_up(L.cin, 32); L.cout_pad = round_up(L.cout, 64);
        L.dgrad_width = L.cin_pad;      // the padded channels too: the layer before reads them as (zero) gradients
        add_seg(t, p + ".conv2d.weight", SEG_CONV, L.cout, L.cin, L.cout_pad, L.cin_pad);
        add_seg(t, p + ".relu.func.weight", SEG_VEC, L.cout, 1, L.cout_pad, 1);
        add_seg(t, p + ".norm.norm.weight", SEG_VEC, L.cout, 1, L.cout_pad, 1);
        add_seg(t, p + ".norm.norm.bias", SEG_VEC, L.cout, 1, L.cout_pad, 1);
        running_floats += (size_t)2 * L.cout_pad;
    }
    // the two layers that read the network's input X: Conv4Space.0 nothing else (no data gradient), Conv4Merge.0 as the last 512
    // channels of [feat_space | feat_channel | X]
    t->sp[0].dgrad_width = 0; t->mg[0].dgrad_width = 1024;
    t->bucket_off[3] = t->n_flat;
    for (int i = 0; i < 6; ++i) {
        Lin& l = t->lin[i];
        l.in = LIN_IN[i]; l.out = LIN_OUT[i]; l.in_pad = round_up(l.in, 32); l.out_pad = round_up(l.out, 64);
        const std::string p = l.name = "Conv4Channel." + std::to_string(LIN_IDX[i]);
        add_seg(t, p + ".weight", SEG_LIN, l.out, l.in, l.out_pad, l.in_pad, i == 0 ? 1 : 0);
        add_seg(t, p + ".bias", SEG_VEC, l.out, 1, l.out_pad, 1);
    }
    for (int i = 0; i < 3; ++i) add_seg(t, "Conv4Channel." + std::to_string(ACT_IDX[i]) + ".func.weight", SEG_VEC, 512, 1, 512, 1);
    t->bucket_off[4] = t->n_flat;
    add_seg(t, "classifier.weight", SEG_LIN, N_CLASSES, 512, CLS_PAD, 512);
    t->bucket_off[5] = t->n_flat;
    for (auto& e : t->bucket_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(h, FFR_ERR_HIP, "hipEventCreate failed");
    // ---- device buffers ---------------------------------------------------------------------------
    for (float** b : {&t->P, &t->Gr, &t->M1, &t->M2}) RC(dev_alloc(h, t->allocs, t->n_flat, b));
    RC(dev_alloc(h, t->allocs, running_floats, &t->running));
    for (float* b : {t->Gr, t->M1, t->M2}) HIPCK(h, hipMemset(b, 0, t->n_flat * 4));
    // ---- parameters: natural layout (host) -> native layout ------------------------------------------
    std::vector<float> flat(t->n_flat, 0.f);
    for (const Seg& sg : t->segs) {
        const float* src = nullptr;
        if (sg.kind == SEG_CONV) src = sd.get(sg.key, {sg.d0, sg.d1, 3, 3});
        else if (sg.kind == SEG_VEC) src = sd.get(sg.key, {sg.d0});
        else src = sd.get(sg.key, {sg.d0, sg.d1});
        if (!src) return sd.rc;
        for (size_t i = 0; i < sg.n_natural; ++i) flat[sg.off + sg.native_index(i)] = src[i];
    }
    HIPCK(h, hipMemcpy(t->P, flat.data(), t->n_flat * 4, hipMemcpyHostToDevice));
    std::vector<float> run(running_floats, 0.f);
    size_t roff = 0;
    // an entry's parameter and its gradient
    auto bind = [&](const std::string& k, float*& p, float*& g) { const size_t o = t->segs[t->seg_of[k]].off; p = t->P + o; g = t->Gr + o; };
    for (int i = 0; i < 15; ++i) {
        TLayer& L = train_layer(t, i);
        const std::string p = L.name;
        bind(p + ".conv2d.weight", L.w, L.gw); bind(p + ".relu.func.weight", L.slope, L.gslope);
        bind(p + ".norm.norm.weight", L.gamma, L.ggamma); bind(p + ".norm.norm.bias", L.beta, L.gbeta);
        const float* rm = sd.get(p + ".norm.norm.running_mean", {L.cout});
        const float* rv = sd.get(p + ".norm.norm.running_var", {L.cout});
        if (!rm || !rv) return sd.rc;
        L.rmean = t->running + roff; L.rvar = t->running + roff + L.cout_pad;
        for (int c = 0; c < L.cout; ++c) { run[roff + c] = rm[c]; run[roff + L.cout_pad + c] = rv[c]; }
        t->running_of[p + ".norm.norm.running_mean"] = {L.rmean, L.cout};
        t->running_of[p + ".norm.norm.running_var"] = {L.rvar, L.cout};
        roff += (size_t)2 * L.cout_pad;
    }
    HIPCK(h, hipMemcpy(t->running, run.data(), running_floats * 4, hipMemcpyHostToDevice));
    for (Lin& l : t->lin) { bind(l.name + ".weight", l.w, l.gw); bind(l.name + ".bias", l.b, l.gb); }
    for (int i = 0; i < 3; ++i) bind("Conv4Channel." + std::to_string(ACT_IDX[i]) + ".func.weight", t->a[i], t->ga[i]);
    bind("classifier.weight", t->clsW, t->gclsW);
    t->adam_step = 0;
    t->nbt = 0;
    return FFR_OK;
}

int ffr_train_info(ffr_handle* h, float** params, float** grads, size_t* n_flat, long long* num_batches_tracked,
                   int* adam_step) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (params) *params = t->P;
    if (grads) *grads = t->Gr;
    if (n_flat) *n_flat = t->n_flat;
    if (num_batches_tracked) *num_batches_tracked = t->nbt;
    if (adam_step) *adam_step = t->adam_step;
    return FFR_OK;
}

// one entry between the host (torch layout) and the device (kernel layout); the running statistics can only be read
static int train_host_copy(ffr_handle* h, const char* who, int which, const char* key, float* host, size_t n, bool set) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (!key || !host) return fail(h, FFR_ERR_ARG, "%s: null argument", who);
    HIPCK(h, hipDeviceSynchronize());
    ParamRef r;
    RC(find_param(h, t, who, which, key, &n, !set, &r));
    if (!r.seg) { HIPCK(h, hipMemcpy(host, r.base, n * 4, hipMemcpyDeviceToHost)); return FFR_OK; }
    std::vector<float> nat(r.seg->n_native, 0.f);
    if (set) for (size_t i = 0; i < n; ++i) nat[r.seg->native_index(i)] = host[i];
    HIPCK(h, hipMemcpy(set ? r.base : nat.data(), set ? nat.data() : r.base, r.seg->n_native * 4, set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    if (!set) for (size_t i = 0; i < n; ++i) host[i] = nat[r.seg->native_index(i)];
    return FFR_OK;
}

int ffr_train_get(ffr_handle* h, int which, const char* key, float* host_out, size_t n) {
    return train_host_copy(h, "ffr_train_get", which, key, host_out, n, false);
}

int ffr_train_set(ffr_handle* h, int which, const char* key, const float* host_in, size_t n) {
    return train_host_copy(h, "ffr_train_set", which, key, const_cast<float*>(host_in), n, true);
}

// device-to-device conversion of one entry: dir 0 = export (kernel layout -> torch layout), 1 = import
static int train_convert(ffr_handle* h, int which, const char* key, float* dev, int dir, void* stream) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (!key || !dev) return fail(h, FFR_ERR_ARG, "ffr_train_export/import: null argument");
    hipStream_t st = (hipStream_t)stream;
    ParamRef r;
    RC(find_param(h, t, "ffr_train_export/import", which, key, nullptr, true, &r));
    if (!r.seg) { HIPCK(h, hipMemcpyAsync(dir ? r.base : dev, dir ? dev : r.base, r.n * 4, hipMemcpyDeviceToDevice, st)); return FFR_OK; }
    const Seg& sg = *r.seg;
    HIPCK(h, launch_seg_convert(r.base, dev, sg.n_natural, sg.kind == SEG_CONV ? 0 : sg.kind == SEG_VEC ? 1 : 2, sg.d1, sg.p1, sg.colperm, dir, st));
    return FFR_OK;
}

int ffr_train_export(ffr_handle* h, int which, const char* key, float* dev_out, void* stream) {
    return train_convert(h, which, key, dev_out, 0, stream);
}

int ffr_train_import(ffr_handle* h, int which, const char* key, const float* dev_in, void* stream) {
    return train_convert(h, which, key, const_cast<float*>(dev_in), 1, stream);
}

int ffr_train_zero_grad(ffr_handle* h, void* stream) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    { hipStream_t st = (hipStream_t)stream; Scope _ps(h, st, FFR_KC_TRAIN_OPTIM, 0.0, 4.0 * t->n_flat); HIPCK(h, hipMemsetAsync(t->Gr, 0, t->n_flat * 4, st)); }
    return FFR_OK;
}

int ffr_train_adam_step(ffr_handle* h, double lr, double beta1, double beta2, double eps, double weight_decay,
                        double clip_value, void* stream) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    t->adam_step += 1;
    hipStream_t st = (hipStream_t)stream;
    TLAUNCH(FFR_KC_TRAIN_OPTIM, launch_adam(t->P, t->Gr, t->M1, t->M2, t->n_flat, lr, beta1, beta2, eps, weight_decay,
                         clip_value > 0.0 ? (float)clip_value : 3.0e38f, t->adam_step, (hipStream_t)stream));
    return FFR_OK;
}

// Gradient buckets for overlapping the data-parallel exchange with the backward: bucket i is the range
// [offsets[i], offsets[i+1]) of the flat gradient buffer; order[k] is the k-th bucket the backward completes.
int ffr_train_buckets(ffr_handle* h, int* n, size_t* offsets, int* order) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (n) *n = TrainState::NBUCKET;
    if (offsets) for (int i = 0; i <= TrainState::NBUCKET; ++i) offsets[i] = t->bucket_off[i];
    static const int ORDER[TrainState::NBUCKET] = {4, 2, 1, 3, 0};
    if (order) for (int i = 0; i < TrainState::NBUCKET; ++i) order[i] = ORDER[i];
    return FFR_OK;
}

// Makes `stream` wait until the last recorded backward has finished bucket i (hipStreamWaitEvent; no host sync).
int ffr_train_bucket_wait(ffr_handle* h, int i, void* stream) {
    TrainState* t;
    FFR_DEVICE_SCOPE(h); RC(get_train(h, &t));
    if (i < 0 || i >= TrainState::NBUCKET) return fail(h, FFR_ERR_ARG, "ffr_train_bucket_wait: bad bucket");
    HIPCK(h, hipStreamWaitEvent((hipStream_t)stream, t->bucket_ev[i], 0));
    return FFR_OK;
}

}  // extern "C"
