// libffrnet_hip.so: the weight packer -- ffr_load_encoder / ffr_load_recnet fold the BatchNorms (and the border-class biases)
// into the convolution weights and lay them out for the kernels: direct, Winograd U, the K-chunk order of k_wino_fused; the
// exact-tiling weight sets are derived on the device when a launch first needs them.  Host code only.
#include "device_util.h"
#include "engine_internal.h"

using namespace ffr_eng;

namespace ffr_eng {

const double BN_EPS = 1e-5;

// ---- host-side state_dict access -----------------------------------------------------------

bool bn_fold(SD& sd, const std::string& p, int C, BNFold& o) {
    const float* g = sd.get(p + ".weight", {C});
    const float* b = sd.get(p + ".bias", {C});
    const float* mu = sd.get(p + ".running_mean", {C});
    const float* var = sd.get(p + ".running_var", {C});
    if (!g || !b || !mu || !var) return false;
    o.s.resize(C); o.t.resize(C);
    for (int c = 0; c < C; ++c) {
        o.s[c] = (double)g[c] / std::sqrt((double)var[c] + BN_EPS);
        o.t[c] = (double)b[c] - (double)mu[c] * o.s[c];
    }
    return true;
}

int upload(ffr_handle* h, std::vector<void*>& owner, const std::vector<float>& v, float** out) {
    void* p = nullptr;
    if (hipMalloc(&p, v.size() * sizeof(float)) != hipSuccess)
        return fail(h, FFR_ERR_NOMEM, "hipMalloc of %zu weight bytes failed", v.size() * sizeof(float));
    owner.push_back(p);
    if (h && &owner == &h->enc_allocs) h->enc_weight_bytes += v.size() * sizeof(float);
    if (h && &owner == &h->rec_allocs) h->rec_weight_bytes += v.size() * sizeof(float);
    HIPCK(h, hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = (float*)p;
    return FFR_OK;
}

// bf16 (round to nearest even) of a double, as the value it represents; exact in float
static double round_bf16(double d) {
    if (d == 0.0 || !std::isfinite(d)) return d;
    if (std::fabs(d) >= 1.2e-38) {                       // normal range: round the double's significand to 8 bits in place
        unsigned long long u;
        memcpy(&u, &d, 8);
        u += 0x00000fffffffffffull + ((u >> 45) & 1);
        u &= ~((1ull << 45) - 1);
        memcpy(&d, &u, 8);
        return d;
    }
    int e;
    std::frexp(d, &e);                                   // |d| = m * 2^e, m in [0.5, 1)
    int q = e - 8;                                       // 8 significand bits
    if (q < -133) q = -133;                              // bf16 subnormals
    return std::nearbyint(std::ldexp(d, -q)) * std::ldexp(1.0, q);     // default rounding mode: ties to even
}

// The three bf16 planes [3][n] of the double-precision weights wd[n] for k_igemm's split-operand form: p1 = bf16(w),
// p2 = bf16(w - p1), p3 = bf16(w - p1 - p2) -- together they carry more of the fold than its fp32 rounding did.
// An optimisation: when the device cannot hold them the layer keeps the fp32 form, logged once, not an error.
void split_bf16x3(double w, unsigned short out[3]) {
    for (int p = 0; p < 3; ++p) {
        const double b = round_bf16(w);
        const float bf = (float)b;
        unsigned u;
        memcpy(&u, &bf, 4);
        out[p] = (unsigned short)(u >> 16);
        w -= b;
    }
}

static int upload_planes(ffr_handle* h, std::vector<void*>& owner, const std::vector<unsigned short>& pl, size_t* counter, unsigned short** out);

int upload_split(ffr_handle* h, std::vector<void*>& owner, const std::vector<double>& wd, unsigned short** out) {
    const size_t n = wd.size();
    std::vector<unsigned short> pl(3 * n);
    for (size_t i = 0; i < n; ++i) {
        unsigned short q[3];
        split_bf16x3(wd[i], q);
        for (int p = 0; p < 3; ++p) pl[(size_t)p * n + i] = q[p];
    }
    return upload_planes(h, owner, pl, &h->split_weight_bytes, out);
}

// The three bf16 planes of ud = G g G^T [36][cout_pad][cin_pad] (double, BN folded) in the order k_wino_fused's split-operand
// form streams them: [cout_pad/64][16-channel K step][xi][2 halves][3 planes][64 lanes][8 bf16]; lane = 32 * (k half) + (output
// channel & 31) carries the channels 16 step + 8 (k half) + 0..7, one 16-byte load per lane and plane.
void pack_wino_split(const double* ud, int cout_pad, int cin_pad, unsigned short* pl) {
    const int nst = cin_pad / 16;
    for (int nb = 0; nb < cout_pad / 64; ++nb)
        for (int s = 0; s < nst; ++s)
            for (int xi = 0; xi < 36; ++xi)
                for (int nt = 0; nt < 2; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 8; ++i) {
                            const int co = nb * 64 + nt * 32 + (lane & 31), ci = 16 * s + 8 * (lane >> 5) + i;
                            unsigned short q[3];
                            split_bf16x3(ud[((size_t)xi * cout_pad + co) * cin_pad + ci], q);
                            const size_t base = ((((size_t)nb * nst + s) * 36 + xi) * 2 + nt) * 3;
                            for (int p = 0; p < 3; ++p) pl[((base + p) * 64 + lane) * 8 + i] = q[p];
                        }
}

// Uploads bf16 planes; *counter (a field of h) takes their bytes when they belong to the encoder.
static int upload_planes(ffr_handle* h, std::vector<void*>& owner, const std::vector<unsigned short>& pl, size_t* counter, unsigned short** out) {
    *out = nullptr;
    void* p = nullptr;
    const size_t bytes = pl.size() * sizeof(unsigned short);
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) e = hipMemcpy(p, pl.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p) hipFree(p);
        (void)hipGetLastError();
        if (!h->split_gave_up_logged) {
            h->split_gave_up_logged = true;
            fprintf(stderr, "ffrnet: no room for the split-operand weight planes (%zu bytes: %s); the layers concerned keep the fp32 kernel\n",
                    bytes, hipGetErrorString(e));
        }
        return FFR_OK;
    }
    owner.push_back(p);
    if (&owner == &h->enc_allocs) { h->enc_weight_bytes += bytes; *counter += bytes; }
    if (&owner == &h->rec_allocs) h->rec_weight_bytes += bytes;
    *out = (unsigned short*)p;
    return FFR_OK;
}

// Pack one convolution: W[cout][cin][R][S] -> [cout_pad][(r*S+s)*cin_pad + ci], with an
// optional per-input-channel affine folded in front (pre-conv BatchNorm: scale into the
// weights, shift into one bias per zero-padding border class) and an optional
// per-output-channel affine behind it (post-conv BatchNorm).
int pack_conv(ffr_handle* h, std::vector<void*>& owner, const float* W, int cout, int cin, int R, int S,
              const BNFold* in_bn, const BNFold* out_bn, const float* slope, int stride, int pad, int pad_mode,
              ConvW* L) {
    L->cin = cin; L->cout = cout; L->R = R; L->S = S; L->stride = stride; L->pad = pad; L->pad_mode = pad_mode;
    L->cin_pad = round_up(cin, 32);
    L->cout_pad = round_up(cout, 64);
    L->border = in_bn ? 1 : 0;
    const int KK = R * S * L->cin_pad;
    std::vector<float> wp((size_t)L->cout_pad * KK, 0.f);
    const int wino_min_cin = h->opt.wino_mincin;
    const bool wino = R == 3 && S == 3 && stride == 1 && pad == 1 && L->cin_pad >= wino_min_cin && wino_min_cin > 0;
    std::vector<double> wd;                      // the fold in double, for the split planes of a layer that always runs direct
    if (!wino) wd.assign(wp.size(), 0.0);
    const int ncls = L->border ? 9 : 1;
    std::vector<float> bias((size_t)ncls * L->cout_pad, 0.f);
    std::vector<double> tap(R * S);
    for (int co = 0; co < cout; ++co) {
        const double g = out_bn ? out_bn->s[co] : 1.0;
        const double b = out_bn ? out_bn->t[co] : 0.0;
        for (int r = 0; r < R; ++r)
            for (int s = 0; s < S; ++s) {
                double tsum = 0.0;
                for (int ci = 0; ci < cin; ++ci) {
                    const double wv = W[(((size_t)co * cin + ci) * R + r) * S + s];
                    const double si = in_bn ? in_bn->s[ci] : 1.0;
                    wp[(size_t)co * KK + (size_t)(r * S + s) * L->cin_pad + ci] = (float)(wv * si * g);
                    if (!wino) wd[(size_t)co * KK + (size_t)(r * S + s) * L->cin_pad + ci] = wv * si * g;
                    if (in_bn) tsum += wv * in_bn->t[ci];
                }
                tap[r * S + s] = tsum;
            }
        if (L->border) {
            // class (rc,cc): rc 0 = top row of taps out of bounds, 1 = none, 2 = bottom row; same for columns
            for (int rc = 0; rc < 3; ++rc)
                for (int cc = 0; cc < 3; ++cc) {
                    double acc = 0.0;
                    for (int r = 0; r < R; ++r) {
                        if ((rc == 0 && r == 0) || (rc == 2 && r == R - 1)) continue;
                        for (int s = 0; s < S; ++s) {
                            if ((cc == 0 && s == 0) || (cc == 2 && s == S - 1)) continue;
                            acc += tap[r * S + s];
                        }
                    }
                    bias[(size_t)(rc * 3 + cc) * L->cout_pad + co] = (float)(g * acc + b);
                }
        } else {
            bias[co] = (float)b;
        }
    }
    RC(upload(h, owner, wp, &L->w));
    RC(upload(h, owner, bias, &L->bias));
    L->w3 = nullptr;
    if (!wino) RC(upload_split(h, owner, wd, &L->w3));
    L->wu = nullptr;
    L->wuc = nullptr;
    L->wu3 = nullptr;
    for (int tau = 0; tau < 4; ++tau) L->wum[tau] = nullptr;
    L->direct = false;          // new weights: the layer's plan returns to Winograd, its calibration is void
    L->sensitivity = -1.0;
    if (wino) {
        // U[xi = i*6+j][co][ci] = (G g G^T)[i][j], same BN folds as the direct weights
        static const double G[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                       {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
        std::vector<float> wu((size_t)36 * L->cout_pad * L->cin_pad, 0.f);
        // layers whose fused launches transform their own input: the fold in double, for the planes of the split-operand K loop
        const bool split = L->cin_pad <= h->opt.wf_phased_maxk && L->cin_pad % 32 == 0;
        std::vector<double> wud;
        if (split) wud.assign(wu.size(), 0.0);
        for (int co = 0; co < cout; ++co) {
            const double g = out_bn ? out_bn->s[co] : 1.0;
            for (int ci = 0; ci < cin; ++ci) {
                const float* gk = W + ((size_t)co * cin + ci) * 9;
                const double sc = (in_bn ? in_bn->s[ci] : 1.0) * g;
                double tmp[6][3];
                for (int i = 0; i < 6; ++i)
                    for (int c = 0; c < 3; ++c) tmp[i][c] = G[i][0] * gk[0 * 3 + c] + G[i][1] * gk[1 * 3 + c] + G[i][2] * gk[2 * 3 + c];
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        const double u = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                        wu[((size_t)(i * 6 + j) * L->cout_pad + co) * L->cin_pad + ci] = (float)(u * sc);
                        if (split) wud[((size_t)(i * 6 + j) * L->cout_pad + co) * L->cin_pad + ci] = u * sc;
                    }
            }
        }
        RC(upload(h, owner, wu, &L->wu));
        // the same weights in the order k_wino_fused streams them (wino_fused.hip: 8-channel K chunks, one 16-byte MFMA
        // fragment per lane: lane = 32 * (k half) + (output channel & 31))
        const int nkc = L->cin_pad / 8, nbn = L->cout_pad / 64;
        std::vector<float> wuc(wu.size());
        for (int nb = 0; nb < nbn; ++nb)
            for (int kc = 0; kc < nkc; ++kc)
                for (int xi = 0; xi < 36; ++xi)
                    for (int nl = 0; nl < 64; ++nl)
                        for (int hf = 0; hf < 2; ++hf) {
                            const int piece = (nl >> 5) * 64 + hf * 32 + (nl & 31);      // = 64 * (32-channel half) + lane
                            float* dst = &wuc[((((size_t)nb * nkc + kc) * 36 + xi) * 128 + piece) * 4];
                            const float* src = &wu[((size_t)xi * L->cout_pad + nb * 64 + nl) * L->cin_pad + kc * 8 + 4 * hf];
                            for (int e = 0; e < 4; ++e) dst[e] = src[e];
                        }
        RC(upload(h, owner, wuc, &L->wuc));
        if (split) {
            std::vector<unsigned short> pl(wino_split_u_elems(L->cout_pad, L->cin_pad));
            pack_wino_split(wud.data(), L->cout_pad, L->cin_pad, pl.data());
            RC(upload_planes(h, owner, pl, &h->wf_split_weight_bytes, &L->wu3));
        }
    }
    L->slope = nullptr;
    if (slope) {
        std::vector<float> sl(L->cout_pad, 0.f);
        for (int co = 0; co < cout; ++co) sl[co] = slope[co];
        RC(upload(h, owner, sl, &L->slope));
    }
    return FFR_OK;
}

void free_list(std::vector<void*>& v) {
    for (void* p : v) hipFree(p);
    v.clear();
}

// get_blocks(num_layers), pretrain/model_ir_se50.py:84-105: units per stage for 50 / 100 / 152 layers
const int STAGE_CH[4][2] = {{64, 64}, {64, 128}, {128, 256}, {256, 512}};
const int UNITS[3][4] = {{3, 4, 14, 3}, {3, 13, 30, 3}, {3, 8, 36, 3}};

static bool block_table(int n_blocks, std::vector<int>& cin, std::vector<int>& depth, std::vector<int>& stride) {
    for (auto& units : UNITS) {
        if (units[0] + units[1] + units[2] + units[3] != n_blocks) continue;
        for (int s = 0; s < 4; ++s)
            for (int u = 0; u < units[s]; ++u) {
                cin.push_back(u == 0 ? STAGE_CH[s][0] : STAGE_CH[s][1]);
                depth.push_back(STAGE_CH[s][1]);
                stride.push_back(u == 0 ? 2 : 1);
            }
        return true;
    }
    return false;
}

// RecNet's ConvLayers in the order of h->sp[9] (Conv4Space, recnet.py:362-371), h->fm[3] (ChannelFlipMerge, :387-390) and
// h->mg[3] (Conv4Merge, :391-394): state_dict prefix, input and output channels.  ffr_layer_get numbers them in this order.
const RecLayer REC_LAYERS[15] = {
    {"Conv4Space.0", 561, 256}, {"Conv4Space.1.conv1", 256, 256}, {"Conv4Space.1.conv2", 256, 256}, {"Conv4Space.2", 256, 128},
    {"Conv4Space.3.conv1", 128, 128}, {"Conv4Space.3.conv2", 128, 128}, {"Conv4Space.4", 128, 49}, {"Conv4Space.5.conv1", 49, 49},
    {"Conv4Space.5.conv2", 49, 49}, {"ChannelFlipMerge.0", 1024, 512}, {"ChannelFlipMerge.1.conv1", 512, 512},
    {"ChannelFlipMerge.1.conv2", 512, 512}, {"Conv4Merge.0", 1536, 512}, {"Conv4Merge.1.conv1", 512, 512}, {"Conv4Merge.1.conv2", 512, 512}};

// The weights of the tile types (4,3), (3,4), (3,3) of one layer, derived ON THE DEVICE from its packed direct weights the first
// time a launch is eligible (round 4 packed them on the host at load time for all 27 layers, 0.7 GB per handle, whether or not
// a batch of >= 256 images ever arrived).  Synchronous (hipMalloc + three small kernels); never inside a stream capture: the
// callers run it from the encoder entry points (ensure_arena_encoder) / before the launch of an operator test.
// The sets are an OPTIMISATION: when the device cannot hold them the layer keeps running on padded F(4x4) tiles -- the failure
// is logged once, remembered per layer (wum_gave_up: no retry on every forward) and is NOT an error of the call (`strict`, the
// operator test that asks for this path by name, is the exception).
int ensure_mixed_weights(ffr_handle* h, ConvW& L, std::vector<void*>& owner, bool strict) {
    if (L.wum[1]) return FFR_OK;
    if (L.wum_gave_up && !strict) return FFR_OK;
    if (!L.wuc || !L.w) return fail(h, FFR_ERR_STATE, "mixed-tile weights asked for a layer without Winograd weights");
    float* um[4] = {L.wuc, nullptr, nullptr, nullptr};
    const auto t0 = std::chrono::steady_clock::now();
    size_t total = 0;
    for (int tau = 1; tau < 4; ++tau) {
        void* p = nullptr;
        const size_t bytes = wino_mixed_u_floats(tau, L.cout_pad, L.cin_pad) * sizeof(float);
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) {
            um[tau] = (float*)p;
            e = launch_wino_weights_mixed(L.w, um[tau], L.cout_pad, L.cin_pad, tau, nullptr);
        }
        if (e != hipSuccess) {          // nothing half-built stays behind: the layer keeps running on padded tiles
            hipDeviceSynchronize();
            for (int k = 1; k <= tau; ++k) if (um[k]) hipFree(um[k]);
            (void)hipGetLastError();    // the failed hipMalloc must not surface in the next launch wrapper
            if (strict) return fail(h, e == hipErrorOutOfMemory ? FFR_ERR_NOMEM : FFR_ERR_HIP, "mixed-tile weights (%zu bytes): %s", bytes, hipGetErrorString(e));
            L.wum_gave_up = true;
            if (!h->mixed_gave_up_logged) {
                h->mixed_gave_up_logged = true;
                fprintf(stderr, "ffrnet: no room for the exact-tiling weight sets (%zu bytes: %s); the layers concerned stay on padded F(4x4) tiles\n",
                        bytes, hipGetErrorString(e));
            }
            return FFR_OK;
        }
        total += bytes;
    }
    HIPCK(h, hipDeviceSynchronize());
    for (int tau = 1; tau < 4; ++tau) owner.push_back(um[tau]);
    if (&owner == &h->enc_allocs) { h->mixed_weight_bytes += total; h->enc_weight_bytes += total; }
    h->mixed_pack_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int tau = 0; tau < 4; ++tau) L.wum[tau] = um[tau];
    return FFR_OK;
}

// Every encoder convolution that a forward of N images of H x W would run on the exact tiling gets its weight sets now.
// Called from the ENCODER entry points only (ffr_reserve, ffr_encoder_forward, ffr_embed*, ffr_encoder_trunk_nhwc, the training
// iteration) with the real input size: the walk below maps blocks to map sizes from (H, W), which an operator call's arena
// size says nothing about.  Readiness is per layer (wum[1] / wum_gave_up), so alternating input shapes cost one walk of 48
// comparisons each and never a second derivation; (mixed_ready_*) only shortcuts the repeated same-shape forward.
// Capture: a stream capture of ffr_embed is safe once ffr_reserve (or one eager forward) ran with the same N, H, W and options.
int prepare_mixed_weights(ffr_handle* h, int N, int H, int W, size_t wino_cap) {
    if (!h->enc_loaded || !h->opt.wf_mixed || !h->opt.wino || !h->opt.wino_fused) return FFR_OK;
    if (h->mixed_ready_n >= N && h->mixed_ready_h == H && h->mixed_ready_w == W) return FFR_OK;     // the common case: one comparison per forward
    int ch = H, cw = W;
    for (Block& b : h->blocks) {
        if (wino_mixed_eligible(h, b.c1, N, ch, cw, b.cin, wino_cap, ConvForce::Auto)) RC(ensure_mixed_weights(h, b.c1, h->enc_allocs, false));
        if (b.stride == 1 && wino_mixed_eligible(h, b.c2, N, ch, cw, b.depth, wino_cap, ConvForce::Auto)) RC(ensure_mixed_weights(h, b.c2, h->enc_allocs, false));
        ch /= b.stride; cw /= b.stride;
    }
    h->mixed_ready_n = N; h->mixed_ready_h = H; h->mixed_ready_w = W;
    return FFR_OK;
}

}  // namespace ffr_eng

// =========================================================================================
extern "C" {

int ffr_load_encoder(ffr_handle* h, const ffr_tensor_desc* t, int n) {
    if (!h || !t || n <= 0) return fail(h, FFR_ERR_ARG, "ffr_load_encoder: bad arguments");
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    hipDeviceSynchronize();
    free_list(h->enc_allocs);
    ++h->generation;
    h->enc_loaded = false;
    h->mixed_ready_n = 0; h->mixed_weight_bytes = 0; h->enc_weight_bytes = 0; h->mixed_pack_s = 0.0; h->split_weight_bytes = 0; h->wf_split_weight_bytes = 0;
    const auto load_t0 = std::chrono::steady_clock::now();
    SD sd; sd.h = h;
    for (int i = 0; i < n; ++i) if (t[i].name) sd.m[t[i].name] = &t[i];
    auto& own = h->enc_allocs;

    // stem (model_ir_se50.py:118-120): BN folded into the weights, [27][64] tap-major
    {
        const float* W = sd.get("input_layer.0.weight", {64, 3, 3, 3});
        BNFold bn;
        if (!W || !bn_fold(sd, "input_layer.1", 64, bn)) return sd.rc;
        const float* sl = sd.get("input_layer.2.weight", {64});
        if (!sl) return sd.rc;
        std::vector<float> w(27 * 64), b(64), s(64);
        for (int co = 0; co < 64; ++co) {
            for (int k = 0; k < 27; ++k) w[k * 64 + co] = (float)((double)W[co * 27 + k] * bn.s[co]);
            b[co] = (float)bn.t[co];
            s[co] = sl[co];
        }
        RC(upload(h, own, w, &h->stem_w));
        RC(upload(h, own, b, &h->stem_b));
        RC(upload(h, own, s, &h->stem_s));
    }
    // Backbone(num_layers, ., mode): the number of bottlenecks tells num_layers (24 / 49 / 50 = 50 / 100 / 152 layers,
    // model_ir_se50.py:84-105), the presence of res_layer.5 the mode ('ir_se' with the SEModule, 'ir' without, :113-116)
    int n_blocks = 0;
    while (sd.m.count("body." + std::to_string(n_blocks) + ".res_layer.1.weight")) ++n_blocks;
    std::vector<int> cin, depth, stride;
    if (!block_table(n_blocks, cin, depth, stride))
        return fail(h, FFR_ERR_KEY, "the state_dict holds %d bottlenecks; Backbone has 24, 49 or 50 (num_layers 50, 100, 152)", n_blocks);
    const bool has_se = sd.m.count("body.0.res_layer.5.fc1.weight") != 0;
    h->blocks.assign(n_blocks, Block());
    for (int i = 0; i < n_blocks; ++i) {
        Block& b = h->blocks[i];
        b.cin = cin[i]; b.depth = depth[i]; b.stride = stride[i];
        const std::string p = "body." + std::to_string(i);
        BNFold bn1, bn2;
        if (!bn_fold(sd, p + ".res_layer.0", b.cin, bn1) || !bn_fold(sd, p + ".res_layer.4", b.depth, bn2)) return sd.rc;
        const float* W1 = sd.get(p + ".res_layer.1.weight", {b.depth, b.cin, 3, 3});
        const float* sl = sd.get(p + ".res_layer.2.weight", {b.depth});
        const float* W2 = sd.get(p + ".res_layer.3.weight", {b.depth, b.depth, 3, 3});
        const float* f1 = has_se ? sd.get(p + ".res_layer.5.fc1.weight", {b.depth / 16, b.depth, 1, 1}) : nullptr;
        const float* f2 = has_se ? sd.get(p + ".res_layer.5.fc2.weight", {b.depth, b.depth / 16, 1, 1}) : nullptr;
        if (!W1 || !sl || !W2 || (has_se && (!f1 || !f2))) return sd.rc;
        RC(pack_conv(h, own, W1, b.depth, b.cin, 3, 3, &bn1, nullptr, sl, 1, 1, 0, &b.c1));
        RC(pack_conv(h, own, W2, b.depth, b.depth, 3, 3, nullptr, &bn2, nullptr, b.stride, 1, 0, &b.c2));
        if (has_se) {
            RC(upload(h, own, std::vector<float>(f1, f1 + (size_t)b.depth / 16 * b.depth), &b.fc1));
            RC(upload(h, own, std::vector<float>(f2, f2 + (size_t)b.depth / 16 * b.depth), &b.fc2));
        }
        b.has_sc = b.cin != b.depth;
        if (b.has_sc) {
            BNFold bns;
            const float* Ws = sd.get(p + ".shortcut_layer.0.weight", {b.depth, b.cin, 1, 1});
            if (!Ws || !bn_fold(sd, p + ".shortcut_layer.1", b.depth, bns)) return sd.rc;
            RC(pack_conv(h, own, Ws, b.depth, b.cin, 1, 1, nullptr, &bns, nullptr, b.stride, 0, 0, &b.sc));
        }
    }
    {   // Backbone.bn (:126,139)
        BNFold bn;
        if (!bn_fold(sd, "bn", 512, bn)) return sd.rc;
        std::vector<float> s(512), tt(512);
        for (int c = 0; c < 512; ++c) { s[c] = (float)bn.s[c]; tt[c] = (float)bn.t[c]; }
        RC(upload(h, own, s, &h->bn_s));
        RC(upload(h, own, tt, &h->bn_t));
    }
    {   // output_layer (:121-125): BN2d -> Flatten(NCHW) -> Linear -> BN1d as ONE GEMM on the NHWC trunk
        BNFold b0, b4;
        if (!bn_fold(sd, "output_layer.0", 512, b0) || !bn_fold(sd, "output_layer.4", 512, b4)) return sd.rc;
        const float* W = sd.get("output_layer.3.weight", {512, 25088});
        const float* bias = sd.get("output_layer.3.bias", {512});
        if (!W || !bias) return sd.rc;
        ConvW& L = h->fc;
        L = ConvW();
        L.cin = L.cin_pad = 25088; L.cout = L.cout_pad = 512; L.R = L.S = 1; L.stride = 1; L.pad = 0;
        std::vector<float> wp((size_t)512 * 25088), bb(512);
        std::vector<double> wd(wp.size());
        for (int o = 0; o < 512; ++o) {
            double acc = bias[o];
            for (int c = 0; c < 512; ++c)
                for (int p = 0; p < 49; ++p) {
                    const double wv = W[(size_t)o * 25088 + c * 49 + p];
                    wp[(size_t)o * 25088 + p * 512 + c] = (float)(wv * b0.s[c] * b4.s[o]);
                    wd[(size_t)o * 25088 + p * 512 + c] = wv * b0.s[c] * b4.s[o];
                    acc += wv * b0.t[c];
                }
            bb[o] = (float)(b4.s[o] * acc + b4.t[o]);
        }
        RC(upload(h, own, wp, &L.w));
        RC(upload(h, own, bb, &L.bias));
        RC(upload_split(h, own, wd, &L.w3));
    }
    h->enc_loaded = true;
    h->enc_load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - load_t0).count();
    return FFR_OK;
}

int ffr_load_recnet(ffr_handle* h, const ffr_tensor_desc* t, int n) {
    if (!h || !t || n <= 0) return fail(h, FFR_ERR_ARG, "ffr_load_recnet: bad arguments");
    FFR_DEVICE_SCOPE(h); RC(check_fwd(h, false, false, 1));
    hipDeviceSynchronize();
    free_list(h->rec_allocs);
    ++h->generation;
    h->rec_loaded = false;
    h->rec_weight_bytes = 0;
    const auto load_t0 = std::chrono::steady_clock::now();
    SD sd; sd.h = h;
    for (int i = 0; i < n; ++i) if (t[i].name) sd.m[t[i].name] = &t[i];
    auto& own = h->rec_allocs;

    // ConvLayer = reflect-pad -> conv3x3 (no bias) -> BN -> PReLU   (recnet.py:52-85)
    auto conv_layer = [&](const std::string& p, int cin, int cout, ConvW* L) -> int {
        const float* W = sd.get(p + ".conv2d.weight", {cout, cin, 3, 3});
        const float* sl = sd.get(p + ".relu.func.weight", {cout});
        BNFold bn;
        if (!W || !sl || !bn_fold(sd, p + ".norm.norm", cout, bn)) return sd.rc;
        return pack_conv(h, own, W, cout, cin, 3, 3, nullptr, &bn, sl, 1, 1, 1, L);
    };
    for (int i = 0; i < 15; ++i) RC(conv_layer(REC_LAYERS[i].prefix, REC_LAYERS[i].cin, REC_LAYERS[i].cout, &rec_conv(h, i)));

    // Conv4Channel (recnet.py:372-386)
    const float* W1 = sd.get("Conv4Channel.0.weight", {32, 561});
    const float* b1 = sd.get("Conv4Channel.0.bias", {32});
    const float* a1 = sd.get("Conv4Channel.1.func.weight", {512});
    const float* W2 = sd.get("Conv4Channel.2.weight", {512, 32});
    const float* b2 = sd.get("Conv4Channel.2.bias", {512});
    const float* W3 = sd.get("Conv4Channel.3.weight", {32, 512});
    const float* b3 = sd.get("Conv4Channel.3.bias", {32});
    const float* a4 = sd.get("Conv4Channel.4.func.weight", {512});
    const float* W5 = sd.get("Conv4Channel.5.weight", {512, 32});
    const float* b5 = sd.get("Conv4Channel.5.bias", {512});
    const float* W6 = sd.get("Conv4Channel.6.weight", {32, 512});
    const float* b6 = sd.get("Conv4Channel.6.bias", {32});
    const float* a7 = sd.get("Conv4Channel.7.func.weight", {512});
    const float* W8 = sd.get("Conv4Channel.8.weight", {512, 32});
    const float* b8 = sd.get("Conv4Channel.8.bias", {512});
    if (!W1 || !b1 || !a1 || !W2 || !b2 || !W3 || !b3 || !a4 || !W5 || !b5 || !W6 || !b6 || !a7 || !W8 || !b8) return sd.rc;
    std::vector<float> w1a(32 * 49), w1bT(512 * 32);
    for (int j = 0; j < 32; ++j) {
        for (int p = 0; p < 49; ++p) w1a[j * 49 + p] = W1[j * 561 + p];
        for (int c = 0; c < 512; ++c) w1bT[c * 32 + j] = W1[j * 561 + 49 + c];
    }
    auto fold = [](const float* Wb /*[32][512]*/, const float* bb, const float* Wa /*[512][32]*/, const float* ba,
                   std::vector<float>& A, std::vector<float>& d) {
        A.assign(32 * 32, 0.f); d.assign(32, 0.f);
        for (int j = 0; j < 32; ++j) {
            double dd = bb[j];
            for (int k = 0; k < 512; ++k) dd += (double)Wb[j * 512 + k] * ba[k];
            d[j] = (float)dd;
            for (int i = 0; i < 32; ++i) {
                double s = 0;
                for (int k = 0; k < 512; ++k) s += (double)Wb[j * 512 + k] * Wa[k * 32 + i];
                A[j * 32 + i] = (float)s;
            }
        }
    };
    std::vector<float> A2, d2, A3, d3;
    fold(W3, b3, W2, b2, A2, d2);
    fold(W6, b6, W5, b5, A3, d3);
    float* p;
    ChannelPathWeights& cw = h->cw;
    RC(upload(h, own, w1a, &p)); cw.w1a = p;
    RC(upload(h, own, w1bT, &p)); cw.w1b = p;
    RC(upload(h, own, std::vector<float>(b1, b1 + 32), &p)); cw.b1 = p;
    RC(upload(h, own, std::vector<float>(a1, a1 + 512), &p)); cw.a1 = p;
    RC(upload(h, own, A2, &p)); cw.A2 = p;
    RC(upload(h, own, d2, &p)); cw.d2 = p;
    RC(upload(h, own, std::vector<float>(a4, a4 + 512), &p)); cw.a4 = p;
    RC(upload(h, own, A3, &p)); cw.A3 = p;
    RC(upload(h, own, d3, &p)); cw.d3 = p;
    RC(upload(h, own, std::vector<float>(a7, a7 + 512), &p)); cw.a7 = p;
    RC(upload(h, own, std::vector<float>(W8, W8 + 512 * 32), &p)); cw.w8 = p;
    RC(upload(h, own, std::vector<float>(b8, b8 + 512), &p)); cw.b8 = p;
    {   // MFMA operand orders of the last linear (k_channel_path P5)
        std::vector<float> w8a((size_t)16 * 64 * 16), b8a((size_t)16 * 2 * 16);
        for (int t = 0; t < 16; ++t) {
            for (int lane = 0; lane < 64; ++lane)
                for (int ks = 0; ks < 16; ++ks)
                    w8a[((size_t)t * 64 + lane) * 16 + ks] = W8[(size_t)(32 * t + (lane & 31)) * 32 + 2 * ks + (lane >> 5)];
            for (int hh = 0; hh < 2; ++hh)
                for (int r = 0; r < 16; ++r) b8a[((size_t)t * 2 + hh) * 16 + r] = b8[acc_row(32 * t, r) + 4 * hh];
        }
        RC(upload(h, own, w8a, &p)); cw.w8a = p;
        RC(upload(h, own, b8a, &p)); cw.b8a = p;
    }
    h->rec_loaded = true;
    h->rec_load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - load_t0).count();
    return FFR_OK;
}

}  // extern "C"
