// libffrnet_hip.so: the convolution planner -- which kernels one convolution launches, with which block
// shape, split and tile, down to the ordered list of its launches.  Pure decisions on the layer, the call and the handle's
// options: nothing here launches, allocates or synchronises; conv.cpp executes the plans.
#include "engine_internal.h"

namespace ffr_eng {

// ---- convolution dispatch --------------------------------------------------------------
// K <= 128: k_wino_fused transforms its own input (V never exists in memory); larger K: a separate transform kernel
// (measured at batch 256: 17.99 / 18.04 / 18.78 ms per forward for a limit of 64 / 128 / 256, 18.67 without)
static bool wino_phased(const ffr_handle* h, int cin_pad, double x_bytes) {
    return cin_pad <= h->opt.wf_phased_maxk && x_bytes <= 1073741824.0;
}

// The fused launch runs in rounds of one block tile per CU, all of the same duration: a last round with few block tiles leaves
// most of the chip idle for a whole block time (784 block tiles of a 128 -> 128 layer at 28x28 = 3.06 rounds took 4: 245 us
// where 3 rounds are 178).  When the last round would be less than a quarter full, the images whose block tiles fill whole
// rounds run fused and the remaining few images (2 % of the batch) on the transform-kernel + batched-GEMM path, whose small
// tiles spread over every CU (the tail split).  Option wf_tailsplit = 0: off.
static bool short_last_round(const ffr_handle* h, long long block_tiles) {
    const long long full = block_tiles / h->num_cus * h->num_cus, rem = block_tiles - full;
    return h->opt.wf_tailsplit != 0 && !h->opt.wf_trace && full > 0 && rem > 0 && rem * 4 <= h->num_cus;
}

// Which form of k_wino_fused a Winograd convolution of T tiles takes: Fused (blocks of 32 tiles x 64 channels), FusedHalf
// (32 x 32) or Unfused (transform kernels + batched GEMM).  A forced form is kept while option wino_fused is on.
ConvForce wino_fused_form(const ffr_handle* h, int cin_pad, int cout_pad, long long T, double x_bytes, ConvForce ask) {
    if (!h->opt.wino_fused || ask == ConvForce::Direct || ask == ConvForce::Unfused) return ConvForce::Unfused;
    if (ask == ConvForce::FusedSplit) return ConvForce::Fused;
    if (ask == ConvForce::Fused || ask == ConvForce::FusedHalf) return ask;
    // One block tile (all 36 xi) occupies a whole CU and cannot be cut: a launch with fewer block tiles than CUs leaves matrix
    // cores idle, where the batched-GEMM path balances K-tiles over every CU (Conv4Space at batch 256: 32..128 block tiles of
    // 32 x 64, 1.07 ms fused vs 0.55 ms unfused).
    const long long min_blocks = h->opt.wf_minblocks;
    const long long mbn = (T + 31) / 32;
    const long long bt_full = mbn * (cout_pad / 64);
    // Second block shape, 32 tiles x 32 channels (half the accumulators and half the work per block, twice the blocks):
    // for launches whose 32 x 64 block tiles cannot fill the chip (stage 4 / RecNet at 128 images: 128 block tiles) or
    // fill their last round badly.  Not with the in-kernel input transform, which every block of a tile group would repeat.
    auto fit = [&](long long bt) {          // share of the launch's rounds that carries work
        const long long full = bt / h->num_cus * h->num_cus, rem = bt - full;
        if (rem == 0 || short_last_round(h, bt)) return 1.0;
        return (double)bt / (double)(full + h->num_cus);
    };
    bool half_n = false;
    if (!wino_phased(h, cin_pad, x_bytes)) {
        if (bt_full < min_blocks) half_n = 2 * bt_full >= min_blocks;
        else half_n = 0.92 * fit(2 * bt_full) > fit(bt_full);       // a half block costs ~8 % more per unit of work
    }
    if (mbn * (cout_pad / (half_n ? 32 : 64)) < min_blocks) return ConvForce::Unfused;
    return half_n ? ConvForce::FusedHalf : ConvForce::Fused;
}

// True when the convolution WOULD run on the exact 4+4+3+3 tiling (k_wino_fused_mixed) once the three extra weight sets exist:
// 14x14 map, zero padding, scratch large enough, and every CU gets at least two blocks.
// ConvForce::Mixed forces it (tests, experiments; 7x7 maps = 4+3 too).
bool wino_mixed_eligible(const ffr_handle* h, const ConvW& L, int N, int H, int W, int in_pitch, size_t wino_cap, ConvForce force) {
    if (!L.wuc || !L.w || L.R != 3 || L.S != 3 || L.stride != 1 || L.pad_mode != 0 || in_pitch != L.cin_pad) return false;
    if (!(H == 14 && W == 14) && !(force == ConvForce::Mixed && H == 7 && W == 7)) return false;
    WinoMixedGeom g;
    if (!wino_mixed_geom(H, W, &g) || wino_mixed_v_floats(g, N, L.cin_pad, nullptr) > wino_cap) return false;
    if (force == ConvForce::Mixed) return true;
    if (force != ConvForce::Auto || !layer_wino(h, L) || !h->opt.wino_fused || !h->opt.wf_mixed) return false;
    // >= 2 blocks per CU: a long block pairs with a short one (16 instead of 18 slots per CU).  With ONE block per CU the (4,4) blocks
    // set the time: a single launch still wins 7 % there because V is 16 % smaller (round 5, tools/mixed7_experiment.py: 256 -> 256
    // at 128 images: 95.1 + 31.8 us padded vs 92.9 + 24.9 us exact), but in the forward, where the transform rides in the combine
    // kernel, it is a tie (14.68 k vs 14.70 k embeddings/s at 128 images) and would cost the 0.7 GB of extra weight sets
    return wino_mixed_blocks(N, H, W, L.cout_pad) >= 2 * h->num_cus;
}

// The one place the path rules live: which path the convolution L takes for call c, with which block shape and
// split.  plan_conv (below) adds the launches.
static ConvPlan conv_path(const ffr_handle* h, const ConvW& L, const ConvCall& c) {
    ConvPlan p;
    if (c.wino_stage == 2 && c.v_chunked) {     // V lies in winoV in k_wino_fused's order: the whole conv must run fused from it
        ConvCall whole = c;
        whole.wino_stage = 0; whole.v_chunked = false;
        p = conv_path(h, L, whole);
        if (!p.takes_v) { p = ConvPlan{}; p.refused = "a ready V was announced for a convolution that cannot take it"; }
        return p;
    }
    const ConvForce f = c.force;
    // exact tiling 4+4+3+3 of a 14x14 map (wino_mixed.hip): the weight sets exist (prepare_mixed_weights), the stores are 4-aligned
    if (L.wum[1] && wino_mixed_eligible(h, L, c.N, c.H, c.W, c.in_pitch, c.wino_cap, f) && c.winoV && c.tile == 0 &&
        (c.wino_stage == 0 || (c.wino_stage == 2 && c.v_mixed)) && ((c.out_pitch | c.out_coff | c.res_pitch | c.cout_store) & 3) == 0)
        { p.path = ConvPlan::Mixed; return p; }
    // Winograd F(4x4,3x3) when the layer has the weights and the caller asks for it or leaves it to option wino / the layer's plan
    if (!L.wu || !c.winoV || c.tile != 0 || (f == ConvForce::Auto ? !layer_wino(h, L) : f == ConvForce::Direct)) return p;
    const int tiles_img = ((c.H + 3) / 4) * ((c.W + 3) / 4);
    const long long T = (long long)c.N * tiles_img;
    const double x_bytes = 4.0 * c.N * c.H * c.W * c.in_pitch;
    const bool phased = wino_phased(h, L.cin_pad, x_bytes);
    const ConvForce form = wino_fused_form(h, L.cin_pad, L.cout_pad, T, x_bytes, f);
    if (form != ConvForce::Unfused && L.wuc && c.wino_stage == 0 && (phased || wino_chunked_floats(T, L.cin_pad) <= c.wino_cap) &&
        T < 0x7fffffffLL) {
        p.path = ConvPlan::Fused;
        p.phased = phased;
        p.half_n = form == ConvForce::FusedHalf;
        // split-operand K loop: the layer has the planes, the launch is the in-kernel-transform form with 32 x 64 blocks, and option
        // wf_split is on (Auto) or the caller asks for it by name.  A caller that forces Fused / FusedHalf gets the fp32 loop.
        p.split = L.wu3 && phased && !p.half_n && (f == ConvForce::FusedSplit || (f == ConvForce::Auto && h->opt.wf_split != 0));
        if (f == ConvForce::FusedSplit && !p.split) { p = ConvPlan{}; p.refused = "the split-operand fused form was asked for a layer or launch that cannot run it"; return p; }
        const int nbn = L.cout_pad / (p.half_n ? 32 : 64);
        const long long block_tiles = (T + 31) / 32 * nbn;
        if (f == ConvForce::Auto && short_last_round(h, block_tiles)) {
            // (leaving 8..64 CUs without a block tile in the last round for the remainder's kernels did not help: 16.78 ms
            // per forward with none, 16.79 / 16.81 / 16.83 / 17.04 with 8 / 16 / 32 / 64)
            const long long full = block_tiles / h->num_cus * h->num_cus;
            const int n_main = (int)((full / nbn) * 32 / tiles_img);       // images whose tiles fit into full / nbn tile groups
            const size_t rem_floats = (size_t)36 * (c.N - n_main) * tiles_img * (L.cin_pad > L.cout_pad ? L.cin_pad : L.cout_pad);
            if (n_main >= 1 && n_main < c.N && rem_floats <= c.wino_cap) {
                p.n_main = n_main;
                // the remainder needs none of the main launch's buffers when that transforms its own input (phased): it
                // runs on the second stream, its short blocks slot in between the rounds of the main launch
                p.side = phased ? h->side : nullptr;
            }
        }
        p.takes_v = !phased && p.n_main == 0 && L.pad_mode == 0 && c.in_pitch == L.cin_pad;
        return p;
    }
    if (f == ConvForce::FusedSplit) p.refused = "the split-operand fused form was asked for a launch that cannot run fused";
    else if (L.wu == L.wuc) p.refused = "Winograd weights exist in the fused kernel's order only, but this launch cannot run fused";
    else if ((size_t)36 * T * L.cin_pad <= c.wino_cap && (size_t)36 * T * L.cout_pad <= c.wino_cap && T < 0x7fffffffLL) p.path = ConvPlan::Unfused;
    return p;
}

// Tile shape and block count of one launch.
//  * large problems (at least a quarter of a tile of K-tiles per persistent block at 128x128):
//    persistent stream-K over 256 CUs x resident blocks, biggest tile that divides cout (tile
//    efficiency measured on the MI355X: 128x128 > 128x64 > 64x64, profiles/r01_conv_sweep*);
//  * split-operand form (split): the same rules with that form's resident blocks (its stages are larger: igemm.hip);
//  * small problems: 64x64 tiles; whole tiles per block when they fill 160..1024 blocks
//    (nothing is cut), else stream-K with at least `min_units` K-tiles per block.
void plan_igemm(long long M, int cout_pad, int nkt, int nbatch, int force_tile, int min_units, int* tile, int* nblocks, int* granule, bool split) {
    auto ntiles = [&](int t) {
        int bm, bn;
        igemm_tile_shape(t, &bm, &bn);
        return ((M + bm - 1) / bm) * (long long)(cout_pad / bn) * nbatch;
    };
    int best = (cout_pad % 128 == 0) ? IGEMM_TILE_128x128 : IGEMM_TILE_128x64;
    // split form: one 128x128 block fills a CU's LDS, so nothing runs beside a block's prologue and epilogue; with fewer than 16
    // K-tiles per tile (the 1x1 shortcuts: 2 / 4 / 8) those outweigh the loop and two 128x64 blocks per CU are faster
    // (batch 256: 56 / 42 / 43 us against 65 / 49 / 49; the 3x3 stride-2 layers with 18-72 K-tiles: 365 / 345 / 345 against 335 / 326 / 310)
    if (split && nkt < 16) best = IGEMM_TILE_128x64;
    const long long big_units = ntiles(best) * nkt;
    const bool large = big_units / (256LL * igemm_resident_blocks(best, split)) >= (nkt + 3) / 4 && M * nbatch >= 1024;
    if (!large) best = IGEMM_TILE_64x64;
    bool exact = false;
    if (large) {
        // a tile shape whose tile count is a multiple of its persistent block count needs no cut at all
        for (int t = IGEMM_TILE_128x128; t <= IGEMM_TILE_128x64; ++t) {
            int bm, bn;
            igemm_tile_shape(t, &bm, &bn);
            if (cout_pad % bn || (split && nkt < 16 && t == IGEMM_TILE_128x128)) continue;
            if (ntiles(t) % (256LL * igemm_resident_blocks(t, split)) == 0) { best = t; exact = true; break; }
        }
    }
    if (force_tile >= 1 && force_tile <= IGEMM_NTILES) { best = force_tile; exact = false; }
    const long long tiles = ntiles(best);
    const long long units = tiles * (long long)nkt;
    const long long pmax = 256LL * igemm_resident_blocks(best, split);
    long long p;
    *granule = 1;
    if (exact || (nkt < 16 && tiles >= pmax && (nkt <= 4 || tiles >= pmax * 8))) {   // whole tiles, nothing is cut
        *granule = nkt;
        p = pmax;
    } else if (large) {
        p = pmax;
        if (p > units / 4) p = units / 4;
    } else if (tiles >= 160 && tiles <= pmax) {
        *granule = nkt;
        p = tiles;
    } else {
        p = units / min_units;
        if (p > pmax) p = pmax;
    }
    if (p < 1) p = 1;
    *tile = best;
    *nblocks = (int)p;
}

// plan_igemm for one k_igemm launch of call c (its forced tile and stream-K scratch) as the plan entry of `path`, with what
// follows from it: the tile grid, whether any tile is cut (the in-launch fix-up runs) and whether the scratch holds the launch
// (gemm.nomem: which piece does not).  run_gemm launches exactly this.
ConvLaunch plan_gemm_launch(const ffr_handle* h, const ConvCall& c, int path, int images, long long M, int cout_pad, int nkt, int nbatch,
                            bool split) {
    ConvLaunch e;
    GemmPlan& g = e.gemm;
    plan_igemm(M, cout_pad, nkt, nbatch, c.tile, h->opt.sk_minunits, &g.tile, &g.nblocks, &g.granule, split);
    int bm, bn;
    igemm_tile_shape(g.tile, &bm, &bn);
    g.mtiles = (int)((M + bm - 1) / bm);
    g.ntiles = cout_pad / bn;
    g.units = (long long)nbatch * g.mtiles * g.ntiles * nkt;
    g.cut = g.granule == 1 && ((g.units % g.nblocks) != 0 || ((g.units / g.nblocks) % nkt) != 0);
    if (g.cut && (size_t)g.nblocks * 2 * bm * bn > c.partial_cap) g.nomem = "stream-K workspace too small";
    else if ((size_t)nbatch * g.mtiles * g.ntiles > c.tickets_cap) g.nomem = "stream-K ticket array too small";
    ffr_conv_launch& r = e.rec;
    r.path = path; r.images = images; r.rows = (int)M;
    r.tile = g.tile; r.nblocks = g.nblocks; r.granule = g.granule; r.nkt = nkt; r.tiles = nbatch * g.mtiles * g.ntiles;
    r.cut = g.cut ? 1 : 0; r.split = split ? 1 : 0;
    return e;
}

// Tile shape and block count of k_gemm_stream for the 36 GEMMs [T x K] * [K x cout_pad] of a Winograd convolution: fewest
// rounds of whole tiles over the resident blocks, weighted by loop efficiency.
static void plan_gemm_stream(long long T, int cout_pad, int* tile, int* nblocks) {
    *tile = IGEMM_TILE_128x64; *nblocks = 768;
    double best = 1e300;
    for (int tt = IGEMM_TILE_128x128; tt <= IGEMM_TILE_128x64; ++tt) {
        int bm, bn;
        igemm_tile_shape(tt, &bm, &bn);
        if (cout_pad % bn) continue;
        const long long tiles = 36LL * ((T + bm - 1) / bm) * (cout_pad / bn);
        const long long pmax = 256LL * igemm_resident_blocks(tt);
        const long long p = pmax > tiles ? tiles : pmax;
        const double rounds = (double)((tiles + p - 1) / p);
        // a block gets 1/R of its CU (R co-resident blocks), so a round of tiles costs bm*bn*R;
        // the 128x64 loop runs at ~92% of the 128x128 loop's rate (measured per layer, r01 traces)
        const double share = (double)((p + 255) / 256);
        const double cost = rounds * bm * bn * share / (tt == IGEMM_TILE_128x128 ? 1.0 : 0.92);
        if (cost < best) { best = cost; *tile = tt; *nblocks = (int)p; }
    }
}

// Call c on its images [n0, n0 + n) alone: every tensor of c moved on by n0 images
ConvCall conv_part(const ConvW& L, const ConvCall& c, int n0, int n) {
    ConvCall q = c;
    q.N = n;
    const size_t px = (size_t)n0 * c.H * c.W;
    if (c.x) q.x = c.x + px * c.in_pitch;
    if (c.out) q.out = c.out + px * c.out_pitch;
    if (c.resid) q.resid = c.resid + px * c.res_pitch;
    if (c.tile_sums) q.tile_sums = c.tile_sums + (size_t)n0 * ((c.H + 3) / 4) * ((c.W + 3) / 4) * L.cout_pad;
    return q;
}

// The two calls of a tail split (path p of call c, p.n_main > 0): c1 = the first n_main images in the fused form of p, c2 = the
// rest through the transform kernels + batched GEMM
static void tail_split_calls(const ConvW& L, const ConvCall& c, const ConvPlan& p, ConvCall* c1, ConvCall* c2) {
    *c1 = conv_part(L, c, 0, p.n_main);
    c1->force = p.half_n ? ConvForce::FusedHalf : p.split ? ConvForce::FusedSplit : ConvForce::Fused;
    *c2 = conv_part(L, c, p.n_main, c.N - p.n_main);
    c2->force = ConvForce::Unfused;
}

// The launch of a convolution that makes one (path p of call c, no tail split), with the values the plan record shows
static ConvLaunch conv_launch(const ffr_handle* h, const ConvW& L, const ConvCall& c, const ConvPlan& p) {
    const long long T = (long long)c.N * ((c.H + 3) / 4) * ((c.W + 3) / 4);
    if (p.path == ConvPlan::Direct) {
        // split-operand form: the layer's weights were split at load time (or by ffr_op_conv's flag) and option igemm_split is on
        const int Ho = (c.H + 2 * L.pad - L.R) / L.stride + 1, Wo = (c.W + 2 * L.pad - L.S) / L.stride + 1;
        return plan_gemm_launch(h, c, FFR_CP_DIRECT, c.N, (long long)c.N * Ho * Wo, L.cout_pad, L.R * L.S * L.cin_pad / 32, 1,
                                L.w3 && h->opt.igemm_split);
    }
    if (p.path == ConvPlan::Unfused && !h->opt.gemm_stream)         // the 36 GEMMs as one batched k_igemm launch
        return plan_gemm_launch(h, c, FFR_CP_UNFUSED_IGEMM, c.N, T, L.cout_pad, L.cin_pad / 32, 36, false);
    ConvLaunch e;
    ffr_conv_launch& r = e.rec;
    r.images = c.N; r.rows = (int)T;
    if (p.path == ConvPlan::Mixed) {
        WinoMixedGeom g;
        wino_mixed_geom(c.H, c.W, &g);
        r.path = FFR_CP_MIXED; r.rows = c.N * (g.n4 + g.n3) * (g.n4 + g.n3);
        r.block_tiles = wino_mixed_blocks(c.N, c.H, c.W, L.cout_pad);
    } else if (p.path == ConvPlan::Fused) {
        r.path = FFR_CP_FUSED; r.phased = p.phased ? 1 : 0; r.half_n = p.half_n ? 1 : 0; r.split = p.split ? 1 : 0;
        r.block_tiles = (int)((T + 31) / 32) * (L.cout_pad / (p.half_n ? 32 : 64));
    } else {                                                        // 36 GEMMs in one persistent k_gemm_stream launch
        r.path = FFR_CP_UNFUSED_STREAM;
        plan_gemm_stream(T, L.cout_pad, &r.tile, &r.nblocks);
        int bm, bn;
        igemm_tile_shape(r.tile, &bm, &bn);
        r.nkt = L.cin_pad / 32; r.granule = r.nkt;                  // whole tiles only: nothing is cut
        r.tiles = (int)(36 * ((T + bm - 1) / bm) * (L.cout_pad / bn));
    }
    return e;
}

// The plan of the convolution L for call c: the path conv_path chooses and every launch it makes, in launch
// order.  Launches, allocates and writes nothing: run_conv executes the entries, the plan record and ffr_plan_conv_host report
// them, run_trunk asks the plan ahead of the launch.
ConvPlan plan_conv(const ffr_handle* h, const ConvW& L, const ConvCall& c) {
    ConvPlan p = conv_path(h, L, c);
    if (p.refused) return p;
    if (!p.n_main) { p.launch[p.n_launch++] = conv_launch(h, L, c, p); return p; }
    // tail split: a header, then the two parts as their own calls plan them, the one enqueued first in front
    ConvCall c1, c2;
    tail_split_calls(L, c, p, &c1, &c2);
    const ConvPlan p1 = plan_conv(h, L, c1), p2 = plan_conv(h, L, c2);
    if (p1.refused || p2.refused) { const char* why = p1.refused ? p1.refused : p2.refused; p = ConvPlan{}; p.refused = why; return p; }
    ffr_conv_launch& r = p.launch[0].rec;
    r.path = FFR_CP_TAIL_SPLIT; r.images = c.N; r.rows = c.N * ((c.H + 3) / 4) * ((c.W + 3) / 4);
    r.n_main = p.n_main; r.side = p.side ? 1 : 0; r.half_n = p.half_n ? 1 : 0; r.phased = p.phased ? 1 : 0; r.split = p.split ? 1 : 0;
    const int rest = p.side ? 1 : 2;            // the rest is enqueued first when it runs on the second stream
    p.launch[3 - rest] = p1.launch[0];
    p.launch[rest] = p2.launch[0];
    p.launch[rest].n0 = p.n_main;
    p.n_launch = 3;
    return p;
}

// Row blocks per image of k_channel_path (1, 2 or 4; forced = option channel_rows, 0 leaves the choice here; 0 is returned for
// a forced value that is none of them).  One block per CU (147.6 of the CU's 160 KB of LDS): rounds x block time, the fewest
// row blocks among equals.  The block times (us: whole image / half / quarter of M_channel's rows) are MEASURED ON THE MI355X
// (profiles/r05_channel_path_phase_trace.txt) and only their ratios matter; this library runs on gfx950 only (ffr_create
// refuses other devices).
int plan_channel_rows(int N, int num_cus, int forced) {
    if (forced) return forced == 1 || forced == 2 || forced == 4 ? forced : 0;
    const double t_block[3] = {181.0, 140.0, 101.0};
    double best = 1e30;
    int row_blocks = 1;
    for (int k = 0; k < 3; ++k) {
        const int rb = 1 << k;
        const double t = (double)(((long long)N * rb + num_cus - 1) / num_cus) * t_block[k];
        if (t < best - 1e-9) { best = t; row_blocks = rb; }
    }
    return row_blocks;
}

}  // namespace ffr_eng
