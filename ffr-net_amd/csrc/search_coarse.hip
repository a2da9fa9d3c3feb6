// search_coarse.hip -- certified bf16 shortlist search (include/ffrnet.h, ffr_coarse_pack / ffr_search_topk_coarse): the top-k
// of ffr_search_topk, bit for bit, with the pass over the whole gallery on the bf16 matrix cores and half the bytes.
//
// Method.  A ranking needs the right k rows and then their exact scores, not every score exact.  The gallery keeps, beside
// its fp32 rows, the plane g^ = bf16(g / |g|) (round to nearest even; |g| the fp32 norm of ffr_row_norms).  A probe is split
// into two bf16 planes, q^ = q / |q| = hi + lo, hi = bf16(q^), lo = bf16(q^ - hi).  The coarse pass ranks every row by
//     c = (sum_k (hi + lo)_k g^_k) * (|q||g| / (|q||g| + 1e-8))
// and keeps the best k' = min(128, max(2k, 32)) rows per probe; the exact fp32 arithmetic of cosine_tile.h then scores those
// k' rows only, and a bound on |c - s| decides per probe whether the shortlist certainly holds the true top-k.
//
// Bound.  u = 2^-8 is the unit round-off of bf16 (8 significant bits).  g^_k = (g_k / |g|)(1 + a_k), |a_k| <= u, and
// (hi + lo)_k = (q_k / |q|)(1 + b_k), |b_k| <= u^2 (lo rounds a residual that is itself <= u |q^_k|).  So
//     |sum (hi + lo)_k g^_k - cos(q, g)| <= (u + u^2 + u^3) sum |q_k||g_k| / (|q||g|) <= u + u^2 + u^3    (Cauchy-Schwarz)
// = 0.0039216.  Products of two bf16 values are exact in fp32; for the accumulation of the 1024 products in the matrix core,
// whose internal rounding is not documented, 2^-13 is allowed (8 x a plain fp32 chain at |partial sums| <= 1).  That
// allowance is assumed, not measured: c never leaves the device, and the tests see it only through the certificates.  The factor
// of c is the exact score's own denominator, <= 1, from the same fp32 norms; the exact score s is within 1e-6 of the cosine.
// Together 0.00405; the constant is FFR_COARSE_EPS = 2^-8 + 2^-12 = 0.00415.  Normalised operands keep every bf16 value in
// [-1, 1]: no denormal and no overflow question in the bf16 path.
//
// Certificate.  The shortlist has coarse scores c_1 >= ... >= c_k'; s_k is the k-th best exact score in it under the total
// order (descending score, ascending index).  A row outside has c <= c_k', so s <= c_k' + eps.  The probe is certified iff
// G <= k' (the shortlist is the gallery) or c_k' + eps < s_k, strictly: then no row left out can even tie the k-th, and the
// top k of the re-scored shortlist under the total order is the exact answer.  A probe that is not certified is searched by
// k_search_topk; either way the caller gets the bits of ffr_search_topk.
// Unsafe norms: a norm that is not zero and lies outside [2^-60, 2^60] (or is not finite) belongs to a sum of squares that
// under- or overflowed, and x / |x| means nothing; so does a zero norm over a row that is not all zeros (every square
// underflowed, yet its dot products, times the 1e8 of the score's floor, need not be small).  Packing such a row sets the
// gallery's sticky flag, and while it is set no probe is certified; such a probe is not certified.  A row of zeros packs to
// zeros: c = 0 = s.
//
// k_coarse_pack     rows + norms -> plane, one wave per row (as k_row_norms), 16-byte stores; ORs the flag.
// k_search_coarse   the bf16 instantiation of search_core.h: the block of k_search_topk with the tile of coarse_tile.h, the
//                   list k' long.  One sorted list per (chunk, probe), index = gallery row, folded by k_topk_merge.
// k_search_rescore  a block per probe.  The shortlist (padded to whole waves of 32 rows) goes through
//                   CosineStreamT<GatherRows>::tile -- the K loop, chain sum and score formula of k_search_topk, so the same
//                   bits -- against a probe tile that holds the probe in column 0 and zeros beside it: 31/32 of the MFMAs
//                   are wasted on Q * k' rows, one fp32 tile (8 us) per block, the blocks side by side.  Then: ranks under
//                   the total order, the certificate, the [k] list of a certified probe, the id of any other appended to
//                   a device list.
// k_probe_gather / k_topk_scatter   the exact pass over the probes that were not certified runs without a host
//                   synchronisation: it is always launched, sized for Q, on the gathered probes, and k_search_topk /
//                   k_topk_merge take the device count -- tiles (probes) past it leave at once.
//
// Subjects (ffr_search_topk_coarse_subjects).  A gallery whose rows carry subject[G] (< 0 = removed) takes the same pass in
// ROW mode under the removal mask -- k_search_coarse_live, the <true, SR_LIVE> instantiation of search_core.h -- so the
// subject merge never runs over the gallery; identities are formed once per probe, on the <= 128 re-scored entries.
// L is the shortlist of the k' best LIVE rows, c_1 >= ... >= c_k'; every live row outside L has c <= c_k', hence exact
// s <= c_k' + eps, eps unchanged.  k' = min(128, max(2k, 32)) for rows (k <= 64) and min(128, max(4k, 64)) for identities
// (k <= 32): a person's rows crowd the head of the list.  The probe is certified iff the plane flag is clear, its norm is
// safe, and either L holds fewer than k' rows or G <= k' (L is then every live row: with removals, G > k' no longer means a
// full list), or -- identities -- at least k entries are alive, and c_k' + eps < s_k, strictly.  An entry is alive iff no
// other entry of its subject comes before it in the total order (descending exact score, ascending index); s_k is the score
// of the k-th alive entry (rows: of the k-th entry).
// Proof for identities.  Let u be one of the first k alive entries.  Its alive entry scores >= s_k > every row outside L, so
// no row of u outside L beats or ties it: it is best(u) over the whole gallery.  Let v be a subject not among them: either
// its best row in L ranks after the k-th alive entry, or v has no row in L and its best row scores below s_k.  Hence the
// first k of {best(u)} over the gallery are the first k alive entries of L, with their scores and indices.  Fewer than k
// alive entries in a full shortlist is not certified: more subjects may lie outside (one person enrolled with more rows than
// the list holds).  The probes that are not certified go through k_search_subjects / k_topk_merge_subjects with the device
// count, and their lists come back with the subject plane.
//
// Filter (ffr_search_topk_coarse_filtered).  Under the per-probe filter of ffr_search_topk_filtered -- row g is admissible for
// probe q iff (tag[g] & qmask[q]) != 0 and (no subjects, or subject[g] >= 0) -- the pass over the plane is the <true, SR_ROWS
// | SR_LIVE, false, true> instantiation of search_core.h (k_search_coarse_filtered, k_search_coarse_filtered_live): rows in
// both modes, no subject merge, the mask word in a register and the 16 tag words beside the norms, LDS as before.  All of
// the above holds per probe with "live row" read as "row admissible for this probe".  L is the k' best admissible rows by
// (descending c, ascending index); every admissible row outside L has c <= c_k', hence s <= c_k' + eps, eps unchanged: the
// bound is about one (q, g) pair and knows no filter.  The probe is certified iff the plane flag is clear, its norm is safe,
// and either L holds fewer than k' rows or G <= k' (L is then every admissible row of this probe: under a filter, as under
// removals, G > k' does not mean a full list), or -- identities -- at least k entries are alive, and c_k' + eps < s_k,
// strictly.  The proof for identities above goes through word for word: a person speaks with the best row the probe may
// see, best(u) and "a row outside L" range over the admissible rows of that one probe, and nothing in it compares rows of
// two probes.  Every listed row is admissible by construction, so k_search_rescore reads no tags; its one change is that a
// short list counts as whole without subjects too (the <false, true> instantiation; the two others are as they were).  A
// probe with mask 0 has an empty list: certified, k slots of padding, what the exact filtered search gives it.
// k_probe_gather takes the mask word of an uncertified probe along, and the exact pass is k_search_filtered with each
// gathered probe's own mask.
// k' and the k limits are those above: 64 rows, 32 identities; beyond them, and at G = 0, the exact filtered search runs alone.
//
// Flops: a coarse search counts 2*Q*G*512, the scores it ranks (the second probe plane, the re-score and the exact pass over
// uncertified probes are not counted).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>

#include "coarse_tile.h"
#include "cosine_tile.h"
#include "device_util.h"
#include "ffr_kernels.h"
#include "search_core.h"

namespace ffr {

namespace {

__global__ __launch_bounds__(256) void k_coarse_pack(const float* __restrict__ x, const float* __restrict__ norms, long long n,
                                                     uint16_t* __restrict__ plane, int* __restrict__ flag) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float nrm = norms[row];
    const float* p = x + row * CT_DIM + 8 * lane;
    *(u32x4*)(plane + row * CT_DIM + 8 * lane) = coarse_round8(p, nrm, nullptr);
    bool unsafe = lane == 0 && !coarse_safe_norm(nrm);
    if (nrm == 0.f) unsafe = coarse_any_nonzero8(p);
    if (unsafe) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256, 1) void k_search_coarse(const SearchArgs a) { search_block<true>(a); }
// under the removal mask: rows with subject < 0 never enter; the shortlist goes out as rows, without a subject plane
__global__ __launch_bounds__(256, 1) void k_search_coarse_live(const SearchArgs a) { search_block<true, SR_LIVE, false>(a); }
// under the per-probe filter: a row enters the list of probe q iff (tag[g] & qmask[q]) != 0 (and, _live, subject >= 0)
__global__ __launch_bounds__(256, 1) void k_search_coarse_filtered(const SearchArgs a) { search_block<true, SR_ROWS, false, true>(a); }
__global__ __launch_bounds__(256, 1) void k_search_coarse_filtered_live(const SearchArgs a) {
    search_block<true, SR_LIVE, false, true>(a);
}

struct RescoreArgs {
    const float* query;       // [Q][512]
    const float* qnorm;       // [Q]
    const float* gallery;     // [G][512]
    const float* gnorm;       // [G]
    const float* sl_s;        // [Q][kp] coarse scores of the shortlist, descending
    const int64_t* sl_i;      // [Q][kp] gallery rows, -1 = padding (at the end)
    const int* plane_flag;
    long long G, index_base;
    float* top_s;             // [Q][k]
    int64_t* top_i;
    int* certified;           // [Q] or null
    int* ulist;               // [Q]
    int* ucount;
    int Q, k, kp;
    const int32_t* subject;   // [G] (SUBJ): every listed row is live, subject >= 0
    int32_t* top_u;           // [Q][k] (SUBJ)
    int distinct;             // (SUBJ) 1: the lists hold subjects, each by its best row
};

// LDS: probe fragments [64][64] f32x4 | exact scores rs[128] | gallery rows ri[128] i64 | sk | (SUBJ) subjects ru[128] i32,
// alive flags ra[128] i32
constexpr size_t RS_OFF_S = (size_t)CT_NG * 64 * 16;
constexpr size_t RS_OFF_I = RS_OFF_S + (size_t)COARSE_MAX_SHORT * 4;
constexpr size_t RS_OFF_K = RS_OFF_I + (size_t)COARSE_MAX_SHORT * 8;
constexpr size_t RS_OFF_U = RS_OFF_K + 16;
constexpr size_t RS_OFF_A = RS_OFF_U + (size_t)COARSE_MAX_SHORT * 4;
constexpr size_t rs_lds_bytes(bool subj) { return subj ? RS_OFF_A + (size_t)COARSE_MAX_SHORT * 4 : RS_OFF_U; }

// SUBJ = false: k_search_rescore of ffr_search_topk_coarse.  SUBJ = true: the shortlist came from k_search_coarse_live; every
// entry carries subject[row], top_u is written beside the list, and with a.distinct the list holds subjects: an entry is
// ALIVE iff no other entry of its subject comes before it in the total order, its place is the number of alive entries
// before it, and s_k is the score of the k-th alive entry (two passes over the <= 128 entries, one barrier between them).
// SHORT: a list shorter than k' is every row its probe may see, also at G > k' -- removals (SUBJ) and the filter leave lists
// short; the third instantiation, <false, true>, is the filtered shortlist of a gallery without subjects.
template <bool SUBJ, bool SHORT = SUBJ>
__global__ __launch_bounds__(256, 1) void k_search_rescore(const RescoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    f32x4* qf = (f32x4*)sm;
    float* rs = (float*)(sm + RS_OFF_S);
    long long* ri = (long long*)(sm + RS_OFF_I);
    float* sk = (float*)(sm + RS_OFF_K);
    int* ru = (int*)(sm + RS_OFF_U);
    int* ra = (int*)(sm + RS_OFF_A);

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k, kp = a.kp;
    const int qi = blockIdx.x;

    cosine_fill_probes(qf, a.query, qi, 1, tid);          // the probe in column 0, zeros beside it
    if (tid < COARSE_MAX_SHORT) {
        ri[tid] = tid < kp ? (long long)a.sl_i[(size_t)qi * kp + tid] : -1;
        rs[tid] = -INFINITY;
        if constexpr (SUBJ) ru[tid] = ri[tid] >= 0 ? a.subject[ri[tid]] : -1;
    }
    const float qn = a.qnorm[qi];
    __syncthreads();

    // exact scores: wave w streams rows 32w .. 32w + 31 of the shortlist; padding reads row 0 (in bounds, G >= 1) and is not kept
    if (w * 32 < kp) {
        const long long mine = ri[w * 32 + n];
        const long long row = mine < 0 ? 0 : mine;
        CosineStreamT<GatherRows> gs(a.gallery, lane);
        gs.prime(row);
        f32x16 acc8[CT_NACC];
        gs.tile(acc8, qf, row);
        const f32x16 acc = COSINE_CHAIN_SUM(acc8);
        if (n == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int slot = cosine_lane_row(w, r, h);
                const long long i = ri[slot];
                if (i >= 0) rs[slot] = cosine_score(acc[r], qn, a.gnorm[i]);
            }
        }
    }
    // a zero norm is safe only over a probe of zeros
    const float* qrow = a.query + (size_t)qi * CT_DIM;
    const int qbad = __syncthreads_or(qn == 0.f && (qrow[tid] != 0.f || qrow[256 + tid] != 0.f));

    // rank of entry tid under the total order
    const bool live = tid < kp && ri[tid] >= 0;
    const bool distinct = SUBJ && a.distinct;
    int rank = INT_MAX;
    bool out = live;                                      // an entry that the list can hold: a row, or its subject's best row
    if (live) {
        const float s = rs[tid];
        const long long i = ri[tid];
        rank = 0;
        if constexpr (SUBJ) {
            const int u = ru[tid];
            bool behind = false;                          // behind another row of its own subject
            for (int e = 0; e < kp; ++e) {
                const bool first = ri[e] >= 0 && (rs[e] > s || (rs[e] == s && ri[e] < i));
                rank += first;
                behind |= first && ru[e] == u;
            }
            if (distinct) out = !behind;
        } else {
            for (int e = 0; e < kp; ++e) rank += ri[e] >= 0 && (rs[e] > s || (rs[e] == s && ri[e] < i));
        }
    }
    if constexpr (SUBJ) {
        if (distinct) {                                   // place among the alive entries (uniform branch: barriers inside)
            if (tid < COARSE_MAX_SHORT) ra[tid] = out;
            __syncthreads();
            if (out) {
                const float s = rs[tid];
                const long long i = ri[tid];
                rank = 0;
                for (int e = 0; e < kp; ++e) rank += ra[e] && (rs[e] > s || (rs[e] == s && ri[e] < i));
            }
        }
    }
    if (out && rank == k - 1) sk[0] = rs[tid];
    const int nv = __syncthreads_count(live);            // listed rows (padding is at the end)
    const int no = SUBJ ? __syncthreads_count(out) : nv; // entries the list can hold
    const bool whole = a.G <= kp || (SHORT && nv < kp);   // every row the probe may see: under a mask or a filter, G > k' need not fill the list
    bool ok = *a.plane_flag == 0 && coarse_safe_norm(qn) && !qbad;
    if (ok && !whole) ok = nv == kp && no >= k && a.sl_s[(size_t)qi * kp + kp - 1] + COARSE_EPS < sk[0];
    if (tid == 0) {
        if (a.certified) a.certified[qi] = ok;
        if (!ok) a.ulist[atomicAdd(a.ucount, 1)] = qi;
    }
    if (!ok) return;
    float* os = a.top_s + (size_t)qi * k;
    int64_t* oi = a.top_i + (size_t)qi * k;
    if (out && rank < k) {
        os[rank] = rs[tid];
        oi[rank] = a.index_base + ri[tid];
        if constexpr (SUBJ) a.top_u[(size_t)qi * k + rank] = ru[tid];
    }
    for (int p = no + tid; p < k; p += 256) {
        os[p] = -INFINITY; oi[p] = -1;
        if constexpr (SUBJ) a.top_u[(size_t)qi * k + p] = -1;
    }
}

__global__ __launch_bounds__(128) void k_probe_gather(const float* __restrict__ query, const float* __restrict__ qnorm,
                                                      const int* __restrict__ ulist, const int* __restrict__ ucount,
                                                      float* __restrict__ uq, float* __restrict__ uqn,
                                                      const uint32_t* __restrict__ qmask, uint32_t* __restrict__ uqm) {
    const int i = blockIdx.x;
    if (i >= *ucount) return;
    const int src = ulist[i];
    ((f32x4*)(uq + (size_t)i * CT_DIM))[threadIdx.x] = ((const f32x4*)(query + (size_t)src * CT_DIM))[threadIdx.x];
    if (threadIdx.x == 0) {
        uqn[i] = qnorm[src];
        if (qmask) uqm[i] = qmask[src];                   // filtered: the probe keeps its own mask in the exact pass
    }
}

__global__ __launch_bounds__(64) void k_topk_scatter(const float* __restrict__ fb_s, const int64_t* __restrict__ fb_i,
                                                     const int32_t* __restrict__ fb_u, const int* __restrict__ ulist,
                                                     const int* __restrict__ ucount, int k, float* __restrict__ top_s,
                                                     int64_t* __restrict__ top_i, int32_t* __restrict__ top_u) {
    const int i = blockIdx.x;
    if (i >= *ucount) return;
    const int dst = ulist[i];
    for (int p = threadIdx.x; p < k; p += 64) {
        top_s[(size_t)dst * k + p] = fb_s[(size_t)i * k + p];
        top_i[(size_t)dst * k + p] = fb_i[(size_t)i * k + p];
        if (fb_u) top_u[(size_t)dst * k + p] = fb_u[(size_t)i * k + p];      // the subject plane, where the lists have one
    }
}

}  // namespace

int coarse_shortlist_size(int k, int distinct) { return distinct ? coarse_shortlist_distinct(k) : coarse_shortlist(k); }
int coarse_max_k(int distinct) { return distinct ? COARSE_MAX_K_DISTINCT : COARSE_MAX_K; }

void coarse_fallback_plan(int Q, long long G, int num_cus, int* ntiles, int* nchunks, long long* chunk_rows) {
    *ntiles = (Q + CT_QT - 1) / CT_QT;
    cosine_chunks(*ntiles, G, 4, num_cus, nchunks, chunk_rows);
}

hipError_t launch_coarse_pack(const float* rows, const float* norms, long long n, uint16_t* plane, int* flag, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_coarse_pack, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, rows, norms, n, plane, flag);
    return hipGetLastError();
}

const void* search_coarse_kernel(bool live, bool filtered) {
    if (filtered) return live ? (const void*)k_search_coarse_filtered_live : (const void*)k_search_coarse_filtered;
    return live ? (const void*)k_search_coarse_live : (const void*)k_search_coarse;
}

hipError_t launch_search_rescore(const float* query, const float* qnorm, int Q, const float* gallery, const float* gnorm,
                                 const float* sl_s, const int64_t* sl_i, const int* plane_flag, long long G, int k, int kp,
                                 long long index_base, float* top_s, int64_t* top_i, int* certified, int* ulist, int* ucount,
                                 hipStream_t stream, const int32_t* subject, int distinct, int32_t* top_u, bool filtered) {
    RescoreArgs a{query, qnorm, gallery, gnorm, sl_s, sl_i, plane_flag, G, index_base, top_s, top_i, certified, ulist, ucount, Q, k, kp,
                  subject, top_u, distinct};
    const size_t lds = rs_lds_bytes(subject != nullptr);
    const void* fn = subject ? (const void*)k_search_rescore<true> : filtered ? (const void*)k_search_rescore<false, true>
                                                                              : (const void*)k_search_rescore<false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    void* args[] = {&a};
    return hipLaunchKernel(fn, dim3((unsigned)Q), dim3(256), args, lds, stream);
}

hipError_t launch_probe_gather(const float* query, const float* qnorm, const int* ulist, const int* ucount, int Q, float* uq,
                               float* uqn, hipStream_t stream, const uint32_t* qmask, uint32_t* uqm) {
    hipLaunchKernelGGL(k_probe_gather, dim3((unsigned)Q), dim3(128), 0, stream, query, qnorm, ulist, ucount, uq, uqn, qmask, uqm);
    return hipGetLastError();
}

hipError_t launch_topk_scatter(const float* fb_s, const int64_t* fb_i, const int* ulist, const int* ucount, int Q, int k,
                               float* top_s, int64_t* top_i, hipStream_t stream, const int32_t* fb_u, int32_t* top_u) {
    hipLaunchKernelGGL(k_topk_scatter, dim3((unsigned)Q), dim3(64), 0, stream, fb_s, fb_i, fb_u, ulist, ucount, k, top_s, top_i, top_u);
    return hipGetLastError();
}

}  // namespace ffr
