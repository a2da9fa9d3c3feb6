/*
 * ffrnet.h -- C ABI of the MI355X-native FFR-Net embedding path (libffrnet_hip.so).
 *
 * The reference (haoosz/FFR-Net) has no FFI layer: its hot path is two Python
 * nn.Module calls.  This header is the boundary a binding (ctypes, cgo, JNI ...)
 * uses instead; each entry point names the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross the boundary;
 *  - every function returns FFR_OK (0) or a negative ffr_status; nothing throws;
 *    ffr_last_error() gives the text of the last failure on that handle;
 *  - "device pointer" = HIP device memory of the handle's device; activations are
 *    fp32; 4-D tensors at the boundary are NCHW contiguous (the reference's layout),
 *    the NHWC layout used inside never leaves the library;
 *  - launches are asynchronous on the hipStream_t passed as `void* stream`
 *    (NULL = the default stream); no hidden device synchronisation.  A call may fork
 *    part of its work onto a second stream the handle owns and joins it back with events
 *    before it returns: for the caller everything is ordered on `stream`, and a call
 *    captured into a hipGraph on `stream` stays one graph;
 *  - one handle per device; a handle is not thread safe.
 */
#ifndef FFRNET_H
#define FFRNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffr_handle ffr_handle;

typedef enum {
    FFR_OK = 0,
    FFR_ERR_ARG = -1,        /* bad argument (null pointer, bad shape, N <= 0 ...)   */
    FFR_ERR_STATE = -2,      /* weights not loaded yet                                */
    FFR_ERR_KEY = -3,        /* a state_dict entry is missing or has the wrong shape  */
    FFR_ERR_HIP = -4,        /* a HIP runtime call failed                             */
    FFR_ERR_NOMEM = -5,      /* device allocation failed                              */
    FFR_ERR_UNSUPPORTED = -6 /* shape the native path does not implement              */
} ffr_status;

/* One named fp32 tensor of a PyTorch state_dict, in HOST memory, C-contiguous.
 * Integer entries (num_batches_tracked) are simply not passed.                     */
typedef struct {
    const char*  name;      /* e.g. "body.3.res_layer.1.weight"                      */
    const float* data;
    int32_t      ndim;      /* 1..4                                                   */
    int64_t      shape[4];
} ffr_tensor_desc;

/* ---- lifetime ------------------------------------------------------------------ */
int  ffr_create(ffr_handle** out, int device);
void ffr_destroy(ffr_handle* h);
const char* ffr_last_error(const ffr_handle* h);      /* h may be NULL: global text  */
const char* ffr_version(void);

/* ---- weights ---------------------------------------------------------------------
 * Replaces Backbone.load_state_dict / RecNet.load_state_dict as used by
 * pretrain/model_ir_se50.py:151-153 and models/trainer.py:98-113,201-214.
 * Eval-mode BatchNorm is folded, weights are re-packed [Cout][R][S][Cin] for the
 * NHWC implicit-GEMM kernels and uploaded; the caller keeps ownership of `t`.
 * Encoder = IR-SE50 (Backbone(50, drop, 'ir_se')): 347 fp32 entries (402 with the
 * integer num_batches_tracked counters, which are not passed).  Backbone(100 | 152, drop, 'ir' | 'ir_se')
 * (pretrain/model_ir_se50.py:84-116) load as well: the number of body.N entries (24 / 49 / 50 bottlenecks) tells
 * num_layers, the presence of res_layer.5 the mode; any other count returns FFR_ERR_KEY.
 * RecNet  = RecNet(512, 7, 'bn', 'prelu'): 106 fp32 entries (121 in all); "classifier.weight"
 * (training-only head, models/recnet.py:396) is ignored if present.               */
int ffr_load_encoder(ffr_handle* h, const ffr_tensor_desc* t, int n);
int ffr_load_recnet(ffr_handle* h, const ffr_tensor_desc* t, int n);

/* ---- forward ---------------------------------------------------------------------
 * Backbone.forward, pretrain/model_ir_se50.py:136-141:
 *   x[N,3,H,W] -> featmap[N,512,H/16,W/16] (after Backbone.bn) and f[N,512]
 *   (output_layer + l2_norm).  f needs H=W=112 (Linear(512*7*7,512), :124); with any
 *   other size pass f = NULL to get the trunk only (e.g. 112x96 -> [N,512,7,6]).
 *   featmap or f may be NULL when not wanted.                                        */
int ffr_encoder_forward(ffr_handle* h, const float* x_nchw, int N, int H, int W,
                        float* featmap_nchw, float* f, void* stream);
/* The same from decoded images: img[N,H,W,3] uint8, HWC, RGB as PIL gives them (device), with the input step of
 * ffr_embed_u8 inside the stem (flip[N] per image, may be NULL).  Bit-identical to ffr_encoder_forward fed with the
 * float tensor torch would build.  f needs H = W = 112; any other size multiple of 16 runs the trunk only.        */
int ffr_encoder_forward_u8(ffr_handle* h, const uint8_t* img_hwc_rgb, const uint8_t* flip, int N, int H, int W,
                           float* featmap_nchw, float* f, void* stream);

/* RecNet.forward(input, label=None), models/recnet.py:398-426:
 *   featmap[N,512,7,7] -> f_new[N,512], feat_new[N,512,7,7] (either may be NULL).    */
int ffr_recnet_forward(ffr_handle* h, const float* featmap_nchw, int N,
                       float* f_new, float* feat_new_nchw, void* stream);

/* encoder + recnet back to back as lfw/lfw_eval.py:240-244 calls them, without the
 * NCHW round trip of featmap: x[N,3,112,112] -> f_new[N,512], f[N,512] (f may be NULL) */
int ffr_embed(ffr_handle* h, const float* x_nchw, int N,
              float* f_new, float* f, void* stream);

/* The same from decoded images: img[N,112,112,3] uint8, HWC, RGB as PIL gives them (device).
 * The reference's input step runs inside the stem kernel (data/dataset.py:70-79,
 * data/dataloader.py:24-28): RGB->BGR swap, horizontal flip where flip[n] != 0 (flip may be
 * NULL; the reference draws ONE flag per pair and applies it to both images), ToTensor (/255),
 * Normalize(0.5, 0.5) -- bit-identical to feeding ffr_embed the float tensor torch would build. */
int ffr_embed_u8(ffr_handle* h, const uint8_t* img_hwc_rgb, const uint8_t* flip, int N,
                 float* f_new, float* f, void* stream);

/* cosine score of lfw/lfw_eval.py:246,248:  sum(a*b) / (|a|*|b| + 1e-8), per row.
 * a, b [n,dim] device fp32 -> score[n] device fp32.                                 */
int ffr_cosine_scores(ffr_handle* h, const float* a, const float* b, int n, int dim,
                      float* score, void* stream);

/* ---- 1:N identification (exact cosine top-k over a gallery) --------------------------------------------------------
 * What the reference's harness lacks: "which of my G enrolled people is this probe?" for masked probes against
 * mask-free enrolments.  Exact brute force in fp32; no approximate index.
 *   score  s(q, g) = dot(q, g) / (|q| |g| + 1e-8), the formula of ffr_cosine_scores and lfw/lfw_eval.py:246; the norms
 *          are fp32 square roots of fp32 sums of squares (ffr_row_norms, as k_cosine computes them); a zero row scores 0.
 *   shapes dim = 512 only (FFR_ERR_UNSUPPORTED otherwise); 1 <= k <= 128, Q >= 1, G >= 0 (FFR_ERR_ARG otherwise).
 *          Rows are contiguous [n][512] fp32, device, 16-byte aligned (FFR_ERR_ARG otherwise); gallery and gallery_norms
 *          may be NULL only when G = 0.
 *   result top_score[Q][k] fp32, top_index[Q][k] int64 (= index_base + gallery row), per probe ordered by DESCENDING
 *          score, ties by ASCENDING index.  When G < k the last k - G slots hold (-inf, -1): they sort after every real
 *          entry, so lists of small or empty shards merge without a special case.
 *   bitwise every (q, g) score is the same fp32 MFMA chain over k wherever it is computed, so repeated calls agree, row q
 *          of a Q-probe call equals the 1-probe call of that probe, and searching contiguous shards of the gallery (each
 *          with its index_base) and merging with ffr_topk_merge equals one search over the whole gallery.
 *   memory the Q x G score matrix never leaves the chip; no host synchronisation; the handle's search scratch (probe norms,
 *          per-chunk lists) grows on demand -- hipMalloc on the first call at a larger shape, which bumps ffr_generation
 *          -- and is reused afterwards, so a call can be captured into a hipGraph once it has run at that shape.
 *          Galleries of 2 GiB and more are supported (64-bit chunk bases, 32-bit offsets inside a chunk).
 *   NaN    inputs holding NaN or inf give unspecified (in-bounds) results.
 * No weights need to be loaded.  Launches are profiled under FFR_KC_SCORE; a search counts flops = 2*Q*G*512.        */
/* norms[n] = |x[r]| of x[n][dim] rows (device); n >= 1.                                                              */
int ffr_row_norms(ffr_handle* h, const float* x, long long n, int dim, float* norms, void* stream);
/* top-k gallery rows of every probe.  query[Q][dim], gallery[G][dim], gallery_norms[G] (ffr_row_norms of the gallery,
 * computed once at enrolment); the probe norms are computed per call.                                                */
int ffr_search_topk(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                    long long G, int dim, int k, long long index_base,
                    float* top_score, int64_t* top_index, void* stream);
/* Merge S sorted lists per probe (score[S][Q][k], index[S][Q][k], e.g. one per rank of a sharded search) into one
 * [Q][k] list in the same total order; slots with index < 0 are padding.  1 <= S <= 4096, 1 <= k <= 128, Q >= 1.     */
int ffr_topk_merge(ffr_handle* h, const float* score, const int64_t* index, int S, int Q, int k,
                   float* out_score, int64_t* out_index, void* stream);

/* ---- subject-labelled search (top-k identities in one pass, and removal) ----------------------------------------------
 * An enrolled person is several gallery rows (images, a template, re-enrolments).  gallery_subject[G] (int32, device, 4-byte
 * aligned) names the subject of every row: a value >= 0 is the subject the row belongs to; a value < 0 marks a REMOVED row,
 * which is still read but is never a candidate and never appears in a result.
 *   order  fix a probe q; s(q, g) is the score of ffr_search_topk, bit for bit.  Row g comes before row g' iff
 *          s(q, g) > s(q, g'), or the scores are equal and g < g'.
 *   rows   distinct = 0: the first k live rows in that order, 1 <= k <= 128.  With no removed row top_score and top_index
 *          are those of ffr_search_topk, bit for bit.
 *   identities  distinct = 1: best(u) is the first row of subject u in that order; the result is the first k of {best(u)},
 *          1 <= k <= 64.  Every listed subject appears once, with its maximum score and the smallest index among the rows
 *          that reach it.  The cap is the search block's LDS (160 KiB per CU, one block per CU): the block needs
 *          71 424 + 512 k bytes to list rows and 20 480 + 256 k more to carry subjects -- 141 056 at k = 64, 190 208 at
 *          k = 128.
 *   result top_score[Q][k] fp32, top_index[Q][k] int64 (= index_base + gallery row), top_subject[Q][k] int32.  Slots beyond
 *          the live rows (or subjects) hold (-inf, -1, -1).  G = 0 gives all padding.
 *   shards searching contiguous shards (each with its index_base) and merging with ffr_topk_merge_subjects equals one
 *          search, in both modes.  Identity mode: let u be in the global top k with best(u) in shard c.  Every subject that
 *          beats u inside c does so with a row of c, so it beats u globally too; fewer than k do, and u is on c's list with
 *          its global score and index.  Other shards may list u with a worse row; the merge keeps the first entry of a
 *          subject and drops the later ones.  A subject outside the global top k is beaten by k subjects whose best rows
 *          are all listed, so it cannot be emitted among the first k.
 *   bitwise, memory, graphs: every guarantee of ffr_search_topk carries over -- results do not depend on Q, on the chunking
 *          or on the sharding; no host synchronisation; the search scratch (probe norms, per-chunk lists with a subject
 *          plane) grows on demand and is reused, so a call can be captured into a hipGraph once it has run at that shape.
 * Errors are those of ffr_search_topk, and FFR_ERR_ARG for a NULL gallery_subject when G > 0, a gallery_subject that is not
 * 4-byte aligned, a NULL top_subject, distinct outside {0, 1}, and k > 64 with distinct = 1.
 * Profiled as one launch under FFR_KC_SCORE with flops = 2*Q*G*512.                                                      */
int ffr_search_topk_subjects(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                             const int32_t* gallery_subject, long long G, int dim, int k, long long index_base,
                             int distinct, float* top_score, int64_t* top_index, int32_t* top_subject, void* stream);
/* Filtered 1:N search: the subject search under a per-probe filter, one call for a batch of probes that may each see
 * another part of the gallery (a camera's watchlists, a tenant's enrolments, the people cleared for a door).
 * gallery_tag[G] is one 32-bit word per enrolled row and query_mask[Q] one per probe (uint32, device, 4-byte aligned).
 *   admissible  row g is admissible for probe q iff (gallery_tag[g] & query_mask[q]) != 0 and (gallery_subject == NULL or
 *          gallery_subject[g] >= 0).  A row with tag 0 is admissible for nobody, a probe with mask 0 gets k slots of
 *          padding, and bit 31 is a bit like any other: the words are unsigned.
 *   result for every probe q, bit for bit what ffr_search_topk_subjects gives that probe, with the same distinct, over the
 *          gallery in which every row inadmissible for q is marked removed: scores, indices, subjects, the tie order and
 *          the (-inf, -1, -1) padding.  With gallery_subject == NULL only distinct = 0 is legal, the result is that of
 *          ffr_search_topk over the admissible rows with their original indices, and top_subject (NULL then, as it is NULL
 *          iff gallery_subject is) is not touched.  Limits as above: k <= 128 rows, k <= 64 identities, dim = 512.
 *   bitwise  a (q, g) score is the same MFMA chain wherever it is computed, so row q of a Q-probe call equals the 1-probe
 *          call with query_mask[q], results do not depend on the chunking, and contiguous shards searched with their
 *          index_base and merged by ffr_topk_merge / ffr_topk_merge_subjects equal one search: the lists hold admissible
 *          rows only, so the merges need not know the filter.  The identity-mode shard argument above holds per probe, with
 *          "rows" read as "rows admissible for this probe": best(u) is the first ADMISSIBLE row of u, in every shard and
 *          globally, and nothing in the argument compares rows of two probes.
 *   cost   every row is still read and scored; the filter costs 4 G + 4 Q bytes more than the subject search.  When a filter
 *          is fixed for long and admits a small share of the gallery, a second gallery of those rows is searched faster.
 *   memory no host synchronisation; the scratch is the search scratch of the handle, so a call can be captured into a
 *          hipGraph once it has run at that shape.
 * Errors are those of ffr_search_topk_subjects (G = 0 gives all padding), and FFR_ERR_ARG for a NULL query_mask, a NULL
 * gallery_tag when G > 0, either of them not 4-byte aligned, distinct = 1 with a NULL gallery_subject, and a NULL top_subject
 * with a non-NULL gallery_subject (or the reverse when G > 0).
 * Profiled as one launch under FFR_KC_SCORE with flops = 2*Q*G*512.                                                      */
int ffr_search_topk_filtered(ffr_handle* h, const float* query, const uint32_t* query_mask, int Q, const float* gallery,
                             const float* gallery_norms, const uint32_t* gallery_tag,
                             const int32_t* gallery_subject /* may be NULL */, long long G, int dim, int k, long long index_base,
                             int distinct, float* top_score, int64_t* top_index,
                             int32_t* top_subject /* NULL iff gallery_subject is NULL */, void* stream);
/* ffr_topk_merge with a subject per entry (subject[S][Q][k]); distinct = 1 keeps the first entry of every subject and
 * needs k <= 64.  Slots with index < 0 are padding.                                                                       */
int ffr_topk_merge_subjects(ffr_handle* h, const float* score, const int64_t* index, const int32_t* subject, int S, int Q,
                            int k, int distinct, float* out_score, int64_t* out_index, int32_t* out_subject, void* stream);

/* ---- certified bf16 shortlist search -------------------------------------------------------------------------------------
 * ffr_search_topk_coarse gives the outputs of ffr_search_topk, bit for bit, for every input without NaN/inf; only the way
 * there differs.  The pass over the whole gallery runs on the bf16 matrix cores over a plane of half the bytes and picks a
 * shortlist; the fp32 arithmetic of ffr_search_topk scores the shortlist; a proven bound certifies, per probe, that the
 * shortlist holds the true top-k, and a probe without that certificate is searched exactly.  No approximate mode.
 *   plane  gallery_plane[G][512] holds bf16(g / |g|) (round to nearest even, uint16_t at this boundary), |g| the norm of
 *          ffr_row_norms: 1 KB per enrolled row beside the 2 KB fp32 row, which stays.  ffr_coarse_pack writes it for the
 *          rows it is given (the rows an enrolment appends; a plane is the same however it was pieced together).
 *   bound  the probe is split into two bf16 planes q / |q| = hi + lo.  With u = 2^-8 (bf16 unit round-off) Cauchy-Schwarz
 *          gives |sum (hi + lo) g^ - cos(q, g)| <= u + u^2 + u^3; 2^-13 is allowed for accumulating the 1024 exact products
 *          in the matrix core (assumed, 8 x a plain fp32 chain: the core's rounding is undocumented and no test can observe
 *          c); the coarse score c = (sum (hi + lo) g^) |q||g| / (|q||g| + 1e-8) uses the norms of the exact
 *          score s, itself within 1e-6 of the cosine.  |c - s| <= 0.00405 < FFR_COARSE_EPS = 2^-8 + 2^-12.
 *   certificate  the pass keeps the k' = min(128, max(2k, 32)) best rows of a probe by (descending c, ascending index),
 *          c_1 >= ... >= c_k', and they are scored exactly; s_k is the k-th best of them in the order of ffr_search_topk.
 *          The probe is certified iff G <= k' or c_k' + FFR_COARSE_EPS < s_k (strictly: no row left out can even tie the
 *          k-th); its answer is the top k of the re-scored shortlist.  Otherwise its answer comes from the exact search.
 *   unsafe a norm that is not zero and outside [2^-60, 2^60], or not finite, is unsafe (its sum of squares under- or
 *          overflowed), and so is a zero norm over a row that is not all zeros (every square underflowed).  ffr_coarse_pack
 *          ORs 1 into *plane_flag (device int, zeroed by the caller at creation, sticky) when it meets such a row; while
 *          the flag is set no probe is certified.  A probe with an unsafe norm is not certified.
 *          A zero row packs to zeros and is safe.
 *   k      the pass serves k <= 64; for 64 < k <= 128 (and for G = 0) the exact search runs alone and every probe is reported
 *          uncertified.
 * Arguments and error codes are those of ffr_search_topk; the plane must be 16-byte aligned and, like the gallery, may be
 * NULL only when G = 0 (plane_flag likewise).  certified[Q] (device, 1 = the certificate held, 0 = searched exactly) may be
 * NULL.  No host synchronisation: the exact pass over the uncertified probes is always launched and leaves at once where a
 * device count says there is nothing to do, so a call can be captured into a hipGraph once it has run at that shape.
 * Profiled under FFR_KC_SCORE; a coarse search counts flops = 2*Q*G*512, the scores it ranks.                          */
#define FFR_COARSE_EPS (0.00390625f + 0.000244140625f)
int ffr_coarse_pack(ffr_handle* h, const float* rows, const float* norms, long long n, int dim,
                    uint16_t* plane, int* plane_flag, void* stream);
int ffr_search_topk_coarse(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                           const uint16_t* gallery_plane, const int* plane_flag, long long G, int dim, int k,
                           long long index_base, float* top_score, int64_t* top_index, int* certified, void* stream);
/* The shortlist search of a subject-labelled gallery: the outputs of ffr_search_topk_subjects with the same arguments, bit
 * for bit, for every input without NaN/inf, every removal pattern and both modes.
 *   method the pass over the plane ranks ROWS in both modes and skips the removed ones (gallery_subject < 0): per probe the
 *          k' best live rows by (descending c, ascending index).  It never merges subjects.  The k' rows are scored exactly,
 *          subject[row] is read again, and identities are formed on those <= 128 entries: in the order of
 *          ffr_search_topk_subjects an entry is ALIVE iff no other entry of its subject comes before it; the answer of
 *          distinct = 1 is the first k alive entries, s_k the score of the k-th.  distinct = 0 lists the first k entries.
 *   k'     distinct = 0: min(128, max(2k, 32)), k <= 64, as ffr_search_topk_coarse.  distinct = 1: min(128, max(4k, 64)),
 *          k <= 32 -- the rows of one person crowd the head of the list (about 8 of them where a person has 8), and at 2k
 *          the k-th identity falls off the list too often to be worth the pass.  For larger k (distinct = 0: 64 < k <= 128,
 *          distinct = 1: 32 < k <= 64) and for G = 0 ffr_search_topk_subjects runs alone and every probe is reported
 *          uncertified.
 *   certificate  L is the shortlist, c_1 >= ... >= c_k' its coarse scores.  Every live row outside L has c <= c_k', hence
 *          s <= c_k' + FFR_COARSE_EPS.  The probe is certified iff the plane flag is clear, its norm is safe, and either L
 *          holds fewer than k' rows or G <= k' (then L is every live row: with removals G > k' no longer means a full list), or
 *          (distinct = 1) at least k entries are alive, and c_k' + FFR_COARSE_EPS < s_k, strictly; distinct = 0 takes the
 *          k-th entry for the k-th alive one.
 *          Identities: let u be one of the first k alive entries.  Its alive entry scores >= s_k > every row outside L, so no
 *          row of u outside L beats or ties it: it is best(u) over the whole gallery.  A subject v that is not among them
 *          has its best row in L behind the k-th alive entry, or no row in L, and then best(v) < s_k.  So the first k of
 *          {best(u)} over the gallery are the first k alive entries of L, scores and indices included.  A full shortlist
 *          with fewer than k alive entries is NOT certified -- more subjects may lie outside (one person enrolled with more
 *          rows than the list holds).
 *   exact  the probes without a certificate are gathered and searched by the kernels of ffr_search_topk_subjects, which take
 *          the device count of such probes; always launched, sized for Q, no host synchronisation: the call can be captured
 *          into a hipGraph once it has run at that shape.  Scratch comes from the handle's search arena.
 * Arguments and error codes are the union of ffr_search_topk_coarse and ffr_search_topk_subjects: FFR_ERR_ARG for k > 64
 * with distinct = 1, distinct outside {0, 1}, rows or plane not 16-byte aligned, subjects not 4-byte aligned, a NULL output,
 * and a NULL gallery pointer (rows, norms, plane, flag, subjects) unless G = 0; FFR_ERR_UNSUPPORTED for dim != 512.
 * certified[Q] may be NULL.  Profiled as one launch under FFR_KC_SCORE with flops = 2*Q*G*512.                          */
int ffr_search_topk_coarse_subjects(ffr_handle* h, const float* query, int Q, const float* gallery, const float* gallery_norms,
                                    const uint16_t* gallery_plane, const int* plane_flag, const int32_t* gallery_subject,
                                    long long G, int dim, int k, long long index_base, int distinct, float* top_score,
                                    int64_t* top_index, int32_t* top_subject, int* certified, void* stream);
/* The shortlist search under a per-probe filter: the outputs of ffr_search_topk_filtered with the same arguments, bit for bit,
 * for every input without NaN/inf, with and without subjects, both modes, every removal pattern and every tag and mask pattern.
 * No approximate mode; certified[Q] says which way each probe went.
 *   method as ffr_search_topk_coarse_subjects, with "live row" read as "row admissible for this probe" (admissible: see
 *          ffr_search_topk_filtered).  The pass over the plane ranks ROWS in both modes, per probe the k' best admissible rows
 *          by (descending c, ascending index), and never merges subjects.  Every listed row is admissible, so the exact
 *          re-score reads no tags; identities are formed on the <= 128 entries as there.  k' and the k limits are the same:
 *          64 rows, 32 identities; above them, and at G = 0, ffr_search_topk_filtered runs alone and certified is all 0.
 *   certificate  L is the k' best admissible rows of the probe, c_1 >= ... >= c_k'.  Every admissible row outside L has
 *          c <= c_k', hence s <= c_k' + FFR_COARSE_EPS (the bound is about one (q, g) pair and knows no filter).  The probe
 *          is certified iff the plane flag is clear, its norm is safe, and either L holds fewer than k' rows or G <= k' (then L
 *          is every admissible row of this probe: under a filter G > k' does not mean a full list), or (distinct = 1) at least
 *          k entries are alive, and c_k' + FFR_COARSE_EPS < s_k, strictly.  The identity proof above holds unchanged: a person
 *          speaks with the best row the probe may see, best(u) and "a row outside L" range over the rows admissible for this
 *          one probe, and nothing in the proof compares rows of two probes.  A probe with mask 0 has an empty shortlist: it
 *          is certified and gets k slots of padding, as the exact filtered search gives it.
 *   exact  the probes without a certificate are gathered WITH their mask words and searched by the kernels of
 *          ffr_search_topk_filtered under the device count; always launched, sized for Q, no host synchronisation: the call
 *          can be captured into a hipGraph once it has run at that shape.  Scratch comes from the handle's search arena.
 *   cost   the pass reads the 1 KB plane row where the exact filtered search reads the 2 KB fp32 row, 4 G + 4 Q bytes more
 *          than ffr_search_topk_coarse_subjects; every row is still read and scored.
 * Arguments and error codes are the union of ffr_search_topk_filtered and ffr_search_topk_coarse_subjects; the plane and its
 * flag, like the rest of the gallery side, may be NULL only when G = 0 (all padding).  certified[Q] may be NULL.
 * Profiled as one launch under FFR_KC_SCORE with flops = 2*Q*G*512.                                                      */
int ffr_search_topk_coarse_filtered(ffr_handle* h, const float* query, const uint32_t* query_mask, int Q, const float* gallery,
                                    const float* gallery_norms, const uint16_t* gallery_plane, const int* plane_flag,
                                    const uint32_t* gallery_tag, const int32_t* gallery_subject /* may be NULL */, long long G,
                                    int dim, int k, long long index_base, int distinct, float* top_score, int64_t* top_index,
                                    int32_t* top_subject /* NULL iff gallery_subject is NULL */, int* certified /* may be NULL */,
                                    void* stream);

/* ---- clustering (unlabelled embeddings -> identities -> one template per identity) ----------------------------------
 * The step in front of enrolment: N unlabelled faces are grouped by single-link clustering at one cosine threshold, and
 * each group is fused into one template row.  The N x N scores never leave the chip; the output is one label per row.
 *   edge   rows i < j are joined iff s(probe = i, gallery row = j) > threshold -- the strict > of the verification
 *          protocol -- with s exactly the fp32 score ffr_search_topk gives for probe i and gallery row j (bit for bit).
 *          The diagonal and i > j are never evaluated.  A zero row scores 0 against everything: it stays alone for any
 *          threshold >= 0.  Clusters are the connected components of the edges (transitive closure).
 *   result rep[N] int64: rep[i] = the SMALLEST row index of i's cluster (so rep[i] <= i, rep[rep[i]] == rep[i], and two rows
 *          share a cluster iff their rep is equal).  The result does not depend on the order in which the device meets
 *          the edges: repeated calls are bitwise equal.
 *   how    a lock-free union-find over parent[N] in the handle's scratch: find walks parent[] to a root; two different
 *          roots are united by atomicCAS(&parent[larger], larger, smaller); on failure the walk continues from the value
 *          the CAS returned.  Termination: parent[x] <= x holds at every instant (a root is only ever re-pointed to a
 *          smaller index), so every walk strictly descends and ends within N hops whatever other waves do, and the larger
 *          root of a retried union strictly decreases: no lock, no spinning, no wait on another wave.  Only roots are
 *          hooked, always under a smaller index, so each finished cluster has one root, its smallest row.
 *   shapes dim = 512 only (FFR_ERR_UNSUPPORTED otherwise).  FFR_ERR_ARG: N < 0 or N >= 2^31, a NaN threshold, a null emb or
 *          rep, emb not 16-byte aligned.  norms[N] = ffr_row_norms(emb), or NULL: computed into the scratch.  N = 0 (and
 *          C = 0 below) succeeds and touches nothing.
 *   memory no host synchronisation; the scratch (norms, parent) grows on demand -- hipMalloc on the first call at a larger
 *          N, which bumps ffr_generation -- so a call can be captured into a hipGraph once it has run at that N.
 *   NaN    rows holding NaN or inf give unspecified (in-bounds) labels.
 * No weights need to be loaded.  Profiled under FFR_KC_SCORE; a clustering counts flops = N*(N-1)*512.               */
int ffr_cluster_threshold(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                          int64_t* rep, void* stream);
/* One template per cluster: templates[c] = t / |t| with t = sum over r of emb[r] / |emb[r]|, r running through
 * order[offsets[c]] .. order[offsets[c+1] - 1] in that sequence (sequential fp32 per component: deterministic, bitwise
 * repeatable).  A zero row contributes zero; an all-zero sum gives a zero template.  order[] holds row indices of emb
 * (int64; for a clustering: the rows sorted by cluster, then by index), offsets[C + 1] is ascending (int64); both are
 * trusted, the caller keeps them in bounds.  norms: ffr_row_norms(emb) or NULL (computed per row, the same values).
 * templates[C][dim] fp32, 16-byte aligned.  Errors as above (C in place of N).                                        */
int ffr_cluster_templates(ffr_handle* h, const float* emb, const float* norms, const int64_t* order, const int64_t* offsets,
                          long long C, int dim, float* templates, void* stream);
/* Extend a clustering by new rows, equal to clustering everything.  emb[N][dim] holds ALL rows, the earlier ones first;
 * the rows [N_old, N) are new.  norms[N] or NULL as above.
 *   prior  prior[N] int64, a labelling in representative form: prior[i] <= i names a row already known to belong with i.
 *          For a row clustered before it is the earlier rep; for a new row it is the row itself, or an earlier row it must
 *          be linked to whatever it scores (a frame of the same track).
 *   scored exactly the pairs i < j with j >= N_old: the N_old x (N - N_old) rectangle plus the triangle among the new
 *          rows.  Roles, score bits and the strict > are those of ffr_cluster_threshold: the smaller index is the probe.
 *   result rep[N] int64 (rep == prior, in place, is allowed): rep[i] = the smallest row of i's connected component under
 *          (links i - prior[i]) + (scored edges).  So rep[i] <= the root of i in prior <= i, rep[rep[i]] == rep[i], and the
 *          labels of OLD rows change where a new row bridges two old clusters.  The components of an edge set do not depend
 *          on the order in which the edges are met: repeated calls are bitwise equal, and
 *          (a) if prior[:N_old] is ffr_cluster_threshold of the first N_old rows at this threshold and prior[j] = j for the
 *              new j, rep equals ffr_cluster_threshold over all N rows, bit for bit -- also batch after batch;
 *          (b) N_old = N scores nothing and returns the flattened prior (rep[i] = the root of i);
 *          (c) N_old = 0 is a full clustering under must-links.
 *   guard  an entry of prior outside [0, i] is read as i: the row starts alone.  The termination argument above rests on
 *          parent[x] <= x, and the seed is the only place where caller data reaches parent[], so it makes that true whatever
 *          it is given.  Deep priors (a chain prior[i] = i - 1) are legal but walked hop by hop, without compression: pass
 *          flattened labels (the rep of an earlier call is flat).
 *   errors as ffr_cluster_threshold; FFR_ERR_ARG also for N_old < 0, N_old > N, and a null or not 8-byte-aligned prior when
 *          N > 0.  N = 0 succeeds and touches nothing.
 *   memory no host synchronisation; the scratch of ffr_cluster_threshold (norms, parent) is shared, grows and bumps
 *          ffr_generation under the same rule; the two calls may alternate freely on one handle.
 * Profiled as one launch under FFR_KC_SCORE with flops = 512 * (2 * N_old * N_new + N_new * (N_new - 1)), N_new = N - N_old. */
int ffr_cluster_extend(ffr_handle* h, const float* emb, const float* norms, long long N_old, long long N, int dim,
                       float threshold, const int64_t* prior, int64_t* rep, void* stream);
/* Remove rows from a single-link clustering, equal to clustering the rest.  emb[N][dim], norms[N] or NULL: as in
 * ffr_cluster_threshold.  All labels use the caller's row numbering: nothing is moved, the caller compacts afterwards if it
 * wants to.  keep[N] uint8: keep[x] != 0 means row x survives.  (Removal from a density-gated clustering is a different
 * problem -- degrees fall, core rows are demoted, border rows choose again: ffr_cluster_density_remove below.)
 *   labels g(x) = rep_in[x] if 0 <= rep_in[x] <= x, else x: the guard of ffr_cluster_extend.  A label r is HIT iff some
 *          removed row d has g(d) == r; a surviving row x is AFFECTED iff g(x) is hit.
 *   result rep[N] int64.  A removed row: -1.  An unaffected survivor: g(x) -- a cluster that loses no row keeps its label; it
 *          had no edge to any other cluster, and removing rows adds none.  An affected survivor: the smallest row of x's
 *          connected component, among the affected survivors only, under
 *            the scored edges: a < b, both affected survivors, s(probe = a, gallery row = b) > threshold; score bits, roles
 *              and the strict > are those of ffr_cluster_threshold;
 *            the links x - prior[x], where prior is not NULL, 0 <= prior[x] <= x, and both ends are affected survivors:
 *              the must-links that outlive the removal.
 *   scored exactly the pairs of affected survivors, m (m - 1) / 2 of them; no pair with an unaffected or a removed row.
 *          With identities of a few rows that is a few thousand rows where a handful is removed, not N.
 *          (a) If rep_in is ffr_cluster_threshold of all N rows at this threshold, or the result of ffr_cluster_extend batch
 *              after batch, and prior is NULL, then rep on the survivors is ffr_cluster_threshold over the survivors alone,
 *              bit for bit once both are put in the same numbering: dropping the removed rows renumbers monotonically, so
 *              "the smallest row" and "the smaller index is the probe" carry over.  With must-links, prior must name for each
 *              row the first SURVIVING row of its tie group; the result then equals ffr_cluster_extend(N_old = 0) over the
 *              survivors with that prior.
 *          (b) Nothing removed: rep[x] = g(x), and no pair is scored.
 *          (c) Everything removed: all labels are -1.
 *          (d) rep == rep_in, in place, is allowed.
 *          (e) Repeated calls are bitwise equal: the result does not depend on the order in which the device lists the rows
 *              or meets the edges.  (The device may score a pair with the roles exchanged; the bits are the same.)
 *          (f) A surviving row's rep may RISE here, the one place in single link where it can: when the representative
 *              itself is removed, or the cluster splits.
 *   guard  whatever rep_in, prior and keep hold, every index stays in [0, N) and every walk ends: the union-find is seeded
 *          with parent[x] = x, or a prior[x] in [0, x] that is itself an affected survivor.
 *   errors as ffr_cluster_threshold; FFR_ERR_ARG also for a null rep_in or keep when N > 0 and for rep_in or prior not 8-byte
 *          aligned.  N = 0 succeeds and touches nothing.
 *   memory no host synchronisation (m stays on the device); the scratch is carved from the clustering arena (norms, parent,
 *          the guarded labels, the hit flags, the list and its count: 20 bytes per row), grows on demand and bumps
 *          ffr_generation under the same rule; the call may alternate freely with the other clustering calls on one handle.
 * Profiled as one launch under FFR_KC_SCORE with flops = 0: the pair count is known on the device only.  A caller that wants
 * a rate computes m from rep_in and keep (the survivors whose label is hit) and uses 512 * m * (m - 1).               */
int ffr_cluster_remove(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                       const int64_t* rep_in, const int64_t* prior, const uint8_t* keep, int64_t* rep, void* stream);
/* Density-gated clustering (DBSCAN over the edge set of ffr_cluster_threshold): a row links clusters only if enough rows
 * lie within the threshold of it.  Single link lets a few in-between rows (a blurred frame, a look-alike) join two people
 * into one cluster; here such sparse rows may attach to a cluster but never connect two, and isolated rows are reported.
 *   edges  exactly those of ffr_cluster_threshold: rows i < j are adjacent iff s(probe = i, gallery row = j) > threshold
 *          (strict), s with the fp32 bits ffr_search_topk returns for that pair; each pair is scored once, in that
 *          orientation, the diagonal never.
 *   degree degree[i] = the number of edges touching i.  Row i is CORE iff degree[i] + 1 >= min_rows (the row counts itself).
 *   core   clusters are the connected components of the edges whose two end points are both core.
 *   border a non-core row with at least one core neighbour joins the cluster of the core neighbour with the highest score
 *          (scores compared as fp32 values; equal scores: the smallest row index).  It never links two clusters.
 *   noise  a non-core row with no core neighbour is a cluster of its own.
 *   result rep[N] int64: rep[i] = the smallest row index among ALL members of i's cluster, core and border together (a
 *          border row can carry a smaller index than every core row of its cluster).  As for ffr_cluster_threshold,
 *          rep[rep[i]] == rep[i] and two rows share a cluster iff their rep is equal.  kind[N] uint8: 2 core, 1 border,
 *          0 noise.  degree[N] int32, or NULL when not wanted.  Every rule above is independent of the order in which the
 *          device meets the edges: repeated calls are bitwise equal.
 *   1, 2   at min_rows = 1 every row is core, at min_rows = 2 exactly the rows with a neighbour: in both cases rep equals
 *          ffr_cluster_threshold's rep bit for bit (computed by the passes below, not by the other call).
 *   how    the triangle of pairs is walked twice by the tile of ffr_cluster_threshold.  Pass 1 adds up degree[] with
 *          integer atomic adds (they commute).  Pass 2 unites core-core edges in the lock-free union-find described above,
 *          under the same termination argument, and for an edge between a core row c and a non-core row x raises best[x]
 *          to (order-preserving bits of s) << 32 | (0xFFFFFFFF - c) with one 64-bit atomic max.  Three N-sized kernels
 *          then take each row's root, the smallest member per root and the labels.  No step waits on another wave.
 *   errors dim = 512 only (FFR_ERR_UNSUPPORTED otherwise).  FFR_ERR_ARG: N < 0 or N >= 2^31, a NaN threshold, min_rows < 1,
 *          a null emb, rep or kind, emb not 16-byte aligned (rep 8, degree and norms 4).  norms as above.  N = 0 succeeds
 *          and touches nothing.
 *   memory no host synchronisation; the scratch is the one of ffr_cluster_threshold (norms, parent) plus degree, root,
 *          minrow and best, 24 bytes per row, and grows and bumps ffr_generation under the same rule.
 * Profiled as one launch under FFR_KC_SCORE with flops = 2*N*(N-1)*512: the triangle is walked twice.  A collection that
 * grows is extended with ffr_cluster_density_extend below.                                                            */
int ffr_cluster_density(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold, int min_rows,
                        int64_t* rep, uint8_t* kind, int32_t* degree, void* stream);
/* Extend a density-gated clustering by new rows, equal to ffr_cluster_density over all rows.  emb[N][dim] holds ALL rows,
 * the earlier ones first; the rows [N_old, N) are new.  norms[N] or NULL as above.
 *   state  kept by the caller between calls, per row: rep[N] int64, degree[N] int32 and best[N] uint64, all three in and
 *          out: the first N_old entries are read, all N are written.  best[i] is the key by which a border row chose its
 *          cluster, (order-preserving bits of the score) << 32 | (0xFFFFFFFF - core row), and 0 for a core or a noise row.
 *          kind[N] uint8 is out only.  The state is valid ONLY for the threshold and the min_rows it was made with.
 *   equal  if (rep, degree, best)[:N_old] is the state this call left for the first N_old rows at this threshold and
 *          min_rows, then rep, kind and degree equal ffr_cluster_density over all N rows bit for bit, and best is bit for
 *          bit the state a call from scratch (N_old = 0) over the N rows leaves -- so it holds batch after batch.
 *          N_old = 0 is the clustering from scratch and produces the state.  N_old = N scores nothing and returns the same
 *          labels.  Unlike ffr_cluster_extend, the rep of an OLD row may also rise: a border row may move to a better core
 *          row of another cluster, and if it was the smallest member, the cluster it left is named by a larger row.
 *   scored the pairs i < j with j >= N_old, twice (degrees, then the gated join, as ffr_cluster_density walks the triangle),
 *          then the pairs of old rows of which one was made core by the new rows: new rows can turn old rows into cores,
 *          and the old edges at those must be treated again.  Their number m is found on the device; nothing is read back.
 *   guard  the kernels read a rep[i] outside [0, i] as "row i starts alone", a negative degree as 0, and a key that names
 *          a row >= N_old, or a row that is not core by the degrees passed, as 0: whatever is passed, every index stays
 *          in [0, N) and every walk ends.  A state that is in range but wrong gives labels with rep[rep[i]] == rep[i] and
 *          nothing more.
 *   errors as ffr_cluster_density and ffr_cluster_extend: FFR_ERR_ARG for N outside [0, 2^31), N_old outside [0, N], a NaN
 *          threshold, min_rows < 1, a null emb, rep, kind, degree or best when N > 0, emb not 16-byte aligned (rep and best
 *          8, degree and norms 4); FFR_ERR_UNSUPPORTED for dim != 512 or a grid over the limit.  N = 0 succeeds and touches
 *          nothing.
 *   memory no host synchronisation; the scratch is shared with the other clustering calls (norms, parent, root, minrow, the
 *          old degrees, one minimum per rep, the list of promoted rows and its count) and grows under the same rule.
 * Profiled as one launch under FFR_KC_SCORE with flops = 512 * (2 * (2 * N_old * N_new + N_new * (N_new - 1)) + 2 * N_old^2),
 * an upper bound: the last term stands for 2 * m * N_old with m <= N_old.                                              */
int ffr_cluster_density_extend(ffr_handle* h, const float* emb, const float* norms, long long N_old, long long N, int dim,
                               float threshold, int min_rows, int64_t* rep, uint8_t* kind, int32_t* degree,
                               unsigned long long* best, void* stream);
/* Remove rows from a density-gated clustering, equal to ffr_cluster_density over the rest.  emb[N][dim], norms[N] or NULL as
 * above; keep[N] uint8, keep[x] != 0 means row x survives.  Nothing moves: all labels stay in the caller's numbering, as in
 * ffr_cluster_remove.
 *   state  rep[N] int64, degree[N] int32 and best[N] uint64, in and out: what ffr_cluster_density_extend leaves for all N rows
 *          at this threshold and min_rows.  kind[N] uint8 is out only.
 *   equal  let kept be the surviving rows in ascending order and o2n the monotone renumbering they define.  On the survivors
 *          o2n[rep], kind and degree equal ffr_cluster_density over emb[kept] bit for bit, and best, with its low word
 *          (0xFFFFFFFF - core row) re-encoded through o2n and its high word (the score bits) untouched, is bit for bit the
 *          state ffr_cluster_density_extend(N_old = 0) leaves over emb[kept].  So extensions and removals interleave freely.
 *          A removed row gets rep = -1, kind = 0, degree = 0, best = 0.  Nothing removed: the state comes back unchanged and
 *          no pair is scored.  Everything removed: every rep is -1.  min_rows = 1: rep equals ffr_cluster_remove on the same
 *          rep and keep bit for bit.  A surviving row's rep may rise, and a border row may move to another cluster.  Repeated
 *          calls are bitwise equal.
 *   how    need = min_rows - 1; g(x) = rep[x] if 0 <= rep[x] <= x, else x.
 *          (1) the removed rows are listed, r of them, and scored against all rows: a surviving row loses one from its degree
 *              per removed neighbour (r * N pairs).  Degrees count all neighbours, so a demotion does not cascade.
 *          (2) a row that was core (old degree >= need) and is removed or no longer core is LOST; a label is HIT iff g of
 *              a lost row names it.  Removing a border or a noise row hits nothing.
 *          (3) the m still-core rows of hit labels start alone and are joined again among themselves, m (m - 1) / 2 pairs as in
 *              ffr_cluster_remove; a core row of an unhit label hangs under the smallest core row with its rep: in an unhit
 *              cluster every core row survived and stayed core.
 *          (4) a non-core survivor keeps its key iff the key's core row survives and is still core (a maximum over a set that
 *              shrank but still holds its maximum).  The q others -- every demoted row, every border row whose chosen core row
 *              was lost -- start from key 0 and are offered every surviving core row adjacent to them (q * N pairs) with the
 *              one 64-bit atomic max of ffr_cluster_density.  A noise row stays noise.
 *          (5) root, smallest member and labels as in ffr_cluster_density, over the survivors.
 *          Pairs may be scored with the roles exchanged; the bits are the same.
 *   guard  a key is dropped and looked for again when it names a row >= N, a removed row, or a row that is not core by the
 *          new degrees; a rep outside [0, x] means "x alone"; a negative degree reads as 0.  Whatever is passed, every index
 *          stays in [0, N) and every walk ends.  A state in range but wrong gives rep[rep[i]] == rep[i] on the survivors and
 *          nothing more.
 *   errors as ffr_cluster_density_extend (without N_old), plus FFR_ERR_ARG for a null keep when N > 0.  N = 0 succeeds and
 *          touches nothing.
 *   memory no host synchronisation: r, m and q stay on the device.  The scratch is carved from the clustering arena (norms,
 *          nine ints per row and three counts) and grows and bumps ffr_generation under the same rule.
 * Profiled as one launch under FFR_KC_SCORE with flops = 0: the pair counts are known on the device only.  The call scores
 * at least r * N pairs where clustering the N_s survivors again scores N_s (N_s - 1): with half of the rows leaving, clustering
 * again is the cheaper way to the same state (ffr_cluster_density_extend with N_old = 0 over the compacted rows).        */
int ffr_cluster_density_remove(ffr_handle* h, const float* emb, const float* norms, long long N, int dim, float threshold,
                               int min_rows, const uint8_t* keep, int64_t* rep, uint8_t* kind, int32_t* degree,
                               unsigned long long* best, void* stream);

/* ---- face alignment (landmarks -> similarity transform -> aligned uint8 crop) ---------------------------------------
 * Replaces the reference's host preprocessing, lfw/gen_lfw112x96.py:6-17 (align) with lfw/matlab_cp2tform.py
 * (get_similarity_transform_for_cv2) in front of cv2.warpAffine: frames and detector landmarks already on the device
 * become the crops ffr_embed_u8 reads, without a host round trip.
 *   fit    landmarks[N][K][2] and tmpl[K][2] are fp32 (x, y) points, 2 <= K <= 16: s = the face's landmarks in its
 *          frame, r = the template points in the crop.  In fp64, with p = r - mean(r), q = s - mean(s), den = sum |p|^2:
 *          a = sum(p . q) / den, b = sum(p.x q.y - p.y q.x) / den, A1 = [a -b tx; b a ty], t = mean(s) - L mean(r) -- the
 *          least squares of the map crop -> frame that findNonreflectiveSimilarity solves (cv2's matrix is its inverse).
 *          The reflective candidate A2 is the same fit with r.x negated and the first column of the result negated.  The
 *          landmarks mapped through each candidate's inverse are compared with r; the non-reflective candidate wins when
 *          the L2 norm of its residual is <= the other's (findSimilarity); a candidate whose linear part is exactly
 *          singular counts as an infinite norm.
 *   A      A[N][6] fp64, row-major 2 x 3, maps crop pixel (x, y) to frame coordinates (dst -> src: the inverse of the
 *          matrix the reference hands to cv2.warpAffine).
 *   valid  valid[N] uint8.  den == 0, both candidates singular (all landmarks equal) or anything not finite -- where the
 *          reference raises -- gives valid = 0 and A = 0; nothing faults.
 *   warp   frames[F][H][W][3] uint8 HWC with pitch_bytes between rows (frame f starts at f * pitch_bytes * H);
 *          frame_index[N] int32 names each face's frame (faces may share one).  crop[N][out_h][out_w][3] uint8,
 *          contiguous: the input of ffr_embed_u8 at 112 x 112.  Output pixel (x, y) samples
 *            sx = (A0 x + A1 y) + A2, sy = (A3 x + A4 y) + A5   in fp64, in this order, without fused multiply-add,
 *                                                               clamped to +-2^20;
 *            fx = (int)floor(sx * 32 + 0.5), ix = fx >> 5, ax = fx & 31 (the same for y): a 1/32-pixel grid;
 *            v  = (sum over the 4 taps of w p + 512) >> 10 per channel, w = (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay;
 *          a tap outside [0,W) x [0,H) contributes 0, decided per tap (constant-0 border).  An exact integer rule in
 *          cv2's manner, bit-reproducible; equality with cv2.warpAffine is NOT claimed.  A face with valid == 0 or a
 *          frame_index outside [0,F) gets an all-zero crop.
 *   errors FFR_ERR_ARG: a null pointer (where not allowed below), N <= 0, K outside 2..16, out_h or out_w outside 1..256,
 *          out_w % 4 != 0, pitch_bytes < 3 W, pitch_bytes * H >= 2^31 (64-bit frame bases, 32-bit offsets inside a
 *          frame), F, H or W < 1, a crop that is not 4-byte aligned.
 * All pointers are device pointers; nothing synchronises with the host.  ffr_align_transforms and ffr_align_warp need
 * no weights.  Launches are profiled under FFR_KC_LAYOUT.                                                            */
int ffr_align_transforms(ffr_handle* h, const float* landmarks, const float* tmpl, int N, int K,
                         double* A, uint8_t* valid, void* stream);
/* valid may be NULL: every face with a frame_index in range is warped.                                               */
int ffr_align_warp(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch_bytes,
                   const int32_t* frame_index, const double* A, const uint8_t* valid, int N,
                   int out_h, int out_w, uint8_t* crop, void* stream);
/* transforms -> warp to 112 x 112 into the handle's alignment scratch -> the pipeline of ffr_embed_u8, all on `stream`:
 * f_new[N][512], f[N][512] (f may be NULL), bit-identical to ffr_embed_u8 fed with ffr_align_warp's crop (an invalid
 * face embeds its zero crop); flip[N] as in ffr_embed_u8 (may be NULL); valid[N] receives the flags, 0 also for a
 * frame_index outside [0,F) (may be NULL).
 * The scratch (transforms, flags, crops) grows on demand -- hipMalloc on the first call at a larger N, which bumps
 * ffr_generation -- and is reused afterwards, so a call can be captured into a hipGraph once it has run at that shape. */
int ffr_embed_aligned(ffr_handle* h, const uint8_t* frames, int F, int H, int W, long long pitch_bytes,
                      const int32_t* frame_index, const float* landmarks, const float* tmpl, int K,
                      const uint8_t* flip, int N, float* f_new, float* f, uint8_t* valid, void* stream);

/* Fold protocol of lfw/lfw_eval.py:110-118,137-162,255-270 on the device: thresholds
 * np.arange(-1, 1, 0.005), same iff score > thr, n_folds contiguous test folds (KFold, no shuffle),
 * best threshold = LAST one reaching the best train accuracy, accuracy on the held-out fold.
 * score[n] fp32, label[n] int32 (1 = same) device; best_thr[n_folds], test_acc[n_folds] doubles,
 * device.  n_folds <= 32.  The reference's average is sum(test_acc) / 10.                     */
int ffr_lfw_fold_accuracy(ffr_handle* h, const float* score, const int32_t* label, int n, int n_folds,
                          double* best_thr, double* test_acc, void* stream);

/* Device workspace the handle holds / would need for batch N (bytes).  The arena
 * grows on the first call with a larger N (hipMalloc, outside any timed loop) and
 * is reused afterwards; ffr_reserve() grows it ahead of time.                       */
size_t ffr_workspace_bytes(const ffr_handle* h, int N, int H, int W);
int    ffr_reserve(ffr_handle* h, int N, int H, int W);

/* ---- measurement -----------------------------------------------------------------
 * Per-kernel-class device timing with hipEvents recorded on the launch stream
 * around every launch (bench.py roofline leg; off by default, adds a few us/launch).
 * Classes: see FFR_KC_*.  ffr_profile_read() synchronises the recorded events and
 * returns, per class, the number of launches, the summed device time in ms and the
 * algorithmic FLOPs (2*MACs), executed FLOPs and bytes (compulsory in+out+weights) of
 * those launches, then clears the log.  Launches that the engine puts on its second
 * stream (the few images split off a fused Winograd launch, which run beside it) count
 * with their launches, FLOPs and bytes but not with their time: it overlaps a launch of
 * the main stream that is already counted.                                              */
enum {
    FFR_KC_CONV_IGEMM = 0,  /* fp32-MFMA implicit-GEMM conv / FC (the dominant kernel) */
    FFR_KC_STEM = 1,
    FFR_KC_SE = 2,
    FFR_KC_COMBINE = 3,
    FFR_KC_HEAD = 4,
    FFR_KC_SELFSIM = 5,
    FFR_KC_CHANNEL = 6,
    FFR_KC_SPACE = 7,
    FFR_KC_LAYOUT = 8,
    FFR_KC_SCORE = 9,
    FFR_KC_WINO = 10,       /* Winograd F(4x4,3x3) input / output transforms (HBM-bound) */
    FFR_KC_WINO_FUSED = 11, /* k_wino_fused: the 36 GEMMs + output transform of a Winograd conv (MFMA-bound; the
                               dominant kernel of the forward) */
    FFR_KC_WGRAD = 12,      /* k_wgrad: weight gradients of the training step as TN GEMMs (MFMA-bound) */
    /* the HBM-bound kernels of the training step (include/ffrnet_train.h), itemised so that the classes sum to the step */
    FFR_KC_TRAIN_BN = 13,     /* train-mode BatchNorm: statistics, apply (+PReLU/residual), backward                  */
    FFR_KC_TRAIN_LOSS = 14,   /* the four loss items and their cotangents, CosFace head kernels                        */
    FFR_KC_TRAIN_OPTIM = 15,  /* clip_grad_value_ + Adam over the flat buffers                                         */
    FFR_KC_TRAIN_XFORM = 16,  /* Winograd weight / gradient transforms, dgrad packing, reflection folds, transposes    */
    FFR_KC_TRAIN_ELEM = 17,   /* the remaining elementwise / layout kernels of RecNet's train forward and backward     */
    FFR_KC_COUNT = 18
};
typedef struct {
    int64_t launches;
    double  ms;
    double  flops;          /* algorithmic: 2*MACs of the direct convolution / GEMM        */
    double  bytes;
    double  flops_executed; /* what the matrix cores really did (Winograd F(4x4,3x3) launches
                               execute 36/144 of the direct MACs, plus tile padding)       */
    double  flops_useful;   /* flops_executed without padding: the multiplies the algorithm the launch runs NEEDS --
                               direct convolution / GEMM: = flops; Winograd F(4x4,3x3): flops / 4 (36 instead of 144
                               multiplies per 4x4 output tile; tiles hanging over 14x14 / 7x7 maps, rows beyond T
                               and zero-padded channels are executed but not useful)       */
} ffr_kclass_stat;
int ffr_profile_enable(ffr_handle* h, int on);
/* Experiment knobs of one handle.  The library reads NO environment variable: every kernel-selection
 * choice that can be switched for an A/B measurement is an option here, and every setting computes the same
 * results (tests/test_gpu_parity.py::test_experiment_knobs_keep_parity).  Defaults = the measured best.
 *   "wino" (1)            0: every 3x3 convolution of the inference path is a direct implicit GEMM
 *   "wino_mincin" (64)    smallest padded input-channel count packed for Winograd; set BEFORE ffr_load_*
 *   "wino_fused" (1)      0: Winograd convolutions run as transform kernels around a batched GEMM (round-1 path)
 *   "wf_phased_maxk" (128) largest padded cin for which k_wino_fused transforms its own input
 *   "wf_minblocks" (200)  fewest 32-tile x 64-channel block tiles for which k_wino_fused is used
 *   "wf_tailsplit" (1)    1: images that do not fill whole rounds of block tiles run beside the launch (second stream)
 *   "se_maxtiles" (256)   SE squeeze from the Winograd epilogue's tile sums for maps of up to that many tiles (0: always its own pass)
 *   "wf_mixed" (1)        1: 14x14 maps (stage 3) are tiled exactly, 4+4+3+3 per dimension, with four tile types F(4x4) / F(4x3) /
 *                         F(3x4) / F(3x3) in one launch (k_wino_fused_mixed) whenever every CU gets two blocks or more; 0: padded
 *                         F(4x4) tiles only.  May be changed at any time: the three extra weight sets are derived on the device the
 *                         first time an ENCODER call (ffr_reserve, ffr_encoder_forward, ffr_embed*, the training iteration) is
 *                         eligible (ffr_memory_stats reports their bytes and seconds).  They are an optimisation: a device that
 *                         cannot hold them (0.7 GB) keeps the layers concerned on padded tiles, logs once and does not fail.
 *                         To capture ffr_embed into a hipGraph call ffr_reserve(N, H, W) (or run one eager forward) first.
 *   "channel_rows" (0)    k_channel_path (RecNet's channel branch): 1 / 2 / 4 blocks per image (128 CT rows of M_channel each);
 *                         0 = chosen from the batch and the CU count (fewer images than CUs -> more blocks per image)
 *   "combine_v" (1)       1: a bottleneck's combine (res * scale + shortcut) also writes the Winograd transform V of its
 *                         output when the next unit's conv1 runs k_wino_fused from V (stage 3 / 4): k_combine_in_c
 *                         replaces k_combine + k_wino_in_c
 *   "wf_split" (1)        1: the k_wino_fused launches that transform their own input (cin <= wf_phased_maxk, 32 x 64 blocks: stages
 *                         1-2) run their K loop in the split-operand form of "igemm_split" below: V is split into three bf16
 *                         pieces in registers after the LDS read, G g G^T comes as three bf16 planes that ffr_load_* split from the
 *                         double-precision fold (1.5 x the fp32 bytes of those layers, ffr_memory_stats: wf_split_weight_bytes; a
 *                         device without room keeps the fp32 loop for the layer, logs once and does not fail).  0: every launch is
 *                         the fp32-MFMA kernel, bit for bit.  The training path and raw-weight callers keep fp32.
 *   "igemm_split" (1)     1: the direct convolutions whose weights ffr_load_encoder split into three bf16 planes (the layers
 *                         that never run Winograd: 3x3 stride 2, the 1x1 shortcuts, and the output_layer GEMM) run k_igemm's
 *                         split-operand form: the same fp32 product as six exact bf16 x bf16 products per term on the bf16
 *                         matrix cores, accumulated in fp32 (error of the order of one fp32 rounding per product, DESIGN.md
 *                         3.2 / 4).  0: every launch is the fp32-MFMA kernel.  Callers that pass raw fp32 weights (ffr_op_conv
 *                         without flags bit1, the training GEMMs, the batched Winograd GEMMs) always run the fp32 form.  The
 *                         planes cost 1.5 x the fp32 weights of those layers (ffr_memory_stats: split_weight_bytes); a device
 *                         that cannot hold them keeps the fp32 form for the layers concerned, logs once and does not fail.
 *   "gemm_stream" (1), "sk_minunits" (18)   round-1 path details (batched-GEMM Winograd, stream-K granule)
 *   "wf_trace", "igemm_trace" (0)   per-launch phase stamps on stderr; only in a -DFFR_TRACE build (tools/trace_build.py),
 *                                    the shipped library returns FFR_ERR_UNSUPPORTED
 * (Round 6 retired the knobs whose A/B is settled -- block -> XCD maps, half blocks, forced tiles, round-1 slicing; the code
 * keeps the measured-best setting of each, EXPERIMENTS.md has the numbers.)
 * Unknown names and out-of-range values return FFR_ERR_ARG.                                                        */
int ffr_set_option(ffr_handle* h, const char* name, long long value);
int ffr_get_option(const ffr_handle* h, const char* name, long long* value);
/* Allocation generation: changes whenever device memory that a caller may have captured into a hipGraph (workspace
 * arena, stream-K tickets, packed weights, training buffers) has been released and re-allocated, and whenever the
 * per-layer arithmetic plan changes (ffr_layer_set_arith, ffr_calibrate): a graph captured before a plan change would
 * replay the old plan.  A graph captured around ffr_embed must be re-captured when this value differs from the one read
 * at capture time.                                                                                                   */
unsigned long long ffr_generation(const ffr_handle* h);

/* ---- per-layer arithmetic ----------------------------------------------------------------------
 * Every 3x3 stride-1 convolution packed for Winograd F(4x4,3x3) (padded cin >= option wino_mincin) is a "layer" of the
 * plan: the encoder's body.i.res_layer.1 of every bottleneck and res_layer.3 of the stride-1 ones (44 for IR-SE50), and
 * RecNet's ConvLayers (Conv4Space, ChannelFlipMerge, Conv4Merge).  Each runs Winograd (the default) or direct; a layer
 * pinned to direct runs exactly the arithmetic it runs under option wino = 0 (which still overrides every plan), so an
 * all-direct plan is bit-identical to wino = 0 and an all-Winograd plan to the default.  The plan applies to every
 * inference forward of the handle (ffr_encoder_forward, ffr_recnet_forward, ffr_embed*, ffr_encoder_trunk_nhwc and the
 * frozen encoder of ffr_train_iteration); RecNet's training step keeps its own ffr_train_option("winograd").
 * ffr_load_encoder / ffr_load_recnet reset that net's layers to Winograd and clear their sensitivities. Index order:
 * encoder layers by bottleneck (res_layer.1 before res_layer.3), then RecNet's in state_dict order.                 */
enum { FFR_ARITH_DIRECT = 0, FFR_ARITH_WINOGRAD = 1 };
typedef struct {
    char   name[64];     /* state_dict prefix of the conv: "body.7.res_layer.1", "Conv4Space.1.conv1.conv2d", ...          */
    int    net;          /* 0 encoder, 1 RecNet                                                                            */
    int    arith;        /* FFR_ARITH_DIRECT / FFR_ARITH_WINOGRAD                                                          */
    double sensitivity;  /* last ffr_calibrate: end-to-end difference with ONLY this layer on Winograd; -1 if none          */
} ffr_layer_info;
int ffr_layer_count(const ffr_handle* h, int* n);
int ffr_layer_get(const ffr_handle* h, int i, ffr_layer_info* out);          /* FFR_ERR_ARG for i outside [0, n)       */
int ffr_layer_set_arith(ffr_handle* h, int i, int arith);                   /* FFR_ERR_ARG for a bad i or arith       */
/* Calibrated arithmetic: pins layers to direct only as far as needed for the handle's forward ON THESE INPUTS, AT THIS N,
 * to differ from its own all-direct forward by at most `tol` of each output tensor's abs-max.
 *   x_nchw [N,3,H,W] (device): the encoder's layers (outputs featmap, and f at 112x112) plus RecNet's when it is loaded and
 *   H = W = 112 (outputs f_new, feat_new) -- XOR -- featmap_nchw [N,512,7,7] (device, H = W = 7): RecNet's layers only.
 *   achieved[4] (host, may be NULL): per output tensor (f, featmap, f_new, feat_new; -1 where absent) the final plan's
 *   max|calibrated - direct| / max|direct| on these inputs.  A forward that is not finite never counts as close: a NaN
 *   difference, and an inf / inf quotient, are +inf (every layer of such a forward ends on direct, achieved = +inf).
 * Method: one all-direct forward as the anchor; one forward per layer with only that layer on Winograd (its sensitivity);
 * the layers sorted by sensitivity, the longest low-sensitivity prefix that stays <= tol / 2 keeps Winograd (every prefix
 * is measured: no monotonicity is assumed); one more forward verifies the plan (the margin of 1/2 is for other images of
 * the same distribution).  Comparisons run on the device; each phase copies one small table to the host.
 * The Winograd kernels depend on N (the exact 4+4+3+3 tiling of stage 3 appears only at large batches): calibrate at the
 * batch size you will run.  Unlike every forward entry point this call SYNCHRONISES `stream` (up to 3 times), allocates and
 * frees device memory, and refuses to run while `stream` is capturing.  Errors: FFR_ERR_ARG for tol <= 0 or NaN, both or
 * neither input, a capturing stream; FFR_ERR_STATE when the net it needs is not loaded.  On error the plan is unchanged. */
int ffr_calibrate(ffr_handle* h, const float* x_nchw, const float* featmap_nchw, int N, int H, int W,
                  double tol, double* achieved, void* stream);
/* Device memory and packing time of the handle (round 5; the reference's counterpart is `net.load_state_dict(...)` +
 * `.to(device)`, models/trainer.py:98-113, which has no packing step).  mixed_tile_* are the three extra Winograd weight
 * sets of the exact 14x14 tiling: derived on the device the first time a batch large enough to use them arrives
 * (ffr_reserve / the first forward of >= 256 images), 0 before.  split_weight_bytes (part of encoder_weight_bytes) are
 * the bf16 planes of the split-operand form of k_igemm (option "igemm_split"), made by ffr_load_encoder;
 * wf_split_weight_bytes (part of encoder_weight_bytes too) those of k_wino_fused's (option "wf_split"), and
 * wf_split_launches counts the k_wino_fused launches that ran in that form since ffr_create (tests read the plan from it). */
typedef struct ffr_mem_stats {
    size_t encoder_weight_bytes, recnet_weight_bytes, mixed_tile_weight_bytes, workspace_bytes;
    double encoder_load_seconds, recnet_load_seconds, mixed_tile_pack_seconds;
    size_t split_weight_bytes;
    size_t wf_split_weight_bytes;
    long long wf_split_launches;
} ffr_mem_stats;
int ffr_memory_stats(const ffr_handle* h, ffr_mem_stats* out);
/* The packer's 3-way bf16 split of the split-operand forms, on the host (no device, no handle; tests): planes[p][i], p = 0..2,
 * are the bf16 pieces (round to nearest even) of w[i]: p1 = bf16(w), p2 = bf16(w - p1), p3 = bf16(w - p1 - p2).       */
int ffr_split_planes_host(const double* w, long long n, unsigned short* planes);
/* fp32-MFMA rate this device delivers on a register-resident v_mfma_f32_32x32x2_f32 loop (iters x 16 MFMAs per
 * wave, 8 waves per CU) and the shader clock it holds meanwhile: the measured denominator of a roofline fraction. */
int ffr_probe_mfma_peak(ffr_handle* h, int iters, double* tflops, double* clock_ghz, void* stream);
int ffr_profile_read(ffr_handle* h, ffr_kclass_stat* out /* [FFR_KC_COUNT] */);

/* ---- single operators (parity tests drive the kernels one at a time) -------------
 * Implicit-GEMM convolution on NHWC fp32, the kernel behind every 3x3 / 1x1 conv of
 * pretrain/model_ir_se50.py:63,67,69 and models/recnet.py:65,82.
 *   x      [N,H,W,in_pitch]  (channels [0,cin_pad) are read; cin_pad % 32 == 0)
 *   w      [cout_pad][R*S*cin_pad]  packed (r,s,ci), cout_pad % 64 == 0
 *   bias   [n_cls][cout_pad], n_cls = 1, or 9 border classes when border_bias != 0
 *   slope  [cout_pad] PReLU slopes or NULL
 *   resid  [N,Ho,Wo,res_pitch] added after the activation, or NULL
 *   out    [N,Ho,Wo,out_pitch], channels [out_coff, out_coff+cout_store) written
 *   pad_mode 0 = zero, 1 = reflect;  flags bit0 = sigmoid at the end; bit1 = run the split-operand form of the kernel
 *   (option "igemm_split") on a device-side split of w into three bf16 planes (tests; synchronises the stream)
 *   tile   0 = heuristic, else 1..4 = forced tile config (128x128, 128x64, 64x64, 256x64);
 *   splitk is ignored (the kernel is stream-K: K is balanced over the blocks by itself) */
typedef struct {
    const float* x; int N, H, W, in_pitch, cin_pad;
    const float* w; const float* bias; const float* slope;
    const float* resid; int res_pitch;
    float* out; int out_pitch, out_coff, cout_store, cout_pad;
    int R, S, stride, pad, pad_mode, border_bias, flags;
    int tile, splitk;
} ffr_conv_desc;
int ffr_op_conv(ffr_handle* h, const ffr_conv_desc* d, void* stream);

/* 3x3 / stride 1 / pad 1 convolution from RAW weights (host, [cout][cin][3][3] as torch stores them,
 * bias[cout], optional PReLU slope[cout]) on x[N,H,W,cin] NHWC (device, cin % 32 == 0), packed on
 * the fly.  use_wino: 0 = direct implicit GEMM, 1 = Winograd F(4x4,3x3) with GEMM and output transform in one kernel
 * (k_wino_fused; input transform inside it for cin <= 128), 2 = Winograd as transform kernels around a batched GEMM, 3 = k_wino_fused
 * with 32 x 32 blocks, 4 = the exact 4+4+3+3 tiling of a 14x14 map with 256 input channels (k_wino_fused_mixed), 5 = as 1 with the
 * split-operand K loop (option "wf_split"; FFR_ERR_UNSUPPORTED for cin > wf_phased_maxk).  Test hook
 * that holds every path to torch's conv2d.  out[N,H,W,cout] NHWC device, cout % 4 == 0.         */
int ffr_op_conv3x3(ffr_handle* h, const float* x_nhwc, int N, int H, int W, int cin,
                   const float* w_host, const float* bias_host, const float* slope_host, int cout,
                   int pad_mode, int use_wino, const float* resid_nhwc, float* out_nhwc, void* stream);

/* The same convolution with the whole epilogue contract of the Winograd kernels (test hook; the hook above stays as it is).
 *   x [N,H,W,in_pitch] (in_pitch >= cin, cin % 32 == 0), out [N,H,W,out_pitch] with channels [out_coff, out_coff + cout_store)
 *   written (cout_store <= cout; 0 = cout), resid [N,H,W,res_pitch] or NULL (res_pitch 0 = cout), flags bit0 = sigmoid.
 *   use_wino -1 leaves the form to the planner (tail split included), 0..5 as above.
 *   in_scale / in_shift [cin] (host, both or neither): a per-input-channel affine in front of the zero padding, folded by the
 *   packer into the weights and the 9 border-class biases (pad_mode 0 only).
 *   tile_sums [T][cout_pad] (device, optional; Winograd forms only): per-tile sums of the stored outputs, T = N * tiles per image
 *   in raster order (the exact 14x14 tiling: slot n * tiles + offset of the tile type + index within the type, wino_mixed.hip).
 * N <= 700.  A form that cannot honour the descriptor fails with the planner's reason (FFR_ERR_STATE / FFR_ERR_UNSUPPORTED);
 * nothing else runs in its place. */
typedef struct {
    const float* x; int N, H, W, cin, in_pitch;
    const float* w_host; const float* bias_host; const float* slope_host; int cout;
    const float* in_scale_host; const float* in_shift_host;
    const float* resid; int res_pitch;
    float* out; int out_pitch, out_coff, cout_store;
    int pad_mode, use_wino, flags;
    float* tile_sums;
} ffr_conv3x3_desc;
int ffr_op_conv3x3_ex(ffr_handle* h, const ffr_conv3x3_desc* d, void* stream);

/* ---- plan record of the convolution launchers (tests) ----------------------------
 * While recording is on, every launch a convolution makes appends one entry, in launch order: the entry of the convolution's
 * plan (plan_conv) that the launcher executed, the same one ffr_plan_conv_host reports.  Off by default (one branch on a bool per
 * launch); switching it on clears the record; a convolution on a capturing stream is refused while it is on (FFR_ERR_STATE).
 *   path    FFR_CP_DIRECT k_igemm | FFR_CP_FUSED k_wino_fused | FFR_CP_UNFUSED_STREAM k_gemm_stream between the transform kernels |
 *           FFR_CP_UNFUSED_IGEMM batched k_igemm between them | FFR_CP_MIXED k_wino_fused_mixed | FFR_CP_TAIL_SPLIT: no launch, the
 *           two entries that follow are the parts of one tail split (the part enqueued first comes first)
 *   images, rows   images of this launch; GEMM rows M of a direct launch, Winograd tiles T otherwise
 *   tile, nblocks, granule, nkt, tiles, cut, split   k_igemm / k_gemm_stream: tile config 1..4, persistent blocks, K-tiles a block
 *           owns at least (1 or nkt), K-tiles per tile, tiles, 1 when a tile is cut (in-launch fix-up), split-operand form
 *   phased, half_n, split, block_tiles   k_wino_fused: in-kernel input transform, 32 x 32 blocks, split-operand K loop, block tiles
 *   n_main, side   FFR_CP_TAIL_SPLIT: images that run fused; 1 when the remainder went to the second stream
 * RecNet's channel launch is recorded too, as FFR_CP_CHANNEL (k_channel_path): images = N, nblocks = N x row blocks per image
 * (1 / 2 / 4 = k_channel_path<4 / 2 / 1>), rows = the rows of M_channel one block evaluates (512 / row blocks).
 * The encoder trunk records the launches between its convolutions as well, one entry each, where it makes them (a bottleneck
 * ends with exactly one combine entry).  images = N in all of them:
 *   FFR_CP_SE_POOL    SE squeeze by its own pooling pass (k_se_pool + k_se_fc): rows = H*W of the pooled map, tiles = slices S
 *   FFR_CP_SE_TILES   SE squeeze from conv2's Winograd tile sums (k_se_fc alone): rows = H*W, tiles = S = tiles per image
 *   FFR_CP_COMBINE | FFR_CP_COMBINE_IN_C | FFR_CP_COMBINE_IN_MIXED   k_combine | k_combine_in_c | k_combine_in_mixed (the latter
 *           two also write V for the next conv1): rows = H*W of the output map, tiles = its 4x4 tiles per image, stride = the
 *           bottleneck's, conv_shortcut = 1 when the shortcut is a convolution's output (0: the input itself, subsampled by
 *           stride), se_scale = 1 when an SE scale is applied (0 in mode 'ir')
 *   FFR_CP_WINO_OUT_IN   conv1 -> conv2 chained transform (k_wino_out_in): rows = Winograd tiles T, tiles = tiles per image
 *           (<= 4: the 256-channel block form, else the 64-channel one) */
enum { FFR_CP_DIRECT = 0, FFR_CP_FUSED = 1, FFR_CP_UNFUSED_STREAM = 2, FFR_CP_UNFUSED_IGEMM = 3, FFR_CP_MIXED = 4, FFR_CP_TAIL_SPLIT = 5,
       FFR_CP_CHANNEL = 6, FFR_CP_SE_POOL = 7, FFR_CP_SE_TILES = 8, FFR_CP_COMBINE = 9, FFR_CP_COMBINE_IN_C = 10,
       FFR_CP_COMBINE_IN_MIXED = 11, FFR_CP_WINO_OUT_IN = 12 };
typedef struct ffr_conv_launch {
    int path, images, rows;
    int tile, nblocks, granule, nkt, tiles, cut, split;
    int phased, half_n, block_tiles;
    int n_main, side;
    int stride, conv_shortcut, se_scale;
} ffr_conv_launch;
int ffr_conv_plan_record(ffr_handle* h, int on);
int ffr_conv_plan_read(ffr_handle* h, ffr_conv_launch* out, int cap, int* n);

/* ---- the planners on the host (no device, no handle; tests) ------------------------
 * plan_igemm for `count` consecutive row counts M, M + 1, ...: tile[i], nblocks[i], granule[i] of k_igemm for [M + i rows] x
 * [cout_pad] with nkt K-tiles per tile and nbatch GEMMs (force_tile 0 = the planner's choice, split != 0 = split-operand form). */
int ffr_plan_igemm_host(long long M, int cout_pad, int nkt, int nbatch, int force_tile, int min_units, int split, int count,
                        int* tile, int* nblocks, int* granule);
/* plan_conv for one layer and one call under default options, with the scratch capacities of the workspace of N images of
 * 112x112 (N >= 8).  Weight sets are presence flags: has_wino (Winograd weights, both orders), has_wu3 (planes of the fused
 * split-operand loop), has_w3 (planes of the direct split-operand form), has_mixed (the exact-tiling sets).  force: -1..5.
 * out[0..23]: [0..8] path (0 direct, 1 mixed, 2 fused, 3 unfused), half_n, phased, split, n_main, side, takes_v, refused,
 *   tiles_img; [9..14] the launch, or the main part of a tail split, and [15..20] the remainder of a tail split (all 0 without
 *   one), 6 values each: kind (0 none, 1 k_igemm, 2 k_wino_fused, 3 k_gemm_stream, 4 mixed), fits (every scratch the launch needs
 *   is large enough), tile, nblocks, granule, cut (tile, nblocks: k_igemm and k_gemm_stream; granule, cut: k_igemm), all read
 *   from the plan's entries, which are what run_conv executes and the plan record shows; [21..23] spare. */
int ffr_plan_conv_host(int cin, int cout, int R, int stride, int pad, int pad_mode, int has_wino, int has_wu3, int has_w3,
                       int has_mixed, int N, int H, int W, int in_pitch, int out_pitch, int out_coff, int cout_store,
                       int res_pitch, int num_cus, int force, long long* out);

/* The row blocks per image of k_channel_path for N images on num_cus CUs: forced = option "channel_rows" (0 = the automatic
 * choice, 1 / 2 / 4 come back as they are, anything else is FFR_ERR_ARG). */
int ffr_plan_channel_rows_host(int N, int num_cus, int forced, int* row_blocks);

/* Encoder trunk only, stopping after `n_blocks` bottlenecks (0 = stem only,
 * 24 = whole body, before Backbone.bn); writes the NHWC activation.  Test hook for
 * the per-stage goldens.                                                            */
int ffr_encoder_trunk_nhwc(ffr_handle* h, const float* x_nchw, int N, int H, int W,
                           int n_blocks, float* out_nhwc, void* stream);

/* RecNet internals for image-level goldens: any pointer may be NULL.
 *   ss_space[N,49,49] M_space[N,49,49]; ss_channel and M_channel are never stored by the fused channel path:
 *   ss_channel0[512,512] / M_channel0[512,512] receive them for ONE image, `image` in [0, N) (debug stores inside the kernel);
 *   feat_space[N,512,7,7] feat_channel_raw[N,512,7,7] (before ChannelFlipMerge)
 *   feat_channel[N,512,7,7] (after ChannelFlipMerge), all NCHW.                     */
int ffr_recnet_debug(ffr_handle* h, const float* featmap_nchw, int N,
                     float* ss_space, float* M_space, float* feat_space,
                     float* feat_channel_raw, float* feat_channel, float* ss_channel0, float* M_channel0,
                     int image, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FFRNET_H */
