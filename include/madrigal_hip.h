/*
 * madrigal_hip.h -- C ABI of libmadrigal_hip.so: MI355X (gfx950) kernels for Madrigal's
 * encode -> fuse -> pairwise-score path.
 *
 * This is the drop-in boundary below the Python classes in madrigal_amd/ (which mirror
 * madrigal.models of the reference).  The reference owns no native code: every entry point
 * replaces an implicit device-kernel call site inside a third-party wheel (ATen/cuBLAS,
 * torch_scatter, torchdrug, PyG); the call site is cited as <reference file>:<line>.
 *
 * Conventions (all entry points)
 *   - plain pointers and sizes, no torch types; every pointer is a DEVICE pointer unless the
 *     name ends in _host; tensors are dense row-major fp32 unless stated;
 *   - returns 0 on success, a negative MDG_E* code on failure; mdg_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - never allocates or frees device memory: scratch is passed in as `workspace`, sized by the
 *     matching *_workspace_bytes() query; never synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream) and the call returns;
 *   - re-entrant, no internal threads, safe under hipGraph capture; no global mutable state apart
 *     from the two diagnostics hooks at the end of this header (tuning switches, clock stamps).
 */
#ifndef MADRIGAL_HIP_H
#define MADRIGAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDG_OK 0
#define MDG_EINVAL (-1)   /* bad argument (shape, alignment, enum) */
#define MDG_EWORKSPACE (-2) /* workspace too small / missing */
#define MDG_ELAUNCH (-3)  /* HIP launch failed */
#define MDG_EUNSUPPORTED (-4)
#define MDG_GATHER_MAX_SOURCES 19 /* source matrices of one mdg_gather_rows_multi call */
#define MDG_COLLATE_MAX_SEGMENTS 4 /* row-gather segments of one mdg_collate_rows call */

/* Arithmetic of the matrix products.  Inputs and outputs stay fp32. */
enum mdg_precision {
  MDG_PREC_F32 = 0,    /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate        */
  MDG_PREC_BF16X3 = 1, /* each fp32 operand split hi+lo bf16; hi*hi + hi*lo + lo*hi on the
                          bf16 MFMA, fp32 accumulate: ~2^-17 relative per product             */
  MDG_PREC_BF16 = 2,   /* operands rounded to bf16 once, fp32 accumulate (cfg "bf16")          */
  MDG_PREC_F16 = 3     /* operands rounded to IEEE half once (v_mfma_f32_32x32x16_f16), fp32
                          accumulate: BASELINE configs[4] "fp16 bilinear head".  Accepted by
                          mdg_bilinear_allpairs only; inputs must stay inside the half range.   */
};

/* What the all-pairs head does with each score tile. */
enum mdg_bilinear_epilogue {
  MDG_EPI_STORE = 0,         /* out[l,i,j] = S            (raw logits, as the reference returns) */
  MDG_EPI_STORE_SIGMOID = 1, /* out[l,i,j] = sigmoid(S)   (train_ddi_batch.py:285)               */
  MDG_EPI_ROWSTATS = 2,      /* nothing is materialised: stats[l,i,0] = sum_j S, stats[l,i,1] =
                                max_j S (roofline stress runs whose [L,N,N] cannot exist; callers who
                                want results rather than statistics: mdg_bilinear_topk)          */
  MDG_EPI_TRIKEYS = 3        /* for callers whose product is ranks (notebooks/normalize_scores.py:36-85 reads
                                the strict lower triangle only): out[l,i,j] for j < i = the order-preserving
                                uint32 key of S[l,i,j] (the bits mdg_rank_normalize sorts), the same value the
                                STORE epilogue puts there; entries with j >= i are unspecified (never written
                                outside the 256 x 256 blocks on the diagonal): half the store stream.
                                Symmetric sweep only (z_head == z_tail, symmetric W, row pitch >= n rounded
                                up to 4); consumed by mdg_rank_normalize_keys_ld.                          */
};

/* Activation fused into mdg_linear's epilogue (madrigal/models/models.py:31, actn2actfunc). */
enum mdg_activation {
  MDG_ACT_NONE = 0, MDG_ACT_RELU = 1, MDG_ACT_GELU = 2 /* exact erf form */, MDG_ACT_SIGMOID = 3, MDG_ACT_TANH = 4,
  MDG_ACT_LEAKYRELU = 5, MDG_ACT_SOFTPLUS = 6, MDG_ACT_SELU = 7
};

const char* mdg_last_error(void);
/* "gfx950" build tag, and the ABI version (bumped on any signature change). */
const char* mdg_build_arch(void);
int mdg_abi_version(void);

/* Diagnostics.  The MDG_* environment variables are experiment switches that select between kernel schedules
 * with identical results; each is read once per process, at its first use.  mdg_tuning_reload() makes every
 * switch re-read the environment at its next use (tests and timing scripts flip one between two launches).
 * mdg_debug_bilinear_stamps hands mdg_bilinear_allpairs a device buffer of `entries` uint64 that receives
 * {shader cycles, 100 MHz ticks} per workgroup of each following launch whose grid fits; NULL switches it off.
 * Neither is meant to be called concurrently with launches from other threads. */
void mdg_tuning_reload(void);
void mdg_debug_bilinear_stamps(void* buffer, int64_t entries);

/* ------------------------------------------------------------------ bilinear DDI head ---- */

/* W_sym[l] = triu(W[l]) + triu(W[l],1)^T for l in [0,L): the `Symmetric` parametrisation the
 * reference recomputes on every forward.  Replaces madrigal/models/models.py:522-524.
 * w_original, w_sym: [L,D,D].  In place (w_sym == w_original) is allowed. */
int mdg_symmetrize(const float* w_original, float* w_sym, int64_t L, int64_t D, void* stream);

/* Scratch for mdg_bilinear_allpairs (hi/lo bf16 images of z_tail and W_sym; 0 for F32). */
size_t mdg_bilinear_allpairs_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D,
                                             int precision);

/* All-pairs bilinear scores  S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j]  for every outcome l,
 * head drug i and tail drug j, with the association order of the reference ((z W) z^T, the
 * inner product rounded to fp32).  Replaces BilinearDDIScorer.bilinear/forward,
 * madrigal/models/models.py:537-547 (two batched cuBLAS GEMMs there), and one chunk of the
 * scoring loop madrigal/evaluate/predict.py:420-429 when called on a label range (pass
 * w_sym + lo*D*D and n_labels = hi-lo).
 *   z_head [n_head,D], z_tail [n_tail,D], w_sym [n_labels,D,D] (already symmetrised), D == 128.
 *   epilogue STORE / STORE_SIGMOID: out [n_labels,n_head,n_tail] fp32, outcome-major.
 *   epilogue ROWSTATS: out [n_labels,n_head,2] fp32.
 * No alignment requirement beyond 4 bytes on out; z_* and w_sym must be 16-byte aligned. */
int mdg_bilinear_allpairs(const float* z_head, const float* z_tail, const float* w_sym, float* out,
                          int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision,
                          int epilogue, void* workspace, size_t workspace_bytes, void* stream);
/* The same with a row pitch: out[(l * n_head + i) * ldo + j], ldo >= n_tail floats.  The MI355X-native layout of a score tensor
 * whose n_tail is not a multiple of 32: with ldo = n_tail rounded up to 32 every row starts on a 128-byte line and the head's
 * 16-byte stores stay whole-line (a contiguous [L,N,N] with such an N is written correctly but with cache-line-straddling
 * stores, 2-3x slower).  The padding columns [n_tail, ldo) may be overwritten with unspecified values. */
int mdg_bilinear_allpairs_ld(const float* z_head, const float* z_tail, const float* w_sym, float* out, int64_t ldo, int64_t n_head,
                             int64_t n_tail, int64_t n_labels, int64_t D, int precision, int epilogue, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The same tensor in 16 bits: out[(l * n_head + i) * ldo + j] = the fp32 score (MDG_EPI_STORE) or 1 / (1 + expf(-score))
 * (MDG_EPI_STORE_SIGMOID) of mdg_bilinear_allpairs' general sweep in `precision` -- the same accumulator bits in all four modes --
 * rounded ONCE, to nearest even, to IEEE half (MDG_SCORE_F16; overflow becomes +-inf) or bfloat16 (MDG_SCORE_BF16): bit for bit
 * the fp32 tensor cast afterwards, with 2 B per score leaving the chip instead of 4 + a cast pass.  For callers that keep or ship
 * the tensor itself: one chunk of the memmap loop madrigal/evaluate/predict.py:420-429 (decoder of madrigal/models/models.py:
 * 537-547) at half the HBM, PCIe and disk bytes.
 *   out: 2-byte aligned, ldo >= n_tail in ELEMENTS, any pitch.  Rows that all start on 4 bytes (out % 4 == 0 and an even ldo;
 *   ldo = n_tail rounded up to 64 puts them on 128-byte lines) are written as whole lines of packed column pairs; any other
 *   layout is written correctly with 2-byte stores, several times slower.  Nothing outside columns [0, n_tail) of a row is
 *   touched, padding included.  z_head == z_tail is allowed and takes the same general sweep (no mirrored store).
 *   epilogue: MDG_EPI_STORE or MDG_EPI_STORE_SIGMOID only.  n_labels <= 65535 per call, D == 128, 256 * ldo * 2 < 2^31.
 *   Workspace: mdg_bilinear_allpairs_workspace_bytes (the same operand images).  No atomics: bit-identical between launches. */
enum mdg_score_type { MDG_SCORE_F16 = 1, MDG_SCORE_BF16 = 2 };
int mdg_bilinear_allpairs16_ld(const float* z_head, const float* z_tail, const float* w_sym, void* out, int64_t ldo, int64_t n_head,
                               int64_t n_tail, int64_t n_labels, int64_t D, int precision, int epilogue, int score_type,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Checkpoint ensemble of the all-pairs head: out[l,i,j] = mean_k sigmoid(z_head_k[i]^T W_sym_k[l] z_tail_k[j]).
 * Replaces get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614.
 * z_head_host / z_tail_host / w_sym_host: HOST arrays of n_models (1..8) device pointers, model k's z_head [n_head,D],
 * z_tail [n_tail,D] and W_sym [n_labels,D,D] (already symmetrised), D == 128, 16-byte aligned.  out[(l * n_head + i) * ldo + j],
 * ldo >= n_tail, fp32, the layout of mdg_bilinear_allpairs_ld.  Per model the logit is the head's own arithmetic in `precision`
 * (MDG_PREC_F32 or MDG_PREC_BF16X3); each sigmoid is 1 / (1 + expf(-s)); the K sigmoids are summed in fp32 in model order and
 * divided once by K.  When z_head_k == z_tail_k for every k (one drug set against itself) only the tiles on / right of the
 * block diagonal are computed and mirrored: out[l] is then exactly symmetric.  Workspace: split-bf16 images of every model's
 * z_tail and W_sym (0 for F32). */
size_t mdg_bilinear_ensemble_sigmoid_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D,
                                                     int n_models, int precision);
int mdg_bilinear_ensemble_sigmoid(const float* const* z_head_host, const float* const* z_tail_host,
                                  const float* const* w_sym_host, int n_models, float* out, int64_t ldo,
                                  int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* The same tensor in 16 bits (ABI 30): out[(l * n_head + i) * ldo + j] = P[l,i,j] of mdg_bilinear_ensemble_sigmoid -- the mean
 * probability get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) deliver --
 * rounded ONCE, to nearest even, to IEEE half (MDG_SCORE_F16) or bfloat16 (MDG_SCORE_BF16): bit for bit the tensor
 * mdg_bilinear_ensemble_sigmoid writes for the same operands, cast afterwards, with 2 B per probability leaving the chip instead
 * of 4 + a cast pass (half subnormals and values that round to 0 or to exactly 1 included).  The same sweeps: with z_head_k ==
 * z_tail_k for every k the symmetric one runs, each element still has one writer and out[l] is exactly symmetric.
 *   Operands, n_models (1..8), precision (MDG_PREC_F32 or MDG_PREC_BF16X3) and argument checks as mdg_bilinear_ensemble_sigmoid.
 *   score_type: MDG_SCORE_F16 or MDG_SCORE_BF16; anything else is refused before a launch.
 *   out: 2-byte aligned, ldo >= n_tail in ELEMENTS, any pitch.  Rows that all start on 4 bytes (out % 4 == 0 and an even ldo;
 *   ldo = n_tail rounded up to 64 puts them on 128-byte lines) are written as packed column pairs; any other layout is written
 *   correctly with 2-byte stores, slower.  Nothing outside columns [0, n_tail) of a row is touched, padding included.
 *   n_labels <= 65535 per call, D == 128, 256 * ldo * 2 < 2^31.
 *   Workspace: the size mdg_bilinear_ensemble_sigmoid_workspace_bytes gives (0 for F32).  No atomics: bit-identical between
 *   launches. */
int mdg_bilinear_ensemble_sigmoid16(const float* const* z_head_host, const float* const* z_tail_host,
                                    const float* const* w_sym_host, int n_models, void* out, int64_t ldo, int64_t n_head,
                                    int64_t n_tail, int64_t n_labels, int64_t D, int precision, int score_type,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Per-row top-k of the checkpoint ensemble (ABI 25): for every outcome l and head row i the k largest
 *   P[l,i,j] = mean_m sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])
 * over the ELIGIBLE tail columns j, and those columns, without materialising [L,N,N].  The probability is the one
 * get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) average over the
 * checkpoints; the lists are what the reference reads off that stored tensor (notebooks/quick_predictions.ipynb cell 8) and, in
 * LOWER mode, the candidates of the pairs notebooks/normalize_scores.py:39-46 ranks.  The mean of sigmoids is not monotone in any
 * one model's logit, so the single-model lists of mdg_bilinear_topk cannot be combined into these.
 *   Operands as mdg_bilinear_ensemble_sigmoid (HOST arrays of n_models = 1..8 device pointers, 16-byte aligned, D == 128);
 *   precision MDG_PREC_F32 or MDG_PREC_BF16X3.  P is bit for bit what mdg_bilinear_ensemble_sigmoid's general sweep (z_head !=
 *   z_tail) writes: the same products, sigmoid 1 / (1 + expf(-s)), fp32 sum in model order, one division by K.
 *   vals [n_labels,n_head,k] fp32, idx [n_labels,n_head,k] int32, order (P descending, column ascending), which is also the tie
 *   rule for what is kept (exact ties are common: many probabilities round to 1); padding -inf / -1.  eligible, k, n_tail and
 *   n_labels as mdg_bilinear_topk.  mask / plane_stride as the *_masked entry points below (mask == NULL: the unmasked kernel,
 *   no mask memory is read).  mdg_bilinear_ensemble_topk_chunk_tiles: the 64-column tail tiles a workgroup sweeps between two
 *   rebuilds of the models' z_head . W_sym products (for tests that want sizes at that boundary).
 *   Workspace: split-bf16 images of every model's z_tail and W_sym (0 for F32), the size mdg_bilinear_ensemble_sigmoid needs.
 * Deterministic: no atomics, the lists live in registers, nothing is stored before the final k stores per row. */
int mdg_bilinear_ensemble_topk_chunk_tiles(void);
size_t mdg_bilinear_ensemble_topk_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_models,
                                                  int precision);
int mdg_bilinear_ensemble_topk(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                               float* vals, int32_t* idx, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision,
                               int k, int eligible, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                               int64_t plane_stride);

/* Threshold selection over the checkpoint ensemble (ABI 26): for every outcome l with its cut thr[l], ALL eligible pairs (i,j) with
 *   P[l,i,j] = mean_m sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])  >=  thr[l]
 * as CSR over the n_labels * n_head rows (l,i), without materialising [L,N,N]: mdg_bilinear_select_*'s contract on the probability
 * get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) average over the
 * checkpoints -- "every pair the ensemble calls an interaction with P >= 0.9", the set the reference's users read off that stored
 * tensor (notebooks/quick_predictions.ipynb cell 8); in LOWER mode the pairs are those of the strict lower triangle
 * notebooks/normalize_scores.py:39-46 ranks.  The mean of sigmoids is not monotone in any one model's logit, so no union or
 * intersection of mdg_bilinear_select_* results gives this set.
 *   Operands as mdg_bilinear_ensemble_topk (HOST arrays of n_models = 1..8 device pointers, 16-byte aligned, D == 128); precision
 *   MDG_PREC_F32 or MDG_PREC_BF16X3.  P is bit for bit what mdg_bilinear_ensemble_sigmoid's general sweep writes; the compare is
 *   on the quotient, P >= thr[l] (thr [n_labels] fp32, device): -inf selects every eligible pair, +inf or a NaN cut none.
 *   mdg_bilinear_ensemble_select_count: row_counts [n_labels,n_head] int32, every entry written, zeros included; the caller's
 *     exclusive prefix sum over the flattened counts is row_ptr.
 *   mdg_bilinear_ensemble_select_fill: row_ptr [n_labels*n_head + 1] int64; cols [T] int32 and vals [T] fp32, T = row_ptr[last]:
 *     the selected columns of row (l,i) in ASCENDING order and their probabilities -- canonical CSR, the order torch.nonzero gives
 *     on the dense mask.  Bounded writes as mdg_bilinear_select_fill: slot s of row r is stored only if 0 <= row_ptr[r] <= s <
 *     row_ptr[r+1]; all slot arithmetic is 64-bit.
 *   eligible, n_tail (>= 1, < 2^31 - 64) and n_labels (<= 65535 per call) as mdg_bilinear_select_*; mask / plane_stride as the
 *   *_masked entry points below (mask == NULL: the unmasked kernel, no mask memory is read).  The tail tiles between two rebuilds of
 *   the models' z_head . W_sym products are mdg_bilinear_ensemble_topk_chunk_tiles().
 *   Workspace: the size mdg_bilinear_ensemble_sigmoid_workspace_bytes gives (0 for F32).
 * Deterministic: every row belongs to one wave that walks the column tiles in ascending order; no atomics; bit-identical from
 * launch to launch. */
size_t mdg_bilinear_ensemble_select_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_models,
                                                    int precision);
int mdg_bilinear_ensemble_select_count(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                       const float* thr, int32_t* row_counts, int64_t n_head, int64_t n_tail, int64_t n_labels,
                                       int64_t D, int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream,
                                       const uint32_t* mask, int64_t plane_stride);
int mdg_bilinear_ensemble_select_fill(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                      const float* thr, const int64_t* row_ptr, int32_t* cols, float* vals, int64_t n_head,
                                      int64_t n_tail, int64_t n_labels, int64_t D, int precision, int eligible, void* workspace,
                                      size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);

/* Per-outcome probability counts of the checkpoint ensemble (ABI 28): for every outcome l, given n_edges ascending finite fp32 edges
 * e[l,0..B-1],
 *   counts[l,b] = #{eligible (i,j) : e[l,b-1] <= P[l,i,j] < e[l,b]},   e[l,-1] = -inf, e[l,B] = +inf        (b = 0..B)
 *   P[l,i,j]    = mean_m sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])
 * -- torch.bucketize(P, e[l], right=True) followed by a bincount, without materialising [L,N,N]: mdg_bilinear_bincount's contract on
 * the probability get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) average
 * over the checkpoints.  With the edges at the probabilities of screened hits (mdg_bilinear_ensemble_topk / _select_fill return
 * exactly these values) the cumulative counts are the hits' exact normalised ranks among all pairs, the quantity
 * notebooks/normalize_scores.py:36-74 computes by ranking the stored lower triangle; with evenly spaced edges they are histograms
 * of the ensemble's probabilities.  The mean of sigmoids is not monotone in any one model's logit, so no combination of
 * mdg_bilinear_bincount results gives these counts.
 *   Operands as mdg_bilinear_ensemble_select_count (HOST arrays of n_models = 1..8 device pointers, 16-byte aligned, D == 128);
 *   precision MDG_PREC_F32 or MDG_PREC_BF16X3.  P is bit for bit what mdg_bilinear_ensemble_sigmoid's general sweep writes; the
 *   compares are on the quotient, e <= P.
 *   edges [n_labels,n_edges] fp32, device; counts [n_labels,n_edges+1] int64, zeroed by the call on `stream`; every row of counts
 *   sums to the number of eligible pairs.  Equal neighbouring edges give an empty bin; unsorted edges give unspecified counts (no
 *   out-of-bounds access).  A NaN probability is counted nowhere.
 *   1 <= n_edges <= mdg_bilinear_bincount_max_edges(); n_labels <= 65535 per call; eligible as mdg_bilinear_topk (NOT_SELF / LOWER
 *   need n_head == n_tail); n_tail < 2^23, as mdg_bilinear_bincount: a workgroup counts its 128 x n_tail probabilities in 32-bit
 *   counters.  n_head == 0 or n_labels == 0: MDG_OK, nothing launched, the counts zeroed where the pointer is not null.
 *   mdg_bilinear_ensemble_bincount_split: the arguments above plus `mask` / `plane_stride` (the rules of the *_masked entry points
 *   below) and counts int64 [2][n_labels][n_edges+1]: table 0 the eligible pairs whose bit is CLEAR, table 1 those whose bit is
 *   SET; a pair `eligible` or the bounds rule out is in neither, whatever its bit.  Nothing is excluded: the two tables sum to the
 *   unsplit counts exactly.  mask == NULL: table 0 is the unsplit result, table 1 zero, and no mask memory is read.
 *   Workspace: the size mdg_bilinear_ensemble_sigmoid_workspace_bytes gives (0 for F32).
 * Deterministic: the workgroups add their counts into `counts` with integer atomics, so the sums are bit-identical from launch to
 * launch. */
size_t mdg_bilinear_ensemble_bincount_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_models,
                                                      int precision);
int mdg_bilinear_ensemble_bincount(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                   const float* edges, int64_t* counts, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D,
                                   int n_edges, int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream);
int mdg_bilinear_ensemble_bincount_split(const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                                         int n_models, const float* edges, int64_t* counts, int64_t n_head, int64_t n_tail,
                                         int64_t n_labels, int64_t D, int n_edges, int precision, int eligible, void* workspace,
                                         size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);

/* Per-pair outcome profiles of the checkpoint ensemble (ABI 29): for every eligible pair (i,j), over the n_labels outcomes of the call,
 *   P[l,i,j]    = mean_m sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])
 *   count[i,j]  = #{l : P[l,i,j] >= thr[l]}                      (the compare is on the quotient, as mdg_bilinear_ensemble_select_*)
 *   margin[i,j] = max_l u_l,  u_l = (P[l,i,j] - thr[l]) * scale[l]  (a subtract, then a multiply, each rounded to fp32; scale == NULL: ones)
 *   best[i,j]   = the lowest l attaining that maximum
 * -- mdg_bilinear_profile's contract on the probability get_twosides_scores_wrapper / get_drugbank_scores_wrapper
 * (madrigal/evaluate/predict.py:466-499, 582-614) average over the checkpoints: "for how many interaction types does the five-seed
 * ensemble flag the pair at P >= 0.9, and which is its strongest", the per-pair reading of the stored tensor
 * (notebooks/quick_predictions.ipynb cell 8), without materialising [L,N,N].  The mean of sigmoids is not monotone in any one
 * model's logit, so neither the counts nor the best outcome can be merged from n_models mdg_bilinear_profile results.
 *   Operands as mdg_bilinear_ensemble_select_count (HOST arrays of n_models = 1..8 device pointers, 16-byte aligned, D == 128);
 *   precision MDG_PREC_F32 or MDG_PREC_BF16X3.  P is bit for bit what mdg_bilinear_ensemble_sigmoid's general sweep (z_head !=
 *   z_tail) writes: the same products, sigmoid 1 / (1 + expf(-s)), fp32 sum in model order, one division by K.
 *   thr [n_labels] fp32 (device), no NaN; scale [n_labels] fp32 (device), finite and > 0, or NULL.  Both are read back and checked
 *   before anything is launched, which synchronises `stream` once (as mdg_bilinear_profile).
 *   count, best (int32) and margin (fp32): [n_head, ldo], ldo >= n_tail.  The running state starts at 0 / -1 / -inf and moves only
 *   on u > margin: exact ties of u -- the rule here, many probabilities round to exactly 1 -- keep the lowest l.  A NaN probability
 *   is never counted and never best.  Ineligible pairs (eligible: mdg_topk_eligible; NOT_SELF / LOWER need n_head == n_tail) get
 *   0 / -1 / -inf.  Every entry [i < n_head, j < n_tail] is written, nothing at columns [n_tail, ldo).  n_labels == 0 writes
 *   0 / -1 / -inf everywhere.  n_labels <= 65535 per call (count and best share a register; merge chunks as for
 *   mdg_bilinear_profile), n_tail < 2^31 - 64, n_head <= 65535 * 128.
 *   mdg_bilinear_ensemble_profile_tiles: the 64-column tail tiles a workgroup owns (for tests that want sizes at that boundary).
 *   Workspace: the size mdg_bilinear_ensemble_sigmoid_workspace_bytes gives (0 for F32).
 * Deterministic: the state lives in registers, one store per entry after the last outcome; no atomics; bit-identical from launch
 * to launch. */
int mdg_bilinear_ensemble_profile_tiles(void);
size_t mdg_bilinear_ensemble_profile_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_models,
                                                     int precision);
int mdg_bilinear_ensemble_profile(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                  const float* thr, const float* scale, int32_t* count, int32_t* best, float* margin, int64_t ldo,
                                  int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision, int eligible,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Spread of the checkpoint ensemble: how much the n_models checkpoints agree on a pair.  For every outcome l, head row i, tail column j
 *   p_m   = sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])                    m = 0..K-1, K = n_models in 1..8
 *   mean  = (p_0 + ... + p_{K-1}) / K      bit for bit mdg_bilinear_ensemble_sigmoid's general sweep (z_head != z_tail) for the same call
 *   std   = sqrt((1/K) sum_m (p_m - mean)^2)                                 population standard deviation (ddof = 0, numpy's default)
 *   bound = fmaf(kappa, std, mean)                                           one rounding; kappa a finite fp32 scalar per call
 * get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) keep every checkpoint's
 * score tensor in memory before they average.  The reference has NO std call of its own: its users take np.stack(...).std(0) of
 * those stored tensors next to the .mean(0) it returns.  Here the per-checkpoint tensors never exist; the second moment is kept in
 * registers beside the running sum of the sweep.  kappa < 0 ranks by a lower confidence bound (hits the seeds agree on), kappa > 0
 * by an upper bound (contested pairs), kappa == 0 gives the mean bit for bit.  The bound is not monotone in the mean, so no
 * composition of the mean's lists gives its ranking.
 *   std is computed in fp32 by Welford's one-pass recurrence (mu += (p - mu) / n; M2 += (p - mu_old) * (p - mu_new)), which does
 *   not cancel; the running sum behind `mean` is untouched by it.  std >= 0 always, never NaN for finite logits, exactly 0.0f for
 *   K == 1 and whenever the K values p_m are equal.  Both entry points share the recurrence's text: their std and bound agree bit
 *   for bit.
 *   Operands as mdg_bilinear_ensemble_topk (HOST arrays of n_models device pointers, 16-byte aligned, D == 128); precision
 *   MDG_PREC_F32 or MDG_PREC_BF16X3; n_labels <= 65535 per call.  A non-finite kappa is refused before a launch.
 *   mdg_bilinear_ensemble_spread: the dense product.  mean, std, bound: fp32 [n_labels, n_head, ldo], ldo >= n_tail, ONE row pitch
 *     for all three (the layout of mdg_bilinear_allpairs_ld), 128 * ldo * 4 < 2^31; a NULL pointer skips that tensor, at least one
 *     must be given (kappa is ignored without `bound`, but must be finite).  Always the general sweep: no mirrored symmetric
 *     variant, no 16-bit outputs.  Nothing outside columns [0, n_tail) of a row is touched.
 *   mdg_bilinear_ensemble_spread_topk: for every outcome and head row the k <= 32 ELIGIBLE tail columns with the largest bound,
 *     ordered by (bound descending, column ascending), which is also the tie rule for what is kept.  bound [n_labels,n_head,k]
 *     fp32, idx [n_labels,n_head,k] int32, mean and std [n_labels,n_head,k] fp32: the kept column's own mean and std, equal bit for
 *     bit to the dense product's at idx.  Rows with fewer than k eligible columns are padded with -inf / -1 / NaN / NaN.
 *     eligible, k, n_tail, mask / plane_stride as mdg_bilinear_ensemble_topk (mask == NULL: the unmasked kernel, no mask memory is
 *     read).  Nothing of [L,N,N] is materialised.
 *   mdg_bilinear_ensemble_spread_chunk_tiles: the 64-column tail tiles a workgroup of either kernel sweeps between two rebuilds of
 *     the models' z_head . W_sym products (narrower than mdg_bilinear_ensemble_topk_chunk_tiles: three registers of state per
 *     element, not one); for tests that want sizes at that boundary.
 *   Workspace: the size mdg_bilinear_ensemble_sigmoid_workspace_bytes gives (0 for F32).
 * Deterministic: no atomics, the state and the lists live in registers; bit-identical from launch to launch. */
int mdg_bilinear_ensemble_spread_chunk_tiles(void);
size_t mdg_bilinear_ensemble_spread_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_models,
                                                    int precision);
int mdg_bilinear_ensemble_spread(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                 float* mean, float* std_, float* bound, float kappa, int64_t ldo, int64_t n_head, int64_t n_tail,
                                 int64_t n_labels, int64_t D, int precision, void* workspace, size_t workspace_bytes, void* stream);
int mdg_bilinear_ensemble_spread_topk(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                      float kappa, float* bound, int32_t* idx, float* mean, float* std_, int64_t n_head,
                                      int64_t n_tail, int64_t n_labels, int64_t D, int precision, int k, int eligible, void* workspace,
                                      size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);

/* Per-row top-k of the all-pairs sweep: for every outcome l and head row i the k largest scores S[l,i,j] (the arithmetic of
 * mdg_bilinear_allpairs' general sweep in `precision`, bit for bit in F32 / BF16X3; the 16-bit modes run the row-statistics
 * sweep, whose fp32 sums are grouped differently: <= 2e-6 of the scale) over the ELIGIBLE tail columns j, and those columns.
 * The screening product of the head -- "for this drug and outcome, which partners" -- without materialising [L,N,N]: what the
 * reference looks up in its stored score / rank tensor (notebooks/quick_predictions.ipynb cell 8) and, in LOWER mode, the
 * candidates of the pairs notebooks/normalize_scores.py:39-46 ranks.
 *   vals [n_labels,n_head,k] fp32, idx [n_labels,n_head,k] int32; each row ordered by (score descending, column ascending),
 *   which is also the tie rule for what is kept; a row with fewer than k eligible columns is padded with -inf / -1.
 *   eligible: MDG_TOPK_ALL (two drug sets), MDG_TOPK_NOT_SELF (j != i), MDG_TOPK_LOWER (j < i, the strict lower triangle;
 *   column tiles wholly on or above the diagonal are not computed); the last two need n_head == n_tail.
 *   1 <= k <= mdg_bilinear_topk_max_k() (32); n_tail >= 1 and < 2^31 - 64; n_labels <= 65535 per call; D == 128.
 * Scores must be finite (a NaN is never kept).  Workspace: the operand images of mdg_bilinear_allpairs (0 for F32).
 * Deterministic: no atomics, the lists live in registers; bit-identical from launch to launch. */
enum mdg_topk_eligible { MDG_TOPK_ALL = 0, MDG_TOPK_NOT_SELF = 1, MDG_TOPK_LOWER = 2 };
int mdg_bilinear_topk_max_k(void);
size_t mdg_bilinear_topk_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision, int k);
int mdg_bilinear_topk(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx, int64_t n_head,
                      int64_t n_tail, int64_t n_labels, int64_t D, int precision, int k, int eligible, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Per-outcome score counts of the all-pairs sweep: for every outcome l, given n_edges ascending finite fp32 edges e[l,0..B-1],
 *   counts[l,b] = #{eligible (i,j) : e[l,b-1] <= S[l,i,j] < e[l,b]},   e[l,-1] = -inf, e[l,B] = +inf        (b = 0..B)
 * -- torch.bucketize(S, e[l], right=True) followed by a bincount, without materialising [L,N,N].  The counting product of the head:
 * with the edges at the scores of screened hits, the cumulative counts give the hits' exact normalised ranks,
 * (1 + #{i>j : S[l,i,j] < s}) / (N (N-1) / 2), the value the reference computes by ranking the whole lower triangle
 * (notebooks/normalize_scores.py:36-74); with evenly spaced edges they are per-outcome score histograms.
 *   edges [n_labels,n_edges] fp32; counts [n_labels,n_edges+1] int64, zeroed by the call on `stream`; every row of counts sums
 *   to the number of eligible pairs.  Equal neighbouring edges give an empty bin.  Edges must be ascending within an outcome: the
 *   kernel cannot check that cheaply, and unsorted edges give unspecified counts (no out-of-bounds access).
 *   Scores and `eligible` (enum mdg_topk_eligible; LOWER skips the column tiles wholly on or above the diagonal) are those of
 *   mdg_bilinear_topk: bit for bit the general sweep's in F32 / BF16X3, <= 2e-6 of the scale off in the 16-bit modes.
 *   1 <= n_edges <= mdg_bilinear_bincount_max_edges() (1024); n_labels <= 65535 per call; D == 128; NOT_SELF / LOWER need
 *   n_head == n_tail.  n_tail < 2^23: a workgroup counts its up to 512 x n_tail scores in 32-bit counters; more is refused (MDG_EINVAL).
 * Scores must be finite (a NaN is counted nowhere).  Workspace: the operand images of mdg_bilinear_allpairs (0 for F32).
 * Deterministic: the workgroups add their counts into `counts` with integer atomics, so the sums are bit-identical from launch
 * to launch. */
int mdg_bilinear_bincount_max_edges(void);
size_t mdg_bilinear_bincount_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_edges, int precision);
int mdg_bilinear_bincount(const float* z_head, const float* z_tail, const float* w_sym, const float* edges, int64_t* counts,
                          int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_edges, int precision, int eligible,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Threshold selection inside the all-pairs sweep (ABI 15): for every outcome l with its cut thr[l], ALL eligible pairs (i,j) with
 *   S[l,i,j] >= thr[l]
 * as CSR over the n_labels * n_head rows (l,i), without materialising [L,N,N].  The set-valued product of the head -- "every pair
 * above a cut", the predicted interaction network of an outcome -- whose size is not known beforehand, hence two sweeps:
 *   mdg_bilinear_select_count: row_counts [n_labels,n_head] int32, the number of selected columns of every row (every entry is
 *     written, zeros included).  The caller's exclusive prefix sum over the flattened counts is row_ptr.
 *   mdg_bilinear_select_fill:  row_ptr [n_labels*n_head + 1] int64; cols [T] int32 and vals [T] fp32, T = row_ptr[last]: the
 *     selected columns of row (l,i) in ASCENDING order and their scores at [row_ptr[l*n_head+i], row_ptr[l*n_head+i+1]) --
 *     canonical CSR, the order torch.nonzero gives on the dense mask (S >= thr) & eligible.
 * The reference has no function of this kind: it reads such sets off its stored score / rank tensor; in LOWER mode the pairs
 * are those of the strict lower triangle notebooks/normalize_scores.py:39-46 ranks.
 *   The rule is >= (it matches the edges of mdg_bilinear_bincount, e <= S, and a cut at the K-th best value includes that
 *   value); thr = -inf selects every eligible pair, +inf none; a NaN score is never selected and a NaN cut selects nothing.
 *   Scores and `eligible` (enum mdg_topk_eligible; LOWER skips the column tiles wholly on or above the diagonal) are those of
 *   mdg_bilinear_topk: bit for bit the general sweep's in F32 / BF16X3, <= 2e-6 of the scale off in the 16-bit modes (there a
 *   score within that distance of the cut may fall on either side of it; count and fill agree with each other exactly).
 *   n_tail >= 1 and < 2^31 - 64; n_labels <= 65535 per call; D == 128; NOT_SELF / LOWER need n_head == n_tail.
 * Deterministic: every row belongs to one wave that walks the column tiles in ascending order; no atomics; bit-identical from
 * launch to launch.  Bounded writes: the fill pass stores slot s of row r only if 0 <= row_ptr[r] <= s < row_ptr[r+1]; with a
 * row_ptr that does not match thr (stale counts) rows are truncated or left partly unwritten, and nothing is stored outside
 * [row_ptr[r], row_ptr[r+1]).  All slot arithmetic is 64-bit.  Workspace: the operand images of mdg_bilinear_allpairs (0 for F32). */
size_t mdg_bilinear_select_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision);
int mdg_bilinear_select_count(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, int32_t* row_counts,
                              int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision, int eligible,
                              void* workspace, size_t workspace_bytes, void* stream);
int mdg_bilinear_select_fill(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const int64_t* row_ptr,
                             int32_t* cols, float* vals, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D,
                             int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream);

/* Known-pair exclusion masks for the in-sweep products (ABI 16).  A screening run looks for NEW interactions: the pairs already
 * in the training network score highest by construction and would fill the 32-entry lists of mdg_bilinear_topk; with the dense
 * tensor the reference's users index them away, without the tensor the restriction has to act inside the sweep.
 *   Layout: mask [planes][ceil(n_head / 32)][ld] 32-bit words, ld = mdg_pair_mask_ld(n_tail) = n_tail rounded up to 64; the word at
 *   [p][i >> 5][j] holds the bit of head row i and tail column j at position i & 31.  A SET bit means "(i, j) is not eligible".
 *   mdg_pair_mask_plane_words(n_head, n_tail) = ceil(n_head / 32) * ld is the size of one plane.  These two functions are the only
 *   place the arithmetic lives.  Bits of pad columns [n_tail, ld) and of pad rows [n_head, 32 ceil(n_head / 32)) are ignored.
 *   mdg_pair_mask_set: ORs the bits of n_pairs listed pairs (heads[q], tails[q]) into plane planes[q] (planes == NULL: plane 0)
 *   of a mask the CALLER has zeroed (or that already holds bits: the call only adds); symmetric != 0 also sets (tails[q], heads[q])
 *   and needs n_head == n_tail.  One thread per pair, one integer atomic OR per bit: duplicates and order do not matter, the
 *   result is deterministic.  A pair with an index outside [0,n_head) x [0,n_tail) x [0,n_planes) is skipped, never stored.
 *   The *_masked entry points take the arguments of their twins plus `mask` (device, 4-byte aligned) and `plane_stride`, the
 *   distance in words between the planes of consecutive outcomes of THIS call: 0 shares one plane between all outcomes, otherwise
 *   >= mdg_pair_mask_plane_words.  An element is eligible when `eligible` allows it AND its bit is clear; an excluded element is
 *   treated exactly like an ineligible one (top-k: never kept, padding -inf / -1 when fewer than k remain; select: never counted
 *   or stored), so order, tie rule, CSR order, bounded writes and determinism are those of the twins, and the scores that remain
 *   are bit for bit the twins'.  mask == NULL forwards to the twin.  The kernels read words [0, ceil(n_head/32)) x [0, ld) of a
 *   plane and nothing else.  Workspace: the twin's query.
 *   Counting excludes nothing: a normalised rank is defined over all N (N - 1) / 2 pairs (notebooks/normalize_scores.py:57), so
 *   mdg_bilinear_bincount takes no mask and its counts stay what they are.  mdg_bilinear_bincount_split (ABI 20) takes the
 *   arguments of mdg_bilinear_bincount plus `mask` and `plane_stride` (the rules above) and counts the two classes SEPARATELY in
 *   the same sweep: counts is int64 [2][n_labels][n_edges + 1], zeroed by the call on `stream`; table 0 holds the eligible pairs
 *   whose bit is CLEAR, table 1 those whose bit is SET; a pair that `eligible` or the bounds rule out is counted in neither,
 *   whatever its bit (a symmetric mask has bits on the diagonal and above it: under LOWER they change nothing).  The two tables
 *   sum to the counts of mdg_bilinear_bincount exactly, in all four precisions: it is the same sweep, and the scores are the
 *   twin's bit for bit.  With the known network as the mask, the cumulative sums of table 1 are the known pairs below every edge:
 *   exact precision / recall / enrichment at any cut and AUROC bounds over the whole pair universe, per outcome, in one pass.
 *   mask == NULL: table 0 is the twin's result, table 1 is zero.  Refusals are the twin's plus the mask's alignment and
 *   plane_stride; a refused call launches nothing and leaves `counts` untouched.  Workspace: mdg_bilinear_bincount_workspace_bytes.
 *   Deterministic like the twin: integer device-scope adds, bit-identical from launch to launch. */
int64_t mdg_pair_mask_ld(int64_t n_tail);
int64_t mdg_pair_mask_plane_words(int64_t n_head, int64_t n_tail);
int mdg_pair_mask_set(uint32_t* mask, int64_t n_planes, int64_t n_head, int64_t n_tail, const int64_t* heads, const int64_t* tails,
                      const int64_t* planes, int64_t n_pairs, int symmetric, void* stream);
int mdg_bilinear_topk_masked(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx, int64_t n_head,
                             int64_t n_tail, int64_t n_labels, int64_t D, int precision, int k, int eligible, void* workspace,
                             size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);
int mdg_bilinear_select_count_masked(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, int32_t* row_counts,
                                     int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision, int eligible,
                                     void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);
int mdg_bilinear_select_fill_masked(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const int64_t* row_ptr,
                                    int32_t* cols, float* vals, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D,
                                    int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream,
                                    const uint32_t* mask, int64_t plane_stride);
int mdg_bilinear_bincount_split(const float* z_head, const float* z_tail, const float* w_sym, const float* edges, int64_t* counts,
                                int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int n_edges, int precision, int eligible,
                                void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride);

/* Per-pair outcome profiles of the all-pairs sweep (ABI 19): the reduction of the sweep over the OUTCOMES instead of over the pairs.
 * With S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j], per-outcome cuts thr[l] and scales scale[l] (finite, > 0; NULL = all ones), three
 * [n_head, ldo] matrices (row pitch ldo >= n_tail elements) -- for every eligible pair (i,j), over the n_labels outcomes of the call:
 *   count[i,j]  int32 = #{l : S[l,i,j] >= thr[l]}              (the compare is on S itself: the test of mdg_bilinear_select_*)
 *   margin[i,j] fp32  = max_l u_l,  u_l = (S[l,i,j] - thr[l]) * scale[l]   (a subtract, then a multiply, each rounded to fp32)
 *   best[i,j]   int32 = the smallest l attaining that maximum
 * The running state starts at margin = -inf, best = -1 and moves only on u > margin, so a pair whose every u is -inf (thr = +inf)
 * or NaN keeps best = -1; a NaN score is never counted and never best.  Ineligible pairs (enum mdg_topk_eligible: the diagonal in
 * NOT_SELF, j >= i in LOWER) get count 0, best -1, margin -inf.  EVERY entry [i,j] with i < n_head, j < n_tail is written (callers
 * need no zeroing); nothing at columns [n_tail, ldo) is touched.  "How many outcomes is this pair flagged for, and which is its
 * strongest": the reference has no function of this kind; it reads such summaries off its stored score tensor.
 *   Scores: in ALL FOUR precisions bit for bit those of mdg_bilinear_allpairs' general sweep (MDG_EPI_STORE); the 16-bit modes run
 *   the same 32x32x16 products here, not the regrouped sums of the row-statistics sweeps.
 *   D == 128; n_labels <= 65535 per call (count and best share a register; merge chunks on the caller's side: counts add, the
 *   larger margin wins, equal margins keep the lower outcome); n_tail < 2^31 - 64; n_head <= 65535 * 256; NOT_SELF / LOWER need
 *   n_head == n_tail.  thr may be +-inf; a NaN in thr, or a scale that is not finite and > 0, is refused with MDG_EINVAL: the call
 *   reads thr and scale back and synchronises `stream` once before it launches (so it cannot be captured into a graph).  A refused
 *   call launches nothing.  n_labels == 0 writes the ineligible values everywhere.
 * Deterministic: a workgroup owns a tile of pairs, walks the outcomes in ascending order and keeps the state in registers; no
 * atomics; bit-identical from launch to launch.  LOWER does no product work for tiles wholly on or above the diagonal.
 * Workspace: the operand images of mdg_bilinear_allpairs (0 for F32). */
size_t mdg_bilinear_profile_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D, int precision);
int mdg_bilinear_profile(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const float* scale,
                         int32_t* count, int32_t* best, float* margin, int64_t ldo, int64_t n_head, int64_t n_tail,
                         int64_t n_labels, int64_t D, int precision, int eligible, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Streaming per-pair top-k over the OUTCOME axis of a score or rank tensor (ABI 24): one chunk x [n_labels, n_head, n_tail] is
 * folded into a running state vals fp32 / idx int32 [k, n_head, n_tail], per pair (i, j) the k best (value, outcome id) of
 * everything folded so far.  Replaces the per-pair "highest 5" reductions the reference runs over its stored [L,N,N] rank tensor:
 * notebooks/fig5/fig5_t2d_mash.ipynb:1442-1448 (np.mean(np.partition(lst, len(lst)-5)[-5:])), :2034-2039 (highest_5_ddi_classes /
 * highest_5_scores / highest_5_mean) and, with largest = 0, the lowest 5 at :2050.
 *   x: element (l, i, j) at x[l * x_outcome_stride + i * ldx + j]; x_type 0 = fp32, MDG_SCORE_F16, MDG_SCORE_BF16 (16-bit values are
 *   widened to fp32 exactly); ldx >= n_tail; aligned to its element size.  labels int32 [n_labels] or NULL: the global outcome id of
 *   each plane (NULL: label_base + l); a plane with a negative label is skipped (the reference's to_delete_classes).  shift, scale
 *   fp32 [n_labels], each or both NULL: the value folded is (x - shift[l]) * scale[l], a subtract, then a multiply, each rounded to
 *   fp32 (never an FMA; NULL = 0 / 1, which leaves x's bits).  Their values are NOT checked here (callers pass finite shifts and
 *   finite scales > 0): the call enqueues on `stream`, needs no workspace and does not synchronise.
 *   State: element (s, i, j) of vals / idx at [s * state_plane_stride + i * lds + j] (one plane stride and one pitch for both,
 *   lds >= n_tail), 1 <= k <= 8.  fresh != 0: the incoming state is ignored.  largest 1 / 0.  eligible: MDG_TOPK_ALL, or
 *   MDG_TOPK_LOWER (only entries with i > j).
 * Semantics, exact and independent of how the outcomes are split into calls and of the order of the calls: slot s of a pair holds
 * the s-th element of all folded (value, id) under ONE total order -- value descending, then id ascending (largest = 0: value
 * ascending, then id ascending).  Empty slots hold (-inf, -1) ((+inf, -1) with largest = 0).  A NaN is never kept, nor is a value
 * equal to the sentinel value.  Values are copies (or the two-step expression above), so results compare bit for bit.  With LOWER
 * and fresh the entries with i <= j receive the sentinels; without fresh they are left untouched.  Nothing outside columns
 * [0, n_tail) of the k * n_head state rows is written, pitch padding included.  n_labels == 0 with fresh writes the sentinels.
 *   Rows of x and of the state that all start on 16 bytes (bases, pitches and strides) move 16 bytes per lane; any other layout
 *   takes an element path, correct and several times slower.  n_head * ceil(n_tail / 256) workgroups must fit 2^31 - 1.
 * Deterministic: a lane owns its pairs' lists in registers over the whole chunk; no atomics, no LDS. */
int mdg_outcome_topk_update(const void* x, int x_type, int64_t x_outcome_stride, int64_t ldx, const int32_t* labels,
                            int64_t label_base, const float* shift, const float* scale, float* vals, int32_t* idx,
                            int64_t state_plane_stride, int64_t lds, int64_t n_head, int64_t n_tail, int64_t n_labels, int k,
                            int fresh, int largest, int eligible, void* stream);

/* ------------------------------------------------------------------------ dense blocks ---- */

/* Y = alpha * act( (X W^T + bias) * scale + shift ) + beta * R      X [M,K] ldx, W [N,K] ldw (nn.Linear
 * layout), Y [M,N] ldy, R [M,N] ldr; bias/scale/shift [N]; any of bias, scale+shift, R may be NULL.
 * Replaces every nn.Linear (+ eval BatchNorm1d folded into scale/shift, + activation, + residual) on
 * the path: MLPEncoder/MLPAdaptor madrigal/models/models.py:178-180,516-518; chemCPA MLP
 * madrigal/chemcpa/chemCPA/model.py:226-231; nn.TransformerEncoderLayer linears models.py:366;
 * embed2latent / latent2embed models.py:411,443; GIN and HGT projections (third-party wheels).
 * K, ldx, ldw multiples of 4 (zero-pad the inner dimension), x and w 16-byte aligned.  ldr == 0 broadcasts one
 * residual row.  The kernel stages "operand images" (K zero-padded to 32; bf16 modes: hi [+ lo] bf16 planes): the
 * image of x (and of w unless w_packed is given) is written into `workspace` by a fused pre-pass; a weight that is
 * reused can be packed once with mdg_pack_operand and passed as w_packed (w may then be NULL). */
size_t mdg_pack_operand_bytes(int64_t rows, int64_t K, int precision);        /* 0: the raw fp32 tensor is used as is */
int mdg_pack_operand(const float* src, int64_t ld, int64_t rows, int64_t K, int precision, void* dst, size_t dst_bytes,
                     void* stream);
/* Image of src^T from src [rows, cols] in one transposing pass (16-bit modes; mdg_pack_operand_bytes(cols, rows, precision) bytes):
 * the weight image of the backward product dx = g W (a dense block with weight W^T) without materialising W^T. */
int mdg_pack_operand_transposed(const float* src, int64_t ld, int64_t rows, int64_t cols, int precision, void* dst, size_t dst_bytes,
                                void* stream);
/* Rows gathered across up to MDG_GATHER_MAX_SOURCES fp32 matrices of one width, standing for
 * torch.cat(sources).index_select(0, idx) without the concatenated copy (the reference stacks the 16 per-cell-line signature
 * matrices, madrigal/models/models.py:753-769, and the [str | kg | cv | tx] embeddings, :781-790, before it indexes them):
 *   out[i, :] = sources[idx[i] / rows_per_source][idx[i] % rows_per_source, :]          i in [0, n)
 * sources_host / source_rows_host / source_ld_host are HOST arrays of n_sources entries (device pointer, row count <=
 * rows_per_source, row stride in floats >= width); idx is a DEVICE array.  An index that is negative or names a row its source
 * does not have gathers a zero row (nothing outside the sources is ever read).  out (nullable) [n, ldo] receives the rows with
 * the columns from width up to width rounded up to 4 zeroed (ldo % 4 == 0); image (nullable; 16-bit modes) receives the same rows as
 * the operand image of mdg_linear_packed_x: the bytes mdg_pack_operand writes for out, mdg_pack_operand_bytes(n, width rounded
 * up to 4, precision) of them.  Sources need 4-byte alignment only; wider loads are used where every row allows them. */
int mdg_gather_rows_multi(const float* const* sources_host, const int64_t* source_rows_host, const int64_t* source_ld_host,
                          int n_sources, int64_t rows_per_source, int64_t width, const int64_t* idx, int64_t n, float* out,
                          int64_t ldo, void* image, size_t image_bytes, int precision, void* stream);
size_t mdg_linear_workspace_bytes(int64_t M, int64_t N, int64_t K, int precision, int w_is_packed);
/* (ABI 18) Edge of the output tile mdg_linear (and its _dropout / _packed_x forms) runs an [M, N] product on: 256 or 128.  The launch path's
 * own decision (shape, precision, MDG_LINEAR_TILE; re-read after mdg_tuning_reload()); launches nothing, needs no device.
 * mdg_linear_rowscaled takes the 128-tile kernel unless MDG_LINEAR_TILE says otherwise. */
int mdg_linear_tile(int64_t M, int64_t N, int precision);
int mdg_linear(const float* x, int64_t ldx, const float* w, int64_t ldw, const void* w_packed, float* y, int64_t ldy, int64_t M,
               int64_t N, int64_t K, const float* bias, const float* scale, const float* shift, int activation,
               const float* residual, int64_t ldr, float alpha, float beta, int precision, void* workspace,
               size_t workspace_bytes, void* stream);
/* Training form: y = dropout(act(x W^T + b), drop_p, drop_seed) + beta * residual in the same epilogue (nn.TransformerEncoderLayer's
 * x + dropout1(out_proj(...)), x + dropout2(linear2(...)), dropout(activation(linear1(x)))): the mask and scale are exactly those of
 * mdg_dropout(seed) on the contiguous [M,N] result, so the fused block equals the three separate launches bit for bit. */
int mdg_linear_dropout(const float* x, int64_t ldx, const float* w, int64_t ldw, const void* w_packed, float* y, int64_t ldy,
                       int64_t M, int64_t N, int64_t K, const float* bias, int act, const float* residual, int64_t ldr, float beta,
                       float drop_p, uint64_t drop_seed, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* Row-wise LayerNorm (nn.LayerNorm, biased variance): y = (x - mean) / sqrt(var + eps) * gamma + beta.
 * norm1/norm2 and the x-attn norms of the fusion transformer, models.py:366,372-373; LayerNorm inside
 * MLPAdaptor, models.py:492.  d multiple of 4, <= 2048. */
int mdg_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y, int64_t ldy, int64_t rows,
                  int64_t d, float eps, void* stream);
/* LayerNorm that also writes y as the packed operand image of the dense block consuming it (mdg_pack_operand_bytes(rows, d,
 * precision) bytes, bit-identical to mdg_linear's own pre-pass; 16-bit modes, d a multiple of 32; y may be NULL when only
 * the image is wanted), and mdg_linear on such an
 * image: the norm -> projection pairs of nn.TransformerEncoderLayer (models.py:366) without the pre-pass in between. */
int mdg_layernorm_packed(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y, int64_t ldy, int64_t rows,
                         int64_t d, float eps, int precision, void* y_packed, size_t y_packed_bytes, void* stream);
size_t mdg_linear_packed_x_workspace_bytes(int64_t M, int64_t N, int64_t K, int precision, int w_is_packed);
int mdg_linear_packed_x(const void* x_packed, int64_t M, int64_t K, const float* w, int64_t ldw, const void* w_packed, float* y,
                        int64_t ldy, int64_t N, const float* bias, int act, const float* residual, int64_t ldr, float alpha,
                        float beta, int precision, void* workspace, size_t workspace_bytes, void* stream);
/* Layer 0 of the fusion transformer (models.py:401-455: embed2latent, then norm1 -> self_attn.in_proj of the first
 * nn.TransformerEncoderLayer) with norm1 and embed2latent folded into one short-K weight: QKV = rstd (T M^T + c) + c2 over the
 * 128-wide token rows T.  mdg_row_rstd writes the one number per row the fold leaves over, rstd[r] = 1 / sqrt(var(h[r]) + eps)
 * (the factor mdg_layernorm applies to row r of h, bit for bit; d multiple of 4, <= 2048).  mdg_linear_rowscaled is mdg_linear
 * with the row-scaled epilogue y[m, n] = row_scale[m] * ((x W^T)[m, n] + bias_pre[n]) + bias[n] (bias_pre and bias nullable),
 * on the 128-tile kernel; workspace: mdg_linear_workspace_bytes. */
int mdg_row_rstd(const float* x, int64_t ldx, float* rstd, int64_t rows, int64_t d, float eps, void* stream);
int mdg_linear_rowscaled(const float* x, int64_t ldx, const float* w, int64_t ldw, const void* w_packed, float* y, int64_t ldy,
                         int64_t M, int64_t N, int64_t K, const float* row_scale, const float* bias_pre, const float* bias,
                         int precision, void* workspace, size_t workspace_bytes, void* stream);
/* A chain of 128-wide dense blocks as ONE launch (ABI 11): the dense part of a GIN layer in inference -- torchdrug's
 * GraphIsomorphismConv as used at madrigal/models/models.py:217,720: edge_linear on the summed bond features added to the
 * aggregated rows, the conv's MLP, eval BatchNorm and the activation --
 *   u0 = e . We^T + x                          (only when e != NULL: e [M, k_e], We [k_in, k_e]; x [M, k_in] is then its residual)
 *   u1 = act(u0 . W1^T + b1)   u2 = act(u1 . W2^T + b2)   ...   y = act((u . Wn^T + bn) * scale + shift)      n = n_stages in 1..3
 * W1 [128, k_in], W2 / W3 [128, 128]; k_in, k_e multiples of 4 in (0, 128]; N must be 128; y [M, 128] with ldy % 4 == 0.
 * The intermediate rows stay on the CU; every stage is bit-identical to the mdg_linear call it replaces.  All weights are given
 * as their operand images (mdg_pack_operand with the same precision: We as [k_in, k_e], the others as [128, K]); biases,
 * scale and shift nullable ([128] each, scale and shift together).  16-bit modes only (MDG_PREC_BF16X3 / MDG_PREC_BF16); all
 * pointers 16-byte aligned; no workspace. */
int mdg_linear_chain128(const float* x, int64_t ldx, int64_t k_in, const float* e, int64_t lde, int64_t k_e, const void* we_packed,
                        int n_stages, const void* w1_packed, const void* w2_packed, const void* w3_packed, const float* b1,
                        const float* b2, const float* b3, const float* scale, const float* shift, int act, float* y,
                        int64_t ldy, int64_t M, int64_t N, int precision, void* stream);

/* ------------------------------------------------------------------- cross-modal fusion ---- */

/* Token sequence of the fusion transformer: seq[i] = [cls?] str kg cv [bottleneck x nb] tx_0..tx_15
 * (each a 128-float row), optional per-token L2 normalisation, then + pe[s] for s < pe_len.
 * Replaces the stack / cat / repeat glue and PositionEncoding* of madrigal/models/models.py:772-775,
 * 799-804,818-822,849-852,581-603.  tx_emb is [16 * n_src, 128], cell-line major.  rows (nullable) selects
 * source drug rows (the multi-modal subset of fusion='transformer_uni_proj', models.py:784-790).
 * token_index (nullable, [n_tok] values i*S+s): emit only those tokens, densely packed -> seq [n_tok,128]. */
int mdg_assemble_tokens(const float* str_emb, const float* kg_emb, const float* cv_emb, const float* tx_emb,
                        const float* bottleneck, const float* cls, const float* pe, const int64_t* rows, const int64_t* token_index,
                        int64_t n_tok, float* seq, int64_t n, int64_t n_src, int nb, int has_cls, int pe_len, int normalize,
                        int64_t D, void* stream);

/* Multi-head self-attention core for S <= 32 tokens per drug (scores, masks, softmax, PV) on the fp32
 * matrix cores; projections are mdg_linear calls.  qkv [n*S, 3d] = q|k|v (in_proj output), out [n*S, d].
 * kpm_bits[i] bit j = key j of drug i is padding (src_key_padding_mask), src_bits[s] bit j = query s
 * may not attend key j (the [S,S] bottleneck mask, models.py:813-816); probs (nullable) receives the
 * per-head attention weights [n,H,S,S] (need_weights=True, average_attn_weights=False, models.py:388-399).
 * Compact mode (row_start != NULL): padded tokens are not stored at all -- qkv / out hold only each drug's
 * live tokens, rows row_start[i] .. row_start[i+1]-1 (at most 32), and row_bits[r] bit j says that query row r
 * may not attend its drug's j-th live key (kpm_bits / src_bits are ignored, probs must be NULL).  Padded
 * tokens never influence live ones, so the live rows equal the dense result.
 * Replaces nn.MultiheadAttention inside nn.TransformerEncoderLayer, models.py:366-367,412. */
int mdg_fusion_attention(const float* qkv, int64_t ld, float* out, int64_t ldo, const uint32_t* kpm_bits,
                         const uint32_t* src_bits, float* probs, const int64_t* row_start, const uint32_t* row_bits, int64_t n,
                         int S, int H, int dh, void* stream);
/* The same forward pass with q, k and v as operands of their own (ABI 13; no weights out): each with its row stride and a column step
 * from one head to the next (hq / hk / hv; 0 = one block of columns shared by every head), ds columns in the score product and dv
 * in the value product (multiples of 4, at most 1024; a partial last 64-column piece is zero-filled), out with its own row stride
 * ldo and head step ho >= dv.  Masks and compact mode as above.  With q = qkv, k = qkv + d, v = qkv + 2d, steps dh and
 * qscale = 1/sqrt(dh) the result is mdg_fusion_attention's bit for bit.
 * Layer 0 of a pre-norm fusion transformer in token space (TransformerFusion._layer0_tokenspace): h = T W_e^T + b_e has rank
 * <= D, so with x_j = r_j [T_j; 1] (r = norm1's per-row factor) the logits are x_j . u_h,i and the head outputs V~_h sum_j P x_j:
 * k = v = X [R, Dp] shared by the heads, q = U [R, H*Dp] from mdg_linear_rowscaled, qscale = 1, and out_proj runs on [O | T].
 * mdg_token_scaled_rows makes X, r and the T columns behind O from the token rows (D = 128, Dp = 132):
 *   r[i] = 1 / sqrt(|R_f [T_i; 1]|^2 / d + eps)   (rf [nr <= Dp, Dp] row-major: |R_f [T;1]| = |W_c T + b_c|, W_c / b_c centred)
 *   X[i] = r[i] [T_i, 1, 0, 0, 0]   (ldx >= Dp),   tail[i] = T_i   (ldtail >= D; all row strides multiples of 4, 16-byte aligned). */
int mdg_fusion_attention_qkv(const float* q, int64_t ldq, int hq, const float* k, int64_t ldk, int hk, const float* v, int64_t ldv,
                             int hv, float* out, int64_t ldo, int ho, const uint32_t* kpm_bits, const uint32_t* src_bits,
                             const int64_t* row_start, const uint32_t* row_bits, int64_t n, int S, int H, int ds, int dv,
                             float qscale, void* stream);
int mdg_token_scaled_rows(const float* tokens, int64_t ldt, const float* rf, int nr, int64_t D, int64_t d, float eps, float* X,
                          int64_t ldx, float* tail, int64_t ldtail, float* rstd, int64_t rows, void* stream);
/* The last layer of the fusion transformer in inference, where only the rows that are pooled continue past the attention (ABI 27;
 * models.py:401-455 with the pooling of :422-443 reading the bottleneck tokens alone; TransformerFusion._layer with keep_rows).
 * Keys and values are needed for all R live rows, queries and outputs for the n_keep kept rows only.  q_slot [R]: the compact index
 * of a kept row, negative for a row that is not kept (a slot >= n_keep counts as not kept).
 *   mdg_layernorm_packed_kept   mdg_layernorm_packed without the fp32 rows, plus a second image y_kept of n_keep rows
 *                               (mdg_pack_operand_bytes(n_keep, d, precision) bytes): row q_slot[r] of it is row r of y_packed, so
 *                               y_kept equals mdg_pack_operand of the kept fp32 rows gathered in slot order, bit for bit.
 *                               16-bit modes, d a multiple of 64.
 *   mdg_fusion_attention_kept   compact mode of mdg_fusion_attention (row_start [n+1] the tile table, row_bits [R]) with q
 *                               [n_keep, ldq] and out [n_keep, ldo] holding the kept rows in slot order, k and v [R, ld] with their
 *                               own base pointers.  Row q_slot[r] of out equals row r of mdg_fusion_attention's output bit for bit;
 *                               query rows that are not kept are never read.  No weights out, no dropout. */
int mdg_layernorm_packed_kept(const float* x, int64_t ldx, const float* gamma, const float* beta, int64_t rows, int64_t d, float eps,
                              int precision, void* y_packed, size_t y_packed_bytes, const int* q_slot, int64_t n_keep, void* y_kept,
                              size_t y_kept_bytes, void* stream);
int mdg_fusion_attention_kept(const float* q, int64_t ldq, const float* k, const float* v, int64_t ld, float* out, int64_t ldo,
                              const int64_t* row_start, const uint32_t* row_bits, const int* q_slot, int64_t n_keep, int64_t n, int H,
                              int dh, void* stream);

/* Cross-attention pooling with one learned query shared by all drugs: out[i,h,:] = softmax_j(q_h . K_ijh / sqrt(dh)) V_ijh.
 * q_proj [H*dh] (already projected), kv_proj [n*Tk, 2*H*dh] = K|V of the Tk allowed key tokens of each drug.
 * Replaces x_attn_mha_layer, madrigal/models/models.py:430-438. */
int mdg_xattn_pool(const float* q_proj, const float* kv_proj, int64_t ld, float* out, int64_t ldo, int64_t n, int Tk, int H, int dh,
                   void* stream);
/* The same pooling in eval mode with a pre-norm layer, folded through V, out_proj, the query residual and latent2embed
 * (models.py:422-443; TransformerFusion._x_attn_pool_folded).  With u_t = x_attn_kv_norm(h_t) the kept key rows:
 *   logit[t, h] = u_t . G[h]                      G [H, d] = W_k,h^T qp_h / sqrt(dh) (the query bias term cancels in the softmax)
 *   P = U [C_1; ...; C_H]^T  [n*Tk, H*D]         C_h = W_le W_o[:, h] W_v,h [D, d]
 *   z[i] = sum_h sum_t softmax_t(logit[i*Tk + t, h]) P[i*Tk + t, h*D : (h+1)*D] + cz     (cz = W_le (W_o b_v + b_o + q) + b_le)
 * mdg_layernorm_logits is mdg_layernorm_packed that also writes logits [rows, H] (H <= 64) from the normalised fp32 rows;
 * y_packed may be NULL (fp32 rows only, any precision), y may be NULL (image only); y and the image equal mdg_layernorm_packed's
 * bit for bit.  mdg_xattn_fold_pool writes z [n, D] from P and the logits (Tk <= 32, D even and <= 256, fixed summation order). */
int mdg_layernorm_logits(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y, int64_t ldy, int64_t rows,
                         int64_t d, float eps, int precision, void* y_packed, size_t y_packed_bytes, const float* G, int H,
                         float* logits, void* stream);
int mdg_xattn_fold_pool(const float* P, int64_t ldp, const float* logits, int64_t ldl, const float* cz, float* z, int64_t ldz,
                        int64_t n, int Tk, int H, int D, void* stream);

/* y = x / max(||x||_2, 1e-12) per row (F.normalize; models.py:849-850,858-859,872,892-893,947-949). d % 4 == 0. */
int mdg_l2_normalize(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t d, void* stream);

/* Masked pooling over the S <= 32 tokens [n,S,128] of each drug; tokens whose bit is set in mask_bits[i] are
 * skipped.  mode 0 = mean, 1 = sum, 2 = max.  Replaces the torch_scatter scatter_mean / scatter_add /
 * scatter_max call sites madrigal/models/models.py:447,451,873,878. */
int mdg_token_pool(const float* tokens, const uint32_t* mask_bits, float* out, int64_t n, int S, int64_t D, int mode, void* stream);

/* ------------------------------------------------------------------- graph aggregations ---- */

/* out[v] = (self_coef_add + *self_coef_dev) * x_self[v] + sum_{e in CSR row v} w[e] * x[col[e]]   (mean: sum / count)
 * col == NULL: the row's neighbours are the contiguous rows [rowptr[v], rowptr[v+1]) of x (segment read-out).
 * Replaces torchdrug GraphIsomorphismConv.message_and_aggregate (sparse.mm + scatter_add) and MeanReadout
 * behind madrigal/models/models.py:217,720-721.  F multiple of 4, <= 256. */
int mdg_csr_aggregate(const float* x, int64_t ldx, const int64_t* rowptr, const int64_t* col, const float* edge_weight,
                      const float* x_self, int64_t ld_self, const float* self_coef_dev, float self_coef_add, int mean, float* out,
                      int64_t ldo, int64_t n_dst, int64_t F, void* stream);

size_t mdg_hgt_attention_workspace_bytes(int64_t n_items, int heads);

/* HGT edge attention + aggregation for one destination node type: per-head softmax over ALL incoming edges
 * of a node (every edge type), weighted sum of relation-transformed values, optional GELU.
 * q [n_dst, ldq>=128]; edge e reads k' at kv + col[e]*ldkv and v' 128 floats later (relation transforms and
 * p_rel/sqrt(D) already applied; ldkv >= 128, with ldkv == 128 the value is simply the next row);
 * col[e] = kv row of edge e, edges sorted by destination; work items (item_dst, item_begin, item_end) split
 * long destination rows, item_ptr [n_dst+1] = items of each destination.
 * Replaces PyG HGTConv.propagate/message (edge softmax + scatter-add) behind models.py:76-79,90-94. */
int mdg_hgt_attention(const float* q, int64_t ldq, const float* kv, int64_t ldkv, const int64_t* col, const int64_t* item_dst,
                      const int64_t* item_begin, const int64_t* item_end, int64_t n_items, const int64_t* item_ptr, float* out,
                      int64_t ldo, int64_t n_dst, int heads, int64_t F, int apply_gelu, void* workspace, size_t workspace_bytes,
                      void* stream);
/* The same for ALL destination node types of a conv in one launch: destinations numbered across the types, query row of
 * destination d at q_base + q_off[d] floats (the types' projection rows differ in width), items / edges / item_ptr of the types
 * concatenated, out [n_dst,128].  (PyG HGTConv runs its message passing per edge type: models.py:76-79.) */
int mdg_hgt_attention_rows(const float* q_base, const int64_t* q_off, const float* kv, int64_t ldkv, const int64_t* col,
                           const int64_t* item_dst, const int64_t* item_begin, const int64_t* item_end, int64_t n_items,
                           const int64_t* item_ptr, float* out, int64_t ldo, int64_t n_dst, int heads, int apply_gelu,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same attention carried out in node-feature space (inference; 4 heads of 32).  Where the relation-transformed key and
 * value of an edge are affine images of the source node's 128-float feature row, the logits are u . x + c with the
 * destination-side block ut [n_dst, n_rel, 4, 132] = [ K^T q (128) | q . kappa | 0 0 0 ] per (destination, relation, head), and
 * the result is st [n_rel, n_dst, 4, 132] (relation-major: one [n_dst, 528] operand per relation for the value block) =
 * [ sum_e p_h(e) x_src(e) (128) | sum_e p_h(e) | 0 0 0 ] over the edges of each relation, p the per-head softmax over ALL
 * incoming edges of the destination (exp / (sum + 1e-16)); rows of relations or destinations without edges are zero.
 * x [n_rows, ldx >= 128] stacked feature rows; src[e] (32-bit) = row of edge e, the nnz edges sorted by (destination,
 * relation); work items of one (item_dst, item_rel) each; rel_ptr [n_dst * n_rel + 1] = first item of every (destination,
 * relation).  Deterministic.
 * mdg_hgt_sum_relations: out [n_rows,128] = act(sum of the n_rel slabs of part [n_rel, n_rows, 128], in order), act = GELU
 * (erf, the dense blocks' MDG_ACT_GELU) or none: the per-relation products of the value block summed. */
size_t mdg_hgt_attention_feat_workspace_bytes(int64_t n_items);
int mdg_hgt_attention_feat(const float* x, int64_t ldx, int64_t n_rows, const float* ut, const int32_t* src, int64_t nnz,
                           const int64_t* item_dst, const int32_t* item_rel, const int64_t* item_begin, const int64_t* item_end,
                           int64_t n_items, const int64_t* rel_ptr, float* st, int64_t n_dst, int n_rel, int heads,
                           void* workspace, size_t workspace_bytes, void* stream);
int mdg_hgt_sum_relations(const float* part, int64_t n_rows, int n_rel, int apply_gelu, float* out, void* stream);

/* ------------------------------------------------------------------------------ losses ---- */

/* InfoNCE finish of SimCLR_NovelDDI.contrastive_loss (madrigal/models/simclr.py:74-108): given
 * sim = F F^T [2B,2B] of the 2B L2-normalised features, apply the too-hard-negative mask ([B,B] bytes,
 * nullable; tiled 2x2, filled with -1e9), drop the diagonal, divide by the temperature -> logits
 * [2B,2B-1] (nullable), labels [2B,2B-1] (nullable, 1 at the other view of the same drug),
 * row_loss [2B] and loss [1] = mean soft-label cross entropy. */
int mdg_infonce_finish(const float* sim, const uint8_t* too_hard_neg, float* logits, float* labels, float* row_loss, float* loss,
                       int64_t B, float temperature, void* stream);
/* Backward of mdg_infonce_finish: dsim [2B,2B] = d loss / d sim (zero diagonal, zero at too-hard negatives), scaled by
 * dloss[0] (device scalar).  The caller chains it through sim = F F^T: dF = (dsim + dsim^T) F. */
int mdg_infonce_bwd(const float* sim, const uint8_t* too_hard_neg, const float* dloss, float* dsim, int64_t B, float temperature,
                    void* stream);

/* pred[e] = f(scores[label[e], head[e], tail[e]]) with f = sigmoid (apply_sigmoid) or identity, and the
 * mean BCE of pred against target with nn.BCELoss's -100 clamp: term [n] and loss [1] (both nullable
 * together).  Replaces the advanced-index gather + BCELoss of train_ddi_batch.py:285-288. */
int mdg_gather_bce(const float* scores, int64_t n_labels, int64_t n_head, int64_t n_tail, const int64_t* label, const int64_t* head,
                   const int64_t* tail, const float* target, float* pred, float* term, float* loss, int64_t n, int apply_sigmoid,
                   void* stream);

/* ------------------------------------------------------------------------- tuning switches ---- *
 * Environment variables read by the library (csrc: once, re-read after mdg_tuning_reload()) or by the Python host layer.  Each
 * changes speed or selects between paths that produce the same results within the tests' bounds; none is needed for normal use.
 * Round 5 removed every switch whose experiment was decided (35 of them: store schedules, wave counts, stream-K, the LSD
 * look-back, ...).  What is left, with defaults:
 *   MDG_RANKS_MSD        [1]  0: rank normalisation by the four-pass LSD sort only (what N > 5793 and flagged outcomes take)
 *   MDG_RANKS_GROUP      [8]  outcomes per launch group of the MSD path (its scratch is reused from group to group)
 *   MDG_RANKS_DIRECT     [0]  test hook: the LSD sort's last pass stores ranks one by one (what N > 16256 takes) at any N
 *   MDG_GROUP_WALK       [0 = by size]  test hook of mdg_group_metrics: 1 every group by the one-thread walk, any other
 *                        non-zero value every group by the 256-thread walk (no one-wave walk is built)
 *   MDG_BILINEAR_SYMMETRIC [1] 0: z_head == z_tail takes the general sweep instead of the symmetric one
 *   MDG_LINEAR_TILE      [0 = by shape]  128 / 256: force the dense block's tile shape
 *   MDG_LINEAR_RAWX      [1]  0: the 128-tile kernel's x through an operand pre-pass instead of rounded while staged
 *   MDG_LINEAR_TAIL128   [1]  0: no row split of a dense block's last partial round of 256-tiles
 *   MDG_KG_GRAPH         [per step kind]  0 / 1: the KG pass of a training step eager / replayed as hipGraphs
 *   MDG_SHARE_SIDES      [1]  0: dropout-free encoders run once per side of a step even when both sides are one batch
 *   MDG_FUSE_SIDES       [1]  0: the two sides of a finetune step through the fusion transformer in two passes
 *   MDG_FUSE_VIEWS       [1]  0: the two views of a contrastive step through the per-row stages in two passes
 *   MDG_SHARD_KG         [1]  0: multi-GPU inference keeps the KG encoder replicated instead of destination-partitioned
 * Build / bench only: MDG_EXTRA_HIPCC_FLAGS (madrigal_amd/build.py, e.g. -DMDG_RANK_STAMPS), MDG_BENCH_* (bench.py). */

/* ---------------------------------------------------------------------- evaluation metrics ---- */

/* Per-outcome classification metrics of T labelled triples, every label in one call.  Replaces
 * madrigal/evaluate/metrics.py:60-191 (get_metrics -> get_metrics_binary per label: sklearn confusion_matrix,
 * precision_recall_curve, roc_auc_score, average_precision_score, matthews_corrcoef, and precision_recall_at_k) after
 * madrigal/evaluate/evaluate.py:191 copied the dense [L,N,N] probabilities to the host.
 *   pred fp32 [T] (finite), target fp32 [T] (0 or 1), label int64 [T] in [0, n_labels);
 *   top-k size: k > 0, or k = 0 and 0 < k_frac < 1 for k = int(k_frac * n_label) per label (0 there sets the status bit 8);
 *   predicted positive <=> pred > threshold (0.5: np.round's rule for preds in [0, 1]).
 * values float64 [13, n_labels] in the reference's key order: fmax, mcc, auroc, auprc, npv, specificity, f1, recall@k,
 * precision@k, ap@k, accuracy, precision, recall (NaN rows for absent labels); count, pos, k_eff int64 [n_labels] (triples,
 * positives and the resolved k per label); status int32 [1]: OR of 1 (NaN / inf pred), 2 (label out of range),
 * 4 (target not 0/1), 8 (k resolved to 0).  Top-k ties: descending score, ties in reverse original order.
 * Needs 0 < T < 2^31, 0 < n_labels <= 65536.  Deterministic: the same inputs give bit-identical values. */
size_t mdg_label_metrics_workspace_bytes(int64_t n_triples, int64_t n_labels);
int mdg_label_metrics(const float* pred, const float* target, const int64_t* label, int64_t n_triples, int64_t n_labels,
                      int64_t k, double k_frac, float threshold, double* values, int64_t* count, int64_t* pos, int64_t* k_eff,
                      int* status, void* workspace, size_t workspace_bytes, void* stream);

/* The same 13 metrics per GROUP, for arbitrary group ids: the drug-stratified evaluation of
 * madrigal/evaluate/predict.py:274-355 (get_drug_specific_scores: get_metrics per drug, one problem per (drug, label)).
 *   pred, target, k, k_frac, threshold as above; group int64 [T] in [0, n_groups), 0 < T < 2^31, 0 < n_groups <= 2^31.
 * Keys: score image in bits 0-31, target in bit 32, group in bits 33-63; the stable LSD sort takes 4 score passes and
 * ceil(bits(n_groups - 1) / 8) group passes (ties inside a group in input order: the top-k tie rule above).  Only the groups
 * present are reported, compact and ascending by group id; with cap = min(T, n_groups) the caller allocates group_id int64 [cap],
 * values float64 [13, cap] (column j = the j-th present group), count / pos / k_eff int64 [cap], n_present int64 [1]; only the
 * first *n_present columns are written.  The walk is picked per group: at most 32 triples by one thread walking serially (the
 * same formulas), larger groups by the 256-thread walk of mdg_label_metrics (MDG_GROUP_WALK forces one of them).
 * inner > 0: also outer_values float64 [13, ceil(n_groups / inner)] and outer_groups int64 [ceil(n_groups / inner)], the mean
 * of each metric over the present groups of outer o = group / inner: an f64 sum in ascending group order divided once (numpy's
 * mean(axis=0) over those rows, bit for bit), NaN and 0 for an outer without groups.  inner = 0: both may be null.
 * status as above with 16 (group out of range) in place of 2.  Deterministic; no atomics except the status word. */
size_t mdg_group_metrics_workspace_bytes(int64_t n_triples, int64_t n_groups);
int mdg_group_metrics(const float* pred, const float* target, const int64_t* group, int64_t n_triples, int64_t n_groups, int64_t k,
                      double k_frac, float threshold, int64_t inner, int64_t* group_id, double* values, int64_t* count, int64_t* pos,
                      int64_t* k_eff, int64_t* n_present, double* outer_values, int64_t* outer_groups, int* status, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------- pretraining retrieval metrics ---- */

/* Match counts of two views X, Y fp32 [n,128] (row-major, 16-byte aligned, 1 <= n <= 65536) of the same n drugs; the true
 * match of row i is column i.  Replaces the CPU torch sweeps of madrigal/evaluate/evaluate.py:406-450
 * (get_inst_dist_topk_accuracy: cosine matrix + torch.topk), madrigal/evaluate/eval_utils.py:159-174
 * (stacked_inst_dist_topk_accuracy on the [2n,2n-1] stacked similarities), :232-247 (foscttm, a Python loop over rows) and
 * :153-156 (alignment_loss).  With x^ = x/|x| and G = X Y^T (one fp32 Gram, exact fp32 MFMA products):
 *   cos_row[i]  = #{j != i : x^_i.y^_j > x^_i.y^_i}     cos_col[j] = #{i != j : x^_i.y^_j > x^_j.y^_j}
 *   same_x[i]   = #{b != i : x^_i.x^_b > x^_i.y^_i}     same_y[i]  = #{b != i : y^_i.y^_b > x^_i.y^_i}
 *   dist_row[i] = #{j : |x_i - y_j| < |x_i - y_i|}      dist_col[j] = #{i : |x_i - y_j| < |x_j - y_j|}   (raw embeddings)
 *   align[i]    = |x^_i - y^_i|^2 (fp32)
 * Ties with the true match do not count against it (strict comparisons: ties count as hits); the true match is excluded by
 * index.  All outputs int32 [n] except align.  status int32 [1]: OR of 1 (NaN / inf input or squared norm), 2 (zero-norm row).
 * Deterministic: integer counts, no atomics on them; bit-identical from run to run. */
size_t mdg_pair_match_counts_workspace_bytes(int64_t n);
int mdg_pair_match_counts(const float* x, const float* y, int64_t n, int64_t d, int* cos_row, int* cos_col, int* same_x, int* same_y,
                          int* dist_row, int* dist_col, float* align, int* status, void* workspace, size_t workspace_bytes,
                          void* stream);
/* uniform_loss (madrigal/evaluate/eval_utils.py:147-150, torch.pdist over all rows): out fp32 [1] =
 * log(mean_{i<j} exp(-t |x^_i - x^_j|^2)) over X fp32 [m,128] (2 <= m <= 65536), |x^_i - x^_j|^2 = 2 - 2 x^_i.x^_j.  fp32 sums per
 * 128 x 128 tile, fp64 across tiles in a fixed order: bit-identical from run to run.  status as above. */
size_t mdg_pair_uniformity_workspace_bytes(int64_t m);
int mdg_pair_uniformity(const float* x, int64_t m, int64_t d, float t, float* out, int* status, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---------------------------------------------------------------------- k-nearest neighbours ---- */

/* For every row i of Q fp32 [nq,128] the k best rows j of Lib fp32 [nl,128] (row-major, 16-byte aligned; 1 <= nq, nl < 2^31 - 128)
 * and their values: vals fp32 [nq,k], idx int32 [nq,k], ordered by (value best-first, then j ascending) -- a total order, so the
 * result is unique.  Replaces the dense matrix + topk of madrigal/evaluate/eval_utils.py:196-203 (knn_classifier: distance_matrix /
 * torch.mm, then similarity.topk) and madrigal/evaluate/evaluate.py:411-418 (the two torch.topk of get_inst_dist_topk_accuracy);
 * nothing of [nq,nl] is stored.  With g = q_i.l_j (the exact-fp32 MFMA chain of mdg_pair_match_counts, bit for bit):
 *   MDG_KNN_COSINE     (g * 1/|q_i|) * 1/|l_j|, larger is better (the value mdg_pair_match_counts compares)
 *   MDG_KNN_DOT        g, larger is better
 *   MDG_KNN_EUCLIDEAN  ranked on d2 = (|q_i|^2 - 2 g) + |l_j|^2 in fp32, smaller is better; vals = sqrt(max(d2, 0))
 * 1 <= k <= min(mdg_knn_max_k() = 32, candidates per row).  skip: NULL, or int32 [nq]: the library index query i must not return
 * (-1: none) -- "the query is itself a row of the library" without a mask; then k <= nl - 1.
 * segments: the library is cut into that many contiguous ranges of whole 128-column tiles (at most ceil(nl / 128) are used), the grid
 * is (row blocks of 128) x segments, and a merge by the full key forms the result; 1 writes it directly.  The result is the same
 * bits for every value.  mdg_knn_default_segments (host only, deterministic, assumes the MI355X's 256 CUs): 1 when the row blocks
 * alone give 2 workgroups per CU, otherwise enough segments to get there, never more than ceil(nl / 128).
 * q_stats fp32 [2,nq], lib_stats fp32 [2,nl]: written by the pre-pass (|x|^2, then 1/|x|).  status int32 [1]: OR of 1 (NaN / inf
 * entry or squared norm) and, for MDG_KNN_COSINE, 2 (zero-norm row); results are meaningless when it is not 0.
 * workspace: mdg_knn_topk_workspace_bytes (host only; 0 for one segment), 16-byte aligned.  No atomics except the status word.
 * metric | MDG_KNN_NO_LISTS (measurement): the same sweep with the list epilogue compiled out; vals fp32 [segments used, nq] receives
 * the row maxima of the values, idx may be NULL, no workspace. */
enum mdg_knn_metric { MDG_KNN_COSINE = 0, MDG_KNN_DOT = 1, MDG_KNN_EUCLIDEAN = 2, MDG_KNN_NO_LISTS = 256 };
int mdg_knn_max_k(void);
int mdg_knn_default_segments(int64_t nq, int64_t nl);
size_t mdg_knn_topk_workspace_bytes(int64_t nq, int64_t nl, int k, int segments);
int mdg_knn_topk(const float* q, const float* lib, int64_t nq, int64_t nl, int64_t d, int k, int metric, const int32_t* skip,
                 int segments, float* q_stats, float* lib_stats, float* vals, int32_t* idx, int* status, void* workspace,
                 size_t workspace_bytes, void* stream);
/* The vote of the kNN classifier (madrigal/evaluate/eval_utils.py:205-218: gather of the neighbours' labels, one-hot scatter,
 * exp(distances / T) weights, sum, sort) on the lists of mdg_knn_topk: w_j = exp(vals[i,j] / T) in fp32 for BOTH metrics (the
 * reference weights Euclidean neighbours by exp(+distance / T) too).  labels uint8 [nl, n_cols].
 *   num_classes == 2 (binary, n_cols >= 1 label columns): per query and column p1 = sum_j w_j labels[idx[i,j], c] for j ascending,
 *     p0 = sum_j w_j - p1; sums fp32 [nq, n_cols, 2] = (p0, p1), pred uint8 [nq, n_cols].
 *   3 <= num_classes <= 64 (n_cols == 1, labels < num_classes): per-class sums fp32 [nq, num_classes], pred uint8 [nq].
 * pred = the class with the largest sum, the lowest class on a tie. */
int mdg_knn_vote(const float* vals, const int32_t* idx, const uint8_t* labels, int64_t nq, int64_t nl, int k, int64_t n_cols,
                 int num_classes, float T, uint8_t* pred, float* sums, void* stream);

/* ---------------------------------------------------------------------- GeomCA ---- */

/* The epsilon-graph evaluation of madrigal/evaluate/GeomCA.py over [n,128] fp32 embeddings (row-major, 16-byte aligned, 1 <= n <
 * 2^31 - 128), decided in squared-distance space: d2(x, y) = max(fmaf(-2, g(x,y), n(x) + n(y)), 0) in fp32, g the exact-fp32 MFMA
 * chain of mdg_pair_match_counts and n(x) = g(x, x) formed by that chain.  d2 is the same bits seen from either row, and bitwise
 * equal rows are at d2 == 0 exactly.  No [n,n] matrix and no edge list is stored.  The thresholds are float32(delta * delta) and
 * float32(epsilon * epsilon), formed by the caller in double.  segments: column segments of a sweep; 0 = the default
 * (mdg_geomca_default_segments, host only, assumes 256 CUs); results are the same for every value (integer atomics only). */
int mdg_geomca_default_chunk(void);
int mdg_geomca_default_segments(int64_t nrow, int64_t ncol);
/* norms fp32 [n] = n(x) (the diagonal of 32-row Gram tiles).  status int32 [1]: 1 when an entry or a norm is NaN / inf; the results
 * of the calls below are meaningless then.  Every call below takes the norms of its inputs from here. */
int mdg_geomca_prep(const float* x, int64_t n, int64_t d, float* norms, int* status, void* stream);
/* GeomCA.py:333-352 (get_sparse_pnts: gudhi.subsampling.sparsify_point_set): walking the rows in input order, row i is kept iff no
 * KEPT row j < i has d2(i, j) < delta2 (strict): the lexicographically first delta-separated subset.  kept_idx int32 [n] receives
 * the kept input rows, ascending, in its first count[0] entries (count: device int32 [1]).  chunk: candidates resolved per step, a
 * multiple of 128 in 128..512; the result is the same for every chunk.  Launches O(n / chunk), no host read.
 * workspace: mdg_geomca_sparsify_workspace_bytes (host only): the compacted kept rows and norms, the chunk's flags and bit matrix. */
size_t mdg_geomca_sparsify_workspace_bytes(int64_t n, int chunk);
int mdg_geomca_sparsify(const float* x, int64_t n, int64_t d, const float* norms, float delta2, int chunk, int segments, int32_t* kept_idx,
                        int* count, void* workspace, size_t workspace_bytes, void* stream);
/* GeomCA.py:354-387 and :423-435 (RipsComplex 1-skeleton, networkx graph, connected_components, extract_subnetworks): vertices
 * v [n,128], the first n_r of them the R set; edge {i, j}, i != j, iff d2(i, j) <= eps2 (non-strict).  label int32 [n]: the smallest
 * vertex index of i's connected component; deg_same / deg_cross int32 [n]: i's neighbours in its own set / in the other set.
 * Hooking + pointer jumping between sweeps; sweeps_host (HOST int [1]) receives the number of sweeps (the last one finds nothing to
 * change).  Reads one flag per sweep (synchronises the stream).  workspace: mdg_geomca_components_workspace_bytes (host only). */
size_t mdg_geomca_components_workspace_bytes(int64_t n);
int mdg_geomca_components(const float* v, int64_t n, int64_t n_r, int64_t d, const float* norms, float eps2, int segments, int32_t* label,
                          int32_t* deg_same, int32_t* deg_cross, int* sweeps_host, void* workspace, size_t workspace_bytes, void* stream);
/* GeomCA.py:250-282 (estimate_distance: cdist of two drawn row sets, distances > 0, np.percentile): x [mx,128], y [my,128] are the
 * gathered rows and ids_x / ids_y int32 the input rows they were drawn from.  Over the pairs with ids_x[a] != ids_y[b]:
 * counts_host (HOST int64 [2]) = {pairs at d2 == 0, M = pairs at d2 > 0}; values_host (HOST double [3]) = {D[k], D[k + 1], pos}, the
 * exact order statistics of the positive d2 values at pos = percentile / 100 * (M - 1), k = floor(pos), k + 1 clamped to M - 1
 * (zeros when M == 0).  A radix select on the fp32 bit pattern, 11 + 11 + 10 bits: three sweeps, one histogram read each
 * (synchronises the stream).  workspace: mdg_geomca_distance_select_workspace_bytes (host only). */
size_t mdg_geomca_distance_select_workspace_bytes(void);
int mdg_geomca_distance_select(const float* x, const float* y, const int32_t* ids_x, const int32_t* ids_y, int64_t mx, int64_t my, int64_t d,
                               const float* x_norms, const float* y_norms, double percentile, int segments, int64_t* counts_host,
                               double* values_host, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------- rank normalisation ---- */

size_t mdg_rank_normalize_workspace_bytes(int64_t n_outcomes, int64_t N);
/* 1 when a call of this size takes the exact-layout MSD path first (the default up to N = 5793, MDG_RANKS_MSD=0 turns it off: one
 * partition + an in-LDS sort per bucket; ranks.hip), 0 when it runs the four-pass LSD sort only.  On the MSD path the first
 * n_outcomes uint32 words of the workspace hold, after the call, one flag per outcome: non-zero = that outcome was handed to the LSD
 * kernels (point masses of equal scores: a bucket of 65 536 keys or more, or more than 1 024 keys in one fine bin).  Diagnostics:
 * the ranks are the same bits. */
int mdg_rank_normalize_fast_path(int64_t n_outcomes, int64_t N);

/* Per outcome l: out[l,i,j] = out[l,j,i] = rank(scores[l,i,j] among the strict lower triangle i > j, ascending,
 * 1-based, ties by flat index) / (N(N-1)/2), diagonal 0; the division is done in double and rounded to fp32
 * like numpy's int64 / float -> float32 store.  Replaces classwise_normalized_rank_3d_numpy + run_slice,
 * notebooks/normalize_scores.py:36-74 (two CPU argsorts of N^2 keys per outcome).  scores, out [n_outcomes,N,N];
 * out may alias scores only if n_outcomes fits one call.  Scores must be finite and < 1e7 (the reference's
 * mask value). */
int mdg_rank_normalize(const float* scores, float* out, int64_t n_outcomes, int64_t N, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The same on row-pitched tensors (mdg_bilinear_allpairs_ld): scores[(l * N + i) * lds + j], out[(l * N + i) * ldo + j]. */
int mdg_rank_normalize_ld(const float* scores, int64_t lds, float* out, int64_t ldo, int64_t n_outcomes, int64_t N, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The same from the order keys of the strict lower triangle as mdg_bilinear_allpairs_ld(..., MDG_EPI_TRIKEYS) writes them
 * (keys[(l * N + i) * ldk + j] for j < i; nothing else of `keys` is read): the head's store stream is halved and the
 * ranks equal those of the materialised scores bit for bit.  out may be the memory of keys (n_outcomes of one call). */
int mdg_rank_normalize_keys_ld(const uint32_t* keys, int64_t ldk, float* out, int64_t ldo, int64_t n_outcomes, int64_t N,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Elementwise geometric mean of K <= 8 equally shaped fp32 tensors (the 5-seed ensembling of normalised ranks,
 * scipy.stats.mstats.gmean in notebooks/generate_embeddings.ipynb): out = exp(mean_k log x_k) in fp32; 0 where any
 * x_k <= 0.  inputs_host is a HOST array of K device pointers (16-byte aligned); n = elements of each tensor. */
int mdg_gmean(const float* const* inputs_host, int K, float* out, int64_t n, void* stream);

/* Parameter space of the HGT conv in training (PyG 2.3 HGTConv, madrigal/models/models.py:76-79,90-94): the composite projection
 * weights of every projected node type from the live parameters -- rows [Wq_t | K_r V_r for every used relation r leaving t] with
 * K_r = blockdiag_h(k_rel[h,r]^T p_rel[r][h] / sqrt(D)) Wk_t, V_r = blockdiag_h(v_rel[h,r]^T) Wv_t (biases likewise) -- and the
 * gradients of kqv_lin / k_rel / v_rel / p_rel from the gradient of those rows.  w_ptrs / b_ptrs: DEVICE arrays of n_types float
 * pointers (kqv weight [3F,cin], rows K | Q | V; bias [3F]); p_ptrs: device array of n_edge_types pointers ([heads] each); rel_*:
 * per used relation its edge type, its source type (index into w_ptrs) and the first row of its K block in big_w (V block: + F);
 * type_row: first row of each type's block.  bwd writes grads = [per type: dW (3F x cin) | db (3F)] | dk_rel | dv_rel | dp_rel
 * [n_edge_types, heads] (zero for unused relations).  Exact fp32, fixed summation order. */
int mdg_hgt_composite_fwd(const void* w_ptrs, const void* b_ptrs, const float* k_rel, const float* v_rel, const void* p_ptrs, const int* rel_r,
                          const int* rel_src, const int* rel_row, int n_rel, const int* type_row, int n_types, float* big_w, float* big_b,
                          int cin, int heads, int n_edge_types, int F, void* stream);
int mdg_hgt_composite_bwd(const void* w_ptrs, const void* b_ptrs, const float* k_rel, const float* v_rel, const void* p_ptrs, const int* rel_r,
                          const int* rel_src, const int* rel_row, int n_rel, const int* type_row, int n_types, const float* dbig_w,
                          const float* dbig_b, float* grads, int cin, int heads, int n_edge_types, int F, void* stream);

/* mdg_hgt_attention that also returns the softmax statistics stats [n_dst, heads, 2] = (max logit, denominator) the
 * backward pass needs; and that backward pass.  dout is the gradient at the attention output BEFORE the activation
 * (call the forward with apply_gelu = 0 and differentiate the activation separately), out_pre that forward output.
 * Reversed edge lists (built by the caller from col / the destination of each edge): the nnz edges stably sorted by
 * key row; t_edge[e'] = forward edge id, t_dst[e'] = its destination; the n_src_rows distinct key rows t_row are cut
 * into work items (t_item_begin/end, t_item_ptr [n_src_rows+1]; t_item_row [n_src_items] = index into t_row of each
 * item's key row, or null: with it a key row of ONE item is written by the gather kernel itself, not through a partial).
 * dq [n_dst,128]; dkv has the layout of kv (lddkv = 128: value rows follow key rows) and only the rows of this call's
 * key rows are written — zero-fill it first.  kv16: optional bf16 mirror of kv (mdg_f32_to_bf16; ldkv must be 128). */
int mdg_hgt_attention_stats(const float* q, int64_t ldq, const float* kv, int64_t ldkv, const int64_t* col,
                            const int64_t* item_dst, const int64_t* item_begin, const int64_t* item_end, int64_t n_items,
                            const int64_t* item_ptr, float* out, int64_t ldo, int64_t n_dst, int heads, int64_t F,
                            int apply_gelu, float* stats, const void* kv16, void* workspace, size_t workspace_bytes, void* stream);
size_t mdg_hgt_attention_bwd_workspace_bytes(int64_t nnz, int64_t n_items, int64_t n_src_items, int heads);
int mdg_hgt_attention_bwd(const float* q, int64_t ldq, const float* kv, int64_t ldkv, const int64_t* col, int64_t nnz,
                          const int64_t* item_dst, const int64_t* item_begin, const int64_t* item_end, int64_t n_items,
                          const int64_t* item_ptr, int64_t n_dst, const float* dout, int64_t lddo, const float* out_pre,
                          int64_t ldp, const float* stats, int heads, const int64_t* t_edge, const int64_t* t_dst,
                          const int64_t* t_item_begin, const int64_t* t_item_end, int64_t n_src_items,
                          const int64_t* t_item_ptr, const int64_t* t_row, int64_t n_src_rows, const int64_t* t_item_row,
                          float* dq, int64_t lddq, float* dkv, int64_t lddkv, const void* kv16, void* workspace, size_t workspace_bytes,
                          void* stream);
/* fp32 -> bf16 (round to nearest even), n a multiple of 8: the 16-bit mirror of the projection buffer the two entry points above
 * gather their k' | v' rows from when kv16 is non-null (the step's reduced-precision "bf16" mode: half the bytes per edge; q, the
 * softmax statistics, every sum and every gradient stay fp32).  kv16 null = rows read from kv itself. */
int mdg_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);

/* ------------------------------------------------------- gathered head (finetune step) ---- */
/* ---- index plumbing of the gathered head's plan (madrigal_amd.ops.triple_plan; the reference feeds a new batch of labelled
 * triples to every step, train_ddi_batch.py:231-354, so the plan is rebuilt per step).  All index arrays are int64 on the device.
 *
 * mdg_plan_gather: for the label-sorted order perm: hs[i] = heads[perm[i]], ts[i] = tails[perm[i]], skey[i] = labels[perm[i]] * n_head
 *   + hs[i], inv_perm[perm[i]] = i; *status |= 1 (a label outside [0, n_labels)) | 2 (a head / tail outside its table).
 * mdg_plan_lower_bounds: out[b] = first i with vals[i] >= b * scale, b = 0 .. n_bounds - 1 (vals ascending, val_bytes = 2 / 4 / 8:
 *   int16 / int32 / int64): CSR pointers of a sorted index list.
 * mdg_plan_cut_count / _fill: the lists of a CSR pointer ptr[n + 1] cut into pieces of <= size entries: first[i] = pieces of the lists
 *   before i (first[n] = totals[0] = all pieces), totals[1] = the longest list; which[j] = the list of piece j (which may be NULL),
 *   start[j] = its first entry, start[total] = ptr[n].  (tiles of 32 and chunks of 256 / 512 triples or pairs of one label, pieces of 64 rows of one drug)
 * mdg_plan_pair_flags: flag[i] = 1 where skey[i] != skey[i - 1] (flag[0] = 0): its inclusive prefix sum is the (label, head) pair of
 *   every sorted triple.  mdg_plan_pair_table: pair_ptr[p] = first triple of pair p (pair_ptr[P] = T), pair_drug[p] = its head drug.
 * mdg_plan_take: out[i] = src[idx[i]] where 0 <= idx[i] < T, else fill. */
int mdg_plan_gather(const int64_t* perm, const int64_t* labels, const int64_t* heads, const int64_t* tails, int64_t T, int64_t n_labels,
                    int64_t n_head, int64_t n_tail, int64_t* hs, int64_t* ts, int64_t* skey, int64_t* inv_perm, int32_t* status, void* stream);
int mdg_plan_lower_bounds(const void* vals, int val_bytes, int64_t T, int64_t scale, int64_t n_bounds, int64_t* out, void* stream);
int mdg_plan_cut_count(const int64_t* ptr, int64_t n, int64_t size, int64_t* first, int64_t* totals, void* stream);
int mdg_plan_cut_fill(const int64_t* ptr, const int64_t* first, int64_t n, int64_t size, int64_t total, int64_t* which, int64_t* start,
                      void* stream);
int mdg_plan_pair_flags(const int64_t* skey, int64_t T, int64_t* flag, void* stream);
int mdg_plan_pair_table(const int64_t* skey, const int64_t* pair_of, int64_t T, int64_t n_head, int64_t P, int64_t* pair_ptr,
                        int64_t* pair_drug, void* stream);
int mdg_plan_take(const int64_t* src, const int64_t* idx, int64_t n, int64_t T, int64_t fill, int64_t* out, void* stream);

/* train_ddi_batch.py:285-288 computes sigmoid(model(...)) [L,N,N] and reads T (label, head, tail) entries of it.  These
 * entry points compute only those entries: score[t] = z_head[head[t]]^T w[label] z_tail[tail[t]].
 * The triples are sorted by label by the caller and cut into tiles of <= 32 triples of ONE label: tile_start [n_tiles+1]
 * (triple offsets), tile_label [n_tiles]; head / tail / score / dscore are in that sorted order.  D must be 128. */
int mdg_bilinear_gather(const float* z_head, const float* z_tail, const float* w, const int64_t* head, const int64_t* tail,
                        const int64_t* tile_start, const int64_t* tile_label, int64_t n_tiles, float* score, int64_t D,
                        void* stream);
/* Backward: gz_head_rows / gz_tail_rows [T,128] receive one gradient row per triple (dscore[t] * w z_tail, dscore[t] *
 * w^T z_head; the caller sums them per drug with mdg_csr_aggregate — no atomics); w_t is w transposed per label (pass
 * w itself when it is symmetric).  dw [n_labels,128,128] (optional) is accumulated through dw_partial
 * [n_chunks,128,128]: chunk_start [n_chunks+1] cuts the sorted triples into chunks of <= 256 triples of one label and
 * label_chunk_ptr [n_labels+1] lists each label's chunks. */
int mdg_bilinear_gather_bwd(const float* z_head, const float* z_tail, const float* w, const float* w_t, const int64_t* head,
                            const int64_t* tail, const int64_t* tile_start, const int64_t* tile_label, int64_t n_tiles,
                            const int64_t* chunk_start, int64_t n_chunks, const int64_t* label_chunk_ptr, int64_t n_labels,
                            const float* dscore, float* gz_head_rows, float* gz_tail_rows, float* dw_partial, float* dw, int64_t D,
                            void* stream);
/* The same with the arithmetic mode of the step: in the 16-bit modes dW runs on the split-bf16 matrix cores (three products of the
 * hi / lo halves of ds * z_head and z_tail, fp32 accumulation: fp32-grade, ~4e-6 of max) as a TN product over the gathered rows;
 * MDG_PREC_F32 = the exact fp32 MFMA kernel of mdg_bilinear_gather_bwd.  The per-triple gradient rows are exact fp32 either way. */
int mdg_bilinear_gather_bwd_prec(const float* z_head, const float* z_tail, const float* w, const float* w_t, const int64_t* head,
                                 const int64_t* tail, const int64_t* tile_start, const int64_t* tile_label, int64_t n_tiles,
                                 const int64_t* chunk_start, int64_t n_chunks, const int64_t* label_chunk_ptr, int64_t n_labels,
                                 const float* dscore, float* gz_head_rows, float* gz_tail_rows, float* dw_partial, float* dw,
                                 int64_t D, int precision, void* stream);
/* Pair-compressed gathered head (same sums as mdg_bilinear_gather / _bwd, grouped per (label, drug) PAIR before the 128 x 128
 * products: the finetune batch holds more labelled triples than (outcome, drug) pairs, train_ddi_batch.py:285-288).
 *   mdg_bilinear_matvec_rows: rows_out[p] = W[tile_label] z[row_index[p]] for pairs cut into tiles of <= 32 pairs of one label
 *       (row_index NULL = identity); exact-fp32 matrix cores.
 *   mdg_gather_rowdot: out[t] = a[ia[t]] . b[ib[t]] over rows of 128 floats (the per-triple score from the per-pair rows).
 * mdg_bilinear_gather_bwd with n_tiles = 0 runs only its dW part; there `tail` NULL means row t of z_tail and `dscore` NULL
 * means weight 1 (the dW sum over pairs). */
int mdg_bilinear_matvec_rows(const float* z, const float* w, const int64_t* row_index, const int64_t* tile_start, const int64_t* tile_label,
                             int64_t n_tiles, float* rows_out, int64_t D, void* stream);
/* The per-pair products in the step's arithmetic mode: MDG_PREC_F32 = the call above; the 16-bit modes run them on the split-bf16
 * matrix cores (z rows split in registers, W from hi / lo bf16 images made inside the call in `workspace`: three products, fp32
 * accumulation -- fp32-grade, ~4e-6 of max).  w [n_labels,128,128]. */
size_t mdg_bilinear_matvec_rows_workspace_bytes(int64_t n_labels, int precision);
int mdg_bilinear_matvec_rows_prec(const float* z, const float* w, int64_t n_labels, const int64_t* row_index, const int64_t* tile_start,
                                  const int64_t* tile_label, int64_t n_tiles, float* rows_out, int64_t D, int precision, void* workspace,
                                  size_t workspace_bytes, void* stream);
int mdg_gather_rowdot(const float* a, const int64_t* ia, const float* b, const int64_t* ib, float* out, int64_t n, int64_t D, void* stream);

/* nn.BCELoss(sigmoid(score), target) per element (log clamp at -100) and/or its gradient w.r.t. the logit times
 * grad_scale (1/T for reduction='mean').  madrigal/utils.py:616-619. */
int mdg_bce_logits(const float* score, const float* target, float* term, float* dscore, int64_t n, float grad_scale, void* stream);
/* Backward of mdg_symmetrize: dw_original = triu(dw_sym) + triu(dw_sym^T, 1). */
int mdg_symmetrize_bwd(const float* dw_sym, float* dw_original, int64_t n_labels, int64_t D, void* stream);

/* ------------------------------------------------------- optimizer ---- */
/* torch.optim.AdamW semantics (madrigal/utils.py:600-613) for every parameter tensor in one launch.  The tensors are cut
 * into chunks of mdg_adamw_chunk_elems() elements: chunk_ptrs [n_chunks,4] = device addresses of the chunk inside
 * (param, grad, exp_avg, exp_avg_sq), chunk_lens [n_chunks], chunk_tensor [n_chunks] = row of hyper [n_tensors,8] =
 * {lr, beta1, beta2, eps, weight_decay, 1/(1-beta1^t), 1/sqrt(1-beta2^t), 0}.  All tables live in device memory. */
int mdg_adamw_chunk_elems(void);
int mdg_adamw_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                    int64_t n_chunks, void* stream);
/* torch.optim.RAdam semantics (madrigal/utils.py:602 OPTIMIZER_CLASSES, `--optimizer radam`) over the same tables, one launch.
 * hyper [n_tensors,8] = {lr, beta1, beta2, eps, weight_decay, 1/(1-beta1^t), rect_t * sqrt(1-beta2^t), decoupled}: the host works
 * out rho_t = rho_inf - 2 t beta2^t / (1-beta2^t) per tensor and passes 0 in slot 6 while rho_t <= 5, where the update is the
 * unrectified p -= lr * m_hat.  Weight decay is L2 (g += wd * p, torch's default and so the reference's) unless `decoupled` != 0. */
int mdg_radam_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                    int64_t n_chunks, void* stream);
/* The reference's LARS (madrigal/utils.py:628-662; selected by pretrain.py:175-176, `--pretrain_optimizer lars`) for every parameter
 * tensor in three launches, whatever the number of tensors.  chunk_ptrs [n_chunks,3] = (param, grad, mu) addresses of chunks of
 * mdg_adamw_chunk_elems() elements, a tensor's chunks consecutive: first_chunk / tensor_chunks [n_tensors].  hyper [n_tensors,5] =
 * {lr, weight_decay, momentum, trust_coefficient, scaled}, scaled = 1 for tensors with more than one dimension:
 *     scaled:   u = g + weight_decay * p;  q = trust_coefficient * |p| / |u| if both norms are > 0 else 1;  u = q * u
 *     unscaled: u = g
 *     mu = momentum * mu + u;  p = p - lr * mu
 * The norms are fixed-order sums (per-chunk fp32 partials, per-tensor sum in double; no atomics): results are reproducible bit for
 * bit and do not depend on the 16-byte alignment of the tensors, which only selects the width of the accesses.  `workspace` is
 * device memory, 16-byte aligned, of mdg_lars_multi_workspace_bytes; nothing is read back to the host. */
size_t mdg_lars_multi_workspace_bytes(int64_t n_chunks, int64_t n_tensors);
int mdg_lars_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                   const int32_t* first_chunk, const int32_t* tensor_chunks, int64_t n_chunks, int64_t n_tensors, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------- backward-pass building blocks ---- */
/* (the finetune step of train_ddi_batch.py:285-354: loss.backward() through the modules above) */

/* Weight (and bias) gradient of y = x W^T + b:  dw[n,k] = sum_m g[m,n] x[m,k],  dbias[n] = sum_m g[m,n] (optional, NULL to
 * skip)  (g [M,N] = dL/dy, x [M,K] the layer input, both row-major with unit inner stride).  The reduction over the M rows
 * is split across the grid (exact fp32 MFMA, partials summed in a fixed order); workspace from
 * mdg_grad_weight_workspace_bytes. */
size_t mdg_grad_weight_workspace_bytes(int64_t M, int64_t N, int64_t K);
int mdg_grad_weight(const float* g, int64_t ldg, const float* x, int64_t ldx, float* dw, float* dbias, int64_t M, int64_t N,
                    int64_t K, void* workspace, size_t workspace_bytes, void* stream);
/* The same in the arithmetic mode of the step's dense blocks.  MDG_PREC_F32: the exact kernel above.  MDG_PREC_BF16 / BF16X3 (N, K, ldg,
 * ldx multiples of 4, 16-byte aligned operands; anything else takes the exact kernel): g and x rounded to bf16 (bf16x3: split hi + lo,
 * three products) while they are staged, fp32 accumulation on v_mfma_f32_16x16x32_bf16 -- what mdg_linear_tn does for large outputs,
 * here for the small ones whose cost is reading g and x once.  dbias is summed from the fp32 g in every mode. */
int mdg_grad_weight_prec(const float* g, int64_t ldg, const float* x, int64_t ldx, float* dw, float* dbias, int64_t M, int64_t N,
                         int64_t K, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* Grouped dense block: G independent products y_g = alpha_g * act(x_g W_g^T + b_g) + beta_g * r_g sharing K, in ONE launch.
 * Replaces the per-node-type linear layers of PyG HGTConv (kqv_lin / out_lin, a HeteroDictLinear each: one GEMM per node
 * type; call site madrigal/models/models.py:76-79,90-94).  The x rows of all groups are stacked in one [rows_total, K] matrix,
 * the W rows (and biases) of all groups in one [w_rows_total, K] matrix (packed with mdg_pack_operand, or raw fp32 where the
 * mode needs no image); `tiles` is a DEVICE table of n_tiles descriptors of mdg_linear_group_tile_words() int64 words, one per
 * 128 x 128 output tile:
 *   0 a_row0  1 a_row_end  2 b_row0  3 b_row_end   tile origin / end of the group's rows in the stacked x and W
 *   4 m_base  5 n_base                             the group's first x row / first W row
 *   6 y_off   7 ldy                                output element (m, n) -> y[y_off + (m - m_base) * ldy + (n - n_base)]
 *   8 res_off (-1: none)  9 ldr                    residual element, same addressing relative to `residual`
 *   10 alpha (float bits) | beta (float bits) << 32          11 unused
 * Offsets and row strides must be multiples of 4 floats.  Workspace (the packed x): mdg_linear_grouped_workspace_bytes. */
int mdg_linear_group_tile_words(void);
size_t mdg_linear_grouped_workspace_bytes(int64_t rows_total, int64_t K, int precision);
int mdg_linear_grouped(const float* x, int64_t ldx, int64_t rows_total, int64_t K, const float* w, int64_t ldw, const void* w_packed,
                       int64_t w_rows_total, const float* bias, const int64_t* tiles, int64_t n_tiles, float* y,
                       const float* residual, int act, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* y[N,K] = g^T x for row-major g [M,N] (row stride ldg) and x [M,K]: the weight gradient dW = dY^T X of a wide layer
 * (autograd of nn.Linear).  Both operands are re-laid out (reduction index M innermost, padded to 64) by one transposing pack
 * launch, then the mdg_linear tile kernel runs: no separate transposes of g and x. */
size_t mdg_linear_tn_workspace_bytes(int64_t M, int64_t N, int64_t K, int precision);
int mdg_linear_tn(const float* g, int64_t ldg, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t M, int64_t N, int64_t K,
                  int precision, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of a wide dense block y = x W^T + b from ONE pass over g = dL/dy [M,N] (16-bit operand modes): the pass writes the operand
 * image of g (for dx = g W through mdg_linear_packed_x with K = N; NULL to skip), the image of g^T (for dW through
 * mdg_linear_tn_packed_g) and dbias = column sums of the fp32 g (NULL to skip).  The separate calls (mdg_linear on g, mdg_linear_tn,
 * mdg_colsum) read g three times.  mdg_linear_backward_pack_bytes(M, N, precision, which): 0 = bytes of the row image, 1 = of the
 * transposed image, 2 = of the workspace (partial column sums). */
size_t mdg_linear_backward_pack_bytes(int64_t M, int64_t N, int precision, int which);
int mdg_linear_backward_pack(const float* g, int64_t ldg, int64_t M, int64_t N, int precision, void* row_image, void* t_image,
                             float* dbias, float drop_p, uint64_t drop_seed, void* workspace, size_t workspace_bytes, void* stream);
/* (drop_p > 0: g is first passed through the backward of the dropout mdg_linear_dropout applied with the same p and seed --
 * element (m, n) kept iff the counter-based hash of (seed, m * N + n) says so, scaled by 1 / (1 - p) -- on load, no pass of its own.) */
size_t mdg_linear_tn_packed_g_workspace_bytes(int64_t M, int64_t N, int64_t K, int precision);
int mdg_linear_tn_packed_g(const void* gt_image, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t M, int64_t N, int64_t K,
                           int precision, void* workspace, size_t workspace_bytes, void* stream);

/* out[c, r] = in[r, c]   (dW = dY^T X and dX = dY W are mdg_linear calls on transposed operands) */
int mdg_transpose(const float* in, int64_t ldi, float* out, int64_t ldo, int64_t rows, int64_t cols, void* stream);

/* out[c] = beta * out[c] + sum_r x[r, c], fixed summation order (bias / LayerNorm / learned-token gradients). */
size_t mdg_colsum_workspace_bytes(int64_t rows, int64_t cols);
int mdg_colsum(const float* x, int64_t ldx, float* out, int64_t rows, int64_t cols, float beta, void* workspace,
               size_t workspace_bytes, void* stream);

/* y = act(pre) and dx = dy * act'(pre), elementwise over n contiguous floats (training keeps the pre-activation). */
int mdg_activation_fwd(const float* pre, float* y, int64_t n, int activation, void* stream);
int mdg_activation_bwd(const float* dy, const float* pre, float* dx, int64_t n, int activation, void* stream);
/* y = dropout(act(pre), p, seed) and its backward dx = act'(pre) * dropout-backward(dy) in one pass each (the FFN's
 * dropout(activation(linear1(x))) of nn.TransformerEncoderLayer in training mode); same mask as mdg_dropout(seed). */
int mdg_activation_dropout_fwd(const float* pre, float* y, int64_t n, int activation, float p, uint64_t seed, void* stream);
int mdg_activation_dropout_bwd(const float* dy, const float* pre, float* dx, int64_t n, int activation, float p, uint64_t seed, void* stream);

/* out[i] = alpha * a[i] + beta * b[i mod nb] (residual adds of the training path; nb < n broadcasts a row over rows). */
int mdg_axpby(const float* a, const float* b, float* out, int64_t n, int64_t nb, float alpha, float beta, void* stream);

/* out[i] = x[i] * scalar[0], scalar in device memory (scaling a stored gradient by the incoming scalar gradient). */
int mdg_mul_device_scalar(const float* x, const float* scalar, float* out, int64_t n, void* stream);

/* HGTConv skip gate (PyG 2.3.1 HGTConv.forward): out = s * o + (1 - s) * x with s = sigmoid(skip[0]) read from device
 * memory; backward: d_o, d_x and rowdot[v] = s (1-s) sum_c dout (o - x) whose sum over rows is d skip. */
int mdg_gated_residual(const float* o, const float* x, const float* skip, float* out, int64_t n, void* stream);
int mdg_gated_residual_bwd(const float* dout, const float* o, const float* x, const float* skip, float* d_o, float* d_x,
                           float* rowdot, int64_t rows, int64_t cols, void* stream);

/* Inverted dropout y = x * keep / (1-p); keep is a counter-based hash of (seed, element index), so calling it again
 * with the same seed on dy is the backward pass (nn.Dropout of the transformer / MLPs / position encoder). */
int mdg_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);

/* nn.BatchNorm1d in training mode over the rows of x [rows, cols] (torchdrug MultiLayerPerceptron batch_norm,
 * chemCPA MLP), fused with the following activation: y = act((x - mean) * rstd * gamma + beta); running statistics are
 * updated in place (momentum, unbiased variance).  stats [5*cols] receives mean | rstd | scale | shift for the backward, and the biased batch variance. */
size_t mdg_batchnorm_workspace_bytes(int64_t rows, int64_t cols);
int mdg_batchnorm_train_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, float* y, int64_t ldy, float* stats, int64_t rows, int64_t cols, float eps,
                            float momentum, int activation, void* workspace, size_t workspace_bytes, void* stream);
/* dy is the gradient at the BN output (before the activation); x, dy, dx contiguous [rows, cols]. */
int mdg_batchnorm_train_bwd(const float* dy, const float* x, const float* stats, float* dx, float* dgamma, float* dbeta,
                            int64_t rows, int64_t cols, void* workspace, size_t workspace_bytes, void* stream);

/* One more momentum update of running_mean / running_var with the batch statistics of an earlier mdg_batchnorm_train_fwd
 * (stats[0:C] mean, stats[4C:5C] biased variance): nn.BatchNorm1d seeing the same rows again.  The reference encodes head side and tail
 * side of one step separately (madrigal/models/models.py:945-946); when both sides are the same batch, the encoders without
 * dropout (GIN, chemCPA) produce the same output twice -- here they run once and their BatchNorm layers replay the update. */
int mdg_batchnorm_replay_update(const float* stats, float* running_mean, float* running_var, int64_t rows, int64_t cols, float eps,
                                float momentum, void* stream);

/* The phases of mdg_batchnorm_train_fwd / _bwd as separate calls, for SyncBatchNorm over drug-sharded ranks: the caller
 * all-reduces the per-column sums between phases (count = rows over all ranks).
 *   mdg_col_reduce mode 0: out[c] = sum_r x;  1: sum_r (x - center[c])^2;  2: sum_r x * (y - center[c]) * rstd[c]
 *   mdg_batchnorm_finalize phase 0: stats[0:C] = sum / count;  phase 1: rstd | scale | shift | variance (stats has 5C entries) from sqsum / count and the
 *   running-statistics update;  then mdg_affine_act(x, stats + 2C, stats + 3C) applies the normalisation.
 *   mdg_batchnorm_bwd_apply: dx from the (all-reduced) sum_dy and sum_dy_xhat.
 * count_dev (optional): the total row count as a device double (itself all-reduced) read by the kernel instead of the
 * host value — no host round trip inside the step. */
int mdg_col_reduce(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* center, const float* rstd, float* out,
                   int64_t rows, int64_t cols, int mode, void* workspace, size_t workspace_bytes, void* stream);
int mdg_batchnorm_finalize(const float* sum, const float* sqsum, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float* stats, double count, const double* count_dev, int64_t cols, float eps,
                           float momentum, int phase, void* stream);
int mdg_batchnorm_bwd_apply(const float* dy, const float* x, const float* stats, const float* sum_dy, const float* sum_dy_xhat,
                            float* dx, int64_t rows, int64_t cols, double count, const double* count_dev, void* stream);

/* y = act(x * scale[c] + shift[c]) per column (eval-mode BatchNorm inside a differentiated graph; shift may be NULL). */
int mdg_affine_act(const float* x, int64_t ldx, const float* scale, const float* shift, float* y, int64_t ldy, int64_t rows,
                   int64_t cols, int activation, void* stream);

/* Training-mode variants of the fusion kernels (nn.MultiheadAttention(dropout=p) drops attention WEIGHTS,
 * models.py:363-379): same arguments as mdg_fusion_attention / mdg_xattn_pool plus the dropout probability and the
 * seed of the counter-based mask; the backward entry points regenerate the mask from the same seed and recompute
 * the attention weights from qkv (nothing else is kept from the forward pass).
 * mdg_fusion_attention_bwd: dqkv [rows, 3d] receives dQ | dK | dV for every row of every tile.
 * mdg_xattn_pool_bwd: dkv [n*Tk, 2d] receives dK | dV; dq_part [n, d] the per-drug gradient of the projected query
 * (the caller sums it over drugs with mdg_colsum). */
int mdg_fusion_attention_dropout(const float* qkv, int64_t ld, float* out, int64_t ldo, const uint32_t* kpm_bits,
                                 const uint32_t* src_bits, float* probs, const int64_t* row_start, const uint32_t* row_bits,
                                 int64_t n, int S, int H, int dh, float p_drop, uint64_t seed, void* stream);
int mdg_fusion_attention_bwd(const float* qkv, int64_t ld, const float* dout, int64_t lddo, float* dqkv, int64_t lddq,
                             const uint32_t* kpm_bits, const uint32_t* src_bits, const int64_t* row_start,
                             const uint32_t* row_bits, int64_t n, int S, int H, int dh, float p_drop, uint64_t seed, void* stream);
int mdg_xattn_pool_dropout(const float* q_proj, const float* kv_proj, int64_t ld, float* out, int64_t ldo, int64_t n, int Tk,
                           int H, int dh, float p_drop, uint64_t seed, void* stream);
int mdg_xattn_pool_bwd(const float* q_proj, const float* kv_proj, int64_t ld, const float* dout, int64_t lddo, float* dkv,
                       int64_t lddkv, float* dq_part, int64_t n, int Tk, int H, int dh, float p_drop, uint64_t seed, void* stream);

/* Backward of mdg_assemble_tokens (rows == NULL): dstr/dkg/dcv [n,128] and dtx [16*n,128] must be zero-filled (tokens
 * that were not emitted leave no gradient); dlearned / dpe are zero-filled [n, S, 128] scratch receiving the per-drug
 * gradients of the cls / bottleneck tokens and of the position table (sum over drugs with mdg_colsum). */
int mdg_assemble_tokens_bwd(const float* dseq, const float* str_emb, const float* kg_emb, const float* cv_emb, const float* tx_emb,
                            const float* bottleneck, const float* cls, const int64_t* token_index, int64_t n_tok, float* dstr,
                            float* dkg, float* dcv, float* dtx, float* dlearned, float* dpe, int64_t n, int nb, int has_cls,
                            int pe_len, int normalize, int64_t D, void* stream);

/* dx of y = x / max(|x|_2, 1e-12) (F.normalize). */
int mdg_l2_normalize_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dx, int64_t lddx, int64_t rows,
                         int64_t d, void* stream);

/* LayerNorm backward (statistics recomputed from x): dx, dgamma, dbeta.  d <= 2048. */
size_t mdg_layernorm_bwd_workspace_bytes(int64_t rows, int64_t d);
int mdg_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, float* dx, int64_t lddx,
                      float* dgamma, float* dbeta, int64_t rows, int64_t d, float eps, void* workspace, size_t workspace_bytes,
                      void* stream);
/* dx = LayerNorm-backward(dy) + extra: x feeds the norm AND a residual connection (pre-norm transformer blocks), `extra` is the
 * gradient that arrives through the residual; added while dx is written instead of by a pass of its own. */
int mdg_layernorm_bwd_add(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, const float* extra,
                          int64_t ldextra, float* dx, int64_t lddx, float* dgamma, float* dbeta, int64_t rows, int64_t d, float eps,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- on-device batch collation from a device-resident drug store (madrigal_amd/collate.py) ----------------------------
 * The reference collates every batch on the host (madrigal/data/data.py:1479-1501: all_molecules[ids],
 * tabular_mod_stores[mod][ids], 16 x tx_store[...][ids]).  The store keeps every drug's modalities on the device: molecules
 * packed (atom_ptr / edge_ptr [n_mols + 1]), the edges of each molecule stably sorted by destination atom, with the
 * store-wide CSR rowptr over destination atoms and the augmented edge rows of the aggregation plan.  Three entry points
 * build the batch of ids[0], ids[1], ... (any order, duplicates allowed).  Every output element has exactly one writer
 * (no atomics): results are deterministic. */
/* Offsets (data.py:1479-1501, the bookkeeping of all_molecules[ids]): rows[i] = id2row[ids[i]], or -1 where ids[i] lies
 * outside [0, n_table) or names an absent drug (id2row < 0); out_atom_ptr / out_edge_ptr [n_ids + 1] = exclusive scans of
 * the per-drug atom / edge counts (0 for an id outside the store), correct for any n_ids (two launches: per-workgroup sums,
 * then each workgroup adds the sums before it); totals[0] = atoms, [1] = edges, [2] = ids outside the store (the status:
 * 0 = every id known), [3] = position of the first such id.  workspace: mdg_collate_offsets_workspace_bytes(n_ids). */
size_t mdg_collate_offsets_workspace_bytes(int64_t n_ids);
int mdg_collate_offsets(const int64_t* ids, int64_t n_ids, const int64_t* id2row, int64_t n_table, const int64_t* atom_ptr,
                        const int64_t* edge_ptr, int64_t n_mols, int64_t* rows, int64_t* out_atom_ptr, int64_t* out_edge_ptr,
                        int64_t* totals, void* workspace, size_t workspace_bytes, void* stream);

/* Molecules (data.py:1479-1501, all_molecules[ids], plus the CSR plan graph_plans.molecule_plan would sort for): one launch
 * over the output rows (tiles of atoms, then tiles of edges; a row finds its drug by bisection of out_atom_ptr / out_edge_ptr).
 * n_atoms / n_edges are totals[0] / totals[1] of mdg_collate_offsets; every rows[i] must be a store row.  Writes
 * node_feature [n_atoms, 67], node2graph [n_atoms], edge_list [n_edges, 3] (source and destination rebased as
 * old - atom_ptr[row] + out_atom_ptr[b], bond type copied), edge_feature [n_edges, 18], edge_weight [n_edges], and the plan:
 * rowptr [n_atoms + 1] (store_rowptr[a] - edge_ptr[row] + out_edge_ptr[b]; rowptr[n_atoms] = n_edges), col [n_edges] (the
 * rebased sources), edge_feat_aug [n_edges, 20], w [n_edges] (nullable: the weights again, for stores with non-unit weights). */
int mdg_collate_molecules(const int64_t* rows, const int64_t* out_atom_ptr, const int64_t* out_edge_ptr, int64_t n_ids,
                          int64_t n_atoms, int64_t n_edges, const int64_t* atom_ptr, const int64_t* edge_ptr,
                          const float* store_node_feature, const int64_t* store_edge_list, const float* store_edge_feature,
                          const float* store_edge_weight, const float* store_edge_feat_aug, const int64_t* store_rowptr,
                          float* node_feature, int64_t* node2graph, int64_t* edge_list, float* edge_feature, float* edge_weight,
                          int64_t* rowptr, int64_t* col, float* edge_feat_aug, float* w, void* stream);

/* Tabular rows (data.py:1479-1501, tabular_mod_stores[mod][ids] and the 16 tx_store[...][ids]): for each of n_segments
 * segments, out[s][b, :] = src[s][rows[b], :] for the segment's n_sources stacked equal-shaped sources (src [n_sources,
 * n_store_rows, width], out [n_sources, n_ids, width], both dense: exact width, no padding), all segments in one launch.
 * The *_host arguments are HOST arrays of n_segments entries.  A negative row is skipped (its output rows stay unwritten).
 * Rows are read with the widest load the segment's width and base addresses allow (16, 8 or 4 bytes). */
int mdg_collate_rows(const float* const* src_host, float* const* out_host, const int64_t* n_sources_host,
                     const int64_t* width_host, int n_segments, int64_t n_store_rows, const int64_t* rows, int64_t n_ids,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADRIGAL_HIP_H */
