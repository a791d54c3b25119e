/*
 * libmi355_retrieval — C ABI of the MI355X-native embed-then-rank hot path.
 *
 * Drop-in boundary.  The reference (vitasoftAI/ImageRetrievalResearch) has no
 * FFI: its "operator interface" for this path is the timm model object plus a handful of torch
 * calls.  Each entry point below names the reference call it replaces (file:line relative to the
 * reference checkout).  Plain pointers and sizes only; no torch types.  All pointers are DEVICE
 * pointers on the current HIP device unless a parameter says "host".  `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); every launch goes on that stream and nothing here
 * synchronises, so torch's `.item()` / `.cpu()` order correctly behind it.
 *
 * Error model: every function returns 0 on success, nonzero otherwise, and never aborts;
 * mi355_last_error() returns a thread-local message for the last failure.
 *
 * The Python host side (imageretrievalresearch_amd/) binds exactly these symbols via ctypes; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 */
#ifndef MI355_RETRIEVAL_H
#define MI355_RETRIEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_ABI_VERSION 3

/* ------------------------------------------------------------------ library / errors */
int mi355_abi_version(void);
const char* mi355_last_error(void);
/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int mi355_device_count(void);

/* ------------------------------------------------------------------ synthetic data
 * Portable counter-based generator, bit-identical to imageretrievalresearch_amd/synth.py.
 * kind 0 = uniform [0,1), 1 = unit normal (Irwin-Hall 4).  out[i] = f(seed, offset + i). */
int mi355_synth_fill(float* out, int64_t n, uint64_t seed, int64_t offset, int kind, void* stream);

/* ------------------------------------------------------------------ rank: cosine + top-k
 * Replaces torch.nn.CosineSimilarity(dim=1, eps=1e-6) + torch.topk at
 *   train/train.py:250-251, :345-356 ; inference/inference.py:226-242 ; notebook raw :231-251.
 * Semantics (pinned): score[q][g] = sum_d (Q[q][d]/max(|Q[q]|,eps)) * (G[g][d]/max(|G[g]|,eps)),
 * fp32 throughout (exact-f32 MFMA); top-k sorted by descending score, ties -> lower index first; a NaN score orders as
 * the largest value (as torch.topk does), two NaNs tie. */

/* out[r][:] = in[r][:] / max(||in[r]||_2, eps); in == out allowed.  rows x dim fp32 row-major.  A row with a NaN element comes
 * out NaN in every element (its norm is NaN, not eps).  in and out may start at any 4-byte aligned address. */
int mi355_l2_normalize_rows(const float* in, float* out, int64_t rows, int dim, float eps, void* stream);

/* Bytes of scratch mi355_rank_topk needs for (Q, G, D, k). */
size_t mi355_rank_workspace_bytes(int64_t Q, int64_t G, int dim, int k);

/* All-pairs cosine + top-k.
 *   queries  [Q][dim] fp32 (raw, normalised internally)
 *   gallery  [G][dim] fp32; gallery_is_normalized != 0 promises rows already went through
 *            mi355_l2_normalize_rows (the resident-gallery fast path), else norms are applied here
 *   out_val  [Q][k] fp32, out_idx [Q][k] int64 (index into gallery + idx_offset)
 *   idx_offset: added to every index (global row of this shard's first row)
 * Arithmetic: fp32 in, fp32 accumulation, fp32 scores.  For Q > 4 and 16-byte aligned gallery rows the products run on the
 * bf16 matrix pipe as a three-way split of each fp32 operand (six bf16 x bf16 products per element, each exact in the
 * fp32 accumulator; dropped terms <= 2^-23 of a product - one fp32 rounding); the environment variable
 * MI355_RANK_EXACT_F32=1 selects the exact fp32 MFMA (an fmaf chain) instead.  A score depends on its query row and
 * gallery row only (not on Q, G, tiles or shards), so sharded and unsharded results are bit-identical.
 * Errors: k < 1, k > G, Q < 1, dim < 1, workspace too small. */
int mi355_rank_topk(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                    int gallery_is_normalized, int k, float eps, int64_t idx_offset,
                    float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Scores only: out[Q][G] fp32 cosine matrix (same kernel as above without the selection). */
int mi355_cosine_scores(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                        int gallery_is_normalized, float eps, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Prepared gallery for RESIDENT galleries (the reference re-reads and re-normalises its gallery for every query,
 * train/train.py:250; here it is normalised once when rows are added, and - optionally - split once into the three bf16 planes
 * the cosine GEMM multiplies, stored in the GEMM's fragment order: 6 B per element, mi355_gallery_planes_bytes(G, dim) bytes).
 * mi355_rank_topk_prepared then does no per-call work on the gallery side at all; k <= 8 and Q > 4 (other shapes: mi355_rank_topk
 * with the fp32 rows).  Values and indices are bit-identical to mi355_rank_topk(gallery_is_normalized = 1) on the same rows. */
size_t mi355_gallery_planes_bytes(int64_t G, int dim);
int mi355_gallery_prepare(const float* gallery_normalized, int64_t G, int dim, void* planes, size_t planes_bytes, void* stream);
int mi355_rank_topk_prepared(const float* queries, int64_t Q, const void* gallery_planes, int64_t G, int dim, int k, float eps,
                             int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Half-precision resident gallery (fp16 rows: half the bytes of fp32 rows, a third of the bf16 planes).
 * Stored row: fp16_rne(l2_normalize_rows(x, eps)), bit for bit the fp32 row mi355_l2_normalize_rows writes for the same x,
 * rounded once to nearest-even (not renormalised after rounding); rows_are_normalized != 0 rounds x as it is.  Row r starts
 * at element r * ld, ld = dim rounded up to a multiple of 64 (128 B); elements dim .. ld-1 are zero.  The buffer is
 * appendable: converting n rows to out + r * ld * 2 bytes writes rows r .. r+n-1.  out must be 16-byte aligned.
 * mi355_gallery_f16_bytes(G, dim) = G * ld * 2. */
size_t mi355_gallery_f16_bytes(int64_t G, int dim);
int mi355_gallery_to_f16(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* out, size_t out_bytes,
                         void* stream);
/* Cosine + top-k against an fp16 gallery (16-byte aligned, layout above).  score = qn . float(row), qn the query normalised as
 * mi355_rank_topk normalises it, fp32 accumulation; the query is carried as two fp16 planes hi = fp16(qn),
 * lo = fp16((qn - hi) * 2^11) with one accumulator each (Q > 4), or as fp32 (Q <= 4): |score - qn . row| ~1e-7, far inside
 * 1e-5.  Order, ties and NaN as mi355_rank_topk; any k in [1, min(1024, G)], any dim >= 1, Q >= 0 (Q = 0 does nothing).
 * workspace: mi355_rank_f16_workspace_bytes(Q, G, dim, k). */
size_t mi355_rank_f16_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_rank_topk_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                        int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Filtered search: the top-k of the rows that are ELIGIBLE for each query.  Row j (global index j + idx_offset) is eligible
 * for query q when
 *   - exclude is NULL, exclude[q] < 0, or exclude[q] != j + idx_offset (leave-one-out: the query's own row), and
 *   - label_mode is MI355_LABEL_ANY (labels unused, may be NULL), MI355_LABEL_SAME and gallery_labels[j] == query_labels[q],
 *     or MI355_LABEL_DIFFERENT and gallery_labels[j] != query_labels[q].
 * query_labels / exclude [Q], gallery_labels [G]: device int64.  Scores are bit for bit those of the unfiltered search, the
 * order is its order (descending, ties to the lower index, NaN first); an ineligible row never appears, NaN or not.  With
 * fewer than k eligible rows the remaining slots are (-inf, -1); k <= G is the only size rule.  Workspace: that of the
 * unfiltered twin (mi355_rank_workspace_bytes / mi355_rank_f16_workspace_bytes).  A prepared gallery has no filtered
 * search: filter with mi355_rank_topk_filtered on its fp32 rows (same results). */
enum { MI355_LABEL_ANY = 0, MI355_LABEL_SAME = 1, MI355_LABEL_DIFFERENT = 2 };
typedef struct mi355_rank_filter {
    const int64_t* query_labels;
    const int64_t* gallery_labels;
    int label_mode;
    const int64_t* exclude;
} mi355_rank_filter;
int mi355_rank_topk_filtered(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                             int gallery_is_normalized, int k, float eps, int64_t idx_offset, const mi355_rank_filter* filter,
                             float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
int mi355_rank_topk_f16_filtered(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                                 int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* Adjusted scores: CSLS (Conneau et al., ICLR 2018) and cohort normalisation (Z-, T-, S-norm) are one affine map of the score
 * with per-query and per-gallery-row coefficients.  For query q and gallery row g, in fp32 and without fused multiply-add:
 *   s = the pair's score as the tiled GEMM of the rows leaves it (fp32 rows: acc * 1/|row|; fp16 rows: the f16 loop's score)
 *   w = aq[q] + ag[g],  c = bq[q] + bg[g]          (a NULL vector counts as 0.0f; at least one of aq / ag is given)
 *   t = fp32(fp32(s * w) - c)
 * aq / bq [Q], ag / bg [G]: device fp32.  mi355_rank_topk_adjusted is the filtered search over t (filter NULL: every row is
 * eligible): descending t, ties to the lower index, NaN largest, (-inf, -1) beyond the eligible rows, and t is what is
 * returned.  For k <= 8 and Q > 4 the map is applied where the fused selection writes its score tile, so no Q x G slab exists;
 * other shapes select from the adjusted slab.  Every Q runs on the tiles (Q <= 4 has no GEMV here): t depends on the pair and
 * the four coefficients alone, not on Q, k, the tile height, the two-launch cut or query_block (> 0: at most that many queries
 * per GEMM call; 0: the library's rule).  mi355_cosine_scores_adjusted writes the slab t [Q][G].  A prepared gallery is searched
 * on its fp32 rows.  Workspace: mi355_rank_adjusted[_f16]_workspace_bytes(Q, G, dim, k), k = 0 for the slab entries.
 * Errors (before any HIP call): a null pointer, aq and ag both NULL, k outside [1, 1024], k > G, a short workspace, fp16 rows
 * that are not 16-byte aligned. */
typedef struct mi355_score_adjust {
    const float* aq;
    const float* bq;
    const float* ag;
    const float* bg;
} mi355_score_adjust;
size_t mi355_rank_adjusted_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
size_t mi355_rank_adjusted_f16_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_rank_topk_adjusted(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                             int k, float eps, int64_t idx_offset, const mi355_score_adjust* adjust, const mi355_rank_filter* filter,
                             int64_t query_block, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                             void* stream);
int mi355_rank_topk_adjusted_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                                 int64_t idx_offset, const mi355_score_adjust* adjust, const mi355_rank_filter* filter,
                                 int64_t query_block, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                                 void* stream);
int mi355_cosine_scores_adjusted(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                                 float eps, const mi355_score_adjust* adjust, int64_t query_block, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream);
int mi355_cosine_scores_adjusted_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                                     const mi355_score_adjust* adjust, int64_t query_block, float* out, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* Statistics of a top-n result val / idx [N][n] (a search's output; idx < 0: a pad), one row each, in float64:
 *   count[r] = the real entries (idx >= 0);  sum = their values added in slot order;  mean64 = sum / count;
 *   std64 = sqrt(sum of (value - mean64)^2 in slot order / count)   (the population deviation)
 * mean[r] = fp32(mean64), std[r] = fp32(std64); a row with no real entry gives mean 0 and std 0.  With a / b (both or neither):
 * std_f = max(std64, min_std), a[r] = fp32(half / std_f), b[r] = fp32(mean64 * half / std_f): the coefficients of a cohort
 * normalisation (half = 1 for a one-sided norm, 0.5 for each side of S-norm).  1 <= n <= 1024; half and min_std finite,
 * min_std >= 0. */
int mi355_topn_stats(const float* val, const int64_t* idx, int64_t N, int n, double half, double min_std, float* mean, float* std,
                     int32_t* count, float* a, float* b, void* stream);

/* The branch the calling thread's last mi355_rank_topk* call took: MI355_RANK_PATH_* of the score stage, | FUSED when the
 * selection ran in the GEMM epilogue, | BITONIC when a score slab was selected with k > 8 (else the small-k selection). */
enum {
    MI355_RANK_PATH_GEMV = 1,           /* k_cos_gemv: Q <= 4 */
    MI355_RANK_PATH_SPLIT = 2,          /* k_cos_gemm_split: the bf16 three-way split */
    MI355_RANK_PATH_EXACT_F32 = 3,      /* k_cos_gemm: MI355_RANK_EXACT_F32=1, or unaligned rows */
    MI355_RANK_PATH_PREPARED = 4,       /* k_cos_gemm_pre */
    MI355_RANK_PATH_F16_GEMM = 5,       /* k_cos_gemm_f16 */
    MI355_RANK_PATH_F16_GEMV = 6,       /* k_cos_gemv_f16 */
    MI355_RANK_PATH_I8_GEMM = 7,        /* k_cos_gemm_i8 */
    MI355_RANK_PATH_I8_GEMV = 8,        /* k_cos_gemv_i8: Q <= 4 */
    MI355_RANK_PATH_PQ = 9,             /* k_pq_scan / k_pq_scores: the table scan over product-quantised rows (mi355_pq_search) */
    MI355_RANK_PATH_BINARY = 10,        /* k_bin_scan: the popcount scan over sign-bit rows (mi355_binary_search) */
    MI355_RANK_PATH_BINARY_ASYM = 11,   /* k_bin_asym_scan: int8 query codes against sign-bit rows on the i8 MFMA
                                           (mi355_binary_asym_search) */
    MI355_RANK_PATH_FP4_GEMM = 12,      /* k_cos_gemm_fp4 */
    MI355_RANK_PATH_FP4_GEMV = 13,      /* k_cos_gemv_fp4: Q <= 4 */
    MI355_RANK_PATH_FUSED = 0x100,
    MI355_RANK_PATH_BITONIC = 0x200
};
int mi355_rank_last_path(void);
/* Developer entries (tests): where a tiled cosine GEMM call is cut into its two launches.  A call over ntx = ceil(G / 128)
 * column tiles and ny = ceil(Q / 128) tiles of 128 queries (Q > 64) with more tiles than `slots` resident workgroups, and a tile
 * count that is no multiple of slots, runs column tiles [0, x1) as 128-query tiles and [x1, ntx) as a second launch of
 * ceil(Q / 64) tiles of 64 queries each; x1 = mi355_rank_round_split(ntx, ny, slots) (host only, no HIP call; ntx >= 0, ny >= 1,
 * slots >= 1, else -1), and x1 == ntx is a single launch.
 * mi355_rank_set_round_slots(slots > 0): the calling thread's searches cut their GEMM calls as if the device had that many
 * slots; 0 restores the device's own count (CUs x resident workgroups of the kernel); negative: an error.  Only the cut moves:
 * the kernels, their LDS and the occupancy query are the same, and by the promise above (a score depends on its two rows only)
 * no result of any entry depends on it.  For tests of the seam between the two launches; it costs speed.
 * mi355_rank_last_tiles(out, n): the cut of the calling thread's last tiled GEMM call, out[0 .. min(n, 5)) = {slots used, query
 * tiles of the main launch, its column tiles, column tiles of the tail launch (0: one launch), query tiles of the tail launch (0
 * without a tail)}; a search of several query blocks reports its last block.  Returns the number of values written, or a negative
 * error (out NULL, n < 1).  All zero before the thread's first such call. */
int mi355_rank_round_split(int ntx, int ny, int slots);
int mi355_rank_set_round_slots(int slots);
int mi355_rank_last_tiles(int* out, int n);

/* Verification ROC (utils/roc_curve_from_scratch.py): genuine / impostor pairs counted per threshold, without a score slab.
 * thresholds: HOST float64 [T], 1 <= T <= MI355_ROC_MAX_THRESHOLDS, finite, ascending (equal neighbours allowed); checked
 * before any HIP call.  thresholds_dev: the same T values on the device (the kernels read them from there).
 * A pair is predicted positive at t iff score >= t compared in float64: an fp32 score is compared in fp32 with the smallest
 * float f such that (double)f >= t, which is that comparison exactly; a NaN score is never >= t.
 * hist [2][T + 1] int64 (zeroed by the call, then filled): hist[0][b] genuine / hist[1][b] impostor pairs whose score is >= exactly
 * b of the thresholds.  Counts are integers: the same every run.
 *
 * mi355_roc_pairs_hist: every (query q, gallery row j) pair, scored with the bits mi355_cosine_scores gives that pair on the
 * same path (split bf16, or MI355_RANK_EXACT_F32=1 / unaligned rows: exact fp32; always the tiled GEMM, also for Q <= 4),
 * genuine iff query_labels[q] == gallery_labels[j]; a pair with exclude[q] == j + idx_offset is not counted (exclude may be
 * NULL; exclude[q] < 0: none).  query_labels / exclude [Q], gallery_labels [G]: device int64.
 * workspace: mi355_roc_pairs_workspace_bytes(Q, G, dim) (normalised queries, split planes, 1 / |row|; no Q x G term).
 * mi355_roc_pairs_hist_f16: the same against an fp16 gallery (mi355_gallery_to_f16 layout), scored with the bits of
 * mi355_rank_topk_f16's tiled kernel.  workspace: mi355_roc_pairs_f16_workspace_bytes(Q, G, dim). */
#define MI355_ROC_MAX_THRESHOLDS 4096
size_t mi355_roc_pairs_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_roc_pairs_hist(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                         float eps, const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude,
                         int64_t idx_offset, const double* thresholds, const double* thresholds_dev, int T, int64_t* hist,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t mi355_roc_pairs_f16_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_roc_pairs_hist_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                             const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                             const double* thresholds, const double* thresholds_dev, int T, int64_t* hist, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The same histogram over n given pair scores (fp32, or float64 with scores_f64 = 1: compared in float64 with thresholds_dev)
 * and int8 class codes actual [n]: 1 genuine, 0 impostor, any other value counted in neither class. */
int mi355_roc_scores_hist(const void* scores, int scores_f64, int64_t n, const int8_t* actual, const double* thresholds,
                          const double* thresholds_dev, int T, int64_t* hist, void* stream);
/* One launch: hist [2][T + 1] -> counts [4][T] int64 (tp, fp, fn, tn; tp[i] = genuine pairs with score >= t_i),
 * totals [2] int64 (genuine, impostor pairs), rates [2][T] float64 (tpr = tp / (tp + fn), fpr = fp / (fp + tn); NaN where
 * the denominator is 0), auc [1] float64 = |trapezoid of tpr over fpr| in threshold order (numpy.trapz(tpr, fpr), unrounded). */
int mi355_roc_finalize(const int64_t* hist, int T, int64_t* counts, int64_t* totals, double* rates, double* auc, void* stream);

/* Cosine range search: every (query q, gallery row j) pair whose score is >= threshold, as a CSR result.
 * Row j (global index j + idx_offset) is a hit iff its score >= threshold compared in float64 (an fp32 score is compared with
 * the smallest float f such that (double)f >= threshold, as in the ROC entries), a NaN score never; filter (may be NULL) as in
 * mi355_rank_topk_filtered.  Scores have the bits mi355_cosine_scores gives the pair on the same path (split bf16, or
 * MI355_RANK_EXACT_F32=1 / unaligned rows: exact fp32; always the tiled GEMM, also for Q <= 4); _f16: the bits of
 * mi355_rank_topk_f16's tiled kernel (fp16 gallery, mi355_gallery_to_f16 layout, 16-byte aligned).
 * Two steps:
 *   mi355_cosine_range[_f16] runs the search: candidates [2][capacity] 8-byte entries (16 * capacity bytes, 8-byte aligned)
 *     hold the hits; *nnz (host) = the exact number of hits.  If *nnz > capacity the candidates are incomplete: search again
 *     with capacity >= *nnz (that call fits).  One host sync per query block (its hit count).  Q >= 0, G >= 0 (Q = 0 or G = 0:
 *     no hit), dim >= 1, threshold finite; every argument is checked before any HIP call.
 *     workspace: mi355_range_workspace_bytes / mi355_range_f16_workspace_bytes(Q, G, dim) (no Q x G term).
 *   mi355_range_compact (after a search with *nnz <= capacity, same candidates, workspace and Q): offsets [Q + 1] int64,
 *     indices [nnz] int64 (global rows: pass the search's idx_offset), scores [nnz] fp32.  The hits of query q are
 *     [offsets[q], offsets[q + 1]), rows ascending; the result is the same bit for bit on every run and every query split. */
size_t mi355_range_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_cosine_range(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                       float eps, double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates,
                       int64_t capacity, int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream);
size_t mi355_range_f16_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_cosine_range_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps, double threshold,
                           int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity, int64_t* nnz,
                           void* workspace, size_t workspace_bytes, void* stream);
int mi355_range_compact(const void* candidates, int64_t capacity, int64_t Q, int64_t nnz, int64_t idx_offset, const void* workspace,
                        size_t workspace_bytes, int64_t* offsets, int64_t* indices, float* scores, void* stream);

/* 8-bit resident gallery (int8 codes and one fp32 scale per row: a quarter of the bytes of fp32 rows, half of fp16 rows).
 * Below, "fp32" means one IEEE rounding per named operation.
 * Row quantiser (gallery rows, and the hi plane of a query): n = the fp32 row mi355_l2_normalize_rows writes for x, bit for
 * bit (rows_are_normalized != 0: n = x as it is); amax = max_i |n_i|.
 *   - any n_i NaN, or amax not finite: scale = NaN, every code 0;
 *   - else amax < 1e-30f: scale = 0, every code 0;
 *   - else scale = amax / 127.0f, inv = 127.0f / amax (fp32 divisions), code_i = clamp(rintf(n_i * inv), -127, 127), rintf rounding
 *     halves to even.
 * codes: int8, row r at byte r * ld, ld = dim rounded up to a multiple of 128; bytes dim .. ld-1 are zero.  scales: fp32 [G].
 * Both are appendable: converting n rows to codes + r * ld, scales + r writes rows r .. r+n-1.  codes must be 16-byte aligned;
 * dim <= 65536.  mi355_gallery_i8_bytes(G, dim) = G * ld.
 * Query planes, made per call from qn = l2_normalize_rows(q): (hi, s_q) = the row quantiser of qn; r_i = fmaf(-(float)hi_i, s_q,
 * qn_i); lo_i = clamp(rintf(r_i * (128.0f / s_q)), -127, 127), |lo_i| <= 64 up to rounding, lo = 0 when s_q is 0 or NaN: the query
 * keeps about 15 bits, its error is 1/256 of the gallery's.
 * Score of query q against row g with codes c and scale s_g: acc_hi = sum_i hi_i c_i and acc_lo = sum_i lo_i c_i, exact in int32;
 * t = fmaf((float)acc_lo, 0x1p-7f, (float)acc_hi) (the conversions round to nearest even); score = (t * s_q) * s_g, two fp32
 * multiplies in that order.  A NaN row scores NaN (it ranks first, as in mi355_rank_topk), a zero row 0, a NaN query NaN
 * everywhere.  The sums are integers, so EVERY path returns these bits for a (query, row) pair: the GEMV (Q <= 4), the tiled
 * GEMM with 64- and 128-query tiles in its main and its tail launch, the fused selection and the score slab, the filtered and the
 * unfiltered search, the range search, and the scan of probed lists (mi355_ivf_scan_i8, in the IVF block).  Order, ties, NaN and
 * pads: the selection of mi355_rank_topk.
 * The gallery argument of every entry is the pair (codes, scales).  Arguments are checked as for the _f16 entries (null, shape, k,
 * alignment, workspace), and dim <= 65536.  workspace: mi355_rank_i8_workspace_bytes(Q, G, dim, k) (both top-k entries),
 * mi355_range_i8_workspace_bytes(Q, G, dim); mi355_cosine_range_i8 is mi355_cosine_range_f16 over int8 rows (results read with
 * mi355_range_compact). */
size_t mi355_gallery_i8_bytes(int64_t G, int dim);
int mi355_gallery_to_i8(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* codes, size_t codes_bytes,
                        float* scales, void* stream);
size_t mi355_rank_i8_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_rank_topk_i8(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, int k, float eps,
                       int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
int mi355_rank_topk_i8_filtered(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, int k,
                                float eps, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                void* workspace, size_t workspace_bytes, void* stream);
size_t mi355_range_i8_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_cosine_range_i8(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, float eps,
                          double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                          int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream);

/* 4-bit resident gallery (e2m1 codes, two per byte, and one fp32 multiplier per row: half the bytes of int8 rows), searched on the
 * block-scaled fp4 matrix instruction of gfx950.  Below, "fp32" means one IEEE rounding per named operation.
 * e2m1: a code is 4 bits, bit 3 the sign, bits 0..2 the index m of the magnitude in {0, 0.5, 1, 1.5, 2, 3, 4, 6} (the OCP
 * encoding).  e2m1(a) of an fp32 a rounds |a| to the nearest magnitude, a tie to the even index:
 *     m = (|a| > 0.25) + (|a| >= 0.75) + (|a| > 1.25) + (|a| >= 1.75) + (|a| > 2.5) + (|a| >= 3.5) + (|a| > 5)
 * (so 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4, and every |a| >= 6 -> 6); the sign bit is set when
 * a < 0 and m != 0: there is no negative zero, a zero is the code 0.  value(code) is the signed magnitude.
 * Packing: dimension 2j is the low nibble of byte j of a row, dimension 2j+1 the high nibble; row r at byte r * ld, ld =
 * ceil(dim / 2) rounded up to a multiple of 128; every nibble from dim on is 0.
 * Row quantiser: n = the fp32 row mi355_l2_normalize_rows writes for x, bit for bit (rows_are_normalized != 0: n = x as it is);
 * amax = max_i |n_i|.
 *   - any n_i NaN, or amax not finite: mult = NaN, every code 0;
 *   - else amax < 1e-30f: mult = 0, every code 0;
 *   - else inv = 6.0f / amax (fp32 division), a_i = n_i * inv (fp32), code_i = e2m1(a_i); n2 = sum_i (2 value(code_i))^2, an
 *     exact integer (<= 144 * dim < 2^24); mult = 1.0f / sqrtf(0.25f * (float)n2): the product is exact, the square root and the
 *     division are fp32, correctly rounded (n2 = 0 cannot happen here; it would give mult = 0).  mult is 1 / |value(codes)|: the
 *     decoded row value(code_i) * mult has unit length, whatever the quantiser's own scale was.
 * mults: fp32 [G] beside the codes.  Both are appendable: converting n rows to codes + r * ld, mults + r writes rows r .. r+n-1.
 * codes must be 16-byte aligned; dim <= 65536.  mi355_gallery_fp4_bytes(G, dim) = G * ld; a row costs ld + 4 bytes.
 * Query planes, made per call from qn = l2_normalize_rows(q), amax_q = max_i |qn_i| (NaN / zero cases as the row quantiser: s_q =
 * NaN or 0, both planes 0):
 *     s_q = amax_q / 6.0f;  inv_q = 6.0f / amax_q                                 (two fp32 divisions)
 *     hi_i = e2m1(qn_i * inv_q)                                                   (fp32 product)
 *     r_i = fmaf(-value(hi_i), s_q, qn_i) / s_q                                   (one fused multiply-add, one fp32 division)
 *     lo_i = e2m1(4.0f * r_i)                                                     (exact product; |r_i| <= 1 up to its two roundings:
 *                                                                                  |value(lo_i)| <= 4)
 * Score of query q against row g with codes c and multiplier mult_g: acc_hi = sum_i value(hi_i) value(c_i), acc_lo = sum_i
 * value(lo_i) value(c_i).  Every product is a multiple of 0.25 of magnitude <= 36, so every partial sum in any order is a
 * multiple of 0.25 below 36 * 65536 = 2^24 * 0.140625: exact in fp32.  t = fmaf(acc_lo, 0.25f, acc_hi); score = (t * s_q) *
 * mult_g, two fp32 multiplies in that order.  A NaN row scores NaN (it ranks first, as in mi355_rank_topk), a zero row 0, a NaN
 * query NaN everywhere.  The sums are exact, so EVERY path returns these bits for a (query, row) pair: the GEMV (Q <= 4, integer
 * dot products of the codes doubled), the tiled GEMM with 64- and 128-query tiles in its main and its tail launch, the fused
 * selection and the score slab, the filtered and the unfiltered search and the range search.  Order, ties, NaN and pads: the
 * selection of mi355_rank_topk.
 * The gallery argument of every entry is the pair (codes, mults).  Arguments are checked as for the _i8 entries (null, shape, k,
 * alignment, workspace, dim <= 65536).  workspace: mi355_rank_fp4_workspace_bytes(Q, G, dim, k) (both top-k entries),
 * mi355_range_fp4_workspace_bytes(Q, G, dim); mi355_cosine_range_fp4 is mi355_cosine_range_i8 over fp4 rows. */
size_t mi355_gallery_fp4_bytes(int64_t G, int dim);
int mi355_gallery_to_fp4(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* codes, size_t codes_bytes,
                         float* mults, void* stream);
size_t mi355_rank_fp4_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_rank_topk_fp4(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, int k, float eps,
                        int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
int mi355_rank_topk_fp4_filtered(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, int k,
                                 float eps, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                 void* workspace, size_t workspace_bytes, void* stream);
size_t mi355_range_fp4_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_cosine_range_fp4(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, float eps,
                           double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                           int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream);

/* Full-gallery ranks: the 1-based rank of every POSITIVE of every query among the query's eligible rows, without a score slab
 * or a sort of the gallery.  Eligible for query q: every gallery row but exclude[q] - idx_offset (exclude may be NULL;
 * exclude[q] < 0: none); positive: an eligible row with gallery_labels[j] == query_labels[q].  The order is the top-k search's:
 * higher score first with NaN above every number and -0 equal to +0, on equal scores the lower row; as one 64-bit composite
 * per (score, row), (order-preserving key of the score << 32) | ~(uint32_t)local row, larger = ranked earlier.  Scores have the
 * bits mi355_cosine_scores gives the pair on the same path (_f16: mi355_rank_topk_f16's tiled kernel), as in the range entries.
 * Four steps:
 *   mi355_positives_range[_f16]: mi355_cosine_range[_f16] without a threshold: every row the filter keeps is a hit whatever its
 *     score, NaN included.  filter: MI355_LABEL_SAME (required) and the exclusion.  Candidates, *nnz, workspace
 *     (mi355_range[_f16]_workspace_bytes) and mi355_range_compact as there: offsets [Q + 1], the positives' rows and scores.
 *   mi355_rank_positives_keys: the composites keys [nnz] of (indices, scores) [nnz] (global rows: pass the search's idx_offset).
 *     The caller sorts each query's segment descending (pos_keys below).
 *   mi355_rank_positives[_f16]: the counting pass, the cosine GEMM again with an epilogue that adds every eligible NON-positive
 *     row of query q to before[offsets[q] + b], b = the number of q's positives ranked before that row, unless b = R_q (such a
 *     row changes no rank and is not counted).  before [nnz] uint32 (zeroed by the call).  offsets [Q + 1] int64 and pos_keys
 *     [nnz] on the device; offsets_host (may be NULL): the same offsets on the host, checked before any HIP call (start at 0,
 *     monotone, at most G per query, end at nnz).  query_block: queries per GEMM call (0: as many as the grid allows; the result
 *     does not depend on it).  Q >= 1, 1 <= G < 2^31 - 128, dim >= 1.  Counts are integers: the same every run.
 *     workspace: mi355_rank_positives[_f16]_workspace_bytes(Q, G, dim) (normalised queries, planes of one call, 1 / |row|).
 *   mi355_rank_positives_finalize (one launch, one wave per query): ranks [nnz] int64, rank of the i-th positive of q (in
 *     pos_keys order) = i + 1 + before[offsets[q]] + .. + before[offsets[q] + i]; ap [Q] float64 = (sum_i (i + 1) / rank_i) / R_q,
 *     the terms added in the order i = 0, 1, ..; first_rank [Q] int64 = rank_0.  A query without positives: ap 0, first_rank 0. */
int mi355_positives_range(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                          float eps, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                          int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream);
int mi355_positives_range_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                              int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity, int64_t* nnz,
                              void* workspace, size_t workspace_bytes, void* stream);
int mi355_rank_positives_keys(const int64_t* indices, const float* scores, int64_t nnz, int64_t idx_offset, uint64_t* keys,
                              void* stream);
size_t mi355_rank_positives_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_rank_positives(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                         float eps, const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude,
                         int64_t idx_offset, const int64_t* offsets, const int64_t* offsets_host, const uint64_t* pos_keys,
                         int64_t nnz, uint32_t* before, int64_t query_block, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t mi355_rank_positives_f16_workspace_bytes(int64_t Q, int64_t G, int dim);
int mi355_rank_positives_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                             const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                             const int64_t* offsets, const int64_t* offsets_host, const uint64_t* pos_keys, int64_t nnz,
                             uint32_t* before, int64_t query_block, void* workspace, size_t workspace_bytes, void* stream);
int mi355_rank_positives_finalize(const int64_t* offsets, const uint32_t* before, int64_t Q, int64_t nnz, int64_t* ranks, double* ap,
                                  int64_t* first_rank, void* stream);

/* Query expansion / database-side augmentation (alpha-QE, DBA; Radenovic, Tolias and Chum, TPAMI 2018): one output row per
 * row r of the neighbour lists vals / idx [R][n] (device fp32 / int64, the output of a search, rank order):
 *   w_j = v_j ^ alpha for a USED slot: v_j > 0 and l_j = idx[r][j] - idx_offset in [0, gallery_rows); every other slot
 *         (pads (-inf, -1), scores <= 0 or NaN, rows outside the gallery) is skipped and its row never read.  alpha 0, 1, 2, 3
 *         give 1, v, v * v, (v * v) * v; other alpha powf(v, alpha).  alpha finite and >= 0.
 *   x   = base_r + sum_j w_j * gallery[l_j], fp32 per element, j = 0 .. n-1 in order, each w_j * row rounded before its add
 *         (no fma); fp16 rows are widened exactly.  base_r: base row r as it is, or with normalize_base (fp32 base only)
 *         l2_normalize_rows(base_r) with the bits of mi355_l2_normalize_rows.
 *   out = l2_normalize_rows(x, eps) bit for bit (MI355_DTYPE_F32), or fp16 of it as mi355_gallery_to_f16 stores it
 *         (MI355_DTYPE_F16, elements dim .. out_ld-1 zeroed).  No atomics: each row depends only on its own base, list and
 *         weights.
 * Rows are base_ld / gallery_ld / out_ld elements apart (>= dim); when dim % 4 == 0, out is 16-byte aligned and out_ld % 4 == 0.
 * workspace: mi355_expand_workspace_bytes(R, dim, out_dtype) (fp16 output: R * dim fp32 sums; fp32 output: none, may be
 * NULL).  Every argument is checked before any HIP call; R = 0 does nothing. */
enum { MI355_DTYPE_F32 = 0, MI355_DTYPE_F16 = 1 };
size_t mi355_expand_workspace_bytes(int64_t R, int dim, int out_dtype);
int mi355_expand_rows(const void* base, int base_dtype, int64_t base_ld, int normalize_base, const void* gallery,
                      int gallery_dtype, int64_t gallery_rows, int64_t gallery_ld, int dim, const float* vals,
                      const int64_t* idx, int64_t R, int n, int64_t idx_offset, float alpha, float eps, void* out,
                      int out_dtype, int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream);

/* k-reciprocal re-ranking (Zhong, Zheng, Cao and Li, CVPR 2017), gallery-graph variant: the neighbourhoods of gallery rows are
 * taken inside the gallery, queries are attached to that graph, d(a, b) = 1 - cos(a, b), and only a shortlist is re-scored.
 * Inputs are the lists of the library's own search: graph [G][k1] int64 = the top-k1 OTHER rows nn(g) of every gallery row
 * (a search with exclude = g), tau [G] = the k1-th of their scores.  1 <= k1 <= MI355_KR_MAX_K1, h = (k1 + 1) / 2, nn_h = the
 * first h of nn.  Sparse rows are CSR: offsets [rows + 1] int64, cols int32 ascending, vals fp32.  No atomics; every sum has
 * a fixed order that depends on its own row only.  Every argument is checked before any HIP call, every index a kernel reads
 * is range-checked before it is used (a bad one is skipped), and zero rows do nothing.
 *
 * mi355_kr_sets: the expanded reciprocal set R*(r) of each of R rows with neighbour lists `lists` [R][k1] int64.
 *   gallery rows (list_vals = tau = NULL, R = G, lists = graph): R(g) = {g} + {j in nn(g) : g in nn(j)};
 *   query rows (list_vals [R][k1] their fp32 scores):            R(q) = {j in nn(q) : list_vals[q][j] >= tau[j]} (may be empty);
 *   R_h(c) = {c} + {j in nn_h(c) : c in nn_h(j)};   R*(r) = R(r) + every R_h(c), c in R(r), with 3 |R_h(c) & R(r)| > 2 |R_h(c)|
 *   (candidates and intersections always against the unexpanded R(r)).  At most (k1 + 1) (h + 1) columns per row.
 *   Two calls: cols = NULL counts and leaves the finished offsets [R + 1]; the caller reads offsets[R], allocates, and calls
 *   again with cols [cols_capacity] and those offsets to fill (a row that does not fit is not written).
 * mi355_kr_weights: vals[p] = exp(-d(r, j)) / sum over row r's columns, j = cols[p], d = 1 - s, s the fp32 dot product of row r of
 *   `rows` and row j of `gallery` (fp32 or fp16 rows, widened exactly, rows_ld / gallery_ld elements apart; both normalised by
 *   the caller).  For gallery rows pass the gallery as `rows`.  dim <= 8192.
 * mi355_kr_local_qe: out row r = (1 / k2) (own row r + gallery rows lists[r][0 .. k2 - 2]), a sparse merge summed in that order
 *   (gallery rows: own = gallery, i.e. the first k2 of [g, nn(g) ...]); 1 <= k2 <= k1 + 1; k2 = 1 copies the own rows bit for bit.
 *   Two calls as mi355_kr_sets: out_cols = out_vals = NULL counts into out_offsets, the second call fills.
 * mi355_kr_score: for query q and slot p of its shortlist (shortlist_vals / shortlist_idx [Q][K], a search's output, LOCAL rows):
 *   m = sum_c min(V'(q)[c], V'(g)[c]), dJ = 1 - m / (2 - m), out[q][p] = 1 - ((1 - lam) dJ + lam (1 - shortlist_vals[q][p])); a
 *   slot whose row is outside [0, G) gets -inf.  out [Q][K] fp32, 1 <= K <= 1024, 0 <= lam <= 1. */
#define MI355_KR_MAX_K1 32
int mi355_kr_sets(const int64_t* lists, const float* list_vals, const float* tau, int64_t R, int k1, const int64_t* graph,
                  int64_t G, int64_t* offsets, int32_t* cols, int64_t cols_capacity, void* stream);
int mi355_kr_weights(const void* rows, int rows_dtype, int64_t rows_ld, int64_t R, const void* gallery, int gallery_dtype,
                     int64_t G, int64_t gallery_ld, int dim, const int64_t* offsets, const int32_t* cols, int64_t nnz,
                     float* vals, void* stream);
int mi355_kr_local_qe(const int64_t* lists, int64_t R, int k1, int k2, const int64_t* own_offsets, const int32_t* own_cols,
                      const float* own_vals, int64_t own_nnz, const int64_t* gallery_offsets, const int32_t* gallery_cols,
                      const float* gallery_vals, int64_t gallery_nnz, int64_t G, int64_t* out_offsets, int32_t* out_cols,
                      float* out_vals, int64_t out_capacity, void* stream);
int mi355_kr_score(const int64_t* query_offsets, const int32_t* query_cols, const float* query_vals, int64_t query_nnz, int64_t Q,
                   const int64_t* gallery_offsets, const int32_t* gallery_cols, const float* gallery_vals, int64_t gallery_nnz,
                   int64_t G, const float* shortlist_vals, const int64_t* shortlist_idx, int K, float lam, float* out,
                   void* stream);

/* Diffusion re-ranking (Iscen et al., CVPR 2017), truncated to a query's shortlist (Yang et al., AAAI 2019): conjugate gradients
 * on the sub-graph of the gallery's kNN graph that the shortlist induces.  All arithmetic is fp32; no atomics on global memory;
 * every sum has a fixed order that depends on its own row or query only.  Every argument is checked before any HIP call and every
 * index a kernel reads is range-checked before it is used.
 *
 * mi355_diffusion_graph: the index rows of a kNN graph nn [G][kd] int64 / nv [G][kd] fp32 (the top-kd OTHER rows of every row
 *   and their scores), 1 <= kd <= MI355_DIFFUSION_MAX_KD, kd < G, gamma an integer in [1, 8]:
 *     a(i, t) = max(nv[i][t], 0)^gamma, by repeated multiplication left to right;
 *     j = nn[i][t]; if i occurs in nn[j] (first at slot u): cols[i][t] = j and w(i, t) = min(a(i, t), a(j, u)); otherwise the slot
 *     is empty, cols[i][t] = -1 and vals[i][t] = 0;
 *     deg[i] = sum_t w(i, t) in slot order;  c_i = 1 / sqrt(deg[i]), 0 for deg[i] = 0;  vals[i][t] = w(i, t) * (c_i * c_j).
 *   The entry of i -> j and that of j -> i hold the same bits.  Two launches; cols / vals [G][kd], deg [G].
 * mi355_diffusion_source: y[q][p] = max(shortlist_vals[q][p], 0)^gamma for p < kq and shortlist_idx[q][p] >= 0, else 0
 *   (shortlist_vals / shortlist_idx [Q][L], a search's output; 1 <= kq <= L <= 1024).
 * mi355_diffusion_solve: for every query q, (I - alpha S_L) f = y[q] by conjugate gradients, S_L the entries of cols / vals whose
 *   row and column are both in shortlist_idx[q] (LOCAL rows; a row outside [0, G) is a pad: isolated, f = -inf; a row that occurs
 *   twice is reached at its earlier position).  f0 = 0, r0 = p0 = y, rs0 = r0 . r0; before each of at most `iters` iterations
 *   the query stops when rs <= 2^-48 rs0 (so at once for y = 0) or when p . A p <= 0; otherwise step = rs / (p . A p),
 *   f += step p, r -= step A p, rs' = r . r, p = r + (rs' / rs) p.  (S p)[i] is summed in slot order; a dot product per thread
 *   in row order, then by xor shuffles in the wave, then over the waves in order: the bits of a query do not depend on the
 *   batch.  One workgroup per query with mi355_diffusion_lds_bytes(L, kd) of LDS (0 for a shape outside 1 <= L <= 1024,
 *   1 <= kd <= 32; at most 160 KiB).  f [Q][L]; iterations [Q] int32 (the iterations done) or NULL; 1 <= iters <= 64; alpha a
 *   finite float in (0, 1); Q = 0 does nothing. */
#define MI355_DIFFUSION_MAX_KD 32
int mi355_diffusion_graph(const int64_t* nn, const float* nv, int64_t G, int kd, int gamma, int32_t* cols, float* vals, float* deg,
                          void* stream);
int mi355_diffusion_source(const float* shortlist_vals, const int64_t* shortlist_idx, int64_t Q, int L, int kq, int gamma, float* y,
                           void* stream);
size_t mi355_diffusion_lds_bytes(int L, int kd);
int mi355_diffusion_solve(const int32_t* cols, const float* vals, int64_t G, int kd, const int64_t* shortlist_idx, const float* y,
                          int64_t Q, int L, float alpha, int iters, float* f, int32_t* iterations, void* stream);

/* Feature-map aggregation: how a backbone's last map becomes the descriptor (csrc/aggregate.hip).  SPoC / MAC / R-MAC (Tolias et
 * al., ICLR 2016), GeM (Radenovic et al., TPAMI 2018) and CroW (Kalantidis et al., ECCV 2016).  fm is [B][C][H][W] fp32,
 * contiguous, 4-byte aligned (a channel row of H*W floats need not be 16-byte aligned: the map is loaded as the flat array it is
 * and handed to its channels through LDS).  1 <= H, W <= 64, C >= 1.  All arithmetic is fp32; every sum has a fixed order that
 * depends on (C, H, W, the regions) alone, never on B or on where an image stands in the batch; no floating-point atomics.  Every
 * argument is checked before any HIP call.  B = 0 does nothing.
 *
 * mi355_aggregate_regions: `regions` is a HOST array [R][4] of (y0, x0, h, w), h, w >= 1, inside the map, 1 <= R <= 64 (it
 *   travels in the kernel arguments).  For image b, region r, channel c, over the region's values x:
 *     MI355_AGG_MEAN: the sum divided by h*w;   MI355_AGG_MAX: the maximum, exact;
 *     MI355_AGG_GEM:  t = max(x, eps_clamp), m = max t, g = m * (mean((t/m)^pc))^(1/pc) - no power of a value above 1 is ever
 *       taken, so large activations and pc = 64 stay finite.  pc = p_channels[c] (DEVICE [C], clamped to [2^-10, 64] where it is
 *       read) or, with p_channels NULL, the scalar p, 0 < p <= 64.  eps_clamp > 0.
 *   Then, if normalize: v[b][r][:] /= max(|v[b][r][:]|_2, eps).  return_regions != 0: out [B][R][C] holds these vectors.  Otherwise
 *   out [B][C] = sum_r v[b][r][:] in the order r = 0 .. R-1, divided again by max(its norm, eps) when normalize.
 *   Two launches: one reads the map once - an image is split over workgroups by channel slab, every region of a channel is pooled
 *   from the slab's copy in LDS - and leaves the pooled values and one partial sum of squares per (b, r, slab) in the workspace;
 *   a small second one adds the partial sums in slab order, normalises, sums the regions and normalises again.
 * mi355_aggregate_crow (alpha = beta = 2): X' = max(X, 0); S[h][w] = sum_c X'[c][h][w]; St = sqrt(S / sqrt(sum_hw S^2)), 0 when
 *   that sum is 0; F[c] = sum_hw St[h][w] X'[c][h][w]; Q[c] = the share of positions with X[c] > 0; I[c] = log(sum_c' Q[c'] / Q[c])
 *   for Q[c] > 0, else 0; out [B][C] = I * F, divided by max(its norm, eps) when normalize.  Four launches, two reads of the map.
 * mi355_aggregate_sum: the second launch of mi355_aggregate_regions alone, for vectors a caller has transformed in between (the
 *   R-MAC regional whitening): out [B][D] = sum_r vecs[b][r][:] (vecs [B][R][D]) in region order, normalised when normalize.
 * mi355_aggregate_workspace_bytes(B, C, R): what either entry needs (mi355_aggregate_crow: with any R); 0 for B = 0 or a
 *   shape outside the limits. */
#define MI355_AGG_MEAN 0
#define MI355_AGG_MAX 1
#define MI355_AGG_GEM 2
#define MI355_AGG_MAX_SIDE 64
#define MI355_AGG_MAX_REGIONS 64
size_t mi355_aggregate_workspace_bytes(int64_t B, int C, int R);
int mi355_aggregate_regions(const float* fm, int64_t B, int C, int H, int W, const int32_t* regions, int R, int pool, float p,
                            const float* p_channels, float eps_clamp, int normalize, int return_regions, float eps, float* out,
                            void* workspace, size_t workspace_bytes, void* stream);
int mi355_aggregate_crow(const float* fm, int64_t B, int C, int H, int W, int normalize, float eps, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);
int mi355_aggregate_sum(const float* vecs, int64_t B, int R, int D, int normalize, float eps, float* out, void* stream);

/* Regional MaxSim re-ranking (csrc/regional.hip): a query image of Rq regional vectors against candidate images of R regional
 * vectors each (Razavian et al. 2016; Tolias et al., ICLR 2016, section 5; the "late interaction" of ColBERT).  Both sides are the
 * fp16 codes of mi355_gallery_to_f16, one row per region: qcodes [Q][Rq][ld], gcodes [rows][R][ld], ld = dim rounded up to a
 * multiple of 64 with zeros behind dim, 16-byte aligned.  1 <= Rq, R <= MI355_REGION_MAX_REGIONS, 1 <= dim <= 65536.  For query q
 * and the row in slot p of its list:
 *     s[i][j] = sum_d float(qcodes[q][i][d]) * float(gcodes[row][j][d])   (fp32 accumulation on v_mfma_f32_16x16x32_f16, the
 *               k-steps in ascending d; every product of two fp16 values is exact in fp32)
 *     m[i] = max_j s[i][j] over the R regions of the row, a[i] = the lowest j that attains it
 *     out_scores[q][p] = sum_i w[i] * m[i], in fp32 in ascending i;  out_matches[q][p][i] = a[i]
 *   w = weights[q] ([Q][Rq] fp32) or, with weights NULL, fp32(1) / fp32(Rq) for every i.  Rq and R are padded to the 16-row tile
 *   inside the kernel: a pad region of the row never reaches the maximum and a pad region of the query adds nothing to the sum.
 *   The bits of a pair depend on the query's codes, its weights and the row alone - not on Q, L, the slot, the other rows of the
 *   list or whether idx was given.
 * idx [Q][L] int64 LOCAL rows, 1 <= L <= 1024; a row may occur twice; a slot outside [0, rows) - the pad -1 or any other value -
 *   is treated as a pad: no row is read, out_scores = -inf and out_matches = -1.  idx NULL: slot p is row p and L must be rows.
 * out_scores [Q][L] fp32; out_matches [Q][L][Rq] int32 or NULL.  One workgroup per (query, slice of the list) keeps the query's
 *   codes in mi355_region_scores_lds_bytes(Rq, dim) of LDS (0 for a shape outside the limits; at most 64 KiB): all of them where
 *   they fit, otherwise one chunk of d at a time with the accumulators in registers.  A candidate's codes are read once.  Every
 *   argument is checked before any HIP call; no atomics; no host sync; Q = 0 does nothing. */
#define MI355_REGION_MAX_REGIONS 64
size_t mi355_region_scores_lds_bytes(int Rq, int dim);
int mi355_region_scores(const void* qcodes, int64_t Q, int Rq, const void* gcodes, int64_t rows, int R, int dim, int ld,
                        const int64_t* idx, int64_t L, const float* weights, float* out_scores, int32_t* out_matches, void* stream);

/* Result diversification (csrc/diversify.hip): maximal marginal relevance (Carbonell and Goldstein, SIGIR 1998) and greedy
 * near-duplicate suppression over a query's shortlist, in two stages.  Every argument is checked before any HIP call; no atomics;
 * no host sync; Q = 0 does nothing.
 *
 * mi355_shortlist_gram: out[q][p][r] = the dot product of gallery rows idx[q][p] and idx[q][r] (idx [Q][L] int64 LOCAL rows,
 *   1 <= L <= MI355_DIVERSIFY_MAX_SHORTLIST; out [Q][L][L] fp32).  rows / rows_dtype / ld / G as in mi355_rescore_candidates: fp32
 *   rows (4-byte aligned, any ld >= dim) or fp16 rows (16-byte aligned, ld a multiple of 8), normalised by the caller; 1 <= dim <=
 *   65536.  The operands are the rows' fp16 values - an fp16 row as it lies, an fp32 element rounded to fp16 (round-to-nearest-even)
 *   on load - columns at or past dim are zero, and the sum is fp32 on v_mfma_f32_16x16x32_f16 with the k-steps in ascending column
 *   order (every product of two fp16 values is exact in fp32).  An entry is 0 where either slot is a pad: -1, or any index outside
 *   [0, G).  The diagonal is computed like any other entry.  An entry's bits depend on the unordered pair of rows alone - not on
 *   L, the slot, the tile, the query or Q - and out[q] is bit-symmetric: only entries at or above the diagonal are computed, each
 *   stored together with its mirror.  One workgroup per (query, pair of 64-slot tiles at or above the diagonal).
 * mi355_mmr_select: greedy selection of k of the L slots of every query, entirely in fp32 without fused multiply-add.  rel / idx
 *   [Q][L] are a search's output (idx < 0: a pad), gram [Q][L][L] that of mi355_shortlist_gram.  oml = fp32(1) - lam; m[p] = 0 and
 *   nothing picked at the start.  For pick t = 0 .. k-1: slot p is eligible if it holds a row, is unpicked and, unless
 *   dedup_or_nan is NaN, m[p] < dedup_or_nan; its value is v[p] = fp32(lam * rel[p]) - fp32(oml * m[p]), a NaN value counting as
 *   -inf; the pick j is the eligible slot of greatest value, ties to the lower position; then m[p] = gram[q][j][p] wherever that
 *   is greater than m[p].  out_val[q][t] = rel[j] (the cosine score: not monotone in t), out_idx[q][t] = idx[q][j] + idx_offset,
 *   out_mmr[q][t] = v[j] (or NULL).  When no slot is eligible the remaining outputs are (-inf, -1, -inf); out_count[q] (or NULL)
 *   is the number of picks.  1 <= k <= L <= MI355_DIVERSIFY_MAX_SHORTLIST; lam a finite float in [0, 1]; dedup_or_nan finite or
 *   NaN.  lam = 1 without a threshold returns the first k slots that hold a row.  One workgroup of L threads (rounded up to
 *   whole waves) per query: a slot's rel and m stay in registers. */
#define MI355_DIVERSIFY_MAX_SHORTLIST 1024
int mi355_shortlist_gram(const void* rows, int rows_dtype, int64_t ld, int64_t G, int dim, const int64_t* idx, int64_t Q, int L,
                         float* out, void* stream);
int mi355_mmr_select(const float* rel, const int64_t* idx, const float* gram, int64_t Q, int L, int k, float lam, float dedup_or_nan,
                     int64_t idx_offset, float* out_val, int64_t* out_idx, float* out_mmr, int32_t* out_count, void* stream);

/* PCA whitening, the fit's hot path: first and second raw moments of embedding rows in float64.
 *   sum[i]      = sum_r x[r][i]                 (device double [dim])
 *   outer[i][j] = sum_r x[r][i] * x[r][j]       (device double [dim][dim], row-major)
 * x[r] = row r (fp32, or fp16 in the mi355_gallery_to_f16 layout; rows ld >= dim elements apart) or, with normalize_rows (fp32
 * rows only), l2_normalize_rows(row, eps) with the bits of mi355_l2_normalize_rows.  Elements are widened to float64 (exact),
 * their products are exact in float64, the sums are float64 (v_mfma_f64_16x16x4_f64): the only rounding is the accumulation.
 * Only tiles on or above the diagonal are computed and every element is written together with its mirror: outer is exactly
 * symmetric.  accumulate != 0 adds to what sum / outer hold (a streaming fit), otherwise they are overwritten.
 * Determinism: the rows are split over workgroups by a rule of (R, dim) alone, the partial tiles are added from the workspace in
 * split order and there are no floating-point atomics - the same call sequence gives the same bits on every run.
 * Any 1 <= dim <= 16384, any R >= 0 (R = 0: nothing with accumulate, zeros without; rows may then be NULL).  NaN / Inf propagate.
 * workspace: mi355_moments_workspace_bytes(R, dim) (0 for R = 0), 16-byte aligned.  Every argument is checked before any HIP call. */
size_t mi355_moments_workspace_bytes(int64_t R, int dim);
int mi355_embedding_moments(const void* rows, int rows_dtype, int64_t R, int64_t ld, int dim, int normalize_rows, float eps,
                            int accumulate, double* sum, double* outer, void* workspace, size_t workspace_bytes, void* stream);

/* PCA whitening, the transform: normalise -> project -> bias -> normalise in one launch.
 *   x'   = row r of x as it is (fp32, or fp16 gallery rows widened exactly), or with normalize_input (fp32 only)
 *          l2_normalize_rows(x_r, eps) with the bits of mi355_l2_normalize_rows
 *   y[j] = bias[j] + sum_i matrix[j][i] * x'[i]: an fp32 fmaf chain that starts from bias[j] and takes i in one fixed order
 *          (per 8 inputs: 0, 4, 1, 5, 2, 6, 3, 7; v_mfma_f32_32x32x2_f32) that depends neither on R nor on the row's position
 *   out  = y (normalize_output = 0, MI355_DTYPE_F32), l2_normalize_rows(y, eps) bit for bit (MI355_DTYPE_F32), or fp16 of that
 *          as mi355_gallery_to_f16 stores it, elements dim_out .. out_ld-1 zeroed (MI355_DTYPE_F16; needs normalize_output).
 * matrix [dim_out][dim_in] and bias [dim_out] are device fp32, 1 <= dim_out <= dim_in.  A row's output depends only on that
 * row, the matrix and the bias.  Rows are x_ld / out_ld elements apart; with normalize_output and dim_out % 4 == 0, out is
 * 16-byte aligned and out_ld % 4 == 0.  workspace: mi355_whiten_workspace_bytes(R, dim_in, dim_out, out_dtype) (fp16 output:
 * R * dim_out fp32; fp32 output: none, may be NULL).  Every argument is checked before any HIP call; R = 0 does nothing. */
size_t mi355_whiten_workspace_bytes(int64_t R, int dim_in, int dim_out, int out_dtype);
int mi355_whiten_rows(const void* x, int x_dtype, int64_t R, int64_t x_ld, int dim_in, int normalize_input, float eps,
                      const float* matrix, const float* bias, int dim_out, int normalize_output, void* out, int out_dtype,
                      int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream);

/* Indices outside [lo, hi) become (-inf, -1) in val / idx [n] (the sharded filtered search: slots no shard filled). */
int mi355_clear_pads(float* val, int64_t* idx, int64_t n, int64_t lo, int64_t hi, void* stream);

/* Retrieval accuracy of ranked lists (Musgrave et al. 2020, "A Metric Learning Reality Check"): idx [Q][k] ranked gallery rows
 * (indices outside [0, G) are misses), query_cls [Q], gallery_cls [G], R [Q] the number of relevant gallery rows of each
 * query (R <= k; ranks past k count as misses).  One wave per query writes per_query[Q][3] float64:
 *   [0] the first rank (0-based) holding a row of the query's class, k if none (precision@1: [0] == 0; recall@K: [0] < K),
 *   [1] R-precision  (1/R) sum_{i<R} rel(i),
 *   [2] MAP@R        (1/R) sum_{i<R} rel(i) * P(i),  P(i) = (1/(i+1)) sum_{j<=i} rel(j);
 * queries with R <= 0 get [k, 0, 0]. */
int mi355_retrieval_metrics(const int64_t* idx, int64_t Q, int k, const int64_t* query_cls, const int64_t* gallery_cls,
                            int64_t G, const int64_t* R, double* per_query, void* stream);

/* Row-wise top-k of an explicit score matrix scores[Q][G] (torch.topk, train/train.py:251).
 * workspace: mi355_rank_workspace_bytes(Q, G, 0, k). */
int mi355_topk_rows(const float* scores, int64_t Q, int64_t G, int k, int64_t idx_offset,
                    float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Merge per-shard candidates: cand_val/cand_idx [Q][ncand] (ncand = shards*k, any
 * order) -> global top-k with the same ordering rule.  Used after the RCCL all-gather.
 * The indices of a row's candidates are distinct.  An index >= 2^62 marks "no candidate" (INT64_MAX, what the selection
 * itself leaves in an empty slot, and the shard pad 1 << 62): its value is ignored, it never takes a slot while a
 * candidate is left, and with fewer than k candidates the remaining slots are (-inf, INT64_MAX).  A candidate whose value is
 * -inf is a candidate and comes before every empty slot.  Values come out with the bits they went in with. */
int mi355_merge_topk(const float* cand_val, const int64_t* cand_idx, int64_t Q, int ncand, int k,
                     float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Sharded search (no reference counterpart: inference/inference.py:271 is single-device).  One int32 tensor
 * per rank goes through the candidate all-gather: packed[q][j] = {bits of the f32 score, LOCAL row index}, slots
 * j >= kk (a shard with fewer than k rows) = {-inf, -1}.  val / idx: (Q, kk) results of mi355_rank_topk on the shard. */
int mi355_pack_candidates(const float* val, const int64_t* idx, int64_t Q, int kk, int k, int32_t* packed, void* stream);
/* Merge of the all-gathered lists packed[world][Q][k][2]: adds shard_offsets[r] (device int64[world]) to rank r's local
 * indices and selects the k best of the world * k candidates of every query (higher score, then lower global index):
 * (Q, k) values + int64 global indices, identical to ranking against the unsharded gallery.  A slot with a negative local
 * index is no candidate; when the shards hold fewer than k candidates for a query the remaining slots are (-inf, INT64_MAX),
 * as in mi355_merge_topk (mi355_clear_pads over [0, total rows) turns them into the (-inf, -1) of a filtered search). */
size_t mi355_merge_packed_workspace_bytes(int64_t Q, int world, int k);
int mi355_merge_packed_topk(const int32_t* packed, const int64_t* shard_offsets, int world, int64_t Q, int k,
                            float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* Row-wise pair cosine, inference/inference.py:226,229: out[i] = cos(a[i], b[i]). */
int mi355_pair_cosine(const float* a, const float* b, int64_t rows, int dim, float eps, float* out,
                      void* stream);

/* utils/contrastive_loss.py:36-61 ContrastiveLoss.forward(fm1, fm2, label, mean):
 *   dis = sum_d (fm2-fm1)^2 ; 0.5*(label*dis + (1-label)*relu(margin - sqrt(dis+1e-9))^2) ;
 *   out[0] = mean or sum over rows (deterministic order).  per_row (optional, may be NULL) gets
 *   the per-row losses. */
int mi355_contrastive_loss(const float* fm1, const float* fm2, int64_t rows, int dim, float label,
                           float margin, int mean, float* out, float* per_row, void* stream);

/* torch.nn.CosineEmbeddingLoss(margin)(x1, x2, target) with a scalar target of +1 or -1 broadcast over the rows —
 * the validation-step loss of train/train.py:214-216, :308-310.  out[0] = mean (or sum). */
int mi355_cosine_embedding_loss(const float* x1, const float* x2, int64_t rows, int dim, float target, float margin,
                                int mean, float* out, void* stream);

/* Hit counting, train/train.py:252-255: counts[0] += #queries whose class equals the class of
 * their top-1 result, counts[1] += #queries whose class is among their top-min(3,k).
 * idx [Q][k] int64 into gallery_cls [G]; counts int64[2] must be zeroed by the caller.  An index outside [0, G)
 * (the pad entry of a list with fewer than k real candidates) counts as a miss. */
int mi355_hit_counts(const int64_t* idx, int64_t Q, int k, const int64_t* query_cls,
                     const int64_t* gallery_cls, int64_t G, int64_t* counts, void* stream);

/* Notebook variant, inference/training_analysis.ipynb raw :240-251: walk each ranked list and keep
 * the first n (<= 8) DISTINCT classes.  out_cls/out_idx [Q][n] int64 (-1 padded), out_val [Q][n].
 * gallery_cls [G]; indices outside [0, G) are skipped. */
int mi355_distinct_class_topn(const int64_t* idx, const float* val, int64_t Q, int k,
                              const int64_t* gallery_cls, int64_t G, int n, int64_t* out_cls, int64_t* out_idx,
                              float* out_val, void* stream);

/* ------------------------------------------------------------------ spherical k-means and clustering scores
 * Nearest centroid: assign[n] = the centroid (row of centroids [K][dim], device fp32, normalised by the call as the queries of
 * every search are) with the highest cosine to resident row n, score[n] that cosine (device int64 [N] / fp32 [N]).  Equal
 * scores go to the lower centroid.  The rows are the gallery side of the tiled cosine GEMM: fp32 rows [N][dim]
 * (rows_are_normalized as in mi355_rank_topk) or the fp16 rows of mi355_gallery_to_f16; every score has the bits of
 * mi355_cosine_scores(centroids, rows) on the same loop.  The centroids go through the GEMM mi355_roc_pairs_hist's query
 * block at a time, or query_block (> 0, smaller) at a time; the result does not depend on it, nor on the launch order.
 * N < 2^31 - 128.  Every argument is checked before any HIP call. */
size_t mi355_nearest_centroid_workspace_bytes(int64_t K, int64_t N, int dim);
int mi355_nearest_centroid(const float* centroids, int64_t K, const float* rows, int64_t N, int dim, int rows_are_normalized, float eps,
                           int64_t query_block, int64_t* assign, float* score, void* workspace, size_t workspace_bytes,
                           void* stream);
size_t mi355_nearest_centroid_f16_workspace_bytes(int64_t K, int64_t N, int dim);
int mi355_nearest_centroid_f16(const float* centroids, int64_t K, const void* rows_f16, int64_t N, int dim, float eps,
                               int64_t query_block, int64_t* assign, float* score, void* workspace, size_t workspace_bytes,
                               void* stream);

/* The members of every cluster as CSR: assign [N] device int64 in [0, K) -> offsets [K + 1] and order [N] (device int64), the
 * rows of cluster k at order[offsets[k] .. offsets[k + 1]) in ascending row index.  A value outside [0, K) is found on the
 * device and reported as an argument error (the call reads one flag word back: one host sync); nothing is read or written
 * out of bounds because of it.  K < 2^24 (one workgroup per cluster). */
size_t mi355_cluster_members_workspace_bytes(int64_t N, int64_t K);
int mi355_cluster_members(const int64_t* assign, int64_t N, int64_t K, int64_t* offsets, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Centroid update of spherical k-means: mi355_cluster_members of assign (offsets / order come out as there), then per
 * cluster the float64 sum of its member rows (fp32 rows [N][dim], or the fp16 rows of mi355_gallery_to_f16 widened exactly)
 * in ascending row order - 256 members at a time, the partial sums then in segment order - and
 * centroids[k] = fp32(sum / |sum|), one rounding.  A cluster without members, or with |sum| < eps, keeps previous[k] bit for
 * bit.  centroids / previous [K][dim] device fp32 (they may be the same buffer), counts [K] device int64.  The same bits on
 * every run and every device.  K < 2^24 and ceil(N / 256) + K < 2^24 (one workgroup per segment).  The two sizers return
 * the same number: the partial sums are float64 for either kind of rows. */
size_t mi355_centroid_update_workspace_bytes(int64_t N, int64_t K, int dim);
int mi355_centroid_update(const float* rows, int64_t N, int dim, const int64_t* assign, int64_t K, const float* previous, float eps,
                          float* centroids, int64_t* counts, int64_t* offsets, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t mi355_centroid_update_f16_workspace_bytes(int64_t N, int64_t K, int dim);
int mi355_centroid_update_f16(const void* rows_f16, int64_t N, int dim, const int64_t* assign, int64_t K, const float* previous,
                              float eps, float* centroids, int64_t* counts, int64_t* offsets, int64_t* order, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Contingency table of two labelings: table[x * Kb + y] = #{i : a[i] == x and b[i] == y}, a / b [N] device int64 in [0, Ka) /
 * [0, Kb), table [Ka][Kb] device int64 (zeroed by the call), N <= 2^40, Ka * Kb <= 2^28.  Exact integer counts (per-workgroup LDS
 * sub-histograms up to 8192 cells, global integer atomics above).  An id out of range is an argument error found on the
 * device (one flag word read back). */
size_t mi355_contingency_workspace_bytes(int64_t N, int64_t Ka, int64_t Kb);
int mi355_contingency(const int64_t* a, const int64_t* b, int64_t N, int64_t Ka, int64_t Kb, int64_t* table, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ DBSCAN and threshold components
 * Clustering without a number of clusters, inside the tiled cosine GEMM: the self-join of N resident rows (fp32 rows [N][dim],
 * gallery_is_normalized as in mi355_rank_topk, or the fp16 rows of mi355_gallery_to_f16) is swept twice, a block of rows at a
 * time as the GEMM's queries; no pair list is ever made.  hit(i, j): the score of query row i against row j (the bits and the
 * comparison of mi355_cosine_range: fp32 score >= the fp32 ceiling of threshold, NaN never, j == i included).
 *   state (device, N entries each): degree int32, parent int32, border uint64.  mi355_dbscan_init: degree = 0, border = 0,
 *     parent[i] = i.
 *   mi355_dbscan_degree[_f16]: queries [rows][dim] device fp32 = rows [q0, q0 + rows) of the same data (normalised by the call
 *     as the queries of every search are); degree[q0 + r] += the hits of query r.  Call it once per block until every row
 *     has been a query; only then start the link sweeps.
 *   mi355_dbscan_link[_f16]: the same sweep again.  Row i is core when degree[i] >= min_samples.  For a hit (i, j), i != j:
 *     both core: their components are joined in parent[] (lock-free union-find, the larger root under the smaller: a finished
 *     component's root is its smallest row); exactly one core: border[the other row] = max(border, score_key(score) << 32 |
 *     ~core row): the highest score wins, equal scores go to the lower core row.
 *   mi355_dbscan_finish: root[i] (device int64) = the smallest core row of row i's cluster - a core row's component, a
 *     non-core row's chosen core row's - or -1 (noise: a non-core row no core row hit or was hit by); core[i] (device uint8).
 * With min_samples = 1 every row is core and root[] is the connected components of the threshold graph.  Every output is the
 * same for any block size, launch order and run.  N < 2^31 - 128.  Every argument is checked before any HIP call; the work
 * is enqueued on the given stream and nothing synchronises. */
size_t mi355_dbscan_workspace_bytes(int64_t rows, int64_t N, int dim);
size_t mi355_dbscan_f16_workspace_bytes(int64_t rows, int64_t N, int dim);
int mi355_dbscan_init(int64_t N, int32_t* degree, int32_t* parent, uint64_t* border, void* stream);
int mi355_dbscan_degree(const float* queries, int64_t q0, int64_t rows, const float* gallery, int64_t N, int dim,
                        int gallery_is_normalized, float eps, double threshold, int32_t* degree, void* workspace,
                        size_t workspace_bytes, void* stream);
int mi355_dbscan_degree_f16(const float* queries, int64_t q0, int64_t rows, const void* gallery_f16, int64_t N, int dim, float eps,
                            double threshold, int32_t* degree, void* workspace, size_t workspace_bytes, void* stream);
int mi355_dbscan_link(const float* queries, int64_t q0, int64_t rows, const float* gallery, int64_t N, int dim,
                      int gallery_is_normalized, float eps, double threshold, int min_samples, const int32_t* degree,
                      int32_t* parent, uint64_t* border, void* workspace, size_t workspace_bytes, void* stream);
int mi355_dbscan_link_f16(const float* queries, int64_t q0, int64_t rows, const void* gallery_f16, int64_t N, int dim, float eps,
                          double threshold, int min_samples, const int32_t* degree, int32_t* parent, uint64_t* border,
                          void* workspace, size_t workspace_bytes, void* stream);
int mi355_dbscan_finish(int64_t N, int min_samples, const int32_t* degree, const int32_t* parent, const uint64_t* border,
                        int64_t* root, uint8_t* core, void* stream);

/* ------------------------------------------------------------------ inverted-file (IVF) search
 * The scan of the lists a query probes.  The gallery's rows stay where they lie and are read through the lists' CSR
 * (offsets [nlist + 1], order [G], device int64: the rows of list l are order[offsets[l] .. offsets[l + 1]), as
 * mi355_cluster_members writes them); no list-ordered copy is made.
 *   queries [Q][dim] device fp32, raw: normalised by the call with the bits of mi355_l2_normalize_rows(queries, eps);
 *   rows: MI355_DTYPE_F32 normalised rows, ld floats apart (ld >= dim), or MI355_DTYPE_F16 rows in the mi355_gallery_to_f16
 *     layout (16-byte aligned, ld a multiple of 8 halves, ld >= dim, the padding zero); G rows;
 *   probes [Q][nprobe] device int64 list ids, those of one query distinct; 1 <= nprobe <= nlist;
 *   cand_val [Q][cap] device fp32, cand_idx [Q][cap] device int64: cap candidate slots per query;
 *   filter: NULL, or the eligibility rule of the filtered searches (exclude compared with row + idx_offset).
 * For query q the rows of probes[q][0], then probes[q][1], ... fill slots 0 .. n_q - 1 in list order, each with
 * (qn . row, order[r] + idx_offset); the slot of an ineligible row, and every slot n_q .. cap - 1, holds (-inf, 2^62), the
 * "no candidate" of mi355_merge_topk, which selects the k best of the slab.  Every slot is written once, by one wave; there
 * are no atomics.
 * Arithmetic: one wave per row, fp32 accumulation, fp16 rows widened exactly.  Lane i takes the elements [4u, 4u + 4) (fp16
 * rows: [8u, 8u + 8)) of the units u = i, i + 64, ... in ascending order, one fused multiply-add each, then the 64 partial
 * sums go through the library's wave reduction: the order depends on dim alone.  A score therefore depends on its query row
 * and its gallery row only - not on Q, nprobe, the list, how queries are grouped, or the query block of the caller.
 * Work: the (query, list) pairs are grouped by list (the kernels of mi355_cluster_members over the flattened probes), each
 * list's pairs are cut into groups of up to 4 queries held in LDS (fewer when 4 rows of dim floats pass 64 KB; one must fit)
 * and its rows into chunks of 64; a small kernel writes the (list, group, chunk) items and their count to device memory and
 * the scan loops over them on a fixed grid sized by the device's CUs.  Slot bases are running sums taken on the device.
 * Nothing is read back between these steps.
 * Errors found on the device are reported after the call from one flag word (one host sync at the end, as in
 * mi355_cluster_members): n_q > cap for some query; a list id outside [0, nlist), an order entry outside [0, G) or offsets
 * that do not ascend within [0, G].  Such an entry is skipped (a bad order entry's slot holds "no candidate") and nothing
 * is read or written out of bounds because of it.  Q = 0 does nothing.  Q * nprobe < 2^31, Q * cap < 2^40, nlist < 2^24.
 * Every argument is checked before any HIP call. */
size_t mi355_ivf_scan_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int64_t cap);
int mi355_ivf_scan(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld, int64_t G,
                   const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe, int64_t cap,
                   int64_t idx_offset, const mi355_rank_filter* filter, float* cand_val, int64_t* cand_idx, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The same scan over the rows of an int8 gallery (mi355_ivf_scan_i8): a quarter of the bytes of fp32 rows per probed row.
 *   codes / scales: the pair mi355_gallery_to_i8 writes - codes 16-byte aligned, rows ld bytes apart, ld a multiple of 128 and
 *     >= dim, the bytes dim .. (dim rounded up to 128) - 1 of a row zero; scales fp32 [G]; G rows; 1 <= dim <= 65536;
 *   queries, offsets, order, probes, cand_val, cand_idx, filter, idx_offset, cap: exactly as in mi355_ivf_scan, and so is the
 *     slot layout: the lists fill slots 0 .. n_q - 1 in probe order, then list order; an ineligible row and every slot
 *     n_q .. cap - 1 hold (-inf, 2^62); every slot is written once, by one wave, with no atomics.
 * Query planes: (hi, lo, s_q) of the int8 block above, made by the call from qn = the bits of mi355_l2_normalize_rows(queries,
 * eps) (one kernel takes the norm and splits: no normalised copy is written), kept as [Q][hi, lo][dim rounded up to 128] bytes
 * and s_q [Q] in the workspace.
 * Score: acc_hi, acc_lo exact in int32; t = fmaf((float)acc_lo, 0x1p-7f, (float)acc_hi); score = (t * s_q) * s_g - the bits
 * mi355_rank_topk_i8 returns for the pair.  A NaN-scale row scores NaN, a zero row 0, a NaN query NaN everywhere.  A score
 * depends on its query and its row only - not on Q, nprobe, the list, the group or the query block of the caller - so a scan
 * that probes every list, merged by mi355_merge_topk, is mi355_rank_topk_i8 bit for bit.
 * Work: the planning kernels and the loop over the (list, group, chunk) items are mi355_ivf_scan's.  One wave per row, 16 bytes
 * of the row per lane and load, up to four loads in flight; the group's planes in LDS (2 bytes per element and query), so a
 * group is up to 8 queries, fewer when 8 * 2 * ld' bytes pass 64 KB (ld' = dim rounded up to 128); one must fit: dim <= 32768.
 * v_dot4_i32_i8 into int32, an integer wave reduction, lanes < n write the slots.
 * Errors: as in mi355_ivf_scan - every argument is checked before any HIP call (Q = 0 does nothing), what is found on the
 * device is reported after the call from the same two flag words behind one host sync, with the same messages.
 * workspace: mi355_ivf_scan_i8_workspace_bytes(Q, nprobe, nlist, dim, cap), 0 for a shape the scan refuses. */
size_t mi355_ivf_scan_i8_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int64_t cap);
int mi355_ivf_scan_i8(const float* queries, int64_t Q, int dim, float eps, const void* codes, const float* scales, int64_t ld,
                      int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe,
                      int64_t cap, int64_t idx_offset, const mi355_rank_filter* filter, float* cand_val, int64_t* cand_idx,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ product-quantised (PQ) resident gallery
 * A row is M bytes: its normalised fp32 row is cut into M sub-vectors of dsub = dim / M elements, and byte m names the nearest
 * of the 256 centroids of sub-quantiser m.  At dim = 1536, M = 96 that is 96 bytes, a 64th of the fp32 row.
 * Below, "fp32" means one IEEE rounding per named operation; no multiply is fused with an add anywhere in this block.
 * Parameters: M % 4 == 0, 4 <= M <= 128, dim % M == 0, 1 <= dsub <= 64.  codebooks: device fp32 [M][256][dsub].  codes: uint8
 * [G][M], row-major and appendable (encoding n rows to codes + r * M writes rows r .. r+n-1); the base is 16-byte aligned.
 * Encode: n = the fp32 row mi355_l2_normalize_rows writes for x, bit for bit (rows_are_normalized != 0: n = x as it is).  For
 * subspace m and centroid c: d = 0.0f, then for i ascending t = n[m*dsub+i] - cb[m][c][i]; d = d + t*t (the subtraction, the
 * multiply and the add each rounded to fp32).  code[m] = the lowest c whose d is strictly below the d of every earlier c (c = 0
 * to begin with).  A NaN distance never wins: a row with a NaN element gets code 0 in the subspaces the NaN touches.  This is
 * the one place where the format departs from the other galleries' "a NaN row ranks first": a code cannot carry a NaN, so such
 * a row scores like any row with those codes.
 * Table (per query, made by every search): qn = the normalised query (the bits above); T[m][c]: acc = 0.0f, then for i ascending
 * acc = acc + qn[m*dsub+i] * cb[m][c][i], the multiply rounded, then the add rounded.
 * Score of (q, g): four accumulators a_j = 0.0f; for m ascending a_{m%4} = a_{m%4} + T[m][code[g][m]]; score = (a0 + a1) +
 * (a2 + a3).  A NaN query scores NaN everywhere.  A score depends on its query row, its code row and the codebooks only - not on
 * Q, G, the row's position in a chunk of the scan, k, the filter or the path (fused selection, score slab, mi355_pq_scores).
 * Top-k: the selection of mi355_rank_topk (descending, NaN first, ties to the lower row, -0 equal to +0, the slots a filter
 * leaves empty (-inf, -1)).  Equal code rows give equal bits, so ties are the normal case here.
 * The scan: one workgroup per (query, chunk of 2048 rows) holds the query's table in LDS (M KB of the 160 KB).  For k <= 8 it
 * selects inside the kernel (k candidates per (query, chunk), merged by the selection of mi355_merge_topk: MI355_RANK_PATH_PQ |
 * FUSED); for 8 < k <= 1024 it writes the score slab of a block of queries and the selection of mi355_topk_rows follows
 * (| BITONIC).  An ineligible row (filter) never enters the selection.  No atomics: one writer per output slot.
 * Centroid update (training): new[m][c] = fp32(S / count), S = the float64 sum of the sub-vectors m of the normalised rows n
 * whose code[m] is c, added ONE AT A TIME IN ASCENDING ROW ORDER (each fp32 element widened exactly; sum and division in
 * float64, one rounding to fp32 at the end), count = their number.  The order is the rows' order alone: it does not depend on
 * the device, its CU count or the launch geometry.  A cell without members keeps its previous centroid bit for bit.  counts:
 * device int64 [M][256].  codebooks and codebooks_out may be the same buffer.
 * Rescoring (mi355_rescore_candidates): out_val[q][r] = the fp32 dot mi355_ivf_scan gives query q and row cand_idx[q][r] -
 * idx_offset of fp32 or fp16 rows (the same routine: one wave per pair, lane-strided units, fused multiply-adds, the wave
 * reduction), for the re-ranking of a PQ shortlist against the rows it was made from.  cand_idx [Q][R] device int64 is left as
 * it is; a negative index, one >= 2^62, or one whose row falls outside [0, G) scores -inf.
 * Every argument is checked before any HIP call (null pointers, shape, k in [1, min(1024, G)], 16-byte alignment of the codes,
 * codes_bytes, workspace).  R, Q or G equal to 0 does nothing.  Workspaces: the _workspace_bytes entry of the same name;
 * mi355_pq_scores takes mi355_pq_search_workspace_bytes(Q, G, dim, M, 0) (k = 0: no selection).  The sizers return 0 for a shape
 * the entry would reject, and for R = 0 / Q = 0. */
size_t mi355_pq_encode_workspace_bytes(int64_t R, int dim, int rows_are_normalized);
int mi355_pq_encode(const float* rows, int64_t R, int dim, int M, int rows_are_normalized, float eps, const float* codebooks,
                    void* codes, size_t codes_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t mi355_pq_update_workspace_bytes(int64_t R, int dim, int rows_are_normalized);
int mi355_pq_update(const float* rows, int64_t R, int dim, int M, int rows_are_normalized, float eps, const void* codes,
                    const float* codebooks, float* codebooks_out, int64_t* counts, void* workspace, size_t workspace_bytes,
                    void* stream);
size_t mi355_pq_search_workspace_bytes(int64_t Q, int64_t G, int dim, int M, int k);
int mi355_pq_scores(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* codes, int64_t G,
                    float* scores, void* workspace, size_t workspace_bytes, void* stream);
int mi355_pq_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* codes, int64_t G,
                    int k, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t mi355_rescore_candidates_workspace_bytes(int64_t Q, int dim);
int mi355_rescore_candidates(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld,
                             int64_t G, const int64_t* cand_idx, int64_t R, int64_t idx_offset, float* out_val, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ IVF-PQ search: the probed lists of a PQ gallery's codes
 * The table scan of the PQ block over the rows of the lists a query probes only.  It indexes the codes a PQ gallery already
 * holds (no residual coding): codebooks, M, dim as in the PQ block; offsets [nlist + 1], order [G] device int64 as in the IVF
 * block; probes [Q][nprobe] device int64 list ids, those of one query distinct, 1 <= nprobe <= min(nlist, 1024).
 * Layout: list_codes uint8 [G][M] is the list-ordered copy of the codes, list_codes[p] = codes[order[p]], base 16-byte aligned:
 * list l is the contiguous byte range [offsets[l] * M, offsets[l + 1] * M), and the scan's 16-byte (M % 16 == 0) or 4-byte code
 * loads are those of the exhaustive scan.
 * Score of (q, row): exactly the PQ score above - the table T[m][c] of the normalised query, four accumulators in order m % 4,
 * then (a0 + a1) + (a2 + a3) - bit for bit.  It depends on the query row, the code row and the codebooks only: not on the list,
 * nprobe, Q, cap, the chunk of the scan, k, the filter or the path.  A search that probes every list therefore returns the
 * values and indices of mi355_pq_search over the same codes, bit for bit.
 * Selection: that of mi355_rank_topk (descending, NaN first, ties to the lower GALLERY ROW, -0 equal to +0).  The scan visits
 * rows in list order, so the tie rule is applied on order[p] + idx_offset, never on the scan position.  The slots that the
 * probed lists or a filter leave empty hold (-inf, -1).
 * filter: NULL, or the eligibility rule of the filtered searches; labels are looked up by gallery row order[p], exclude is
 * compared with order[p] + idx_offset.  Returned indices are order[p] + idx_offset.
 * cap: an upper bound on the rows any one query probes (the host knows it from the list lengths); cap >= k.  Per block of 256
 * queries: their tables, then per query the running sums base[0 .. nprobe] of its probed lists' lengths (n_q = base[nprobe]),
 * then a grid of (cdiv(cap, 2048), queries) workgroups: workgroup (c, q) owns positions [2048 c, min(2048 (c + 1), n_q)) of
 * query q's concatenated lists, finds the list of a position in base[] (held in LDS beside the table: M KB + 8 (nprobe + 1)
 * bytes) and returns at once, with empty candidates, when 2048 c >= n_q.  For k <= 8 it selects inside the kernel (k candidates
 * per (query, chunk), merged by the selection of mi355_merge_topk); for 8 < k <= 1024 it writes a (queries, cap) slab of
 * (value, index) candidates with (-inf, 2^62) from n_q on and the selection of mi355_merge_topk follows; the query block
 * shrinks so that the slab stays under 512 MB.  No atomics: one writer per output slot.  The result does not depend on the
 * chunk length.
 * Errors found on the device are reported after the call from one flag read-back (one host sync at the end, as in
 * mi355_ivf_scan): n_q > cap for some query; a list id outside [0, nlist), an order entry outside [0, G) or offsets that do not
 * ascend within [0, G].  Such an entry is skipped and nothing is read or written out of bounds because of it.
 * Every argument is checked before any HIP call: null pointers, the PQ shape rules, 16-byte alignment of list_codes, G >= 1,
 * 1 <= nprobe <= min(nlist, 1024), nlist < 2^24, k in [1, min(1024, cap)], Q * nprobe < 2^31, Q * cap <= 2^40, the filter, the
 * workspace.  Q = 0 does nothing.  The sizer returns 0 for a shape the entry would reject, and for Q = 0. */
size_t mi355_ivfpq_search_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int M, int64_t cap, int k);
int mi355_ivfpq_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* list_codes,
                       int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe,
                       int64_t cap, int k, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ residual IVF-PQ: codes of row - centroid(list)
 * The IVF-PQ search above over codes that describe a row's offset from the centroid of its list, so that the lists pay for
 * accuracy as well as for time.  Bit for bit, with "fp32" as in the PQ block:
 * Normalisation: rn = the row mi355_l2_normalize_rows writes, as everywhere.
 * List: l = the row's list - the nearest of the unit centroids [nlist][dim] (mi355_nearest_centroid), or the caller's choice.
 * Residual: e[i] = rn[i] - centroids[l][i], one fp32 subtraction per element (mi355_ivfpq_residuals).
 * Codes and codebooks: the PQ contract applied unchanged to the rows e - mi355_pq_encode / mi355_pq_update with
 * rows_are_normalized = 1, so that nothing is normalised again; training is the same Lloyd loop over residual rows.
 * Score of (q, g): coarse(q, l_g) + s(q, g), one fp32 addition.  s is the PQ score of g's code row against the table of the
 * normalised query - (a0 + a1) + (a2 + a3), the table built from the residual codebooks: one table per query, since q . e does
 * not depend on the list.  coarse(q, l) = the fp32 dot of the normalised query with centroids[l] with the bits
 * mi355_rescore_candidates gives that pair over the centroids as rows (the same routine: one wave per pair, lane-strided
 * units, fused multiply-adds, the wave reduction).  A row lies in one list, so its score depends on the query and the row
 * alone: not on nprobe, the order of the probes, Q, cap, k, the path or the filter.
 * Selection, filter, cap, probes, flags, limits and argument checks: those of mi355_ivfpq_search (ties to the lower GALLERY
 * ROW, pads (-inf, -1), a bad list id counts as an empty list - its coarse term is never read - and raises the flag).
 * mi355_ivfpq_residual_search: mi355_ivfpq_search's arguments and centroids [nlist][dim] device fp32 (unit rows, dense).  Per
 * query block a launch of one wave per (query, probed list) writes coarse[q][j] into the workspace; the scan stages the
 * query's nprobe terms in LDS behind base[] (4 nprobe bytes more: 143,368 bytes at M = 128, nprobe = 1024) and adds the
 * term of the list the position lies in to the position's lookups.  Its sizer asks for those terms on top of the plain one's
 * bytes.
 * mi355_ivfpq_residuals: rows [R][dim] device fp32 (raw, or rn itself with rows_are_normalized != 0), assignments [R] device
 * int64 -> residuals [R][dim] device fp32 (may be rows itself), one vectorised pass.  R <= 2^31, dim <= 8192, nlist < 2^24.
 * An assignment outside [0, nlist) is found on the device (its row is left unwritten) and reported as an argument error from
 * one flag word read back (one host sync).  workspace: MI355_IVFPQ_RESIDUALS_WORKSPACE bytes (the flag).  R = 0 does nothing. */
#define MI355_IVFPQ_RESIDUALS_WORKSPACE 512
int mi355_ivfpq_residuals(const float* rows, int64_t R, int dim, int rows_are_normalized, float eps, const int64_t* assignments,
                          const float* centroids, int64_t nlist, float* residuals, void* workspace, size_t workspace_bytes,
                          void* stream);
size_t mi355_ivfpq_residual_search_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int M, int64_t cap, int k);
int mi355_ivfpq_residual_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M,
                                const void* list_codes, int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist,
                                const int64_t* probes, int nprobe, int64_t cap, int k, int64_t idx_offset,
                                const mi355_rank_filter* filter, const float* centroids, float* out_val, int64_t* out_idx,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ binary (sign-bit) resident gallery
 * A row is dim bits: bit j says whether element j of the normalised row reaches a trained centre.  At dim = 1536 that is 192
 * bytes, twice the PQ row at M = 96 and an eighth of the int8 row.  The score of a pair is a Hamming distance - integer
 * arithmetic and one fp32 division - so everything below is bit for bit, with no tolerance anywhere.  The format is a shortlist
 * generator for a search that rescores (mi355_rescore_candidates): its own order is coarse.
 * Parameters: 1 <= dim <= 65536.  W = ceil(dim / 32) words; a row is stored as ld = W rounded up to a multiple of 4 uint32
 * words (a multiple of 16 bytes): codes [G][ld], row-major and appendable (encoding n rows to codes + r * ld writes rows
 * r .. r+n-1); the base is 16-byte aligned.  mi355_binary_bytes(R, dim) = R * ld * 4 (0 for a shape the entries reject).
 * center: device fp32 [dim], or NULL for zeros.  Embeddings that are pooled activations are positive in nearly every element,
 * so their raw signs are all ones: the centre (the column mean of the normalised rows) is what makes the bits informative.
 * Encode: n = the fp32 row mi355_l2_normalize_rows writes for x into a 16-byte aligned buffer, bit for bit
 * (rows_are_normalized != 0: n = x as it is).  Bit j lives in word j / 32 at position j % 32 and is 1 iff n[j] >= center[j]: a
 * comparison, no arithmetic, so no rounding; a NaN on either side gives 0.  Pad bits (j >= dim) and pad words are 0.  A gallery
 * row cannot carry a NaN: a row with a NaN element gets 0 bits there and scores like any row with those bits - the departure
 * from "a NaN row ranks first" that the PQ block makes too.  Queries are encoded by the same routine with the same centre.
 * Distance h(q, g) = popcount of the xor of the two code rows, an integer in [0, dim].
 * Score of (q, g) = float(dim - 2 h) / float(dim): both conversions exact, one IEEE fp32 division - the cosine of the two +-1
 * vectors.  A query whose normalised row n holds a NaN (a NaN or an infinite element of x always gives one) scores NaN against
 * every row; its row of mi355_binary_distances is -1.  A score depends on the two code rows alone - not on Q, G, k, the
 * filter, the chunk of the scan or the path.
 * Top-k: the selection of mi355_rank_topk (descending, NaN first, ties to the lower row, the slots a filter leaves empty
 * (-inf, -1)), k in [1, min(1024, G)].  At most dim + 1 distinct scores exist, so ties are the normal case.  An ineligible
 * row (filter) never enters the selection.
 * The scan: one workgroup per (chunk of 256 rows, block of 64 queries); the chunk's rows pass through LDS into registers, one
 * row per lane, and a query's words are wave-uniform.  It selects inside the kernel on the integer key (h, row).  For k <= 8
 * k candidates per (query, chunk) are merged by the selection of mi355_merge_topk (MI355_RANK_PATH_BINARY | FUSED).  For
 * 8 < k <= 1024 (| BITONIC) no score slab exists either: each chunk leaves its 8 best rows; with b the k-th best of those, a
 * row of the top-k that a chunk did not report lies in a chunk whose 8th row is not worse than b, a query has at most k / 8
 * such chunks, and every row of them is scored again; the selection of mi355_merge_topk over both sets is the exact top-k.
 * No atomics: one writer per output slot.
 * Every argument is checked before any HIP call (null pointers, shape, k, 16-byte alignment of the codes, codes_bytes,
 * workspace).  R, Q or G equal to 0 does nothing.  G < 2^31.  Workspace of both searching entries:
 * mi355_binary_search_workspace_bytes (k = 0: distances only; 0 for a shape the entry would reject, and for Q = 0).
 * dist: device int32 [Q][G]. */
size_t mi355_binary_bytes(int64_t R, int dim);
int mi355_binary_encode(const float* rows, int64_t R, int dim, int rows_are_normalized, float eps, const float* center, void* codes,
                        size_t codes_bytes, void* stream);
size_t mi355_binary_search_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_binary_distances(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G,
                           int32_t* dist, void* workspace, size_t workspace_bytes, void* stream);
int mi355_binary_search(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G, int k,
                        int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ binary gallery, asymmetric search: an int8 query against
 * the sign bits.  The symmetric search above cuts the query down to sign bits too, so every element of it counts the same,
 * whether it lies far from the centre or right on it, and a pair can take dim + 1 score values only.  Here the gallery stays
 * what it is - the codes of mi355_binary_encode, searchable without re-encoding - and the query keeps 8 bits per element.
 * "fp32" = one IEEE rounding per named operation; everything after the quantiser is integer arithmetic and one fp32 division,
 * so this block is bit for bit too.
 * Query side, per call: n = the fp32 row mi355_l2_normalize_rows writes for the query (the same row_inv_norm and the same
 * vec rule as the encoder).  r_j = n_j - center_j in fp32 (centre NULL: zeros).  amax = max |r_j| over j < dim.  u = the
 * int8 row quantiser of the int8 gallery block applied to r: inv = 127 / amax, u_j = clamp(rintf(r_j * inv), -127, 127)
 * (round-half-even).  A NaN in r, or a non-finite amax, makes a NaN query (codes 0).  amax < 1e-30 makes every code 0.
 * L1 = sum |u_j| <= 127 * 65536 < 2^23.
 * Distance m(q, g) = sum over j of |u_j| * [(u_j > 0 and bit_j(g) == 0) or (u_j < 0 and bit_j(g) == 1)]: a Hamming distance
 * weighted by the query's magnitudes, an integer in [0, L1].  With s_j = 2 bit_j - 1: L1 - 2 m = sum u_j s_j.  With P = the sum
 * of u_j over the set bits of g and Upos = the sum of the positive u_j: m = Upos - P.  Any summation order gives the same
 * integer.
 * Score = float(L1 - 2 m) / float(L1): both conversions exact (|L1 - 2 m| < 2^24), one IEEE fp32 division.  L1 == 0 scores
 * 0.0f against every row.  A NaN query scores NaN against every row; its row of mi355_binary_asym_distances is -1.
 * Order, ties, pads, filters: as mi355_binary_search - lower m first, then the lower row.  Distinct m give distinct scores
 * (the exact quotients of two m differ by at least 2 / L1 > 2^-22 and lie in [-1, 1], where an fp32 rounding moves a value by
 * at most 2^-25), so the order by score IS the order by m and the selection runs on the integer key (m, row).
 * A score depends on the query row, the centre and the code row alone - not on Q, G, k, the filter, the path or the stream.
 * The scan: one workgroup per (chunk of 256 rows, block of 64 queries).  The chunk's words pass through LDS; per 32
 * dimensions a lane expands the bits of its rows to bytes of 0 / 1 and v_mfma_i32_32x32x32_i8 sums them against the queries'
 * codes (P, exact in int32).  The endings and the k > 8 route are those of mi355_binary_search: MI355_RANK_PATH_BINARY_ASYM |
 * FUSED for k <= 8, | BITONIC for 8 < k <= 1024 (8 rows per chunk, the saturated chunks scored again by the same contract).
 * No atomics: one writer per output slot.
 * Arguments and their checks as mi355_binary_distances / mi355_binary_search; the workspace of both is
 * mi355_binary_asym_search_workspace_bytes (k = 0: distances only; 0 for a shape the entry would reject, and for Q = 0).
 * mi355_binary_asym_query_codes writes what the search makes of the queries: codes int8 [Q][dim] in plain order, l1 int32 [Q],
 * nanflag int32 [Q] (1: a NaN query); it needs no workspace.  dist: device int32 [Q][G]. */
size_t mi355_binary_asym_search_workspace_bytes(int64_t Q, int64_t G, int dim, int k);
int mi355_binary_asym_query_codes(const float* queries, int64_t Q, int dim, float eps, const float* center, int8_t* codes, int32_t* l1,
                                  int32_t* nanflag, void* stream);
int mi355_binary_asym_distances(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G,
                                int32_t* dist, void* workspace, size_t workspace_bytes, void* stream);
int mi355_binary_asym_search(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G, int k,
                             int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ graph search: a beam walk over neighbour lists
 * A best-first search over a graph on the rows of a resident gallery.  The result is approximate against the exhaustive
 * search, but a pure function of its inputs: every index, every score bit and both counters are specified here.
 *   queries [Q][dim] device fp32, raw: normalised by the call with the bits of mi355_l2_normalize_rows(queries, eps);
 *   rows: as in mi355_ivf_scan (MI355_DTYPE_F32 rows ld floats apart, or MI355_DTYPE_F16 rows 16-byte aligned with ld a
 *     multiple of 8 halves and zero padding); G rows, G < 2^31;
 *   graph [G][degree] device int32, dense: row r lists the neighbours of r, -1 is a pad; 2 <= degree <= 64;
 *   seeds [Q][nseed] device int64 row ids, -1 is skipped; 1 <= nseed <= 64;
 *   1 <= k <= ef <= 512, 1 <= max_iters, nseed + max_iters * degree <= 16384, 1 <= dim <= 4096.
 * Score s(q, r): exactly what mi355_rescore_candidates returns for the pair (the same routine: one wave per row, lane-strided
 * units, fused multiply-adds, the wave reduction).  It depends on the query and the row only.
 * Beam order: that of mi355_merge_topk - NaN first, then descending score, ties (-0 equal to +0) to the lower row.
 * Per query: visited = {}, the beam empty.
 *   1. For each seed in order: -1 and a row already visited are skipped; every other row is marked visited, scored and put
 *      into the beam, which keeps its best ef entries.
 *   2. For it = 0 .. max_iters - 1: p = the first beam entry in beam order that has not been expanded; none: stop.  p is marked
 *      expanded.  For j = 0 .. degree - 1, n = graph[p][j]: -1 and a visited n (self-loops, duplicates within a list) are
 *      skipped; every other n is marked visited and scored.  The new beam is the best ef of the old beam and the new rows.  A
 *      row that drops out of the beam stays visited.
 *   3. out_val / out_idx [Q][k]: the first k beam entries that the filter (NULL, or the eligibility rule of the filtered
 *      searches) accepts, indices + idx_offset; the remaining slots hold (-inf, -1).  The filter never changes the walk.
 *   4. out_iters / out_visited [Q] device int32 (either may be NULL): the number of expansions, and the size of the visited set.
 * The kernel: one workgroup of 16 waves per query; the normalised query, the beam and the visited set (an open-addressing
 * table of the power of two at or above 2 * (nseed + max_iters * degree) slots: it cannot fill, and membership does not depend
 * on the order of insertion) live in LDS, at the limits 153 KB of the 160.  One hop is one coalesced read of p's list, the
 * visited filter, one wave per new row, and a merge by rank into the sorted beam.  Every loop has a bound known before it
 * starts; no workgroup waits on another; there are no global atomics.
 * A seed or a graph entry outside [0, G) other than -1 is never dereferenced: it raises a flag word that is read back once
 * behind the launch (one host sync at the end, as in mi355_ivf_scan) and the call fails with a message.
 * Every argument is checked before any HIP call.  Q = 0 does nothing.  The sizer returns 0 for a shape the entry would
 * reject, and for Q = 0. */
size_t mi355_graph_search_workspace_bytes(int64_t Q, int dim, int nseed, int ef, int degree, int max_iters);
int mi355_graph_search(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld, int64_t G,
                       const int32_t* graph, int degree, const int64_t* seeds, int nseed, int k, int ef, int max_iters,
                       int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, int32_t* out_iters,
                       int32_t* out_visited, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ backbone models
 * Replaces timm.create_model(name, num_classes=N) and the methods the reference calls on it
 * (inference/inference.py:102,110,133,146,199-201 ; train/train.py:194-195,288,396 ;
 *  train/train_efficientnet.py:226,230 ; train/train_vit_triplet.py:354-357).
 * Names: "efficientnet_b3a" ("efficientnet_b3"), "rexnet_150", "rexnet_200",
 *        "swin_base_patch4_window7_224".  Input 224x224 (effnet/rexnet accept any H,W multiple of 32).
 */
typedef struct mi355_model* mi355_model_t;

/* num_classes: 0 = identity classifier (pooled features out), >0 = Linear head of that width. */
int mi355_model_create(const char* name, int num_classes, mi355_model_t* out);
void mi355_model_destroy(mi355_model_t m);

/* Parameter/buffer table in timm-0.4.12 state-dict order.  kind: 0 = trainable parameter,
 * 1 = float buffer (BN running stats), 2 = int64 buffer (num_batches_tracked, relative_position_index). */
int mi355_model_num_tensors(mi355_model_t m);
int mi355_model_tensor_info(mi355_model_t m, int i, const char** name, int* ndim, int64_t shape[4],
                            int* kind);
int mi355_model_feature_dim(mi355_model_t m);   /* D: 1536 / 1920 / 2560 / 1024 */
int mi355_model_num_classes(mi355_model_t m);

/* Hand one state-dict tensor (HOST pointer, fp32, contiguous, numel elements) to the model by its
 * timm key — the load_state_dict half of inference/inference.py:117-124.  int64 buffers are ignored. */
int mi355_model_set_tensor(mi355_model_t m, const char* name, const float* host_data, int64_t numel);

/* One-time pack (SURVEY §5 "checkpoint"): fold eval-mode BN into the conv weights, round to bf16,
 * lay out for the kernels, upload to the current device.  Must be called after the last set_tensor
 * and again whenever weights change. */
int mi355_model_pack(mi355_model_t m, void* stream);

/* forward_features: x [B][3][H][W] fp32 NCHW (device) ->
 *   effnet/rexnet: out [B][D][H/32][W/32] fp32 NCHW (un-pooled, as timm returns it)
 *   swin:          out [B][D] fp32 (timm's swin forward_features pools)
 * forward: -> out [B][num_classes] fp32 logits, or [B][D] pooled features when num_classes == 0.
 * pooled_out (optional, may be NULL): [B][D] fp32 global-average-pooled features (get_fm,
 * train/train.py:84-103) produced on the way. */
int mi355_model_forward_features(mi355_model_t m, const float* x, int B, int H, int W, float* out,
                                 float* pooled_out, void* stream);
int mi355_model_forward(mi355_model_t m, const float* x, int B, int H, int W, float* out,
                        float* pooled_out, void* stream);

/* The same forward with the pre-processing fused into the stem's input load: images
 * [B][h][w][3] uint8 on the device (one size for the batch) -> SquarePad(fill) (utils/square_pad.py:20-36) -> ToTensor
 * (/255) -> Normalize(mean, std: HOST float[3]) (inference/inference.py:48-52) -> optional conv_input (conv_input_w:
 * DEVICE fp32 [3][3][3][3] as Conv2d(3,3,3,1,1,bias=False).weight, NULL = none) + SiLU (inference/inference.py:101-105)
 * -> stem, in ONE kernel: no fp32 NCHW batch is written.  Output as mi355_model_forward (features_only = 0) or
 * mi355_model_forward_features (1) for an S x S input, S = max(h, w).  Bit-identical to running the separate
 * mi355_square_pad_normalize / mi355_conv_input_silu / forward chain.  Conv backbones only (efficientnet, rexnet). */
int mi355_model_forward_u8(mi355_model_t m, const unsigned char* images, int B, int h, int w, int fill,
                           const float* mean, const float* stdv, const float* conv_input_w, int features_only,
                           float* out, float* pooled_out, void* stream);

/* Ragged batches of decoded images: the images of a batch may all have different sizes.  They are packed in
 * one device buffer `pixels` of pixels_bytes bytes and described by desc[B][3] int64 = {byte offset of the image in pixels,
 * h, w}, each image uint8 RGB HWC.  The descriptors come twice with the same content: desc_host (HOST) is what the library
 * checks and plans with, desc_dev (DEVICE) is what the kernels read; the caller keeps desc_dev alive until the work has run.
 * Checked before any HIP call: non-null pointers, B >= 1, 1 <= h, w <= 16384, every image inside pixels_bytes.
 *
 * mi355_resize_batch_u8: transforms.Resize((out_h, out_w)) of train/train.py:48 on every image, bit-exact with Pillow as
 * mi355_resize_bilinear_u8 (same tables, same integer MACs) -> out [B][out_h][out_w][3] uint8, in two launches for the
 * whole batch.  pad != 0: SquarePad(fill) (utils/square_pad.py:20-36) first - each image is resampled as its own virtual
 * S x S square, S = max(h, w), whose border reads `fill`.  workspace: mi355_resize_batch_workspace_bytes(...) device bytes
 * (the per-call plan and the horizontal-pass rows).  Tables for sizes a device sees for the first time are uploaded with one
 * copy and one stream synchronise per call; nothing else synchronises. */
size_t mi355_resize_batch_workspace_bytes(const int64_t* desc_host, int B, int out_h, int out_w, int pad);
int mi355_resize_batch_u8(const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                          int B, int out_h, int out_w, int pad, int fill, unsigned char* out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* mi355_model_forward_u8 for a ragged batch.  transform:
 *   0 "pad"         SquarePad(fill) -> ToTensor -> Normalize, inference/inference.py:48-52: every image must have the same
 *                   longer side S (224 for swin); the pre-processing is fused into the stem / patch embedding, which reads
 *                   each image's descriptor.  Bit-identical per image to mi355_square_pad_normalize + mi355_model_forward
 *                   at the same B.  out_size and the workspace are not used.
 *   1 "resize"      Resize((out_size, out_size)) (train/train.py:48) with mi355_resize_batch_u8 into the workspace, then
 *                   mi355_model_forward_u8 on that uniform batch.
 *   2 "pad_resize"  SquarePad(fill) then Resize, likewise.
 * mean / stdv: HOST float[3]; conv_input_w: as mi355_model_forward_u8 (conv backbones only); out / pooled_out as
 * mi355_model_forward (features_only = 0) or _features (1) at S x S, S = the common longer side or out_size.  Also checked
 * before any HIP call: fill in 0..255, nonzero std, out_size in 1..16384 (and >= 32; 224 for swin) for transforms 1 and 2,
 * the workspace size. */
size_t mi355_model_forward_images_workspace_bytes(const int64_t* desc_host, int B, int transform, int out_size);
int mi355_model_forward_images(mi355_model_t m, const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host,
                               const int64_t* desc_dev, int B, int transform, int out_size, int fill, const float* mean,
                               const float* stdv, const float* conv_input_w, int features_only, float* out, float* pooled_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Debug/parity tap: copy the bf16 NHWC activation the executor produced for layer `tap_name`
 * (e.g. "stem", "blocks.1.0") during the LAST forward into out as fp32 NCHW.  Taps are recorded
 * only after mi355_model_enable_taps(m, 1). */
int mi355_model_enable_taps(mi355_model_t m, int enable);
int mi355_model_read_tap(mi355_model_t m, const char* tap_name, float* out, int64_t out_numel,
                         int64_t shape[4], void* stream);

/* Parity tool: run ONLY the layers behind tap `from_tap` up to and including the one that records tap `to_tap` on an
 * activation supplied by the caller: x [B][C][h][w] fp32 NCHW on the device (rounded to bf16 on the way in; feed it the
 * oracle's bf16-rounded tap of the previous layer).  Taps are recorded as in a normal forward (enable them first), so a
 * layer is compared with the oracle on the ORACLE's input and errors do not compound through the network. */
int mi355_model_run_between_taps(mi355_model_t m, const char* from_tap, const char* to_tap, const float* x, int B,
                                 int C, int h, int w, void* stream);

/* Algorithmic HBM bytes of one forward at batch B (layer-granular model) and the
 * MACs; used by bench.py's roofline. */
int mi355_model_traffic(mi355_model_t m, int B, int H, int W, double* act_bytes, double* weight_bytes,
                        double* macs);

/* Per-kernel-family view of the same model, for the roofline of the dominant kernel.  Arrays of n >= 8
 * doubles indexed by kind: 0 stem, 1 1x1-conv GEMM, 2 depthwise, 3 SE, 4 other, 5 window attention, 6 layernorm,
 * 7 fused expand+depthwise (pairs the executor runs as one kernel; bytes are still the layer-granular model). */
int mi355_model_traffic_kinds(mi355_model_t m, int B, int H, int W, double* bytes_by_kind, double* macs_by_kind, int n);

/* Executor options: "microbatch" (images per pass through the layer plan; 0 = whole batch),
 * "fuse" (1 = run expand+depthwise pairs on whole-image tiles as one LDS-resident kernel; default 1),
 * "fuse_block" (1 = run whole MBConv blocks of the 14x14 / 7x7 stages - expand, depthwise, SE, gated projection, residual -
 *  as ONE kernel per block; default 1), "fuse_block_min_batch" (use it only for batches of at least this many images;
 *  default 192: one workgroup per image needs about a CU per image to win),
 * "fuse_sweep" (1 = run expand+depthwise of the 112x112 .. 28x28 blocks with the row-sweep kernel, MFMA depthwise from an
 *  LDS row window; default 1), "fuse_band" (older band kernel for shapes the row-sweep kernel does not cover),
 * "profile" (1 = bracket every op with hipEvents on the launch stream; resets the accumulators). */
int mi355_model_set_option(mi355_model_t m, const char* key, int64_t value);
/* Accumulated per-kind kernel time (ms) and launch counts since "profile" was enabled; synchronises. */
int mi355_model_profile_read(mi355_model_t m, double* ms_by_kind, int64_t* launches_by_kind, int n);

/* Per-op profile table (plan order): average launch ms since "profile" was enabled, algorithmic bytes at
 * batch B, kind, and a text label (labels: max_ops * label_stride chars).  Returns the number of ops
 * (callers size the arrays with max_ops >= that; 1024 is always enough).  Developer/bench tool. */
int mi355_model_profile_ops(mi355_model_t m, int B, int H, int W, int max_ops, double* avg_ms, double* bytes,
                            int* kinds, char* labels, int label_stride);

/* The launch plan of one chunk of a forward: which ops each launch covers and which kernel runs them, resolved from the op
 * list, the options, the caller's whole batch B, the chunk's nb images (1 <= nb <= B) and the input size; pooled != 0 asks
 * for the plan of mi355_model_forward (pooled embedding), 0 for that of mi355_model_forward_features.  Host-only: needs no
 * packed weights and makes no HIP call.  Step s covers the ops [first_op[s], first_op[s] + n_ops[s]) and runs as how[s];
 * the steps cover every op exactly once, in order.  *arena_bytes: the activation arena one chunk of nb images needs.
 * Returns the number of steps (arrays of max_steps entries are filled as far as they reach; 1024 is always enough) or a
 * negative error.  Developer / test tool. */
enum {
    MI355_PLAN_OP = 0,          /* one op, its own kernel */
    MI355_PLAN_FUSED_LATE = 1,  /* expand + depthwise on a whole-image tile (14x14 / 7x7 maps) */
    MI355_PLAN_SWEEP = 2,       /* expand + depthwise, row-sweep kernel */
    MI355_PLAN_BAND = 3,        /* expand + depthwise, row-band kernel */
    MI355_PLAN_BLOCK = 4,       /* expand, depthwise, SE and gated projection: the whole MBConv block in one kernel */
    MI355_PLAN_HEAD_GAP = 5,    /* head 1x1 conv + global average pool */
    MI355_PLAN_LN_STATS = 6     /* LayerNorm as a row-statistics pass; the next GEMM step applies it in its epilogue */
};
int mi355_model_plan(mi355_model_t m, int B, int nb, int H, int W, int pooled, int max_steps, int* first_op, int* n_ops,
                     int* how, size_t* arena_bytes);

/* Diagnosis of the whole-MBConv-block kernel (option "block_stamps" = 1): per-phase shader-cycle counts of the LAST forward,
 * averaged over its images.  out[op][16] in plan order (rows of ops that did not run as a block kernel stay 0); the 16
 * buckets are listed at the end of k_mbconv_block (csrc/mbconv_block.hip).  Synchronises the device.  Returns the number
 * of ops (size out with 16 * max_ops doubles, max_ops >= that; 1024 is always enough) or a negative error.  Developer tool. */
int mi355_model_block_stamps(mi355_model_t m, double* out, int max_ops);

/* timm ClassifierHead / get_fm on an un-pooled map (train/train.py:84-103 get_fm; :194-195 fm = forward_features(x);
 * lbl = model.head(fm)): fm [B][C][HW] fp32 NCHW (device) -> pooled_out (optional) [B][C] fp32 global average ->
 * out [B][N] = Linear(weight [N][C] fp32 device, bias [N] or NULL) on the bf16-rounded pooled features with bf16-rounded
 * weights and fp32 accumulation (the rounding points of the in-model classifier).  weight NULL: pooling only. */
int mi355_pool_linear(const float* fm, int B, int C, int HW, const float* weight, const float* bias, int N, float* out,
                      float* pooled_out, void* stream);

/* Stand-alone 1x1-conv / linear kernel (the model executor's GEMM): out[M][N] bf16 = act(A[M][K] bf16 * W^T + bias).
 * W is bf16 [ceil16(N)][ldw] with ldw = K rounded up to 32, zero padded; bias fp32 [ceil16(N)]; K, N multiples of 8.
 * act: 0 none, 1 SiLU, 2 ReLU, 3 ReLU6, 4 GELU, 5 sigmoid. */
int mi355_gemm_bf16(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int ldw, int act,
                    void* stream);

/* Developer entry: the same GEMM with every operand the model executor uses (tests reach each dispatch branch through it).
 *   out[m][n] = act( sum_k A'[m][k] W[n][k] + bias[n] ) (+ res[m][n] for n < res_n), one rounding (bf16 out) or none (fp32 out)
 *   A'[m][k]  = bf16( a_relu6 ? relu6(A[m][k] * g) : A[m][k] * g ),  g = gate[m / rows_per_img][k]  (A' = A when gate is NULL
 *               and a_relu6 is 0; relu6(A) when gate is NULL and a_relu6 is 1)
 *   ln_stats [M][2] (mean, rstd) + ln_colsum [ceil16(N)]: LayerNorm-folded epilogue, acc -> rstd (acc - mean colsum) before the bias
 *   splitk_ws (splitk_ws_bytes): fp32 scratch that enables the split-K path; M_sel: the rows that decide split-K (0: M)
 * W is bf16 [ceil16(N)][ldw], bias fp32 [ceil16(N)], all pointers 16-byte aligned device pointers; res / gate / ln / workspace
 * may be NULL.  path (host, may be NULL) receives the branch that ran: MI355_GEMM_PATH_* in the low byte, and for the kernels
 * templated on the tile width the number of 16-column sub-tiles (MI355_GEMM_PATH_NT).  Every argument is checked before any HIP
 * call.  The environment variables the dispatcher reads (MI355_GEMM_WIDE, ...) apply as in the model. */
typedef struct mi355_gemm_ex_args {
    const void* A; int lda;
    const void* W; int ldw;
    const float* bias;
    const void* res; int ldr; int res_n;
    const float* gate; int gate_ld; int rows_per_img; int a_relu6;
    void* out; int ldo; int out_f32;
    int M, N, K, act;
    int64_t M_sel;
    void* splitk_ws; size_t splitk_ws_bytes;
    const float* ln_stats; const float* ln_colsum;
} mi355_gemm_ex_args;

enum {
    MI355_GEMM_PATH_TILE_M64_BK32 = 1,    /* k_gemm_bf16<1, NT, 32>: M <= 64, K < 64 */
    MI355_GEMM_PATH_TILE_M64_BK64 = 2,    /* k_gemm_bf16<1, NT, 64>: M <= 64, K >= 64 */
    MI355_GEMM_PATH_TILE = 3,             /* k_gemm_bf16<2, NT, 32> */
    MI355_GEMM_PATH_BIG = 4,              /* k_gemm_big<false, false, 64> */
    MI355_GEMM_PATH_BIG_KTAIL = 5,        /* k_gemm_big<false, true, 64> */
    MI355_GEMM_PATH_BIG32 = 6,            /* k_gemm_big<false, false, 32> */
    MI355_GEMM_PATH_BIG32_KTAIL = 7,      /* k_gemm_big<false, true, 32> */
    MI355_GEMM_PATH_BIG_GATED = 8,        /* k_gemm_big<true, false, 64> */
    MI355_GEMM_PATH_BIG_GATED_KTAIL = 9,  /* k_gemm_big<true, true, 64> */
    MI355_GEMM_PATH_STREAM = 10,          /* k_gemm_stream<NT, 1> */
    MI355_GEMM_PATH_PROJ = 11,            /* k_proj_lds<NT, KST> */
    MI355_GEMM_PATH_SPLITK = 12,          /* k_gemm_splitk + k_splitk_reduce */
    MI355_GEMM_PATH_WIDE = 13             /* k_gemm_wide<MI> (MI355_GEMM_WIDE=1) */
};
#define MI355_GEMM_PATH_KIND(p) ((p) & 0xff)
#define MI355_GEMM_PATH_NT(p) (((p) >> 8) & 0xff)

int mi355_gemm_bf16_ex(const mi355_gemm_ex_args* args, int* path, void* stream);

/* Developer entry: one depthwise conv of the convolutional backbones with its SE squeeze partials, then (when SE weights are
 * given) the SE gate on those partials, through the model's launchers.
 *   out[b][oy][ox][c] = bf16( act( sum_{ky,kx} in[b][oy*stride - k/2 + ky][ox*stride - k/2 + kx][c] w[ky*k + kx][c] + bias[c] ) )
 *                       (zero padding), Ho = (H - 1) / stride + 1, Wo likewise
 *   s[b][c] = (sum over oy, ox of the un-rounded activated output) / (Ho * Wo)
 *   gate[b][c] = sigmoid( sum_j se_w2t[j][c] act1( sum_c' se_w1[j][c'] s[b][c'] + se_b1[j] ) + se_b2[c] )
 * in [B][H][W][C] bf16 NHWC, w [k*k][C] bf16 (pack_dw's layout), bias [C] fp32, out [B][Ho][Wo][C] bf16: 16-byte aligned
 * device pointers, C a multiple of 8.  SE (optional, all five pointers or none): se_w1 / se_w2t [rd][C] fp32 holding bf16
 * values, se_b1 [rd] / se_b2 [C] fp32, gate [B][C] fp32.  k 3 or 5, stride 1 or 2, act / act1 as for mi355_gemm_bf16.
 * choice: MI355_DW_CHOICE_AUTO takes the model's decision (MI355_DW_TILED / MI355_DW_MFMA, read once per process); DIRECT,
 * TILED and MFMA force one kernel and are rejected for shapes that kernel does not take.  path (host, may be NULL) receives
 * MI355_DW_PATH(kind, k, stride, arg, se) of the kernels that ran.  Every argument is checked before any HIP call.
 * squeeze (optional, device [B][C] fp32) receives s computed ON THE HOST from the depthwise kernel's squeeze partials (copied
 * back, summed in the SE kernels' fixed order, times 1 / (Ho * Wo)); it is not read back from k_se / k_se_small, so it checks
 * the partials, and the gate checks what the SE kernels make of them.  Synchronises the stream (the squeeze partials are a per-call scratch buffer). */
typedef struct mi355_dwconv_ex_args {
    const void* in; const void* w; const float* bias; void* out;
    int B, H, W, C, k, stride, act, choice;
    const float* se_w1; const float* se_b1; const float* se_w2t; const float* se_b2;
    int rd, act1;
    float* gate;
    float* squeeze;
} mi355_dwconv_ex_args;

enum { MI355_DW_CHOICE_AUTO = 0, MI355_DW_CHOICE_DIRECT = 1, MI355_DW_CHOICE_TILED = 2, MI355_DW_CHOICE_MFMA = 3 };

enum {
    MI355_DW_PATH_DIRECT = 1,       /* k_dwconv<KS, S>, arg = pixels per thread (DW_PX) */
    MI355_DW_PATH_LDS3 = 2,         /* k_dw3_lds<NU>: 3x3 stride 1, C <= 48, even W; arg = NU = C / 8 */
    MI355_DW_PATH_TILED = 3,        /* k_dw_tiled<KS, PX>: stride 1 (opt-in MI355_DW_TILED); arg = PX */
    /* SE kernel, in MI355_DW_PATH_SE(p); 0 when no SE ran */
    MI355_DW_PATH_SE_SMALL = 1,     /* k_se_small: rd <= 16, C <= 1024 */
    MI355_DW_PATH_SE_FULL = 2       /* k_se */
};
#define MI355_DW_PATH(kind, ks, s, arg, se) ((kind) | (ks) << 8 | (s) << 12 | (arg) << 16 | (se) << 24)
#define MI355_DW_PATH_KIND(p) ((p) & 0xff)
#define MI355_DW_PATH_KS(p) (((p) >> 8) & 0xf)
#define MI355_DW_PATH_S(p) (((p) >> 12) & 0xf)
#define MI355_DW_PATH_ARG(p) (((p) >> 16) & 0xff)
#define MI355_DW_PATH_SE(p) (((p) >> 24) & 0xff)

int mi355_dwconv_se_ex(const mi355_dwconv_ex_args* args, int* path, void* stream);

/* Developer entry: the fused front half of one MBConv / RexNet block (1x1 expand -> bias + act_e -> depthwise k x k -> bias +
 * act_d, plus the SE squeeze sums) through the model's launchers: k_fused_late and k_fused_band (csrc/fused_mbconv.hip) and
 * k_sweep_mbconv (csrc/sweep_mbconv.hip).  The expanded tensor E never leaves the LDS.
 *   E[b][y][x][n]  = bf16( act_e( sum_c X[b][y][x][c] We[n][c] + be[n] ) )
 *   v[b][oy][ox][n] = act_d( sum_{ky,kx} E[b][oy*stride - k/2 + ky][ox*stride - k/2 + kx][n] Wd[ky*k + kx][n] + bd[n] )   (zero padding)
 *   D = bf16(v), Ho = (H - 1) / stride + 1, Wo likewise;  sum over blk of pool[b][blk][n] = sum over oy, ox of the un-rounded v
 * X [B][H][W][Cin] bf16 NHWC; We [ceil16(mid)][ceil32(Cin)] bf16 in GEMM packing, zero padded; be [ceil16(mid)] fp32; Wd [k*k][mid]
 * bf16; bd [mid] fp32; D [B][Ho][Wo][mid] bf16; pool (may be NULL) [B][nblk][mid] fp32 with nblk = *pool_nblk: 1 for the late and
 * sweep kernels, ceil(Ho / band rows) for the band kernel.  All 16-byte aligned device pointers; Cin and mid multiples of 8.
 * kernel: MI355_FRONT_KERNEL_AUTO takes the decision of the model's launch plan under default options (an error when the plan
 * would run the pair unfused); LATE, SWEEP and BAND force one kernel and are rejected for shapes that kernel does not take.
 * band_rows (BAND): output rows per workgroup, 0 = the largest that fits the LDS (what the model uses), else 1 .. that value.
 * sweep_variant / sweep_csplit (SWEEP): the model options of the same names (0 = default).
 * path (host, may be NULL) receives MI355_FRONT_PATH_LATE / _BAND / _SWEEP (...) of the instantiation that ran.  Every argument is
 * checked before any HIP call.  Does not synchronise. */
typedef struct mi355_mbconv_front_args {
    const void* X; const void* We; const float* be; const void* Wd; const float* bd; void* D; float* pool;
    int B, H, W, Cin, mid, k, stride, act_e, act_d;
    int kernel, band_rows, sweep_variant, sweep_csplit;
} mi355_mbconv_front_args;

enum { MI355_FRONT_KERNEL_AUTO = 0, MI355_FRONT_KERNEL_LATE = 1, MI355_FRONT_KERNEL_SWEEP = 2, MI355_FRONT_KERNEL_BAND = 3 };
/* activation instance of k_sweep_mbconv: compiled for SiLU / SiLU, for SiLU / none, or reading act_e / act_d at run time */
enum { MI355_FRONT_ACT_SILU_SILU = 1, MI355_FRONT_ACT_SILU_NONE = 2, MI355_FRONT_ACT_RUNTIME = 3 };
/* shape classes of k_sweep_mbconv: k_stride_map */
enum {
    MI355_SWEEP_CLASS_3_2_112 = 1, MI355_SWEEP_CLASS_3_1_56 = 2, MI355_SWEEP_CLASS_5_2_56 = 3, MI355_SWEEP_CLASS_5_1_28 = 4,
    MI355_SWEEP_CLASS_3_2_28 = 5, MI355_SWEEP_CLASS_3_2_56 = 6, MI355_SWEEP_CLASS_3_1_28 = 7
};
/* family = MI355_FRONT_KERNEL_*; late: NIW images' worth of channels per slab (slab = 128 NIW), PX pixels per depthwise thread;
 * band: KST k-steps, PX, MC channels per slab, TH output rows per workgroup; sweep: class, KST, NS channel tiles per pass, the
 * tuning variant that ran (0 when the request does not apply), activation instance, workgroups per image */
#define MI355_FRONT_PATH_BASE(family, ks, s) ((family) | ((ks) == 5) << 2 | ((s) == 2) << 3)
#define MI355_FRONT_PATH_LATE(ks, s, niw, px) (MI355_FRONT_PATH_BASE(MI355_FRONT_KERNEL_LATE, ks, s) | (niw) << 4 | (px) << 8)
#define MI355_FRONT_PATH_BAND(ks, s, kst, px, mc, th) \
    (MI355_FRONT_PATH_BASE(MI355_FRONT_KERNEL_BAND, ks, s) | (kst) << 4 | (px) << 8 | (mc) << 12 | (th) << 20)
#define MI355_FRONT_PATH_SWEEP(ks, s, cls, kst, ns, variant, act, csplit) \
    (MI355_FRONT_PATH_BASE(MI355_FRONT_KERNEL_SWEEP, ks, s) | (cls) << 4 | (kst) << 8 | (ns) << 12 | (variant) << 14 | (act) << 17 | (csplit) << 19)
#define MI355_FRONT_PATH_FAMILY(p) ((p) & 3)
#define MI355_FRONT_PATH_KS(p) (((p) >> 2 & 1) ? 5 : 3)
#define MI355_FRONT_PATH_S(p) (((p) >> 3 & 1) ? 2 : 1)

int mi355_mbconv_front_ex(const mi355_mbconv_front_args* args, int* pool_nblk, int* path, void* stream);

/* Developer entry: one whole MBConv / RexNet block of a 14-wide or 7-wide map in ONE launch of k_mbconv_block
 * (csrc/mbconv_block.hip), through the model's launcher and with the operand layouts the model's executor passes.
 *   E, v, D as for mi355_mbconv_front_ex (act_e must be SiLU);  s[b][n] = (1 / (Ho Wo)) sum over oy, ox of the un-rounded v
 *   r[b][j] = se_act( sum_n W1[j][n] s[b][n] + b1[j] ),  g[b][n] = sigmoid( sum_j W2[j][n] r[b][j] + b2[n] )       (fp32)
 *   A[b][p][n] = bf16( relu6?( D[b][p][n] g[b][n] ) )                                       (ReLU6 when a_relu6)
 *   Y[b][p][o] = bf16( sum_n A[b][p][n] Wp[o][n] + bp[o] + (has_res && o < res_n ? X[b][p][o] : 0) )
 * X [B][H][W][Cin] bf16 NHWC; We [ceil16(mid)][ceil32(Cin)] bf16 zero padded, be [ceil16(mid)] fp32; Wd [k*k][mid] bf16, bd [mid]
 * fp32; W1 and W2 [rd][mid] bf16 (W2 transposed), b1 [rd], b2 [mid] fp32; Wp [ceil16(Cout)][ceil32(mid)] bf16 zero padded, bp
 * [ceil16(Cout)] fp32; D [B][Ho Wo][mid] bf16 (the kernel's scratch: the depthwise output, readable afterwards); Y [B][Ho][Wo][Cout]
 * bf16.  All 16-byte aligned device pointers.  Cin, mid, Cout multiples of 8; has_res needs stride 1 and res_n a multiple of 8 in
 * 8 .. min(Cin, Cout), otherwise res_n = 0; norot 0..15: bit0 slabs, bit1 SE FC1 groups, bit2 SE FC2 chunks, bit3 projection
 * columns are NOT rotated by image (the bits of the result do not depend on it).  Shapes the kernel does not take (the model
 * then runs the unfused chain) are rejected.  path (host, may be NULL) receives MI355_BLOCK_PATH(...): the instantiation that
 * ran and the launcher's run-time choices.  Every argument is checked before any HIP call.  Does not synchronise.
 * mi355_mbconv_block_how: the same path (or the same "unsupported" error) from the shape alone; touches no device. */
typedef struct mi355_mbconv_block_args {
    const void* X; const void* We; const float* be; const void* Wd; const float* bd;
    const void* W1; const float* b1; const void* W2; const float* b2; const void* Wp; const float* bp;
    void* D; void* Y;
    int B, H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d, se_act, a_relu6, has_res, res_n, norot;
} mi355_mbconv_block_args;

/* instantiation: depthwise k (3 / 5), stride, map width WI (7 / 14), KST expand k-steps, NTW projection column tiles per wave, ACT_D
 * depthwise activation; run time: xwide = X rows Kp + 16 apart in the LDS (0: the compact ceil8(Cin) + 8), whole = the projection
 * stages whole super-chunks (PROJ_WHOLE; 0: double-buffered K chunks), nsc = super-chunks of the projection's K, js = SE FC2 slices */
#define MI355_BLOCK_PATH(ks, s, wi, kst, ntw, act_d, xwide, whole, nsc, js)                                                      \
    (((ks) == 5) | ((s) == 2) << 1 | ((wi) == 14) << 2 | (kst) << 3 | (ntw) << 7 | (act_d) << 10 | ((xwide) != 0) << 13 |      \
     ((whole) != 0) << 14 | (nsc) << 15 | (js) << 20)
#define MI355_BLOCK_PATH_KS(p) (((p) & 1) ? 5 : 3)
#define MI355_BLOCK_PATH_S(p) (((p) >> 1 & 1) ? 2 : 1)
#define MI355_BLOCK_PATH_WI(p) (((p) >> 2 & 1) ? 14 : 7)
#define MI355_BLOCK_PATH_KST(p) (((p) >> 3) & 15)
#define MI355_BLOCK_PATH_NTW(p) (((p) >> 7) & 7)
#define MI355_BLOCK_PATH_ACT_D(p) (((p) >> 10) & 7)
#define MI355_BLOCK_PATH_XWIDE(p) (((p) >> 13) & 1)
#define MI355_BLOCK_PATH_WHOLE(p) (((p) >> 14) & 1)
#define MI355_BLOCK_PATH_NSC(p) (((p) >> 15) & 31)
#define MI355_BLOCK_PATH_JS(p) (((p) >> 20) & 15)

int mi355_mbconv_block_ex(const mi355_mbconv_block_args* args, int* path, void* stream);
int mi355_mbconv_block_how(int H, int W, int Cin, int mid, int Cout, int k, int stride, int rd, int act_e, int act_d, int* path);

/* Developer entry: one stem call of the convolutional backbones (3x3 stride 2 pad 1, 3 -> Cout, + bias + act) through the
 * model's launchers, in either input form.  Exactly one of x and images is non-null.
 *   out[b][oy][ox][co] = bf16( act( bias[co] + sum_{ky,kx,ci} in[b][ci][2 oy - 1 + ky][2 ox - 1 + kx] w[(ky*3 + kx)*3 + ci][co] ) )
 *                        (zero padding), out [B][Ho][Wo][Cout] bf16 NHWC, Ho = (H - 1) / 2 + 1, Wo likewise
 *   w [27][Cout] fp32 in pack_stem's tap order (ky*3 + kx)*3 + ci, bias [Cout] fp32; Cout a multiple of 8, <= 256.
 *   fp32 form  x [B][3][H][W] fp32 NCHW is `in`.
 *   uint8 form images [B][H][W][3] uint8 (every image H x W) -> SquarePad(fill) to S x S, S = max(H, W) -> /255 ->
 *              (v - mean) / stdv (HOST float[3]) -> optional conv_input (conv_input_w: device fp32 [3][3][3][3]) + SiLU with
 *              no rounding in between, zero outside the S x S square -> `in` of the stem; Ho = Wo = (S - 1) / 2 + 1.
 *              Ragged (desc_host and desc_dev non-null, the same [B][3] int64 {byte offset into images, h, w} on the host
 *              and on the device; images_bytes = size of the packed buffer): H == W == S and every image's max(h, w) == S.
 * Bits: the uint8 form equals mi355_square_pad_normalize (-> mi355_conv_input_silu) -> the fp32 form; ragged equals uniform
 * per image.  path (host, may be NULL) receives what ran: MI355_STEM_PATH_F32_LOAD16 (W % 4 == 0: 16-byte staging loads) or
 * _F32_LOAD4, or MI355_STEM_PATH_U8 | _CONV_INPUT | _RAGGED.  x, w, bias, out: 16-byte aligned; conv_input_w: 4-byte aligned.
 * Every argument is checked before any HIP call.  Does not synchronise. */
typedef struct mi355_stem_ex_args {
    const float* x;
    const unsigned char* images; int64_t images_bytes;
    const int64_t* desc_host; const int64_t* desc_dev;
    int B, H, W;
    int fill; const float* mean; const float* stdv;
    const float* conv_input_w;
    const float* w; const float* bias; void* out;
    int Cout, act;
} mi355_stem_ex_args;

enum {
    MI355_STEM_PATH_F32_LOAD16 = 1,     /* k_stem, input band staged with 16-byte loads (W % 4 == 0) */
    MI355_STEM_PATH_F32_LOAD4 = 2,      /* k_stem, input band staged with 4-byte loads */
    MI355_STEM_PATH_U8 = 3,             /* k_stem_u8<CONV_INPUT, RAGGED> */
    MI355_STEM_PATH_CONV_INPUT = 0x100,
    MI355_STEM_PATH_RAGGED = 0x200
};

int mi355_stem_ex(const mi355_stem_ex_args* args, int* path, void* stream);

/* Developer entry: head 1x1 conv + bias + act + global average pool in one kernel (k_head_gap) through the model's launcher.
 *   pooled[b][n] = (1 / HW) sum_p float( bf16( act( sum_k A[b * HW + p][k] W[n][k] + bias[n] ) ) ),  p = 0 .. HW-1 in order
 *   pooled_bf16 (optional) [B][ldp] bf16: the same values rounded once.  Bit for bit mi355_gemm_bf16_ex (bf16 out) -> mi355_gap.
 * A [B * HW][lda] bf16, W bf16 [ceil16(N)][ldw] zero padded past K, bias fp32 [ceil16(N)], pooled fp32 [B][ldp]; all 16-byte
 * aligned device pointers.  Rejected for shapes the kernel does not take: 1 <= HW <= 64, 32 <= K <= 512, lda a multiple of
 * 8 and >= K, ldw a multiple of 32 and >= K rounded up to 32, N a multiple of 8, act none (0) or SiLU (1); and ldp >= N, even.
 * path (host, may be NULL) receives MI355_HEAD_GAP_PATH(act, KSMAX) of the instantiation: KSMAX 12 (K <= 384) or 16.
 * Every argument is checked before any HIP call.  Does not synchronise. */
#define MI355_HEAD_GAP_PATH(act, ksmax) ((act) | (ksmax) << 8)
#define MI355_HEAD_GAP_PATH_ACT(p) ((p) & 0xff)
#define MI355_HEAD_GAP_PATH_KSMAX(p) (((p) >> 8) & 0xff)
int mi355_head_gap_ex(const void* A, int lda, const void* W, int ldw, const float* bias, float* pooled, void* pooled_bf16, int ldp,
                      int B, int HW, int N, int K, int act, int* path, void* stream);

/* Developer entry: global average pool (k_gap).  in [B][HW][C] bf16 -> pooled [B][C] fp32 = (sum_p in[b][p][c]) * (1 / HW),
 * fp32, the pixels added in ascending order; pooled_bf16 (optional) [B][C] bf16, the same values rounded once.  C a multiple
 * of 8; 16-byte aligned device pointers.  Every argument is checked before any HIP call.  Does not synchronise. */
int mi355_gap(const void* in, int B, int HW, int C, float* pooled, void* pooled_bf16, void* stream);

/* Developer entries: the two layout kernels behind forward_features, the taps and mi355_model_run_between_taps.
 *   mi355_nhwc_to_nchw: in [B][HW][C] bf16 -> out [B][Cvalid][HW] fp32, out[b][c][p] = float(in[b][p][c]) (exact), c < Cvalid.
 *   mi355_nchw_to_nhwc: in [B][Cvalid][HW] fp32 -> out [B][HW][C] bf16, out[b][p][c] = bf16(in[b][c][p]) (nearest even) for
 *                       c < Cvalid and zero for Cvalid <= c < C.
 * 1 <= Cvalid <= C.  Every argument is checked before any HIP call.  Neither synchronises. */
int mi355_nhwc_to_nchw(const void* in, float* out, int B, int HW, int C, int Cvalid, void* stream);
int mi355_nchw_to_nhwc(const float* in, void* out, int B, int HW, int C, int Cvalid, void* stream);

/* Developer entry: one Swin window-attention layer (window 7, head_dim 32) through the model's kernel.
 *   qkv [B][res*res][3C] bf16 (channel = which * C + head * 32 + d, tokens in image order), out [B][res*res][C] bf16,
 *   bias_table [169][heads] fp32 (timm relative_position_bias_table), packed to the kernel's dense layout by the model's
 *   packing routine; shift 0 or 3 (cyclic shift + -100 mask of timm's shifted windows, res > 7).
 *   out = softmax(q k^T 32^-0.5 + bias + mask) v per (image, window, head).  res a multiple of 7, C == 32 * heads.
 * Every argument is checked before any HIP call.  Synchronises the stream (the packed bias is a per-call scratch buffer). */
int mi355_window_attention(const void* qkv, const float* bias_table, void* out, int B, int res, int C, int heads, int shift,
                           void* stream);

/* Developer entry: one Swin window-attention layer with the window side as an argument (head_dim 32).
 *   window 7: exactly mi355_window_attention (same kernel, same checks, same bits).
 *   window 14: the 14x14-window kernel of swin_s3_base_224's 14x14 stage.  qkv / out as above, bias_table [729][heads] fp32
 *   (timm relative_position_bias_table, (2*14-1)^2 rows), copied to the kernel's head-major layout by the model's packing
 *   routine; res a multiple of 14, shift 0 only (no mask).
 * Every argument is checked before any HIP call.  Synchronises the stream (the packed bias is a per-call scratch buffer). */
int mi355_window_attention_ws(const void* qkv, const float* bias_table, void* out, int B, int res, int C, int heads, int window,
                              int shift, void* stream);

/* Developer entry: one Swin LayerNorm over the channel dim through the model's launcher (k_layernorm, eps inside the square root).
 *   merge 0: in [rows][C] bf16.  merge 1: in [rows / (gh*gw)][2*gh][2*gw][C/4] bf16, and row (b, oy, ox) is timm's PatchMerging
 *            concat [x(2oy, 2ox), x(2oy+1, 2ox), x(2oy, 2ox+1), x(2oy+1, 2ox+1)], gathered on load; rows a multiple of gh*gw.
 *   stats 0: out [rows][C] bf16 = (x - mean) rstd gamma + beta.  stats 1: out [rows][2] fp32 (mean, rstd), what the
 *            LayerNorm-folded GEMM epilogue reads as ln_stats; gamma and beta may be NULL.  merge with stats is rejected.
 *   C is one of 96, 192, 384, 768, 1536, 128, 256, 512, 1024, 2048; gamma, beta fp32 [C]; all pointers 16-byte aligned.
 * Every argument is checked before any HIP call.  Does not synchronise. */
int mi355_swin_layernorm(const void* in, const float* gamma, const float* beta, void* out, int64_t rows, int C, int merge, int gh, int gw,
                         int stats, float eps, void* stream);

/* Developer entry: Swin's patch embedding (4x4 stride-4 conv 3 -> embed, bias, LayerNorm(embed)) through the model's kernels.
 * Exactly one of x and images is non-null:
 *   x      fp32 [B][3][H][224], H a multiple of 4 in [4, 224] (the width stays 224: the kernel is laid out for 56 patches a row);
 *   images uint8 [B][h][w][3] with max(h, w) == 224 and H == 224: SquarePad(fill) -> /255 -> (v - mean) / stdv applied on load
 *          (mean, stdv HOST float[3]); with desc_dev (device int64 [..][3] = {byte offset into images, h, w}) a ragged packed
 *          batch whose image b is desc_dev[b0 + b] (h, w unused; every descriptor's longer side must be 224).
 *   weight fp32 [embed][3][4][4] on the device (timm patch_embed.proj.weight), packed by the model's routine (bf16-rounded,
 *          transposed); bias, gamma, beta fp32 [embed]; embed 128 or 96; out [B][(H/4)*56][embed] bf16.
 * Every argument is checked before any HIP call.  Synchronises the stream (the packed weight is a per-call scratch buffer). */
int mi355_swin_patch_embed(const float* x, const unsigned char* images, const int64_t* desc_dev, int b0, int B, int H, int h, int w,
                           int fill, const float* mean, const float* stdv, const float* weight, const float* bias, const float* gamma,
                           const float* beta, int embed, float eps, void* out, void* stream);

/* Developer entry: Swin's final LayerNorm(C) + mean over the L tokens of each image through the model's kernels.
 *   in [B][L][C] bf16, gamma / beta fp32 [C], pooled [B][C] fp32, pooled_bf16 [B][C] bf16 (the same values rounded once).
 *   C is 1024 or 768, L >= 1.  Every argument is checked before any HIP call.  Does not synchronise. */
int mi355_swin_ln_token_mean(const void* in, const float* gamma, const float* beta, float* pooled, void* pooled_bf16, int B, int L, int C,
                             float eps, void* stream);

/* Inference pre-processing: SquarePad(fill) -> ToTensor -> Normalize, utils/square_pad.py:20-36 +
 * inference/inference.py:48-52.  img: uint8 RGB, HWC (h, w, 3) on the device; mean/std: HOST float[3];
 * out: fp32 (3, S, S) with S = max(h, w), i.e. one image slot of the model's NCHW input batch. */
int mi355_square_pad_normalize(const unsigned char* img, int h, int w, int fill, const float* mean, const float* stdv,
                               float* out, void* stream);

/* Training-time resize: transforms.Resize((out_h, out_w)) of train/train.py:48-50 applied to a PIL
 * image, i.e. PIL.Image.resize((out_w, out_h), BILINEAR) — Pillow's two-pass antialiased resample (Resample.c, 8-bit
 * path), reproduced bit-exactly.  img / out: uint8 RGB HWC on the device; tmp: device scratch of h * out_w * 3 bytes,
 * needed only when both sides change (may be NULL otherwise). */
int mi355_resize_bilinear_u8(const unsigned char* img, int h, int w, unsigned char* out, int out_h, int out_w,
                             unsigned char* tmp, void* stream);

/* Score booster (utils/score_booster.py:1-37) over n fp32 scores on the device.
 * mode 0: cos_sim_score_with_threshold (score >= threshold ? (s+eps)/(eps+alpha) : |(s+alpha/eps)/(2 eps)|),
 * mode 1: cos_sim_score_booster(mode="for_pos"), mode 2: mode="for_neg".  out may alias scores. */
int mi355_score_boost(const float* scores, int64_t n, float eps, float alpha, float threshold, int mode, float* out,
                      void* stream);

/* conv_input pre-stem (inference/inference.py:103-105): out = SiLU(Conv2d(3,3,3,1,1,bias=False)(x)),
 * x/out [B][3][H][W] fp32 NCHW, w [3][3][3][3] fp32 (device). */
int mi355_conv_input_silu(const float* x, const float* w, int B, int H, int W, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355_RETRIEVAL_H */
