/*
 * xfmr_search.h -- the refined item search of libxfmr_hip.so: a bf16 MFMA shortlist, an exact f32 re-rank of the
 * shortlist, and a per-query proof that the short answer is the exact search's answer.
 *
 * The reference searches with LanceIndex.search(...).refine_factor(4) (xfmr_rec/index.py:214-255): a compressed first
 * pass fetches refine_factor * top_k candidates, the full vectors re-rank them. xfmr_topk_tiled (xfmr_hip.h) replaced
 * that with an exact scan at the f32 MFMA rate. This entry is the two-stage form on top of the same pieces:
 *   coarse   every eligible item (1 <= j < n_rows, not in the query's sorted exclusion list) is scored against every
 *            query with v_mfma_f32_32x32x16_bf16: the query rounded to bf16 (nearest even) in the kernel, the item rows
 *            read from table_bf16, the metric's epilogue the exact search's. The k_short best (score, index) pairs
 *            per query are kept (order: higher score, then lower index) together with tau, an upper bound on the
 *            coarse score of every eligible item that was NOT kept (-inf when all were kept).
 *   refine   every kept item is scored again in f32 with the exact search's arithmetic -- the bits xfmr_topk_tiled
 *            reports for the item --, non-finite scores are dropped, the best k leave, padded with -1 / -inf.
 *   proof    out_certified[q] = 1 exactly when the k results are provably xfmr_topk_tiled's: every eligible item was
 *            kept, or the k-th refined score is strictly greater than tau + bound_q, where bound_q bounds
 *            |coarse score - exact score| over the query's items (DESIGN.md "Refined search"). A query that is zero,
 *            non-finite or longer than 2^40, a table whose largest row norm is not a finite number <= 2^40, and a
 *            non-finite coarse score anywhere in the query's row leave the query uncertified. The flag may be
 *            pessimistic; it is never wrong.
 * Conventions as in xfmr_hip.h: caller-owned device buffers, work enqueued on `stream`, nothing read back, 0 or a
 * negative XFMR_E* code returned, every refusal before any launch. XFMR_ABI_VERSION stays 3.
 */
#ifndef XFMR_SEARCH_H
#define XFMR_SEARCH_H

#include "xfmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the scratch of one xfmr_search_refined call; 0 when a size is not positive. */
size_t xfmr_search_refined_workspace(int64_t n_query, int64_t n_rows, int32_t k_short);

/* What the call does for these sizes, as integers, touching no device: out[0] = queries per workgroup, out[1] = items per
 * tile, out[2] = catalogue slices, out[3] = items per slice, out[4] = dynamic LDS bytes of the coarse kernel, out[5] =
 * k_short = max(k, min(k * refine_factor, 128)), out[6] = the running list's length (k_short rounded up to a power of
 * two), out[7] = the 16-deep k-steps of query fragments a lane keeps in registers. Returns the code the search returns
 * for the sizes (XFMR_EINVAL: a size or refine_factor not positive; XFMR_EUNSUPPORTED: k > 128, H > 1024 or H not a
 * multiple of 8, n_rows or n_query >= 2^31). */
int xfmr_search_refined_plan(int64_t n_query, int64_t n_rows, int32_t H, int32_t k, int32_t refine_factor, int32_t out[8]);

/* query (n_query, H) f32; table (n_rows, H) f32 and table_bf16 its bf16 copy (xfmr_table_prepare: nearest even, bit
 * for bit); table_rnorm (cosine) / table_sqnorm (l2) as xfmr_topk_tiled takes them, the other may be NULL;
 * table_max_norm = the largest row norm over rows 1 .. n_rows - 1 and table_max_rnorm = the largest table_rnorm entry
 * over the same rows, computed once by the caller (they enter the bound only: a value that is too large costs
 * certificates, one that is too small makes them wrong). exclude / exclude_offsets: CSR of excluded items per query,
 * each row sorted ascending, or both NULL. k <= k_short <= 128. out_idx (n_query, k) int64, out_score (n_query, k)
 * f32, out_certified (n_query) bytes. Refusals in this order: XFMR_EINVAL (a pointer, a size, k_short < k, the
 * exclusion pair, the metric, the norm array the metric needs), XFMR_EUNSUPPORTED (the sizes as in the plan query,
 * k_short > 128), XFMR_EALIGN (query, table, table_bf16 or workspace not 16-byte aligned), XFMR_EWORKSPACE. */
int xfmr_search_refined(const float* query, const float* table, const void* table_bf16, const float* table_rnorm,
                        const float* table_sqnorm, float table_max_norm, float table_max_rnorm, int64_t n_rows,
                        int64_t n_query, int32_t H, const int64_t* exclude, const int64_t* exclude_offsets, int32_t k,
                        int32_t k_short, int32_t metric, int64_t* out_idx, float* out_score, uint8_t* out_certified,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XFMR_SEARCH_H */
