// The pieces of the exact search that more than one source file needs (retrieval.hip: the searches and the rank paths;
// search.hip: the refined search). Each is written ONCE here: the order (tt_better), the eligibility tests (tt_finite,
// tt_excluded), the score formula (rk_score), the query norm (rk_query_sqnorm), the scalar mirror of the f32 score tile
// (rk_chain_dot, rk_item_score), the sort (tt_sort), the streaming top-k's merge (tt_merge), the slice plan
// (tiled_plan) and the entries' common refusals (search_check). Everything has internal linkage: a source file that
// includes this header gets its own copy and exports nothing new.
#pragma once
#include "common.h"

namespace {

constexpr int TOPK_MAX_H = 1024;
constexpr int TT_Q = 32;   // queries per workgroup of a tile kernel (one 32-row MFMA tile)
constexpr int TT_N = 128;  // items per tile (4 waves x 32)
constexpr int TT_IDX_NONE = 0x7fffffff;  // "no item" in every (score, index) list; as a rank, XFMR_RANK_NONE
static_assert(TT_IDX_NONE == XFMR_RANK_NONE, "a dead target's item and its rank are the same sentinel");

// ---- shared pieces ------------------------------------------------------------------------------------------------
// best first: score descending, then item index ascending (a total order over distinct items)
__device__ __forceinline__ bool tt_better(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// the scores the tiled search can return and the rank path counts: neither infinity nor NaN
__device__ __forceinline__ bool tt_finite(float s) { return s > -INFINITY && s < INFINITY; }

// 1 - distance; rq = 1 / |q|, qq = |q|^2, rn = 1 / |e| (cosine), ee = |e|^2 (l2)
__device__ __forceinline__ float rk_score(int metric, float dot, float rq, float qq, float rn, float ee) {
  if (metric == XFMR_METRIC_COSINE) return dot * rq * rn;  // 1 - (1 - cos)
  if (metric == XFMR_METRIC_DOT) return dot;                // 1 - (1 - dot)
  return 1.f - (qq - 2.f * dot + ee);                       // 1 - |q - e|^2
}

__device__ __forceinline__ float rk_inv_norm(float qq) { return 1.f / fmaxf(sqrtf(qq), 1e-8f); }

// |q|^2 by 8 threads per query (part = the thread's place among them); every thread of the aligned group gets the value
__device__ __forceinline__ float rk_query_sqnorm(const float* qr, int H, int part) {
  float qq = 0.f;
  for (int h = 4 * part; h < H; h += 32) {
    const float4 v = *reinterpret_cast<const float4*>(qr + h);
    qq = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, qq))));
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) qq += __shfl_xor(qq, o, 64);
  return qq;
}

// Best-first bitonic sort of LISTS lists of len entries each (len a power of two) in LDS, by all 256 threads; ends on a
// barrier. One list: no index division.
template <int LISTS>
__device__ __forceinline__ void tt_sort(float* S, int* I, int len) {
  const int half = len >> 1;
  for (int size = 2; size <= len; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int x = threadIdx.x; x < LISTS * half; x += 256) {
        const int i = LISTS == 1 ? 0 : x / half, p = LISTS == 1 ? x : x % half;
        const int e = 2 * p - (p & (stride - 1)), f = e + stride;
        const bool up = (e & size) == 0;  // "up" blocks hold the better element first
        float* s = S + i * len;
        int* ix = I + i * len;
        const float se = s[e], sf = s[f];
        const int ie = ix[e], jf = ix[f];
        if (tt_better(sf, jf, se, ie) == up) { s[e] = sf; s[f] = se; ix[e] = jf; ix[f] = ie; }
      }
      __syncthreads();
    }
  }
}

// number of entries of the best-first list (s, ix)[0..n) that are better than (v, iv)
__device__ __forceinline__ int tt_count_better(const float* s, const int* ix, int n, float v, int iv) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tt_better(s[mid], ix[mid], v, iv)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// item `it` in the sorted list ex[lo..hi)
__device__ __forceinline__ bool tt_excluded(const int64_t* ex, int64_t lo, int64_t hi, int it) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ex[mid] < it) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && ex[lo] == it;
}

struct ScoreArgs {  // what a score and a slice need: the head of every tile kernel's arguments
  const float* q; const float* table; const float* rnorm; const float* sqnorm; int n_rows; int n_query;
  const int64_t* excl; const int64_t* excl_off;  // CSR of excluded items per query, each row SORTED (may be null)
  int H, metric, splits;
  int64_t slice;  // items per slice, a multiple of TT_N
};

// Query prologue: thread group tid >> 3 gets |q|^2 of query q0 + (tid >> 3); rows past n_query give 0
__device__ __forceinline__ float tile_query_sqnorm(const ScoreArgs& a, int q0) {
  const int i = threadIdx.x >> 3;
  const bool real = q0 + i < a.n_query;
  const float qq = rk_query_sqnorm(a.q + (int64_t)(real ? q0 + i : 0) * a.H, a.H, threadIdx.x & 7);
  return real ? qq : 0.f;
}

// the scalar mirror of the f32 score tile (retrieval.hip: tile_dots): one (query, item) dot product in its k order
__device__ __forceinline__ float rk_chain_dot(const float* sQ, const float* e, int H) {
  float acc = 0.f;
  for (int c = 0; c < H; c += 8) {
    const float4 x0 = *reinterpret_cast<const float4*>(sQ + c), y0 = *reinterpret_cast<const float4*>(e + c);
    float4 x1 = make_float4(0.f, 0.f, 0.f, 0.f), y1 = x1;
    if (c + 4 < H) {
      x1 = *reinterpret_cast<const float4*>(sQ + c + 4);
      y1 = *reinterpret_cast<const float4*>(e + c + 4);
    }
    acc = fmaf(x0.x, y0.x, acc); acc = fmaf(x1.x, y1.x, acc);
    acc = fmaf(x0.y, y0.y, acc); acc = fmaf(x1.y, y1.y, acc);
    acc = fmaf(x0.z, y0.z, acc); acc = fmaf(x1.z, y1.z, acc);
    acc = fmaf(x0.w, y0.w, acc); acc = fmaf(x1.w, y1.w, acc);
  }
  return acc;
}

// an item's own term of the score, fetched when ok
struct ItemTerm { float rn, ee; };
__device__ __forceinline__ ItemTerm rk_item_term(const ScoreArgs& a, int it, bool ok) {
  ItemTerm t = {0.f, 0.f};
  if (ok) {
    if (a.metric == XFMR_METRIC_COSINE) t.rn = a.rnorm[it];
    else if (a.metric == XFMR_METRIC_L2) t.ee = a.sqnorm[it];
  }
  return t;
}

// the tile's score of (query in sQ, item it), bit for bit
__device__ __forceinline__ float rk_item_score(const ScoreArgs& a, const float* sQ, float rq, float qq, int it) {
  const ItemTerm t = rk_item_term(a, it, true);
  return rk_score(a.metric, rk_chain_dot(sQ, a.table + (int64_t)it * a.H, a.H), rq, qq, t.rn, t.ee);
}

// ---- the streaming top-k of the tile kernels ---------------------------------------------------------------------------
constexpr int TT_C = 128;        // candidate list per query (a power of two: tt_sort)
constexpr int TT_KMAX = 128;
constexpr int TT_MAX_SPLITS = 16;
constexpr int TT_TARGET_WG = 512;  // 256 CUs x 2 resident workgroups

// Sorts every query's candidates and merges them into its running list (buffer `cur` -> 1 - cur); new thresholds.
// Called by all threads of the workgroup; returns the new buffer index. k and kp by value: a reference to the kernel's
// arguments would escape wherever the merge is not inlined, and the tile loop's global loads would become flat ones.
__device__ int tt_merge(int k, int kp, float* cS, int* cI, float* lS, int* lI, int cur, int* cnt, float* thrS, int* thrI,
                        int* flag) {
  const int tid = threadIdx.x;
  for (int x = tid; x < TT_Q * TT_C; x += 256) {
    const int i = x / TT_C, e = x % TT_C;
    if (e >= min(cnt[i], TT_C)) { cS[x] = -INFINITY; cI[x] = TT_IDX_NONE; }
  }
  __syncthreads();
  tt_sort<TT_Q>(cS, cI, TT_C);
  // merge path: rank of an entry = its place in its own list + the entries of the other list that are better
  const int nxt = 1 - cur;
  for (int x = tid; x < TT_Q * (kp + TT_C); x += 256) {
    const int i = x / (kp + TT_C), e = x % (kp + TT_C);
    const float* ls = lS + (cur * TT_Q + i) * kp;
    const int* li = lI + (cur * TT_Q + i) * kp;
    const float* cs = cS + i * TT_C;
    const int* ci = cI + i * TT_C;
    float v; int iv, rank;
    if (e < kp) { v = ls[e]; iv = li[e]; rank = e + tt_count_better(cs, ci, TT_C, v, iv); }
    else { v = cs[e - kp]; iv = ci[e - kp]; rank = (e - kp) + tt_count_better(ls, li, kp, v, iv); }
    if (rank < kp) { lS[(nxt * TT_Q + i) * kp + rank] = v; lI[(nxt * TT_Q + i) * kp + rank] = iv; }
  }
  __syncthreads();
  if (tid < TT_Q) {
    thrS[tid] = lS[(nxt * TT_Q + tid) * kp + k - 1];
    thrI[tid] = lI[(nxt * TT_Q + tid) * kp + k - 1];
    cnt[tid] = 0;
  }
  if (tid == 0) *flag = 0;
  __syncthreads();
  return nxt;
}

// ---- host: one plan, one layout, one set of checks ------------------------------------------------------------------
struct TiledPlan {
  int splits; int64_t slice;  // catalogue slices and the items in each (a multiple of TT_N)
  unsigned qtiles;            // query tiles
  dim3 grid() const { return dim3(qtiles, (unsigned)splits); }
};

static TiledPlan tiled_plan(int64_t n_query, int64_t n_rows) {
  const int64_t qtiles = (n_query + TT_Q - 1) / TT_Q;
  const int64_t itiles = (n_rows + TT_N - 1) / TT_N;
  int64_t s = (TT_TARGET_WG + qtiles - 1) / qtiles;
  if (s > TT_MAX_SPLITS) s = TT_MAX_SPLITS;
  if (s > itiles) s = itiles;
  if (s < 1) s = 1;
  TiledPlan p;
  p.slice = ((itiles + s - 1) / s) * TT_N;
  p.splits = (int)((n_rows + p.slice - 1) / p.slice);
  p.qtiles = (unsigned)qtiles;
  return p;
}

static int tiled_kp(int k) {
  int kp = 1;
  while (kp < k) kp <<= 1;
  return kp;
}

static size_t tiled_lds_bytes(int kp) {
  return (size_t)TT_Q * TT_C * 8 + (size_t)2 * TT_Q * kp * 8;
}

// The search entries' common refusals, in their common precedence: EINVAL (pointers, sizes, the exclusion pair, the
// metric, the norm array the metric needs) < EUNSUPPORTED < EALIGN; the workspace size is the caller's, last.
// scan = xfmr_topk: always needs table_rnorm, does not test the query's alignment, puts no bound on n_query.
// own_valid / own_supported: the entry's own pointers and sizes (outputs, k or the targets).
static int search_check(const float* query, const float* table, const float* rnorm, const float* sqnorm, int64_t n_rows,
                        int64_t n_query, int32_t H, const int64_t* excl, const int64_t* excl_off, int32_t metric,
                        const void* workspace, bool scan, bool own_valid, bool own_supported) {
  if (!query || !table || !workspace || !own_valid) return XFMR_EINVAL;
  if (n_rows <= 0 || n_query <= 0 || H <= 0) return XFMR_EINVAL;
  if ((excl == nullptr) != (excl_off == nullptr)) return XFMR_EINVAL;
  if (metric < XFMR_METRIC_COSINE || metric > XFMR_METRIC_L2) return XFMR_EINVAL;
  if ((scan || metric == XFMR_METRIC_COSINE) && !rnorm) return XFMR_EINVAL;
  if (!scan && metric == XFMR_METRIC_L2 && !sqnorm) return XFMR_EINVAL;
  if ((H & 3) || H > TOPK_MAX_H || n_rows >= (1ll << 31) || (!scan && n_query >= (1ll << 31)) || !own_supported)
    return XFMR_EUNSUPPORTED;
  if ((!scan && !xf_aligned16(query)) || !xf_aligned16(table) || !xf_aligned16(workspace)) return XFMR_EALIGN;
  return XFMR_OK;
}

static void fill_score_args(ScoreArgs& a, const float* query, const float* table, const float* rnorm, const float* sqnorm,
                            int64_t n_rows, int64_t n_query, int32_t H, const int64_t* excl, const int64_t* excl_off,
                            int32_t metric, const TiledPlan& p) {
  a.q = query; a.table = table; a.rnorm = rnorm; a.sqnorm = sqnorm; a.n_rows = (int)n_rows; a.n_query = (int)n_query;
  a.excl = excl; a.excl_off = excl_off; a.H = H; a.metric = metric; a.splits = p.splits; a.slice = p.slice;
}

}  // namespace
