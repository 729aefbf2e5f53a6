// Refined item search (include/xfmr_search.h): a bf16 MFMA shortlist, an exact f32 re-rank of it, and a per-query
// certificate that the short answer is xfmr_topk_tiled's answer. DESIGN.md "Refined search" derives the bound.
//
// The reference never scans in full precision: LanceIndex.search runs a compressed first pass and .refine_factor(4)
// re-ranks four times top_k candidates with the full vectors (xfmr_rec/index.py:214-255). Here the first pass is a full
// scan at the bf16 MFMA rate and the second one is the exact search's own arithmetic, so a certified row IS the exact
// search's row, bit for bit. Two launches:
//   coarse_kernel  topk_tiled_kernel's grid (query tiles x catalogue slices) and its streaming top-k (tt_merge, the
//                  candidate lists and the running lists in LDS, k = k_short), with the score tile on
//                  v_mfma_f32_32x32x16_bf16: the workgroup's 32 query rows are rounded to bf16 ONCE into registers (a
//                  lane keeps the A fragments of its row for every k-step), the item rows come from table_bf16 by
//                  16-byte loads straight into B fragments. Up to H = 384 the next tile's fragments are loaded while
//                  this tile's MFMAs and epilogue run (two register images, the loop unrolled by two so that no
//                  image is copied); above, the fragments stream in chunks of 16 k-steps. The epilogue is rk_score on
//                  the f32 query norm and the f32 item terms: coarse and exact scores differ in the dot product only.
//                  A non-finite coarse score of an item in range raises the query's `bad` flag instead of entering
//                  a list.
//   refine_kernel  one workgroup per query: the slices' lists -> tt_sort -> the k_short best = the shortlist; tau =
//                  its last score when the shortlist is full, -inf otherwise; every kept item scored again by
//                  rk_item_score (the exact tile's bits); non-finite scores dropped; tt_sort; the best k leave;
//                  certified = !bad && (shortlist not full || k-th refined score > tau + sr_bound).
// No float atomics; every list is sorted by tt_better before it is used: two calls give the same bits.
#include "retrieval_common.h"
#include "xfmr_search.h"

namespace {

constexpr int SR_KS_PRE = 24;     // k-steps a lane keeps per image in the prefetching form: H <= 384
constexpr int SR_KS_MAX = 64;     // ... of query fragments in the streaming form: H <= 1024
constexpr int SR_CHUNK = 16;      // k-steps per chunk of the streaming form
constexpr int SR_MERGE_MAX = TT_MAX_SPLITS * TT_KMAX;
static_assert(16 * SR_KS_MAX == TOPK_MAX_H, "the streaming form holds a whole query row");

// ---- the bound: |coarse score - exact score| for any item of the query ----------------------------------------------
// DESIGN.md "Refined search". nq = |q| and M = the largest item norm; SR_BETA covers the two bf16 roundings and both f32
// accumulations of a dot product, SR_INFL the f32 errors of nq, M, rq, rn and of this function's own arithmetic, SR_DELTA
// what underflow can add. +inf where an assumption fails (nothing is certified by the bound then).
constexpr float SR_BETA = 0.0078125f + 0.000244140625f;  // 2^-7 + 2^-12
constexpr float SR_INFL = 1.001953125f;                  // 1 + 2^-9
constexpr float SR_DELTA = 8.673617379884035e-19f;       // 2^-60
constexpr float SR_ULPS = 9.5367431640625e-07f;          // 2^-20
constexpr float SR_NORM_MAX = 1099511627776.f;           // 2^40

__host__ __device__ __forceinline__ float sr_bound(int metric, float qq, float max_norm, float max_rnorm) {
  const float nq = sqrtf(qq);
  if (!(qq > 0.f) || !(nq <= SR_NORM_MAX) || !(max_norm >= 0.f) || !(max_norm <= SR_NORM_MAX) || !(max_rnorm >= 0.f) ||
      !(max_rnorm < INFINITY))
    return INFINITY;
  const float d = SR_BETA * SR_INFL * nq * max_norm + SR_DELTA;  // the dot product
  if (metric == XFMR_METRIC_DOT) return d;
  if (metric == XFMR_METRIC_L2) return 2.f * d + SR_ULPS * ((nq + max_norm) * (nq + max_norm) + 1.f);
  return SR_BETA * SR_INFL + SR_ULPS + SR_DELTA * (1.f / fmaxf(nq, 1e-8f)) * max_rnorm * SR_INFL;
}

// ---- the coarse pass ------------------------------------------------------------------------------------------------
struct CoarseArgs : ScoreArgs {
  const __bf16* tb;               // table_bf16
  float* ws_score; int* ws_idx;   // [n_query][splits][k]
  int* ws_bad;                    // [n_query][splits]
  int k, kp;                      // k_short and its power of two
};

__device__ __forceinline__ bf16x8 sr_zero() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
  return z;
}

// the lane's item (accumulator column) of the tile at t0, as retrieval.hip's tile_col: row 0 (padding) and rows past the
// slice are not ok and read row 0
// `term`: the item's own term of the score, fetched HERE, ahead of the tile's fragment loads: the vector-memory counter
// retires in order, so an epilogue that waited for a term issued behind the next tile's fragments would drain them too
struct CoarseCol { bool ok; int j; const __bf16* e; ItemTerm term; };
__device__ __forceinline__ CoarseCol coarse_col(const CoarseArgs& a, int64_t t0, int64_t hi, int w, int lane) {
  const int64_t j64 = t0 + 32 * w + (lane & 31);
  const bool ok = j64 >= 1 && j64 < hi;
  const int j = ok ? (int)j64 : 0;
  return {ok, j, a.tb + (int64_t)j * a.H + 8 * (lane >> 5), rk_item_term(a, j, ok)};
}

// N k-steps of the lane's item row from e (the lane half's offset folded in): lane half h2 of step s holds dims
// 16 s + 8 h2 .. + 7, zeros past Hrem (H is a multiple of 8: a fragment is inside the row or not read at all)
template <int N>
__device__ __forceinline__ void sr_load(bf16x8 (&v)[N], const __bf16* e, int Hrem, int h2) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    v[s] = sr_zero();
    if (16 * s + 8 * h2 < Hrem) v[s] = *reinterpret_cast<const bf16x8*>(e + 16 * s);
  }
}

template <int KS, bool PRE>
__global__ __launch_bounds__(256) void coarse_kernel(CoarseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sr_lds[];
  __shared__ float sQQ[TT_Q], sRQ[TT_Q], thrS[TT_Q];
  __shared__ int thrI[TT_Q], cnt[TT_Q], bad[TT_Q], flag;
  float* cS = reinterpret_cast<float*>(sr_lds);
  int* cI = reinterpret_cast<int*>(cS + TT_Q * TT_C);
  float* lS = reinterpret_cast<float*>(cI + TT_Q * TT_C);
  int* lI = reinterpret_cast<int*>(lS + 2 * TT_Q * a.kp);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h2 = lane >> 5;
  const int H = a.H;
  const int q0 = blockIdx.x * TT_Q;
  const int split = blockIdx.y;
  const int64_t lo = split * a.slice;
  const int64_t hi = lo + a.slice < a.n_rows ? lo + a.slice : a.n_rows;
  const float qq = tile_query_sqnorm(a, q0);
  if ((tid & 7) == 0) {
    const int i = tid >> 3;
    sQQ[i] = qq;
    sRQ[i] = rk_inv_norm(qq);
    thrS[i] = -INFINITY;
    thrI[i] = TT_IDX_NONE;
    cnt[i] = 0;
    bad[i] = 0;
  }
  for (int x = tid; x < TT_Q * a.kp; x += 256) { lS[x] = -INFINITY; lI[x] = TT_IDX_NONE; }
  if (tid == 0) flag = 0;
  // the lane's query row (rows past n_query read the last query and are masked by the epilogue), rounded to bf16
  bf16x8 qf[KS];
  {
    const float* qr = a.q + (int64_t)min(q0 + (lane & 31), a.n_query - 1) * H + 8 * h2;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = sr_zero();
      if (16 * s + 8 * h2 < H) {
        const float4 x = *reinterpret_cast<const float4*>(qr + 16 * s);
        const float4 y = *reinterpret_cast<const float4*>(qr + 16 * s + 4);
        qf[s][0] = (__bf16)x.x; qf[s][1] = (__bf16)x.y; qf[s][2] = (__bf16)x.z; qf[s][3] = (__bf16)x.w;
        qf[s][4] = (__bf16)y.x; qf[s][5] = (__bf16)y.y; qf[s][6] = (__bf16)y.z; qf[s][7] = (__bf16)y.w;
      }
    }
  }
  __syncthreads();
  int cur = 0;

  // the epilogue of one score tile: scores, masks, threshold, candidates (topk_tiled_kernel's, plus the bad flag)
  auto offer = [&](const f32x16& acc, const CoarseCol& col) {
    const int j = col.j;
    const ItemTerm term = col.term;
    float sc[16];
    unsigned pending = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = xf_acc_row(r, lane);
      const float s = rk_score(a.metric, acc[r], sRQ[i], sQQ[i], term.rn, term.ee);
      sc[r] = s;
      if (col.ok && q0 + i < a.n_query) {
        if (tt_finite(s)) pending |= 1u << r;
        else bad[i] = 1;  // (excluded or not: pessimistic at worst)
      }
    }
    while (true) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!((pending >> r) & 1u)) continue;
        const int i = xf_acc_row(r, lane);
        bool drop = !tt_better(sc[r], j, thrS[i], thrI[i]);
        if (!drop && a.excl) drop = tt_excluded(a.excl, a.excl_off[q0 + i], a.excl_off[q0 + i + 1], j);
        if (!drop) {
          const int pos = atomicAdd(&cnt[i], 1);
          if (pos < TT_C) { cS[i * TT_C + pos] = sc[r]; cI[i * TT_C + pos] = j; }
          else { flag = 1; continue; }  // list full: offered again after the merge
        }
        pending &= ~(1u << r);
      }
      __syncthreads();
      if (!flag) break;
      __syncthreads();
      cur = tt_merge(a.k, a.kp, cS, cI, lS, lI, cur, cnt, thrS, thrI, &flag);
    }
  };

  if constexpr (PRE) {
    // two register images of a tile's item fragments: while one is multiplied, the other is in flight
    auto dots = [&](const bf16x8 (&v)[KS]) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (16 * s < H) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[s], v[s], acc, 0, 0, 0);
      }
      return acc;
    };
    bf16x8 va[KS], vb[KS];
    CoarseCol ca = coarse_col(a, lo, hi, w, lane), cb = ca;
    sr_load<KS>(va, ca.e, H, h2);
    for (int64_t t0 = lo; t0 < hi; t0 += 2 * TT_N) {
      const bool more = t0 + TT_N < hi;
      if (more) {
        cb = coarse_col(a, t0 + TT_N, hi, w, lane);
        sr_load<KS>(vb, cb.e, H, h2);
      }
      offer(dots(va), ca);
      if (!more) break;
      if (t0 + 2 * TT_N < hi) {
        ca = coarse_col(a, t0 + 2 * TT_N, hi, w, lane);
        sr_load<KS>(va, ca.e, H, h2);
      }
      offer(dots(vb), cb);
    }
  } else {
    for (int64_t t0 = lo; t0 < hi; t0 += TT_N) {
      const CoarseCol col = coarse_col(a, t0, hi, w, lane);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < KS; c += SR_CHUNK) {
        if (16 * c < H) {
          bf16x8 v[SR_CHUNK];
          sr_load<SR_CHUNK>(v, col.e + 16 * c, H - 16 * c, h2);
#pragma unroll
          for (int s = 0; s < SR_CHUNK; ++s) {
            if (16 * (c + s) < H) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[c + s], v[s], acc, 0, 0, 0);
          }
        }
      }
      offer(acc, col);
    }
  }
  cur = tt_merge(a.k, a.kp, cS, cI, lS, lI, cur, cnt, thrS, thrI, &flag);
  for (int x = tid; x < TT_Q * a.k; x += 256) {
    const int i = x / a.k, e = x % a.k;
    if (q0 + i >= a.n_query) continue;
    const int64_t o = ((int64_t)(q0 + i) * a.splits + split) * a.k + e;
    a.ws_score[o] = lS[(cur * TT_Q + i) * a.kp + e];
    a.ws_idx[o] = lI[(cur * TT_Q + i) * a.kp + e];
  }
  if (tid < TT_Q && q0 + tid < a.n_query) a.ws_bad[(int64_t)(q0 + tid) * a.splits + split] = bad[tid];
}

// ---- shortlist, refine, certificate ---------------------------------------------------------------------------------
struct RefineArgs : ScoreArgs {
  const float* ws_score; const int* ws_idx; const int* ws_bad;
  int k, ks;  // top_k and k_short
  float max_norm, max_rnorm;
  int64_t* out_idx; float* out_score; uint8_t* out_cert;
};

__global__ __launch_bounds__(256) void refine_kernel(RefineArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TOPK_MAX_H];
  __shared__ float sS[SR_MERGE_MAX];
  __shared__ int sI[SR_MERGE_MAX];
  __shared__ int sBad;
  const int tid = threadIdx.x, H = a.H;
  const int64_t qi = blockIdx.x;
  const float* qr = a.q + qi * H;
  for (int h = tid; h < H; h += 256) sQ[h] = qr[h];
  const float qq = rk_query_sqnorm(qr, H, tid & 7);
  const float rq = rk_inv_norm(qq);
  const int n = a.splits * a.ks;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int x = tid; x < np2; x += 256) {
    if (x < n) { sS[x] = a.ws_score[qi * n + x]; sI[x] = a.ws_idx[qi * n + x]; }
    else { sS[x] = -INFINITY; sI[x] = TT_IDX_NONE; }
  }
  if (tid == 0) sBad = 0;
  __syncthreads();
  if (tid < a.splits && a.ws_bad[qi * a.splits + tid]) sBad = 1;
  tt_sort<1>(sS, sI, np2);
  __syncthreads();  // (a list of one entry is sorted without a barrier)
  // the shortlist: the ks best coarse pairs; full = some eligible item may have been left out, none scores above tau
  const bool full = sI[a.ks - 1] != TT_IDX_NONE;
  const float tau = full ? sS[a.ks - 1] : -INFINITY;
  const bool any_bad = sBad != 0;
  float s = -INFINITY;
  int it = TT_IDX_NONE;
  if (tid < a.ks && sI[tid] != TT_IDX_NONE) {
    const float v = rk_item_score(a, sQ, rq, qq, sI[tid]);
    if (tt_finite(v)) { s = v; it = sI[tid]; }
  }
  __syncthreads();
  int kp = 1;
  while (kp < a.ks) kp <<= 1;
  if (tid < kp) { sS[tid] = s; sI[tid] = it; }  // (ks <= 128 <= the workgroup: threads ks .. kp - 1 hold the padding)
  __syncthreads();
  tt_sort<1>(sS, sI, kp);
  for (int e = tid; e < a.k; e += 256) {
    const bool real = sI[e] != TT_IDX_NONE;
    a.out_idx[qi * a.k + e] = real ? (int64_t)sI[e] : -1;
    a.out_score[qi * a.k + e] = real ? sS[e] : -INFINITY;
  }
  if (tid == 0) {
    const float sk = sI[a.k - 1] != TT_IDX_NONE ? sS[a.k - 1] : -INFINITY;
    const bool proven = !full || sk > tau + sr_bound(a.metric, qq, a.max_norm, a.max_rnorm);
    a.out_cert[qi] = (!any_bad && proven) ? 1 : 0;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static int sr_k_short(int k, int refine_factor) {
  const int64_t want = (int64_t)k * refine_factor;
  const int ks = (int)(want < TT_KMAX ? want : TT_KMAX);
  return ks < k ? k : ks;
}

static bool sr_prefetches(int H) { return H <= 16 * SR_KS_PRE; }

// the workspace, in 4-byte words: the slices' scores, their items, the bad flags
struct SearchWs { size_t score, idx, bad, end; };
static SearchWs search_ws(int64_t n_query, int splits, int ks) {
  const size_t n = (size_t)n_query * (size_t)splits * (size_t)ks;
  return {0, n, 2 * n, 2 * n + (size_t)n_query * (size_t)splits};
}

template <int KS, bool PRE>
static int launch_coarse(const CoarseArgs& a, const TiledPlan& p, size_t lds, hipStream_t stream) {
  if (hipFuncSetAttribute((const void*)coarse_kernel<KS, PRE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return XFMR_EHIP;
  hipLaunchKernelGGL((coarse_kernel<KS, PRE>), p.grid(), dim3(256), lds, stream, a);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // namespace

extern "C" {

size_t xfmr_search_refined_workspace(int64_t n_query, int64_t n_rows, int32_t k_short) {
  if (n_query <= 0 || n_rows <= 0 || k_short <= 0) return 0;
  return search_ws(n_query, tiled_plan(n_query, n_rows).splits, k_short).end * sizeof(int);
}

int xfmr_search_refined_plan(int64_t n_query, int64_t n_rows, int32_t H, int32_t k, int32_t refine_factor, int32_t out[8]) {
  if (!out || n_query <= 0 || n_rows <= 0 || H <= 0 || k <= 0 || refine_factor <= 0) return XFMR_EINVAL;
  if ((H & 7) || H > TOPK_MAX_H || n_rows >= (1ll << 31) || n_query >= (1ll << 31) || k > TT_KMAX) return XFMR_EUNSUPPORTED;
  const TiledPlan p = tiled_plan(n_query, n_rows);
  const int ks = sr_k_short(k, refine_factor), kp = tiled_kp(ks);
  out[0] = TT_Q; out[1] = TT_N; out[2] = p.splits; out[3] = (int32_t)p.slice; out[4] = (int32_t)tiled_lds_bytes(kp);
  out[5] = ks; out[6] = kp; out[7] = sr_prefetches(H) ? SR_KS_PRE : SR_KS_MAX;
  return XFMR_OK;
}

int xfmr_search_refined(const float* query, const float* table, const void* table_bf16, const float* table_rnorm,
                        const float* table_sqnorm, float table_max_norm, float table_max_rnorm, int64_t n_rows,
                        int64_t n_query, int32_t H, const int64_t* exclude, const int64_t* exclude_offsets, int32_t k,
                        int32_t k_short, int32_t metric, int64_t* out_idx, float* out_score, uint8_t* out_certified,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const bool own = table_bf16 && out_idx && out_score && out_certified && k > 0 && k_short >= k;
  const int rc = search_check(query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric,
                              workspace, false, own, k_short <= TT_KMAX && !(H & 7));
  if (rc != XFMR_OK) return rc;
  if (!xf_aligned16(table_bf16)) return XFMR_EALIGN;
  if (workspace_bytes < xfmr_search_refined_workspace(n_query, n_rows, k_short)) return XFMR_EWORKSPACE;
  const TiledPlan p = tiled_plan(n_query, n_rows);
  const SearchWs ws = search_ws(n_query, p.splits, k_short);
  int* wsp = (int*)workspace;
  CoarseArgs c{};
  fill_score_args(c, query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric, p);
  c.tb = (const __bf16*)table_bf16;
  c.ws_score = (float*)(wsp + ws.score); c.ws_idx = wsp + ws.idx; c.ws_bad = wsp + ws.bad;
  c.k = k_short; c.kp = tiled_kp(k_short);
  const size_t lds = tiled_lds_bytes(c.kp);
  const int lrc = sr_prefetches(H) ? launch_coarse<SR_KS_PRE, true>(c, p, lds, (hipStream_t)stream)
                                   : launch_coarse<SR_KS_MAX, false>(c, p, lds, (hipStream_t)stream);
  if (lrc != XFMR_OK) return lrc;
  RefineArgs r{};
  fill_score_args(r, query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric, p);
  r.ws_score = c.ws_score; r.ws_idx = c.ws_idx; r.ws_bad = c.ws_bad; r.k = k; r.ks = k_short;
  r.max_norm = table_max_norm; r.max_rnorm = table_max_rnorm;
  r.out_idx = out_idx; r.out_score = out_score; r.out_cert = out_certified;
  hipLaunchKernelGGL(refine_kernel, dim3((unsigned)n_query), dim3(256), 0, (hipStream_t)stream, r);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // extern "C"
