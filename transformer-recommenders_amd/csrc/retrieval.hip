// Exact top-k retrieval + ranking metrics for the validation path.
//
// The reference validates one user at a time: encode(history) -> LanceDB IVF_HNSW_PQ search over the item embeddings
// with the history prefiltered out -> top_k ids -> seven torchmetrics retrieval metrics on a synthesised score vector
// (xfmr_rec/trainer.py:186-211, 266-325; index.py:214-255; metrics.py:17-79). Here a batch of users is scored EXACTLY
// against the whole table (the ANN's limit of full probing): a scan for one query (xfmr_topk), score tiles on the matrix
// cores for a user set (xfmr_topk_tiled), or every target's exact rank with no list at all (xfmr_target_ranks); the seven
// metrics come from a ranked list or from the ranks. xfmr_candidate_ranks ranks the targets among a GIVEN candidate list
// instead (the sampled-candidate protocol, re-ranking) under the same rules. Each section below describes its kernels.
// The contract between the paths: a target's rank is its place in the tiled list, the score the rank pre-pass reports is
// the list's score bit for bit, and the rank metrics are the list metrics bit for bit. It holds because each piece is
// written ONCE: the order (tt_better), the eligibility test (tt_finite), the score formula (rk_score), the query norm
// (rk_query_sqnorm), the 32 x 32 score tile (tile_* and its scalar mirror rk_chain_dot), the sort (tt_sort) and the
// metrics arithmetic (ms_*). The pieces that the refined search (search.hip) needs too are in retrieval_common.h.
// metric: cosine (reference default, index.py:47), dot, or l2; score = 1 - distance as index.py:248-251 appends it.
#include "retrieval_common.h"

namespace {

constexpr int TOPK_MAX = 1024;

// ---- the 32 x 32 score tile of the tiled search and the rank path ---------------------------------------------------
// A workgroup owns TT_Q queries and one slice of the catalogue; wave w scores the 32 items t0 + 32 w + (lane & 31) of
// every TT_N-item tile against the 32 queries with v_mfma_f32_32x32x2_f32 -- exact f32, bit for bit a k-ordered fmaf
// chain. Operands come straight from global memory, not through LDS: the 32 query rows are shared by the four waves (L1
// hits), every item row is read by one wave once per query tile, and the f32 MFMA rate (64 FLOP/clk/SIMD) needs only
// 16 B/clk per CU of item rows. (ScoreArgs, the query prologue and the scalar mirror: retrieval_common.h.)

// the lane's query row (accumulator row block; rows past n_query read the last query and are masked by the epilogues)
__device__ __forceinline__ const float* tile_query_ptr(const ScoreArgs& a, int q0, int lane) {
  return a.q + (int64_t)min(q0 + (lane & 31), a.n_query - 1) * a.H + 4 * (lane >> 5);
}

// the lane's item (accumulator column) of the tile at t0: row 0 (padding) and rows past the slice are not ok and read row 0
struct TileCol { bool ok; int j; const float* e; };
__device__ __forceinline__ TileCol tile_col(const ScoreArgs& a, int64_t t0, int64_t hi, int w, int lane) {
  const int64_t j64 = t0 + 32 * w + (lane & 31);
  const bool ok = j64 >= 1 && j64 < hi;
  const int j = ok ? (int)j64 : 0;
  return {ok, j, a.table + (int64_t)j * a.H + 4 * (lane >> 5)};
}

// k-step order, tile and mirror alike: chunk c = 0, 8, ... takes four MFMAs, one per float4 component; in each, lane
// half 0 supplies dim c + component and lane half 1 dim c + 4 + component (zeros past H), and k = 0 is added before
// k = 1. So a dot product is the fmaf chain over dims c + {0, 4, 1, 5, 2, 6, 3, 7}. Change both or neither.
__device__ __forceinline__ f32x16 tile_dots(const float* qa, const float* eb, int H, int h2) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
  for (int c = 0; c < H; c += 8, qa += 8, eb += 8) {  // (bumped pointers: the lane half's offset stays folded in them)
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (c + 4 * h2 < H) {
      x = *reinterpret_cast<const float4*>(qa);
      y = *reinterpret_cast<const float4*>(eb);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
  }
  return acc;
}

// ---- scan top-k (xfmr_topk) -------------------------------------------------------------------------------------------
// One workgroup per query: scores for every item (16 lanes per item, 16-byte pieces) into an n_query x n_rows
// workspace, the query's history and the padding row masked out, the k-th largest score by a 4-pass radix select,
// ordered compaction (ties: lower item index first), tt_sort of the k survivors. The right kernel for ONE query (a
// single query would fill one row of a 32-row MFMA tile) and the wrong one for a user set (6 040 users x a 6 MB table =
// 36 GB of table reads). Its scores differ from the tile's in summation order only.
struct TopkArgs {
  const float* q; const float* table; const float* rnorm; int64_t n_rows;
  const int64_t* excl; const int64_t* excl_off;  // CSR of excluded item indices per query (may be null)
  float* scores;                                 // [B][n_rows] scratch
  int64_t* out_idx; float* out_score;
  int H, k, metric;
};

__device__ __forceinline__ unsigned key_of(float f) {
  const unsigned b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// The scan admits a +inf score and rejects only -inf (its own mask) and NaN, where tt_finite rejects all three: that is
// this entry's behaviour since its first version and stays.
__device__ __forceinline__ bool scan_admits(float s) { return s > -INFINITY; }

__global__ __launch_bounds__(256) void topk_kernel(TopkArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TOPK_MAX_H];
  __shared__ unsigned hist[256];
  __shared__ int sh[4], wcnt[4], weq[4];
  __shared__ float sScore[TOPK_MAX];
  __shared__ int sIdx[TOPK_MAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t qi = blockIdx.x;
  const int H = a.H;
  const int64_t V = a.n_rows;
  float* sc = a.scores + qi * V;
  float qq = 0.f;
  for (int h = tid; h < H; h += 256) {
    const float v = a.q[qi * H + h];
    sQ[h] = v;
    qq += v * v;
  }
  qq = xf_wave_sum(qq);
  if (lane == 0) sh[w] = __float_as_int(qq);
  __syncthreads();
  qq = __int_as_float(sh[0]) + __int_as_float(sh[1]) + __int_as_float(sh[2]) + __int_as_float(sh[3]);
  const float rq = rk_inv_norm(qq);
  __syncthreads();
  // ---- scores ------------------------------------------------------------------------------------------------
  {
    const int g = tid >> 4, j = tid & 15;
    for (int64_t it = g; it < V; it += 16) {
      const float* e = a.table + it * H;
      float dot = 0.f, ee = 0.f;
      for (int h = 4 * j; h < H; h += 64) {
        const float4 x = *reinterpret_cast<const float4*>(e + h);
        const float4 y = *reinterpret_cast<const float4*>(sQ + h);
        dot = fmaf(x.x, y.x, fmaf(x.y, y.y, fmaf(x.z, y.z, fmaf(x.w, y.w, dot))));
        ee = fmaf(x.x, x.x, fmaf(x.y, x.y, fmaf(x.z, x.z, fmaf(x.w, x.w, ee))));
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        dot += __shfl_xor(dot, o, 64);
        ee += __shfl_xor(ee, o, 64);
      }
      if (j == 0) {
        const float rn = a.metric == XFMR_METRIC_COSINE ? a.rnorm[it] : 0.f;
        sc[it] = it == 0 ? -INFINITY : rk_score(a.metric, dot, rq, qq, rn, ee);  // row 0 is the padding item
      }
    }
  }
  __syncthreads();
  if (a.excl) {
    for (int64_t x = a.excl_off[qi] + tid; x < a.excl_off[qi + 1]; x += 256) {
      const int64_t it = a.excl[x];
      if (it >= 0 && it < V) sc[it] = -INFINITY;
    }
  }
  __syncthreads();
  // ---- k-th largest admitted score: 4-pass radix select -----------------------------------------------------------
  if (tid == 0) sh[3] = 0;
  __syncthreads();
  {
    int n = 0;
    for (int64_t it = tid; it < V; it += 256) n += scan_admits(sc[it]) ? 1 : 0;
    if (n) atomicAdd(&sh[3], n);
  }
  __syncthreads();
  const int avail = sh[3];
  const int k = a.k < avail ? a.k : avail;
  unsigned T = 0;
  int need = 0;
  if (avail > a.k) {
    unsigned prefix = 0;
    need = a.k;
    for (int p = 3; p >= 0; --p) {
      hist[tid] = 0;
      __syncthreads();
      const int shift = 8 * p;
      for (int64_t it = tid; it < V; it += 256) {
        const float v = sc[it];
        if (!scan_admits(v)) continue;
        const unsigned key = key_of(v);
        if (p == 3 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        int cum = 0, d = 255;
        for (; d > 0; --d) {
          if (cum + (int)hist[d] >= need) break;
          cum += (int)hist[d];
        }
        sh[0] = d; sh[1] = need - cum;
      }
      __syncthreads();
      prefix |= (unsigned)sh[0] << shift;
      need = sh[1];
      __syncthreads();
    }
    T = prefix;  // take every key > T and the first `need` (by item index) of the keys == T
  }
  // ---- ordered compaction of the survivors ------------------------------------------------------------------------
  if (tid == 0) { sh[0] = 0; sh[1] = 0; }
  __syncthreads();
  for (int64_t i0 = 0; i0 < V; i0 += 256) {
    const int64_t it = i0 + tid;
    bool gt = false, eq = false;
    float v = -INFINITY;
    if (it < V) {
      v = sc[it];
      if (scan_admits(v)) {
        if (avail <= a.k) gt = true;
        else {
          const unsigned key = key_of(v);
          gt = key > T;
          eq = key == T;
        }
      }
    }
    const unsigned long long beq = __ballot(eq);
    if (lane == 0) weq[w] = __popcll(beq);
    __syncthreads();
    int eq_before = sh[1];
    for (int x = 0; x < w; ++x) eq_before += weq[x];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    eq_before += __popcll(beq & below);
    const bool take = gt || (eq && eq_before < need);
    const unsigned long long bt = __ballot(take);
    if (lane == 0) wcnt[w] = __popcll(bt);
    __syncthreads();
    int at = sh[0];
    for (int x = 0; x < w; ++x) at += wcnt[x];
    at += __popcll(bt & below);
    if (take && at < TOPK_MAX) { sScore[at] = v; sIdx[at] = (int)it; }
    __syncthreads();
    if (tid == 0) {
      sh[0] += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      sh[1] += weq[0] + weq[1] + weq[2] + weq[3];
    }
    __syncthreads();
  }
  // ---- the survivors, best first ------------------------------------------------------------------------------------
  int np2 = 1;
  while (np2 < k) np2 <<= 1;
  for (int i = k + tid; i < np2; i += 256) { sScore[i] = -INFINITY; sIdx[i] = TT_IDX_NONE; }
  __syncthreads();
  tt_sort<1>(sScore, sIdx, np2);
  for (int i = tid; i < a.k; i += 256) {
    a.out_idx[qi * a.k + i] = i < k ? (int64_t)sIdx[i] : -1;  // fewer than k candidates: padded like metrics.py:61-64
    a.out_score[qi * a.k + i] = i < k ? sScore[i] : -INFINITY;
  }
}

// ---- tiled top-k: score tiles and a streaming top-k (xfmr_topk_tiled) ------------------------------------------------
// topk_tiled_kernel: per score tile, the epilogue masks row 0, rows past the slice and scores that are not tt_finite,
// and keeps a per-query threshold (the current k-th best). Only scores that beat it are checked against the query's
// exclusion list (binary search) and appended to an LDS candidate list; when a list fills, or at the end of the slice,
// the candidates are sorted and merged into the running top-k. A tile whose candidates overflowed a list is re-offered
// after the merge (against the new threshold). 32 queries per workgroup rather than 64 because each query's candidate
// list and running top-k (double-buffered) live in LDS: 96 KB at k = 128.
// grid = (query tiles, slices), slices chosen so that the grid covers the chip (tiled_plan); topk_merge_kernel then
// merges each query's per-slice lists into the final sorted k. Scratch: n_query x slices x k (score, index) pairs, no
// per-(query, item) workspace. No float atomics: the candidate order inside a list depends on LDS atomics, the result
// does not (every list is sorted by tt_better), so runs are bit-identical.

struct TiledArgs : ScoreArgs {
  float* ws_score; int* ws_idx;  // [n_query][splits][k]
  int k, kp;
};

__global__ __launch_bounds__(256) void topk_tiled_kernel(TiledArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tt_lds[];
  __shared__ float sQQ[TT_Q], sRQ[TT_Q], thrS[TT_Q];
  __shared__ int thrI[TT_Q], cnt[TT_Q], flag;
  float* cS = reinterpret_cast<float*>(tt_lds);
  int* cI = reinterpret_cast<int*>(cS + TT_Q * TT_C);
  float* lS = reinterpret_cast<float*>(cI + TT_Q * TT_C);
  int* lI = reinterpret_cast<int*>(lS + 2 * TT_Q * a.kp);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
  }
  for (int x = tid; x < TT_Q * a.kp; x += 256) { lS[x] = -INFINITY; lI[x] = TT_IDX_NONE; }
  if (tid == 0) flag = 0;
  __syncthreads();
  int cur = 0;
  const float* qa = tile_query_ptr(a, q0, lane);
  for (int64_t t0 = lo; t0 < hi; t0 += TT_N) {
    const TileCol col = tile_col(a, t0, hi, w, lane);
    const int j = col.j;
    const f32x16 acc = tile_dots(qa, col.e, a.H, lane >> 5);
    // ---- epilogue: scores, masks, threshold, candidates ------------------------------------------------------------
    const ItemTerm term = rk_item_term(a, j, col.ok);
    float sc[16];
    unsigned pending = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = xf_acc_row(r, lane);
      const float s = rk_score(a.metric, acc[r], sRQ[i], sQQ[i], term.rn, term.ee);
      sc[r] = s;
      if (col.ok && q0 + i < a.n_query && tt_finite(s)) pending |= 1u << r;
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
  }
  cur = tt_merge(a.k, a.kp, cS, cI, lS, lI, cur, cnt, thrS, thrI, &flag);
  for (int x = tid; x < TT_Q * a.k; x += 256) {
    const int i = x / a.k, e = x % a.k;
    if (q0 + i >= a.n_query) continue;
    const int64_t o = ((int64_t)(q0 + i) * a.splits + split) * a.k + e;
    a.ws_score[o] = lS[(cur * TT_Q + i) * a.kp + e];
    a.ws_idx[o] = lI[(cur * TT_Q + i) * a.kp + e];
  }
}

// one workgroup per query: the query's splits x k (score, index) pairs -> tt_sort -> the best k
constexpr int TT_MERGE_MAX = TT_MAX_SPLITS * TT_KMAX;
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* ws_score, const int* ws_idx, int splits, int k,
                                                         int64_t* out_idx, float* out_score) {
  __shared__ float sS[TT_MERGE_MAX];
  __shared__ int sI[TT_MERGE_MAX];
  const int tid = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const int n = splits * k;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int x = tid; x < np2; x += 256) {
    if (x < n) { sS[x] = ws_score[qi * n + x]; sI[x] = ws_idx[qi * n + x]; }
    else { sS[x] = -INFINITY; sI[x] = TT_IDX_NONE; }
  }
  __syncthreads();
  tt_sort<1>(sS, sI, np2);
  for (int e = tid; e < k; e += 256) {
    const bool real = sI[e] != TT_IDX_NONE;  // (only finite scores ever enter a list)
    out_idx[qi * k + e] = real ? (int64_t)sI[e] : -1;
    out_score[qi * k + e] = real ? sS[e] : -INFINITY;
  }
}

// squared row norms for the l2 metric, one wave per row
__global__ __launch_bounds__(256) void table_sqnorm_kernel(const float* table, float* out, int64_t n_rows, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  float s = 0.f;
  for (int c = lane; c < H; c += 64) {
    const float v = table[row * H + c];
    s += v * v;
  }
  s = xf_wave_sum(s);
  if (lane == 0) out[row] = s;
}

// ---- full-catalogue target ranks (xfmr_target_ranks) -------------------------------------------------------------------
// Every one of the seven metrics is a function of the ranks of a row's distinct targets among the eligible items and of
// the number of distinct targets: no ranked list is needed, so no cutoff limit either. An item is ELIGIBLE for a query
// when it is in [1, n_rows), not in the query's exclusion list and its score is tt_finite (what topk_tiled_kernel can
// return); rank(t) = 1 + the eligible items that are tt_better than t. Three launches:
//   rank_prep_kernel    one workgroup per query. The scores of the query's targets (rk_item_score); the best-first
//                       order of the targets (a count per entry, ties between repeats by entry order; targets that
//                       are not eligible go last and are "dead"); and a histogram of the query's distinct, in-range
//                       excluded items with a finite score, binned by how many live targets beat them.
//   rank_tile_kernel    topk_tiled_kernel's grid and score tile. The epilogue bins every unmasked (query, item) by b =
//                       the live targets of the query that beat the item (one comparison against the worst target:
//                       most items end there; else a binary search over the sorted targets in LDS) with an integer
//                       LDS atomic. No exclusion lookup: excluded items are counted in here and taken out by the prep
//                       histogram. RK_T live targets per pass; a tile whose rows have more passes over its slice
//                       again for the next RK_T.
//   rank_finish_kernel  per query: slices added in index order and prefix-summed over b within each pass, the excluded
//                       items prefix-summed over the whole list. The m-th best live target t_m is beaten by exactly the
//                       counted items of its pass with b <= m, less itself and less the excluded ones with b <= m:
//                       rank = (sum_{b <= m} hist[b]) - 1 - (sum_{b <= m} exb[b]) + 1.
// Integer counts only: two calls give the same bits.
constexpr int RK_T = 128;

struct RankArgs : ScoreArgs {
  const int64_t* tgt; const int64_t* tgt_off;
  // workspace (RankWs), indexed by CSR entry relative to tgt_off[0]
  float* tS; int* tI;  // entry order: score and item (-inf, TT_IDX_NONE: dead)
  float* sS; int* sI;  // each query's entries best first
  int* pos;            // an entry's place in that order
  int* exb;            // per place: excluded items in bin b; after the finish, the ranks by place
  int* nlive;          // [n_query]
  int* hist;           // [splits][n_targets]
  int* out_rank; float* out_tscore;
  int64_t n_targets;
};

__global__ __launch_bounds__(256) void rank_prep_kernel(RankArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TOPK_MAX_H];
  __shared__ int sLive;
  const int tid = threadIdx.x, H = a.H;
  const int qi = blockIdx.x;
  const float* qr = a.q + (int64_t)qi * H;
  for (int h = tid; h < H; h += 256) sQ[h] = qr[h];
  const float qq = rk_query_sqnorm(qr, H, tid & 7);
  const float rq = rk_inv_norm(qq);
  const int64_t base = a.tgt_off[0];
  const int64_t e0 = a.tgt_off[qi] - base, e1 = a.tgt_off[qi + 1] - base;
  const int64_t x0 = a.excl ? a.excl_off[qi] : 0, x1 = a.excl ? a.excl_off[qi + 1] : 0;
  if (tid == 0) sLive = 0;
  __syncthreads();
  // ---- the targets' scores ------------------------------------------------------------------------------------
  int live = 0;
  for (int64_t e = e0 + tid; e < e1; e += 256) {
    const int64_t t = a.tgt[base + e];
    float s = -INFINITY;
    int it = TT_IDX_NONE;
    if (t >= 1 && t < a.n_rows && !(a.excl && tt_excluded(a.excl, x0, x1, (int)t))) {
      const float v = rk_item_score(a, sQ, rq, qq, (int)t);
      if (tt_finite(v)) { s = v; it = (int)t; ++live; }
    }
    a.tS[e] = s;
    a.tI[e] = it;
    a.exb[e] = 0;
    if (a.out_tscore) a.out_tscore[base + e] = s;
  }
  if (live) atomicAdd(&sLive, live);
  __syncthreads();
  const int nl = sLive;
  if (tid == 0) a.nlive[qi] = nl;
  // ---- best-first order: an entry's place = the entries that go before it ----------------------------------------
  for (int64_t e = e0 + tid; e < e1; e += 256) {
    const float s = a.tS[e];
    const int it = a.tI[e];
    int p = 0;
    for (int64_t f = e0; f < e1; ++f) {
      const float sf = a.tS[f];
      const int jf = a.tI[f];
      p += (tt_better(sf, jf, s, it) || (sf == s && jf == it && f < e)) ? 1 : 0;
    }
    a.pos[e] = p;
    a.sS[e0 + p] = s;
    a.sI[e0 + p] = it;
  }
  __syncthreads();
  // ---- the excluded items that the tile pass will count: bin b = the live targets that beat them ------------------
  if (a.excl && nl > 0) {
    for (int64_t x = x0 + tid; x < x1; x += 256) {
      const int64_t it = a.excl[x];
      if (it < 1 || it >= a.n_rows || (x > x0 && a.excl[x - 1] == it)) continue;
      const float v = rk_item_score(a, sQ, rq, qq, (int)it);
      if (!tt_finite(v)) continue;
      const int b = tt_count_better(a.sS + e0, a.sI + e0, nl, v, (int)it);
      if (b < nl) atomicAdd(&a.exb[e0 + b], 1);
    }
  }
}

__global__ __launch_bounds__(256) void rank_tile_kernel(RankArgs a) {
  __shared__ float sQQ[TT_Q], sRQ[TT_Q];
  __shared__ int sLive[TT_Q], sN[TT_Q];
  __shared__ int64_t sE0[TT_Q];
  __shared__ float tS[TT_Q * RK_T];
  __shared__ int tI[TT_Q * RK_T], hist[TT_Q * RK_T];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * TT_Q;
  const int split = blockIdx.y;
  const int64_t lo = split * a.slice;
  const int64_t hi = lo + a.slice < a.n_rows ? lo + a.slice : a.n_rows;
  const float qq = tile_query_sqnorm(a, q0);
  if ((tid & 7) == 0) {
    const int i = tid >> 3;
    const bool real = q0 + i < a.n_query;
    sQQ[i] = qq;
    sRQ[i] = rk_inv_norm(qq);
    sLive[i] = real ? a.nlive[q0 + i] : 0;
    sE0[i] = real ? a.tgt_off[q0 + i] - a.tgt_off[0] : 0;
  }
  __syncthreads();
  int maxlive = 0;
  for (int i = 0; i < TT_Q; ++i) maxlive = max(maxlive, sLive[i]);
  const float* qa = tile_query_ptr(a, q0, lane);
  for (int c0 = 0; c0 < maxlive; c0 += RK_T) {
    for (int x = tid; x < TT_Q * RK_T; x += 256) {
      const int i = x / RK_T, m = x % RK_T;
      if (c0 + m < sLive[i]) { tS[x] = a.sS[sE0[i] + c0 + m]; tI[x] = a.sI[sE0[i] + c0 + m]; }
      hist[x] = 0;
    }
    if (tid < TT_Q) sN[tid] = min(max(sLive[tid] - c0, 0), RK_T);
    __syncthreads();
    for (int64_t t0 = lo; t0 < hi; t0 += TT_N) {
      const TileCol col = tile_col(a, t0, hi, w, lane);
      const int j = col.j;
      const f32x16 acc = tile_dots(qa, col.e, a.H, lane >> 5);
      // ---- epilogue: scores, masks, bins ----------------------------------------------------------------------------
      const ItemTerm term = rk_item_term(a, j, col.ok);
      if (col.ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = xf_acc_row(r, lane);
          const int n = sN[i];  // (0 for the rows past n_query)
          const float s = rk_score(a.metric, acc[r], sRQ[i], sQQ[i], term.rn, term.ee);
          if (n == 0 || !tt_finite(s)) continue;
          const float* ts = tS + i * RK_T;
          const int* ti = tI + i * RK_T;
          if (tt_better(ts[n - 1], ti[n - 1], s, j)) continue;  // behind every target of this pass: no bin
          atomicAdd(&hist[i * RK_T + tt_count_better(ts, ti, n - 1, s, j)], 1);
        }
      }
    }
    __syncthreads();
    for (int x = tid; x < TT_Q * RK_T; x += 256) {
      const int i = x / RK_T, m = x % RK_T;
      if (m < sN[i]) a.hist[(int64_t)split * a.n_targets + sE0[i] + c0 + m] = hist[x];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rank_finish_kernel(RankArgs a) {
  __shared__ int sScan[256], sExcl[256];
  __shared__ int sCarry;
  static_assert(256 % RK_T == 0, "the scan restarts at multiples of RK_T");
  const int tid = threadIdx.x;
  const int qi = blockIdx.x;
  const int64_t base = a.tgt_off[0];
  const int64_t e0 = a.tgt_off[qi] - base, e1 = a.tgt_off[qi + 1] - base;
  const int nl = a.nlive[qi];
  if (tid == 0) sCarry = 0;
  __syncthreads();
  for (int m0 = 0; m0 < nl; m0 += 256) {
    const int m = m0 + tid;
    int v = 0, x = 0;
    if (m < nl) {
      for (int s = 0; s < a.splits; ++s) v += a.hist[(int64_t)s * a.n_targets + e0 + m];
      x = a.exb[e0 + m];
    }
    // a pass of the tile kernel bins against its own RK_T targets only (its bin 0 holds every item ahead of the pass's
    // first target): the counted items restart at every pass, the excluded ones (binned over the whole list) do not
    sScan[tid] = v;
    sExcl[tid] = x;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int t = (tid >= o && (tid - o) / RK_T == tid / RK_T) ? sScan[tid - o] : 0;
      const int u = tid >= o ? sExcl[tid - o] : 0;
      __syncthreads();
      sScan[tid] += t;
      sExcl[tid] += u;
      __syncthreads();
    }
    if (m < nl) a.exb[e0 + m] = sScan[tid] - (sCarry + sExcl[tid]);
    __syncthreads();
    if (tid == 255) sCarry += sExcl[255];
    __syncthreads();
  }
  for (int64_t e = e0 + tid; e < e1; e += 256)
    a.out_rank[base + e] = a.tI[e] != TT_IDX_NONE ? a.exb[e0 + a.pos[e]] : TT_IDX_NONE;
}

// ---- ranks among given candidates (xfmr_candidate_ranks) -----------------------------------------------------------------
// The sampled-candidate protocol and re-ranking: query q's items are S_q = distinct(candidates_q U targets_q) instead of
// the catalogue, eligibility, order and score are the ones above, rank(t) = 1 + the eligible items of S_q that are
// tt_better than t. S_q is walked as one list of nc + nt places: the candidate places (each list SORTED ascending, so a
// repeat is the place whose left neighbour holds the same id) and then the target places (one counts when it is the
// target's first entry and the target is not a candidate: a binary search). n_candidates dot products, not n_rows, so
// there is no MFMA tile to fill: one lane per place runs rk_item_score, the tile's fmaf chain, and a wave has 64 rows in
// flight by 16-byte loads. Two launches:
//   cand_init_kernel   one wave per query: out_rank = 1 (XFMR_RANK_NONE for a target that is not eligible) and the
//                      targets' scores. Skipped by the score-only form (no targets).
//   cand_count_kernel  grid (query, part). The query row is staged in LDS once. Per chunk of CD_T target entries: their
//                      scores into LDS (the chain again: no workspace), then the workgroup's batches of CD_B places
//                      (batch b belongs to part b % parts, so a list of thousands spreads over the grid and a short one
//                      costs the other parts two loads): scores of the batch into LDS, then every (place, target) pair
//                      is compared once, 256 threads as (target, slice of the batch), counts kept in registers over the
//                      batches, added over the slices by an integer LDS atomic and to out_rank by one integer global
//                      atomic per live target, chunk and workgroup. A query with more than CD_T entries scores its
//                      places once per chunk.
// Integer counts only: two calls give the same bits.
constexpr int CD_T = 128;  // target entries per chunk
constexpr int CD_B = 256;  // places per batch: one per thread
constexpr int CD_MAX_PARTS = 256;
constexpr int CD_TARGET_WG = 1024;

struct CandArgs : ScoreArgs {
  const int64_t* cand; const int64_t* cand_off;
  const int64_t* tgt; const int64_t* tgt_off;  // null: the score-only form
  int* out_rank; float* out_tscore; float* out_cscore;
  int parts;
};

// id in the sorted list v[lo..hi)
__device__ __forceinline__ bool cd_listed(const int64_t* v, int64_t lo, int64_t hi, int64_t id) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && v[lo] == id;
}

// the score of item id for the query in sQ when the item is eligible, -inf otherwise
__device__ __forceinline__ float cd_eligible_score(const CandArgs& a, const float* sQ, float rq, float qq, int64_t x0,
                                                   int64_t x1, int64_t id) {
  if (id < 1 || id >= a.n_rows || (a.excl && tt_excluded(a.excl, x0, x1, (int)id))) return -INFINITY;
  const float v = rk_item_score(a, sQ, rq, qq, (int)id);
  return tt_finite(v) ? v : -INFINITY;
}

// the query row into sQ (all threads of the workgroup; the caller's barrier follows); |q|^2 in every thread
__device__ __forceinline__ float cd_stage_query(const CandArgs& a, int qi, float* sQ) {
  const float* qr = a.q + (int64_t)qi * a.H;
  for (int h = threadIdx.x; h < a.H; h += blockDim.x) sQ[h] = qr[h];
  return rk_query_sqnorm(qr, a.H, threadIdx.x & 7);
}

__global__ __launch_bounds__(64) void cand_init_kernel(CandArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TOPK_MAX_H];
  const int qi = blockIdx.x;
  const float qq = cd_stage_query(a, qi, sQ);
  const float rq = rk_inv_norm(qq);
  const int64_t x0 = a.excl ? a.excl_off[qi] : 0, x1 = a.excl ? a.excl_off[qi + 1] : 0;
  __syncthreads();
  for (int64_t e = a.tgt_off[qi] + threadIdx.x; e < a.tgt_off[qi + 1]; e += 64) {
    const float s = cd_eligible_score(a, sQ, rq, qq, x0, x1, a.tgt[e]);
    a.out_rank[e] = tt_finite(s) ? 1 : TT_IDX_NONE;
    if (a.out_tscore) a.out_tscore[e] = s;
  }
}

__global__ __launch_bounds__(256) void cand_count_kernel(CandArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TOPK_MAX_H];
  __shared__ float bS[CD_B], tS[CD_T];
  __shared__ int bI[CD_B], tI[CD_T], cnt[CD_T];
  const int tid = threadIdx.x;
  const int qi = blockIdx.x, part = blockIdx.y;
  const int64_t c0 = a.cand_off[qi], t0 = a.tgt ? a.tgt_off[qi] : 0;
  const int64_t nc = a.cand_off[qi + 1] - c0, nt = a.tgt ? a.tgt_off[qi + 1] - t0 : 0;
  const int64_t places = nc + nt;
  if ((int64_t)part * CD_B >= places) return;  // (uniform: no batch for this part)
  const int64_t x0 = a.excl ? a.excl_off[qi] : 0, x1 = a.excl ? a.excl_off[qi + 1] : 0;
  const float qq = cd_stage_query(a, qi, sQ);
  const float rq = rk_inv_norm(qq);
  __syncthreads();
  for (int64_t m0 = 0; m0 == 0 || m0 < nt; m0 += CD_T) {
    const int n = (int)(nt - m0 < CD_T ? nt - m0 : CD_T);  // entries of this chunk (0: the score-only form)
    if (tid < CD_T) {
      float s = -INFINITY;
      int64_t id = 0;
      if (tid < n) {
        id = a.tgt[t0 + m0 + tid];
        s = cd_eligible_score(a, sQ, rq, qq, x0, x1, id);
      }
      tS[tid] = s;
      tI[tid] = tt_finite(s) ? (int)id : TT_IDX_NONE;
      cnt[tid] = 0;
    }
    // threads as (entry m, slice of the batch): n2 = the power of two that holds the chunk's entries
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    const int m = tid & (n2 - 1), i0 = (tid / n2) * n2;
    int beat = 0;
    for (int64_t b0 = (int64_t)part * CD_B; b0 < places; b0 += (int64_t)a.parts * CD_B) {
      const int64_t x = b0 + tid;
      float s = -INFINITY;
      int it = TT_IDX_NONE;  // a place that does not count
      if (x < nc) {
        const int64_t id = a.cand[c0 + x];
        s = cd_eligible_score(a, sQ, rq, qq, x0, x1, id);
        if (a.out_cscore && m0 == 0) a.out_cscore[c0 + x] = s;
        if (tt_finite(s) && !(x > 0 && a.cand[c0 + x - 1] == id)) it = (int)id;
      } else if (x < places && n > 0) {
        const int64_t f = x - nc, id = a.tgt[t0 + f];
        bool counts = id >= 1 && id < a.n_rows && !cd_listed(a.cand, c0, c0 + nc, id);
        for (int64_t g = 0; counts && g < f; ++g) counts = a.tgt[t0 + g] != id;
        if (counts) {
          s = cd_eligible_score(a, sQ, rq, qq, x0, x1, id);
          if (tt_finite(s)) it = (int)id;
        }
      }
      __syncthreads();  // (the previous batch's reads; the chunk's tS / tI / cnt)
      bS[tid] = s;
      bI[tid] = it;
      __syncthreads();
      if (m < n && tI[m] != TT_IDX_NONE) {
        const float ts = tS[m];
        const int ti = tI[m];
        for (int i = i0; i < i0 + n2; ++i) beat += (bI[i] != TT_IDX_NONE && tt_better(bS[i], bI[i], ts, ti)) ? 1 : 0;
      }
    }
    if (beat) atomicAdd(&cnt[m], beat);
    __syncthreads();
    if (tid < n && cnt[tid]) atomicAdd(&a.out_rank[t0 + m0 + tid], cnt[tid]);
    __syncthreads();
  }
}

// ---- the seven metrics: from a ranked list, or from the ranks ---------------------------------------------------------
// v = ndcg, map, auroc, precision, recall, hit, mrr with torchmetrics' definitions for a strictly decreasing score
// vector over [recommendations | missing targets] (metrics.py:66-79). The list torchmetrics sees: max(len(rec), top_k)
// slots of recommendations (padding never matches a target), then the missing targets; every metric only looks at the
// first K = top_k slots (+ the number of targets). Both walks below feed the SAME float expressions in the same order
// (ms_gain, ms_idcg, ms_values), so their per-row values are the same bits.
constexpr int MS_ROWS = 256;
constexpr int MS_VALS = 8;  // XFMR_NUM_RM sums + the number of rows

// distinct targets (target_ids = set(target_ids), metrics.py:66), eligible or not
__device__ __forceinline__ int ms_distinct(const int64_t* t, int n) {
  int nt = 0;
  for (int i = 0; i < n; ++i) {
    bool dup = false;
    for (int j = 0; j < i; ++j) dup |= t[j] == t[i];
    nt += dup ? 0 : 1;
  }
  return nt;
}

__device__ __forceinline__ float ms_gain(int slot) { return 1.f / log2f((float)slot + 2.f); }  // slot = rank - 1

__device__ __forceinline__ float ms_idcg(int nt, int K) {
  float idcg = 0.f;
  for (int i = 0; i < (nt < K ? nt : K); ++i) idcg += ms_gain(i);
  return idcg;
}

// one hit at rank r (1 = best) joins a cutoff's running sums
__device__ __forceinline__ void ms_hit(int r, int& hits, float& dcg, float& ap_sum, float& rr) {
  ++hits;
  dcg += ms_gain(r - 1);
  ap_sum += (float)hits / (float)r;
  if (rr == 0.f) rr = 1.f / (float)r;
}

// pairs = (hit, non-hit behind it) among the K slots, neg_seen = the non-hits among them
__device__ __forceinline__ void ms_values(float dcg, float ap_sum, float rr, int hits, int64_t pairs, int64_t neg_seen,
                                          int nt, int K, float v[7]) {
  const float idcg = ms_idcg(nt, K);
  v[0] = idcg > 0.f ? dcg / idcg : 0.f;
  v[1] = hits > 0 ? ap_sum / (float)hits : 0.f;
  v[2] = (hits > 0 && neg_seen > 0) ? (float)pairs / ((float)hits * (float)neg_seen) : 0.f;
  v[3] = (float)hits / (float)K;
  v[4] = (float)hits / (float)nt;
  v[5] = hits > 0 ? 1.f : 0.f;
  v[6] = rr;
}

// One query's seven metrics from its list: rec (B,k) ranked item indices (-1 = padding), targets CSR. Returns false
// (v all zero) when the user has no target (the reference returns {} for it, metrics.py:58-59).
__device__ __forceinline__ bool metrics_row(const int64_t* rec, const int64_t* tgt, const int64_t* tgt_off, int64_t b, int k,
                                            int top_k, float v[7]) {
  const int64_t* t = tgt + tgt_off[b];
  const int nt_raw = (int)(tgt_off[b + 1] - tgt_off[b]);
  for (int i = 0; i < 7; ++i) v[i] = 0.f;
  const int nt = ms_distinct(t, nt_raw);
  if (nt == 0) return false;
  const int64_t* r = rec + b * k;
  const int K = top_k;
  float dcg = 0.f, ap_sum = 0.f, rr = 0.f;
  int hits = 0, pairs = 0, neg_seen = 0;
  for (int i = 0; i < K; ++i) {
    bool rel = false;
    if (i < k && r[i] >= 0) {
      for (int j = 0; j < nt_raw; ++j) rel |= t[j] == r[i];
    }
    if (rel) ms_hit(i + 1, hits, dcg, ap_sum, rr);
    else {
      ++neg_seen;
      pairs += hits;  // each earlier positive outranks this negative
    }
  }
  ms_values(dcg, ap_sum, rr, hits, pairs, neg_seen, nt, K, v);
  return true;
}

// one thread per query: out (B,7), valid[b] = 0 when the user has no target
__global__ void metrics_kernel(const int64_t* rec, const int64_t* tgt, const int64_t* tgt_off, int B, int k, int top_k,
                               float* out, uint8_t* valid) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float v[7];
  valid[b] = metrics_row(rec, tgt, tgt_off, b, k, top_k, v);
  float* o = out + (int64_t)b * 7;
  for (int i = 0; i < 7; ++i) o[i] = v[i];
}

// ---- the metrics and their sums in one call (xfmr_retrieval_metrics_sum, xfmr_rank_metrics_sum) ----------------------
// 256-row workgroups, one row per lane. The seven values and the count of the rows that are valid and used go to fp64
// (lanes past n_query and rows left out: exact zeros), are added across the wave by xor shuffles (a fixed tree), across
// the four waves through LDS in a fixed order, and leave as ONE 8-double record per workgroup and cutoff.
// metrics_final_kernel: workgroup ci adds cutoff ci's records in index order (lane t takes records t, t + 256, ...) and
// finishes with the same tree. No atomics, no dependence on which workgroup finishes first: the same input gives the
// same doubles on every launch.
__device__ __forceinline__ void ms_block_sum(double acc[MS_VALS], double (*sP)[MS_VALS], double* dst) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int i = 0; i < MS_VALS; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < MS_VALS; ++i) sP[w][i] = acc[i];
  }
  __syncthreads();
  if (tid < MS_VALS) dst[tid] = (sP[0][tid] + sP[1][tid]) + (sP[2][tid] + sP[3][tid]);
}

// a row's record: its values and a one when it counts, exact zeros otherwise
__device__ __forceinline__ void ms_record(const float v[7], bool counts, double acc[MS_VALS]) {
#pragma unroll
  for (int i = 0; i < MS_VALS; ++i) acc[i] = 0.0;
  if (counts) {
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[i] = (double)v[i];
    acc[7] = 1.0;
  }
}

__global__ __launch_bounds__(MS_ROWS) void metrics_sum_kernel(const int64_t* rec, const int64_t* tgt, const int64_t* tgt_off,
                                                              const uint8_t* use, int64_t B, int k, int top_k, float* out,
                                                              uint8_t* valid, double* partial) {
  __shared__ double sP[MS_ROWS / 64][MS_VALS];
  const int64_t b = (int64_t)blockIdx.x * MS_ROWS + threadIdx.x;
  float v[7];
  bool counts = false;
  if (b < B) {
    const bool ok = metrics_row(rec, tgt, tgt_off, b, k, top_k, v);
    if (out) {
      for (int i = 0; i < 7; ++i) out[b * 7 + i] = v[i];
    }
    if (valid) valid[b] = ok;
    counts = ok && (!use || use[b]);
  }
  double acc[MS_VALS];
  ms_record(v, counts, acc);
  ms_block_sum(acc, sP, partial + (int64_t)blockIdx.x * MS_VALS);
}

__global__ __launch_bounds__(MS_ROWS) void metrics_final_kernel(const double* partial, int64_t n_partial, int n_cut,
                                                                double* sums) {
  __shared__ double sP[MS_ROWS / 64][MS_VALS];
  const int ci = blockIdx.x;
  double acc[MS_VALS];
#pragma unroll
  for (int i = 0; i < MS_VALS; ++i) acc[i] = 0.0;
  for (int64_t p = threadIdx.x; p < n_partial; p += MS_ROWS) {
#pragma unroll
    for (int i = 0; i < MS_VALS; ++i) acc[i] += partial[(p * n_cut + ci) * MS_VALS + i];
  }
  ms_block_sum(acc, sP, sums + (int64_t)ci * MS_VALS);
}

// From the ranks, at up to 8 cutoffs. The hits of a row at cutoff K are its distinct targets with rank <= K in
// ascending rank (distinct eligible items have distinct ranks and the repeats of one target share a rank: picking the
// next larger rank each time skips repeats); they are walked ONCE, every cutoff that still reaches the rank takes the hit.
constexpr int RK_MAX_CUTOFFS = 8;
struct RankCutoffs { int k[RK_MAX_CUTOFFS]; int n; };

__global__ __launch_bounds__(MS_ROWS) void rank_metrics_sum_kernel(const int* ranks, const int64_t* tgt,
                                                                   const int64_t* tgt_off, const uint8_t* use, int64_t B,
                                                                   RankCutoffs c, float* out, uint8_t* valid,
                                                                   double* partial) {
  __shared__ double sP[MS_ROWS / 64][MS_VALS];
  const int64_t b = (int64_t)blockIdx.x * MS_ROWS + threadIdx.x;
  float dcg[RK_MAX_CUTOFFS], ap_sum[RK_MAX_CUTOFFS], rr[RK_MAX_CUTOFFS];
  int hits[RK_MAX_CUTOFFS];
  int64_t rank_sum[RK_MAX_CUTOFFS];
#pragma unroll
  for (int ci = 0; ci < RK_MAX_CUTOFFS; ++ci) { dcg[ci] = ap_sum[ci] = rr[ci] = 0.f; hits[ci] = 0; rank_sum[ci] = 0; }
  int nt = 0;
  if (b < B) {
    const int64_t e0 = tgt_off[b];
    const int n = (int)(tgt_off[b + 1] - e0);
    const int* rk = ranks + e0;
    nt = ms_distinct(tgt + e0, n);
    int kmax = 0;
#pragma unroll
    for (int ci = 0; ci < RK_MAX_CUTOFFS; ++ci) kmax = ci < c.n ? max(kmax, c.k[ci]) : kmax;
    int prev = 0;
    while (nt > 0) {
      int r = TT_IDX_NONE;
      for (int i = 0; i < n; ++i) {
        const int x = rk[i];
        if (x > prev && x < r) r = x;
      }
      if (r == TT_IDX_NONE || r > kmax) break;
#pragma unroll
      for (int ci = 0; ci < RK_MAX_CUTOFFS; ++ci) {
        if (ci < c.n && r <= c.k[ci]) {
          ms_hit(r, hits[ci], dcg[ci], ap_sum[ci], rr[ci]);
          rank_sum[ci] += r;
        }
      }
      prev = r;
    }
    if (valid) valid[b] = nt > 0;
  }
  const bool used = b < B && nt > 0 && (!use || use[b]);
#pragma unroll
  for (int ci = 0; ci < RK_MAX_CUTOFFS; ++ci) {
    if (ci >= c.n) break;
    float v[7];
    if (b < B) {
      for (int i = 0; i < 7; ++i) v[i] = 0.f;
      if (nt > 0) {
        const int K = c.k[ci], h = hits[ci];
        // each hit outranks the non-hits behind it among the K slots: (K - r_j) - (h - 1 - j), summed over the hits
        const int64_t pairs = (int64_t)h * K - rank_sum[ci] - (int64_t)h * (h - 1) / 2;
        ms_values(dcg[ci], ap_sum[ci], rr[ci], h, pairs, (int64_t)K - h, nt, K, v);
      }
      if (out) {
        for (int i = 0; i < 7; ++i) out[(b * c.n + ci) * 7 + i] = v[i];
      }
    }
    double acc[MS_VALS];
    ms_record(v, used, acc);
    if (ci) __syncthreads();  // (the previous cutoff's sP reads)
    ms_block_sum(acc, sP, partial + ((int64_t)blockIdx.x * c.n + ci) * MS_VALS);
  }
}

// ---- host: one plan, one layout, one set of checks ------------------------------------------------------------------
// the rank workspace, in ints: six per-entry arrays, the per-query live counts, one histogram per slice
struct RankWs { size_t tS, tI, sS, sI, pos, exb, nlive, hist, end; };
static RankWs rank_ws(int64_t n_query, int64_t n_targets, int splits) {
  const size_t t = (size_t)n_targets, q = (size_t)n_query;
  return {0, t, 2 * t, 3 * t, 4 * t, 5 * t, 6 * t, 6 * t + q, 6 * t + q + (size_t)splits * t};
}

// parts of cand_count_kernel's grid: enough workgroups to cover the chip when there are few queries, never more than the
// batches the longest possible list has (`places` bounds every query's candidates + targets)
static int cand_parts(int64_t n_query, int64_t places) {
  int64_t p = (CD_TARGET_WG + n_query - 1) / n_query;
  const int64_t batches = (places + CD_B - 1) / CD_B;
  if (p > batches) p = batches;
  if (p > CD_MAX_PARTS) p = CD_MAX_PARTS;
  return p < 1 ? 1 : (int)p;
}

static int64_t ms_partials(int64_t n_query) { return (n_query + MS_ROWS - 1) / MS_ROWS; }

// the two sum entries' second launch: cutoff ci's records -> sums[ci]
static int launch_metrics_final(const double* partial, int64_t n_partial, int n_cut, double* sums, hipStream_t stream) {
  hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)n_cut), dim3(MS_ROWS), 0, stream, partial, n_partial, n_cut, sums);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // namespace

extern "C" {

size_t xfmr_topk_workspace(int64_t n_query, int64_t n_rows) {
  if (n_query <= 0 || n_rows <= 0) return 0;
  return (size_t)n_query * (size_t)n_rows * sizeof(float);
}

int xfmr_topk(const float* query, const float* table, const float* table_rnorm, int64_t n_rows, int64_t n_query,
              int32_t H, const int64_t* exclude, const int64_t* exclude_offsets, int32_t k, int32_t metric,
              int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = search_check(query, table, table_rnorm, nullptr, n_rows, n_query, H, exclude, exclude_offsets, metric,
                              workspace, true, out_idx && out_score && k > 0, k <= TOPK_MAX);
  if (rc != XFMR_OK) return rc;
  if (workspace_bytes < xfmr_topk_workspace(n_query, n_rows)) return XFMR_EWORKSPACE;
  TopkArgs a{};
  a.q = query; a.table = table; a.rnorm = table_rnorm; a.n_rows = n_rows; a.excl = exclude; a.excl_off = exclude_offsets;
  a.scores = (float*)workspace; a.out_idx = out_idx; a.out_score = out_score; a.H = H; a.k = k; a.metric = metric;
  hipLaunchKernelGGL(topk_kernel, dim3((unsigned)n_query), dim3(256), 0, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xfmr_retrieval_metrics(const int64_t* rec_idx, const int64_t* targets, const int64_t* target_offsets, int32_t n_query,
                           int32_t k, int32_t top_k, float* out, uint8_t* valid, void* stream) {
  if (!rec_idx || !targets || !target_offsets || !out || !valid || n_query <= 0 || k <= 0 || top_k <= 0)
    return XFMR_EINVAL;
  hipLaunchKernelGGL(metrics_kernel, dim3((n_query + 63) / 64), dim3(64), 0, (hipStream_t)stream, rec_idx, targets,
                     target_offsets, n_query, k, top_k, out, valid);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

size_t xfmr_retrieval_metrics_sum_workspace(int64_t n_query) { return xfmr_rank_metrics_sum_workspace(n_query, 1); }

int xfmr_retrieval_metrics_sum(const int64_t* rec_idx, const int64_t* targets, const int64_t* target_offsets,
                               const uint8_t* use, int64_t n_query, int32_t k, int32_t top_k, double* sums, float* out,
                               uint8_t* valid, void* workspace, size_t workspace_bytes, void* stream) {
  if (!rec_idx || !targets || !target_offsets || !sums || !workspace || n_query <= 0 || k <= 0 || top_k <= 0)
    return XFMR_EINVAL;
  if (n_query >= (1ll << 31)) return XFMR_EUNSUPPORTED;  // (xfmr_retrieval_metrics takes an int32 row count)
  if (workspace_bytes < xfmr_retrieval_metrics_sum_workspace(n_query)) return XFMR_EWORKSPACE;
  const int64_t n_partial = ms_partials(n_query);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(metrics_sum_kernel, dim3((unsigned)n_partial), dim3(MS_ROWS), 0, (hipStream_t)stream, rec_idx, targets,
                     target_offsets, use, n_query, k, top_k, out, valid, partial);
  XF_LAUNCH_CHECK();
  return launch_metrics_final(partial, n_partial, 1, sums, (hipStream_t)stream);
}

size_t xfmr_topk_tiled_workspace(int64_t n_query, int64_t n_rows, int32_t k) {
  if (n_query <= 0 || n_rows <= 0 || k <= 0) return 0;
  const size_t n = (size_t)n_query * (size_t)tiled_plan(n_query, n_rows).splits * (size_t)k;
  return n * sizeof(float) + n * sizeof(int);
}

int xfmr_topk_tiled(const float* query, const float* table, const float* table_rnorm, const float* table_sqnorm,
                    int64_t n_rows, int64_t n_query, int32_t H, const int64_t* exclude, const int64_t* exclude_offsets,
                    int32_t k, int32_t metric, int64_t* out_idx, float* out_score, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const int rc = search_check(query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric,
                              workspace, false, out_idx && out_score && k > 0, k <= TT_KMAX);
  if (rc != XFMR_OK) return rc;
  if (workspace_bytes < xfmr_topk_tiled_workspace(n_query, n_rows, k)) return XFMR_EWORKSPACE;
  const TiledPlan p = tiled_plan(n_query, n_rows);
  TiledArgs a{};
  fill_score_args(a, query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric, p);
  a.ws_score = (float*)workspace; a.ws_idx = (int*)(a.ws_score + (size_t)n_query * (size_t)p.splits * (size_t)k);
  a.k = k; a.kp = tiled_kp(k);
  const size_t lds = tiled_lds_bytes(a.kp);
  if (hipFuncSetAttribute((const void*)topk_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return XFMR_EHIP;
  hipLaunchKernelGGL(topk_tiled_kernel, p.grid(), dim3(256), lds, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_query), dim3(256), 0, (hipStream_t)stream, a.ws_score,
                     a.ws_idx, p.splits, k, out_idx, out_score);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

size_t xfmr_target_ranks_workspace(int64_t n_query, int64_t n_rows, int64_t n_targets) {
  if (n_query <= 0 || n_rows <= 0 || n_targets < 0) return 0;
  return rank_ws(n_query, n_targets, tiled_plan(n_query, n_rows).splits).end * sizeof(int);
}

int xfmr_target_ranks(const float* query, const float* table, const float* table_rnorm, const float* table_sqnorm,
                      int64_t n_rows, int64_t n_query, int32_t H, const int64_t* exclude, const int64_t* exclude_offsets,
                      const int64_t* targets, const int64_t* target_offsets, int64_t n_targets, int32_t metric,
                      int32_t* out_rank, float* out_target_score, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = search_check(query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric,
                              workspace, false, targets && target_offsets && out_rank && n_targets >= 0,
                              n_targets < (1ll << 31));
  if (rc != XFMR_OK) return rc;
  if (workspace_bytes < xfmr_target_ranks_workspace(n_query, n_rows, n_targets)) return XFMR_EWORKSPACE;
  const TiledPlan p = tiled_plan(n_query, n_rows);
  const RankWs ws = rank_ws(n_query, n_targets, p.splits);
  RankArgs a{};
  fill_score_args(a, query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric, p);
  a.tgt = targets; a.tgt_off = target_offsets;
  int* w = (int*)workspace;
  a.tS = (float*)(w + ws.tS); a.tI = w + ws.tI; a.sS = (float*)(w + ws.sS); a.sI = w + ws.sI;
  a.pos = w + ws.pos; a.exb = w + ws.exb; a.nlive = w + ws.nlive; a.hist = w + ws.hist;
  a.out_rank = out_rank; a.out_tscore = out_target_score; a.n_targets = n_targets;
  hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)n_query), dim3(256), 0, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_tile_kernel, p.grid(), dim3(256), 0, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)n_query), dim3(256), 0, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xfmr_candidate_ranks(const float* query, const float* table, const float* table_rnorm, const float* table_sqnorm,
                         int64_t n_rows, int64_t n_query, int32_t H, const int64_t* candidates,
                         const int64_t* candidate_offsets, const int64_t* exclude, const int64_t* exclude_offsets,
                         const int64_t* targets, const int64_t* target_offsets, int32_t metric, int32_t* out_rank,
                         float* out_target_score, float* out_candidate_score, void* stream) {
  // with targets: their offsets and out_rank; without: no target output, and the candidates' scores are the result
  const bool own = candidates && candidate_offsets &&
                   (targets ? target_offsets && out_rank
                            : !target_offsets && !out_rank && !out_target_score && out_candidate_score);
  // (no workspace: the table, whose own checks these are, stands in for it)
  const int rc = search_check(query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric,
                              table, false, own, true);
  if (rc != XFMR_OK) return rc;
  // The list sizes live on the device: the ends of both offset arrays are read back (the call's one wait) and checked
  // last, still before any launch.
  int64_t ends[4] = {0, 0, 0, 0};
  const hipStream_t st = (hipStream_t)stream;
  bool read = hipMemcpyAsync(ends, candidate_offsets, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipMemcpyAsync(ends + 1, candidate_offsets + n_query, 8, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (read && targets)
    read = hipMemcpyAsync(ends + 2, target_offsets, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipMemcpyAsync(ends + 3, target_offsets + n_query, 8, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (!read || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    return XFMR_EHIP;
  }
  const int64_t n_cand = ends[1] - ends[0], n_tgt = ends[3] - ends[2];
  if (n_cand < 0 || n_tgt < 0) return XFMR_EINVAL;
  if (n_cand >= (1ll << 31) || n_tgt >= (1ll << 31)) return XFMR_EUNSUPPORTED;
  CandArgs a{};
  fill_score_args(a, query, table, table_rnorm, table_sqnorm, n_rows, n_query, H, exclude, exclude_offsets, metric,
                  TiledPlan{1, 0, 0});
  a.cand = candidates; a.cand_off = candidate_offsets; a.tgt = targets; a.tgt_off = target_offsets;
  a.out_rank = out_rank; a.out_tscore = out_target_score; a.out_cscore = out_candidate_score;
  a.parts = cand_parts(n_query, n_cand + n_tgt);
  if (targets) {
    hipLaunchKernelGGL(cand_init_kernel, dim3((unsigned)n_query), dim3(64), 0, st, a);
    XF_LAUNCH_CHECK();
  }
  if (n_cand + n_tgt > 0) {
    hipLaunchKernelGGL(cand_count_kernel, dim3((unsigned)n_query, (unsigned)a.parts), dim3(256), 0, st, a);
    XF_LAUNCH_CHECK();
  }
  return XFMR_OK;
}

size_t xfmr_rank_metrics_sum_workspace(int64_t n_query, int32_t n_cutoffs) {
  if (n_query <= 0 || n_cutoffs <= 0) return 0;
  return (size_t)ms_partials(n_query) * (size_t)n_cutoffs * MS_VALS * sizeof(double);
}

int xfmr_rank_metrics_sum(const int32_t* ranks, const int64_t* targets, const int64_t* target_offsets, const uint8_t* use,
                          int64_t n_query, const int32_t* cutoffs, int32_t n_cutoffs, double* sums, float* out,
                          uint8_t* valid, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ranks || !targets || !target_offsets || !cutoffs || !sums || !workspace || n_query <= 0) return XFMR_EINVAL;
  if (n_cutoffs <= 0 || n_cutoffs > RK_MAX_CUTOFFS) return XFMR_EINVAL;
  RankCutoffs c{};
  c.n = n_cutoffs;
  for (int i = 0; i < n_cutoffs; ++i) {
    if (cutoffs[i] <= 0) return XFMR_EINVAL;
    c.k[i] = cutoffs[i];
  }
  if (n_query >= (1ll << 31)) return XFMR_EUNSUPPORTED;
  if (workspace_bytes < xfmr_rank_metrics_sum_workspace(n_query, n_cutoffs)) return XFMR_EWORKSPACE;
  const int64_t n_partial = ms_partials(n_query);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(rank_metrics_sum_kernel, dim3((unsigned)n_partial), dim3(MS_ROWS), 0, (hipStream_t)stream, ranks,
                     targets, target_offsets, use, n_query, c, out, valid, partial);
  XF_LAUNCH_CHECK();
  return launch_metrics_final(partial, n_partial, n_cutoffs, sums, (hipStream_t)stream);
}

int xfmr_table_sqnorm(const float* table, float* table_sqnorm, int64_t n_rows, int32_t H, void* stream) {
  if (!table || !table_sqnorm || n_rows <= 0 || H <= 0) return XFMR_EINVAL;
  hipLaunchKernelGGL(table_sqnorm_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     table, table_sqnorm, n_rows, H);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // extern "C"
