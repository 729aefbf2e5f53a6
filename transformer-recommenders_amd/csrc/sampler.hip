// Device-side sequence samplers: SeqDataset.__getitem__ + collate of the reference (xfmr_rec/data.py:669-805) for a
// whole batch in one launch, so that batches are born in HBM (above ~1e4 sequences/s the
// reference's per-row numpy sampling -- a Python loop over positions, a set difference over the catalogue per row --
// is the bottleneck of the training path).
//
// Two kernels, one workgroup of 256 threads per batch row, five stages each; the first four are the same code, written
// over a random stream (tests/sampler_model.py states them the same way). For the row's history h[0..n), labels lab[0..n):
//   row        offsets and length. A length outside [1, max_history] is written as zeros and nothing of the row is read
//              (the LDS below is sized from max_history).
//   positions  data.py:669-688: all of 0..n-2 if there are <= max_seq_length of them, else max_seq_length of them
//              uniformly without replacement, sorted: every position gets a hashed key, the L smallest keys win
//              (bitwise search for the L-th smallest key, ties by position), order-preserving compaction
//   positives  data.py:690-722: for each sampled position p a uniform draw among the later positions (within
//              pos_lookahead if > 0) whose label is positive, via the prefix count of labels; 0 if there is none
//   collate    data.py:789-805: rows right-padded with 0 to `width`
//   negatives  data.py:724-747: as many items as sampled positions, uniform over the catalogue minus the row's
//              history, without replacement while that set is large enough. One algorithm per kernel, below.
// A stream is a counter-based hash, draw(purpose, counter): reproducible, independent of the launch geometry -- and
// necessarily different from numpy's generator: parity with the reference is distributional (oracle/sampler.py), the
// kernels' own values are held exactly (tests/sampler_model.py).
//
// xfmr_seq_sample (seq_sample_kernel; DeviceSeqDataset.sample_batch):
//   rows       batch row b samples dataset row rows[b]. The row index is not checked: the entry is given no row count.
//   stream     a hash of (seed, dataset row, purpose, counter).
//   negatives  rejection sampling by thread 0 against two catalogue-sized bitmaps per batch row (the workspace).
// xfmr_seq_sample_rows (seq_sample_rows_kernel; DeviceSeqLoader, the epoch loop):
//   rows       batch row b samples dataset row order[first + b] of a device-resident epoch order: no per-batch upload.
//              A batch row past n_order, or a row index outside the dataset, is a zero row too.
//   stream     a function of (seed, epoch, dataset row, purpose, counter) alone: a row samples the same values in every
//              batch, slot and launch geometry.
//   negatives  drawn by the whole workgroup, no catalogue-sized memory anywhere. The row's distinct items are sorted in
//              LDS (bitonic, over the prefix-count / positive-list region once the positives are written). With D
//              distinct items hs[0..D) the j-th admissible item (0-based, A = n_items - D of them) is
//              j + 1 + #{i : hs[i] - 1 - i <= j} -- one binary search -- so a draw is a uniform RANK in [0, A) and never
//              lands in the history. Regimes of data.py:743-747: A == 0 -> ranks over the whole catalogue (D := 0);
//              fewer admissible items than draws -> every slot draws its own rank (with replacement); otherwise no
//              duplicates: while A >= 4 cnt, rounds in which every open slot draws a rank and keeps it unless a filled
//              slot, or an open slot of LOWER index, holds the same rank (a rule on slot and round: deterministic, and
//              symmetric in the items, hence uniform over ordered draws without replacement; an open slot closes with
//              probability > 3/4 per round). If A < 4 cnt, or a slot is still open after REJECT_ROUNDS rounds, the exact path
//              runs instead: the cnt smallest hashed keys among ranks 0..A-1 (the positions' selection), in key order.
//   outputs    len_out[b] = number of sampled positions of row b.
#include "common.h"

namespace {

constexpr int MAX_HIST = 8192;
constexpr int REJECT_ROUNDS = 32;
constexpr size_t ROWS_MAX_LDS = 160 * 1024;

struct StageArgs {  // what the shared stages need: the head of both kernels' arguments
  const int64_t* items; const uint8_t* labels; const int64_t* offsets;
  int64_t* hist_out; int64_t* pos_out; int64_t* neg_out;
  int width, max_len, lookahead, max_hist;
  int64_t n_items;
};
struct SampleArgs : StageArgs {
  const int64_t* rows;
  uint32_t* bitmaps;  // [batch][2][words]
  int words;
  uint64_t seed;
};
struct RowsArgs : StageArgs {
  const int64_t* order;
  int64_t n_rows, n_order, first;
  int32_t* len_out;
  uint64_t seed, epoch;
};

// Dynamic LDS of one row, in ints: P [max_hist + 1] | posidx [max_hist] | sel [width] | nkey [width] (rows only) | 8 spare.
// The launchers size from `end`, the kernels carve from the offsets. max_hist <= MAX_HIST; for `rows`, width <= 256 * 32.
struct RowLds { int P, posidx, sel, nkey; size_t end; };
__host__ __device__ inline RowLds row_lds(int max_hist, int width, bool rows) {
  const int sel = 2 * max_hist + 1;
  return {0, max_hist + 1, sel, rows ? sel + width : 0, (size_t)sel + (rows ? 2 : 1) * (size_t)width + 8};
}

// ---- the two streams ------------------------------------------------------------------------------------------------
struct SeqStream {
  uint64_t seed; int64_t row;
  __device__ __forceinline__ uint32_t draw(uint32_t purpose, uint32_t ctr) const {
    uint32_t x = xf_hash32((uint32_t)seed ^ (uint32_t)(seed >> 32) * 0x9e3779b9u ^ (uint32_t)row * 0x85ebca6bu);
    x = xf_hash32(x ^ (purpose * 0xc2b2ae35u) ^ ctr);
    return xf_hash32(x + 0x27d4eb2fu * ctr);
  }
};

struct RowKey { uint32_t k0, k1; };
__device__ __forceinline__ RowKey row_key(uint64_t seed, uint64_t epoch, int64_t row) {
  uint32_t a = xf_hash32((uint32_t)seed ^ xf_hash32((uint32_t)(seed >> 32) + 0x9e3779b9u));
  a = xf_hash32(a ^ (uint32_t)epoch * 0x85ebca6bu);
  a = xf_hash32(a + (uint32_t)(epoch >> 32) * 0xc2b2ae35u);
  uint32_t b = xf_hash32(a ^ 0x27d4eb2fu);
  a = xf_hash32(a ^ (uint32_t)row);
  b = xf_hash32(b + (uint32_t)((uint64_t)row >> 32) * 0x165667b1u + ((uint32_t)row * 0x9e3779b9u));
  return RowKey{a, b};
}
struct RowsStream {
  RowKey key;
  __device__ __forceinline__ uint32_t draw(uint32_t purpose, uint32_t ctr) const {
    const uint32_t x = xf_hash32(key.k0 ^ (purpose * 0xc2b2ae35u) ^ ctr);
    return xf_hash32((x ^ key.k1) + 0x27d4eb2fu * ctr);
  }
};

// uniform integer in [0, n) from 32 random bits (multiply-shift: bias < n / 2^32)
__device__ __forceinline__ uint32_t below(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// ---- workgroup sums and counts --------------------------------------------------------------------------------------
__device__ int block_sum_i(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// exclusive count of `p` over the threads in front of this one, and the workgroup's total (uniform)
__device__ __forceinline__ int block_excl(bool p, int* wcnt, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(p);
  if (lane == 0) wcnt[w] = __popcll(bal);
  __syncthreads();
  int before = 0;
  for (int k = 0; k < w; ++k) before += wcnt[k];
  before += __popcll(bal & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
  total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  __syncthreads();
  return before;
}

// ---- the stages both kernels share ----------------------------------------------------------------------------------
struct Row { int64_t o0; int n; };  // events [o0, o0 + n) of items / labels; n == 0: the batch row is written as zeros
// `known`: the row index may be used on offsets (uniform over the workgroup, as is the result)
__device__ __forceinline__ Row read_row(const int64_t* offsets, int64_t row, bool known, int max_hist) {
  Row r{0, 0};
  if (known) {
    r.o0 = offsets[row];
    const int64_t len = offsets[row + 1] - r.o0;
    r.n = len >= 1 && len <= max_hist ? (int)len : 0;
  }
  return r;
}

__device__ __forceinline__ void write_zero_row(int64_t* ho, int64_t* po, int64_t* no, int width) {
  for (int k = threadIdx.x; k < width; k += 256) { ho[k] = 0; po[k] = 0; no[k] = 0; }
}

// The `want` smallest keys s.draw(purpose, i) among i in [0, m), ties by index: their indices, ascending, into
// out[0..min(m, want)). Returns that count (uniform). out is LDS; a barrier stands behind the last write.
template <class Stream>
__device__ int select_smallest(const Stream s, uint32_t purpose, int m, int want, int* out, int* red, int* wcnt) {
  const int tid = threadIdx.x;
  uint32_t T = 0xffffffffu;
  int need_eq = 0;
  if (m > want) {
    uint32_t t = 0;  // smallest T with count(key <= T) >= want, bit by bit from the top
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = t | ((1u << bit) - 1u);
      int c = 0;
      for (int i = tid; i < m; i += 256) c += s.draw(purpose, (uint32_t)i) <= cand ? 1 : 0;
      if (block_sum_i(c, red) < want) t |= 1u << bit;
    }
    T = t;
    int lt = 0;
    for (int i = tid; i < m; i += 256) lt += s.draw(purpose, (uint32_t)i) < T ? 1 : 0;
    need_eq = want - block_sum_i(lt, red);  // how many of the keys == T are taken (lowest indices first)
  }
  int n_sel = 0, n_eq = 0;
  for (int i0 = 0; i0 < m && n_sel < want; i0 += 256) {
    const int i = i0 + tid;
    bool lt = false, eq = false;
    if (i < m) {
      if (m <= want) lt = true;
      else {
        const uint32_t k = s.draw(purpose, (uint32_t)i);
        lt = k < T;
        eq = k == T;
      }
    }
    int tot_eq, tot;
    const int eq_before = n_eq + block_excl(eq, wcnt, tot_eq);
    const bool take = lt || (eq && eq_before < need_eq);
    const int at = n_sel + block_excl(take, wcnt, tot);
    if (take && at < want) out[at] = i;
    n_sel += tot;
    n_eq += tot_eq;
  }
  __syncthreads();
  return n_sel < want ? n_sel : want;
}

// P[i] = number of positive labels in front of position i, for i in [0, n]; posidx[0..P[n]) = the positions with a positive
// label, ascending. Returns P[n] (uniform). P and posidx are LDS; a barrier stands behind the write of P[n].
__device__ int label_prefix(const uint8_t* lab, int n, int* P, int* posidx, int* wcnt) {
  const int tid = threadIdx.x;
  int n_pos = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    const bool p = i < n && lab[i] != 0;
    int tot;
    const int before = n_pos + block_excl(p, wcnt, tot);
    if (i < n) {
      P[i] = before;
      if (p) posidx[before] = i;
    }
    n_pos += tot;
  }
  if (tid == 0) P[n] = n_pos;
  __syncthreads();
  return n_pos;
}

// History and positives of the cnt sampled positions sel[0..cnt), right-padded with 0 to `width`: data.py:690-722, 789-805.
// Reads sel, P and posidx (LDS) and writes none of them: no barrier stands behind the reads, whoever writes that LDS next
// puts one in front.
template <class Stream>
__device__ __forceinline__ void write_history_positives(const Stream s, const int64_t* h, int n, int lookahead, int width,
                                                        int cnt, const int* sel, const int* P, const int* posidx,
                                                        int64_t* ho, int64_t* po) {
  for (int k = threadIdx.x; k < width; k += 256) {
    int64_t hv = 0, pv = 0;
    if (k < cnt) {
      const int p = sel[k];
      hv = h[p];
      const int start = p + 1;
      const int end = lookahead > 0 ? (start + lookahead < n ? start + lookahead : n) : n;
      const int c = P[end] - P[start];
      if (c > 0) pv = h[posidx[P[start] + (int)below(s.draw(2u, (uint32_t)k), (uint32_t)c)]];
    }
    ho[k] = hv;
    po[k] = pv;
  }
}

// ---- negatives of xfmr_seq_sample: rejection against two bitmaps over the catalogue, by thread 0 ------------------------
__device__ __forceinline__ void negatives_bitmap(const SeqStream s, const int64_t* h, int n, int cnt, int64_t n_items,
                                                 uint32_t* inhist, int words, int64_t* no, int width, int* red) {
  const int tid = threadIdx.x;
  uint32_t* chosen = inhist + words;
  for (int k = tid; k < 2 * words; k += 256) inhist[k] = 0u;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int64_t it = h[i];
    if (it >= 1 && it <= n_items) atomicOr(&inhist[it >> 5], 1u << (it & 31));
  }
  __syncthreads();
  int distinct = 0;
  for (int k = tid; k < words; k += 256) distinct += __popc(inhist[k]);
  distinct = block_sum_i(distinct, red);
  if (tid == 0) {
    const int64_t n_cand = n_items - distinct;
    const bool any_item = n_cand == 0;          // data.py:743-744: nothing left -> the whole catalogue
    const bool replace = !any_item ? n_cand < cnt : n_items < cnt;  // data.py:745-747
    uint32_t ctr = 0;
    for (int k = 0; k < cnt; ++k) {
      int64_t x = 0;
      for (int attempt = 0;; ++attempt) {
        x = 1 + (int64_t)below(s.draw(3u, ctr++), (uint32_t)n_items);
        const uint32_t bit = 1u << (x & 31);
        const bool bad = (!any_item && (inhist[x >> 5] & bit)) || (!replace && (chosen[x >> 5] & bit));
        if (!bad) break;
        if (attempt >= 64) {  // crowded catalogue: walk forward from the draw to the first admissible item
          for (int64_t t = 0; t < n_items; ++t) {
            const int64_t y = 1 + (x - 1 + t) % n_items;
            const uint32_t by = 1u << (y & 31);
            if (!((!any_item && (inhist[y >> 5] & by)) || (!replace && (chosen[y >> 5] & by)))) { x = y; break; }
          }
          break;
        }
      }
      chosen[x >> 5] |= 1u << (x & 31);
      no[k] = x;
    }
    for (int k = cnt; k < width; ++k) no[k] = 0;
  }
}

// ---- negatives of xfmr_seq_sample_rows: ranks among the admissible items, by the whole workgroup ------------------------
// rank (0-based) among the items of 1..n_items that are not in hs[0..D) -> the item
__device__ __forceinline__ int64_t admissible_item(const uint32_t* hs, int D, uint32_t j) {
  int lo = 0, hi = D;  // first i with hs[i] - 1 - i > j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (hs[mid] - 1u - (uint32_t)mid <= j) lo = mid + 1; else hi = mid;
  }
  return (int64_t)j + 1 + lo;
}

// hs: LDS for the row's distinct items, sorted (2 max_hist words: over P / posidx, which must be free, with a barrier
// behind their last read); sel [width]: a slot's rank; nkey [width]: exact path, the selected ranks' keys
__device__ __forceinline__ void negatives_ranked(const RowsStream s, const int64_t* h, int n, int cnt, int64_t n_items,
                                                 uint32_t* hs, int* sel, uint32_t* nkey, int64_t* no, int width,
                                                 int* red, int* wcnt) {
  const int tid = threadIdx.x;
  int N = 1;
  while (N < n) N <<= 1;  // <= 2 n - 1 <= 2 max_hist words
  for (int i = tid; i < N; i += 256) {
    const int64_t v = i < n ? h[i] : 0;
    hs[i] = v >= 1 && v <= n_items ? (uint32_t)v : 0xffffffffu;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t x = hs[i], y = hs[i | j];
        if ((x > y) == ((i & k) == 0)) { hs[i] = y; hs[i | j] = x; }
      }
      __syncthreads();
    }
  // in-place order-preserving removal of duplicates and of the filler (a chunk writes at or below what it has read)
  int D = 0;
  for (int i0 = 0; i0 < N; i0 += 256) {
    const int i = i0 + tid;
    const uint32_t v = i < N ? hs[i] : 0xffffffffu;
    const bool first = v != 0xffffffffu && (i == 0 || hs[i - 1] != v);
    int tot;
    const int at = D + block_excl(first, wcnt, tot);  // (its barriers stand between the reads above and the writes below)
    if (first) hs[at] = v;
    D += tot;
    __syncthreads();
  }

  const bool any_item = n_items - D == 0;  // data.py:743-744: nothing left -> the whole catalogue
  if (any_item) D = 0;
  const uint32_t A = (uint32_t)(n_items - D);  // admissible items: ranks 0..A-1
  uint32_t* val = (uint32_t*)sel;              // [cnt] a slot's rank; bit 31: the slot is filled
  constexpr uint32_t FILLED = 0x80000000u;
  bool exact = false;
  if (A < (uint32_t)cnt) {  // with replacement
    for (int k = tid; k < cnt; k += 256) val[k] = below(s.draw(3u, (uint32_t)k), A);
  } else if ((uint64_t)A < 4ull * (uint64_t)cnt) {
    exact = true;
  } else {
    for (int k = tid; k < cnt; k += 256) val[k] = 0;
    int open = cnt;
    for (int r = 0; r < REJECT_ROUNDS && open > 0; ++r) {
      __syncthreads();
      for (int k = tid; k < cnt; k += 256)
        if (!(val[k] & FILLED)) val[k] = below(s.draw(16u + (uint32_t)r, (uint32_t)k), A);
      __syncthreads();
      uint32_t keep = 0;  // bit b: this thread's b-th slot closes this round (cnt <= width <= 256 * 32)
      int still = 0, b = 0;
      for (int k = tid; k < cnt; k += 256, ++b) {
        const uint32_t x = val[k];
        if (x & FILLED) continue;
        bool ok = true;
        for (int q = 0; q < cnt; ++q) {
          const uint32_t y = val[q];
          ok = ok && !((y & ~FILLED) == x && ((y & FILLED) || q < k));
        }
        if (ok) keep |= 1u << b; else ++still;
      }
      __syncthreads();
      b = 0;
      for (int k = tid; k < cnt; k += 256, ++b)
        if (keep >> b & 1u) val[k] |= FILLED;
      open = block_sum_i(still, red);
    }
    exact = open > 0;
  }
  __syncthreads();
  if (exact) {
    // the cnt smallest keys among the A ranks, then in key order (a uniform ordered draw without replacement)
    select_smallest(s, 4u, (int)A, cnt, sel, red, wcnt);
    for (int k = tid; k < cnt; k += 256) nkey[k] = s.draw(4u, (uint32_t)sel[k]);
    __syncthreads();
    for (int k = tid; k < cnt; k += 256) {
      const uint32_t x = nkey[k];
      int at = 0;
      for (int q = 0; q < cnt; ++q) at += nkey[q] < x || (nkey[q] == x && q < k) ? 1 : 0;
      no[at] = admissible_item(hs, D, (uint32_t)sel[k]);
    }
  } else {
    for (int k = tid; k < cnt; k += 256) no[k] = admissible_item(hs, D, val[k] & ~FILLED);
  }
  for (int k = cnt + tid; k < width; k += 256) no[k] = 0;
}

// ---- the kernels: a row's five stages ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seq_sample_kernel(SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  __shared__ int red[4], wcnt[4];  // block_sum_i's and block_excl's
  const int b = blockIdx.x;
  int64_t* ho = a.hist_out + (int64_t)b * a.width;
  int64_t* po = a.pos_out + (int64_t)b * a.width;
  int64_t* no = a.neg_out + (int64_t)b * a.width;
  const int64_t row = a.rows[b];
  const Row r = read_row(a.offsets, row, true, a.max_hist);
  if (r.n == 0) {  // (uniform over the workgroup)
    write_zero_row(ho, po, no, a.width);
    return;
  }
  const int64_t* h = a.items + r.o0;
  const SeqStream s{a.seed, row};
  const RowLds lds = row_lds(a.max_hist, a.width, false);
  int *P = smem + lds.P, *posidx = smem + lds.posidx, *sel = smem + lds.sel;
  const int L = a.max_len < a.width ? a.max_len : a.width;
  // candidate positions 0..n-2: the last item only ever serves as a positive
  const int cnt = select_smallest(s, 1u, r.n - 1, L, sel, red, wcnt);  // = min(n - 1, L)
  label_prefix(a.labels + r.o0, r.n, P, posidx, wcnt);
  write_history_positives(s, h, r.n, a.lookahead, a.width, cnt, sel, P, posidx, ho, po);
  negatives_bitmap(s, h, r.n, cnt, a.n_items, a.bitmaps + (int64_t)b * 2 * a.words, a.words, no, a.width, red);
}

__global__ __launch_bounds__(256) void seq_sample_rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  __shared__ int red[4], wcnt[4];  // block_sum_i's and block_excl's
  const int b = blockIdx.x;
  int64_t* ho = a.hist_out + (int64_t)b * a.width;
  int64_t* po = a.pos_out + (int64_t)b * a.width;
  int64_t* no = a.neg_out + (int64_t)b * a.width;
  const int64_t row = a.first + b < a.n_order ? a.order[a.first + b] : -1;
  const Row r = read_row(a.offsets, row, row >= 0 && row < a.n_rows, a.max_hist);
  if (r.n == 0) {  // (uniform over the workgroup)
    write_zero_row(ho, po, no, a.width);
    if (threadIdx.x == 0) a.len_out[b] = 0;
    return;
  }
  const int64_t* h = a.items + r.o0;
  const RowsStream s{row_key(a.seed, a.epoch, row)};
  const RowLds lds = row_lds(a.max_hist, a.width, true);
  int *P = smem + lds.P, *posidx = smem + lds.posidx, *sel = smem + lds.sel;
  const int L = a.max_len < a.width ? a.max_len : a.width;
  // candidate positions 0..n-2: the last item only ever serves as a positive
  const int cnt = select_smallest(s, 1u, r.n - 1, L, sel, red, wcnt);  // = min(n - 1, L)
  label_prefix(a.labels + r.o0, r.n, P, posidx, wcnt);
  write_history_positives(s, h, r.n, a.lookahead, a.width, cnt, sel, P, posidx, ho, po);
  if (threadIdx.x == 0) a.len_out[b] = cnt;
  __syncthreads();  // P, posidx and sel are free from here on
  negatives_ranked(s, h, r.n, cnt, a.n_items, (uint32_t*)smem, sel, (uint32_t*)(smem + lds.nkey), no, a.width, red, wcnt);
}

// ---- host side --------------------------------------------------------------------------------------------------------
size_t words_for(int64_t n_items) { return (size_t)((n_items + 1 + 31) / 32); }

void fill_stage_args(StageArgs& a, const int64_t* items, const uint8_t* labels, const int64_t* offsets, int32_t width,
                     int32_t max_seq_length, int32_t pos_lookahead, int64_t n_items, int32_t max_history,
                     int64_t* hist_out, int64_t* pos_out, int64_t* neg_out) {
  a.items = items; a.labels = labels; a.offsets = offsets;
  a.hist_out = hist_out; a.pos_out = pos_out; a.neg_out = neg_out;
  a.width = width; a.max_len = max_seq_length; a.lookahead = pos_lookahead; a.max_hist = max_history;
  a.n_items = n_items;
}

// The refusals both entries share. `own`: the entry's own pointers are there and its own sizes are in range.
int sample_check(const StageArgs& a, int32_t batch, bool own) {
  if (!own || !a.items || !a.labels || !a.offsets || !a.hist_out || !a.pos_out || !a.neg_out) return XFMR_EINVAL;
  if (batch <= 0 || a.width <= 0 || a.max_len <= 0 || a.lookahead < 0 || a.n_items <= 0 || a.max_hist <= 0)
    return XFMR_EINVAL;
  if (a.n_items >= (1ll << 31) || a.max_hist > MAX_HIST) return XFMR_EUNSUPPORTED;
  return XFMR_OK;
}

template <class Args>
int launch_sampler(void (*kernel)(Args), const Args& a, int32_t batch, bool rows, void* stream) {
  const size_t smem = row_lds(a.max_hist, a.width, rows).end * sizeof(int);
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return XFMR_EHIP;
  hipLaunchKernelGGL(kernel, dim3(batch), dim3(256), smem, (hipStream_t)stream, a);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // namespace

extern "C" {

size_t xfmr_seq_sample_workspace(int32_t batch, int64_t n_items) {
  if (batch <= 0 || n_items <= 0) return 0;
  return (size_t)batch * 2 * words_for(n_items) * sizeof(uint32_t);
}

int xfmr_seq_sample(const int64_t* items, const uint8_t* labels, const int64_t* offsets, const int64_t* rows,
                    int32_t batch, int32_t width, int32_t max_seq_length, int32_t pos_lookahead, int64_t n_items,
                    int32_t max_history, uint64_t seed, int64_t* hist_out, int64_t* pos_out, int64_t* neg_out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  SampleArgs a{};
  fill_stage_args(a, items, labels, offsets, width, max_seq_length, pos_lookahead, n_items, max_history, hist_out,
                  pos_out, neg_out);
  if (const int rc = sample_check(a, batch, rows && workspace)) return rc;
  if (workspace_bytes < xfmr_seq_sample_workspace(batch, n_items)) return XFMR_EWORKSPACE;
  a.rows = rows; a.bitmaps = (uint32_t*)workspace; a.words = (int)words_for(n_items); a.seed = seed;
  return launch_sampler(seq_sample_kernel, a, batch, false, stream);
}

size_t xfmr_seq_sample_rows_workspace(int32_t batch, int32_t width) {
  (void)batch; (void)width;
  return 0;  // everything a row needs is held in LDS
}

int xfmr_seq_sample_rows(const int64_t* items, const uint8_t* labels, const int64_t* offsets, int64_t n_rows,
                         const int64_t* order, int64_t n_order, int64_t first, int32_t batch, int32_t width,
                         int32_t max_seq_length, int32_t pos_lookahead, int64_t n_items, int32_t max_history,
                         uint64_t seed, uint64_t epoch, int64_t* hist_out, int64_t* pos_out, int64_t* neg_out,
                         int32_t* len_out, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  RowsArgs a{};
  fill_stage_args(a, items, labels, offsets, width, max_seq_length, pos_lookahead, n_items, max_history, hist_out,
                  pos_out, neg_out);
  if (const int rc = sample_check(a, batch, order && len_out && n_rows > 0 && n_order >= 0 && first >= 0)) return rc;
  if (width > 256 * 32 || row_lds(max_history, width, true).end * sizeof(int) > ROWS_MAX_LDS) return XFMR_EUNSUPPORTED;
  if (workspace_bytes < xfmr_seq_sample_rows_workspace(batch, width)) return XFMR_EWORKSPACE;
  a.order = order; a.n_rows = n_rows; a.n_order = n_order; a.first = first; a.len_out = len_out;
  a.seed = seed; a.epoch = epoch;
  return launch_sampler(seq_sample_rows_kernel, a, batch, true, stream);
}

}  // extern "C"
