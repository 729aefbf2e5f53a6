// MFMA GEMMs for the encoder's Linear layers (forward, dX, dW) with fused epilogues.
//
//   C[M,N] = A'[M,K] * B'[N,K]^T,  A' = A or A^T, B' = B or B^T as stored (fp32, row-major)
//
// One workgroup = 4 waves (2x2) computes a BM x BN tile; each wave owns (BM/2)x(BN/2) as 32x32 MFMA
// accumulators. K is walked in BK=32 slices: global fp32 -> registers (prefetch of slice k+1 is in
// flight while slice k is multiplied) -> converted to the MFMA element type on the way into LDS.
// These GEMMs are skinny (K = H or I <= 1024, except dW where K = tokens and the split-K grid supplies
// the parallelism); the operands are L2 / Infinity-Cache resident between the kernels of one step.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "internal.h"

// A per-row scalar that is broadcast into packed-fp32 arithmetic (v_pk_add/mul/fma_f32 on register pairs) is made
// opaque right before its use: hipcc otherwise packs NEIGHBOURING rows' scalars (mean[ps], mean[ps + 1]) into one
// 64-bit register and broadcasts the odd one with op_sel:[..] (the LOW result lane reads the HIGH dword). Every build
// of the LayerNorm-backward epilogue that contained such an instruction produced intermittently wrong rows in exactly
// the passes that used them; every build without one was bit-reproducible (DESIGN.md section 4 has the table).
#define XF_PIN_SCALAR(x) asm volatile("" : "+v"(x))
#ifndef XF_LN_DIAG
#define XF_LN_DIAG 0  // 32 (with -DXF_LN_EPI_MIN_WAVES=1): the unpinned build that reproduces the fault (scripts/probe/lnbwd_determinism.py)
#endif
#ifndef XF_GEMM_PF
#define XF_GEMM_PF 1  // operand K slices in flight per workgroup (gemm_kernel)
#endif
#ifndef XF_DW_PF
#define XF_DW_PF 1    // ... of the split-K weight-gradient GEMMs (experiment builds: -DXF_DW_PF=2)
#endif
// Barrier of the fused FFN kernels' chunk loops. 1: s_waitcnt lgkmcnt(0) + s_barrier through inline asm -- the LDS hand-off
// only; __syncthreads() (and __builtin_amdgcn_s_barrier: the backend puts s_waitcnt 0 in front of every S_BARRIER on
// this target) also drains vmcnt, i.e. every weight / activation prefetch issued since the last barrier.
// Probe build (-DXF_FFN_STAMP): wave 0 of every workgroup of ffn_fwd_fused_kernel writes s_memtime stamps of its phases to
// the buffer behind XFMR_FFN_STAMPS (scripts/probe/ffn_fwd_stamps.py); not part of the product build.
#ifdef XF_FFN_STAMP
#define XF_STAMP(i) do { if (stamp_on) st_buf[(i)] = __builtin_readcyclecounter(); } while (0)
#else
#define XF_STAMP(i) do {} while (0)
#endif
#ifndef XF_FFN_ASM_BARRIER
#define XF_FFN_ASM_BARRIER 1
#endif
#if XF_FFN_ASM_BARRIER
#define XF_LOOP_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#else
#define XF_LOOP_BARRIER() __syncthreads()
#endif
// The same for the LDS exchanges inside the two LayerNorm epilogues (their barriers sit right behind global stores)
#ifndef XF_EPI_ASM_BARRIER
#define XF_EPI_ASM_BARRIER 1
#endif
#if XF_EPI_ASM_BARRIER
#define XF_EPI_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#else
#define XF_EPI_BARRIER() __syncthreads()
#endif
#ifndef XF_FFN_MIN_WAVES
#define XF_FFN_MIN_WAVES 2
#endif
#ifndef XF_LN_EPI_MIN_WAVES
#define XF_LN_EPI_MIN_WAVES 3  // launch bound (waves per SIMD) of the two LayerNorm-fused epilogues: DESIGN.md section 4
#endif

namespace {

// EPI_DROP_RES_LN: EPI_DROP_RES whose tile spans whole output rows (BN == N): the LayerNorm that follows the Linear
// (TF:modeling_bert.py:292,349) is applied in the epilogue -- C = pre-LayerNorm sum (the backward needs it), Y / Y16 =
// the normalised output (fp32 residual stream + bf16 GEMM operand), mean / rstd per row.
// EPI_DX_LNBWD: a dX GEMM (+ residual gradient) whose output rows are the gradient of a LayerNorm OUTPUT: the LayerNorm
// backward runs in the epilogue -- C = gradient of the LayerNorm input, D16 = its dropout-scaled bf16 copy (the
// gradient of the Linear that fed the LayerNorm), one partial record [3][128] (d gamma, d beta, d bias) per workgroup.
// EPI_DROP_RES_LN_RE / _RED: EPI_DROP_RES_LN whose residual operand is not loaded from a stored fp32 tensor but RE-DERIVED
// from what the LayerNorm that produced it stored for its backward (its input, mean, rstd; gamma, beta) -- xf_ln_out_drop4;
// _RED: ... followed by the dropout of that output (layer 0: the residual is the embedding LayerNorm's dropped-out output).
// EPI_DROP_RES_LN_INFER: EPI_DROP_RES_LN (loaded residual) of the forward-only pass (xfmr_encoder_infer): Y / Y16 only -- no C
// (pre), mean or rstd store, which only a backward reads. Same arithmetic in the same order: the same Y bits.
// EPI_GELU_INFER: EPI_GELU without the C2 store (the pre-activation or gelu' the FFN2 dX epilogue would read); xf_gelu and
// xf_gelu_both evaluate gelu by the same expression, so C has EPI_GELU's bits with or without XF_AUX_GELU_GRAD.
// Separate instantiations: the variants cost registers the plain form does not pay.
enum { EPI_STORE = 0, EPI_GELU = 1, EPI_DROP_RES = 2, EPI_GELU_GRAD = 3, EPI_SPLITK = 4, EPI_DROP_RES_LN = 5,
       EPI_DX_LNBWD = 6, EPI_DROP_RES_LN_RE = 7, EPI_DROP_RES_LN_RED = 8, EPI_DROP_RES_LN_INFER = 9,
       EPI_GELU_INFER = 10 };
constexpr bool epi_res_ln(int epi) {
  return epi == EPI_DROP_RES_LN || epi == EPI_DROP_RES_LN_RE || epi == EPI_DROP_RES_LN_RED || epi == EPI_DROP_RES_LN_INFER;
}
// residual operand of the EPI_DROP_RES_LN family: 0 = loaded (GemmArgs.R), 1 = re-derived, 2 = re-derived + dropout
constexpr int epi_res_mode(int epi) { return epi == EPI_DROP_RES_LN_RE ? 1 : epi == EPI_DROP_RES_LN_RED ? 2 : 0; }

struct GemmArgs {
  const void* A; const void* B; void* C;  // fp32, or bf16 where the storage mask says so
  int64_t lda, ldb, ldc;
  int64_t M; int N; int K;
  int k_chunk;            // split-K: split z handles [z*k_chunk, min(K,(z+1)*k_chunk)); 0 = whole K
  int nt_n, nt_m, nt_z;   // tiles along N, M and the number of K splits (the launch is one-dimensional: see tile_of)
  // Two-region row map of the whole-row (N == 128) kernels: M-tiles [0, nt_full) are BM rows tall, tiles [nt_full, nt_m)
  // `short_rows` (< BM) -- see row_tiles. nt_full == 0: every tile BM rows (the plain map).
  int nt_full, short_rows;
  const float* bias;      // [N] or null
  const float* R;         // residual / residual-grad [M,ldc] or null
  const void* P;          // pre-activation for gelu' [M,ldc]
  void* C2;               // pre-activation output for EPI_GELU
  int aux_grad;           // C2 / P hold gelu'(pre) instead of pre (XF_AUX_GELU_GRAD)
  uint32_t s16;           // XF_S16_* storage mask (bf16 policy only)
  float* bias_part;       // EPI_SPLITK with A' = dy^T: row sums of A' over this split's K range -> [splits][M]
  XfDropout drop;
  // EPI_DROP_RES_LN
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  float* Y; void* Y16; float* ln_mean; float* ln_rstd;  // (Y null: the fp32 output is not stored)
  // EPI_DROP_RES_LN_RE / _RED: the residual = LayerNorm(rp_pre; rp_mean, rp_rstd, rp_gamma, rp_beta), then rp_drop (_RED)
  const float* rp_pre; const float* rp_mean; const float* rp_rstd; const float* rp_gamma; const float* rp_beta;
  XfDropout rp_drop;
  // EPI_DX_LNBWD (ln_gamma as above; `drop` = the dropout of the Linear that fed the LayerNorm)
  const float* lnb_x; const float* lnb_mean; const float* lnb_rstd;  // saved LayerNorm input and statistics
  void* D16; float* lnb_partials;
  XfDropout drop2;  // EPI_DX_LNBWD: dropout that was applied to the LayerNorm OUTPUT (embedding site); off otherwise
};

// gelu of eight bf16 values riding in a float4, rounded back to bf16
__device__ __forceinline__ float4 xf_gelu_bf16x8(float4 raw4) {
  const uint4 raw = *reinterpret_cast<const uint4*>(&raw4);
  float4 lo = xf_bf16x4_to_f32(make_uint2(raw.x, raw.y)), hi = xf_bf16x4_to_f32(make_uint2(raw.z, raw.w));
  lo.x = xf_gelu(lo.x); lo.y = xf_gelu(lo.y); lo.z = xf_gelu(lo.z); lo.w = xf_gelu(lo.w);
  hi.x = xf_gelu(hi.x); hi.y = xf_gelu(hi.y); hi.z = xf_gelu(hi.z); hi.w = xf_gelu(hi.w);
  const uint2 a = xf_f32x4_to_bf16(lo), b = xf_f32x4_to_bf16(hi);
  const uint4 o = make_uint4(a.x, a.y, b.x, b.y);
  return *reinterpret_cast<const float4*>(&o);
}

// One operand tile (ROWS x BK, fp32 in memory) in flight in registers, then committed to an LDS image of the
// MFMA element type.
//   TRANS = false: memory [rows][K]  -> image [ROWS][BK + pad]  (K-contiguous; fragments are 16-byte row reads)
//   TRANS = true : memory [K][rows]  -> image [BK][ROWS + pad]  (natural layout, coalesced 8/16-byte commits);
//                  the MFMA fragment (8 consecutive k for one row) is then a COLUMN of the image: two
//                  ds_read_b64_tr_b16 for bf16, one ds_read_b32 for fp32 -- no scattered, bank-conflicting
//                  transposing stores (they were 63-78 % of the LDS cycles of the dX / dW GEMMs).
template <class P, int ROWS, int BK, bool TRANS>
struct OperandTile {
  using elem = typename P::elem;
  static constexpr int N4 = ROWS * BK / 4 / 256;  // float4 per thread
  // TRANS bf16: row stride = 64 B (mod 256 B) so the 4 rows of a transposed read hit 4 distinct bank windows
  static constexpr int LD = TRANS ? (sizeof(elem) == 2 ? ROWS + 32 : ROWS + 4) : xf_ld<P>(BK);
  static constexpr int IMG_ELEMS = TRANS ? BK * LD : ROWS * LD;
  float4 reg[N4];

  // bf16 storage: 16-byte pieces (8 elements along the contiguous dimension, which is a feature dimension: a multiple
  // of 8) -- N8 pieces per thread, the raw bytes ride in reg[i]. (8-byte pieces moved half the bytes per vector
  // memory instruction; these GEMMs are bound by the CU's memory-instruction throughput, not by HBM or L2.)
  static constexpr int N8 = ROWS * BK / 8 / 256;
  __device__ __forceinline__ void load16(const __bf16* src, int64_t ld, int64_t row0, int64_t rows_total, int k0,
                                         int kend) {
    static_assert(N8 >= 1, "tile too small for 16-byte bf16 pieces");
    const int tid = threadIdx.x;
    constexpr int CH = TRANS ? ROWS / 8 : BK / 8;
#pragma unroll
    for (int i = 0; i < N8; ++i) {
      const int c = tid + i * 256;
      const int a = c / CH, b8 = (c % CH) * 8;
      const int64_t gr = row0 + (TRANS ? b8 : a);
      const int gk = k0 + (TRANS ? a : b8);
      uint4 raw = make_uint4(0u, 0u, 0u, 0u);
      if (gr < rows_total && gk < kend)
        raw = *reinterpret_cast<const uint4*>(TRANS ? src + (int64_t)gk * ld + gr : src + gr * ld + gk);
      reg[i] = *reinterpret_cast<const float4*>(&raw);
    }
  }
  template <bool S16>
  __device__ __forceinline__ void load(const void* srcv, int64_t ld, int64_t row0, int64_t rows_total, int k0,
                                       int kend) {
    if (S16) {
      load16(reinterpret_cast<const __bf16*>(srcv), ld, row0, rows_total, k0, kend);
      return;
    }
    const float* src = reinterpret_cast<const float*>(srcv);
    const int tid = threadIdx.x;
    if (!TRANS) {
      constexpr int CH = BK / 4;  // 16-byte chunks per row
#pragma unroll
      for (int i = 0; i < N4; ++i) {
        const int c = tid + i * 256;
        const int r = c / CH, kk = (c % CH) * 4;
        const int64_t gr = row0 + r;
        const int gk = k0 + kk;
        float4 v = make_float4(0, 0, 0, 0);
        if (gr < rows_total && gk < kend) {
          const float* p = src + gr * ld + gk;
          if (gk + 3 < kend) v = *reinterpret_cast<const float4*>(p);
          else { v.x = p[0]; if (gk + 1 < kend) v.y = p[1]; if (gk + 2 < kend) v.z = p[2]; }
        }
        reg[i] = v;
      }
    } else {
      constexpr int R4 = ROWS / 4;
#pragma unroll
      for (int i = 0; i < N4; ++i) {
        const int c = tid + i * 256;
        const int k = c / R4, rc = (c % R4) * 4;
        const int64_t gr = row0 + rc;
        const int gk = k0 + k;
        float4 v = make_float4(0, 0, 0, 0);
        if (gk < kend && gr < rows_total) {
          const float* p = src + (int64_t)gk * ld + gr;
          if (gr + 3 < rows_total) v = *reinterpret_cast<const float4*>(p);
          else { v.x = p[0]; if (gr + 1 < rows_total) v.y = p[1]; if (gr + 2 < rows_total) v.z = p[2]; }
        }
        reg[i] = v;
      }
    }
  }
  // TRANS tiles only: every thread's pieces cover the SAME 4 operand rows (256 % (ROWS/4) == 0) at different k:
  // acc += the pieces in flight = this thread's share of the row sums over k (the bias gradient when A' = dy^T)
  // (fp32 pieces: 4 rows -> acc[0]; bf16 pieces: 8 rows -> acc[0], acc[1])
  template <bool S16>
  __device__ __forceinline__ void add_rowsum(float4 (&acc)[2]) const {
    if (S16) {
#pragma unroll
      for (int i = 0; i < N8; ++i) {
        const uint4 raw = *reinterpret_cast<const uint4*>(&reg[i]);
        const float4 lo = xf_bf16x4_to_f32(make_uint2(raw.x, raw.y)), hi = xf_bf16x4_to_f32(make_uint2(raw.z, raw.w));
        acc[0].x += lo.x; acc[0].y += lo.y; acc[0].z += lo.z; acc[0].w += lo.w;
        acc[1].x += hi.x; acc[1].y += hi.y; acc[1].z += hi.z; acc[1].w += hi.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < N4; ++i) {
        const float4 v = reg[i];
        acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w;
      }
    }
  }
  template <bool S16>
  __device__ __forceinline__ void commit(elem* dst) const {
    const int tid = threadIdx.x;
    if (S16) {
      constexpr int CH = TRANS ? ROWS / 8 : BK / 8;
#pragma unroll
      for (int i = 0; i < N8; ++i) {
        const int c = tid + i * 256;
        *reinterpret_cast<float4*>(dst + (c / CH) * LD + (c % CH) * 8) = reg[i];
      }
    } else {
      constexpr int CH = TRANS ? ROWS / 4 : BK / 4;
#pragma unroll
      for (int i = 0; i < N4; ++i) {
        const int c = tid + i * 256;
        xf_store4<P>(dst + (c / CH) * LD + (c % CH) * 4, reg[i]);
      }
    }
  }
};

// MFMA fragments of one 32-row block (rows row0..row0+31 of the operand) for the k-step starting at k0.
template <class P, bool TRANS>
struct Frag;
template <>
struct Frag<PrecBF16, false> {
  using type = bf16x8;
  static constexpr int KS = 16;
  __device__ static __forceinline__ type get(const __bf16* img, int ld, int row0, int k0) {
    const int l = xf_lane();
    return *reinterpret_cast<const bf16x8*>(img + (row0 + (l & 31)) * ld + k0 + 8 * (l >> 5));
  }
};
template <>
struct Frag<PrecBF16, true> {
  using type = bf16x8;
  static constexpr int KS = 16;
  // image [k][row]: lane (row i = l&31, h = l>>5) needs IMG[k0 + 8h + 0..7][row0 + i]: per 16-lane group two
  // transposed 4-row x 16-column block reads (lane 4q+p supplies row q, columns 4p..4p+3).
  __device__ static __forceinline__ type get(const __bf16* img, int ld, int row0, int k0) {
    const int l = xf_lane(), g16 = l >> 4, li = l & 15, q = li >> 2, p = li & 3;
    const __bf16* base = img + (k0 + 8 * (g16 >> 1) + q) * ld + row0 + 16 * (g16 & 1) + 4 * p;
    union { xf_s16x4 v[2]; bf16x8 f; } a;
    a.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) xf_s16x4*)(base));
    a.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) xf_s16x4*)(base + 4 * ld));
    return a.f;
  }
};
template <>
struct Frag<PrecF32, false> {
  using type = float;
  static constexpr int KS = 2;
  __device__ static __forceinline__ type get(const float* img, int ld, int row0, int k0) {
    const int l = xf_lane();
    return img[(row0 + (l & 31)) * ld + k0 + (l >> 5)];
  }
};
template <>
struct Frag<PrecF32, true> {
  using type = float;
  static constexpr int KS = 2;
  __device__ static __forceinline__ type get(const float* img, int ld, int row0, int k0) {
    const int l = xf_lane();
    return img[(k0 + (l >> 5)) * ld + row0 + (l & 31)];
  }
};
__device__ __forceinline__ f32x16 xf_mma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 xf_mma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// XCD-aware tile order. Workgroups are dealt round-robin over the 8 XCDs (each with its own L2), so workgroups d and
// d + 8 share an L2 and d, d + 1 do not. With the plain (n fastest) order the N-tiles of one M-tile -- which all read
// the SAME A rows -- land on different XCDs and every one of them fetches A from the fabric again: measured at
// T = 102 400 (FETCH_SIZE), the FFN1 GEMM fetched 206 MB for 52 MB of activations, the gelu' GEMM 308 MB for 131 MB.
// Here the workgroups of one XCD (d % 8) walk the N-tiles of one M-tile (one K split for the dW GEMMs) back to back,
// so the re-reads hit that XCD's L2.
struct TileIdx { int n, m, z; bool valid; };
__device__ __forceinline__ TileIdx tile_of(const int nt_n, const int nt_m, const int nt_z, const int d = blockIdx.x) {
  const int xcd = d & 7, slot = d >> 3;
  TileIdx t;
  if (nt_z > 1) {  // split-K: the (m, n) tiles of one split share its A and B slices
    const int per = nt_n * nt_m;
    t.z = (slot / per) * 8 + xcd;
    const int r = slot % per;
    t.n = r % nt_n;
    t.m = r / nt_n;
    t.valid = t.z < nt_z;
  } else {
    t.z = 0;
    t.n = slot % nt_n;
    t.m = (slot / nt_n) * 8 + xcd;
    t.valid = t.m < nt_m;
  }
  return t;
}

// Rows of M-tile m under the two-region map: first row, and the tile's row limit written into g.M (every row test of the
// kernels and their epilogues is `m < g.M` on the workgroup's own copy of the arguments, so a short tile is a tile whose
// rows past the limit are masked exactly like the rows past the end of the matrix).
__device__ __forceinline__ int64_t xf_tile_rows(GemmArgs& g, const int m, const int BM) {
  if (g.nt_full <= 0 || m < g.nt_full) return (int64_t)m * BM;
  const int64_t m0 = (int64_t)g.nt_full * BM + (int64_t)(m - g.nt_full) * g.short_rows;
  g.M = min(g.M, m0 + g.short_rows);
  return m0;
}
// The per-CU tile count of a whole-row kernel: M / BM tiles over the chip's CUs is rarely whole (1600 tiles over 256 CUs =
// 6.25: 64 CUs run a seventh tile while 192 idle -- 101 -> 119 us on the fused FFN forward). When the
// rows left over after `per_cu` full tiles per CU are few (<= 32 per CU), they are dealt as ONE short tile per CU instead
// of a few full ones on a few CUs: the short tiles are dispatched last and land where slots free up. Rows are
// independent in these kernels (GEMM rows, LayerNorm rows): outputs are bit-identical under any row map.
static int xf_num_cus() {
  static const int n = [] {
    int dev = 0, cu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
    return cu > 0 ? cu : 256;
  }();
  return n;
}
// The M-tiles of a whole-row kernel for M rows on `cus` compute units (GemmArgs nt_m, nt_full, short_rows). Pure.
struct RowTiles { int nt_m, nt_full, short_rows; };
static RowTiles row_tiles(int64_t M, int BM, int64_t cus, bool short_on) {
  RowTiles t{(int)((M + BM - 1) / BM), 0, 0};
  // MEASURED AND NOT KEPT AS THE DEFAULT (round 3, batch 512, alternating runs on one box): 3.297 / 3.312 / 3.290 ms per step
  // with the short tiles against 3.278 / 3.288 / 3.279 with the plain map; per kernel 103.3 vs 101.0 us (fused FFN forward),
  // 126.4 vs 127.0 (backward), 62.6 vs 61.1, 43.6 vs 43.5 (the two LayerNorm-fused GEMMs). A lone short tile costs about what
  // a lone full tile costs -- its time is the latency chain of staging, K loop and epilogue, not its rows -- so dealing the
  // tail over all CUs moves it around without shortening it. XFMR_ROW_TILES_SHORT=1 turns the map on (experiments).
  if (!short_on || cus < 1) return t;
  const int64_t per_cu = M / (BM * cus), rem = M - per_cu * BM * cus;
  if (per_cu < 1 || rem <= 0 || rem > 32 * cus) return t;
  const int64_t each = (((rem + cus - 1) / cus) + 15) / 16 * 16;  // rows per short tile: a multiple of 16
  t.nt_full = (int)(per_cu * cus);
  t.short_rows = (int)each;
  t.nt_m = t.nt_full + (int)((rem + each - 1) / each);
  return t;
}

// Epilogue of a 64 x 128 tile that spans whole output rows (N == 128), computed by 2 x 2 waves (wave = 32 rows x 64
// columns, acc[j] = its 32 x 32 block j): bias + dropout + residual -> C (the pre-LayerNorm sum, kept for the backward),
// LayerNorm -> Y (fp32) / Y16 (bf16 GEMM operand), mean / rstd per row. `smem`: >= 4 strips of 16 x 68 floats + 128
// floats, free of live data (the callers alias their operand images after a barrier).
// KEEP = false (the forward-only forms): what only a backward reads -- C, mean, rstd -- is not stored.
template <int RES, bool KEEP = true>  // RES: epi_res_mode
__device__ __forceinline__ void epi_drop_res_ln_64x128(const f32x16 (&acc)[2], unsigned char* smem, const GemmArgs& g,
                                                       const int64_t m0, const int wid, const int lane) {
  // The wave owns 32 rows x 64 columns; a row's other 64 columns are with the partner wave (wc ^ 1). Lane ->
  // (row = prow + 4 ps + 16 hf, columns c0 .. c0 + 3): 16 lanes per row, 8 rows per lane, all kept in registers.
  constexpr int LPRL = 16, RPPL = 4, NPL = 4, WM = 32, WN = 64, NI = 2, SCR_LD = WN + 4;
  constexpr int64_t LDC = 128;  // (N == ldc == 128 by construction: offsets are shifts, not 64-bit multiplies)
  const int wr = wid >> 1, wc = wid & 1;
  float* const scr = reinterpret_cast<float*>(smem) + wid * (16 * SCR_LD);
  float* const red = reinterpret_cast<float*>(smem) + 4 * 16 * SCR_LD;  // [2 wr][2 wc][32 rows] x 2 (sum, sumsq)
  const int prow = lane / LPRL, li = lane % LPRL, c0 = li * 4;
  const int n = wc * WN + c0;  // (n0 == 0: one N tile)
  const float4 bias = g.bias ? *reinterpret_cast<const float4*>(g.bias + n) : make_float4(0, 0, 0, 0);
  float4 gp = make_float4(0, 0, 0, 0), bp = gp;  // gamma / beta of the LayerNorm whose output is the residual
  if constexpr (RES != 0) {
    gp = *reinterpret_cast<const float4*>(g.rp_gamma + n);
    bp = *reinterpret_cast<const float4*>(g.rp_beta + n);
  }
  float4 vv[2][NPL];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const int64_t mb = m0 + wr * WM + 16 * hf;
    float4 aux[NPL];
    float amu[NPL], ars[NPL];
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      aux[ps] = make_float4(0, 0, 0, 0);
      amu[ps] = ars[ps] = 0.f;
      const int64_t m = mb + prow + RPPL * ps;
      if constexpr (RES == 0) {
        if (m < g.M) aux[ps] = *reinterpret_cast<const float4*>(g.R + m * LDC + n);
      } else if (m < g.M) {
        aux[ps] = *reinterpret_cast<const float4*>(g.rp_pre + m * LDC + n);
        amu[ps] = g.rp_mean[m];
        ars[ps] = g.rp_rstd[m];
      }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 8; ++r)
        scr[(xf_acc_row(8 * hf + r, lane) - 16 * hf) * SCR_LD + j * 32 + (lane & 31)] = acc[j][8 * hf + r];
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const int row = prow + RPPL * ps;
      const int64_t m = mb + row;
      float4 v = *reinterpret_cast<const float4*>(scr + row * SCR_LD + c0);
      v.x += bias.x; v.y += bias.y; v.z += bias.z; v.w += bias.w;
      if (g.drop.on) {
        xf_drop4(g.drop, (uint32_t)m, (uint32_t)(n), v);
      }
      float4 res = aux[ps];
      if constexpr (RES != 0) {
        XF_PIN_SCALAR(amu[ps]);  // (per-row scalars broadcast into four-wide arithmetic: see XF_PIN_SCALAR)
        XF_PIN_SCALAR(ars[ps]);
        res = xf_ln_out_drop4<RES == 2>(res, amu[ps], ars[ps], gp, bp, g.rp_drop, (uint32_t)m, (uint32_t)(n));
      }
      v.x += res.x; v.y += res.y; v.z += res.z; v.w += res.w;
      if (m >= g.M) v = make_float4(0, 0, 0, 0);
      else if constexpr (KEEP) *reinterpret_cast<float4*>(reinterpret_cast<float*>(g.C) + m * LDC + n) = v;
      vv[hf][ps] = v;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
  XF_EPI_BARRIER();  // every wave is done with its scratch strip before `red` (behind the strips) is written
  auto row_reduce = [&](float x) { return xf_row16_sum(x); };  // the 16 lanes that hold a row's 64 columns of this wave
  float mean[2][NPL];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const float4 v = vv[hf][ps];
      const float s = row_reduce((v.x + v.y) + (v.z + v.w));
      if (li == 0) red[(wr * 2 + wc) * 32 + 16 * hf + prow + RPPL * ps] = s;
    }
  XF_EPI_BARRIER();
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const int rr = 16 * hf + prow + RPPL * ps;
      mean[hf][ps] = (red[(wr * 2) * 32 + rr] + red[(wr * 2 + 1) * 32 + rr]) * (1.f / 128.f);
    }
  XF_EPI_BARRIER();
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      float4& v = vv[hf][ps];
      const float mu = mean[hf][ps];
      v.x -= mu; v.y -= mu; v.z -= mu; v.w -= mu;
      const float s = row_reduce((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
      if (li == 0) red[(wr * 2 + wc) * 32 + 16 * hf + prow + RPPL * ps] = s;
    }
  XF_EPI_BARRIER();
  const float4 gm = *reinterpret_cast<const float4*>(g.ln_gamma + n);
  const float4 bt = *reinterpret_cast<const float4*>(g.ln_beta + n);
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const int rr = 16 * hf + prow + RPPL * ps;
      const int64_t m = m0 + wr * WM + rr;
      const float var = (red[(wr * 2) * 32 + rr] + red[(wr * 2 + 1) * 32 + rr]) * (1.f / 128.f);
      const float rs = rsqrtf(var + g.ln_eps);
      if (m >= g.M) continue;
      const float4 o = xf_ln_affine4(vv[hf][ps], rs, gm, bt);
      if (g.Y) *reinterpret_cast<float4*>(g.Y + m * LDC + n) = o;  // (null: the consumer re-derives it)
      if (g.Y16) xf_st4<true>(g.Y16, m * LDC + n, o);
      if constexpr (KEEP) {
        if (wc == 0 && li == 0) {
          g.ln_mean[m] = mean[hf][ps];
          g.ln_rstd[m] = rs;
        }
      }
    }
}

// Epilogue of a 64 x 128 dX tile whose rows are gradients of a LayerNorm OUTPUT (2 x 2 waves, acc[j] = the wave's 32 x 32
// block j): + residual gradient (dropout of the LayerNorm output where drop2 is on) -> LayerNorm backward -> C (gradient of
// the LayerNorm input, fp32), D16 (its dropout-scaled bf16 copy: the gradient of the Linear that fed the LayerNorm), one
// partial record [3][128] (d gamma, d beta, d bias) per tile. `smem`: >= 4 strips of 16 x 68 floats + 896 floats.
__device__ __forceinline__ void epi_dx_lnbwd_64x128(const f32x16 (&acc)[2], unsigned char* smem, const GemmArgs& g,
                                                    const int64_t m0, const int tile_m, const int wid, const int lane) {
  // Same lane map as EPI_DROP_RES_LN: lane -> (row = prow + 4 ps + 16 hf, columns c0 .. c0 + 3). A half strip
  // (16 rows) at a time: the two row sums of the LayerNorm backward are exchanged with the partner wave per half.
  constexpr int LPRL = 16, RPPL = 4, NPL = 4, WM = 32, WN = 64, NI = 2, SCR_LD = WN + 4;
  constexpr int64_t LDC = 128;  // (N == ldc == 128 by construction: offsets are shifts, not 64-bit multiplies)
  const int wr = wid >> 1, wc = wid & 1;
  float* const scr = reinterpret_cast<float*>(smem) + wid * (16 * SCR_LD);
  float* const red = reinterpret_cast<float*>(smem) + 4 * 16 * SCR_LD;  // [2 hf][2 wr][2 wc][16 rows][2]
  float* const colred = red + 2 * 2 * 2 * 16 * 2;                       // [2 wr][3][128]
  const int prow = lane / LPRL, li = lane % LPRL, c0 = li * 4;
  const int n = wc * WN + c0;
  const float4 gam = *reinterpret_cast<const float4*>(g.ln_gamma + n);
  float4 dgam = make_float4(0, 0, 0, 0), dbet = dgam, dbias = dgam;
  auto row_reduce = [&](float x) { return xf_row16_sum(x); };
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const int64_t mb = m0 + wr * WM + 16 * hf;
    float4 aux[NPL], xv[NPL];
    float mu[NPL], rs[NPL];
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      aux[ps] = xv[ps] = make_float4(0, 0, 0, 0);
      mu[ps] = rs[ps] = 0.f;
      const int64_t m = mb + prow + RPPL * ps;
      if (m < g.M) {
        if (g.R) aux[ps] = *reinterpret_cast<const float4*>(g.R + m * LDC + n);
        xv[ps] = *reinterpret_cast<const float4*>(g.lnb_x + m * LDC + n);
        mu[ps] = g.lnb_mean[m];
        rs[ps] = g.lnb_rstd[m];
      }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        // Second line of defence (round 4; the first is the pinned per-row scalars below + the build's ISA audit): every
        // build of this epilogue that produced intermittently wrong rows stored the strip straight
        // from the MFMA accumulator file (ds_write_b32 v, aN); here each value passes through an ordinary VGPR first
        // (v_accvgpr_read_b32), so the LDS store no longer depends on the AGPR read port beside resident MFMA waves.
        // 16 moves per half strip: within noise of the kernel's time (measured with the tile's ~900 vector instructions).
        float v = acc[j][8 * hf + r];
#if !(XF_LN_DIAG & 32)
        XF_PIN_SCALAR(v);
#endif
        scr[(xf_acc_row(8 * hf + r, lane) - 16 * hf) * SCR_LD + j * 32 + (lane & 31)] = v;
      }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    float4 gv[NPL], xh[NPL];
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const int row = prow + RPPL * ps;
      const int64_t m = mb + row;
      float4 dy = *reinterpret_cast<const float4*>(scr + row * SCR_LD + c0);
      dy.x += aux[ps].x; dy.y += aux[ps].y; dy.z += aux[ps].z; dy.w += aux[ps].w;
      if (g.drop2.on) {
        xf_drop4(g.drop2, (uint32_t)m, (uint32_t)(n), dy);
      }
      if (m >= g.M) dy = make_float4(0, 0, 0, 0);
      float4 h;
#if !(XF_LN_DIAG & 32)
      // each per-row scalar is pinned in a 32-bit VGPR of its own: see XF_PIN_SCALAR
      XF_PIN_SCALAR(mu[ps]);
      XF_PIN_SCALAR(rs[ps]);
#endif
      h.x = (xv[ps].x - mu[ps]) * rs[ps]; h.y = (xv[ps].y - mu[ps]) * rs[ps];
      h.z = (xv[ps].z - mu[ps]) * rs[ps]; h.w = (xv[ps].w - mu[ps]) * rs[ps];
      dgam.x += dy.x * h.x; dgam.y += dy.y * h.y; dgam.z += dy.z * h.z; dgam.w += dy.w * h.w;
      dbet.x += dy.x; dbet.y += dy.y; dbet.z += dy.z; dbet.w += dy.w;
      float4 gg;
      gg.x = dy.x * gam.x; gg.y = dy.y * gam.y; gg.z = dy.z * gam.z; gg.w = dy.w * gam.w;
      gv[ps] = gg; xh[ps] = h;
      const float s1 = row_reduce((gg.x + gg.y) + (gg.z + gg.w));
      const float s2 = row_reduce((gg.x * h.x + gg.y * h.y) + (gg.z * h.z + gg.w * h.w));
      if (li == 0) {
        float* rp = red + ((((hf * 2 + wr) * 2 + wc) * 16) + row) * 2;
        rp[0] = s1; rp[1] = s2;
      }
    }
    XF_EPI_BARRIER();  // (also: the scratch strip may be overwritten by the next half)
#pragma unroll
    for (int ps = 0; ps < NPL; ++ps) {
      const int row = prow + RPPL * ps;
      const int64_t m = mb + row;
      const float* r0 = red + ((((hf * 2 + wr) * 2 + 0) * 16) + row) * 2;
      const float* r1 = red + ((((hf * 2 + wr) * 2 + 1) * 16) + row) * 2;
      const float mg = (r0[0] + r1[0]) * (1.f / 128.f), mgx = (r0[1] + r1[1]) * (1.f / 128.f);
      if (m >= g.M) continue;
      const float4 gg = gv[ps], h = xh[ps];
      float4 d;
      d.x = rs[ps] * (gg.x - mg - h.x * mgx); d.y = rs[ps] * (gg.y - mg - h.y * mgx);
      d.z = rs[ps] * (gg.z - mg - h.z * mgx); d.w = rs[ps] * (gg.w - mg - h.w * mgx);
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(g.C) + m * LDC + n) = d;
      float4 dl = d;
      if (g.drop.on) {
        xf_drop4(g.drop, (uint32_t)m, (uint32_t)(n), dl);
      }
      if (g.D16) xf_st4<true>(g.D16, m * LDC + n, dl);
      dbias.x += dl.x; dbias.y += dl.y; dbias.z += dl.z; dbias.w += dl.w;
    }
  }
  // column sums of the workgroup's 64 rows: the 4 row groups of the wave (lanes with equal li), then the two
  // waves that share the columns (wr = 0, 1), fixed order
  auto fold = [&](float4& v) {
#pragma unroll
    for (int o = LPRL; o < 64; o <<= 1) {
      v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64);
      v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
    }
  };
  fold(dgam); fold(dbet); fold(dbias);
  if (prow == 0) {
    *reinterpret_cast<float4*>(&colred[(wr * 3 + 0) * 128 + n]) = dgam;
    *reinterpret_cast<float4*>(&colred[(wr * 3 + 1) * 128 + n]) = dbet;
    *reinterpret_cast<float4*>(&colred[(wr * 3 + 2) * 128 + n]) = dbias;
  }
  XF_EPI_BARRIER();
  for (int o = threadIdx.x; o < 3 * 128; o += 256)
    g.lnb_partials[(int64_t)tile_m * 3 * 128 + o] = colred[o] + colred[3 * 128 + o];
}

// S = XF_S16_* storage mask (compile time: a runtime switch between the fp32 and bf16 load paths cost the
// forward / dX GEMMs 15-80 %).
template <class P, int BM, int BN, int BK, bool TA, bool TB, int EPI, uint32_t S>
// (Launch bound of the two LayerNorm-fused epilogues: three waves per SIMD -- a speed choice, 129.4 k against 127.6 k
//  sequences/s with the default bound. Round 1 believed this bound was what made them run-to-run deterministic; the
//  cause was the packed-fp32 op_sel form described at XF_PIN_SCALAR above, which the default-bound schedule happened
//  to contain and this one did not. With the scalars pinned, both bounds are bit-reproducible.)
__device__ __forceinline__ void gemm_body(const GemmArgs& g_in, const int bid) {  // bid: workgroup index within THIS GEMM
  GemmArgs g = g_in;  // (device-side step counter -> dropout key: xf_drop_resolve)
  if (EPI != EPI_SPLITK) XF_CHAIN_PRIO();
  g.drop = xf_drop_resolve(g.drop); g.drop2 = xf_drop_resolve(g.drop2);
  if constexpr (EPI == EPI_DROP_RES_LN_RED) g.rp_drop = xf_drop_resolve(g.rp_drop);
  using elem = typename P::elem;
  using TileA = OperandTile<P, BM, BK, TA>;
  using TileB = OperandTile<P, BN, BK, TB>;
  using FA = Frag<P, TA>;
  using FB = Frag<P, TB>;
  constexpr bool a16 = S & XF_S16_A, b16 = S & XF_S16_B, c16 = S & XF_S16_C, p16 = S & XF_S16_P;
  static_assert(S == 0 || sizeof(elem) == 2, "bf16 storage needs the bf16 policy");
  constexpr int SCR_LD = (BN / 2) + 4;  // per-wave 16 x (BN/2) fp32 transposition scratch (rows 16-byte aligned)
  constexpr size_t OPER_BYTES = (size_t)(TileA::IMG_ELEMS + TileB::IMG_ELEMS) * sizeof(elem);
  constexpr size_t SCR_BYTES = (size_t)4 * 16 * SCR_LD * sizeof(float);
  // the LayerNorm-fused epilogues keep their exchange records BEHIND the four scratch strips: row sums [4 waves][32]
  // (EPI_DROP_RES_LN); [2 hf][2 wr][2 wc][16][2] row sums + [2 wr][3][128] column records (EPI_DX_LNBWD). With 32-deep
  // K slices the operand images are smaller than strips + records, so the records are part of the size.
  constexpr size_t RED_BYTES = epi_res_ln(EPI) ? (size_t)4 * 32 * sizeof(float)
                               : EPI == EPI_DX_LNBWD  ? (size_t)(2 * 2 * 2 * 16 * 2 + 2 * 3 * 128) * sizeof(float)
                                                      : 0;
  constexpr size_t EPI_BYTES = SCR_BYTES + RED_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[OPER_BYTES > EPI_BYTES ? OPER_BYTES : EPI_BYTES];
  elem* const sA = reinterpret_cast<elem*>(smem);
  elem* const sB = sA + TileA::IMG_ELEMS;

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 32, NI = WN / 32;
  const TileIdx tix = tile_of(g.nt_n, g.nt_m, g.nt_z, bid);
  if (!tix.valid) return;  // (whole workgroup: the grid is padded to a multiple of 8 M-tiles / K splits)
  const int64_t m0 = (epi_res_ln(EPI) || EPI == EPI_DX_LNBWD) ? xf_tile_rows(g, tix.m, BM) : (int64_t)tix.m * BM;
  const int n0 = tix.n * BN;
  int kbeg = 0, kend = g.K;
  if (g.k_chunk > 0) {
    kbeg = tix.z * g.k_chunk;
    kend = min(g.K, kbeg + g.k_chunk);
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // XF_GEMM_PF operand slices in flight in registers. Measured with two (both slices of a K = 128 GEMM issued up front):
  // 58 more VGPRs, one workgroup fewer per CU, 3.77 against 3.67 ms/step -- co-resident workgroups hide the round
  // trips better than a deeper prefetch inside one; a launch bound of 5 waves for the forward GEMMs (96 VGPRs) changed
  // nothing (3.758 / 3.759). One slice it stays.
  constexpr int PF = EPI == EPI_SPLITK ? XF_DW_PF : XF_GEMM_PF;  // (split-K dW: a dozen 128-deep slices; one workgroup more per CU wins)
  TileA ta[PF];
  TileB tb[PF];
  const bool do_bias = (EPI == EPI_SPLITK) && TA && g.bias_part != nullptr && tix.n == 0;
  float4 bsum[2] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
  const int nk = (kend - kbeg + BK - 1) / BK;
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (p < nk) {
      ta[p].template load<a16>(g.A, g.lda, m0, g.M, kbeg + p * BK, kend);
      tb[p].template load<b16>(g.B, g.ldb, n0, g.N, kbeg + p * BK, kend);
    }
  auto k_slice = [&](TileA& tac, TileB& tbc, const int kt) {
    __syncthreads();
    if (do_bias) tac.template add_rowsum<a16>(bsum);
    tac.template commit<a16>(sA);
    tbc.template commit<b16>(sB);
    __syncthreads();
    if (kt + PF < nk) {  // the slice PF steps ahead goes into the registers just committed
      tac.template load<a16>(g.A, g.lda, m0, g.M, kbeg + (kt + PF) * BK, kend);
      tbc.template load<b16>(g.B, g.ldb, n0, g.N, kbeg + (kt + PF) * BK, kend);
    }
#pragma unroll
    for (int k0 = 0; k0 < BK; k0 += FA::KS) {
      typename FA::type fa[MI];
      typename FB::type fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = FA::get(sA, TileA::LD, wr * WM + i * 32, k0);
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = FB::get(sB, TileB::LD, wc * WN + j * 32, k0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = xf_mma(fa[i], fb[j], acc[i][j]);
    }
  };
#pragma unroll 1
  for (int kt0 = 0; kt0 < nk; kt0 += PF) {
    k_slice(ta[0], tb[0], kt0);
    if constexpr (PF > 1) {
      if (kt0 + 1 < nk) k_slice(ta[PF - 1], tb[PF - 1], kt0 + 1);
    }
  }

  // ---- epilogue ----------------------------------------------------------------------------------------------
  // The wave's 32 x (NI*32) accumulator strip goes through a per-wave LDS transposition so that every global access
  // of the epilogue (C, residual, pre-activation) is a 16-byte (8-byte for bf16) piece of a row-contiguous run that
  // covers the wave's whole column range: full 128-byte lines even for bf16 outputs when the wave owns 64 columns
  // (one wave instruction = 4-8 rows x 128-256 B instead of 2 rows x 32 scattered 4- or 2-byte elements).
  __syncthreads();  // everyone is done with the operand images the scratch aliases
  if constexpr (epi_res_ln(EPI)) {
    if constexpr (BM == 64 && BN == 128)
      epi_drop_res_ln_64x128<epi_res_mode(EPI), EPI != EPI_DROP_RES_LN_INFER>(acc[0], smem, g, m0, wid, lane);
    return;
  }
  if constexpr (EPI == EPI_DX_LNBWD) {
    if constexpr (BM == 64 && BN == 128) epi_dx_lnbwd_64x128(acc[0], smem, g, m0, tix.m, wid, lane);
    return;
  }
  if (do_bias) {  // combine the threads that share an operand row group (4 rows fp32, 8 rows bf16), fixed order
    constexpr int RQ = a16 ? 8 : 4, RG = BM / RQ, G = 256 / RG;
    float4* red = reinterpret_cast<float4*>(smem);
    red[threadIdx.x] = bsum[0];
    if (a16) red[256 + threadIdx.x] = bsum[1];
    __syncthreads();
    if (threadIdx.x < RG) {
#pragma unroll
      for (int half = 0; half < (a16 ? 2 : 1); ++half) {
        float4 s = red[half * 256 + threadIdx.x];
#pragma unroll
        for (int q = 1; q < G; ++q) {
          const float4 v = red[half * 256 + threadIdx.x + q * RG];
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const int64_t m = m0 + RQ * threadIdx.x + 4 * half;
        float* dst = g.bias_part + (int64_t)tix.z * g.M + m;
        if (m < g.M) dst[0] = s.x;
        if (m + 1 < g.M) dst[1] = s.y;
        if (m + 2 < g.M) dst[2] = s.z;
        if (m + 3 < g.M) dst[3] = s.w;
      }
    }
    __syncthreads();
  }
  constexpr int CW = NI * 32;        // columns this wave owns
  // columns per lane: one 16-byte piece of the OUTPUT row -- 4 fp32 or 8 bf16 (8-byte bf16 pieces moved half the
  // bytes per vector-memory instruction)
  constexpr bool out16 = c16 && EPI != EPI_SPLITK;
  constexpr int CPL = out16 ? 8 : 4, Q = CPL / 4;
  constexpr int LPR = CW / CPL;      // lanes per row
  constexpr int RPP = 64 / LPR;      // rows per pass
  constexpr int NPASS = 16 / RPP;    // passes per half strip (16 rows: the scratch stays below the operand images)
  float* const scr = reinterpret_cast<float*>(smem) + wid * (16 * SCR_LD);
  const int64_t zoff = (EPI == EPI_SPLITK) ? (int64_t)tix.z * g.M * g.ldc : 0;
  const int prow = lane / LPR, c0 = (lane % LPR) * CPL;
  const void* aux_src = (EPI == EPI_GELU_GRAD) ? g.P : (const void*)g.R;
  constexpr bool aux16 = (EPI == EPI_GELU_GRAD) && p16;
  constexpr bool has_aux = (EPI == EPI_STORE || EPI == EPI_DROP_RES || EPI == EPI_GELU_GRAD);
  const int n = n0 + wc * WN + c0;
  const bool ncol = n < g.N;  // (N is a multiple of CPL: checked by the callers)
  float4 bias[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    bias[q] = make_float4(0, 0, 0, 0);
    if (EPI != EPI_SPLITK && EPI != EPI_GELU_GRAD && g.bias && ncol)
      bias[q] = *reinterpret_cast<const float4*>(g.bias + n + 4 * q);
  }
  auto ld_aux = [&](int64_t idx, float4 (&dst)[Q]) {
    if (aux16 && Q == 2) {
      const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(aux_src) + idx);
      dst[0] = xf_bf16x4_to_f32(make_uint2(raw.x, raw.y));
      dst[Q - 1] = xf_bf16x4_to_f32(make_uint2(raw.z, raw.w));
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q) dst[q] = xf_ld4<aux16>(aux_src, idx + 4 * q);
    }
  };
  auto st_out = [&](void* base, int64_t idx, const float4 (&v)[Q]) {
    if (out16) {  // Q == 2: eight bf16 = one 16-byte store
      const uint2 lo = xf_f32x4_to_bf16(v[0]), hi = xf_f32x4_to_bf16(v[Q - 1]);
      *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(base) + idx) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else {
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + idx) = v[0];
    }
  };
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {  // accumulator registers 8*hf .. 8*hf+7 hold the strip's rows 16*hf .. 16*hf+15
      const int64_t mb = m0 + wr * WM + i * 32 + 16 * hf;
      // issue the epilogue operand loads first: their latency hides under the LDS round trip
      float4 aux[NPASS][Q];
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
#pragma unroll
        for (int q = 0; q < Q; ++q) aux[ps][q] = make_float4(0, 0, 0, 0);
        const int64_t m = mb + prow + RPP * ps;
        if (has_aux && aux_src && ncol && m < g.M) ld_aux(m * g.ldc + n, aux[ps]);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 8; ++r)
          scr[(xf_acc_row(8 * hf + r, lane) - 16 * hf) * SCR_LD + j * 32 + (lane & 31)] = acc[i][j][8 * hf + r];
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave re-reads its own writes
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int row = prow + RPP * ps;
        const int64_t m = mb + row;
        if (!ncol || m >= g.M) continue;
        const int64_t o = m * g.ldc + n;
        float4 v[Q], d[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          v[q] = *reinterpret_cast<const float4*>(scr + row * SCR_LD + c0 + 4 * q);
          v[q].x += bias[q].x; v[q].y += bias[q].y; v[q].z += bias[q].z; v[q].w += bias[q].w;
          const float4 ax = aux[ps][q];
          if (EPI == EPI_STORE) {
            v[q].x += ax.x; v[q].y += ax.y; v[q].z += ax.z; v[q].w += ax.w;
          } else if (EPI == EPI_GELU) {
            if (g.aux_grad) {  // C2 <- gelu'(pre): both values from one erf / exp
              v[q].x = xf_gelu_both(v[q].x, d[q].x); v[q].y = xf_gelu_both(v[q].y, d[q].y);
              v[q].z = xf_gelu_both(v[q].z, d[q].z); v[q].w = xf_gelu_both(v[q].w, d[q].w);
            } else {
              d[q] = v[q];
              v[q].x = xf_gelu(v[q].x); v[q].y = xf_gelu(v[q].y); v[q].z = xf_gelu(v[q].z); v[q].w = xf_gelu(v[q].w);
            }
          } else if (EPI == EPI_GELU_INFER) {
            v[q].x = xf_gelu(v[q].x); v[q].y = xf_gelu(v[q].y); v[q].z = xf_gelu(v[q].z); v[q].w = xf_gelu(v[q].w);
          } else if (EPI == EPI_DROP_RES) {
            if (g.drop.on) {
              xf_drop4(g.drop, (uint32_t)m, (uint32_t)(n + 4 * q), v[q]);
            }
            v[q].x += ax.x; v[q].y += ax.y; v[q].z += ax.z; v[q].w += ax.w;
          } else if (EPI == EPI_GELU_GRAD) {
            if (g.aux_grad) {
              v[q].x *= ax.x; v[q].y *= ax.y; v[q].z *= ax.z; v[q].w *= ax.w;
            } else {
              v[q].x *= xf_gelu_grad(ax.x); v[q].y *= xf_gelu_grad(ax.y);
              v[q].z *= xf_gelu_grad(ax.z); v[q].w *= xf_gelu_grad(ax.w);
            }
          }
        }
        if (EPI == EPI_GELU) st_out(g.C2, o, d);
        st_out(g.C, zoff + o, v);
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();  // the next half strip overwrites the scratch
    }
  }
}
// Tile and slice depth per call: gemm_plan. These GEMMs are skinny (K <= 1024): bound by the CU's memory-instruction
// throughput and by how many workgroups are co-resident, not by the matrix core. Many small workgroups
// win -- 64 x 64 tiles with 64-deep slices for the forward / dX GEMMs (64 x 128 once N >= 256): measured 1.874 vs 1.888 ms/step
// against 32-deep (whole-K 128-deep slices: 2.026); 128-deep slices only pay for the split-K dW GEMMs, on 128 x 64 tiles:
// twice the workgroups of 128 x 128 at half the LDS and registers each -- the split-K GEMMs are a latency chain of a dozen K
// slices per workgroup and want co-resident workgroups (measured +1.4 ... 2 % of the step at batch 512 / 128 against
// 128 x 128; 64 x 64 no better).
template <class P, int BM, int BN, int BK, bool TA, bool TB, int EPI, uint32_t S>
__global__ __launch_bounds__(256, (epi_res_ln(EPI) || EPI == EPI_DX_LNBWD) ? XF_LN_EPI_MIN_WAVES : 1) void gemm_kernel(const GemmArgs g_in) {
  gemm_body<P, BM, BN, BK, TA, TB, EPI, S>(g_in, (int)blockIdx.x);
}
// Up to four GEMMs of one tile configuration in one launch: workgroups [start[i], start[i + 1]) are GEMM i's. The
// weight-gradient GEMMs of a layer -- FFN2, FFN1, out-proj, QKV -- go out together once the layer's last operand (dQKV)
// exists: at small batches every launch costs its ramp and its tail -- 16 launches of 7.8 us at batch 32 (round 3).
struct GemmGroup { GemmArgs g[4]; int start[5]; };
template <class P, int BM, int BN, int BK, bool TA, bool TB, int EPI, uint32_t S>
__global__ __launch_bounds__(256, 1) void gemm_group_kernel(const GemmGroup p) {
  const int b = (int)blockIdx.x;
  const int i = (b >= p.start[1]) + (b >= p.start[2]) + (b >= p.start[3]);  // (unused entries start at the grid's end)
  gemm_body<P, BM, BN, BK, TA, TB, EPI, S>(p.g[i], b - p.start[i]);
}

struct FfnFwdArgs {
  const __bf16* X;    // [M][128]
  const __bf16* W1;   // [I][128]
  const float* b1;    // [I]
  const __bf16* W2;   // [128][I]
  __bf16* U;          // [M][I] pre-activation out: the FFN2 dX epilogue evaluates gelu'(u) (null: not stored -- inference)
  __bf16* G;          // [M][I] gelu(u) out: the dW2 operand (null: not stored)
  int I;
  GemmArgs e;         // the LayerNorm epilogue's arguments: M, N = 128, ldc = 128, bias = b2, R, C, drop, ln_*, Y, Y16
  unsigned long long* stamps;  // probe build only
};

// One weight chunk of the fused FFN forward in flight in registers: W1 rows [c CH, +CH) x 128 (image [CH][136]) or
// W2 columns [c CH, +CH) of all 128 rows (image [128][CH + 8]); 16-byte pieces, CH / 16 per thread.
template <int N, class F>
__device__ __forceinline__ void xf_static_for(F&& fn) {  // fn(integral_constant<int, 0>) ... fn(<N - 1>): indices are
  if constexpr (N > 0) {                                  // constants at the source level (register arrays stay in registers)
    xf_static_for<N - 1>(fn);
    fn(std::integral_constant<int, N - 1>{});
  }
}
template <int CH>
struct WeightChunk {
  static constexpr int NW = CH / 16, PC = CH / 8, H = 128, LDH = H + 8, LDC = CH + 8;
  bf16x8 reg[NW];  // (a native vector type: HIP's uint4 / float4 structs are copied with memcpy between address
                   //  spaces, which kept this array in scratch memory)
  __device__ __forceinline__ void load_w1(const __bf16* W1, int c, int tid) {
    xf_static_for<NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int p = tid + i * 256, row = p >> 4, ch = p & 15;
      reg[i] = *reinterpret_cast<const bf16x8*>(W1 + (int64_t)(c * CH + row) * H + ch * 8);
    });
  }
  __device__ __forceinline__ void commit_w1(__bf16* sW, int tid) const {
    xf_static_for<NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int p = tid + i * 256, row = p >> 4, ch = p & 15;
      *reinterpret_cast<bf16x8*>(sW + row * LDH + ch * 8) = reg[i];
    });
  }
  __device__ __forceinline__ void load_w2(const __bf16* W2, int I, int c, int tid) {
    xf_static_for<NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int p = tid + i * 256, row = p / PC, ch = p % PC;
      reg[i] = *reinterpret_cast<const bf16x8*>(W2 + (int64_t)row * I + c * CH + ch * 8);
    });
  }
  __device__ __forceinline__ void commit_w2(__bf16* sW, int tid) const {
    xf_static_for<NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int p = tid + i * 256, row = p / PC, ch = p % PC;
      *reinterpret_cast<bf16x8*>(sW + row * LDC + ch * 8) = reg[i];
    });
  }
};

// CH: columns of I per chunk: 128 (two workgroups' worth of registers) or 64. RE: the residual (this layer's LayerNorm 1
// output) is re-derived from pre1 / mean1 / rstd1 in the epilogue (EPI_DROP_RES_LN_RE) instead of loaded. KEEP = false (the
// forward-only form, ffn_fwd_infer_kernel): U, G, pre, mean and rstd are not stored -- the row-major pass over sG only turns
// u into gelu(u) in place.
template <int CH, bool RE, bool KEEP>
__device__ __forceinline__ void ffn_fwd_fused_body(const FfnFwdArgs& f_in) {
  FfnFwdArgs f = f_in;  // (device-side step counter -> dropout key: xf_drop_resolve)
  XF_CHAIN_PRIO();
  f.e.drop = xf_drop_resolve(f.e.drop);
  constexpr int H = 128, LDH = H + 8, LDC = CH + 8, BM = 64;
  constexpr int NJ = CH / 64;           // 32-column blocks of the u chunk per wave (2 x 2 waves over 64 x CH)
  constexpr int W_ELEMS = CH * LDH > H * LDC ? CH * LDH : H * LDC;
  __shared__ __attribute__((aligned(16))) __bf16 sG[BM * LDC];
  __shared__ __attribute__((aligned(16))) __bf16 sW[W_ELEMS];
  __shared__ float sB1[1024];  // b1: a global load inside the chunk loop would be a vmcnt(0) drain per chunk
  static_assert(W_ELEMS >= BM * LDH, "the x tile is staged through sW");
  static_assert(W_ELEMS * 2 >= 4 * 16 * 68 * 4 + 128 * 4, "the LayerNorm epilogue's scratch aliases sW");
  using FR = Frag<PrecBF16, false>;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, tid = threadIdx.x;
  const int wr = wid >> 1, wc = wid & 1;
  const TileIdx tix = tile_of(1, f.e.nt_m, 1);
  if (!tix.valid) return;
  const int64_t m0 = xf_tile_rows(f.e, tix.m, BM);
  const int64_t M = f.e.M;
  const int I = f.I, nchunk = I / CH;
#ifdef XF_FFN_STAMP
  const bool stamp_on = f.stamps && threadIdx.x == 0;
  unsigned long long* st_buf = f.stamps + (int64_t)blockIdx.x * 64;
#endif
  XF_STAMP(0);

  // two weight chunks in flight, each for a whole chunk period: W1(c + 1) from the first GEMM of chunk c on, W2(c + 1)
  // from its second GEMM on (with ONE set, issued a GEMM ahead, the L2 round trip was exposed twice per chunk)
  WeightChunk<CH> wa, wb;
  constexpr int PC = CH / 8;  // 16-byte pieces per row of a [rows][CH] image

  // x tile -> sW (as a [64][136] image) -> this wave's A fragments of all 8 k-steps
  {
    uint4 xr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = tid + i * 256, row = p >> 4, ch = p & 15;
      xr[i] = make_uint4(0u, 0u, 0u, 0u);
      if (m0 + row < M) xr[i] = *reinterpret_cast<const uint4*>(f.X + (m0 + row) * H + ch * 8);
    }
    wa.load_w1(f.W1, 0, tid);
    wb.load_w2(f.W2, I, 0, tid);
    for (int i = tid; i < I; i += 256) sB1[i] = f.b1[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = tid + i * 256, row = p >> 4, ch = p & 15;
      *reinterpret_cast<uint4*>(sW + row * LDH + ch * 8) = xr[i];
    }
  }
  __syncthreads();
  bf16x8 xa[H / 16];
#pragma unroll
  for (int ks = 0; ks < H / 16; ++ks) xa[ks] = FR::get(sW, LDH, wr * 32, ks * 16);
  XF_STAMP(1);

  f32x16 accy[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) accy[j][r] = 0.f;

  for (int c = 0; c < nchunk; ++c) {
    XF_LOOP_BARRIER();  // the previous chunk's second GEMM (or the fragment reads above) is done with sW and sG
    if (c < 2) XF_STAMP(2 + 6 * c);
    wa.commit_w1(sW, tid);  // W1 chunk c
    XF_LOOP_BARRIER();
    if (c < 2) XF_STAMP(3 + 6 * c);
    if (c + 1 < nchunk) wa.load_w1(f.W1, c + 1, tid);
    f32x16 accu[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) accu[j][r] = 0.f;
    {  // the B fragments of the next k-step are read while this one's MFMAs run
      bf16x8 fb[2][NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[0][j] = FR::get(sW, LDH, wc * (CH / 2) + j * 32, 0);
#pragma unroll
      for (int ks = 0; ks < H / 16; ++ks) {
        if (ks + 1 < H / 16) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) fb[(ks + 1) & 1][j] = FR::get(sW, LDH, wc * (CH / 2) + j * 32, (ks + 1) * 16);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) accu[j] = xf_mma(xa[ks], fb[ks & 1][j], accu[j]);
      }
    }
    // u = acc + b1 -> bf16 -> sG (accumulator layout: element r of lane l = row (r&3) + 8 (r>>2) + 4 (l>>5), col l&31)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wc * (CH / 2) + j * 32 + (lane & 31);
      const float b = sB1[c * CH + col];
#pragma unroll
      for (int r = 0; r < 16; ++r) sG[(wr * 32 + xf_acc_row(r, lane)) * LDC + col] = (__bf16)(accu[j][r] + b);
    }
    if (c < 2) XF_STAMP(4 + 6 * c);
    XF_LOOP_BARRIER();  // sG holds u; every wave is done with the W1 chunk
    if (c < 2) XF_STAMP(5 + 6 * c);
    // row-major pass over sG in 16-byte pieces: u and g = gelu(u) -> HBM, g back in place (the second GEMM's A operand)
#pragma unroll
    for (int i = 0; i < BM * PC / 256; ++i) {
      const int p = tid + i * 256, row = p / PC, ch = p % PC;
      float4* cell = reinterpret_cast<float4*>(sG + row * LDC + ch * 8);
      const float4 u8 = *cell;
      const float4 g8 = xf_gelu_bf16x8(u8);
      if constexpr (KEEP) {
        if (m0 + row < M) {
          if (f.U) *reinterpret_cast<float4*>(f.U + (m0 + row) * I + c * CH + ch * 8) = u8;
          if (f.G) *reinterpret_cast<float4*>(f.G + (m0 + row) * I + c * CH + ch * 8) = g8;
        }
      }
      *cell = g8;
    }
    wb.commit_w2(sW, tid);  // W2 chunk c
    if (c < 2) XF_STAMP(6 + 6 * c);
    XF_LOOP_BARRIER();
    if (c < 2) XF_STAMP(7 + 6 * c);
    if (c + 1 < nchunk) wb.load_w2(f.W2, I, c + 1, tid);
#pragma unroll
    for (int ks = 0; ks < CH / 16; ++ks) {
      const bf16x8 fa = FR::get(sG, LDC, wr * 32, ks * 16);
      bf16x8 fb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = FR::get(sW, LDC, wc * 64 + j * 32, ks * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j) accy[j] = xf_mma(fa, fb[j], accy[j]);
    }
  }
  XF_STAMP(14);
  __syncthreads();  // everyone is done with sW: the epilogue's scratch aliases it
  XF_STAMP(15);
  epi_drop_res_ln_64x128<RE ? 1 : 0, KEEP>(accy, reinterpret_cast<unsigned char*>(sW), f.e, m0, wid, lane);
  XF_STAMP(16);
}
template <int CH, bool RE = false>
__global__ __launch_bounds__(256, CH == 128 ? XF_FFN_MIN_WAVES : 3) void ffn_fwd_fused_kernel(const FfnFwdArgs f_in) {
  ffn_fwd_fused_body<CH, RE, true>(f_in);
}
template <int CH>
__global__ __launch_bounds__(256, CH == 128 ? XF_FFN_MIN_WAVES : 3) void ffn_fwd_infer_kernel(const FfnFwdArgs f_in) {
  ffn_fwd_fused_body<CH, false, false>(f_in);
}

// ---- fused FFN backward, dX chain (bf16 storage, H = 128) ----------------------------------------------------------------
//   dI = (dy W2) * gelu'(u)  ->  dx = dI W1 (+ residual gradient)  ->  LayerNorm 1 backward
// in ONE kernel, the mirror of ffn_fwd_fused_kernel: a workgroup owns 64 token rows and walks I in 64-column chunks; the
// second GEMM reads the dI chunk from LDS. dI is still WRITTEN once (bf16): it is the dW1 GEMM's operand. Same MFMA
// order as the two launches it replaces (the FFN2 dX GEMM with the gelu' epilogue, the FFN1 dX GEMM with the LayerNorm
// backward epilogue): bit-identical dI, dx, d_lin and partial records. Per layer at T = 102 400, I = 512: 418 MB instead of
// 523 MB.
// Two forms of the weight staging (template parameter RING, picked per launch: xf_ffn_bwd_dx_fused_ex). Per tile both run
// the same MFMAs on the same operands in the same order and the same epilogue: every output is bit-identical.
//   RING = false, the register-staged form (XFMR_FFN_REG_STAGE=1): a W2 / W1 chunk travels global -> registers ->
//   ds_write into a padded image, one image buffer for both.
//   LDS: sF [64][68] fp32 (dy W2 chunk: accumulator layout -> row-major) + sG [64][72] (the dI chunk: A operand of the
//   second GEMM; the u chunk never goes through LDS: a thread multiplies the piece it loaded) + sW 24 KB (the W2 chunk as
//   a [128 k][64 + 32] image, then the W1 chunk as [64 k][128 + 32]: both are B operands stored k-major, read through
//   ds_read_b64_tr_b16; the dy tile before the first chunk, the epilogue's scratch after the last) = 51 KB.
//   RING = true (the default): the chunks come by global_load_lds_dwordx4 (dw_ring.hip's helpers) into UNPADDED images
//   swizzled on the source address (SwzImg<64> for the [128 k][64] W2 chunk, SwzImg<128> for the [64 k][128] W1 chunk), each
//   one chunk ahead of its use: W2 (c + 1) is issued behind the barrier that ends chunk c's row-major pass and lands in
//   sF's bytes (dead from that pass to the next dG store) while GEMM 2 of chunk c runs; W1 (c) is issued at the top of
//   chunk c into its own 16 KB and lands during GEMM 1 and the gelu' arithmetic. No weight ever sits in a VGPR.
//   LDS: one array, sF 17 KB (= the W2 image + 1 KB) + sG 9 KB + the W1 image 16 KB = 42 KB; the dy tile is staged over
//   sG and the head of the W1 image, the epilogue's scratch over sF and sG.
//   Waits: the DMA is asm-issued, outside hipcc's s_waitcnt bookkeeping, and the chunk loop's barriers do not wait on
//   vmcnt. Every wait for an image is s_waitcnt vmcnt(0) at a point where nothing else of this wave that matters is in
//   flight (in front of the dI stores; at the top of the chunk, where the u chunk is needed too), followed by a barrier
//   before anyone reads the image.
struct FfnBwdArgs {
  const __bf16* DY;   // [M][128] gradient of the FFN2 Linear's output
  const __bf16* W2;   // [128][I]
  const __bf16* U;    // [M][I] pre-activation saved by the fused forward
  const __bf16* W1;   // [I][128]
  __bf16* DI;         // [M][I] out: gradient of the FFN1 Linear's output
  int I;
  GemmArgs e;         // epi_dx_lnbwd_64x128's arguments
};

template <bool RING>
__global__ __launch_bounds__(256, 3) void ffn_bwd_dx_fused_kernel(const FfnBwdArgs f_in) {
  FfnBwdArgs f = f_in;  // (device-side step counter -> dropout key: xf_drop_resolve)
  XF_CHAIN_PRIO();
  f.e.drop = xf_drop_resolve(f.e.drop); f.e.drop2 = xf_drop_resolve(f.e.drop2);
  constexpr int H = 128, BM = 64, CH = 64, LDH = H + 8, LDC = CH + 8;
  constexpr int LDF = CH + 4;
  constexpr int EPI_BYTES = (4 * 16 * 68 + 2 * 2 * 2 * 16 * 2 + 2 * 3 * 128) * 4;  // epi_dx_lnbwd_64x128's scratch
  using FN = Frag<PrecBF16, false>;
  using FT = Frag<PrecBF16, true>;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, tid = threadIdx.x;
  const int wr = wid >> 1, wc = wid & 1;
  const TileIdx tix = tile_of(1, f.e.nt_m, 1);
  if (!tix.valid) return;
  const int64_t m0 = xf_tile_rows(f.e, tix.m, BM);
  const int64_t M = f.e.M;
  const int I = f.I, nchunk = I / CH;

  bf16x8 ur[2];  // u chunk in flight (native vectors: see WeightChunk)
  auto load_u = [&](int c) {  // u[m0 + row][c CH + ..]: 64 rows of 8 pieces
    xf_static_for<2>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const int p = tid + i * 256, row = p >> 3, ch = p & 7;
      bf16x8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.f;
      if (m0 + row < M) z = *reinterpret_cast<const bf16x8*>(f.U + (m0 + row) * I + c * CH + ch * 8);
      ur[i] = z;
    });
  };
  // piece i of the row-major pass, 8 columns: dI = dG * gelu'(u) with u straight from the registers it was loaded into
  auto di_piece = [&](const float* sF, const int i) {
    const int p = tid + i * 256, row = p >> 3, ch = p & 7;
    const float4 g0 = *reinterpret_cast<const float4*>(sF + row * LDF + ch * 8);
    const float4 g1 = *reinterpret_cast<const float4*>(sF + row * LDF + ch * 8 + 4);
    const bf16x8 u8 = ur[i];
    bf16x8 d8;
    d8[0] = (__bf16)(g0.x * xf_gelu_grad((float)u8[0])); d8[1] = (__bf16)(g0.y * xf_gelu_grad((float)u8[1]));
    d8[2] = (__bf16)(g0.z * xf_gelu_grad((float)u8[2])); d8[3] = (__bf16)(g0.w * xf_gelu_grad((float)u8[3]));
    d8[4] = (__bf16)(g1.x * xf_gelu_grad((float)u8[4])); d8[5] = (__bf16)(g1.y * xf_gelu_grad((float)u8[5]));
    d8[6] = (__bf16)(g1.z * xf_gelu_grad((float)u8[6])); d8[7] = (__bf16)(g1.w * xf_gelu_grad((float)u8[7]));
    return d8;
  };
  // dG (fp32, accumulator layout: element r of lane l = row (r&3) + 8 (r>>2) + 4 (l>>5), col l&31) -> sF
  auto store_dg = [&](float* sF, const f32x16& accg) {
    const int col = wc * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) sF[(wr * 32 + xf_acc_row(r, lane)) * LDF + col] = accg[r];
  };

  f32x16 accx[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) accx[j][r] = 0.f;

  if constexpr (RING) {
    constexpr int F_BYTES = BM * LDF * 4, G_BYTES = BM * LDC * 2, W2_BYTES = H * CH * 2, W1_BYTES = CH * H * 2;
    // ONE shared array (a second __shared__ object next to an LDS-DMA target makes hipcc serialise on vmcnt(0))
    __shared__ __attribute__((aligned(16))) unsigned char smem[F_BYTES + G_BYTES + W1_BYTES];
    static_assert(W2_BYTES <= F_BYTES, "the W2 chunk image lands in sF's bytes");
    static_assert(BM * LDH * 2 <= G_BYTES + W1_BYTES, "the dy tile is staged over sG and the W1 image");
    static_assert(EPI_BYTES <= F_BYTES + G_BYTES, "the epilogue's scratch aliases sF and sG");
    static_assert(F_BYTES % 1024 == 0 && G_BYTES % 1024 == 0, "DMA targets on 1-KiB instruction boundaries");
    float* const sF = reinterpret_cast<float*>(smem);
    __bf16* const sW2 = reinterpret_cast<__bf16*>(smem);
    __bf16* const sG = reinterpret_cast<__bf16*>(smem + F_BYTES);
    __bf16* const sW1 = reinterpret_cast<__bf16*>(smem + F_BYTES + G_BYTES);
    __bf16* const sY = sG;
    using I2 = SwzImg<CH>;  // W2 chunk image [128 k][64]: 8 rows per 1-KiB instruction
    using I1 = SwzImg<H>;   // W1 chunk image [64 k][128]: 4 rows per instruction
    const int w = __builtin_amdgcn_readfirstlane(wid);
    // four instructions per wave and image: wave w fetches image rows [32 w, +32) of W2[k][c CH + ..] ...
    auto issue_w2 = [&](int c) {
      xf_static_for<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const int row0 = 32 * w + I2::kRowsPerInstr * j, k = I2::gather_row(row0);
        xf_glds16_raw_so(f.W2, (uint32_t)(k * I + c * CH + 8 * I2::gather_src_chunk(k)) * 2u, sW2 + row0 * CH);
      });
    };
    // ... and rows [16 w, +16) of W1[c CH + k][..]
    auto issue_w1 = [&](int c) {
      xf_static_for<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const int row0 = 16 * w + I1::kRowsPerInstr * j, k = I1::gather_row(row0);
        xf_glds16_raw_so(f.W1, (uint32_t)((c * CH + k) * H + 8 * I1::gather_src_chunk(k)) * 2u, sW1 + row0 * H);
      });
    };

    // dy tile -> sY (a [64][136] image) -> this wave's A fragments of all 8 k-steps; the first W2 chunk is on its way
    issue_w2(0);
    {
      uint4 yr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + i * 256, row = p >> 4, ch = p & 15;
        yr[i] = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + row < M) yr[i] = *reinterpret_cast<const uint4*>(f.DY + (m0 + row) * H + ch * 8);
      }
      load_u(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + i * 256, row = p >> 4, ch = p & 15;
        *reinterpret_cast<uint4*>(sY + row * LDH + ch * 8) = yr[i];
      }
    }
    XF_LOOP_BARRIER();
    bf16x8 ya[H / 16];
#pragma unroll
    for (int ks = 0; ks < H / 16; ++ks) ya[ks] = FN::get(sY, LDH, wr * 32, ks * 16);

    for (int c = 0; c < nchunk; ++c) {
      xf_wait_vm<0>();    // this wave's pieces of W2 chunk c (and its u chunk) have landed
      XF_LOOP_BARRIER();  // ... everyone's; the previous chunk's second GEMM (or the fragment reads above) is done with sW1 and sG
      issue_w1(c);
      f32x16 accg;
#pragma unroll
      for (int r = 0; r < 16; ++r) accg[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < H / 16; ++ks) accg = xf_mma(ya[ks], I2::frag_tr(sW2, wc * 32, ks * 16), accg);
      XF_LOOP_BARRIER();  // every wave is done with the W2 image: sF takes its bytes
      store_dg(sF, accg);
      XF_LOOP_BARRIER();  // sF holds dG
      // row-major pass -> sG, the second GEMM's A operand, and -> HBM (16-byte pieces: a wave instruction = 8 rows x 128 B)
      bf16x8 d8[2];
      xf_static_for<2>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, row = p >> 3, ch = p & 7;
        d8[i] = di_piece(sF, i);
        *reinterpret_cast<bf16x8*>(sG + row * LDC + ch * 8) = d8[i];
      });
      xf_wait_vm<0>();  // this wave's pieces of W1 chunk c (issued a GEMM and the gelu' arithmetic ago); the stores go after it
      xf_static_for<2>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, row = p >> 3, ch = p & 7;
        if (m0 + row < M) *reinterpret_cast<bf16x8*>(f.DI + (m0 + row) * I + c * CH + ch * 8) = d8[i];
      });
      XF_LOOP_BARRIER();  // sG holds dI, the W1 image is whole, everyone is done with sF
      if (c + 1 < nchunk) { issue_w2(c + 1); load_u(c + 1); }
#pragma unroll
      for (int ks = 0; ks < CH / 16; ++ks) {
        const bf16x8 fa = FN::get(sG, LDC, wr * 32, ks * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[j] = xf_mma(fa, I1::frag_tr(sW1, wc * 64 + j * 32, ks * 16), accx[j]);
      }
    }
    __syncthreads();  // everyone is done with the images: the epilogue's scratch aliases them
    epi_dx_lnbwd_64x128(accx, smem, f.e, m0, tix.m, wid, lane);
  } else {
    constexpr int LD1 = CH + 32;  // W2 chunk image [128 k][CH rows]
    constexpr int LD2 = H + 32;   // W1 chunk image [CH k][128 rows]
    constexpr int W_ELEMS = H * LD1 > CH * LD2 ? H * LD1 : CH * LD2;
    __shared__ __attribute__((aligned(16))) float sF[BM * LDF];  // dG = dy W2 chunk, fp32, accumulator layout -> row-major
    __shared__ __attribute__((aligned(16))) __bf16 sG[BM * LDC];
    __shared__ __attribute__((aligned(16))) __bf16 sW[W_ELEMS];
    static_assert(W_ELEMS >= BM * LDH, "the dy tile is staged through sW");
    static_assert(W_ELEMS * 2 >= EPI_BYTES, "the epilogue's scratch aliases sW");
    bf16x8 wa[4], wb[4];  // W2 chunk, W1 chunk in flight
    auto load_w2 = [&](int c) {  // W2[k][c CH + j]: 128 rows of 8 pieces
      xf_static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, k = p >> 3, ch = p & 7;
        wa[i] = *reinterpret_cast<const bf16x8*>(f.W2 + (int64_t)k * I + c * CH + ch * 8);
      });
    };
    auto commit_w2 = [&]() {
      xf_static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, k = p >> 3, ch = p & 7;
        *reinterpret_cast<bf16x8*>(sW + k * LD1 + ch * 8) = wa[i];
      });
    };
    auto load_w1 = [&](int c) {  // W1[c CH + k][n]: 64 rows of 16 pieces
      xf_static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, k = p >> 4, ch = p & 15;
        wb[i] = *reinterpret_cast<const bf16x8*>(f.W1 + (int64_t)(c * CH + k) * H + ch * 8);
      });
    };
    auto commit_w1 = [&]() {
      xf_static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, k = p >> 4, ch = p & 15;
        *reinterpret_cast<bf16x8*>(sW + k * LD2 + ch * 8) = wb[i];
      });
    };

    // dy tile -> sW (as a [64][136] image) -> this wave's A fragments of all 8 k-steps
    {
      uint4 yr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + i * 256, row = p >> 4, ch = p & 15;
        yr[i] = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + row < M) yr[i] = *reinterpret_cast<const uint4*>(f.DY + (m0 + row) * H + ch * 8);
      }
      load_w2(0);
      load_u(0);
      load_w1(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + i * 256, row = p >> 4, ch = p & 15;
        *reinterpret_cast<uint4*>(sW + row * LDH + ch * 8) = yr[i];
      }
    }
    __syncthreads();
    bf16x8 ya[H / 16];
#pragma unroll
    for (int ks = 0; ks < H / 16; ++ks) ya[ks] = FN::get(sW, LDH, wr * 32, ks * 16);

    for (int c = 0; c < nchunk; ++c) {
      XF_LOOP_BARRIER();  // the previous chunk's second GEMM (or the fragment reads above) is done with sW and sG
      commit_w2();
      XF_LOOP_BARRIER();
      if (c + 1 < nchunk) load_w2(c + 1);
      f32x16 accg;
#pragma unroll
      for (int r = 0; r < 16; ++r) accg[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < H / 16; ++ks) accg = xf_mma(ya[ks], FT::get(sW, LD1, wc * 32, ks * 16), accg);
      store_dg(sF, accg);
      XF_LOOP_BARRIER();  // sF holds dG; every wave is done with the W2 chunk
      // row-major pass -> HBM (16-byte pieces: a wave instruction = 8 rows x 128 B) and -> sG, the second GEMM's A operand
      xf_static_for<2>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int p = tid + i * 256, row = p >> 3, ch = p & 7;
        const bf16x8 d8 = di_piece(sF, i);
        if (m0 + row < M) *reinterpret_cast<bf16x8*>(f.DI + (m0 + row) * I + c * CH + ch * 8) = d8;
        *reinterpret_cast<bf16x8*>(sG + row * LDC + ch * 8) = d8;
      });
      commit_w1();
      XF_LOOP_BARRIER();
      if (c + 1 < nchunk) { load_w1(c + 1); load_u(c + 1); }
#pragma unroll
      for (int ks = 0; ks < CH / 16; ++ks) {
        const bf16x8 fa = FN::get(sG, LDC, wr * 32, ks * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) accx[j] = xf_mma(fa, FT::get(sW, LD2, wc * 64 + j * 32, ks * 16), accx[j]);
      }
    }
    __syncthreads();  // everyone is done with sW: the epilogue's scratch aliases it
    epi_dx_lnbwd_64x128(accx, reinterpret_cast<unsigned char*>(sW), f.e, m0, tix.m, wid, lane);
  }
}

// Deterministic column sums of a [rows, cols] fp32 matrix: block (x, y) sums rows [y*rows_per, (y+1)*rows_per)
// of 64 columns with 4 row groups in flight (each wave instruction reads 256 contiguous bytes), combines the
// groups through LDS in a fixed order and writes dst[y*cols + col]. Used for bias gradients (two levels) and
// for the split-K slab reduction (rows = slabs, cols = elements of the weight).
template <class T>
__global__ __launch_bounds__(256) void rowsum_kernel(float* dst, const T* src, int64_t rows, int64_t cols,
                                                     int64_t rows_per) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + c;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < rows) ? r0 + rows_per : rows;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < cols) {
    int64_t r = r0 + rg;
    for (; r + 12 < r1; r += 16) {
      s0 += (float)src[r * cols + col];
      s1 += (float)src[(r + 4) * cols + col];
      s2 += (float)src[(r + 8) * cols + col];
      s3 += (float)src[(r + 12) * cols + col];
    }
    for (; r < r1; r += 4) s0 += (float)src[r * cols + col];
  }
  red[rg][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rg == 0 && col < cols) dst[(int64_t)blockIdx.y * cols + col] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

template <class T>
int launch_rowsum(float* dst, const T* src, int64_t rows, int64_t cols, int64_t rows_per, hipStream_t st) {
  const int64_t ny = (rows + rows_per - 1) / rows_per;
  hipLaunchKernelGGL((rowsum_kernel<T>), dim3((unsigned)((cols + 63) / 64), (unsigned)ny), dim3(256), 0, st, dst, src,
                     rows, cols, rows_per);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

// Several row reductions in one launch: a one-dimensional grid of exactly the 64-column blocks the segments have
// (first[i] = index of segment i's first block; a (max blocks, segments) grid launched 57 k workgroups for 12 k that had
// work). A block is 16 row groups x 16 lanes of 4 columns: 16-byte loads, 16 of
// them in flight per thread = 256 rows per round trip. The LayerNorm partial records of the fused dX GEMMs are 1600
// rows of 128 columns (T / 64 workgroups): with 4 row groups of 64 one-column lanes such a segment was a 25-iteration
// latency chain on two workgroups and set the kernel's time (88 us for 247 MB; 4-byte loads: 967 k wave instructions).
// Fixed summation order: bit-reproducible. Segments whose base / ld / cols are not multiples of 4 floats take the
// one-column form.
struct MultiSegs { XfReduceSeg s[64]; int first[65]; int n; };
__global__ __launch_bounds__(256) void multi_rowsum_kernel(MultiSegs m) {
  __shared__ __attribute__((aligned(16))) float red[16][64];
  int si = 0;
#pragma unroll
  for (int step = 32; step > 0; step >>= 1)  // the last segment whose first block is <= blockIdx.x
    if (si + step < m.n && m.first[si + step] <= (int)blockIdx.x) si += step;
  const XfReduceSeg sg = m.s[si];
  const int bx = (int)blockIdx.x - m.first[si];
  const bool vec = !((sg.cols | sg.ld) & 3) && !(reinterpret_cast<uintptr_t>(sg.src) & 15);
  if (sg.pad) {
    // Short and wide (xf_multi_rowsum marks them: <= 64 rows, >= 256 columns, 16-byte pieces): 256 columns per block, 4 row
    // groups of 64 lanes x 4 columns, every row of the segment in flight at once. The split-K slabs of a small batch are
    // 15-50 rows: in the 64-column form a block moved 4-13 KB and the launch was bound by its 70 k blocks (config 4: 140 us
    // for 360 MB).
    const int cq = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int col = bx * 256 + 4 * cq;
    float4 s[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) s[u] = make_float4(0, 0, 0, 0);
    if (col < sg.cols) {
      const float* src = sg.src + col;
      const int64_t ld = sg.ld;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int r = rg + 4 * u;
        if (r < sg.rows) s[u] = *reinterpret_cast<const float4*>(src + r * ld);
      }
    }
    auto add4 = [](const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
    const float4 t = add4(add4(add4(add4(s[0], s[1]), add4(s[2], s[3])), add4(add4(s[4], s[5]), add4(s[6], s[7]))),
                          add4(add4(add4(s[8], s[9]), add4(s[10], s[11])), add4(add4(s[12], s[13]), add4(s[14], s[15]))));
    float4* red4 = reinterpret_cast<float4*>(&red[0][0]);  // [4 row groups][64 lanes]
    red4[rg * 64 + cq] = t;
    __syncthreads();
    if (rg == 0 && col < sg.cols)
      *reinterpret_cast<float4*>(sg.dst + col) = add4(add4(red4[cq], red4[64 + cq]), add4(red4[128 + cq], red4[192 + cq]));
    return;
  }
  if (vec) {
    const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int col = bx * 64 + 4 * cq;
    float4 s[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) s[u] = make_float4(0, 0, 0, 0);
    if (col < sg.cols) {
      const float* src = sg.src + col;
      const int64_t ld = sg.ld;
      int r = rg;
      for (; r + 240 < sg.rows; r += 256) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const float4 v = *reinterpret_cast<const float4*>(src + (r + 16 * u) * ld);
          s[u].x += v.x; s[u].y += v.y; s[u].z += v.z; s[u].w += v.w;
        }
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {  // the last, partial round: still all loads issued together
        if (r + 16 * u < sg.rows) {
          const float4 v = *reinterpret_cast<const float4*>(src + (r + 16 * u) * ld);
          s[u].x += v.x; s[u].y += v.y; s[u].z += v.z; s[u].w += v.w;
        }
      }
    }
    auto add4 = [](const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
    const float4 t = add4(add4(add4(add4(s[0], s[1]), add4(s[2], s[3])), add4(add4(s[4], s[5]), add4(s[6], s[7]))),
                          add4(add4(add4(s[8], s[9]), add4(s[10], s[11])), add4(add4(s[12], s[13]), add4(s[14], s[15]))));
    *reinterpret_cast<float4*>(&red[rg][4 * cq]) = t;
    __syncthreads();
    if (threadIdx.x < 64) {
      const int c = threadIdx.x, oc = bx * 64 + c;
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) acc += red[g][c];
      if (oc < sg.cols) sg.dst[oc] = acc;
    }
    return;
  }
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = bx * 64 + c;
  float s[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) s[u] = 0.f;
  if (col < sg.cols) {
    const float* src = sg.src + col;
    const int64_t ld = sg.ld;
    int r = rg;
    for (; r + 60 < sg.rows; r += 64) {
#pragma unroll
      for (int u = 0; u < 16; ++u) s[u] += src[(r + 4 * u) * ld];
    }
    for (; r < sg.rows; r += 4) s[0] += src[r * ld];
  }
  red[rg][c] = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) +
               (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])));
  __syncthreads();
  if (rg == 0 && col < sg.cols) sg.dst[col] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// ================================================================================================================
// Host side: the switches, the plan of a call (gemm_plan), one launch routine per kernel family, the entry points
// ================================================================================================================
constexpr uint32_t SAB = XF_S16_A | XF_S16_B, SABC = SAB | XF_S16_C, SABCP = SABC | XF_S16_P;
// ---- the gemm_kernel instantiations: (operation, policy, storage mask, tile, slice depth) -> kernel. The lists bound the set:
// S16 names the masks an operation is ever launched with besides 0 (all fp32); a combination outside them has no kernel.
using GemmKernel = void (*)(const GemmArgs);
template <class P, bool TA, bool TB, int EPI, uint32_t S>
GemmKernel tile_kernel_of(int bm, int bn, int bk) {
  // the one slice depth beside 32: 128 for the bf16 split-K dW GEMMs, 64 for the other bf16 GEMMs, none for fp32
  constexpr int DEEP = P::kId != XFMR_PREC_BF16 ? 32 : EPI == EPI_SPLITK ? 128 : 64;
  const bool deep = bk == DEEP;
  if (bm == 64 && bn == 128) return deep ? gemm_kernel<P, 64, 128, DEEP, TA, TB, EPI, S> : gemm_kernel<P, 64, 128, 32, TA, TB, EPI, S>;
  if (bm == 128 && bn == 64) return deep ? gemm_kernel<P, 128, 64, DEEP, TA, TB, EPI, S> : gemm_kernel<P, 128, 64, 32, TA, TB, EPI, S>;
  if (bm == 64) return deep ? gemm_kernel<P, 64, 64, DEEP, TA, TB, EPI, S> : gemm_kernel<P, 64, 64, 32, TA, TB, EPI, S>;
  return deep ? gemm_kernel<P, 128, 128, DEEP, TA, TB, EPI, S> : gemm_kernel<P, 128, 128, 32, TA, TB, EPI, S>;
}
template <bool TA, bool TB, int EPI, uint32_t... S16>
GemmKernel tile_kernel_in(int precision, uint32_t s16, int bm, int bn, int bk) {
  if (precision == XFMR_PREC_F32) return s16 ? nullptr : tile_kernel_of<PrecF32, TA, TB, EPI, 0>(bm, bn, bk);
  if (precision != XFMR_PREC_BF16) return nullptr;
  if (s16 == 0) return tile_kernel_of<PrecBF16, TA, TB, EPI, 0>(bm, bn, bk);
  GemmKernel k = nullptr;
  (void)((s16 == S16 ? (k = tile_kernel_of<PrecBF16, TA, TB, EPI, S16>(bm, bn, bk), true) : false) || ...);
  return k;
}
GemmKernel tile_kernel(GemmOp op, int precision, uint32_t s16, int bm, int bn, int bk) {
  switch (op) {
    case kGemmFwdBias:
      return tile_kernel_in<false, false, EPI_STORE, XF_S16_C, (XF_S16_C | XF_S16_B), SABC>(precision, s16, bm, bn, bk);
    case kGemmFwdGelu:
      return tile_kernel_in<false, false, EPI_GELU, XF_S16_C, (XF_S16_C | XF_S16_B), SABC>(precision, s16, bm, bn, bk);
    case kGemmFwdDropRes: return tile_kernel_in<false, false, EPI_DROP_RES, XF_S16_A, SAB>(precision, s16, bm, bn, bk);
    case kGemmLnFwd: return tile_kernel_in<false, false, EPI_DROP_RES_LN, XF_S16_A, SAB>(precision, s16, bm, bn, bk);
    // (the re-derived forms exist for the storage the encoder runs them with: bf16 A and B operands -- the plan checks)
    case kGemmLnFwdRe: return tile_kernel_of<PrecBF16, false, false, EPI_DROP_RES_LN_RE, SAB>(bm, bn, bk);
    case kGemmLnFwdReDrop: return tile_kernel_of<PrecBF16, false, false, EPI_DROP_RES_LN_RED, SAB>(bm, bn, bk);
    case kGemmDx:
      return tile_kernel_in<false, true, EPI_STORE, XF_S16_A, (XF_S16_A | XF_S16_C), SAB, SABC>(precision, s16, bm, bn, bk);
    case kGemmDxGelu:
      return tile_kernel_in<false, true, EPI_GELU_GRAD, (XF_S16_A | XF_S16_C | XF_S16_P), SABCP>(precision, s16, bm, bn, bk);
    case kGemmDxLnBwd: return tile_kernel_in<false, true, EPI_DX_LNBWD, XF_S16_A, SAB>(precision, s16, bm, bn, bk);
    case kGemmDw: case kGemmDwDeferred: case kGemmDwGroup:
      return tile_kernel_in<true, true, EPI_SPLITK, XF_S16_A, SAB>(precision, s16, bm, bn, bk);
    default: return nullptr;
  }
}
// The forward-only instantiation that goes with a kGemmLnFwd plan (same tile, slice depth and grid; EPI_DROP_RES_LN_INFER):
// for the storage the encoder runs it with -- bf16 A and B operands on the whole-row tile. Null: no such kernel.
// ... and with a kGemmFwdGelu plan (EPI_GELU_INFER): all fp32, or every operand bf16 (the encoder's two storages)
GemmKernel gelu_infer_kernel(int precision, uint32_t s16, int bm, int bn, int bk) {
  return tile_kernel_in<false, false, EPI_GELU_INFER, SABC>(precision, s16, bm, bn, bk);
}
GemmKernel ln_infer_kernel(int precision, uint32_t s16, int bm, int bn, int bk) {
  if (precision != XFMR_PREC_BF16 || s16 != SAB || bm != 64 || bn != 128) return nullptr;
  return bk == 64 ? gemm_kernel<PrecBF16, 64, 128, 64, false, false, EPI_DROP_RES_LN_INFER, SAB>
                  : gemm_kernel<PrecBF16, 64, 128, 32, false, false, EPI_DROP_RES_LN_INFER, SAB>;
}

}  // namespace

#include "gemm_plan.inc"

namespace {

// What an entry returns before it launches, in the order of its checks: the key's early ones, its pointers' alignment, a
// check of its own that sits between (the residual operand, the workspace), the key's other ones
int plan_rc(const GemmPlan& p, bool aligned, int between = XFMR_OK) {
  return p.rc_shape ? p.rc_shape : !aligned ? XFMR_EALIGN : between ? between : p.rc;
}

void set_tiles(GemmArgs& g, const GemmPlan& p) {
  g.nt_n = p.nt_n; g.nt_m = p.nt_m; g.nt_z = p.nt_z; g.nt_full = p.nt_full; g.short_rows = p.short_rows;
}
// ---- the launch of gemm_kernel: the plan's instantiation, tile counts, storage mask, grid and LDS
int launch_tile(const GemmPlan& p, GemmArgs g, hipStream_t st) {
  set_tiles(g, p);
  g.s16 = p.s16;
  hipLaunchKernelGGL((GemmKernel)p.kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), (size_t)p.lds, st, g);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}
// The split-K weight-gradient GEMM of one Linear over M tokens: dw[N,K] = dy^T[N,M] * x[M,K]. A' = dy^T (dy stored [M][N]),
// B'[K rows][M] = x^T, C = the slabs [splits][N][K]; bias_part: [splits][N] column sums of dy, or null.
GemmArgs dw_args(const XfDwItem& t, int64_t M, const GemmPlan& p) {
  GemmArgs g{};
  g.A = t.dy; g.B = t.x; g.C = t.slabs; g.lda = t.N; g.ldb = t.K; g.ldc = t.K;
  g.M = t.N; g.N = t.K; g.K = (int)M; g.k_chunk = p.k_chunk;
  g.s16 = p.s16; g.bias_part = t.bias_part;
  g.drop = xf_make_dropout(0.f, 0, 0);
  set_tiles(g, p);
  return g;
}
// ---- the launch of gemm_group_kernel: every item's plan is of family kGemmGroup, i.e. on the kernel's one tile
int launch_group(const XfDwItem* items, const GemmPlan* plans, int n, int64_t M, hipStream_t st) {
  GemmGroup p{};
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    p.g[i] = dw_args(items[i], M, plans[i]);
    p.start[i] = (int)total;
    total += plans[i].grid;
    if (total > 0x7fffffffll) return XFMR_EUNSUPPORTED;
    *items[i].splits = plans[i].splits;
  }
  for (int i = n; i <= 4; ++i) p.start[i] = (int)total;
  hipLaunchKernelGGL((gemm_group_kernel<PrecBF16, 128, 64, 128, true, true, EPI_SPLITK, SAB>), dim3((unsigned)total),
                     dim3((unsigned)plans[0].block), (size_t)plans[0].lds, st, p);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

// residual operand of the EPI_DROP_RES_LN family: `residual` (loaded) or `res` (re-derived) -- exactly one
int set_ln_residual(GemmArgs& g, const float* residual, const XfLnResidual* res, XfSeed seed) {
  if ((residual != nullptr) == (res != nullptr)) return XFMR_EINVAL;
  g.R = residual;
  if (!res) return xf_aligned16(residual) ? XFMR_OK : XFMR_EALIGN;
  if (!res->pre || !res->mean || !res->rstd || !res->gamma || !res->beta) return XFMR_EINVAL;
  if (!xf_aligned16(res->pre) || !xf_aligned16(res->gamma) || !xf_aligned16(res->beta)) return XFMR_EALIGN;
  g.rp_pre = res->pre; g.rp_mean = res->mean; g.rp_rstd = res->rstd; g.rp_gamma = res->gamma; g.rp_beta = res->beta;
  g.rp_drop = xf_make_dropout(res->dropout_p, seed, res->site);
  return XFMR_OK;
}

int linear_ln_fwd(const void* x, const float* w, const float* bias, float* pre, int64_t M, int32_t N, int32_t K,
                  const float* residual, const XfLnResidual* res, float dropout_p, XfSeed seed, uint32_t site,
                  const float* gamma, const float* beta, float eps, float* y, void* y16, float* mean, float* rstd,
                  int32_t precision, uint32_t s16, hipStream_t st, bool infer = false) {
  // infer: the forward-only form -- the kGemmLnFwd plan on its EPI_DROP_RES_LN_INFER instantiation; pre / mean / rstd are not taken
  if (!x || !w || !gamma || !beta || (!y && !y16)) return XFMR_EINVAL;
  if (infer ? (pre || mean || rstd || res) : (!pre || !mean || !rstd)) return XFMR_EINVAL;
  const GemmKey k{!res ? kGemmLnFwd : res->dropout_p > 0.f ? kGemmLnFwdReDrop : kGemmLnFwdRe, M, N, K, precision, s16, 1, xf_num_cus()};
  GemmPlan p = gemm_plan(k, gemm_switches_once());
  if (infer && !p.rc) {
    p.kernel = (const void*)ln_infer_kernel(p.precision, p.s16, p.bm, p.bn, p.bk);
    if (!p.kernel) p.rc = XFMR_EUNSUPPORTED;
  }
  GemmArgs g{};
  g.A = x; g.B = w; g.C = pre; g.lda = K; g.ldb = K; g.ldc = N; g.M = M; g.N = N; g.K = K; g.k_chunk = 0;
  g.bias = bias;
  const int res_rc = set_ln_residual(g, residual, res, seed);
  if (const int rc = plan_rc(p, xf_aligned16(x) && xf_aligned16(w) && xf_aligned16(pre) && xf_aligned16(y), res_rc)) return rc;
  g.drop = xf_make_dropout(dropout_p, seed, site);
  g.ln_gamma = gamma; g.ln_beta = beta; g.ln_eps = eps; g.Y = y; g.Y16 = y16; g.ln_mean = mean; g.ln_rstd = rstd;
  return launch_tile(p, g, st);
}

int ffn_fwd_fused(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2, void* u16,
                  void* g16, float* pre, int64_t M, int32_t H, int32_t I, const float* residual, const XfLnResidual* res,
                  float dropout_p, XfSeed seed, uint32_t site, const float* gamma, const float* beta, float eps, float* y,
                  void* y16, float* mean, float* rstd, hipStream_t st, bool infer = false) {
  // infer: the forward-only form (ffn_fwd_infer_kernel) on the kGemmFfnFwd plan; u16 / g16 / pre / mean / rstd are not taken
  if (!x16 || !w1_16 || !b1 || !w2_16 || !gamma || !beta || (!y && !y16)) return XFMR_EINVAL;
  if (infer ? (u16 || g16 || pre || mean || rstd || res) : (!pre || !mean || !rstd)) return XFMR_EINVAL;
  GemmPlan p = gemm_plan(GemmKey{res ? kGemmFfnFwdRe : kGemmFfnFwd, M, H, I, XFMR_PREC_BF16, 0, 1, xf_num_cus()}, gemm_switches());
  if (!p.rc_shape && res && res->dropout_p > 0.f) p.rc_shape = XFMR_EUNSUPPORTED;  // (no dropout on this kernel's residual)
  const bool aligned = xf_aligned16(x16) && xf_aligned16(w1_16) && xf_aligned16(w2_16) && xf_aligned16(pre) && xf_aligned16(y) &&
                       xf_aligned16(u16) && xf_aligned16(g16) && xf_aligned16(y16) && xf_aligned16(b1) && xf_aligned16(b2) &&
                       xf_aligned16(gamma) && xf_aligned16(beta);  // (a null pointer is aligned)
  FfnFwdArgs f{};
  f.X = (const __bf16*)x16; f.W1 = (const __bf16*)w1_16; f.b1 = b1; f.W2 = (const __bf16*)w2_16; f.U = (__bf16*)u16; f.G = (__bf16*)g16;
  f.I = I;
#ifdef XF_FFN_STAMP
  if (const char* e = getenv("XFMR_FFN_STAMPS")) f.stamps = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
  GemmArgs& g = f.e;
  g.C = pre; g.ldc = H; g.M = M; g.N = H; g.K = I; g.bias = b2;
  const int res_rc = set_ln_residual(g, residual, res, seed);
  if (const int rc = plan_rc(p, aligned, res_rc)) return rc;
  g.drop = xf_make_dropout(dropout_p, seed, site);
  g.ln_gamma = gamma; g.ln_beta = beta; g.ln_eps = eps; g.Y = y; g.Y16 = y16; g.ln_mean = mean; g.ln_rstd = rstd;
  set_tiles(g, p);
  const auto kernel = infer ? (p.ffn_chunk == 64 ? ffn_fwd_infer_kernel<64> : ffn_fwd_infer_kernel<128>)
                      : p.ffn_chunk == 64 ? (res ? ffn_fwd_fused_kernel<64, true> : ffn_fwd_fused_kernel<64, false>)
                                          : (res ? ffn_fwd_fused_kernel<128, true> : ffn_fwd_fused_kernel<128, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, st, f);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // namespace


extern "C" {

int xf_gemm_plan(int32_t op, int64_t M, int32_t N, int32_t K, int32_t precision, uint32_t s16, int32_t items, int32_t cus,
                 const int32_t sw[16], int32_t out[24]) {
  static_assert(sizeof(GemmSwitches) == 16 * sizeof(int32_t), "xf_gemm_switches writes the struct as sixteen integers");
  GemmSwitches s;
  memcpy(&s, sw, sizeof s);
  const GemmPlan p = gemm_plan(GemmKey{(GemmOp)op, M, N, K, precision, s16, items, cus}, s);
  const int32_t fields[20] = {p.family, p.epi, p.precision, (int32_t)p.s16, p.bm, p.bn, p.bk, p.splits, p.k_chunk, p.nt_n, p.nt_m,
                              p.nt_z, p.nt_full, p.short_rows, p.grid, p.block, p.lds, p.ffn_chunk, p.ffn_ring, p.records};
  for (int i = 0; i < 24; ++i) out[i] = (i < 20 && p.rc == XFMR_OK) ? fields[i] : 0;
  return p.rc;
}
void xf_gemm_switches(int32_t sw[16]) {
  const GemmSwitches s = gemm_switches();
  memcpy(sw, &s, sizeof s);
}

// thin readers of the plan: the generic slab plan of one weight gradient over M tokens; the M-tiles (= LayerNorm partial
// records) of the whole-row kernels for M rows on this device
int xf_dw_split_plan(int64_t M, int32_t N, int32_t K, int* k_chunk) {
  return dw_split_plan(M, N, K, gemm_switches_once().dw_maxsplit, k_chunk);
}
int xf_ln_row_tiles(int64_t M) {
  return gemm_plan(GemmKey{kGemmDxLnBwd, M, 8, 128, XFMR_PREC_BF16, 0, 1, xf_num_cus()}, gemm_switches_once()).records;
}

// internal (norm.hip): dst[c] = sum over all rows
int xf_rowsum(float* dst, const float* src, int64_t rows, int64_t cols, hipStream_t st) {
  return launch_rowsum(dst, src, rows, cols, rows, st);
}

int xf_linear_fwd_ex(const void* x, const float* w, const float* bias, void* y, int64_t M, int32_t N, int32_t K,
                     int32_t epilogue, const float* residual, void* aux_out, float dropout_p, XfSeed seed,
                     uint32_t site, int32_t precision, uint32_t s16, hipStream_t st) {
  if (!x || !w || !y) return XFMR_EINVAL;
  const bool gelu = epilogue == XFMR_EPI_BIAS_GELU, res = epilogue == XFMR_EPI_BIAS_DROP_RES;
  const GemmKey k{gelu ? kGemmFwdGelu : res ? kGemmFwdDropRes : kGemmFwdBias, M, N, K, precision, s16, 1, 0};
  const GemmPlan p = gemm_plan(k, gemm_switches_once());
  if (const int rc = plan_rc(p, xf_aligned16(x) && xf_aligned16(w) && xf_aligned16(y))) return rc;
  if ((epilogue != XFMR_EPI_BIAS && !gelu && !res) || (gelu && !aux_out) || (res && !residual)) return XFMR_EINVAL;
  GemmArgs g{};
  g.A = x; g.B = w; g.C = y; g.lda = K; g.ldb = K; g.ldc = N; g.M = M; g.N = N; g.K = K; g.k_chunk = 0;
  g.bias = bias; g.R = epilogue == XFMR_EPI_BIAS ? nullptr : residual; g.C2 = aux_out; g.P = nullptr;
  g.aux_grad = (s16 & XF_AUX_GELU_GRAD) != 0;
  g.drop = xf_make_dropout(dropout_p, seed, site);
  return launch_tile(p, g, st);
}

int xf_linear_ln_fwd_ex(const void* x, const float* w, const float* bias, float* pre, int64_t M, int32_t N, int32_t K,
                        const float* residual, float dropout_p, XfSeed seed, uint32_t site, const float* gamma,
                        const float* beta, float eps, float* y, void* y16, float* mean, float* rstd, int32_t precision,
                        uint32_t s16, hipStream_t st) {
  if (!residual || !y) return XFMR_EINVAL;
  return linear_ln_fwd(x, w, bias, pre, M, N, K, residual, nullptr, dropout_p, seed, site, gamma, beta, eps, y, y16, mean,
                       rstd, precision, s16, st);
}
int xf_linear_ln_fwd_re(const void* x, const float* w, const float* bias, float* pre, int64_t M, int32_t N, int32_t K,
                        const XfLnResidual* res, float dropout_p, XfSeed seed, uint32_t site, const float* gamma,
                        const float* beta, float eps, float* y, void* y16, float* mean, float* rstd, int32_t precision,
                        uint32_t s16, hipStream_t st) {
  if (!res) return XFMR_EINVAL;
  return linear_ln_fwd(x, w, bias, pre, M, N, K, nullptr, res, dropout_p, seed, site, gamma, beta, eps, y, y16, mean, rstd,
                       precision, s16, st);
}

int xf_linear_gelu_fwd_infer(const void* x, const float* w, const float* bias, void* y, int64_t M, int32_t N, int32_t K,
                             int32_t precision, uint32_t s16, hipStream_t st) {
  if (!x || !w || !y) return XFMR_EINVAL;
  GemmPlan p = gemm_plan(GemmKey{kGemmFwdGelu, M, N, K, precision, s16, 1, 0}, gemm_switches_once());
  if (!p.rc) {  // the plan's tile, slice depth and grid on the instantiation that stores no auxiliary output
    p.kernel = (const void*)gelu_infer_kernel(p.precision, p.s16, p.bm, p.bn, p.bk);
    if (!p.kernel) p.rc = XFMR_EUNSUPPORTED;
  }
  if (const int rc = plan_rc(p, xf_aligned16(x) && xf_aligned16(w) && xf_aligned16(y))) return rc;
  GemmArgs g{};
  g.A = x; g.B = w; g.C = y; g.lda = K; g.ldb = K; g.ldc = N; g.M = M; g.N = N; g.K = K; g.k_chunk = 0;
  g.bias = bias;
  g.drop = xf_make_dropout(0.f, 0, 0);
  return launch_tile(p, g, st);
}

int xf_linear_ln_fwd_infer(const void* x, const float* w, const float* bias, int64_t M, int32_t N, int32_t K,
                           const float* residual, const float* gamma, const float* beta, float eps, float* y, void* y16,
                           int32_t precision, uint32_t s16, hipStream_t st) {
  if (!residual || !y) return XFMR_EINVAL;
  return linear_ln_fwd(x, w, bias, nullptr, M, N, K, residual, nullptr, 0.f, XfSeed(0, nullptr), 0, gamma, beta, eps, y, y16,
                       nullptr, nullptr, precision, s16, st, true);
}

int xfmr_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int32_t N, int32_t K,
                    int32_t epilogue, const float* residual, float* aux_out, float dropout_p, uint64_t seed,
                    uint32_t site, int32_t precision, void* stream) {
  return xf_linear_fwd_ex(x, w, bias, y, M, N, K, epilogue, residual, aux_out, dropout_p, seed, site, precision, 0,
                          (hipStream_t)stream);
}

int xf_ffn_fwd_fused_ex(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2,
                        void* u16, void* g16, float* pre, int64_t M, int32_t H, int32_t I, const float* residual, float dropout_p,
                        XfSeed seed, uint32_t site, const float* gamma, const float* beta, float eps, float* y,
                        void* y16, float* mean, float* rstd, hipStream_t st) {
  if (!residual || !y) return XFMR_EINVAL;
  return ffn_fwd_fused(x16, w1_16, b1, w2_16, b2, u16, g16, pre, M, H, I, residual, nullptr, dropout_p, seed, site, gamma,
                       beta, eps, y, y16, mean, rstd, st);
}
int xf_ffn_fwd_fused_re(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2,
                        void* u16, void* g16, float* pre, int64_t M, int32_t H, int32_t I, const XfLnResidual* res,
                        float dropout_p, XfSeed seed, uint32_t site, const float* gamma, const float* beta, float eps,
                        float* y, void* y16, float* mean, float* rstd, hipStream_t st) {
  if (!res) return XFMR_EINVAL;
  return ffn_fwd_fused(x16, w1_16, b1, w2_16, b2, u16, g16, pre, M, H, I, nullptr, res, dropout_p, seed, site, gamma, beta,
                       eps, y, y16, mean, rstd, st);
}

int xf_ffn_fwd_fused_infer(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2, int64_t M,
                           int32_t H, int32_t I, const float* residual, const float* gamma, const float* beta, float eps,
                           float* y, void* y16, hipStream_t st) {
  if (!residual || !y) return XFMR_EINVAL;
  return ffn_fwd_fused(x16, w1_16, b1, w2_16, b2, nullptr, nullptr, nullptr, M, H, I, residual, nullptr, 0.f, XfSeed(0, nullptr),
                       0, gamma, beta, eps, y, y16, nullptr, nullptr, st, true);
}

int xf_ffn_bwd_dx_fused_ex(const void* dy16, const void* w2_16, const void* u16, const void* w1_16, void* di16, int64_t M,
                           int32_t H, int32_t I, const float* residual_grad, const float* ln_x, const float* ln_mean,
                           const float* ln_rstd, const float* ln_gamma, float dropout_p, XfSeed seed, uint32_t site,
                           float* dx, void* d_lin16, float* partials, int* blocks_out, hipStream_t st) {
  if (!dy16 || !w2_16 || !u16 || !w1_16 || !di16 || !ln_x || !ln_mean || !ln_rstd || !ln_gamma || !dx || !partials ||
      !blocks_out)
    return XFMR_EINVAL;
  const GemmPlan p = gemm_plan(GemmKey{kGemmFfnBwd, M, H, I, XFMR_PREC_BF16, 0, 1, xf_num_cus()}, gemm_switches());
  if (const int rc = plan_rc(p, xf_aligned16(dy16) && xf_aligned16(w2_16) && xf_aligned16(u16) && xf_aligned16(w1_16) &&
                                    xf_aligned16(di16) && xf_aligned16(dx) && xf_aligned16(ln_x) && xf_aligned16(residual_grad) &&
                                    xf_aligned16(d_lin16) && xf_aligned16(ln_gamma)))
    return rc;
  FfnBwdArgs f{};
  f.DY = (const __bf16*)dy16; f.W2 = (const __bf16*)w2_16; f.U = (const __bf16*)u16; f.W1 = (const __bf16*)w1_16;
  f.DI = (__bf16*)di16; f.I = I;
  GemmArgs& g = f.e;
  g.C = dx; g.ldc = H; g.M = M; g.N = H; g.K = I; g.R = residual_grad;
  g.drop = xf_make_dropout(dropout_p, seed, site);
  g.drop2 = xf_make_dropout(0.f, 0, 0);
  g.ln_gamma = ln_gamma; g.lnb_x = ln_x; g.lnb_mean = ln_mean; g.lnb_rstd = ln_rstd; g.D16 = d_lin16;
  g.lnb_partials = partials;
  set_tiles(g, p);
  *blocks_out = p.records;
  const dim3 grid((unsigned)p.grid), block((unsigned)p.block);
  if (p.ffn_ring) hipLaunchKernelGGL(ffn_bwd_dx_fused_kernel<true>, grid, block, 0, st, f);
  else hipLaunchKernelGGL(ffn_bwd_dx_fused_kernel<false>, grid, block, 0, st, f);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xf_linear_bwd_dx_ex(const void* dy, const float* w, void* dx, int64_t M, int32_t N, int32_t K,
                        const float* residual_grad, const void* gelu_pre, int32_t precision, uint32_t s16,
                        hipStream_t st) {
  if (!dy || !w || !dx) return XFMR_EINVAL;
  const GemmKey k{gelu_pre ? kGemmDxGelu : kGemmDx, M, N, K, precision, s16, 1, 0};
  const GemmPlan p = gemm_plan(k, gemm_switches_once());
  if (const int rc = plan_rc(p, xf_aligned16(dy) && xf_aligned16(w) && xf_aligned16(dx))) return rc;
  // dx[M,K] = dy[M,N] * w[N,K]: contraction over N; B' [K rows][N] = w^T -> w is stored [N][K] = K-major
  GemmArgs g{};
  g.A = dy; g.B = w; g.C = dx; g.lda = N; g.ldb = K; g.ldc = K; g.M = M; g.N = K; g.K = N; g.k_chunk = 0;
  g.bias = nullptr; g.R = residual_grad; g.P = gelu_pre; g.C2 = nullptr;
  g.aux_grad = (s16 & XF_AUX_GELU_GRAD) != 0;
  g.drop = xf_make_dropout(0.f, 0, 0);
  return launch_tile(p, g, st);
}

int xf_linear_bwd_dx_lnbwd_ex(const void* dy, const float* w, int64_t M, int32_t N, int32_t K,
                              const float* residual_grad, const float* ln_x, const float* ln_mean, const float* ln_rstd,
                              const float* ln_gamma, float dropout_p, XfSeed seed, uint32_t site, float* dx,
                              void* d_lin16, float* partials, int* blocks_out, int32_t precision, uint32_t s16,
                              hipStream_t st, float out_dropout_p, uint32_t out_site) {
  if (!dy || !w || !dx || !ln_x || !ln_mean || !ln_rstd || !ln_gamma || !partials || !blocks_out) return XFMR_EINVAL;
  const GemmKey k{kGemmDxLnBwd, M, N, K, precision, s16, 1, xf_num_cus()};
  const GemmPlan p = gemm_plan(k, gemm_switches_once());
  if (const int rc = plan_rc(p, xf_aligned16(dy) && xf_aligned16(w) && xf_aligned16(dx) && xf_aligned16(ln_x))) return rc;
  GemmArgs g{};
  g.A = dy; g.B = w; g.C = dx; g.lda = N; g.ldb = K; g.ldc = K; g.M = M; g.N = K; g.K = N; g.k_chunk = 0;
  g.R = residual_grad;
  g.drop = xf_make_dropout(dropout_p, seed, site);
  g.ln_gamma = ln_gamma; g.lnb_x = ln_x; g.lnb_mean = ln_mean; g.lnb_rstd = ln_rstd; g.D16 = d_lin16;
  g.lnb_partials = partials;
  g.drop2 = xf_make_dropout(out_dropout_p, seed, out_site);
  *blocks_out = p.records;  // the records of the row map this launch runs
  return launch_tile(p, g, st);
}

int xfmr_linear_bwd_dx(const float* dy, const float* w, float* dx, int64_t M, int32_t N, int32_t K,
                       const float* residual_grad, const float* gelu_pre, int32_t precision, void* stream) {
  return xf_linear_bwd_dx_ex(dy, w, dx, M, N, K, residual_grad, gelu_pre, precision, 0, (hipStream_t)stream);
}

size_t xfmr_linear_bwd_dw_workspace(int64_t M, int32_t N, int32_t K) {  // enough for every token count <= M
  return (size_t)dw_split_bound(M, N, K) * (size_t)N * (size_t)K * sizeof(float);
}
size_t xf_linear_bwd_dw_slab_bytes(int64_t M, int32_t N, int32_t K) { return xfmr_linear_bwd_dw_workspace(M, N, K); }

int xf_linear_bwd_dw_ex(const void* dy, const void* x, float* dw, int64_t M, int32_t N, int32_t K, int32_t precision,
                        void* workspace, size_t workspace_bytes, uint32_t s16, hipStream_t st) {
  if (!dy || !x || !dw || !workspace) return XFMR_EINVAL;
  const GemmKey k{kGemmDw, M, N, K, precision, s16, 1, 0};
  const GemmPlan p = gemm_plan(k, gemm_switches_once());
  const int room = (!p.rc_shape && workspace_bytes < xfmr_linear_bwd_dw_workspace(M, N, K)) ? XFMR_EWORKSPACE : XFMR_OK;
  if (const int rc = plan_rc(p, xf_aligned16(dy) && xf_aligned16(x) && xf_aligned16(workspace), room)) return rc;
  const XfDwItem one{dy, x, N, K, (float*)workspace, nullptr, nullptr};
  if (const int rc = launch_tile(p, dw_args(one, M, p), st)) return rc;
  return launch_rowsum(dw, (const float*)workspace, p.splits, (int64_t)N * K, p.splits, st);
}

int xf_linear_bwd_dw_deferred(const void* dy, const void* x, int64_t M, int32_t N, int32_t K, int32_t precision,
                              uint32_t s16, float* slabs, float* bias_part, int* splits_out, hipStream_t st) {
  if (!dy || !x || !slabs || !splits_out) return XFMR_EINVAL;
  const GemmKey k{kGemmDwDeferred, M, N, K, precision, s16, 1, 0};
  const GemmPlan p = gemm_plan(k, gemm_switches_once());
  if (const int rc = plan_rc(p, xf_aligned16(dy) && xf_aligned16(x) && xf_aligned16(slabs))) return rc;
  const XfDwItem one{dy, x, N, K, slabs, bias_part, splits_out};
  if (p.family == kGemmRing) return xf_dw_ring_launch_plans(&one, &p, 1, M, st);  // dw_ring.hip
  *splits_out = p.splits;
  if (p.family == kGemmNone) return XFMR_OK;  // XFMR_EXP_SKIP_DW
  return launch_tile(p, dw_args(one, M, p), st);
}

// internal (encoder.hip): the split-K weight-gradient GEMMs of up to FOUR Linears over the same M tokens in ONE launch -- the
// ring kernel when it takes every item, else gemm_group_kernel when every item is groupable, else one launch each. Results
// are those of xf_linear_bwd_dw_deferred bit for bit (the same plan per item: same tiles, same slabs, same order inside each).
int xf_linear_bwd_dw_group(const XfDwItem* items, int n, int64_t M, int32_t precision, uint32_t s16, hipStream_t st) {
  if (!items || n < 1 || n > 4) return XFMR_EINVAL;
  GemmPlan p[4];
  const auto all_of = [&](const GemmSwitches& sw, int family) {  // plans every item; true: pointers in order, all of `family`
    bool all = true;
    for (int i = 0; i < n; ++i) {
      const XfDwItem& t = items[i];
      p[i] = gemm_plan(GemmKey{kGemmDwGroup, M, t.N, t.K, precision, s16, n, 0}, sw);
      all = all && p[i].family == family && t.dy && t.x && t.slabs && t.splits && xf_aligned16(t.dy) && xf_aligned16(t.x) &&
            xf_aligned16(t.slabs);
    }
    return all;
  };
  GemmSwitches sw = gemm_switches_once();
  if (all_of(sw, kGemmRing)) return xf_dw_ring_launch_plans(items, p, n, M, st);  // dw_ring.hip
  sw.dw_ring = 0;  // (the ring takes a launch whole or not at all)
  if (all_of(sw, kGemmGroup)) return launch_group(items, p, n, M, st);
  for (int i = 0; i < n; ++i) {
    const XfDwItem& t = items[i];
    const int rc = xf_linear_bwd_dw_deferred(t.dy, t.x, M, t.N, t.K, precision, s16, t.slabs, t.bias_part, t.splits, st);
    if (rc != XFMR_OK) return rc;
  }
  return XFMR_OK;
}

int xf_multi_rowsum(const XfReduceSeg* segs, int nseg, hipStream_t st) {
  for (int base = 0; base < nseg; base += 64) {
    MultiSegs m{};
    const int n = nseg - base < 64 ? nseg - base : 64;
    int blocks = 0;
    // tall segments first: a block's lifetime grows with its segment's rows (the LayerNorm records: 1600 rows, 6 round
    // trips; a weight slab: 62-115 rows, one) and the blocks dispatched last set the launch's end
    int order[64];
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order, order + n, [&](int x, int y) { return segs[base + x].rows > segs[base + y].rows; });
    static const bool wide_on = [] { const char* e = getenv("XFMR_ROWSUM_WIDE"); return !(e && *e == '0'); }();  // A/B
    for (int i = 0; i < n; ++i) {
      m.s[i] = segs[base + order[i]];
      m.first[i] = blocks;
      XfReduceSeg& sg = m.s[i];
      const bool wide = wide_on && sg.rows <= 64 && sg.cols >= 256 && !((sg.cols | sg.ld) & 3) &&
                        !(reinterpret_cast<uintptr_t>(sg.src) & 15) && !(reinterpret_cast<uintptr_t>(sg.dst) & 15);
      sg.pad = wide ? 1 : 0;  // (the field is the launch's own: callers leave it 0)
      blocks += sg.cols > 0 ? (wide ? (sg.cols + 255) / 256 : (sg.cols + 63) / 64) : 0;
    }
    m.first[n] = blocks;
    m.n = n;
    if (blocks <= 0) continue;
    hipLaunchKernelGGL(multi_rowsum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, m);
    XF_LAUNCH_CHECK();
  }
  return XFMR_OK;
}

int xfmr_linear_bwd_dw(const float* dy, const float* x, float* dw, int64_t M, int32_t N, int32_t K,
                       int32_t precision, void* workspace, size_t workspace_bytes, void* stream) {
  return xf_linear_bwd_dw_ex(dy, x, dw, M, N, K, precision, workspace, workspace_bytes, 0, (hipStream_t)stream);
}

// the column sums' plan is the row kernels' (norm.hip row_plan): records of rows_per_block rows each, then their sum
size_t xfmr_colsum_workspace(int64_t M, int32_t N) {  // enough for every row count <= M
  return (size_t)row_plan(RowKey{kRowColsum, M, N, 0, 0}).room * (size_t)N * sizeof(float);
}
int xf_colsum_ex(const void* a, bool a16, float* out, int64_t M, int32_t N, void* workspace, hipStream_t st) {
  if (!a || !out || !workspace) return XFMR_EINVAL;
  const RowPlan p = row_plan(RowKey{kRowColsum, M, N, 0, 0});
  if (p.rc) return p.rc;
  int rc = a16 ? launch_rowsum((float*)workspace, (const __bf16*)a, M, N, p.rows_per_block, st)
               : launch_rowsum((float*)workspace, (const float*)a, M, N, p.rows_per_block, st);
  if (rc) return rc;
  return launch_rowsum(out, (const float*)workspace, p.records, N, p.records, st);
}
int xfmr_colsum(const float* a, float* out, int64_t M, int32_t N, void* workspace, void* stream) {
  return xf_colsum_ex(a, false, out, M, N, workspace, (hipStream_t)stream);
}

}  // extern "C"
