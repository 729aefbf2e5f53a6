// Entry points shared between the translation units of libxfmr_hip.so but NOT part of the public C ABI
// (include/xfmr_hip.h): the same operators with type-erased activation pointers and a storage mask, used by the
// whole-encoder launch sequences to keep MFMA-only intermediates in HBM as bf16 (see common.h "Activation
// storage"). The public functions are these with mask 0.
#pragma once
#include "common.h"

enum : uint32_t {
  XF_S16_A = 1u,    // GEMM operand A (activations / incoming gradient)
  XF_S16_B = 2u,    // GEMM operand B when it is an activation (dW)
  XF_S16_C = 4u,    // GEMM output (and the pre-activation side output of the GELU epilogue)
  XF_S16_P = 8u,    // pre-activation input of the gelu' epilogue
  // (not a storage bit) the GELU Linear's auxiliary tensor holds gelu'(pre) instead of pre: the forward epilogue has
  // erf and exp(-x^2/2) in registers anyway, and the backward dX epilogue becomes one multiply
  XF_AUX_GELU_GRAD = 0x100u,
};

// ---- gemm.hip: the plan of one call of the GEMM family (linear forward / dX / dW, the LayerNorm-fused and the fused FFN
// kernels): which kernel runs, with which tile, slabs, grid and LDS, as ONE pure function of the call's key and the
// environment switches (tests/test_gemm_plan_host.py walks the table without a GPU).
enum GemmOp : int32_t {
  kGemmFwdBias = 0, kGemmFwdGelu, kGemmFwdDropRes,  // xf_linear_fwd_ex by epilogue
  kGemmLnFwd, kGemmLnFwdRe, kGemmLnFwdReDrop,       // xf_linear_ln_fwd_ex / _re: residual loaded | re-derived | re-derived + dropout
  kGemmDx, kGemmDxGelu, kGemmDxLnBwd,               // xf_linear_bwd_dx_ex (gelu_pre null | given), xf_linear_bwd_dx_lnbwd_ex
  kGemmDw, kGemmDwDeferred, kGemmDwGroup,           // xf_linear_bwd_dw_ex | _deferred | one item of _group
  kGemmFfnFwd, kGemmFfnFwdRe, kGemmFfnBwd,          // xf_ffn_fwd_fused_ex | _re, xf_ffn_bwd_dx_fused_ex (N = H, K = I)
  kGemmOps
};
enum GemmFamily : int32_t {
  kGemmNone = 0,  // nothing is launched: the call is refused (GemmPlan::rc), or XFMR_EXP_SKIP_DW
  kGemmTile,      // gemm_kernel
  kGemmGroup,     // gemm_group_kernel: this item's share of the launch
  kGemmRing,      // dw_ring.hip dw_ring_kernel: this item's share of the launch
  kGemmFfnFwdKernel, kGemmFfnBwdKernel,  // ffn_fwd_fused_kernel, ffn_bwd_dx_fused_kernel
};
struct GemmKey {  // in the entry points' own terms: M rows (tokens), N output and K input features of the Linear
  GemmOp op;
  int64_t M; int32_t N, K;
  int32_t precision; uint32_t s16;  // the mask as the caller passes it
  int32_t items;                    // kGemmDwGroup: weights in the launch (1 ... 4)
  int32_t cus;                      // compute units of the device (the whole-row kernels' row map): the plan touches no device
};
// The environment, read in one place (gemm_switches). All but the last two once per process; XFMR_FFN_CHUNK and
// XFMR_FFN_REG_STAGE on every call (the tests flip them inside one process).
struct GemmSwitches {
  int32_t tile_bm, tile_bn, tile_bk, tile_set;  // XFMR_GEMM_TILE="bm,bn,bk" (64|128, 64|128, 32|128); set at all
  int32_t dw_bm, dw_bn, dw_tile_set;            // XFMR_DW_TILE="bm,bn": the 128 x 64 split-K tile
  int32_t pad_lds;                              // XFMR_GEMM_PAD_LDS: dynamic LDS bytes of the tile kernel (occupancy experiments)
  int32_t dw_maxsplit;                          // XFMR_DW_MAXSPLIT: 1 ... 256, default 128
  int32_t row_tiles_short;                      // XFMR_ROW_TILES_SHORT: the two-region row map (measured, not the default)
  int32_t skip_dw;                              // XFMR_EXP_SKIP_DW=1: the deferred dW launches nothing (gradients are garbage)
  int32_t dw_ring;                              // XFMR_DW_RING: off only on '0'
  int32_t dwr_tokens, dwr_minwg;                // XFMR_DWR_TOKENS >= 128 (3072), XFMR_DWR_MINWG >= 1 (64): the ring's slab plan
  int32_t ffn_chunk;                            // XFMR_FFN_CHUNK: 64, anything else = 128
  int32_t ffn_reg_stage;                        // XFMR_FFN_REG_STAGE: register-staged weight chunks in the fused FFN backward
};
struct GemmPlan {
  int32_t rc_shape;  // the code of the checks an entry makes BEFORE it looks at its pointers' alignment
  int32_t rc;        // what the call returns for this key when its pointers are in order
  int32_t family, epi, precision; uint32_t s16;  // kernel family, epilogue id, policy and storage mask instantiated
  int32_t bm, bn, bk;
  int32_t splits, k_chunk;                        // weight gradients: slabs and tokens per slab
  int32_t nt_n, nt_m, nt_z, nt_full, short_rows;  // GemmArgs' tile counts and row map
  int32_t grid, block, lds;                       // grid x (group / ring: this item's workgroups), threads, dynamic LDS bytes
  int32_t ffn_chunk, ffn_ring;                    // fused FFN: forward chunk width | backward LDS-DMA ring (0: register-staged)
  int32_t records;                                // LayerNorm partial records written (*blocks_out)
  const void* kernel;                             // kGemmTile: the gemm_kernel instantiation (gemm.hip tile_kernel)
};
GemmPlan gemm_plan(const GemmKey& k, const GemmSwitches& sw);
const GemmSwitches& gemm_switches_once();  // the once-per-process switches (the two per-call ones at their defaults)
GemmSwitches gemm_switches();              // ... with the two per-call ones as the environment has them now
// dw_ring.hip's geometry, which the plan needs: stage depth and ring length are compile-time switches for A/B builds
// (scripts/build_variant.sh; the measurements are with the kernel)
#ifndef XF_DWR_RT
#define XF_DWR_RT 64
#endif
#ifndef XF_DWR_NST
#define XF_DWR_NST 4
#endif
constexpr int kDwRingTile = 128;                  // tile width in features, both ways
constexpr uint64_t kDwRingOffsetLimit = 1ull << 32;  // the gather's byte offsets into an operand are 32-bit
constexpr int kDwRingLds = 2 * XF_DWR_NST * XF_DWR_RT * kDwRingTile * 2;  // dy and x images of every stage, bf16: 128 KB

// ---- norm.hip (row_plan.inc): the plan of one call of the row kernels -- LayerNorm forward, gather + LayerNorm forward,
// LayerNorm backward, the two-level column sum (xf_colsum_ex) -- as ONE pure function of the call's key (DESIGN.md section 4;
// tests/test_row_plan_host.py walks the table without a GPU).
enum RowOp : int32_t { kRowLnFwd = 0, kRowGatherLnFwd, kRowLnBwd, kRowColsum, kRowOps };
enum RowForm : int32_t {
  kRowNone = 0,  // nothing is launched: the call is refused (RowPlan::rc)
  kRowGeneric,   // ln_fwd[_infer]_kernel / ln_bwd_kernel <NPL>: one wave per row, NPL columns per lane; colsum: rowsum_kernel
  kRowFloat4,    // ln_fwd_v4[_infer]_kernel / ln_bwd_v4_kernel <LPR>: H = 4 * LPR, LPR lanes per row, 16 bytes per lane
};
struct RowKey {
  RowOp op;
  int64_t rows;
  int32_t H;        // row width (colsum: the columns N)
  int32_t keep;     // forward: pre / mean / rstd are stored for a backward
  int32_t aligned;  // every pointer the float4 kernels touch is aligned for them: the entry looks at its pointers, the plan does not
};
struct RowPlan {
  int32_t rc;                 // what the call returns for this key: XFMR_EINVAL, XFMR_EUNSUPPORTED (H > 1024) or XFMR_OK
  int32_t form, width;        // RowForm; NPL | LPR (colsum: columns per workgroup)
  int32_t grid, block, lds;   // workgroups (colsum: of the first level), threads, dynamic LDS bytes
  int32_t rows_per_block;
  int32_t records;            // partial records this launch writes (LayerNorm backward: *blocks_out; forward: none)
  int32_t room;               // the most records ANY row count <= rows writes: what the two workspace queries size for
  const void* kernel;         // the LayerNorm instantiation (colsum: rowsum_kernel by element type, gemm.hip)
};
RowPlan row_plan(const RowKey& k);

extern "C" {
// The row plan as integers. out: form, width, grid, block, lds, rows_per_block, records, room, then zeros (all zeros when
// refused). Returns RowPlan::rc; touches no device.
int xf_row_plan(int32_t op, int64_t rows, int32_t H, int32_t keep, int32_t aligned, int32_t out[12]);
// The plan and the switches as integers. out: family, epi, precision, s16, bm, bn, bk, splits, k_chunk, nt_n, nt_m, nt_z,
// nt_full, short_rows, grid, block, lds, ffn_chunk, ffn_ring, records, then zeros (all zeros when refused); sw: the fields
// of GemmSwitches in their order. Returns GemmPlan::rc; touches no device.
int xf_gemm_plan(int32_t op, int64_t M, int32_t N, int32_t K, int32_t precision, uint32_t s16, int32_t items, int32_t cus,
                 const int32_t sw[16], int32_t out[24]);
void xf_gemm_switches(int32_t sw[16]);
int xf_linear_fwd_ex(const void* x, const float* w, const float* bias, void* y, int64_t M, int32_t N, int32_t K,
                     int32_t epilogue, const float* residual, void* aux_out, float dropout_p, XfSeed seed,
                     uint32_t site, int32_t precision, uint32_t s16, hipStream_t st);
// FFN forward in one kernel (bf16 storage, H = 128, I a multiple of 128): u16 <- bf16(x W1^T + b1), g16 <- gelu(u16) (either may be null),
// pre <- dropout(g16 W2^T + b2) + residual, y / y16 / mean / rstd <- LayerNorm(pre). gemm.hip: ffn_fwd_fused_kernel.
int xf_ffn_fwd_fused_ex(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2,
                        void* u16, void* g16, float* pre, int64_t M, int32_t H, int32_t I, const float* residual, float dropout_p,
                        XfSeed seed, uint32_t site, const float* gamma, const float* beta, float eps, float* y,
                        void* y16, float* mean, float* rstd, hipStream_t st);
// The residual operand of the two LayerNorm-fused forward kernels as "re-derived": the OUTPUT of an earlier LayerNorm,
// recomputed from what that LayerNorm stored for its backward (xf_ln_out_drop4) instead of loaded from a stored fp32 copy.
// dropout_p / site: dropout that was applied to that output (the embedding LayerNorm); 0: none.
struct XfLnResidual {
  const float* pre; const float* mean; const float* rstd; const float* gamma; const float* beta;
  float dropout_p; uint32_t site;
};
// xf_ffn_fwd_fused_ex / xf_linear_ln_fwd_ex with residual = *res; y may be null (the fp32 output is not stored: y16 is then
// required -- whoever takes the output as ITS residual re-derives it the same way). The fused FFN takes no dropout on its
// residual (it is always a layer's own LayerNorm 1 output).
int xf_ffn_fwd_fused_re(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2,
                        void* u16, void* g16, float* pre, int64_t M, int32_t H, int32_t I, const XfLnResidual* res,
                        float dropout_p, XfSeed seed, uint32_t site, const float* gamma, const float* beta, float eps,
                        float* y, void* y16, float* mean, float* rstd, hipStream_t st);
int xf_linear_ln_fwd_re(const void* x, const float* w, const float* bias, float* pre, int64_t M, int32_t N, int32_t K,
                        const XfLnResidual* res, float dropout_p, XfSeed seed, uint32_t site, const float* gamma,
                        const float* beta, float eps, float* y, void* y16, float* mean, float* rstd, int32_t precision,
                        uint32_t s16, hipStream_t st);
// The forward-only forms (xfmr_encoder_infer): the plans of xf_linear_fwd_ex (GELU epilogue), xf_linear_ln_fwd_ex and
// xf_ffn_fwd_fused_ex on instantiations that store nothing a backward would read -- no auxiliary GELU output, no pre / mean /
// rstd, no u16 / g16. No dropout (eval); the residual is loaded. The outputs are the training forms' bits.
int xf_linear_gelu_fwd_infer(const void* x, const float* w, const float* bias, void* y, int64_t M, int32_t N, int32_t K,
                             int32_t precision, uint32_t s16, hipStream_t st);
int xf_linear_ln_fwd_infer(const void* x, const float* w, const float* bias, int64_t M, int32_t N, int32_t K,
                           const float* residual, const float* gamma, const float* beta, float eps, float* y, void* y16,
                           int32_t precision, uint32_t s16, hipStream_t st);
int xf_ffn_fwd_fused_infer(const void* x16, const void* w1_16, const float* b1, const void* w2_16, const float* b2, int64_t M,
                           int32_t H, int32_t I, const float* residual, const float* gamma, const float* beta, float eps,
                           float* y, void* y16, hipStream_t st);
// The dX chain of the FFN backward in one kernel (bf16 storage, H = 128, I a multiple of 64; after the fused forward:
// u16 = the saved pre-activation): di16 <- (dy16 W2) * gelu'(u16), then exactly xf_linear_bwd_dx_lnbwd_ex on di16 / W1.
int xf_ffn_bwd_dx_fused_ex(const void* dy16, const void* w2_16, const void* u16, const void* w1_16, void* di16, int64_t M,
                           int32_t H, int32_t I, const float* residual_grad, const float* ln_x, const float* ln_mean,
                           const float* ln_rstd, const float* ln_gamma, float dropout_p, XfSeed seed, uint32_t site,
                           float* dx, void* d_lin16, float* partials, int* blocks_out, hipStream_t st);
int xf_linear_bwd_dx_ex(const void* dy, const float* w, void* dx, int64_t M, int32_t N, int32_t K,
                        const float* residual_grad, const void* gelu_pre, int32_t precision, uint32_t s16,
                        hipStream_t st);
int xf_linear_bwd_dw_ex(const void* dy, const void* x, float* dw, int64_t M, int32_t N, int32_t K, int32_t precision,
                        void* workspace, size_t workspace_bytes, uint32_t s16, hipStream_t st);
int xf_colsum_ex(const void* a, bool a16, float* out, int64_t M, int32_t N, void* workspace, hipStream_t st);
// Deferred form of the weight gradient for the whole-encoder backward: the split-K slabs [splits][N*K] are left in
// `slabs` and, when bias_part is given, the column sums of dy (the Linear's bias gradient) are left as partial rows
// [splits][N] -- both are reduced later by ONE xf_multi_rowsum launch for the whole backward instead of one
// (dW) + two (bias) small launches per Linear. Returns the number of splits in *splits.
size_t xf_linear_bwd_dw_slab_bytes(int64_t M, int32_t N, int32_t K);
int xf_linear_bwd_dw_deferred(const void* dy, const void* x, int64_t M, int32_t N, int32_t K, int32_t precision,
                              uint32_t s16, float* slabs, float* bias_part, int* splits, hipStream_t st);
// up to four of them over the same M tokens in one launch (gemm.hip: gemm_group_kernel)
struct XfDwItem { const void* dy; const void* x; int32_t N, K; float* slabs; float* bias_part; int* splits; };
int xf_linear_bwd_dw_group(const XfDwItem* items, int n, int64_t M, int32_t precision, uint32_t s16, hipStream_t st);
// the slab plan of one weight-gradient GEMM over M tokens (gemm.hip): token chunk per slab, returns the slab count
int xf_dw_split_plan(int64_t M, int32_t N, int32_t K, int* k_chunk);
// dw_ring.hip: the LDS-DMA ring form of the same GEMMs (same plan, same slab layout) for the shapes it takes
bool xf_dw_ring_takes(const XfDwItem* items, int n, int64_t M, int32_t precision, uint32_t s16);
int xf_dw_ring_launch(const XfDwItem* items, int n, int64_t M, hipStream_t st);  // plans for itself (the probes)
int xf_dw_ring_launch_plans(const XfDwItem* items, const GemmPlan* plans, int n, int64_t M, hipStream_t st);
// dst[c] = sum_r src[r * ld + c], r < rows, c < cols, for every segment, in one launch (deterministic order)
struct XfReduceSeg { const float* src; float* dst; int rows; int cols; int ld; int pad; };
int xf_multi_rowsum(const XfReduceSeg* segs, int nseg, hipStream_t st);
int xf_rowsum(float* dst, const float* src, int64_t rows, int64_t cols, hipStream_t st);
int xf_attn_fwd_ex(const void* qkv, const uint8_t* key_mask, void* ctx, float* lse, int32_t B, int32_t L, int32_t A,
                   int32_t H, float dropout_p, XfSeed seed, uint32_t site, int32_t precision, bool s16,
                   bool causal, hipStream_t st, const int32_t* seq_offsets = nullptr,  // packed rows: xfmr_encoder_cfg
                   bool stream_keys = false);  // the key-streaming form at any L (XFMR_ATTN_STREAM_KEYS): generic kernels, and
                                               // bf16 at head size 32 without seq_offsets -- its streaming two-kernel
                                               // form, bit-identical to the two-kernel panel form
int xf_attn_bwd_ex(const void* qkv, const uint8_t* key_mask, const void* ctx, const float* lse, const void* d_ctx,
                   void* d_qkv, int32_t B, int32_t L, int32_t A, int32_t H, float dropout_p, XfSeed seed,
                   uint32_t site, int32_t precision, bool s16, bool causal, hipStream_t st,
                   const int32_t* seq_offsets = nullptr, bool stream_keys = false);
// loss.hip: deterministic totals of per-block fp64 records [24][nblocks] (each block = rows_per_block queries) ->
// losses[14], stats[16]; counts = device {n_valid, n_query}; tot = 24 doubles of scratch
int xf_loss_finalize(const double* blockpart, int nblocks, int rows_per_block, const int* counts, int mode,
                     int64_t n_rows, int64_t positions, float* losses, float* stats, double* tot, hipStream_t st);
// Linear (+ bias, dropout, residual) with the LayerNorm that follows it applied in the GEMM epilogue (N == 128, bf16
// policy): pre = the LayerNorm input (saved for the backward), y / y16 = the output, mean / rstd per row.
int xf_linear_ln_fwd_ex(const void* x, const float* w, const float* bias, float* pre, int64_t M, int32_t N, int32_t K,
                        const float* residual, float dropout_p, XfSeed seed, uint32_t site, const float* gamma,
                        const float* beta, float eps, float* y, void* y16, float* mean, float* rstd, int32_t precision,
                        uint32_t s16, hipStream_t st);
// dx_ln_in[M,128] = LayerNormBackward(dy[M,N] * w[N,128] + residual_grad) in one kernel (bf16 policy): the dX GEMM whose
// output is the gradient of a LayerNorm output applies that LayerNorm's backward in its epilogue. d_lin16 (bf16,
// optional) = the dropout-scaled copy; partials[*blocks_out][3][128] = d gamma / d beta / d bias partial records.
// out_dropout_p / out_site: dropout that was applied to the LayerNorm OUTPUT (the embedding LayerNorm).
int xf_linear_bwd_dx_lnbwd_ex(const void* dy, const float* w, int64_t M, int32_t N, int32_t K,
                              const float* residual_grad, const float* ln_x, const float* ln_mean, const float* ln_rstd,
                              const float* ln_gamma, float dropout_p, XfSeed seed, uint32_t site, float* dx,
                              void* d_lin16, float* partials, int* blocks_out, int32_t precision, uint32_t s16,
                              hipStream_t st, float out_dropout_p = 0.f, uint32_t out_site = 0);
// number of 64-row M-tiles (one LayerNorm partial record each) the whole-row kernels run for M rows: >= (M + 63) / 64
// (GemmPlan::records on this device; short last-round tiles: gemm.hip row_tiles)
int xf_ln_row_tiles(int64_t M);
// LayerNorm forward variants that also write a bf16 copy of the output (the operand of the GEMMs that consume it;
// the fp32 output stays the residual stream). y16 / out16 may be null. mean / rstd (and the gather's pre) all null: the
// forward-only instantiations, which store none of them and write the same output bits (xfmr_encoder_infer).
int xf_layernorm_fwd_ex(const float* x, const float* gamma, const float* beta, float* y, void* y16, float* mean,
                        float* rstd, int64_t rows, int32_t H, float eps, hipStream_t stream);
int xf_embed_ln_fwd_ex(const int64_t* item_idx, const float* table, int64_t n_rows, const float* pos_emb,
                       const float* type_emb, const float* gamma, const float* beta, float* out, void* out16,
                       float* pre, float* mean, float* rstd, uint8_t* key_mask, int32_t B, int32_t L, int32_t H,
                       float eps, float dropout_p, XfSeed seed, uint32_t site, hipStream_t stream);
int xf_embed_ln_fwd_packed_ex(const int64_t* item_idx, const float* table, int64_t n_rows, const float* pos_emb,
                              const float* type_emb, const float* gamma, const float* beta, float* out, void* out16,
                              float* pre, float* mean, float* rstd, uint8_t* key_mask, int64_t rows, const int32_t* row_pos,
                              int32_t H, float eps, float dropout_p, XfSeed seed, uint32_t site, hipStream_t stream);
int xf_embed_param_grads_packed(const float* d_pre, float* d_pos, float* d_type, const int32_t* offs, int32_t B, int32_t L,
                                int32_t H, int32_t max_pos, hipStream_t st);
// encoder.hip: the forms a training step takes for this configuration (EncPlan), as integers: Tplan, T, mix, causal, fuse_ln,
// fuse_ffn, rederive, fuse_ffn_bwd, dw_buffers_per_layer, dw_side, group_dw, lin_copy, half_layer, then zeros. Returns
// check_cfg's code; reads the cfg's pointers only for being null or not.
int xf_encoder_plan(const xfmr_encoder_cfg* cfg, int32_t out[16]);
// attention.hip: the kernels xf_attn_fwd_ex (bwd = 0) / xf_attn_bwd_ex (bwd = 1) would launch for these arguments (AttnPlan), as
// integers: form (AttnForm), kernels, grid x, grid y, block, dynamic LDS bytes of the first and of the second kernel, then
// zero. packed = seq_offsets given; switches = the bits of xf_attn_switches, which the real entries read from the
// environment (1: XFMR_ATTN_FWD_SPLIT, 2: XFMR_ATTN_BWD_SPLIT, 4: XFMR_ATTN_BWD_FORM=roles). Returns the code the call would
// return for its shape, precision and layout (check_shape first); touches no device.
int xf_attn_plan(int32_t bwd, int32_t precision, int32_t s16, int32_t B, int32_t L, int32_t A, int32_t H, int32_t causal,
                 int32_t packed, int32_t stream_keys, int32_t switches, int32_t out[8]);
int xf_attn_switches();
// loss.hip: what xfmr_sampled_loss[_prepared, _lists] would launch for this key (LossPlan), as integers. The key: T positions (or
// list rows), H, n_rows, the xfmr_loss_cfg fields, whether d_tok and table_bf16 are given, the device's compute units, and
// `switches`, the bits of xf_loss_switches, which the real entries read from the environment (bit 0: XFMR_LOSS_Q_FP32,
// bit 1: XFMR_LOSS_LOGM256 not off, bits 2-32: XFMR_LOSS_NSPLIT, bits 33-63: XFMR_LOSS_NSPLIT_GRAD; 0 = unset or <= 0).
// out: family (0 generic bf16, 1 generic fp32, 2 LDS-DMA), hard-negative prologue, qprep launch, number of passes; two
// passes of 11 -- role (0 gradient or a generic call's only kernel, 1 logging), HEAD_* code (generic: template width), ALL
// (generic), grid x, y, z, nsplit, record buffer (0 part, 1 part2), query image, in-kernel finish, pin_part --; the combine
// kernel's need_grad, nsplit, nsplit_loss, values' buffer, lse_from_grad, skip_train_head, values-only variant, blocks;
// then zeros. Returns the code the call would return for the key (all zeros then); touches no device.
int xf_loss_plan(int64_t T, int32_t H, int64_t n_rows, int32_t train_head, int32_t all_heads, int32_t mask_false_negatives,
                 int32_t mode, int32_t precision, int32_t num_hard_negatives, uint32_t flags, int32_t has_d_tok,
                 int32_t has_table_bf16, int32_t cus, uint64_t switches, int32_t out[40]);
// The plan's later fields, for the same key (xf_loss_plan's layout stays as its test reads it): ext[0] = the gradient pass
// keeps no count of the counted logits (a lean InfoNCE code beside a logging pass, or under XFMR_LOSS_STATS_ELSEWHERE);
// then zeros. Same return code.
int xf_loss_plan_ext(int64_t T, int32_t H, int64_t n_rows, int32_t train_head, int32_t all_heads, int32_t mask_false_negatives,
                     int32_t mode, int32_t precision, int32_t num_hard_negatives, uint32_t flags, int32_t has_d_tok,
                     int32_t has_table_bf16, int32_t cus, uint64_t switches, int32_t ext[8]);
uint64_t xf_loss_switches();
// d_lin (optional): the gradient of the Linear output feeding this LayerNorm (dropout-scaled dx), bf16 if lin16
// d_gamma == d_beta == d_bias == nullptr defers the reduction of `partials` ([blocks][3][H], blocks returned in
// *blocks_out) to the caller (xf_multi_rowsum)
int xf_layernorm_bwd_impl(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                          float* dx, void* d_lin, bool lin16, float* d_gamma, float* d_beta, float* d_bias,
                          int64_t rows, int32_t H, XfDropout drop_out, XfDropout drop_lin, void* partials,
                          hipStream_t st, int* blocks_out = nullptr);
}
// norm.hip -> session.hip (C++ linkage, like gemm_plan: nothing outside the library calls it): xfmr_pool's rule over the
// session store -- sequence i = rows [0, lens[i]) of slot slots[i] of tok [n_slots][max_len][H] with that slot's mask bytes,
// and xfmr_l2_normalize_fwd in the same launch. An empty sequence or a slot out of range: a zero row.
int pool_slots_launch(const float* tok, const uint8_t* mask, const int32_t* slots, const int32_t* lens, int32_t n,
                      int32_t n_slots, int32_t max_len, int32_t H, int32_t mode, int32_t normalize, float eps, float* out,
                      hipStream_t st);
