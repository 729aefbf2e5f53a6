// Whole-encoder forward / backward: the launch sequence of BertEmbeddings + N x BertLayer over the
// kernels of this library, with a deterministic carve of the caller's activation workspace.
// Host code only (no kernels here): everything is enqueued on the caller's stream, nothing synchronises,
// so one training step can be captured into a hipGraph.
#include <math.h>
#include <stdlib.h>
#include <new>
#include <string.h>

#include "internal.h"

namespace {

struct LayerParams {
  int64_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
};
struct ParamLayout {
  int64_t pos, type, eg, eb;
  int64_t total;
};

int64_t layer_base(const xfmr_encoder_cfg* c, int i, ParamLayout* pl) {
  const int64_t H = c->hidden, I = c->inter;
  pl->pos = 0;
  pl->type = pl->pos + (int64_t)c->max_pos * H;
  pl->eg = pl->type + 2 * H;
  pl->eb = pl->eg + H;
  const int64_t first = pl->eb + H;
  const int64_t per = 3 * H * H + 3 * H + H * H + H + 2 * H + I * H + I + H * I + H + 2 * H;
  pl->total = first + per * c->layers;
  return first + per * i;
}
LayerParams layer_params(const xfmr_encoder_cfg* c, int i) {
  ParamLayout pl;
  const int64_t H = c->hidden, I = c->inter;
  int64_t o = layer_base(c, i, &pl);
  LayerParams p;
  p.wqkv = o; o += 3 * H * H;
  p.bqkv = o; o += 3 * H;
  p.wo = o; o += H * H;
  p.bo = o; o += H;
  p.ln1g = o; o += H;
  p.ln1b = o; o += H;
  p.w1 = o; o += I * H;
  p.b1 = o; o += I;
  p.w2 = o; o += H * I;
  p.b2 = o; o += H;
  p.ln2g = o; o += H;
  p.ln2b = o; o += H;
  return p;
}

// Activation storage: with the bf16 MFMA policy the tensors that are only ever MFMA operands are kept in HBM as
// bf16 ("mixed" storage; bit-identical products, half the bytes): qkv, ctx, the GELU output g, and in backward the
// gradients d_lin / d_ctx / dQKV / dI that feed the dX and dW GEMMs. f1 holds gelu'(pre) -- not the pre-activation: the forward
// epilogue has erf and exp(-x^2/2) in registers, the backward epilogue multiplies -- and is bf16 too. Everything that is added,
// normalised or reduced elementwise (residual streams, LayerNorm inputs, statistics) stays fp32.
// XFMR_ACT_FP32=1 keeps every activation fp32 (A/B measurements).
struct LayerActs {
  void *qkv, *ctx, *f1, *g;                                           // bf16 when mixed
  float *lse, *pre1, *mean1, *rstd1, *x1, *pre2, *mean2, *rstd2, *x2;  // always fp32
  void *x1b, *x2b;  // mixed storage: bf16 copies of the LayerNorm outputs (GEMM operands; x1 / x2 stay the residuals -- or go
                    // unwritten where the residual is re-derived: EncPlan::rederive)
};
// Per-layer reduction inputs of the backward pass, reduced by ONE launch at its end (xf_multi_rowsum): split-K slabs
// of the four weight gradients, partial rows of the two bias gradients that are column sums (b1, bqkv -- produced by
// the dW GEMMs themselves), LayerNorm partial records (d gamma, d beta, and the bias gradients bo / b2).
struct RedBufs {
  float *w2, *w1, *wo, *wqkv, *b1, *bqkv, *ln2, *ln1;
};
struct Acts {
  float *emb_pre, *emb_mean, *emb_rstd, *x0;
  void* x0b;      // bf16 copy of x0 (mixed storage)
  float* emb_ln;  // embedding LayerNorm partial records
  float *dA, *dB;
  void *dLin, *dCtx, *dI, *dQKV;  // bf16 when mixed
  void* dLin2;  // in-line form: the out-proj Linear's output gradient (dLin keeps the FFN2 Linear's until the layer's
                // weight-gradient GEMMs have gone out together: xf_linear_bwd_dw_group)
  void* wbf;      // bf16 copy of the flat parameter buffer (mixed storage): the B operand of the forward / dX GEMMs
  void* scratch;  // ln-bwd partials / dW slabs / colsum partials (used one at a time)
  size_t scratch_bytes;
  size_t total;
};
// The gradient buffers one layer's weight-gradient GEMMs read: dLin in its two roles (gradient of the FFN2 / of the out-proj
// Linear's output), dI and dQKV. One set PER LAYER for the side-stream dW GEMMs (xfmr_encoder_bwd) -- no buffer is
// rewritten while a weight-gradient GEMM may still read it; otherwise every layer's set is the shared buffers of Acts.
struct GradBufs { void *dLinF, *dLinO, *dI, *dQKV; };

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// fp32 parameters -> the bf16 copy the MFMA B operands are staged from (the bf16 policy rounds them at staging time
// anyway: identical products, half the L2 -> LDS bytes of the most re-read operand)
__global__ __launch_bounds__(256) void params_to_bf16_kernel(const float* src, __bf16* dst, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) xf_st4<true>(dst, 4 * i, *reinterpret_cast<const float4*>(src + 4 * i));
}

bool mixed_storage(const xfmr_encoder_cfg* c) {
  static const bool force_fp32 = [] {
    const char* e = getenv("XFMR_ACT_FP32");
    return e && *e && *e != '0';
  }();
  return c->precision == XFMR_PREC_BF16 && !force_fp32;
}
// measurement events of the call's configuration (xfmr_encoder_cfg.profile_*): event `which` of the pair, on `st`, when
// this is the part and the layer the caller named
int prof(const xfmr_encoder_cfg* c, int kind, int layer, int which, hipStream_t st) {
  if (c->profile_kernel != kind || c->profile_layer != layer || !c->profile_events[which]) return XFMR_OK;
  return hipEventRecord((hipEvent_t)c->profile_events[which], st) == hipSuccess ? XFMR_OK : XFMR_EHIP;
}

// Which form every part of a training step takes: a pure function of the configuration (its XFMR_ENC_* flag bits included)
// and of three environment variables, made once per call (make_plan) and read by carve(), xfmr_encoder_fwd and
// xfmr_encoder_bwd. Both calls of a step get the same cfg, so they agree on it (f1 holds u after the fused FFN kernel,
// gelu'(u) after the two-kernel form; the workspace has per-layer gradient buffers exactly where the backward uses them).
struct EncPlan {
  // Tplan: what the workspace is carved for and the forms are decided with (batch x seq_len); T: the rows the row-wise
  // kernels run -- fewer in the packed layout
  int64_t Tplan, T;
  bool mix, causal;  // bf16 storage of the MFMA-only tensors (LayerActs); the reference's attention mask
  bool fuse_ln, fuse_ffn, rederive, fuse_ffn_bwd, dw_buffers_per_layer, dw_side, group_dw, lin_copy;  // (make_plan)
  int half_layer;  // the layer behind which the upper half of the gradient is reduced early; -1: none
};
constexpr int64_t kDwSideTokens = 40960;
// the token counts (batch x seq_len) from which the LayerNorm-fused GEMMs and the fused FFN kernel run: make_plan has the reasons
constexpr int64_t kFfnFusedTokens = 16384;
int64_t ln_fused_min_tokens() {
  static const int64_t min_tokens = [] { const char* e = getenv("XFMR_LN_FUSED_MIN_TOKENS"); return e ? (int64_t)atoll(e) : (int64_t)12288; }();
  return min_tokens;
}
EncPlan make_plan(const xfmr_encoder_cfg* c) {
  EncPlan p{};
  const uint32_t f = c->flags;
  p.Tplan = (int64_t)c->batch * c->seq_len;
  p.T = c->seq_offsets ? c->packed_rows : p.Tplan;
  p.mix = mixed_storage(c);
  p.causal = !(f & XFMR_ENC_BIDIRECTIONAL);
  // out-proj / FFN2 GEMM + LayerNorm as one kernel (and LayerNorm backward in the dX GEMM epilogues): its 64 x 128 tiles
  // are T / 64 workgroups -- below one per CU (T < 16 384) the two-kernel form with 64 x 64 tiles is faster (batch 32:
  // -1.5 % fused; batch 128: +0.9 %; 512: +1.8 %)
  // (round 4: from 12 288 tokens -- batch 64 x 200: 0.876 against 0.889 ms with the two LayerNorm-fused GEMMs and the FFN as
  //  separate GEMMs; at batch 32 nothing in it, 0.662 against 0.661-0.672. XFMR_LN_FUSED_MIN_TOKENS for experiments.)
  p.fuse_ln = p.mix && c->hidden == 128 && p.Tplan >= ln_fused_min_tokens() && !(f & XFMR_ENC_LN_UNFUSED);
  // FFN1 -> GELU -> FFN2 -> LayerNorm as one forward kernel (gemm.hip: ffn_fwd_fused_kernel): the same conditions plus I a
  // multiple of its chunk widths
  // (the fused FFN pair keeps its 16 384 tokens: at 12 800 it measured 0.887 against 0.876 ms for the separate GEMMs)
  p.fuse_ffn = p.fuse_ln && p.Tplan >= kFfnFusedTokens && (c->inter % 128) == 0 && c->inter <= 1024 && !(f & XFMR_ENC_FFN_UNFUSED);
  // Under the LayerNorm-fused forms the fp32 LayerNorm outputs x0, x1 and x2 (of every layer but the last) are not stored: the
  // backward never reads them, and their one reader -- the next kernel's residual operand -- re-derives them from pre / mean /
  // rstd, which are stored for the backward anyway (XfLnResidual). XFMR_LN_STORE_X=1 (read per call: tests, A/B timing)
  // stores them and loads the residual as before; results are bit-identical either way.
  const char* const store_x = getenv("XFMR_LN_STORE_X");
  p.rederive = p.fuse_ln && !(store_x && *store_x && *store_x != '0');
  // the FFN backward's dX chain + LayerNorm 1 backward as one kernel
  p.fuse_ffn_bwd = p.fuse_ffn && p.fuse_ln && !(f & XFMR_ENC_FFN_BWD_UNFUSED);
  // Shapes whose backward runs the weight-gradient GEMMs on the side stream (xfmr_encoder_bwd): those of the LayerNorm-fused
  // dX GEMMs. The workspace holds one GradBufs per layer for them.
  // (round 2 set T >= 65 536: at batch 128 x 200 tokens the step is 1.36 ms of ~70 launches from one host thread and the 32 extra event
  //  calls cost more than the overlap gives -- 1.40 vs 1.355 ms; batch 256: even; batch 512: -2.4 %)
  // (round 4, with the ring weight-gradient kernel: from 40 960 tokens -- batch 256 x 200 dense 1.925-1.927 against 1.941-1.943 ms,
  //  MovieLens-like packed batches of 512 (~50 k rows) 1.912 against 1.942; packed batches of 256 (~25 k rows) 1.265 against
  //  1.237: in line below)
  // (+236 MB per layer at T = 102 400, I = 512: only when the backward will use the side stream)
  const bool side_any = (f & XFMR_ENC_DW_SIDE_ANY) != 0;
  p.dw_buffers_per_layer = p.mix && c->layers <= 64 && (side_any || (c->hidden == 128 && p.Tplan >= kDwSideTokens)) &&
                           c->context && !(f & XFMR_ENC_DW_INLINE);
  // (the per-layer gradient buffers make this independent of the LayerNorm-fused forms: a dW GEMM only ever reads the
  //  GradBufs of ITS layer and activations of the forward)
  // (packed rows: the workspace has the per-layer buffers whenever the PADDED size asks for them; whether the side stream pays
  //  is a question of the rows actually run -- ~50 000 packed rows of a MovieLens-like batch of 512: 1.915 in line against
  //  1.95 ms on the side stream, like a dense batch of 256)
  p.dw_side = p.dw_buffers_per_layer && (side_any || p.T >= kDwSideTokens || !c->seq_offsets);
  // In line (no side stream) the four weight-gradient GEMMs of the layer go out in ONE launch once its last operand
  // (dQKV) exists (xf_linear_bwd_dw_group; same slabs bit for bit): 16 launches of ~8 us become 4 at batch 32. On the side
  // stream each GEMM keeps its own launch: there the FFN2 one starts underneath the FFN dX kernel, long before dQKV exists.
  // (grouped on the side stream too: 3.245-3.265 against 3.244-3.269 ms/step at batch 512, 6.09-6.16 against 6.07-6.10 at 1024)
  p.group_dw = !(f & XFMR_ENC_DW_UNPAIRED) && !p.dw_side && p.mix;  // (bf16 storage: the dLin copies exist; fp32 keeps one launch each)
  p.lin_copy = c->hidden_dropout > 0.f || p.mix;  // the LayerNorm backward writes d_lin: without dropout and with fp32 storage d_lin IS dx
  p.half_layer = ((c->grads_half_event || (f & XFMR_ENC_REDUCE_HALF_EARLY)) && c->layers >= 2) ? c->layers / 2 : -1;
  return p;
}

// The caller's activation workspace, carved once per call. Every layer's block of a kind has the same size, so layer i's
// pointers are a walk over one block from layer 0's offset plus i strides: the order of a block's tensors is written once
// (take_*) and serves the stride and the lookup. base may be null (size query: null pointers, total valid).
struct Bump {
  unsigned char* base;
  size_t o;
  void* bytes(size_t n) { void* p = base ? base + o : nullptr; o += up256(n); return p; }
  float* f32(size_t n) { return reinterpret_cast<float*>(bytes(n * sizeof(float))); }
};
struct Workspace {
  Acts a;
  unsigned char* base;
  int layers;
  bool per_layer;  // EncPlan::dw_buffers_per_layer
  size_t T, TH, TI, lse, es, xb, slab_w2, slab_w1, slab_wo, slab_wqkv, b1, bqkv, lnrec;  // element counts; es, xb: bytes
  size_t grads0, grads_stride, red0, red_stride, act0, act_stride;  // byte offset of layer 0's block, bytes per layer

  RedBufs take_red(Bump& k) const {
    RedBufs r;
    r.w2 = k.f32(slab_w2); r.w1 = k.f32(slab_w1); r.wo = k.f32(slab_wo); r.wqkv = k.f32(slab_wqkv);
    r.b1 = k.f32(b1); r.bqkv = k.f32(bqkv);
    r.ln2 = k.f32(lnrec); r.ln1 = k.f32(lnrec);
    return r;
  }
  LayerActs take_acts(Bump& k, bool last) const {
    LayerActs l;
    l.qkv = k.bytes(3 * TH * es); l.lse = k.f32(lse);
    l.ctx = k.bytes(TH * es);
    l.pre1 = k.f32(TH); l.mean1 = k.f32(T); l.rstd1 = k.f32(T); l.x1 = k.f32(TH);
    l.f1 = k.bytes(TI * es); l.g = k.bytes(TI * es);
    l.pre2 = k.f32(TH); l.mean2 = k.f32(T); l.rstd2 = k.f32(T); l.x2 = k.f32(TH);
    l.x1b = k.bytes(xb); l.x2b = k.bytes(last ? 0 : xb);  // (nothing reads the last layer's: 0 bytes, nothing behind it)
    return l;
  }
  RedBufs red(int i) const { Bump k{base, red0 + (size_t)i * red_stride}; return take_red(k); }
  LayerActs layer(int i) const { Bump k{base, act0 + (size_t)i * act_stride}; return take_acts(k, i + 1 == layers); }
  // Layer i's gradient buffers as the workspace has them: the shared ones (dLin in both roles), or its own set -- layer 0
  // keeps the shared dLin / dI / dQKV and has only dLinO of its own, in front of the other layers' blocks.
  GradBufs grads(int i) const {
    if (!per_layer) return {a.dLin, a.dLin, a.dI, a.dQKV};
    Bump k{base, i ? grads0 + up256(TH * es) + (size_t)(i - 1) * grads_stride : grads0};
    if (i == 0) return {a.dLin, k.bytes(TH * es), a.dI, a.dQKV};
    return {k.bytes(TH * es), k.bytes(TH * es), k.bytes(TI * es), k.bytes(3 * TH * es)};  // (evaluated left to right)
  }
};

Workspace carve(const xfmr_encoder_cfg* c, const EncPlan& plan, unsigned char* base) {
  const int64_t T = plan.Tplan;
  const int32_t H = c->hidden, I = c->inter;
  Workspace w{};
  w.base = base; w.layers = c->layers; w.per_layer = plan.dw_buffers_per_layer;
  w.T = (size_t)T; w.TH = w.T * H; w.TI = w.T * I;
  w.lse = (size_t)c->batch * c->heads * c->seq_len;
  w.es = plan.mix ? 2 : 4;  // bytes per element of the MFMA-only tensors
  w.xb = plan.mix ? w.TH * 2 : 0;
  Bump k{base, 0};
  Acts& a = w.a;
  a.emb_pre = k.f32(w.TH); a.emb_mean = k.f32(w.T); a.emb_rstd = k.f32(w.T); a.x0 = k.f32(w.TH);
  a.x0b = k.bytes(w.xb);
  a.dA = k.f32(w.TH); a.dB = k.f32(w.TH);
  a.dLin = k.bytes(w.TH * w.es); a.dCtx = k.bytes(w.TH * w.es);
  a.dLin2 = k.bytes(w.TH * w.es);
  a.dI = k.bytes(w.TI * w.es); a.dQKV = k.bytes(3 * w.TH * w.es);
  w.grads0 = k.o;
  w.grads_stride = 2 * up256(w.TH * w.es) + up256(w.TI * w.es) + up256(3 * w.TH * w.es);
  if (w.per_layer) k.o += up256(w.TH * w.es) + (size_t)(c->layers - 1) * w.grads_stride;
  a.wbf = k.bytes(plan.mix ? (size_t)xfmr_param_count(c) * 2 : 0);
  const size_t ln_ws = xfmr_layernorm_bwd_workspace(T, H);
  size_t sc = ln_ws;
  for (size_t s : {xfmr_linear_bwd_dw_workspace(T, 3 * H, H), xfmr_linear_bwd_dw_workspace(T, I, H),
                   xfmr_linear_bwd_dw_workspace(T, H, I), xfmr_linear_bwd_dw_workspace(T, H, H),
                   xfmr_colsum_workspace(T, 3 * H), xfmr_colsum_workspace(T, I)})
    if (s > sc) sc = s;
  a.scratch = k.bytes(sc);
  a.scratch_bytes = sc;
  // LayerNorm partial records [blocks][3][H]: from the LayerNorm backward kernel, or one per 64-row tile from the dX GEMM
  // that applies the LayerNorm backward in its epilogue
  w.lnrec = ln_ws / sizeof(float);
  const size_t lnrec_fused = (size_t)xf_ln_row_tiles(T) * 3 * H;
  if (lnrec_fused > w.lnrec) w.lnrec = lnrec_fused;
  a.emb_ln = k.f32(w.lnrec);
  w.slab_w2 = xf_linear_bwd_dw_slab_bytes(T, H, I) / sizeof(float); w.slab_w1 = xf_linear_bwd_dw_slab_bytes(T, I, H) / sizeof(float);
  w.slab_wo = xf_linear_bwd_dw_slab_bytes(T, H, H) / sizeof(float); w.slab_wqkv = xf_linear_bwd_dw_slab_bytes(T, 3 * H, H) / sizeof(float);
  w.b1 = 256 * (size_t)I; w.bqkv = 256 * 3 * (size_t)H;  // <= 256 splits (dw_split_plan)
  w.red0 = k.o; w.take_red(k); w.red_stride = k.o - w.red0;  // (one block walked for its size)
  w.act0 = k.o = w.red0 + (size_t)c->layers * w.red_stride;
  w.take_acts(k, false); w.act_stride = k.o - w.act0;
  a.total = w.act0 + (size_t)c->layers * w.act_stride - up256(w.xb);  // (the last layer has no x2b)
  return w;
}

int check_cfg(const xfmr_encoder_cfg* c) {
  if (!c) return XFMR_EINVAL;
  if (c->batch <= 0 || c->seq_len <= 0 || c->hidden <= 0 || c->heads <= 0 || c->inter <= 0 || c->layers <= 0)
    return XFMR_EINVAL;
  if (c->seq_len > c->max_pos) return XFMR_EINVAL;
  if ((c->hidden != c->heads * 32 && c->hidden != c->heads * 64) || (c->inter & 3)) return XFMR_EUNSUPPORTED;
  if (c->precision != XFMR_PREC_F32 && c->precision != XFMR_PREC_BF16) return XFMR_EINVAL;
  if (c->flags & ~(uint32_t)XFMR_ENC_FLAGS_ALL) return XFMR_EINVAL;  // unknown flag bits
  if (c->profile_kernel < XFMR_PROF_NONE || c->profile_kernel > XFMR_PROF_REDUCE) return XFMR_EINVAL;
  if (c->seq_offsets) {  // packed rows (ABI 3)
    if (!c->row_pos || c->packed_rows <= 0 || c->packed_rows > (int64_t)c->batch * c->seq_len) return XFMR_EINVAL;
    // the kernels that walk a sequence by its offsets: the bf16 policy's head-size-32 causal attention (the one-workgroup forms
    // up to 512 rows per sequence, the key-streaming forms beyond); everything else is row-wise and does not care
    if (!mixed_storage(c) || c->hidden != c->heads * 32 || (c->flags & XFMR_ENC_BIDIRECTIONAL))
      return XFMR_EUNSUPPORTED;
  } else if (c->row_pos || c->packed_rows) {
    return XFMR_EINVAL;
  }
  return XFMR_OK;
}

// ---- the forward-only pass (xfmr_encoder_infer): the same forms as the training forward, nothing kept for a backward
// What one run of the forward routine (encoder_forward) reads and writes beside the caller's tensors: the embedding LayerNorm's
// buffers, the bf16 parameter copy, every layer's LayerActs. Training hands it the workspace's per-layer blocks; the
// forward-only pass two sets that alternate by layer, with nulls where nothing is kept.
struct FwdBufs {
  float *emb_pre, *emb_mean, *emb_rstd, *x0;
  void *x0b, *wbf;
  float* ln_tmp;  // forward-only, LayerNorm as a launch of its own: the [T][H] pre-LayerNorm sum between the two launches
  LayerActs set[2];
  const Workspace* ws;  // training: layer i's block is ws->layer(i); null: set[i & 1]
  bool keep;            // training: pre / mean / rstd, u / gelu(u) / gelu'(u) are stored for the backward
  LayerActs layer(int i) const { return ws ? ws->layer(i) : set[i & 1]; }
};
// The forward-only workspace: sized by the rows actually run (plan.T), whatever the layer count -- the embedding LayerNorm's
// output, one qkv / ctx / lse, two sets of LayerNorm outputs, the [T][I] gelu output and the [T][H] pre-LayerNorm sum only
// where the plan runs those as launches of their own, the bf16 parameter copy. base may be null (size query).
struct InferSpace { FwdBufs b; size_t total; };
InferSpace carve_infer(const xfmr_encoder_cfg* c, const EncPlan& plan, unsigned char* base) {
  const size_t T = (size_t)plan.T, TH = T * c->hidden, TI = T * c->inter, es = plan.mix ? 2 : 4;
  const size_t xb = plan.mix ? TH * 2 : 0;
  Bump k{base, 0};
  InferSpace s{};
  FwdBufs& b = s.b;
  b.x0 = k.f32(TH); b.x0b = k.bytes(xb);
  LayerActs shared{};
  shared.qkv = k.bytes(3 * TH * es); shared.ctx = k.bytes(TH * es);
  shared.lse = k.f32((size_t)c->batch * c->heads * c->seq_len);
  shared.g = k.bytes(plan.fuse_ffn ? 0 : TI * es);
  b.ln_tmp = k.f32(plan.fuse_ln ? 0 : TH);
  for (LayerActs& l : b.set) {
    l = shared;
    l.x1 = k.f32(TH); l.x1b = k.bytes(xb); l.x2 = k.f32(TH); l.x2b = k.bytes(xb);
  }
  b.wbf = k.bytes(plan.mix ? (size_t)xfmr_param_count(c) * 2 : 0);
  s.total = k.o;
  return s;
}
// What the call asks of its caller: the carve, and in the padded layout never less than a smaller batch or a shorter seq_len
// would need -- a workspace sized for the largest batch serves every smaller one. The carve alone steps DOWN where a form
// sets in (the fused FFN needs no [T][I] buffer, the LayerNorm-fused GEMMs no [T][H] one); the floor is the carve of the last
// token count below each such step, and is overtaken within a fifth more tokens. (Packed rows: the forms follow batch x
// seq_len, the size the rows run -- no step, no floor.)
size_t infer_bytes(const xfmr_encoder_cfg* c, const EncPlan& plan, size_t carved) {
  size_t need = carved;
  if (c->seq_offsets) return need;
  for (const int64_t tokens : {kFfnFusedTokens - 1, ln_fused_min_tokens() - 1}) {
    if (tokens < 1 || tokens >= plan.Tplan || tokens > 0x7fffffff) continue;
    xfmr_encoder_cfg below = *c;
    below.batch = 1; below.seq_len = below.max_pos = (int32_t)tokens;
    const size_t n = carve_infer(&below, make_plan(&below), nullptr).total;
    if (n > need) need = n;
  }
  return need;
}
int check_infer_cfg(const xfmr_encoder_cfg* c) {
  if (const int rc = check_cfg(c)) return rc;
  return (c->hidden_dropout != 0.f || c->attn_dropout != 0.f) ? XFMR_EINVAL : XFMR_OK;  // this entry is eval
}

enum { SITE_EMB = 0 };
inline uint32_t site_attn(int i) { return 1 + 4 * (uint32_t)i; }
inline uint32_t site_out(int i) { return 2 + 4 * (uint32_t)i; }
inline uint32_t site_ffn(int i) { return 3 + 4 * (uint32_t)i; }

#define XF_TRY(expr)            \
  do {                          \
    int _rc = (expr);           \
    if (_rc != XFMR_OK) return _rc; \
  } while (0)

}  // namespace

extern "C" {

const char* xfmr_strerror(int code) {
  switch (code) {
    case XFMR_OK: return "ok";
    case XFMR_EINVAL: return "invalid argument";
    case XFMR_EUNSUPPORTED:
      return "shape not supported by the gfx950 kernels (head size must be 32 or 64; the fused loss takes any d_model that is a "
             "multiple of 32 up to 1024 in the bf16 policy and up to 512 in fp32; attention takes any L in the padded layout, "
             "packed rows need the bf16 policy, head size 32 and causal, at any length: the one-workgroup forms run at L <= 512 "
             "and the key-streaming forms beyond)";
    case XFMR_EWORKSPACE: return "workspace too small";
    case XFMR_EHIP: return "HIP launch failed";
    case XFMR_EALIGN: return "pointer or leading dimension not 16-byte aligned";
    case XFMR_ECOMM: return "RCCL not loadable or an RCCL call failed (xfmr_comm_last_error)";
    default: return "unknown error";
  }
}
int xfmr_abi_version(void) { return XFMR_ABI_VERSION; }

int64_t xfmr_param_count(const xfmr_encoder_cfg* cfg) {
  if (!cfg || cfg->layers <= 0) return XFMR_EINVAL;
  ParamLayout pl;
  layer_base(cfg, 0, &pl);
  return pl.total;
}

int32_t xfmr_param_offsets(const xfmr_encoder_cfg* cfg, int64_t* offsets, int32_t capacity) {
  if (!cfg || !offsets) return XFMR_EINVAL;
  const int32_t n = 4 + 16 * cfg->layers;
  if (capacity < n) return XFMR_EINVAL;
  ParamLayout pl;
  layer_base(cfg, 0, &pl);
  const int64_t H = cfg->hidden;
  int k = 0;
  offsets[k++] = pl.pos; offsets[k++] = pl.type; offsets[k++] = pl.eg; offsets[k++] = pl.eb;
  for (int i = 0; i < cfg->layers; ++i) {
    const LayerParams p = layer_params(cfg, i);
    offsets[k++] = p.wqkv; offsets[k++] = p.wqkv + H * H; offsets[k++] = p.wqkv + 2 * H * H;
    offsets[k++] = p.bqkv; offsets[k++] = p.bqkv + H; offsets[k++] = p.bqkv + 2 * H;
    offsets[k++] = p.wo; offsets[k++] = p.bo; offsets[k++] = p.ln1g; offsets[k++] = p.ln1b;
    offsets[k++] = p.w1; offsets[k++] = p.b1; offsets[k++] = p.w2; offsets[k++] = p.b2;
    offsets[k++] = p.ln2g; offsets[k++] = p.ln2b;
  }
  return n;
}

size_t xfmr_encoder_workspace_bytes(const xfmr_encoder_cfg* cfg) {
  if (check_cfg(cfg)) return 0;
  return carve(cfg, make_plan(cfg), nullptr).a.total;
}

// The caller-owned side stream of xfmr_encoder_bwd's weight-gradient GEMMs + the events of its fork / join.
struct XfContext {
  hipStream_t side;
  hipEvent_t ev_in, ev_done;
};
int xfmr_context_create(void** context) {
  if (!context) return XFMR_EINVAL;
  XfContext* c = new (std::nothrow) XfContext{};
  if (!c) return XFMR_EHIP;
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
      hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, lo) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming) != hipSuccess) {
    xfmr_context_destroy(c);
    return XFMR_EHIP;
  }
  *context = c;
  return XFMR_OK;
}
int xfmr_context_destroy(void* context) {
  if (!context) return XFMR_EINVAL;
  XfContext* c = (XfContext*)context;
  if (c->ev_in) (void)hipEventDestroy(c->ev_in);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->side) (void)hipStreamDestroy(c->side);
  delete c;
  return XFMR_OK;
}

}  // extern "C"

namespace {

// The residual operand of a "Linear + dropout + residual + LayerNorm": the output of an earlier LayerNorm, either loaded
// (x: the stored fp32 copy) or, under EncPlan::rederive, re-derived from what that LayerNorm stored for its backward (re).
struct Residual { const float* x; XfLnResidual re; };

// The forward pass, written once: xfmr_encoder_fwd and xfmr_encoder_infer differ in the buffers they hand it (FwdBufs) and in
// nothing else. With bufs.keep off (forward-only) every product goes through the same kernel form, in the same order, on an
// instantiation that stores nothing a backward would read; the residual is always the stored fp32 LayerNorm output.
int encoder_forward(const xfmr_encoder_cfg* cfg, const EncPlan& plan, const FwdBufs& a, const float* params,
                    const int64_t* item_idx, const float* table, int64_t n_rows, float* tok, uint8_t* key_mask, hipStream_t st) {
  const int B = cfg->batch, L = cfg->seq_len, H = cfg->hidden, I = cfg->inter, A = cfg->heads;
  const int32_t* const offs = cfg->seq_offsets;
  const int64_t T = plan.T;
  const int prec = cfg->precision;
  const bool mix = plan.mix, keep = a.keep, rederive = plan.rederive && keep;
  const float hdrop = cfg->hidden_dropout, eps = cfg->ln_eps;
  const XfSeed sd(cfg->seed, keep ? cfg->step_device : nullptr);
  ParamLayout pl;
  layer_base(cfg, 0, &pl);
  float* const x0 = rederive ? nullptr : a.x0;
  if (offs) {
    XF_TRY(xf_embed_ln_fwd_packed_ex(item_idx, table, n_rows, params + pl.pos, params + pl.type, params + pl.eg,
                                     params + pl.eb, x0, mix ? a.x0b : nullptr, a.emb_pre, a.emb_mean, a.emb_rstd, key_mask,
                                     T, cfg->row_pos, H, eps, hdrop, sd, SITE_EMB, st));
  } else {
    XF_TRY(xf_embed_ln_fwd_ex(item_idx, table, n_rows, params + pl.pos, params + pl.type, params + pl.eg,
                              params + pl.eb, x0, mix ? a.x0b : nullptr, a.emb_pre, a.emb_mean, a.emb_rstd, key_mask, B,
                              L, H, eps, hdrop, sd, SITE_EMB, st));
  }
  if (cfg->embed_event && hipEventRecord((hipEvent_t)cfg->embed_event, st) != hipSuccess) return XFMR_EHIP;  // key_mask is written
  // the layer input as a residual: the embedding LayerNorm's dropped-out output, then each layer's LayerNorm 2
  Residual x{x0, {a.emb_pre, a.emb_mean, a.emb_rstd, params + pl.eg, params + pl.eb, hdrop, SITE_EMB}};
  const void* xg = mix ? a.x0b : (const void*)a.x0;  // the same activations as the GEMM operand
  if (mix) {
    const int64_t n4 = pl.total / 4;  // (every tensor size is a multiple of 4: H, I multiples of 32)
    hipLaunchKernelGGL(params_to_bf16_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, params,
                       (__bf16*)a.wbf, n4);
    XF_LAUNCH_CHECK();
  }
  const uint32_t sA = mix ? XF_S16_A : 0, sB = mix ? XF_S16_B : 0, sC = mix ? XF_S16_C : 0;
  auto W = [&](int64_t off) -> const float* {  // weight operand: the bf16 copy under mixed storage
    return mix ? reinterpret_cast<const float*>((const __bf16*)a.wbf + off) : params + off;
  };
  // pre <- dropout(in W^T + bias) + res; y / y16 / mean / rstd <- LayerNorm(pre): in the GEMM epilogue with the residual
  // re-derived or loaded (the tile spans whole rows), or as two launches. Forward-only: pre / mean / rstd are null -- the
  // epilogue form that does not store them, or the two launches with the sum in a.ln_tmp and no statistics out.
  auto linear_ln = [&](const void* in, int64_t w, int64_t bias, int K, const Residual& res, uint32_t site, int64_t gamma,
                       int64_t beta, float* pre, float* y, void* y16, float* mean, float* rstd) -> int {
    if (rederive)
      return xf_linear_ln_fwd_re(in, W(w), params + bias, pre, T, H, K, &res.re, hdrop, sd, site, params + gamma,
                                 params + beta, eps, y, y16, mean, rstd, prec, sA | sB, st);
    if (plan.fuse_ln && !keep)
      return xf_linear_ln_fwd_infer(in, W(w), params + bias, T, H, K, res.x, params + gamma, params + beta, eps, y, y16, prec,
                                    sA | sB, st);
    if (plan.fuse_ln)
      return xf_linear_ln_fwd_ex(in, W(w), params + bias, pre, T, H, K, res.x, hdrop, sd, site, params + gamma,
                                 params + beta, eps, y, y16, mean, rstd, prec, sA | sB, st);
    float* const sum = keep ? pre : a.ln_tmp;
    XF_TRY(xf_linear_fwd_ex(in, W(w), params + bias, sum, T, H, K, XFMR_EPI_BIAS_DROP_RES, res.x, nullptr, hdrop, sd, site,
                            prec, sA | sB, st));
    return xf_layernorm_fwd_ex(sum, params + gamma, params + beta, y, y16, mean, rstd, T, H, eps, st);
  };
  for (int i = 0; i < cfg->layers; ++i) {
    const LayerActs l = a.layer(i);
    const LayerParams p = layer_params(cfg, i);
    const bool last = i == cfg->layers - 1;
    // the fp32 LayerNorm outputs (null: not stored) and their bf16 copies (null: fp32 storage / nobody reads it)
    float* const x1 = rederive ? nullptr : l.x1;
    float* const out = last ? tok : (rederive ? nullptr : l.x2);
    void* const x1b = mix ? l.x1b : nullptr;
    void* const x2b = (mix && !last) ? l.x2b : nullptr;
    XF_TRY(xf_linear_fwd_ex(xg, W(p.wqkv), params + p.bqkv, l.qkv, T, 3 * H, H, XFMR_EPI_BIAS, nullptr, nullptr,
                            0.f, 0, 0, prec, sC | sA | sB, st));
    XF_TRY(prof(cfg, XFMR_PROF_ATTN_FWD, i, 0, st));
    XF_TRY(xf_attn_fwd_ex(l.qkv, key_mask, l.ctx, l.lse, B, L, A, H, cfg->attn_dropout, sd, site_attn(i), prec,
                          mix, plan.causal, st, offs));
    XF_TRY(prof(cfg, XFMR_PROF_ATTN_FWD, i, 1, st));
    XF_TRY(linear_ln(l.ctx, p.wo, p.bo, H, x, site_out(i), p.ln1g, p.ln1b, l.pre1, x1, x1b, l.mean1, l.rstd1));
    XF_TRY(prof(cfg, XFMR_PROF_FFN_FWD, i, 0, st));
    const Residual r1{x1, {l.pre1, l.mean1, l.rstd1, params + p.ln1g, params + p.ln1b, 0.f, 0}};
    if (plan.fuse_ffn) {  // FFN1 -> GELU -> FFN2 -> dropout + residual + LayerNorm in one kernel; f1 <- the PRE-activation, g <- gelu
      XF_TRY(rederive ? xf_ffn_fwd_fused_re(l.x1b, W(p.w1), params + p.b1, W(p.w2), params + p.b2, l.f1, l.g, l.pre2, T, H,
                                            I, &r1.re, hdrop, sd, site_ffn(i), params + p.ln2g, params + p.ln2b, eps, out,
                                            x2b, l.mean2, l.rstd2, st)
             : !keep  ? xf_ffn_fwd_fused_infer(l.x1b, W(p.w1), params + p.b1, W(p.w2), params + p.b2, T, H, I, r1.x,
                                               params + p.ln2g, params + p.ln2b, eps, out, x2b, st)
                      : xf_ffn_fwd_fused_ex(l.x1b, W(p.w1), params + p.b1, W(p.w2), params + p.b2, l.f1, l.g, l.pre2, T, H,
                                            I, r1.x, hdrop, sd, site_ffn(i), params + p.ln2g, params + p.ln2b, eps, out,
                                            x2b, l.mean2, l.rstd2, st));
    } else {
      const void* const x1g = mix ? (const void*)l.x1b : (const void*)l.x1;
      if (keep)
        XF_TRY(xf_linear_fwd_ex(x1g, W(p.w1), params + p.b1, l.g, T, I, H, XFMR_EPI_BIAS_GELU, nullptr, l.f1, 0.f, 0, 0, prec,
                                sC | sA | sB | XF_AUX_GELU_GRAD, st));  // f1 <- gelu'(pre)
      else
        XF_TRY(xf_linear_gelu_fwd_infer(x1g, W(p.w1), params + p.b1, l.g, T, I, H, prec, sC | sA | sB, st));
      XF_TRY(linear_ln(l.g, p.w2, p.b2, I, r1, site_ffn(i), p.ln2g, p.ln2b, l.pre2, out, x2b, l.mean2, l.rstd2));
    }
    XF_TRY(prof(cfg, XFMR_PROF_FFN_FWD, i, 1, st));
    // what the next layer takes as its input: the residual, and the same activations as the GEMM operand
    x = Residual{out, {l.pre2, l.mean2, l.rstd2, params + p.ln2g, params + p.ln2b, 0.f, 0}};
    xg = mix ? (const void*)l.x2b : (const void*)out;
  }
  return XFMR_OK;
}

}  // namespace

extern "C" {

int xfmr_encoder_fwd(const xfmr_encoder_cfg* cfg, const float* params, const int64_t* item_idx,
                     const float* table, int64_t n_rows, float* tok, uint8_t* key_mask, void* acts,
                     size_t acts_bytes, void* stream) {
  XF_TRY(check_cfg(cfg));
  if (!params || !item_idx || !table || !tok || !key_mask || !acts) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(acts) || !xf_aligned16(tok) || !xf_aligned16(table)) return XFMR_EALIGN;
  const EncPlan plan = make_plan(cfg);
  const Workspace ws = carve(cfg, plan, (unsigned char*)acts);
  const Acts& a = ws.a;
  if (acts_bytes < a.total) return XFMR_EWORKSPACE;
  FwdBufs b{};
  b.emb_pre = a.emb_pre; b.emb_mean = a.emb_mean; b.emb_rstd = a.emb_rstd; b.x0 = a.x0; b.x0b = a.x0b; b.wbf = a.wbf;
  b.ws = &ws; b.keep = true;
  return encoder_forward(cfg, plan, b, params, item_idx, table, n_rows, tok, key_mask, (hipStream_t)stream);
}

size_t xfmr_encoder_infer_workspace_bytes(const xfmr_encoder_cfg* cfg) {
  if (check_cfg(cfg)) return 0;
  const EncPlan plan = make_plan(cfg);
  return infer_bytes(cfg, plan, carve_infer(cfg, plan, nullptr).total);
}

int xfmr_encoder_infer(const xfmr_encoder_cfg* cfg, const float* params, const int64_t* item_idx, const float* table,
                       int64_t n_rows, float* tok, uint8_t* key_mask, void* workspace, size_t workspace_bytes, void* stream) {
  XF_TRY(check_infer_cfg(cfg));
  if (!params || !item_idx || !table || !tok || !key_mask || !workspace) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(workspace) || !xf_aligned16(tok) || !xf_aligned16(table)) return XFMR_EALIGN;
  const EncPlan plan = make_plan(cfg);
  const InferSpace s = carve_infer(cfg, plan, (unsigned char*)workspace);
  if (workspace_bytes < infer_bytes(cfg, plan, s.total)) return XFMR_EWORKSPACE;
  return encoder_forward(cfg, plan, s.b, params, item_idx, table, n_rows, tok, key_mask, (hipStream_t)stream);
}

int xfmr_encoder_bwd(const xfmr_encoder_cfg* cfg, const float* params, float* grads, float* d_tok,
                     const uint8_t* key_mask, void* acts, size_t acts_bytes, void* stream) {
  XF_TRY(check_cfg(cfg));
  if (!params || !grads || !d_tok || !key_mask || !acts) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(grads) || !xf_aligned16(acts) || !xf_aligned16(d_tok)) return XFMR_EALIGN;
  const EncPlan plan = make_plan(cfg);
  const Workspace ws = carve(cfg, plan, (unsigned char*)acts);
  const Acts& a = ws.a;
  if (acts_bytes < a.total) return XFMR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const XfSeed sd(cfg->seed, cfg->step_device);
  const int B = cfg->batch, L = cfg->seq_len, H = cfg->hidden, I = cfg->inter, A = cfg->heads;
  const int32_t* const offs = cfg->seq_offsets;
  const int64_t T = plan.T;
  const int prec = cfg->precision;
  const bool mix = plan.mix, dw_side = plan.dw_side, lin_copy = plan.lin_copy;
  const uint32_t sA = mix ? XF_S16_A : 0, sC = mix ? XF_S16_C : 0, sP = mix ? XF_S16_P : 0,
                 sAB = mix ? (XF_S16_A | XF_S16_B) : 0, sB = mix ? XF_S16_B : 0;
  auto W = [&](int64_t off) -> const float* {  // weight operand: the bf16 copy the forward pass made
    return mix ? reinterpret_cast<const float*>((const __bf16*)a.wbf + off) : params + off;
  };
  ParamLayout pl;
  layer_base(cfg, 0, &pl);
  const XfDropout off = xf_make_dropout(0.f, 0, 0);
  float* dX = d_tok;  // gradient w.r.t. the current layer's output
  // Two reduction lists when the caller wants the UPPER half of the flat gradient early (cfg->grads_half_event): the
  // tensors of layers >= layers / 2 are the contiguous tail of the buffer (xfmr_param_half_offset); their slabs and
  // records are reduced as soon as layer layers / 2 has enqueued its last producer, the event is recorded behind that
  // launch, and the data-parallel exchange of that half runs underneath the lower layers' backward.
  XfReduceSeg segs[12 * 64 + 2], segs_hi[12 * 64 + 2];
  int nseg = 0, nseg_hi = 0;
  if (cfg->layers > 64) return XFMR_EUNSUPPORTED;
  const float* const hi_begin = plan.half_layer >= 0 ? grads + layer_params(cfg, plan.half_layer).wqkv : nullptr;
  auto seg = [&](const float* src, float* dst, int rows, int64_t cols, int64_t ld) {
    if (hi_begin && dst >= hi_begin) segs_hi[nseg_hi++] = XfReduceSeg{src, dst, rows, (int)cols, (int)ld, 0};
    else segs[nseg++] = XfReduceSeg{src, dst, rows, (int)cols, (int)ld, 0};
  };
  // one LayerNorm backward's partial records [blocks][3][H]: d gamma, d beta, d bias of the Linear in front (< 0: none)
  auto ln_segs = [&](const float* rec, int blocks, int64_t gamma, int64_t beta, int64_t bias) {
    seg(rec, grads + gamma, blocks, H, 3 * H);
    seg(rec + H, grads + beta, blocks, H, 3 * H);
    if (bias >= 0) seg(rec + 2 * H, grads + bias, blocks, H, 3 * H);
  };
  // LayerNorm backward in the epilogue of the dX GEMM that produces its input gradient (whole-row 64 x 128 tiles: same
  // conditions as the forward fusion): LN1 with the FFN1 dX GEMM of its layer, LN2 of layer i-1 with the QKV dX GEMM of
  // layer i. The top layer's LN2 and the embedding LayerNorm keep their own launches.
  const bool fuse_lnb = plan.fuse_ln;
  // The weight-gradient GEMMs (16 of the backward's launches, 0.49 ms at batch 512) run on the LOW-PRIORITY side stream of
  // the caller's xfmr_context: the dX -> LayerNorm -> attention chain keeps the CUs it wants, and the dW workgroups fill
  // what its 64-row-tile kernels leave idle in their last rounds (section 4 of DESIGN.md). Same priority was measured in
  // round 1 and gained nothing (each side slowed by what the overlap gave). Dependencies: a dW GEMM starts after an event
  // recorded behind the producers of its operands; the gradient buffers the chain used to reuse layer after layer (dLin in
  // both roles, dI, dQKV) exist once PER LAYER in this mode, so nothing a dW GEMM reads is rewritten before the chain
  // joins the side stream in front of the reduction launch (with two sets alternating by layer parity and
  // write-after-read events the chain kept stalling on the lagging side stream: 0.4 % instead of 2 %).
  // No context, or XFMR_ENC_DW_INLINE: everything on `st`.
  XfContext* const ctx = (XfContext*)cfg->context;
  hipStream_t const side = dw_side ? ctx->side : nullptr;
  hipEvent_t const ev_in = dw_side ? ctx->ev_in : nullptr, ev_done = dw_side ? ctx->ev_done : nullptr;
  bool side_used = false;
  int side_rc = XFMR_OK;
  auto dw_stream = [&]() -> hipStream_t {  // everything enqueued on `st` so far is visible to the side stream
    if (!dw_side) return st;
    if (hipEventRecord(ev_in, st) != hipSuccess || hipStreamWaitEvent(side, ev_in, 0) != hipSuccess) side_rc = XFMR_EHIP;
    side_used = true;
    return side;
  };
  // In line the four gradient buffers of a layer are four different shared buffers, all live to the end of the layer (the
  // next writer of any of them is the next layer): what the grouped weight-gradient launch needs.
  auto grad_bufs = [&](int i) { return dw_side ? ws.grads(i) : GradBufs{a.dLin, a.dLin2, a.dI, a.dQKV}; };
  bool ln2_done = false;  // layer i's LN2 backward already ran inside layer i+1's QKV dX GEMM
  bool emb_ln_done = false;  // ... and the embedding LayerNorm's inside layer 0's
  // (a lambda so that a failing launch still reaches the join below: the side stream's GEMMs read the caller's buffers)
  const int chain_rc = [&]() -> int {
  for (int i = cfg->layers - 1; i >= 0; --i) {
    const LayerActs l = ws.layer(i);
    const RedBufs r = ws.red(i);
    const LayerParams p = layer_params(cfg, i);
    const LayerActs prev = i > 0 ? ws.layer(i - 1) : LayerActs{};
    // dLinF: gradient of the FFN2 Linear's output (dropout-scaled d(pre2)); dLinO: of the out-proj Linear's output
    const GradBufs gb = grad_bufs(i);
    int blocks = 0;
    // LayerNorm 2 -> dA = d(pre2); d_lin = gradient of the FFN output Linear (dropout-scaled copy of it)
    if (!ln2_done) {
      XF_TRY(xf_layernorm_bwd_impl(dX, l.pre2, l.mean2, l.rstd2, params + p.ln2g, a.dA, lin_copy ? gb.dLinF : nullptr,
                                   mix, nullptr, nullptr, nullptr, T, H, off,
                                   xf_make_dropout(cfg->hidden_dropout, sd, site_ffn(i)), r.ln2, st, &blocks));
      ln_segs(r.ln2, blocks, p.ln2g, p.ln2b, p.b2);
    }
    const void* const dlin_ffn = lin_copy ? gb.dLinF : (const void*)a.dA;
    const void* const dlin_out = lin_copy ? gb.dLinO : (const void*)dX;
    // The layer's four weight-gradient GEMMs (operand pair, slabs, bias partial rows, where the gradient goes): FFN2, FFN1,
    // out-proj, QKV. Grouped they go out together once the last operand (dQKV) exists; otherwise each one as soon as its
    // operands do, on dw_stream().
    int splits[4] = {0, 0, 0, 0};
    const XfDwItem items[4] = {
        {dlin_ffn, l.g, (int32_t)H, (int32_t)I, r.w2, nullptr, &splits[0]},
        {gb.dI, mix ? (const void*)l.x1b : (const void*)l.x1, (int32_t)I, (int32_t)H, r.w1, r.b1, &splits[1]},
        {dlin_out, l.ctx, (int32_t)H, (int32_t)H, r.wo, nullptr, &splits[2]},
        // (the dW operand: the bf16 copy of the layer's input under mixed storage)
        {gb.dQKV, i > 0 ? (mix ? prev.x2b : (const void*)prev.x2) : (mix ? a.x0b : (const void*)a.x0), (int32_t)(3 * H),
         (int32_t)H, r.wqkv, r.bqkv, &splits[3]}};
    const int64_t dw_w[4] = {p.w2, p.w1, p.wo, p.wqkv}, dw_b[4] = {-1, p.b1, -1, p.bqkv};
    auto dw = [&](int k, bool launch) -> int {  // item k's own launch (grouped: the group launch has done it), its segments
      const XfDwItem& it = items[k];
      if (launch) XF_TRY(xf_linear_bwd_dw_deferred(it.dy, it.x, T, it.N, it.K, prec, sAB, it.slabs, it.bias_part, it.splits, dw_stream()));
      seg(it.slabs, grads + dw_w[k], *it.splits, (int64_t)it.N * it.K, (int64_t)it.N * it.K);
      if (it.bias_part) seg(it.bias_part, grads + dw_b[k], *it.splits, it.N, it.N);
      return XFMR_OK;
    };
    if (!plan.group_dw) XF_TRY(dw(0, true));
    XF_TRY(prof(cfg, XFMR_PROF_FFN_BWD, i, 0, st));  // (in the unfused forms: FFN2 dX ... LayerNorm 1 backward on `st`)
    if (plan.fuse_ffn_bwd) {  // FFN2 dX * gelu'(u) -> dI -> FFN1 dX (+= d(pre2)) -> LayerNorm 1 backward in one kernel
      XF_TRY(xf_ffn_bwd_dx_fused_ex(dlin_ffn, W(p.w2), l.f1, W(p.w1), gb.dI, T, H, I, a.dA, l.pre1, l.mean1, l.rstd1,
                                    params + p.ln1g, cfg->hidden_dropout, sd, site_out(i), dX, gb.dLinO, r.ln1,
                                    &blocks, st));
    } else {
      // (after the fused FFN forward f1 holds the pre-activation u, not gelu'(u): the epilogue evaluates gelu'(u))
      XF_TRY(xf_linear_bwd_dx_ex(dlin_ffn, W(p.w2), gb.dI, T, H, I, nullptr, l.f1, prec,
                                 sA | sC | sP | sB | (plan.fuse_ffn ? 0 : XF_AUX_GELU_GRAD), st));
    }
    if (!plan.group_dw) XF_TRY(dw(1, true));  // + b1 partial rows
    if (plan.fuse_ffn_bwd) {  // (done above)
    } else if (fuse_lnb) {  // dX of FFN1 (+= d(pre2)) and LayerNorm 1 backward in one kernel -> dX = d(pre1), dLin
      XF_TRY(xf_linear_bwd_dx_lnbwd_ex(gb.dI, W(p.w1), T, I, H, a.dA, l.pre1, l.mean1, l.rstd1, params + p.ln1g,
                                       cfg->hidden_dropout, sd, site_out(i), dX, gb.dLinO, r.ln1, &blocks, prec,
                                       sA | sB, st));
    } else {
      XF_TRY(xf_linear_bwd_dx_ex(gb.dI, W(p.w1), a.dA, T, I, H, a.dA, nullptr, prec, sA | sB, st));  // += d(pre2)
      // LayerNorm 1 -> dX = d(pre1)
      XF_TRY(xf_layernorm_bwd_impl(a.dA, l.pre1, l.mean1, l.rstd1, params + p.ln1g, dX, lin_copy ? gb.dLinO : nullptr,
                                   mix, nullptr, nullptr, nullptr, T, H, off,
                                   xf_make_dropout(cfg->hidden_dropout, sd, site_out(i)), r.ln1, st, &blocks));
    }
    XF_TRY(prof(cfg, XFMR_PROF_FFN_BWD, i, 1, st));
    ln_segs(r.ln1, blocks, p.ln1g, p.ln1b, p.bo);
    if (!plan.group_dw) XF_TRY(dw(2, true));
    XF_TRY(xf_linear_bwd_dx_ex(dlin_out, W(p.wo), a.dCtx, T, H, H, nullptr, nullptr, prec, sA | sC | sB, st));  // d(ctx)
    XF_TRY(prof(cfg, XFMR_PROF_ATTN_BWD, i, 0, st));
    XF_TRY(xf_attn_bwd_ex(l.qkv, key_mask, l.ctx, l.lse, a.dCtx, gb.dQKV, B, L, A, H, cfg->attn_dropout, sd,
                          site_attn(i), prec, mix, plan.causal, st, offs));
    XF_TRY(prof(cfg, XFMR_PROF_ATTN_BWD, i, 1, st));
    if (plan.group_dw) {
      XF_TRY(prof(cfg, XFMR_PROF_DW, i, 0, st));  // (the in-line form: the layer's four weight-gradient GEMMs are ONE launch)
      XF_TRY(xf_linear_bwd_dw_group(items, 4, T, prec, sAB, st));
      XF_TRY(prof(cfg, XFMR_PROF_DW, i, 1, st));
      for (int k = 0; k < 4; ++k) XF_TRY(dw(k, false));
    } else {
      XF_TRY(dw(3, true));
    }
    ln2_done = false;
    if (fuse_lnb && i > 0) {  // dX of QKV (+= d(pre1)) and layer i-1's LayerNorm 2 backward -> dA = d(pre2), dLin
      const RedBufs rp = ws.red(i - 1);
      const LayerParams pp = layer_params(cfg, i - 1);
      XF_TRY(xf_linear_bwd_dx_lnbwd_ex(gb.dQKV, W(p.wqkv), T, 3 * H, H, dX, prev.pre2, prev.mean2, prev.rstd2,
                                       params + pp.ln2g, cfg->hidden_dropout, sd, site_ffn(i - 1), a.dA,
                                       grad_bufs(i - 1).dLinF, rp.ln2, &blocks, prec, sA | sB, st));
      ln_segs(rp.ln2, blocks, pp.ln2g, pp.ln2b, pp.b2);
      ln2_done = true;
    } else if (fuse_lnb) {  // layer 0: dX of QKV (+= d(pre1)) and the EMBEDDING LayerNorm backward -> dA
      XF_TRY(xf_linear_bwd_dx_lnbwd_ex(gb.dQKV, W(p.wqkv), T, 3 * H, H, dX, a.emb_pre, a.emb_mean, a.emb_rstd,
                                       params + pl.eg, 0.f, sd, 0, a.dA, nullptr, a.emb_ln, &blocks, prec,
                                       sA | sB, st, cfg->hidden_dropout, SITE_EMB));
      ln_segs(a.emb_ln, blocks, pl.eg, pl.eb, -1);
      emb_ln_done = true;
    } else {
      XF_TRY(xf_linear_bwd_dx_ex(gb.dQKV, W(p.wqkv), dX, T, 3 * H, H, dX, nullptr, prec, sA | sB, st));  // += d(pre1)
    }
    if (i == plan.half_layer) {  // every producer of the upper half's slabs / records is enqueued: finish that half now
      hipStream_t rs = dw_stream();  // (the side stream when the dW GEMMs run there: the chain itself does not wait)
      XF_TRY(xf_multi_rowsum(segs_hi, nseg_hi, rs));
      if (cfg->grads_half_event && hipEventRecord((hipEvent_t)cfg->grads_half_event, rs) != hipSuccess) return XFMR_EHIP;
    }
  }
  if (!emb_ln_done) {
    int blocks = 0;
    XF_TRY(xf_layernorm_bwd_impl(dX, a.emb_pre, a.emb_mean, a.emb_rstd, params + pl.eg, a.dA, nullptr, false, nullptr,
                                 nullptr, nullptr, T, H, xf_make_dropout(cfg->hidden_dropout, sd, SITE_EMB), off,
                                 a.emb_ln, st, &blocks));
    ln_segs(a.emb_ln, blocks, pl.eg, pl.eb, -1);
  }
  // (Measured and not kept: the weight-gradient GEMMs on a side stream beside the dX -> LayerNorm -> attention chain.
  // The kernels do overlap, and each slows down by what the overlap would have gained: 1.910 vs 1.904 ms/step.)
  // (Measured and not kept: reducing each layer's slabs and records on the side stream as soon as they are enqueued, so that
  // only layer 0's are left for the end: 3.41 vs 3.34 ms/step -- the low-priority reductions slow the chain's tail.)
  // the position / type embedding gradients need only the chain's last output: in front of the join, underneath whatever
  // the side stream still has to do
  if (offs) XF_TRY(xf_embed_param_grads_packed(a.dA, grads + pl.pos, grads + pl.type, offs, B, L, H, cfg->max_pos, st));
  else XF_TRY(xfmr_embed_param_grads(a.dA, grads + pl.pos, grads + pl.type, B, L, H, cfg->max_pos, stream));
  return XFMR_OK;
  }();
  if (side_used) {  // the chain joins the side stream: the reduction launch reads every slab
    if (hipEventRecord(ev_done, side) != hipSuccess || hipStreamWaitEvent(st, ev_done, 0) != hipSuccess) side_rc = XFMR_EHIP;
  }
  if (chain_rc != XFMR_OK) return chain_rc;
  if (side_rc != XFMR_OK) return side_rc;
  XF_TRY(prof(cfg, XFMR_PROF_REDUCE, cfg->profile_layer, 0, st));
  XF_TRY(xf_multi_rowsum(segs, nseg, st));  // every weight / bias / LayerNorm gradient of the encoder, one launch
  XF_TRY(prof(cfg, XFMR_PROF_REDUCE, cfg->profile_layer, 1, st));
  if (cfg->grads_half_event && plan.half_layer < 0 &&  // (a one-layer encoder has no upper half: the event marks the whole buffer)
      hipEventRecord((hipEvent_t)cfg->grads_half_event, st) != hipSuccess)
    return XFMR_EHIP;
  return XFMR_OK;
}

// (internal.h) the plan as integers, for the host test of its rules; dereferences nothing behind the cfg's pointers
int xf_encoder_plan(const xfmr_encoder_cfg* cfg, int32_t out[16]) {
  XF_TRY(check_cfg(cfg));
  if (!out) return XFMR_EINVAL;
  const EncPlan p = make_plan(cfg);
  const int32_t v[16] = {(int32_t)p.Tplan, (int32_t)p.T, p.mix, p.causal, p.fuse_ln, p.fuse_ffn, p.rederive,
                         p.fuse_ffn_bwd, p.dw_buffers_per_layer, p.dw_side, p.group_dw, p.lin_copy, p.half_layer};
  memcpy(out, v, sizeof(v));
  return XFMR_OK;
}

int64_t xfmr_param_half_offset(const xfmr_encoder_cfg* cfg) {
  if (!cfg || cfg->layers <= 0) return XFMR_EINVAL;
  if (cfg->layers < 2) return 0;
  return layer_params(cfg, cfg->layers / 2).wqkv;
}

}  // extern "C"
