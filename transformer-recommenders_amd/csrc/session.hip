// The session encoder (include/xfmr_session.h): per-session K / V panels in one caller-owned state buffer, and the pass that
// appends new tokens to them -- the forward-only Linear / LayerNorm forms of xfmr_encoder_infer on the new rows only, with
// two kernels of its own per layer in place of the whole-sequence attention: APPEND (store the rows' K, V and mask bytes at
// (slot, layer, head, pos)) and ATTEND (every (new row, head) against its slot's cached keys 0 .. pos).
//
// The attend kernel is the hot path: at 1024 sessions of 200 events it reads every session's panels once per layer and does
// two flops per byte -- bound by the read. One WAVE per (row, head) pair, K and V straight into registers (no LDS: nothing is
// shared between pairs, and a pair's keys are read once). A key row is head_size elements = 64 ... 256 bytes; each lane
// reads 16 of them, so a key takes LPK = 4, 8 or 16 lanes and one wave load covers 64 / LPK consecutive keys = 1 KiB of
// contiguous panel. The dot product is finished by xor-shuffles inside the LPK lanes; every group of LPK lanes keeps ITS OWN
// running (max, sum, accumulator) over the keys it sees, so the key loop has no exchange between groups at all, and the
// 64 / LPK partial softmaxes are merged once behind the loop. Keys are taken kSessChunk at a time: all of a chunk's loads
// are issued before its first use (2 ... 8 loads of K and of V in flight per lane), and the running maximum moves once per
// chunk. Registers do not grow with the session length; keys beyond pos are never read.
#include <math.h>
#include <string.h>

#include "internal.h"
#include "xfmr_session.h"

namespace {

constexpr int kSessChunk = 32;    // keys one wave takes per online-softmax step
constexpr int kSessMaxLayers = 64;

#define XF_TRY(expr)                \
  do {                              \
    int _rc = (expr);               \
    if (_rc != XFMR_OK) return _rc; \
  } while (0)

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Bump {
  unsigned char* base;
  size_t o;
  void* bytes(size_t n) { void* p = base ? base + o : nullptr; o += up256(n); return p; }
  float* f32(size_t n) { return reinterpret_cast<float*>(bytes(n * sizeof(float))); }
};

// What a cfg means here: checked once, read by every entry.
struct SessShape {
  int H, A, I, layers, hs, max_len;
  bool kv16;  // K / V element type: bf16 under XFMR_PREC_BF16
  bool mix;   // bf16 activation storage (qkv, ctx, gelu output, LayerNorm copies, the parameter copy): EncPlan::mix
};
int session_shape(const xfmr_encoder_cfg* c, SessShape* s) {
  if (!c) return XFMR_EINVAL;
  if (c->seq_offsets || c->row_pos || c->packed_rows) return XFMR_EINVAL;  // this entry has its own row arrays
  int32_t plan[16];
  XF_TRY(xf_encoder_plan(c, plan));  // check_cfg's code (sizes, head size, precision, flag bits)
  if (c->flags & XFMR_ENC_BIDIRECTIONAL) return XFMR_EUNSUPPORTED;  // an append changes every earlier row there
  if (c->hidden_dropout != 0.f || c->attn_dropout != 0.f) return XFMR_EINVAL;
  if (c->layers > kSessMaxLayers) return XFMR_EUNSUPPORTED;
  s->H = c->hidden; s->A = c->heads; s->I = c->inter; s->layers = c->layers; s->hs = c->hidden / c->heads;
  s->max_len = c->max_pos;
  s->kv16 = c->precision == XFMR_PREC_BF16;
  s->mix = plan[2] != 0;
  return XFMR_OK;
}

// The state buffer. Panel (slot, layer, head) = [K: max_len x hs | V: max_len x hs] elements at
// ((slot * layers + layer) * heads + head) * 2 * max_len * hs.
struct SessState {
  void* kv; uint8_t* mask; float* tok; void* wbf;
  size_t mask_bytes, total;
};
SessState carve_state(const xfmr_encoder_cfg* c, const SessShape& s, int32_t n_slots, unsigned char* base) {
  Bump k{base, 0};
  SessState st{};
  const size_t rows = (size_t)n_slots * s.max_len;
  st.kv = k.bytes(rows * s.layers * 2 * s.H * (s.kv16 ? 2 : 4));
  st.mask_bytes = (rows + 3) & ~(size_t)3;
  st.mask = (uint8_t*)k.bytes(st.mask_bytes);
  st.tok = k.f32(rows * s.H);
  st.wbf = k.bytes(s.mix ? (size_t)xfmr_param_count(c) * 2 : 0);
  st.total = k.o;
  return st;
}
// The scratch of one append call of up to R rows.
struct SessWork {
  float *x, *x1, *sum;
  void *xb, *x1b, *qkv, *ctx, *g;
  uint8_t* km;
  int32_t* pos_safe;
  size_t total;
};
SessWork carve_work(const SessShape& s, int64_t R, unsigned char* base) {
  const size_t RH = (size_t)R * s.H, es = s.mix ? 2 : 4, xb = s.mix ? RH * 2 : 0;
  Bump k{base, 0};
  SessWork w{};
  w.x = k.f32(RH); w.xb = k.bytes(xb); w.x1 = k.f32(RH); w.x1b = k.bytes(xb); w.sum = k.f32(RH);
  w.qkv = k.bytes(3 * RH * es); w.ctx = k.bytes(RH * es); w.g = k.bytes((size_t)R * s.I * es);
  w.km = (uint8_t*)k.bytes((size_t)R);
  w.pos_safe = (int32_t*)k.bytes((size_t)R * 4);
  w.total = k.o;
  return w;
}

__global__ __launch_bounds__(256) void session_params_bf16_kernel(const float* src, __bf16* dst, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) xf_st4<true>(dst, 4 * i, *reinterpret_cast<const float4*>(src + 4 * i));
}

// A row the caller got wrong (slot or position out of range) stores nothing anywhere and reads position row 0.
__device__ __forceinline__ bool sess_row_ok(int slot, int pos, int n_slots, int max_len) {
  return slot >= 0 && slot < n_slots && pos >= 0 && pos < max_len;
}
__global__ __launch_bounds__(256) void session_pos_kernel(const int32_t* row_slot, const int32_t* row_pos, int32_t* pos_safe,
                                                          int64_t n_rows, int n_slots, int max_len) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n_rows) pos_safe[r] = sess_row_ok(row_slot[r], row_pos[r], n_slots, max_len) ? row_pos[r] : 0;
}

struct SessRows {
  const int32_t* slot; const int32_t* pos;
  int64_t n_rows;
  int n_slots, max_len, H, A, layers, layer;
  void* kv; uint8_t* mask;
};
__device__ __forceinline__ int64_t sess_panel(const SessRows& a, int slot, int head, int hs) {
  return (((int64_t)slot * a.layers + a.layer) * a.A + head) * 2 * a.max_len * hs;
}

// APPEND: K and V of every new row (columns [H, 3H) of its qkv row) into the panels, four elements per thread; the mask byte
// by the row's first thread.
template <int HS, bool KV16, bool SRC16>
__global__ __launch_bounds__(256) void session_append_kernel(SessRows a, const void* qkv, const uint8_t* km) {
  const int quads = a.H / 2;  // 2H / 4 per row
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows * quads) return;
  const int64_t r = i / quads;
  const int c = (int)(i % quads) * 4;  // column of [K | V]
  const int slot = a.slot[r], pos = a.pos[r];
  if (!sess_row_ok(slot, pos, a.n_slots, a.max_len)) return;
  const int which = c / a.H, col = c % a.H, head = col / HS, d = col % HS;
  const float4 v = xf_ld4<SRC16>(qkv, r * 3 * a.H + a.H + c);
  xf_st4<KV16>(a.kv, sess_panel(a, slot, head, HS) + ((int64_t)which * a.max_len + pos) * HS + d, v);
  if (c == 0) a.mask[(int64_t)slot * a.max_len + pos] = km[r];
}

// 16 bytes of a panel row as floats: E = 4 fp32 or 8 bf16
template <bool KV16>
__device__ __forceinline__ void sess_unpack(const uint4& raw, float* f) {
  if (KV16) {
    f[0] = __uint_as_float(raw.x << 16); f[1] = __uint_as_float(raw.x & 0xffff0000u);
    f[2] = __uint_as_float(raw.y << 16); f[3] = __uint_as_float(raw.y & 0xffff0000u);
    f[4] = __uint_as_float(raw.z << 16); f[5] = __uint_as_float(raw.z & 0xffff0000u);
    f[6] = __uint_as_float(raw.w << 16); f[7] = __uint_as_float(raw.w & 0xffff0000u);
  } else {
    f[0] = __uint_as_float(raw.x); f[1] = __uint_as_float(raw.y); f[2] = __uint_as_float(raw.z); f[3] = __uint_as_float(raw.w);
  }
}

// ATTEND: ctx[r, head] = softmax(q . K[0 .. pos] / sqrt(hs)) V over the row's slot, keys with mask byte 0 skipped, ctx = 0 when
// no key is visible. One wave per (row, head); fp32 arithmetic throughout. Q16: qkv and ctx are bf16 (bf16 storage).
template <int HS, bool KV16, bool Q16>
__global__ __launch_bounds__(256) void session_attend_kernel(SessRows a, const void* qkv, void* ctx, float scale_log2e) {
  constexpr int E = KV16 ? 8 : 4;        // elements per lane
  constexpr int LPK = HS / E;            // lanes per key
  constexpr int KPS = 64 / LPK;          // keys per wave load
  constexpr int U = kSessChunk / KPS;    // loads per chunk
  static_assert(U >= 1 && U * KPS == kSessChunk, "the chunk is a whole number of wave loads");
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= a.n_rows * a.A) return;
  const int64_t r = pair / a.A;
  const int head = (int)(pair % a.A);
  const int sub = lane % LPK, grp = lane / LPK;
  const int slot = a.slot[r], pos = a.pos[r];
  const int64_t out = r * a.H + head * HS + sub * E;
  const bool ok = sess_row_ok(slot, pos, a.n_slots, a.max_len);

  float q[E];
  {
    const int64_t qi = r * 3 * a.H + head * HS + sub * E;
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const float4 v = xf_ld4<Q16>(qkv, qi + e);
      q[e] = v.x * scale_log2e; q[e + 1] = v.y * scale_log2e; q[e + 2] = v.z * scale_log2e; q[e + 3] = v.w * scale_log2e;
    }
  }
  float m = -INFINITY, l = 0.f, acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;

  const int nkeys = ok ? pos + 1 : 0;  // (uniform over the wave: the shuffles below run under no divergent condition)
  const int esz = KV16 ? 2 : 4;
  const char* const kbase = (const char*)a.kv + (ok ? sess_panel(a, slot, head, HS) : 0) * esz + sub * 16;
  const char* const vbase = kbase + (int64_t)a.max_len * HS * esz;
  const uint8_t* const mrow = a.mask + (int64_t)(ok ? slot : 0) * a.max_len;
  for (int base = 0; base < nkeys; base += kSessChunk) {
    uint4 kr[U], vr[U];
    bool vis[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPS + grp;
      kr[u] = vr[u] = make_uint4(0, 0, 0, 0);
      vis[u] = false;
      if (key < nkeys) {  // keys beyond pos are never read: a slot's stale rows do not matter
        kr[u] = *reinterpret_cast<const uint4*>(kbase + (int64_t)key * HS * esz);
        vr[u] = *reinterpret_cast<const uint4*>(vbase + (int64_t)key * HS * esz);
        vis[u] = mrow[key] != 0;
      }
    }
    float s[U], cm = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[E], dot = 0.f;
      sess_unpack<KV16>(kr[u], kf);
#pragma unroll
      for (int e = 0; e < E; ++e) dot = __builtin_fmaf(q[e], kf[e], dot);
#pragma unroll
      for (int o = LPK / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      s[u] = vis[u] ? dot : -INFINITY;  // (a select: whatever a masked or unwritten row holds never reaches the sum)
      cm = fmaxf(cm, s[u]);
    }
    const float m_new = fmaxf(m, cm);
    if (m_new > -INFINITY) {
      const float corr = xf_exp2(m - m_new);  // m = -inf: 0
      l *= corr;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] *= corr;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!vis[u]) continue;
        const float p = xf_exp2(s[u] - m_new);
        float vf[E];
        sess_unpack<KV16>(vr[u], vf);
        l += p;
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_fmaf(p, vf[e], acc[e]);
      }
      m = m_new;
    }
  }
  // the 64 / LPK partial softmaxes -> one
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    const float m_o = __shfl_xor(m, o, 64), l_o = __shfl_xor(l, o, 64);
    float acc_o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc_o[e] = __shfl_xor(acc[e], o, 64);
    const float m_n = fmaxf(m, m_o);
    if (m_n > -INFINITY) {
      const float c1 = xf_exp2(m - m_n), c2 = xf_exp2(m_o - m_n);
      l = l * c1 + l_o * c2;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = acc[e] * c1 + acc_o[e] * c2;
      m = m_n;
    }
  }
  if (grp != 0) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;  // no visible key: ctx = 0
#pragma unroll
  for (int e = 0; e < E; e += 4)
    xf_st4<Q16>(ctx, out + e, make_float4(acc[e] * inv, acc[e + 1] * inv, acc[e + 2] * inv, acc[e + 3] * inv));
}

// The last layer's rows into the state (what xfmr_session_pool reads) and into tok_out; a refused row: a zero tok_out row.
__global__ __launch_bounds__(256) void session_store_kernel(SessRows a, const float* x, float* tok_state, float* tok_out) {
  const int quads = a.H / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows * quads) return;
  const int64_t r = i / quads;
  const int c = (int)(i % quads) * 4;
  const int slot = a.slot[r], pos = a.pos[r];
  const bool ok = sess_row_ok(slot, pos, a.n_slots, a.max_len);
  const float4 v = ok ? *reinterpret_cast<const float4*>(x + r * a.H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) *reinterpret_cast<float4*>(tok_state + ((int64_t)slot * a.max_len + pos) * a.H + c) = v;
  if (tok_out) *reinterpret_cast<float4*>(tok_out + r * a.H + c) = v;
}

template <int HS, bool KV16, bool S16>
int launch_pair(const SessRows& a, const void* qkv, const uint8_t* km, void* ctx, hipStream_t st) {
  const int64_t quads = a.n_rows * (a.H / 2), pairs = a.n_rows * a.A;
  hipLaunchKernelGGL((session_append_kernel<HS, KV16, S16>), dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, a, qkv, km);
  XF_LAUNCH_CHECK();
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)HS);
  hipLaunchKernelGGL((session_attend_kernel<HS, KV16, S16>), dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, a, qkv, ctx,
                     scale_log2e);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}
int append_attend(const SessShape& s, const SessRows& a, const void* qkv, const uint8_t* km, void* ctx, hipStream_t st) {
  const bool h32 = s.hs == 32;
  if (s.mix) return h32 ? launch_pair<32, true, true>(a, qkv, km, ctx, st) : launch_pair<64, true, true>(a, qkv, km, ctx, st);
  if (s.kv16) return h32 ? launch_pair<32, true, false>(a, qkv, km, ctx, st) : launch_pair<64, true, false>(a, qkv, km, ctx, st);
  return h32 ? launch_pair<32, false, false>(a, qkv, km, ctx, st) : launch_pair<64, false, false>(a, qkv, km, ctx, st);
}

}  // namespace

extern "C" {

size_t xfmr_session_state_bytes(const xfmr_encoder_cfg* cfg, int32_t n_slots) {
  SessShape s;
  if (session_shape(cfg, &s) || n_slots <= 0) return 0;
  return carve_state(cfg, s, n_slots, nullptr).total;
}

size_t xfmr_session_workspace_bytes(const xfmr_encoder_cfg* cfg, int64_t max_rows) {
  SessShape s;
  if (session_shape(cfg, &s) || max_rows <= 0 || max_rows > 0x7fffffff / 4) return 0;
  return carve_work(s, max_rows, nullptr).total;
}

int xfmr_session_plan(const xfmr_encoder_cfg* cfg, int32_t out[8]) {
  SessShape s;
  XF_TRY(session_shape(cfg, &s));
  if (!out) return XFMR_EINVAL;
  const int esz = s.kv16 ? 2 : 4, lpk = s.hs * esz / 16;
  const int32_t v[8] = {kSessChunk, lpk, 64 / lpk, esz, s.mix, s.max_len};
  memcpy(out, v, sizeof(v));
  return XFMR_OK;
}

int xfmr_session_init(const xfmr_encoder_cfg* cfg, const float* params, void* state, size_t state_bytes, int32_t n_slots,
                      void* stream) {
  SessShape s;
  XF_TRY(session_shape(cfg, &s));
  if (!params || !state || n_slots <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(state)) return XFMR_EALIGN;
  const SessState t = carve_state(cfg, s, n_slots, (unsigned char*)state);
  if (state_bytes < t.total) return XFMR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (xf_zero_async(t.mask, t.mask_bytes, st) != hipSuccess) return XFMR_EHIP;
  if (s.mix) {
    const int64_t n4 = xfmr_param_count(cfg) / 4;  // (every tensor size is a multiple of 4: H, I multiples of 4)
    hipLaunchKernelGGL(session_params_bf16_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, params,
                       (__bf16*)t.wbf, n4);
    XF_LAUNCH_CHECK();
  }
  return XFMR_OK;
}

int xfmr_session_append(const xfmr_encoder_cfg* cfg, const float* params, void* state, size_t state_bytes, int32_t n_slots,
                        const int64_t* item_idx, const int32_t* row_slot, const int32_t* row_pos, int64_t n_rows,
                        const float* table, int64_t n_table_rows, float* tok_out, void* workspace, size_t workspace_bytes,
                        void* stream) {
  SessShape s;
  XF_TRY(session_shape(cfg, &s));
  if (!params || !state || !item_idx || !row_slot || !row_pos || !table || !workspace) return XFMR_EINVAL;
  if (n_slots <= 0 || n_rows <= 0 || n_rows > 0x7fffffff / 4 || n_table_rows <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(state) || !xf_aligned16(table) || !xf_aligned16(workspace) ||
      !xf_aligned16(tok_out))
    return XFMR_EALIGN;
  const SessState t = carve_state(cfg, s, n_slots, (unsigned char*)state);
  if (state_bytes < t.total) return XFMR_EWORKSPACE;
  const SessWork w = carve_work(s, n_rows, (unsigned char*)workspace);
  if (workspace_bytes < w.total) return XFMR_EWORKSPACE;

  hipStream_t st = (hipStream_t)stream;
  const int H = s.H, I = s.I, prec = cfg->precision;
  const float eps = cfg->ln_eps;
  const bool mix = s.mix;
  const int64_t R = n_rows;
  int64_t off[4 + 16 * kSessMaxLayers];
  if (xfmr_param_offsets(cfg, off, 4 + 16 * kSessMaxLayers) < 0) return XFMR_EINVAL;
  const uint32_t sA = mix ? XF_S16_A : 0, sB = mix ? XF_S16_B : 0, sC = mix ? XF_S16_C : 0;
  auto W = [&](int64_t o) -> const float* {  // weight operand: the bf16 copy xfmr_session_init made under bf16 storage
    return mix ? reinterpret_cast<const float*>((const __bf16*)t.wbf + o) : params + o;
  };
  const XfSeed none(0, nullptr);

  hipLaunchKernelGGL(session_pos_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, row_slot, row_pos, w.pos_safe,
                     R, n_slots, s.max_len);
  XF_LAUNCH_CHECK();
  XF_TRY(xf_embed_ln_fwd_packed_ex(item_idx, table, n_table_rows, params + off[0], params + off[1], params + off[2],
                                   params + off[3], w.x, mix ? w.xb : nullptr, nullptr, nullptr, nullptr, w.km, R,
                                   w.pos_safe, H, eps, 0.f, none, 0, st));
  SessRows a{row_slot, row_pos, R, n_slots, s.max_len, H, s.A, s.layers, 0, t.kv, t.mask};
  // y / y16 <- LayerNorm(in W^T + bias + res): the two-launch form of the forward-only pass
  auto linear_ln = [&](const void* in, int64_t wo, int64_t bo, int K, const float* res, int64_t gamma, int64_t beta, float* y,
                       void* y16) -> int {
    XF_TRY(xf_linear_fwd_ex(in, W(wo), params + bo, w.sum, R, H, K, XFMR_EPI_BIAS_DROP_RES, res, nullptr, 0.f, none, 0, prec,
                            sA | sB, st));
    return xf_layernorm_fwd_ex(w.sum, params + gamma, params + beta, y, y16, nullptr, nullptr, R, H, eps, st);
  };
  for (int i = 0; i < s.layers; ++i) {
    const int64_t* p = off + 4 + 16 * i;  // xfmr_param_offsets' order: wq wk wv bq bk bv wo bo ln1g ln1b w1 b1 w2 b2 ln2g ln2b
    const void* const xg = mix ? (const void*)w.xb : (const void*)w.x;
    XF_TRY(xf_linear_fwd_ex(xg, W(p[0]), params + p[3], w.qkv, R, 3 * H, H, XFMR_EPI_BIAS, nullptr, nullptr, 0.f, none, 0, prec,
                            sC | sA | sB, st));
    a.layer = i;
    XF_TRY(append_attend(s, a, w.qkv, w.km, w.ctx, st));
    XF_TRY(linear_ln(w.ctx, p[6], p[7], H, w.x, p[8], p[9], w.x1, mix ? w.x1b : nullptr));
    const void* const x1g = mix ? (const void*)w.x1b : (const void*)w.x1;
    XF_TRY(xf_linear_gelu_fwd_infer(x1g, W(p[10]), params + p[11], w.g, R, I, H, prec, sC | sA | sB, st));
    XF_TRY(linear_ln(w.g, p[12], p[13], I, w.x1, p[14], p[15], w.x, mix ? w.xb : nullptr));  // (x is read by nothing any more)
  }
  const int64_t quads = R * (H / 4);
  hipLaunchKernelGGL(session_store_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, a, w.x, t.tok, tok_out);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xfmr_session_pool(const xfmr_encoder_cfg* cfg, const void* state, size_t state_bytes, int32_t n_slots,
                      const int32_t* slots, const int32_t* lens, int32_t n, int32_t mode, int32_t normalize, float eps,
                      float* out, void* stream) {
  SessShape s;
  XF_TRY(session_shape(cfg, &s));
  if (!state || n_slots <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(state)) return XFMR_EALIGN;
  const SessState t = carve_state(cfg, s, n_slots, (unsigned char*)const_cast<void*>(state));
  if (state_bytes < t.total) return XFMR_EWORKSPACE;
  return pool_slots_launch(t.tok, t.mask, slots, lens, n, n_slots, s.max_len, s.H, mode, normalize, eps, out,
                           (hipStream_t)stream);
}

}  // extern "C"
