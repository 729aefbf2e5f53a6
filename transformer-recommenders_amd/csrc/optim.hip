// The optimizer step's options on the device (include/xfmr_hip.h, K18b): gradient norm / clip coefficient / scheduled
// learning rate into a 32-byte control record (xfmr_opt_prepare), the AdamW update that consumes it (xfmr_adamw_ctl), and
// the gradient accumulation of micro-batches (xfmr_grad_accumulate). All three are HBM-bound passes over the flat buffer
// with 16-byte accesses; nothing here uses an atomic, so every result is a function of its inputs alone.
#include <float.h>
#include <math.h>

#include "internal.h"

namespace {

constexpr int kNormThreads = 1024;   // 16 waves: one workgroup per CU keeps 16 KiB of loads in flight per round
constexpr int kNormMaxBlocks = 256;  // the fixed grid: one workgroup per CU of an MI355X at most
constexpr int kNormWaves = kNormThreads / 64;

struct NormRec {  // one per workgroup of the first launch
  double sumsq;
  float max_abs;
  uint32_t nonfinite;
};
static_assert(sizeof(NormRec) == 16, "NormRec");
static_assert(sizeof(xfmr_opt_ctl) == 32, "xfmr_opt_ctl is a 32-byte record");

int norm_blocks(int64_t n) {
  const int64_t n4 = n / 4;
  int64_t b = (n4 + kNormThreads - 1) / kNormThreads;
  if (b > kNormMaxBlocks) b = kNormMaxBlocks;
  return (int)(b < 1 ? 1 : b);
}

// the factor of a LambdaLR with the lr_lambda of transformers.optimization.get_*_schedule_with_warmup, s completed steps
__host__ __device__ inline double lr_lambda(int sched, int64_t W, int64_t T, int64_t s) {
  if (sched == XFMR_SCHED_CONSTANT) return 1.0;
  if (s < W) return (double)s / (double)(W > 1 ? W : 1);
  if (sched == XFMR_SCHED_WARMUP_CONSTANT) return 1.0;
  const int64_t span_i = T - W;
  const double span = (double)(span_i > 1 ? span_i : 1);
  if (sched == XFMR_SCHED_WARMUP_LINEAR) return fmax(0.0, (double)(T - s) / span);
  const double progress = (double)(s - W) / span;
  return fmax(0.0, 0.5 * (1.0 + cos(3.14159265358979323846 * progress)));
}

struct NormAcc {
  double sumsq = 0.0;
  float max_abs = 0.f;
  uint32_t nonfinite = 0;
  __device__ __forceinline__ void take(float x, float gs) {
    const float gr = x * gs;  // what the update sees (adamw_ctl_kernel), squared in fp64
    const float a = fabsf(gr);
    nonfinite += !(a <= FLT_MAX);  // NaN and inf
    max_abs = fmaxf(max_abs, a);   // (a NaN leaves the maximum as it is; it is counted above)
    const double d = (double)gr;
    sumsq += d * d;
  }
  __device__ __forceinline__ void take4(const float4& q, float gs) {
    take(q.x, gs); take(q.y, gs); take(q.z, gs); take(q.w, gs);
  }
  __device__ __forceinline__ void wave_fold() {  // butterfly over the 64 lanes: a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sumsq += __shfl_xor(sumsq, o, 64);
      max_abs = fmaxf(max_abs, __shfl_xor(max_abs, o, 64));
      nonfinite += __shfl_xor(nonfinite, o, 64);
    }
  }
};

// launch (a): grid-stride over the 16-byte groups, two loads in flight per thread; the n % 4 tail goes to workgroup 0
__global__ __launch_bounds__(kNormThreads) void grad_norm_partial_kernel(const float* g, int64_t n, float gs, NormRec* rec) {
  __shared__ NormRec red[kNormWaves];
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * kNormThreads;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  NormAcc acc;
  int64_t i = (int64_t)blockIdx.x * kNormThreads + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const float4 a = g4[i], b = g4[i + stride];
    acc.take4(a, gs);
    acc.take4(b, gs);
  }
  if (i < n4) acc.take4(g4[i], gs);
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * n4) acc.take(g[4 * n4 + threadIdx.x], gs);
  acc.wave_fold();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = NormRec{acc.sumsq, acc.max_abs, acc.nonfinite};
  __syncthreads();
  if (threadIdx.x == 0) {
    NormRec r = red[0];
#pragma unroll
    for (int w = 1; w < kNormWaves; ++w) {
      r.sumsq += red[w].sumsq;
      r.max_abs = fmaxf(r.max_abs, red[w].max_abs);
      r.nonfinite += red[w].nonfinite;
    }
    rec[blockIdx.x] = r;
  }
}

struct CtlArgs {
  const NormRec* rec; int blocks;
  int clip_mode; float clip_val;
  float lr; float lambda;  // lambda: the host's value, used when step_dev is null
  int sched; int64_t warmup, total;
  const uint32_t* step_dev; int step_off;
  xfmr_opt_ctl* ctl;
};

// launch (b): one workgroup, record t in thread t (blocks <= 256), folded in a fixed order
__global__ __launch_bounds__(kNormMaxBlocks) void opt_ctl_kernel(const CtlArgs a) {
  __shared__ NormRec red[kNormMaxBlocks / 64];
  NormAcc acc;
  if ((int)threadIdx.x < a.blocks) {
    const NormRec r = a.rec[threadIdx.x];
    acc.sumsq = r.sumsq; acc.max_abs = r.max_abs; acc.nonfinite = r.nonfinite;
  }
  acc.wave_fold();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = NormRec{acc.sumsq, acc.max_abs, acc.nonfinite};
  __syncthreads();
  if (threadIdx.x != 0) return;
  NormRec r = red[0];
#pragma unroll
  for (int w = 1; w < kNormMaxBlocks / 64; ++w) {
    r.sumsq += red[w].sumsq;
    r.max_abs = fmaxf(r.max_abs, red[w].max_abs);
    r.nonfinite += red[w].nonfinite;
  }
  const float norm = (float)sqrt(r.sumsq);
  float coef = 1.f;
  if (a.clip_mode == XFMR_CLIP_NORM) {
    const float c = a.clip_val / (norm + 1e-6f);  // torch.nn.utils.clip_grad_norm_, fp32
    coef = c > 1.f ? 1.f : c;                     // (a NaN stays a NaN: error_if_nonfinite=False)
  }
  float lam = a.lambda;
  if (a.step_dev) {
    const int64_t s = (int64_t)*a.step_dev + a.step_off - 1;  // completed optimizer steps
    lam = (float)lr_lambda(a.sched, a.warmup, a.total, s);
  }
  xfmr_opt_ctl out;
  out.grad_norm = norm; out.grad_max_abs = r.max_abs; out.clip_coef = coef; out.lr = a.lr * lam;
  out.nonfinite = r.nonfinite; out.pad[0] = out.pad[1] = out.pad[2] = 0;
  *a.ctl = out;
}

template <int CLIP>
__device__ __forceinline__ float clipped(float g, float gscale, float coef, float cv) {
  const float gr = g * gscale;
  if (CLIP == XFMR_CLIP_NORM) return gr * coef;
  if (CLIP == XFMR_CLIP_VALUE) return gr > cv ? cv : (gr < -cv ? -cv : gr);  // torch.clamp: a NaN stays a NaN
  return gr;
}

// adamw_kernel (norm.hip) with the gradient clipped and the learning rate read from the control record: the same four
// streams of 16-byte accesses, the same tail, the same arithmetic on the (clipped) gradient.
template <int CLIP>
__global__ void adamw_ctl_kernel(float* p, const float* g, float* m, float* v, int64_t n, const xfmr_opt_ctl* ctl, float b1,
                                 float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, float cv,
                                 const uint32_t* step_dev, int step_off) {
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const float lr = ctl->lr;
  const float coef = CLIP == XFMR_CLIP_NORM ? ctl->clip_coef : 1.f;
  if (step_dev) {
    const double t = (double)((int64_t)*step_dev + step_off);
    bc1 = (float)(1.0 - pow((double)b1, t));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
  }
  if (i + 3 < n) {
    float4 pp = *reinterpret_cast<float4*>(p + i);
    const float4 gg = *reinterpret_cast<const float4*>(g + i);
    float4 mm = *reinterpret_cast<float4*>(m + i);
    float4 vv = *reinterpret_cast<float4*>(v + i);
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gr = clipped<CLIP>(ga[j], gscale, coef, cv);
      float pj = pa[j] * (1.f - lr * wd);
      ma[j] = b1 * ma[j] + (1.f - b1) * gr;
      va[j] = b2 * va[j] + (1.f - b2) * gr * gr;
      const float denom = sqrtf(va[j]) / bc2_sqrt + eps;
      pa[j] = pj - (lr / bc1) * (ma[j] / denom);
    }
    *reinterpret_cast<float4*>(p + i) = pp;
    *reinterpret_cast<float4*>(m + i) = mm;
    *reinterpret_cast<float4*>(v + i) = vv;
  } else {
    for (int64_t k = i; k < n; ++k) {
      const float gr = clipped<CLIP>(g[k], gscale, coef, cv);
      float pj = p[k] * (1.f - lr * wd);
      m[k] = b1 * m[k] + (1.f - b1) * gr;
      v[k] = b2 * v[k] + (1.f - b2) * gr * gr;
      const float denom = sqrtf(v[k]) / bc2_sqrt + eps;
      p[k] = pj - (lr / bc1) * (m[k] / denom);
    }
  }
}

// acc = first ? g : acc + g; thread i owns 16-byte group i, the first n % 4 threads also own the tail elements
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* acc, const float* g, int64_t n4, int64_t n, int first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) {
    float4 x = reinterpret_cast<const float4*>(g)[i];
    if (!first) {
      const float4 a = reinterpret_cast<const float4*>(acc)[i];
      x.x = a.x + x.x; x.y = a.y + x.y; x.z = a.z + x.z; x.w = a.w + x.w;
    }
    reinterpret_cast<float4*>(acc)[i] = x;
  }
  if (i < n - 4 * n4) {
    const int64_t k = 4 * n4 + i;
    acc[k] = first ? g[k] : acc[k] + g[k];
  }
}

int check_cfg(const xfmr_opt_cfg* c) {
  if (!c) return XFMR_EINVAL;
  if (c->clip_mode < XFMR_CLIP_NONE || c->clip_mode > XFMR_CLIP_VALUE) return XFMR_EINVAL;
  if (c->clip_mode != XFMR_CLIP_NONE && !(c->clip_val > 0.f)) return XFMR_EINVAL;
  if (c->sched < XFMR_SCHED_CONSTANT || c->sched > XFMR_SCHED_WARMUP_COSINE) return XFMR_EINVAL;
  if (c->warmup_steps < 0 || c->total_steps < 0) return XFMR_EINVAL;
  if (!c->step_device && c->step <= 0) return XFMR_EINVAL;
  return XFMR_OK;
}

}  // namespace

extern "C" {

float xfmr_lr_lambda(int32_t sched, int64_t warmup_steps, int64_t total_steps, int64_t completed_steps) {
  if (sched < XFMR_SCHED_CONSTANT || sched > XFMR_SCHED_WARMUP_COSINE) return NAN;
  return (float)lr_lambda(sched, warmup_steps, total_steps, completed_steps);
}

size_t xfmr_opt_workspace(int64_t n) { return n > 0 ? (size_t)norm_blocks(n) * sizeof(NormRec) : 0; }

int xfmr_opt_prepare(const xfmr_opt_cfg* cfg, const float* grads, int64_t n, void* workspace, xfmr_opt_ctl* ctl,
                     void* stream) {
  if (int rc = check_cfg(cfg)) return rc;
  if (!grads || !workspace || !ctl || n <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(grads) || !xf_aligned16(workspace) || !xf_aligned16(ctl)) return XFMR_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = norm_blocks(n);
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(blocks), dim3(kNormThreads), 0, st, grads, n, cfg->grad_scale,
                     (NormRec*)workspace);
  XF_LAUNCH_CHECK();
  CtlArgs a{};
  a.rec = (const NormRec*)workspace; a.blocks = blocks; a.clip_mode = cfg->clip_mode; a.clip_val = cfg->clip_val;
  a.lr = cfg->lr; a.sched = cfg->sched; a.warmup = cfg->warmup_steps; a.total = cfg->total_steps;
  a.step_dev = cfg->step_device; a.step_off = cfg->step_offset; a.ctl = ctl;
  a.lambda = cfg->step_device ? 1.f : xfmr_lr_lambda(cfg->sched, cfg->warmup_steps, cfg->total_steps, cfg->step - 1);
  hipLaunchKernelGGL(opt_ctl_kernel, dim3(1), dim3(kNormMaxBlocks), 0, st, a);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xfmr_adamw_ctl(const xfmr_opt_cfg* cfg, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, const xfmr_opt_ctl* ctl, void* stream) {
  if (int rc = check_cfg(cfg)) return rc;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !ctl || n <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(params) || !xf_aligned16(grads) || !xf_aligned16(exp_avg) || !xf_aligned16(exp_avg_sq) ||
      !xf_aligned16(ctl))
    return XFMR_EALIGN;
  float bc1 = 1.f, bc2_sqrt = 1.f;
  if (!cfg->step_device) {
    bc1 = (float)(1.0 - pow((double)cfg->beta1, (double)cfg->step));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)cfg->beta2, (double)cfg->step));
  }
  const int64_t threads = (n + 3) / 4;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define XF_ADAMW_CTL(MODE)                                                                                              \
  hipLaunchKernelGGL(adamw_ctl_kernel<MODE>, grid, block, 0, st, params, grads, exp_avg, exp_avg_sq, n, ctl, cfg->beta1, \
                     cfg->beta2, cfg->eps, cfg->weight_decay, bc1, bc2_sqrt, cfg->grad_scale, cfg->clip_val,             \
                     cfg->step_device, (int)cfg->step_offset)
  if (cfg->clip_mode == XFMR_CLIP_NORM) XF_ADAMW_CTL(XFMR_CLIP_NORM);
  else if (cfg->clip_mode == XFMR_CLIP_VALUE) XF_ADAMW_CTL(XFMR_CLIP_VALUE);
  else XF_ADAMW_CTL(XFMR_CLIP_NONE);
#undef XF_ADAMW_CTL
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xfmr_grad_accumulate(float* acc, const float* grads, int64_t n, int32_t first, void* stream) {
  if (!acc || !grads || n <= 0) return XFMR_EINVAL;
  if (!xf_aligned16(acc) || !xf_aligned16(grads)) return XFMR_EALIGN;
  const int64_t n4 = n / 4;
  const int64_t work = n4 > 3 ? n4 : (n4 > n - 4 * n4 ? n4 : n - 4 * n4);
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc,
                     grads, n4, n, first ? 1 : 0);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

}  // extern "C"
