// The plan of one call of the GEMM family (internal.h: GemmKey, GemmSwitches -> GemmPlan) and the environment switches: pure host
// code, no device touched. Included by gemm.hip after its kernels and tile_kernel (the gemm_kernel instantiation table).
// DESIGN.md section 4 states the rules; tests/test_gemm_plan_host.py restates them and walks them through xf_gemm_plan.
namespace {

constexpr int kDwMaxSplitCap = 256;  // the most XFMR_DW_MAXSPLIT can ask for, and what the slab room is carved for

int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
char env_first(const char* name) { const char* e = getenv(name); return e ? *e : '\0'; }  // (unset or empty: NUL)
bool env_on(const char* name) { const char c = env_first(name); return c && c != '0'; }

// ---- the weight gradients' slabs. Reduction dimension = M (tokens): ~1024 workgroups over the weight's 64 x 64 output tiles
// and the slabs, <= max_split deterministic slabs: the 128 x 128 / 384 x 128 weights have few output tiles and need the
// splits for parallelism (64 -> 128: +0.9 % of the step at batch 512; 256 no better).
int64_t dw_slabs_wanted(int N, int K, int max_split) {
  const int64_t tiles = ((N + 63) / 64) * ((K + 63) / 64);
  int64_t want = (1024 + tiles - 1) / tiles;
  if (want > max_split) want = max_split;
  return want < 1 ? 1 : want;
}
constexpr int kDwSlice = 128;  // the deep K slice: a slab's token chunk is a multiple of it
int dw_split_plan(int64_t M, int N, int K, int max_split, int* k_chunk) {
  const int64_t want = dw_slabs_wanted(N, K, max_split);
  int64_t chunk = (M + want - 1) / want;
  chunk = ((chunk + kDwSlice - 1) / kDwSlice) * kDwSlice;
  // at least two deep slices per slab once there are tokens for it: at batch 32 (6400 tokens) 50 one-slice slabs per
  // weight made the slab traffic (write + reduction) the larger part of the weight gradients -- 25 slabs: 0.760 against
  // 0.847 ms/step; batch 128 and up already have >= 256 tokens per slab (round 3, one box)
  if (M >= 4096 && chunk < 256) chunk = 256;
  if (chunk < 64) chunk = 64;
  *k_chunk = (int)chunk;
  return (int)((M + chunk - 1) / chunk);
}
// The room: the most slabs dw_split_plan gives for ANY token count <= M. The plan is not monotone in M (4 095 tokens: 32
// slabs of 128; 4 096: 16 of 256), and the packed layout (xfmr_encoder_cfg.seq_offsets) carves its slab buffers for batch x
// seq_len tokens and then launches with the real row count -- round 4: a 128 x 32 batch of 2 750 real rows wrote 22 slabs
// into room for 16. chunk >= max(kDwSlice, M / want)  =>  slabs <= min(ceil(M / kDwSlice), want), with want at its cap
// whatever XFMR_DW_MAXSPLIT says. The ring's plan (dw_ring_plan) never has more slabs than dw_split_plan.
int dw_split_bound(int64_t M, int N, int K) {
  const int64_t want = dw_slabs_wanted(N, K, kDwMaxSplitCap), by_rows = (M + kDwSlice - 1) / kDwSlice;
  const int64_t bound = by_rows < want ? by_rows : want;
  int k_chunk;
  const int plan = dw_split_plan(M, N, K, gemm_switches_once().dw_maxsplit, &k_chunk);
  return bound > plan ? (int)bound : plan;
}

// Whether dw_ring.hip's kernel takes a weight gradient (bf16 operands in HBM, 128-wide tiles both ways, operands within the
// 32-bit byte offsets of the gather); XFMR_DW_RING=0 keeps the generic kernel (A/B runs).
bool dw_ring_takes(const GemmKey& k, const GemmSwitches& sw) {
  const int items = k.op == kGemmDwGroup ? k.items : 1;
  if (!sw.dw_ring || items < 1 || items > 4 || k.precision != XFMR_PREC_BF16 || (k.s16 & SAB) != SAB || k.M <= 0) return false;
  if (k.N <= 0 || k.K <= 0 || (k.N % kDwRingTile) || (k.K % kDwRingTile)) return false;
  const int64_t widest = k.N > k.K ? k.N : k.K;
  return (uint64_t)k.M * (uint64_t)widest * 2u < kDwRingOffsetLimit;
}
// The ring kernel's own slab plan (reasons and measurements: dw_ring.hip): ~XFMR_DWR_TOKENS tokens per slab, at least
// XFMR_DWR_MINWG workgroups per weight, never more slabs than the generic plan. A function of the weight alone -- not of how
// many weights share the launch -- so that the grouped launch and a layer's four side-stream launches write the same slabs.
int dw_ring_plan(int64_t M, int N, int K, const GemmSwitches& sw, int* k_chunk) {
  const int launch_tiles = (N / kDwRingTile) * (K / kDwRingTile);
  int generic_chunk;
  const int generic = dw_split_plan(M, N, K, sw.dw_maxsplit, &generic_chunk);
  int64_t want = (M + sw.dwr_tokens - 1) / sw.dwr_tokens;
  const int64_t lo = (sw.dwr_minwg + launch_tiles - 1) / launch_tiles;
  if (want < lo) want = lo;
  if (want > generic) want = generic;
  if (want < 1) want = 1;
  int64_t chunk = (M + want - 1) / want;
  chunk = ((chunk + kDwSlice - 1) / kDwSlice) * kDwSlice;
  if (chunk < generic_chunk) chunk = generic_chunk;  // (never finer than the generic plan: its slab count is the room's bound)
  *k_chunk = (int)chunk;
  return (int)((M + chunk - 1) / chunk);
}

// The grid of a whole-row kernel (64-row tiles spanning the 128 columns, one-dimensional, padded so that every XCD gets whole
// groups: see tile_of), with the row map. False: the grid does not fit 31 bits.
bool whole_row_grid(GemmPlan& p, const GemmKey& k, const GemmSwitches& sw) {
  const RowTiles t = row_tiles(k.M, 64, k.cus, sw.row_tiles_short != 0);
  p.nt_n = 1; p.nt_z = 1; p.nt_m = t.nt_m; p.nt_full = t.nt_full; p.short_rows = t.short_rows;
  const int64_t groups = (t.nt_m + 7) / 8;
  if (groups * 8 > 0x7fffffffll) return false;
  p.grid = (int32_t)(groups * 8); p.block = 256;
  return true;
}
GemmPlan gemm_refuse(int rc, bool before_pointers) {
  GemmPlan p{};
  p.rc = rc; p.rc_shape = before_pointers ? rc : XFMR_OK;
  return p;
}

}  // namespace

// XFMR_GEMM_TILE, XFMR_DW_TILE, XFMR_GEMM_PAD_LDS, XFMR_DW_MAXSPLIT, XFMR_ROW_TILES_SHORT, XFMR_EXP_SKIP_DW, XFMR_DW_RING,
// XFMR_DWR_TOKENS and XFMR_DWR_MINWG are experiment switches a whole run is started under: read ONCE per process.
const GemmSwitches& gemm_switches_once() {
  static const GemmSwitches once = [] {
    GemmSwitches s{};
    if (const char* e = getenv("XFMR_GEMM_TILE")) { s.tile_set = 1; sscanf(e, "%d,%d,%d", &s.tile_bm, &s.tile_bn, &s.tile_bk); }
    if (const char* e = getenv("XFMR_DW_TILE")) { s.dw_tile_set = 1; sscanf(e, "%d,%d", &s.dw_bm, &s.dw_bn); }
    s.pad_lds = env_int("XFMR_GEMM_PAD_LDS", 0);
    s.dw_maxsplit = std::clamp(env_int("XFMR_DW_MAXSPLIT", 128), 1, kDwMaxSplitCap);
    s.row_tiles_short = env_on("XFMR_ROW_TILES_SHORT");
    s.skip_dw = env_first("XFMR_EXP_SKIP_DW") == '1';
    s.dw_ring = env_first("XFMR_DW_RING") != '0';
    s.dwr_tokens = std::max(env_int("XFMR_DWR_TOKENS", 3072), 128);
    s.dwr_minwg = std::max(env_int("XFMR_DWR_MINWG", 64), 1);
    s.ffn_chunk = 64;
    return s;
  }();
  return once;
}
// XFMR_FFN_CHUNK=128 (tiling only -- what the kernel stores does not depend on it: the wider chunk, two workgroups per CU --
// measured slower) and XFMR_FFN_REG_STAGE=1 (the register-staged weight chunks of the fused FFN backward) are read on EVERY
// call of the fused FFN entries, so that one test process can cover both forms and A/B timing stays inside one library.
GemmSwitches gemm_switches() {
  GemmSwitches s = gemm_switches_once();
  s.ffn_chunk = env_int("XFMR_FFN_CHUNK", 64) == 64 ? 64 : 128;
  s.ffn_reg_stage = env_on("XFMR_FFN_REG_STAGE");
  return s;
}

GemmPlan gemm_plan(const GemmKey& k, const GemmSwitches& sw) {
  const int64_t M = k.M;
  const int N = k.N, K = k.K;
  const bool bf16 = k.precision == XFMR_PREC_BF16;
  GemmPlan p{};
  p.precision = k.precision;

  if (k.op == kGemmFfnFwd || k.op == kGemmFfnFwdRe || k.op == kGemmFfnBwd) {  // H = N, I = K; bf16 storage throughout
    const bool fwd = k.op != kGemmFfnBwd;
    if (M <= 0) return gemm_refuse(XFMR_EINVAL, true);
    // (the forward stages b1 in 4 KB of LDS)
    if (N != 128 || K <= 0 || (K % (fwd ? 128 : 64)) || (fwd && K > 1024)) return gemm_refuse(XFMR_EUNSUPPORTED, true);
    p.family = fwd ? kGemmFfnFwdKernel : kGemmFfnBwdKernel;
    p.epi = !fwd ? EPI_DX_LNBWD : k.op == kGemmFfnFwdRe ? EPI_DROP_RES_LN_RE : EPI_DROP_RES_LN;
    p.precision = XFMR_PREC_BF16; p.bm = 64; p.bn = 128;
    if (fwd) p.ffn_chunk = sw.ffn_chunk == 64 ? 64 : 128;
    else p.ffn_ring = !sw.ffn_reg_stage;
    if (!whole_row_grid(p, k, sw)) return gemm_refuse(XFMR_EUNSUPPORTED, false);
    if (!fwd) p.records = p.nt_m;
    return p;
  }

  // ---- the operation's epilogue and the storage bits it keeps (GemmOp's order); the GEMM in the kernel's own terms: gm x gn
  // outputs, contraction in spans of kspan -- forward M x N over K; dX (dx) M x K over N; dW N x K over a slab's tokens
  struct OpForm { int epi; uint32_t keep; bool dx; };
  static constexpr OpForm kForms[kGemmFfnFwd] = {
      {EPI_STORE, SABC, false}, {EPI_GELU, SABC, false}, {EPI_DROP_RES, SABC, false},
      {EPI_DROP_RES_LN, SAB, false}, {EPI_DROP_RES_LN_RE, SAB, false}, {EPI_DROP_RES_LN_RED, SAB, false},
      {EPI_STORE, SABCP, true}, {EPI_GELU_GRAD, SABCP, true}, {EPI_DX_LNBWD, SAB, true},
      {EPI_SPLITK, SAB, false}, {EPI_SPLITK, SAB, false}, {EPI_SPLITK, SAB, false}};
  if (k.op < 0 || k.op >= kGemmFfnFwd) return gemm_refuse(XFMR_EINVAL, true);
  const OpForm f = kForms[k.op];
  p.epi = f.epi; p.s16 = k.s16 & f.keep;
  const bool dw = f.epi == EPI_SPLITK, whole_row = epi_res_ln(f.epi) || f.epi == EPI_DX_LNBWD;
  const int64_t gm = dw ? N : M;
  const int gn = (dw || f.dx) ? K : N;
  int kspan = f.dx ? N : K;
  if (whole_row) {  // the tile spans one whole 128-column LayerNorm row: 64 x 128 tiles, one N-tile; bf16 policy only
    if (M <= 0 || kspan <= 0) return gemm_refuse(XFMR_EINVAL, true);
    if (gn != 128 || (kspan & 7) || !bf16) return gemm_refuse(XFMR_EUNSUPPORTED, true);
    // (the re-derived forms exist for the storage the encoder runs them with: bf16 A and B operands)
    if (epi_res_mode(f.epi) != 0 && p.s16 != SAB) return gemm_refuse(XFMR_EUNSUPPORTED, false);
  } else {
    if (k.op == kGemmDwGroup && (k.items < 1 || k.items > 4)) return gemm_refuse(XFMR_EINVAL, true);
    if (M <= 0 || N <= 0 || K <= 0) return gemm_refuse(XFMR_EINVAL, true);
    if ((K & 3) || (N & 3)) return gemm_refuse(XFMR_EUNSUPPORTED, true);
    if ((k.s16 & ~XF_AUX_GELU_GRAD) && !bf16) return gemm_refuse(XFMR_EINVAL, false);
    if ((k.s16 & SABCP) && ((K & 7) || (N & 7))) return gemm_refuse(XFMR_EUNSUPPORTED, false);  // 16-byte bf16 pieces
  }

  int splits = 1;
  if (dw) {
    const bool skip = k.op == kGemmDwDeferred && sw.skip_dw;  // XFMR_EXP_SKIP_DW: the generic slab count, no launch
    if (k.op != kGemmDw && !skip && dw_ring_takes(k, sw)) {  // the ring takes the deferred and the grouped form
      p.family = kGemmRing; p.s16 = SAB;
      p.bm = p.bn = kDwRingTile; p.bk = XF_DWR_RT;
      p.splits = dw_ring_plan(M, N, K, sw, &p.k_chunk);
      p.nt_n = K / kDwRingTile; p.nt_m = N / kDwRingTile; p.nt_z = p.splits;
      const int64_t grid = (int64_t)((p.splits + 7) / 8) * 8 * p.nt_n * p.nt_m;  // whole groups of slabs per XCD
      if (grid > 0x7fffffffll) return gemm_refuse(XFMR_EUNSUPPORTED, false);
      p.grid = (int32_t)grid; p.block = 512; p.lds = kDwRingLds;
      return p;
    }
    splits = p.splits = dw_split_plan(M, N, K, sw.dw_maxsplit, &p.k_chunk);
    kspan = p.k_chunk;
    if (skip) return p;
  }

  // ---- the tile and the slice depth (the reasons and measurements are with gemm_kernel)
  p.bm = 64; p.bn = (whole_row || (gn >= 256 && p.epi != EPI_GELU_GRAD)) ? 128 : 64;
  if (dw && gm > 64 && gn > 64) {
    p.bm = 128; p.bn = 64;
    if (sw.dw_bm) { p.bm = sw.dw_bm; p.bn = sw.dw_bn; }
  }
  if (sw.tile_bm && !whole_row) { p.bm = sw.tile_bm; p.bn = sw.tile_bn; }
  if (p.bm < 1 || p.bn < 1) return gemm_refuse(XFMR_EINVAL, false);  // (a malformed override)
  const int deep = dw ? 128 : 64;
  p.bk = (bf16 && sw.tile_bk != 32 && kspan % deep == 0) ? deep : 32;
  p.kernel = (const void*)tile_kernel(k.op, k.precision, p.s16, p.bm, p.bn, p.bk);
  if (!p.kernel) return gemm_refuse(XFMR_EINVAL, false);
  // the grouped launch takes the bf16 production form on gemm_group_kernel's one tile: tile, slabs and counts are this plan's
  const bool group = k.op == kGemmDwGroup && k.items > 1 && bf16 && p.s16 == SAB && !sw.tile_set && !sw.dw_tile_set && N > 64 &&
                     K > 64 && !((N | K) & 7) && p.bm == 128 && p.bn == 64 && p.bk == 128;
  p.family = group ? kGemmGroup : kGemmTile;
  p.block = 256; p.lds = group ? 0 : sw.pad_lds;
  if (whole_row) {
    if (!whole_row_grid(p, k, sw)) return gemm_refuse(XFMR_EUNSUPPORTED, false);
    if (p.epi == EPI_DX_LNBWD) p.records = p.nt_m;
    return p;
  }
  p.nt_n = (gn + p.bn - 1) / p.bn;
  p.nt_m = (int)((gm + p.bm - 1) / p.bm);
  p.nt_z = splits;
  // one-dimensional launch, padded so that every XCD gets whole groups (see tile_of)
  const int64_t groups = splits > 1 ? (splits + 7) / 8 : (p.nt_m + 7) / 8;
  const int64_t per = splits > 1 ? (int64_t)p.nt_n * p.nt_m : p.nt_n;
  if (groups * per * 8 > 0x7fffffffll) return gemm_refuse(XFMR_EUNSUPPORTED, false);
  p.grid = (int32_t)(groups * per * 8);
  return p;
}
