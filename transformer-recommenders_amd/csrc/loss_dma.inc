// loss_main_dma_kernel: the bf16 production path of the fused sampled loss (included by the per-width loss_dma_h*.hip).
//
// Same math and partial-record format as loss_main_kernel; what differs is how a tile of 64 negatives
// reaches the matrix cores:
//   * rows are gathered by item id from a bf16 copy of the frozen table with LDS-DMA
//     (global_load_lds_dwordx4: no staging registers, no conversion, no ds_write), two tile buffers deep:
//     the gather of tile t+1 is in flight while tile t is multiplied, item ids one more tile ahead;
//   * the image is unpadded and XOR-swizzled on the SOURCE address (SwzImg), so the S^T fragment reads are
//     bank-conflict-free and the dQ product reads its transposed fragments from the SAME image with
//     ds_read_b64_tr_b16 -- there is no second [h][j] copy of the tile.
//
// HEAD >= 0 (gradient pass): only that head's reductions + its gradient weights and the dQ product.
// HEAD = -2: the logging pass without the InfoNCE log-sum-exp (its value comes from the gradient pass of the same step).
// HEAD = -1 (logging pass): values only -- evaluates all seven heads and
//               the statistics (the reference does that every step, trainer.py:250-264). Keeping the two
//               roles in separate launches keeps both under 256 registers (2 waves/SIMD, no scratch); the
//               S^T tiles are recomputed, which costs MFMA time the VALU-bound logging pass has to spare.
// HEAD: the train head (gradient pass) as a compile-time constant, or -1 for the logging pass.
// XFL_DBG (experiments only, never defined in the product build): bit 0 drops the per-element epilogue, bit 1 the
// S^T product, bit 2 the dQ product, bit 3 the gather -- to see which of VALU / MFMA / LDS / DMA overlap.
#ifndef XFL_DBG
#define XFL_DBG 0
#endif
// (A fused gradient + logging pass at one wave per SIMD was measured: 1.98 ms against 0.68 + 0.97 ms for the two
// launches at two / three waves per SIMD -- a lone wave exposes every LDS and VALU latency.)
// One H = 256 gradient pass runs as TWO column-halves of dQ (blockIdx.z): InfoNCE WITHOUT false-negative masking
// (the full-catalogue softmax of BASELINE config 4), whose online-max rescaling of all 128 dQ accumulator registers
// spilled even at one wave per SIMD (344 B/lane; 1.95 ms, 184 TFLOP/s at config 4). In halves a wave holds Q (64
// registers) and 64 accumulators, two waves fit a SIMD and, scores and weights recomputed per half, the pass takes
// 1.73 ms. The other heads keep one pass at one wave per SIMD (measured: 473-477 TFLOP/s; in halves they spill).
// H = 384 (the reference's default d_model: the all-MiniLM item table, models.py:80-91): two tile buffers are 96 KiB, so
// one workgroup per CU and one wave per SIMD whatever the registers; the online-maximum InfoNCE runs as three dQ column
// parts of 128 (64 accumulator registers beside the 96 of Q).
// (The parts rule itself, loss_dma_hparts, and the experiment build XFL_H256_LEAN_HALVES: loss_common.h.)
// Waves per SIMD of the masked logging kernels at H <= 128. This pass is bound by vector-instruction ISSUE: a plain fp32
// wave64 instruction holds the SIMD 4 cycles (scripts/probe/valu_rates.hip; a transcendental 8), and two resident waves
// cannot keep the pipe full once each spends time waiting -- a third one can (profiles/r02_loss_passes_pmc.md: 47 %
// VALU-busy at two waves). Three waves = 168 registers: round 2's build of it spilled 236 B per lane INSIDE the tile loop, which is fatal
// here (scratch accesses count in vmcnt: the wait for a reload drains the in-flight LDS-DMA gather) -- 798 against 493 us.
// With one epilogue form per tile loop, 32-bit gather offsets recomputed per call, multiplicity-0 padding columns instead of
// a validity test and no SLP-packed arithmetic (Makefile) both variants -- without the log-sum-exp (-3: the logging pass
// of an InfoNCE-trained step, the benchmark's) and with it (-4) -- need 147 registers: three waves, no scratch at all.
// What it bought: 471 -> 440 us (-3), not the 380 a free third wave would give: at three waves the vector pipe is 80 %
// busy (SQ_ACTIVE_INST_VALU 4.4 cycles per instruction x 1.98e8 instructions / 1024 SIMDs against 1.07e6 cycles), i.e.
// a wave64 instruction costs this pass ~4 issue cycles whichever wave it comes from (profiles/r03_loss_passes_pmc.md).
#ifndef XFL_LOGM_WAVES
#define XFL_LOGM_WAVES 3
#endif
#ifndef XFL_LOGU256_PK
#define XFL_LOGU256_PK 0  // the unmasked logging epilogue at H = 256 on pairs (experiment: spills)
#endif
#ifndef XFL_GRAD_WAVES
#define XFL_GRAD_WAVES 2  // the masked-InfoNCE gradient pass at H <= 128 (experiment: 3)
#endif
#ifndef XFL_LOGM_LSE_WAVES
#define XFL_LOGM_LSE_WAVES 3
#endif
template <int H, int HEAD_CODE>
constexpr int loss_dma_waves() {
  return (H <= 128 && HEAD_CODE == HEAD_LOG_MASKED) ? XFL_LOGM_WAVES  // (the unmasked form needs 178 registers: two waves)
         : (H <= 128 && HEAD_CODE == HEAD_LOG_MASKED_LSE) ? XFL_LOGM_LSE_WAVES
         : (H <= 128 && HEAD_CODE == HEAD_INFONCE_MASKED) ? XFL_GRAD_WAVES
         // values-only passes keep no dQ accumulators: two waves per SIMD up to H = 256 (two
         // 64 KB tile-buffer pairs + side data = 152 KB of LDS per CU)
         : (H <= 128 || (H <= 256 && (HEAD_CODE < 0 || loss_dma_hparts(H, HEAD_CODE) > 1))) ? 2 : 1;
}
// The tile loop's two address economies, per variant (both leave every value as it is). Budgets: 168 registers for the
// three-wave masked logging kernels, 256 for the others, the parent's waves per SIMD, no scratch in the tile loop.
//  * unrolled: the two sub-blocks of a tile and the two tile buffers as compile-time constants, so the LDS fragment reads
//    take their sub-block / buffer offsets as immediates (tile_step in the kernel). The two lean InfoNCE gradient codes up
//    to H = 256 -- the benchmark's gradient pass among them: 214-218 registers at H = 128, as rolled. Everything else
//    STAYED ROLLED: with four sub-block bodies in the loop the compiler's register demand leaves the budget (H = 128: the
//    masked logging kernels 141-149 -> 168 + 184-236 B of scratch, the lean BPR / cosine codes 200-211 -> 256 + 164-416 B,
//    the general heads worse; H = 64 the same picture; the two InfoNCE codes at H = 384: 84-228 B, and there the offsets
//    exceed the 16-bit field anyway). XFL_TILE_UNROLL=0: rolled everywhere (A/B).
//  * gather_resident: the NI per-piece (row, swizzled chunk) lane constants of the gather kept in registers across the
//    loop: the gradient passes at two waves per SIMD or fewer up to H = 256. Not the logging passes (three waves at 168
//    registers, or two whose register count decides how many more fit: H = 64 unmasked 95 -> 105 loses the fifth wave),
//    not H = 384 (NI = 12: 24 registers; 20-250 B of scratch in most variants), and not the three general heads that sit
//    at the register limit already -- the two cosine heads and the online-maximum InfoNCE (H = 128: 238-242 -> 256 + up
//    to 28 B more scratch; H = 256 InfoNCE 136 -> 240 B). They recompute the constants per call, with an unsigned
//    divide. XFL_GATHER_RESIDENT=0: recomputed everywhere (A/B).
#ifndef XFL_TILE_UNROLL
#define XFL_TILE_UNROLL 1
#endif
#ifndef XFL_GATHER_RESIDENT
#define XFL_GATHER_RESIDENT 1
#endif
template <int H, int HEAD_CODE>
constexpr bool loss_dma_unrolled() {
  return XFL_TILE_UNROLL != 0 && H <= 256 && (HEAD_CODE == HEAD_INFONCE_MASKED || HEAD_CODE == HEAD_INFONCE_PINNED);
}
template <int H, int HEAD_CODE>
constexpr bool loss_dma_gather_resident() {
  return XFL_GATHER_RESIDENT != 0 && loss_dma_waves<H, HEAD_CODE>() <= 2 && H <= 256 && HEAD_CODE > (int)XFMR_LOSS_INFONCE;
}
// (Balanced spans -- one workgroup per resident slot, each walking an equal contiguous run of the (query block, tile)
// units, at most two query prologues each, no partly filled last round -- were built and measured for the logging
// kernels in round 3: 417 us against 399 for one workgroup per (query block, split) on the same box, 405-408 with two
// or three such workgroups per slot, 454 at two per CU. Equal workgroups started together stay in phase -- prologues,
// side-data chunks and gather waits of a CU's three workgroups coincide instead of hiding behind each other's
// arithmetic -- and that costs more than the 0.17 of a round the plain grid leaves empty. Removed.)
// The per-query half of loss_main_dma_kernel's prologue, once per call instead of once per column split: query qi's fp32 row
// rounded to bf16 into row qi of `qimg` (RegRows' own conversion), and {|q|^2, q . e_pos} into qaux[qi]. Same lane map
// (lane & 31 = the query, lane >> 5 = the half of the row) and the same RegRows calls in the same order as that
// prologue, compiled in the same translation unit with the same flags: the values are the ones it computes.
template <int H>
__global__ __launch_bounds__(256) void loss_qprep_kernel(LossArgs a, __bf16* qimg, float2* qaux) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int Nq = a.counts[1];
  const int qi = blockIdx.x * QB + (tid >> 6) * 32 + (lane & 31);
  if ((int)blockIdx.x * QB >= Nq) return;
  const bool qvalid = qi < Nq;
  const int row = qvalid ? a.qrow[qi] : 0;
  const int pos_item = qvalid ? a.qpos[qi] : -2;
  RegRows<PrecBF16, H> qreg, preg;
  float qq = qreg.load_safe_sq(a.tok + (int64_t)row * H, qvalid);
  preg.load_safe(a.table + (int64_t)(qvalid ? pos_item : 0) * H, qvalid);
  float pos_dot = qreg.dot_partial(preg);
  pos_dot += xf_half_swap(pos_dot);
  qq += xf_half_swap(qq);
  if (qvalid) {
    qreg.store_image(qimg + (int64_t)qi * H);
    if (lane < 32) qaux[qi] = make_float2(qq, pos_dot);
  }
}
template <int H>
int xf_launch_loss_qprep_t(const LossArgs& a, __bf16* qimg, float2* qaux, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((loss_qprep_kernel<H>), dim3(grid.x), dim3(256), 0, st, a, qimg, qaux);
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

// QIMG: the query rows come from the bf16 image (LossArgs::qimg). A compile-time form: with both prologues behind a
// run-time test in one kernel the masked logging pass at H = 128 needed 168 registers and spilled 64 B per lane (143
// and none with either prologue alone), and the H = 256 logging kernels spilled 170-220 B.
// COUNT = false (LossArgs::no_count; the two lean InfoNCE codes only): the epilogue keeps no count, R_CNTD is written 0.
template <int H, int HEAD_CODE, bool QIMG, bool COUNT = true>
__global__ __launch_bounds__(256, (loss_dma_waves<H, HEAD_CODE>())) void loss_main_dma_kernel(
    LossArgs a, const __bf16* tbf) {
  static_assert(COUNT || HEAD_CODE == HEAD_INFONCE_MASKED || HEAD_CODE == HEAD_INFONCE_PINNED, "every other head needs its count");
  constexpr bool UNROLLED = loss_dma_unrolled<H, HEAD_CODE>();
  constexpr bool SPLIT_SUM = H > 128;  // the lean InfoNCE epilogues' running sum (loss_common.h)
  constexpr bool PINNED = HEAD_CODE == HEAD_INFONCE_PINNED;  // unmasked InfoNCE, row maximum known (loss_common.h)
  constexpr bool LEAN = HEAD_CODE == HEAD_INFONCE_MASKED || PINNED;  // lean epilogue only
  constexpr bool LOGU = HEAD_CODE == HEAD_LOG_UNMASKED_CATALOG;  // ... its unmasked full-catalogue form (loss_common.h)
  constexpr bool LOGM = HEAD_CODE == HEAD_LOG_MASKED || HEAD_CODE == HEAD_LOG_MASKED_LSE || LOGU;  // logging fast path
  constexpr bool BPRM = HEAD_CODE == HEAD_BPR_MASKED;  // masked BPR over shared negatives, lean epilogue (loss_common.h)
  constexpr bool COSM = HEAD_CODE == HEAD_CCL_MASKED || HEAD_CODE == HEAD_CONTR_MASKED;  // masked cosine heads, lean epilogue
  constexpr int HEAD = LEAN   ? (int)XFMR_LOSS_INFONCE
                       : BPRM ? (int)XFMR_LOSS_PAIRWISE_LOGISTIC
                       : HEAD_CODE == HEAD_CCL_MASKED   ? (int)XFMR_LOSS_ALIGNMENT_CONTRASTIVE
                       : HEAD_CODE == HEAD_CONTR_MASKED ? (int)XFMR_LOSS_CONTRASTIVE
                                                        : (LOGM ? -1 : HEAD_CODE);
  constexpr bool GRAD = HEAD >= 0;
  constexpr bool ALL = HEAD < 0;
  // gradient weights with exact zeros inside the margin (see the dQ product in the tile loop)
  constexpr bool SPARSE_W = COSM || (!LEAN && !BPRM && (HEAD == (int)XFMR_LOSS_PAIRWISE_HINGE || HEAD == (int)XFMR_LOSS_CONTRASTIVE ||
                                                        HEAD == (int)XFMR_LOSS_ALIGNMENT_CONTRASTIVE));
  if (GRAD) XF_CHAIN_PRIO();
  using SI = SwzImg<H>;
  constexpr int TILE_ELEMS = BN * H;
  constexpr size_t TILE_BYTES = (size_t)TILE_ELEMS * 2;
  constexpr size_t SCR_BYTES = 4 * 32 * 33 * sizeof(float);
  constexpr size_t MAIN_BYTES = (2 * TILE_BYTES > SCR_BYTES) ? 2 * TILE_BYTES : SCR_BYTES;
  // gather instructions per wave per tile: one instruction = 64 lanes x 16 B = 1 KiB of the row-major image, i.e.
  // 64 / CPR rows (H = 384: 1 1/3 rows -- every lane derives its own (row, chunk) from its position in the image)
  constexpr int NI = BN * SI::CPR / 64 / 4;
  static_assert(BN * SI::CPR % 256 == 0, "a tile must be a whole number of wave instructions per wave");
  constexpr int CH = 16;                            // tiles per side-data chunk
  // ONE shared array (a second __shared__ object next to an LDS-DMA target makes hipcc serialise on vmcnt(0))
  __shared__ __attribute__((aligned(16))) unsigned char smem[MAIN_BYTES + 3 * CH * BN * 4];
  __bf16* const sEb = reinterpret_cast<__bf16*>(smem);
  float* const sScratch = reinterpret_cast<float*>(smem);  // epilogue only: aliases the tile buffers
  // item id (-1: past the end), inverse norm and multiplicity of every column of the current chunk of CH tiles. They are
  // staged here by ordinary loads BETWEEN chunks, when no gather is in flight: hipcc drains the LDS-DMA
  // (vmcnt(0)) at the first use of any ordinary load's result, so inside a chunk the loop issues none.
  int* const sNid = reinterpret_cast<int*>(smem + MAIN_BYTES);  // [CH][BN]
  float* const sRc = reinterpret_cast<float*>(sNid + CH * BN);           // [CH][BN]
  float* const sMul = sRc + CH * BN;                                     // [CH][BN]

  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (LDS-DMA base needs it)
  const int Nq = a.counts[1];
  const int N = (a.mode == XFMR_NEG_CATALOG) ? (int)a.n_rows : a.counts[2];  // columns = distinct negative items
  const int ntiles = (N + BN - 1) / BN;
  const int qb0 = blockIdx.x * QB;
  if (qb0 >= Nq) return;
  const int split = blockIdx.y;
  const int t_beg = (int)((int64_t)ntiles * split / a.nsplit);
  const int t_end = (int)((int64_t)ntiles * (split + 1) / a.nsplit);

  // ---- per-query prologue (identical arithmetic to loss_main_kernel<PrecBF16>) -------------------------
  const int qi = qb0 + wid * 32 + (lane & 31);
  const bool qvalid = qi < Nq;
  const int row = qvalid ? a.qrow[qi] : 0;
  const int pos_item = qvalid ? a.qpos[qi] : -2;
  RegRows<PrecBF16, H> qreg;
  // (the query row is read ONCE: operand and |q|^2 from the same fp32 pieces -- round 2 read it again for the norm: with
  //  two column splits 4 x the algorithmic bytes, VERDICT r2)
  float pos_dot, qq;
  if constexpr (QIMG) {
    // several column splits walk these queries: the operand comes from the bf16 image loss_qprep_kernel wrote once for
    // the call (the same rounding of the same fp32 pieces, so every logit keeps its bits), |q|^2 and the positive's dot
    // product -- functions of the query alone, taken there with the arithmetic of the other branch -- from its record:
    // half the bytes per split, no fp32 -> bf16 conversion, no positive row gathered and multiplied per split.
    // Nothing below needs the fp32 row itself (the in-kernel finish of a one-split gradient pass does; it never runs
    // with the image).
    const int qs = qvalid ? qi : 0;
    qreg.load_safe(a.qimg + (int64_t)qs * H, qvalid);
    const float2 ax = a.qaux[qs];
    qq = qvalid ? ax.x : 0.f;
    pos_dot = qvalid ? ax.y : 0.f;
  } else {
    qq = qreg.load_safe_sq(a.tok + (int64_t)row * H, qvalid);  // row 0 / item 0 stand in for lanes past the end
    RegRows<PrecBF16, H> preg;
    preg.load_safe(a.table + (int64_t)(qvalid ? pos_item : 0) * H, qvalid);
    pos_dot = qreg.dot_partial(preg);
    pos_dot += xf_half_swap(pos_dot);
    qq += xf_half_swap(qq);
  }
  const float rq = 1.f / fmaxf(sqrtf(qq), 1e-8f);
  const float rcpos = qvalid ? a.rnorm[pos_item] : 1.f;
  const float cpos = pos_dot * rq * rcpos;
  const float sc2 = a.scale * kLog2e;
  const bool catalog = (a.mode == XFMR_NEG_CATALOG);
  const int head = a.train_head;
  const bool do_grad = GRAD && a.need_grad;
  RowState st{0.f, pos_dot * sc2, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, INFINITY, -INFINITY, 0.f};
  if (PINNED) {  // the logging pass saw every counted logit of the row (the same bf16 products, bit for bit)
    float smax = pos_dot;
    if (qvalid)
      for (int s = 0; s < a.pin_nsplit; ++s) smax = fmaxf(smax, a.pin_part[((int64_t)s * a.T + qi) * REC + R_SMAX]);
    st.m = ceilf(smax * sc2);  // (a whole power of two, as the online form keeps it: loss_epilogue_t)
  }
  const RowConst kc{pos_dot, cpos, pos_dot * (1.f - a.margin), sc2, rq, a.margin, pos_item, head,
                    a.mask_fn != 0, catalog, head <= XFMR_LOSS_CONTRASTIVE};
  constexpr int HP = loss_dma_hparts(H, HEAD_CODE);  // dQ column parts (grid.z)
  constexpr int NO = GRAD ? H / 32 / HP : 1;     // no gradient accumulators in the values-only pass
  const int hpart = HP > 1 ? (int)blockIdx.z : 0;
  f32x16 o[NO];
#pragma unroll
  for (int i = 0; i < NO; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;

  float lean_cnt = 0.f;  // LEAN: see loss_epilogue_infonce_masked
  // LOGM: pos / |e_pos| and (1 - margin) |q| (loss_epilogue_logging_masked); 1 / rq = max(|q|, 1e-8)
  LogConst lk{pos_dot, sc2, pos_dot * sc2, pos_dot * (1.f - a.margin), pos_dot * (1.f - a.margin) * kLog2e,
              pos_dot * rcpos, (1.f - a.margin) * fmaxf(sqrtf(qq), 1e-8f), pos_item, 0.f, 0.f};
  lk.kexp = xf_exp2(-lk.clog2e);
  lk.k2m = xf_exp2(-lk.m);
  const float ycap = fminf(100.f, lk.clog2e + 100.f);  // loss_epilogue_logging_masked_pk, SHARE form
  LogAcc la = log_acc_zero();                           // its pairwise partial sums (LOGM only)
  // one exponential per logit when every row of the wave has its constants in range (and, for the log-sum-exp, the
  // temperature is 1): see loss_epilogue_logging_masked
  const bool log_share = LOGM && !__any(fabsf(lk.clog2e) > 64.f) &&
                         (HEAD_CODE != HEAD_LOG_MASKED_LSE || (sc2 == kLog2e && !__any(fabsf(lk.m) > 64.f)));

  // ---- gather pipeline -------------------------------------------------------------------------------------
  const int* __restrict__ nitem = a.neg_item;
  const float* __restrict__ nrc = catalog ? a.rnorm : a.neg_rc;
  const float* __restrict__ nmul = catalog ? nullptr : a.neg_mult;
  // (the table base is wave-uniform -- an SGPR pair -- and the lane's byte offset 32 bits: the launcher keeps tables of
  //  4 GiB and more off this kernel)
  // (readfirstlane returns a SIGNED int: widen through uint32_t, or a low dword with bit 31 set sign-extends over the high one)
  const uint32_t tbf_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)tbf);
  const uint32_t tbf_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uintptr_t)tbf >> 32));
  const __bf16* const tbf_u = reinterpret_cast<const __bf16*>(((uint64_t)tbf_hi << 32) | (uint64_t)tbf_lo);
  // Per-piece lane constants of the gather -- the image row r of this lane's 16-byte piece and the byte offset of its
  // swizzled source chunk. Variants at two waves per SIMD or fewer have the registers to keep all NI pairs resident across
  // the tile loop (pinned by opaque moves, or the compiler rematerialises them per call); three-wave variants recompute
  // them per call (loss_dma_gather_resident).
  constexpr bool GRES = loss_dma_gather_resident<H, HEAD_CODE>();
  uint32_t g_row[GRES ? NI : 1], g_cb[GRES ? NI : 1];
  if constexpr (GRES) {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const uint32_t g = (uint32_t)((wid * NI + k) * 64) + (uint32_t)lane;
      const uint32_t r = g / (uint32_t)SI::CPR, c = g % (uint32_t)SI::CPR;
      g_row[k] = r;
      g_cb[k] = 16u * (c ^ (uint32_t)SI::swz((int)r));
      asm volatile("" : "+v"(g_row[k]), "+v"(g_cb[k]));
    }
  }
  auto issue_gather = [&](int lt, int buf) {  // lt: tile index inside the chunk
    __bf16* base = sEb + buf * TILE_ELEMS;
    if constexpr (GRES) {
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const int id = max(sNid[lt * BN + (int)g_row[k]], 0);  // past-the-end columns read the (finite) padding row
        xf_glds16_raw_so(tbf_u, (uint32_t)id * (uint32_t)(2 * H) + g_cb[k], base + (wid * NI + k) * 512);
      }
    } else {
      // (the lane index made opaque here: the per-piece lane constants -- row, swizzled position -- are then recomputed
      //  per call, a few vector instructions, instead of living in NI registers across the whole tile loop, where the
      //  register-bound variants spilled them and reloaded one in front of every piece: a vmcnt wait that serialises the
      //  pieces of a gather)
      uint32_t ln = (uint32_t)lane;
      asm volatile("" : "+v"(ln));
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const int q = wid * NI + k;
        const uint32_t g = (uint32_t)(q * 64) + ln;  // this lane's 16-byte piece of the image: row g / CPR, position g % CPR
        const uint32_t r = g / (uint32_t)SI::CPR, c = g % (uint32_t)SI::CPR;  // (unsigned: no sign fix-ups)
        const int id = max(sNid[lt * BN + (int)r], 0);  // past-the-end columns read the (finite) padding row
        xf_glds16_raw_so(tbf_u, (uint32_t)id * (uint32_t)(2 * H) + 16u * (c ^ (uint32_t)SI::swz((int)r)), base + q * 512);
      }
    }
  };

  // The tile loop exists once per compile-time form of the masked logging epilogue (SHARE: one exponential per logit;
  // otherwise the two-exponential form): a wave-uniform decision taken ONCE, outside the loop. With both
  // forms (x the past-the-end check) inlined side by side in one loop body the kernel needed 234 registers; one form
  // per loop fits the 168 of three waves per SIMD without a spill in the loop -- and a spill there is fatal: scratch
  // accesses count in vmcnt, so the wait for a reload drains the LDS-DMA gather that is in flight.
  // (written as a fully unrolled two-trip loop of which one trip runs, so that the other kernels of this template keep
  //  their exact code: NFORM = 1 there)
  constexpr int NFORM = LOGM ? 2 : 1;
  const int form_sel = (LOGM && !log_share) ? 1 : 0;
#pragma unroll
  for (int form = 0; form < NFORM; ++form) {
  if (form != form_sel) continue;
  for (int c0 = t_beg; c0 < t_end; c0 += CH) {
    const int c1 = min(c0 + CH, t_end);
    __syncthreads();  // the previous chunk's side data (and tiles) are no longer read; no DMA is in flight
    for (int e = tid; e < (c1 - c0) * BN; e += 256) {
      const int j = c0 * BN + e;
      const int jc = j < N ? j : N - 1;
      const int it = catalog ? jc : nitem[jc];
      // Past-the-end columns of the last tile. Masked logging kernels and the lean BPR gradient pass: a DUPLICATE of the last real
      // column with multiplicity 0 -- it adds nothing to any sum or count, and the minimum / maximum of the counted logits
      // see a value they already have -- so their epilogue needs no validity test at all. Everyone else: item -1.
      sNid[e] = (j < N || LOGM || BPRM || COSM) ? it : -1;
      sRc[e] = nrc[jc];
      sMul[e] = ((LOGM || BPRM || COSM) && j >= N) ? 0.f : (nmul ? nmul[jc] : 1.f);
    }
    __syncthreads();
    issue_gather(0, 0);  // every chunk starts at buffer 0
    // Unrolled form (loss_dma_unrolled): the tiles of the chunk in PAIRS -- buffers 0 and 1, the second trip skipped for the
    // tail of an odd count -- and both sub-blocks of a tile unrolled, so the sub-block's row offset sb * 32 * H * 2 and the
    // buffer's buf * TILE_BYTES are compile-time. The swizzle reads the row's low four bits only and both are multiples of
    // 32 rows: every fragment address is then a lane constant -- computed once, resident -- plus a constant that goes
    // into the ds_read's 16-bit offset field, instead of being rebuilt per sub-block. One sub-block's temporaries live at a
    // time (sched_barrier, as between the epilogues' runs). Rolled form: TU = 1, buf = lt & 1, the sub-block loop as it is.
    constexpr int TU = UNROLLED ? 2 : 1, SBU = UNROLLED ? 2 : 1;  // tiles per trip; sub-block unroll count
    static_assert(BN / 32 == 2, "two sub-blocks per tile");
    for (int tile0 = c0; tile0 < c1; tile0 += TU) {
#pragma unroll
    for (int tu = 0; tu < TU; ++tu) {
      const int tile = tile0 + tu;
      if (TU > 1 && tile >= c1) break;
      const int lt = tile - c0, buf = UNROLLED ? tu : (lt & 1);
      // this wave's gather of `tile` has landed; then everyone's has, and all reads of the other buffer are done.
      // Raw barrier + asm wait: nothing else in the loop waits on vmcnt.
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (tile + 1 < c1 && !((XFL_DBG & 8) && lt > 0)) issue_gather(lt + 1, buf ^ 1);
      const __bf16* E = sEb + buf * TILE_ELEMS;
#pragma unroll SBU
      for (int sb = 0; sb < BN / 32; ++sb) {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        if (XFL_DBG & 2) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = sRc[lt * BN + sb * 32 + r] * (float)(lane + r);
        } else SI::tile_nreg(s, E, sb * 32, qreg.regs());
        if (XFL_DBG & 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) st.l += s[r];
        } else if (PINNED) {
          if ((tile + 1) * BN <= N)
            loss_epilogue_infonce_pinned<false, COUNT, SPLIT_SUM>(s, st.l, lean_cnt, pos_dot, sc2, st.m, pos_item, catalog,
                                                       &sNid[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
          else
            loss_epilogue_infonce_pinned<true, COUNT, SPLIT_SUM>(s, st.l, lean_cnt, pos_dot, sc2, st.m, pos_item, catalog,
                                                      &sNid[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
        } else if (LEAN) {
          if ((tile + 1) * BN <= N)
            loss_epilogue_infonce_masked<false, COUNT, SPLIT_SUM>(s, st.l, lean_cnt, pos_dot, sc2, st.m, pos_item,
                                                       &sNid[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
          else
            loss_epilogue_infonce_masked<true, COUNT, SPLIT_SUM>(s, st.l, lean_cnt, pos_dot, sc2, st.m, pos_item,
                                                      &sNid[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
        } else if (BPRM) {
          loss_epilogue_bpr_masked(s, st.logi, st.cnt_d, st.sw, pos_dot, pos_dot * (1.f - a.margin), pos_item,
                                   &sNid[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
        } else if (COSM) {
          loss_epilogue_cos_masked(s, st.contr, st.cnt_c, lk.kpos_c, lk.kappa_c, pos_item, &sNid[lt * BN + sb * 32],
                                   &sRc[lt * BN + sb * 32], &sMul[lt * BN + sb * 32], hh);
        } else if (LOGM) {
          constexpr bool LSE = HEAD_CODE == HEAD_LOG_MASKED_LSE;
          const int* nid_sb = &sNid[lt * BN + sb * 32];
          const float* rc_sb = &sRc[lt * BN + sb * 32];
          const float* mu_sb = &sMul[lt * BN + sb * 32];
          // (no validity test: past-the-end columns are multiplicity-0 duplicates, see the staging loop)
          // (the unmasked form at H = 256 spills 16 registers inside the loop when written on pairs: it keeps the
          //  one-logit-at-a-time epilogue)
          constexpr bool PK = XFL_LOG_PK && !(LOGU && H > 128 && !XFL_LOGU256_PK);
          constexpr bool FENCE = LOGU && H > 128;
          if (PK) {
            if (form == 0) loss_epilogue_logging_masked_pk<LSE, true, !LOGU, FENCE>(s, st, la, lk, ycap, nid_sb, rc_sb, mu_sb, hh);
            else loss_epilogue_logging_masked_pk<LSE, false, !LOGU, FENCE>(s, st, la, lk, ycap, nid_sb, rc_sb, mu_sb, hh);
          } else {
            if (form == 0) loss_epilogue_logging_masked<false, LSE, true, !LOGU>(s, st, lk, nid_sb, rc_sb, mu_sb, hh);
            else loss_epilogue_logging_masked<false, LSE, false, !LOGU>(s, st, lk, nid_sb, rc_sb, mu_sb, hh);
          }
        } else loss_epilogue_t<ALL, HEAD>(s, st, o, kc, &sNid[lt * BN + sb * 32], &sRc[lt * BN + sb * 32],
                                          &sMul[lt * BN + sb * 32], hh);
        if (GRAD && do_grad && !(XFL_DBG & 4)) {
          // Hinge-type heads (the cosine contrastive term relu(c - 1 + margin) of CCL / ContrastiveLoss, PairwiseHinge): a
          // pair inside its margin has gradient weight exactly 0, and most pairs are -- a 32 x 32 block whose weights are
          // ALL zero adds nothing to dQ, so its H / 16 MFMAs and transposed reads are skipped (wave-uniform test: 16 ORs
          // and one compare per block; exact). BASELINE config 5 (CCL, H = 256): the dQ product is half of the pass's
          // matrix work. Softmax / logistic heads have no exact zeros beyond the masked columns: no test there.
          bool any_w = true;
          if (SPARSE_W) {
            uint32_t bits = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) bits |= __float_as_uint(s[r]);
            any_w = __any((bits << 1) != 0u);
          }
          if (any_w) {
#pragma unroll
            for (int i = 0; i < NO; ++i) SI::tile_xb_tr(o[i], E, hpart * NO + i, sb * 32, s);
          }
        }
        if (UNROLLED) __builtin_amdgcn_sched_barrier(0);
      }
    }
    }
  }

  }

  st.cnt_d += lean_cnt;
  if (BPRM) st.logi *= kLn2;  // (log2 sums -> natural-log softplus sum)
  if (COSM) st.contr *= rq;   // (the hinge sums were taken without the 1 / |q|)
  if (LOGM) log_acc_fold(la, st);  // (zeros where the one-logit-at-a-time epilogue ran)
  if (LOGM) loss_logging_masked_finish(st, rq);
  if (HEAD == XFMR_LOSS_INFONCE) st.sw = st.l;  // the weights of this head are the softmax terms themselves
  const RowState ms = merge_halves(st);
  write_partial(ms, a.part + ((int64_t)split * a.T + qi) * REC, lane < 32 && qvalid && hpart == 0, pos_dot, rq, qq);
  if (GRAD && do_grad) {
    __syncthreads();  // sScratch aliases the tile buffers other waves may still be reading
    if (!QIMG && HP == 1 && a.d_tok != nullptr) {  // (one split: never launched with the image)
      // ---- one column split: finish the rows here (the arithmetic of loss_combine_kernel, on the accumulators) -----
      // The lane holds, of its query's dQ^T, the h-runs h0 = 32 i + 8 g + 4 hh .. + 3 (i < NO, g < 4); the other half of
      // the row is with lane ^ 32.
      const float z2pos = pos_dot * sc2;
      const float epos = exp2f(z2pos - ms.m);  // m >= z2pos
      const float ltot = ms.l + epos;
      const float inv_d = 1.f / (ms.cnt_d + 1e-9f), inv_c = 1.f / (ms.cnt_c + 1e-9f);
      constexpr bool cosh = HEAD <= XFMR_LOSS_CONTRASTIVE;
      const float* ep = a.table + (int64_t)(qvalid ? pos_item : 0) * H;
      const float* qp = a.tok + (int64_t)row * H;
      float dotp = 0.f;
#pragma unroll
      for (int i = 0; i < NO; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int h0 = 32 * i + 8 * g + 4 * hh;
          const float4 e4 = *reinterpret_cast<const float4*>(ep + h0);
          const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
          float4 q4 = make_float4(0, 0, 0, 0);
          if (cosh) q4 = *reinterpret_cast<const float4*>(qp + h0);
          const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float Ou = o[i][4 * g + u], e = ev[u];
            float gr;
            if (HEAD == XFMR_LOSS_INFONCE) gr = a.scale * (Ou / ltot - (1.f - epos / ltot) * e);
            else if (HEAD == XFMR_LOSS_NCE) gr = -xf_sigmoid(-pos_dot) * e + Ou * inv_d;
            else if (HEAD == XFMR_LOSS_PAIRWISE_HINGE || HEAD == XFMR_LOSS_PAIRWISE_LOGISTIC)
              gr = (Ou - (1.f - a.margin) * ms.sw * e) * inv_d;
            else if (HEAD == XFMR_LOSS_CONTRASTIVE) gr = Ou * inv_c;
            else gr = -rcpos * e + Ou * inv_c;  // ALIGNMENT_CONTRASTIVE
            if (cosh) dotp = fmaf(gr * qv[u], rq, dotp);
            o[i][4 * g + u] = gr;
          }
        }
      if (cosh) {  // dL/dq_hat -> dL/dq through q / max(|q|, 1e-8)
        dotp += xf_half_swap(dotp);
        const bool clamped = sqrtf(qq) < 1e-8f;
#pragma unroll
        for (int i = 0; i < NO; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 q4 = *reinterpret_cast<const float4*>(qp + 32 * i + 8 * g + 4 * hh);
            const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float gr = o[i][4 * g + u];
              o[i][4 * g + u] = clamped ? gr * rq : rq * (gr - qv[u] * rq * dotp);
            }
          }
      }
      // transposed store, row by row, to the query's own d_tok row (lane pair j -> query qb0 + 32 wid + j)
      float* scr = sScratch + wid * 32 * 33;
      const int qj = qb0 + wid * 32 + (lane >> 1);
      const int64_t drow = qj < Nq ? (int64_t)a.qrow[qj] : -1;
#pragma unroll
      for (int i = 0; i < NO; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) scr[(lane & 31) * 33 + xf_acc_row(r, lane)] = o[i][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (drow >= 0) {
          const int j = lane >> 1, half = lane & 1;
          float* dst = a.d_tok + drow * H + 32 * i + 16 * half;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float4 v;
            v.x = scr[j * 33 + 16 * half + 4 * u + 0]; v.y = scr[j * 33 + 16 * half + 4 * u + 1];
            v.z = scr[j * 33 + 16 * half + 4 * u + 2]; v.w = scr[j * 33 + 16 * half + 4 * u + 3];
            *reinterpret_cast<float4*>(dst + 4 * u) = v;
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      return;
    }
    float* base = a.partO + (int64_t)split * a.T * H;
#pragma unroll
    for (int i = 0; i < NO; ++i)
      xf_store_tile_T(sScratch + wid * 32 * 33, o[i], 1.f, base + (hpart * NO + i) * 32, H, qb0 + wid * 32, Nq);
  }
}

// ---- the launcher: every (H, code) that is built, and nothing else -----------------------------------------------------
// The logging passes -1 / -2, the six general gradient heads, the five lean gradient codes; up to H = 256 the three fast
// logging epilogues (loss_dma_form never asks for them beyond).
constexpr bool loss_dma_built(int H, int code) {
  if (code <= HEAD_LOG_MASKED) return code >= HEAD_LOG_UNMASKED_CATALOG && H <= 256;
  return code != (int)XFMR_LOSS_ALIGNMENT && code <= HEAD_CONTR_MASKED;  // (AlignmentLoss has no gradient pass)
}
template <int H, int HEAD_CODE>
int xfl_launch_code(const LossArgs& a, const __bf16* tbf, dim3 grid, hipStream_t st) {
  if constexpr (loss_dma_built(H, HEAD_CODE)) {
    constexpr bool LEAN_NCE = HEAD_CODE == HEAD_INFONCE_MASKED || HEAD_CODE == HEAD_INFONCE_PINNED;
    if constexpr (LEAN_NCE) {
      if (a.no_count) {
        if (a.qimg != nullptr) hipLaunchKernelGGL((loss_main_dma_kernel<H, HEAD_CODE, true, false>), grid, dim3(256), 0, st, a, tbf);
        else hipLaunchKernelGGL((loss_main_dma_kernel<H, HEAD_CODE, false, false>), grid, dim3(256), 0, st, a, tbf);
        XF_LAUNCH_CHECK();
        return XFMR_OK;
      }
    } else if (a.no_count) return XFMR_EINVAL;  // (loss_plan asks for it with the two lean InfoNCE codes only)
    if (a.qimg != nullptr) hipLaunchKernelGGL((loss_main_dma_kernel<H, HEAD_CODE, true>), grid, dim3(256), 0, st, a, tbf);
    else hipLaunchKernelGGL((loss_main_dma_kernel<H, HEAD_CODE, false>), grid, dim3(256), 0, st, a, tbf);
    XF_LAUNCH_CHECK();
    return XFMR_OK;
  }
  return XFMR_EINVAL;
}
// code: loss_dma_form's; grid: (query blocks, column splits, loss_dma_hparts(H, code))
template <int H>
int xfl_launch_form(const LossArgs& a, const __bf16* tbf, int code, dim3 grid, hipStream_t st) {
  switch (code) {
    case -1: return xfl_launch_code<H, -1>(a, tbf, grid, st);
    case -2: return xfl_launch_code<H, -2>(a, tbf, grid, st);
    case HEAD_LOG_MASKED: return xfl_launch_code<H, HEAD_LOG_MASKED>(a, tbf, grid, st);
    case HEAD_LOG_MASKED_LSE: return xfl_launch_code<H, HEAD_LOG_MASKED_LSE>(a, tbf, grid, st);
    case HEAD_LOG_UNMASKED_CATALOG: return xfl_launch_code<H, HEAD_LOG_UNMASKED_CATALOG>(a, tbf, grid, st);
    case XFMR_LOSS_ALIGNMENT_CONTRASTIVE: return xfl_launch_code<H, XFMR_LOSS_ALIGNMENT_CONTRASTIVE>(a, tbf, grid, st);
    case XFMR_LOSS_CONTRASTIVE: return xfl_launch_code<H, XFMR_LOSS_CONTRASTIVE>(a, tbf, grid, st);
    case XFMR_LOSS_INFONCE: return xfl_launch_code<H, XFMR_LOSS_INFONCE>(a, tbf, grid, st);
    case XFMR_LOSS_NCE: return xfl_launch_code<H, XFMR_LOSS_NCE>(a, tbf, grid, st);
    case XFMR_LOSS_PAIRWISE_HINGE: return xfl_launch_code<H, XFMR_LOSS_PAIRWISE_HINGE>(a, tbf, grid, st);
    case XFMR_LOSS_PAIRWISE_LOGISTIC: return xfl_launch_code<H, XFMR_LOSS_PAIRWISE_LOGISTIC>(a, tbf, grid, st);
    case HEAD_INFONCE_MASKED: return xfl_launch_code<H, HEAD_INFONCE_MASKED>(a, tbf, grid, st);
    case HEAD_INFONCE_PINNED: return xfl_launch_code<H, HEAD_INFONCE_PINNED>(a, tbf, grid, st);
    case HEAD_BPR_MASKED: return xfl_launch_code<H, HEAD_BPR_MASKED>(a, tbf, grid, st);
    case HEAD_CCL_MASKED: return xfl_launch_code<H, HEAD_CCL_MASKED>(a, tbf, grid, st);
    case HEAD_CONTR_MASKED: return xfl_launch_code<H, HEAD_CONTR_MASKED>(a, tbf, grid, st);
    default: return XFMR_EINVAL;
  }
}
