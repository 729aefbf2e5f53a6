// The plan of one call of the row kernels -- LayerNorm forward (plain or fused with the embedding gather), LayerNorm
// backward, the two-level column sum --: which instantiation runs, on which grid, how many partial records it writes and how
// much record room any call with no more rows can need. ONE pure function of the key: no device, no environment
// (internal.h RowKey / RowPlan; tests/test_row_plan_host.py walks it without a GPU). Included by norm.hip after its kernels.

namespace {

#define XF_ROW_KERNELS(FORM, W, FWD, INFER, BWD)                                                                        \
  {FORM, W, {{(const void*)INFER<W, false>, (const void*)FWD<W, false>}, {(const void*)INFER<W, true>, (const void*)FWD<W, true>}}, \
   (const void*)BWD<W>}
// (form, width) -> kernels, in the order the plan tries them: float4 takes H = 4 * LPR exactly, with aligned pointers; generic
// takes every H <= 64 * NPL, so an unaligned H = 64 / 128 / 256 lands on NPL = 1 / 2 / 4. Nothing takes H > 1024.
const struct RowKernels { int32_t form, width; const void* fwd[2][2]; const void* bwd; } kRowKernels[] = {  // fwd[gather][keep]
    XF_ROW_KERNELS(kRowFloat4, 16, ln_fwd_v4_kernel, ln_fwd_v4_infer_kernel, ln_bwd_v4_kernel),
    XF_ROW_KERNELS(kRowFloat4, 32, ln_fwd_v4_kernel, ln_fwd_v4_infer_kernel, ln_bwd_v4_kernel),
    XF_ROW_KERNELS(kRowFloat4, 64, ln_fwd_v4_kernel, ln_fwd_v4_infer_kernel, ln_bwd_v4_kernel),
    XF_ROW_KERNELS(kRowGeneric, 1, ln_fwd_kernel, ln_fwd_infer_kernel, ln_bwd_kernel),
    XF_ROW_KERNELS(kRowGeneric, 2, ln_fwd_kernel, ln_fwd_infer_kernel, ln_bwd_kernel),
    XF_ROW_KERNELS(kRowGeneric, 4, ln_fwd_kernel, ln_fwd_infer_kernel, ln_bwd_kernel),
    XF_ROW_KERNELS(kRowGeneric, 8, ln_fwd_kernel, ln_fwd_infer_kernel, ln_bwd_kernel),
    XF_ROW_KERNELS(kRowGeneric, kMaxPerLane, ln_fwd_kernel, ln_fwd_infer_kernel, ln_bwd_kernel),
};
#undef XF_ROW_KERNELS

int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// `blocks` workgroups asked for, each a whole number of `unit` rows: rows per block, and the blocks that then have rows
void row_map(RowPlan& p, int64_t rows, int64_t blocks, int unit) {
  p.rows_per_block = (int32_t)(cdiv64(cdiv64(rows, blocks), unit) * unit);
  p.records = (int32_t)cdiv64(rows, p.rows_per_block);
}

}  // namespace

RowPlan row_plan(const RowKey& k) {
  RowPlan p{};
  p.form = kRowNone;
  const bool colsum = k.op == kRowColsum;
  // The record room is not monotone in the row count (whole iterations per block), so it is a bound of its own: one record
  // per 4 rows up to 1 024 (LayerNorm backward), per 256 rows up to 128 (column sums). Given for a refused key too: the size
  // queries return no code.
  if (colsum) p.room = (int32_t)clamp64(cdiv64(k.rows, 256), 1, 128);
  if (k.op == kRowLnBwd) p.room = (int32_t)clamp64(cdiv64(k.rows, 4), 1, 1024);
  p.rc = (k.op < 0 || k.op >= kRowOps || k.rows <= 0 || k.H <= 0) ? XFMR_EINVAL : XFMR_OK;
  if (p.rc) return p;
  p.block = 256;
  if (colsum) {
    // 256 rows per block, at most 128 blocks, four row groups per block (rowsum_kernel; the second level sums the records)
    p.form = kRowGeneric;
    p.width = 64;  // columns per workgroup
    row_map(p, k.rows, p.room, 4);
    p.grid = (int32_t)(cdiv64(k.H, 64) * p.records);
    return p;
  }
  const RowKernels* e = nullptr;
  for (const RowKernels& t : kRowKernels)
    if (!e && (t.form == kRowFloat4 ? (k.aligned && k.H == 4 * t.width) : k.H <= 64 * t.width)) e = &t;
  if (!e) {
    p.rc = XFMR_EUNSUPPORTED;
    return p;
  }
  p.form = e->form;
  p.width = e->width;
  if (k.op != kRowLnBwd) {
    // one wave per row, or 64 / LPR rows per wave; four waves per workgroup
    p.rows_per_block = p.form == kRowFloat4 ? 4 * (64 / p.width) : 4;
    p.grid = (int32_t)cdiv64(k.rows, p.rows_per_block);
    p.kernel = e->fwd[k.op == kRowGatherLnFwd][k.keep != 0];
    return p;
  }
  // 32 rows per workgroup, <= 1024 workgroups (measured at T = 25 600: 1.859 ms/step; 64 rows / 512: 1.877;
  // 16 rows / 2048: 1.891 -- the partial records the final reduction reads grow with the workgroup count).
  // Small steps (round 4): 32 rows per workgroup are 8 dependent row round trips per wave on rows / 32 CUs -- 1 024 tokens
  // of H = 384 (the reference's default model) took 33 us per LayerNorm backward, a quarter of that step. Below 16 384 rows:
  // 16 per workgroup; below 4 096: one wave-iteration (4 waves x 64 / lanes-per-row rows).
  const int iter_rows = k.H == 64 ? 16 : k.H == 128 ? 8 : 4;  // rows of one workgroup iteration, by width alone: the
                                                              // generic kernel of an unaligned call keeps the row map
  const int per = k.rows >= 16384 ? 32 : k.rows >= 4096 ? 16 : iter_rows;
  row_map(p, k.rows, clamp64(cdiv64(k.rows, per), 1, 1024), iter_rows);
  p.grid = p.records;
  p.lds = p.form == kRowFloat4 ? 0 : 12 * k.H * (int32_t)sizeof(float);  // [4][3][H]; the float4 kernels' is static
  p.kernel = e->bwd;
  return p;
}
