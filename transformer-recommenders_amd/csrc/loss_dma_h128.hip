// LDS-DMA bf16 main kernel of the fused sampled loss, H = 128: every form that
// loss_dma_built (loss_dma.inc) names for this width, and loss_qprep_kernel. One translation unit per hidden size: build
// time, and the Makefile's per-width flags. No rule lives here: loss_common.h (forms, parts), loss.hip (loss_plan).
#include "loss_common.h"
#include "loss_dma.inc"

int xf_launch_loss_dma_128(const LossArgs& a, const void* table_bf16, int code, dim3 grid, hipStream_t st) {
  return xfl_launch_form<128>(a, (const __bf16*)table_bf16, code, grid, st);
}
int xf_launch_loss_qprep_128(const LossArgs& a, __bf16* qimg, float2* qaux, dim3 grid, hipStream_t st) {
  return xf_launch_loss_qprep_t<128>(a, qimg, qaux, grid, st);
}
