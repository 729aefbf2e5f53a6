// LDS-DMA bf16 main kernel of the fused sampled loss, H = 128: six gradient-pass instantiations (one per head
// with a negative term) + the logging pass. One translation unit per hidden size to keep build time down.
#include "loss_common.h"
#include "loss_dma.inc"

int xf_launch_loss_dma_128(const LossArgs& a, const void* table_bf16, int head, dim3 grid, hipStream_t st) {
  const __bf16* tbf = (const __bf16*)table_bf16;
  dim3 block(256);
  switch (head) {
    // logging pass: masking on + in-batch negatives (the reference's default and only training form) take the fast
    // epilogue (loss_epilogue_logging_masked); everything else the general one
    case -1:
      if (a.mask_fn && a.mode == XFMR_NEG_SHARED)
        xfl_launch_dma<128, HEAD_LOG_MASKED_LSE>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, -1>(a, tbf, grid, block, st);
      break;
    case -2:
      if (a.mask_fn && a.mode == XFMR_NEG_SHARED)
        xfl_launch_dma<128, HEAD_LOG_MASKED>(a, tbf, grid, block, st);
      else if (!a.mask_fn && a.mode == XFMR_NEG_CATALOG)  // full-catalogue softmax (config 4's form)
        xfl_launch_dma<128, HEAD_LOG_UNMASKED_CATALOG>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, -2>(a, tbf, grid, block, st);
      break;
    case XFMR_LOSS_ALIGNMENT_CONTRASTIVE:  // masking on + in-batch negatives: the lean cosine epilogue
      if (a.mask_fn && a.mode == XFMR_NEG_SHARED)
        xfl_launch_dma<128, HEAD_CCL_MASKED>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, XFMR_LOSS_ALIGNMENT_CONTRASTIVE>(a, tbf, grid, block, st);
      break;
    case XFMR_LOSS_CONTRASTIVE:  // masking on + in-batch negatives: the lean cosine epilogue
      if (a.mask_fn && a.mode == XFMR_NEG_SHARED)
        xfl_launch_dma<128, HEAD_CONTR_MASKED>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, XFMR_LOSS_CONTRASTIVE>(a, tbf, grid, block, st);
      break;
    case XFMR_LOSS_INFONCE:
      if (a.mask_fn) xfl_launch_dma<128, HEAD_INFONCE_MASKED>(a, tbf, grid, block, st);
      else if (a.pin_part) xfl_launch_dma<128, HEAD_INFONCE_PINNED>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, XFMR_LOSS_INFONCE>(a, tbf, grid, block, st);
      break;
    case XFMR_LOSS_NCE:
      xfl_launch_dma<128, XFMR_LOSS_NCE>(a, tbf, grid, block, st); break;
    case XFMR_LOSS_PAIRWISE_HINGE:
      xfl_launch_dma<128, XFMR_LOSS_PAIRWISE_HINGE>(a, tbf, grid, block, st); break;
    case XFMR_LOSS_PAIRWISE_LOGISTIC:  // BPR: masking on + in-batch negatives (the reference's training form) take the lean epilogue
      if (a.mask_fn && a.mode == XFMR_NEG_SHARED && !a.tau)
        xfl_launch_dma<128, HEAD_BPR_MASKED>(a, tbf, grid, block, st);
      else xfl_launch_dma<128, XFMR_LOSS_PAIRWISE_LOGISTIC>(a, tbf, grid, block, st);
      break;
    default: return XFMR_EINVAL;
  }
  XF_LAUNCH_CHECK();
  return XFMR_OK;
}

int xf_launch_loss_qprep_128(const LossArgs& a, __bf16* qimg, float2* qaux, dim3 grid, hipStream_t st) {
  return xf_launch_loss_qprep_t<128>(a, qimg, qaux, grid, st);
}
