// The host-side halves of the segmentation criterion's entries, for loss_seg_region.hip: cvx_seg_loss (loss_seg.hip) and cvx_seg_loss_opts
// (loss_seg_opts.hip) are "chain" (every launch up to and including the finalize) followed by the adjoint of the bilinear resize.  The
// region criterion runs a chain, adds its own term to the gradient plane the chain leaves, and launches the adjoint itself.  The chain
// functions launch the kernels the entries launched before the split, with the same arguments and in the same order; they do not clear
// bad_target (the entry does) and they check no argument (the entry has).  Internal to the library: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What a chain leaves on the device: the fp32 gradient plane (batch, nc, oh, ow), not yet normalised, and its normaliser --
// norm_mode 0: norm_const; 1: acc[1] where that is positive, else 1 (resize_grad_rows_kernel's rule).
struct SegChainOut {
  float* dlogits;
  const double* acc;
  int norm_mode;
  double norm_const;
};

// workspace: cvx_seg_loss_workspace_bytes() bytes
void seg_plain_chain(const float* rows_f32, int ld, int batch, int nc, int ih, int iw, int oh, int ow, const int64_t* target, int mode, float alpha,
                     float gamma, int64_t ignore_index, float* loss_out, int32_t* bad_target, void* workspace, hipStream_t st, SegChainOut* out);
// workspace: cvx_seg_loss_opts_workspace_bytes() bytes; ohem_theta < 0: no OHEM
void seg_opts_chain(const float* rows_f32, int ld, int batch, int nc, int ih, int iw, int oh, int ow, const int64_t* target, const float* class_weight,
                    float label_smoothing, int64_t ignore_index, float ohem_theta, int64_t ohem_min_kept, float* loss_out, int32_t* bad_target,
                    double* stats_out, void* workspace, hipStream_t st, SegChainOut* out);
