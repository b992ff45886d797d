/* cvx_engine.h -- C ABI of the MI355X (gfx950) detection engine, libcvx_engine.so.
 *
 * The reference (calmiLovesAI/ComputerVision.pytorch) has no C/FFI boundary: its hot path is
 * torch.nn / ATen calls made from Python.  This header is the boundary a maintainer binds instead
 * (ctypes stub in INTEGRATION.md); each entry point names the reference interface it replaces,
 * as file:line under the reference tree.
 *
 * Conventions: plain pointers and sizes only (no torch types); every function returns 0 on success
 * and -1 on failure with the message available from cvx_last_error(); all device pointers are HIP
 * device memory owned by the caller unless stated; work is enqueued on the hipStream_t passed at
 * creation (stream-ordered, no host synchronisation inside).  One engine per device, externally
 * synchronised.  Activations are NHWC fp16, accumulation fp32, parameters/gradients fp32.
 */
#ifndef CVX_ENGINE_H
#define CVX_ENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVX_ABI_VERSION 6

const char* cvx_last_error(void);
int cvx_abi_version(void);

/* ---- graph description (built by the Python mirror of core/models/yolov8/yolo_v8.py:16-107) ---- */
enum { CVX_BUF_ACT_F16 = 0, CVX_BUF_PRED_F32 = 1 };
typedef struct {
  int32_t h, w, c; /* per image; PRED buffers: h*w = anchors, c = no (=nc+64) */
  int32_t kind;
} cvx_buf_desc;

typedef struct {
  int32_t buf;     /* index into the buffer table, -1 = none */
  int32_t coff;    /* first channel of the slice */
  int32_t c;       /* channels in the slice */
  int32_t pix_off; /* first pixel row (PRED buffers: anchor offset of the level), else 0 */
} cvx_view;

enum { CVX_OP_CONV = 1, CVX_OP_MAXPOOL5 = 2, CVX_OP_UPSAMPLE2 = 3,
       /* DLA-34 / CenterNet ops (core/models/centernet_model.py), forward and backward: */
       CVX_OP_MAXPOOL2 = 4, /* 2x2 stride-2 max pool (Tree.downsample, :128-129) */
       CVX_OP_DWCONVT = 5,  /* depthwise ConvTranspose2d, kernel 2*stride, padding stride/2 (IDAUp.up_i, :256); w_off -> fp32 [C][2f][2f] */
       CVX_OP_COPY = 6,     /* channel-slice copy (a tensor that lives in two concat buffers) */
       /* DeepLabv3+ / ResNet ops (core/models/deeplabv3plus.py, core/models/resnet.py), forward and backward: */
       CVX_OP_MAXPOOL3S2 = 7, /* 3x3 stride-2 pad-1 max pool (resnet.py:163) */
       CVX_OP_AVGPOOL = 8,    /* global average pool -> (B, 1, 1, C) (ASPPPooling, deeplabv3plus.py:30) */
       CVX_OP_RESIZE = 9,     /* bilinear resize (ih, iw) -> (oh, ow), align_corners = False (deeplabv3plus.py:38,117-122) */
       /* SSD / VGG ops (core/models/ssd_model.py), forward and backward: */
       CVX_OP_MAXPOOL3S1 = 10, /* 3x3 stride-1 pad-1 max pool (VGG pool5, :30) */
       CVX_OP_L2NORM = 11,     /* x / (||x||_2 over channels + 1e-10) * weight[c] (L2Normalize, :113-128); gamma_off -> weight (C floats) */
       CVX_OP_DROPOUT = 12 };  /* nn.Dropout (deeplabv3plus.py:67): k = drop probability in units of 2^-16; identity in eval mode.
                                  Training: inverted dropout, the mask a counter-based hash of (cvx_engine_set_seed, training pass, op,
                                  element) -- a different draw than torch's Philox stream, the same distribution */
/* CVX_OP_MAXPOOL2 also serves ceil_mode = True (:18): oh = ceil(ih / 2), windows clipped at the border. */
enum { CVX_ACT_BN_SILU = 1, CVX_ACT_BIAS = 2,
       CVX_ACT_BN_RELU = 3,   /* Conv + BN + ReLU (trainable: batch statistics, backward) */
       CVX_ACT_BN_LINEAR = 4, /* Conv + BN (Tree.project, ResNet downsample; trainable) */
       /* epilogues without BatchNorm (trainable: dy = g * [out > 0] / g, bias gradient = column sums): */
       CVX_ACT_BIAS_RELU = 5,   /* Conv + bias + ReLU, fp16 output (head 3x3, :314-318) */
       CVX_ACT_BIAS_LINEAR = 6 }; /* Conv + bias, fp16 output, no activation (SSD ExtraLayer, ssd_model.py:90-110) */
#define CVX_OPF_RES_PRE_ACT 1 /* cvx_op_desc.flags: the residual is added before the activation (BasicBlock, :20-27) */
#define CVX_OPF_CONV_BIAS 2   /* a BN_* conv that also has a bias of its own at bias_off (VGG-BN: Conv2d(bias=True) + BatchNorm) */
#define CVX_OPF_RAW_F16 4     /* training: a BN_SILU conv (no residual, no bias) may keep its raw output in fp16 between the convolution and its
                                 normalisation pass -- and keeps THAT, not the normalised value, for the backward pass: 6 instead of 12 bytes
                                 per element around the forward BatchNorm.  The batch statistics still come from the fp32 accumulators.  For
                                 layers whose rounding the outputs do not see (YOLOv8: the neck and the head, modules 12 .. 22) */

typedef struct {
  int32_t type;
  cvx_view in, out, res;  /* res: residual added after the activation (Bottleneck shortcut) */
  int32_t ih, iw, oh, ow; /* spatial size of the input / output views */
  int32_t k, stride, pad, dil;
  int32_t act;            /* CONV: CVX_ACT_BN_SILU (modules.py:29-30) or CVX_ACT_BIAS (modules.py:424-425 last layer) */
  int32_t needs_dgrad;    /* 0 for the stem (input is the image) */
  int32_t w_cin;          /* input channels of the stored weight tensor (stem: 3, its view is zero-padded to 8) */
  /* element offsets into the caller's flat fp32 arenas; weights are stored [cout][kh][kw][cin] */
  int64_t w_off;
  int64_t gamma_off, beta_off; /* BN affine (param arena) */
  int64_t bias_off;            /* CVX_ACT_BIAS */
  int64_t rmean_off, rvar_off; /* BN running statistics (stats arena) */
  int32_t lane; /* 0 / 1: the main chain.  >= 2: an independent tail (Detect levels 1, 2) the engine MAY run on its high-priority lane
                   stream beside the main chain, forked at the first such op and joined after the last (a hint: results do not depend on it) */
  int32_t flags; /* CVX_OPF_* */
} cvx_op_desc;

typedef struct cvx_engine cvx_engine;

/* Every op kind and epilogue has a backward pass except: ReLU with a POST-activation residual, and CVX_ACT_BIAS_RELU / _BIAS_LINEAR with a
 * residual.  A graph that contains one of those, or none of whose convolutions asks for a data gradient, can only run
 * cvx_engine_forward(training = 0).  The op that reads `image_buf` may be the YOLO stem (below) or any
 * convolution with 3 stored input channels and needs_dgrad = 0 (the image is converted to NHWC fp16, 8 channels; its weight gradient
 * reads that copy).
 *
 * Builds an engine for a fixed input size.  `image_buf` is the index of the buffer-table entry (c == 8) that stands for
 * the caller's NCHW fp32 images; exactly one op may read it: the 3 -> 16..80 channel 3x3 stride-2 BN+SiLU stem, which runs
 * in fp32 straight from the caller's tensor (no fp16 copy of the image is made).
 * Replaces: Yolo8.__init__ graph construction, core/models/yolov8/yolo_v8.py:17-62.  *
 * Threading: the auxiliary HIP streams (weight gradients, lanes) are ONE set per device shared by all engines of the process (the
 * hardware-queue budget).  All engines of a device must therefore be driven from one host thread (or be externally
 * serialised), and while a hipGraph capture of one engine's step is open no other engine of that device may launch: its kernels would
 * land on the shared streams that the capture has pulled into capture mode. */
int cvx_engine_create(cvx_engine** out, const cvx_buf_desc* bufs, int32_t nbufs, const cvx_op_desc* ops, int32_t nops,
                      int32_t image_buf, int32_t pred_buf, int32_t device, void* hip_stream);
int cvx_engine_destroy(cvx_engine* e);

/* Binds the caller-owned flat arenas (fp32): parameters, gradients (same layout) and BN running
 * statistics.  Replaces: nn.Module parameter/buffer storage (state_dict tensors are views of these). */
int cvx_engine_bind(cvx_engine* e, float* params, float* grads, int64_t n_params, float* stats, int64_t n_stats);

/* Changes the HIP stream subsequent calls enqueue on (e.g. a stream that is being captured into a hipGraph). */
int cvx_engine_set_stream(cvx_engine* e, void* hip_stream);
/* The stream the data-parallel gradient exchange is to be queued on (hipStream_t): the engine's own weight-gradient stream (lowest
 * priority, shared by all engines of the process).  cvx_engine_grads_ready / cvx_engine_backward_exchange fold a range's weight-gradient
 * slabs and queue its all-reduce there, behind the weight gradients they depend on.  The engine works three hardware queues (the caller's
 * stream, this one, the Detect lanes); a process that puts MORE than four to work pays 2.2-2.5x on every train step on this runtime
 * (6.5 -> 16 ms with the exchange on a stream of its own beside an engine that then had three) -- so do not create a
 * stream for the exchange: the fourth queue is RCCL's internal stream's, or the caller's launch stream's.
 * Replaces: the side stream DDP's reducer owns (torch/nn/parallel/distributed.py). */
void* cvx_engine_exchange_stream(cvx_engine* e);

/* BatchNorm hyper-parameters (core/models/yolov8/torch_utils.py:17-19: eps 1e-3, momentum 0.03). */
int cvx_engine_set_bn(cvx_engine* e, float eps, float momentum);
/* Eval-mode cross-layer fusion: a Bottleneck's 3x3 -> 3x3 (+ shortcut) and a whole Detect level as ONE tile-resident launch each
 * (csrc/conv_chain.hip).  Parity-green but measured 1-6 % slower than the per-layer kernels at batch 32, so since round 4 the kernel is part
 * of the TUNING build only (tools/build_tuning.sh, -DCVX_WITH_CHAIN; include/cvx_engine_experimental.h): in the release library
 * cvx_engine_set_fusion(e, 1) FAILS with an error that says so (enable = 0 is accepted) and cvx_engine_fused_groups returns 0.
 * Replaces: the module-by-module execution of Bottleneck.forward / Detect.forward, core/models/yolov8/modules.py:124-135, 428-433. */
/* Inference with constant weights: the caller vouches that no parameter of the bound arena changed since this engine's PREVIOUS
 * cvx_engine_forward.  The next forward (only that one) then skips the fp32 -> fp16 weight conversion and the kernels' packed weight
 * images (40 us of a 1.4-ms YOLOv8-n forward, 90-220 us of the bigger models') -- provided they were made under the current batch plan and
 * by a forward of the same mode, or a training one (an eval forward does not prepare the data-gradient images); otherwise the call has no effect.
 * BatchNorm folding (running statistics -> scale / shift) is never skipped.  The reference has no counterpart: torch converts nothing. */
int cvx_engine_keep_shadows(cvx_engine* e);
int cvx_engine_set_fusion(cvx_engine* e, int32_t enable);
int32_t cvx_engine_fused_groups(const cvx_engine* e);

/* Seed of the CVX_OP_DROPOUT masks (default 0).  Replaces: torch.manual_seed for the model's nn.Dropout layers. */
int cvx_engine_set_seed(cvx_engine* e, uint64_t seed);

/* Forward pass.  images: (B,3,H,W) fp32 NCHW in [0,1], 8-byte aligned; pred: (B, A, no) fp32, anchors of the three
 * levels concatenated (80x80, 40x40, 20x20 order), channels = [64 DFL logits | nc class logits].
 * training != 0: batch statistics + running-stat update, activations kept for backward; `images` must stay valid and
 * unchanged until the backward pass of this forward has been enqueued AND has finished (the stem's weight gradient
 * reads it).
 * Replaces: Yolo8.forward, core/models/yolov8/yolo_v8.py:78-107 (+ Conv/C2f/SPPF/Detect in modules.py). */
int cvx_engine_forward(cvx_engine* e, const float* images, int32_t batch, int32_t training, float* pred);

/* Backward pass of the last training forward.  dpred: (B, A, no) fp16 = loss_scale * dLoss/dpred.
 * Parameter gradients are ACCUMULATED (+=, unscaled by 1/loss_scale) into the bound gradient arena.
 * Replaces: loss.backward() through the model, core/trainer/yolo8_train.py:103,108. */
int cvx_engine_backward(cvx_engine* e, const void* dpred_f16, float loss_scale);

/* Debug/inspection: copies activation (which=0) or gradient (which=1) buffer `buf` of the last planned
 * batch, NHWC fp16, into dst (device or host memory, `bytes` must equal batch*h*w*c*2).  which=2 / 3: `buf` is the index
 * of a conv op and the tensor is its normalised output xhat = (y-mean)*invstd / the gradient w.r.t. its raw output,
 * dense (batch, oh, ow, cout) fp16 -- the per-layer operands of the backward pass (training plans only).   which=4: the normalised output as the backward passes USE it, fp32 (bytes = batch*h*w*c*4): the kept fp16 xhat widened, or --
 * for a CVX_OPF_RAW_F16 layer, which keeps its raw fp16 output instead -- (y - mean) * invstd computed as they compute it. */
int cvx_engine_debug_copy(cvx_engine* e, int32_t buf, int32_t which, void* dst, int64_t bytes);

/* Segmented backward for data-parallel training: the same pass as cvx_engine_backward, cut into op ranges so that the
 * caller can exchange the gradients of finished parameter ranges (RCCL all-reduce on its own stream) while the rest of the
 * pass still runs.  Protocol: begin; then for ranges that tile the op list from the last op down to op 0:
 * range(op_hi, op_lo) followed at any later point by grads_ready(op_hi, op_lo, stream) -- `stream` is made to wait for
 * the range's BN/bias gradients (main stream) and weight gradients (side stream) and then folds the range's
 * weight-gradient slabs into the gradient arena ON `stream`; after it the parameter range of those ops is final there;
 * end() joins the side stream.  The caller makes the engine's stream wait for `stream` before the optimiser step.
 * Replaces: loss.backward() + DistributedDataParallel's bucketed all-reduce hooks (the reference trains single-GPU,
 * core/trainer/yolo8_train.py:93-111; BASELINE.json north_star asks for the overlapped exchange). */
int cvx_engine_backward_begin(cvx_engine* e, const void* dpred_f16, float loss_scale);
int cvx_engine_backward_range(cvx_engine* e, int32_t op_hi, int32_t op_lo);
int cvx_engine_grads_ready(cvx_engine* e, int32_t op_hi, int32_t op_lo, void* hip_stream);
int cvx_engine_backward_end(cvx_engine* e);

/* Per-kernel-class timing with HIP events recorded on the engine's launch stream.  Classes: 0 conv forward
 * (implicit GEMM), 1 conv data-gradient, 2 conv weight-gradient, 3 BN+SiLU forward passes, 4 BN+SiLU backward
 * passes, 5 misc (layout, pool, upsample, weight shadows, bias sums), 6 gradient-slab reduction.
 * cvx_engine_profile(e, 1) starts a window; cvx_engine_profile_read synchronises, returns the summed kernel
 * time (ms), algorithmic FLOPs, algorithmic bytes and launch count per class since the window start, and
 * restarts the window. */
int cvx_engine_profile(cvx_engine* e, int32_t enable);
int cvx_engine_profile_read(cvx_engine* e, int32_t n_classes, double* ms, double* flops, double* bytes, int64_t* launches);
/* Same window, per record instead of per class: writes one CSV line "class,op,flops,bytes,ms" per timed scope to
 * `path` (op = index into the op list, -1 for whole-pass scopes) and restarts the window.  Tuning aid. */
int cvx_engine_profile_dump(cvx_engine* e, const char* path);

/* Tuning aid: while `buf` (device memory, 8 x u64 per workgroup of the largest launch) is set, thread 0 of every
 * workgroup of the DMA-ring / halo convolution kernels stores 100 MHz wall-clock stamps at five phases
 * (entry, operands issued, first K-step landed, K loop done, epilogue done).  NULL switches it off. */
int cvx_debug_clock_buffer(void* buf);

/* Tuning aid / test hook: the tiling the row-band convolution kernel (csrc/conv_tile.hip: 3x3, stride 1, pad 1 on small maps) would
 * choose for a launch -- out[0..7] = rows per tile, pixel groups per wave (MT), 16-channel tiles per workgroup (NTW), channel blocks,
 * workgroups, K-steps per weight chunk, LDS bytes, estimated microseconds x 100.  Returns 0, or -1 when the kernel does not take the
 * shape.  (No reference counterpart: the reference leaves the choice of algorithm to cuDNN behind nn.Conv2d, core/models/yolov8/modules.py:19-33.) */
int cvx_debug_conv_tile_plan(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t* out8);
/* Test hooks of the same kernel.  cvx_debug_conv_tile_ring reports the weight ring of that plan -- out[0..7] = K-steps per chunk (KSC),
 * chunks (NCH), ring slots (R: 2 = one chunk, requested whole; 3 or 4 = a ring), K-steps per tap (SPT), 1-KiB DMA pieces per wave and chunk
 * (PW), pieces of the halo patch (PP), MT and NTW of the plan (a chunk has KSC * NTW pieces).  Returns 0, or -1 when the kernel does not take the shape.
 * cvx_debug_conv_tile_force(tr, ntw) makes every plan of the process use tr rows per tile and / or ntw 16-channel tiles per workgroup
 * (0: the cost model's choice; ntw one of 1, 2, 3, 4, 5, 6, 9), so that a small map runs the instantiations the cost model picks at batch
 * 16 .. 32 only; a shape the forced pair has no plan for is one the kernel does not take (cvx_debug_conv_tile_plan returns -1,
 * cvx_conv2d_nhwc(mode | 0x2000) is an error and launches nothing, the dispatcher passes the shape on).  Returns the previous pair as
 * (tr << 8) | ntw, or -1 for other arguments (nothing changes).  Process-wide: restore (0, 0).  (No reference counterpart, as above.) */
int cvx_debug_conv_tile_ring(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t* out8);
int cvx_debug_conv_tile_force(int32_t tr, int32_t ntw);
/* Test hook: which of its compiled tile configurations the LDS-DMA ring convolution kernel (csrc/conv_igemm_dma.hip) runs for a launch of
 * `pixels` output pixels (of the largest phase class for a merged data gradient), cin gathered and cout produced channels and ntaps taps --
 * out[0..3] = tile rows (128, 64 or 32), channel tiles per workgroup (16-channel tiles for 128 / 64 rows: 1..6 or 8; 32-channel pairs for
 * 32 rows: 1..4), channel blocks (gridDim.y), DMA passes per K-step.  The launcher calls the same function.  Returns 0, or -1 on bad
 * arguments.  (No reference counterpart: the reference leaves the choice of algorithm to cuDNN behind nn.Conv2d, core/models/yolov8/modules.py:19-33.) */
int cvx_debug_conv_dma_plan(int64_t pixels, int32_t cin, int32_t cout, int32_t ntaps, int32_t* out4);
/* Test hooks, likewise for the two persistent kernels with LDS-resident weights; the launchers call the same functions.
 * 3x3 / stride 1 halo kernel (csrc/conv_halo.hip) on a batch x h x w map, cin gathered (16, 32, 64, 80, 128 or 144: anything else is an
 * error) and cout produced channels -- out[0..3] = output rows per tile TH (8, 4 or 2), channel tiles per workgroup (16-channel tiles for
 * TH 8 / 4: 1..6 or 8; 32-channel pairs for TH 2: 1..4), channel blocks (gridDim.y), tile streams per workgroup (1 or 2).
 * 1x1 / stride 1 pointwise kernel (csrc/conv_pw.hip) on `pixels` pixels, cin gathered (a multiple of 8, at most 512: anything else is an
 * error) and cout produced channels -- out[0..3] = 32-wide K-steps (1, 2, 3, 4, 6, 8, 12 or 16), 16-channel tiles per workgroup (1..6 or
 * 8), channel blocks, 16-pixel groups per wave tile (2 or 1).  Both return 0, or -1 on bad arguments.  (No reference counterpart, as above.) */
int cvx_debug_conv_halo_plan(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t* out4);
int cvx_debug_conv_pw_plan(int64_t pixels, int32_t cin, int32_t cout, int32_t* out4);
/* Test hook: the persistent convolution kernels size their grids for 1 / div of the chip (1: all of it), so that every workgroup walks
 * many tiles of a small map.  Returns the previous divisor, or -1 for div < 1 (nothing changes).  Process-wide: restore it. */
int cvx_debug_conv_grid_div(int32_t div);
/* Test hooks of the weight gradient's five kernels (csrc/conv_wgrad*.hip).  Both take the layer of cvx_conv2d_wgrad_nhwc with operand pixel
 * pitches x_ld >= cin / dy_ld >= cout (images follow each other without a gap), a kernel -- 0: whatever cvx_conv_wgrad_launch's cascade takes,
 * 1 k3, 2 stream, 3 halo, 4 gemm, 5 generic -- and a pixel-split count -- 0: the count the engine gives that kernel (wide != 0: as one of
 * the last launches of the backward pass), > 0: the caller's.  A forced kernel keeps every condition that makes it correct (the `*_can`
 * functions beside the kernels say which) and drops the dispatcher's preferences; the gemm kernel is forced on dense dy only.  A shape the
 * kernel cannot run is an error (-1), before anything is launched or written.
 * cvx_debug_conv_wgrad_plan needs no GPU.  out[0] = kernel (1 .. 5), out[1] = pixel splits, out[2] + (out[3] << 31) = bytes of the slabs
 * (splits * cout * k * k * round_up(cin, 16) * 4), out[4 ..] = what the launcher derives, by the planners it calls itself:
 *   k3:      configuration (0 .. 7 = CfgA .. CfgH), R, Wc, column blocks, ring slots, stride-2 flag, chunks, chunks per split, workgroups per split
 *   stream:  CO_T, JW, WN, WK, tap blocks, R (3x3) or Qd (1x1), ring slots, chunks, chunks per split, workgroups per split, CI_T
 *   halo:    CO_T, CI_T, taps per workgroup (3 or 9), pixel tiles, tiles per split, workgroups per split
 *   gemm, generic: output-channel rows and weight columns of the tile, tiles per split
 * cvx_debug_conv2d_wgrad_nhwc launches that kernel and reduces its slabs into dw [cout][k][k][cin] as cvx_conv2d_wgrad_nhwc does; the
 * workspace holds at least the slab bytes the plan reports.  (No reference counterpart, as above.) */
int cvx_debug_conv_wgrad_plan(int32_t batch, int32_t ih, int32_t iw, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dil,
                              int32_t x_ld, int32_t dy_ld, int32_t kernel, int32_t nsplit, int32_t wide, int32_t* out16);
int cvx_debug_conv2d_wgrad_nhwc(const void* x_f16, const void* dy_f16, int32_t batch, int32_t ih, int32_t iw, int32_t cin, int32_t cout, int32_t k,
                                int32_t stride, int32_t pad, int32_t dil, int32_t x_ld, int32_t dy_ld, int32_t kernel, int32_t nsplit, float* dw,
                                void* workspace, int64_t workspace_bytes, void* hip_stream);

/* Bytes of device memory the engine currently owns (workspaces). */
int64_t cvx_engine_workspace_bytes(const cvx_engine* e);
/* Counts re-plans: a forward with a different batch size (or the first training forward after eval-only ones) frees and
 * re-allocates every per-batch buffer.  A caller that captured launches into a hipGraph must drop the graph when this
 * number changes -- the graph holds the old buffer addresses. */
int64_t cvx_engine_plan_generation(const cvx_engine* e);

/* Copies one level of pred into an NCHW fp32 tensor (B, no, H, W) -- the reference's output format
 * (core/models/yolov8/modules.py:431-433) -- and the inverse for incoming NCHW gradients. */
int cvx_pred_level_to_nchw(const float* pred, int32_t batch, int32_t anchors, int32_t no, int32_t a_off, int32_t h, int32_t w,
                           float* out_nchw, void* hip_stream);
int cvx_nchw_grad_to_dpred(const float* grad_nchw, int32_t batch, int32_t anchors, int32_t no, int32_t a_off, int32_t h, int32_t w,
                           float scale, void* dpred_f16, void* hip_stream);

/* ---- v8 detection loss: TaskAlignedAssigner + BCE + CIoU + DFL, forward AND gradient --------------
 * pred (B,A,no) fp32; targets: n_targets rows [batch_idx, cls, cx, cy, w, h] (normalised, the
 * yolo8_collate dict flattened, core/data/collate.py:25-29); level_hw: 3 x (h, w); strides: 3.
 * Outputs: loss_items[3] = (box, cls, dfl) * gains (device fp32), dpred (B,A,no) fp16 =
 * loss_scale * d(sum(items) * B)/dpred.  workspace: cvx_loss_v8_workspace_bytes() bytes.
 * Replaces: Loss.__call__, core/algorithms/yolo_v8.py:75-124; TaskAlignedAssigner, core/utils/bboxes.py:275-470;
 * BboxLoss, core/loss/ultralytics_loss.py:25-57; bbox_iou, core/utils/ultralytics_iou.py:64-117. */
int64_t cvx_loss_v8_workspace_bytes(int32_t batch, int32_t anchors, int32_t nc, int32_t max_targets_per_image);
int cvx_loss_v8(const float* pred, int32_t batch, int32_t anchors, int32_t nc, const float* targets, int32_t n_targets,
                int32_t max_targets_per_image, const int32_t* level_hw, const float* strides, int32_t n_levels, float gain_box,
                float gain_cls, float gain_dfl, float loss_scale, float* loss_items, void* dpred_f16, void* workspace,
                int64_t workspace_bytes, void* hip_stream);
/* Same with an explicit row pitch (multiple of 4, >= 64 + nc) of pred and dpred; columns beyond 64 + nc are neither read
 * nor written (the caller keeps the padding of dpred zero). */
int cvx_loss_v8_strided(const float* pred, int32_t pred_ld, int32_t batch, int32_t anchors, int32_t nc, const float* targets,
                        int32_t n_targets, int32_t max_targets_per_image, const int32_t* level_hw, const float* strides, int32_t n_levels,
                        float gain_box, float gain_cls, float gain_dfl, float loss_scale, float* loss_items, void* dpred_f16,
                        void* workspace, int64_t workspace_bytes, void* hip_stream);

/* Per-anchor assignment of the last cvx_loss_v8* call made with this workspace and the same (batch, anchors,
 * max_targets): index of the assigned target row (-1: background) and its normalised target score (device arrays of
 * batch*anchors).  Replaces: reading TaskAlignedAssigner's target_gt_idx / fg_mask / target_scores, bboxes.py:330-345. */
int cvx_loss_v8_assignment(const void* workspace, int32_t batch, int32_t anchors, int32_t max_targets_per_image, int32_t* gt_index,
                           float* norm_score, void* hip_stream);
/* yolo8_collate's dict (core/data/collate.py:25-29; fp32 device arrays batch_idx (n), cls (n), bboxes (n,4)) -> the
 * (n,6) target rows cvx_loss_v8 reads, grouped by image in stable order.  Replaces: Loss.preprocess, yolo_v8.py:51-65. */
int cvx_pack_targets(const float* batch_idx, const float* cls, const float* bboxes, int32_t n, float* rows, void* hip_stream);

/* ---- input side: letterbox pre-processing -------------------------------
 * cvx_letterbox_u8_to_nchw: uint8 (h, w, 3) HWC image in DEVICE memory -> one (3, H, W) fp32 image of the network's input batch
 * (out_chw = batch tensor + b*3*H*W), values in [0, 1].  letterbox != 0: the reference's letter_box -- aspect-preserving
 * cv2.resize(INTER_NEAREST) to (int(h*s), int(w*s)), s = min(H/h, W/w), centred on a (128,128,128) canvas; letterbox == 0: plain
 * nearest resize to (H, W) (the reference uses INTER_CUBIC there: not built).  swap_rb: BGR source -> RGB planes (cv2.cvtColor).
 * Asynchronous on hip_stream.  cvx_letterbox_geometry: the same size / padding arithmetic on the host (the decode side needs it).
 * Replaces: letter_box + TF.to_tensor in read_image_and_convert_to_tensor, core/utils/image_process.py:29-66 (image file I/O stays
 * with the caller). */
int cvx_letterbox_geometry(int32_t h, int32_t w, int32_t H, int32_t W, int32_t* new_h, int32_t* new_w, int32_t* top, int32_t* left, double* scale);
int cvx_letterbox_u8_to_nchw(const uint8_t* image_hwc, int32_t h, int32_t w, int32_t letterbox, int32_t swap_rb, float* out_chw, int32_t H,
                             int32_t W, void* hip_stream);
/* The same for a batch of pictures of different sizes in ONE launch, asynchronous on hip_stream.  jobs: n_jobs rows in DEVICE memory --
 * src uint8 (h, w, 3) HWC in device memory, out the slot of out_nchw (slots, 3, H, W) the picture goes to.  The geometry of each picture is
 * worked out on the device with cvx_letterbox_geometry's arithmetic and the pixels by the device function cvx_letterbox_u8_to_nchw runs,
 * so slot `out` is bit-identical to that entry's output for the same picture.  A picture that collapses to nothing at this size (the
 * per-image entry fails on it) leaves its slot all padding: callers that know the sizes check first.  24 bytes per job.
 * Replaces: the per-image loop over read_image_and_convert_to_tensor in predict / scripts/detect.py:detect_video. */
typedef struct cvx_letterbox_job {
  const uint8_t* src;
  int32_t h, w, out, reserved;
} cvx_letterbox_job;
int cvx_letterbox_batch_u8_to_nchw(const cvx_letterbox_job* jobs, int32_t n_jobs, int32_t letterbox, int32_t swap_rb, float* out_nchw, int32_t H,
                                   int32_t W, void* hip_stream);

/* ---- optimiser ------------------------------------------------------------------------------------
 * torch.optim.Adam semantics (core/trainer/lr_scheduler.py:37-43): lr, betas, eps, no weight decay;
 * `step` counts from 1.  found_inf (device int32, may be NULL): when non-zero the update is skipped
 * (GradScaler.step semantics, core/trainer/yolo8_train.py:104).  zero_grad: clear g afterwards. */
int cvx_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, int32_t step, const int32_t* found_inf, int32_t zero_grad, void* hip_stream);
int cvx_check_finite(const float* grads, int64_t n, int32_t* found_inf, void* hip_stream);
/* Same update with the step state resident on the device -- state[0] = lr (written by the host when the schedule
 * changes it), state[1] = step count, state[2..3] = derived bias-correction factors, advanced by the call itself --
 * so a captured hipGraph of the whole train step can be replayed without changing any kernel argument.
 * grad_scale multiplies every gradient first (1/world_size after a SUM all-reduce of the arena; 1 otherwise). */
int cvx_adam_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                      float* state, const int32_t* found_inf, int32_t zero_grad, float grad_scale, void* hip_stream);

/* ---- weight average (ModelEMA) ---------------------------------------------------------------------
 * cvx_ema_update: ema[i] <- rn(rn(ema[i] * d) + rn(one_minus_d * src[i])) over n floats: three correctly rounded fp32 operations in
 *   this order, never contracted -- bit for bit what torch's `v *= d; v += (1 - d) * msd[k]` leaves.  The caller forms d and 1 - d in
 *   double precision and casts them.  ema and src are 16-byte aligned and distinct.  Asynchronous on hip_stream.
 *   Replaces: ModelEMA.update, core/trainer/lr_scheduler.py:55-80 (one launch per arena instead of two torch kernels per state_dict entry).
 * cvx_adam_ema_step_dev: cvx_adam_step_dev with the average of the parameters in the same pass -- ema moves toward the parameter value
 *   the step stores; on a step skipped by found_inf toward the unchanged parameters, as a loop that calls ema.update(model) after
 *   every scaler.step does.  params, grads, exp_avg, exp_avg_sq come out bit for bit as cvx_adam_step_dev leaves them.
 *   Replaces: optimizer.step + ModelEMA.update on the parameters, core/trainer/lr_scheduler.py:37-43 and :55-80. */
int cvx_ema_update(float* ema, const float* src, int64_t n, float d, float one_minus_d, void* hip_stream);
int cvx_adam_ema_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                          float* state, const int32_t* found_inf, int32_t zero_grad, float grad_scale, float* ema, float d, float one_minus_d,
                          void* hip_stream);

/* ---- optimisers with parameter groups: SGD, AdamW, frozen groups, clipping by the global norm -----------
 * group_map: one byte per 16-byte chunk of the arenas, (n + 3) / 4 bytes (arena offsets and sizes are multiples of 4 floats, so a chunk
 *   belongs to at most one parameter): a group id below n_groups, or CVX_OPTIM_UNMAPPED for "no trainable parameter here: do not touch".
 *   The caller refuses any other id before it launches (a kernel cannot return a status; an id the caller let through is left alone).
 * group_state: device float[n_groups][CVX_OPTIM_GROUP_FLOATS], written by the host only when a learning rate changes:
 *   [0] lr  [1] decay_coupled, the lambda added to the gradient (SGD)  [2] decay_factor, fp32 of the host double 1 - lr * lambda (ADAM kind:
 *   torch.optim.AdamW's param.mul_(1 - lr * wd))  [3] frozen (non-zero: the group stands still)  [4] momentum  [5] nesterov (SGD)
 *   [6] lr / (1 - beta1^t), filled by the call itself (ADAM kind)  [7] reserved.
 * state: device float[4] = [group 0's lr, step count, group 0's lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)], advanced by the call itself and
 *   only on a step that is not skipped; all groups share the step count.  A one-group ADAM run keeps the state cvx_adam_step_dev keeps.
 * cvx_optim_step, per element i of group k: g1 = rn(grads[i] * grad_scale); with a clip_state g2 = rn(g1 * clip_state[1]), else g2 = g1.
 *   Skipped step (found_inf non-zero, or clip_state[2] non-zero), frozen group or unmapped chunk: params and the buffers keep their bits;
 *   grads[i] is zeroed whenever zero_grad is set, for frozen and unmapped chunks too.
 *   CVX_OPTIM_SGD (torch.optim.SGD, dampening 0; buf1 = momentum buffer, buf2 unused): g3 = rn(g2 + rn(lambda * p)); b = rn(rn(mu * b) + g3);
 *   d = nesterov ? rn(g3 + rn(mu * b)) : b; p = rn(p - rn(lr * d)) -- every operation rounded on its own, never contracted.
 *   CVX_OPTIM_ADAM (torch.optim.AdamW; buf1 = exp_avg, buf2 = exp_avg_sq): p = rn(p * decay_factor), then cvx_adam_step_dev's own arithmetic
 *   with the group's lr / (1 - beta1^t): one group, decay_factor 1 and a map without holes give cvx_adam_step_dev's bits.
 *   ema (may be NULL): the weight average in the same pass, ema[i] <- rn(rn(ema[i] * d) + rn(one_minus_d * p)) toward the value of p the
 *   step stores -- toward the unchanged p on a skipped step and for frozen groups; unmapped chunks are not averaged.
 *   All arenas 16-byte aligned, ema != params, n_groups <= CVX_OPTIM_MAX_GROUPS.  Two launches: the 1-thread state advance and the update.
 *   Replaces: torch.optim.SGD / AdamW .step over per-parameter tensors (the reference offers Adam only, core/trainer/lr_scheduler.py:37-43).
 * cvx_grad_norm: the global L2 norm of grad_scale * grads over the chunks whose group is neither unmapped nor frozen, into
 *   clip_state = [norm, coef = min(1, max_norm / (norm + 1e-6)), non-finite marker] (torch.nn.utils.clip_grad_norm_'s coefficient).
 *   Deterministic: one partial per workgroup of a grid that depends on n alone, then one workgroup that adds the partials in a fixed
 *   tree; no floating-point atomics.  A norm that is not finite sets the marker and raises found_inf (may be NULL): the launch replaces
 *   cvx_check_finite for a step that clips, and cvx_optim_step skips on the marker -- where torch would scale every gradient by NaN.
 *   workspace: cvx_grad_norm_workspace(n) floats of device memory (at most 1024); a smaller one is refused.
 *   Replaces: torch.nn.utils.clip_grad_norm_ (one norm launch per parameter, then a host-visible total). */
enum { CVX_OPTIM_SGD = 0, CVX_OPTIM_ADAM = 1 };
#define CVX_OPTIM_MAX_GROUPS 16
#define CVX_OPTIM_GROUP_FLOATS 8
#define CVX_OPTIM_UNMAPPED 255
int cvx_optim_step(int32_t kind, float* params, float* grads, float* buf1, float* buf2, int64_t n, const uint8_t* group_map, float* group_state,
                   int32_t n_groups, float* state, float beta1, float beta2, float eps, const int32_t* found_inf, int32_t zero_grad,
                   float grad_scale, const float* clip_state, float* ema, float d, float one_minus_d, void* hip_stream);
int64_t cvx_grad_norm_workspace(int64_t n);
int cvx_grad_norm(const float* grads, int64_t n, const uint8_t* group_map, const float* group_state, int32_t n_groups, float grad_scale,
                  float max_norm, float* clip_state, int32_t* found_inf, float* workspace, int64_t workspace_floats, void* hip_stream);

/* ---- eval tail: DFL decode + sigmoid, then class-aware NMS ---------------------------------------
 * cvx_decode: pred (B,A,no) -> y (B, 4+nc, A) fp32 [cx,cy,w,h (pixels), class scores]
 *   Replaces: Detect eval branch, core/models/yolov8/modules.py:434-446.
 * cvx_nms: y -> per image up to max_det (1 .. 16384) rows [x1,y1,x2,y2,conf,cls] + the anchor index of each row;
 *   counts[b] = rows kept (-1: more candidates than the 16384 the in-LDS sort holds -- raise conf_thres).  Semantics = oracle/nms_ref.py (torchvision 0.14.1 batched_nms restated, both strategies).
 *   Replaces: non_max_suppression, core/utils/ultralytics_ops.py:131-264. */
int cvx_decode(const float* pred, int32_t batch, int32_t anchors, int32_t nc, const int32_t* level_hw, const float* strides,
               int32_t n_levels, float* y, void* hip_stream);
/* Same with an explicit row pitch of pred (>= 64 + nc): class counts that are not multiples of 8 (VOC: 20) run with the
 * class columns padded to the next multiple of 8; the padding is never read. */
int cvx_decode_strided(const float* pred, int32_t pred_ld, int32_t batch, int32_t anchors, int32_t nc, const int32_t* level_hw,
                       const float* strides, int32_t n_levels, float* y, void* hip_stream);
/* SSD decode: loc (batch, A, 4) regressions and conf (batch, A, nc+1) logits in the reference's output format, priors (A, 4)
 * corner boxes -> boxes (batch, A, 4) clipped corners, prob (batch, A, nc+1) softmax.
 * Replaces: torch.softmax + Ssd._parse_mbox_loc, core/algorithms/ssd.py:246-247,285-325. */
int cvx_ssd_decode(const float* loc, const float* conf, const float* priors, int32_t batch, int32_t anchors, int32_t num_classes_plus_bg,
                   float variance_xy, float variance_wh, float* boxes, float* prob, void* hip_stream);
/* cvx_ssd_decode that also returns, per score column, the largest probability of the whole batch (class_max: num_classes_plus_bg floats, may be
 * NULL): the caller's per-class loop (ssd.py:246-274) skips the classes nothing passes the threshold in after ONE host read. */
int cvx_ssd_decode_max(const float* loc, const float* conf, const float* priors, int32_t B, int32_t A, int32_t num_classes_plus_bg,
                       float variance_xy, float variance_wh, float* boxes, float* prob, float* class_max, void* hip_stream);
/* Column range [col0, col0 + c) of fp32 rows (batch, anchors, ld), pixels a_off .. a_off + h*w, as an NCHW block written at
 * out[b * out_bstride + out_off + ch * h*w + pix]: SSD flattens its head maps in NCHW order and concatenates the levels
 * (core/models/ssd_model.py:177-183).  Asynchronous on hip_stream. */
int cvx_pred_cols_to_nchw(const float* rows, int32_t ld, int32_t col0, int32_t c, int32_t batch, int32_t anchors, int32_t a_off, int32_t hw,
                          float* out, int64_t out_bstride, int64_t out_off, void* hip_stream);
/* YOLOv7 anchor decode.  pred: fp32 rows (batch, sum_l h_l*w_l, pred_ld) as the engine's YOLOv7 graph writes them (one row per
 * pixel, levels in the order of the network's outputs, columns a*(5+nc)+k for anchor a); anchors_wh: n_levels x 3 x (w, h) in
 * input pixels, already selected through anchors_mask.  dec: (batch, 3*sum, 5+nc) = the reference's `decoded_outputs`
 * (normalised cx, cy, w, h, objectness, class probabilities; level, anchor, pixel order).  y (optional): the same candidates as
 * (batch, 4+nc, 3*sum) channel-major [cx, cy, w, h, objectness*class_k] -- what cvx_nms_variant(CVX_NMS_VANILLA) takes, i.e. the
 * per-class greedy NMS of YOLOv7._nms with score = objectness * best class probability.
 * Replaces: YOLOv7.decode_box, core/algorithms/yolo_v7.py:234-346. */
int cvx_yolo7_decode(const float* pred, int32_t pred_ld, int32_t batch, int32_t nc, const int32_t* level_hw, const float* anchors_wh,
                     int32_t n_levels, int32_t input_h, int32_t input_w, float* dec, float* y, void* hip_stream);
enum { CVX_NMS_TV0141_CUDA = 0, /* torchvision 0.14.1's own switch for CUDA tensors: coordinate trick up to 5000 candidates */
       CVX_NMS_TV0141_CPU = 1,  /* ... for CPU tensors: up to 1000 candidates */
       CVX_NMS_OFFSET = 2,      /* _batched_nms_coordinate_trick: boxes + cls*(max+1), one class-agnostic pass */
       CVX_NMS_VANILLA = 3 };   /* _batched_nms_vanilla: per-class passes on the unshifted boxes */
#define CVX_NMS_BOXES_XYXY 0x100 /* OR-ed into `variant`: rows 0..3 of y are corner boxes already (no cx,cy,w,h conversion) */
int64_t cvx_nms_workspace_bytes(int32_t batch, int32_t anchors);
int cvx_nms(const float* y, int32_t batch, int32_t anchors, int32_t nc, float conf_thres, float iou_thres, int32_t max_det,
            float* out_rows, int32_t* out_index, int32_t* counts, void* workspace, int64_t workspace_bytes, void* hip_stream);
/* cvx_nms = cvx_nms_variant(CVX_NMS_TV0141_CUDA): what the reference's GPU predict path executes through
 * torchvision.ops.batched_nms (core/utils/ultralytics_ops.py:247). */
int cvx_nms_variant(const float* y, int32_t batch, int32_t anchors, int32_t nc, float conf_thres, float iou_thres, int32_t max_det,
                    int32_t variant, float* out_rows, int32_t* out_index, int32_t* counts, void* workspace, int64_t workspace_bytes,
                    void* hip_stream);

/* ---- Soft-NMS (Bodla et al., ICCV 2017; csrc/soft_nms.hip) -----------------------------------------------------
 * A sibling of cvx_nms_variant: the same y (batch, 4+nc, anchors), the same outputs -- out_rows (batch, max_det, 6) [x1, y1, x2, y2, final
 * score, cls], out_index (batch, max_det) the anchor of each row, counts (batch) -- and one workgroup per block of the batch (an image;
 * a (class, image) pair for SSD).  The score of a box that overlaps a better one decays instead of the box disappearing.  Every fp32
 * operation below is rounded on its own (no contraction).  tests/soft_nms_restatement.py restates the rules in numpy float32.
 *   candidates  an anchor whose best class score is > conf_thres; its class is the first arg max.  Boxes: hw = w * 0.5f, x1 = cx - hw,
 *               x2 = cx + hw, likewise y (cvx_nms's box_corners); with CVX_NMS_BOXES_XYXY in `flags` rows 0..3 are taken as they are.
 *   order       score descending, then anchor ascending (the 64-bit key of cvx_nms).  "Position" is the position in this order.
 *   segments    the candidates of one class; the whole block with CVX_SOFT_NMS_CLASS_AGNOSTIC in `flags`.  Candidates of different
 *               segments never touch each other.
 *   walk        of a segment: every candidate starts live with s = score.  Repeat: M = the live candidate with the largest s, the
 *               lowest position among equals (a candidate whose s is not >= 0 -- only a degenerate overlap above 1 gets one there -- is
 *               never taken).  The segment stops when method != HARD and s_M is not > min_score.  M is emitted with final score s_M and
 *               dies.  For every other live i of the segment o = IoU(M, i), cvx_nms's IoU to the bit (box_overlap.h:iou_value), and
 *                 CVX_SOFT_NMS_HARD      o > iou_thres removes i; its score is not touched.
 *                 CVX_SOFT_NMS_LINEAR    o > iou_thres gives s_i = s_i * (1.0f - o).
 *                 CVX_SOFT_NMS_GAUSSIAN  o > 0 gives s_i = s_i * E((o * o) / sigma).
 *               A NaN overlap satisfies neither comparison: it never decays or removes anything.
 *   E(x)        the library's own exp(-x): x >= 80 gives 0.0f; else t = -x, k = rintf(t * 1.44269504f), r = (t - k * 0.693359375f)
 *               - k * -2.12194440e-4f, p = 1/720 then p = p * r + c for c = 1/120, 1/24, 1/6, 1/2, 1, 1 (the fp32 quotients; a rounded
 *               product, then a rounded add), and ldexpf(p, k), which is exact.  Within 1e-6 relative of exp(-x) on [0, 20].
 *   merge       a segment's emissions come out in non-increasing score.  The emitted candidates of all segments are merged by (final
 *               score descending, position ascending); the first max_det leave, rows and indices past the count are zero.
 *   capacity    16384 candidates per block: more sets counts[b] = -1 (rows zero), never truncated.
 * Consequence: CVX_SOFT_NMS_HARD without CVX_SOFT_NMS_CLASS_AGNOSTIC is cvx_nms_variant(CVX_NMS_VANILLA) bit for bit in rows, indices
 * and counts.  Two calls give the same bits.
 * Refused: thresholds outside [0, 1]; sigma outside [0.05, 10] (so that x <= 20); min_score outside [0, 1); max_det outside [1, 16384];
 * an unknown method or flag.  sigma and min_score are checked, and ignored, in the methods that do not use them.
 * workspace: cvx_soft_nms_workspace_bytes(batch, anchors) bytes of device memory. */
enum { CVX_SOFT_NMS_HARD = 0, CVX_SOFT_NMS_LINEAR = 1, CVX_SOFT_NMS_GAUSSIAN = 2 };
#define CVX_SOFT_NMS_CLASS_AGNOSTIC 0x200 /* OR-ed into `flags` beside CVX_NMS_BOXES_XYXY: one segment per block */
int64_t cvx_soft_nms_workspace_bytes(int32_t batch, int32_t anchors);
int cvx_soft_nms(const float* y, int32_t batch, int32_t anchors, int32_t nc, float conf_thres, float iou_thres, int32_t max_det,
                 int32_t method, float sigma, float min_score, int32_t flags, float* out_rows, int32_t* out_index, int32_t* counts,
                 void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- CenterNet heat-map decode (BASELINE.json configs[3]) -----------------------------------------------------
 * pred: (B, H*W, pred_ld) fp32 head tensor, heat-map logits in columns [0, nc), the two channels the reference reads as
 * centre offsets at reg_col (its "wh" head), the two it reads as sizes at wh_col (its "reg" head).  Per image: sigmoid,
 * the reference's 3x3 max-pool over (x, class), top-K (score desc, flat index asc), boxes = clamp([x+dx, y+dy, w, h] / (W, H))
 * as xyxy in [0, 1], mask score >= conf, class-agnostic greedy DIoU-NMS (a box survives a kept one when DIoU <= nms_thr).
 * Outputs: boxes (B,K,4), scores (B,K), classes (B,K), topk_index (B,K) = (y*W+x)*nc+c (-1: fewer than K peaks) for the whole
 * top-K list; keep (B,K) = list positions of the survivors in descending score; counts (B) = survivors (-1: more than 2048
 * scores tie at the K-th value).  The letterbox inverse (a few scalars per image) stays with the caller.
 * Replaces: CenterNetA.decode_boxes, core/algorithms/centernet.py:271-338; diou_nms, core/utils/nms.py:9-31. */
int64_t cvx_centernet_decode_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t nc);
int cvx_centernet_decode(const float* pred, int32_t pred_ld, int32_t batch, int32_t h, int32_t w, int32_t nc, int32_t reg_col, int32_t wh_col,
                         int32_t k, float conf, float nms_thr, int32_t use_nms, float* boxes, float* scores, int32_t* classes,
                         int32_t* topk_index, int32_t* keep, int32_t* counts, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- single-op entry points (unit tests and other model families reuse them) -----------------------
 * NHWC fp16 convolution, weights [cout][kh][kw][cin] fp16.  mode 0: out fp16 = conv; mode 1: out fp16 =
 * silu(conv*scale+shift); mode 2: out fp32 = conv + bias; mode 3 (the training epilogue): out fp32 = conv, and the
 * per-channel (sum, sum of squares) are added into `shift` viewed as zeroed fixed-point replica slabs.  mode | 0x100 runs the GEMM-shaped
 * kernel (conv_gemm.hip) whatever the dispatcher would pick (needs cin % 8 == 0, cout % 4 == 0); mode | 0x8000 likewise the
 * LDS-DMA ring kernel (conv_igemm_dma.hip), mode | 0x10000 the 3x3 halo kernel (conv_halo.hip) and mode | 0x20000 the pointwise kernel
 * (conv_pw.hip); a shape outside the forced kernel is an error and launches nothing.  Replaces: F.conv2d as used by Conv.forward, core/models/yolov8/modules.py:29-30. */
int cvx_conv2d_nhwc(const void* x_f16, int32_t batch, int32_t ih, int32_t iw, int32_t cin, const void* w_f16, int32_t cout, int32_t k,
                    int32_t stride, int32_t pad, int32_t dil, int32_t mode, const float* scale_or_bias, const float* shift, void* out,
                    void* hip_stream);
/* data gradient: dx (B,ih,iw,cin) fp16 from dy (B,oh,ow,cout) fp16 and w_t [cin][kh][kw][cout] fp16.  A strided gradient takes the
 * engine's route: the pixel-shuffle GEMM where that applies, else one merged launch of its 2..4 phase classes (one launch per class
 * when a class has no pixels or no taps). */
int cvx_conv2d_dgrad_nhwc(const void* dy_f16, int32_t batch, int32_t ih, int32_t iw, int32_t cin, const void* wt_f16, int32_t cout,
                          int32_t k, int32_t stride, int32_t pad, int32_t dil, void* dx_f16, void* hip_stream);
/* weight gradient: dw [cout][kh][kw][cin] fp32 (overwritten) from x and dy; workspace >= cvx_conv2d_wgrad_workspace_bytes */
int64_t cvx_conv2d_wgrad_workspace_bytes(int32_t batch, int32_t oh, int32_t ow, int32_t cin, int32_t cout, int32_t k);
int cvx_conv2d_wgrad_nhwc(const void* x_f16, const void* dy_f16, int32_t batch, int32_t ih, int32_t iw, int32_t cin, int32_t cout,
                          int32_t k, int32_t stride, int32_t pad, int32_t dil, float* dw, void* workspace, int64_t workspace_bytes,
                          void* hip_stream);


/* ---- streaming ops on dense NHWC fp16 tensors (the kernels the engine runs between the convolutions) ----------------
 * Train-mode BatchNorm + SiLU.  y: raw conv output FP32 (B*hw, C); statistics are taken from it, running statistics
 * updated (momentum, unbiased variance); out = silu(gamma*xhat+beta) (+res) fp16, xhat = (y-mean)*invstd fp16 (the
 * operand of the backward op), mean / invstd (C) returned.  C multiple of 8, <= 2048.
 * Replaces: Conv.forward's bn + act, core/models/yolov8/modules.py:29-30 (eps / momentum: torch_utils.py:17-19). */
int cvx_bn_silu_train_nhwc(const float* y_f32, int32_t batch, int32_t hw, int32_t c, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, const void* res_f16, void* out_f16, void* xhat_f16,
                           float* mean, float* invstd, void* hip_stream);
/* Its backward: dy (gradient w.r.t. the raw conv output) from gout (gradient w.r.t. out); dgamma / dbeta are ACCUMULATED
 * (scaled by inv_scale); gres (optional) receives the residual branch's gradient = gout (+= when res_accumulate). */
int cvx_bn_silu_bwd_nhwc(const void* xhat_f16, const void* gout_f16, int32_t batch, int32_t hw, int32_t c, const float* gamma,
                         const float* beta, const float* invstd, float inv_scale, float* dgamma, float* dbeta, void* dy_f16, void* gres_f16,
                         int32_t res_accumulate, void* hip_stream);
/* The same two passes for the other Conv + BatchNorm blocks of the reference (C up to 2048).  act: 0 SiLU, 1 ReLU, 2 none.
 * res_pre = 1: the residual joins the PRE-activation, out = act(gamma*xhat + beta + res) (Bottleneck.forward, resnet.py:139-141:
 * out += identity; out = relu(out)) and gres receives the pre-activation gradient dz; res_pre = 0: out = act(.) + res, gres
 * receives gout.  ReLU's backward mask [out > 0] is kept by the forward pass in the lowest mantissa bit of xhat (so xhat of a ReLU layer is
 * accurate to one fp16 ulp instead of half); SiLU with a pre-activation residual (YOLOv7 RepConv: silu(bn(conv3x3) + bn(conv1x1)),
 * yolov7_model.py:250-262) needs the residual's forward VALUE in `out_f16`; otherwise out_f16 may be NULL.  ReLU with a post-activation
 * residual is refused.
 * Replaces: nn.BatchNorm2d + nn.ReLU in training mode (resnet.py:121-143, deeplabv3plus.py:19-27,63-68) and their autograd. */
int cvx_bn_act_train_nhwc(const float* y_f32, int32_t batch, int32_t hw, int32_t c, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, const void* res_f16, int32_t act, int32_t res_pre,
                          void* out_f16, void* xhat_f16, float* mean, float* invstd, void* hip_stream);
int cvx_bn_act_bwd_nhwc(const void* xhat_f16, const void* gout_f16, const void* out_f16, int32_t batch, int32_t hw, int32_t c,
                        const float* gamma, const float* beta, const float* invstd, int32_t act, int32_t res_pre, float inv_scale,
                        float* dgamma, float* dbeta, void* dy_f16, void* gres_f16, int32_t res_accumulate, void* hip_stream);
/* Test hooks of the two backward passes (csrc/bn_act.hip), as the engine calls them.  cvx_debug_bn_bwd_plan (host only): how they walk
 * `rows` = batch * hw rows of c channels -- out4 = rows per workgroup, rows per step of a workgroup, rows of one trip (the steps a thread
 * keeps in flight; shorter remainders go row by row), workgroups.
 * cvx_debug_bn_bwd_views is cvx_bn_act_bwd_nhwc on strided operands: gout / fwd / gres are channel-slice views, element (b, pix, ch) at
 * p[b * bstride + pix * ld + ch] (pitches in multiples of 8 elements); kept_f16 and dy_f16 stay dense.  mean != NULL: kept_f16 is the raw
 * conv output rounded to fp16 and xhat = (kept - mean) * invstd is formed on the fly (SiLU without a pre-activation residual only).
 * (No reference counterpart.) */
int cvx_debug_bn_bwd_plan(int64_t rows, int32_t c, int32_t* out4);
int cvx_debug_bn_bwd_views(const void* kept_f16, int32_t batch, int32_t hw, int32_t c, const float* gamma, const float* beta,
                           const float* invstd, const float* mean, int32_t act, int32_t res_pre, float inv_scale, const void* gout_f16,
                           int64_t gout_bstride, int32_t gout_ld, const void* fwd_f16, int64_t fwd_bstride, int32_t fwd_ld, void* gres_f16,
                           int64_t gres_bstride, int32_t gres_ld, int32_t res_accumulate, float* dgamma, float* dbeta, void* dy_f16,
                           void* hip_stream);
/* 5x5 / stride 1 / pad 2 max pool (SPPF, core/models/yolov8/modules.py:312-318) and its backward; argmax (optional in
 * the forward): one byte per element, the window tap 0..24 of the first maximum in row-major scan order. */
int cvx_maxpool5_nhwc(const void* x_f16, int32_t batch, int32_t h, int32_t w, int32_t c, void* out_f16, uint8_t* argmax, void* hip_stream);
int cvx_maxpool5_bwd_nhwc(const void* gout_f16, const uint8_t* argmax, int32_t batch, int32_t h, int32_t w, int32_t c, void* gin_f16,
                          int32_t accumulate, void* hip_stream);
/* The inference-only pooling / resampling / normalisation kernels of the DLA, ResNet + DeepLab and VGG + SSD graphs on dense NHWC fp16
 * tensors (unit parity tests, host code that wants one op); they synchronise before returning.
 *   cvx_maxpool_nhwc: kernel 2 / stride 2 (ceil_mode 0 | 1: centernet_model.py:128, ssd_model.py:16-18), kernel 3 / pad 1 / stride 1 | 2
 *     (ssd_model.py:30, resnet.py:163); output (batch, oh, ow, c) with torch's output-size rule.
 *   cvx_avgpool_global_nhwc: (batch, hw, c) -> (batch, 1, c) mean in fp32 (deeplabv3plus.py:30).
 *   cvx_resize_bilinear_nhwc: align_corners = False (deeplabv3plus.py:38,117-122).
 *   cvx_l2norm_nhwc: x / (sqrt(sum_c x^2) + 1e-10) * weight[c] (ssd_model.py:113-128). */
int cvx_maxpool_nhwc(const void* x_f16, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t kernel, int32_t stride, int32_t ceil_mode,
                     void* out_f16, void* hip_stream);
int cvx_avgpool_global_nhwc(const void* x_f16, int32_t batch, int32_t hw, int32_t c, void* out_f16, void* hip_stream);
int cvx_resize_bilinear_nhwc(const void* x_f16, int32_t batch, int32_t ih, int32_t iw, int32_t c, int32_t oh, int32_t ow, void* out_f16,
                             void* hip_stream);
int cvx_l2norm_nhwc(const void* x_f16, const float* weight, int32_t batch, int32_t hw, int32_t c, void* out_f16, void* hip_stream);
/* Bilinear resize (align_corners = False) of fp32 rows (batch, ih*iw, ld) -- e.g. a PRED buffer holding segmentation logits --
 * into an NCHW fp32 tensor (batch, c, oh, ow).  Asynchronous on hip_stream.
 * Replaces: F.interpolate(x, size=input_shape, mode="bilinear", align_corners=False), core/models/deeplabv3plus.py:147. */
int cvx_resize_bilinear_rows_to_nchw(const float* rows_f32, int32_t ld, int32_t batch, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                     float* out_nchw, void* hip_stream);
/* The fused segmentation criterion of the DeepLabv3+ step: loss = base (no region term), or base_weight * base + weight * region.
 * Both structs are plain host data, passed by pointer and read before the call returns.
 * rows: the engine's fp32 logits rows (batch, ih*iw, ld) at decoder resolution; target: (batch, oh, ow) int64 class indices at label
 * resolution (= the network input size).  Per label pixel the nc logits are interpolated bilinearly (align_corners = False,
 * deeplabv3plus.py:147) with the device function cvx_resize_bilinear_rows_to_nchw uses (bit-identical values): z_c, lse their
 * log-sum-exp, p their softmax, t the target.  Valid pixels: t != ignore_index and t in [0, nc).
 * base 1, focal loss: alpha * (1 - pt)^gamma * ce, ce = lse - z_t, pt = exp(-ce), mean over ALL batch*oh*ow pixels (focal_loss.py:14-22;
 *   ignored pixels contribute 0 to the sum and count in the mean, like the reference's .mean()).
 * base 2, cross-entropy: mean over the valid pixels (nn.CrossEntropyLoss(reduction="mean"), segmentation_2d.py:61).  Its options, in use
 *   when class_weight != NULL || label_smoothing > 0 || ohem_theta >= 0 (not in the reference), with w = class_weight (nc floats on
 *   the device; null: all ones), W = sum_c w_c, eps = label_smoothing in [0, 1):
 *     l    = (1 - eps) w_t (lse - z_t) + (eps / nc) sum_c w_c (lse - z_c)
 *     loss = sum_{i in S} l_i / sum_{i in S} w_{t_i}, S = the valid pixels -- torch's F.cross_entropy(weight=, ignore_index=,
 *            label_smoothing=, reduction="mean"); an empty S gives nan and a zero gradient.
 *   OHEM (ohem_theta >= 0; a negative value turns it off): key = fp32 max(lse - z_t, 0), ohem_theta = fp32(-ln thresh),
 *   K = ohem_min_kept >= 1 counted over the whole batch, theta_min = the K-th largest key of the valid pixels (-inf when there are fewer
 *   than K); S = the valid pixels with key > ohem_theta or key >= theta_min.  Ties at theta_min are all kept.  The selection is a radix
 *   select over the keys' bit patterns: no sort, integer atomics only.  Without an option the value and the gradient are those of the
 *   option-free kernel to the bit (unit weights and eps 0 through the options kernel give the same bits, too).
 * base 0: no base term; takes region != 0 and base_weight 0 (and a base term takes base_weight > 0 when there is a region term).
 * region != 0, the Dice / Tversky / focal-Tversky loss over the valid pixels of a group -- the batch, or each image when per_image != 0 --
 *   with y the one-hot target:
 *     I_c = sum p_c y_c, P_c = sum p_c, Y_c = sum y_c, D_c = (1 - alpha - beta) I_c + alpha P_c + beta Y_c + smooth,
 *     T_c = (I_c + smooth) / D_c (1 when D_c == 0), L_c = (1 - T_c)^gamma, group loss = sum_c m_c v_c L_c / sum_c m_c v_c (0 when that is 0),
 *     m_c = [Y_c > 0] when skip_absent != 0, else 1; v = region_class_weight (nc floats on the device; null: ones);
 *     region = mean of the group losses.  alpha = beta = 0.5 is the Dice loss, gamma != 1 the focal Tversky loss.  nc <= 1024.
 *   OHEM selects pixels for the base term only.
 * region == 2, the Lovasz-Softmax loss (Berman et al., CVPR 2018), the surrogate of the mean IoU.  weight, base_weight, per_image,
 *   skip_absent and region_class_weight are read as above; alpha, beta, gamma and smooth are ignored.  Groups and valid pixels as above;
 *   the pixel index inside a group is its linear (b, y, x) index.  Per group and class c, over the group's valid pixels:
 *     f = [t == c], e = f ? 1 - p_c : p_c, in fp32 from exp(z_c - lse) (1 - p_c clamped at 0); G_c = sum f (the Y_c of the stats).
 *     For e alone the two interpolation weights of a pixel come from a source coordinate formed in double -- the fp32 coordinate the
 *     rest of the criterion shares with cvx_resize_bilinear_rows_to_nchw puts up to 3e-6 on a logit, and the keys are held to 1e-6 of
 *     float64 --; the gradient's p_k are the shared values.
 *     The pixels are ordered by e descending, ties by ascending pixel index; the order is that of the fp32 bit patterns of e, which are
 *     non-negative and so order as uint32.  Along that order I_k = G_c - #foreground among the first k + 1, U_k = G_c + #background
 *     among the first k + 1, J_k = 1 - I_k / U_k, Delta_k = J_k - J_{k-1} with J_{-1} = 0, and L_c = sum_k e_(k) Delta_k.  With the
 *     state before element k: Delta = 1 / U_prev at a foreground element, I_prev / (U_prev (U_prev + 1)) at a background one; the
 *     first element of a class with G_c = 0 has Delta = 1.  I and U are integers: Delta is exact to one division in double and no
 *     prefix sum is a floating-point sum.
 *     group loss = sum_c m_c v_c L_c / sum_c m_c v_c (0 when that is 0), m_c = [G_c > 0] when skip_absent != 0 (the paper's
 *     classes="present"), else 1 ("all"); lovasz = the mean of the group losses over the G groups; a group without a valid pixel
 *     contributes 0 and still counts.  loss = base_weight * base + weight * lovasz.
 *     Gradient: h_c(pixel) = (1/G) m_c v_c / sum m v * s * Delta_{rank_c(pixel)}, s = -1 where t == c and +1 elsewhere;
 *     d lovasz / d z_k = p_k (h_k - sum_c p_c h_c) at a valid pixel, 0 elsewhere.
 *   The order comes from a segmented, stable radix sort on the device (four 8-bit passes; ranks are ballot counts, never the arrival
 *   order of atomics; kernel boundaries are the only synchronisation between workgroups).  Any bit pattern is a legal key: logits that
 *   are not finite give some order and no store outside the segment.  Classes without a target pixel under skip_absent, and groups
 *   without a valid pixel, are not sorted.  nc <= 1024, a group has fewer than 2^31 pixels, and base_weight fits base as for region 1;
 *   otherwise the entry refuses.  region_stats_out: (G, nc, 4) = 0, 0, Y_c, L_c (L_c = 0 for a class that was not sorted).
 *   cvx_seg_criterion_lovasz_view (host only) writes three byte offsets into the TRAINING workspace: the sorted keys (uint32, the bit
 *   patterns of e), the payload (uint32: the pixel index inside its group in bits 0..30, the foreground flag in bit 31) and the segment
 *   table (G, nc, 2) int64 = element offset into the two arrays and length (the group's valid pixels; 0 for a class that was not
 *   sorted).  They hold the last training call's order until the next call.  The workspace holds two ping-pong buffers of key + payload,
 *   2 * 8 bytes per (pixel, class) in training -- 1.4 GB at batch 16, 513 x 513, 21 classes -- next to the gradient plane's 4;
 *   evaluation (value only: the chain stops at L_c) carries a one-byte payload and no gradient plane: 10 bytes against 20.
 *   Launches: 22 and one memset for the term in training (21 in evaluation), plus the base's and the adjoint.
 * Every floating-point sum runs in a fixed order (per-workgroup trees, then the partials in index order; no floating-point atomics): two
 * calls give the same bits.
 * cvx_seg_criterion_loss: loss_out: 1 float (device).  dpred: (batch, ih*iw, ld) fp16 = loss_scale * dLoss/drows (columns nc..ld-1 zero) --
 *   the operand of cvx_engine_backward.  bad_target: 1 int32 (device), set non-zero when a label is neither ignore_index nor in [0, nc)
 *   (torch raises a device assert there; the pixel is skipped).  stats_out: 4 doubles (device), written by base 2 with options: pixels in
 *   S, valid pixels, theta_min, the denominator sum w_t (may be null otherwise).  region_stats_out: (G, nc, 4) doubles (device),
 *   G = per_image ? batch : 1: I, P, Y, T (may be null without a region term).  Launches: 3 (13 under OHEM), plus 4 for a region term;
 *   5 for a region term alone.
 * cvx_seg_criterion_eval, one validation batch: the arg max of the interpolated logits is taken (the lowest class wins a tie, like
 *   torch.argmax) and confusion[target * nc + argmax] += 1 for targets in [0, nc); other targets are left out, as SegmentationMetrics
 *   does.  confusion: (nc, nc) int64 (device) that ACCUMULATES over calls -- the caller zeroes it.  loss_out: the criterion's value of this
 *   batch over all valid pixels (OHEM is never applied in evaluation; a label that is neither ignore_index nor a class contributes
 *   nothing); with a region term the value-only region chain follows and loss_out holds base_weight * base + weight * region (with
 *   base 0 the pass still counts the matrix).  No gradient and no full-resolution tensor is written.  A workgroup counts in LDS for
 *   nc <= 90 (nc * nc uint32 cells, 32 KB) and adds its non-zero cells to the matrix with 64-bit atomics; larger nc goes to the matrix
 *   directly.
 * workspace: cvx_seg_criterion_workspace_bytes(dims, crit, for_eval) bytes (0: bad arguments).  After a training call with OHEM the fp32
 * keys of that call, (batch, oh, ow) with -1 at pixels that are not valid, start CVX_SEG_OPTS_KEY_OFFSET bytes into it, whatever else
 * the criterion holds.  Asynchronous on hip_stream, no host read.
 * Replaces: F.interpolate + FocalLoss.forward / nn.CrossEntropyLoss + loss.backward() down to the classifier's output,
 * core/trainer/segmentation_trainer.py:121-130; F.interpolate + criterion(preds, targets) + torch.argmax(preds, dim=1) +
 * SegmentationMetrics.add_batch, segmentation_trainer.py:141-150 and core/algorithms/segmentation_2d.py:154-157. */
#define CVX_SEG_OPTS_KEY_OFFSET 4096
#define CVX_SEG_DIMS_BYTES 28
#define CVX_SEG_CRITERION_BYTES 128
typedef struct cvx_seg_dims {
  int32_t ld, batch, nc, ih, iw, oh, ow;
} cvx_seg_dims;
typedef struct cvx_seg_criterion {
  int32_t base; /* 0 none, 1 focal, 2 cross-entropy */
  float focal_alpha, focal_gamma;
  const float* class_weight;
  float label_smoothing;
  int64_t ignore_index;
  float ohem_theta;
  int64_t ohem_min_kept;
  int32_t region; /* 0 none, 1 Dice / Tversky, 2 Lovasz-Softmax */
  double base_weight, weight, alpha, beta, gamma, smooth;
  int32_t per_image, skip_absent;
  const float* region_class_weight;
} cvx_seg_criterion;
int64_t cvx_seg_criterion_workspace_bytes(const cvx_seg_dims* dims, const cvx_seg_criterion* crit, int32_t for_eval);
int cvx_seg_criterion_loss(const float* rows_f32, const cvx_seg_dims* dims, const int64_t* target, const cvx_seg_criterion* crit, float loss_scale,
                           float* loss_out, void* dpred_f16, int32_t* bad_target, double* stats_out, double* region_stats_out, void* workspace,
                           void* hip_stream);
int cvx_seg_criterion_eval(const float* rows_f32, const cvx_seg_dims* dims, const int64_t* target, const cvx_seg_criterion* crit, int64_t* confusion,
                           float* loss_out, double* region_stats_out, void* workspace, void* hip_stream);
int cvx_seg_criterion_lovasz_view(const cvx_seg_dims* dims, const cvx_seg_criterion* crit, int64_t offsets_out[3]);
/* VOC mAP evaluation of a detector (get_map at IoU min_overlap), accumulated on the device batch by batch.
 * cvx_det_match, once per batch: rows (batch, max_det, 6) [x1,y1,x2,y2,score,cls] fp32 and counts (batch) int32 exactly as cvx_nms /
 * cvx_nms_variant write them; a count of -1 (or one past max_det) adds 1 to the overflow counter and the image contributes nothing.
 * box_mode 0: the boxes are final; 1: x -> (x - px) * gx, y -> (y - py) * gy in fp32 with one rounding per operation, box_map (batch, 4)
 * fp32 [px, py, gx, gy] (core/utils/boxes.py:undo_letterbox for both letterbox settings).  Then the coordinates are truncated towards
 * zero, as the writers' int() does.  gt (batch, max_gt, 6) int32 [cls, l, t, r, b, difficult], gt_counts (batch) int32.  quantize != 0:
 * the score becomes what str(float32)[:6] keeps of it (4 decimals; exact for scores in [1e-4, 1]).  One workgroup per image: per
 * detection the ground truth of its class with the largest IoU (+1 pixel convention, integer products and one fp64 division, strict >,
 * first in order wins a tie, difficult boxes included); of the detections that chose one non-difficult ground truth with IoU >=
 * min_overlap the first by (score descending, row ascending) is the TP, the others are FP; a difficult match is neither.  Appends
 * (score fp32, class int32, flag int32: 0 FP, 1 TP, 2 neither) to rec_score / rec_class / rec_flag (capacity records each) in (image, row)
 * order at the device cursor; gt_per_class (nc) int64 counts the non-difficult ground truths.  state: 4 int64 (device), zeroed by the
 * caller before the first batch: [cursor, overflow (NMS overflow, bad counts, no room left), scores below 1e-4, classes outside [0, nc)].
 * max_det <= 16384, max_gt <= 1024.  No host read; asynchronous on hip_stream.
 * cvx_det_ap, once per evaluation, over the records in get_map's order (class ascending, score descending, stable): seg_off (nc + 1)
 * int64 = the first record of each class.  Per class: inclusive scans of TP and FP, rec = tp / max(gt, 1) and prec = tp / max(tp + fp, 1)
 * in fp64 (written to prec / rec, one double per record), voc_ap (suffix maximum, sum over the recall change points) and the values at
 * the last record whose score reaches score_threshold (record 0 when none does).  stats: (nc * 8 + 8) doubles: per class [ap, precision,
 * recall, f1, tp, detections, ground truths, 0], then [mAP over the classes with a ground truth, their number].
 * Replaces: get_map and voc_ap, core/metrics/mAP.py:107-148, 302-834, and the text files the evaluate_on_voc writers exchange with it,
 * core/algorithms/yolo_v8.py:244-326 (yolo_v7.py:94-186, ssd.py:96-188, centernet.py:137-229). */
int cvx_det_match(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                  const int32_t* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc, double min_overlap, int32_t quantize,
                  float* rec_score, int32_t* rec_class, int32_t* rec_flag, int64_t capacity, int64_t* state, int64_t* gt_per_class,
                  void* hip_stream);
int cvx_det_ap(const float* score, const int32_t* flag, const int64_t* seg_off, const int64_t* gt_per_class, int32_t nc,
               double score_threshold, int32_t quantize, double* prec, double* rec, double* stats, void* hip_stream);
/* Diagnostics of a detector beside its VOC mAP (csrc/det_diag.hip).  Additive: CVX_ABI_VERSION stays 6.
 * cvx_det_confusion, once per batch, one launch: rows, counts, box_mode, box_map, gt, gt_counts, nc and quantize exactly as cvx_det_match
 * takes them (max_det <= 16384, max_gt <= 1024), conf in [0, 1] and iou in [0, 1).  The rule is the project's statement of Ultralytics'
 * ConfusionMatrix.process_batch with the ties decided, per image:
 *   take part   a detection whose class lies in [0, nc) and whose score reaches conf: rint(s * 1e4) / 1e4 >= conf in fp64 on the cut score
 *               with quantize, s >= conf without (cvx_det_ap's threshold rule).  The others count nowhere.
 *   overlap     cvx_det_match's, on the boxes mapped and truncated as there (integers, +1 pixel convention, one fp64 division), between a
 *               detection and a ground truth of ANY class; a candidate pair has overlap > iou (strict).
 *   choice      each detection picks its candidate of largest overlap, the lowest ground-truth index on a tie; difficult ground truths are
 *               candidates.  A detection that chose a difficult ground truth counts nowhere.
 *   winner      each non-difficult ground truth keeps, of the detections that chose it, the one of largest overlap, the lowest row on a
 *               tie: confusion[class of the detection][class of the ground truth] += 1.
 *   the rest    every other detection that takes part: confusion[its class][nc] += 1 -- one that lost its ground truth is NOT tried on
 *               its second choice; every non-difficult ground truth without a winner: confusion[nc][its class] += 1.
 * confusion (nc + 1, nc + 1) int64 indexed [predicted][true], nc = background; images_per_class (nc) int64: the images that hold a
 * non-difficult ground truth of the class (the reference's counter_images_per_class); state (4) int64 [images seen, images skipped
 * (a count below 0 or above max_det, a gt_count outside [0, max_gt]: the image contributes nothing), class indices outside [0, nc) of
 * detections or ground truths (the box takes part in nothing), unused].  All three are device memory, zeroed by the caller before the
 * first batch and added to with integer atomics: the same bytes on every run.  No host read; asynchronous on hip_stream.
 * cvx_det_conf_curves, once per evaluation, two launches: score, prec, rec, flag and seg_off as cvx_det_ap takes and leaves them
 * (class ascending, score descending), gt_per_class (nc) of cvx_det_match, images_per_class (nc) of cvx_det_confusion, 2 <= points <= 4096,
 * window odd in 1 .. 65535, ref_points: the nine doubles of numpy's logspace(-2, 0, 9) on the device.  With P = points and x_k =
 * (double)k / (double)(P - 1): n_k = the records of the class that reach x_k (the threshold rule above); precision, recall = prec, rec at
 * record n_k - 1 and F1 = R * P * 2 / (P + R == 0 ? 1 : P + R), or (1, 0, 0) when n_k = 0 -- the operating point at conf_threshold = x_k.
 * mean F1: the sum over the classes with gt_per_class > 0 in ascending class, divided by their number (0 without one).  smooth(y)[i] =
 * (sum over j = 0 .. window - 1, ascending, of y[clamp(i - window / 2 + j, 0, P - 1)]) / window, applied to the mean and to every class's
 * F1; best index = the first maximum of a smoothed curve.  Miss rates: fppi_j = (double)(FP flags among records 0 .. j) / (double)
 * images_per_class; per reference point the last record j with fppi_j <= the point gives 1 - rec[j], 1.0 when there is none or
 * images_per_class is 0 (log_average_miss_rate, core/metrics/mAP.py:34-70, up to its final exp(mean(log(max(1e-10, .)))), the host's).
 * fp64 without contraction throughout.  out: out_words >= 3 * nc * P + 2 * P + 10 * nc + 1 words of 8 bytes: precision (nc, P), recall
 * (nc, P), f1 (nc, P), mean f1 (P), smoothed mean f1 (P), miss rates (nc, 9) as doubles, then the best indices (nc + 1) as int64, the mean
 * curve's last.  No host read; asynchronous on hip_stream. */
int cvx_det_confusion(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                      const int32_t* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc, double conf, double iou, int32_t quantize,
                      int64_t* confusion, int64_t* images_per_class, int64_t* state, void* hip_stream);
int cvx_det_conf_curves(const float* score, const double* prec, const double* rec, const int32_t* flag, const int64_t* seg_off,
                        const int64_t* gt_per_class, const int64_t* images_per_class, int32_t nc, int32_t quantize, int32_t points,
                        int32_t window, const double* ref_points, double* out, int64_t out_words, void* hip_stream);
/* COCO detection metric of a detector (pycocotools' COCOeval(gt, dt, 'bbox'): iouThrs linspace(.5, .95, 10), recThrs linspace(0, 1, 101),
 * maxDets 1 / 10 / 100, areas all / small / medium / large, useCats), accumulated on the device batch by batch.
 * cvx_coco_match, once per batch: rows, counts, box_mode and box_map as cvx_det_match takes them.  truncate != 0: the mapped corners are
 * cut towards zero (the VOC writers' int()); quantize != 0: the score becomes what str(float32)[:6] keeps (cvx_det_match's rule).  Box
 * widths x2 - x1 and y2 - y1 are taken in fp32 and widened; everything after is fp64 without contraction.  gt (batch, max_gt, 7) fp64
 * [cls, x, y, w, h, area, iscrowd], gt_counts (batch) int32.  iou_thrs: the 10 thresholds, fp64 on the device.  One workgroup per image:
 * the rows ordered by (class, score descending, row), each class cut to 100, then evaluateImg's greedy walk for each (class present, area
 * range a, threshold t).  Appends per detection, in (image, row) order at the device cursor: rec_score fp32, rec_class int32, rec_rank int32
 * (place in its (image, class) list; >= 100: not evaluated), rec_matched and rec_ignored int64 (bit a * 10 + t).  npig (nc, 4) int64 counts
 * the ground truths that are neither crowd nor outside the area range.  state: 4 int64 (device), zeroed by the caller: [cursor, overflow
 * (NMS overflow, bad counts, no room left), unusable scores (below 1e-4 when quantize, negative or NaN otherwise), classes outside
 * [0, nc)].  max_det <= 16384 and max_gt <= 1024, together within the 160 KB LDS.  No host read; asynchronous on hip_stream.
 * cvx_coco_accumulate, once per evaluation, over the records in (class ascending, score descending, stable) order: rank, matched, ignored
 * in that order, seg_off (nc + 1) int64 = the first record of each class, rec_thrs: the 101 recall thresholds, fp64 on the device.  One
 * workgroup per (class, area, maxDet): precision (10, 101, nc, 4, 3) and recall (10, nc, 4, 3) fp64, -1 where the class has no counted
 * ground truth in the area range.
 * cvx_coco_summarize: stats (12) fp64 = AP, AP50, AP75, APs, APm, APl (maxDets 100), AR1, AR10, AR100, ARs, ARm, ARl: means over the
 * entries > -1 (-1 when there is none), summed in a fixed order.
 * Replaces: COCOeval.evaluate / accumulate / summarize as core/metrics/mAP.py:930-959 (get_coco_map) and the detectors' evaluate_on_coco
 * (core/algorithms/yolo_v8.py:330-381) call them, and the JSON files they exchange. */
int cvx_coco_match(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                   int32_t truncate, int32_t quantize, const double* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc,
                   const double* iou_thrs, float* rec_score, int32_t* rec_class, int32_t* rec_rank, int64_t* rec_matched, int64_t* rec_ignored,
                   int64_t capacity, int64_t* state, int64_t* npig, void* hip_stream);
int cvx_coco_accumulate(const int32_t* rank, const int64_t* matched, const int64_t* ignored, const int64_t* seg_off, const int64_t* npig,
                        int32_t nc, const double* rec_thrs, double* precision, double* recall, void* hip_stream);
int cvx_coco_summarize(const double* precision, const double* recall, int32_t nc, double* stats, void* hip_stream);
/* CenterNet's CombinedLoss with its gradient.  rows: the engine's fp32 head rows (batch, anchors = h*w, ld): heat-map logits in columns
 * [0, nc), the loss's "reg" pair at columns col_a, col_a+1 (= the model output's columns nc, nc+1) and its "wh" pair at col_b, col_b+1 (= the
 * output's last two) -- the reference's loss names are swapped against the heads that produce them, reproduced as is.  Targets as
 * centernet_collate builds them: heat_true (batch, h, w, nc) fp32, true_a / true_b (batch, K, 2), mask (batch, K) fp32, indices (batch, K)
 * int64 = y*w + x.  loss_items: 4 floats (device): total, heat-map focal, L1(a), L1(b) (unweighted).  dpred: (batch, anchors, ld) fp16 =
 * loss_scale * dLoss/drows.  bad_index: set non-zero when a masked object's index lies outside [0, anchors).  Asynchronous on hip_stream.
 * Replaces: CombinedLoss.__call__ + loss.backward() down to the head outputs, core/loss/centernet_loss.py:5-67,
 * core/trainer/centernet_train.py:104-118. */
int64_t cvx_centernet_loss_workspace_bytes(int32_t batch, int32_t anchors);
int cvx_centernet_loss(const float* rows_f32, int32_t ld, int32_t batch, int32_t anchors, int32_t nc, int32_t col_a, int32_t col_b,
                       const float* heat_true, const float* true_a, const float* true_b, const float* mask, const int64_t* indices,
                       int32_t max_objects, float hm_weight, float a_weight, float b_weight, float loss_scale, float* loss_items, void* dpred_f16,
                       int32_t* bad_index, void* workspace, void* hip_stream);
/* SSD's MultiBoxLossV2 with its gradient.  loc (batch, anchors, 4) and conf (batch, anchors, nc1 = num_classes + 1) fp32 as the model
 * returns them; y_true (batch, anchors, 4 + nc1 + 1) fp32 as ssd_collate encodes it: box targets, one-hot class incl. background, positive
 * flag.  Softmax cross-entropy (probabilities clamped at 1e-7) on the positives and on the k hardest negatives of the WHOLE batch
 * (k = sum over images of min(ratio * num_pos, anchors - num_pos), 100 when no image has a positive; hardness = sum of the non-background
 * probabilities), smooth-L1 on the positives, total = (1 - alpha) * conf + alpha * loc with both sums divided by sum(num_pos or 1).  The
 * top-k is a radix SELECT (no sort); keys equal to the k-th are taken in flat-index order (torch.topk leaves that choice open).
 * loss_items: 3 floats (device): total, loc, conf.  dloc / dconf: grad_scale * dLoss/d(loc, conf), fp32, same shapes.  Asynchronous.
 * Replaces: MultiBoxLossV2.__call__ + loss.backward() down to the model outputs, core/loss/multi_box_loss.py:77-192. */
int64_t cvx_multibox_loss_workspace_bytes(int32_t batch, int32_t anchors);
int cvx_multibox_loss(const float* loc, const float* conf, const float* y_true, int32_t batch, int32_t anchors, int32_t nc1, float neg_pos_ratio,
                      float alpha, float grad_scale, float* loss_items, float* dloc, float* dconf, void* workspace, void* hip_stream);
/* YOLOv7's loss (Yolo7Loss) with its gradient.  rows: the engine's fp32 head rows (batch, anchors, ld): level l (coarsest first, level_hw =
 * {h0, w0, h1, w1, h2, w2}) occupies rows a_off_l .. + h_l*w_l in (gj, gi) order, anchor a of a cell in columns a*(5+nc) .. : x, y, w, h,
 * objectness, classes.  anchors_px: 9 (w, h) pairs in pixels, level-major (the reference's anchors[anchors_mask[l]]); strides {32, 16, 8};
 * targets: (n_targets, 6) fp32 [image, class, cx, cy, w, h] normalised; img_size = imgs[b].shape[1] (the reference scales all four
 * coordinates by it).  Candidate generation (find_3_positive), SimOTA assignment per image (build_targets: dynamic k = int(sum of the
 * top-20 IoUs) >= 1, the k cheapest candidates, conflicts to the cheapest ground truth) and the CIoU / objectness / class terms all run on
 * the device.  loss_items: 4 floats: total, box * box_ratio, obj * obj_ratio, cls * cls_ratio.  dpred: (batch, anchors, ld) fp16 =
 * loss_scale * dLoss/drows.  bad: bit 0 = more than 64 ground truths in an image, bit 1 = more than 2880 candidates (both truncated).
 * Replaces: Yolo7Loss.__call__ + loss.backward() down to the head outputs, core/loss/yolo7_loss.py:14-444. */
int64_t cvx_yolo7_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t ld, int32_t n_targets);
int cvx_yolo7_loss(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, const int32_t* level_hw, const float* anchors_px, const float* strides,
                   const float* targets, int32_t n_targets, float img_size, float box_ratio, float obj_ratio, float cls_ratio, float label_smoothing,
                   float loss_scale, float* loss_items, void* dpred_f16, int32_t* bad, void* workspace, void* hip_stream);
/* Test hook, host only (launches nothing): where cvx_yolo7_loss keeps its assignment inside a workspace of
 * cvx_yolo7_loss_workspace_bytes(batch, anchors, ld, n_targets) bytes, from the launcher's own layout function.  offsets[0..3] = byte
 * offsets of: the candidate lists, int32 [3 levels][cap][5] = image, anchor, gj, gi, target row, in list order; the matched lists, int32
 * [3 levels][batch][cmax][4] = anchor, gj, gi, target row, in list order; their lengths, int32 [batch][3]; the state block, whose first
 * seven int32 are the candidate count per level, the matched count per level and the overflow bits.  offsets[4] = cap (candidate slots
 * per level), offsets[5] = cmax (2880).  Returns 0, or -1 on bad arguments.  (No reference counterpart: find_3_positive / build_targets
 * return their lists as Python objects, core/loss/yolo7_loss.py:129-398.) */
int cvx_debug_yolo7_loss_layout(int32_t batch, int32_t anchors, int32_t ld, int32_t n_targets, int64_t* offsets);
/* CenterNet target drawing on the device: what centernet_collate does per image on the CPU.  labels: (batch, max_boxes, 5) fp32 rows
 * [class id, cx, cy, w, h] (normalised), counts (batch) valid rows (<= max_boxes = cfg.train.max_num_boxes).  Outputs in the reference's
 * formats: heatmap (batch, fh, fw, nc) -- per object a (2r+1)^2 Gaussian, r the CornerNet radius of its integer size, merged by maximum;
 * reg (batch, max_boxes, 2) = fractional part of the centre; wh = integer (w, h); reg_mask; indices = y*fw + x as float32.  Asynchronous.
 * Replaces: CenterNet.generate_targets, core/algorithms/centernet.py:66-112 + core/utils/gaussian.py:5-57 (called from collate.py:52-68). */
int cvx_centernet_draw_targets(const float* labels, const int32_t* counts, int32_t batch, int32_t max_boxes, int32_t fh, int32_t fw, int32_t nc,
                               float* heatmap, float* reg, float* wh, float* reg_mask, float* indices, void* hip_stream);
/* SSD target encoding on the device: what ssd_collate does per image on the CPU.  labels: (batch, max_boxes, 5) fp32 rows
 * [class id (0-based), cx, cy, w, h] (normalised), counts (batch) valid rows per image; priors (anchors, 4) fp32 corner boxes
 * (Ssd._get_ssd_anchors).  y_true: (batch, anchors, 4 + nc1 + 1) fp32: encoded box | one-hot class incl. the background column 0 | positive
 * flag -- the input of cvx_multibox_loss.  workspace: batch * max_boxes int32.  Asynchronous on hip_stream.
 * Replaces: Ssd.generate_targets + _encode_box, core/algorithms/ssd.py:327-480 (called from core/data/collate.py:32-49). */
int cvx_ssd_encode_targets(const float* labels, const int32_t* counts, int32_t batch, int32_t max_boxes, const float* priors, int32_t anchors, int32_t nc1,
                           float overlap_threshold, float variance_xy, float variance_wh, float* y_true, int32_t* workspace, void* hip_stream);
/* Adjoint of cvx_resize_bilinear_rows_to_nchw: a gradient w.r.t. the full-resolution logits (batch, nc, oh, ow) fp32 -> scale * the
 * gradient w.r.t. the rows (batch, ih*iw, ld) fp16 (a deterministic gather).  For callers that compute their own loss on the
 * model's NCHW output.  Asynchronous on hip_stream. */
int cvx_resize_bilinear_nchw_grad_to_rows(const float* grad_nchw, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                          float scale, void* dpred_f16, int32_t ld, void* hip_stream);
/* Training forms of the ResNet / DeepLab pooling and resampling ops (dense NHWC fp16; they synchronise before returning):
 *   cvx_maxpool3_train_nhwc: the 3x3 / pad 1 / stride 1 | 2 max pool that also stores `argmax` (one byte per OUTPUT element, the
 *     window tap dy*3+dx of the first maximum in row-major scan order = torch's choice); cvx_maxpool3_bwd_nhwc routes gout through it
 *     (resnet.py:163 + autograd);
 *   cvx_avgpool_global_bwd_nhwc: gin (+)= gout / hw on every pixel (deeplabv3plus.py:30);
 *   cvx_resize_bilinear_bwd_nhwc: the adjoint of cvx_resize_bilinear_nhwc (align_corners = False) as a deterministic gather
 *     (deeplabv3plus.py:38,117-122);
 *   cvx_dropout_nhwc: inverted dropout, out (+)= keep ? x / (1 - p) : 0, the mask a counter-based hash of (seed, element index) --
 *     the same call with the same seed on the output gradient is its backward (deeplabv3plus.py:67).  The mask is NOT torch's
 *     Philox sample: same distribution, different draw.
 * accumulate != 0 adds onto the existing contents of the gradient tensor. */
int cvx_maxpool3_train_nhwc(const void* x_f16, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride, void* out_f16, uint8_t* argmax,
                            void* hip_stream);
int cvx_maxpool3_bwd_nhwc(const void* gout_f16, const uint8_t* argmax, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride,
                          void* gin_f16, int32_t accumulate, void* hip_stream);
int cvx_avgpool_global_bwd_nhwc(const void* gout_f16, int32_t batch, int32_t hw, int32_t c, void* gin_f16, int32_t accumulate, void* hip_stream);
/* Gradient of cvx_l2norm_nhwc (L2Normalize, ssd_model.py:113-128): gin (+)= w*g/(n+eps) - x*(sum_c w g x)/(n (n+eps)^2), and
 * dweight[c] += inv_scale * sum over pixels of g*x/(n+eps) (fixed summation order).  c <= 512. */
int cvx_l2norm_bwd_nhwc(const void* x_f16, const void* gout_f16, const float* weight, int32_t batch, int32_t hw, int32_t c, float inv_scale,
                        void* gin_f16, float* dweight, int32_t accumulate, void* hip_stream);
/* Adjoint of cvx_pred_cols_to_nchw: a gradient laid out like its output (element (b, ch, pix) at grad[b*grad_bstride + grad_off + ch*hw + pix]:
 * SSD's NCHW-order flattening, ssd_model.py:177-183) -> scale * gradient in fp16 on columns [col0, col0 + c) of rows a_off .. a_off + hw. */
int cvx_nchw_cols_grad_to_pred(const float* grad, int64_t grad_bstride, int64_t grad_off, int32_t c, int32_t batch, int32_t anchors, int32_t a_off,
                               int32_t hw, float scale, void* dpred_f16, int32_t ld, int32_t col0, void* hip_stream);
/* Gradient of the 2x2 stride-2 max pool of cvx_maxpool_nhwc (floor or ceil mode): x is the forward input, the first maximum of each
 * window in row-major scan order takes the gradient (torch's rule).  Replaces: nn.MaxPool2d(2, 2) autograd (yolov7_model.py:74-86). */
int cvx_maxpool2_bwd_nhwc(const void* x_f16, const void* gout_f16, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t ceil_mode,
                          void* gin_f16, int32_t accumulate, void* hip_stream);
/* Depthwise ConvTranspose2d of CenterNet's IDAUp.up_i (kernel 2f, stride f, padding f/2, groups = c, no bias; centernet_model.py:256) on a dense
 * NHWC fp16 tensor, and its gradients: gin (+)= data gradient, dweight[c][2f][2f] += inv_scale * weight gradient (fp32, deterministic).
 * weight: fp32 [c][2f][2f] (the master tensor).  Replaces: nn.ConvTranspose2d forward + autograd. */
int cvx_dwconvt_nhwc(const void* x_f16, int32_t batch, int32_t ih, int32_t iw, int32_t c, int32_t f, const float* weight, void* out_f16,
                     void* hip_stream);
int cvx_dwconvt_bwd_nhwc(const void* x_f16, const void* gout_f16, int32_t batch, int32_t ih, int32_t iw, int32_t c, int32_t f, const float* weight,
                         void* gin_f16, int32_t accumulate, float* dweight, float inv_scale, void* hip_stream);
int cvx_resize_bilinear_bwd_nhwc(const void* gout_f16, int32_t batch, int32_t ih, int32_t iw, int32_t c, int32_t oh, int32_t ow, void* gin_f16,
                                 int32_t accumulate, void* hip_stream);
int cvx_dropout_nhwc(const void* x_f16, int32_t batch, int32_t hw, int32_t c, float p, uint64_t seed, void* out_f16, int32_t accumulate,
                     void* hip_stream);

/* nearest-neighbour x2 upsample (nn.Upsample(scale_factor=2), core/models/yolov8/yolo_v8.py:39,41) and its backward */
int cvx_upsample2_nhwc(const void* x_f16, int32_t batch, int32_t h, int32_t w, int32_t c, void* out_f16, void* hip_stream);
int cvx_upsample2_bwd_nhwc(const void* gout_f16, int32_t batch, int32_t h, int32_t w, int32_t c, void* gin_f16, int32_t accumulate,
                           void* hip_stream);
/* The stem (model.0: Conv(3, c, 3, 2), core/models/yolov8/yolo_v8.py:28) in fp32 from NCHW fp32 images: weight fp32
 * [cout][kh][kw][ci]; train = batch statistics + running update, eval = folded scale / shift; wgrad: dw [cout][3][3][3]
 * (overwritten) from dy fp16 (B, h/2, w/2, cout). */
int cvx_stem_train_nchw(const float* images, int32_t batch, int32_t h, int32_t w, const float* weight, int32_t cout, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean, float* running_var, void* out_f16,
                        void* xhat_f16, float* mean, float* invstd, void* hip_stream);
int cvx_stem_eval_nchw(const float* images, int32_t batch, int32_t h, int32_t w, const float* weight, int32_t cout, const float* scale,
                       const float* shift, void* out_f16, void* hip_stream);
int cvx_stem_wgrad_nchw(const float* images, int32_t batch, int32_t h, int32_t w, const void* dy_f16, int32_t cout, float* dw,
                        void* hip_stream);
/* The stem's backward pass as the engine runs it: BatchNorm + SiLU backward fused with the weight gradient (the gradient of
 * the raw conv output is formed in registers and never stored).  gout: gradient w.r.t. the stem's activation, fp16
 * (B, h/2, w/2, cout); xhat / invstd from cvx_stem_train_nchw; dgamma / dbeta accumulated, dw [cout][3][3][3] overwritten,
 * all scaled by inv_scale. */
int cvx_stem_backward_nchw(const float* images, int32_t batch, int32_t h, int32_t w, const void* xhat_f16, const void* gout_f16, int32_t cout,
                           const float* gamma, const float* beta, const float* invstd, float inv_scale, float* dgamma, float* dbeta, float* dw,
                           void* hip_stream);
/* The same pass where the engine keeps no xhat (round 5; images with 16-byte granular rows, >= 2 pixel splits: every YOLOv8 training shape): the
 * kernel recomputes the conv output from the images and `weight` ([cout][3][3][3] fp32, as cvx_stem_train_nchw takes it) and normalises it with the
 * forward's batch mean / invstd (cvx_stem_train_nchw's outputs),
 * and the BatchNorm-backward sums come out of the same pass (no reduction over gout beforehand).  Fails with an error on shapes the one-pass
 * kernel does not take (the engine falls back to cvx_stem_backward_nchw's route there). */
int cvx_stem_backward_recompute_nchw(const float* images, int32_t batch, int32_t h, int32_t w, const float* weight, const void* gout_f16, int32_t cout,
                                     const float* gamma, const float* beta, const float* mean, const float* invstd, float inv_scale,
                                     float* dgamma, float* dbeta, float* dw, void* hip_stream);

/* ---- device-side detection training augmentation (csrc/augment.hip) ------------------------------------------------------------------
 * One job per source picture: 1 per plain output, 4 per mosaic output (quad 0 top-left, 1 bottom-left, 2 bottom-right, 3 top-right;
 * quad = -1 marks a plain job).  src: uint8 HWC (ih, iw, 3) in device memory, resized to (nh, nw) with OpenCV's INTER_CUBIC in its
 * uint8 fixed-point form and pasted at (dx, dy) on a canvas of 128 with cv2_paste's clipping (dx / dy may be negative, the picture may
 * overhang).  flip: plain jobs mirror the CANVAS after the paste, mosaic jobs mirror the SOURCE before the resize.  out: index of the
 * output image; [x0, x1) x [y0, y1): the part of that output this job fills (the whole image for a plain job, its quadrant for a
 * mosaic job).  64 bytes. */
typedef struct cvx_aug_job {
  const uint8_t* src;
  int32_t ih, iw, nh, nw, dx, dy, flip, out, x0, y0, x1, y1, quad, reserved;
} cvx_aug_job;
/* The image half, one launch for the whole batch, asynchronous on hip_stream.  job_start: (batch + 1) int32, jobs
 * job_start[b] .. job_start[b+1] belong to output b (1 or 4 of them); luts: (batch, 3, 256) uint8, the hue / saturation / value tables;
 * out_nchw: (batch, 3, H, W) fp32.  Per pixel: paste + bicubic tap -> RGB2HSV (OpenCV's 8-bit integer form) -> the three LUTs -> HSV2RGB
 * (OpenCV's float form, bytes by round-half-even) -> byte / 255.  All tables are device memory.
 * Replaces: DetectionDataset.get_random_data's image half (core/data/detection_dataset.py:180-205), mosaic_body's (:245-268) and the
 * composition + colour transform of mosaic_for_voc / mosaic_for_coco (:321-341), cv2_paste (core/utils/image_process.py:132-158),
 * TF.to_tensor (detection_dataset.py:101) and the torch.stack of yolo7_collate / yolo8_collate (core/data/collate.py:12,24). */
int cvx_aug_images(const cvx_aug_job* jobs, const int32_t* job_start, const uint8_t* luts, int32_t batch, float* out_nchw, int32_t H, int32_t W,
                   void* hip_stream);
/* The box half, one launch, asynchronous.  boxes: (n_boxes, 5) fp32 rows (x1, y1, x2, y2, cls) in source pixels, job after job;
 * job_box_start: (n_jobs + 1) int32, the rows of job j are job_box_start[j] .. job_box_start[j+1].  In fp32 and the reference's operation
 * order (no fused multiply-add): x * nw / iw + dx, the flip, the clamps to the output, keep w > 1 && h > 1, for mosaic jobs merge_bboxes
 * against the cuts (taken from the job's rect), then / W, / H and (cx, cy, w, h).  targets: (n_boxes, 6) fp32 rows
 * [image, cls, cx, cy, w, h]; the kept boxes in source order (a scan, not atomics) fill rows 0 .. *count, the rest get image = -1;
 * count: 1 int32 (device).  The reference's np.random.shuffle of the boxes is not reproduced, and a mosaic source's width is its
 * column count (the reference reads rows first, :224).
 * Replaces: the box halves of get_random_data (:207-218) and mosaic_body (:228-231,270-287), merge_bboxes (:405-449), the label
 * normalisation of __getitem__ (:100-130) and the image-index column + concatenation of the collate functions (collate.py:8-13,20-23). */
int cvx_aug_boxes(const cvx_aug_job* jobs, const int32_t* job_box_start, int32_t n_jobs, const float* boxes, int32_t n_boxes, int32_t H, int32_t W,
                  float* targets, int32_t* count, void* hip_stream);
/* The image half without the colour transform: paste + bicubic tap -> byte / 255, what DetectionDataset(train=False) composes
 * (get_random_data(random=False), detection_dataset.py:137-150; there is no flip and no HSV step, and RGB -> HSV -> RGB would not be the
 * identity in 8 bits).  Same jobs, job_start and output as cvx_aug_images, no tables.  A sibling entry point rather than a flag in
 * cvx_aug_job.reserved: it is a second instance of the same kernel template, so the colour instance keeps its code (csrc/augment.hip). */
int cvx_aug_images_plain(const cvx_aug_job* jobs, const int32_t* job_start, int32_t batch, float* out_nchw, int32_t H, int32_t W, void* hip_stream);
/* The box half with per-image output, for the target kernels that take padded labels (cvx_ssd_encode_targets,
 * cvx_centernet_draw_targets): one workgroup per output image, asynchronous.  jobs, job_box_start, boxes as for cvx_aug_boxes; job_start
 * (batch + 1) int32 as for cvx_aug_images.  labels: (batch, max_boxes, 5) fp32 rows [cls, cx, cy, w, h], the kept boxes of image b in
 * source order from row 0, unused rows zero; counts: (batch) int32 = min(kept, max_boxes); overflow: 1 int32 (device), cleared on the
 * stream first and set non-zero when any image kept more than max_boxes (its first max_boxes boxes survive).  The arithmetic is the device
 * function cvx_aug_boxes uses, so the rows of image b are bit-identical to cvx_aug_boxes' rows with image index b. */
int cvx_aug_boxes_padded(const cvx_aug_job* jobs, const int32_t* job_start, const int32_t* job_box_start, int32_t batch, const float* boxes,
                         int32_t n_boxes, int32_t H, int32_t W, int32_t max_boxes, float* labels, int32_t* counts, int32_t* overflow, void* hip_stream);
/* Stage 2 of the training augmentation: a random affine / perspective warp of every canvas and MixUp inside the
 * batch, behind the launches above, which then write into scratch.  One view per output image b, in device memory.  m: the matrix M
 * (row-major, canvas pixel -> output pixel) of canvas b; inv: its inverse (inverted in float64 on the host, then rounded); s: the zoom
 * drawn for M, used by the area test of the boxes; partner: the output whose warped canvas is mixed into output b, or -1; r, r1: the
 * weights of the own and the partner's canvas (r1 = 1 - r in fp32, taken on the host).  96 bytes. */
typedef struct cvx_aug_view {
  float m[9], inv[9], s;
  int32_t partner;
  float r, r1;
  int32_t reserved[2];
} cvx_aug_view;
/* The image half of stage 2, one launch, asynchronous.  canvases: (batch, 3, H, W) fp32, what cvx_aug_images / cvx_aug_images_plain wrote;
 * out_nchw: the final batch, same shape, another buffer.  Output pixel (x, y), integer coordinates without a half-pixel shift (as
 * cv2.warpPerspective): (u', v', w) = inv . (x, y, 1), u = u' / w, v = v' / w (always divided), x0 = floor(u), lx = u - x0, likewise y,
 * the four taps mixed bilinearly, a tap outside the canvas being the canvas grey 128 / 255.  With a partner p (0 <= p < batch):
 * out_b = warp_b(canvas_b) * r + warp_p(canvas_p) * r1, each canvas through its own matrix.  Every fp32 operation is rounded on its own,
 * in the order written at the head of the stage-2 part of csrc/augment.hip; the identity matrix returns the canvas bit for bit.
 * Modelled on YOLOv5's random_perspective (cv2.warpPerspective, borderValue 114 there) and mixup; the reference has neither. */
int cvx_aug_warp_mix(const float* canvases, const cvx_aug_view* views, int32_t batch, float* out_nchw, int32_t H, int32_t W, void* hip_stream);
/* The box half of stage 2, one launch, asynchronous.  labels_in (batch, cap_in, 5) / counts_in (batch): what cvx_aug_boxes_padded wrote
 * for the canvases.  A label goes back to pixel corners, its four corners through m with the divide, the new box is their min / max
 * clipped to [0, W] x [0, H]; it is kept iff w2 > min_wh, h2 > min_wh, w2 h2 / (w1 s h1 s) > min_area_ratio and
 * max(w2 / h2, h2 / w2) < max_aspect (YOLOv5's box_candidates without its epsilon).  Output b carries the kept boxes of its own canvas in
 * stage-1 order, then those of its partner's canvas (through the partner's own view), ordered by a scan, no atomics.
 * compact != 0 (one workgroup): out (cap_out, 6) rows [image, cls, cx, cy, w, h] in image order from row 0, the other rows with
 * image = -1; counts: 1 int32, the number of rows; overflow is not touched.
 * compact == 0 (one workgroup per output): out (batch, cap_out, 5), zero rows after the kept ones; counts (batch) = min(kept, cap_out);
 * overflow: 1 int32, cleared on the stream first, non-zero when an output kept more than cap_out (its first cap_out survive) -- the form
 * cvx_ssd_encode_targets / cvx_centernet_draw_targets read in place. */
int cvx_aug_boxes_warp(const float* labels_in, const int32_t* counts_in, int32_t cap_in, const cvx_aug_view* views, int32_t batch, int32_t H,
                       int32_t W, float min_wh, float min_area_ratio, float max_aspect, int32_t compact, float* out, int32_t cap_out,
                       int32_t* counts, int32_t* overflow, void* hip_stream);

/* ---- device-side segmentation input pipeline (csrc/seg_pipeline.hip) ------------------------------------------------------------------
 * One job per output image.  image: uint8 HWC (ih, iw, 3) in device memory; mask: its label picture, uint8 (ih, iw, 3) colour coded
 * (mask_channels = 3) or uint8 (ih, iw) class indices (mask_channels = 1).  (rh, rw): the size the reference's Resize gives the picture;
 * (i, j): the crop origin (row, column) inside it, 0 <= i <= rh - H, 0 <= j <= rw - W; flip: mirror the crop.  Validation is a job with
 * (rh, rw) = (H, W), i = j = flip = 0.  64 bytes. */
typedef struct cvx_seg_job {
  const uint8_t* image;
  const uint8_t* mask;
  int32_t ih, iw, rh, rw, i, j, flip, mask_channels, reserved[4];
} cvx_seg_job;
/* One launch for the whole batch, asynchronous on hip_stream.  jobs: (batch) in device memory; colours: (n_colours, 3) uint8 in device
 * memory, the colour of class k in row k (n_colours <= 256; not read for index masks); mean3 / std3: 3 HOST floats each (passed by
 * value to the kernel).  out_nchw: (batch, 3, H, W) fp32 = (bilinear resize of byte / 255 - mean) / std; targets: (batch, H, W) int64.
 * No resized intermediate is stored: an output pixel maps back through flip and crop to the resized picture and on to the four taps of
 * the source, with torch's fp32 coordinate arithmetic (align_corners = False, no antialiasing).  label_mode 0: the taps' class indices are
 * mixed as floats and rounded half to even (what torchvision's F.resize does to an integer tensor; the reference's behaviour); 1: nearest
 * (floor(dst * in / out)).  A colour that is not in the table is class 0, as in the reference's 2^24-entry table.
 * Replaces: ToTensor, RGB2idx / label_indices, Resize, RandomCrop (the crop itself), RandomHorizontalFlip (the mirror itself), Normalize and
 * the DataLoader's default collate, core/data/segmentation_dataset.py:70-198,256-293. */
int cvx_seg_pipeline(const cvx_seg_job* jobs, int32_t batch, const uint8_t* colours, int32_t n_colours, int32_t label_mode, const float* mean3,
                     const float* std3, float* out_nchw, int64_t* targets, int32_t H, int32_t W, void* hip_stream);

/* The training recipe on top of it: zoom, rotation, padding, photometric distortion and Gaussian blur, one job per output image.  The
 * first 48 bytes are cvx_seg_job's fields up to mask_channels; (rh, rw) is the size after Resize(base) AND the zoom, and the origin (i, j)
 * may be negative or exceed rh - H / rw - W: what lies outside the picture is padding.  cos / sin: the rotation about the crop's centre,
 * rounded to fp32 by the host.  flags: CVX_SEG_AUG_* bits; beta (added, in [0, 1] units), alpha (contrast factor), sat (saturation
 * factor), hue (degrees, |hue| <= 360) are read only when their bit is set.  blur_k: 0, 3, 5, 7 or 9 taps, read when CVX_SEG_AUG_BLUR is
 * set; taps[t], t < blur_k.  128 bytes. */
#define CVX_SEG_AUG_BRIGHTNESS 1
#define CVX_SEG_AUG_CONTRAST 2
#define CVX_SEG_AUG_CONTRAST_LAST 4 /* contrast after the HSV step instead of before it */
#define CVX_SEG_AUG_SATURATION 8
#define CVX_SEG_AUG_HUE 16
#define CVX_SEG_AUG_BLUR 32
typedef struct cvx_seg_aug_job {
  const uint8_t* image;
  const uint8_t* mask;
  int32_t ih, iw, rh, rw, i, j, flip, mask_channels;
  float cos, sin;
  int32_t flags;
  float beta, alpha, sat, hue;
  int32_t blur_k;
  float taps[9];
  int32_t reserved[3];
} cvx_seg_aug_job;
/* One launch for the whole batch, asynchronous on hip_stream; jobs, colours, mean3, std3, out_nchw, targets, label_mode as
 * cvx_seg_pipeline; fill3: 3 HOST floats, the padding colour in 0 ... 255.  Every fp32 operation below is rounded on its own, in the
 * order written.  Per output pixel (x, y):
 *  1. geometry: x' = flip ? W - 1 - x : x; px = (x' + 0.5) - W/2, py = (y + 0.5) - H/2; u = ((cos px + sin py) + W/2) + j,
 *     v = ((cos py - sin px) + H/2) + i: the continuous coordinate in the resized picture; inside iff 0 <= u < rw and 0 <= v < rh.
 *     Source coordinate max((iw / rw) u - 0.5, 0), taps and clamps as cvx_seg_pipeline; nearest is floor((u - 0.5) (iw / rw)) clamped to
 *     [0, iw - 1].  With cos = 1, sin = 0 u is the half-integer x' + j + 0.5, so a job without rotation, colour, blur and padding gives
 *     cvx_seg_pipeline's result bit for bit.
 *  2. outside: the image takes fill[c] / 255, the target ignore_index.
 *  3. photometric, on inside pixels only, on the [0, 1] value after the bilinear mix, each only when its bit is set: clip(v + beta);
 *     clip(v alpha) here unless CONTRAST_LAST; the hexcone HSV step when SATURATION or HUE is set (mx / mn = max / min of r, g, b,
 *     d = mx - mn, S = mx > 0 ? d / mx : 0; H = 0 if d = 0, else 60 ((g - b) / d) (+ 360 if negative) when mx = r, else
 *     60 ((b - r) / d) + 120 when mx = g, else 60 ((r - g) / d) + 240; S = clip(S sat); H = H + hue, - 360 if >= 360, then + 360 if
 *     < 0; hh = H / 60, sector = int(hh), f = hh - sector, sector 6 counts as 0; p = mx (1 - S), q = mx (1 - S f),
 *     t = mx (1 - S (1 - f)); (r, g, b) = (mx,t,p) (q,mx,p) (p,mx,t) (p,q,mx) (t,p,mx) (mx,p,q) for sectors 0 ... 5); clip(v alpha) here
 *     when CONTRAST_LAST.  clip is to [0, 1].
 *  4. blur (BLUR set, blur_k = 2 r + 1): horizontal pass sum_t taps[t] c(x + t - r, y), then the vertical pass over its results, both
 *     accumulated in tap order from the first product.  c beyond the crop's edge is what steps 1-3 give at that position of the
 *     extended plane, not a reflection.
 *  5. out = (c - mean) / std.  Targets come from steps 1-2 alone and follow label_mode.
 * unlisted_mode 0: a mask colour that is not in the table is class 0; 1: it is ignore_index (label_mode 1 only: an ignore value
 * cannot be mixed as a float).  32 x 16 output pixels per workgroup; a blurred image holds the tile with its halo and the horizontal
 * pass in LDS (20736 bytes), an image without blur does not touch it.
 * The reference has no such stage (its transforms end at RandomHorizontalFlip, core/data/segmentation_dataset.py:268-273). */
int cvx_seg_pipeline_aug(const cvx_seg_aug_job* jobs, int32_t batch, const uint8_t* colours, int32_t n_colours, int32_t label_mode,
                         int32_t unlisted_mode, int32_t ignore_index, const float* fill3, const float* mean3, const float* std3,
                         float* out_nchw, int64_t* targets, int32_t H, int32_t W, void* hip_stream);

/* ---- data-parallel gradient exchange over RCCL (csrc/comm.hip), SURVEY.md section 8(b) / 8(e) --------------------------------------
 * One process per GPU.  Rank 0 calls cvx_comm_unique_id (128 bytes, ncclGetUniqueId), ships them to every rank by any means, all ranks
 * call cvx_comm_create (ncclCommInitRank; RCCL is dlopen'ed on first use).  `comm` below is the ncclComm_t.
 * cvx_allreduce_grads: SUM all-reduce of the engine's whole flat gradient arena on `hip_stream` (after cvx_engine_backward).
 * cvx_engine_backward_exchange: the overlapped form, the whole data-parallel backward pass in one call -- `buckets` holds n_buckets rows
 *   (op_hi, op_lo, p_start, p_end), op ranges in backward order with their slice of the gradient arena (graph.grad_buckets); each range
 *   is queued on the engine's stream, `comm_stream` waits for it, folds its weight-gradient slabs and all-reduces its slice while the next
 *   range runs; on return the engine's stream waits for the last exchange.  The mean's 1/world belongs to the optimiser step.
 * The reference has no distributed path; north_star: RCCL all-reduce of gradients overlapped with the backward pass. */
int cvx_comm_unique_id(void* out128);
int cvx_comm_create(void** comm, const void* unique_id128, int32_t rank, int32_t world, int32_t device);
int cvx_comm_destroy(void* comm);
int cvx_allreduce_f32(float* data, int64_t count, void* comm, void* hip_stream);
int cvx_allreduce_grads(cvx_engine* e, void* comm, void* hip_stream);
int cvx_engine_backward_exchange(cvx_engine* e, const void* dpred_f16, float loss_scale, void* comm, const int64_t* buckets, int32_t n_buckets,
                                 void* comm_stream);

/* ---- output side of batched prediction (csrc/render.hip) ------------------------------------------------------------------------------
 * All three entries are one launch, asynchronous on hip_stream, and read nothing back.  A frame is a uint8 HWC picture in device memory
 * with its own size and row stride in bytes (stride >= 3 * w); the frames of a batch may differ.  24 bytes per job. */
typedef struct cvx_frame_job {
  uint8_t* data;
  int32_t h, w, stride, reserved;
} cvx_frame_job;
/* NMS rows -> original-image coordinates.  rows (batch, max_det, 6) fp32 [x1, y1, x2, y2, score, cls] and counts (batch) int32 as cvx_nms,
 * cvx_nms_variant and the SSD / CenterNet decode tails leave them; box_mode 0: the boxes are final and are copied, 1: (x - px) * gx with
 * box_map (batch, 4) fp32 [px, py, gx, gy] -- the device function cvx_det_match maps its boxes with, two roundings per coordinate, so the
 * result is undo_letterbox's to the bit.  out_rows (batch, max_det, 6): score and class copied, the rows past the count zero; out_counts
 * (batch).  A count of -1 (the NMS overflow mark) or above max_det gives out count 0 and adds 1 to *overflow (1 int32, device, cleared
 * by the caller).
 * Replaces: core/utils/boxes.py:undo_letterbox after the .cpu() of YOLOv8.decode_box (reference core/algorithms/yolo_v8.py:229-242,
 * reverse_letter_box_numpy, core/utils/image_process.py:69-97). */
int cvx_det_to_image(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map, float* out_rows,
                     int32_t* out_counts, int32_t* overflow, void* hip_stream);
/* Paints the detections of frame b -- rows[b, 0 .. counts[b]) in image coordinates -- into jobs[b], in place.  (max_h, max_w): the largest
 * frame of the batch (the grid).  Painter's order: box 0 first; per box the outline, the label tag, the label text.  Coordinates are
 * truncated towards zero (boxes.astype(int)).  Outline of thickness t: the pixels inside the box grown by t / 2 and outside the box shrunk
 * by (t + 1) / 2 (integer divisions), clipped to the frame; x1 < x0 or y1 < y0 (or a NaN) paints nothing.  Label "{cls}:{p}%": cls the
 * class index, p = tenths / 10 with one decimal, tenths = rint(double(score * 100.0f) * 10.0) -- Python's '{:.1f}'.format of the fp32
 * product; the project's own 5 x 7 font at font_scale; the tag is (6 * chars + 1) * font_scale wide and 9 * font_scale high, its left edge
 * at x0, above the box when y0 - height >= 0 and otherwise from y0 down.  Colours: entry (cls + 1) mod lut_entries of lut (entries x 3
 * bytes in the frame's channel order) for the outline, each channel * 7 / 10 for the tag, text black when the channel sum exceeds 382 and
 * white otherwise.  Every painted pixel is written once; no pixel is read.
 * Replaces: Draw.draw_boxes_on_image / show_detection_results (reference core/utils/visualize.py) behind every detector's predict; the
 * reference's colour table and OpenCV's Hershey font are not reproduced. */
int cvx_draw_detections(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* rows, const int32_t* counts, int32_t max_det,
                        const uint8_t* lut, int32_t lut_entries, int32_t thickness, int32_t font_scale, void* hip_stream);
/* Colours a segmentation result and blends it 50/50 into RGB frame b, in place, with no full-resolution logits or colour image in memory.
 * logits_rows (batch, lh * lw, ld) fp32 as the DeepLab engine's forward leaves them, for a (net_h, net_w) network input.  Per frame pixel:
 * the nearest pixel at network size (cv2.resize(..., INTER_NEAREST)'s index rule), the nc logits there by the taps of
 * cvx_resize_bilinear_rows_to_nchw / cvx_seg_criterion_eval (bit-identical), arg max (the lowest class wins a tie), lut (nc x 3 bytes, RGB), and
 * (a + b) / 2 rounded half to even per channel; bgr_out != 0 writes the pixel as B, G, R.
 * Replaces: postprocess_seg2d, cv2.resize(INTER_NEAREST), cv2.addWeighted(.5, .5) and [..., ::-1] in DeeplabV3PlusA.predict
 * (reference core/algorithms/segmentation_2d.py:20-30, 80-113). */
int cvx_seg_overlay(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* logits_rows, int32_t ld, int32_t nc, int32_t lh,
                    int32_t lw, int32_t net_h, int32_t net_w, const uint8_t* lut, int32_t bgr_out, void* hip_stream);

/* ---- tiled prediction for large frames (csrc/tiles.hip) -----------------------------------------------------------
 * A frame larger than the network input is cut into overlapping tiles at network size (zoom 1), the tiles run as one batch, and the rows
 * of all tiles of a frame are merged across the tile borders.  Both entries are one launch, asynchronous on hip_stream, with their tables
 * in device memory, and read nothing back.  The reference predicts one letterboxed image at a time and has no counterpart: the rules are
 * the project's own, restated in numpy in tests/tiled_restatement.py.  40 bytes per job. */
typedef struct cvx_tile_job {
  const uint8_t* src;
  int32_t h, w, stride, y0, x0, th, tw, out;
} cvx_tile_job;
/* Slot `out` of out_nchw (slots, 3, H, W) fp32 receives the crop [y0, y0 + th) x [x0, x0 + tw) of the uint8 HWC frame `src` (h x w, row
 * pitch `stride` bytes: padded rows are read in place), anchored top-left.  Each value is (float)byte / 255.0f, a true fp32 division as in
 * cvx_letterbox_u8_to_nchw; everything outside the crop, and any pixel a bad job would read outside the frame, is 128.0f / 255.0f.
 * swap_rb != 0 swaps the first and third channel.  No resampling.  Any positive H, W; 16-byte stores where W % 4 == 0. */
int cvx_tiles_u8_to_nchw(const cvx_tile_job* jobs, int32_t n_jobs, int32_t swap_rb, float* out_nchw, int32_t H, int32_t W, void* hip_stream);
/* Greedy suppression across the slots of each frame, one workgroup per frame.  rows (slots, max_det_in, 6) fp32 [x1, y1, x2, y2, score,
 * cls] and counts (slots) int32 as cvx_det_to_image leaves them: boxes in the slot's own pixels.  slot_map (slots, 4) int32 [frame, x0,
 * y0, reserved], frame_hw (frames, 2) int32 [h, w].  Per frame f:
 *   candidates  the rows r < counts[s] of every slot with slot_map[s].frame == f; ordinal s * max_det_in + r.  A count below 0 or above
 *               max_det_in contributes nothing and adds 1 to *overflow (1 int32, device, cleared by the caller).
 *   boxes       x + (float)x0, y + (float)y0 -- one fp32 add -- then fminf(fmaxf(v, 0), w or h); score and class are copied.
 *   order       score descending, then ordinal ascending (the 64-bit key of cvx_nms, the ordinal in the low word).
 *   greedy      candidate i is dropped when an earlier kept j, of the same class unless class_agnostic, has metric(i, j) > threshold.
 *               metric 0: inter / (area_i + area_j - inter), cvx_nms's IoU to the bit; metric 1 (IoS): inter / fminf(area_i, area_j).
 *               fp32, every operation rounded on its own; a NaN (0 / 0 of a degenerate box) never suppresses.  Stops at max_det_out kept.
 *   outputs     out_rows (frames, max_det_out, 6) the kept rows in order, the rest zero; out_counts (frames); out_source (frames,
 *               max_det_out) the ordinal of each kept row, -1 past the count.
 *   capacity    8192 candidates per frame: beyond it out_counts[f] = -1, the frame's rows are zero and *overflow grows by 1 -- flagged,
 *               never truncated.
 * workspace: cvx_det_merge_workspace_bytes(frames) bytes of device memory (8 MB of suppression masks per frame). */
int64_t cvx_det_merge_workspace_bytes(int32_t frames);
int cvx_det_merge_tiles(const float* rows, const int32_t* counts, int32_t slots, int32_t max_det_in, const int32_t* slot_map,
                        const int32_t* frame_hw, int32_t frames, int32_t metric, float threshold, int32_t class_agnostic, int32_t max_det_out,
                        float* out_rows, int32_t* out_counts, int32_t* out_source, int32_t* overflow, void* workspace, int64_t workspace_bytes,
                        void* hip_stream);

/* ---- sliding-window segmentation for large frames (csrc/seg_tiles.hip) ----------------------------------------------
 * The tiles of a frame (render.tile_grid, cvx_tiles_u8_to_nchw with full_frame off) run through the DeepLab engine as slots of one batch;
 * cvx_seg_stitch blends their up-sampled logits per frame pixel and writes the label, the overlay and the confusion counts.  One launch
 * for all frames, asynchronous on hip_stream, tables in device memory, nothing read back, no full-resolution logits in memory.  The
 * reference has no counterpart: the rules are the project's own, restated in numpy in tests/seg_tiled_restatement.py.
 * The tile grid of a frame is the product of ny tiles along y and nx tiles along x: tile (ty, tx) is slot first_slot + ty * nx + tx,
 * and tile_axes holds (start, extent) int32 pairs -- ny of them from y_off, nx of them from x_off (offsets in int32 elements).  24 bytes. */
typedef struct cvx_seg_tile_frame {
  int32_t first_slot, ny, nx, y_off, x_off, reserved;
} cvx_seg_tile_frame;
/* A uint8 (h, w) map of a frame -- labels out, targets in -- with its row pitch in bytes; data NULL: this frame has none.  16 bytes. */
typedef struct cvx_seg_map {
  uint8_t* data;
  int32_t pitch, reserved;
} cvx_seg_map;
/* logits_rows (slots, lh * lw, ld) fp32 as the engine's forward leaves them for a (net_h, net_w) input; tile_frames / jobs / label_maps /
 * target_maps have one entry per frame; (max_h, max_w): the largest frame (the grid).  Per frame pixel (y, x), over the tiles that cover
 * it (y0 <= y < y0 + th and x0 <= x < x0 + tw) in row-major order, ty outer:
 *   z_k[c]  the logit at the tile-local pixel (y - y0, x - x0) by the taps of cvx_resize_bilinear_rows_to_nchw at scale lh / net_h,
 *           lw / net_w (a slot is a full network input whatever the tile's extent), bit-identical to that entry's output;
 *   w_k     weight_mode 0 ("mean"): 1.0f; 1 ("linear"): (float)(min(dy + 1, th - dy) * min(dx + 1, tw - dx)), an integer below 2^24;
 *   acc[c]  = fmaf(w_k, z_k[c], acc[c]) from 0.0f -- one rounding per tile, no division by the weight sum;
 *   label   the arg max of acc, the lowest class winning a tie.
 * Outputs, each optional: label_maps[f] receives the label byte; draw != 0 blends lut[label] (nc x 3 bytes, RGB) 50/50 into the frame in
 * place as cvx_seg_overlay does (bgr_out != 0 writes B, G, R); with target_maps and confusion (nc x nc int64, added to, never cleared)
 * confusion[target][label] += 1 where target < nc (a per-workgroup LDS histogram: nc <= 128 on this path).  nc <= 256: labels are bytes. */
int cvx_seg_stitch(const float* logits_rows, int32_t slots, int32_t ld, int32_t nc, int32_t lh, int32_t lw, int32_t net_h, int32_t net_w,
                   const cvx_seg_tile_frame* tile_frames, const int32_t* tile_axes, int32_t n_axes, const cvx_frame_job* jobs, int32_t frames,
                   int32_t max_h, int32_t max_w, const cvx_seg_map* label_maps, const cvx_seg_map* target_maps, int64_t* confusion,
                   const uint8_t* lut, int32_t weight_mode, int32_t draw, int32_t bgr_out, void* hip_stream);

/* ---- multi-object tracking on the device video path (csrc/track.hip) ------------------------------------------------
 * A ByteTrack-style tracker: two association stages by score, constant-velocity prediction with an alpha-beta update, greedy IoU
 * association.  One launch per batch of frames, the state in device memory, nothing read back.  The rules are the project's own, restated
 * in numpy in tests/track_restatement.py; the kernel is held to the restatement bit for bit.
 * Replaces: nothing, the reference has no counterpart.
 * The state of one stream.  All zero means "no tracks, frame 0, next id 0": creating or resetting a tracker is a memset.  The live tracks
 * are the entries [0, n_tracks) of every array; their order inside the table is not part of the contract (everything observable is keyed
 * by the track id), and the entries past n_tracks are unspecified.  cls holds the class as the rows carry it (a float). */
#define CVX_TRACK_CAP 1024
typedef struct cvx_track_stream {
  int32_t frame, next_id, n_tracks, reserved;
  int32_t id[CVX_TRACK_CAP], hits[CVX_TRACK_CAP], miss[CVX_TRACK_CAP];
  float cls[CVX_TRACK_CAP];
  float p[CVX_TRACK_CAP][4]; /* x1, y1, x2, y2 */
  float v[CVX_TRACK_CAP][4]; /* per frame */
} cvx_track_stream;
/* Host memory, read during the call.  Defaults: high 0.5, new_score 0.6, iou_high 0.2, iou_low 0.5, alpha 0.75, beta 0.25, min_hits 3,
 * max_age 30, class_agnostic 0.  The four thresholds lie in [0, 1], min_hits >= 1, max_age >= 0. */
typedef struct cvx_track_params {
  float high, new_score, iou_high, iou_low, alpha, beta;
  int32_t min_hits, max_age, class_agnostic, reserved;
} cvx_track_params;
/* rows (batch, max_det, 6) fp32 [x1, y1, x2, y2, score, cls] and counts (batch) int32 as cvx_det_to_image and cvx_det_merge_tiles leave
 * them.  The frames are in time order; frame b belongs to stream frame_stream[b] (NULL: all to stream 0), the frames of a stream are
 * processed in batch order, and the streams are independent (one workgroup each).  state: cvx_track_state_bytes(streams) bytes of device
 * memory, `streams` cvx_track_stream in a row, carried from call to call.  out_ids (batch, max_det) int32: the track id of each row or -1.
 * A frame_stream value outside [0, streams) makes the frame a no-op: its ids are -1 and *overflow (1 int32, device, cleared by the caller)
 * grows by 1.  All arithmetic is fp32, every operation rounded on its own.  Per frame of a stream, n = counts[b]; a count below 0 or above
 * max_det adds 1 to *overflow and the frame is processed as n = 0:
 *   1 count     frame += 1; out_ids[b, :] = -1.
 *   2 predict   every live track: p = p + v per coordinate.
 *   3 split     a row with a NaN coordinate is ignored throughout (id -1, no match, no birth); high: score >= high; low: the rest of
 *               the n rows (a NaN score is low).
 *   4 stage 1   candidate pairs (live track, high row), of the same class unless class_agnostic, with iou(p, box) > iou_high -- the
 *               IoU of cvx_nms (box_overlap.h:iou_value), a NaN never passes.  Greedy over the pairs sorted by (IoU descending, track id
 *               ascending, row index ascending): a pair is taken when neither its track nor its row is taken yet.
 *   5 stage 2   the same with iou_low, between the low rows and the tracks still unmatched with hits >= min_hits and miss == 0.
 *   6 update    every matched pair: r = z - p; p = p + alpha * r; v = v + beta * r per coordinate (mul, then add); hits += 1; miss = 0;
 *               cls = the row's class; out_ids[b, d] = id when hits >= min_hits or frame <= min_hits, else it stays -1.
 *   7 unmatched a track with hits < min_hits is deleted; otherwise miss += 1 and the track is deleted when miss > max_age.
 *   8 births    in row order, every unmatched high row with score >= new_score: id = next_id++, p = box, v = 0, hits = 1, miss = 0,
 *               cls = the row's; out_ids[b, d] = id when 1 >= min_hits or frame <= min_hits.  When the stream already holds
 *               CVX_TRACK_CAP tracks the row is skipped, next_id does not move and *overflow grows by 1: flagged, never evicted. */
int64_t cvx_track_state_bytes(int32_t streams);
int cvx_track_update(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream, int32_t streams,
                     const cvx_track_params* params, void* state, int32_t* out_ids, int32_t* overflow, void* hip_stream);
/* ---- a Kalman motion model and a minimum-cost association for the tracker, both optional (csrc/track.hip) ----------
 * cvx_track_update with two choices more: the same arguments, state, flags and frame rules, except for what `model` replaces.  The rules
 * are restated in numpy in tests/track_model_restatement.py and the kernel is held to the restatement bit for bit.  With motion alpha-beta
 * and assign greedy every byte is cvx_track_update's.  Additive: CVX_ABI_VERSION stays 6 (no existing entry or struct changes).
 * Replaces: nothing, the reference has no counterpart.
 * ext: cvx_track_ext_bytes(streams) bytes of device memory, 16-byte aligned, carried from call to call with state: per stream
 * float cov[CVX_TRACK_CAP][4], the covariance (Pxx, Pxv, Pvv, reserved 0) of the track in the same slot of cvx_track_stream.  All zero means
 * "nothing seen"; it is read and written under the Kalman motion only, by the stream's workgroup.
 *
 * motion = CVX_TRACK_MOTION_KALMAN: a constant-velocity Kalman filter per coordinate (the four corners stay the state).  The four
 *   coordinates share one noise scale s = max(y2 - y1, min_scale) of the track's box (fmaxf: min_scale for a NaN), and the covariance
 *   recurrence does not see the measurements, so one symmetric 2 x 2 covariance per track serves all four.  alpha and beta are ignored.
 *   Every line is one rounded fp32 operation per operator, in the order written; the division is correctly rounded:
 *   8 births    v = 0; a = init_pos * r_pos; a = a * s; Pxx = a * a; Pxv = 0; b = init_vel * q_vel; b = b * s; Pvv = b * b, s of the row's box.
 *   2 predict   s of the box before the move; p = p + v; a = Pxv + Pxv; a = a + Pvv; b = q_pos * s; b = b * b; a = a + b; Pxx = Pxx + a;
 *               Pxv = Pxv + Pvv (the old Pvv); c = q_vel * s; c = c * c; Pvv = Pvv + c.  Every live track in every frame of its stream.
 *   6 update    s of the predicted box; e = r_pos * s; e = e * e; e = Pxx + e; kx = Pxx / e; kv = Pxv / e; per coordinate r = z - p;
 *               p = p + kx * r; v = v + kv * r (mul, then add); then Pvv = Pvv - kv * Pxv; Pxv = Pxv - kx * Pxv; Pxx = Pxx - kx * Pxx.
 * assign = CVX_TRACK_ASSIGN_OPTIMAL: stages 1 and 2 as a minimum-cost assignment over the same candidate tracks and rows.  A pair is
 *   allowed when iou(p, box) > the stage's threshold (a NaN never passes) and the classes agree unless class_agnostic; its cost is the
 *   integer rint((1 - iou) * 65536) of cvx_mot_frames.  (a) An allowed pair that is the only allowed pair of its track and of its row is
 *   taken.  (b) Candidates without an allowed pair are set aside.  (c) The remaining tracks in ascending id and the remaining rows in
 *   ascending row index are assigned by the solver of cvx_mot_frames (csrc/assign_solver.h): the number of pairs is maximal and among those
 *   the cost sum minimal; the smaller side drives, the tracks when the sides are equal; a forbidden cell costs 2^27 and a pair on one is
 *   dropped; rows inserted in order, the lowest column wins a tie.  max_det <= CVX_TRACK_OPTIMAL_MAX_DET.
 * Host memory, read during the call.  Defaults: alpha-beta, greedy, q_pos 1/20, q_vel 1/160, r_pos 1/20, init_pos 2, init_vel 10,
 * min_scale 1.  The five weights are finite and >= 0, min_scale is finite and > 0. */
#define CVX_TRACK_MOTION_ALPHA_BETA 0
#define CVX_TRACK_MOTION_KALMAN 1
#define CVX_TRACK_ASSIGN_GREEDY 0
#define CVX_TRACK_ASSIGN_OPTIMAL 1
#define CVX_TRACK_OPTIMAL_MAX_DET 4096
typedef struct cvx_track_model {
  int32_t motion, assign;
  float q_pos, q_vel, r_pos, init_pos, init_vel, min_scale;
} cvx_track_model;
int64_t cvx_track_ext_bytes(int32_t streams);
int cvx_track_update_model(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream, int32_t streams,
                           const cvx_track_params* params, const cvx_track_model* model, void* state, void* ext, int32_t* out_ids,
                           int32_t* overflow, void* hip_stream);
/* cvx_draw_detections for tracked rows: ids (batch, max_det) int32 as cvx_track_update leaves them.  A row whose id is negative paints
 * nothing.  The label is "{id % 1000000}:{cls}" and the outline colour entry (id + 1) mod lut_entries, so an object keeps its colour
 * while it keeps its id; tag and text colours follow from it by cvx_draw_detections's rules, and geometry, painter's order and the
 * once-written pixels are that entry's (one kernel body).
 * Replaces: nothing, the reference has no counterpart. */
int cvx_draw_tracks(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* rows, const int32_t* counts, int32_t max_det,
                    const int32_t* ids, const uint8_t* lut, int32_t lut_entries, int32_t thickness, int32_t font_scale, void* hip_stream);

/* ---- multi-scale and flip test-time augmentation for segmentation (csrc/seg_tta.hip) --------------------------------
 * The network runs on the batch at several zooms and on its mirror image; the class scores of all views are fused per pixel at the
 * picture's size.  Both entries are one launch, asynchronous on hip_stream, and read nothing back.  The reference has no counterpart: the
 * rules are the project's own, restated in numpy in tests/seg_tta_restatement.py.
 * cvx_seg_tta_inputs: images (batch, c, h, w) fp32 -> out (batch * (1 + with_flip), c, oh, ow) fp32.  Image b of the output is the
 * bilinear resize of image b (align_corners = False, no antialiasing: the taps bilinear_src(y, (float)h / (float)oh, h) and
 * bilinear_src(x, (float)w / (float)ow, w) of csrc/bilinear.h, the value bilinear_mix); with with_flip, image batch + b is the resized
 * picture mirrored, out[batch + b, :, y, x] = out[b, :, y, ow - 1 - x] -- the resize first, the mirror second.  At (oh, ow) == (h, w) the
 * plain half is a bit-exact copy (every tap has lam == 0).  batch * c <= 65535, oh <= 65535. */
int cvx_seg_tta_inputs(const float* images_nchw, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t with_flip,
                       float* out_nchw, void* hip_stream);
/* One view of the fusion: rows (batch, lh * lw, ld) fp32 (device) as the DeepLab engine's forward leaves them for that view's input;
 * flip != 0: the view saw the mirrored picture.  24 bytes. */
typedef struct cvx_seg_view {
  const float* rows;
  int32_t lh, lw, flip, reserved;
} cvx_seg_view;
/* views_host: 1 <= n_views <= 16 entries in HOST memory, read before the call returns and handed to the kernel by value (no device table,
 * nothing to keep alive).  Per output pixel (b, y, x), over the views in table order:
 *   xs      flip_k ? ow - 1 - x : x;
 *   z_k[c]  the logit by the taps bilinear_src(y, (float)lh_k / (float)oh, lh_k) and bilinear_src(xs, (float)lw_k / (float)ow, lw_k), mixed
 *           with bilinear_mix: bit-identical to cvx_resize_bilinear_rows_to_nchw's output for that view at (oh, ow), read at (y, xs) -- one
 *           interpolation from the logit level to the output size, as in cvx_seg_criterion_eval;
 *   mode 0  ("logits") acc[c] = acc[c] + z_k[c] from 0.0f, one rounded add per view;
 *   mode 1  ("prob")   m_k = max_c z_k[c], e = expf(z_k[c] - m_k), acc[c] += e / sum_c e.
 * Outputs, each optional (at least one): labels (batch, oh, ow) uint8, the arg max of acc with strict > (the lowest class wins a tie;
 * nc <= 256); with target (batch, oh, ow) int64 and confusion (nc, nc) int64 (added to, never cleared) confusion[target * nc + label] += 1
 * for targets in [0, nc), others skipped -- an LDS histogram per workgroup for nc <= 90 and direct 64-bit atomics above, as cvx_seg_criterion_eval;
 * probs_nchw (batch, nc, oh, ow) fp32 = acc[c] / n_views, mode 1 only (refused in mode 0).  The padding columns nc .. ld - 1 are never
 * read as classes.  batch, oh <= 65535. */
int cvx_seg_fuse(const cvx_seg_view* views_host, int32_t n_views, int32_t ld, int32_t batch, int32_t nc, int32_t oh, int32_t ow, int32_t mode,
                 uint8_t* labels, const int64_t* target, int64_t* confusion, float* probs_nchw, void* hip_stream);

/* ---- scale and flip test-time augmentation for the detectors (csrc/det_tta.hip) -------------------------------------
 * The network runs on the batch at a few zooms <= 1 and on its mirror image, every view at the network's own input size, and the boxes of
 * all views of a frame are mapped back to the picture and fused.  Both entries are one launch, asynchronous on hip_stream, and read nothing
 * back.  The reference has no counterpart: the rules are the project's own, restated in numpy in tests/det_tta_restatement.py.
 * One view: the picture resized to (h, w) sits at (top, left) of the (H, W) network input; flip != 0: the whole input is mirrored along x
 * after that.  24 bytes. */
typedef struct cvx_det_view {
  int32_t h, w, top, left, flip, reserved;
} cvx_det_view;
/* images (batch, 3, H, W) fp32 -> out ((n_views * batch), 3, H, W) fp32, slot k * batch + b = view k of picture b.  views_host: 1 <=
 * n_views <= 8 entries in HOST memory, read before the call returns and handed to the kernel by value; every rectangle lies inside the
 * input.  With xs = flip_k ? W - 1 - x : x, pixel (y, x) of slot k * batch + b is
 *   inside   top_k <= y < top_k + h_k and left_k <= xs < left_k + w_k: the bilinear resize of the picture to (h_k, w_k) at (y - top_k,
 *            xs - left_k) -- align_corners = False, no antialiasing: the taps bilinear_src(y - top_k, (float)H / (float)h_k, H) and
 *            bilinear_src(xs - left_k, (float)W / (float)w_k, W) of csrc/bilinear.h, the value bilinear_mix;
 *   outside  pad (the letterbox's grey is 128.0f / 255.0f).
 * The resize first, the mirror second.  A view with (h, w) == (H, W) and no flip is a bit-exact copy (every tap has lam == 0).  Slots
 * past n_views * batch are not written.  Any positive H, W; 16-byte stores where W % 4 == 0. */
int cvx_det_tta_inputs(const float* images_nchw, int32_t batch, int32_t H, int32_t W, const cvx_det_view* views_host, int32_t n_views, float pad,
                       float* out_nchw, void* hip_stream);
/* Fuses the views of each frame, one workgroup per frame.  rows (views * frames, max_det_in, 6) fp32 [x1, y1, x2, y2, score, cls] and
 * counts (views * frames) int32 as cvx_det_to_image leaves them, slot s = k * frames + f: what the tail reports for view k of frame f.
 * view_map (views * frames, 4) fp32 [ax, cx, ay, cy], frame_hw (frames, 2) int32 [h, w].  Per frame f:
 *   candidates  the rows r < counts[s] of the slots k * frames + f; ordinal s * max_det_in + r.  A count below 0 or above max_det_in
 *               contributes nothing and adds 1 to *overflow (1 int32, device, cleared by the caller).
 *   boxes       t1 = x1 * ax + cx, t2 = x2 * ax + cx -- a rounded product, then a rounded add --, x1' = fminf(t1, t2), x2' = fmaxf(t1, t2)
 *               (a flipped view has ax < 0), then fminf(fmaxf(v, 0), w); likewise y with ay, cy and h.  Score and class are copied.
 *   order       score descending, then ordinal ascending (the 64-bit key of cvx_nms, the ordinal in the low word).
 *   greedy      cvx_det_merge_tiles's walk under metric 0: candidate i is dropped when an earlier kept j, of the same class unless
 *               class_agnostic, has IoU(i, j) > threshold (cvx_nms's IoU to the bit; a NaN never suppresses).  Stops at max_det_out kept.
 *   members     of a kept row i: itself and every candidate j != i, before or behind it, kept or not, of its class (unless
 *               class_agnostic) with IoU(i, j) > threshold.
 *   mode 0      ("nms") the kept rows' own boxes.
 *   mode 1      ("vote") over the members j in sorted order, from 0.0f: weight w = score_i for j == i, else IoU(i, j) * score_j;
 *               Wt = Wt + w; X_c = X_c + w * box_j[c] for the four corners -- every operation rounded on its own, in that order -- and
 *               the box is X_c / Wt.  A kept row without another member, or with Wt not above 0, keeps its own box bit for bit.
 *   score_mode  0 ("max"): score_i.  1 ("views"): (score_i * (float)m) / (float)views, m the number of distinct views (ordinal /
 *               max_det_in / frames) among the members.  The rows stay in kept order either way.
 *   outputs     out_rows (frames, max_det_out, 6), zero past the count; out_counts (frames); out_source (frames, max_det_out) the ordinal
 *               of each kept row, -1 past the count; out_members (frames, max_det_out) the members of each kept row, 0 past the count.
 *   capacity    8192 candidates per frame: beyond it out_counts[f] = -1, the frame's rows are zero and *overflow grows by 1 -- flagged,
 *               never truncated.
 * workspace: cvx_det_merge_workspace_bytes(frames) bytes of device memory (the layout of cvx_det_merge_tiles). */
int cvx_det_fuse_views(const float* rows, const int32_t* counts, int32_t max_det_in, const float* view_map, const int32_t* frame_hw,
                       int32_t frames, int32_t views, float threshold, int32_t class_agnostic, int32_t mode, int32_t score_mode,
                       int32_t max_det_out, float* out_rows, int32_t* out_counts, int32_t* out_source, int32_t* out_members, int32_t* overflow,
                       void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- Weighted Boxes Fusion of several sources per frame (csrc/box_fusion.hip) --------------------------------------
 * The sources are the views of a test-time augmentation or the members of a detector ensemble.  rows, counts, view_map, frame_hw and the
 * candidates, their ordinals and their boxes are those of cvx_det_fuse_views, `sources` in the place of `views` (1 to 32).  weights
 * (sources) fp32 on the device, positive and finite.  One workgroup per frame; per frame f:
 *   skipped     a row whose score is below skip_score, or whose mapped and clamped box does not have x2 > x1 and y2 > y1.
 *   order       class ascending (the fp32 value; the bits, for the non-negative classes the tails emit), then s = score * weights[k]
 *               descending, then ordinal ascending.  class_agnostic: one segment per frame, (s, ordinal) alone.
 *   clusters    each class segment is walked in order.  Candidate j joins the cluster c of its segment with the largest
 *               IoU(fused_c, box_j) (cvx_nms's IoU to the bit) strictly above iou_thr, the lowest c among equals; a NaN never matches.
 *               No match opens a cluster: fused = box_j bit for bit, sw = s_j, sx = s_j * box_j per corner, n = 1, smax = s_j, first = j.
 *               A match updates it: sw = sw + s_j, sx = sx + s_j * box_j, n += 1, fused = sx / sw -- every operation rounded on its own.
 *   score       m = fminf((float)n, W), W the fp32 sum of weights in index order.  conf_mode 0 ("avg"): ((sw / (float)n) * m) / W;
 *               1 ("max"): (smax * m) / W; with rescale == 0 sw / (float)n or smax as it stands.
 *   outputs     the clusters of the frame by (score descending, first ordinal ascending), the first max_det_out: out_rows (frames,
 *               max_det_out, 6) [fused box, score, class of the first member], zero past the count; out_counts (frames); out_source the
 *               ordinal of the first member, -1 past the count; out_members n, 0 past the count.
 *   capacity    8192 rows per frame before skipping: beyond it out_counts[f] = -1, the frame's rows are zero and *overflow grows by 1.
 *               A count below 0 or above max_det_in contributes nothing and adds 1 to *overflow.
 * workspace: cvx_det_wbf_workspace_bytes(frames) bytes of device memory (under 1 MB per frame). */
int64_t cvx_det_wbf_workspace_bytes(int32_t frames);
int cvx_det_fuse_wbf(const float* rows, const int32_t* counts, int32_t max_det_in, const float* view_map, const int32_t* frame_hw,
                     int32_t frames, int32_t sources, const float* weights, float iou_thr, float skip_score, int32_t class_agnostic,
                     int32_t conf_mode, int32_t rescale, int32_t max_det_out, float* out_rows, int32_t* out_counts, int32_t* out_source,
                     int32_t* out_members, int32_t* overflow, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- connected-component regions of label maps (csrc/seg_regions.hip) ------------------------------------------------
 * Boxes from label maps: the connected regions of each class of a uint8 label map (cvx_seg_stitch's, cvx_seg_fuse's), in the detectors'
 * row format, so that cvx_draw_detections, cvx_draw_tracks, cvx_track_update, cvx_det_match and cvx_coco_match take them as they are.
 * All frames of a batch run together: a fixed number of launches (five, six with a map) whatever the maps hold, asynchronous on
 * hip_stream, tables in device memory, nothing read back.  The reference has no counterpart: the rules are the project's own, restated in
 * numpy in tests/seg_regions_restatement.py, and the kernels are held to the restatement bit for bit.
 * An fp32 (h, w) plane of a frame with its row pitch in ELEMENTS; data NULL: this frame has none.  16 bytes. */
typedef struct cvx_seg_plane {
  const float* data;
  int32_t pitch, reserved;
} cvx_seg_plane;
/* An int32 (h, w) map of a frame with its row pitch in ELEMENTS; data NULL: this frame has none.  16 bytes. */
typedef struct cvx_seg_imap {
  int32_t* data;
  int32_t pitch, reserved;
} cvx_seg_imap;
/* label_maps (frames) with data != NULL and frame_hw (frames, 2) int32 [h, w] on the device; (max_h, max_w): the largest frame (the grid
 * and the workspace planes).  class_mask_host: 8 uint32 in HOST memory, read before the call returns; bit (c & 31) of word c >> 5 selects
 * label c.  Per frame f with label map L:
 *   selected    a pixel is selected when bit L[y, x] of the mask is set; the others belong to no region and connect nothing.
 *   regions     a region is a maximal set of selected pixels of equal label connected through 4-neighbours (connectivity 4) or
 *               8-neighbours (connectivity 8).
 *   seed        the smallest linear index y * w + x of a region's pixels: its first pixel in raster order.
 *   statistics  exact integers: area, min_x, min_y, max_x, max_y.
 *   score       without `conf` 1.0f.  With conf (one entry per frame, every one with data, fp32 per pixel and its own
 *               pitch) each pixel gives q = (uint32) rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 65535.0f), a NaN
 *               gives 0; S is the sum of q over the region in a 64-bit integer; score = (float)((double) S / ((double) area * 65535.0)).
 *               No floating-point atomic anywhere: two calls give the same bits.
 *   filter      the regions with area >= min_area (>= 1) are the frame's candidates; total[f] is their number, always written.
 *   order       area descending, then seed ascending -- a strict total order; the 64-bit key of csrc/lds_sort.h,
 *               ((0xFFFFFFFF - area) << 32) | seed.
 *   row         [(float) min_x, (float) min_y, (float)(max_x + 1), (float)(max_y + 1), score, (float) label].
 *   outputs     rows (frames, max_det, 6), zero past the count; counts[f] = min(total[f], max_det); areas and seeds (frames, max_det)
 *               int32, -1 past the count.  region_maps (optional table, optional per frame): the row index of the pixel's region, -1 for
 *               unselected pixels and for regions that were filtered or cut by max_det.  clean_maps (optional table, optional per frame):
 *               L with every selected pixel of a region below min_area replaced by `fill` (0 .. 255); written whatever the capacity says.
 *   capacity    8192 candidates per frame (the in-LDS sort of cvx_det_merge_tiles): beyond it counts[f] = -1, the frame's rows are zero,
 *               its region map is all -1 and *overflow (1 int32, device, cleared by the caller) grows by 1 -- flagged, never truncated;
 *               total[f] still says how far over it was.  The other frames of the batch are unaffected.
 *   bad frames  h <= 0, w <= 0, h * w >= 2^31, h > max_h or w > max_w: a no-op with count 0 and total 0 that adds 1 to *overflow.
 * 1 <= max_det <= 8192.  workspace: cvx_seg_regions_workspace_bytes(frames, max_h, max_w) bytes of device memory, 8-byte aligned: 28 bytes
 * per pixel of a max_h x max_w plane per frame (parent 4, area 4, q sum 8, min_x 4, max_x 4, max_y 4) plus 33 KB per frame; 0 for sizes
 * the entry refuses (max_h * max_w >= 2^31). */
int64_t cvx_seg_regions_workspace_bytes(int32_t frames, int32_t max_h, int32_t max_w);
int cvx_seg_regions(const cvx_seg_map* label_maps, const int32_t* frame_hw, int32_t frames, int32_t max_h, int32_t max_w,
                    const uint32_t* class_mask_host, int32_t connectivity, int32_t min_area, int32_t max_det, int32_t fill,
                    const cvx_seg_plane* conf, const cvx_seg_imap* region_maps, const cvx_seg_map* clean_maps, float* rows, int32_t* counts,
                    int32_t* total, int32_t* areas, int32_t* seeds, int32_t* overflow, void* workspace, int64_t workspace_bytes,
                    void* hip_stream);

/* ---- boundary metrics of label maps (csrc/seg_boundary.hip) --------------------------------------------------------------
 * The counts behind trimap mIoU (the DeepLab papers' band around the target's label changes), Boundary IoU (Cheng et al., CVPR 2021) and the
 * boundary F-score BF (Csurka et al. 2013, DAVIS) of predicted label maps against target label maps.  All frames of a batch run together:
 * three launches whatever the maps hold, asynchronous on hip_stream, tables in device memory, nothing read back.  The reference has no
 * counterpart: the rules are the project's own, restated in numpy in tests/seg_boundary_restatement.py, and the kernels are held to the
 * restatement bit for bit -- every quantity is an integer.  Additive: CVX_ABI_VERSION stays 6 (no existing entry or struct changes).
 * pred_maps / target_maps (frames) cvx_seg_map, read in place, and frame_hw (frames, 2) int32 [h, w] on the device; (max_h, max_w): the
 * largest frame (the grid and the workspace planes).  widths (frames, K) int32 on the device, 1 <= K <= 8, every width d_k in 1 .. 64;
 * dmax is the largest width of the frame.  1 <= nc <= 255.  Per frame with prediction P and target G:
 *   void        G'[p] = G[p] if G[p] < nc, else VOID; P'[p] = P[p] if G[p] < nc and P[p] < nc, else VOID.  VOID differs from every class; a
 *               VOID pixel takes part in no count and its planes hold 0.
 *   distance    for a map M and a pixel p of class c, D_M^e(p) is the smallest d >= 1 such that the square of Chebyshev radius d around p
 *               holds a pixel q with M[q] != c or, with e = edge, reaches outside the picture; dmax + 1 if no d <= dmax does.  With
 *               e = noedge the picture border does not count.
 *   contour     K_M = { p : M[p] is a class and D_M^noedge(p) = 1 }.
 *   nearest     for p in K_A of class c, N_{A->B}(p) is the smallest Chebyshev distance from p to a q in K_B with B[q] = c (0 allowed);
 *               dmax + 1 if there is none within dmax.
 *   trimap      (K, nc, nc) int64: trimap[k][G'[p]][P'[p]] += 1 for every p with both labels classes and D_G^noedge(p) <= d_k.
 *   biou        (K, nc, 3) int64 (I, Gb, Pb): Gb counts G'[p] = c and D_G^edge(p) <= d_k, Pb counts P'[p] = c and D_P^edge(p) <= d_k, I
 *               the pixels where both hold.  The band of class c equals mask & ~erode(mask, 3 x 3 ones, d_k iterations, zero border).
 *   bf          (K, nc, 4) int64 (mp, cp, mg, cg): cp = |{p in K_P : P'[p] = c}|, mp those of them with N_{P->G}(p) <= d_k; cg and mg the
 *               same with the roles swapped.
 *   planes      optional (NULL: none): (frames, 6, max_h, max_w) uint8, of frame f the (h, w) corner of each plane -- D_G^edge,
 *               D_G^noedge, D_P^edge, D_P^noedge (1 .. dmax + 1), then N_{P->G} + 1 and N_{G->P} + 1 on the contour (1 .. dmax + 2) and 0 off it.
 * The three tables are added to, never cleared.  A frame whose entry in either table has data NULL is skipped; so is a frame with
 * h <= 0, w <= 0, h > max_h, w > max_w or a width outside 1 .. 64 (the widths live on the device: the host side of the call cannot see
 * them, computervision.pytorch_amd/seg_boundary.py refuses them before the upload).  Refused with a message and without a launch: nc outside 1 .. 255, K outside
 * 1 .. 8, max_h * max_w >= 2^31, a short workspace.  workspace: cvx_seg_boundary_workspace_bytes(frames, max_h, max_w) bytes of device
 * memory: 6 bytes per pixel of a max_h x max_w plane per frame (G', P', the two run radii, the two contour planes); 0 for sizes the entry
 * refuses. */
#define CVX_SEG_BOUNDARY_MAX_WIDTH 64
#define CVX_SEG_BOUNDARY_MAX_WIDTHS 8
int64_t cvx_seg_boundary_workspace_bytes(int32_t frames, int32_t max_h, int32_t max_w);
int cvx_seg_boundary(const cvx_seg_map* pred_maps, const cvx_seg_map* target_maps, const int32_t* frame_hw, int32_t frames, int32_t max_h,
                     int32_t max_w, int32_t nc, const int32_t* widths, int32_t K, int64_t* trimap, int64_t* biou, int64_t* bf, uint8_t* planes,
                     void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- tracking evaluation: CLEAR-MOT and the identity measures (csrc/track_eval.hip) -----------------------------------
 * Scores the ids of cvx_track_update against ground-truth identities: MOTA, MOTP and their counts (Bernardin & Stiefelhagen 2008), IDF1,
 * IDP, IDR (Ristani et al. 2016).  The rules are the project's own, with every tie decided; on inputs without ties they are
 * py-motmetrics' and the MOTChallenge devkit's.  They are restated in numpy in tests/track_eval_restatement.py and the kernels are held
 * to the restatement bit for bit: behind the quantisation of the IoU everything is an integer.  Additive: CVX_ABI_VERSION stays 6.
 *
 * cvx_mot_frames: rows (batch, max_det, 6), counts (batch) and ids (batch, max_det) as cvx_track_update takes and leaves them;
 * gt (batch, max_gt <= 1024, 6) fp32 [x1, y1, x2, y2, cls, identity] and gt_counts (batch); frame_stream as in cvx_track_update.  One
 * workgroup per stream walks its frames in batch order; asynchronous on hip_stream, nothing read back.  state:
 * cvx_mot_state_bytes(streams, max_gt_ids, max_track_ids) bytes of device memory carried from call to call, per stream (rounded up to 8 bytes)
 *   cvx_mot_stream_header, then int32 arrays of max_gt_ids entries each -- mem (1 + the track of the identity's last match, 0: none), last (the
 *   stream's frame number of that match, frames counted from 1), present, matched (frames), gap (1: unmatched in its last present frame) --
 *   then c (max_gt_ids, max_track_ids) int32.  All zero means "nothing seen": creating or resetting an evaluator is a memset.
 * workspace: cvx_mot_workspace_bytes(streams) bytes (a 1024 x 1024 int32 cost matrix per stream, used when a frame's matrix has more than
 * 16384 cells; smaller ones live in LDS).
 * Per frame of a stream, in order:
 *   hypotheses  the rows d < count with ids[d] >= 0, in row order; beyond 1024 of them the rest are skipped (flag excess).  Skipped and
 *               flagged one by one: a box with a NaN (flag nan), an id >= max_track_ids (flag track), a row whose id an earlier row
 *               that passed these two checks carries (flag dup_row).
 *   truths      the gt rows g < gt_count; skipped and flagged: a box with a NaN (nan), an identity that is not an integer in
 *               [0, max_gt_ids) (identity), an identity an earlier row that passed these checks carries (dup_gt).
 *   frame       a count outside [0, max_det], a gt_count outside [0, max_gt] or a stream outside [0, streams) skips the whole frame (flag
 *               frame; a bad stream is flagged in stream 0).  Otherwise the stream's frame number grows by 1.
 *   gate        a pair (truth, hypothesis) is allowed when iou_value(truth, hypothesis) >= iou (box_overlap.h, the IoU of cvx_nms; a NaN
 *               never passes) and the classes are equal or class_agnostic.  Its cost is rint((1 - iou_value) * 65536) as an integer, every
 *               fp32 operation rounded on its own.  c[identity, id] grows by 1 for every allowed pair, matched or not.
 *   1 keep      an identity with mem > 0 and last == frame - 1 keeps that track when the track is among the hypotheses and the pair is
 *               allowed: a match, never a switch.
 *   2 assign    the remaining truths and hypotheses, each in order: the assignment with the maximal number of allowed pairs and, among
 *               those, the minimal sum of costs, as the solver below finds it.  A new pair is a switch when mem > 0 and mem - 1 is
 *               another track, however old.  Every match sets mem and last.
 *   3 count     objects += truths, hypotheses += hypotheses, matches, cost += the costs of the matches, misses = truths - matches,
 *               false positives = hypotheses - matches.
 *   4 identity  present += 1; matched += 1 on a match.  A match with gap == 1 and matched > 0 before it is a fragmentation.  gap becomes
 *               0 on a match and 1 otherwise.
 *   solver      rows: the smaller side (the truths when both are equal), columns: the other; a forbidden cell costs 2^27.  Rows are
 *               inserted in order by shortest augmenting paths with 64-bit potentials (the classical O(n^2 m) method: from the new row,
 *               repeatedly relax the slacks of the unvisited columns through the row of the column visited last, take the unvisited
 *               column of minimal slack -- the lowest index on a tie --, lower the potentials by that slack, until a free column is
 *               reached; then flip the path).  The pairs on forbidden cells are dropped.
 * cvx_mot_summary: one launch per stream's table row and one that sums them, after the last frame (it changes no state and may be
 * called again later).  table (streams + 1, CVX_MOT_TABLE_WORDS) int64 on the device, the last row the sum over the streams:
 *   0 frames, 1 objects, 2 hypotheses, 3 matches, 4 misses, 5 false positives, 6 switches, 7 fragmentations, 8 cost, 9 mostly tracked
 *   (5 * matched >= 4 * present), 10 partly tracked, 11 mostly lost (5 * matched < present), 12 IDTP, 13 .. 19 the flags nan, dup_row, dup_gt,
 *   identity, track, frame, excess, 20 identities seen, 21 tracks with a non-zero column of c, 22 .. 23 zero.
 * IDTP is the maximum of sum c[o, h] over the partial one-to-one matchings of identities to tracks: the solver on the non-empty rows and
 * columns of c with cost -c (a zero cell is as good as no pair).  This equals Ristani's minimum of FN + FP on the graph with dummy nodes,
 * whose total is sum n_o + sum n_h - 2 IDTP.  IDFN = objects - IDTP, IDFP = hypotheses - IDTP; the scores follow in double on the host. */
#define CVX_MOT_FRAME_CAP 1024
#define CVX_MOT_MAX_GT_IDS 1024
#define CVX_MOT_MAX_TRACK_IDS 4096
#define CVX_MOT_HEADER_WORDS 16
#define CVX_MOT_TABLE_WORDS 24
typedef struct cvx_mot_stream_header {
  int64_t v[CVX_MOT_HEADER_WORDS]; /* the table's words 0 .. 8, then the seven flags */
} cvx_mot_stream_header;
typedef struct cvx_mot_params {
  float iou;
  int32_t class_agnostic, max_gt_ids, max_track_ids, reserved[2];
} cvx_mot_params;
int64_t cvx_mot_state_bytes(int32_t streams, int32_t max_gt_ids, int32_t max_track_ids);
int64_t cvx_mot_workspace_bytes(int32_t streams);
int cvx_mot_frames(const float* rows, const int32_t* counts, const int32_t* ids, int32_t batch, int32_t max_det, const float* gt,
                   const int32_t* gt_counts, int32_t max_gt, const int32_t* frame_stream, int32_t streams, const cvx_mot_params* params, void* state,
                   void* workspace, int64_t workspace_bytes, void* hip_stream);
int cvx_mot_summary(void* state, int32_t streams, int32_t max_gt_ids, int32_t max_track_ids, int64_t* table, void* hip_stream);

/* (The tile-resident chain kernel's unit entry points -- cvx_chain_pair_unit / _conv_unit / _detect_unit, csrc/conv_chain.hip -- live in
 * include/cvx_engine_experimental.h: the kernel measured slower than the per-layer launches and is built into the tuning library only.) */


#ifdef __cplusplus
}
#endif
#endif /* CVX_ENGINE_H */
