/*
 * b2h.h -- C ABI of libb2h.so, the MI355X (gfx950) body->hand keypoint path.
 *
 * The reference (benoriol/hand_pose_sl) has no FFI: its boundary for this path
 * is the Python duck type of `ConvModel` (body2hand/src/models/HandPoseModels.py
 * :17-64).  Each entry point below names the reference interface it replaces;
 * the Python mirror that binds them with ctypes is hand_pose_sl_amd/conv_model.py
 * and INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*, NULL = the null stream);
 *   - every function returns B2H_OK (0) or a negative b2h_status; the message of
 *     the last failure on the calling thread is b2h_last_error();
 *   - "device pointer" = memory of the current HIP device (hipMalloc or a
 *     PyTorch-ROCm tensor's data_ptr()); the library never frees caller memory;
 *   - launches are asynchronous on `stream`; nothing here synchronises the
 *     device except b2h_load_weights (a one-off staging copy) and b2h_stream_sync.
 */
#ifndef B2H_H_
#define B2H_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B2H_VERSION 100 /* 0.1.0 */

typedef enum b2h_status {
    B2H_OK = 0,
    B2H_ERR_INVALID = -1,     /* bad argument (the Python mirror raises ValueError)   */
    B2H_ERR_SHAPE = -2,       /* shape the model cannot take (RuntimeError)           */
    B2H_ERR_NO_WEIGHTS = -3,  /* forward before b2h_load_weights                      */
    B2H_ERR_HIP = -4,         /* a HIP runtime call failed                            */
    B2H_ERR_NO_DEVICE = -5,   /* no gfx950 device visible                             */
    B2H_ERR_UNSUPPORTED = -6  /* kernel variant cannot run this configuration         */
} b2h_status;

/* Which hand-written kernel computes the four-layer stack. */
typedef enum b2h_kernel {
    B2H_KERNEL_AUTO = 0,      /* the faster exact-fp32 kernel for the model's width: F32_MFMA, except
                                 F32_VALU at conv_channels <= 8 and 33..39 (measured crossovers) and above
                                 64 (the only kernel there) */
    B2H_KERNEL_F32_VALU = 1,  /* fp32 FMA on the vector ALU; any conv_channels <= 128 (cross-check kernel,
                                 and the whole path for 65..128 channels) */
    B2H_KERNEL_F32_MFMA = 2,  /* exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32); any conv_channels <= 64
                                 (33..64: a one-wave-per-SIMD wide variant) */
    B2H_KERNEL_BF16_MFMA = 3, /* bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16); any
                                 conv_channels <= 64 (33..64: the wide kernel, two k-steps per tap) */
    B2H_KERNEL_F16_MFMA = 4,  /* fp16 operands, fp32 accumulate (v_mfma_f32_16x16x32_f16); <= 64 likewise */
    B2H_KERNEL_F16X3_MFMA = 5 /* any conv_channels <= 64 (33..64: a one-wave-per-SIMD wide variant).
                                 fp32-grade: every operand split into f16 hi + lo, three f16 MFMAs per
                                 product (hi.hi + hi.lo + lo.hi), fp32 accumulate; needs |x| < 65504:
                                 a model with a weight outside that range is refused
                                 (B2H_ERR_UNSUPPORTED), an activation beyond it becomes inf / NaN */
} b2h_kernel;

/* Pre/post-processing fused around the stack (b2h_forward_fused). */
enum {
    B2H_PRE_CHEST_DIFF = 1,   /* body -= body[:, 1]  ChestDifference, steps/utils.py:203-210 */
    B2H_PRE_NORMALIZE = 2,    /* body /= factor      NormalizeFixedFactor, steps/utils.py:180-190 */
    B2H_POST_DENORMALIZE = 4, /* pred *= factor      steps/traintest.py:270-271,387-388 */
    B2H_POST_MASK_TAIL = 8    /* pred[i, n_frames[i]:] = 0   mask_output, steps/utils.py:309-312 */
};

typedef struct b2h_model b2h_model; /* opaque; owns the packed device weights */

/* Library / device ------------------------------------------------------- */

int b2h_version(void);
/* 0 for the shipped library.  Non-zero = a development build with parts of a kernel removed or instrumented
 * (csrc/dev/b2h_dev.h, B2H_ABLATE): its results may be WRONG by construction; the Python binding refuses to
 * load such a library unless B2H_ALLOW_ABLATE=1 is set (the measurement scripts under tools/ set it). */
int b2h_build_flags(void);
const char* b2h_last_error(void);
/* Number of visible HIP devices whose arch is gfx950 (0 when none). */
int b2h_device_count(void);

/* Model lifetime ---------------------------------------------------------
 * Replaces ConvModel.__init__(conv_channels, activation, pos_emb)
 * (HandPoseModels.py:18-37).  `activation` must be "ReLU" (B2H_ERR_INVALID
 * otherwise, mirroring the ValueError at :34-37).  1 <= conv_channels <= 128 (the reference's
 * --conv-channels is a free integer, default 30: run.py:37); the matrix-core kernels cover 1..64.
 * The model is bound to the HIP device current at creation; b2h_forward / b2h_forward_fused (and
 * b2h_tenc_forward for its model) return B2H_ERR_INVALID when called while another device is current. */
int b2h_create(int conv_channels, const char* activation, int pos_emb, b2h_model** out);
int b2h_destroy(b2h_model* m);

/* Replaces model.load_state_dict(...) (infer_utterance.py:109,
 * infer_utterance_h5.py:113, steps/traintest.py:62).  Tensors are fp32,
 * contiguous, in the reference's state_dict layout:
 *   w1 (C, 24|25, 5)  b1 (C)   w2, w3 (C, C, 5)  b2, b3 (C)   w4 (42, C, 5)  b4 (42)
 * `on_device` != 0: the eight pointers are device pointers, else host pointers.
 * Repacks into the kernels' fragment layouts (fp32 / bf16 / fp16) and uploads;
 * synchronous.  May be called again to replace the weights. */
int b2h_load_weights(b2h_model* m, const float* w1, const float* b1, const float* w2,
                     const float* b2, const float* w3, const float* b3, const float* w4,
                     const float* b4, int on_device);

/* Replaces ConvModel.forward(inp) (HandPoseModels.py:40-64), inference only.
 *   x : device, fp32, (B, T, 12, 2) contiguous  -- read only
 *   y : device, fp32, (B, T, 21, 2) contiguous  -- written (value-identical to
 *       the reference's non-contiguous view, :60-62)
 * T >= 1; pos_emb models require T == 100 (B2H_ERR_SHAPE, as torch.cat raises
 * in the reference, :78-84).  B == 0 is a no-op.  x and y must be 16-byte aligned and must
 * not overlap (B2H_ERR_INVALID otherwise).
 * Streams: a BF16_MFMA / F16_MFMA launch of <= 32 channels with >= 256 chunks per CU (e.g. >= 65 536 sequences of
 * <= 208 frames on 256 CUs) hands out its work dynamically, through a claim counter in device memory that the
 * model keeps per stream HANDLE VALUE (64 per model).  Launches on further handles, on hipStreamPerThread (one
 * value for a different stream in every host thread) and on a stream under capture use the static distribution
 * (same bits, 1-3 % slower).  The counter assumes that one handle value is one ordered queue, so a caller must
 * not pass one model a handle value that names different streams at the same time (other than
 * hipStreamPerThread).  Destroying a stream and creating one that reuses its value is safe: ROCm's
 * hipStreamDestroy waits for the stream's work (tests/test_poisoned_buffers.py pins both). */
int b2h_forward(b2h_model* m, const float* x, float* y, int64_t B, int64_t T, int kernel,
                void* stream);

/* Forward with the reference's item transforms and de-normalisation fused in
 * (run.py:85-90,102 order):
 *   body : device fp32 (B, T, 12, 2) raw pixel keypoints
 *   y    : device fp32 (B, T, 21, 2)
 *   flags: OR of B2H_PRE_* / B2H_POST_*;  factor: 1280 in the reference
 *   n_frames: device int64 (B) valid lengths, or NULL (required by MASK_TAIL) */
int b2h_forward_fused(b2h_model* m, const float* body, float* y, int64_t B, int64_t T,
                      int flags, float factor, const int64_t* n_frames, int kernel,
                      void* stream);

/* Target transform of the training item (right hand relative to the wrist):
 *   hand_out = (hand - body[:, 4]) / factor     WristDifference + Normalize,
 * steps/utils.py:194-201,180-190.  flags: bit0 wrist diff, bit1 normalize.
 *   body (B,T,12,2), hand / hand_out (B,T,21,2), all device fp32, no alignment beyond fp32's 4 bytes. */
int b2h_target_transform(const float* body, const float* hand, float* hand_out, int64_t B,
                         int64_t T, int flags, float factor, void* stream);

/* Evaluation metric of the reference: maskedPoseL1 (steps/utils.py:413-428) --
 *   loss = mean_i( mean(|pred[i, :n_frames[i]] - target[i, :n_frames[i]]|) ),  i < B.
 * pred, target: device fp32 (B, T, 21, 2); n_frames: device int64 (B) or NULL (= T);
 * per_seq: device fp32 (B) scratch that receives the per-sequence means; loss: device fp32 (1).
 * A sequence with n_frames 0 contributes NaN, as torch's mean of an empty tensor does.  The float pointers of the four
 * metric entry points need no alignment beyond fp32's 4 bytes, n_frames its int64's 8.
 * "Pixel distance" (L12Pixels, steps/utils.py:291-299) is loss / 21 * 1280 on the host. */
int b2h_masked_l1(const float* pred, const float* target, const int64_t* n_frames, int64_t B,
                  int64_t T, float* per_seq, float* loss, void* stream);

/* The evaluation loop's other loss, `--loss confL1` = poderatedPoseL1 (steps/utils.py:431-452;
 * chosen at traintest.py:41-42,207-208):
 *   loss = sum_i( mean(|pred[i, :n_i] * s[i, :n_i, :, None] - target[i, :n_i] * s[i, :n_i, :, None]|) )
 * -- a SUM over the batch (the class does not divide by B).  scores: device fp32 (B, T, 21), the
 * OpenPose confidence of each target joint; everything else as b2h_masked_l1. */
int b2h_weighted_l1(const float* pred, const float* target, const float* scores, const int64_t* n_frames,
                    int64_t B, int64_t T, float* per_seq, float* loss, void* stream);
/* The same two losses over (B, T, n_joints, 2) predictions, 1 <= n_joints <= 1024 (scores (B, T, n_joints)): the
 * targets of `--predict right_index` (4 joints) and `right_3fingers` (12) beside the whole hand's 21
 * (L12Pixels(4 | 12 | 21, 1280), traintest.py:21-28).  b2h_masked_l1 / b2h_weighted_l1 are these with 21. */
int b2h_masked_l1_joints(const float* pred, const float* target, const int64_t* n_frames, int64_t B, int64_t T,
                         int n_joints, float* per_seq, float* loss, void* stream);
int b2h_weighted_l1_joints(const float* pred, const float* target, const float* scores, const int64_t* n_frames,
                           int64_t B, int64_t T, int n_joints, float* per_seq, float* loss, void* stream);

/* Training (ConvModel) ------------------------------------------------------
 * The reference trains ConvModel with the loop body of steps/traintest.py:111-121:
 *   prediction = model(body_kp); mask_output(...); loss = criterion(...); loss.backward(); optimizer.step()
 * These entry points are that forward and backward (HandPoseModels.py:40-64 under autograd) and the
 * gradients of its two losses (steps/utils.py:413-452).  All arithmetic is exact fp32 (VALU FMA),
 * whatever kernel the inference path uses.  They read the weights straight from the caller's eight
 * fp32 tensors, never from the model's packed buffers: b2h_load_weights is not needed (nor called),
 * and an optimizer may update the tensors in place between launches.
 * b2h_adam_step below is that optimizer: torch.optim.Adam's update of every tensor in one launch.
 *   params: host array of the 8 device fp32 tensors in state_dict order (w1, b1, ..., w4, b4), layouts
 *           as b2h_load_weights.
 * Like b2h_forward they are stream-ordered and asynchronous: none synchronises, allocates or reads
 * device memory on the host, so they can be captured into a HIP graph.  Arguments are checked as
 * b2h_forward checks them (current device, 16-byte alignment of x / y / dy / dx / workspace, no overlap
 * of an output with any operand, T == 100 for pos_emb models: B2H_ERR_SHAPE). */

/* y = ConvModel(x), HandPoseModels.py:40-64: x (B, T, 12, 2) -> y (B, T, 21, 2), device fp32.
 * Saves nothing for the backward pass (b2h_backward recomputes what it needs).  B == 0 is a no-op. */
int b2h_train_forward(b2h_model* m, const float* const* params, const float* x, float* y, int64_t B,
                      int64_t T, void* stream);
/* Bytes of device workspace b2h_backward needs for a (B, T) batch of this model (0 for B < 1). */
size_t b2h_backward_workspace_bytes(const b2h_model* m, int64_t B, int64_t T);
/* loss.backward() through ConvModel.forward (HandPoseModels.py:40-64 under autograd), B >= 1:
 *   dy    : device fp32 (B, T, 21, 2), dL/dy
 *   dx    : device fp32 (B, T, 12, 2) dL/dx, or NULL; with pos_emb the constant channel 0 gets none
 *   grads : host array of 8 device fp32 tensors shaped like params, OVERWRITTEN (not accumulated)
 * Deterministic: the frame tiles and their per-workgroup partial sums in `workspace` depend on (B, T)
 * and the width only, and a second kernel adds those partials in a fixed order (no atomics), so the
 * same inputs give the same bits on any device and stream; dx of a sequence does not depend on the
 * other sequences of the batch.  The workspace's prior contents do not matter. */
int b2h_backward(b2h_model* m, const float* const* params, const float* x, const float* dy, float* dx,
                 float* const* grads, int64_t B, int64_t T, void* workspace, size_t workspace_bytes,
                 void* stream);
/* dL/dpred of maskedPoseL1 (steps/utils.py:413-428, used at traintest.py:111-121):
 *   dpred[i, t < n_i] = (g / B) * sign(pred - target) / (n_i * 42),  0 at t >= n_i,
 * g = *dloss (device fp32 scalar: no host read); n_frames as b2h_masked_l1 (NULL = T, clamped to
 * [0, T] as slicing does); sign(0) = 0 as torch.nn.L1Loss has it.  A sequence with n_i = 0
 * contributes no gradient (its forward loss is NaN).  pred, target and dpred of the four gradient entry points must be
 * 16-byte aligned and dpred must overlap no input (B2H_ERR_INVALID); scores and dloss are fp32 (4 bytes), n_frames int64. */
int b2h_masked_l1_backward(const float* pred, const float* target, const int64_t* n_frames, int64_t B,
                           int64_t T, const float* dloss, float* dpred, void* stream);
/* dL/dpred of poderatedPoseL1 (steps/utils.py:431-452): with s = scores[i, t, joint],
 *   dpred[i, t < n_i] = g * sign(pred * s - target * s) / (n_i * 42) * s   (no / B: the class sums). */
int b2h_weighted_l1_backward(const float* pred, const float* target, const float* scores,
                             const int64_t* n_frames, int64_t B, int64_t T, const float* dloss,
                             float* dpred, void* stream);
/* The two gradients over (B, T, n_joints, 2), as b2h_masked_l1_joints; the two above are these with 21 (42 in their
 * formulas is 2 * n_joints). */
int b2h_masked_l1_joints_backward(const float* pred, const float* target, const int64_t* n_frames, int64_t B,
                                  int64_t T, int n_joints, const float* dloss, float* dpred, void* stream);
int b2h_weighted_l1_joints_backward(const float* pred, const float* target, const float* scores,
                                    const int64_t* n_frames, int64_t B, int64_t T, int n_joints,
                                    const float* dloss, float* dpred, void* stream);

/* TransformerEnc -------------------------------------------
 * The reference's second text-free body->hand model, `TransformerEnc(ninp, nhead, nhid, nout,
 * nlayers, dropout)` (HandPoseModels.py:118-178), as its CLIs build it: ninp = 24, nhead = 4,
 * nhid = 128, nout = 42 (infer_utterance.py:99-101).  The entry points of this block are the inference path
 * (dropout = identity); training is b2h_tenc_train_forward / b2h_tenc_backward below.
 * b2h_tenc_create accepts exactly that geometry, 1 <= nlayers <= 16, 1 <= max_len <= 128
 * (100 in the reference, :125) and returns B2H_ERR_UNSUPPORTED for anything else. */
typedef struct b2h_tenc b2h_tenc;
/* Arithmetic of the Linear layers (attention, softmax and LayerNorm are fp32 in both):
 *   B2H_TENC_F32   fp32 operands on v_mfma_f32_16x16x4_f32 (default);
 *   B2H_TENC_F16X3 every operand split into f16 hi + lo, three v_mfma_f32_16x16x32_f16 per product
 *                  (hi.hi + hi.lo + lo.hi, fp32 accumulate): fp32-grade error (22 significant
 *                  bits per operand) at 3/16 of the matrix cycles, valid while every activation
 *                  and weight is below 65504 in magnitude (f16 range): b2h_tenc_forward returns
 *                  B2H_ERR_UNSUPPORTED for a model with a parameter outside it. */
typedef enum b2h_tenc_kernel { B2H_TENC_F32 = 0, B2H_TENC_F16X3 = 1 } b2h_tenc_kernel;
int b2h_tenc_create(int ninp, int nhead, int nhid, int nout, int nlayers, int max_len, b2h_tenc** out);
int b2h_tenc_destroy(b2h_tenc* m);
/* Selects the kernel for later b2h_tenc_forward calls (no reload of the weights needed). */
int b2h_tenc_set_kernel(b2h_tenc* m, int kernel);
/* Replaces load_state_dict.  `tensors`: 5 + 12*nlayers fp32 contiguous arrays in this order
 * (state_dict names of the reference):
 *   pos_encoder.pe (max_len,1,24); pose2hidden_projection.weight (128,24), .bias (128);
 *   per layer i, transformer_encoder.layers.i.: self_attn.in_proj_weight (384,128),
 *     self_attn.in_proj_bias (384), self_attn.out_proj.weight (128,128), self_attn.out_proj.bias,
 *     linear1.weight (128,128), linear1.bias, linear2.weight (128,128), linear2.bias,
 *     norm1.weight, norm1.bias, norm2.weight, norm2.bias (128 each);
 *   hidden2pose_projection.weight (42,128), .bias (42). */
int b2h_tenc_load_weights(b2h_tenc* m, const float* const* tensors, int count, int on_device);
/* Bytes of device scratch b2h_tenc_forward needs for a (B, T) batch (2560 B per frame). */
size_t b2h_tenc_workspace_bytes(const b2h_tenc* m, int64_t B, int64_t T);
/* Replaces TransformerEnc.forward(src) (HandPoseModels.py:152-178): x (B,T,12,2) -> y (B,T,21,2),
 * device fp32.  T <= max_len (the reference's `src + pe[:T]` raises beyond it): B2H_ERR_SHAPE.
 * `workspace`: device memory of at least b2h_tenc_workspace_bytes(m, B, T).  x and the workspace must be 16-byte aligned
 * (B2H_ERR_INVALID otherwise); y needs no alignment beyond its fp32's 4 bytes (its stores are buffer stores). */
int b2h_tenc_forward(b2h_tenc* m, const float* x, float* y, int64_t B, int64_t T, void* workspace,
                     size_t workspace_bytes, void* stream);

/* TransformerEnc forward with the reference's item transforms fused into its first and last kernel
 * (SURVEY.md 8f N1 for the second model; order of run.py:85-90,102 and traintest.py:270-271):
 *   body: device fp32 (B, T, 12, 2) raw pixel keypoints; flags / factor / n_frames as for
 *   b2h_forward_fused -- B2H_PRE_CHEST_DIFF and B2H_PRE_NORMALIZE are applied to the rows as they
 *   enter the model, BEFORE the positional encoding is added (HandPoseModels.py:167);
 *   B2H_POST_DENORMALIZE and B2H_POST_MASK_TAIL in the store of hidden2pose_projection's output. */
int b2h_tenc_forward_fused(b2h_tenc* m, const float* body, float* y, int64_t B, int64_t T, int flags,
                           float factor, const int64_t* n_frames, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Training (TransformerEnc) ----------------------------------------------------
 * The reference trains TransformerEnc with the same loop body as ConvModel (steps/traintest.py:87-121), the
 * model built with dropout = --transformer-dropout.  These entry points are its forward in .train() mode and
 * its backward (HandPoseModels.py:154-178 under autograd: PositionalEncoding :101-103 with its dropout,
 * pose2hidden_projection, torch's post-norm nn.TransformerEncoderLayer with ReLU, hidden2pose_projection).
 * All arithmetic is exact fp32, whatever b2h_tenc_set_kernel selected: on the vector ALU by default, the attentions
 * and the Linear layers on the matrix cores after b2h_tenc_set_train_kernel / b2h_tenc_set_train_linear (declared with
 * the TextPoseTransformer switches below).  The parameters are
 * read straight from the caller's tensors (b2h_tenc_load_weights is neither needed nor called), so an
 * optimizer may update them in place between launches.
 * b2h_adam_step below is that optimizer: torch.optim.Adam's update of every tensor in one launch.
 *   params: host array of the 5 + 12*nlayers device fp32 tensors in the order of b2h_tenc_load_weights
 *           (pos_encoder.pe first), 4-byte aligned.
 *   p     : the dropout probability (the reference passes one value everywhere), 0 <= p <= 1.
 *   masks : NULL when p == 0 (nothing is dropped or scaled); else a host array of 1 + 4*nlayers device
 *           uint8 keep-masks (1 = keep; kept values are scaled by 1 / (1 - p), everything is dropped at
 *           p == 1).  b2h_dropout_masks below draws them and b2h_tenc_mask_numel gives their element counts; a
 *           caller may as well fill them from a generator of its own.  In this order:
 *             pos (B, T, 24); then per layer: attn (B, 4, T, T) on the softmax probabilities,
 *             drop1 (B, T, 128) on out_proj's output, ff (B, T, 128) after linear1's ReLU,
 *             drop2 (B, T, 128) on linear2's output.
 *           The masks need no alignment (they are bytes); those of b2h_dropout_masks are 16-byte aligned.
 * Like b2h_tenc_forward they are stream-ordered and asynchronous: none synchronises, allocates or reads
 * device memory on the host, so they can be captured into a HIP graph.  1 <= T <= max_len; x, y, dy, dx, the
 * saved buffer and the scratch must be 16-byte aligned and no output may overlap another operand
 * (B2H_ERR_INVALID). */

/* Sizes of what autograd keeps for the reference between `prediction = model(body_kp)` and `loss.backward()`
 * (steps/traintest.py:94,119: the activations of HandPoseModels.py:154-178), which the caller owns here.
 * Bytes a (B, T) batch needs: which = 0, the saved-activation buffer b2h_tenc_train_forward fills for
 * b2h_tenc_backward (608 + 4624*nlayers bytes per frame); which = 1, the scratch of b2h_tenc_backward.
 * 0 for a NULL model, B < 1, T < 1 or another `which`. */
size_t b2h_tenc_train_bytes(const b2h_tenc* m, int64_t B, int64_t T, int which);
/* y = TransformerEnc(x) in .train() mode with the given dropout masks, HandPoseModels.py:154-178:
 * x (B, T, 12, 2) -> y (B, T, 21, 2), device fp32; fills `saved` (device, >= b2h_tenc_train_bytes(m, B, T, 0)).
 * B == 0 is a no-op. */
int b2h_tenc_train_forward(b2h_tenc* m, const float* const* params, const float* x, const uint8_t* const* masks,
                           float p, float* y, void* saved, size_t saved_bytes, int64_t B, int64_t T, void* stream);
/* loss.backward() through TransformerEnc.forward (HandPoseModels.py:154-178 under autograd,
 * traintest.py:111-121), B >= 1.  Needs neither x nor y: the loop overwrites the prediction's tail in place
 * (mask_output, steps/utils.py:309-312) before the loss.
 *   masks, p: the same as in the forward;  dy: device fp32 (B, T, 21, 2), dL/dy
 *   saved   : what b2h_tenc_train_forward wrote for this batch (read only)
 *   dx      : device fp32 (B, T, 12, 2) dL/dx, or NULL
 *   grads   : host array of 4 + 12*nlayers device fp32 tensors shaped like params without pe (a buffer: no
 *             gradient), OVERWRITTEN (not accumulated)
 *   scratch : device, >= b2h_tenc_train_bytes(m, B, T, 1); its prior contents do not matter.
 * Deterministic: the per-workgroup partial sums of the parameter gradients depend on (B, T) only and are
 * added in a fixed order by a second kernel (no atomics), so the same inputs give the same bits on any
 * device and stream; dx of a sequence does not depend on the other sequences of the batch. */
int b2h_tenc_backward(b2h_tenc* m, const float* const* params, const uint8_t* const* masks, float p,
                      const float* dy, const void* saved, size_t saved_bytes, float* dx, float* const* grads,
                      void* scratch, size_t scratch_bytes, int64_t B, int64_t T, void* stream);

/* TextPoseTransformer --------------------------------------------------------
 * The reference's text-conditioned model and the default of its CLIs (`--model TextPoseTransformer`,
 * run.py:32-36,148-151; infer_utterance.py:27-28,102-103): `TextPoseTransformer(n_tokens, n_joints, joints_dim,
 * nhead, nhid, nout, n_enc_layers, n_dec_layers, dropout)` (HandPoseModels.py:181-230) = a token embedding (not
 * scaled), pose2hidden_projection, torch.nn.Transformer(nhid, nhead, n_enc_layers, n_dec_layers, nhid) with the
 * token embeddings as source and the projected pose as target, hidden2pose_projection.  Post-norm layers, ReLU,
 * eps 1e-5, both stacks end with their LayerNorm; the reference passes no mask of any kind (:211), so padded
 * token id 0 is attended like any other, and never applies its two positional encodings.  The entry points of
 * this block are the inference path (dropout = identity); training is b2h_tpt_train_forward / b2h_tpt_backward
 * below.  Tokenisation stays with the caller: the model's boundary is integer ids (:201, traintest.py:105-107).
 * Two arithmetics, the b2h_tenc_kernel values above: B2H_TENC_F32, exact fp32 on the matrix cores, is the default
 * and stays it; B2H_TENC_F16X3 (b2h_tpt_set_kernel) splits every operand of every Linear and of both attention
 * products into f16 hi + lo and uses three v_mfma_f32_16x16x32_f16 per product with fp32 accumulation, projects
 * Q, K and V inside the attention kernels (self- and cross-attention) and keeps the same 2e-5 parity bar.  It is
 * valid while every weight, embedding row and activation is below 65504 in magnitude (f16 range):
 * b2h_tpt_forward returns B2H_ERR_UNSUPPORTED for a model with a parameter outside it. */
typedef struct b2h_tpt b2h_tpt;
/* Replaces TextPoseTransformer.__init__ (HandPoseModels.py:181-230) as run.py:148-151 calls it.  `ninp` is
 * n_joints * joints_dim.  Accepts the geometries the reference's CLIs build, in any combination:
 *   ninp in {16, 24, 42, 58}: 8 body joints (run.py:100-101, infer_utterance_h5.py:83-84), 12 body joints
 *                             (infer_utterance.py:79-80), 21 = 9 hand + 12 body (`--predict right_3fingers`,
 *                             run.py:96-97), 29 = 12 body + 17 hand (`--predict right_index`, run.py:92-93)
 *   nout in {8, 24, 42}     : 4 (right_index), 12 (right_3fingers) or 21 (right_hand) joints x 2
 * with nhead = 4, nhid = 128, 1 <= n_enc_layers, n_dec_layers <= 16 and n_tokens >= 1; B2H_ERR_UNSUPPORTED for
 * anything else.  Wherever this header writes (B, T, 12, 2) and (B, T, 21, 2) for this model's input and output,
 * read (B, T, ninp / 2, 2) and (B, T, nout / 2, 2).  Bound to the current HIP device. */
int b2h_tpt_create(int n_tokens, int ninp, int nhead, int nhid, int nout, int n_enc_layers, int n_dec_layers,
                   b2h_tpt** out);
int b2h_tpt_destroy(b2h_tpt* m);
/* Selects the kernel (a b2h_tenc_kernel value) for later b2h_tpt_forward calls; no reload of the weights needed.
 * B2H_ERR_INVALID for a NULL model or an unknown value.  Training is exact fp32 whatever is selected. */
int b2h_tpt_set_kernel(b2h_tpt* m, int kernel);
/* Replaces load_state_dict for this model (HandPoseModels.py:181-230; traintest.py:62).  `tensors`:
 * 9 + 12*n_enc_layers + 18*n_dec_layers fp32 contiguous arrays in state_dict order WITHOUT the two `pe` buffers
 * (token_pos_encoder.pe, pose_pos_encoder.pe: constructed at :187-190, never applied):
 *   per encoder layer i, transformer.encoder.layers.i.: self_attn.in_proj_weight (384,128), .in_proj_bias (384),
 *     self_attn.out_proj.weight (128,128), .bias, linear1.weight (128,128), .bias, linear2.weight (128,128), .bias,
 *     norm1.weight, .bias, norm2.weight, .bias (128 each);
 *   transformer.encoder.norm.weight, .bias;
 *   per decoder layer i, transformer.decoder.layers.i.: self_attn.* (4 tensors as above), multihead_attn.* (the same
 *     4 shapes), linear1.*, linear2.*, norm1.*, norm2.*, norm3.*;
 *   transformer.decoder.norm.weight, .bias;
 *   token_embedding.weight (n_tokens,128); hidden2pose_projection.weight (nout,128), .bias (nout);
 *   pose2hidden_projection.weight (128,ninp), .bias (128).
 * `on_device` as for b2h_load_weights; synchronous; may be called again to replace the weights. */
int b2h_tpt_load_weights(b2h_tpt* m, const float* const* tensors, int count, int on_device);
/* Bytes of device scratch b2h_tpt_forward and b2h_tpt_forward_fused need: a function of (B, S, T) and the layer
 * counts only -- B*S*(2560 + 1024*n_dec_layers) + B*T*3584, i.e. 2560 + 1024*n_dec_layers per token and 3584 per
 * frame, for every T (the kernels for T > 128 use the regions the fp32 path already has: Q | K | V rows, the cross
 * query and the memory's K | V; they need nothing more).  A model with ninp 42 or 58 adds 256 per frame: the chain
 * kernel reads its pose rows from a copy at a 64-float pitch.  0 for a NULL model or a negative size. */
size_t b2h_tpt_workspace_bytes(const b2h_tpt* m, int64_t B, int64_t S, int64_t T);
/* Replaces TextPoseTransformer.forward(input_tokens, input_pose) (HandPoseModels.py:181-230, :201-222; called at
 * traintest.py:105-107 and through run.py:148-151):
 *   tokens : device int64 (B, S) token ids  -- read only.  An id outside [0, n_tokens) never reads outside the
 *            embedding table: the whole output of ITS sequence becomes NaN, no other sequence is touched
 *            (nn.Embedding raises on the host; this entry point does not synchronise)
 *   x      : device fp32 (B, T, 12, 2)      -- read only
 *   y      : device fp32 (B, T, 21, 2)      -- written
 * 1 <= S <= 128 and 1 <= T <= 128 (B2H_ERR_SHAPE; the reference's datasets feed S = 40, T = 100:
 * text_pose_dataset.py:467-470).  B == 0 is a no-op.  x and the workspace must be 16-byte aligned, tokens and y
 * 8-byte aligned.  `workspace`: device memory of at least b2h_tpt_workspace_bytes(m, B, S, T); its prior contents
 * do not matter.  Stream-ordered and asynchronous, no atomics: the same inputs give the same bits on any stream,
 * and a sequence's output does not depend on the rest of the batch. */
int b2h_tpt_forward(b2h_tpt* m, const int64_t* tokens, const float* x, float* y, int64_t B, int64_t S,
                    int64_t T, void* workspace, size_t workspace_bytes, void* stream);
/* The same forward with the reference's item transforms inside the model's own kernels and with long targets:
 * what `infer_utterance.py` runs around its default model at its default `--max-frames 200`.
 *   body    : device fp32 (B, T, 12, 2), raw pixel keypoints (or already transformed ones with flags = 0)
 *   flags, factor, n_frames: as for b2h_tenc_forward_fused.  B2H_PRE_CHEST_DIFF and B2H_PRE_NORMALIZE are applied to
 *             the pose rows as they enter pose2hidden_projection (the model adds no positional encoding),
 *             B2H_POST_DENORMALIZE and B2H_POST_MASK_TAIL (needs n_frames, device int64 (B)) in the store of
 *             hidden2pose_projection's output.
 * 1 <= S <= 128 and 1 <= T <= B2H_TPT_MAX_FRAMES (B2H_ERR_SHAPE).  Everything else -- tokens, alignment, NULL
 * rules, B == 0, the workspace, token ids outside the table, determinism -- is as for b2h_tpt_forward.  With
 * flags == 0 and T <= 128 it launches exactly what b2h_tpt_forward launches: the same bits.  For T > 128 the
 * decoder's self-attention walks the keys in blocks with an online softmax (b2h_attn_long_f32 / b2h_attn_long_h3);
 * in B2H_TENC_F16X3 the Q, K, V projections then run in the per-frame chain instead of inside the attention kernel.
 * b2h_tpt_forward itself keeps T <= 128 because a pinned test requires its refusal of T = 129; a later change
 * allowed to touch that test should route it here. */
#define B2H_TPT_MAX_FRAMES 1024
int b2h_tpt_forward_fused(b2h_tpt* m, const int64_t* tokens, const float* body, float* y, int64_t B, int64_t S,
                          int64_t T, int flags, float factor, const int64_t* n_frames, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The B2H_PRE_* flags transform body-only rows (ninp 16 or 24: ChestDifference has the chest at joint 1 of either).
 * A model with ninp 42 or 58 answers them with B2H_ERR_INVALID: its rows are made by b2h_tpt_build_item, which
 * applies them, and enter b2h_tpt_forward_fused with the B2H_POST_* flags only. */

/* Key-padding masks as key lengths.  The reference pads every sentence to 40 ids with 0 and every utterance to
 * --max-frames with zero rows and calls nn.Transformer without a mask, so the padding is attended.  Padding here is
 * always a suffix, so torch's three boolean masks are one length per sequence: for an attention over Tk key rows and a
 * device array klen (int64 (B), 8-byte aligned) sequence b attends to its key rows 0 .. kl - 1 only, with
 *   kl = clamp(klen[b], 1, Tk)        -- torch's key_padding_mask[b][j] = (j >= kl).
 * Keys from kl on have probability exactly 0 and are not read; all query rows are computed, padded ones included
 * (finite, as in torch).  One deviation from torch: a length of 0 counts as 1 (torch gives NaN for a row with every key
 * masked); a length above Tk counts as Tk.
 *   text_len  : the encoder's self-attention (src_key_padding_mask) and the decoder's cross-attention
 *               (memory_key_padding_mask);  frame_len: the decoder's self-attention (tgt_key_padding_mask).
 * Either may be NULL on its own; with both NULL every entry point below is its parent, launch for launch and bit
 * for bit.  A model trained with masks must be run with masks.
 *
 * lengths[b] = 1 + (last s with tokens[b][s] != pad_id), 1 if every id is pad_id: the text_len of token rows padded
 * at the end with pad_id (0 in the reference, which is also its tokenizer's <unk>: a sentence that really ends in
 * <unk> loses those tokens).  tokens (B, S) and lengths (B): device int64, 8-byte aligned, not overlapping
 * (B2H_ERR_INVALID); B >= 0, S >= 1 (B2H_ERR_SHAPE); B == 0 is a no-op.  One launch, capturable. */
int b2h_token_lengths(const int64_t* tokens, int64_t B, int64_t S, int64_t pad_id, int64_t* lengths, void* stream);
/* b2h_tpt_forward_fused with key lengths; n_frames (B2H_POST_MASK_TAIL) stays an argument of its own, usually the same
 * array as frame_len.  Exact fp32 only: with B2H_TENC_F16X3 selected and a non-NULL length it returns
 * B2H_ERR_UNSUPPORTED -- call b2h_tpt_set_kernel(m, B2H_TENC_F32).  Neither y nor the workspace may overlap a length
 * array (B2H_ERR_INVALID).  A sequence's output is the same bits alone and inside any batch, as without lengths. */
int b2h_tpt_forward_masked(b2h_tpt* m, const int64_t* tokens, const float* body, float* y, int64_t B, int64_t S,
                           int64_t T, int flags, float factor, const int64_t* n_frames, const int64_t* text_len,
                           const int64_t* frame_len, void* workspace, size_t workspace_bytes, void* stream);

/* The geometry of a model and whether weights are loaded; any output pointer may be NULL. */
int b2h_tpt_info(const b2h_tpt* m, int* n_tokens, int* ninp, int* nout, int* n_enc_layers, int* n_dec_layers,
                 int* has_weights);

/* The model input of `--predict right_index` / `right_3fingers` from raw body and right-hand keypoints, in the
 * order of run.py:85-104: WristDifference on the hand with the RAW body wrist (joint 4) and ChestDifference on the
 * body (B2H_PRE_CHEST_DIFF, steps/utils.py:194-210), / factor on both (B2H_PRE_NORMALIZE), then
 *   B2H_PREDICT_RIGHT_INDEX    (BuildIndexItem, :217-236)  : body 0..11, hand 0..4, hand 9..20      -> (B, T, 29, 2)
 *   B2H_PREDICT_RIGHT_3FINGERS (Build3fingerItem, :238-259): hand 13..20, hand 0, body 0..11        -> (B, T, 21, 2)
 *   body (B, T, 12, 2), right_hand (B, T, 21, 2), item: device fp32, 8-byte aligned, item overlapping neither input.
 * flags: B2H_PRE_* only.  Every element is one subtraction and one true division: equal to torch's, bit for bit. */
enum b2h_predict { B2H_PREDICT_RIGHT_HAND = 0, B2H_PREDICT_RIGHT_INDEX = 1, B2H_PREDICT_RIGHT_3FINGERS = 2 };
int b2h_tpt_build_item(const float* body, const float* right_hand, float* item, int64_t B, int64_t T, int predict,
                       int flags, float factor, void* stream);

/* Training (TextPoseTransformer) -------------------------------------------------
 * The reference trains its default model with `prediction = model(batch["text_tokens"], batch["input_kp"])`,
 * mask_output, the criterion, loss.backward() and optimizer.step() (traintest.py:105-121).  These entry points
 * are TextPoseTransformer.forward in .train() mode (HandPoseModels.py:201-222 under autograd: token_embedding,
 * pose2hidden_projection, torch's post-norm nn.Transformer with ReLU and its two final LayerNorms,
 * hidden2pose_projection) and its backward, built like the TransformerEnc pair above: exact fp32 on the
 * vector ALU, one kernel per operation, the parameters read straight from the caller's tensors
 * (b2h_tpt_load_weights is neither needed nor called).
 * b2h_adam_step below is that optimizer: torch.optim.Adam's update of every tensor in one launch.
 *   params: host array of the 9 + 12*n_enc_layers + 18*n_dec_layers device fp32 tensors in the order of
 *           b2h_tpt_load_weights, 4-byte aligned.
 *   tokens: device int64 (B, S), 8-byte aligned.  An id outside [0, n_tokens) never indexes anything: its
 *           sequence's y becomes NaN in the forward, and the backward skips it in the embedding gradient.
 *   p     : the dropout probability (the reference passes one value everywhere), 0 <= p <= 1.
 *   masks : NULL when p == 0; else a host array of 4*n_enc_layers + 6*n_dec_layers device uint8 keep-masks
 *           (1 = keep; kept values are scaled by 1 / (1 - p), everything is dropped at p == 1).  b2h_dropout_masks
 *           below draws them and b2h_tpt_mask_numel gives their element counts; a caller may as well fill them
 *           from a generator of its own.  In the order of torch's layers:
 *             per encoder layer: attn (B, 4, S, S), drop1, ff, drop2 (B, S, 128 each);
 *             per decoder layer: self_attn (B, 4, T, T), drop1 (B, T, 128), cross_attn (B, 4, T, S),
 *               drop2, ff, drop3 (B, T, 128 each).
 *           There is no embedding or positional mask: the reference never applies its positional encoders.  The
 *           masks need no alignment (they are bytes).
 * 1 <= S <= 128 and 1 <= T <= B2H_TPT_MAX_FRAMES (B2H_ERR_SHAPE; the reference's trainer pads every item to
 * --max-frames 200, run.py:28).  For T <= 128 each decoder attention is one workgroup per (sequence, head) with the
 * whole score matrix in LDS; for T > 128 the decoder's two attentions and their backwards walk the keys and the
 * queries in blocks (kernel_train_attn_long.h: an online softmax that saves each row's log-sum-exp, a key-owner and
 * a query-owner backward kernel that recompute the probabilities from it), and everything else is the same launch
 * list.  Stream-ordered and asynchronous: none synchronises, allocates or reads device memory on the
 * host, so they can be captured into a HIP graph.  x, y, dy, dx, the saved buffer and the scratch must be
 * 16-byte aligned and no output may overlap another operand (B2H_ERR_INVALID). */

/* Bytes a (B, S, T) batch needs, pure functions of (B, S, T) and the layer counts.
 *   which = 0, the saved-activation buffer b2h_tpt_train_forward fills for b2h_tpt_backward:
 *     B*S * (1040 + 4624*n_enc_layers + 1024*n_dec_layers) + B*T * (1040 + 4*ceil4(ninp) + 6688*n_dec_layers)
 *     (ceil4: rounded up to a multiple of 4; 1136 per frame for the default ninp = 24)
 *   which = 1, the scratch of b2h_tpt_backward, with N = max(B*S, B*T):
 *     N * 3584 + B*S * 2048 + clamp(ceil(N / 128), 1, 64) * 198144
 *   for T > 128 in addition: which = 0, B*T * 32*n_dec_layers (the log-sum-exp of every (frame, head) of both
 *     decoder attentions); which = 1, B*T * 32 (the backward's two row terms per (frame, head)).
 * 0 for a NULL model, B < 1, S < 1, T < 1 or another `which`. */
size_t b2h_tpt_train_bytes(const b2h_tpt* m, int64_t B, int64_t S, int64_t T, int which);
/* y = TextPoseTransformer(tokens, x) in .train() mode with the given dropout masks (HandPoseModels.py:201-222):
 * x (B, T, 12, 2) -> y (B, T, 21, 2), device fp32; fills `saved` (device, >= b2h_tpt_train_bytes(m, B, S, T, 0)).
 * B == 0 is a no-op. */
int b2h_tpt_train_forward(b2h_tpt* m, const float* const* params, const int64_t* tokens, const float* x,
                          const uint8_t* const* masks, float p, float* y, void* saved, size_t saved_bytes,
                          int64_t B, int64_t S, int64_t T, void* stream);
/* loss.backward() through TextPoseTransformer.forward (HandPoseModels.py:201-222 under autograd,
 * traintest.py:105-121), B >= 1.  Needs neither x nor y.
 *   tokens, masks, p: the same as in the forward;  dy: device fp32 (B, T, 21, 2), dL/dy
 *   saved   : what b2h_tpt_train_forward wrote for this batch (read only)
 *   dx      : device fp32 (B, T, 12, 2) dL/dinput_pose, or NULL
 *   grads   : host array of device fp32 tensors shaped like params, OVERWRITTEN (not accumulated); the gradient
 *             of token_embedding.weight is dense, rows of ids the batch does not contain are +0
 *   scratch : device, >= b2h_tpt_train_bytes(m, B, S, T, 1); its prior contents do not matter.
 * Deterministic (no atomics): the partial sums of the parameter gradients depend on (B, S, T) only and are
 * added in a fixed order, the embedding gradient adds its rows in ascending token position, and the memory's
 * gradient adds the decoder layers in descending order; dx of a sequence does not depend on the other
 * sequences of the batch. */
int b2h_tpt_backward(b2h_tpt* m, const float* const* params, const int64_t* tokens, const uint8_t* const* masks,
                     float p, const float* dy, const void* saved, size_t saved_bytes, float* dx,
                     float* const* grads, void* scratch, size_t scratch_bytes, int64_t B, int64_t S, int64_t T,
                     void* stream);
/* The pair with key lengths (see b2h_token_lengths above): text_len and frame_len are device int64 (B), 8-byte
 * aligned, read-only operands that no output may overlap (B2H_ERR_INVALID), each NULL or not on its own; pass the
 * backward what the forward got.  In the backward the rows kl .. Tk - 1 of every attention's dK and dV are written
 * as +0, so the gradient of a padded frame row is exactly 0 when dy is 0 there.  All four training attention routes
 * take them; the summation order of a sequence is a function of (S, T) and its own two lengths.  Capturable like their
 * parents; b2h_tpt_train_bytes is unchanged.  b2h_tpt_train_forward / b2h_tpt_backward are these with NULL, NULL. */
int b2h_tpt_train_forward_masked(b2h_tpt* m, const float* const* params, const int64_t* tokens, const float* x,
                                 const uint8_t* const* masks, float p, float* y, void* saved, size_t saved_bytes,
                                 int64_t B, int64_t S, int64_t T, const int64_t* text_len, const int64_t* frame_len,
                                 void* stream);
int b2h_tpt_backward_masked(b2h_tpt* m, const float* const* params, const int64_t* tokens, const uint8_t* const* masks,
                            float p, const float* dy, const void* saved, size_t saved_bytes, float* dx,
                            float* const* grads, void* scratch, size_t scratch_bytes, int64_t B, int64_t S, int64_t T,
                            const int64_t* text_len, const int64_t* frame_len, void* stream);
/* Which kernels the training calls use where there is a choice.  This switch covers the decoder's two attentions at
 * T > 128 (the Linear layers have a switch of their own, b2h_tpt_set_train_linear below):
 *   B2H_TRAIN_VALU  the default of every new model: kernel_train_attn_long.h, fp32 FMAs on the vector ALU
 *   B2H_TRAIN_MFMA  kernel_train_attn_mfma.h: the same grids, operands, saved layouts and mathematics with all six
 *                   products on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain); deterministic like
 *                   the default, but in its own summation order, so not bitwise equal to it
 * At T <= 128, for the encoder at every T and for b2h_tpt_train_bytes the switch has no effect.  The routes share
 * every layout, so either backward accepts either forward's saved buffer (hand_pose_sl_amd's autograd Function runs
 * a backward under the setting of its own forward, for reproducible bits).  Both routes' LDS caps are
 * raised at b2h_tpt_create, so switching between captures is safe.  B2H_ERR_INVALID: NULL model, other value. */
typedef enum b2h_train_kernel { B2H_TRAIN_VALU = 0, B2H_TRAIN_MFMA = 1 } b2h_train_kernel;
int b2h_tpt_set_train_kernel(b2h_tpt* m, int kernel);
/* Unmangled name of the decoder's self-attention forward kernel that b2h_tpt_train_forward would launch at T frames
 * under the current settings: "b2h_tt_sdpa" or, after b2h_tpt_set_train_whole below, "b2h_mw_sdpa" (T <= 128),
 * "b2h_lt_sdpa" or "b2h_mt_sdpa"; static storage, for tests and
 * for matching rocprofv3 kernel-trace rows.  NULL for a NULL model or T < 1. */
const char* b2h_tpt_train_attn_name(const b2h_tpt* m, int64_t T);
/* A second, independent switch (the same enum): which kernels run the Linear layers of the training calls, forward
 * and backward, in the encoder and the decoder at every (B, S, T):
 *   B2H_TRAIN_VALU  the default of every new model: b2h_tt_linear / _dx / _dw of kernel_tenc_train.h
 *   B2H_TRAIN_MFMA  kernel_train_linear_mfma.h: b2h_ml_linear / _dx / _dw, the same arguments, epilogues, slab
 *                   contract and per-element summation order on v_mfma_f32_16x16x4_f32 (exact fp32); as
 *                   deterministic as the default
 * It leaves alone LayerNorm, the embedding, the attentions (b2h_tpt_set_train_kernel), b2h_tpt_train_bytes and every
 * layout, inference, and TransformerEnc, which has switches of its own (below).  Either backward accepts either forward's
 * saved buffer.  Both trios' LDS caps are raised at b2h_tpt_create, so switching between captures is safe.
 * B2H_ERR_INVALID: NULL model, other value (nothing changes). */
int b2h_tpt_set_train_linear(b2h_tpt* m, int kernel);
/* Unmangled name of the Linear forward kernel that b2h_tpt_train_forward would launch under the current setting:
 * "b2h_tt_linear" or "b2h_ml_linear"; static storage.  NULL for a NULL model. */
const char* b2h_tpt_train_linear_name(const b2h_tpt* m);
/* A third, independent switch (the same enum): which whole-matrix pair runs every training attention of at most
 * 128 x 128 -- the encoder's self-attention (S x S) at every T, and at T <= 128 the decoder's self-attention (T x T)
 * and cross-attention (T x S):
 *   B2H_TRAIN_VALU  the default of every new model: b2h_tt_sdpa / _bwd of kernel_train_attn.h
 *   B2H_TRAIN_MFMA  b2h_mw_sdpa / _bwd of kernel_train_attn_whole_mfma.h: the same arguments, one workgroup per
 *                   (sequence, head), no buffer besides the operands, all six products on v_mfma_f32_16x16x4_f32 in
 *                   the default's summation order.  y is bitwise equal to the default's; the backward sums
 *                   rowsum(dSd o S) in its own fixed order, so the gradients are exact fp32 but not bitwise equal
 * At T > 128 the decoder's attentions stay with b2h_tpt_set_train_kernel.  b2h_tpt_train_bytes does not depend on the
 * switch (the pair needs no LSE or D buffer), so either backward accepts either forward's saved buffer.  Both pairs'
 * LDS caps are raised at b2h_tpt_create, so switching between captures is safe.  B2H_ERR_INVALID: NULL model, other
 * value (nothing changes). */
int b2h_tpt_set_train_whole(b2h_tpt* m, int kernel);
/* Unmangled name of the encoder's self-attention forward kernel that b2h_tpt_train_forward would launch under the
 * current setting: "b2h_tt_sdpa" or "b2h_mw_sdpa"; static storage.  NULL for a NULL model.  After
 * b2h_tpt_set_train_whole(m, B2H_TRAIN_MFMA), b2h_tpt_train_attn_name(m, T) is "b2h_mw_sdpa" too at T <= 128. */
const char* b2h_tpt_train_enc_attn_name(const b2h_tpt* m);
/* The same two switches for TransformerEnc's training calls (b2h_tenc_train_forward / b2h_tenc_backward), over the same
 * enum, independent of each other; B2H_TRAIN_VALU is the default of every new model.
 *   b2h_tenc_set_train_kernel  the self-attention of every layer (T <= 128 always): b2h_tt_sdpa / _bwd of
 *     kernel_train_attn.h, or with B2H_TRAIN_MFMA b2h_mw_sdpa / _bwd of kernel_train_attn_whole_mfma.h: the same
 *     arguments, one workgroup per (sequence, head), no buffer besides the operands, all six products on
 *     v_mfma_f32_16x16x4_f32 in the default's summation order.  y is bitwise equal to the default's; the backward
 *     sums rowsum(dSd o S) in its own fixed order, so the gradients are exact fp32 but not bitwise equal.
 *   b2h_tenc_set_train_linear  every Linear, forward and backward: b2h_tt_linear / _dx / _dw, or b2h_ml_linear /
 *     _dx / _dw (bitwise equal to the default's).
 * b2h_tenc_train_bytes and every layout do not depend on either, so either backward accepts either forward's saved
 * buffer.  All LDS caps are raised at b2h_tenc_create, so switching between captures is safe.
 * B2H_ERR_INVALID: NULL model, other value (nothing changes). */
int b2h_tenc_set_train_kernel(b2h_tenc* m, int kernel);
int b2h_tenc_set_train_linear(b2h_tenc* m, int kernel);
/* Unmangled name of the attention forward kernel that b2h_tenc_train_forward would launch at T frames under the current
 * setting: "b2h_tt_sdpa" or "b2h_mw_sdpa"; static storage.  NULL for a NULL model or a T the training calls refuse
 * (T < 1, T > the model's max_len). */
const char* b2h_tenc_train_attn_name(const b2h_tenc* m, int64_t T);
/* Unmangled name of the Linear forward kernel that b2h_tenc_train_forward would launch: "b2h_tt_linear" or
 * "b2h_ml_linear"; static storage.  NULL for a NULL model. */
const char* b2h_tenc_train_linear_name(const b2h_tenc* m);

/* Dropout keep-masks ---------------------------------------------------------
 * The masks of b2h_tenc_train_forward / b2h_tpt_train_forward (uint8, 1 = keep with probability 1 - p) from one
 * HIP kernel (kernel_dropout_masks.h), so that a host needs no random generator of its own to train with dropout.
 * Counter based, Philox4x32-10 (multipliers D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85; ten rounds, the key
 * bumped between rounds).  Element e of mask number k, e the flat index in the mask's contiguous layout:
 *   block b = e / 4;  counter (b mod 2^32, b >> 32, k, s), s = (step + *step_dev) mod 2^32 (without the *step_dev
 *   term when step_dev is NULL);  key (seed mod 2^32, seed >> 32);  word = output word e mod 4 of that block;
 *   keep = word >= thr, thr = ceil((double)p * 2^32) compared in 64 bits: p == 0 keeps everything, p == 1 nothing.
 * A byte depends on (seed, s, k, e, p) only: not on the launch grid, on how many masks the call has or on the size of
 * any other mask; p is exact to 2^-32.
 *   masks, numel: HOST arrays of n_masks device pointers (16-byte aligned, written) and element counts; mask i of the
 *                 call has number first_index + i, so the masks of a step may be drawn in several calls.  For the
 *                 training forwards number them from 0 in the order their comments above list.
 *   step        : the training step; a captured HIP graph that shall draw new masks on every replay passes the
 *                 device word step_dev (read by the kernel, never written) and advances it itself between replays.
 * One launch per 64 masks, their pointers and sizes in the kernel arguments.  Stream-ordered and asynchronous: it
 * does not synchronise, allocate or read device memory on the host, so it can be captured.  Nothing is written
 * past numel[i] bytes.  B2H_ERR_INVALID, before anything is launched: NULL masks or numel with n_masks > 0,
 * n_masks < 0, first_index < 0, a NULL or not 16-byte-aligned mask pointer, numel[i] < 0, p outside [0, 1] or NaN.
 * n_masks == 0 or all sizes 0 is a no-op (B2H_OK). */
int b2h_dropout_masks(uint8_t* const* masks, const int64_t* numel, int n_masks, int first_index, float p,
                      uint64_t seed, uint64_t step, const uint64_t* step_dev, void* stream);
/* How many keep-masks the model's training forward takes for this batch (4*n_enc_layers + 6*n_dec_layers;
 * 1 + 4*nlayers) and, in numel[0 .. min(count, capacity)), their element counts in the order documented at the
 * training forwards (numel may be NULL with capacity 0).  0 for a NULL model or a shape the forward refuses.  Pure
 * host functions: nothing is read from the device. */
int64_t b2h_tpt_mask_numel(const b2h_tpt* m, int64_t B, int64_t S, int64_t T, int64_t* numel, int capacity);
int64_t b2h_tenc_mask_numel(const b2h_tenc* m, int64_t B, int64_t T, int64_t* numel, int capacity);

/* optimizer.step() --------------------------------------------------------------
 * The last line of the reference's loop body (steps/traintest.py:121, torch.optim.Adam(model.parameters(), lr) at :48):
 * Adam with amsgrad = False, maximize = False and classic L2 weight decay, for every tensor of a model from one HIP
 * kernel (kernel_adam.h), so that a host applies the gradients of b2h_backward / b2h_tenc_backward / b2h_tpt_backward
 * without an optimizer of its own.  Per element, fp32, every line one rounding or one fused multiply-add (marked F):
 *   g' = g + wd * p                         F   only if wd != 0
 *   m  = m + (g' - m) * (1 - b1)            F   after the subtraction
 *   v  = v * b2 + ((1 - b2) * g') * g'      F   after the two products v * b2 and (1 - b2) * g'
 *   den = sqrt(v) / bc2s + eps                  IEEE square root and division
 *   p  = p + (-step_size) * (m / den)       F   after the division
 * with t = step + *step_dev (without the *step_dev term when step_dev is NULL), bc2s = sqrt(1 - b2^t) and
 * step_size = lr / (1 - b1^t) evaluated in double and rounded to float once; b^t by repeated squaring.
 *   params, grads, exp_avg, exp_avg_sq, numel: HOST arrays of n_tensors device pointers (fp32, contiguous, 4-byte
 *                 aligned; a tensor whose four pointers are all 16-byte aligned takes the 16-byte path) and element
 *                 counts.  params, exp_avg and exp_avg_sq are updated in place; grads is only read.  exp_avg and
 *                 exp_avg_sq start as zeros.  The pointers of a tensor with numel 0 are not looked at.
 *   lr, lr_dev  : the learning rate, or when lr_dev is not NULL the device float that replaces it (only read), so a
 *                 captured step follows a schedule (adjust_learning_rate, steps/utils.py:301-307).
 *   beta1, beta2, eps, weight_decay: torch's betas, eps, weight_decay.  Each beta stands for the shortest decimal
 *                 that rounds to the float given (0.999f means 0.999), because 1 - beta2 taken from the float's exact
 *                 value would be off by 1e-5 of itself; lr, eps and weight_decay are taken as the floats they are.
 *   step, step_dev: the first update is step 1.  A captured HIP graph passes the device word step_dev (read by the
 *                 kernel, never written), e.g. the number of updates made so far with step = 1, and advances it
 *                 itself between replays; step + *step_dev must be >= 1.
 * One launch per 80 tensors, their pointers and sizes in the kernel arguments; the result does not depend on how the
 * tensors are grouped into calls.  Stream-ordered and asynchronous: it does not synchronise, allocate or read device
 * memory on the host, so it can be captured.  Nothing is written past numel[i] elements.  B2H_ERR_INVALID, before
 * anything is launched: a NULL array with n_tensors > 0, n_tensors < 0, numel[i] < 0, a NULL or not 4-byte-aligned
 * pointer of a tensor with numel[i] > 0, two of the four arrays of one tensor overlapping, a beta outside [0, 1),
 * eps < 0, weight_decay < 0, lr < 0 with lr_dev NULL, NaN in any of these, step < 1 with step_dev NULL, step < 0
 * otherwise.  n_tensors == 0 or all sizes 0 is a no-op (B2H_OK). */
int b2h_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, const int64_t* step_dev, void* stream);

/* Between backward and the update: gradient clipping, a non-finite guard, warmup ----
 * What a transformer training loop has between loss.backward() and optimizer.step(), decided on the device and left in
 * device words, so that a captured step (whose host code never runs again) clips, skips and warms up on every replay:
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) with the 2-norm, "skip the update when a gradient is not
 * finite", and a per-step schedule of the learning rate (kernel_step_control.h).  Two stages:
 *   1. only when max_norm > 0 or guard != 0: partial sums of squares.  One flat index runs over the 16-byte chunks
 *      (4 floats, the last one of a tensor shorter) of all tensors in the order given; block b of 1024 chunks gives
 *        partial[b] = sum of fma(x, x, .) over its elements in a fixed order, in double
 *      (the product of two floats is exact in double, so nothing overflows or underflows for any fp32 gradients, where
 *      the fp32 norm of torch overflows near 1.8e19); workspace holds the partials.
 *   2. one workgroup adds the partials in a fixed order and stores, with t = step + *step_dev (without the *step_dev
 *      term when step_dev is NULL) the 1-based index of the update about to be made, all in double:
 *        total = sum of partial[]                      0 when stage 1 did not run
 *        norm  = sqrt(total)
 *        *norm_out  = (float)norm
 *        *apply_out = guard ? isfinite(total) : 1
 *        *skipped  += !apply                            a plain read-modify-write: zero it once before the first step
 *        *scale_out = apply == 0  ? 0.0f
 *                   : max_norm > 0 ? (float)(c >= 1 ? 1 : c) with c = max_norm / (norm + 1e-6)
 *                   : 1.0f                              torch's clamped clip_coef; a NaN norm gives a NaN scale, as
 *                                                       torch does, when the guard is off
 *        *lr_out    = (float)(base * f(t))              base = base_lr, or *base_lr_dev when that is not NULL
 *          B2H_SCHED_NONE      f = 1
 *          B2H_SCHED_LINEAR    f = t >= W ? 1 : t / W                  from t >= W on, the base rate's own bits
 *          B2H_SCHED_INV_SQRT  f = t <= W ? t / W : sqrt(W / t)        W = warmup_steps >= 1
 * The words are a function of the numel list and the values alone: not of the stream, the device, the grid or the
 * pointers' alignment.  grads is only read; p.grad stays unscaled: b2h_adam_step_guarded applies *scale_out.
 *   grads, numel: HOST arrays of n_tensors device pointers (fp32, contiguous, 4-byte aligned; a 16-byte aligned tensor
 *                 is read 16 bytes at a time) and element counts.  Not looked at, and may be NULL, when stage 1 does not
 *                 run; the pointer of a tensor with numel 0 is not looked at.
 *   norm_out, scale_out, lr_out (float, 4-byte aligned), apply_out, skipped (int64, 8-byte aligned): device words; any
 *                 of them may be NULL and is then not stored.  base_lr_dev (4), step_dev (8) are only read.
 *   workspace   : b2h_step_prepare_bytes(numel, n_tensors) bytes of device memory, 16-byte aligned: 8 bytes per 4096
 *                 gradient elements; every partial is stored before it is read, so it needs no initialising.  May be
 *                 NULL when stage 1 does not run or that size is 0.  b2h_step_prepare_bytes is a pure host function
 *                 (0 for a NULL array, n_tensors <= 0 or a negative size).
 * One launch per 80 tensors for stage 1, one for stage 2.  Stream-ordered and asynchronous: it does not synchronise,
 * allocate or read device memory on the host, so it can be captured.  B2H_ERR_INVALID, before anything is launched:
 * n_tensors < 0, NaN max_norm, a schedule that is no B2H_SCHED_* value, warmup_steps < 1 with a schedule, step < 1 with
 * a schedule and step_dev NULL (step < 0 otherwise), base_lr < 0 or NaN with base_lr_dev NULL, a misaligned word or
 * workspace; and when stage 1 runs: a NULL array with n_tensors > 0, numel[i] < 0, a NULL or misaligned gradient with
 * numel[i] > 0, a NULL or too small workspace; an output overlapping another output, base_lr_dev, step_dev or a
 * gradient.  n_tensors == 0 is no error: the norm is 0. */
enum { B2H_SCHED_NONE = 0, B2H_SCHED_LINEAR = 1, B2H_SCHED_INV_SQRT = 2 };
size_t b2h_step_prepare_bytes(const int64_t* numel, int n_tensors);
int b2h_step_prepare(const float* const* grads, const int64_t* numel, int n_tensors, float max_norm, int guard,
                     float base_lr, const float* base_lr_dev, int schedule, int64_t warmup_steps, int64_t step,
                     const int64_t* step_dev, float* norm_out, float* scale_out, int64_t* apply_out, int64_t* skipped,
                     float* lr_out, void* workspace, size_t workspace_bytes, void* stream);
/* b2h_adam_step behind the words of b2h_step_prepare (b2h_adam_guarded_k, kernel_adam.h): per element
 *   g <- g * *grad_scale_dev                   one fp32 rounding, as g.mul_(clip_coef) in torch; grads is not written
 * then the listing of b2h_adam_step unchanged; and when *apply_dev == 0 nothing is read or written beyond that word:
 * params, exp_avg and exp_avg_sq keep their bits (the caller then leaves the step count alone: add *apply_dev to it).
 * Pass b2h_step_prepare's lr_out as lr_dev for the warmed-up rate.  grad_scale_dev (float, 4-byte aligned) and
 * apply_dev (int64, 8-byte aligned) are only read; either may be NULL (no scaling; no guard), and with both NULL the
 * result has the bits of b2h_adam_step's.  Everything else, the refusals included, is b2h_adam_step's; in addition
 * B2H_ERR_INVALID for a misaligned word and for a word inside an array the call updates. */
int b2h_adam_step_guarded(float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, int n_tensors, float lr, const float* lr_dev,
                          float beta1, float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                          const float* grad_scale_dev, const int64_t* apply_dev, void* stream);

/* The training set on the device: one kernel builds every batch -------------------
 * What the reference's datasets and transforms do per utterance on the host (FastTextPoseDataset.__getitem__ and
 * TextPoseH5Dataset.__getitem__, dataloaders/text_pose_dataset.py:430-476, 652-688: frame selection, padding, clipping;
 * then WristDifference, ChestDifference, NormalizeFixedFactor and one Build*Item of steps/utils.py:180-277 in
 * run.py:83-104's order) and torch's default collate stacks, from a store that stays on the GPU (kernel_build_batch.h).
 * Store:
 *   rows    (n_rows, 3 J) fp32, J = n_body + 42: every frame of every utterance back to back; a row is
 *           [x * J | y * J | c * J], the joints n_body body, then 21 left hand, then 21 right hand.  n_body = 8 is the
 *           reference's HDF5 row (n_frames, 150) (array2item, text_pose_dataset.py:587-612); n_body = 12 the same rule,
 *           162 wide, for utterances loaded from OpenPose JSON (body joints BODY_HEAD_KEYPOINTS, :14).
 *   offsets (n_utt + 1) int64, ascending, offsets[n_utt] <= n_rows: utterance u owns rows offsets[u] .. offsets[u+1]-1.
 *   tokens  (n_utt, S) int64 or NULL (then S is ignored); 1 <= S <= 128.  Tokenising stays with the caller.
 * Batch: utt (B) int64 names the utterances, start (B) int64 or NULL (= 0) the crop offsets.  With len the row count of
 * utt[b]: n_frames[b] = min(len, T); the window starts at clamp(start[b], 0, len - T) if len > T and at 0 otherwise
 * (select_jsons, :52-68).  Frames t >= len are zeros put in before any transform (TextPoseH5Dataset.pad, :614-624)
 * or, with B2H_BATCH_PAD_FRAME0, the window's first frame again, transformed like any frame (the JSON datasets' pad,
 * :511-519).  An utterance without rows gives zeros and n_frames 0 either way.
 *   B2H_BATCH_DIF_ENCODING: hand -= raw body wrist (joint 4), then body -= chest (joint 1)   (run.py:85-87)
 *   B2H_BATCH_NORMALIZE   : body and hand / factor, a true division                           (run.py:89-90)
 *   predict (enum b2h_predict): RIGHT_HAND input = body (B, T, n_body, 2), target = right hand (B, T, 21, 2);
 *           RIGHT_INDEX (B, T, 29, 2) / (B, T, 4, 2) and RIGHT_3FINGERS (B, T, 21, 2) / (B, T, 12, 2) in
 *           b2h_tpt_build_item's joint orders, n_body = 12 only (B2H_ERR_INVALID with 8: no model takes 25 or 17
 *           joints).  target_conf (B, T, target joints), or NULL: the target joints' confidences.
 *   text_tokens (B, S) = tokens[utt[b]], NULL exactly when tokens is; n_frames (B) int64.
 * Every output element is a copy, or one fp32 subtraction and one correctly rounded fp32 division: equal to torch's,
 * bit for bit.  utt[b] outside [0, n_utt) (or offsets of it outside 0 <= lo <= hi <= n_rows) indexes nothing: every
 * float of that sequence becomes a quiet NaN, its tokens -1, its n_frames 0 -- the models turn an id outside their
 * table into a NaN sequence and the losses return NaN: loud, never a neighbour's data.
 * One launch, no atomics, every output word written once; stream-ordered, asynchronous, allocates nothing and reads
 * no device memory on the host, so it can be captured.  B2H_ERR_INVALID, before any device work: n_body not 8 or 12,
 * an unknown predict or flag bit, a finger mode with n_body 8, factor not > 0 with B2H_BATCH_NORMALIZE, S outside
 * [1, 128] with tokens, tokens without text_tokens or the reverse, a NULL or not 8-byte-aligned pointer, an output
 * overlapping the store, utt, start or another output, a pointer that is not memory of the current device.
 * B2H_ERR_SHAPE: B, T, n_utt or n_rows negative, T > 2^24, B > 2^31 - 1.  B * T == 0 is a no-op (B2H_OK). */
enum b2h_batch_flags { B2H_BATCH_DIF_ENCODING = 1, B2H_BATCH_NORMALIZE = 2, B2H_BATCH_PAD_FRAME0 = 4 };
int b2h_build_batch(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                    const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t B, int64_t T,
                    int predict, int flags, float factor, float* input_kp, float* target_kp, float* target_conf,
                    int64_t* text_tokens, int64_t* n_frames, void* stream);

/* A captured epoch: its plan, the planned batch build and the step word -----------
 * What torch.randperm and the per-batch crop draws give the eager loop (run.py:135 `shuffle`, select_jsons,
 * text_pose_dataset.py:52-68), for a whole epoch from one launch (kernel_epoch_plan.h), so that a training step captured
 * into a HIP graph is replayed through an epoch with no host work in between: b2h_epoch_plan once per epoch, then per
 * step b2h_build_batch_planned ... b2h_adam_step, b2h_epoch_record.
 *
 * b2h_epoch_plan writes utt_plan (n_utt) int64 and start_plan (n_utt) int64 (NULL allowed when random_crop is 0, and
 * then meaning 0; given without random_crop it is filled with zeros).  Every entry is a pure function of its index:
 *   utt_plan[i]   = i without shuffle.  With shuffle, perm(i): a 4-round balanced Feistel network over [0, 2^(2h)), h
 *                   the smallest value >= 1 with 2^(2h) >= n_utt, re-applied while the value is >= n_utt (cycle
 *                   walking), a permutation of [0, n_utt) for every (seed, epoch).  One pass over x, mask = 2^h - 1:
 *                   L = x >> h, R = x & mask; four times, r = 0 .. 3: (L, R) = (R, L ^ (P(R, 1 + r) & mask));
 *                   x = L << h | R.
 *   start_plan[i] = the crop start of utterance u = utt_plan[i]: with len = offsets[u+1] - offsets[u] and
 *                   room = max(len - T, 0), floor(P(i, 0) * (room + 1) / 2^32): uniform in [0, room], 0 for an
 *                   utterance that fits.  The meaning of DeviceLoader.draw_starts, with other bits, as the native
 *                   dropout masks relate to torch's.
 *   P(c, tag)     = output word 0 of the Philox4x32-10 block (b2h_dropout_masks' generator) with counter
 *                   (c, tag, epoch lo, epoch hi) and key (seed lo, seed hi): tags 1 .. 4 are the Feistel rounds, tag 0
 *                   the crop draws.
 * offsets is the store's (n_utt + 1) int64 array, read only with random_crop (it may be NULL otherwise).  One launch,
 * one lane per entry, no sort, no atomics, no LDS; stream-ordered, asynchronous, allocates nothing and reads no device
 * memory on the host, so it can be captured.  B2H_ERR_INVALID, before any device work: shuffle or random_crop not 0 or
 * 1, utt_plan NULL, start_plan or offsets NULL with random_crop, a pointer not 8-byte aligned, utt_plan, start_plan and
 * offsets overlapping, a pointer that is not memory of the current device.  B2H_ERR_SHAPE: n_utt or T negative,
 * n_utt > 2^30.  n_utt == 0 is a no-op (B2H_OK). */
int b2h_epoch_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int shuffle, int random_crop, uint64_t seed,
                   uint64_t epoch, int64_t* utt_plan, int64_t* start_plan, void* stream);

/* b2h_build_batch over a plan: utt_plan and start_plan (n_plan entries each; start_plan NULL = 0) take the place of utt
 * and start, and sequence b reads entry p = *step * B + b, `step` a device int64 word that is only read.  If *step < 0
 * or p >= n_plan the sequence is built as an unknown utterance -- quiet NaN floats, tokens -1, n_frames 0 -- so a
 * replay past the end of the plan is loud, never a stale batch; the last step of a plan that is no multiple of B has
 * such sequences behind its entries.  Everything else, the launch included (the same kernel, one extra wave-uniform
 * 8-byte load per thread), is b2h_build_batch's; so are the refusals, which name utt_plan, start_plan and step, plus
 * B2H_ERR_SHAPE for n_plan < 0 or > 2^40.  utt_plan may be NULL when n_plan is 0. */
int b2h_build_batch_planned(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                            const int64_t* tokens, int64_t S, const int64_t* utt_plan, const int64_t* start_plan,
                            int64_t n_plan, const int64_t* step, int64_t B, int64_t T, int predict, int flags, float factor,
                            float* input_kp, float* target_kp, float* target_conf, int64_t* text_tokens, int64_t* n_frames,
                            void* stream);

/* The batch build with data augmentation: scale, rotation, mirror, jitter ---------
 * Every sequence is scaled, rotated and mirrored about its own chest and its input joints are jittered, drawn and
 * applied inside the build launch (kernel_build_batch_aug.h).  The reference has no augmentation; the definition is this
 * project's own and tests/augment_ref.py restates it in numpy float32, bit for bit.  b2h_build_batch and
 * b2h_build_batch_planned are untouched.
 *
 * Arguments: the store as b2h_build_batch; utt, start, n_plan, step as b2h_build_batch_planned, except that step may be
 * NULL; B .. stream as b2h_build_batch.
 *   step != NULL: sequence b reads plan entry p = *step * B + b under the planned build's rules; p is its draw index.
 *   step == NULL: sequence b reads utt[b] and start[b] (B entries; n_plan is not looked at) and its draw index is
 *                 p = entry0 + b, so an eager epoch that passes entry0 = i * B for batch i builds what the replayed
 *                 step builds.
 *   key: two device uint64 words {seed, epoch}, only read: a caller rewrites epoch in place between epochs without
 *        capturing again.
 * Meaning: "augment the raw frame, then do what b2h_build_batch does".  For a live frame a virtual store row is formed;
 * selection, padding, B2H_BATCH_DIF_ENCODING, B2H_BATCH_NORMALIZE and the predict gather apply to it unchanged.  Frames
 * of zero padding stay zeros and get no jitter; B2H_BATCH_PAD_FRAME0 frames are live and their jitter uses their own t.
 * Draws: Philox4x32-10 (b2h_dropout_masks' generator), key (seed lo, seed hi); d(w) = float(w >> 8) * 2^-24 * 2 - 1, in
 * [-1, 1) and exact in fp32.  Counter word 1 is a tag: 0 .. 4 belong to b2h_epoch_plan, 16 and 17 are these.
 *   sequence block, counter (p, 16, epoch lo, epoch hi): word 0 the scale, 1 the rotation, 2 the mirror, 3 unused.
 *     s = 1 + scale * d(w0);  t = rotate_tan * d(w1);  t2 = t * t;  den = 1 + t2;  c = (1 - t2) / den;
 *     sn = (t + t) / den -- the rational form of a rotation by theta with tan(theta / 2) = t, without sinf / cosf, whose
 *     bits would differ between device and host;  mirror = w2 < ceil(double(mirror_p) * 2^32), compared in 64 bits.
 *   virtual row: joint q reads store joint q' = mirror ? M(q) : q, its confidence copied unchanged.  M swaps the left- and
 *     the right-hand block joint for joint and the body's sides: [0, 1, 5, 6, 7, 2, 3, 4, 9, 8, 11, 10] for n_body 12
 *     (BODY_25 joints 0 - 7, 15 - 18), the first eight of those for n_body 8.  With (cx, cy) the frame's raw chest (body
 *     joint 1, which M fixes):  dx = x - cx;  dy = y - cy;  if (mirror) dx = -dx;  rx = c * dx - sn * dy;
 *     ry = sn * dx + c * dy;  x' = cx + s * rx;  y' = cy + s * ry.  A joint OpenPose missed (0, 0, conf 0) is transformed
 *     like any other: the reference's own transforms treat it no differently.
 *   jitter: on input_kp only, after the difference encoding and before the division by factor.  Input joint j (the index
 *     in input_kp, not the store joint) of frame t takes words 2 (j & 1) and 2 (j & 1) + 1 of the block with counter
 *     (p, 17 | t << 8, epoch lo, j >> 1):  v.x = v.x + jitter * d(w_x);  v.y = v.y + jitter * d(w_y).  The epoch enters
 *     the jitter with its LOW 32 bits only; t < 2^24 by the limit on T.  target_kp, target_conf, text_tokens and n_frames
 *     never see it.
 * Each fp32 operation above is one correctly rounded operation, never contracted into a fused multiply-add.  A stage
 * whose parameters are 0 is not run, so that it changes no bit (cx + (x - cx) is not x in fp32; v + 0 * d turns -0 into
 * +0): with scale and rotate_tan both 0 the rotation-and-scale stage is skipped (y' = y; x' = x, or cx + dx under a
 * mirror), with jitter 0 nothing is added.  With all four 0 the outputs are b2h_build_batch's, bit for bit.
 * One launch on b2h_build_batch's grid, every output word written once, no LDS, no atomics; stream-ordered,
 * asynchronous, allocates nothing, reads `aug` during the call and no device memory on the host: capturable under
 * b2h_build_batch's conditions.  Refusals, before any device work: b2h_build_batch_planned's (with step NULL,
 * b2h_build_batch's), plus B2H_ERR_INVALID for aug NULL, a b2h_augment field outside its range or not finite (the
 * message names the field), key NULL, not 8-byte aligned, overlapping an output or not memory of the current device;
 * B2H_ERR_SHAPE for n_plan > 2^32, entry0 < 0 or entry0 + B > 2^32 (a draw index has 32 bits). */
typedef struct b2h_augment {   /* host memory, read during the call */
    float scale;       /* s uniform in [1 - scale, 1 + scale];            0 <= scale < 1        */
    float rotate_tan;  /* t = tan(theta / 2) uniform in [-rotate_tan, rotate_tan]; 0 <= . <= 1  */
    float mirror_p;    /* probability of a left/right mirror;             0 <= . <= 1           */
    float jitter;      /* uniform noise of +-jitter pixels on input_kp;   0 <= . , finite       */
} b2h_augment;
int b2h_build_batch_aug(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                        const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t n_plan,
                        const int64_t* step, int64_t entry0, const b2h_augment* aug, const uint64_t* key, int64_t B, int64_t T,
                        int predict, int flags, float factor, float* input_kp, float* target_kp, float* target_conf,
                        int64_t* text_tokens, int64_t* n_frames, void* stream);

/* The end of a captured step: one work-item reads s = *step, stores *loss to losses[s] if 0 <= s < n_losses, and in
 * every case stores *step = s + 1.  Stream-ordered after the Adam update it is the only writer of the step word inside
 * a step (no atomics), and the per-batch losses stay on the device until the epoch's one copy.  loss, losses: device
 * fp32, 4-byte aligned (losses may be NULL when n_losses is 0); step: device int64, 8-byte aligned.  Allocates nothing,
 * can be captured.  B2H_ERR_INVALID, before any device work: a NULL or misaligned pointer, step overlapping loss or
 * losses, loss inside losses, a pointer that is not memory of the current device.  B2H_ERR_SHAPE: n_losses negative. */
int b2h_epoch_record(const float* loss, float* losses, int64_t n_losses, int64_t* step, void* stream);

/* Whole-store inference: window plan, row write-back, per-joint error ---------------
 * The reference's stream-shaped caller (infer_utterance_h5.py -> steps/traintest.py:332-391) runs a trained model over a
 * whole keypoint store in batches and writes the predictions out as store rows.  Here: a plan of windows that covers
 * every frame of every utterance once, b2h_build_batch per slice of the plan, the model, and b2h_scatter_rows, the
 * inverse of b2h_build_batch's target transform (kernel_scatter_rows.h).
 *
 * b2h_window_plan is a HOST function: offsets and the three plan arrays are host memory, nothing touches the GPU.  For
 * utterance u with L = offsets[u+1] - offsets[u] rows, in ascending order of u, as entries (utt, start, skip):
 *   L == 0                      no entry
 *   B2H_COVER_FIRST             (u, 0, 0): the reference's `--frames-selection first`; rows at or past T get no entry
 *   B2H_COVER_ALL, L <= T       (u, 0, 0)
 *   B2H_COVER_ALL, L >  T       k = ceil(L / T) entries: (u, i T, 0) for i = 0 .. k-2, then (u, L - T, k T - L)
 * The last window of a long utterance is a full window that ends with the utterance, so the model sees T real frames
 * and no start is changed by b2h_build_batch's clamp; skip counts its leading frames that the window before it covers
 * already, which the write-back drops.  Every row is therefore addressed by exactly one (entry, frame >= skip).
 * Returns the number of entries and fills the first min(count, capacity) of each array; with capacity 0 the arrays may
 * be NULL (call once for the count, once to fill).  Returns -1, with the message in b2h_last_error, for T < 1, n_utt or
 * capacity negative, an unknown coverage, offsets NULL with n_utt > 0, offsets that do not ascend from
 * offsets[0] >= 0, or a plan array that is NULL where an entry must be stored. */
enum b2h_coverage { B2H_COVER_ALL = 0, B2H_COVER_FIRST = 1 };
int64_t b2h_window_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int coverage, int64_t* utt_plan,
                        int64_t* start_plan, int64_t* skip_plan, int64_t capacity);

/* A batch of predictions written back into store rows.  The store (rows, n_rows, offsets, n_utt, n_body), utt, start,
 * B, T, predict, flags and factor are b2h_build_batch's and mean the same; skip (B) int64 or NULL (= 0).  pred is
 * (B, T, nt, 2) fp32 with nt = 21, 4 or 12 target joints of `predict`; rows_out is (n_rows, 3 J) fp32, initialised by
 * the caller (normally a copy of rows): only the addressed words are written.  With len the row count of utt[b],
 * n = min(len, T) and the window of b2h_build_batch, frame t of sequence b is written iff utt[b] is known, len > 0 and
 * max(skip[b], 0) <= t < n, to row (window start + t), joint d = the store joint behind target joint j:
 *   v = pred[b, t, j];  B2H_BATCH_NORMALIZE: v = fl(v * factor);  B2H_BATCH_DIF_ENCODING: v = fl(v + w), w the RAW body
 *   wrist (joint 4) of the same row of `rows`;  rows_out[row][d] = v.x, [J + d] = v.y, [2 J + d] = conf.
 * Each step is one correctly rounded fp32 operation (never a fused multiply-add), so fl(fl(p f) + w) is reproducible
 * anywhere.  B2H_BATCH_PAD_FRAME0 is accepted and changes nothing: padded frames are never written.  An unknown id (or
 * offsets of it outside 0 <= lo <= hi <= n_rows) writes nothing.  Two sequences of one launch that address the same word
 * leave it unspecified; a plan of b2h_window_plan never does.  One launch, one lane per (b, t, j), no atomics;
 * stream-ordered, asynchronous, allocates nothing, can be captured.  Refusals: b2h_build_batch's for the arguments
 * they share, in its order; then B2H_ERR_INVALID for conf not finite, a NULL (rows, rows_out only with n_rows > 0;
 * offsets, utt, pred) or not 8-byte-aligned pointer (pred is read as float2), rows_out overlapping any other operand, a
 * pointer that is not memory of the current device.  B * T == 0 is a no-op (B2H_OK). */
int b2h_scatter_rows(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                     const int64_t* utt, const int64_t* start, const int64_t* skip, int64_t B, int64_t T,
                     int predict, int flags, float factor, const float* pred, float conf,
                     float* rows_out, void* stream);

/* Overlapping windows, blended in the write-back.  A frame at the edge of a window is predicted with context on one
 * side only, so windows that merely touch can make the trajectory jump at every boundary.  b2h_window_plan_overlap is
 * b2h_window_plan with B2H_COVER_ALL for windows that overlap by `overlap` = K frames (a HOST function, the same
 * protocol and arrays).  With stride s = T - K, for utterance u of L rows:
 *   L == 0     no entry
 *   L <= T     (u, 0, 0)
 *   L >  T     n = ceil((L - T) / s) + 1 entries: (u, i s, 0) for i = 0 .. n-2, then (u, L - T, (n-1) s - (L - T))
 * The last window is again a full one that ends with the utterance; skip counts its leading frames that lie before
 * row (n-1) s.  Every window after an utterance's first therefore begins its used frames (start + skip) exactly K rows
 * before the end of the window before it, K <= T / 2 keeps a window's first K and last K frames apart, and with K = 0
 * the plan is b2h_window_plan's, entry for entry.  Returns -1 as b2h_window_plan does, and for overlap < 0 or
 * 2 overlap > T (the message names both numbers). */
int64_t b2h_window_plan_overlap(const int64_t* offsets, int64_t n_utt, int64_t T, int64_t overlap, int64_t* utt_plan,
                                int64_t* start_plan, int64_t* skip_plan, int64_t capacity);

/* b2h_scatter_rows for such a plan.  utt_plan, start_plan and skip_plan are the WHOLE plan (n_plan entries each) in
 * device memory; pred (B, T, nt, 2) holds the predictions of entries entry0 .. entry0 + B - 1 and pred_before
 * (T, nt, 2) those of entry entry0 - 1.  For entry e, e - 1 is its predecessor if it exists and has the same utt, e + 1
 * its successor likewise; windows are b2h_build_batch's (the clamped start), skips below 0 count as 0, and with
 * w = max(start[e-1] + T - (start[e] + skip[e]), 0), or 0 without a predecessor:
 *   frame t of entry e is written iff utt is known, len > 0 and skip[e] <= t < end, where end = min(len, T) without a
 *   successor, else min(that, start[e+1] + skip[e+1] - start[e]): the tail a successor blends is left to the successor;
 *   for p = t - skip[e] < w (the blend region) with pa the predecessor's value of the same row -- its frame
 *   t + start[e] - start[e-1], read from pred (b > 0) or pred_before (b == 0) -- and pb the entry's own:
 *     B2H_BLEND_LINEAR   wb = fl((float)(p + 1) / (float)(w + 1)), wa = fl(1 - wb), v = fl(fl(wa pa) + fl(wb pb))
 *     B2H_BLEND_CENTRE   v = 2 p >= w ? pb : pa   (a select: each window keeps the frames nearer to its centre)
 *   elsewhere v = pb; then * factor, + wrist and the three stores exactly as b2h_scatter_rows.
 * (In a plan not made by b2h_window_plan_overlap a predecessor's frame before its frame 0 does not exist: v = pb.)
 * Every addressed word is written by one lane of one launch over the plan -- no read-modify-write, no atomics, no
 * dependence on the order of the launches -- and with K = 0 the result is b2h_scatter_rows's, bit for bit.
 * pred_before may be NULL when entry0 == 0 or entry entry0 - 1 belongs to another utterance.  Which of the two holds is
 * in device memory, which no host check reads: a caller passes it whenever entry0 > 0.  With NULL nothing is read
 * through it and entry entry0 is written as if it had no predecessor.  It may alias pred.  Stream-ordered,
 * asynchronous, allocates nothing, can be captured; one launch, 64-bit indices.  Refusals: b2h_scatter_rows's scalar
 * checks in its order (n_plan negative is a negative shape), then B2H_ERR_INVALID for an unknown blend and for
 * entry0 < 0 or entry0 + B > n_plan; B * T == 0 is then a no-op; then the size limits (n_plan <= 2^40), a NULL
 * (utt_plan, start_plan and skip_plan are all required) or not 8-byte-aligned pointer, pred_before included, rows_out
 * overlapping any other operand, pred_before included, a pointer that is not memory of the current device. */
enum b2h_blend { B2H_BLEND_LINEAR = 0, B2H_BLEND_CENTRE = 1 };
int b2h_scatter_rows_blend(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                           const int64_t* utt_plan, const int64_t* start_plan, const int64_t* skip_plan, int64_t n_plan,
                           int64_t entry0, int64_t B, int64_t T, int predict, int flags, float factor,
                           const float* pred, const float* pred_before, int blend, float conf,
                           float* rows_out, void* stream);

/* Per-utterance, per-joint pixel error of the right hand of one store against another of the same shape.  For joint j
 * of a row: dx = fl(xa - xb), dy likewise, d = sqrt(fl(fl(dx dx) + fl(dy dy))), each step correctly rounded fp32; the
 * row counts iff the TRUE store's confidence of that joint is > 0 (OpenPose writes 0 for a joint it did not detect).
 * utt_sum[u][j] is the fp32 sum of d over the counted rows of u in ascending row order, utt_count[u][j] their number;
 * every word is written, 0 for an utterance without rows (or with offsets outside 0 <= lo <= hi <= n_rows).  With
 * total_sum and total_count (21 each; both or neither): total_sum[j] = sum over u ascending of (double)utt_sum[u][j],
 * total_count[j] likewise.  Two launches, no atomics, fixed orders: the same bits on every run and stream.  Rows, utt_sum
 * and utt_count need 4-byte alignment, offsets, total_sum and total_count 8.  B2H_ERR_INVALID: n_body not 8 or 12, one
 * total without the other, a NULL (rows only with n_rows > 0, offsets and the per-utterance outputs only with
 * n_utt > 0) or misaligned pointer, an output overlapping an input or another output, a pointer that is not memory of the
 * current device.  B2H_ERR_SHAPE: n_rows or n_utt negative, n_rows > 2^40, n_utt > 2^30.  n_utt == 0 zeroes the totals. */
int b2h_joint_error(const float* rows_pred, const float* rows_true, int64_t n_rows, const int64_t* offsets,
                    int64_t n_utt, int n_body, float* utt_sum, int32_t* utt_count,
                    double* total_sum, int64_t* total_count,
                    void* stream);

/* Introspection / measurement -------------------------------------------- */

/* conv_channels, pos_emb and whether weights are loaded. */
int b2h_model_info(const b2h_model* m, int* conv_channels, int* pos_emb, int* has_weights);
/* 1 if `kernel` can run this model (width, pos_emb), else 0. */
int b2h_kernel_supported(const b2h_model* m, int kernel);
/* Name of the __global__ function `kernel` resolves to for this model (for
 * matching rocprofv3 kernel-trace rows); static storage.  The plain (unfused) instantiation; for the
 * persistent 16-bit kernel the streaming one, b2h_fwd_mfma16<PREC, false, true>, which every launch of
 * >= 1 MiB of traffic runs (smaller launches run its <PREC, false, false> twin: default cache policy). */
const char* b2h_kernel_name(const b2h_model* m, int kernel);
/* Time `iters` back-to-back launches of b2h_forward on `stream` with HIP events
 * recorded on that stream; returns the average milliseconds per launch. */
int b2h_time_forward(b2h_model* m, const float* x, float* y, int64_t B, int64_t T, int kernel,
                     int iters, void* stream, float* avg_ms);
int b2h_stream_sync(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* B2H_H_ */
