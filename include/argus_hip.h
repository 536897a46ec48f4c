/*
 * argus_hip.h — C ABI of libargus_hip.so, the MI355X (gfx950) kernels behind the argus training
 * hot path. Plain C: raw device pointers, sizes, an opaque HIP stream; no torch types.
 *
 * The reference (pculbertson/argus) has no FFI; its device work is dispatched implicitly through
 * torchvision / pypose / torch.optim / DDP. Each entry point below replaces one of
 * those implicit kernels and names the reference call site it stands in for. The Python host layer
 * (argus_amd/_lib.py, ctypes) binds exactly these symbols; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Activations are NHWC, channel-contiguous, dtype ARGUS_F32 or ARGUS_BF16 (frozen inference also
 *    ARGUS_F16, below).
 *  - Conv weights are OHWI ("KRSC"): w[k][r][s][c]. The stem (7x7, C=3) uses a padded compute layout
 *    w[k][r(8)][s(8)][c(4)] (r=7, s=7, c=3 zero) and an NHWC4 input (channel 3 zero).
 *  - Statistics, losses, gradients of parameters and optimizer state are fp32.
 *  - Every call enqueues on `stream` (hipStream_t; NULL = legacy default) and returns 0 on success or
 *    a nonzero code; argus_last_error() then describes it. The library never allocates device memory:
 *    callers pass workspaces sized by the *_bytes() queries. No call synchronises the device.
 */
#ifndef ARGUS_HIP_H
#define ARGUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* argus_stream_t; /* hipStream_t */

/* ARGUS_FP8 (conv fwd / dgrad and weight-prep entry points): bf16 activations, GEMM operands in OCP
 * MX-fp8 (e4m3 + one E8M0 scale per 32 K-elements of a row) for the MFMA
 * v_mfma_scale_f32_16x16x128_f8f6f4 where the conv pass allows it (reduction channels % 128 == 0, not
 * the stem): the activation operand (and a BN-backward apply prologue) is quantized while staging, the
 * weights are the pre-quantized copies argus_conv_weight_prep(_batch) writes with ARGUS_FP8 (e4m3 rows
 * [rows][cols] then scales [rows][cols/32], in the bf16 copy's buffer). The other passes and every
 * non-conv entry point (pass ARGUS_BF16) run bf16. */
/* ARGUS_F16 (frozen inference only): IEEE binary16 tensors, NHWC, 8 elements per 16-byte chunk like bf16;
 * v_mfma_f32_16x16x32_f16 with fp32 accumulation; every store rounds to nearest even and saturates to
 * +-65504 (NaN stays NaN). Served by the entry points of a frozen forward and no others:
 *   argus_images_to_nhwc4, argus_images_u8_to_nhwc4,
 *   argus_conv_weight_prep (stem descriptor only: writes w_fwd, ignores w_dgrad),
 *   argus_conv_fwd (stem descriptor only, scale = shift = stat_part = NULL),
 *   argus_maxpool_fwd, argus_avgpool_fwd, argus_conv_fold_bn,
 *   argus_conv_infer, argus_conv_infer_splits, _max_splits, _workspace_bytes,
 *   argus_stem_infer, argus_stem_infer_roi, argus_frames_resample,
 *   argus_pool_fc_gelu (and argus_pose_tail, which is fp32 and takes no dtype).
 * Every other entry point that takes a dtype rejects it before anything is launched: the launching ones
 * return ARGUS_ERR_ARG, the planning queries their "not served" value (0, or -1 where that is their error),
 * and argus_last_error() names the dtype. There is no fp16 training path. */
enum { ARGUS_F32 = 0, ARGUS_BF16 = 1, ARGUS_FP8 = 2, ARGUS_F16 = 3 };
enum { ARGUS_OK = 0, ARGUS_ERR_ARG = 1, ARGUS_ERR_SHAPE = 2, ARGUS_ERR_HIP = 3 };

/* One override of the kernel-selection policy (keys: argus_conv_policy_default). */
typedef struct {
  int32_t key, value;
} argus_tuning;

typedef struct {
  int32_t n, h, w; /* images, input spatial */
  int32_t c;       /* input channels (3 for the stem) */
  int32_t k;       /* output channels */
  int32_t r, s;    /* filter size */
  int32_t stride, pad;
  int32_t ho, wo; /* output spatial */
  int32_t stem;   /* 1: the 7x7/2 stem (NHWC4 input, padded weights) */
  /* Optional per-call overrides of the library's kernel-selection policy (experiments, autotuning and
   * the kernel-coverage tests): n_tuning entries of `tuning`; 0 / NULL = the library defaults. The
   * library keeps no mutable selection state: a call sees its own overrides and nothing else. */
  int32_t n_tuning;
  const argus_tuning* tuning;
} argus_conv_desc;

int argus_abi_version(void);
const char* argus_last_error(void);

/* ---- input / weight layout ------------------------------------------------------------------ */
/* (B,3*ncam,H,W) fp32 NCHW -> (B*ncam,H,W,4) NHWC4 of dtype; replaces the reshape at
 * argus/models.py:81 plus the layout change cuDNN does internally. */
int argus_images_to_nhwc4(int dtype, int64_t nimg, int h, int w, const float* x, void* out,
                          argus_stream_t stream);
/* Same, from uint8 images (B,3*ncam,H,W) as CameraCubePoseDataset(uint8=True) yields them: the
 * `.to(torch.float32) / 255.0` of argus/data.py:214-215 runs on the device (4x less H2D traffic). */
int argus_images_u8_to_nhwc4(int dtype, int64_t nimg, int h, int w, const uint8_t* x, void* out,
                             argus_stream_t stream);
/* fp32 master weight -> compute copies: w_fwd[k][r][s][c] (dtype; padded [k][8][8][4] for the
 * stem) and w_dgrad[c][r][s][k] (dtype; ignored for the stem). The master is read with element
 * strides {sk, sc, sr, ss} (so an OIHW nn.Parameter or a channels-last view both work);
 * strides == NULL means OHWI contiguous. */
int argus_conv_weight_prep(const argus_conv_desc* d, int dtype, const float* w_master,
                           const int64_t* strides, void* w_fwd, void* w_dgrad,
                           argus_stream_t stream);

/* ---- convolution (torchvision Conv2d, bias=False; models.py:43) ------------------------------ */
/* Batched weight_prep (one launch for a whole network): the host writes a table of `count`
 * conversions (argus_conv_weight_prep_table: per conv its descriptor, fp32 master pointer and
 * element strides {sk, sc, sr, ss} (NULL strides = OHWI contiguous), w_fwd and w_dgrad destinations
 * (w_dgrad array NULL or entry ignored for the stem)) into host_table, copies it to device memory
 * once, and then argus_conv_weight_prep_batch does what argus_conv_weight_prep does for every entry.
 * The table holds raw device pointers: rebuild it if any of them changes. */
size_t argus_conv_weight_prep_table_bytes(int count);
int argus_conv_weight_prep_table(int count, const argus_conv_desc* descs, const float* const* w_master,
                                 const int64_t* strides, void* const* w_fwd, void* const* w_dgrad,
                                 void* host_table, size_t table_bytes, int* nblocks);
int argus_conv_weight_prep_batch(int dtype, int count, const void* device_table, int nblocks,
                                 argus_stream_t stream);
/* y = conv(x', w) where x' = relu(x*pro_scale+pro_shift) per input channel when pro_scale != NULL
 * (the producer's BatchNorm+ReLU applied while staging; zero padding stays zero), else x.
 * If stat_part != NULL, per-(row-tile, channel) {sum, M2} of y (fp32 accumulators, before
 * rounding; M2 about the tile mean) are written: float2[argus_conv_fwd_stat_rows(d)][k], each row
 * tile covering argus_conv_fwd_stat_tile(d) output pixels (the last one possibly fewer); a negative
 * stat tile (ragged tiling) also writes int32 pixel counts[rows] after them, so stat_part must then
 * hold 2*rows*k floats + rows ints. */
int argus_conv_fwd(const argus_conv_desc* d, int dtype, const void* x, const void* w_fwd, void* y,
                   const float* pro_scale, const float* pro_shift, float* stat_part,
                   argus_stream_t stream);
/* y == NULL (bf16, not the stem, stat_part given): statistics only, nothing stored (ABI 14; the
 * bottleneck's conv3 before argus_conv_fwd_bn_out). */
/* argus_conv_fwd with its BN+ReLU prologue (pro_scale / pro_shift required) that also stores the
 * staged input x' = relu(x*pro_scale+pro_shift) to x_out, bit-identical to argus_bn_apply(relu = 1)
 * of x (ABI 16; 1x1 stride-1 convs, bf16 or fp32): the bottleneck's conv3 statistics pass applies bn2
 * to y2 while staging it and writes a2 (the operand of the fused tail and of conv3's weight gradient),
 * replacing the separate bn2 apply pass of torchvision's Bottleneck.forward (argus/models.py:43). */
int argus_conv_fwd_apply_out(const argus_conv_desc* d, int dtype, const void* x, const void* w_fwd, void* y,
                             const float* pro_scale, const float* pro_shift, float* stat_part, void* x_out,
                             argus_stream_t stream);
/* Bottleneck tail in one forward pass (ABI 14; replaces conv3 + bn3 + the residual add + ReLU of
 * torchvision's Bottleneck.forward, argus/models.py:43 -> torchvision resnet.py, in train mode after
 * argus_bn_finalize of bn3, or eval mode with argus_bn_eval_coeffs): the 1x1 stride-1 conv's C tile t
 * (rounded to bf16, as argus_conv_fwd stores it) gives out = relu(t*scale + shift + res'), res' = res *
 * res_scale + res_shift when res_scale != NULL (the downsample BN) else res, with argus_bn_apply's
 * mask bits (one byte per 16-byte chunk). Bit-identical to argus_conv_fwd + argus_bn_apply. y: optional
 * store of t (NULL: not stored). bf16 only; every tensor NHWC. */
int argus_conv_fwd_bn_out(const argus_conv_desc* d, int dtype, const void* x, const void* w_fwd,
                          const float* scale, const float* shift, const void* res, const float* res_scale,
                          const float* res_shift, void* out, uint8_t* mask_bits, void* y, argus_stream_t stream);
/* ---- frozen inference (ABI 21, added later without a version change: detect by symbol) ----------
 * A deployed model's convolutions: eval-mode BatchNorm folded into the weights once, then one launch per
 * conv. Together they replace nn.Conv2d + nn.BatchNorm2d.eval() [+ add] + nn.ReLU of torchvision's
 * Bottleneck.forward (argus/models.py:43). Served: 1x1 (pad 0) and 3x3 (pad 1) convs of stride 1 or 2, c
 * and k multiples of 64, any h x w, dtype ARGUS_F32, ARGUS_BF16 or ARGUS_F16 (anything else: ARGUS_ERR_ARG); not the
 * stem, which keeps argus_conv_fwd + argus_maxpool_fwd with argus_bn_eval_coeffs. Nothing here allocates
 * or synchronises: every call can be captured into a graph.
 *
 * argus_conv_fold_bn: from the fp32 master weight (element strides as argus_conv_weight_prep; NULL = OHWI
 * contiguous) and the BN parameters / running statistics, bias[k] (fp32) = the shift and
 * w_fold[k][r][s][c] = T(w * scale[k]) (one fp32 multiply, round to nearest even; the w_fwd layout), with
 * scale / shift bit-identical to argus_bn_eval_coeffs. */
int argus_conv_fold_bn(const argus_conv_desc* d, int dtype, const float* w_master, const int64_t* strides,
                       const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, void* w_fold, float* bias, argus_stream_t stream);
/* The reduction (r*s*c) of argus_conv_infer may be split over workgroups when its output tiles alone
 * leave the chip idle. _splits: the library's choice for this shape (>= 1; 0 = shape / dtype not
 * served); _max_splits: the largest accepted value = the k-steps of the reduction (r*s*c / 64 in bf16
 * and fp16, / 32 in fp32); _workspace_bytes: what `splits` slices need (0 for splits <= 1): one uint32 ticket per
 * output tile at the start of the workspace (padded to a multiple of 4096 bytes: up to 1024 tiles, and so
 * every shape the library splits on its own, has its slabs at the same offset, which is what lets one
 * workspace serve convs of different tile counts one after another), then the fp32 slabs. */
int argus_conv_infer_splits(const argus_conv_desc* d, int dtype);
int argus_conv_infer_max_splits(const argus_conv_desc* d, int dtype);
size_t argus_conv_infer_workspace_bytes(const argus_conv_desc* d, int dtype, int splits);
/* out = [relu](conv(x, w_fold) + bias[k] [+ res]) over NHWC tensors; res (may be NULL) has out's layout and
 * dtype; the sum is made in fp32 and rounded once. splits: 0 = argus_conv_infer_splits, 1 = no split (no
 * workspace touched, workspace may be NULL), up to argus_conv_infer_max_splits: the slices' fp32 partial
 * tiles are summed in slice order by the last-arriving workgroup of each output tile, so the result is
 * bitwise reproducible for a given `splits`. The workspace (16-byte aligned) is caller-provided; its
 * ticket words must be zero on entry - zero the workspace once - and every call leaves them zero. One
 * workspace serves the launches of one stream in order, never two concurrent launches. */
int argus_conv_infer(const argus_conv_desc* d, int dtype, const void* x, const void* w_fold, const float* bias,
                     const void* res, int relu, void* out, int splits, void* workspace, size_t workspace_bytes,
                     argus_stream_t stream);
/* ---- frozen gradient (ABI 21, added without a version change: detect by symbol) -----------------
 * The input gradient of the folded network: what torch.autograd.grad gives through nn.Conv2d +
 * nn.BatchNorm2d.eval() + nn.ReLU of torchvision's Bottleneck.forward with the model in eval mode
 * (argus/models.py:66-90 under torch.autograd.grad after model.eval()). With BN folded the network is
 * conv + bias + ReLU, so its backward is one data-gradient GEMM per conv over the same folded weights, the
 * producer's ReLU derivative applied in the epilogue. `d` is always the forward conv's descriptor, of the
 * four kinds argus_conv_infer serves; dtype ARGUS_F32 or ARGUS_BF16 (ARGUS_F16, ARGUS_FP8 and unknown
 * values: ARGUS_ERR_ARG, "dtype" in the message; there is no fp16 gradient). No weight gradients. Nothing
 * here allocates or synchronises: every call can be captured into a graph.
 *
 * argus_conv_fold_bn_dgrad: argus_conv_fold_bn's inputs; w_fold_dgrad[c][r'][s'][k] = T(w[k][c][r][s] *
 * scale[k]) with r' = R-1-r, s' = S-1-s: the transposed, 180-degree-rotated filter, [C][R*S*K], each element
 * the same single fp32 multiply and rounding as argus_conv_fold_bn's (the two copies hold identical values
 * in different places). */
int argus_conv_fold_bn_dgrad(const argus_conv_desc* d, int dtype, const float* w_master, const int64_t* strides,
                             const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, void* w_fold_dgrad, argus_stream_t stream);
/* Plan of argus_conv_infer_dgrad for `d`: *splits = splits_in, or the library's choice when splits_in == 0
 * (argus_conv_infer_splits' cost model on the mirrored problem: n*h*w rows, c columns, r*s*k reduction);
 * *max_splits = the k-steps of the reduction (r*s*k / 64 in bf16, / 32 in fp32); *workspace_bytes = what
 * *splits slices need (0 for <= 1), laid out as argus_conv_infer's. splits_in outside 0..max: ARGUS_ERR_ARG. */
int argus_conv_infer_dgrad_plan(const argus_conv_desc* d, int dtype, int splits_in, int* splits, int* max_splits,
                                size_t* workspace_bytes);
/* dx = (mask_src > 0 ? 1 : 0) * (conv_transpose(dy, w) + addend): dy (n, ho, wo, k); dx, addend (may be
 * NULL) and mask_src (may be NULL: no mask) (n, h, w, c), all NHWC in dtype; the sum is made in fp32 and
 * rounded once. mask_src is the conv's own input activation, the post-ReLU output of its producer: the
 * epilogue applies that ReLU's derivative (> 0, so 0 and NaN mask to 0). Every element of dx is written,
 * the pixels a stride-2 conv never reads included (their conv_transpose term is 0). splits / workspace
 * exactly as argus_conv_infer (same ticket protocol, the tickets zero on entry and on return, bitwise
 * reproducible for a given `splits`). */
int argus_conv_infer_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* w_fold_dgrad,
                           const void* addend, const void* mask_src, void* dx, int splits, void* workspace,
                           size_t workspace_bytes, argus_stream_t stream);
/* ---- frozen fine-tuning (ABI 21, added without a version change: detect by symbol) --------------
 * Parameter gradients of the folded network: what loss.backward() leaves in .grad through nn.Conv2d +
 * nn.BatchNorm2d.eval() of torchvision's Bottleneck.forward with the model in eval mode (argus/models.py:66-90,
 * argus/train.py:298-321 after model.eval()). From a conv's input x and the masked output gradient dm that
 * argus_conv_infer_dgrad's chain produces, argus_conv_wgrad(x, dm) is dL/d(w_fold); the two entries below add
 * dL/d(bias) and the chain rule through argus_conv_fold_bn back to (w, gamma, beta). Nothing here allocates or
 * synchronises: every call can be captured into a graph. No floating-point atomics; plain vector stores.
 *
 * argus_bias_grad: db[k] (fp32) = sum_p dm[p][k] over an NHWC [pixels][channels] tensor in dtype ARGUS_F32 or
 * ARGUS_BF16 (ARGUS_F16, ARGUS_FP8 and unknown values: ARGUS_ERR_ARG, "dtype" in the message); channels a
 * multiple of 64, dm 16-byte aligned. The pixels may be sliced over workgroups: splits 0 = the library's
 * choice, 1 = no split (no workspace touched, workspace may be NULL), up to *max_splits of the plan
 * (min(pixels, 64)); each slice stores an fp64 partial row and the last-arriving workgroup of a 64-column
 * block adds the slices in slice order, so the result is bitwise reproducible for a given `splits`. A thread
 * adds runs of at most 64 rows in fp32, everything above in fp64, rounded once:
 * |db[k] - exact| <= 64 * 2^-24 * sum_p |dm[p][k]|. Workspace (16-byte aligned): uint32 tickets in the first
 * 4096 bytes, zero on entry and on return, the partial rows from byte 4096 on - argus_conv_infer_workspace_bytes'
 * layout, so one zeroed-once workspace serves argus_conv_infer, argus_conv_infer_dgrad and this entry in
 * stream order, and consecutive calls of different shapes.
 * argus_bias_grad_plan: as argus_conv_infer_dgrad_plan: *splits = splits_in or the library's choice for
 * splits_in == 0, *max_splits, *workspace_bytes = what *splits slices need (0 for <= 1). */
int argus_bias_grad_plan(int dtype, int64_t pixels, int channels, int splits_in, int* splits, int* max_splits,
                         size_t* workspace_bytes);
int argus_bias_grad(int dtype, int64_t pixels, int channels, const void* dm, float* db, int splits, void* workspace,
                    size_t workspace_bytes, argus_stream_t stream);
/* The derivative of argus_conv_fold_bn (fp32 throughout; `d` as for the fold, w_master read through `strides`
 * as the fold reads it, NULL = OHWI contiguous). With invstd = 1 / sqrt(running_var + eps) and scale = gamma *
 * invstd, bit-identical to argus_bn_eval_coeffs, dwf [k][r*s*c] = dL/d(w_fold) as argus_conv_wgrad writes it and
 * db = dL/d(bias):
 *   dw[k][j] = scale[k] * dwf[k][j]       OHWI contiguous; dw == dwf (in place) is allowed
 *   dgamma[k] = invstd[k] * (sum_j dwf[k][j] * w[k][j] - running_mean[k] * db[k])
 *   dbeta[k] = db[k]                      dbeta == db is allowed
 * The fold's rounding of w * scale to the compute dtype is treated as the identity (straight-through). The row
 * sum is 64 lane-strided partials and a fixed 6-level tree (at most 72 + 6 additions deep), one launch per
 * conv, one wave per filter row, no workspace. dwf and dw 16-byte aligned. */
int argus_conv_fold_bn_bwd(const argus_conv_desc* d, const float* w_master, const int64_t* strides,
                           const float* gamma, const float* running_mean, const float* running_var, float eps,
                           const float* dwf, const float* db, float* dw, float* dgamma, float* dbeta,
                           argus_stream_t stream);
/* Table-driven folds (ABI 21, added without a version change: detect by symbol): one launch for the folds of
 * many convs and one for their derivatives, as argus_conv_weight_prep_batch is for argus_conv_weight_prep. A
 * fine-tuning step re-folds every trainable conv twice per step and differentiates every fold once; at two to
 * sixteen images these launches are short and their count is the cost.
 *
 * argus_conv_fold_bn_table writes `count` table entries of ARGUS_CONV_FOLD_ENTRY_BYTES each into host_table
 * (table_bytes >= count * ARGUS_CONV_FOLD_ENTRY_BYTES) from `src`, one argus_conv_fold_src per conv:
 *   desc                       the conv, of the kinds argus_conv_fold_bn serves (not the stem)
 *   w_master, strides          as argus_conv_fold_bn (strides: 4 host int64, NULL = OHWI contiguous)
 *   gamma, beta, running_mean, running_var, eps
 *   w_fold, bias               argus_conv_fold_bn's outputs
 *   w_fold_dgrad               argus_conv_fold_bn_dgrad's output, or NULL: that copy is not written
 *   dwf, dw, db, dgamma, dbeta argus_conv_fold_bn_bwd's operands (dw may be dwf; db may be another entry's
 *                              dbeta, which that entry's own db feeds: a downsample shares conv3's bias sum).
 *                              All five NULL in every entry: a table for the fold alone (*nblocks_bwd = 0).
 * and returns the two grid sizes. The caller copies host_table to device memory once; the table holds raw
 * device pointers and the shapes, so it is rebuilt only when one of them changes. The launching entries cannot
 * check a device table: pass the count and the grid sizes the table call returned.
 *
 * argus_conv_fold_bn_batch(dtype ARGUS_F32 or ARGUS_BF16; ARGUS_F16 stays on argus_conv_fold_bn): one launch
 * that writes w_fold, bias and (where given) w_fold_dgrad of every entry, each bit-identical to
 * argus_conv_fold_bn / argus_conv_fold_bn_dgrad. A workgroup owns a 64(k) x 64(c) tile of one filter tap: it
 * reads the master tile once, forms T(w * scale[k]), stores the forward rows directly and the transposed,
 * rotated rows through the LDS, both with 16-byte stores.
 * argus_conv_fold_bn_bwd_batch: one launch, one wave per filter row of every entry, argus_conv_fold_bn_bwd's
 * arithmetic in its order: bit-identical to it, in place or not. */
#define ARGUS_CONV_FOLD_ENTRY_BYTES 176
typedef struct {
  argus_conv_desc desc;
  const float* w_master;
  const int64_t* strides;
  const float *gamma, *beta, *running_mean, *running_var;
  float eps;
  void* w_fold;
  float* bias;
  void* w_fold_dgrad;
  const float* dwf;
  float* dw;
  const float* db;
  float *dgamma, *dbeta;
} argus_conv_fold_src;
int argus_conv_fold_bn_table(int count, const argus_conv_fold_src* src, void* host_table, size_t table_bytes,
                             int* nblocks_fold, int* nblocks_bwd);
int argus_conv_fold_bn_batch(int dtype, int count, const void* device_table, int nblocks, argus_stream_t stream);
int argus_conv_fold_bn_bwd_batch(int count, const void* device_table, int nblocks, argus_stream_t stream);

int argus_conv_fwd_stat_rows(const argus_conv_desc* d, int dtype);
int argus_conv_fwd_stat_tile(const argus_conv_desc* d, int dtype);
/* The partial layout (rows, tile as above) of a statistics-only argus_conv_fwd (y == NULL, no
 * prologue; ABI 16): bf16 1x1 stride-1 convs with 64..512 input channels run on a persistent kernel
 * (policy key 44) that writes one {sum, M2} row per row split and the int32 pixel counts after them
 * (negative tile: ragged rows); other convs as argus_conv_fwd_stat_rows / _stat_tile. */
int argus_conv_fwd_stats_only_rows(const argus_conv_desc* d, int dtype);
int argus_conv_fwd_stats_only_tile(const argus_conv_desc* d, int dtype);
/* The BatchNorm train-mode finalize of a forward conv's statistics (argus_bn_finalize's arguments
 * past its partial layout), for argus_conv_fwd_fin. workspace: argus_bn_workspace_bytes(k), zeroed once
 * (every call leaves it zeroed); running_mean / running_var / num_batches_tracked may be NULL. */
typedef struct argus_bn_fwd_fin {
  void* workspace;
  const float* gamma;
  const float* beta;
  float eps;
  float momentum;
  float* running_mean;
  float* running_var;
  int64_t* num_batches_tracked;
  float* mean;
  float* invstd;
  float* scale;
  float* shift;
} argus_bn_fwd_fin;
/* argus_conv_fwd (stat_part required) followed by argus_bn_finalize of its partials (the layout
 * argus_conv_fwd_stat_rows / _tile, or _stats_only_rows / _tile when y == NULL), with the finalize
 * folded into the conv's last-arriving workgroups where the producing kernel's row tiles align with
 * argus_bn_finalize's merge groups (otherwise it is launched after the conv): mean, invstd, scale, shift
 * and the running statistics are bit-identical to the two calls either way (ABI 18). Replaces the
 * BatchNorm2d train forward's statistics pass of torchvision's Bottleneck (argus/models.py:43). */
int argus_conv_fwd_fin(const argus_conv_desc* d, int dtype, const void* x, const void* w_fwd, void* y,
                       const float* pro_scale, const float* pro_shift, float* stat_part,
                       const argus_bn_fwd_fin* fin, argus_stream_t stream);
/* Bytes a stat_part buffer needs for argus_conv_fwd of d (stats_only = 0) or for its statistics-only
 * form (y == NULL, stats_only = 1): 2*rows*k floats plus, for a ragged tiling (negative tile), int32
 * counts[rows] after them (ABI 17). Size every statistics workspace with it; rows*k*2 floats alone is
 * too small for the ragged stem and the persistent statistics-only forward. 0 for a bad descriptor. */
size_t argus_conv_fwd_stat_part_bytes(const argus_conv_desc* d, int dtype, int stats_only);
/* dx = dgrad(dy, w_dgrad) [+ addend]: when addend != NULL (same NHWC layout as dx; may be dx itself
 * for in-place accumulation) it is added, element-wise masked by addend_mask when that is non-NULL
 * (the bn_apply ReLU mask: the residual path of a bottleneck, dx += relu'(out) * dout). */
int argus_conv_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* w_dgrad,
                     void* dx, const void* addend, const uint8_t* addend_mask, argus_stream_t stream);
/* dgrad whose output feeds the backward of a BatchNorm (+ReLU): the BN-backward reduction
 * (argus_bn_bwd_reduce) runs in the dgrad epilogue instead of as its own pass over dz.
 * With v = dgrad(dy, w_dgrad) [+ addend] (addend unmasked, may alias dm), the kernel stores
 * dm = v * mask (mask_mode 2: y*scale+shift > 0, the BN's own ReLU; 3: mask_bits of argus_bn_apply,
 * a block output) and writes part float2[rows][C] = {sum dm, sum dm*(y-mean)*invstd}, rows =
 * argus_conv_dgrad_bn_rows(d, dtype) (C = d->c) — the input of argus_bn_bwd_finalize. Optional second
 * branch (mask_mode 3): y2/mean2/invstd2 -> part2 (the downsample BN of a bottleneck sharing dm).
 * Replaces the ATen batch_norm_backward reduction behind loss.backward() (argus/train.py:316). */
typedef struct {
  const void* y;
  const float* mean;
  const float* invstd;
  int32_t mask_mode;
  int32_t reserved;
  const float* scale;
  const float* shift;
  const uint8_t* mask_bits;
  const void* y2;
  const float* mean2;
  const float* invstd2;
  float* part;
  float* part2;
  /* Optional: with workspace != NULL (argus_bn_workspace_bytes(c), zero-filled once) the BN-backward
   * finalize (argus_bn_bwd_finalize) is folded into the same launch: the last workgroups merge the
   * partials and write dgamma/dbeta (may be NULL) and ca/cb/cc with gamma (+ the second branch). */
  void* workspace;
  const float* gamma;
  float* dgamma;
  float* dbeta;
  float* ca;
  float* cb;
  float* cc;
  const float* gamma2;
  float* dgamma2;
  float* dbeta2;
  float* ca2;
  float* cb2;
  float* cc2;
  /* Optional (ABI 15): with y_x != NULL the main branch's y is not read but recomputed in the kernel as
   * the 1x1 stride-1 convolution of y_x (NHWC, y_k channels, the same pixel grid as dm) with y_w (the
   * bf16 w_fwd copy of that conv, [C][y_k], argus_conv_weight_prep): bit-identical to the y that
   * argus_conv_fwd would have stored, so y itself need not exist (argus_conv_fwd_bn_out with y = NULL).
   * bf16, mask_mode 3, y_k a multiple of 64; y must then be NULL. */
  const void* y_x;
  const void* y_w;
  int32_t y_k;
  int32_t reserved2;
} argus_bn_bwd_epilogue;
/* Optional BN-backward apply folded into the dgrad's operand staging: with `pro` != NULL the `dy`
 * argument of argus_conv_dgrad_bn holds dm (the masked gradient of a BN output) and the dgrad consumes
 * dy = ca*dm + cb*y + cc (per channel; argus_bn_bwd_apply's formula), which it also stores to dy_out
 * for the weight gradient. Kernels that cannot stage it run argus_bn_bwd_apply first (same result).
 * `bn` may be NULL with a prologue: a plain dgrad (no BN-backward epilogue) of the applied dy.
 * dy_out may be NULL when argus_conv_dgrad_stages_prologue(d, dtype) is 1 (1x1 dgrads on the
 * register-staged kernel): dy is then never stored, and the weight gradient stages the same apply
 * from dm itself (argus_conv_wgrad_apply). */
typedef struct {
  const void* y;
  const float* ca;
  const float* cb;
  const float* cc;
  void* dy_out;
} argus_bn_bwd_prologue;
int argus_conv_dgrad_bn_rows(const argus_conv_desc* d, int dtype);
/* 1 when argus_conv_dgrad_bn stages an apply prologue inside the dgrad kernel for this conv (so
 * dy_out may be NULL), 0 when it materialises dy with argus_bn_bwd_apply first. */
int argus_conv_dgrad_stages_prologue(const argus_conv_desc* d, int dtype);
int argus_conv_dgrad_bn(const argus_conv_desc* d, int dtype, const void* dy, const void* w_dgrad,
                        void* dm, const void* addend, const argus_bn_bwd_epilogue* bn,
                        const argus_bn_bwd_prologue* pro, argus_stream_t stream);
/* MX-fp8 stored operands (ABI 16; ARGUS_FP8 networks, the 3x3 stride-1 convs of Bottleneck.conv2 in
 * torchvision's ResNet-50 layers 2-4, argus/models.py:43). An "x8" tensor is the MX-fp8 copy of a bf16
 * NHWC tensor [P][C]: P*C e4m3 bytes (OCP, the value / 2^e rounded to nearest even) followed by P*C/32
 * E8M0 scale bytes (127 + e, one per 32 consecutive channels of a pixel), e chosen as ARGUS_FP8's
 * staging quantizer chooses it; argus_bn_apply_x8 / argus_bn_bwd_apply_x8 write it beside their bf16
 * output. argus_conv_fwd_x8 is argus_conv_fwd(ARGUS_FP8) without a prologue, its input read as the x8
 * copy x8 (bit-identical to quantizing the bf16 input while staging); argus_conv_dgrad_bn_x8 is
 * argus_conv_dgrad_bn(ARGUS_FP8) with dy read as x8 (bn NULL, or mask mode 2; no addend / prologue /
 * y recompute). Both need the fp8 weight copies of argus_conv_weight_prep(ARGUS_FP8): policy key 37
 * bit 8 (forward of 3x3 stride-1 convs) and bit 2 (3x3 data gradients). argus_conv_x8_ok(d, pass)
 * is 1 when pass 0 (forward) / 1 (data gradient) of d is served (C resp. K % 128 == 0, the LDS-halo
 * shapes, the policy bits). */
int argus_conv_x8_ok(const argus_conv_desc* d, int pass);
int argus_conv_fwd_x8(const argus_conv_desc* d, const void* x8, const void* w_fwd, void* y, float* stat_part,
                      argus_stream_t stream);
int argus_conv_dgrad_bn_x8(const argus_conv_desc* d, const void* dy8, const void* w_dgrad, void* dm,
                           const argus_bn_bwd_epilogue* bn, argus_stream_t stream);
/* Kernel-selection policy: the library's immutable default of a key (-1 for an unknown key); a conv
 * descriptor may override keys for its own call (argus_conv_desc.tuning; an unknown key there makes
 * the call fail with ARGUS_ERR_ARG). Every default is the measured best.
 * key 0..2 force the row tile (64|128, 0 = heuristic) of pass fwd/dgrad/wgrad, key 3..5 the column
 * tile, key 6 the wgrad split target (workgroups), key 7 the largest K (= taps*C) served by the
 * 4-workgroups-per-CU single-buffer forward/dgrad kernel, key 8 the smallest K served by the bf16
 * global->LDS (glds) forward/dgrad kernel (0 disables it), key 9 the fewest workgroups for which
 * that kernel is chosen, key 10 enables (1) or disables (0) the LDS-halo kernel for 3x3 stride-1
 * forward/dgrad, key 11 the same for the 3x3 stride-1 weight gradient and key 12 its split target,
 * key 13 the fewest workgroups for the fwd/dgrad halo kernel (1 also allows its 64-channel variant
 * at any size), key 14 the most (64 x 64) channel tiles for the wgrad halo kernel, key 19 the bf16
 * stem forward on the LDS-patch kernel (1) or the implicit GEMM (0), key 27 the split target of the
 * register-staged 3x3 weight gradient, key 34 the bf16 stem weight gradient on the LDS-patch kernel
 * (1) or on the register-staged weight-gradient kernel (0), key 35 the fewest GEMM rows (output
 * pixels) for which the forward uses 128-row tiles (fewer: 64), key 36 the fewest GEMM rows for the
 * glds kernel, key 37 which ARGUS_FP8 passes take MX-fp8 operands (bits: 1 forward, 2 data gradient of
 * a 3x3 conv, 4 data gradient of a 1x1 conv, 8 forward of a 3x3 stride-1 conv; default 10;
 * argus_conv_weight_prep follows the same key), key 42 the
 * workgroups per CU (4 or 3) the small-K BN-epilogue / apply-prologue data gradients are built for,
 * key 43 the bottleneck conv1 data gradients on the persistent kernel (1) or the igemm (0), key 44 the
 * statistics-only 1x1 forwards on the persistent kernel (1) or the igemm (0), key 45 the 1x1 bf16
 * weight gradients on the LDS-DMA ring kernel with 128 x 128 tiles (1), 128 x 256 tiles where
 * Cin % 256 == 0 for the BN-backward-apply form (2) or both forms (3), or the register-staged one (0);
 * key 46 the pixel count up to which 1x1 weight gradients take half the split target (key 6); key 47
 * the stride-2 plain bf16 weight gradients (1x1, 3x3) on the DMA kernel with gathered x rows: 0 never,
 * 1 at every size, a larger value up to that many output pixels (default 131072); key 48 the LDS ring
 * stages (2..5, default 4) of the 128 x 256 BN-backward-apply form of that kernel; key 49 the most
 * 128-column tiles for which a 1x1 data gradient stages its apply prologue itself (more: dy is
 * materialised first; 0 = always staged; default 4); key 51 the 3x3 halo forward / data gradient with a
 * four-stage weight ring where the tile's halo fits 384 positions (1) or the three-stage ring (0,
 * default); key 53 (ABI 21) the passes of an ARGUS_F32 conv that run the bf16x3 split arithmetic (bits: 1
 * forward, 2 data gradient, 4 weight gradient; default 0 = the exact fp32 MFMA): tensors, accumulators,
 * epilogues and BN statistics stay fp32, each GEMM operand is split while staged into hi = bf16(x) and
 * lo = bf16(x - hi), and hi*hi + hi*lo + lo*hi is accumulated in fp32 on the bf16 MFMA, in that fixed
 * order (deterministic), |error| <= 4 * 2^-16 * sum |a*b| per output. gfx950 has no TF32 / xf32 MFMA:
 * this is what torch.set_float32_matmul_precision("high") stands for here. Honoured by every conv entry
 * point given ARGUS_F32 (argus_conv_fwd, _fwd_apply_out, _fwd_fin, argus_conv_dgrad, _dgrad_bn,
 * argus_conv_wgrad, _wgrad_apply), ignored for ARGUS_BF16 / ARGUS_FP8; weight prep, the statistics /
 * workspace queries and argus_conv_launch_info do not depend on it. Non-finite inputs and inputs above
 * the bf16 maximum (~3.39e38) give NaN; lo parts that are bf16 subnormals may be flushed to zero.
 * Key 50 was removed and is unknown, like key 30; key 52 is unknown.
 * (Keys scaled with the batch keep a smaller batch's kernel selection that of the larger one:
 * tests/test_gpu_parity.py stage-checks the benched configurations' kernels that way.) */
int argus_conv_policy_default(int key);
/* Which tile a pass launches and its algorithmic work: pass 0 fwd, 1 dgrad, 2 wgrad. Returns a
 * tag (kind*10^7 + dtype*10^6 + tile_m*1000 + tile_n; kind 1 igemm, 2 wgrad) and writes
 * 2*P*K*R*S*C flops (P = n*ho*wo output pixels). */
int argus_conv_launch_info(const argus_conv_desc* d, int dtype, int pass, int64_t* flops);
/* dw (fp32, OHWI 7x7x3 for the stem) = sum over pixels of dy x im2col(x'), x' as in conv_fwd. */
size_t argus_conv_wgrad_workspace_bytes(const argus_conv_desc* d, int dtype);
int argus_conv_wgrad(const argus_conv_desc* d, int dtype, const void* x, const float* pro_scale,
                     const float* pro_shift, const void* dy, float* dw, void* workspace,
                     size_t workspace_bytes, argus_stream_t stream);
/* Weight gradient whose dy = ca*dm + cb*y + cc (BN-backward apply, argus_bn_bwd_apply's formula) is
 * formed while staging its operand from dm (ap->dy_out is ignored): dy is never materialised. Used
 * for the stem (whose dy feeds nothing else) and for the 1x1 convs whose dgrad stages the same apply
 * (argus_conv_dgrad_stages_prologue). Runs the register-staged wgrad kernel; the input x has no
 * BN prologue. */
int argus_conv_wgrad_apply(const argus_conv_desc* d, int dtype, const void* x, const void* dm,
                           const argus_bn_bwd_prologue* ap, float* dw, void* workspace,
                           size_t workspace_bytes, argus_stream_t stream);
/* Data gradient of the stem convolution: autograd's grad_input of resnet.conv1 (torchvision conv1, 7x7
 * stride 2 pad 3, 3 -> 64 channels; argus/models.py:43) under loss.backward() (argus/train.py:316) when
 * the images require grad, i.e. F.conv2d's gradient with respect to its input. `d` is a stem descriptor
 * (stem = 1, c = 3, k = 64); dtype ARGUS_F32 or ARGUS_BF16 (anything else: ARGUS_ERR_ARG). `dy` is
 * (n, ho, wo, 64) NHWC in dtype; with `ap` it holds dm and the kernel consumes ca*dm + cb*y + cc per
 * channel, formed while staging with argus_bn_bwd_apply's formula and rounding (bf16: rounded to bf16
 * before the product; ap->dy_out is ignored, nothing is materialised). `w_fwd` is the stem's compute copy
 * [64][8][8][4] that argus_conv_weight_prep writes. `dx_nchw` is fp32 (n, 3, h, w) planar (folded over the
 * cameras: the (B, 3*n_cams, H, W) images layout); every element is written, accumulation is fp32 (fp32
 * mode: the exact fp32 MFMA), each output sums its own 9..16 taps in a fixed order: bit-reproducible, no
 * atomics. Allocates nothing, synchronises nothing, capturable. */
int argus_conv_stem_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* w_fwd,
                          const argus_bn_bwd_prologue* ap, float* dx_nchw, argus_stream_t stream);
/* Data and weight gradient of one 1x1 stride-1 conv in one pass over its output gradient (torch's
 * convolution backward with output_mask (grad_input, grad_weight) for Bottleneck.conv3 of ResNet-50
 * layer 1 and of the first block's downsample, reached from loss.backward() at argus/train.py:316;
 * replaces argus_conv_dgrad_bn (argus_conv_dgrad) +
 * argus_conv_wgrad_apply for that conv). `dm`, `pro` as in argus_conv_dgrad_bn with an apply
 * prologue (pro->dy_out must be NULL: dy is never stored); `bn` a mask-mode-2 BN-backward epilogue
 * (its partial rows: argus_conv_dgrad_wgrad_bn_rows; with bn->workspace the finalize is folded), or
 * NULL for a plain dx, optionally dx += addend (may alias dx; the first block's downsample);
 * x = the conv input (for dw, fp32 OHWI). bf16 only, C = 64 input and K = 256 output channels
 * (argus_conv_dgrad_wgrad_ok); workspace: argus_conv_dgrad_wgrad_workspace_bytes. */
int argus_conv_dgrad_wgrad_ok(const argus_conv_desc* d, int dtype);
size_t argus_conv_dgrad_wgrad_workspace_bytes(const argus_conv_desc* d, int dtype);
int argus_conv_dgrad_wgrad_bn_rows(const argus_conv_desc* d, int dtype);
int argus_conv_dgrad_wgrad_bn(const argus_conv_desc* d, int dtype, const void* dm, const void* w_dgrad,
                              const void* x, void* dx, const void* addend, const argus_bn_bwd_epilogue* bn,
                              const argus_bn_bwd_prologue* pro, float* dw, void* workspace,
                              size_t workspace_bytes, argus_stream_t stream);

/* ---- kernel timer (bench.py roofline) ------------------------------------------------------------
 * While enabled, conv and BN kernel launches whose demangled instantiation name (e.g.
 * "argus::igemm_kernel<__bf16, 128, 128, false, true>", as c++filt prints rocprofv3's kernel name)
 * starts with `filter` (NULL or "" = all) are dispatched with hipExtLaunchKernelGGL start/stop
 * events, i.e. timed by the dispatch packet on the launch stream. enable() clears old records;
 * count() synchronizes the recorded events, aggregates per name and returns the number of names;
 * get(i) returns name, launches, total milliseconds, total algorithmic flops (0 for BN kernels) and
 * total algorithmic HBM bytes (each operand read once and each result written once; for wgrad the
 * fp32 split partials it writes count too). */
int argus_ktimer_enable(const char* filter);
/* argus_ktimer_enable restricted to launches on `stream` (e.g. the caller's main stream: the
 * critical path of a step whose weight gradients run on a side stream). */
int argus_ktimer_enable_on(const char* filter, argus_stream_t stream);
int argus_ktimer_disable(void);
int argus_ktimer_count(void);
int argus_ktimer_get(int index, char* name, int name_len, int64_t* launches, double* total_ms,
                     double* work, double* bytes);

/* ---- BatchNorm2d (train: batch stats, eps, momentum; eval: running stats) --------------------- */
/* Workspace of argus_bn_finalize / argus_bn_bwd_finalize / the folded finalize of argus_conv_dgrad_bn
 * for up to `channels` channels. Its first 16 KiB hold inter-workgroup ticket counters: zero-fill the workspace ONCE when it is allocated;
 * the kernels leave the counters zero (do not share one workspace between concurrent streams). */
size_t argus_bn_workspace_bytes(int channels);
/* From tile partials float2[rows][C] = {sum, M2 (sum of squared deviations from the tile mean)},
 * tile t holding min(tile_rows, count - t*tile_rows) elements per channel (as argus_conv_fwd
 * writes them; tile_rows < 0, as argus_conv_fwd_stat_tile reports for a producer with ragged tiles:
 * row r holds counts[r] <= |tile_rows| elements, the int32 counts[rows] stored right after the
 * float2[rows][C] partials, i.e. at (const int*)(part + 2*rows*C)): merged
 * in fp64 (Chan), gives mean, invstd, the fused apply coefficients
 * scale = gamma*invstd, shift = beta - mean*scale; updates running stats (momentum, unbiased
 * variance) and num_batches_tracked when those pointers are non-NULL. */
int argus_bn_finalize(int channels, int rows, int tile_rows, const float* part, int64_t count,
                      const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                      float* scale, float* shift, void* workspace, argus_stream_t stream);
int argus_bn_eval_coeffs(int channels, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps,
                         float* scale, float* shift, argus_stream_t stream);
/* out = [relu]( y*scale+shift + residual' ), residual' = res*res_scale+res_shift (if res_scale),
 * res (if res), else 0. out may alias y. If mask_out != NULL it also receives the ReLU mask of out:
 * one byte per 16-byte chunk (8 bf16 / 4 fp32 channels), bit j set <=> element j of the chunk > 0,
 * i.e. mask_out[(pixel*channels + c) / E] bit (c % E).
 * Channels: a multiple of E; above 256 chunks (2048 bf16 / 1024 fp32 channels) a multiple of 256 chunks,
 * else ARGUS_ERR_SHAPE before any launch. The same holds for argus_bn_apply_x8, argus_bn_bwd_reduce,
 * argus_bn_bwd_apply and argus_bn_bwd_apply_x8. */
int argus_bn_apply(int dtype, int64_t pixels, int channels, const void* y, const float* scale,
                   const float* shift, const void* res, const float* res_scale,
                   const float* res_shift, int relu, void* out, uint8_t* mask_out,
                   argus_stream_t stream);
/* argus_bn_apply (bf16, channels % 32 == 0) that also writes the x8 copy of out to out8 (ABI 16;
 * argus_conv_fwd_x8). */
int argus_bn_apply_x8(int64_t pixels, int channels, const void* y, const float* scale, const float* shift,
                      const void* res, const float* res_scale, const float* res_shift, int relu, void* out,
                      uint8_t* mask_out, void* out8, argus_stream_t stream);
/* Backward. mask_mode: 0 none; 1 relu mask from the tensor `mask` (>0, e.g. a block output);
 * 2 relu mask recomputed from y as (y*scale+shift > 0); 3 relu mask from the bits `mask` written
 * by argus_bn_apply. dm = dz*mask.
 * reduce: part float2[rows][C] = {sum dm, sum dm*(y-mean)*invstd}; rows = argus_bn_bwd_rows().
 * Optional second branch (y2 != NULL; modes 0/1/3): a second BN whose output was summed with the
 * first before the same ReLU (bn3 + the downsample BN of a bottleneck) shares dm, so both are
 * reduced / applied in one pass: part2 = {sum dm, sum dm*(y2-mean2)*invstd2}, dy2 = ca2*dm + cb2*y2 + cc2. */
int argus_bn_bwd_rows(int64_t pixels, int channels);
int argus_bn_bwd_reduce(int dtype, int64_t pixels, int channels, const void* dz, int mask_mode,
                        const void* mask, const void* y, const float* scale,
                        const float* shift, const float* mean, const float* invstd, float* part,
                        const void* y2, const float* mean2, const float* invstd2, float* part2,
                        argus_stream_t stream);
/* dgamma/dbeta (fp32, written) and coefficients so that dy = ca*dm + cb*y + cc. */
int argus_bn_bwd_finalize(int channels, int rows, const float* part, int64_t count,
                          const float* gamma, const float* mean, const float* invstd,
                          float* dgamma, float* dbeta, float* ca, float* cb, float* cc,
                          void* workspace, argus_stream_t stream);
/* dy = ca*dm + cb*y + cc (dtype); if dm_out != NULL also writes dm (the masked dz). */
int argus_bn_bwd_apply(int dtype, int64_t pixels, int channels, const void* dz, int mask_mode,
                       const void* mask, const void* y, const float* scale, const float* shift,
                       const float* ca, const float* cb, const float* cc, void* dy, void* dm_out,
                       const void* y2, const float* ca2, const float* cb2, const float* cc2, void* dy2,
                       argus_stream_t stream);
/* dy = ca*dm + cb*y + cc from an already-masked dm (mask mode 0, bf16, channels % 32 == 0), plus the
 * x8 copy of dy in dy8 (ABI 16; argus_conv_dgrad_bn_x8). */
int argus_bn_bwd_apply_x8(int64_t pixels, int channels, const void* dm, const void* y, const float* ca,
                          const float* cb, const float* cc, void* dy, void* dy8, argus_stream_t stream);

/* ---- pooling (MaxPool2d(3,2,1) fused with the stem's BN+ReLU; AdaptiveAvgPool2d(1)) ----------- */
int argus_maxpool_fwd(int dtype, int n, int h, int w, int c, const void* y, const float* scale,
                      const float* shift, void* out, uint8_t* argmax, argus_stream_t stream);
int argus_maxpool_bwd(int dtype, int n, int h, int w, int c, const void* dout,
                      const uint8_t* argmax, void* dz, argus_stream_t stream);
/* maxpool backward with the stem BatchNorm's backward reduction fused (the pooled tensor is
 * relu(y*scale+shift), y the stem conv output): stores dm = dz * (y*scale+shift > 0) and
 * part float2[argus_maxpool_bwd_bn_rows()][c] = {sum dm, sum dm*(y-mean)*invstd}, the input of
 * argus_bn_bwd_finalize. y == NULL: plain argus_maxpool_bwd. */
int argus_maxpool_bwd_bn_rows(int dtype, int n, int h, int w, int c);
int argus_maxpool_bwd_bn(int dtype, int n, int h, int w, int c, const void* dout, const uint8_t* argmax,
                         void* dm, const void* y, const float* scale, const float* shift,
                         const float* mean, const float* invstd, float* part, argus_stream_t stream);
/* argus_maxpool_bwd_bn with argus_bn_bwd_finalize folded in (ABI 13; c % 64 == 0): the last workgroups
 * of the pass merge `part` (write-through, deterministic fixed order) and write dgamma/dbeta (may be
 * NULL) and ca/cb/cc exactly as argus_bn_bwd_finalize(c, rows, part, n*h*w, gamma, mean, invstd, ...)
 * would; `workspace` is an argus_bn_workspace_bytes(c) BN workspace (zeroed once, not shared between
 * concurrent streams). workspace == NULL: argus_maxpool_bwd_bn. Backward of the torchvision stem
 * bn1 -> relu -> maxpool inside self.resnet(x) (models.py:43,84) under loss.backward() (train.py:316). */
int argus_maxpool_bwd_bn_fin(int dtype, int n, int h, int w, int c, const void* dout, const uint8_t* argmax,
                             void* dm, const void* y, const float* scale, const float* shift,
                             const float* mean, const float* invstd, float* part, const float* gamma,
                             float* dgamma, float* dbeta, float* ca, float* cb, float* cc, void* workspace,
                             argus_stream_t stream);
int argus_avgpool_fwd(int dtype, int n, int hw, int c, const void* x, float* feat,
                      argus_stream_t stream);
int argus_avgpool_bwd(int dtype, int n, int hw, int c, const float* dfeat, void* dx,
                      argus_stream_t stream);
/* argus_avgpool_bwd through the ReLU that produced the pooled tensor: dx = dfeat/hw * (out > 0), `out` the
 * (n, hw, c) post-ReLU activation in dtype (the last Bottleneck's output under torch.autograd.grad in eval
 * mode, argus/models.py:66-90). ARGUS_F32 or ARGUS_BF16. */
int argus_avgpool_bwd_relu(int dtype, int n, int hw, int c, const float* dfeat, const void* out, void* dx,
                           argus_stream_t stream);

/* ---- FC / MLP head (nn.Linear + exact GELU; models.py:56-64,88), fp32 ------------------------ */
/* C[m][n] = sum_k opA(A)[m][k] * opB(B)[k][n]; opA(A)[m][k] = trans_a ? A[k*lda+m] : A[m*lda+k],
 * opB(B)[k][n] = trans_b ? B[n*ldb+k] : B[k*ldb+n].
 * epilogue 0: C = acc; 1: C = acc + bias[n]; 2: aux = acc + bias[n], C = gelu(aux);
 * 3: C = acc * gelu'(aux[m][n]) (backward through a GELU whose pre-activation is aux, ld = ldc);
 * 4: C += acc. Small-output / long-K products split K over workgroups (deterministic fixed-order
 * reduce) when a workspace of argus_gemm_f32_workspace_bytes() is given (NULL: no split). */
size_t argus_gemm_f32_workspace_bytes(int m, int n, int k);
int argus_gemm_f32(int m, int n, int k, const float* a, int lda, int trans_a, const float* b,
                   int ldb, int trans_b, float* c, int ldc, const float* bias, int epilogue,
                   float* aux, void* workspace, size_t workspace_bytes, argus_stream_t stream);
/* out[n] = sum_m x[m*ld + n] (bias gradients). */
int argus_colsum_f32(int m, int n, const float* x, int ld, float* out, argus_stream_t stream);
int argus_gelu_f32(int64_t count, const float* x, float* y, argus_stream_t stream);
int argus_gelu_bwd_f32(int64_t count, const float* x, const float* dy, float* dx,
                       argus_stream_t stream);

/* ---- SE(3) geodesic loss (geometric_loss_fn, argus/train.py:105-119; pypose Exp/Inv/@/Log) ---- */
/* loss[b] = |Log(Exp(pred_b) @ target_b^-1)|^2 ; dpred[b] = grad_scale * d loss[b] / d pred[b]
 * (dpred may be NULL). pred (B,6) [rho, phi]; target (B,7) [t, qx, qy, qz, qw]. */
int argus_se3_loss(int batch, const float* pred, const float* target, float* loss, float* dpred,
                   float grad_scale, argus_stream_t stream);

/* se(3) -> SE(3) exponential (pypose se3.Exp; get_pose, argus/utils.py:179-189): out (B,7) =
 * [t, qx, qy, qz, qw]; canonical_w != 0 flips q to w >= 0. */
int argus_se3_exp(int batch, const float* xi, float* out, int canonical_w, argus_stream_t stream);

/* ---- frozen pose session: the two ends of the forward fused (PoseSession, argus_amd/pose_session.py) ---- */
/* Where argus_stem_infer reads its frames. Channel c of pixel (y, x) of image i is element
 * base[i*stride_img + c*stride_c + (y0 + y)*stride_y + (x0 + x)*stride_x] (strides in elements, >= 0; within
 * one image the offsets from the crop origin must fit 31 bits). Planar (B, 3*n_cams, H, W): stride_img = 3*H*W,
 * stride_c = H*W, stride_y = W, stride_x = 1. Interleaved camera frames (B, n_cams, Hs, Ws, 3): stride_img =
 * 3*Hs*Ws, stride_c = 1, stride_y = 3*Ws, stride_x = 3, with (y0, x0) the crop origin. */
typedef struct {
  const void* base;
  int32_t in_dtype; /* 0 uint8 (v / 255), 1 fp32 */
  int64_t stride_img, stride_c, stride_y, stride_x;
  int32_t src_h, src_w; /* the source frame; y0 + h <= src_h and x0 + w <= src_w are checked */
  int32_t y0, x0;       /* crop origin */
} argus_frame_src;

/* out[n][ph][pw][k] = T(max over the 3x3 / stride 2 / pad 1 window of relu(conv7x7s2p3(x)[..][k] * scale[k] +
 * shift[k])): resnet.conv1 -> bn1.eval() -> relu -> maxpool (torchvision resnet.py; argus/models.py:84) in one
 * launch, from the frames as the camera delivers them: replaces the `.permute(0, 3, 1, 2)` + `cat` + center
 * crop of argus/validate_real.py:58-75 and, in a frozen session, argus_images[_u8]_to_nhwc4 + argus_conv_fwd
 * (stem) + argus_maxpool_fwd. A pixel becomes T(v) (uint8: T(v / 255.0f)), the bits argus_images_to_nhwc4
 * stores; w_fwd is argus_conv_weight_prep's padded stem copy [64][8][8][4]; scale / shift (fp32,
 * argus_bn_eval_coeffs) are applied to the fp32 accumulator and the result is rounded to T once. out:
 * (n_img, H2, W2, 64) NHWC with H1 = (h - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1. out_dtype (T; the frames have
 * their own in_dtype) is ARGUS_BF16 or ARGUS_F16
 * (ARGUS_F32, ARGUS_FP8 and unknown values: ARGUS_ERR_ARG, "dtype" in the message); k = 64; h, w >= 8. Nothing
 * allocates or synchronises (graph-capturable); every bad argument is refused before a launch. */
int argus_stem_infer(int out_dtype, int n_img, int h, int w, int k, const argus_frame_src* src, const void* w_fwd,
                     const float* scale, const float* shift, void* out, argus_stream_t stream);

/* A region of interest per image, resampled to h x w (added at ABI 21 without a version change: detect by
 * symbol). rois: device memory, [n_img][4] fp32 = (y0, x0, height, width) in source pixels (fractional values
 * allowed), read by every launch, so a captured graph follows what the caller writes there. The filter is the
 * antialiased triangle of PIL / F.interpolate(mode="bilinear", antialias=True, align_corners=False). Per axis,
 * with source length S, output length n, origin o and extent e (pixel j covers [j, j + 1)):
 *   s = e / n, r = max(s, 1), c_i = o + (i + 0.5) * s,
 *   taps j = max(0, floor(c_i - r + 0.5)) .. min(S, floor(c_i + r + 0.5)) - 1,
 *   t_ij = max(0, 1 - |j + 0.5 - c_i| / r), w_ij = t_ij / sum_j t_ij
 * and a pixel is sum_y wy * sum_x wx * v in fp32 (uint8: v / 255.0f), rounded to T once. At unit scale and an
 * integer origin that is the crop, bit for bit. Served (the CALLER validates: the values live on the device):
 * finite, 0 <= o, o + e <= S, n / 4 <= e <= 4 n (at most 9 taps an axis). For any other bit pattern the result
 * is unspecified but every read stays inside the frame. src->y0 and src->x0 must be 0 (the region holds the
 * origin); one image's offsets over the WHOLE frame must fit 31 bits. out_dtype ARGUS_BF16 or ARGUS_F16
 * (anything else: ARGUS_ERR_ARG, "dtype" in the message); h, w >= 8; nothing allocates or synchronises; every
 * bad argument is refused before a launch.
 *
 * argus_frames_resample writes x0 (n_img, h, w, 4) of T: the NHWC4 tensor argus_images_to_nhwc4 would write
 * for the resampled frames (channel 3 = 0). argus_stem_infer_roi is argus_stem_infer on those pixels without
 * the tensor: the same device function fills its patch, so it equals argus_stem_infer fed x0 bit for bit. */
int argus_frames_resample(int out_dtype, int n_img, int h, int w, const argus_frame_src* src, const float* rois,
                          void* x0, argus_stream_t stream);
int argus_stem_infer_roi(int out_dtype, int n_img, int h, int w, int k, const argus_frame_src* src, const float* rois,
                         const void* w_fwd, const float* scale, const float* shift, void* out, argus_stream_t stream);

/* g0[n][j] = gelu(b_fc[j] + sum_c w_fc[j][c] * mean_p x[n][p][c]): avgpool + resnet.fc + the nn.GELU() of
 * argus/models.py:85-88 in one launch (replaces argus_avgpool_fwd + argus_gemm_f32 (+ its split reduce) +
 * argus_gelu_f32 of a frozen session). x (n, hw, c) of x_dtype (ARGUS_BF16 or ARGUS_F16; anything else
 * ARGUS_ERR_ARG, "dtype"), w_fc (rdim, c) / b_fc / g0 (n, rdim) fp32, fp32 arithmetic. n <= 16 (more:
 * ARGUS_ERR_ARG: this is the deployment path), c a multiple of 64. The reduction over c is split over
 * workgroups in slices of 64 channels, summed in slice order by the last to arrive: bit-reproducible. The
 * workspace (argus_pool_fc_gelu_workspace_bytes; 0 = not served) starts with 256 bytes of ticket words that
 * must be zero on entry and are zero again on return (zero the buffer once); one sized for the largest n
 * serves every smaller n. */
size_t argus_pool_fc_gelu_workspace_bytes(int n, int c, int rdim);
int argus_pool_fc_gelu(int x_dtype, int n, int hw, int c, const void* x, const float* w_fc, const float* b_fc, int rdim,
                       float* g0, void* workspace, size_t workspace_bytes, argus_stream_t stream);

/* The output MLP and the exponential in one launch: pred = output_mlp.4(gelu(output_mlp.2(gelu(output_mlp.0(g0)))))
 * (argus/models.py:58-64, 89-90; w0 (128, d), w2 (128, 128), w4 (6, 128), all fp32) and pose = se3.Exp(pred)
 * (get_pose, argus/utils.py:179-189): replaces three argus_gemm_f32 and argus_se3_exp. output_mlp.0's
 * reduction over d (a multiple of 64) is split over workgroups like argus_pool_fc_gelu's; the last arriver
 * finishes alone. pred (batch, 6); pose (batch, 7) [t, qx, qy, qz, qw], bit-identical to argus_se3_exp of that
 * pred (the same device function). batch <= 16 (more: ARGUS_ERR_ARG). Workspace as argus_pool_fc_gelu's. */
size_t argus_pose_tail_workspace_bytes(int batch, int d);
int argus_pose_tail(int batch, int d, const float* g0, const float* w0, const float* b0, const float* w2,
                    const float* b2, const float* w4, const float* b4, float* pred, float* pose, int canonical_w,
                    void* workspace, size_t workspace_bytes, argus_stream_t stream);

/* Region-of-interest conditioning of the pose head (argus_roi_embed, argus_pose_tail_roi: added at ABI 21
 * without a version change: detect by symbol; csrc/head.hip). Image i = b * n_cams + c was resampled from the
 * region rois[i] = (y0, x0, eh, ew) of a frame_h x frame_w frame to the network's h x w; its features are
 *   rho[b][4c + 0] = (y0 + eh / 2 - frame_h / 2) / frame_h     rho[b][4c + 2] = ln(eh / h)
 *   rho[b][4c + 1] = (x0 + ew / 2 - frame_w / 2) / frame_w     rho[b][4c + 3] = ln(ew / w)
 * and output_mlp.0's pre-activation gains e[b][j] = sum_k w_r[j][k] * rho[b][k] (w_r (128, 4 n_cams) fp32, the
 * parameter roi_embed.weight): e is accumulated from 0 with fmaf over k = 0 .. 4 n_cams - 1 in ascending order,
 * fp32, logf for the logarithms. One device function states a feature and one states e for both entry points:
 * they produce the same bits from the same region. Inside the domain argus_stem_infer_roi serves the first two
 * features lie in [-1/2, 1/2] and the last two in [-ln 4, ln 4]. For ANY bits in rois the kernels only compute
 * numbers from them (nothing is indexed by a region's value): a non-finite region gives a non-finite result.
 * No atomics, bit-reproducible; nothing allocates or synchronises; capturable.
 *
 * argus_roi_embed (training and eval, any batch): z (batch, 128) holds output_mlp.0's acc + bias on entry
 * (argus_gemm_f32 epilogue 1) and z + e on return; g (batch, 128, may be NULL) receives gelu(z); rho (batch,
 * 4 n_cams, may be NULL) receives the features, the operand of the weight gradient dz^T rho. Refused before the
 * launch (ARGUS_ERR_ARG, the message names the argument): null rois, w_r or z; batch, n_cams, frame_h or frame_w
 * <= 0; h or w < 8; h > frame_h or w > frame_w; n_cams > 16.
 *
 * argus_pose_tail_roi: argus_pose_tail whose last arriver forms the pre-activation (slice sum + b0[j]) + e. The
 * features and w_r are staged before the ticket, so the last arriver waits for no further memory round trip. With
 * w_r = 0 pred and pose equal argus_pose_tail's bit for bit. Serves batch * n_cams <= 16 (more: ARGUS_ERR_ARG);
 * otherwise refuses what argus_pose_tail and argus_roi_embed refuse. Workspace: argus_pose_tail_workspace_bytes. */
int argus_roi_embed(int batch, int n_cams, int frame_h, int frame_w, int h, int w, const float* rois,
                    const float* w_r, float* z, float* g, float* rho, argus_stream_t stream);
int argus_pose_tail_roi(int batch, int d, const float* g0, const float* w0, const float* b0, const float* w2,
                        const float* b2, const float* w4, const float* b4, float* pred, float* pose, int canonical_w,
                        int n_cams, int frame_h, int frame_w, int h, int w, const float* rois, const float* w_r,
                        void* workspace, size_t workspace_bytes, argus_stream_t stream);

/* argus_roi_from_pose (added at ABI 21 without a version change: detect by symbol; csrc/track.hip): the region
 * of interest of every camera image around the cube a pose places in front of the cameras, in place on the
 * buffer argus_stem_infer_roi / argus_frames_resample / argus_batch_gather_resample read. Issued after
 * argus_pose_tail on its pose output it closes a tracker inside a captured graph: a replay ends by writing the
 * region the next replay reads. With index it aims a training batch's regions at the labelled cubes.
 * poses: device, [n_poses][7] = [t(3), qx, qy, qz, qw] (argus_se3_exp's layout); sample b reads pose b, or with
 * index (device, batch int64) pose clamp(index[b], 0, n_poses - 1). cameras: device, [n_cams][16] = [R row-major
 * (9), t (3), fx, fy, cx, cy]: a world point X has camera coordinates Y = R X + t (+x right, +y down, +z
 * forward) and pixel (u, v) = (fx Yx / Yz + cx, fy Yy / Yz + cy), v the row. cfg: HOST memory, read before the
 * launch. jitter: device, [batch * n_cams][3] = (ln s, dy, dx), or NULL. home, rois, used: device,
 * [batch * n_cams][4] = (y0, x0, height, width); valid: device, batch * n_cams int32. For image i = b * n_cams + c:
 *   1. invalid if a pose value is non-finite or n2 = |q|^2 is 0 or non-finite; else q <- q / sqrt(n2);
 *   2. the corners X_k = t + R(q) (+-half_extent), Y_k = R_c X_k + t_c; invalid if a Y_k is non-finite or
 *      Y_k.z < z_near;
 *   3. [v_min, v_max], [u_min, u_max] = the ranges of the eight pixels, (c_y, c_x) their midpoints, sigma = margin *
 *      max((v_max - v_min) / h, (u_max - u_min) / w); invalid if one of the three is non-finite;
 *   4. jitter: sigma <- sigma * exp(ln s), then c_y += dy * sigma * h, c_x += dx * sigma * w;
 *   5. smooth < 1: with p = rois[i] at the start of the launch, sigma_p = p.height / h, c_p = p.origin + p.extent / 2:
 *      sigma <- sigma_p + smooth * (sigma - sigma_p), c <- c_p + smooth * (c - c_p) (a non-finite jitter or p makes
 *      sigma or c non-finite: the image is invalid);
 *   6. sigma clamped to [max(scale_lo, 1/4), min(scale_hi, 4, frame_h / h, frame_w / w)] (the upper bound wins);
 *      per axis (frame S, output n) e = min(sigma * n, S) clamped to [n / 4, min(4 n, S)], o = clamp(c - e / 2, 0,
 *      S - e), one fp32 step down where o + e > S in double, then max(o, 0);
 *   7. an invalid image: rois[i] = home[i];
 *   8. valid[i] = 1 or 0, used[i] = rois[i] as it was when the launch started (either may be NULL).
 * fp32 arithmetic, contracted to fma (tests/track_reference.py is the fp64 statement); no atomics, bit-reproducible.
 * For ANY bit pattern of the poses a written region is home[i] or lies in the domain argus_stem_infer_roi serves
 * (finite, 0 <= o, o + e <= S, n / 4 <= e <= 4 n): the caller validates home, nobody has to validate the pose.
 * Refused before any launch (ARGUS_ERR_ARG, the message names the argument): a size <= 0, h or w < 8, h > frame_h
 * or w > frame_w; null poses / cameras / cfg / home / rois; n_poses < batch without an index; a non-finite or
 * non-positive half_extent, margin or z_near; scale_lo > scale_hi; smooth outside (0, 1]; cameras, home, rois or
 * used not 16-byte aligned. Allocates nothing; capturable. */
typedef struct argus_track_cfg {
  float half_extent[3];
  float margin;
  float scale_lo, scale_hi;
  float z_near;
  float smooth;
} argus_track_cfg;
int argus_roi_from_pose(int64_t batch, int n_cams, int frame_h, int frame_w, int h, int w, const float* poses,
                        int64_t n_poses, const int64_t* index, const float* cameras, const argus_track_cfg* cfg,
                        const float* jitter, const float* home, float* rois, float* used, int32_t* valid,
                        argus_stream_t stream);

/* ---- photometric training augmentations (argus/data.py:41-103; csrc/augment.hip) -------------
 * src: uint8 images (n_img, 3, H, W) planar (a B x 6 x H x W sample batch is 2B such images);
 * dst: fp32 (same shape) = augmented src / 255; params: n_img AugParams records of
 * argus_augment_params_bytes() bytes each (device memory; layout in augment.hip / augment.py);
 * scratch: argus_augment_scratch_bytes() bytes. Random erasing (two rectangles) -> Planckian gains
 * -> ColorJiggle (sampled op order) -> 5x5 Gaussian blur (reflect) -> 3x3 motion blur (zero border)
 * -> plasma shadow (diamond-square map) -> salt-and-pepper, per image. */
size_t argus_augment_params_bytes(void);
size_t argus_augment_scratch_bytes(int64_t n_img, int h, int w);
int argus_augment_photometric(int64_t n_img, int h, int w, const uint8_t* src, float* dst, const void* params,
                              float* scratch, argus_stream_t stream);

/* ---- device-resident dataset (ABI 21, added without a version change: detect by symbol;
 * csrc/resident.hip, argus_amd/resident.py) ---------------------------------------------------------
 * argus_batch_gather_occlude: one launch builds a batch from cropped uint8 frames kept in device memory: out[b] = store[index[b]]
 * with every pixel covered by one of its camera image's n_arcs occluder arcs set to 0 in all three
 * channels. store: (n_samples, 3*n_cams, h, w) planar uint8; index: batch int64 entries in device
 * memory - an entry outside [0, n_samples) is CLAMPED to that range (the launch cannot report it);
 * arcs: batch*n_cams*n_arcs records of argus_arc_record_bytes() bytes in device memory, image
 * (b, cam)'s records at (b*n_cams + cam)*n_arcs (n_arcs may be 0: arcs is then ignored); a record is
 * 12 int32 {x0, y0, x1, y1, width, mode, sx, sy, ex, ey, 0, 0}: the box of ImageDraw.arc in
 * SOURCE-frame pixels (the crop's origin there is crop_y0, crop_x0), mode 0 nothing / 1 full ellipse
 * / 2 span <= 180 degrees / 3 span > 180, (sx, sy) and (ex, ey) = round(2^20 (cos, sin)) of the start
 * and end angle (clockwise from 3 o'clock, y down). The covered set is the integer closed form stated
 * in resident.hip; every coordinate lies in [0, 8192) (a record outside covers nothing; a crop outside:
 * ARGUS_ERR_SHAPE). out: (batch, 3*n_cams, h, w), written once per byte (no atomics: deterministic,
 * independent of the arc order); must not overlap store. Allocates nothing; capturable. */
size_t argus_arc_record_bytes(void);
/* Host only: the np.random draws of the reference's draw_spaghetti (argus/utils.py:252-275) for n_arcs arcs
 * on a src_h x src_w frame, continued from a numpy RandomState's MT19937 state (mt_key: 624 words,
 * *mt_pos: its position; both updated, so the RandomState can go on from them). Per arc, in order:
 * randint(0, W), randint(0, H), randint(x0, W), randint(y0, H), randint(0, 360) twice,
 * int(uniform(width_lo, width_hi)). params: n_arcs x 7 int32 {x0, y0, x1, y1, a0, a1, width}. */
int argus_sample_arc_params(uint32_t* mt_key, int* mt_pos, int64_t n_arcs, int src_h, int src_w, double width_lo,
                            double width_hi, int32_t* params);
int argus_batch_gather_occlude(int64_t batch, int n_cams, int h, int w, const uint8_t* store, int64_t n_samples,
                               const int64_t* index, const void* arcs, int n_arcs, int crop_y0, int crop_x0,
                               uint8_t* out, argus_stream_t stream);
/* argus_batch_gather_resample (added at ABI 21 without a version change: detect by symbol): the training
 * counterpart of argus_frames_resample. One launch builds a batch from UNCROPPED uint8 frames kept in device
 * memory, each camera image through a region of interest of its own. store: (n_samples, 3*n_cams, src_h, src_w)
 * planar uint8; index: as argus_batch_gather_occlude's, clamped the same way; rois: device memory,
 * [batch*n_cams][4] fp32 = (y0, x0, height, width) in source pixels; arcs: argus_batch_gather_occlude's records
 * in source-frame pixels (n_arcs == 0 ignores arcs); out: (batch, 3*n_cams, h, w) uint8.
 * One output byte: the per-axis taps and weights are those of argus_frames_resample (the formula above it: at
 * most 9 taps, clamped into the frame for any bit pattern of the region); a source pixel covered by one of its
 * image's arcs has value 0 and keeps its weight (the arcs are drawn on the frame, then the frame is resampled);
 * px = sum_y wy * (sum_x wx * v / 255.0f) in fp32, the inner sum first, taps ascending, each step one fmaf from
 * 0; the byte is (uint8) rintf(255.0f * px) clamped to [0, 255]. At unit scale and an integer origin that is
 * argus_batch_gather_occlude on the cropped store, bit for bit. Each byte is written once, no atomics:
 * deterministic and independent of the arc order. The CALLER validates the regions (they live on the device):
 * finite, 0 <= o, o + e <= S, n / 4 <= e <= 4 n; for anything else the result is unspecified but every read
 * stays inside the frame. Refused before any launch: a null pointer (ARGUS_ERR_ARG), a non-positive size
 * (ARGUS_ERR_ARG), h or w < 8, src_h or src_w > 8192, h > src_h or w > src_w, one image's offsets not fitting
 * 31 bits (ARGUS_ERR_SHAPE), out overlapping store (ARGUS_ERR_ARG); the message names the argument. Allocates
 * nothing; capturable. */
int argus_batch_gather_resample(int64_t batch, int n_cams, int src_h, int src_w, int h, int w, const uint8_t* store,
                                int64_t n_samples, const int64_t* index, const float* rois, const void* arcs,
                                int n_arcs, uint8_t* out, argus_stream_t stream);

/* ---- optimizer step (clip_grad_norm_ + Adam, argus/train.py:232,317-320) --------------------- */
size_t argus_sumsq_workspace_bytes(int64_t count);
/* out[0] = sqrt(sum x^2) (fp32, deterministic two-level reduction). */
int argus_global_norm(int64_t count, const float* x, float* out, void* workspace,
                      argus_stream_t stream);
/* g' = grad_scale*g (e.g. 1/world after a SUM all-reduce); if norm != NULL (norm[0] = |g|),
 * g' *= min(1, max_norm/(grad_scale*norm[0]+1e-6)) (clip_grad_norm_); then Adam (torch
 * semantics, bias corrections bc1 = 1-beta1^t, bc2 = 1-beta2^t); writes param, m, v. */
int argus_adam_step(int64_t count, float* param, const float* grad, float* exp_avg,
                    float* exp_avg_sq, const float* norm, float grad_scale, float max_norm,
                    float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                    float bc2, argus_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARGUS_HIP_H */
