// extern "C" surface of libargus_hip.so (include/argus_hip.h) + error reporting.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "internal.h"

namespace argus {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

bool f16_unserved(int dtype, const char* who) {
  if (dtype != ARGUS_F16) return false;
  set_error(std::string(who) + ": dtype ARGUS_F16 is served by the frozen-inference entry points only");
  return true;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return ARGUS_ERR_HIP;
  }
  return ARGUS_OK;
}

}  // namespace argus

using namespace argus;

extern "C" {

int argus_abi_version(void) { return 21; }

const char* argus_last_error(void) { return g_last_error.c_str(); }

int argus_images_to_nhwc4(int dtype, int64_t nimg, int h, int w, const float* x, void* out, argus_stream_t stream) {
  if (nimg <= 0 || h <= 0 || w <= 0 || !x || !out) { set_error("images_to_nhwc4: bad arguments"); return ARGUS_ERR_ARG; }
  return images_to_nhwc4(dtype, nimg, h, w, x, out, (hipStream_t)stream);
}

int argus_images_u8_to_nhwc4(int dtype, int64_t nimg, int h, int w, const uint8_t* x, void* out,
                             argus_stream_t stream) {
  if (nimg <= 0 || h <= 0 || w <= 0 || !x || !out) { set_error("images_u8_to_nhwc4: bad arguments"); return ARGUS_ERR_ARG; }
  return images_u8_to_nhwc4(dtype, nimg, h, w, x, out, (hipStream_t)stream);
}

int argus_conv_weight_prep(const argus_conv_desc* d, int dtype, const float* w, const int64_t* strides, void* wf,
                           void* wd, argus_stream_t stream) {
  if (d && !d->stem && f16_unserved(dtype, "conv_weight_prep (not a stem descriptor)")) return ARGUS_ERR_ARG;
  if (!d || !w) { set_error("conv_weight_prep: null argument"); return ARGUS_ERR_ARG; }
  return conv_weight_prep(*d, dtype, w, strides, wf, wd, (hipStream_t)stream);
}

size_t argus_conv_weight_prep_table_bytes(int count) { return conv_weight_prep_table_bytes(count); }

int argus_conv_weight_prep_table(int count, const argus_conv_desc* descs, const float* const* w_master,
                                 const int64_t* strides, void* const* w_fwd, void* const* w_dgrad, void* host_table,
                                 size_t table_bytes, int* nblocks) {
  return conv_weight_prep_table(count, descs, w_master, strides, w_fwd, w_dgrad, host_table, table_bytes, nblocks);
}

int argus_conv_weight_prep_batch(int dtype, int count, const void* device_table, int nblocks, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_weight_prep_batch")) return ARGUS_ERR_ARG;
  return conv_weight_prep_batch(dtype, count, device_table, nblocks, (hipStream_t)stream);
}

int argus_conv_fwd(const argus_conv_desc* d, int dtype, const void* x, const void* w, void* y, const float* sc,
                   const float* sh, float* stats, argus_stream_t stream) {
  if (d && (!d->stem || sc || sh || stats) && f16_unserved(dtype, "conv_fwd (not a plain stem forward)")) return ARGUS_ERR_ARG;
  if (!d || !x || !w || (!y && !stats) || (sc == nullptr) != (sh == nullptr)) {
    set_error("conv_fwd: bad arguments");
    return ARGUS_ERR_ARG;
  }
  return conv_fwd(*d, dtype, x, w, y, sc, sh, stats, (hipStream_t)stream);
}

int argus_conv_fwd_fin(const argus_conv_desc* d, int dtype, const void* x, const void* w, void* y, const float* sc,
                       const float* sh, float* stats, const argus_bn_fwd_fin* fin, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_fwd_fin")) return ARGUS_ERR_ARG;
  if (!d || !x || !w || !stats || !fin || !fin->workspace || !fin->gamma || !fin->beta ||
      (sc == nullptr) != (sh == nullptr)) {
    set_error("conv_fwd_fin: bad arguments");
    return ARGUS_ERR_ARG;
  }
  if (int e = conv_fwd(*d, dtype, x, w, y, sc, sh, stats, (hipStream_t)stream, nullptr, fin)) return e;
  if (g_ffin_folded) return ARGUS_OK;
  // not folded (the producer's tiles do not align with the merge groups): the separate finalize
  const bool so = y == nullptr && sc == nullptr;
  const int rows = so ? conv_fwd_stats_only_rows(*d, dtype) : conv_fwd_stat_rows(*d, dtype);
  const int tile = so ? conv_fwd_stats_only_tile(*d, dtype) : conv_fwd_stat_tile(*d, dtype == ARGUS_FP8 ? ARGUS_BF16 : dtype);
  return argus_bn_finalize(d->k, rows, tile, stats, (int64_t)d->n * d->ho * d->wo, fin->gamma, fin->beta, fin->eps,
                           fin->momentum, fin->running_mean, fin->running_var, fin->num_batches_tracked, fin->mean,
                           fin->invstd, fin->scale, fin->shift, fin->workspace, stream);
}

int argus_conv_fwd_apply_out(const argus_conv_desc* d, int dtype, const void* x, const void* w, void* y,
                             const float* sc, const float* sh, float* stats, void* x_out, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_fwd_apply_out")) return ARGUS_ERR_ARG;
  if (!d || !x || !w || (!y && !stats) || !sc || !sh || !x_out) {
    set_error("conv_fwd_apply_out: bad arguments");
    return ARGUS_ERR_ARG;
  }
  return conv_fwd(*d, dtype, x, w, y, sc, sh, stats, (hipStream_t)stream, x_out);
}

int argus_conv_fwd_bn_out(const argus_conv_desc* d, int dtype, const void* x, const void* w_fwd, const float* scale,
                          const float* shift, const void* res, const float* res_scale, const float* res_shift, void* out,
                          uint8_t* mask_bits, void* y, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_fwd_bn_out")) return ARGUS_ERR_ARG;
  if (!d) {
    set_error("conv_fwd_bn_out: bad arguments");
    return ARGUS_ERR_ARG;
  }
  return conv_fwd_bn_out(*d, dtype, x, w_fwd, scale, shift, res, res_scale, res_shift, out, mask_bits, y,
                         (hipStream_t)stream);
}
int argus_conv_fwd_stat_rows(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_fwd_stat_rows")) return 0;
  return d ? conv_fwd_stat_rows(*d, dtype) : 0;
}
int argus_conv_fwd_stats_only_rows(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_fwd_stats_only_rows")) return 0;
  return d ? conv_fwd_stats_only_rows(*d, dtype) : 0;
}
int argus_conv_fwd_stats_only_tile(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_fwd_stats_only_tile")) return 0;
  return d ? conv_fwd_stats_only_tile(*d, dtype) : 0;
}
size_t argus_conv_fwd_stat_part_bytes(const argus_conv_desc* d, int dtype, int stats_only) {
  if (f16_unserved(dtype, "conv_fwd_stat_part_bytes")) return 0;
  if (!d || conv_check_desc(*d)) return 0;
  const int rows = stats_only ? conv_fwd_stats_only_rows(*d, dtype) : conv_fwd_stat_rows(*d, dtype);
  const int tile = stats_only ? conv_fwd_stats_only_tile(*d, dtype) : conv_fwd_stat_tile(*d, dtype);
  if (rows <= 0) return 0;
  // float2 {sum, M2} [rows][k], then int32 pixel counts [rows] when the tiling is ragged (tile < 0)
  return (size_t)rows * d->k * 2 * sizeof(float) + (tile < 0 ? (size_t)rows * sizeof(int32_t) : 0);
}

int argus_conv_fold_bn(const argus_conv_desc* d, int dtype, const float* w_master, const int64_t* strides,
                       const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, void* w_fold, float* bias, argus_stream_t stream) {
  if (!d || !w_master || !gamma || !beta || !running_mean || !running_var || !w_fold || !bias) {
    set_error("conv_fold_bn: null argument");
    return ARGUS_ERR_ARG;
  }
  return conv_fold_bn(*d, dtype, w_master, strides, gamma, beta, running_mean, running_var, eps, w_fold, bias,
                      (hipStream_t)stream);
}

int argus_conv_fold_bn_table(int count, const argus_conv_fold_src* src, void* host_table, size_t table_bytes,
                             int* nblocks_fold, int* nblocks_bwd) {
  return conv_fold_bn_table(count, src, host_table, table_bytes, nblocks_fold, nblocks_bwd);
}

int argus_conv_fold_bn_batch(int dtype, int count, const void* device_table, int nblocks, argus_stream_t stream) {
  return conv_fold_bn_batch(dtype, count, device_table, nblocks, (hipStream_t)stream);
}

int argus_conv_infer_splits(const argus_conv_desc* d, int dtype) { return d ? conv_infer_splits(*d, dtype) : 0; }
int argus_conv_infer_max_splits(const argus_conv_desc* d, int dtype) {
  return d ? conv_infer_max_splits(*d, dtype) : 0;
}
size_t argus_conv_infer_workspace_bytes(const argus_conv_desc* d, int dtype, int splits) {
  return d ? conv_infer_ws_bytes(*d, dtype, splits) : 0;
}

int argus_conv_infer(const argus_conv_desc* d, int dtype, const void* x, const void* w_fold, const float* bias,
                     const void* res, int relu, void* out, int splits, void* workspace, size_t workspace_bytes,
                     argus_stream_t stream) {
  if (!d || !x || !w_fold || !bias || !out) { set_error("conv_infer: null argument"); return ARGUS_ERR_ARG; }
  return conv_infer(*d, dtype, x, w_fold, bias, res, relu, out, splits, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int argus_conv_fold_bn_dgrad(const argus_conv_desc* d, int dtype, const float* w_master, const int64_t* strides,
                             const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, void* w_fold_dgrad, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_fold_bn_dgrad")) return ARGUS_ERR_ARG;
  if (!d || !w_master || !gamma || !beta || !running_mean || !running_var || !w_fold_dgrad) {
    set_error("conv_fold_bn_dgrad: null argument");
    return ARGUS_ERR_ARG;
  }
  return conv_fold_bn_dgrad(*d, dtype, w_master, strides, gamma, beta, running_mean, running_var, eps, w_fold_dgrad,
                            (hipStream_t)stream);
}

int argus_conv_infer_dgrad_plan(const argus_conv_desc* d, int dtype, int splits_in, int* splits, int* max_splits,
                                size_t* workspace_bytes) {
  if (f16_unserved(dtype, "conv_infer_dgrad_plan")) return ARGUS_ERR_ARG;
  if (!d || !splits || !max_splits || !workspace_bytes) {
    set_error("conv_infer_dgrad_plan: null argument");
    return ARGUS_ERR_ARG;
  }
  return conv_infer_dgrad_plan(*d, dtype, splits_in, splits, max_splits, workspace_bytes);
}

int argus_conv_infer_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* w_fold_dgrad,
                           const void* addend, const void* mask_src, void* dx, int splits, void* workspace,
                           size_t workspace_bytes, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_infer_dgrad")) return ARGUS_ERR_ARG;
  if (!d || !dy || !w_fold_dgrad || !dx) { set_error("conv_infer_dgrad: null argument"); return ARGUS_ERR_ARG; }
  return conv_infer_dgrad(*d, dtype, dy, w_fold_dgrad, addend, mask_src, dx, splits, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

int argus_conv_policy_default(int key) { return policy_default(key); }

int argus_conv_launch_info(const argus_conv_desc* d, int dtype, int pass, int64_t* flops) {
  if (f16_unserved(dtype, "conv_launch_info")) return -1;
  return d ? conv_launch_info(*d, dtype, pass, flops) : -1;
}

int argus_conv_fwd_stat_tile(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_fwd_stat_tile")) return 0;
  return d ? conv_fwd_stat_tile(*d, dtype) : 0;
}

int argus_conv_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* wt, void* dx, const void* addend,
                     const uint8_t* addend_mask,
                     argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_dgrad")) return ARGUS_ERR_ARG;
  if (!d || !dy || !wt || !dx) { set_error("conv_dgrad: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_dgrad(*d, dtype, dy, wt, dx, addend, addend_mask, (hipStream_t)stream);
}

int argus_conv_dgrad_bn_rows(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_dgrad_bn_rows")) return -1;
  return d ? conv_dgrad_bn_rows(*d, dtype) : -1;
}
int argus_conv_dgrad_stages_prologue(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_dgrad_stages_prologue")) return 0;
  return d ? conv_dgrad_stages_prologue(*d, dtype) : 0;
}

int argus_conv_dgrad_bn(const argus_conv_desc* d, int dtype, const void* dy, const void* wt, void* dm,
                        const void* addend, const argus_bn_bwd_epilogue* bn, const argus_bn_bwd_prologue* pro,
                        argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_dgrad_bn")) return ARGUS_ERR_ARG;
  if (!d || !dy || !wt || !dm) { set_error("conv_dgrad_bn: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_dgrad_bn(*d, dtype, dy, wt, dm, addend, bn, pro, (hipStream_t)stream);
}

int argus_conv_x8_ok(const argus_conv_desc* d, int pass) { return d ? conv_x8_ok(*d, pass) : 0; }

int argus_conv_fwd_x8(const argus_conv_desc* d, const void* x8, const void* w, void* y, float* stats,
                      argus_stream_t stream) {
  if (!d) { set_error("conv_fwd_x8: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_fwd_x8(*d, x8, w, y, stats, (hipStream_t)stream);
}

int argus_conv_dgrad_bn_x8(const argus_conv_desc* d, const void* dy8, const void* wt, void* dm,
                           const argus_bn_bwd_epilogue* bn, argus_stream_t stream) {
  if (!d || !dy8 || !wt || !dm) { set_error("conv_dgrad_bn_x8: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_dgrad_bn_x8(*d, dy8, wt, dm, bn, (hipStream_t)stream);
}

int argus_conv_wgrad_apply(const argus_conv_desc* d, int dtype, const void* x, const void* dm,
                           const argus_bn_bwd_prologue* ap, float* dw, void* ws, size_t ws_bytes, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_wgrad_apply")) return ARGUS_ERR_ARG;
  if (!d || !x || !dm || !ap || !dw || !ws) { set_error("conv_wgrad_apply: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_wgrad_apply(*d, dtype, x, dm, *ap, dw, ws, ws_bytes, (hipStream_t)stream);
}

int argus_conv_stem_dgrad(const argus_conv_desc* d, int dtype, const void* dy, const void* w_fwd,
                          const argus_bn_bwd_prologue* ap, float* dx_nchw, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_stem_dgrad")) return ARGUS_ERR_ARG;
  if (!d || !dy || !w_fwd || !dx_nchw) { set_error("conv_stem_dgrad: null argument"); return ARGUS_ERR_ARG; }
  return conv_stem_dgrad(*d, dtype, dy, w_fwd, ap, dx_nchw, (hipStream_t)stream);
}

int argus_conv_dgrad_wgrad_ok(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_dgrad_wgrad_ok")) return 0;
  return d && !conv_check_desc(*d) && conv_dgw_ok(*d, dtype) ? 1 : 0;
}

size_t argus_conv_dgrad_wgrad_workspace_bytes(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_dgrad_wgrad_workspace_bytes")) return 0;
  return d && !conv_check_desc(*d) ? conv_dgw_ws_bytes(*d, dtype) : 0;
}

int argus_conv_dgrad_wgrad_bn_rows(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_dgrad_wgrad_bn_rows")) return -1;
  return d && !conv_check_desc(*d) ? conv_dgw_rows(*d, dtype) : -1;
}

int argus_conv_dgrad_wgrad_bn(const argus_conv_desc* d, int dtype, const void* dm, const void* w_dgrad,
                              const void* x, void* dx, const void* addend, const argus_bn_bwd_epilogue* bn,
                              const argus_bn_bwd_prologue* pro, float* dw, void* workspace,
                              size_t workspace_bytes, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_dgrad_wgrad_bn")) return ARGUS_ERR_ARG;
  if (!d) { set_error("conv_dgrad_wgrad_bn: bad arguments"); return ARGUS_ERR_ARG; }
  return conv_dgw(*d, dtype, dm, w_dgrad, x, dx, addend, bn, pro, dw, workspace, workspace_bytes,
                  (hipStream_t)stream);
}

size_t argus_conv_wgrad_workspace_bytes(const argus_conv_desc* d, int dtype) {
  if (f16_unserved(dtype, "conv_wgrad_workspace_bytes")) return 0;
  return d ? conv_wgrad_ws(*d, dtype) : 0;
}

int argus_conv_wgrad(const argus_conv_desc* d, int dtype, const void* x, const float* sc, const float* sh,
                     const void* dy, float* dw, void* ws, size_t ws_bytes, argus_stream_t stream) {
  if (f16_unserved(dtype, "conv_wgrad")) return ARGUS_ERR_ARG;
  if (!d || !x || !dy || !dw || !ws || (sc == nullptr) != (sh == nullptr)) {
    set_error("conv_wgrad: bad arguments");
    return ARGUS_ERR_ARG;
  }
  return conv_wgrad(*d, dtype, x, sc, sh, dy, dw, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
