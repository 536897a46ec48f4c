// Internal (C++) launcher declarations shared by the .hip translation units and capi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/argus_hip.h"

namespace argus {

void set_error(const std::string& msg);
int check_launch(const char* what);
// ARGUS_F16 is served by the frozen-inference entry points alone (argus_hip.h lists them). Every other
// extern "C" entry that takes a dtype calls this first: true (and the "dtype" error set) for ARGUS_F16, so
// no launcher that picks `dtype == ARGUS_BF16 ? bf16 : float` ever sees 2-byte tensors as fp32.
bool f16_unserved(int dtype, const char* who);

int conv_fwd_bn_out(const argus_conv_desc& d, int dtype, const void* x, const void* w, const float* sc,
                    const float* sh, const void* res, const float* rsc, const float* rsh, void* out, uint8_t* bits,
                    void* y, hipStream_t st);
int conv_fwd(const argus_conv_desc& d, int dtype, const void* x, const void* w, void* y,
             const float* sc, const float* sh, float* stats, hipStream_t st, void* pro_out = nullptr,
             const argus_bn_fwd_fin* fin = nullptr);
// set by a forward launch that folded its statistics finalize (argus_conv_fwd_fin; conv.hip)
extern thread_local int g_ffin_folded;
int conv_fwd_stat_rows(const argus_conv_desc& d, int dtype);
int conv_fwd_x8(const argus_conv_desc& d, const void* x8, const void* w, void* y, float* stats, hipStream_t st);
int conv_dgrad_bn_x8(const argus_conv_desc& d, const void* dy8, const void* wt, void* dm, const argus_bn_bwd_epilogue* bn,
                     hipStream_t st);
int conv_x8_ok(const argus_conv_desc& d, int pass);
// BN workspace layout (bn.hip): [0, kBnCounterBytes) ticket counters, then double2 group results
constexpr size_t kBnCounterBytes = 16384;
int conv_fwd_stat_tile(const argus_conv_desc& d, int dtype);
// the partial-row layout of a statistics-only forward (argus_conv_fwd with y == NULL)
int conv_fwd_stats_only_rows(const argus_conv_desc& d, int dtype);
int conv_fwd_stats_only_tile(const argus_conv_desc& d, int dtype);

// Kernel-selection policy (argus_conv_policy_default): the immutable library table overlaid with one
// call's overrides (argus_conv_desc.tuning). Host-only; built per call, never stored.
enum TuneKey : int {
  kForceBm = 0,         // 0..2: row tile of pass fwd / dgrad / wgrad (0 = heuristic)
  kForceBn = 3,         // 3..5: column tile
  kWgradTarget = 6,     // weight-gradient split target (workgroups)
  kSmallKMax = 7,       // largest K on the single-buffer OCC 3/4 igemm
  kGldsMinK = 8,        // smallest K on the glds forward / dgrad (0 = off)
  kGldsMinGrid = 9,     // fewest workgroups for the glds kernel
  kHaloEnable = 10,     // 3x3 stride-1 forward / dgrad on the LDS-halo kernel
  kWgHaloEnable = 11,   // 3x3 stride-1 weight gradient on the LDS-halo kernel
  kWgHaloTarget = 12,   // ... its split target
  kHaloMinGrid = 13,    // fewest workgroups for the forward / dgrad halo kernel
  kWgHaloMaxTiles = 14, // most 64 x 64 channel tiles for the halo weight gradient
  kStemLdsFwd = 19,     // bf16 stem forward on the LDS-patch kernel
  kWgradTarget3x3 = 27, // split target of the register-staged 3x3 weight gradient (Cout > 64)
  kStemLdsWgrad = 34,   // bf16 stem weight gradient on the LDS-patch kernel
  kFwdBm128Rows = 35,   // fewest forward GEMM rows for 128-row tiles
  kGldsMinRows = 36,    // fewest GEMM rows (largest phase) for the glds kernel
  kFp8Passes = 37,      // ARGUS_FP8: which passes take MX-fp8 operands (1 fwd | 2 3x3 dgrad | 4 1x1 dgrad | 8 3x3 s1 fwd)
  kDgradApStaged = 38,  // 1x1 dgrad with an apply prologue: register-staged (1) or apply kernel + glds (0)
  kGldsDgrad = 39,      // data gradients may run on the glds kernel (forwards: key 8 alone)
  kHaloDgrad = 40,      // 3x3 data gradients may run on the LDS-halo kernel (forwards: key 10 alone)
  kGldsDgradStages = 41,  // LDS ring depth of the glds data gradients (3, or 2: 96 KB)
  kBwdSmallKOcc = 42,     // workgroups per CU the small-K BN-epilogue / apply-prologue dgrads are built for (4 or 3)
  kP1x1Dgrad = 43,        // the persistent 1x1 dgrad (apply prologue + mask-bits BN epilogue) for conv1 (1 on)
  kP1x1FwdStats = 44,     // statistics-only 1x1 forwards on the persistent kernel (conv_p1x1.hip; 1 on)
  kWgradDma = 45,         // 1x1 bf16 weight gradients on the LDS-DMA ring kernel (conv_wgdma.hip)
  kWgradSmallP = 46,      // 1x1 weight gradients over at most this many pixels: half the split target
  kWgradDmaGather = 47,   // ... and the stride-2 (1x1 / 3x3) plain ones, x rows gathered (1 on, >1 pixel cap)
  kWgradDmaStages = 48,   // LDS ring stages of the 128 x 256 apply DMA weight gradient (2..5)
  kDgradApMaxCols = 49,   // 1x1 dgrads stage the apply prologue up to this many 128-column tiles (0: any)
  kHaloDeepRing = 51,     // 3x3 halo fwd / dgrad (128 columns, <= 384 halo positions): four weight stages (1 on)
  kF32Split = 53,         // ARGUS_F32: passes on the bf16x3 split arithmetic (1 fwd | 2 dgrad | 4 wgrad); 52 is no key
  kNumTuneKeys = 54
};
struct Policy {
  int v[kNumTuneKeys];
  int operator[](int key) const { return v[key]; }
};
int policy_default(int key);  // -1: not a key
// The policy of one call: the defaults + d.tuning (the keys were validated by the conv entry point).
Policy policy_of(const argus_conv_desc& d);
// ARGUS_OK, or ARGUS_ERR_ARG (+ set_error) when d.tuning holds an unknown key or n_tuning < 0.
int check_tuning(const argus_conv_desc& d);
int conv_launch_info(const argus_conv_desc& d, int dtype, int pass, int64_t* flops);
size_t conv_weight_prep_table_bytes(int count);
int conv_weight_prep_table(int count, const argus_conv_desc* descs, const float* const* w, const int64_t* strides,
                           void* const* wf, void* const* wd, void* host_table, size_t bytes, int* nblocks);
int conv_weight_prep_batch(int dtype, int count, const void* device_table, int nblocks, hipStream_t st);
int conv_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* wt, void* dx,
               const void* addend, const uint8_t* addend_mask, hipStream_t st);
int conv_dgrad_bn_rows(const argus_conv_desc& d, int dtype);
int conv_check_desc(const argus_conv_desc& d);  // conv.hip's descriptor validation (ARGUS_OK or an error)
// fused 1x1 data + weight gradient (conv_dgw.hip)
bool conv_dgw_ok(const argus_conv_desc& d, int dtype);
size_t conv_dgw_ws_bytes(const argus_conv_desc& d, int dtype);
int conv_dgw_rows(const argus_conv_desc& d, int dtype);
int conv_dgw(const argus_conv_desc& d, int dtype, const void* dm, const void* wd, const void* x, void* dx,
             const void* addend, const argus_bn_bwd_epilogue* bn, const argus_bn_bwd_prologue* pro, float* dw,
             void* ws, size_t ws_bytes, hipStream_t st);
int conv_dgrad_stages_prologue(const argus_conv_desc& d, int dtype);
int conv_dgrad_bn(const argus_conv_desc& d, int dtype, const void* dy, const void* wt, void* dm,
                  const void* addend, const argus_bn_bwd_epilogue* bn, const argus_bn_bwd_prologue* pro,
                  hipStream_t st);
size_t conv_wgrad_ws(const argus_conv_desc& d, int dtype);
int conv_wgrad_apply(const argus_conv_desc& d, int dtype, const void* x, const void* dm,
                     const argus_bn_bwd_prologue& ap, float* dw, void* ws, size_t ws_bytes, hipStream_t st);
// the stem's data gradient (stem_dgrad.hip): dx (n, 3, h, w) fp32 planar from dy, or from dm through `ap`
int conv_stem_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* w_fwd,
                    const argus_bn_bwd_prologue* ap, float* dx, hipStream_t st);
int conv_wgrad(const argus_conv_desc& d, int dtype, const void* x, const float* sc,
               const float* sh, const void* dy, float* dw, void* ws, size_t ws_bytes,
               hipStream_t st);
int conv_weight_prep(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides,
                     void* wf, void* wd, hipStream_t st);
// frozen inference (conv_infer.hip): both BN folds, split choice / bound / workspace, forward
int conv_fold_bn(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                 const float* beta, const float* rm, const float* rv, float eps, void* wf, float* bias,
                 hipStream_t st);
int conv_fold_bn_dgrad(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                       const float* beta, const float* rm, const float* rv, float eps, void* wfd, hipStream_t st);
// One entry of the table behind argus_conv_fold_bn_batch (conv_infer.hip) and argus_conv_fold_bn_bwd_batch
// (conv_infer_wgrad.hip): a conv's fold and its derivative, every pointer a device pointer. blk0 / row0: the first
// workgroup of this entry in the fold grid (64 x 64 tiles per tap) and in the backward grid (4 filter rows each).
struct FoldEntry {
  const float* w;
  long long sk, sc, sr, ss;
  const float *gamma, *beta, *rm, *rv;
  void* wf;
  float* bias;
  void* wfd;
  const float* dwf;
  float* dw;
  const float* db;
  float *dgamma, *dbeta;
  float eps;
  int K, R, S, C, blk0, row0, vec_w, pad[2];
};
static_assert(sizeof(FoldEntry) == ARGUS_CONV_FOLD_ENTRY_BYTES, "argus_hip.h: ARGUS_CONV_FOLD_ENTRY_BYTES");
int conv_fold_bn_table(int count, const argus_conv_fold_src* src, void* host_table, size_t bytes, int* nblocks_fold,
                       int* nblocks_bwd);
int conv_fold_bn_batch(int dtype, int count, const void* device_table, int nblocks, hipStream_t st);
int conv_fold_bn_bwd_batch(int count, const void* device_table, int nblocks, hipStream_t st);
// whether argus_conv_fold_bn_bwd reads this master with 16-byte loads (the row is OHWI-contiguous in memory)
bool fold_bwd_vec_w(const argus_conv_desc& d, const float* w, long long sk, long long sc, long long sr, long long ss);
int conv_infer_splits(const argus_conv_desc& d, int dtype);
int conv_infer_max_splits(const argus_conv_desc& d, int dtype);
size_t conv_infer_ws_bytes(const argus_conv_desc& d, int dtype, int splits);
int conv_infer(const argus_conv_desc& d, int dtype, const void* x, const void* w, const float* bias, const void* res,
               int relu, void* out, int splits, void* ws, size_t ws_bytes, hipStream_t st);
// what the frozen convs serve (ARGUS_OK, or an error with its message set; F16 only where serves_f16), and the
// forward's tiling of a served descriptor: rows per tile, output tiles, bytes of ticket words
int infer_check(const argus_conv_desc& d, int dtype, const char* who, bool serves_f16);
int infer_bm(const argus_conv_desc& d);
int infer_tiles(const argus_conv_desc& d);
size_t infer_ticket_bytes(const argus_conv_desc& d);
// frozen gradient (conv_infer_bwd.hip): the plan, the data gradient
int conv_infer_dgrad_plan(const argus_conv_desc& d, int dtype, int splits_in, int* splits, int* max_splits,
                          size_t* ws_bytes);
int conv_infer_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* wfd, const void* addend,
                     const void* mask_src, void* dx, int splits, void* ws, size_t ws_bytes, hipStream_t st);
int images_to_nhwc4(int dtype, int64_t nimg, int h, int w, const float* x, void* out,
                    hipStream_t st);
int images_u8_to_nhwc4(int dtype, int64_t nimg, int h, int w, const uint8_t* x, void* out,
                       hipStream_t st);

}  // namespace argus
