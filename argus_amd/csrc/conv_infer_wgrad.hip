// Frozen fine-tuning: what the parameter gradients of a BN-folded conv need beside argus_conv_wgrad
// (conv_infer_bwd.hip is the data gradient of the same network). With eval-mode BatchNorm folded,
//   y = conv(x, w_fold) + bias,  w_fold[k][j] = w[k][j] * scale[k],  bias[k] = beta[k] - mean[k] * scale[k],
//   scale[k] = gamma[k] * invstd[k],  invstd[k] = 1 / sqrt(var[k] + eps)     (bnfin.h bn_eval_coeff),
// and loss.backward() through nn.Conv2d + nn.BatchNorm2d.eval() of torchvision's Bottleneck.forward
// (argus/models.py:66-90 with the model in eval mode, argus/train.py:316) gives, from the masked output
// gradient dm of the conv,
//   dL/d w_fold = argus_conv_wgrad(x, dm)                      (an existing entry)
//   dL/d bias   = sum over pixels of dm                        (bias_grad_kernel)
//   dL/d w, dL/d gamma, dL/d beta by the chain rule through the fold   (fold_bn_bwd_kernel).
// The bf16 rounding of the folded weight is treated as the identity (straight-through).
#include <algorithm>
#include <string>

#include "bnfin.h"
#include "internal.h"
#include "ktimer.h"

namespace argus {

// ---- bias gradient ------------------------------------------------------------------------------------
// db[k] = sum_p dm[p][k] over an NHWC [P][K] tensor. grid (K / 64 column blocks, splits): a workgroup sums the
// pixels [z * P / splits, (z + 1) * P / splits) of its 64 columns. Thread (row group pg, chunk ch) walks rows
// pg, pg + PG, ... of the slice with 16-byte loads, kBiasBatch in flight (clamped addresses, selects: common.h
// kLoadBatch).
// Accumulation (the rule of stats_finalize): a thread adds runs of at most kBiasRun = 64 rows in fp32; the runs,
// the row groups and the slices are added in fp64, each in a fixed order, and the result is rounded to fp32
// once. A run of n <= 64 terms adds at most (n - 1) * 2^-24 of the sum of its magnitudes and the final rounding
// 2^-24 of the result, so
//   |db[k] - sum_p dm[p][k]| <= 64 * 2^-24 * sum_p |dm[p][k]|   (3.9e-6: the fp64 part adds < 1e-12 of it),
// at any P, and the result is bitwise reproducible for a given `splits`.
// Split hand-off as infer_gemm.h: a slice stores its fp64 partial row, takes bnfin.h's ticket on its column
// block and the last arriver adds the slices in slice order 0..splits-1 and resets the ticket.
constexpr int kBiasCols = 64;    // columns per workgroup
constexpr int kBiasRun = 64;     // rows of one fp32 run
constexpr int kBiasBatch = 4;    // loads in flight
constexpr int kBiasMaxSplits = 64;
constexpr int kBiasCUs = 256;
constexpr int kBiasMinRows = 256;  // the library's own split leaves a slice at least this many pixels
constexpr size_t kBiasTicketBytes = 4096;  // argus_conv_infer_workspace_bytes' ticket region: slabs at 4096

template <typename T>
__global__ __launch_bounds__(256) void bias_grad_kernel(long long P, int K, const T* __restrict__ dm,
                                                        float* __restrict__ db, int splits, unsigned* tickets,
                                                        double* part) {
  constexpr int E = Chunk<T>::E, CH = kBiasCols / E, PG = 256 / CH;  // chunks per row, row groups
  __shared__ double red[PG][kBiasCols];
  __shared__ int flag;
  const int tid = threadIdx.x, cb = blockIdx.x, z = blockIdx.y;
  const int ch = tid % CH, pg = tid / CH;
  const long long p0 = z * P / splits, p1 = (z + 1) * P / splits;
  const T* col = dm + (size_t)cb * kBiasCols + ch * E;
  double acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.0;
  for (long long rb = p0 + pg; rb < p1; rb += (long long)PG * kBiasRun) {
    float s[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = 0.f;
    for (int i = 0; i < kBiasRun; i += kBiasBatch) {
      if (rb + (long long)i * PG >= p1) break;  // (uniform per thread: the rest of the run is empty)
      u32x4 v[kBiasBatch];
#pragma unroll
      for (int u = 0; u < kBiasBatch; ++u) {
        const long long p = rb + (long long)(i + u) * PG;
        v[u] = ld16(col + (size_t)(p < p1 ? p : p1 - 1) * K);
      }
#pragma unroll
      for (int u = 0; u < kBiasBatch; ++u) {
        const bool on = rb + (long long)(i + u) * PG < p1;
        float f[E];
        ChunkCvt<T>::unpack(v[u], f);
#pragma unroll
        for (int e = 0; e < E; ++e) s[e] += on ? f[e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += (double)s[e];
  }
#pragma unroll
  for (int e = 0; e < E; ++e) red[pg][ch * E + e] = acc[e];
  __syncthreads();
  double tot = 0.0;
  if (tid < kBiasCols) {
    for (int g = 0; g < PG; ++g) tot += red[g][tid];
    if (splits == 1) db[cb * kBiasCols + tid] = (float)tot;
    else part[(size_t)z * K + cb * kBiasCols + tid] = tot;
  }
  if (splits == 1) return;
  if (!fin_ticket<kPlainStores>(tickets + cb, (unsigned)splits, &flag)) return;
  if (tid < kBiasCols) {
    const double* mine = part + cb * kBiasCols + tid;
    double v = 0.0;
    for (int zb = 0; zb < splits; zb += kBiasBatch) {
      double t[kBiasBatch];
#pragma unroll
      for (int u = 0; u < kBiasBatch; ++u) t[u] = mine[(size_t)min(zb + u, splits - 1) * K];
#pragma unroll
      for (int u = 0; u < kBiasBatch; ++u) v += zb + u < splits ? t[u] : 0.0;
    }
    db[cb * kBiasCols + tid] = (float)v;
  }
}

static int bias_grad_max_splits(int64_t pixels) { return (int)std::min<int64_t>(pixels, kBiasMaxSplits); }

// powers of two while the grid leaves CUs idle and every slice keeps kBiasMinRows pixels
static int bias_grad_splits(int64_t pixels, int channels) {
  const int cbs = channels / kBiasCols;
  int s = 1;
  while (cbs * s < kBiasCUs && 2 * s <= kBiasMaxSplits && pixels / (2 * s) >= kBiasMinRows) s *= 2;
  return s;
}

static size_t bias_grad_ws_bytes(int channels, int splits) {
  return splits <= 1 ? 0 : kBiasTicketBytes + (size_t)splits * channels * sizeof(double);
}

static int bias_grad_plan(int dtype, int64_t pixels, int channels, int splits_in, int* splits, int* max_splits,
                          size_t* ws_bytes) {
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16) {
    set_error("bias_grad: dtype must be ARGUS_F32 or ARGUS_BF16 (no ARGUS_F16, ARGUS_FP8 gradients)");
    return ARGUS_ERR_ARG;
  }
  if (pixels <= 0 || channels <= 0) { set_error("bias_grad: bad sizes"); return ARGUS_ERR_ARG; }
  if (channels % kBiasCols) { set_error("bias_grad: channels must be a multiple of 64"); return ARGUS_ERR_SHAPE; }
  if ((size_t)(channels / kBiasCols) * sizeof(unsigned) > kBiasTicketBytes) {
    set_error("bias_grad: more than 65536 channels");
    return ARGUS_ERR_SHAPE;
  }
  const int mx = bias_grad_max_splits(pixels);
  if (splits_in < 0 || splits_in > mx) {
    set_error("bias_grad: splits " + std::to_string(splits_in) + " outside 0.." + std::to_string(mx) +
              " (argus_bias_grad_plan)");
    return ARGUS_ERR_ARG;
  }
  const int sp = splits_in ? splits_in : bias_grad_splits(pixels, channels);
  if (splits) *splits = sp;
  if (max_splits) *max_splits = mx;
  if (ws_bytes) *ws_bytes = bias_grad_ws_bytes(channels, sp);
  return ARGUS_OK;
}

// ---- the fold's derivative ----------------------------------------------------------------------------
// One wave per filter row k (4 rows per workgroup, K / 4 workgroups: 128 for a 512 x 4608 layer-4 conv2), no
// cross-workgroup reduction. Lane l takes the 16-byte chunks l, l + 64, ... of the row [R*S*C]:
//   dw[k][j]   = scale[k] * dwf[k][j]                              (stored as it goes; dw may be dwf)
//   dot        = sum_j dwf[k][j] * w[k][j]   per-lane partials in chunk order (row / 64 fused multiply-adds:
//                72 for the longest row, 4608), then wave_sum's fixed 6-level butterfly
//   dgamma[k]  = invstd[k] * (dot - mean[k] * db[k]),  dbeta[k] = db[k].
// At most 78 roundings deep, so |dgamma error| <= 78 * 2^-24 = 4.7e-6 of invstd * (sum_j |dwf * w| + |mean * db|).
// scale / invstd are bn_eval_coeff's expressions, so dw == dwf * scale of argus_bn_eval_coeffs bit for bit.
// w is read through its strides: 16-byte loads when the row is OHWI-contiguous in memory (NULL strides, and the
// channels-last OIHW view of such storage), four gathered elements per chunk otherwise; the same elements in
// the same order either way.
struct FoldBwdStrides { long long sk, sc, sr, ss; };
constexpr int kFoldBwdBatch = 4;

// filter row k of one conv, by one wave: the body of both kernels below
template <bool kVecW>
ARGUS_DEV void fold_bn_bwd_row(const float* __restrict__ w, FoldBwdStrides st, const float* __restrict__ gamma,
                               const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                               const float* dwf, const float* db, float* dw, float* dgamma, float* dbeta, int R, int S,
                               int C, int k) {
  const int lane = threadIdx.x & 63;
  const float inv = 1.f / sqrtf(rv[k] + eps);
  const float sc = gamma[k] * inv;
  const int J = R * S * C, nch = J / 4;
  const float* wk = w + (size_t)k * st.sk;
  const float* gk = dwf + (size_t)k * J;
  float* ok = dw + (size_t)k * J;
  float s = 0.f;
  for (int cb = lane; cb < nch; cb += 64 * kFoldBwdBatch) {
    f32x4 g[kFoldBwdBatch], wv[kFoldBwdBatch];
#pragma unroll
    for (int u = 0; u < kFoldBwdBatch; ++u) {
      const int j = 4 * min(cb + 64 * u, nch - 1);  // (clamped: masked below)
      g[u] = *reinterpret_cast<const f32x4*>(gk + j);
      if constexpr (kVecW) {
        wv[u] = *reinterpret_cast<const f32x4*>(wk + j);
      } else {
        const int rs = j / C, c = j - rs * C, r = rs / S, s0 = rs - r * S;  // C % 4 == 0: a chunk stays in its tap
        const float* p = wk + r * st.sr + s0 * st.ss + c * st.sc;
        wv[u] = f32x4{p[0], p[st.sc], p[2 * st.sc], p[3 * st.sc]};
      }
    }
#pragma unroll
    for (int u = 0; u < kFoldBwdBatch; ++u) {
      const int c4 = cb + 64 * u;
      const bool on = c4 < nch;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = on ? fmaf(g[u][e], wv[u][e], s) : s;
      if (on) *reinterpret_cast<f32x4*>(ok + 4 * c4) = g[u] * sc;
    }
  }
  const float dot = wave_sum(s);
  if (lane == 0) {
    const float b = db[k];
    dgamma[k] = inv * (dot - rm[k] * b);
    dbeta[k] = b;
  }
}

template <bool kVecW>
__global__ __launch_bounds__(256) void fold_bn_bwd_kernel(const float* __restrict__ w, FoldBwdStrides st,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ rm, const float* __restrict__ rv,
                                                          float eps, const float* dwf, const float* db, float* dw,
                                                          float* dgamma, float* dbeta, int R, int S, int C) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);  // (K % 64 == 0: whole waves)
  fold_bn_bwd_row<kVecW>(w, st, gamma, rm, rv, eps, dwf, db, dw, dgamma, dbeta, R, S, C, k);
}

// argus_conv_fold_bn_bwd_batch: the same rows for every entry of a table in one launch. A workgroup (4 rows)
// finds its entry by search over the entries' first workgroup (weight_prep_batch_kernel's search); vec_w is the
// host's choice of fold_bn_bwd_kernel<true / false> for that master. An entry whose db is another entry's dbeta
// slot (a downsample under conv3) reads a word its owner rewrites with the value it already holds.
__global__ __launch_bounds__(256) void fold_bn_bwd_kernel_batch(const FoldEntry* __restrict__ tab, int count) {
  int lo = 0, hi = count - 1;
  const int b = blockIdx.x;
  while (lo < hi) {  // last entry with row0 <= b
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].row0 <= b) lo = mid; else hi = mid - 1;
  }
  const FoldEntry e = tab[lo];
  const int k = (b - e.row0) * 4 + (threadIdx.x >> 6);
  const FoldBwdStrides st{e.sk, e.sc, e.sr, e.ss};
  if (e.vec_w)
    fold_bn_bwd_row<true>(e.w, st, e.gamma, e.rm, e.rv, e.eps, e.dwf, e.db, e.dw, e.dgamma, e.dbeta, e.R, e.S, e.C, k);
  else
    fold_bn_bwd_row<false>(e.w, st, e.gamma, e.rm, e.rv, e.eps, e.dwf, e.db, e.dw, e.dgamma, e.dbeta, e.R, e.S, e.C,
                           k);
}

bool fold_bwd_vec_w(const argus_conv_desc& d, const float* w, long long sk, long long sc, long long sr,
                    long long ss) {
  return sc == 1 && ss == d.c && sr == (long long)d.s * d.c && sk % 4 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
}

static int fold_bn_bwd(const argus_conv_desc& d, const float* w, const int64_t* strides, const float* gamma,
                       const float* rm, const float* rv, float eps, const float* dwf, const float* db, float* dw,
                       float* dgamma, float* dbeta, hipStream_t st) {
  if (int e = infer_check(d, ARGUS_F32, "conv_fold_bn_bwd", false)) return e;
  FoldBwdStrides fs;
  if (strides) fs = {strides[0], strides[1], strides[2], strides[3]};
  else fs = {(long long)d.r * d.s * d.c, 1, (long long)d.s * d.c, d.c};  // OHWI contiguous
  const bool vec = fold_bwd_vec_w(d, w, fs.sk, fs.sc, fs.sr, fs.ss);
  if ((reinterpret_cast<uintptr_t>(dwf) | reinterpret_cast<uintptr_t>(dw)) & 15) {
    set_error("conv_fold_bn_bwd: dwf and dw must be 16-byte aligned");
    return ARGUS_ERR_ARG;
  }
  const double el = (double)d.k * d.r * d.s * d.c;
  g_launch_work = 3.0 * el;
  g_launch_bytes = 12.0 * el + 28.0 * d.k;
  const dim3 grid(d.k / 4);
  if (vec)
    timed_launch("argus::fold_bn_bwd_kernel<true>", fold_bn_bwd_kernel<true>, grid, dim3(256), st, w, fs, gamma, rm,
                 rv, eps, dwf, db, dw, dgamma, dbeta, d.r, d.s, d.c);
  else
    timed_launch("argus::fold_bn_bwd_kernel<false>", fold_bn_bwd_kernel<false>, grid, dim3(256), st, w, fs, gamma, rm,
                 rv, eps, dwf, db, dw, dgamma, dbeta, d.r, d.s, d.c);
  return check_launch("fold_bn_bwd_kernel");
}

int conv_fold_bn_bwd_batch(int count, const void* device_table, int nblocks, hipStream_t st) {
  if (!device_table) { set_error("conv_fold_bn_bwd_batch: null argument"); return ARGUS_ERR_ARG; }
  if (count <= 0 || nblocks <= 0) {
    set_error("conv_fold_bn_bwd_batch: count and nblocks must be positive (argus_conv_fold_bn_table; a table "
              "without the backward operands has no backward grid)");
    return ARGUS_ERR_ARG;
  }
  g_launch_work = g_launch_bytes = 0.0;  // (the shapes live in the device table)
  timed_launch("argus::fold_bn_bwd_kernel_batch", fold_bn_bwd_kernel_batch, dim3(nblocks), dim3(256), st,
               reinterpret_cast<const FoldEntry*>(device_table), count);
  return check_launch("fold_bn_bwd_kernel_batch");
}

}  // namespace argus

using namespace argus;

extern "C" int argus_bias_grad_plan(int dtype, int64_t pixels, int channels, int splits_in, int* splits,
                                    int* max_splits, size_t* workspace_bytes) {
  if (!splits || !max_splits || !workspace_bytes) {
    set_error("bias_grad_plan: null argument");
    return ARGUS_ERR_ARG;
  }
  return bias_grad_plan(dtype, pixels, channels, splits_in, splits, max_splits, workspace_bytes);
}

extern "C" int argus_bias_grad(int dtype, int64_t pixels, int channels, const void* dm, float* db, int splits,
                               void* workspace, size_t workspace_bytes, argus_stream_t stream) {
  size_t need = 0;
  int mx = 0;
  if (int e = bias_grad_plan(dtype, pixels, channels, splits, &splits, &mx, &need)) return e;
  if (!dm || !db) { set_error("bias_grad: null argument"); return ARGUS_ERR_ARG; }
  if (reinterpret_cast<uintptr_t>(dm) & 15) { set_error("bias_grad: dm must be 16-byte aligned"); return ARGUS_ERR_ARG; }
  if (splits > 1 && (!workspace || workspace_bytes < need)) {
    set_error("bias_grad: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) +
              " needed for " + std::to_string(splits) + " splits (argus_bias_grad_plan)");
    return ARGUS_ERR_ARG;
  }
  if (splits > 1 && (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    set_error("bias_grad: workspace must be 16-byte aligned");
    return ARGUS_ERR_ARG;
  }
  unsigned* tk = splits > 1 ? reinterpret_cast<unsigned*>(workspace) : nullptr;
  double* part = splits > 1 ? reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + kBiasTicketBytes) : nullptr;
  const dim3 grid(channels / kBiasCols, splits);
  hipStream_t st = (hipStream_t)stream;
  g_launch_work = (double)pixels * channels;
  g_launch_bytes = (dtype == ARGUS_BF16 ? 2.0 : 4.0) * (double)pixels * channels + 4.0 * channels;
  if (dtype == ARGUS_BF16)
    timed_launch("argus::bias_grad_kernel<__bf16>", bias_grad_kernel<bf16>, grid, dim3(256), st, (long long)pixels,
                 channels, (const bf16*)dm, db, splits, tk, part);
  else
    timed_launch("argus::bias_grad_kernel<float>", bias_grad_kernel<float>, grid, dim3(256), st, (long long)pixels,
                 channels, (const float*)dm, db, splits, tk, part);
  return check_launch("bias_grad_kernel");
}

extern "C" int argus_conv_fold_bn_bwd(const argus_conv_desc* d, const float* w_master, const int64_t* strides,
                                      const float* gamma, const float* running_mean, const float* running_var,
                                      float eps, const float* dwf, const float* db, float* dw, float* dgamma,
                                      float* dbeta, argus_stream_t stream) {
  if (!d || !w_master || !gamma || !running_mean || !running_var || !dwf || !db || !dw || !dgamma || !dbeta) {
    set_error("conv_fold_bn_bwd: null argument");
    return ARGUS_ERR_ARG;
  }
  return fold_bn_bwd(*d, w_master, strides, gamma, running_mean, running_var, eps, dwf, db, dw, dgamma, dbeta,
                     (hipStream_t)stream);
}

extern "C" int argus_conv_fold_bn_bwd_batch(int count, const void* device_table, int nblocks, argus_stream_t stream) {
  return conv_fold_bn_bwd_batch(count, device_table, nblocks, (hipStream_t)stream);
}
