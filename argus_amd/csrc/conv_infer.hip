// Frozen-inference convolutions: eval-mode BatchNorm folded into the weights once (fold_bn), then one
// launch per conv with bias + residual + ReLU in its epilogue (conv_infer_kernel). Replaces
// nn.Conv2d + nn.BatchNorm2d.eval() [+ add] + nn.ReLU of torchvision's Bottleneck.forward
// (argus/models.py:43) for a deployed model, where M = images * Ho * Wo is a few hundred rows.
//
// The kernel is infer_gemm.h's tile GEMM (tiling, staging, split-K and its hand-off live there) with the
// forward's two policies: a GEMM row is an output pixel, and the epilogue is bias + residual + ReLU.
#include <algorithm>

#include "infer_gemm.h"

namespace argus {

constexpr int kInferMaxSplits = 16;   // slab budget: 16 slabs of <= 16 KB per tile
constexpr int kInferCUs = 256;

struct InferParams {
  InferGemm g;  // a = x, b = w_fold [K][R*S*C], out (M, K)
  const float* bias;
  const void* res;
  int H, W, C, Ho, Wo, stride, pad, S, relu;
  FastDiv fd_hw, fd_w, fd_c, fd_s;
};

// ---- fold ---------------------------------------------------------------------------------------------
// One product and one rounding, two layouts: v = T(w[k][c][r][s] * scale[k]) (one fp32 multiply, then round to
// nearest even; fp16 saturates to +-65504: from_f32<f16>), scale / shift = bn_eval_coeff (bnfin.h).
//   forward        w_fold[k][r][s][c] = v, bias[k] = shift[k]
//   data gradient  w_fold_dgrad[c][R-1-r][S-1-s][k] = v (the transposed filter, taps rotated by 180 degrees)
struct FoldStrides { long long sk, sc, sr, ss; };

template <typename T, bool kDgrad>
__global__ __launch_bounds__(256) void fold_bn_kernel(const float* __restrict__ w, FoldStrides st,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ rm, const float* __restrict__ rv,
                                                      float eps, T* __restrict__ wf, float* __restrict__ bias, int K,
                                                      int R, int S, int C) {
  const int inner = kDgrad ? K : C;  // the fastest index of the output, under its R*S taps
  const int row = R * S * inner;
  const int total = K * R * S * C;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int o = i / row, rem = i - o * row;
    const int rs = rem / inner, in = rem - rs * inner;
    const int r0 = rs / S, s0 = rs - r0 * S;  // the output's tap
    const int k = kDgrad ? in : o, c = kDgrad ? o : in;
    const int r = kDgrad ? R - 1 - r0 : r0, s = kDgrad ? S - 1 - s0 : s0;
    float sc, sh;
    bn_eval_coeff(gamma, beta, rm, rv, eps, k, sc, sh);
    wf[i] = from_f32<T>(w[k * st.sk + c * st.sc + r * st.sr + s * st.ss] * sc);
    if constexpr (!kDgrad)
      if (rem == 0) bias[k] = sh;
  }
}

// ---- table-driven fold --------------------------------------------------------------------------------
// Both layouts of every conv of a table in one launch (argus_conv_fold_bn_batch). A workgroup owns the 64(k) x
// 64(c) tile of one tap of one entry, found by search over the entries' first workgroup as in
// weight_prep_batch_kernel. Thread (row = tid / 4, cq = 16 * (tid % 4)) reads 16 consecutive channels of filter
// k0 + row through the master's strides (16-byte loads when the channels are contiguous), forms v exactly as
// fold_bn_kernel does and stores its piece of the forward row w_fold[k][r][s][c0 + cq ..]. The transposed copy
// goes through the LDS: the same thread then holds 16 consecutive filters of channel c0 + row and stores its
// piece of w_fold_dgrad[c][R-1-r][S-1-s][k0 + cq ..], so both copies leave in 16-byte stores, four lanes to a
// 256-byte (fp32) / 128-byte (bf16) row segment; fold_bn_kernel<T, true> gathers this copy with a stride of a
// whole filter row per element instead.
// LDS layout: the tile holds fp32 values (already rounded to T, so both copies pack the same bits), element
// (k, c) at k * 129 + 8 * (k / 16) + c + 8 * (c / 16). ds_write_b32 / ds_read_b32 bank 32-lane halves over 32
// dwords; a half is 8 rows x 4 quarters. Writing column 16 q + j of rows k..k+7 lands on bank k + 24 q + const,
// reading row 16 q + j at columns c..c+7 on bank c + 24 q + const (mod 32): {0, 24, 16, 8} + 0..7, all
// distinct, so neither side conflicts (a plain pitch of 65 puts quarters 0 and 2 on the same banks).
constexpr int kFoldPitch = 129;  // 1 mod 32, >= 64 + 2 * 24 columns of skew
ARGUS_DEV int fold_lds(int k, int c) { return k * kFoldPitch + 8 * (k >> 4) + c + 8 * (c >> 4); }

template <typename T>
__global__ __launch_bounds__(256) void fold_bn_kernel_batch(const FoldEntry* __restrict__ tab, int count) {
  int lo = 0, hi = count - 1;
  const int b = blockIdx.x;
  while (lo < hi) {  // last entry with blk0 <= b
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const FoldEntry e = tab[lo];
  const int local = b - e.blk0;
  const int RS = e.R * e.S, ct = e.C / 64;
  const int rs = local % RS, rem = local / RS;
  const int c0 = (rem % ct) * 64, k0 = (rem / ct) * 64;
  const int r = rs / e.S, s = rs - r * e.S;
  __shared__ float tile[64 * kFoldPitch];
  const int row = threadIdx.x >> 2, cq = (threadIdx.x & 3) * 16;
  constexpr int E = Chunk<T>::E;
  float sc, sh;
  bn_eval_coeff(e.gamma, e.beta, e.rm, e.rv, e.eps, k0 + row, sc, sh);
  const float* src = e.w + (long long)(k0 + row) * e.sk + r * e.sr + s * e.ss + (long long)(c0 + cq) * e.sc;
  float f[16];
  if (e.sc == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + j);
      f[j] = v.x; f[j + 1] = v.y; f[j + 2] = v.z; f[j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = src[j * e.sc];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) f[j] = to_f32(from_f32<T>(f[j] * sc));  // the one multiply and the one rounding
  T* dst = reinterpret_cast<T*>(e.wf) + ((size_t)(k0 + row) * RS + rs) * e.C + c0 + cq;
#pragma unroll
  for (int j = 0; j < 16; j += E) {
    float g[E];
#pragma unroll
    for (int u = 0; u < E; ++u) g[u] = f[j + u];
    st16(dst + j, ChunkCvt<T>::pack(g));
  }
  if (rs == 0 && c0 == 0 && cq == 0) e.bias[k0 + row] = sh;  // once per filter
  if (!e.wfd) return;  // (uniform: the whole entry has no second copy)
#pragma unroll
  for (int j = 0; j < 16; ++j) tile[fold_lds(row, cq + j)] = f[j];
  __syncthreads();
  float t[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = tile[fold_lds(cq + j, row)];  // row = channel, 16 consecutive filters
  T* dd = reinterpret_cast<T*>(e.wfd) + ((size_t)(c0 + row) * RS + (RS - 1 - rs)) * e.K + k0 + cq;
#pragma unroll
  for (int j = 0; j < 16; j += E) {
    float g[E];
#pragma unroll
    for (int u = 0; u < E; ++u) g[u] = t[j + u];
    st16(dd + j, ChunkCvt<T>::pack(g));
  }
}

// ---- forward ------------------------------------------------------------------------------------------
// a row = one output pixel (nimg, oh, ow); off: element offset of its window's (0, 0) tap before padding
template <int AR>
struct InferFwdA {
  int off[AR], ih[AR], iw[AR];
  struct Step { int dh, dw, ch, tap; };
  ARGUS_DEV void row(const InferParams& p, int i, int m) {
    const int nimg = fdiv(m, p.fd_hw), rem = m - nimg * (p.Ho * p.Wo);
    const int oh = fdiv(rem, p.fd_w), ow = rem - oh * p.Wo;
    ih[i] = oh * p.stride;
    iw[i] = ow * p.stride;
    off[i] = ((nimg * p.H + ih[i]) * p.W + iw[i]) * p.C;
  }
  ARGUS_DEV Step step(const InferParams& p, int k0, int ch0) const {
    const int t = fdiv(k0, p.fd_c), ci0 = k0 - t * p.C;
    const int r = fdiv(t, p.fd_s), s = t - r * p.S;
    Step st;
    st.dh = r - p.pad;
    st.dw = s - p.pad;
    st.ch = ci0 + ch0;
    st.tap = (st.dh * p.W + st.dw) * p.C + st.ch;
    return st;
  }
  ARGUS_DEV bool at(const InferParams& p, const Step& st, int i, int& o) const {
    const int h = ih[i] + st.dh, w = iw[i] + st.dw;
    o = off[i] + st.tap;
    return (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;  // rows outside the image read zero
  }
};

// out = [relu](acc + bias [+ res])
template <typename T, int NIT>
struct InferFwdEpi {
  static constexpr int E = Chunk<T>::E;
  float bv[E];
  u32x4 rv[NIT];
  ARGUS_DEV void init(const InferParams& p, int col) { BwdEpiAcc<T, 3>::ld(bv, p.bias + col); }
  ARGUS_DEV void prefetch(const InferParams& p, int it, size_t at) {
    if (p.res) rv[it] = ld16(reinterpret_cast<const T*>(p.res) + at);
  }
  ARGUS_DEV void apply(const InferParams& p, int it, float (&f)[E]) const {
#pragma unroll
    for (int j = 0; j < E; ++j) f[j] += bv[j];
    if (p.res) {
      float r[E];
      ChunkCvt<T>::unpack(rv[it], r);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] += r[j];
    }
    if (p.relu) {
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] = fmaxf(f[j], 0.f);
    }
  }
};

template <typename T, int BM>
__global__ __launch_bounds__(256, 2) void conv_infer_kernel(const InferParams p) {
  infer_gemm_tile<T, BM, InferFwdA, InferFwdEpi>(p);
}

struct InferFwdKernel {
  static constexpr const char* name = "conv_infer_kernel";
  template <typename T, int BM> static auto kernel() { return conv_infer_kernel<T, BM>; }
};

// ---- host ---------------------------------------------------------------------------------------------
static bool infer_16bit(int dtype) { return dtype == ARGUS_BF16 || dtype == ARGUS_F16; }

// the four non-stem conv kinds of ResNet-50 in F32 / BF16, and in F16 where `who` serves it (the forward, not
// the data gradient); sets the error message when not served
int infer_check(const argus_conv_desc& d, int dtype, const char* who, bool serves_f16) {
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16 && !(serves_f16 && dtype == ARGUS_F16)) {
    set_error(std::string(who) + (serves_f16 ? ": dtype must be ARGUS_F32, ARGUS_BF16 or ARGUS_F16"
                                             : ": dtype must be ARGUS_F32 or ARGUS_BF16 (no ARGUS_F16, ARGUS_FP8 "
                                               "gradients)"));
    return ARGUS_ERR_ARG;
  }
  if (int e = conv_check_desc(d)) return e;
  const bool k1 = d.r == 1 && d.s == 1 && d.pad == 0, k3 = d.r == 3 && d.s == 3 && d.pad == 1;
  if (d.stem || !(k1 || k3) || d.stride < 1 || d.stride > 2 || d.c % 64 || d.k % 64) {
    set_error(std::string(who) + ": serves 1x1 (pad 0) and 3x3 (pad 1) convs of stride 1 or 2 with c, k multiples "
                                 "of 64 (not the stem)");
    return ARGUS_ERR_SHAPE;
  }
  return ARGUS_OK;
}

static int infer_bke(int dtype) { return infer_16bit(dtype) ? 64 : 32; }
static int infer_nk(const argus_conv_desc& d, int dtype) { return d.r * d.s * d.c / infer_bke(dtype); }
// 32-row tiles while 64-row tiles would not give every CU one
int infer_bm(const argus_conv_desc& d) {
  const int M = d.n * d.ho * d.wo;
  return cdiv(M, 64) * (d.k / kInferBN) >= kInferCUs ? 64 : 32;
}
int infer_tiles(const argus_conv_desc& d) { return cdiv(d.n * d.ho * d.wo, infer_bm(d)) * (d.k / kInferBN); }
// One workspace serves every conv of a session: the ticket words of one launch must never be the slab bytes of
// another, so the ticket region has one size (4 KB: 1024 tiles) for every shape the split rule below can choose
// (tiles * splits <= 256); only a caller-forced split of a larger grid grows it. (Padded to 256 bytes per shape, a
// 65..128-tile conv found the slabs of a <= 64-tile conv in its tickets 64.. from the second forward on.)
size_t infer_ticket_bytes(const argus_conv_desc& d) { return ((size_t)infer_tiles(d) * 4 + 4095) / 4096 * 4096; }

int conv_infer_max_splits(const argus_conv_desc& d, int dtype) {
  return infer_check(d, dtype, "conv_infer_max_splits", true) ? 0 : infer_nk(d, dtype);
}

// Default split, from the measured sweep with operands from beyond the L2, as in a replayed forward
// (profiles/infer_splits.txt): past its fixed cost a launch takes about 0.30 us (bf16) /
// 0.50 us (fp32) per k-step of its slice, and the in-launch reduction adds about 0.6 us + 0.014 us per
// workgroup of the grid (slab round trip, ticket, the last arriver's serial sum). Among the powers of two
// that keep tiles * splits within one workgroup per CU, take the cheapest by that model (ties: fewer
// slices). Shapes with more than 128 tiles, or 128 tiles and a short reduction, stay unsplit.
int conv_infer_splits(const argus_conv_desc& d, int dtype) {
  if (infer_check(d, dtype, "conv_infer_splits", true)) return 0;
  const int tiles = infer_tiles(d), nk = infer_nk(d, dtype);
  const int step = infer_16bit(dtype) ? 300 : 500;  // ns per k-step (fp16: bf16's fit, reused unfitted)
  int best = 1, best_cost = step * nk;
  for (int s = 2; s <= kInferMaxSplits && s <= nk && tiles * s <= kInferCUs; s *= 2) {
    const int cost = step * cdiv(nk, s) + 600 + 14 * tiles * s;
    if (cost < best_cost) { best = s; best_cost = cost; }
  }
  return best;
}

size_t conv_infer_ws_bytes(const argus_conv_desc& d, int dtype, int splits) {
  if (splits <= 1 || infer_check(d, dtype, "conv_infer_workspace_bytes", true)) return 0;
  return infer_ticket_bytes(d) + (size_t)splits * infer_tiles(d) * infer_bm(d) * kInferBN * sizeof(float);
}

// both folds: `bias` is written by the forward layout only
template <bool kDgrad>
static int fold_bn(const argus_conv_desc& d, int dtype, const char* who, const float* w, const int64_t* strides,
                   const float* gamma, const float* beta, const float* rm, const float* rv, float eps, void* wf,
                   float* bias, hipStream_t st) {
  if (int e = infer_check(d, dtype, who, !kDgrad)) return e;
  FoldStrides fs;
  if (strides) fs = {strides[0], strides[1], strides[2], strides[3]};
  else fs = {(long long)d.r * d.s * d.c, 1, (long long)d.s * d.c, d.c};  // OHWI contiguous
  const int total = d.k * d.r * d.s * d.c;
  const int blocks = std::min(cdiv(total, 256), 4096);
  auto launch = [&](auto* out) {
    using T = std::remove_pointer_t<decltype(out)>;
    hipLaunchKernelGGL((fold_bn_kernel<T, kDgrad>), dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       out, bias, d.k, d.r, d.s, d.c);
  };
  if (dtype == ARGUS_BF16) launch((bf16*)wf);
  else if (dtype == ARGUS_F32) launch((float*)wf);
  else if constexpr (!kDgrad) launch((f16*)wf);  // (F16 stays forward-only: infer_check)
  return check_launch(kDgrad ? "fold_bn_kernel (dgrad layout)" : "fold_bn_kernel");
}

int conv_fold_bn(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                 const float* beta, const float* rm, const float* rv, float eps, void* wf, float* bias,
                 hipStream_t st) {
  return fold_bn<false>(d, dtype, "conv_fold_bn", w, strides, gamma, beta, rm, rv, eps, wf, bias, st);
}

int conv_fold_bn_dgrad(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                       const float* beta, const float* rm, const float* rv, float eps, void* wfd, hipStream_t st) {
  return fold_bn<true>(d, dtype, "conv_fold_bn_dgrad", w, strides, gamma, beta, rm, rv, eps, wfd, nullptr, st);
}

int conv_fold_bn_table(int count, const argus_conv_fold_src* src, void* host_table, size_t bytes, int* nblocks_fold,
                       int* nblocks_bwd) {
  if (!src || !host_table || !nblocks_fold || !nblocks_bwd) {
    set_error("conv_fold_bn_table: null argument");
    return ARGUS_ERR_ARG;
  }
  if (count <= 0) { set_error("conv_fold_bn_table: count must be positive"); return ARGUS_ERR_ARG; }
  const size_t need = (size_t)count * sizeof(FoldEntry);
  if (bytes < need) {
    set_error("conv_fold_bn_table: table of " + std::to_string(bytes) + " bytes, " + std::to_string(need) +
              " needed for " + std::to_string(count) + " entries (ARGUS_CONV_FOLD_ENTRY_BYTES each)");
    return ARGUS_ERR_ARG;
  }
  auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  FoldEntry* tab = reinterpret_cast<FoldEntry*>(host_table);
  long long blk = 0, row = 0;
  int with_bwd = 0;
  for (int i = 0; i < count; ++i) {
    const argus_conv_fold_src& s = src[i];
    const argus_conv_desc& d = s.desc;
    const std::string who = "conv_fold_bn_table: entry " + std::to_string(i);
    if (int e = infer_check(d, ARGUS_F32, who.c_str(), false)) return e;
    if (!s.w_master || !s.gamma || !s.beta || !s.running_mean || !s.running_var || !s.w_fold || !s.bias) {
      set_error(who + ": null argument");
      return ARGUS_ERR_ARG;
    }
    const int nb = (s.dwf != nullptr) + (s.dw != nullptr) + (s.db != nullptr) + (s.dgamma != nullptr) +
                   (s.dbeta != nullptr);
    if (nb != 0 && nb != 5) {
      set_error(who + ": null argument (dwf, dw, db, dgamma, dbeta: all five or none)");
      return ARGUS_ERR_ARG;
    }
    with_bwd += nb == 5;
    if (misaligned(s.w_fold) || misaligned(s.w_fold_dgrad)) {
      set_error(who + ": w_fold and w_fold_dgrad must be 16-byte aligned");
      return ARGUS_ERR_ARG;
    }
    if (misaligned(s.dwf) || misaligned(s.dw)) {
      set_error(who + ": dwf and dw must be 16-byte aligned");
      return ARGUS_ERR_ARG;
    }
    FoldEntry& t = tab[i];
    t = FoldEntry{};
    t.w = s.w_master;
    if (s.strides) { t.sk = s.strides[0]; t.sc = s.strides[1]; t.sr = s.strides[2]; t.ss = s.strides[3]; }
    else { t.sk = (long long)d.r * d.s * d.c; t.sc = 1; t.sr = (long long)d.s * d.c; t.ss = d.c; }  // OHWI contiguous
    t.gamma = s.gamma; t.beta = s.beta; t.rm = s.running_mean; t.rv = s.running_var; t.eps = s.eps;
    t.wf = s.w_fold; t.bias = s.bias; t.wfd = s.w_fold_dgrad;
    t.dwf = s.dwf; t.dw = s.dw; t.db = s.db; t.dgamma = s.dgamma; t.dbeta = s.dbeta;
    t.K = d.k; t.R = d.r; t.S = d.s; t.C = d.c;
    t.blk0 = (int)blk; t.row0 = (int)row;
    t.vec_w = fold_bwd_vec_w(d, t.w, t.sk, t.sc, t.sr, t.ss);
    blk += (long long)(d.k / 64) * (d.c / 64) * d.r * d.s;
    row += d.k / 4;
    if (blk > INT32_MAX) { set_error("conv_fold_bn_table: more than 2^31 tiles"); return ARGUS_ERR_SHAPE; }
  }
  if (with_bwd != 0 && with_bwd != count) {
    set_error("conv_fold_bn_table: null argument (the backward operands are given for every entry or for none)");
    return ARGUS_ERR_ARG;
  }
  *nblocks_fold = (int)blk;
  *nblocks_bwd = with_bwd ? (int)row : 0;
  return ARGUS_OK;
}

int conv_fold_bn_batch(int dtype, int count, const void* device_table, int nblocks, hipStream_t st) {
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16) {
    set_error("conv_fold_bn_batch: dtype must be ARGUS_F32 or ARGUS_BF16 (ARGUS_F16 folds per conv: "
              "argus_conv_fold_bn)");
    return ARGUS_ERR_ARG;
  }
  if (!device_table) { set_error("conv_fold_bn_batch: null argument"); return ARGUS_ERR_ARG; }
  if (count <= 0 || nblocks <= 0) {
    set_error("conv_fold_bn_batch: count and nblocks must be positive (argus_conv_fold_bn_table)");
    return ARGUS_ERR_ARG;
  }
  g_launch_work = g_launch_bytes = 0.0;  // (the shapes live in the device table)
  const FoldEntry* tab = reinterpret_cast<const FoldEntry*>(device_table);
  if (dtype == ARGUS_BF16)
    timed_launch("argus::fold_bn_kernel_batch<__bf16>", fold_bn_kernel_batch<bf16>, dim3(nblocks), dim3(256), st, tab,
                 count);
  else
    timed_launch("argus::fold_bn_kernel_batch<float>", fold_bn_kernel_batch<float>, dim3(nblocks), dim3(256), st, tab,
                 count);
  return check_launch("fold_bn_kernel_batch");
}

int conv_infer(const argus_conv_desc& d, int dtype, const void* x, const void* w, const float* bias, const void* res,
               int relu, void* out, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
  if (int e = infer_check(d, dtype, "conv_infer", true)) return e;
  const int nk = infer_nk(d, dtype);
  if (splits == 0) splits = conv_infer_splits(d, dtype);
  if (splits < 0 || splits > nk) {
    set_error("conv_infer: splits " + std::to_string(splits) + " outside 0.." + std::to_string(nk) +
              " (argus_conv_infer_max_splits)");
    return ARGUS_ERR_ARG;
  }
  InferParams p{};
  if (int e = infer_gemm_workspace(p.g, d, "conv_infer", "argus_conv_infer_workspace_bytes", splits,
                                   conv_infer_ws_bytes(d, dtype, splits), ws, ws_bytes))
    return e;
  p.g.a = x; p.g.b = w; p.g.out = out; p.bias = bias; p.res = res;
  p.g.M = d.n * d.ho * d.wo; p.g.N = d.k; p.g.brow = d.r * d.s * d.c; p.g.nk = nk; p.g.ntiles = d.k / kInferBN;
  p.H = d.h; p.W = d.w; p.C = d.c; p.Ho = d.ho; p.Wo = d.wo;
  p.stride = d.stride; p.pad = d.pad; p.S = d.s; p.relu = relu;
  p.fd_hw = make_fastdiv(d.ho * d.wo); p.fd_w = make_fastdiv(d.wo);
  p.fd_c = make_fastdiv(d.c); p.fd_s = make_fastdiv(d.s);
  const double es = infer_16bit(dtype) ? 2.0 : 4.0, px = (double)p.g.M;
  g_launch_work = 2.0 * px * d.k * p.g.brow;
  g_launch_bytes = es * ((double)d.n * d.h * d.w * d.c + (double)d.k * p.g.brow + px * d.k * (res ? 2 : 1)) + 4.0 * d.k;
  const int bm = infer_bm(d);
  if (dtype == ARGUS_BF16) infer_launch<InferFwdKernel, bf16>(p, bm, st);
  else if (dtype == ARGUS_F16) infer_launch<InferFwdKernel, f16>(p, bm, st);
  else infer_launch<InferFwdKernel, float>(p, bm, st);
  return check_launch("conv_infer_kernel");
}

}  // namespace argus
