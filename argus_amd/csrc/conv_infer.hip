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
