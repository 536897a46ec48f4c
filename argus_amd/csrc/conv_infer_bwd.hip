// Frozen gradient: the data gradient of a BN-folded conv (conv_infer.hip is its forward). With eval-mode
// BatchNorm folded into the weights the network is conv + bias + ReLU, so the input gradient that
// torch.autograd.grad computes through nn.Conv2d + nn.BatchNorm2d.eval() + nn.ReLU of torchvision's
// Bottleneck.forward (argus/models.py:66-90 with the model in eval mode) is, per conv,
//   dx = relu'(x) * (conv_transpose(dy, w_fold) [+ addend]),
// x the conv's own input (the post-ReLU output of its producer), the addend the residual branch's gradient.
//
// GEMM: M = n*h*w rows (one per dx pixel), N = c columns, reduction over (r', s', k) against
// w_fold_dgrad[c][r'][s'][k], the transposed filter with its taps rotated by 180 degrees: tap (r', s') of a dx
// pixel (ih, iw) reads dy at ((ih - (R-1-pad) + r') / stride, (iw - (S-1-pad) + s') / stride) when both are
// whole and inside the output; otherwise the A row is zero for that k-step (a per-row predicate: a stride-2
// conv spends three quarters of its MACs on zeros, in 6 of the 52 launches of a latency-bound chain).
// The kernel is infer_gemm.h's tile GEMM (tiling, staging, split-K and its hand-off live there, shared with the
// forward) with the data gradient's two policies: a GEMM row is a dx pixel, and the epilogue is addend + mask.
#include <algorithm>

#include "infer_gemm.h"

namespace argus {

struct InferBwdParams {
  InferGemm g;         // a = dy, b = w_fold_dgrad [C][R*S*K], out = dx (M, C)
  const void* addend;  // (M, C) or NULL
  const void* mask;    // (M, C) or NULL
  int H, W, K, Ho, Wo, sh, dh0, dw0, S;  // sh = stride - 1 (stride 1 or 2: a shift and a mask)
  FastDiv fd_hw, fd_w, fd_k, fd_s;
};

// ---- data gradient ------------------------------------------------------------------------------------
// a row = one dx pixel (nimg, ih, iw); img: element offset of its image in dy
template <int AR>
struct InferBwdA {
  int img[AR], ih[AR], iw[AR];
  struct Step { int dh, dw, ch; };
  ARGUS_DEV void row(const InferBwdParams& p, int i, int m) {
    const int nimg = fdiv(m, p.fd_hw), rem = m - nimg * (p.H * p.W);
    ih[i] = fdiv(rem, p.fd_w);
    iw[i] = rem - ih[i] * p.W;
    img[i] = nimg * p.Ho * p.Wo * p.K;
  }
  ARGUS_DEV Step step(const InferBwdParams& p, int k0, int ch0) const {
    const int t = fdiv(k0, p.fd_k), ko0 = k0 - t * p.K;
    const int r = fdiv(t, p.fd_s), s = t - r * p.S;
    Step st;
    st.dh = r - p.dh0;
    st.dw = s - p.dw0;
    st.ch = ko0 + ch0;
    return st;
  }
  // the tap contributes only where (ih + dh, iw + dw) is a whole multiple of the stride inside the output
  ARGUS_DEV bool at(const InferBwdParams& p, const Step& st, int i, int& o) const {
    const int th = ih[i] + st.dh, tw = iw[i] + st.dw;
    const int oh = th >> p.sh, ow = tw >> p.sh;  // (arithmetic shift: negative stays negative)
    o = img[i] + (oh * p.Wo + ow) * p.K + st.ch;
    return ((th | tw) & p.sh) == 0 && (unsigned)oh < (unsigned)p.Ho && (unsigned)ow < (unsigned)p.Wo;
  }
};

// dx = (mask_src > 0) * (acc [+ addend])
template <typename T, int NIT>
struct InferBwdEpi {
  static constexpr int E = Chunk<T>::E;
  u32x4 av[NIT], mv[NIT];
  ARGUS_DEV void init(const InferBwdParams&, int) {}
  ARGUS_DEV void prefetch(const InferBwdParams& p, int it, size_t at) {
    if (p.addend) av[it] = ld16(reinterpret_cast<const T*>(p.addend) + at);
    if (p.mask) mv[it] = ld16(reinterpret_cast<const T*>(p.mask) + at);
  }
  ARGUS_DEV void apply(const InferBwdParams& p, int it, float (&f)[E]) const {
    if (p.addend) {
      float a[E];
      ChunkCvt<T>::unpack(av[it], a);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] += a[j];
    }
    if (p.mask) {
      float x[E];
      ChunkCvt<T>::unpack(mv[it], x);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] = x[j] > 0.f ? f[j] : 0.f;  // NaN and 0 mask to 0
    }
  }
};

template <typename T, int BM>
__global__ __launch_bounds__(256, 2) void conv_infer_dgrad_kernel(const InferBwdParams p) {
  infer_gemm_tile<T, BM, InferBwdA, InferBwdEpi>(p);
}

struct InferBwdKernel {
  static constexpr const char* name = "conv_infer_dgrad_kernel";
  template <typename T, int BM> static auto kernel() { return conv_infer_dgrad_kernel<T, BM>; }
};

// dx = dfeat / hw * (out > 0): avgpool_bwd_kernel (bn.hip) through the last block's ReLU
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_relu_kernel(int64_t nchunks, int hw, int C,
                                                               const float* __restrict__ dfeat,
                                                               const T* __restrict__ out, T* __restrict__ dx) {
  constexpr int E = Chunk<T>::E;
  const float inv = 1.f / (float)hw;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i * E;
    const int c0 = (int)(e % C);
    const int64_t img = e / ((int64_t)hw * C);
    float f[E], x[E];
    ChunkCvt<T>::unpack(ld16(out + e), x);
#pragma unroll
    for (int j = 0; j < E; ++j) f[j] = x[j] > 0.f ? dfeat[img * C + c0 + j] * inv : 0.f;
    st16(dx + e, ChunkCvt<T>::pack(f));
  }
}

// ---- host ---------------------------------------------------------------------------------------------
// The mirrored problem as a forward descriptor: a stride-1 conv of the same filter over the dx grid with the
// channel roles swapped has this GEMM's rows (n*h*w), columns (c) and reduction (r*s*k), so the forward's
// tile choice, split rule and workspace layout apply to it as they stand.
static argus_conv_desc infer_bwd_mirror(const argus_conv_desc& d) {
  argus_conv_desc m = d;
  m.c = d.k; m.k = d.c; m.stride = 1; m.ho = d.h; m.wo = d.w;
  m.n_tuning = 0; m.tuning = nullptr;
  return m;
}

int conv_infer_dgrad_plan(const argus_conv_desc& d, int dtype, int splits_in, int* splits, int* max_splits,
                          size_t* ws_bytes) {
  if (int e = infer_check(d, dtype, "conv_infer_dgrad_plan", false)) return e;
  const argus_conv_desc m = infer_bwd_mirror(d);
  const int mx = conv_infer_max_splits(m, dtype);
  if (mx <= 0) return ARGUS_ERR_SHAPE;  // (the mirrored tensor exceeds 32-bit offsets: message set)
  if (splits_in < 0 || splits_in > mx) {
    set_error("conv_infer_dgrad: splits " + std::to_string(splits_in) + " outside 0.." + std::to_string(mx) +
              " (argus_conv_infer_dgrad_plan)");
    return ARGUS_ERR_ARG;
  }
  const int sp = splits_in ? splits_in : conv_infer_splits(m, dtype);
  if (splits) *splits = sp;
  if (max_splits) *max_splits = mx;
  if (ws_bytes) *ws_bytes = conv_infer_ws_bytes(m, dtype, sp);
  return ARGUS_OK;
}

int conv_infer_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* wfd, const void* addend,
                     const void* mask_src, void* dx, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
  int mx = 0;
  size_t need = 0;
  if (int e = conv_infer_dgrad_plan(d, dtype, splits, &splits, &mx, &need)) return e;
  const argus_conv_desc m = infer_bwd_mirror(d);
  InferBwdParams p{};
  if (int e = infer_gemm_workspace(p.g, m, "conv_infer_dgrad", "argus_conv_infer_dgrad_plan", splits, need, ws,
                                   ws_bytes))
    return e;
  p.g.a = dy; p.g.b = wfd; p.g.out = dx; p.addend = addend; p.mask = mask_src;
  p.g.M = d.n * d.h * d.w; p.g.N = d.c; p.g.brow = d.r * d.s * d.k; p.g.nk = mx; p.g.ntiles = d.c / kInferBN;
  p.H = d.h; p.W = d.w; p.K = d.k; p.Ho = d.ho; p.Wo = d.wo;
  p.sh = d.stride - 1; p.dh0 = d.r - 1 - d.pad; p.dw0 = d.s - 1 - d.pad; p.S = d.s;
  p.fd_hw = make_fastdiv(d.h * d.w); p.fd_w = make_fastdiv(d.w);
  p.fd_k = make_fastdiv(d.k); p.fd_s = make_fastdiv(d.s);
  const double es = dtype == ARGUS_BF16 ? 2.0 : 4.0, px = (double)p.g.M;
  g_launch_work = 2.0 * px * d.c * p.g.brow;
  g_launch_bytes = es * ((double)d.n * d.ho * d.wo * d.k + (double)d.c * p.g.brow +
                         px * d.c * (1 + (addend ? 1 : 0) + (mask_src ? 1 : 0)));
  const int bm = infer_bm(m);
  if (dtype == ARGUS_BF16) infer_launch<InferBwdKernel, bf16>(p, bm, st);
  else infer_launch<InferBwdKernel, float>(p, bm, st);
  return check_launch("conv_infer_dgrad_kernel");
}

}  // namespace argus

using namespace argus;

extern "C" int argus_avgpool_bwd_relu(int dtype, int n, int hw, int c, const float* dfeat, const void* out, void* dx,
                                      argus_stream_t stream) {
  if (f16_unserved(dtype, "avgpool_bwd_relu")) return ARGUS_ERR_ARG;
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16) {
    set_error("avgpool_bwd_relu: dtype must be ARGUS_F32 or ARGUS_BF16");
    return ARGUS_ERR_ARG;
  }
  if (n <= 0 || hw <= 0 || c <= 0 || !dfeat || !out || !dx) {
    set_error("avgpool_bwd_relu: bad arguments");
    return ARGUS_ERR_ARG;
  }
  const int E = dtype == ARGUS_BF16 ? 8 : 4;
  if (c % E) { set_error("avgpool_bwd_relu: bad channels"); return ARGUS_ERR_SHAPE; }
  const int64_t nch = (int64_t)n * hw * c / E;
  const int blocks = (int)std::min<int64_t>((nch + 255) / 256, 4096);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ARGUS_BF16)
    hipLaunchKernelGGL(avgpool_bwd_relu_kernel<bf16>, dim3(blocks), dim3(256), 0, st, nch, hw, c, dfeat,
                       (const bf16*)out, (bf16*)dx);
  else
    hipLaunchKernelGGL(avgpool_bwd_relu_kernel<float>, dim3(blocks), dim3(256), 0, st, nch, hw, c, dfeat,
                       (const float*)out, (float*)dx);
  return check_launch("avgpool_bwd_relu_kernel");
}
