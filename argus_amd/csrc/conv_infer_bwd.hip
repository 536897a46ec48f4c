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
// Tiling, staging, split-K and its hand-off are conv_infer_kernel's, unchanged: 64- or 32-row x 64-column
// tiles, swizzled 128-byte LDS rows, LDS double buffer + 2-deep register ring, grid.z slices with fp32 slabs
// in register order, a ticket per tile, the last arriver sums slabs 0..splits-1 in order and resets the ticket
// (plain slab stores -> every wave drains -> barrier -> one lane: agent-scope release fence, drain, relaxed
// agent-scope fetch_add; the last arriver: agent-scope acquire fence + drain before the plain slab loads).
#include <algorithm>

#include "igemm.h"
#include "ktimer.h"

namespace argus {

constexpr int kInferBwdBN = 64;  // dx channels per tile (conv_infer.hip: kInferBN)

struct InferBwdParams {
  const void* dy;
  const void* w;       // w_fold_dgrad [C][R*S*K]
  const void* addend;  // (M, C) or NULL
  const void* mask;    // (M, C) or NULL
  void* dx;
  float* slabs;       // [tile][split][BM * 64] fp32, in the accumulator's register order
  unsigned* tickets;  // [tile]
  int M, H, W, C, K, Ho, Wo, sh, dh0, dw0, S, RSK;  // sh = stride - 1 (stride 1 or 2: a shift and a mask)
  int nk, splits, ntiles;
  FastDiv fd_hw, fd_w, fd_k, fd_s;
};

// ---- fold ---------------------------------------------------------------------------------------------
// wfd[c][R-1-r][S-1-s][k] = T(w[k][c][r][s] * scale[k]): fold_bn_kernel's product and rounding, elsewhere
struct FoldBwdStrides { long long sk, sc, sr, ss; };

template <typename T>
__global__ __launch_bounds__(256) void fold_bn_dgrad_kernel(const float* __restrict__ w, FoldBwdStrides st,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ rm, const float* __restrict__ rv,
                                                            float eps, T* __restrict__ wfd, int K, int R, int S, int C) {
  const int RSK = R * S * K;
  const int total = C * RSK;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i / RSK, rem = i - c * RSK;
    const int rs = rem / K, k = rem - rs * K;
    const int r = R - 1 - rs / S, s = S - 1 - (rs - (rs / S) * S);
    float sc, sh;
    bn_eval_coeff(gamma, beta, rm, rv, eps, k, sc, sh);
    wfd[i] = from_f32<T>(w[k * st.sk + c * st.sc + r * st.sr + s * st.ss] * sc);
  }
}

// ---- data gradient ------------------------------------------------------------------------------------
template <typename T, int BM>
__global__ __launch_bounds__(256, 2) void conv_infer_dgrad_kernel(const InferBwdParams p) {
  constexpr int E = Chunk<T>::E;
  constexpr int BN = kInferBwdBN;
  constexpr int BKE = 8 * E;  // reduction elements per k-step: one 128-byte LDS row
  constexpr int MI = BM / 32, NI = BN / 32;
  constexpr int AR = BM / 32, BR = BN / 32;
  constexpr int LD = BN + 4;  // fp32 epilogue tile, padded rows (16-byte aligned)
  constexpr int STAGE_B = 2 * (BM + BN) * 128, EPI_B = BM * LD * 4;
  constexpr int LDS_BYTES = STAGE_B > EPI_B ? STAGE_B : EPI_B;
  // the only LDS object: operand staging, then the "last arriver" flag, then the fp32 C tile
  __shared__ __attribute__((aligned(16))) u32x4 lds[LDS_BYTES / 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cidx = tid & 7;
  const int tile = blockIdx.x;
  const int mt = tile / p.ntiles, nt = tile - mt * p.ntiles;
  const T* __restrict__ A = reinterpret_cast<const T*>(p.dy);
  const T* __restrict__ B = reinterpret_cast<const T*>(p.w);

  // a row = one dx pixel (nimg, ih, iw); a_img: element offset of its image in dy
  int a_img[AR], a_ih[AR], a_iw[AR];
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = mt * BM + (tid >> 3) + 32 * i;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const int nimg = fdiv(mm, p.fd_hw), rem = mm - nimg * (p.H * p.W);
    a_ih[i] = fdiv(rem, p.fd_w);
    a_iw[i] = rem - a_ih[i] * p.W;
    a_img[i] = nimg * p.Ho * p.Wo * p.K;
  }
  const T* b_row[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) b_row[i] = B + (size_t)(nt * BN + (tid >> 3) + 32 * i) * p.RSK + cidx * E;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Stage {
    u32x4 a[AR], b[BR];
    bool ok[AR];
  };

  // a k-step never straddles a filter tap: K is a multiple of 64 >= BKE
  const int smask = p.sh;  // stride - 1: 0 or 1
  auto load = [&](int kt, Stage& S) {
    const int k0 = kt * BKE;
    const int t = fdiv(k0, p.fd_k), ko0 = k0 - t * p.K;
    const int r = fdiv(t, p.fd_s), s = t - r * p.S;
    const int dh = r - p.dh0, dw = s - p.dw0;
    const int ch = ko0 + cidx * E;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      // the tap contributes only where (ih + dh, iw + dw) is a whole multiple of the stride inside the output
      const int th = a_ih[i] + dh, tw = a_iw[i] + dw;
      const int oh = th >> p.sh, ow = tw >> p.sh;  // (arithmetic shift: negative stays negative)
      const bool ok = a_ok[i] && ((th | tw) & smask) == 0 && (unsigned)oh < (unsigned)p.Ho &&
                      (unsigned)ow < (unsigned)p.Wo;
      S.a[i] = ld16(A + (ok ? a_img[i] + (oh * p.Wo + ow) * p.K + ch : ch));  // other rows are zeroed in store()
      S.ok[i] = ok;
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) S.b[i] = ld16(b_row[i] + k0);
  };

  auto store = [&](int buf, Stage& S) {
    u32x4* L = lds + buf * (BM + BN) * 8;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int row = (tid >> 3) + 32 * i;
      L[row * 8 + (cidx ^ swz8(row))] = sel(S.ok[i], S.a[i]);
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int row = (tid >> 3) + 32 * i;
      L[BM * 8 + row * 8 + (cidx ^ swz8(row))] = S.b[i];
    }
  };

  const int g = lane >> 4, i16 = lane & 15;
  auto compute = [&](int buf) {
    const u32x4* L = lds + buf * (BM + BN) * 8;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4 fa[MI], fb[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int row = wm * (BM / 2) + mi * 16 + i16;
        fa[mi] = L[row * 8 + ((4 * s2 + g) ^ swz8(row))];
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = wn * (BN / 2) + ni * 16 + i16;
        fb[ni] = L[BM * 8 + row * 8 + ((4 * s2 + g) ^ swz8(row))];
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) Mma<T>::run(acc[mi][ni], fa[mi], fb[ni]);
    }
  };

  // this slice's k-steps [kb, kb + nk): LDS double buffer + 2-deep register ring (conv_infer_kernel's loop)
  const int z = blockIdx.z;
  const int kb = (int)((long long)z * p.nk / p.splits);
  const int nk = (int)((long long)(z + 1) * p.nk / p.splits) - kb;
  if (nk > 0) {
    Stage S0, S1;
    load(kb, S0);
    store(0, S0);
    if (nk > 1) load(kb + 1, S1);
    if (nk > 2) load(kb + 2, S0);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      compute(0);
      store(1, S1);
      if (kt + 3 < nk) load(kb + kt + 3, S1);
      __syncthreads();
      compute(1);
      if (kt + 2 < nk) {
        store(0, S0);
        if (kt + 4 < nk) load(kb + kt + 4, S0);
      }
      __syncthreads();
    }
    if (kt < nk) {
      compute(0);
      __syncthreads();
    }
  }

  if (p.splits > 1) {
    // conv_infer_kernel's hand-off, statement for statement. Slab element ((mi * NI + ni) * 256 + tid) * 4 + r:
    // 16-byte stores, and the reducer's thread tid reads back exactly the registers it would have held
    constexpr int SLAB = BM * BN;
    float* slab = p.slabs + ((size_t)tile * p.splits + z) * SLAB;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        *reinterpret_cast<f32x4*>(slab + ((mi * NI + ni) * 256 + tid) * 4) = acc[mi][ni];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its slab stores
    __syncthreads();
    int* flag = reinterpret_cast<int*>(lds);
    if (tid == 0) {
      fin_gu32* cnt = (fin_gu32*)(p.tickets + tile);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the fence's own wait may be dropped: keep it
      const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = t == (unsigned)p.splits - 1u;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // reusable by the next launch
      }
      *flag = last;
    }
    __syncthreads();
    const bool last = *flag != 0;
    __syncthreads();  // the flag word is part of the C tile below
    if (!last) return;
    // fixed-order sum of the slabs 0..splits-1 (this workgroup's own included); loads in batches of 4
    const float* base = p.slabs + (size_t)tile * p.splits * SLAB;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < p.splits; z0 += 4) {
      f32x4 v[4][MI][NI];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int zz = z0 + u < p.splits ? z0 + u : p.splits - 1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            v[u][mi][ni] = *reinterpret_cast<const f32x4*>(base + (size_t)zz * SLAB + ((mi * NI + ni) * 256 + tid) * 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool on = z0 + u < p.splits;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[mi][ni] += on ? v[u][mi][ni] : zero;
          }
      }
    }
  }

  // ---- epilogue: fp32 C tile through LDS; dx = (mask_src > 0) * (acc [+ addend]) in fp32, rounded once ----
  float* Cs = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Cs[(wm * (BM / 2) + mi * 16 + g * 4 + r) * LD + wn * (BN / 2) + ni * 16 + i16] = acc[mi][ni][r];
  __syncthreads();
  constexpr int CPR = BN / E;     // 16-byte output chunks per row
  constexpr int RPP = 256 / CPR;  // rows per pass
  constexpr int NIT = BM / RPP;
  static_assert(NIT * RPP == BM, "epilogue row partition");
  const int c = tid % CPR;
  const int col = nt * BN + c * E;
  T* __restrict__ O = reinterpret_cast<T*>(p.dx);
  const T* Ad = reinterpret_cast<const T*>(p.addend);
  const T* Mk = reinterpret_cast<const T*>(p.mask);
  u32x4 av[NIT], mv[NIT];
  bool ok[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int m = mt * BM + tid / CPR + RPP * it;
    ok[it] = m < p.M;
    if (Ad && ok[it]) av[it] = ld16(Ad + (size_t)m * p.C + col);
    if (Mk && ok[it]) mv[it] = ld16(Mk + (size_t)m * p.C + col);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (!ok[it]) continue;
    const int rr = tid / CPR + RPP * it;
    const int m = mt * BM + rr;
    float f[E];
#pragma unroll
    for (int j = 0; j < E; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(Cs + rr * LD + c * E + j);
      f[j] = v.x; f[j + 1] = v.y; f[j + 2] = v.z; f[j + 3] = v.w;
    }
    if (Ad) {
      float a[E];
      ChunkCvt<T>::unpack(av[it], a);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] += a[j];
    }
    if (Mk) {
      float x[E];
      ChunkCvt<T>::unpack(mv[it], x);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] = x[j] > 0.f ? f[j] : 0.f;  // NaN and 0 mask to 0
    }
    st16(O + (size_t)m * p.C + col, ChunkCvt<T>::pack(f));
  }
}

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
// F32 / BF16 and the four conv kinds of argus_conv_infer (conv_infer.hip infer_check's rule); sets the message
static int infer_bwd_check(const argus_conv_desc& d, int dtype, const char* who) {
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16) {
    set_error(std::string(who) + ": dtype must be ARGUS_F32 or ARGUS_BF16 (no ARGUS_F16, ARGUS_FP8 gradients)");
    return ARGUS_ERR_ARG;
  }
  if (int e = conv_check_desc(d)) return e;
  const bool k1 = d.r == 1 && d.s == 1 && d.pad == 0, k3 = d.r == 3 && d.s == 3 && d.pad == 1;
  if (d.stem || !(k1 || k3) || d.stride < 1 || d.stride > 2 || d.c % 64 || d.k % 64) {
    set_error(std::string(who) + ": serves the convs argus_conv_infer serves: 1x1 (pad 0) and 3x3 (pad 1) of stride 1 "
                                 "or 2 with c, k multiples of 64 (not the stem)");
    return ARGUS_ERR_SHAPE;
  }
  return ARGUS_OK;
}

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
  if (int e = infer_bwd_check(d, dtype, "conv_infer_dgrad_plan")) return e;
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

int conv_fold_bn_dgrad(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                       const float* beta, const float* rm, const float* rv, float eps, void* wfd, hipStream_t st) {
  if (int e = infer_bwd_check(d, dtype, "conv_fold_bn_dgrad")) return e;
  FoldBwdStrides fs;
  if (strides) fs = {strides[0], strides[1], strides[2], strides[3]};
  else fs = {(long long)d.r * d.s * d.c, 1, (long long)d.s * d.c, d.c};  // OHWI contiguous
  const int total = d.k * d.r * d.s * d.c;
  const int blocks = std::min(cdiv(total, 256), 4096);
  if (dtype == ARGUS_BF16)
    hipLaunchKernelGGL(fold_bn_dgrad_kernel<bf16>, dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       (bf16*)wfd, d.k, d.r, d.s, d.c);
  else
    hipLaunchKernelGGL(fold_bn_dgrad_kernel<float>, dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       (float*)wfd, d.k, d.r, d.s, d.c);
  return check_launch("fold_bn_dgrad_kernel");
}

template <typename T, int BM>
static const char* infer_bwd_name() {
  static const std::string s =
      std::string("argus::conv_infer_dgrad_kernel<") + type_name<T>() + ", " + std::to_string(BM) + ">";
  return s.c_str();
}

template <typename T>
static void infer_bwd_launch(const InferBwdParams& p, int bm, dim3 grid, hipStream_t st) {
  if (bm == 64) timed_launch(infer_bwd_name<T, 64>(), conv_infer_dgrad_kernel<T, 64>, grid, dim3(256), st, p);
  else timed_launch(infer_bwd_name<T, 32>(), conv_infer_dgrad_kernel<T, 32>, grid, dim3(256), st, p);
}

int conv_infer_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* wfd, const void* addend,
                     const void* mask_src, void* dx, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
  int mx = 0;
  size_t need = 0;
  if (int e = conv_infer_dgrad_plan(d, dtype, splits, &splits, &mx, &need)) return e;
  if (splits > 1 && (!ws || ws_bytes < need)) {
    set_error("conv_infer_dgrad: workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) +
              " needed for " + std::to_string(splits) + " splits (argus_conv_infer_dgrad_plan)");
    return ARGUS_ERR_ARG;
  }
  if (splits > 1 && (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("conv_infer_dgrad: workspace must be 16-byte aligned");
    return ARGUS_ERR_ARG;
  }
  const argus_conv_desc m = infer_bwd_mirror(d);
  const int bm = infer_bm(m);
  InferBwdParams p{};
  p.dy = dy; p.w = wfd; p.addend = addend; p.mask = mask_src; p.dx = dx;
  p.tickets = reinterpret_cast<unsigned*>(ws);
  p.slabs = splits > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + infer_ticket_bytes(m)) : nullptr;
  p.M = d.n * d.h * d.w; p.H = d.h; p.W = d.w; p.C = d.c; p.K = d.k; p.Ho = d.ho; p.Wo = d.wo;
  p.sh = d.stride - 1; p.dh0 = d.r - 1 - d.pad; p.dw0 = d.s - 1 - d.pad; p.S = d.s; p.RSK = d.r * d.s * d.k;
  p.nk = mx; p.splits = splits; p.ntiles = d.c / kInferBwdBN;
  p.fd_hw = make_fastdiv(d.h * d.w); p.fd_w = make_fastdiv(d.w);
  p.fd_k = make_fastdiv(d.k); p.fd_s = make_fastdiv(d.s);
  const double es = dtype == ARGUS_BF16 ? 2.0 : 4.0, px = (double)p.M;
  g_launch_work = 2.0 * px * d.c * p.RSK;
  g_launch_bytes = es * ((double)d.n * d.ho * d.wo * d.k + (double)d.c * p.RSK +
                         px * d.c * (1 + (addend ? 1 : 0) + (mask_src ? 1 : 0)));
  const dim3 grid(cdiv(p.M, bm) * p.ntiles, 1, splits);
  if (dtype == ARGUS_BF16) infer_bwd_launch<bf16>(p, bm, grid, st);
  else infer_bwd_launch<float>(p, bm, grid, st);
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
