// Frozen-inference convolutions: eval-mode BatchNorm folded into the weights once (fold_bn), then one
// launch per conv with bias + residual + ReLU in its epilogue (conv_infer_kernel). Replaces
// nn.Conv2d + nn.BatchNorm2d.eval() [+ add] + nn.ReLU of torchvision's Bottleneck.forward
// (argus/models.py:43) for a deployed model, where M = images * Ho * Wo is a few hundred rows.
//
// The kernel is the register-staged implicit GEMM of conv.hip (swizzled 128-byte LDS rows, LDS double
// buffer + 2-deep register ring) on 64- or 32-row x 64-column tiles, and it splits the reduction
// (R*S*C) over grid.z when the tiles alone leave most CUs idle: every slice stores its fp32 accumulators
// as a slab, takes a ticket on its output tile, and the workgroup that draws the last ticket sums the
// slabs in slice order 0..splits-1 (so the result does not depend on arrival order), applies the
// epilogue and resets the ticket. Nobody waits: every other slice exits after its ticket.
// Hand-off (MI355X_MICROARCH.md §Workgroup dispatch; bnfin.h fin_ticket is the in-tree precedent): plain
// slab stores -> every wave drains (s_waitcnt vmcnt(0)) -> workgroup barrier -> one lane: agent-scope
// release fence, second drain, relaxed agent-scope fetch_add; the last arriver: agent-scope acquire
// fence + drain before the workgroup's plain slab loads. Correct for any placement of a tile's slices.
#include <algorithm>

#include "igemm.h"
#include "ktimer.h"

namespace argus {

constexpr int kInferBN = 64;          // output channels per tile
constexpr int kInferMaxSplits = 16;   // slab budget: 16 slabs of <= 16 KB per tile
constexpr int kInferCUs = 256;

struct InferParams {
  const void* x;
  const void* w;
  const float* bias;
  const void* res;
  void* out;
  float* slabs;       // [tile][split][BM * 64] fp32, in the accumulator's register order
  unsigned* tickets;  // [tile]
  int M, H, W, C, K, Ho, Wo, stride, pad, S, RSC;
  int nk, splits, relu, ntiles;
  FastDiv fd_hw, fd_w, fd_c, fd_s;
};

// ---- fold ---------------------------------------------------------------------------------------------
// w_fold[k][r][s][c] = T(w[k][c][r][s] * scale[k]) (one fp32 multiply, then round to nearest even; fp16
// saturates to +-65504: from_f32<f16>),
// bias[k] = shift[k]; scale / shift = bn_eval_coeff (bnfin.h)
struct FoldStrides { long long sk, sc, sr, ss; };

template <typename T>
__global__ __launch_bounds__(256) void fold_bn_kernel(const float* __restrict__ w, FoldStrides st,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ rm, const float* __restrict__ rv,
                                                      float eps, T* __restrict__ wf, float* __restrict__ bias, int K,
                                                      int R, int S, int C) {
  const int RSC = R * S * C;
  const int total = K * RSC;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i / RSC, rem = i - k * RSC;
    const int rs = rem / C, c = rem - rs * C;
    const int r = rs / S, s = rs - r * S;
    float sc, sh;
    bn_eval_coeff(gamma, beta, rm, rv, eps, k, sc, sh);
    wf[i] = from_f32<T>(w[k * st.sk + c * st.sc + r * st.sr + s * st.ss] * sc);
    if (rem == 0) bias[k] = sh;
  }
}

// ---- forward ------------------------------------------------------------------------------------------
template <typename T, int BM>
__global__ __launch_bounds__(256, 2) void conv_infer_kernel(const InferParams p) {
  constexpr int E = Chunk<T>::E;
  constexpr int BN = kInferBN;
  constexpr int BKE = 8 * E;  // K elements per k-step: one 128-byte LDS row
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
  const T* __restrict__ A = reinterpret_cast<const T*>(p.x);
  const T* __restrict__ B = reinterpret_cast<const T*>(p.w);

  int a_off[AR], a_ih[AR], a_iw[AR];
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = mt * BM + (tid >> 3) + 32 * i;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const int nimg = fdiv(mm, p.fd_hw), rem = mm - nimg * (p.Ho * p.Wo);
    const int oh = fdiv(rem, p.fd_w), ow = rem - oh * p.Wo;
    a_ih[i] = oh * p.stride;
    a_iw[i] = ow * p.stride;
    a_off[i] = ((nimg * p.H + a_ih[i]) * p.W + a_iw[i]) * p.C;
  }
  const T* b_row[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) b_row[i] = B + (size_t)(nt * BN + (tid >> 3) + 32 * i) * p.RSC + cidx * E;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Stage {
    u32x4 a[AR], b[BR];
    bool ok[AR];
  };

  // a k-step never straddles a filter tap: C is a multiple of 64 >= BKE
  auto load = [&](int kt, Stage& S) {
    const int k0 = kt * BKE;
    const int t = fdiv(k0, p.fd_c), ci0 = k0 - t * p.C;
    const int r = fdiv(t, p.fd_s), s = t - r * p.S;
    const int dh = r - p.pad, dw = s - p.pad;
    const int ch = ci0 + cidx * E;
    const int tap = (dh * p.W + dw) * p.C + ch;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int ih = a_ih[i] + dh, iw = a_iw[i] + dw;
      const bool ok = a_ok[i] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      S.a[i] = ld16(A + (ok ? a_off[i] + tap : ch));  // rows outside the image are zeroed in store()
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

  // this slice's k-steps [kb, kb + nk): LDS double buffer + 2-deep register ring (conv.hip's main loop)
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
    // slab element ((mi * NI + ni) * 256 + tid) * 4 + r: 16-byte stores, and the reducer's thread tid reads
    // back exactly the registers it would have held
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
    // (clamped addresses, x + 0 = x selects: common.h kLoadBatch), so a batch pays one memory latency
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

  // ---- epilogue: fp32 C tile through LDS; out = [relu](acc + bias [+ res]) in fp32, rounded once ----
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
  float bv[E];
  BwdEpiAcc<T, 3>::ld(bv, p.bias + col);
  T* __restrict__ O = reinterpret_cast<T*>(p.out);
  const T* __restrict__ Rs = reinterpret_cast<const T*>(p.res);
  u32x4 rv[NIT];
  bool ok[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int m = mt * BM + tid / CPR + RPP * it;
    ok[it] = m < p.M;
    if (Rs && ok[it]) rv[it] = ld16(Rs + (size_t)m * p.K + col);
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
      f[j] = v.x + bv[j]; f[j + 1] = v.y + bv[j + 1]; f[j + 2] = v.z + bv[j + 2]; f[j + 3] = v.w + bv[j + 3];
    }
    if (Rs) {
      float r[E];
      ChunkCvt<T>::unpack(rv[it], r);
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] += r[j];
    }
    if (p.relu) {
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] = fmaxf(f[j], 0.f);
    }
    st16(O + (size_t)m * p.K + col, ChunkCvt<T>::pack(f));
  }
}

// ---- host ---------------------------------------------------------------------------------------------
static bool infer_dtype_ok(int dtype) { return dtype == ARGUS_F32 || dtype == ARGUS_BF16 || dtype == ARGUS_F16; }
static bool infer_16bit(int dtype) { return dtype == ARGUS_BF16 || dtype == ARGUS_F16; }

// the four non-stem conv kinds of ResNet-50; sets the error message when not served
static int infer_check(const argus_conv_desc& d, int dtype, const char* who) {
  if (!infer_dtype_ok(dtype)) {
    set_error(std::string(who) + ": dtype must be ARGUS_F32, ARGUS_BF16 or ARGUS_F16");
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
  return infer_check(d, dtype, "conv_infer_max_splits") ? 0 : infer_nk(d, dtype);
}

// Default split, from the measured sweep with operands from beyond the L2, as in a replayed forward
// (profiles/infer_splits.txt): past its fixed cost a launch takes about 0.30 us (bf16) /
// 0.50 us (fp32) per k-step of its slice, and the in-launch reduction adds about 0.6 us + 0.014 us per
// workgroup of the grid (slab round trip, ticket, the last arriver's serial sum). Among the powers of two
// that keep tiles * splits within one workgroup per CU, take the cheapest by that model (ties: fewer
// slices). Shapes with more than 128 tiles, or 128 tiles and a short reduction, stay unsplit.
int conv_infer_splits(const argus_conv_desc& d, int dtype) {
  if (infer_check(d, dtype, "conv_infer_splits")) return 0;
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
  if (splits <= 1 || infer_check(d, dtype, "conv_infer_workspace_bytes")) return 0;
  return infer_ticket_bytes(d) + (size_t)splits * infer_tiles(d) * infer_bm(d) * kInferBN * sizeof(float);
}

int conv_fold_bn(const argus_conv_desc& d, int dtype, const float* w, const int64_t* strides, const float* gamma,
                 const float* beta, const float* rm, const float* rv, float eps, void* wf, float* bias,
                 hipStream_t st) {
  if (int e = infer_check(d, dtype, "conv_fold_bn")) return e;
  FoldStrides fs;
  if (strides) fs = {strides[0], strides[1], strides[2], strides[3]};
  else fs = {(long long)d.r * d.s * d.c, 1, (long long)d.s * d.c, d.c};  // OHWI contiguous
  const int total = d.k * d.r * d.s * d.c;
  const int blocks = std::min(cdiv(total, 256), 4096);
  if (dtype == ARGUS_BF16)
    hipLaunchKernelGGL(fold_bn_kernel<bf16>, dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       (bf16*)wf, bias, d.k, d.r, d.s, d.c);
  else if (dtype == ARGUS_F16)
    hipLaunchKernelGGL(fold_bn_kernel<f16>, dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       (f16*)wf, bias, d.k, d.r, d.s, d.c);
  else
    hipLaunchKernelGGL(fold_bn_kernel<float>, dim3(blocks), dim3(256), 0, st, w, fs, gamma, beta, rm, rv, eps,
                       (float*)wf, bias, d.k, d.r, d.s, d.c);
  return check_launch("fold_bn_kernel");
}

template <typename T, int BM>
static const char* infer_name() {
  static const std::string s =
      std::string("argus::conv_infer_kernel<") + type_name<T>() + ", " + std::to_string(BM) + ">";
  return s.c_str();
}

template <typename T>
static void infer_launch(const InferParams& p, int bm, dim3 grid, hipStream_t st) {
  if (bm == 64) timed_launch(infer_name<T, 64>(), conv_infer_kernel<T, 64>, grid, dim3(256), st, p);
  else timed_launch(infer_name<T, 32>(), conv_infer_kernel<T, 32>, grid, dim3(256), st, p);
}

int conv_infer(const argus_conv_desc& d, int dtype, const void* x, const void* w, const float* bias, const void* res,
               int relu, void* out, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
  if (int e = infer_check(d, dtype, "conv_infer")) return e;
  const int nk = infer_nk(d, dtype);
  if (splits == 0) splits = conv_infer_splits(d, dtype);
  if (splits < 0 || splits > nk) {
    set_error("conv_infer: splits " + std::to_string(splits) + " outside 0.." + std::to_string(nk) +
              " (argus_conv_infer_max_splits)");
    return ARGUS_ERR_ARG;
  }
  const size_t need = conv_infer_ws_bytes(d, dtype, splits);
  if (splits > 1 && (!ws || ws_bytes < need)) {
    set_error("conv_infer: workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) +
              " needed for " + std::to_string(splits) + " splits (argus_conv_infer_workspace_bytes)");
    return ARGUS_ERR_ARG;
  }
  if (splits > 1 && (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("conv_infer: workspace must be 16-byte aligned");
    return ARGUS_ERR_ARG;
  }
  const int bm = infer_bm(d);
  InferParams p{};
  p.x = x; p.w = w; p.bias = bias; p.res = res; p.out = out;
  p.tickets = reinterpret_cast<unsigned*>(ws);
  p.slabs = splits > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + infer_ticket_bytes(d)) : nullptr;
  p.M = d.n * d.ho * d.wo; p.H = d.h; p.W = d.w; p.C = d.c; p.K = d.k; p.Ho = d.ho; p.Wo = d.wo;
  p.stride = d.stride; p.pad = d.pad; p.S = d.s; p.RSC = d.r * d.s * d.c;
  p.nk = nk; p.splits = splits; p.relu = relu; p.ntiles = d.k / kInferBN;
  p.fd_hw = make_fastdiv(d.ho * d.wo); p.fd_w = make_fastdiv(d.wo);
  p.fd_c = make_fastdiv(d.c); p.fd_s = make_fastdiv(d.s);
  const double es = infer_16bit(dtype) ? 2.0 : 4.0, px = (double)p.M;
  g_launch_work = 2.0 * px * d.k * p.RSC;
  g_launch_bytes = es * ((double)d.n * d.h * d.w * d.c + (double)d.k * p.RSC + px * d.k * (res ? 2 : 1)) + 4.0 * d.k;
  const dim3 grid(cdiv(p.M, bm) * p.ntiles, 1, splits);
  if (dtype == ARGUS_BF16) infer_launch<bf16>(p, bm, grid, st);
  else if (dtype == ARGUS_F16) infer_launch<f16>(p, bm, grid, st);
  else infer_launch<float>(p, bm, grid, st);
  return check_launch("conv_infer_kernel");
}

}  // namespace argus
