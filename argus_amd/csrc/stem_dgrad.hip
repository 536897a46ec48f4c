// Data gradient of the ResNet-50 stem convolution (torchvision conv1: 7x7, stride 2, pad 3, 3 -> 64
// channels): autograd's grad_input of resnet.conv1 under loss.backward(), i.e. d loss / d images.
//
// Formulation: a stride-2 transposed 7x7 conv is four stride-1 convs, one per parity class of the
// output pixel. Output pixel (h, w) = (2m + ph, 2q + pw) sums dy[m + dr][q + dc][k] * w[k][r][s][c]
// over dr, dc in -1..2 with r = 3 + ph - 2 dr, s = 3 + pw - 2 dc (r, s = -1 do not exist: classes with
// an even coordinate have 3 taps along it, odd ones 4: 9, 12, 12 or 16 taps a pixel). So on the
// half-resolution grid (m, q), which is exactly the ho x wo grid of dy, the whole data gradient is ONE
// 4x4 stride-1 conv from 64 channels to 16 = (ph, pw, c(4)) followed by a depth-to-space. That fills
// the N = 16 of v_mfma_f32_16x16x32_bf16 (v_mfma_f32_16x16x4_f32 in fp32) with no thin dimension:
// M = 16 consecutive q, K = 64 channels per (dr, dc), 16 shifts. 39 of the 256 (shift, n) columns are
// structural zeros and c = 3 is padding: 1.74x the algorithmic flops, still far below the memory time.
// Every output element is the sum of its own taps in a fixed order inside one accumulator: no atomics,
// no overlap-add, bit-reproducible.
//
// A workgroup (4 waves) owns a 4 x 32 half-resolution tile = 8 x 64 output pixels x 3 channels. It
// stages the (4+3) x (32+3) dy halo tile in LDS once (loaded into registers one tile ahead, beside the
// previous tile's MFMAs; through the BN-backward apply
// dy = ca*dm + cb*y + cc when fused: argus_bn_bwd_apply's formula, rounded to bf16 in bf16 mode, zero
// outside the image AFTER the apply), and keeps the regrouped weights B[shift][k][n] in LDS for its
// whole run of tiles (built once per workgroup from the stem's w_fwd copy [64][8][8][4]; no new weight
// layout in global memory). Wave w owns tile row w: two 16-position M blocks. Pixel rows in LDS are
// padded by 32 bytes (160 B bf16, 288 B fp32): the 16 lanes of every ds_read_b128 lane group then hit 16
// distinct 16-byte slots of the 256-byte bank row. The accumulators go through LDS to planar fp32 NCHW
// rows, written as coalesced 256-byte runs.
#include <algorithm>

#include "common.h"
#include "internal.h"
#include "ktimer.h"

namespace argus {

namespace {
constexpr int kDM = 4, kDQ = 32;               // half-resolution tile (rows m, columns q)
constexpr int kHR = kDM + 3, kHC = kDQ + 3;    // dy halo tile: pixel (m0 - 1 + pr, q0 - 1 + pc)
constexpr int kORS = 2 * kDQ + 2;              // output staging: row stride (floats)
constexpr int kOCS = 2 * kDM * kORS + 20;      // ... channel stride (bank offset 4: c and g rarely collide)
constexpr int kDgMaxGrid = 512;                // persistent workgroups (2 per CU in bf16)

template <typename T>
struct DgCfg {
  static constexpr int E = Chunk<T>::E;                 // elements per 16 bytes
  static constexpr int KV = 4 * E;                      // channels per 64-byte k-chunk (one MFMA operand row)
  static constexpr int KC = 64 / KV;                    // k-chunks per pixel: 2 (bf16) / 4 (fp32)
  static constexpr int CH = 64 / E;                     // 16-byte chunks per pixel
  static constexpr int PS = 64 * (int)sizeof(T) + 32;   // LDS pixel stride, bytes
  static constexpr int WB = 16 * KC * 16 * 64;          // B[shift][kc][n][KV]
  static constexpr int DyB = kHR * kHC * PS;
  static constexpr int LdsB = WB + DyB;
  static_assert(DyB >= 3 * kOCS * 4, "output staging reuses the dy tile");
  static_assert(LdsB <= 160 * 1024, "LDS");
  static_assert(256 % CH == 0, "a thread stages one fixed channel chunk");
};
}  // namespace

struct StemDgParams {
  const void* dy;             // dy, or dm of the fused BN-backward apply: (n, Ho, Wo, 64)
  const void* y;              // apply: y (same layout), else null
  const float *ca, *cb, *cc;  // apply: dy = ca*dm + cb*y + cc per channel
  const void* w;              // w_fwd of the stem: [64][8][8][4]
  float* dx;                  // (n, 3, H, W) fp32
  int n, H, W, Ho, Wo, tiles;
};

template <typename T, bool AP>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const StemDgParams p) {
  using Cf = DgCfg<T>;
  constexpr int E = Cf::E, KV = Cf::KV, KC = Cf::KC, CH = Cf::CH, PS = Cf::PS;
  __shared__ __attribute__((aligned(16))) uint8_t lds[Cf::LdsB];
  uint8_t* wl = lds;
  uint8_t* dyl = lds + Cf::WB;
  float* outl = reinterpret_cast<float*>(dyl);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;

  // ---- B[shift][kc][n = (ph, pw, c)][kk] = w[k = kc*KV + kk][3 + ph - 2 dr][3 + pw - 2 dc][c], else 0 ----
  for (int i = tid; i < Cf::WB / 16; i += 256) reinterpret_cast<u32x4*>(wl)[i] = u32x4{0u, 0u, 0u, 0u};
  __syncthreads();
  {
    const T* W = reinterpret_cast<const T*>(p.w);
    T* B = reinterpret_cast<T*>(wl);
    for (int idx = tid; idx < 64 * 49; idx += 256) {
      const int k = idx / 49, t = idx - k * 49, r = t / 7, s = t - r * 7;
      const int ph = (r + 1) & 1, pw = (s + 1) & 1;
      const int dr = (3 + ph - r) >> 1, dc = (3 + pw - s) >> 1;  // -1..2 (the differences are even)
      const int shift = (dr + 1) * 4 + (dc + 1);
      const int kc = k / KV, kk = k - kc * KV;
      const T* src = W + k * 256 + r * 32 + s * 4;
      T* dst = B + ((shift * KC + kc) * 16 + (ph * 2 + pw) * 4) * KV + kk;
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * KV] = src[c];
    }
  }

  const int ch = tid % CH;  // this thread's 16-byte channel chunk of every dy pixel it stages
  float ca[E], cb[E], cc[E];
  if constexpr (AP) {
#pragma unroll
    for (int j = 0; j < E; ++j) { ca[j] = p.ca[ch * E + j]; cb[j] = p.cb[ch * E + j]; cc[j] = p.cc[ch * E + j]; }
  }

  const int tq = cdiv(p.Wo, kDQ), tpi = cdiv(p.Ho, kDM) * tq;
  const T* DY = reinterpret_cast<const T*>(p.dy);
  const T* Y = reinterpret_cast<const T*>(p.y);
  // the dy halo tile of one output tile, in registers: loaded a tile ahead, so the loads of tile t + 1 are
  // in flight while tile t's MFMAs run (applied when fused; zero outside the image, after the apply)
  constexpr int kIters = (kHR * kHC * CH + 255) / 256;
  struct Stage {
    u32x4 d[kIters], y[AP ? kIters : 1];
    unsigned ok;  // bit i: chunk i is a pixel of the image
  } S;
  auto load = [&](int tile) {
    const int img = tile / tpi, rem = tile - img * tpi;
    const int m0 = (rem / tq) * kDM, q0 = (rem % tq) * kDQ;
    S.ok = 0u;
#pragma unroll
    for (int i = 0; i < kIters; ++i) {
      const int px = (tid + 256 * i) / CH;
      const int pr = px / kHC, pc = px - pr * kHC;
      const int oh = m0 - 1 + pr, ow = q0 - 1 + pc;
      const bool ok = px < kHR * kHC && (unsigned)oh < (unsigned)p.Ho && (unsigned)ow < (unsigned)p.Wo;
      const size_t off = ok ? (((size_t)img * p.Ho + oh) * p.Wo + ow) * 64 + ch * E : 0;
      S.d[i] = ld16(DY + off);
      if constexpr (AP) S.y[i] = ld16(Y + off);
      S.ok |= ok ? 1u << i : 0u;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < kIters; ++i) {
      const int px = (tid + 256 * i) / CH;
      u32x4 v = S.d[i];
      if constexpr (AP) {  // argus_bn_bwd_apply's formula, fp32, rounded to the compute dtype
        float d[E], yv[E];
        unpack(v, d);
        unpack(S.y[i], yv);
#pragma unroll
        for (int j = 0; j < E; ++j) d[j] = fmaf(ca[j], d[j], fmaf(cb[j], yv[j], cc[j]));
        v = pack(d);
      }
      if (!((S.ok >> i) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
      if (px < kHR * kHC) *reinterpret_cast<u32x4*>(dyl + px * PS + ch * 16) = v;
    }
  };

  if ((int)blockIdx.x < p.tiles) load(blockIdx.x);
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int img = tile / tpi, rem = tile - img * tpi;
    const int m0 = (rem / tq) * kDM, q0 = (rem % tq) * kDQ;
    __syncthreads();  // the weights are staged; the previous tile's output staging has been read
    store();
    __syncthreads();
    if (tile + (int)gridDim.x < p.tiles) load(tile + gridDim.x);

    // ---- MFMA: wave = tile row, two blocks of 16 q; 16 shifts x KC k-chunks ----
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const uint8_t* abase = dyl + (wave * kHC + i16) * PS + g * 16;
    const uint8_t* bbase = wl + i16 * 64 + g * 16;
#pragma unroll 4
    for (int sh = 0; sh < 16; ++sh) {
      const int dr1 = sh >> 2, dc1 = sh & 3;  // dr + 1, dc + 1: halo row wave + dr1, column 16 j + i16 + dc1
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(bbase + (sh * KC + kc) * 1024);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const u32x4 a = *reinterpret_cast<const u32x4*>(abase + (dr1 * kHC + dc1 + 16 * j) * PS + kc * 64);
          if constexpr (sizeof(T) == 2) {
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                             __builtin_bit_cast(bf16x8, b), acc[j], 0, 0, 0);
          } else {  // exact fp32: k = kc*16 + 4g + e in step e (the same permutation on both operands)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc[j], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the dy tile is reused as the output staging

    // ---- depth-to-space: C[q = 16 j + 4 g + e][n = i16 = (ph, pw, c)] -> out[c][2 wave + ph][2 q + pw] ----
    {
      const int c = i16 & 3, pw = (i16 >> 2) & 1, ph = i16 >> 3;
      if (c < 3) {
        float* o = outl + c * kOCS + (2 * wave + ph) * kORS + pw;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) o[2 * (16 * j + 4 * g + e)] = acc[j][e];
      }
    }
    __syncthreads();
    float* DX = p.dx + (size_t)img * 3 * p.H * p.W;
#pragma unroll
    for (int i = 0; i < 3 * 2 * kDM * 2 * kDQ / 256; ++i) {
      const int idx = tid + 256 * i;
      const int c = idx / (2 * kDM * 2 * kDQ), row = (idx / (2 * kDQ)) % (2 * kDM), col = idx % (2 * kDQ);
      const int h = 2 * m0 + row, w = 2 * q0 + col;
      if (h < p.H && w < p.W) DX[((size_t)c * p.H + h) * p.W + w] = outl[c * kOCS + row * kORS + col];
    }
  }
}

int conv_stem_dgrad(const argus_conv_desc& d, int dtype, const void* dy, const void* w, const argus_bn_bwd_prologue* ap,
                    float* dx, hipStream_t st) {
  if (dtype != ARGUS_F32 && dtype != ARGUS_BF16) {
    set_error("conv_stem_dgrad: dtype must be ARGUS_F32 or ARGUS_BF16");
    return ARGUS_ERR_ARG;
  }
  if (int e = conv_check_desc(d)) return e;
  if (!d.stem || d.k != 64) {
    set_error("conv_stem_dgrad: not a stem descriptor (stem = 1, 3 -> 64 channels, 7x7 stride 2 pad 3)");
    return ARGUS_ERR_ARG;
  }
  if (!dy || !w || !dx) { set_error("conv_stem_dgrad: null argument"); return ARGUS_ERR_ARG; }
  if (ap && (!ap->y || !ap->ca || !ap->cb || !ap->cc)) {
    set_error("conv_stem_dgrad: bad apply arguments");
    return ARGUS_ERR_ARG;
  }
  StemDgParams p;
  p.dy = dy;
  p.y = ap ? ap->y : nullptr;
  p.ca = ap ? ap->ca : nullptr; p.cb = ap ? ap->cb : nullptr; p.cc = ap ? ap->cc : nullptr;
  p.w = w;
  p.dx = dx;
  p.n = d.n; p.H = d.h; p.W = d.w; p.Ho = d.ho; p.Wo = d.wo;
  p.tiles = d.n * cdiv(d.ho, kDM) * cdiv(d.wo, kDQ);
  const size_t es = dtype == ARGUS_BF16 ? 2 : 4;
  g_launch_work = 2.0 * d.n * d.ho * d.wo * 64 * 147;  // algorithmic flops / bytes (ktimer)
  g_launch_bytes = (double)d.n * d.ho * d.wo * 64 * es * (ap ? 2 : 1) + (double)d.n * 3 * d.h * d.w * 4;
  const dim3 grid(std::min(p.tiles, dtype == ARGUS_BF16 ? kDgMaxGrid : kDgMaxGrid / 2)), block(256);
  if (dtype == ARGUS_BF16) {
    if (ap) timed_launch("argus::stem_dgrad_kernel<__bf16, true>", stem_dgrad_kernel<bf16, true>, grid, block, st, p);
    else timed_launch("argus::stem_dgrad_kernel<__bf16, false>", stem_dgrad_kernel<bf16, false>, grid, block, st, p);
  } else {
    if (ap) timed_launch("argus::stem_dgrad_kernel<float, true>", stem_dgrad_kernel<float, true>, grid, block, st, p);
    else timed_launch("argus::stem_dgrad_kernel<float, false>", stem_dgrad_kernel<float, false>, grid, block, st, p);
  }
  return check_launch("stem_dgrad_kernel");
}

}  // namespace argus
