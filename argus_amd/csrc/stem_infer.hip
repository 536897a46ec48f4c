// Frozen-inference stem in one launch: camera frames -> conv1 (7x7, stride 2, pad 3, 3 -> 64) -> bn1.eval()
// -> ReLU -> max-pool 3x3 / stride 2 / pad 1 (torchvision resnet.py conv1 / bn1 / relu / maxpool, reached from
// argus/models.py:84), replacing argus_images[_u8]_to_nhwc4 + argus_conv_fwd (stem) + argus_maxpool_fwd of
// the frozen session and the host-side transpose + crop of the deployment loop (argus/validate_real.py:58-75).
//
// A workgroup owns a 3 x 15 tile of the pooled output. Its 8 x 32 conv tile (stem_tile.h: stem_fwd_kernel's
// patch, filter copy and MFMA loop) has origin (2*ph0 - 1, 2*pw0 - 1); the pooled tile needs its first 7 rows
// and 31 columns. The frames are read straight from the caller's tensor through argus_frame_src (any strides,
// uint8 or fp32, a crop origin) into the NHWC4 LDS patch as from_f32<T>(pixel_f32(v)): the bits
// argus_images_to_nhwc4 writes to x0. scale / shift are applied to the fp32 accumulator, conv positions outside
// the conv output are set to 0 after the ReLU (exact: every pool window holds a valid value >= 0), the tile is
// staged in LDS as T and the max is taken over T values: rounding is monotone, so this is the fp32 max rounded
// once. Neither x0 nor the conv output y0 (the largest tensor of the forward) touches memory.
//
// 256 threads, 41.5 KB LDS (stem_fwd_kernel's). No statistics, no argmax: inference only.
#include "internal.h"
#include "ktimer.h"
#include "stem_tile.h"

namespace argus {

namespace {
constexpr int kPTH = 3, kPTW = 15;  // pooled tile: rows 0..6 x columns 0..30 of the 8 x 32 conv tile
}

template <typename T>
struct StemInferParams {
  const void* base;   // frames (argus_frame_src), already advanced by the crop origin
  long long stride_img;
  int stride_c, stride_y, stride_x;  // elements; within one image every offset fits 31 bits (checked)
  const T* w;         // w_fwd of the stem: [64][8][8][4]
  const float* scale; // bn1.eval() coefficients (argus_bn_eval_coeffs)
  const float* shift;
  T* out;             // (n, H2, W2, 64)
  int n, H, W, H1, W1, H2, W2, tpr, tpi;
};

template <typename T, typename In>
__global__ __launch_bounds__(256, 3) void stem_infer_kernel(const StemInferParams<T> p) {
  static_assert(sizeof(T) == 2, "stem_infer_kernel: bf16 or fp16");
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsB];
  uint2* patch = reinterpret_cast<uint2*>(lds);
  T* wl = reinterpret_cast<T*>(lds + kPatchB);

  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int img = tile / p.tpi, rem = tile - img * p.tpi;
  const int ph0 = (rem / p.tpr) * kPTH, pw0 = (rem % p.tpr) * kPTW;
  const int oh0 = 2 * ph0 - 1, ow0 = 2 * pw0 - 1;  // conv tile origin (row / column -1: pool padding)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- stage the input patch (zero outside the image) and the 64 x 224 filter ----
  const In* X = reinterpret_cast<const In*>(p.base) + (long long)img * p.stride_img;
  const int ih0 = 2 * oh0 - 3, iw0 = 2 * ow0 - 3;
  In pv[kPatchPT][3];
  bool pok[kPatchPT];
#pragma unroll
  for (int i = 0; i < kPatchPT; ++i) {
    const int q = tid + 256 * i;
    const int pr = q / kPC, pc = q - pr * kPC;
    const int ih = ih0 + pr, iw = iw0 + pc;
    pok[i] = q < kPR * kPC && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
    const int off = pok[i] ? ih * p.stride_y + iw * p.stride_x : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) pv[i][c] = X[off + c * p.stride_c];
  }
  u32x4 wv[7];
  stem_w_load(p.w, tid, wv);
#pragma unroll
  for (int i = 0; i < kPatchPT; ++i) {
    const int q = tid + 256 * i;
    const T v[4] = {from_f32<T>(pixel_f32(pv[i][0])), from_f32<T>(pixel_f32(pv[i][1])),
                    from_f32<T>(pixel_f32(pv[i][2])), from_f32<T>(0.f)};
    if (q < kPR * kPC) patch[q] = pok[i] ? __builtin_bit_cast(uint2, v) : make_uint2(0u, 0u);
  }
  stem_w_store(wl, tid, wv);
  __syncthreads();

  f32x4 acc[4][4];
  stem_tile_mma<T>(lds, wl, wave, lane, acc);
  __syncthreads();  // LDS is reused below

  // ---- bn1 + ReLU on the fp32 accumulator, 0 outside the conv output, one rounding to T, into LDS ----
  const int g = lane >> 4, i16 = lane & 15;
  T* Cs = reinterpret_cast<T*>(lds);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const float sc = p.scale[ni * 16 + i16], sh = p.shift[ni * 16 + i16];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wave * 64 + mi * 16 + g * 4 + r;
        const int oh = oh0 + (m >> 5), ow = ow0 + (m & 31);
        const bool in = (unsigned)oh < (unsigned)p.H1 && (unsigned)ow < (unsigned)p.W1;
        const float z = in ? fmaxf(fmaf(acc[mi][ni][r], sc, sh), 0.f) : 0.f;
        Cs[m * kLD + ni * 16 + i16] = from_f32<T>(z);
      }
  }
  __syncthreads();

  // ---- 3x3 / 2 max over the staged tile: one thread per (pooled pixel, 16-byte channel chunk) ----
  for (int it = tid; it < kPTH * kPTW * 8; it += 256) {
    const int px = it >> 3, c = it & 7;
    const int pr = px / kPTW, pc = px - pr * kPTW;
    const int ph = ph0 + pr, pw = pw0 + pc;
    if (ph >= p.H2 || pw >= p.W2) continue;
    float best[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) best[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        float v[8];
        ChunkCvt<T>::unpack(*reinterpret_cast<const u32x4*>(Cs + ((2 * pr + r) * kTW + 2 * pc + t) * kLD + c * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = fmaxf(best[j], v[j]);
      }
    st16(p.out + (((size_t)img * p.H2 + ph) * p.W2 + pw) * 64 + c * 8, ChunkCvt<T>::pack(best));
  }
}

template <typename T, typename In>
static int stem_infer_run(const StemInferParams<T>& p, hipStream_t st, const char* name) {
  timed_launch(name, stem_infer_kernel<T, In>, dim3(p.n * p.tpi), dim3(256), st, p);
  return check_launch("stem_infer_kernel");
}

}  // namespace argus

using namespace argus;

extern "C" int argus_stem_infer(int out_dtype, int n_img, int h, int w, int k, const argus_frame_src* src,
                                const void* w_fwd, const float* scale, const float* shift, void* out,
                                argus_stream_t stream) {
  const int dtype = out_dtype;  // T: what the patch, the filter copy and `out` hold
  if (dtype != ARGUS_BF16 && dtype != ARGUS_F16) {
    set_error("stem_infer: dtype must be ARGUS_BF16 or ARGUS_F16 (the fp32 stem runs on argus_conv_fwd)");
    return ARGUS_ERR_ARG;
  }
  if (!src || !src->base || !w_fwd || !scale || !shift || !out) {
    set_error("stem_infer: null argument");
    return ARGUS_ERR_ARG;
  }
  if (n_img <= 0 || h < 8 || w < 8 || k != 64) {
    set_error("stem_infer: needs n_img > 0, h and w >= 8, k == 64");
    return ARGUS_ERR_ARG;
  }
  if (src->in_dtype != 0 && src->in_dtype != 1) {
    set_error("stem_infer: in_dtype must be 0 (uint8) or 1 (fp32)");
    return ARGUS_ERR_ARG;
  }
  if (src->y0 < 0 || src->x0 < 0 || src->src_h <= 0 || src->src_w <= 0 || (int64_t)src->y0 + h > src->src_h ||
      (int64_t)src->x0 + w > src->src_w) {
    set_error("stem_infer: the crop (y0 + h, x0 + w) leaves the source frame");
    return ARGUS_ERR_ARG;
  }
  // the kernel indexes one image with 32-bit element offsets from its crop origin
  const int64_t span = 2 * src->stride_c + (int64_t)(h - 1) * src->stride_y + (int64_t)(w - 1) * src->stride_x;
  if (src->stride_img < 0 || src->stride_c < 0 || src->stride_y < 0 || src->stride_x < 0 ||
      src->stride_c >= (1LL << 30) || src->stride_y >= (1LL << 30) || src->stride_x >= (1LL << 30) ||
      span >= (1LL << 31)) {
    set_error("stem_infer: frame strides must be >= 0 and one image's offsets must fit 31 bits");
    return ARGUS_ERR_ARG;
  }
  const int h1 = (h - 1) / 2 + 1, w1 = (w - 1) / 2 + 1;
  const int h2 = (h1 - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1;
  const int tpr = (w2 + kPTW - 1) / kPTW, tpi = ((h2 + kPTH - 1) / kPTH) * tpr;
  if ((int64_t)n_img * tpi >= (1LL << 31)) {
    set_error("stem_infer: too many tiles");
    return ARGUS_ERR_SHAPE;
  }
  const size_t esz = src->in_dtype == 0 ? 1 : 4;
  const char* base = reinterpret_cast<const char*>(src->base) +
                     ((int64_t)src->y0 * src->stride_y + (int64_t)src->x0 * src->stride_x) * (int64_t)esz;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](auto tag) {
    typedef decltype(tag) T;
    StemInferParams<T> p;
    p.base = base;
    p.stride_img = src->stride_img;
    p.stride_c = (int)src->stride_c; p.stride_y = (int)src->stride_y; p.stride_x = (int)src->stride_x;
    p.w = reinterpret_cast<const T*>(w_fwd);
    p.scale = scale; p.shift = shift;
    p.out = reinterpret_cast<T*>(out);
    p.n = n_img; p.H = h; p.W = w; p.H1 = h1; p.W1 = w1; p.H2 = h2; p.W2 = w2; p.tpr = tpr; p.tpi = tpi;
    const bool f = sizeof(T) == 2 && dtype == ARGUS_F16;
    if (src->in_dtype == 0)
      return stem_infer_run<T, uint8_t>(p, st, f ? "argus::stem_infer_kernel<_Float16, unsigned char>"
                                                 : "argus::stem_infer_kernel<__bf16, unsigned char>");
    return stem_infer_run<T, float>(p, st, f ? "argus::stem_infer_kernel<_Float16, float>"
                                             : "argus::stem_infer_kernel<__bf16, float>");
  };
  return dtype == ARGUS_F16 ? run(f16{}) : run(bf16{});
}
