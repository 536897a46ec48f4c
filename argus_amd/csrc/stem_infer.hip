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
//
// Below it: the region of interest. stem_infer_roi_kernel is the same launch with every patch pixel resampled
// from a per-image region read from device memory; frames_resample_kernel writes those pixels as the NHWC4 tensor.
#include "internal.h"
#include "ktimer.h"
#include "roi_taps.h"
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

// ---- region of interest: the frames resampled to (H, W) on the way into the patch -------------------------
// Per image a region (y0, x0, height, width) in source pixels, read from device memory by every launch, is
// resampled to the network's H x W with the antialiased triangle filter of PIL / F.interpolate(mode="bilinear",
// antialias=True, align_corners=False). Per axis (source length S, output length n, origin o, extent e; pixel j
// covers [j, j + 1)): s = e / n, r = max(s, 1), c_i = o + (i + 0.5) s, taps j from max(0, floor(c_i - r + 0.5))
// to min(S, floor(c_i + r + 0.5)) - 1 with t_ij = max(0, 1 - |j + 0.5 - c_i| / r), w_ij = t_ij / sum_j t_ij. A
// pixel is sum_y wy (sum_x wx pixel_f32(v)) in fp32, taps ascending, then from_f32<T> once. Both kernels below
// build the per-axis taps of their tile in LDS with roi_axis and evaluate pixels with roi_pixel: equal bits.
//
// Direct 2-D taps (at most 9 x 9, the served 1/4 <= s <= 4), no separable pass: at unit scale every pixel has
// one tap and the kernel is stem_infer_kernel plus the tap tables.
// kRoiTaps, RoiTaps and roi_axis live in roi_taps.h (shared with resident.hip).

// X: one image; offsets fit 31 bits over the whole source frame (checked by the callers' entry points)
template <typename In>
ARGUS_DEV void roi_pixel(const In* X, int stride_c, int stride_y, int stride_x, const RoiTaps& ty, const RoiTaps& tx,
                         float (&px)[3]) {
  px[0] = px[1] = px[2] = 0.f;
  const int ny = ty.cnt, nx = tx.cnt;
  const int col = tx.lo * stride_x;
  // loops over the taps that exist: a row's 9 taps unrolled behind `kx < nx` guards (weight and value 0 beyond
  // nx, the same bits) measured slower at every scale, 13.3 -> 20.6 us at unit scale, 48 -> 55 us at 2.9x
  for (int ky = 0; ky < ny; ++ky) {
    const In* row = X + ((ty.lo + ky) * stride_y + col);
    float r[3] = {0.f, 0.f, 0.f};
    for (int kx = 0; kx < nx; ++kx) {
      const float wx = tx.w[kx];
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = fmaf(wx, pixel_f32(row[kx * stride_x + c * stride_c]), r[c]);
    }
    const float wy = ty.w[ky];
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = fmaf(wy, r[c], px[c]);
  }
}

struct RoiSrc {
  const void* base;
  long long stride_img;
  int stride_c, stride_y, stride_x, src_h, src_w;
  const float* rois;  // [n][4] = (y0, x0, height, width), device memory
};

// taps of output rows i0 .. i0 + nr - 1 (into ty) and columns j0 .. j0 + nc - 1 (into tx) of image img
ARGUS_DEV void roi_tile_taps(const RoiSrc& s, int img, int H, int W, int i0, int nr, int j0, int nc, int tid,
                             RoiTaps* ty, RoiTaps* tx) {
  if (tid < nr + nc) {
    const float* roi = s.rois + 4 * (size_t)img;
    const bool isrow = tid < nr;
    const int k = isrow ? tid : tid - nr;
    roi_axis(isrow ? s.src_h : s.src_w, isrow ? H : W, roi[isrow ? 0 : 1], roi[isrow ? 2 : 3],
             (isrow ? i0 : j0) + k, isrow ? ty[k] : tx[k]);
  }
}

// argus_stem_infer_roi: stem_infer_kernel with every patch pixel from roi_pixel. From the filter copy on, the
// statements are stem_infer_kernel's (kept apart so that kernel's code stays as it was measured).
template <typename T, typename In>
__global__ __launch_bounds__(256, 3) void stem_infer_roi_kernel(const StemInferParams<T> p, const RoiSrc s) {
  static_assert(sizeof(T) == 2, "stem_infer_roi_kernel: bf16 or fp16");
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsB];
  __shared__ RoiTaps ty[kPR], tx[kPC];
  uint2* patch = reinterpret_cast<uint2*>(lds);
  T* wl = reinterpret_cast<T*>(lds + kPatchB);

  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int img = tile / p.tpi, rem = tile - img * p.tpi;
  const int ph0 = (rem / p.tpr) * kPTH, pw0 = (rem % p.tpr) * kPTW;
  const int oh0 = 2 * ph0 - 1, ow0 = 2 * pw0 - 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const In* X = reinterpret_cast<const In*>(s.base) + (long long)img * s.stride_img;
  const int ih0 = 2 * oh0 - 3, iw0 = 2 * ow0 - 3;
  roi_tile_taps(s, img, p.H, p.W, ih0, kPR, iw0, kPC, tid, ty, tx);
  u32x4 wv[7];
  stem_w_load(p.w, tid, wv);
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < kPatchPT; ++i) {
    const int q = tid + 256 * i;
    if (q >= kPR * kPC) break;
    const int pr = q / kPC, pc = q - pr * kPC;
    uint2 out = make_uint2(0u, 0u);
    if ((unsigned)(ih0 + pr) < (unsigned)p.H && (unsigned)(iw0 + pc) < (unsigned)p.W) {
      float px[3];
      roi_pixel(X, s.stride_c, s.stride_y, s.stride_x, ty[pr], tx[pc], px);
      const T v[4] = {from_f32<T>(px[0]), from_f32<T>(px[1]), from_f32<T>(px[2]), from_f32<T>(0.f)};
      out = __builtin_bit_cast(uint2, v);
    }
    patch[q] = out;
  }
  stem_w_store(wl, tid, wv);
  __syncthreads();

  f32x4 acc[4][4];
  stem_tile_mma<T>(lds, wl, wave, lane, acc);
  __syncthreads();  // LDS is reused below

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

// argus_frames_resample: the same pixels as the (n, H, W, 4) tensor argus_images_to_nhwc4 would write. A
// workgroup owns 8 rows x 32 columns: one pixel a thread, 256-byte row segments.
constexpr int kRsH = 8, kRsW = 32;

template <typename T, typename In>
__global__ __launch_bounds__(256) void frames_resample_kernel(const RoiSrc s, T* x0, int H, int W, int tpr, int tpi) {
  static_assert(sizeof(T) == 2, "frames_resample_kernel: bf16 or fp16");
  __shared__ RoiTaps ty[kRsH], tx[kRsW];
  const int tile = blockIdx.x;
  const int img = tile / tpi, rem = tile - img * tpi;
  const int i0 = (rem / tpr) * kRsH, j0 = (rem % tpr) * kRsW;
  const int tid = threadIdx.x, pr = tid / kRsW, pc = tid % kRsW;
  roi_tile_taps(s, img, H, W, i0, kRsH, j0, kRsW, tid, ty, tx);
  __syncthreads();
  if (i0 + pr >= H || j0 + pc >= W) return;
  const In* X = reinterpret_cast<const In*>(s.base) + (long long)img * s.stride_img;
  float px[3];
  roi_pixel(X, s.stride_c, s.stride_y, s.stride_x, ty[pr], tx[pc], px);
  const T v[4] = {from_f32<T>(px[0]), from_f32<T>(px[1]), from_f32<T>(px[2]), from_f32<T>(0.f)};
  *reinterpret_cast<uint2*>(x0 + (((size_t)img * H + i0 + pr) * W + j0 + pc) * 4) = __builtin_bit_cast(uint2, v);
}

// The checks argus_stem_infer_roi and argus_frames_resample share (argus_stem_infer's, with the whole source
// frame in place of the crop); fills s.
static int roi_check(const char* who, int dtype, int n_img, int h, int w, const argus_frame_src* src,
                     const float* rois, bool others_null, RoiSrc& s) {
  const std::string me(who);
  if (dtype != ARGUS_BF16 && dtype != ARGUS_F16) {
    set_error(me + ": dtype must be ARGUS_BF16 or ARGUS_F16");
    return ARGUS_ERR_ARG;
  }
  if (!src || !src->base || !rois || others_null) {
    set_error(me + ": null argument");
    return ARGUS_ERR_ARG;
  }
  if (n_img <= 0 || h < 8 || w < 8) {
    set_error(me + ": needs n_img > 0, h and w >= 8");
    return ARGUS_ERR_ARG;
  }
  if (src->in_dtype != 0 && src->in_dtype != 1) {
    set_error(me + ": in_dtype must be 0 (uint8) or 1 (fp32)");
    return ARGUS_ERR_ARG;
  }
  if (src->y0 != 0 || src->x0 != 0 || src->src_h <= 0 || src->src_w <= 0) {
    set_error(me + ": needs src_h and src_w > 0 and y0 = x0 = 0 (the region of interest holds the origin)");
    return ARGUS_ERR_ARG;
  }
  // the kernels index one image with 32-bit element offsets over the whole source frame
  const int64_t span = 2 * src->stride_c + (int64_t)(src->src_h - 1) * src->stride_y +
                       (int64_t)(src->src_w - 1) * src->stride_x;
  if (src->stride_img < 0 || src->stride_c < 0 || src->stride_y < 0 || src->stride_x < 0 ||
      src->stride_c >= (1LL << 30) || src->stride_y >= (1LL << 30) || src->stride_x >= (1LL << 30) ||
      span >= (1LL << 31)) {
    set_error(me + ": frame strides must be >= 0 and one image's offsets must fit 31 bits");
    return ARGUS_ERR_ARG;
  }
  s.base = src->base;
  s.stride_img = src->stride_img;
  s.stride_c = (int)src->stride_c; s.stride_y = (int)src->stride_y; s.stride_x = (int)src->stride_x;
  s.src_h = src->src_h; s.src_w = src->src_w;
  s.rois = rois;
  return ARGUS_OK;
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

extern "C" int argus_frames_resample(int out_dtype, int n_img, int h, int w, const argus_frame_src* src,
                                     const float* rois, void* x0, argus_stream_t stream) {
  RoiSrc s;
  if (int rc = roi_check("frames_resample", out_dtype, n_img, h, w, src, rois, !x0, s)) return rc;
  const int tpr = (w + kRsW - 1) / kRsW, tpi = ((h + kRsH - 1) / kRsH) * tpr;
  if ((int64_t)n_img * tpi >= (1LL << 31)) {
    set_error("frames_resample: too many tiles");
    return ARGUS_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool u8 = src->in_dtype == 0;
  auto run = [&](auto tag, const char* nu8, const char* nf32) {
    typedef decltype(tag) T;
    T* out = reinterpret_cast<T*>(x0);
    if (u8)
      timed_launch(nu8, frames_resample_kernel<T, uint8_t>, dim3(n_img * tpi), dim3(256), st, s, out, h, w, tpr, tpi);
    else
      timed_launch(nf32, frames_resample_kernel<T, float>, dim3(n_img * tpi), dim3(256), st, s, out, h, w, tpr, tpi);
    return check_launch("frames_resample_kernel");
  };
  return out_dtype == ARGUS_F16 ? run(f16{}, "argus::frames_resample_kernel<_Float16, unsigned char>",
                                      "argus::frames_resample_kernel<_Float16, float>")
                                : run(bf16{}, "argus::frames_resample_kernel<__bf16, unsigned char>",
                                      "argus::frames_resample_kernel<__bf16, float>");
}

extern "C" int argus_stem_infer_roi(int out_dtype, int n_img, int h, int w, int k, const argus_frame_src* src,
                                    const float* rois, const void* w_fwd, const float* scale, const float* shift,
                                    void* out, argus_stream_t stream) {
  RoiSrc s;
  if (int rc = roi_check("stem_infer_roi", out_dtype, n_img, h, w, src, rois, !w_fwd || !scale || !shift || !out, s))
    return rc;
  if (k != 64) {
    set_error("stem_infer_roi: needs k == 64");
    return ARGUS_ERR_ARG;
  }
  const int h1 = (h - 1) / 2 + 1, w1 = (w - 1) / 2 + 1;
  const int h2 = (h1 - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1;
  const int tpr = (w2 + kPTW - 1) / kPTW, tpi = ((h2 + kPTH - 1) / kPTH) * tpr;
  if ((int64_t)n_img * tpi >= (1LL << 31)) {
    set_error("stem_infer_roi: too many tiles");
    return ARGUS_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool u8 = src->in_dtype == 0;
  auto run = [&](auto tag, const char* nu8, const char* nf32) {
    typedef decltype(tag) T;
    StemInferParams<T> p;
    p.base = nullptr;  // the frames are in s
    p.stride_img = 0;
    p.stride_c = p.stride_y = p.stride_x = 0;
    p.w = reinterpret_cast<const T*>(w_fwd);
    p.scale = scale; p.shift = shift;
    p.out = reinterpret_cast<T*>(out);
    p.n = n_img; p.H = h; p.W = w; p.H1 = h1; p.W1 = w1; p.H2 = h2; p.W2 = w2; p.tpr = tpr; p.tpi = tpi;
    if (u8)
      timed_launch(nu8, stem_infer_roi_kernel<T, uint8_t>, dim3(p.n * p.tpi), dim3(256), st, p, s);
    else
      timed_launch(nf32, stem_infer_roi_kernel<T, float>, dim3(p.n * p.tpi), dim3(256), st, p, s);
    return check_launch("stem_infer_roi_kernel");
  };
  return out_dtype == ARGUS_F16 ? run(f16{}, "argus::stem_infer_roi_kernel<_Float16, unsigned char>",
                                      "argus::stem_infer_roi_kernel<_Float16, float>")
                                : run(bf16{}, "argus::stem_infer_roi_kernel<__bf16, unsigned char>",
                                      "argus::stem_infer_roi_kernel<__bf16, float>");
}
