// Device-resident dataset: build one training batch from cropped uint8 frames that already live in
// HBM (argus_amd/resident.py). One launch gathers out[b] = store[index[b]] and blackens the pixels
// the "spaghetti" occluder arcs cover (argus/utils.py:252-275: ImageDraw.arc, fill 0), replacing the
// PNG decode + PIL drawing + pickling of the DataLoader workers.
//
// Arc definition (restated in int64 numpy by tests/arc_reference.py, bit for bit). A
// record is 12 int32: x0, y0, x1, y1, wd, mode, sx, sy, ex, ey, 0, 0 in SOURCE-frame pixels (the
// reference draws on the full frame and crops afterwards); mode 0 nothing / 1 full ellipse / 2 span
// <= 180 / 3 span > 180; (sx, sy), (ex, ey) = round(2^20 (cos, sin)) of the start / end angle, fixed on
// the host. For a pixel (px, py): X = 2 px - (x0 + x1), Y = 2 py - (y0 + y1), A = x1 - x0 + 1,
// B = y1 - y0 + 1.
//   in_ell(X, Y, A, B) = A > 0 && B > 0 && X^2 B^2 + Y^2 A^2 <= A^2 B^2
//   stroke = in_ell(X, Y, A, B) && !in_ell(X, Y, A - 2 wd, B - 2 wd)
//   sector(u, v): c1 = sx v - sy u >= 0, c2 = u ey - v ex >= 0; mode 1 true, 2 c1 && c2, 3 c1 || c2
//   A > 1 && B > 1: covered = stroke && sector(X (B - 1), Y (A - 1))   (PIL's angles are parametric)
//   A == 1 (vertical line, one-pixel box): covered = stroke && Y 2^20 in [lo, hi], the range of
//     (B - 1) sin t the angles sweep: hi = (B - 1) 2^20 if sector(0, 1) else (B - 1) max(sy, ey), lo =
//     -(B - 1) 2^20 if sector(0, -1) else (B - 1) min(sy, ey); B == 1 (horizontal line): lo, hi the same
//     with A - 1 and cos, and covered = stroke && X + 1 >= floor((lo + 2^19) / 2^20) && X <= floor((hi +
//     2^19) / 2^20) (PIL rounds these ends to whole doubled coordinates; a pixel owns [X, X + 2)).
// Integers only. Supported frame: every coordinate in [0, 8192), so |X|, |Y| < 2^14, A, B <= 2^13 and
// every product stays inside 64 bits; a record outside that range (or with x1 < x0, y1 < y0) covers
// nothing.
//
// Pixel-parallel: a thread owns a run of up to 16 consecutive pixels of one row, tests them against
// the image's arcs (staged through LDS once per workgroup, 64 at a time) and writes each output byte
// exactly once - no atomics, no read-modify-write of `out`, so the result does not depend on the arc
// order. Runs start at the 16-byte boundaries of the output row's first channel: a full run whose
// source and destination are both 16-byte aligned moves as one 16-byte load and store per channel,
// anything else (row heads and tails, misaligned planes) byte by byte.
#include "common.h"
#include "internal.h"

namespace argus {

struct ArcRec {
  int x0, y0, x1, y1, wd, mode, sx, sy, ex, ey, pad0, pad1;
};
static_assert(sizeof(ArcRec) == 48, "arc record: 12 int32");

constexpr int kArcChunk = 64;    // records staged in LDS at a time
constexpr int kArcFrame = 8192;  // supported source-frame side

ARGUS_DEV bool arc_in_ell(int X, int Y, int A, int B) {
  if (A <= 0 || B <= 0) return false;
  const uint64_t a2 = (uint64_t)((uint32_t)A * (uint32_t)A), b2 = (uint64_t)((uint32_t)B * (uint32_t)B);
  return (uint64_t)(uint32_t)(X * X) * b2 + (uint64_t)(uint32_t)(Y * Y) * a2 <= a2 * b2;
}

ARGUS_DEV bool arc_sector(int u, int v, const ArcRec& r) {
  const bool c1 = (int64_t)r.sx * v - (int64_t)r.sy * u >= 0;
  const bool c2 = (int64_t)u * r.ey - (int64_t)v * r.ex >= 0;
  return r.mode == 1 || (r.mode == 2 && c1 && c2) || (r.mode == 3 && (c1 || c2));
}

// a degenerate (line) box: is the doubled offset T along the line inside the range of D (cos | sin)
// that the angles sweep; s, e = that component of the end directions. rounded (horizontal lines): PIL
// rounds the two ends to whole doubled coordinates and a pixel owns [T, T + 2)
ARGUS_DEV bool arc_line(int T, int D, int s, int e, bool plus, bool minus, int mode, bool rounded) {
  if (mode == 1) return true;
  if (mode != 2 && mode != 3) return false;
  const int64_t one = (int64_t)1 << 20;
  const int64_t hi = plus ? D * one : (int64_t)D * (s > e ? s : e);
  const int64_t lo = minus ? -D * one : (int64_t)D * (s < e ? s : e);
  if (rounded) {  // floor((v + 2^19) / 2^20): an arithmetic shift floors
    const int64_t rl = (lo + one / 2) >> 20, rh = (hi + one / 2) >> 20;
    return T + 1 >= rl && T <= rh;
  }
  const int64_t t = T * one;
  return t >= lo && t <= hi;
}

ARGUS_DEV bool arc_valid(const ArcRec& r) {
  return r.mode >= 1 && r.mode <= 3 && r.x0 >= 0 && r.y0 >= 0 && r.x1 >= r.x0 && r.y1 >= r.y0 && r.x1 < kArcFrame &&
         r.y1 < kArcFrame;
}

ARGUS_DEV bool arc_covers(int px, int py, const ArcRec& r) {
  const int X = 2 * px - (r.x0 + r.x1), Y = 2 * py - (r.y0 + r.y1);
  const int A = r.x1 - r.x0 + 1, B = r.y1 - r.y0 + 1;
  const int wd = r.wd < 1 ? 1 : (r.wd > kArcFrame ? kArcFrame : r.wd);
  if (!arc_in_ell(X, Y, A, B) || arc_in_ell(X, Y, A - 2 * wd, B - 2 * wd)) return false;
  if (A > 1 && B > 1) return arc_sector(X * (B - 1), Y * (A - 1), r);
  if (A == 1) return arc_line(Y, B - 1, r.sy, r.ey, arc_sector(0, 1, r), arc_sector(0, -1, r), r.mode, false);
  return arc_line(X, A - 1, r.sx, r.ex, arc_sector(1, 0, r), arc_sector(-1, 0, r), r.mode, true);
}

// grid: tiles * n_img workgroups of 256 threads; thread i of an image's tiles owns run (i % segs) of row
// (i / segs); segs = ceil(w / 16) + 1 (the row's head run).
__global__ __launch_bounds__(256) void gather_occlude_kernel(int n_cams, int h, int w, int segs, int tiles,
                                                             const uint8_t* __restrict__ store, int64_t n_samples,
                                                             const int64_t* __restrict__ index,
                                                             const ArcRec* __restrict__ arcs, int n_arcs, int crop_y0,
                                                             int crop_x0, uint8_t* __restrict__ out) {
  __shared__ ArcRec recs[kArcChunk];
  const int64_t img = blockIdx.x / tiles;  // b * n_cams + cam
  const int tile = (int)(blockIdx.x - img * tiles);
  const int64_t b = img / n_cams;
  const int cam = (int)(img - b * n_cams);
  const int64_t hw = (int64_t)h * w;
  int64_t sample = index[b];  // an index outside [0, n_samples) is clamped (the device cannot report it)
  sample = sample < 0 ? 0 : (sample >= n_samples ? n_samples - 1 : sample);
  const uint8_t* src = store + (sample * n_cams + cam) * 3 * hw;
  uint8_t* dst = out + img * 3 * hw;

  const int i = tile * 256 + (int)threadIdx.x;
  const int row = i / segs, seg = i - row * segs;
  // runs of the row: [0, head), [head, head + 16), ... with head = bytes up to dst's next 16-byte boundary
  int xb = 0, xe = 0;
  if (row < h) {
    const int head = (int)((16 - ((reinterpret_cast<uintptr_t>(dst) + (uint64_t)row * w) & 15)) & 15);
    xb = seg == 0 ? 0 : head + (seg - 1) * 16;
    xe = head + seg * 16;
    xb = xb > w ? w : xb;
    xe = xe > w ? w : xe;
  }
  const int len = xe - xb;
  const int py = crop_y0 + row, px0 = crop_x0 + xb;

  unsigned mask = 0;  // bit k: pixel xb + k is covered
  for (int a0 = 0; a0 < n_arcs; a0 += kArcChunk) {
    const int na = n_arcs - a0 < kArcChunk ? n_arcs - a0 : kArcChunk;
    if (a0) __syncthreads();
    {
      const int* g = reinterpret_cast<const int*>(arcs + (img * n_arcs + a0));
      int* l = reinterpret_cast<int*>(recs);
      for (int k = threadIdx.x; k < na * 12; k += 256) l[k] = g[k];
    }
    __syncthreads();
    if (len > 0) {
      for (int a = 0; a < na; ++a) {
        const ArcRec& r = recs[a];
        if (!arc_valid(r) || py < r.y0 || py > r.y1 || px0 + len - 1 < r.x0 || px0 > r.x1) continue;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < len && arc_covers(px0 + k, py, r)) mask |= 1u << k;
      }
    }
  }
  if (len <= 0) return;
  const int64_t off = (int64_t)row * w + xb;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t* s = src + c * hw + off;
    uint8_t* d = dst + c * hw + off;
    if (len == 16 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
      u32x4 v = ld16(s);
      if (mask) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned m4 = (mask >> (4 * j)) & 15u;
          const unsigned keep = ((m4 & 1u) ? 0u : 0xFFu) | ((m4 & 2u) ? 0u : 0xFF00u) | ((m4 & 4u) ? 0u : 0xFF0000u) |
                                ((m4 & 8u) ? 0u : 0xFF000000u);
          v[j] &= keep;
        }
      }
      st16(d, v);
    } else {
      for (int k = 0; k < len; ++k) d[k] = (mask >> k) & 1u ? (uint8_t)0 : s[k];
    }
  }
}

// ---- host: the np.random draws of draw_spaghetti (argus/utils.py:252-275), continued from a
// RandomState's MT19937 state. A Python loop over RandomState.randint / uniform costs about as much per
// B=64 batch as the fused train step; this restates numpy's legacy algorithms (public: MT19937, the
// masked-rejection bounded integers of randint, the 53-bit double of uniform) so the stream is the same.
struct Mt {
  uint32_t* key;
  int pos;
  uint32_t next() {
    if (pos >= 624) {
      for (int i = 0; i < 624; ++i) {
        const uint32_t y = (key[i] & 0x80000000u) | (key[(i + 1) % 624] & 0x7FFFFFFFu);
        key[i] = key[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
      }
      pos = 0;
    }
    uint32_t y = key[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
  }
  // RandomState.randint(lo, hi): lo + a draw in [0, hi - 1 - lo]; no draw when that range is 0
  int bounded(int lo, int hi) {
    const uint32_t rng = (uint32_t)(hi - 1 - lo);
    if (rng == 0) return lo;
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v;
    while ((v = next() & mask) > rng) {}
    return lo + (int)v;
  }
  double uniform(double lo, double hi) {
    const uint32_t a = next() >> 5, b = next() >> 6;
    return lo + (hi - lo) * ((a * 67108864.0 + b) / 9007199254740992.0);
  }
};

}  // namespace argus

using namespace argus;

extern "C" {

int argus_sample_arc_params(uint32_t* mt_key, int* mt_pos, int64_t n_arcs, int src_h, int src_w, double width_lo,
                            double width_hi, int32_t* params) {
  if (!mt_key || !mt_pos || !params || n_arcs < 0 || src_h <= 0 || src_w <= 0 || *mt_pos < 0 || *mt_pos > 624) {
    set_error("sample_arc_params: bad arguments");
    return ARGUS_ERR_ARG;
  }
  Mt mt{mt_key, *mt_pos};
  for (int64_t i = 0; i < n_arcs; ++i) {
    int32_t* p = params + i * 7;
    p[0] = mt.bounded(0, src_w);
    p[1] = mt.bounded(0, src_h);
    p[2] = mt.bounded(p[0], src_w);
    p[3] = mt.bounded(p[1], src_h);
    p[4] = mt.bounded(0, 360);
    p[5] = mt.bounded(0, 360);
    p[6] = (int32_t)mt.uniform(width_lo, width_hi);
  }
  *mt_pos = mt.pos;
  return ARGUS_OK;
}

size_t argus_arc_record_bytes(void) { return sizeof(ArcRec); }

int argus_batch_gather_occlude(int64_t batch, int n_cams, int h, int w, const uint8_t* store, int64_t n_samples,
                               const int64_t* index, const void* arcs, int n_arcs, int crop_y0, int crop_x0,
                               uint8_t* out, argus_stream_t stream) {
  if (batch <= 0 || n_cams <= 0 || h <= 0 || w <= 0 || n_samples <= 0 || !store || !out || !index || n_arcs < 0 ||
      (n_arcs > 0 && !arcs)) {
    set_error("batch_gather_occlude: bad arguments");
    return ARGUS_ERR_ARG;
  }
  if (crop_y0 < 0 || crop_x0 < 0 || (int64_t)crop_y0 + h > kArcFrame || (int64_t)crop_x0 + w > kArcFrame) {
    set_error("batch_gather_occlude: the crop must lie inside an 8192 x 8192 source frame");
    return ARGUS_ERR_SHAPE;
  }
  const int segs = (w + 15) / 16 + 1;  // one more than the full runs: the row's head
  const int64_t tiles = ((int64_t)h * segs + 255) / 256;
  const int64_t blocks = tiles * batch * n_cams;
  if (blocks > 0x7FFFFFFFLL) {
    set_error("batch_gather_occlude: batch too large for one launch");
    return ARGUS_ERR_SHAPE;
  }
  hipLaunchKernelGGL(gather_occlude_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_cams, h, w,
                     segs, (int)tiles, store, n_samples, index, reinterpret_cast<const ArcRec*>(arcs), n_arcs, crop_y0,
                     crop_x0, out);
  return check_launch("batch_gather_occlude");
}

}  // extern "C"
