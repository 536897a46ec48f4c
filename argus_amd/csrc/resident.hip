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
#include "roi_taps.h"

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

// ---- batch build with a region of interest per camera image (argus_batch_gather_resample) -----------------
// out[b][cam] = the region rois[b * n_cams + cam] of the UNCROPPED frame store[index[b]][cam], occluded by its
// arcs in source-frame coordinates, resampled to h x w with the taps of roi_axis (roi_taps.h: the deployed
// filter of argus_frames_resample, tap for tap). A byte is (uint8) rintf(255 px) with
// px = sum_y wy (sum_x wx v / 255.0f), each sum a chain of fmaf from 0 over ascending taps, as roi_pixel's.
//
// A workgroup owns an 8 x 64 output tile of one image, all three channels:
//   1. threads 0 .. 71 build the 8 row and 64 column tap tables in LDS;
//   2. the tile's source footprint (rows lo(first row) .. hi(last row), columns from the 16-pixel boundary at or
//      below lo(first column)) is staged into LDS as uint8 in runs of 16 pixels; then every group of 4 staged
//      pixels is tested against the image's arcs once (records through LDS 64 at a time, the bounding-box
//      rejects of gather_occlude_kernel) and its covered pixels are set to 0 in LDS by the thread that owns it;
//   3. per channel: a horizontal pass (a thread owns one column's taps in registers and every fourth footprint
//      row) writes fp32 sums to LDS, a vertical pass (128 threads, 4 pixels each) makes the bytes; four lanes'
//      words are gathered into one 16-byte store where the output run is whole and aligned.
// The separable order IS the definition's order (the inner sum runs over x), so nothing is approximated. At
// s = r = 4 the footprint has fewer than 7 s + 2 r + 1 = 37 rows and 63 s + 2 r + 1 = 261 columns (+ 15 of
// alignment): 38 rows of 288 bytes per channel. A tap entry whose taps leave that window (no served region; any
// other bit pattern) gets no taps: every LDS and global read stays in bounds, the pixel is unspecified.
// LDS: 32.1 KB footprint + 9.5 KB fp32 rows of one channel + 3 KB records + 3.1 KB taps = 47.7 KB, three
// workgroups a CU.
constexpr int kRrH = 8, kRrW = 64;
constexpr int kRrFH = 38;                                 // footprint rows
constexpr int kRrFP = 288;                                // footprint row pitch, bytes: 18 runs of 16

__global__ __launch_bounds__(256) void gather_resample_kernel(int n_cams, int src_h, int src_w, int h, int w, int tpr,
                                                              int tpi, const uint8_t* __restrict__ store,
                                                              int64_t n_samples, const int64_t* __restrict__ index,
                                                              const float* __restrict__ rois,
                                                              const ArcRec* __restrict__ arcs, int n_arcs,
                                                              uint8_t* __restrict__ out) {
  __shared__ ArcRec recs[kArcChunk];
  __shared__ RoiTaps ty[kRrH], tx[kRrW];
  __shared__ __attribute__((aligned(16))) uint8_t foot[3 * kRrFH * kRrFP + 16];  // + 16: taps of weight 0 past the end
  __shared__ __attribute__((aligned(16))) float hbuf[kRrFH * kRrW];

  const int tid = threadIdx.x;
  const int64_t img = blockIdx.x / tpi;  // b * n_cams + cam
  const int rem = (int)(blockIdx.x - img * tpi);
  const int i0 = (rem / tpr) * kRrH, j0 = (rem % tpr) * kRrW;
  const int nr = min(kRrH, h - i0), nc = min(kRrW, w - j0);
  const int64_t b = img / n_cams;
  const int cam = (int)(img - b * n_cams);
  const int shw = src_h * src_w, ohw = h * w;
  int64_t sample = index[b];  // clamped as gather_occlude_kernel does
  sample = sample < 0 ? 0 : (sample >= n_samples ? n_samples - 1 : sample);
  const uint8_t* src = store + (sample * n_cams + cam) * 3 * (int64_t)shw;
  uint8_t* dst = out + img * 3 * (int64_t)ohw;

  // ---- 1. tap tables ----
  if (tid < kRrH + kRrW) {
    const float* roi = rois + 4 * img;
    const bool isrow = tid < kRrH;
    const int k = isrow ? tid : tid - kRrH;
    RoiTaps& t = isrow ? ty[k] : tx[k];
    if (k < (isrow ? nr : nc)) {
      roi_axis(isrow ? src_h : src_w, isrow ? h : w, roi[isrow ? 0 : 1], roi[isrow ? 2 : 3], (isrow ? i0 : j0) + k, t);
    } else {  // past the image's edge: no taps
#pragma unroll
      for (int q = 0; q < kRoiTaps; ++q) t.w[q] = 0.f;
      t.lo = 0;
      t.cnt = 0;
    }
  }
  __syncthreads();
  // lo and lo + cnt do not decrease along an axis: the first entry starts the footprint, the last one ends it
  const int fy0 = ty[0].lo, fxa = tx[0].lo & ~15;
  const int fh = min(max(ty[nr - 1].lo + ty[nr - 1].cnt - fy0, 0), kRrFH);
  const int fw = min(max(tx[nc - 1].lo + tx[nc - 1].cnt - fxa, 0), kRrFP);
  const int nseg = (fw + 15) >> 4;

  // ---- 2. footprint: 16-byte runs into LDS, then every group of 4 staged pixels against the arcs once ----
  const int nq = 4 * nseg;  // groups of 4 pixels in a footprint row
  for (int u = tid; u < fh * nseg; u += 256) {  // fy0 + fr < src_h: fh ends at a tap
    const int fr = u / nseg, seg = u - fr * nseg;
    const int px0 = fxa + 16 * seg, len = min(16, src_w - px0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* s = src + ((int64_t)c * shw + (fy0 + fr) * src_w + px0);
      u32x4 v = {0u, 0u, 0u, 0u};
      if (len == 16 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        v = ld16(s);
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < len) v[k >> 2] |= (unsigned)s[k] << (8 * (k & 3));
      }
      *reinterpret_cast<u32x4*>(foot + ((c * kRrFH + fr) * kRrFP + 16 * seg)) = v;
    }
  }
  // groups, not runs of 16: at unit scale a tile has about 60 runs but 240 groups, work for all four waves
  for (int a0 = 0; a0 < n_arcs; a0 += kArcChunk) {
    const int na = n_arcs - a0 < kArcChunk ? n_arcs - a0 : kArcChunk;
    if (a0) __syncthreads();
    {
      const int* g = reinterpret_cast<const int*>(arcs + (img * n_arcs + a0));
      int* l = reinterpret_cast<int*>(recs);
      for (int k = tid; k < na * 12; k += 256) l[k] = g[k];
    }
    __syncthreads();  // the records, and (first chunk) the staged footprint
    for (int q = tid; q < fh * nq; q += 256) {
      const int fr = q / nq, qx = q - fr * nq;
      const int py = fy0 + fr, px0 = fxa + 4 * qx, len = min(4, src_w - px0);
      if (len <= 0) continue;
      unsigned m = 0;  // bit k: pixel px0 + k is covered
      for (int a = 0; a < na; ++a) {
        const ArcRec& r = recs[a];
        if (!arc_valid(r) || py < r.y0 || py > r.y1 || px0 + len - 1 < r.x0 || px0 > r.x1) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < len && arc_covers(px0 + k, py, r)) m |= 1u << k;
      }
      if (m) {  // this thread's own words: no other thread touches them
        const unsigned keep = ((m & 1u) ? 0u : 0xFFu) | ((m & 2u) ? 0u : 0xFF00u) | ((m & 4u) ? 0u : 0xFF0000u) |
                              ((m & 8u) ? 0u : 0xFF000000u);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<unsigned*>(foot + ((c * kRrFH + fr) * kRrFP + 4 * qx)) &= keep;
      }
    }
  }

  // ---- 3. per channel: horizontal pass to fp32 rows, vertical pass to bytes ----
  const int lane = tid & 63, wave = tid >> 6;
  float wx[kRoiTaps];
  int relx = tx[lane].lo - fxa, cx = tx[lane].cnt;
  {
    const bool ok = relx >= 0 && relx + cx <= kRrFP;
#pragma unroll
    for (int k = 0; k < kRoiTaps; ++k) wx[k] = ok ? tx[lane].w[k] : 0.f;
    if (!ok) relx = 0, cx = 0;
  }
  int kmax = cx;  // the wave's columns differ by a tap at most: one uniform trip count, weight 0 past a column's own
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, __shfl_xor(kmax, off));
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  const int vi = tid >> 4, vseg = tid & 15;  // vertical pass (tid < 128): output row, run of 4 columns
  int rely = 0, cy = 0;
  if (tid < 128) {
    rely = ty[vi].lo - fy0, cy = ty[vi].cnt;
    if (rely < 0 || rely + cy > kRrFH) rely = 0, cy = 0;
  }
  __syncthreads();  // the footprint is staged

#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const uint8_t* fc = foot + c * kRrFH * kRrFP + relx;
    for (int r = wave; r < fh; r += 4) {
      const uint8_t* p = fc + r * kRrFP;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < kRoiTaps; ++k) {
        if (k >= kmax) break;
        acc = fmaf(wx[k], pixel_f32(p[k]), acc);
      }
      hbuf[r * kRrW + lane] = acc;
    }
    __syncthreads();
    if (tid < 128) {
      float px[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < cy; ++k) {
        const float wy = ty[vi].w[k];
        const float4 hv = *reinterpret_cast<const float4*>(hbuf + (rely + k) * kRrW + 4 * vseg);
        px[0] = fmaf(wy, hv.x, px[0]);
        px[1] = fmaf(wy, hv.y, px[1]);
        px[2] = fmaf(wy, hv.z, px[2]);
        px[3] = fmaf(wy, hv.w, px[3]);
      }
      unsigned v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v |= (unsigned)(int)fminf(fmaxf(rintf(255.0f * px[k]), 0.f), 255.f) << (8 * k);
      const int l4 = lane & ~3;
      const u32x4 q = {(unsigned)__shfl((int)v, l4), (unsigned)__shfl((int)v, l4 + 1), (unsigned)__shfl((int)v, l4 + 2),
                       (unsigned)__shfl((int)v, l4 + 3)};
      if (vi < nr) {
        uint8_t* drow = dst + ((int64_t)c * ohw + (i0 + vi) * w + j0);
        const int jg = 16 * (vseg >> 2);
        if (jg + 16 <= nc && (reinterpret_cast<uintptr_t>(drow + jg) & 15) == 0) {
          if ((lane & 3) == 0) st16(drow + jg, q);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (4 * vseg + k < nc) drow[4 * vseg + k] = (uint8_t)(v >> (8 * k));
        }
      }
    }
    if (c < 2) __syncthreads();  // hbuf is rewritten
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

int argus_batch_gather_resample(int64_t batch, int n_cams, int src_h, int src_w, int h, int w, const uint8_t* store,
                                int64_t n_samples, const int64_t* index, const float* rois, const void* arcs,
                                int n_arcs, uint8_t* out, argus_stream_t stream) {
  const char* null_arg = !store ? "store" : !index ? "index" : !rois ? "rois" : !out ? "out"
                         : (n_arcs > 0 && !arcs) ? "arcs" : nullptr;
  if (null_arg) {
    set_error(std::string("batch_gather_resample: ") + null_arg + " is null");
    return ARGUS_ERR_ARG;
  }
  const char* size_arg = batch <= 0 ? "batch" : n_cams <= 0 ? "n_cams" : n_samples <= 0 ? "n_samples"
                         : n_arcs < 0 ? "n_arcs" : src_h <= 0 ? "src_h" : src_w <= 0 ? "src_w" : nullptr;
  if (size_arg) {
    set_error(std::string("batch_gather_resample: ") + size_arg + " must be positive (n_arcs: not negative)");
    return ARGUS_ERR_ARG;
  }
  if (h < 8 || w < 8) {
    set_error("batch_gather_resample: h and w must be at least 8");
    return ARGUS_ERR_SHAPE;
  }
  if (src_h > kArcFrame || src_w > kArcFrame) {
    set_error("batch_gather_resample: src_h and src_w must not exceed 8192");
    return ARGUS_ERR_SHAPE;
  }
  if (h > src_h || w > src_w) {
    set_error("batch_gather_resample: h > src_h or w > src_w (the output is at most the frame: scale >= 1 somewhere)");
    return ARGUS_ERR_SHAPE;
  }
  // the kernel indexes one image (3 planes) with 32-bit offsets
  if (3 * (int64_t)src_h * src_w >= (1LL << 31) || 3 * (int64_t)h * w >= (1LL << 31)) {
    set_error("batch_gather_resample: one image's offsets (3 * src_h * src_w) must fit 31 bits");
    return ARGUS_ERR_SHAPE;
  }
  const int tpr = (w + kRrW - 1) / kRrW, tpi = ((h + kRrH - 1) / kRrH) * tpr;
  const int64_t blocks = (int64_t)tpi * batch * n_cams;
  if (blocks > 0x7FFFFFFFLL || batch > 0x7FFFFFFFLL) {
    set_error("batch_gather_resample: batch too large for one launch");
    return ARGUS_ERR_SHAPE;
  }
  {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(store), o0 = reinterpret_cast<uintptr_t>(out);
    const uint64_t sb = (uint64_t)n_samples * n_cams * 3 * src_h * src_w, ob = (uint64_t)batch * n_cams * 3 * h * w;
    if (s0 < o0 + ob && o0 < s0 + sb) {
      set_error("batch_gather_resample: out overlaps store");
      return ARGUS_ERR_ARG;
    }
  }
  hipLaunchKernelGGL(gather_resample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_cams, src_h,
                     src_w, h, w, tpr, tpi, store, n_samples, index, rois, reinterpret_cast<const ArcRec*>(arcs), n_arcs,
                     out);
  return check_launch("batch_gather_resample");
}

}  // extern "C"
