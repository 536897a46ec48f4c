// Closed-loop tracking: the region of interest the NEXT replay resamples, from the pose THIS replay produced
// (argus_roi_from_pose; argus_amd/track.py). The same launch aims the resident loader's training
// regions at the labelled cube. tests/track_reference.py restates the definition in fp64, step for step.
//
// Image i = b * n_cams + c. Pose [t(3), qx, qy, qz, qw] (argus_se3_exp's layout), camera [R row-major (9), t (3),
// fx, fy, cx, cy]: Y = R X + t with +x right, +y down, +z forward, pixel (u, v) = (fx Yx / Yz + cx,
// fy Yy / Yz + cy), v the row.
//   1. invalid if a pose value is non-finite or n2 = |q|^2 is 0 or non-finite; q <- q / sqrt(n2)
//   2. corners X_k = t + R(q) (+-ax, +-ay, +-az), Y_k = Rc X_k + tc; invalid if a Y_k is non-finite or Y_k.z < z_near
//   3. [v_min, v_max], [u_min, u_max] over the corners; c = the midpoints; sigma = margin max((v_max - v_min) / h,
//      (u_max - u_min) / w); invalid if sigma or c is non-finite
//   4. jitter (js, jy, jx): sigma <- sigma exp(js); cy += jy sigma h; cx += jx sigma w
//   5. smooth < 1: with p = the region at the start of the launch, sigma_p = p.height / h, c_p = p.origin +
//      p.extent / 2: sigma <- sigma_p + smooth (sigma - sigma_p), c <- c_p + smooth (c - c_p)
//      (a non-finite jitter or previous region makes sigma or c non-finite here: invalid as in step 3)
//   6. sigma clamped to [max(scale_lo, 1/4), min(scale_hi, 4, Hs / h, Ws / w)] (the upper bound wins);
//      e = min(sigma n, S) clamped to [n / 4, min(4 n, S)] per axis; o = clamp(c - e / 2, 0, S - e), one fp32 step
//      down if o + e > S in float64 (check_roi's arithmetic), then max(o, 0): sample_rois' closing guard
//   7. an invalid image gets home[i]
//   8. valid[i] = 1 / 0; used[i] = the region at the start of the launch
//
// Eight lanes serve an image, one corner each; the four ranges and the validity meet in three xor-shuffle steps
// that never leave the group of eight (no LDS, no atomics, no order that could vary: bit-reproducible). Every
// lane of a group loads the same pose and camera words (one broadcast request each), lane 0 also the previous and
// the home region, all issued before the first use. Lane 0 finishes steps 3-8 and writes the region as one 16-byte
// store. A 256-thread workgroup serves 32 images: the deployed session's batch * n_cams <= 16 is one workgroup,
// half of it idle, at the end of a dependent chain; the arithmetic of one corner is the critical path.
//
// Memory safety of the consumer (argus_stem_infer_roi reads whatever this writes): a written region is either
// home[i] (validated by the caller) or passes step 6, whose clamps see finite values only: the pose cannot steer
// it outside check_roi's domain, whatever its bits.
#include "common.h"
#include "internal.h"

namespace argus {

constexpr int kTrackLanes = 8;                       // lanes per image: the cube's corners
constexpr int kTrackImages = 256 / kTrackLanes;      // images per workgroup

struct TrackParams {
  float ax, ay, az, margin, lo, hi, z_near, smooth;  // lo, hi: step 6's bounds on sigma, already combined
  int n_cams, frame_h, frame_w, h, w;
};

// a bit test: no comparison a compiler may fold under a finite-math assumption
ARGUS_DEV bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// steps 6's per-axis end: extent and origin of one axis. sigma, c finite.
ARGUS_DEV void track_axis(float sigma, float c, int n, int S, float& o, float& e) {
  const float fn = (float)n, fS = (float)S;
  e = fminf(sigma * fn, fS);
  e = fminf(fmaxf(e, 0.25f * fn), fminf(4.f * fn, fS));
  o = fminf(fmaxf(c - 0.5f * e, 0.f), fS - e);
  if ((double)o + (double)e > (double)S) o = __uint_as_float(__float_as_uint(o) - 1u);  // o > 0 here: e <= S
  o = fmaxf(o, 0.f);
}

__global__ __launch_bounds__(256) void roi_from_pose_kernel(TrackParams P, int64_t n_img, const float* __restrict__ poses,
                                                            int64_t n_poses, const int64_t* __restrict__ index,
                                                            const float* __restrict__ cameras,
                                                            const float* __restrict__ jitter,
                                                            const float* __restrict__ home, float* rois,
                                                            float* __restrict__ used, int32_t* __restrict__ valid) {
  const int k = threadIdx.x & (kTrackLanes - 1);
  const int64_t slot = (int64_t)blockIdx.x * kTrackImages + (threadIdx.x >> 3);
  const bool live = slot < n_img;
  const int64_t i = live ? slot : n_img - 1;  // idle groups compute the last image again and store nothing
  const int64_t b = i / P.n_cams;
  const int cam = (int)(i - b * P.n_cams);
  int64_t row = b;
  if (index) {  // clamped as argus_batch_gather_resample clamps it
    row = index[b];
    row = row < 0 ? 0 : (row >= n_poses ? n_poses - 1 : row);
  }
  // ---- every load of the launch, before the first use ----
  const float* pp = poses + row * 7;
  float p[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) p[j] = pp[j];
  const float4* cp = reinterpret_cast<const float4*>(cameras + (int64_t)cam * 16);
  const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];  // R00 R01 R02 R10 | R11 R12 R20 R21 | R22 tx ty tz | fx fy cx cy
  float4 prev = {0.f, 0.f, 0.f, 0.f}, hm = prev;
  float js = 0.f, jy = 0.f, jx = 0.f;
  if (k == 0) {
    prev = *reinterpret_cast<const float4*>(rois + 4 * i);
    hm = *reinterpret_cast<const float4*>(home + 4 * i);
    if (jitter) js = jitter[3 * i], jy = jitter[3 * i + 1], jx = jitter[3 * i + 2];
  }

  // ---- 1. the pose ----
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; ++j) ok = ok && finite_f32(p[j]);
  const float n2 = p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6];
  ok = ok && finite_f32(n2) && n2 > 0.f;
  const float inv = 1.f / sqrtf(ok ? n2 : 1.f);
  const float qx = p[3] * inv, qy = p[4] * inv, qz = p[5] * inv, qw = p[6] * inv;
  // ---- 2. this lane's corner ----
  const float sx = (k & 1) ? P.ax : -P.ax, sy = (k & 2) ? P.ay : -P.ay, sz = (k & 4) ? P.az : -P.az;
  const float X0 = p[0] + ((1.f - 2.f * (qy * qy + qz * qz)) * sx + 2.f * (qx * qy - qz * qw) * sy + 2.f * (qx * qz + qy * qw) * sz);
  const float X1 = p[1] + (2.f * (qx * qy + qz * qw) * sx + (1.f - 2.f * (qx * qx + qz * qz)) * sy + 2.f * (qy * qz - qx * qw) * sz);
  const float X2 = p[2] + (2.f * (qx * qz - qy * qw) * sx + 2.f * (qy * qz + qx * qw) * sy + (1.f - 2.f * (qx * qx + qy * qy)) * sz);
  const float Yx = c0.x * X0 + c0.y * X1 + c0.z * X2 + c2.y;
  const float Yy = c0.w * X0 + c1.x * X1 + c1.y * X2 + c2.z;
  const float Yz = c1.z * X0 + c1.w * X1 + c2.x * X2 + c2.w;
  ok = ok && finite_f32(Yx) && finite_f32(Yy) && finite_f32(Yz) && !(Yz < P.z_near);
  // ---- 3. project; ranges over the eight lanes ----
  const float rz = 1.f / (ok ? Yz : 1.f);
  const float u = c3.x * Yx * rz + c3.z, v = c3.y * Yy * rz + c3.w;
  // fminf / fmaxf drop a NaN operand, so a non-finite pixel is folded into the flag: the same images as "a
  // non-finite range" (an infinite or NaN end makes the midpoint or sigma non-finite)
  ok = ok && finite_f32(u) && finite_f32(v);
  float vmin = v, vmax = v, umin = u, umax = u;
  int all_ok = ok ? 1 : 0;
#pragma unroll
  for (int off = 1; off < kTrackLanes; off <<= 1) {
    vmin = fminf(vmin, __shfl_xor(vmin, off));
    vmax = fmaxf(vmax, __shfl_xor(vmax, off));
    umin = fminf(umin, __shfl_xor(umin, off));
    umax = fmaxf(umax, __shfl_xor(umax, off));
    all_ok &= __shfl_xor(all_ok, off);
  }
  if (k != 0 || !live) return;

  // ---- lane 0: steps 3-8 ----
  const float fh = (float)P.h, fw = (float)P.w;
  float cy = 0.5f * (vmin + vmax), cx = 0.5f * (umin + umax);
  float sigma = P.margin * fmaxf((vmax - vmin) / fh, (umax - umin) / fw);
  bool good = all_ok != 0 && finite_f32(sigma) && finite_f32(cy) && finite_f32(cx);
  if (jitter) {
    sigma *= expf(js);
    cy += jy * sigma * fh;
    cx += jx * sigma * fw;
  }
  if (P.smooth < 1.f) {
    const float sp = prev.z / fh, py = prev.x + 0.5f * prev.z, px = prev.y + 0.5f * prev.w;
    sigma = sp + P.smooth * (sigma - sp);
    cy = py + P.smooth * (cy - py);
    cx = px + P.smooth * (cx - px);
  }
  good = good && finite_f32(sigma) && finite_f32(cy) && finite_f32(cx);
  float4 out = hm;
  if (good) {
    sigma = fminf(fmaxf(sigma, P.lo), P.hi);
    track_axis(sigma, cy, P.h, P.frame_h, out.x, out.z);
    track_axis(sigma, cx, P.w, P.frame_w, out.y, out.w);
  }
  *reinterpret_cast<float4*>(rois + 4 * i) = out;
  if (used) *reinterpret_cast<float4*>(used + 4 * i) = prev;
  if (valid) valid[i] = good ? 1 : 0;
}

}  // namespace argus

using namespace argus;

extern "C" {

int argus_roi_from_pose(int64_t batch, int n_cams, int frame_h, int frame_w, int h, int w, const float* poses,
                        int64_t n_poses, const int64_t* index, const float* cameras, const argus_track_cfg* cfg,
                        const float* jitter, const float* home, float* rois, float* used, int32_t* valid,
                        argus_stream_t stream) {
  auto refuse = [](const std::string& what) {
    set_error("roi_from_pose: " + what);
    return ARGUS_ERR_ARG;
  };
  const char* null_arg = !poses ? "poses" : !cameras ? "cameras" : !cfg ? "cfg" : !home ? "home" : !rois ? "rois" : nullptr;
  if (null_arg) return refuse(std::string(null_arg) + " is null");
  const char* size_arg = batch <= 0 ? "batch" : n_cams <= 0 ? "n_cams" : frame_h <= 0 ? "frame_h"
                         : frame_w <= 0 ? "frame_w" : n_poses <= 0 ? "n_poses" : nullptr;
  if (size_arg) return refuse(std::string(size_arg) + " must be positive");
  if (h < 8 || w < 8) return refuse("h and w must be at least 8");
  if (h > frame_h || w > frame_w) return refuse("h > frame_h or w > frame_w");
  if (!index && n_poses < batch) return refuse("n_poses < batch without an index");
  if (batch > (0x7FFFFFFFLL - kTrackImages) / n_cams) return refuse("batch too large for one launch");
  auto positive = [](float x) { return std::isfinite(x) && x > 0.f; };
  if (!positive(cfg->half_extent[0]) || !positive(cfg->half_extent[1]) || !positive(cfg->half_extent[2]))
    return refuse("cfg->half_extent must be finite and positive");
  if (!positive(cfg->margin)) return refuse("cfg->margin must be finite and positive");
  if (!positive(cfg->z_near)) return refuse("cfg->z_near must be finite and positive");
  if (!(cfg->scale_lo <= cfg->scale_hi)) return refuse("cfg->scale_lo > cfg->scale_hi (or a NaN)");
  if (!(cfg->smooth > 0.f && cfg->smooth <= 1.f)) return refuse("cfg->smooth must lie in (0, 1]");
  // 16-byte accesses: a camera, and one region of rois / home / used
  const char* align_arg = (reinterpret_cast<uintptr_t>(cameras) & 15) ? "cameras"
                          : (reinterpret_cast<uintptr_t>(home) & 15) ? "home"
                          : (reinterpret_cast<uintptr_t>(rois) & 15) ? "rois"
                          : (reinterpret_cast<uintptr_t>(used) & 15) ? "used" : nullptr;
  if (align_arg) return refuse(std::string(align_arg) + " must be 16-byte aligned");

  TrackParams P;
  P.ax = cfg->half_extent[0], P.ay = cfg->half_extent[1], P.az = cfg->half_extent[2];
  P.margin = cfg->margin, P.z_near = cfg->z_near, P.smooth = cfg->smooth;
  P.lo = fmaxf(cfg->scale_lo, 0.25f);
  P.hi = fminf(fminf(cfg->scale_hi, 4.f), fminf((float)frame_h / (float)h, (float)frame_w / (float)w));
  P.n_cams = n_cams, P.frame_h = frame_h, P.frame_w = frame_w, P.h = h, P.w = w;
  const int64_t n_img = batch * n_cams;
  const unsigned blocks = (unsigned)((n_img + kTrackImages - 1) / kTrackImages);
  hipLaunchKernelGGL(roi_from_pose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, n_img, poses, n_poses,
                     index, cameras, jitter, home, rois, used, valid);
  return check_launch("roi_from_pose");
}

}  // extern "C"
