// The stem's 8 x 32 output tile on the LDS input patch: the geometry, the filter staging and the MFMA loop
// shared by stem_fwd_kernel / stem_wgrad_kernel (stem.hip) and stem_infer_kernel (stem_infer.hip).
#pragma once
#include "igemm.h"

namespace argus {

constexpr int kTH = 8, kTW = 32;           // output tile
constexpr int kPR = 2 * kTH + 5;           // patch rows (21)
constexpr int kPC = 2 * kTW + 6;           // patch columns (70): column pc = input column 2*ow0 - 3 + pc
constexpr int kWS = 7 * 32 + 8;            // LDS weight row stride, elements (224 + 8: 464 B, conflict-free)
constexpr int kPatchB = kPR * kPC * 8;     // 11760
constexpr int kWB = 64 * kWS * 2;          // 29696
constexpr int kLD = 64 + 8;                // C staging row stride, elements
constexpr int kLdsB = (kPatchB + kWB) > 256 * kLD * 2 ? (kPatchB + kWB) : 256 * kLD * 2;
constexpr int kPatchPT = (kPR * kPC + 255) / 256;  // patch pixels per thread (6)

// the 64 x 224 filter (rows 0..6 of w_fwd's [64][8][8][4]): 64 rows x 28 chunks of 16 B, 7 a thread
template <typename T>
ARGUS_DEV void stem_w_load(const T* w, int tid, u32x4 (&wv)[7]) {
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int q = tid + 256 * i;
    const int n = q / 28, ch = q - n * 28;
    wv[i] = ld16(w + n * 256 + ch * 8);
  }
}
template <typename T>
ARGUS_DEV void stem_w_store(T* wl, int tid, const u32x4 (&wv)[7]) {
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int q = tid + 256 * i;
    const int n = q / 28, ch = q - n * 28;
    *reinterpret_cast<u32x4*>(wl + n * kWS + ch * 8) = wv[i];
  }
}

// wave w owns tile rows 2w, 2w+1 (64 pixels) x 64 channels; filter rows 0..6 in order. acc[mi][ni][r] is
// tile pixel w*64 + mi*16 + g*4 + r (row = pixel / 32, column = pixel % 32), channel ni*16 + i16.
template <typename T>
ARGUS_DEV void stem_tile_mma(const uint8_t* pb, const T* wl, int wave, int lane, f32x4 (&acc)[4][4]) {
  const int g = lane >> 4, i16 = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    u32x4 fa[4], fb[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int tr = 2 * wave + (mi >> 1), j = (mi & 1) * 16 + i16;
      fa[mi] = *reinterpret_cast<const u32x4*>(pb + ((2 * tr + r) * kPC + 2 * j + 2 * g) * 8);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      fb[ni] = *reinterpret_cast<const u32x4*>(wl + (ni * 16 + i16) * kWS + r * 32 + g * 8);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        Mma<T>::run(acc[mi][ni], fa[mi], fb[ni]);
  }
}

}  // namespace argus
