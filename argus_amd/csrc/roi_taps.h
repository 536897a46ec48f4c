// Per-axis taps of the region-of-interest resampling (include/argus_hip.h, argus_frames_resample), shared by
// the deployed kernels (stem_infer.hip) and the training loader's batch build (resident.hip): one definition,
// so train and deploy weigh the same source pixels with the same fp32 bits.
#pragma once
#include "common.h"

namespace argus {

constexpr int kRoiTaps = 9;

struct RoiTaps {
  float w[kRoiTaps];  // normalised; 0 beyond cnt
  int lo, cnt;        // source pixels lo .. lo + cnt - 1, inside [0, S) for ANY bit pattern of the region
};

ARGUS_DEV void roi_axis(int S, int n, float o, float e, int i, RoiTaps& out) {
  const float s = e / (float)n, r = fmaxf(s, 1.f);
  const float c = fmaf((float)i + 0.5f, s, o);
  // clamped as floats (fmaxf drops a NaN), then as integers ((float)S may round up): 0 <= lo <= hi <= S
  const float fs = (float)S;
  const int lo = min((int)fminf(fmaxf(floorf(c - r + 0.5f), 0.f), fs), S);
  const int hi = min((int)fminf(fmaxf(floorf(c + r + 0.5f), 0.f), fs), S);
  const int cnt = min(max(hi - lo, 0), kRoiTaps);
  float t[kRoiTaps], sum = 0.f;
#pragma unroll
  for (int k = 0; k < kRoiTaps; ++k) {
    t[k] = k < cnt ? fmaxf(0.f, 1.f - fabsf((float)(lo + k) + 0.5f - c) / r) : 0.f;
    sum += t[k];
  }
#pragma unroll
  for (int k = 0; k < kRoiTaps; ++k) out.w[k] = t[k] / sum;
  out.lo = lo;
  out.cnt = cnt;
}

}  // namespace argus
