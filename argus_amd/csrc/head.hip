// FC / MLP head (nn.Linear + exact-erf GELU): resnet.fc 2048->1024 (argus/models.py:56) and the
// output MLP 2048->128->128->6 (models.py:58-64, GELU at :88). fp32 throughout: these GEMMs are
// < 0.03 GFLOP/sample and latency-bound, so a simple LDS-tiled kernel on the exact
// f32 MFMA (v_mfma_f32_16x16x4_f32) keeps the head at fp32 accuracy in every precision mode.
#include "bnfin.h"
#include "internal.h"
#include "se3.h"

namespace argus {

ARGUS_DEV float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
ARGUS_DEV float gelu_grad(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// 64x64 output tile, 256 threads (4 waves, 2x2, each 32x32 = 2x2 MFMA blocks), K-tile 32. The next
// K-tile's global loads are issued into registers before the current one's MFMAs (one exposed global
// latency per K-tile: these GEMMs have few tiles and are latency-bound, so the split heuristic below
// keeps every slice at <= 4 K-tiles).
ARGUS_DEV void epilogue_store(float v, int m, int n, float* __restrict__ C, int ldc, const float* __restrict__ bias,
                               int epi, float* __restrict__ aux) {
  float* dst = C + (size_t)m * ldc + n;
  switch (epi) {
    case 0: *dst = v; break;
    case 1: *dst = v + bias[n]; break;
    case 2: v += bias[n]; aux[(size_t)m * ldc + n] = v; *dst = gelu_f(v); break;
    case 3: *dst = v * gelu_grad(aux[(size_t)m * ldc + n]); break;
    default: *dst += v; break;
  }
}

constexpr int kGemmKT = 32;

// element e (0..7) of this thread's share of a 64 x 32 operand tile: (row 0..63, k 0..31); `t` = the
// operand is stored [k][row] (k-major: consecutive threads walk rows) instead of [row][k]
ARGUS_DEV void gemm_tile_pos(int tid, int e, int t, int& row, int& kk) {
  const int idx = tid + 256 * e;
  if (t) { kk = idx >> 6; row = idx & 63; } else { row = idx >> 5; kk = idx & 31; }
}

// split-K slice z covers k in [z*kc, min(K, (z+1)*kc)); with splits > 1 the raw partial tile goes to
// ws[z][M][N] and gemm_reduce_kernel applies the epilogue after a fixed-order sum.
__global__ __launch_bounds__(256) void gemm_f32_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                       int ta, const float* __restrict__ B, int ldb, int tb,
                                                       float* __restrict__ C, int ldc, const float* __restrict__ bias,
                                                       int epi, float* __restrict__ aux, int kc,
                                                       float* __restrict__ ws) {
  __shared__ float As[kGemmKT][65];  // [k][m]
  __shared__ float Bs[kGemmKT][65];  // [k][n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kbeg = blockIdx.z * kc, kend = min(K, kbeg + kc);
  float ra[8], rb[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int mm, kk;
      gemm_tile_pos(tid, e, ta, mm, kk);
      const int gm = m0 + mm, gk = k0 + kk;
      ra[e] = (gm < M && gk < kend) ? (ta ? A[(size_t)gk * lda + gm] : A[(size_t)gm * lda + gk]) : 0.f;
      int nn, kb;
      gemm_tile_pos(tid, e, tb ? 0 : 1, nn, kb);
      const int gn = n0 + nn, gk2 = k0 + kb;
      rb[e] = (gn < N && gk2 < kend) ? (tb ? B[(size_t)gn * ldb + gk2] : B[(size_t)gk2 * ldb + gn]) : 0.f;
    }
  };
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += kGemmKT) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int mm, kk, nn, kb;
      gemm_tile_pos(tid, e, ta, mm, kk);
      gemm_tile_pos(tid, e, tb ? 0 : 1, nn, kb);
      As[kk][mm] = ra[e];
      Bs[kb][nn] = rb[e];
    }
    __syncthreads();
    if (k0 + kGemmKT < kend) load(k0 + kGemmKT);  // in flight during this tile's MFMAs
#pragma unroll
    for (int s = 0; s < kGemmKT / 4; ++s) {
      const int kk = 4 * s + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float a = As[kk][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float b = Bs[kk][wn * 32 + j * 16 + (lane & 15)];
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
        if (m >= M || n >= N) continue;
        if (ws) ws[((size_t)blockIdx.z * M + m) * N + n] = acc[i][j][r];
        else epilogue_store(acc[i][j][r], m, n, C, ldc, bias, epi, aux);
      }
    }
}

__global__ __launch_bounds__(256) void gemm_reduce_kernel(int M, int N, int splits, const float* __restrict__ ws,
                                                          float* __restrict__ C, int ldc, const float* __restrict__ bias,
                                                          int epi, float* __restrict__ aux) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * N) return;
  float v = 0.f;
  for (int zb = 0; zb < splits; zb += kLoadBatch) {
    float t[kLoadBatch];  // in flight together (common.h kLoadBatch); clamped, masked below
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) t[u] = ws[(size_t)min(zb + u, splits - 1) * M * N + e];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) v += zb + u < splits ? t[u] : 0.f;
  }
  const int m = (int)(e / N), n = (int)(e - (int64_t)m * N);
  epilogue_store(v, m, n, C, ldc, bias, epi, aux);
}

__global__ void colsum_kernel(int M, int N, const float* __restrict__ x, int ld, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int mb = 0; mb < M; mb += kLoadBatch) {
    float t[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) t[u] = x[(size_t)min(mb + u, M - 1) * ld + n];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) s += mb + u < M ? t[u] : 0.f;
  }
  out[n] = s;
}

__global__ void gelu_kernel(int64_t n, const float* __restrict__ x, float* __restrict__ y) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = gelu_f(x[i]);
}
__global__ void gelu_bwd_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ dy,
                                float* __restrict__ dx) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dx[i] = dy[i] * gelu_grad(x[i]);
}

// ------------------------------------------------------------------------------------------------
// Region-of-interest conditioning (NCameraCNNConfig.roi_frame_hw): image i = b * n_cams + c was resampled from
// the region (y0, x0, eh, ew) of an Hs x Ws frame to the network's h x w, and output_mlp.0's pre-activation gains
// e[b][j] = sum_k w_r[j][k] * rho[b][k] over the 4 n_cams region features
//   rho[b][4c + 0] = (y0 + eh / 2 - Hs / 2) / Hs     rho[b][4c + 2] = ln(eh / h)
//   rho[b][4c + 1] = (x0 + ew / 2 - Ws / 2) / Ws     rho[b][4c + 3] = ln(ew / w)
// (rho[b] and the regions of sample b share their flat index: b * 4 n_cams + k). roi_feature is the one
// statement of a feature and roi_embed_dot the one statement of e (from 0, fmaf, k ascending): the training
// launch (argus_roi_embed) and the deployed tail (argus_pose_tail_roi) produce the same bits from the same
// region. Only the feature number selects a load; nothing is indexed by a region's value.
// ------------------------------------------------------------------------------------------------
constexpr int kRoiMaxCams = 16;
constexpr int kRoiMaxFeat = 4 * kRoiMaxCams;
constexpr int kEmbedCols = 128;  // output_mlp.0's width

struct RoiFrame {
  int n_cams;
  float frame_h, frame_w, h, w;
};

// feature f (0..3) of the region r = (y0, x0, eh, ew)
ARGUS_DEV float roi_feature(const float* __restrict__ r, int f, const RoiFrame& F) {
  switch (f) {
    case 0: return (fmaf(0.5f, r[2], r[0]) - 0.5f * F.frame_h) / F.frame_h;
    case 1: return (fmaf(0.5f, r[3], r[1]) - 0.5f * F.frame_w) / F.frame_w;
    case 2: return logf(r[2] / F.h);
    default: return logf(r[3] / F.w);
  }
}

// e of column j: wr is w_r with element (j, k) at wr[j * sj + k * sk]
ARGUS_DEV float roi_embed_dot(const float* wr, int sj, int sk, int j, const float* rho, int nfeat) {
  float e = 0.f;
  for (int k = 0; k < nfeat; ++k) e = fmaf(wr[j * sj + k * sk], rho[k], e);
  return e;
}

// one workgroup of 128 threads per sample: z[b][j] += e[b][j], g = gelu(z), rho saved for the weight gradient
__global__ __launch_bounds__(kEmbedCols) void roi_embed_kernel(RoiFrame F, const float* __restrict__ rois,
                                                                 const float* __restrict__ w_r, float* __restrict__ z,
                                                                 float* __restrict__ g, float* __restrict__ rho) {
  __shared__ float rs[kRoiMaxFeat];
  const int b = blockIdx.x, j = threadIdx.x, nfeat = 4 * F.n_cams;
  if (j < nfeat) {
    const float v = roi_feature(rois + (size_t)b * nfeat + (j & ~3), j & 3, F);
    rs[j] = v;
    if (rho) rho[(size_t)b * nfeat + j] = v;
  }
  __syncthreads();
  const size_t o = (size_t)b * kEmbedCols + j;
  const float v = z[o] + roi_embed_dot(w_r, nfeat, 1, j, rs, nfeat);
  z[o] = v;
  if (g) g[o] = gelu_f(v);
}

// ------------------------------------------------------------------------------------------------
// Frozen pose head for rows <= 16 (the deployment path: one pose per replay, latency-bound): the
// avg-pool + resnet.fc + GELU and the output MLP + se(3) Exp in two launches, where the session had
// avgpool_fwd, gemm_f32 (+ its split reduce), gelu and three more gemm_f32 in the graph and a clone +
// se3_exp outside it. Both split their long reduction (2048 channels) over workgroups in slices of 64
// channels; a slice's raw partial goes to the caller's workspace, the workgroups take bnfin.h's ticket
// (fin_ticket<kPlainStores>), and the last arriver sums the slices in slice order (its own included), so
// the result does not depend on which workgroup came last. Workspace: kHeadTicketBytes of ticket words
// (zero on entry and on return), then float partials [column block][slice][row][128].
// ------------------------------------------------------------------------------------------------
constexpr int kHeadRows = 16;          // most rows (batch * n_cams, or batch) served
constexpr int kHeadSlice = 64;         // reduction channels per workgroup
constexpr int kHeadCols = 128;         // output columns per workgroup
constexpr size_t kHeadTicketBytes = 256;
static_assert(kEmbedCols == kHeadCols, "the region term is added to output_mlp.0's 128 columns");

// part[row][jl] = sum over the slice's 64 channels of w[j0 + jl][c0 + .] * f[row][.] for jl < 128:
// thread (jl = tid / 2, half = tid % 2) holds its 32 weights in registers, sums them in channel order and
// adds the two halves (lower + upper). Rows of w past `nout` are clamped and not stored.
ARGUS_DEV void head_slice_dot(int tid, int rows, const float* __restrict__ w, int ldw, int j0, int c0, int nout,
                              const float (*f)[kHeadSlice], float* part) {
  const int jl = tid >> 1, half = tid & 1;
  const int j = min(j0 + jl, nout - 1);
  f32x4 wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    wv[i] = *reinterpret_cast<const f32x4*>(w + (size_t)j * ldw + c0 + half * 32 + i * 4);
  for (int row = 0; row < rows; ++row) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(wv[i][e], f[row][half * 32 + i * 4 + e], s);
    const float o = __shfl_xor(s, 1, 64);
    if (half == 0 && j0 + jl < nout) part[row * kHeadCols + jl] = s + o;
  }
}

// the last arriver's sum of column jl over the slices, in slice order (kLoadBatch loads in flight)
ARGUS_DEV float head_slice_sum(const float* part, int slices, int rows, int row, int jl) {
  float v = 0.f;
  for (int sb = 0; sb < slices; sb += kLoadBatch) {
    float t[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u)
      t[u] = part[((size_t)min(sb + u, slices - 1) * rows + row) * kHeadCols + jl];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) v += sb + u < slices ? t[u] : 0.f;
  }
  return v;
}

// grid (c / 64 slices, ceil(rdim / 128) column blocks); a ticket per column block
template <typename T>
__global__ __launch_bounds__(256) void pool_fc_gelu_kernel(int n, int hw, int c, const T* __restrict__ x,
                                                           const float* __restrict__ w, const float* __restrict__ b,
                                                           int rdim, float* __restrict__ g0, unsigned* tickets,
                                                           float* part) {
  constexpr int E = Chunk<T>::E, CH = kHeadSlice / E, PG = 256 / CH;  // chunks per slice row, pixel groups
  __shared__ float feat[kHeadRows][kHeadSlice];
  __shared__ float red[PG][kHeadSlice + 4];
  __shared__ int flag;
  const int tid = threadIdx.x, slice = blockIdx.x, jb = blockIdx.y, slices = gridDim.x;
  const int c0 = slice * kHeadSlice;
  // ---- this slice's channel means: pixel group pg sums pixels pg, pg + PG, ... in order; the groups in order ----
  const int ch = tid % CH, pg = tid / CH;
  for (int row = 0; row < n; ++row) {
    float s[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = 0.f;
    const T* xr = x + (size_t)row * hw * c + c0 + ch * E;
    for (int pb = pg; pb < hw; pb += PG * 4) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld16(xr + (size_t)min(pb + u * PG, hw - 1) * c);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[E];
        ChunkCvt<T>::unpack(v[u], f);
#pragma unroll
        for (int e = 0; e < E; ++e) s[e] += pb + u * PG < hw ? f[e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) red[pg][ch * E + e] = s[e];
    __syncthreads();
    if (tid < kHeadSlice) {
      float t = 0.f;
      for (int g = 0; g < PG; ++g) t += red[g][tid];
      feat[row][tid] = t / (float)hw;
    }
    __syncthreads();
  }
  float* mine = part + ((size_t)jb * slices + slice) * n * kHeadCols;
  head_slice_dot(tid, n, w, c, jb * kHeadCols, c0, rdim, feat, mine);
  if (!fin_ticket<kPlainStores>(tickets + jb, (unsigned)slices, &flag)) return;
  const float* all = part + (size_t)jb * slices * n * kHeadCols;
  const int jl = tid & (kHeadCols - 1), j = jb * kHeadCols + jl;
  if (j < rdim)
    for (int row = tid >> 7; row < n; row += 2)
      g0[(size_t)row * rdim + j] = gelu_f(head_slice_sum(all, slices, n, row, jl) + b[j]);
}

// grid d / 64 slices of output_mlp.0; the last arriver finishes the MLP and the exponential alone. ROI
// (argus_pose_tail_roi): the pre-activation of output_mlp.0 gains the region term e. Every workgroup stages the
// features (batch * n_cams <= 16 regions) and w_r, transposed to [k][column], in LDS BEFORE the ticket: whichever
// arrives last already holds them, so its critical path gains 4 n_cams LDS fmafs a column and no memory round trip.
template <bool ROI>
__global__ __launch_bounds__(256) void pose_tail_kernel(int batch, int d, const float* __restrict__ g0,
                                                        const float* __restrict__ w0, const float* __restrict__ b0,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        const float* __restrict__ w4, const float* __restrict__ b4,
                                                        float* __restrict__ pred, float* __restrict__ pose, int canon,
                                                        unsigned* tickets, float* part, RoiFrame F,
                                                        const float* __restrict__ rois, const float* __restrict__ w_r) {
  __shared__ float feat[kHeadRows][kHeadSlice];
  __shared__ float h1[kHeadRows][kHeadCols], h2[kHeadRows][kHeadCols];
  __shared__ float pr[kHeadRows * 6];
  __shared__ int flag;
  __shared__ float rs[ROI ? kHeadRows * 4 : 1];               // rho, flat [b][4c + f]
  __shared__ float wrs[ROI ? kRoiMaxFeat * kHeadCols : 1];    // w_r as [k][column]
  const int tid = threadIdx.x, slice = blockIdx.x, slices = gridDim.x;
  const int nfeat = ROI ? 4 * F.n_cams : 0;
  if constexpr (ROI) {
    if (tid < batch * nfeat) rs[tid] = roi_feature(rois + (tid & ~3), tid & 3, F);
    for (int i = tid; i < kHeadCols * nfeat; i += 256) wrs[(i % nfeat) * kHeadCols + i / nfeat] = w_r[i];
  }
  for (int i = tid; i < batch * kHeadSlice; i += 256)
    feat[i / kHeadSlice][i % kHeadSlice] = g0[(size_t)(i / kHeadSlice) * d + slice * kHeadSlice + i % kHeadSlice];
  __syncthreads();
  head_slice_dot(tid, batch, w0, d, 0, slice * kHeadSlice, kHeadCols, feat, part + (size_t)slice * batch * kHeadCols);
  if (!fin_ticket<kPlainStores>(tickets, (unsigned)slices, &flag)) return;
  const int jl = tid & (kHeadCols - 1);
  for (int row = tid >> 7; row < batch; row += 2) {  // output_mlp.0 (+ the region term) + GELU
    float v = head_slice_sum(part, slices, batch, row, jl) + b0[jl];
    if constexpr (ROI) v += roi_embed_dot(wrs, 1, kHeadCols, jl, rs + row * nfeat, nfeat);
    h1[row][jl] = gelu_f(v);
  }
  __syncthreads();
  for (int row = tid >> 7; row < batch; row += 2) {  // output_mlp.2 + GELU
    float s = 0.f;
    for (int k = 0; k < kHeadCols; k += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w2 + jl * kHeadCols + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(wv[e], h1[row][k + e], s);
    }
    h2[row][jl] = gelu_f(s + b2[jl]);
  }
  __syncthreads();
  if (tid < batch * 6) {  // output_mlp.4
    const int row = tid / 6, o = tid - row * 6;
    float s = 0.f;
    for (int k = 0; k < kHeadCols; k += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w4 + o * kHeadCols + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(wv[e], h2[row][k + e], s);
    }
    s += b4[o];
    pr[tid] = s;
    pred[tid] = s;
  }
  __syncthreads();
  if (tid < batch) se3_exp_one(pr + tid * 6, pose + tid * 7, canon);  // argus_se3_exp's function on this pred
}

static size_t head_ws_bytes(int rows, int k, int nout) {
  return kHeadTicketBytes + (size_t)((nout + kHeadCols - 1) / kHeadCols) * (k / kHeadSlice) * rows * kHeadCols * sizeof(float);
}

}  // namespace argus

using namespace argus;

extern "C" {

// split-K slices: up to 512 workgroups, each slice >= 128 of K (<= 4 K-tiles once K allows)
static int gemm_splits(int m, int n, int k) {
  const int tiles = ((m + 63) / 64) * ((n + 63) / 64);
  int splits = 1;
  while (tiles * splits < 512 && k / (splits * 2) >= 128) splits *= 2;
  return splits;
}

size_t argus_gemm_f32_workspace_bytes(int m, int n, int k) {
  const int splits = gemm_splits(m, n, k);
  return splits > 1 ? (size_t)splits * m * n * sizeof(float) : 0;
}

int argus_gemm_f32(int m, int n, int k, const float* a, int lda, int ta, const float* b, int ldb, int tb, float* c,
                   int ldc, const float* bias, int epi, float* aux, void* ws, size_t ws_bytes, argus_stream_t stream) {
  if (m <= 0 || n <= 0 || k <= 0 || !a || !b || !c || epi < 0 || epi > 4 || ((epi == 1 || epi == 2) && !bias) ||
      ((epi == 2 || epi == 3) && !aux)) {
    set_error("gemm_f32: bad arguments");
    return ARGUS_ERR_ARG;
  }
  int splits = gemm_splits(m, n, k);
  if (splits > 1 && (!ws || ws_bytes < (size_t)splits * m * n * sizeof(float))) splits = 1;  // no workspace
  const int kc = ((k + splits - 1) / splits + kGemmKT - 1) / kGemmKT * kGemmKT;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((n + 63) / 64, (m + 63) / 64, splits);
  hipLaunchKernelGGL(gemm_f32_kernel, grid, dim3(256), 0, st, m, n, k, a, lda, ta, b, ldb, tb, c, ldc, bias, epi, aux,
                     kc, splits > 1 ? (float*)ws : (float*)nullptr);
  if (int e = check_launch("gemm_f32_kernel")) return e;
  if (splits > 1) {
    hipLaunchKernelGGL(gemm_reduce_kernel, dim3((unsigned)(((int64_t)m * n + 255) / 256)), dim3(256), 0, st, m, n,
                       splits, (const float*)ws, c, ldc, bias, epi, aux);
    return check_launch("gemm_reduce_kernel");
  }
  return ARGUS_OK;
}

int argus_colsum_f32(int m, int n, const float* x, int ld, float* out, argus_stream_t stream) {
  hipLaunchKernelGGL(colsum_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, n, x, ld, out);
  return check_launch("colsum_kernel");
}

int argus_gelu_f32(int64_t count, const float* x, float* y, argus_stream_t stream) {
  const int blocks = (int)std::min<int64_t>((count + 255) / 256, 4096);
  hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, count, x, y);
  return check_launch("gelu_kernel");
}

int argus_gelu_bwd_f32(int64_t count, const float* x, const float* dy, float* dx, argus_stream_t stream) {
  const int blocks = (int)std::min<int64_t>((count + 255) / 256, 4096);
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, count, x, dy, dx);
  return check_launch("gelu_bwd_kernel");
}

size_t argus_pool_fc_gelu_workspace_bytes(int n, int c, int rdim) {
  if (n <= 0 || n > kHeadRows || c <= 0 || c % kHeadSlice || rdim <= 0) return 0;
  return head_ws_bytes(n, c, rdim);
}

int argus_pool_fc_gelu(int x_dtype, int n, int hw, int c, const void* x, const float* w_fc, const float* b_fc, int rdim,
                       float* g0, void* workspace, size_t workspace_bytes, argus_stream_t stream) {
  const int dtype = x_dtype;
  if (dtype != ARGUS_BF16 && dtype != ARGUS_F16) {
    set_error("pool_fc_gelu: dtype must be ARGUS_BF16 or ARGUS_F16");
    return ARGUS_ERR_ARG;
  }
  if (!x || !w_fc || !b_fc || !g0 || !workspace) { set_error("pool_fc_gelu: null argument"); return ARGUS_ERR_ARG; }
  if (n <= 0 || n > kHeadRows) {
    set_error("pool_fc_gelu: serves 1..16 rows (the deployment path; larger batches use argus_avgpool_fwd + argus_gemm_f32)");
    return ARGUS_ERR_ARG;
  }
  if (hw <= 0 || rdim <= 0 || c <= 0) { set_error("pool_fc_gelu: bad sizes"); return ARGUS_ERR_ARG; }
  if (c % kHeadSlice) { set_error("pool_fc_gelu: channels must be a multiple of 64"); return ARGUS_ERR_SHAPE; }
  if ((int64_t)n * hw * c >= (1LL << 31)) { set_error("pool_fc_gelu: tensor exceeds 2^31 elements"); return ARGUS_ERR_SHAPE; }
  const int jbs = (rdim + kHeadCols - 1) / kHeadCols;
  if ((size_t)jbs * sizeof(unsigned) > kHeadTicketBytes) { set_error("pool_fc_gelu: rdim too large"); return ARGUS_ERR_SHAPE; }
  if (workspace_bytes < head_ws_bytes(n, c, rdim)) {
    set_error("pool_fc_gelu: workspace too small (argus_pool_fc_gelu_workspace_bytes)");
    return ARGUS_ERR_ARG;
  }
  unsigned* tk = reinterpret_cast<unsigned*>(workspace);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + kHeadTicketBytes);
  const dim3 grid(c / kHeadSlice, jbs);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ARGUS_F16)
    hipLaunchKernelGGL(pool_fc_gelu_kernel<f16>, grid, dim3(256), 0, st, n, hw, c, (const f16*)x, w_fc, b_fc, rdim, g0, tk, part);
  else
    hipLaunchKernelGGL(pool_fc_gelu_kernel<bf16>, grid, dim3(256), 0, st, n, hw, c, (const bf16*)x, w_fc, b_fc, rdim, g0, tk, part);
  return check_launch("pool_fc_gelu_kernel");
}

size_t argus_pose_tail_workspace_bytes(int batch, int d) {
  if (batch <= 0 || batch > kHeadRows || d <= 0 || d % kHeadSlice) return 0;
  return head_ws_bytes(batch, d, kHeadCols);
}

// what argus_pose_tail refuses, for both entry points (`who` prefixes the message)
static int pose_tail_check(const char* who, int batch, int d, const float* g0, const float* w0, const float* b0,
                           const float* w2, const float* b2, const float* w4, const float* b4, const float* pred,
                           const float* pose, const void* workspace, size_t workspace_bytes) {
  const std::string p = std::string(who) + ": ";
  if (!g0 || !w0 || !b0 || !w2 || !b2 || !w4 || !b4 || !pred || !pose || !workspace) {
    set_error(p + "null argument");
    return ARGUS_ERR_ARG;
  }
  if (batch <= 0 || batch > kHeadRows) {
    set_error(p + "serves batch 1..16 (the deployment path; larger batches use argus_gemm_f32 + argus_se3_exp)");
    return ARGUS_ERR_ARG;
  }
  if (d <= 0) { set_error(p + "bad sizes"); return ARGUS_ERR_ARG; }
  if (d % kHeadSlice) { set_error(p + "d must be a multiple of 64"); return ARGUS_ERR_SHAPE; }
  if (workspace_bytes < head_ws_bytes(batch, d, kHeadCols)) {
    set_error(p + "workspace too small (argus_pose_tail_workspace_bytes)");
    return ARGUS_ERR_ARG;
  }
  return ARGUS_OK;
}

// the frame / network sizes both region entry points refuse; nullptr = served
static const char* roi_frame_refusal(int n_cams, int frame_h, int frame_w, int h, int w) {
  if (n_cams <= 0) return "n_cams must be positive";
  if (frame_h <= 0) return "frame_h must be positive";
  if (frame_w <= 0) return "frame_w must be positive";
  if (h < 8 || w < 8) return "h and w must be at least 8";
  if (h > frame_h || w > frame_w) return "h > frame_h or w > frame_w";
  if (n_cams > kRoiMaxCams) return "n_cams exceeds 16";
  return nullptr;
}

int argus_pose_tail(int batch, int d, const float* g0, const float* w0, const float* b0, const float* w2,
                    const float* b2, const float* w4, const float* b4, float* pred, float* pose, int canonical_w,
                    void* workspace, size_t workspace_bytes, argus_stream_t stream) {
  if (int e = pose_tail_check("pose_tail", batch, d, g0, w0, b0, w2, b2, w4, b4, pred, pose, workspace, workspace_bytes))
    return e;
  unsigned* tk = reinterpret_cast<unsigned*>(workspace);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + kHeadTicketBytes);
  hipLaunchKernelGGL(pose_tail_kernel<false>, dim3(d / kHeadSlice), dim3(256), 0, (hipStream_t)stream, batch, d, g0, w0,
                     b0, w2, b2, w4, b4, pred, pose, canonical_w, tk, part, RoiFrame{}, (const float*)nullptr,
                     (const float*)nullptr);
  return check_launch("pose_tail_kernel");
}

int argus_pose_tail_roi(int batch, int d, const float* g0, const float* w0, const float* b0, const float* w2,
                        const float* b2, const float* w4, const float* b4, float* pred, float* pose, int canonical_w,
                        int n_cams, int frame_h, int frame_w, int h, int w, const float* rois, const float* w_r,
                        void* workspace, size_t workspace_bytes, argus_stream_t stream) {
  if (int e = pose_tail_check("pose_tail_roi", batch, d, g0, w0, b0, w2, b2, w4, b4, pred, pose, workspace,
                              workspace_bytes))
    return e;
  auto refuse = [](const std::string& what) {
    set_error("pose_tail_roi: " + what);
    return ARGUS_ERR_ARG;
  };
  if (!rois) return refuse("rois is null");
  if (!w_r) return refuse("w_r is null");
  if (const char* why = roi_frame_refusal(n_cams, frame_h, frame_w, h, w)) return refuse(why);
  if (batch * n_cams > kHeadRows)
    return refuse("serves batch * n_cams 1..16 (the deployment path; larger batches use argus_roi_embed)");
  unsigned* tk = reinterpret_cast<unsigned*>(workspace);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + kHeadTicketBytes);
  const RoiFrame F{n_cams, (float)frame_h, (float)frame_w, (float)h, (float)w};
  hipLaunchKernelGGL(pose_tail_kernel<true>, dim3(d / kHeadSlice), dim3(256), 0, (hipStream_t)stream, batch, d, g0, w0,
                     b0, w2, b2, w4, b4, pred, pose, canonical_w, tk, part, F, rois, w_r);
  return check_launch("pose_tail_roi_kernel");
}

int argus_roi_embed(int batch, int n_cams, int frame_h, int frame_w, int h, int w, const float* rois,
                    const float* w_r, float* z, float* g, float* rho, argus_stream_t stream) {
  auto refuse = [](const std::string& what) {
    set_error("roi_embed: " + what);
    return ARGUS_ERR_ARG;
  };
  const char* null_arg = !rois ? "rois" : !w_r ? "w_r" : !z ? "z" : nullptr;
  if (null_arg) return refuse(std::string(null_arg) + " is null");
  if (batch <= 0) return refuse("batch must be positive");
  if (const char* why = roi_frame_refusal(n_cams, frame_h, frame_w, h, w)) return refuse(why);
  const RoiFrame F{n_cams, (float)frame_h, (float)frame_w, (float)h, (float)w};
  hipLaunchKernelGGL(roi_embed_kernel, dim3((unsigned)batch), dim3(kEmbedCols), 0, (hipStream_t)stream, F, rois, w_r,
                     z, g, rho);
  return check_launch("roi_embed_kernel");
}

}  // extern "C"
