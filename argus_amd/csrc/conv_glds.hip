// Implicit-GEMM convolution (forward / dgrad, bf16, no BN prologue) with global->LDS DMA staging.
//
// Why a second kernel: the register-staged igemm_kernel (conv.hip) moves every operand byte
// global -> VGPR -> LDS; on gfx950 a ds_write_b128 costs ~13 cycles of VGPR->LDS transfer per wave
// instruction (~79 B/clk/CU, MI355X_MICROARCH.md §LDS), which for its 128x128 tile exceeds the MFMA
// time per k-step. Here both operands go straight to LDS with global_load_lds_dwordx4 (no VGPR, no
// ds_write), through a 3-stage LDS ring with a counted vmcnt and raw s_barrier, so two k-steps of
// loads are in flight while the MFMAs of the current one run (cdna_hip_programming.md §5,
// "Pipelining across barriers").
//
// Geometry: each wave computes a 64x64 output tile (4x4 v_mfma_f32_16x16x32_bf16 blocks); the
// workgroup is (BM/64) x (BN/64) waves: 256x128 (8 waves) or 256x64 (4 waves). K-step = one tap x 64
// input channels. LDS images are [row][64 k] bf16 (128 B rows), 16-byte slot j of row r holding
// k-chunk j ^ swz8(r) (conflict-free ds_read_b128 fragment reads); glds writes lane-linear 1 KB
// pieces (8 rows), so the swizzle is applied on the per-lane global source address. Out-of-image
// taps and rows past M read a 16-byte zero page. BN statistics are emitted per 64-row wave tile or
// per 128-row half tile, in the same partial layout as igemm_kernel's 64- / 128-row tiles.
#include "common.h"
#include "igemm.h"
#include "internal.h"
#include "ktimer.h"
#include "lds_dma.h"

namespace argus {

// NSTAGE 3: k-steps kt+1 and kt+2 in flight during compute(kt) (144 KB LDS for 256 x 128); 2: kt+1
// only, 96 KB, so a workgroup fits beside one side-stream weight-gradient workgroup (64 KB) on a CU
template <int BM, int BN, int BW, int NSTAGE = 3>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64, 1) void igemm_glds_kernel(const IgParams p) {
  constexpr int WM = BM / 64, WN = BN / 64, NW = WM * WN, NT = NW * 64;
  constexpr int STAGE = (BM + BN) * 128;      // bytes per pipeline stage (A image, then B image)
  static_assert(NSTAGE == 2 || NSTAGE == 3, "glds ring depth");
  constexpr int LD = BN + 8;                   // epilogue C row stride (elements)
  constexpr int EPI = BM * LD * 2;
  constexpr int LDS0 = NSTAGE * STAGE > EPI ? NSTAGE * STAGE : EPI;
  constexpr int RED_B = (NT / (BN / 8)) * BN * 8;  // BN-backward column sums
  constexpr int LDS_BYTES = LDS0 > RED_B ? LDS0 : RED_B;
  constexpr int AI = BM * 8 / NT;              // A glds per thread per stage
  constexpr int BI = BN * 8 / NT;              // B glds per thread per stage
  constexpr int GPS = AI + BI;                 // glds per wave per stage (vmcnt unit)
  static_assert(AI * NT == BM * 8 && BI * NT == BN * 8, "tile / thread mismatch");
  __shared__ __attribute__((aligned(1024))) u32x4 lds[LDS_BYTES / 16];

  const IgPhase& ph = p.ph[blockIdx.z];
  const int mtiles = (ph.M + BM - 1) / BM;
  const int ntiles = p.N / BN;
  const int nwg = mtiles * ntiles;
  // the folded finalize's ticket flag: the last 16 bytes of the LDS array (bn_fin_arrive's scratch is its
  // first NT * 32 bytes), so the 2-stage ring stays at exactly 96 KB
  int& fin_flag = *reinterpret_cast<int*>(&lds[LDS_BYTES / 16 - 1]);
  if ((int)blockIdx.x >= nwg) {
    if constexpr (BW != 0) {
      const int e = blockIdx.x - nwg;
      bwd_epi_zero_rows<BN, NT>(p.bb, e, mtiles, ntiles, p.N);
      if (p.fin.mode && mtiles + e / ntiles < p.bb.prow)
        bn_fin_arrive<NT, BN>(p.fin, blockIdx.z * p.bb.prow + mtiles + e / ntiles, e % ntiles,
                              reinterpret_cast<double2*>(lds), &fin_flag);
    }
    return;
  }
  if (ph.K == 0 && p.addend == p.c && !p.addend_mask && BW == 0) return;  // in-place += 0
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int mt = bid / ntiles, nt = bid - mt * ntiles;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const bf16* __restrict__ A = reinterpret_cast<const bf16*>(p.a);
  const bf16* __restrict__ B = reinterpret_cast<const bf16*>(p.b);
  const uint32_t lds0 = (uint32_t)(uintptr_t)lds;

  // this thread's A rows (output pixels) and the k-chunk each of its glds fetches
  const int HWq = ph.Hq * ph.Wq;
  int a_off[AI], a_ih[AI], a_iw[AI], a_ch[AI];
  bool a_ok[AI];
  const bool a_ident = a_rows_ident(p, &ph);  // 1x1 / stride-1 GEMM: input pixel = GEMM row
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = 8 * (i * NW + wave) + (lane >> 3);
    const int m = mt * BM + row;
    a_ok[i] = m < ph.M;
    a_row_offset(p, ph, HWq, a_ok[i] ? m : 0, a_ident, a_off[i], a_ih[i], a_iw[i]);
    a_ch[i] = ((lane & 7) ^ swz8(row)) * 8;
  }
  const bf16* b_src[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int row = 8 * (i * NW + wave) + (lane >> 3);
    b_src[i] = B + (size_t)(nt * BN + row) * p.ldb + ((lane & 7) ^ swz8(row)) * 8;
  }
  const void* zero = (const void*)lds_dma_zero_page;

  auto issue = [&](int kt, int stage) {
    const int k0 = kt * 64;
    const int t = k0 / p.Cin;
    const int ci0 = k0 - t * p.Cin;
    const int dh = ph.dh[t], dw = ph.dw[t], boff = ph.boff[t];
    const int tap = (dh * p.W + dw) * p.lda + ci0;
    const uint32_t base = lds0 + stage * STAGE + wave * 1024;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int ih = a_ih[i] + dh, iw = a_iw[i] + dw;
      const bool ok = a_ok[i] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      lds_dma16(ok ? (const void*)(A + a_off[i] + tap + a_ch[i]) : zero, base + i * NW * 1024);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) lds_dma16(b_src[i] + boff + ci0, base + BM * 128 + i * NW * 1024);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, i16 = lane & 15;
  auto compute = [&](int stage) {
    const char* L = reinterpret_cast<const char*>(lds) + stage * STAGE;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4 fa[4], fb[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int row = wm * 64 + mi * 16 + i16;
        fa[mi] = *reinterpret_cast<const u32x4*>(L + row * 128 + (((4 * s2 + g) ^ swz8(row)) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int row = wn * 64 + ni * 16 + i16;
        fb[ni] = *reinterpret_cast<const u32x4*>(L + BM * 128 + row * 128 + (((4 * s2 + g) ^ swz8(row)) << 4));
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) Mma<bf16>::run(acc[mi][ni], fa[mi], fb[ni]);
    }
  };

  // ---- main loop: NSTAGE-deep ring ----
  const int nk = ph.K / 64;
  if (nk > 0) issue(0, 0);
  if constexpr (NSTAGE == 3) {  // k-steps kt+1 and kt+2 in flight during compute(kt)
    if (nk > 1) issue(1, 1);
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) wait_vm<GPS>(); else wait_vm<0>();
      lds_dma_barrier();  // stage kt landed for every wave; every wave finished reading stage kt-1
      if (kt + 2 < nk) issue(kt + 2, (kt + 2) % NSTAGE);
      compute(kt % NSTAGE);
    }
  } else {  // k-step kt+1 in flight during compute(kt)
    for (int kt = 0; kt < nk; ++kt) {
      wait_vm<0>();
      lds_dma_barrier();  // stage kt landed for every wave; every wave finished reading stage kt-1 (= kt+1's)
      if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
      compute(kt & 1);
    }
  }
  wait_vm<0>();
  __syncthreads();  // LDS is reused below

  // ---- BN statistics per 64-row (one wave) or 128-row (two waves) tile: {sum, M2} per column ----
  if (p.stats) {
    float2* red = reinterpret_cast<float2*>(lds);  // [WM][BN]
    bn_stats_wave<NT, BN, WM>(tid, lane, g, acc, StatRowsBelow<64>(ph.M - mt * BM, wm), p.stat_tile == 64, red, wm, wn * 64,
                              p.stats + nt * BN, p.N, (size_t)mt);
    __syncthreads();
    bn_stats_merge<NT, BN, WM>(tid, StatRowsBelow<64>(ph.M - mt * BM, wm), p.stat_tile == 64, red, p.stats + nt * BN, p.N,
                               (size_t)mt);
    if (p.ffin.mode) {  // the statistics finalize folded in (bnfin.h): BM / stat_tile partial rows a tile
      bn_fwd_fin_arrive<NT, BN>(p.ffin, mt, nt, reinterpret_cast<double2*>(lds), &fin_flag);
      __syncthreads();
    }
  }

  // ---- epilogue: stage the C tile in LDS, then 16-byte coalesced (+addend) stores ----
  bf16* Cs = reinterpret_cast<bf16*>(lds);
  epi_stage<bf16, LD>(g, i16, acc, Cs, wm * 64, wn * 64);
  __syncthreads();
  BwdEpiAcc<bf16, BW> bwd;
  if constexpr (BW != 0) bwd.init(p.bb, nt * BN + (tid % (BN / 8)) * 8);
  epi_store<bf16, BW, NT, BN, BM, LD>(tid, p, Cs, nt * BN, bwd, EpiRows{p, ph, HWq, mt * BM, c_rows_ident(p, ph)},
                                      [&](int, size_t off, EpiIn& in) { epi_load<bf16, BW>(p, off, in); });
  epi_bwd_finish<bf16, BW, NT, BN>(tid, p, bwd, lds, blockIdx.z * p.bb.prow + mt, nt, &fin_flag);
}

template <int BM, int BN, int BW, int NS>
static const char* glds_name() {
  static const std::string s = std::string("argus::igemm_glds_kernel<") + std::to_string(BM) + ", " +
                               std::to_string(BN) + ", " + std::to_string(BW) + ", " + std::to_string(NS) + ">";
  return s.c_str();
}

template <int BM, int BN, int BW, int NS>
static void launch_glds1(const IgParams& p0, int maxM, hipStream_t st) {
  IgParams p = p0;
  plan_fin(p, BM);
  plan_ffin(p, BM);
  dim3 grid(cdiv(maxM, BM) * (p.N / BN), 1, p.nphase);
  timed_launch(glds_name<BM, BN, BW, NS>(), igemm_glds_kernel<BM, BN, BW, NS>, grid,
               dim3((BM / 64) * (BN / 64) * 64), st, p);
}

template <int BM, int BN, int NS>
static void launch_glds_ns(const IgParams& p, int maxM, hipStream_t st) {
  switch (bwd_variant(p.bb)) {
    case 2: launch_glds1<BM, BN, 2, NS>(p, maxM, st); break;
    case 3: launch_glds1<BM, BN, 3, NS>(p, maxM, st); break;
    case 4: launch_glds1<BM, BN, 4, NS>(p, maxM, st); break;
    default: launch_glds1<BM, BN, 0, NS>(p, maxM, st);
  }
}

// policy key 41: ring depth of the data gradients (the forwards keep 3: no side stream beside them)
template <int BM, int BN>
static void launch_glds(const IgParams& p, int maxM, hipStream_t st) {
  if (!p.fwd && (*p.pol)[kGldsDgradStages] == 2) launch_glds_ns<BM, BN, 2>(p, maxM, st);
  else launch_glds_ns<BM, BN, 3>(p, maxM, st);
}

// policy key 8: smallest K (taps*C) served by the glds kernel (0 = off); 512 -> 1024 after the
// non-temporal epilogue stores (convbench B=64: fwd+dgrad 5.32 -> 5.20 ms). Key 9: fewest workgroups.
bool igemm_glds_ok(const IgParams& p, int maxM, int maxK) {
  const int min_k = (*p.pol)[kGldsMinK];
  if (min_k <= 0 || p.stem || p.pro_scale || p.ap.y || (!p.fwd && !(*p.pol)[kGldsDgrad]) || maxK < min_k || p.Cin % 64 || p.lda % 8 ||
      p.ldb % 8 || maxM < (*p.pol)[kGldsMinRows])
    return false;
  if (p.stats && p.stat_tile != 128 && p.stat_tile != 64) return false;
  for (int i = 0; i < p.nphase; ++i)
    if (p.ph[i].K % 64) return false;
  // measured (tools/convbench.py): a win only with >= one 8-wave workgroup per CU; the 4-wave
  // 256x64 tile and sub-CU-count grids lose to the register-staged kernel
  return !(p.N % 128 || cdiv(maxM, 256) * (p.N / 128) < (*p.pol)[kGldsMinGrid]);
}

bool igemm_glds_launch(const IgParams& p, int maxM, int maxK, hipStream_t st) {
  if (!igemm_glds_ok(p, maxM, maxK)) return false;
  launch_glds<256, 128>(p, maxM, st);
  return true;
}

}  // namespace argus
