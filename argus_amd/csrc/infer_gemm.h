// The tile GEMM of the frozen convs: the one device body behind conv_infer_kernel (conv_infer.hip) and
// conv_infer_dgrad_kernel (conv_infer_bwd.hip), and the host helpers their two launchers share.
//
// It is the register-staged implicit GEMM of conv.hip (swizzled 128-byte LDS rows, LDS double buffer + 2-deep
// register ring) on 64- or 32-row x 64-column tiles, and it splits the reduction over grid.z when the tiles
// alone leave most CUs idle: every slice stores its fp32 accumulators as a slab, takes a ticket on its output
// tile (bnfin.h fin_ticket<kPlainStores>), and the workgroup that draws the last ticket sums the slabs in slice
// order 0..splits-1 (so the result does not depend on arrival order), applies the epilogue and resets the
// ticket. Nobody waits: every other slice exits after its ticket.
//
// A kernel is this body plus two compile-time policies (types, never objects chosen at run time):
//  A policy   which element of the A tensor row i reads at a k-step, and whether it reads one at all:
//               void row(const P&, int i, int m)                 per-row set-up for GEMM row m
//               Step step(const P&, int k0, int ch0)             the k-step's filter tap; Step::ch = the address
//                                                                a predicated-off row loads instead
//               bool at(const P&, const Step&, int i, int& off)  element offset and predicate of row i
//  epilogue   the side operands of an output chunk and what they do to its E fp32 values:
//               void init(const P&, int col)                     per-thread column operands, once
//               void prefetch(const P&, int it, size_t at)       per-row operands, issued before the C tile is read
//               void apply(const P&, int it, float (&f)[E])      f -> what is rounded once and stored
// P is the kernel's by-value parameter struct; its member `g` holds the fields this body reads.
#pragma once
#include <string>

#include "igemm.h"
#include "ktimer.h"

namespace argus {

constexpr int kInferBN = 64;  // output columns per tile

struct InferGemm {
  const void* a;      // the A tensor (NHWC activations); rows are addressed by the A policy
  const void* b;      // [N][brow]: the folded weights, one row per output column
  void* out;          // (M, N)
  float* slabs;       // [tile][split][BM * 64] fp32, in the accumulator's register order
  unsigned* tickets;  // [tile]
  int M, N, brow;     // GEMM rows, columns (= the row length of out and its side operands), B row length
  int nk, splits, ntiles;  // k-steps, slices of them (grid.z), column tiles (N / 64)
};

// (p by value: taken by reference to the kernel's argument, the fp32 64-row kernels compile to 100-104 VGPRs
// instead of 94 and lose a wave of occupancy)
template <typename T, int BM, template <int> class APolicy, template <typename, int> class Epilogue, typename P>
ARGUS_DEV void infer_gemm_tile(const P p) {
  const InferGemm& q = p.g;
  constexpr int E = Chunk<T>::E;
  constexpr int BN = kInferBN;
  constexpr int BKE = 8 * E;  // reduction elements per k-step: one 128-byte LDS row
  constexpr int MI = BM / 32, NI = BN / 32;
  constexpr int AR = BM / 32, BR = BN / 32;
  constexpr int LD = BN + 4;  // fp32 epilogue tile, padded rows (16-byte aligned)
  constexpr int STAGE_B = 2 * (BM + BN) * 128, EPI_B = BM * LD * 4;
  constexpr int LDS_BYTES = STAGE_B > EPI_B ? STAGE_B : EPI_B;
  // the only LDS object: operand staging, then the "last arriver" flag, then the fp32 C tile
  __shared__ __attribute__((aligned(16))) u32x4 lds[LDS_BYTES / 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cidx = tid & 7;
  const int tile = blockIdx.x;
  const int mt = tile / q.ntiles, nt = tile - mt * q.ntiles;
  const T* __restrict__ A = reinterpret_cast<const T*>(q.a);
  const T* __restrict__ B = reinterpret_cast<const T*>(q.b);

  APolicy<AR> ap;
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = mt * BM + (tid >> 3) + 32 * i;
    a_ok[i] = m < q.M;
    ap.row(p, i, a_ok[i] ? m : 0);
  }
  const T* b_row[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) b_row[i] = B + (size_t)(nt * BN + (tid >> 3) + 32 * i) * q.brow + cidx * E;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Stage {
    u32x4 a[AR], b[BR];
    bool ok[AR];
  };

  // a k-step never straddles a filter tap: the channels of the reduction are a multiple of 64 >= BKE
  auto load = [&](int kt, Stage& S) {
    const int k0 = kt * BKE;
    const auto step = ap.step(p, k0, cidx * E);
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int off;
      const bool in = ap.at(p, step, i, off);
      const bool ok = a_ok[i] && in;
      S.a[i] = ld16(A + (ok ? off : step.ch));  // rows that read nothing are zeroed in store()
      S.ok[i] = ok;
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) S.b[i] = ld16(b_row[i] + k0);
  };

  auto store = [&](int buf, Stage& S) {
    u32x4* L = lds + buf * (BM + BN) * 8;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int row = (tid >> 3) + 32 * i;
      L[row * 8 + (cidx ^ swz8(row))] = sel(S.ok[i], S.a[i]);
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int row = (tid >> 3) + 32 * i;
      L[BM * 8 + row * 8 + (cidx ^ swz8(row))] = S.b[i];
    }
  };

  const int g = lane >> 4, i16 = lane & 15;
  auto compute = [&](int buf) {
    const u32x4* L = lds + buf * (BM + BN) * 8;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4 fa[MI], fb[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int row = wm * (BM / 2) + mi * 16 + i16;
        fa[mi] = L[row * 8 + ((4 * s2 + g) ^ swz8(row))];
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = wn * (BN / 2) + ni * 16 + i16;
        fb[ni] = L[BM * 8 + row * 8 + ((4 * s2 + g) ^ swz8(row))];
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) Mma<T>::run(acc[mi][ni], fa[mi], fb[ni]);
    }
  };

  // this slice's k-steps [kb, kb + nk): LDS double buffer + 2-deep register ring (conv.hip's main loop)
  const int z = blockIdx.z;
  const int kb = (int)((long long)z * q.nk / q.splits);
  const int nk = (int)((long long)(z + 1) * q.nk / q.splits) - kb;
  if (nk > 0) {
    Stage S0, S1;
    load(kb, S0);
    store(0, S0);
    if (nk > 1) load(kb + 1, S1);
    if (nk > 2) load(kb + 2, S0);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      compute(0);
      store(1, S1);
      if (kt + 3 < nk) load(kb + kt + 3, S1);
      __syncthreads();
      compute(1);
      if (kt + 2 < nk) {
        store(0, S0);
        if (kt + 4 < nk) load(kb + kt + 4, S0);
      }
      __syncthreads();
    }
    if (kt < nk) {
      compute(0);
      __syncthreads();
    }
  }

  if (q.splits > 1) {
    // slab element ((mi * NI + ni) * 256 + tid) * 4 + r: 16-byte stores, and the reducer's thread tid reads
    // back exactly the registers it would have held
    constexpr int SLAB = BM * BN;
    float* slab = q.slabs + ((size_t)tile * q.splits + z) * SLAB;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        *reinterpret_cast<f32x4*>(slab + ((mi * NI + ni) * 256 + tid) * 4) = acc[mi][ni];
    const bool last = fin_ticket<kPlainStores>(q.tickets + tile, (unsigned)q.splits, reinterpret_cast<int*>(lds));
    __syncthreads();  // the flag word is part of the C tile below
    if (!last) return;
    // fixed-order sum of the slabs 0..splits-1 (this workgroup's own included); loads in batches of 4
    // (clamped addresses, x + 0 = x selects: common.h kLoadBatch), so a batch pays one memory latency
    const float* base = q.slabs + (size_t)tile * q.splits * SLAB;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < q.splits; z0 += 4) {
      f32x4 v[4][MI][NI];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int zz = z0 + u < q.splits ? z0 + u : q.splits - 1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            v[u][mi][ni] = *reinterpret_cast<const f32x4*>(base + (size_t)zz * SLAB + ((mi * NI + ni) * 256 + tid) * 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool on = z0 + u < q.splits;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[mi][ni] += on ? v[u][mi][ni] : zero;
          }
      }
    }
  }

  // ---- epilogue: fp32 C tile through LDS; the policy's arithmetic in fp32, rounded once ----
  float* Cs = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Cs[(wm * (BM / 2) + mi * 16 + g * 4 + r) * LD + wn * (BN / 2) + ni * 16 + i16] = acc[mi][ni][r];
  __syncthreads();
  constexpr int CPR = BN / E;     // 16-byte output chunks per row
  constexpr int RPP = 256 / CPR;  // rows per pass
  constexpr int NIT = BM / RPP;
  static_assert(NIT * RPP == BM, "epilogue row partition");
  const int c = tid % CPR;
  const int col = nt * BN + c * E;
  Epilogue<T, NIT> epi;
  epi.init(p, col);
  T* __restrict__ O = reinterpret_cast<T*>(q.out);
  bool ok[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int m = mt * BM + tid / CPR + RPP * it;
    ok[it] = m < q.M;
    if (ok[it]) epi.prefetch(p, it, (size_t)m * q.N + col);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (!ok[it]) continue;
    const int rr = tid / CPR + RPP * it;
    const int m = mt * BM + rr;
    float f[E];
#pragma unroll
    for (int j = 0; j < E; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(Cs + rr * LD + c * E + j);
      f[j] = v.x; f[j + 1] = v.y; f[j + 2] = v.z; f[j + 3] = v.w;
    }
    epi.apply(p, it, f);
    st16(O + (size_t)m * q.N + col, ChunkCvt<T>::pack(f));
  }
}

// ---- host: what the two launchers share ---------------------------------------------------------------
// Checks the split workspace of `who` and fills the split fields of g. `m`: the GEMM as a forward descriptor
// (the data gradient passes its mirror), `hint`: the entry point that reports `need`.
inline int infer_gemm_workspace(InferGemm& g, const argus_conv_desc& m, const char* who, const char* hint, int splits,
                                size_t need, void* ws, size_t ws_bytes) {
  if (splits > 1 && (!ws || ws_bytes < need)) {
    set_error(std::string(who) + ": workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) +
              " needed for " + std::to_string(splits) + " splits (" + hint + ")");
    return ARGUS_ERR_ARG;
  }
  if (splits > 1 && (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error(std::string(who) + ": workspace must be 16-byte aligned");
    return ARGUS_ERR_ARG;
  }
  g.tickets = reinterpret_cast<unsigned*>(ws);
  g.slabs = splits > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + infer_ticket_bytes(m)) : nullptr;
  g.splits = splits;
  return ARGUS_OK;
}

// One launch of a kernel family F { static constexpr const char* name; template <typename T, int BM> static auto
// kernel(); } under its demangled instantiation name (the kernel timer and the committed profiles key on it).
template <typename F, typename T, int BM, typename P>
inline void infer_launch_bm(const P& p, dim3 grid, hipStream_t st) {
  static const std::string name =
      std::string("argus::") + F::name + "<" + type_name<T>() + ", " + std::to_string(BM) + ">";
  timed_launch(name.c_str(), F::template kernel<T, BM>(), grid, dim3(256), st, p);
}

template <typename F, typename T, typename P>
inline void infer_launch(const P& p, int bm, hipStream_t st) {
  const dim3 grid(cdiv(p.g.M, bm) * p.g.ntiles, 1, p.g.splits);
  if (bm == 64) infer_launch_bm<F, T, 64>(p, grid, st);
  else infer_launch_bm<F, T, 32>(p, grid, st);
}

}  // namespace argus
