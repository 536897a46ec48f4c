// LDS-DMA primitives of the kernels that fill LDS with global_load_lds (conv_glds.hip, conv_halo.hip,
// conv_wgdma.hip): counted vmcnt waits, the 16-byte DMA, the compiler-fenced barrier, the zero page that
// out-of-range rows read, and the 32-byte-slot swizzle of the pixel-major weight-gradient images.
#pragma once
#include "common.h"

namespace argus {

namespace {
// 64 zero bytes (static storage); one per translation unit: the build has no relocatable device code
// (conv.hip includes this header for swz32 alone: there the page is unused and internal, so it is dropped)
__device__ __attribute__((aligned(64))) u32x4 lds_dma_zero_page[4];
}  // namespace

// s_waitcnt vmcnt(N) with expcnt / lgkmcnt left at their maxima (gfx9 encoding).
template <int N> ARGUS_DEV void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}

// vmcnt(min(n, K) * D) for a runtime n: at most n groups of D DMAs each stay in flight
template <int K, int D = 1> ARGUS_DEV void wait_vm_le(int n) {
  if constexpr (K == 0) {
    wait_vm<0>();
  } else {
    if (n >= K) wait_vm<K * D>();
    else wait_vm_le<K - 1, D>(n);
  }
}

// 16 bytes per lane, global -> LDS (the wave's 64 lanes fill 1 KB from lds_byte_addr on)
ARGUS_DEV void lds_dma16(const void* src, uint32_t lds_byte_addr) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(uintptr_t)lds_byte_addr, 16, 0,
                                   0);
}

// s_barrier without the compiler's own waitcnt(0): the counted wait before it orders the DMAs
ARGUS_DEV void lds_dma_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// bf16 LDS image of the weight gradients: rows of 256 B = 8 slots of 32 B; slot XOR swz32(row) makes the
// 8 rows a ds_read_b64_tr_b16 half-wave touches land on 8 distinct slots.
ARGUS_DEV int swz32(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

}  // namespace argus
