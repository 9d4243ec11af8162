// Device side of the pair-exclusion mask (layout: pairmask.hip / include/madrigal_hip.h) for the in-sweep products that honour
// it (topk.hip, select.hip): the kernel's view of a mask, the LDS-DMA that brings the words of one 64-column tile next to the
// tile itself, and the bit of an accumulator element.
//
// A sweep wave owns 32 (32x32 MFMA) or 64 (16x16x32) consecutive head rows starting at a multiple of its height, i.e. one or
// two row blocks of the mask, and every column tile is 64 columns: ONE wave-instruction `global_load_lds_dword` per row block
// and tile -- lane c fetches word [row block][tcol0 + c] into LDS word c of the wave's slot -- brings every bit the wave needs
// for the tile, 256 coalesced bytes.  The words travel the way the tile does (LDS-DMA, no VGPR destination, completion on the
// issuing wave's vmcnt), so they join the hand-counted `s_waitcnt vmcnt(N)` chain of the sweep as one (two) more instruction(s)
// per tile group and hipcc never sees a load whose use would make it drain the tiles in flight (a plain global load would: its
// first use waits vmcnt(0)).  After the wait of iteration s the wave reads its own words of tile s with ds_read_b32.
#pragma once
#include "bilinear_tiles.h"

namespace {

struct PairMask {
  const unsigned* words;     // plane 0
  int64_t plane_stride;      // words from the plane of outcome l to that of l + 1; 0: one plane shared by all outcomes
  int64_t ld;                // mdg_pair_mask_ld(n_tail): words per row block
  int64_t nrb;               // row blocks per plane: ceil(n_head / 32)
};

constexpr int PAIRMASK_SLOT = 256;      // bytes one DMA writes: 64 lanes x 4

// LDS-DMA of one dword per lane: LDS destination = wave-uniform base + lane * 4; M0 handled as in glds16.
__device__ __forceinline__ void glds4(const void* gsrc, unsigned lds_dst_uniform) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst_uniform);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(dst)
               : "memory");
}

// Words [rb][tcol0 .. tcol0 + 63] of `plane` -> the 256 bytes at LDS address `lds_dst`.  tcol0 is a multiple of 64 below ld, so
// every lane's column is inside the padded row; a row block past the last one (rows >= n_head only) is clamped onto it, as the
// z_head row is: the read stays inside [0, nrb) x [0, ld).
__device__ __forceinline__ void pairmask_dma(const PairMask& m, const unsigned* plane, int64_t rb, int64_t tcol0, int lane, unsigned lds_dst) {
  rb = rb < m.nrb ? rb : m.nrb - 1;
  glds4(plane + rb * m.ld + tcol0 + lane, lds_dst);
}

__device__ __forceinline__ unsigned pairmask_word(const char* slot, int c) { return *reinterpret_cast<const unsigned*>(slot + 4 * c); }

// Bit `bit` (a compile-time constant after unrolling) of `w`, spread over the word: 0 or 0xFFFFFFFF (one v_bfe_i32).
__device__ __forceinline__ unsigned pairmask_spread(unsigned w, int bit) { return static_cast<unsigned>(static_cast<int>(w << (31 - bit)) >> 31); }

// x, or a NaN (all bits set) where the spread bit is set: two VALU operations per element, no compare.
__device__ __forceinline__ float pairmask_nan_if(float x, unsigned w, int bit) {
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) | pairmask_spread(w, bit));
}

}  // namespace
