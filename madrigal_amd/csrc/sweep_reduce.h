// What the row-owning reducing sweeps of the all-pairs head -- topk.hip, select.hip, bincount.hip -- share.
//
// In each of them a workgroup of 8 waves owns BM head rows of one outcome l (blockIdx.y) and walks the 64-column tiles of z_tail in
// ascending order through three stage buffers filled by LDS-DMA with prefetch distance two; every head row belongs to ONE wave.  The
// score arithmetic is that of the row-statistics sweeps of bilinear.hip (`bilinear_allpairs_kernel<MODE, ROWSTATS, 8>` for f32 /
// bf16x3, `bilinear_rowstats16_kernel` for the single-product 16-bit modes).
//
// Shared here: the 16x16x32 MFMA wrapper, the tile count under LOWER, the LDS layout behind the stage buffers (mask slots, then a
// product's own tables) and the whole launch side: argument checks, mask arguments, the dynamic-LDS limit and the launch.
// NOT shared: the sweep text itself (prologue, ring, waits).  Each kernel carries it, because every way of sharing it that was tried
// -- the epilogue as a callable, the ring as a stepped object, the prologue as a function -- moved hipcc's schedule and cost
// 0.2 - 2.9 % in some instantiation.
#pragma once
#include "pairmask.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4v;

template <int MODE>
__device__ __forceinline__ f32x4v mma16x16(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
  if constexpr (MODE == MDG_PREC_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

constexpr int SWEEP_NW = 8;        // waves per workgroup

// LDS of a MASKED sweep behind the three stage buffers: per stage buffer and wave, NMW slots of 256 bytes -- the mask words of the
// wave's row block(s) for the 64 columns of that buffer's tile (NMW = 1 on 32x32, 2 on 16x16x32).  sweep_lds_bytes is also where a
// product's own LDS starts (bincount's edge and counter tables).
template <int NMW> constexpr int sweep_mask_stage = SWEEP_NW * NMW * PAIRMASK_SLOT;
template <bool MASKED, int NMW> constexpr int sweep_lds_bytes = 3 * STAGE_BYTES + (MASKED ? 3 * sweep_mask_stage<NMW> : 0);

// column tiles a workgroup with head rows [row0, row0 + BM) has to visit: LOWER needs columns j <= last row - 1 only
__device__ __forceinline__ int sweep_tiles(int eligible, int64_t row0, int BM, int64_t n_head, int64_t n_tail) {
  const int nst = static_cast<int>((n_tail + BN - 1) / BN);
  if (eligible != MDG_TOPK_LOWER) return nst;
  const int64_t last = (row0 + BM < n_head ? row0 + BM : n_head) - 1;      // columns [0, last) are eligible for some row
  const int need = static_cast<int>((last + BN - 1) / BN);
  return need < 1 ? 1 : (need < nst ? need : nst);
}

// ---- launch side ------------------------------------------------------------------------------------------------------------
// The argument checks the three products share; `fn` is the entry point's name, so every message reads as the product's own.
inline int sweep_check_sizes(const char* fn, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible) {
  MDG_CHECK_ARG(D_ == D, "%s: D must be %d (got %lld)", fn, D, (long long)D_);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "%s: negative size", fn);
  MDG_CHECK_ARG(n_labels <= 65535, "%s: n_labels %lld > 65535 per call", fn, (long long)n_labels);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || eligible == MDG_TOPK_NOT_SELF || eligible == MDG_TOPK_LOWER, "%s: unknown eligible mode %d", fn,
                eligible);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3 || precision == MDG_PREC_BF16 || precision == MDG_PREC_F16,
                "%s: unknown precision %d", fn, precision);
  return MDG_OK;
}

// The operands of a sweep that launches: not null (`others`: the product's own pointers), aligned, and a workspace for the images.
inline int sweep_check_operands(const char* fn, const float* z_head, const float* z_tail, const float* w_sym, bool others, int64_t n_tail,
                                int64_t n_labels, int precision, const void* workspace, size_t workspace_bytes) {
  MDG_CHECK_ARG(z_head && z_tail && w_sym && others, "%s: null pointer", fn);
  MDG_CHECK_ARG(mdg_aligned16(z_head) && mdg_aligned16(z_tail) && mdg_aligned16(w_sym), "%s: z_head, z_tail and w_sym must be 16-byte aligned", fn);
  const size_t need = head_images_workspace_bytes(n_tail, n_labels, D, precision);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("%s: workspace of %zu bytes (16-byte aligned) required, got %zu", fn, need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  return MDG_OK;
}

// The mask arguments of the *_masked / *_split entry points, checked and put into the kernel argument.
inline int sweep_mask_args(const char* fn, PairMask& m, const uint32_t* mask, int64_t plane_stride, int64_t n_head, int64_t n_tail) {
  MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(mask) & 3u) == 0, "%s: mask must be 4-byte aligned", fn);
  MDG_CHECK_ARG(plane_stride == 0 || plane_stride >= mdg_pair_mask_plane_words(n_head, n_tail),
                "%s: plane_stride %lld is neither 0 (shared plane) nor >= the %lld words of a plane", fn, (long long)plane_stride,
                (long long)mdg_pair_mask_plane_words(n_head, n_tail));
  m.words = mask;
  m.plane_stride = plane_stride;
  m.ld = mdg_pair_mask_ld(n_tail);
  m.nrb = mdg_cdiv(n_head, 32);
  return MDG_OK;
}

// Launch of a product's sweep kernel `k` of the layout with NMW * 32 rows per wave; `extra`: the product's own LDS behind
// sweep_lds_bytes.  A masked sweep uses more dynamic LDS than the default limit.
template <bool MASKED, int NMW, typename KA>
int sweep_launch(void (*k)(KA), const KA& a, int64_t n_labels, int extra, hipStream_t st, const char* fn) {
  constexpr int lds = sweep_lds_bytes<MASKED, NMW>;
  if constexpr (MASKED) {
    const int rc = mdg_raise_dynamic_lds(reinterpret_cast<const void*>(k), lds + extra, fn);
    if (rc != MDG_OK) return rc;
  }
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * NMW * SWEEP_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL(k, grid, dim3(64 * SWEEP_NW), lds + extra, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

}  // namespace
