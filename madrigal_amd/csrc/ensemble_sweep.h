// What the sweeps over a checkpoint ensemble of the all-pairs head -- ensemble.hip, ensemble_store16.hip, ensemble_topk.hip,
// ensemble_select.hip, ensemble_bincount.hip, ensemble_profile.hip -- share.
//
// In each of them a workgroup owns head rows of one outcome at a time, 32 per wave; per model m it rebuilds T_m = z_head_m[rows] .
// W_sym_m[l] (build_t) and sweeps 64-column tiles of z_tail_m through two stage buffers filled by LDS-DMA, the sigmoids of the
// models summed in registers (ensemble.hip has the arithmetic and the reasons).
//
// Shared here, device side: the constants of that layout, the operand head of the kernel arguments, pick, sigmoid_head, build_t and
// the clamped 32-bit eligibility test -- functions and constants that were functions and constants in every file, so hipcc sees the
// text it saw before (scripts/kernel_text_diff.py: the assembly of the five files is what it was).  Host side, for the four reducing
// products (ensemble.hip has a launch side of its own: a one-launch split kernel and another image layout): the argument checks,
// the workspace size, the operand head and the per-model operand images.
// NOT shared: the sweep text itself (mask prefetch, ring, waits, the sums into psum).  Each kernel carries it, as the single-model
// sweeps do (sweep_reduce.h); DESIGN.md 4ak has what the one attempt at sharing it did.
#pragma once
#include "sweep_reduce.h"

namespace {

constexpr int MAXK = 8;                // checkpoints per call
constexpr int SLAB_BYTES = 8192;       // per wave: [32 rows][64 columns] fp32 (T half while rebuilding, finished tile when mirroring)
// The K >= 2 layout: 4 waves per workgroup, one per SIMD (512 VGPRs: T, the running sums, the product's state), two stage buffers and
// one slab per wave.  (ensemble.hip's K = 1 kernel runs 8 waves: kWaves / kLds there.)
constexpr int ENS_NW = 4;
constexpr int ENS_CH = 6;              // tail tiles per chunk (running sums: 6 x 32 VGPRs; T rebuilt for a third of the chunk's MFMA work)
constexpr int ENS_LDS = 2 * STAGE_BYTES + ENS_NW * SLAB_BYTES;

// The head of every kernel-argument struct of the family
struct EnsOperands {
  const float* z_head[MAXK];   // fp32 rows (T prologue)
  TileSrc zt[MAXK];            // tail operand images (fp32, or hi/lo bf16)
  TileSrc w[MAXK];             // W_sym images, all outcomes; nrows = D
};

// a[k] for a wave-uniform k without dynamic indexing of the kernel arguments (scalar selects)
template <typename T>
__device__ __forceinline__ T pick(const T (&a)[MAXK], int k) {
  T v = a[0];
#pragma unroll
  for (int i = 1; i < MAXK; ++i)
    if (k == i) v = a[i];
  return v;
}

__device__ __forceinline__ float sigmoid_head(float s) { return 1.0f / (1.0f + expf(-s)); }   // MDG_EPI_STORE_SIGMOID's formula

// Eligibility of the element in row wrow0 + lr, column tcol0 + lc of a tile from the tile's 32-bit distances (wave-uniform, clamped):
// dcr = tcol0 - wrow0, nr = n_head - wrow0, nc = n_tail - tcol0.  select.hip's test: col - row keeps its sign and its zero through
// the clamp; a lane's lr and lc differ from element to element by compile-time constants only.
__device__ __forceinline__ int ens_clamp(int64_t x) {
  return static_cast<int>(x < -(int64_t(1) << 30) ? -(int64_t(1) << 30) : (x > (int64_t(1) << 30) ? (int64_t(1) << 30) : x));
}
__device__ __forceinline__ bool ens_eligible(int mode, int lr, int lc, int dcr, int nr, int nc) {
  const int d = dcr + lc - lr;                                                          // column - row
  const bool pair = mode == MDG_TOPK_NOT_SELF ? d != 0 : d < 0;                         // (bitwise: selects, no branches)
  return (lr < nr) & (lc < nc) & ((mode == MDG_TOPK_ALL) | pair);
}

// stage_dma (bilinear_tiles.h) of a workgroup of NW = 4 or 8 waves with the tail rows of the tile permuted on the SOURCE address:
// LDS row 32 t + r <- tail row row0 + 2 r + t (store16.hip's store16_stage_dma).  The LDS image, its swizzle and compute_tile_spread
// are those of stage_dma; lane (r, h) of the product then holds columns 2 r (accumulator tile 0) and 2 r + 1 (tile 1) of the same 16
// rows -- the column pair of one dword of a 16-bit tensor (ensemble_store16.hip).
template <int MODE, int NW>
__device__ __forceinline__ void stage_dma_pairs(const TileSrc& s, int64_t row0, char* lds, int wave, int lane) {
  static_assert(NW == 4 || NW == 8, "the K >= 2 and the K = 1 workgroup");
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int i = 0; i < 32 / NW; ++i) {
      const int p = wave + NW * i;
      const int row = 2 * p + (lane >> 5), c = (lane & 31) ^ (row & 15);
      int64_t gr = row0 + 2 * (row & 31) + (row >> 5);
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.f32 + gr * D + c * 4, lds_addr(lds + p * 1024));
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16 / NW; ++i) {
      const int p = wave + NW * i;
      const int row = 4 * p + (lane >> 4), c = (lane & 15) ^ (row & 15);
      int64_t gr = row0 + 2 * (row & 31) + (row >> 5);
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.hi + gr * D + c * 8, lds_addr(lds + p * 1024));
      if constexpr (MODE == MDG_PREC_BF16X3) glds16(s.lo + gr * D + c * 8, lds_addr(lds + LO_OFF + p * 1024));
    }
  }
}

// T = z_head[32 rows of this wave] . W_sym[l] -> At, the same fp32 values as the head's prologue: per 32-column tile the MFMA
// chain runs over k in the same order with the same products (compute_tile), only the loop nest is k-outer so that the z operand
// is held one k step at a time (8 VGPRs instead of a 64-VGPR fragment: the running sums of the chunk stay resident).  W_sym[l]
// (symmetric: its rows are its columns) is staged whole, rows 0..63 in stage buffer 0 and 64..127 in buffer 1.
template <int MODE, int NW>
__device__ __forceinline__ void build_t(AFrag<MODE>& At, const float* zrow, const TileSrc& wl, char* smem, char* slab, int tid,
                                        int r, int h) {
  {
    u32x4 r0[32 / NW], r1[32 / NW];
    stage_load<MODE, NW>(wl, 0, tid, r0);
    stage_load<MODE, NW>(wl, 64, tid, r1);
    __syncthreads();                                // every wave is done with the stage buffers
    stage_write<MODE, NW>(smem, tid, r0);
    stage_write<MODE, NW>(smem + STAGE_BYTES, tid, r1);
    __syncthreads();
  }
  f32x16 acc[4];                                    // output columns 32 c .. 32 c + 31
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[c][v] = 0.f;
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(zrow + 8 * q + 4 * h);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 b = *reinterpret_cast<const float4*>(smem + (c >> 1) * STAGE_BYTES + tile_off<512>(32 * (c & 1) + r, 2 * q + h));
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[c], 0, 0, 0);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[c], 0, 0, 0);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[c], 0, 0, 0);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[c], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // one k step of operands live at a time
    }
  } else {
    static_assert(MODE == MDG_PREC_BF16X3, "fp32 and split-bf16 operands");
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float4 v0 = *reinterpret_cast<const float4*>(zrow + 16 * s + 8 * h);
      const float4 v1 = *reinterpret_cast<const float4*>(zrow + 16 * s + 8 * h + 4);
      bf16x8 ahi, alo;
      split8<MODE>(v0, v1, ahi, alo);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const char* lds = smem + (c >> 1) * STAGE_BYTES;
        const int j = 32 * (c & 1) + r;
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(j, 2 * s + h));
        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(lds + LO_OFF + tile_off<256>(j, 2 * s + h));
        acc[c] = mma16<MODE>(alo, bh, acc[c]);
        acc[c] = mma16<MODE>(ahi, bl, acc[c]);
        acc[c] = mma16<MODE>(ahi, bh, acc[c]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // T (fp32) -> this wave's slab, one 64-column half at a time, and back as the A fragment (the head's afrag_from_slab)
#pragma unroll
  for (int st = 0; st < 2; ++st) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = acc_row(v, h), n = 32 * t + r;
        *reinterpret_cast<float*>(slab + tile_off<256>(row, n >> 2) + (n & 3) * 4) = acc[2 * st + t][v];
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    afrag_from_slab<MODE>(At, slab, st, r, h);
  }
  __syncthreads();                                  // every wave is done reading W from the stage buffers
}

// ---- launch side of the reducing products (top-k, select, bincount, profile) ---------------------------------------------------
// Per model the operand images of the single-model head, one after the other.
inline size_t ens_workspace_bytes(int64_t n_tail, int64_t n_labels, int64_t D_, int n_models, int precision) {
  if (n_models <= 0) return 0;
  return static_cast<size_t>(n_models) * head_images_workspace_bytes(n_tail, n_labels, D_, precision);
}

// The size checks the four products share; `fn` is the entry point's name, so every message reads as the product's own.
inline int ens_check_sizes(const char* fn, int n_models, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision,
                           int eligible) {
  MDG_CHECK_ARG(n_models >= 1 && n_models <= MAXK, "%s: n_models must be in 1..%d (got %d)", fn, MAXK, n_models);
  const int rc = sweep_check_sizes(fn, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3, "%s: precision %d not offered (MDG_PREC_F32 or MDG_PREC_BF16X3)", fn,
                precision);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail, "%s: NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)",
                fn, (long long)n_head, (long long)n_tail);
  return MDG_OK;
}

// The operands of a sweep that launches: a column to sweep, no null pointer (`others`: the product's own pointers), every model's
// arrays aligned, and a workspace for the images.
inline int ens_check_operands(const char* fn, const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                              bool others, int64_t n_tail, int64_t n_labels, int precision, const void* workspace, size_t workspace_bytes) {
  MDG_CHECK_ARG(n_tail >= 1, "%s: n_tail must be at least 1", fn);
  MDG_CHECK_ARG(z_head && z_tail && w_sym && others, "%s: null pointer", fn);
  for (int m = 0; m < n_models; ++m) {
    MDG_CHECK_ARG(z_head[m] && z_tail[m] && w_sym[m], "%s: null pointer for model %d", fn, m);
    MDG_CHECK_ARG(mdg_aligned16(z_head[m]) && mdg_aligned16(z_tail[m]) && mdg_aligned16(w_sym[m]),
                  "%s: z_head, z_tail and w_sym must be 16-byte aligned (model %d)", fn, m);
  }
  const size_t need = ens_workspace_bytes(n_tail, n_labels, D, n_models, precision);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("%s: workspace of %zu bytes (16-byte aligned) required, got %zu", fn, need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  return MDG_OK;
}

// The operand head of the kernel arguments, but for the image pointers; unused slots repeat model 0 (never read).  A null `z_head`
// (a call without outcomes) leaves the rows null.
inline void ens_fill_operands(EnsOperands& a, const float* const* z_head, int n_models, int64_t n_tail) {
  for (int m = 0; m < MAXK; ++m) {
    a.z_head[m] = z_head ? z_head[m < n_models ? m : 0] : nullptr;
    a.zt[m].nrows = n_tail;
    a.w[m].nrows = D;
  }
}

// The models' operand images (zhi | whi | zlo | wlo per model) made in `ws` on the stream, and the image pointers of the head;
// `what` names the step in the message of a failed launch.
template <int MODE>
int ens_make_images(EnsOperands& a, const float* const* z_tail, const float* const* w_sym, int n_models, int64_t n_tail, int64_t n_labels,
                    char* ws, hipStream_t st, const char* what) {
  const size_t per = head_images_workspace_bytes(n_tail, n_labels, D, MODE);
  for (int m = 0; m < n_models; ++m) make_head_images<MODE>(a.zt[m], a.w[m], z_tail[m], w_sym[m], n_tail, n_labels, ws ? ws + m * per : nullptr, st);
  MDG_CHECK_LAUNCH(what);
  for (int m = n_models; m < MAXK; ++m) { a.zt[m] = a.zt[0]; a.w[m] = a.w[0]; }      // unused slots repeat model 0 (never read)
  return MDG_OK;
}

}  // namespace
