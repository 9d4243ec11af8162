// Per-pair outcome profiles of the all-pairs bilinear head for gfx950 (mdg_bilinear_profile).
//
//   S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j];  for every eligible pair (i, j), over the n_labels outcomes of the call:
//     count[i,j]  = #{l : S[l,i,j] >= thr[l]}
//     margin[i,j] = max_l u_l,  u_l = (S[l,i,j] - thr[l]) * scale[l]      (a subtract, then a multiply, each rounded to fp32)
//     best[i,j]   = the smallest l that attains the maximum (-1 if no u_l ever exceeded -inf)
//
// The sweep of bilinear.hip with the loop order turned round.  Every other in-sweep product (top-k, bincount, select) runs one
// workgroup per (row block, outcome) and reduces over pairs; the reduction here runs over the outcomes, which those grids spread
// across blockIdx.y.  So a workgroup here holds a TILE OF PAIRS -- 256 head rows (8 waves x 32) x 64 tail columns -- walks the
// outcomes in ascending order and keeps the per-pair state in registers:
//   resident   the 64 tail rows in LDS (staged once), the wave's 32 z_head rows as the A fragment Az in registers;
//   per l      W_sym[l] arrives by LDS-DMA in two halves (buffers W0 / W1) while the products of outcome l-1 run; the wave forms
//              its 32 rows of T = z_head W_sym[l] exactly as the sweep's prologue does (the tile product over the two halves, bounced
//              through the wave's fp32 slab, afrag_from_slab), multiplies them against the resident tile (the same accumulator
//              layout) and updates, per accumulator element, one packed u32 (count << 16 | best + 1) and one fp32 margin.  The tile
//              product is compute_tile_spread with an empty store hook: compute_tile's MFMA sequence per accumulator with the
//              operand reads pinned one step ahead, where compute_tile lets all of a tile's reads be hoisted (64-128 registers);
//   end        three plain vector stores per element, lane = column (128-byte segments).  No atomics, no LDS beyond the buffers
//              named here; nothing depends on timing: bit-identical from launch to launch.
// Arithmetic: per accumulator element the MFMA sequence of T and of the score is the general sweep's (bilinear_allpairs_kernel,
// STORE: same fragments, same k order, same rounding of T to the operand format), in ALL FOUR precisions -- the single-product
// 16-bit modes run the 32x32x16 path here too, not the 16x16x32 regrouping of the row-statistics sweeps -- so every compared score
// equals mdg_bilinear_allpairs' STORE tensor bit for bit in F32, BF16X3, BF16 and F16.
// Synchronisation per outcome (all LDS-DMA of a wave is retired by a full `s_waitcnt vmcnt(0)`: the kernel has no other
// vector-memory traffic in flight inside the loop, its stores come after it):
//   s_waitcnt vmcnt(0); s_barrier     (A) W_sym[l] (and, for l = 0, the resident tile) has landed for every wave
//   T from W0 / W1 -> slab -> At      slabs are wave-private: a wavefront fence and wave barrier order their write and read
//   s_waitcnt lgkmcnt(0); s_barrier   (B) every wave has finished reading W0 / W1
//   issue the DMA of W_sym[l+1]       lands under the products below and under the other waves' tails of (B)
//   products with the resident tile, state update
// Eligibility does not depend on l: a wave whose tile lies wholly on or above the diagonal (LOWER) does no product work at all,
// a tile the diagonal crosses carries a 32-bit per-lane mask computed once, every other tile is `plain`.  An ineligible element
// becomes NaN before the update (never counted, never best) and its state stays at the sentinels count 0 / best -1 / margin -inf,
// which is what is stored for it.  A workgroup whose whole tile is ineligible stores the sentinels and leaves.
// LDS: W0 + W1 (2 x 32 KB) + 8 slabs (64 KB) + the resident tile (32 KB) = 160 KB, one workgroup per CU.
// Registers: Az + At + accumulators + state = 224 of the 256 a wave has here (f32 / bf16x3); the kernel must compile to ZERO scratch
// (check with -Rpass-analysis=kernel-resource-usage; DESIGN.md 4w has the figures and what it took).
#include "bilinear_tiles.h"

#include <math.h>
#include <vector>

namespace {

struct ProfileArgs {
  const float* z_head;
  TileSrc zt;
  TileSrc w;                  // W_sym (this call's labels); nrows = D
  const float* thr;           // [n_labels]
  const float* scale;         // [n_labels] or null (all ones)
  int* count;                 // [n_head, ldo]
  int* best;
  float* margin;
  int64_t n_head, n_tail, ldo;
  int n_labels;
  int eligible;               // mdg_topk_eligible
};

constexpr int PROFILE_LDS = 2 * STAGE_BYTES + 8 * 8192 + STAGE_BYTES;
constexpr int PROFILE_BM = 256;

// glds16 (bilinear_tiles.h) with the source as scalar base + 32-bit lane offset; M0 is set and restored in the same statement.
__device__ __forceinline__ void profile_glds16(unsigned voff, const void* sbase, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_dst_uniform)
               : "memory");
}

// x, through a register the optimiser cannot see into: what is computed from the result stays where it is computed.
__device__ __forceinline__ int profile_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <int MODE>
__global__ __launch_bounds__(512, 1) void bilinear_profile_kernel(const ProfileArgs p) {
  constexpr int NW = 8, BM = PROFILE_BM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf0 = smem;
  char* const wbuf1 = smem + STAGE_BYTES;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  char* const slab = smem + 2 * STAGE_BYTES + wave * 8192;       // [32 rows][64 cols] fp32, chunk-swizzled
  char* const res = smem + 2 * STAGE_BYTES + 8 * 8192;
  const int mode = p.eligible;
  // LOWER: the last row block has the most column tiles below the diagonal -- it goes first
  const int64_t rbk = mode == MDG_TOPK_LOWER ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int64_t row0 = rbk * BM, tcol0 = static_cast<int64_t>(blockIdx.x) * BN;
  // this wave's rows: wrow0 .. wrow0 + 31 (in a scalar register: the branches on it below are wave-uniform)
  const int64_t wrow0 = row0 + __builtin_amdgcn_readfirstlane(wave) * 32;

  unsigned cb[2][16];                            // count << 16 | best + 1 of element (t, v)
  float mg[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) { cb[t][v] = 0u; mg[t][v] = -INFINITY; }

  // LOWER: column j is eligible for row i when j < i.  Workgroup-uniform: nothing of the tile is (no barrier has been met yet)
  const bool wg_work = p.n_labels > 0 && !(mode == MDG_TOPK_LOWER && tcol0 >= row0 + BM - 1);
  // wave-uniform: nothing of the tile is eligible for my rows, or my rows do not exist
  const bool active = wg_work && wrow0 < p.n_head && !(mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31);

  if (wg_work) {
    // W_sym[l] by LDS-DMA: the pieces stage_dma would issue (same LDS image, same source swizzle), but W has exactly D rows -- no
    // row clamp -- and a lane's source offset inside W_sym[l] is the same for every l and, up to a constant, for every piece of
    // the wave: ONE 32-bit register `woff` for the whole kernel, the rest is scalar (base of the outcome + piece constant).
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const unsigned smem_lds = lds_addr(smem);
    unsigned woff;
    if constexpr (MODE == MDG_PREC_F32) {
      const int row = 2 * wave + (lane >> 5);                     // piece p = wave + 8 i holds rows 2 p, 2 p + 1: row & 15 does not depend on i
      woff = static_cast<unsigned>(row * 512 + (((lane & 31) ^ (row & 15)) << 4));
    } else {
      const int row = 4 * wave + (lane >> 4);                     // piece p = wave + 8 i holds rows 4 p .. 4 p + 3
      woff = static_cast<unsigned>(row * 256 + (((lane & 15) ^ (row & 15)) << 4));
    }
    auto w_dma = [&](int64_t l) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const unsigned dst = smem_lds + st * STAGE_BYTES + uwave * 1024;
        if constexpr (MODE == MDG_PREC_F32) {
          const char* const src = reinterpret_cast<const char*>(p.w.f32 + l * D * D) + st * 64 * 512;
#pragma unroll
          for (int i = 0; i < 4; ++i) profile_glds16(woff, src + i * 8192, dst + i * 8192);
        } else {
          const char* const src = reinterpret_cast<const char*>(p.w.hi + l * D * D) + st * 64 * 256;
#pragma unroll
          for (int i = 0; i < 2; ++i) profile_glds16(woff, src + i * 8192, dst + i * 8192);
          if constexpr (MODE == MDG_PREC_BF16X3) {
            const char* const srcl = reinterpret_cast<const char*>(p.w.lo + l * D * D) + st * 64 * 256;
#pragma unroll
            for (int i = 0; i < 2; ++i) profile_glds16(woff, srcl + i * 8192, dst + LO_OFF + i * 8192);
          }
        }
      }
    };
    stage_dma<MODE>(p.zt, tcol0, res, wave, lane, NW);
    w_dma(0);

    AFrag<MODE> Az;
    {
      int64_t zr = wrow0 + r;
      zr = zr < p.n_head ? zr : p.n_head - 1;
      afrag_from_global<MODE>(Az, p.z_head + zr * D, h);
    }
    // whole tile eligible for every row of the wave (rows / columns past the end are computed on clamped operands and never stored)
    const bool plain = mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31);
    unsigned emask = 0xFFFFFFFFu;                // bit 16 t + v: element (t, v) is eligible
    if (!plain) {
      const int dcr = static_cast<int>(tcol0 - wrow0);            // |dcr| < 64 + 32 here: the diagonal crosses the tile
      emask = 0u;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int d = dcr + 32 * t + r - acc_row(v, h);         // column - row
          const bool ok = mode == MDG_TOPK_NOT_SELF ? d != 0 : d < 0;
          emask |= (ok ? 1u : 0u) << (16 * t + v);
        }
    }

    const int L = p.n_labels;
    for (int l = 0; l < L; ++l) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();              // (A)
      // (uniform values, moved to scalar registers)
      const float thr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.thr[l])));
      const float scl = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.scale ? p.scale[l] : 1.0f)));
      // The LDS addresses of the loop body (operand reads, slab writes and reads: some 60 distinct swizzled offsets per lane) do not
      // depend on l, and hoisted out of the loop they would occupy registers the state needs.  An opaque zero added to the lane
      // index keeps their arithmetic inside the iteration, next to its use.
      // Likewise between the three phases of an iteration (T half 0, T half 1, products), which would share them.
      AFrag<MODE> At;
      if (active) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          __builtin_amdgcn_sched_barrier(0);     // keeps the operand reads of one phase from being hoisted into the one before (registers)
          const int ol = profile_opaque(lane), r = ol & 31, h = ol >> 5;
          f32x16 acc[2];
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
          compute_tile_spread<MODE>(Az, st == 0 ? wbuf0 : wbuf1, r, h, acc, [](int) {});
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
              const int row = acc_row(v, h), n = 32 * t + r;
              *reinterpret_cast<float*>(slab + tile_off<256>(row, n >> 2) + (n & 3) * 4) = acc[t][v];
            }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          afrag_from_slab<MODE>(At, slab, st, r, h);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();       // the slab is read before the next half (or outcome) overwrites it
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();              // (B)
      if (l + 1 < L) w_dma(l + 1);
      if (active) {
        const int ol = profile_opaque(lane), r = ol & 31, h = ol >> 5;
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
        compute_tile_spread<MODE>(At, res, r, h, acc, [](int) {});
        __builtin_amdgcn_sched_barrier(0);
        if (!plain) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = ((emask >> (16 * t + v)) & 1u) ? acc[t][v] : __builtin_nanf("");
        }
        const unsigned tag = static_cast<unsigned>(l) + 1u;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float x = acc[t][v];
            cb[t][v] += x >= thr ? 0x10000u : 0u;
            const float u = (x - thr) * scl;
            const bool up = u > mg[t][v];
            mg[t][v] = up ? u : mg[t][v];
            cb[t][v] = up ? ((cb[t][v] & 0xFFFF0000u) | tag) : cb[t][v];
          }
      }
    }
  }

  // every entry of the tile inside [n_head, n_tail): the profile, or the sentinels the state started from
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int64_t col = tcol0 + 32 * t + r;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = wrow0 + acc_row(v, h);
      if (row < p.n_head && col < p.n_tail) {
        const int64_t o = row * p.ldo + col;
        p.count[o] = static_cast<int>(cb[t][v] >> 16);
        p.best[o] = static_cast<int>(cb[t][v] & 0xFFFFu) - 1;
        p.margin[o] = mg[t][v];
      }
    }
  }
}

template <int MODE>
int launch_profile(ProfileArgs& a, const float* z_tail, const float* w_sym, char* ws, hipStream_t st) {
  const char* const fn = "mdg_bilinear_profile";
  make_head_images<MODE>(a.zt, a.w, z_tail, w_sym, a.n_tail, a.n_labels, ws, st);
  MDG_CHECK_LAUNCH(fn);
  // the whole LDS of a CU: above the default limit of dynamic LDS
  const int rc = mdg_raise_dynamic_lds(reinterpret_cast<const void*>(bilinear_profile_kernel<MODE>), PROFILE_LDS, fn);
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_tail, BN)), static_cast<unsigned>(mdg_cdiv(a.n_head, PROFILE_BM)));
  hipLaunchKernelGGL((bilinear_profile_kernel<MODE>), grid, dim3(512), PROFILE_LDS, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

}  // namespace

extern "C" size_t mdg_bilinear_profile_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision) {
  (void)n_head;
  return head_images_workspace_bytes(n_tail, n_labels, D_, precision);
}

extern "C" int mdg_bilinear_profile(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const float* scale,
                                    int32_t* count, int32_t* best, float* margin, int64_t ldo, int64_t n_head, int64_t n_tail,
                                    int64_t n_labels, int64_t D_, int precision, int eligible, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* const fn = "mdg_bilinear_profile";
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || eligible == MDG_TOPK_NOT_SELF || eligible == MDG_TOPK_LOWER, "%s: unknown eligible mode %d", fn,
                eligible);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "%s: negative size", fn);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail,
                "%s: eligible NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)", fn, (long long)n_head,
                (long long)n_tail);
  MDG_CHECK_ARG(D_ == D, "%s: D must be %d (got %lld)", fn, D, (long long)D_);
  MDG_CHECK_ARG(n_labels <= 65535, "%s: n_labels %lld > 65535 per call", fn, (long long)n_labels);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "%s: n_tail %lld does not fit the int32 tile indices", fn, (long long)n_tail);
  MDG_CHECK_ARG(n_head <= int64_t(65535) * PROFILE_BM, "%s: n_head %lld > %lld rows per call", fn, (long long)n_head,
                (long long)(int64_t(65535) * PROFILE_BM));
  MDG_CHECK_ARG(ldo >= n_tail, "%s: ldo %lld < n_tail %lld", fn, (long long)ldo, (long long)n_tail);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3 || precision == MDG_PREC_BF16 || precision == MDG_PREC_F16,
                "%s: unknown precision %d", fn, precision);
  if (n_head == 0 || n_tail == 0) return MDG_OK;
  MDG_CHECK_ARG(count && best && margin, "%s: null output pointer", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_labels > 0) {
    MDG_CHECK_ARG(z_head && z_tail && w_sym && thr, "%s: null pointer", fn);
    MDG_CHECK_ARG(mdg_aligned16(z_head) && mdg_aligned16(z_tail) && mdg_aligned16(w_sym), "%s: z_head, z_tail and w_sym must be 16-byte aligned",
                  fn);
    const size_t need = mdg_bilinear_profile_workspace_bytes(n_head, n_tail, n_labels, D_, precision);
    if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
      mdg_set_error("%s: workspace of %zu bytes (16-byte aligned) required, got %zu", fn, need, workspace_bytes);
      return MDG_EWORKSPACE;
    }
    // the cuts and scales are read back (at most 2 x 256 KB) and checked before anything is launched
    std::vector<float> host(static_cast<size_t>(n_labels) * (scale ? 2 : 1));
    hipError_t e = hipMemcpyAsync(host.data(), thr, static_cast<size_t>(n_labels) * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && scale) e = hipMemcpyAsync(host.data() + n_labels, scale, static_cast<size_t>(n_labels) * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      mdg_set_error("%s: reading thr / scale back failed: %s", fn, hipGetErrorString(e));
      return MDG_ELAUNCH;
    }
    for (int64_t l = 0; l < n_labels; ++l) {
      MDG_CHECK_ARG(!isnan(host[l]), "%s: thr[%lld] is NaN (use -inf to flag every eligible pair, +inf to flag none)", fn, (long long)l);
      if (scale) {
        const float s = host[n_labels + l];
        MDG_CHECK_ARG(isfinite(s) && s > 0.f, "%s: scale[%lld] = %g is not finite and positive", fn, (long long)l, (double)s);
      }
    }
  }
  ProfileArgs a{};
  a.z_head = z_head;
  a.thr = thr;
  a.scale = scale;
  a.count = count; a.best = best; a.margin = margin;
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.n_labels = static_cast<int>(n_labels);
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  char* ws = static_cast<char*>(workspace);
  // no outcome: the sentinels everywhere (the kernel stages and computes nothing then; the fp32 instantiation needs no images)
  switch (n_labels == 0 ? static_cast<int>(MDG_PREC_F32) : precision) {
    case MDG_PREC_F32: return launch_profile<MDG_PREC_F32>(a, z_tail, w_sym, ws, st);
    case MDG_PREC_BF16X3: return launch_profile<MDG_PREC_BF16X3>(a, z_tail, w_sym, ws, st);
    case MDG_PREC_BF16: return launch_profile<MDG_PREC_BF16>(a, z_tail, w_sym, ws, st);
    default: return launch_profile<MDG_PREC_F16>(a, z_tail, w_sym, ws, st);
  }
}
