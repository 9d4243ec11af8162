// Per-pair outcome profiles over the checkpoint-ensembled all-pairs head for gfx950 (mdg_bilinear_ensemble_profile).
//
//   P[l,i,j] = (sum_{m<K} sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])) / K                                K = 1..8 checkpoints
//   for every eligible pair (i, j), over the n_labels outcomes of the call:
//     count[i,j]  = #{l : P[l,i,j] >= thr[l]}                              (the compare is on the quotient, as in ensemble_select.hip)
//     margin[i,j] = max_l u_l,  u_l = (P[l,i,j] - thr[l]) * scale[l]       (a subtract, then a multiply, each rounded to fp32)
//     best[i,j]   = the smallest l that attains the maximum (-1 if no u_l ever exceeded -inf)
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614, average the sigmoids
// of the checkpoints; "which pairs does the ensemble flag for the most interaction types" is read off that tensor.)  The mean of K
// sigmoids is not monotone in any one model's logit, so neither the counts nor the best outcome can be merged from K single-model
// profiles (profile.hip); here nothing of [L,N,N] is materialised.
//
// Two existing kernels joined: profile.hip's contract and state on ensemble_select.hip's sweep, with that sweep's two outer loops
// interchanged.  There a workgroup owns one outcome and walks its tail tiles; here a workgroup (4 waves, one per SIMD, 128 head
// rows) owns G tail tiles of 64 columns for its whole life and walks the outcomes in ascending order:
//   per l        thr[l] and scale[l] into scalar registers;
//   per (l, m)   build_t: T_m = z_head_m[rows] . W_sym_m[l] (W staged whole in the two stage buffers, the wave's T bounced through
//                its fp32 slab into the A fragment), then the workgroup's tiles of z_tail_m through the two-buffer LDS-DMA ring,
//                compute_tile_spread, sigmoid 1 / (1 + expf(-s)) added to psum[g] (G x 32 VGPRs) in model order;
//   after m=K-1  P = psum / K; elements `eligible` rules out become NaN (ensemble_select.hip's spelling); per accumulator element
//                one packed u32 (count << 16 | best + 1, hence n_labels <= 65535 per call) and one fp32 margin are updated, the
//                margin only on u > margin: the lowest l of a tie stays.  A NaN is never counted and never best.
//   end          three plain vector stores per element, lane = column (128-byte segments), once, after the loop.
// build_t, pick, sigmoid_head, the eligibility test and the layout's constants are ensemble_sweep.h's, shared by the family; the
// ring is this file's own text (sharing sweep text has moved hipcc's schedule before).  The score arithmetic per
// accumulator element is therefore ensemble.hip's general (non-symmetric) sweep bit for bit, in F32 and BF16X3.
// Grid = (column groups, row blocks), column groups fastest: the resident workgroups walk l in step and share each W_sym_m[l] and
// the models' tail images in L2.  LOWER: row blocks are reversed (the last one has the most work); a workgroup wholly on or above
// the diagonal stores the sentinels 0 / -1 / -inf and leaves before any barrier; tiles right of the workgroup's last row are not
// swept by any wave (workgroup-uniform), a wave skips the products of a tile right of ITS last row (wave-uniform, it still meets
// every barrier).  The state of an element that is never updated is the sentinels, which is what is stored for it.
// Waits.  Every stage barrier waits vmcnt(0): the only vector-memory operations a wave has in flight inside the loop are the
// LDS-DMAs of the tile about to be read and build_t's own loads; the stores come after the loop.
// No atomics, no LDS beyond the stage buffers and the slabs (96 KiB): bit-identical from launch to launch.
// Registers: T 64 + accumulators 32 + psum 32 G + state 64 G of the 512 a wave has at one wave per SIMD; the kernel must compile to
// ZERO scratch (check with -Rpass-analysis=kernel-resource-usage; DESIGN.md 4aj has the table).
#include "ensemble_sweep.h"

#include <math.h>
#include <vector>

namespace {

constexpr int ENS_PRO_G = 3;                // tail tiles a workgroup owns (the register table behind the choice)
constexpr int ENS_PRO_BM = 32 * ENS_NW;

struct EnsProArgs : EnsOperands {
  const float* thr;            // [n_labels]
  const float* scale;          // [n_labels] or null (all ones)
  int* count;                  // [n_head, ldo]
  int* best;
  float* margin;
  int64_t n_head, n_tail, ldo;
  int n_labels;
  int n_models;
  int eligible;                // mdg_topk_eligible
};

template <int MODE, int G>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_profile_kernel(const EnsProArgs p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = ENS_PRO_BM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.n_models, mode = p.eligible, L = p.n_labels;
  const float kf = static_cast<float>(K);
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  // LOWER: the last row block has the most column tiles below the diagonal -- it goes first
  const int64_t rbk = mode == MDG_TOPK_LOWER ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int64_t row0 = rbk * BM;
  const int64_t col0 = static_cast<int64_t>(blockIdx.x) * (G * BN);       // the workgroup's columns: col0 .. col0 + 64 G - 1
  const int64_t wrow0 = row0 + wave * 32;        // this wave's rows: wrow0 .. wrow0 + 31

  unsigned cb[G][2][16];                         // count << 16 | best + 1 of element (g, t, v)
  float mg[G][2][16];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) { cb[g][t][v] = 0u; mg[g][t][v] = -INFINITY; }

  // Tiles of the group some wave has to sweep (workgroup-uniform): those that start below n_tail and, under LOWER, left of the
  // workgroup's last row (column j is eligible for row i when j < i).  0: nothing of the group is eligible, or there is no outcome
  // -- the workgroup stores the sentinels and leaves; it meets no barrier.
  int ng = 0;
  if (L > 0) {
    const int64_t left = p.n_tail - col0;                                  // >= 1: the grid covers n_tail
    ng = left >= G * BN ? G : static_cast<int>((left + BN - 1) / BN);
    if (mode == MDG_TOPK_LOWER) {
      const int64_t last = (row0 + BM < p.n_head ? row0 + BM : p.n_head) - 1;   // columns [0, last) are eligible for some row
      const int64_t need = last - col0;                                    // columns of the group left of `last`
      const int lim = need <= 0 ? 0 : (need >= G * BN ? G : static_cast<int>((need + BN - 1) / BN));
      ng = ng < lim ? ng : lim;
    }
  }

  if (ng > 0) {
    int64_t zr = wrow0 + (tid & 31);
    zr = zr < p.n_head ? zr : p.n_head - 1;
    AFrag<MODE> At;
    int par = 0;             // stage buffer of the next stage
    for (int l = 0; l < L; ++l) {
      // (uniform values, moved to scalar registers)
      const float thr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.thr[l])));
      const float scl = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.scale ? p.scale[l] : 1.0f)));
      float psum[G][2][16];
      for (int m = 0; m < K; ++m) {
        {
          int t_o = tid;
          asm volatile("" : "+v"(t_o));
          const int r = t_o & 31, h = (t_o >> 5) & 1;
          TileSrc wl = pick(p.w, m);
          if constexpr (MODE == MDG_PREC_F32) wl.f32 += static_cast<int64_t>(l) * D * D;
          else { wl.hi += static_cast<int64_t>(l) * D * D; wl.lo += static_cast<int64_t>(l) * D * D; }
          build_t<MODE, NW>(At, pick(p.z_head, m) + zr * D, wl, smem, slab, t_o, r, h);
        }
        const TileSrc zt = pick(p.zt, m);
        {
          // the group's first tile; the buffer was last read by build_t, and every wave has passed its closing barrier
          int ln = tid & 63;
          asm volatile("" : "+v"(ln));
          stage_dma<MODE>(zt, col0, smem + par * STAGE_BYTES, wave, ln, NW);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (g < ng) {
            // lane-dependent offsets recomputed per stage (hoisted out of the loops they would hold many VGPRs per unrolled stage)
            int lane = tid & 63;
            asm volatile("" : "+v"(lane));
            const int r = lane & 31, h = lane >> 5;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's DMAs
            __builtin_amdgcn_s_barrier();                                       // ... for every wave; every wave is done with the other buffer
            char* const cur = smem + par * STAGE_BYTES;
            char* const nxt = smem + (par ^ 1) * STAGE_BYTES;
            if (g + 1 < ng) stage_dma<MODE>(zt, col0 + static_cast<int64_t>(g + 1) * BN, nxt, wave, lane, NW);
            par ^= 1;
            const int64_t tcol0 = col0 + static_cast<int64_t>(g) * BN;
            // wave-uniform: no column of this tile is below any of my rows.  The wave still meets every barrier above.
            if (!(mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31)) {
              f32x16 acc[2];
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
              compute_tile_spread<MODE>(At, cur, r, h, acc, [](int) {});
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                  const float sg = sigmoid_head(acc[t][v]);
                  psum[g][t][v] = m == 0 ? sg : psum[g][t][v] + sg;
                  if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four sigmoids' temporaries at a time
                }
            }
          }
        }
      }
      // ---- outcome l is complete for every tile of the group: quotient, eligibility, state ----
      {
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int r = lane & 31, h = lane >> 5;
        const unsigned tag = static_cast<unsigned>(l) + 1u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int64_t tcol0 = col0 + static_cast<int64_t>(g) * BN;
          // (wave-uniform) the tile was swept: psum[g] holds this outcome's sums
          if (g < ng && !(mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31)) {
            float pr[2][16];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) {
                pr[t][v] = psum[g][t][v] / kf;                                      // P = sum / K
                if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);               // four divisions' temporaries at a time
              }
            // whole tile eligible for every row of the wave (wave-uniform): no per-element masking
            const bool plain = tcol0 + BN <= p.n_tail && wrow0 + 32 <= p.n_head &&
                               (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
            if (!plain) {
              const int dcr = ens_clamp(tcol0 - wrow0), nr = ens_clamp(p.n_head - wrow0), ncl = ens_clamp(p.n_tail - tcol0);
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v)
                  pr[t][v] = ens_eligible(mode,acc_row(v, h), 32 * t + r, dcr, nr, ncl) ? pr[t][v] : __builtin_nanf("");
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) {
                const float x = pr[t][v];
                cb[g][t][v] += x >= thr ? 0x10000u : 0u;
                const float u = (x - thr) * scl;
                const bool up = u > mg[g][t][v];
                mg[g][t][v] = up ? u : mg[g][t][v];
                cb[g][t][v] = up ? ((cb[g][t][v] & 0xFFFF0000u) | tag) : cb[g][t][v];
              }
          }
        }
      }
    }
  }

  // every entry of the group inside [n_head, n_tail): the profile, or the sentinels the state started from
  {
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int64_t col = col0 + g * BN + 32 * t + r;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t row = wrow0 + acc_row(v, h);
          if (row < p.n_head && col < p.n_tail) {
            const int64_t o = row * p.ldo + col;
            p.count[o] = static_cast<int>(cb[g][t][v] >> 16);
            p.best[o] = static_cast<int>(cb[g][t][v] & 0xFFFFu) - 1;
            p.margin[o] = mg[g][t][v];
          }
        }
      }
  }
}

template <int MODE>
int launch_ens_profile(EnsProArgs& a, const float* const* z_tail, const float* const* w_sym, char* ws, hipStream_t st, const char* fn) {
  if (a.n_labels > 0) {
    const int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, a.n_labels, ws, st, fn);
    if (rc != MDG_OK) return rc;
  }
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_tail, ENS_PRO_G * BN)), static_cast<unsigned>(mdg_cdiv(a.n_head, ENS_PRO_BM)));
  hipLaunchKernelGGL((ensemble_profile_kernel<MODE, ENS_PRO_G>), grid, dim3(64 * ENS_NW), ENS_LDS, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

}  // namespace

extern "C" int mdg_bilinear_ensemble_profile_tiles(void) { return ENS_PRO_G; }

extern "C" size_t mdg_bilinear_ensemble_profile_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_models,
                                                                int precision) {
  (void)n_head;
  return ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
}

extern "C" int mdg_bilinear_ensemble_profile(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                             const float* thr, const float* scale, int32_t* count, int32_t* best, float* margin, int64_t ldo,
                                             int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "mdg_bilinear_ensemble_profile";
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "%s: n_tail %lld does not fit the int32 column indices", fn, (long long)n_tail);
  MDG_CHECK_ARG(n_head <= int64_t(65535) * ENS_PRO_BM, "%s: n_head %lld > %lld rows per call", fn, (long long)n_head,
                (long long)(int64_t(65535) * ENS_PRO_BM));
  MDG_CHECK_ARG(ldo >= n_tail, "%s: ldo %lld < n_tail %lld", fn, (long long)ldo, (long long)n_tail);
  if (n_head == 0 || n_tail == 0) return MDG_OK;
  MDG_CHECK_ARG(count && best && margin, "%s: null output pointer", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_labels > 0) {
    rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, thr != nullptr, n_tail, n_labels, precision, workspace, workspace_bytes);
    if (rc != MDG_OK) return rc;
    // the cuts and scales are read back (at most 2 x 256 KB) and checked before anything is launched, as mdg_bilinear_profile does
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
  EnsProArgs a{};
  ens_fill_operands(a, n_labels > 0 ? z_head : nullptr, n_models, n_tail);
  a.thr = thr;
  a.scale = scale;
  a.count = count; a.best = best; a.margin = margin;
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.n_labels = static_cast<int>(n_labels);
  a.n_models = n_models;
  a.eligible = eligible;
  char* ws = static_cast<char*>(workspace);
  // no outcome: the sentinels everywhere (the kernel stages and computes nothing then; the fp32 instantiation needs no images)
  if (n_labels == 0 || precision == MDG_PREC_F32) return launch_ens_profile<MDG_PREC_F32>(a, z_tail, w_sym, ws, st, fn);
  return launch_ens_profile<MDG_PREC_BF16X3>(a, z_tail, w_sym, ws, st, fn);
}
