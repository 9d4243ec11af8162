// Threshold selection over the checkpoint-ensembled all-pairs head for gfx950 (mdg_bilinear_ensemble_select_count / _fill).
//
//   for every outcome l with its cut thr[l]: all eligible pairs (i, j) with
//       P[l,i,j] = (sum_{m<K} sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])) / K   >=   thr[l]          K = 1..8 checkpoints
//   as CSR over the n_labels * n_head rows (l, i): row_ptr, then per hit its column j and its probability.
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614, average the sigmoids
// of the checkpoints; the reference then reads such sets off the stored tensor.)  The mean of K sigmoids is not monotone in any one
// model's logit, so no union or intersection of single-model selections gives this set; here nothing of [L,N,N] is materialised.
//
// Two existing kernels joined: select.hip's contract on ensemble_topk.hip's sweep.
//   score arithmetic: ensemble_topk.hip's, which is ensemble.hip's general (non-symmetric) sweep bit for bit.  A workgroup (4 waves,
//     128 head rows of one outcome, one wave per SIMD) walks its tail tiles in chunks of CH; for every chunk it rebuilds
//     T_m = z_head_m[rows] . W_sym_m[l] (build_t) for m = 0..K-1 and sweeps the chunk with it (compute_tile_spread), sigmoid
//     1 / (1 + expf(-s)), the running sums of the chunk (psum, CH x 32 VGPRs) staying in registers across the models, divided once
//     by K; the compare is on that quotient (P >= thr, not sum >= thr * K).  With K = 1 the one T is built for the first chunk only.
//     build_t, pick, sigmoid_head, the eligibility test and the layout's constants are ensemble_sweep.h's, shared by the family;
//     the two-buffer ring is this file's own text (sharing sweep text has moved hipcc's schedule before).
//   epilogue: select.hip's, run on the chunk's finished tiles after its last model, in ascending tile order.  The tile index of that
//     loop is a run-time value and the tile's sums are picked by wave-uniform selects: ONE copy of the 32 inlined takes (DESIGN.md
//     4af: six copies inside the unrolled stage loop sent psum to scratch).  Every wave owns 32 head rows, 32 lanes per row (the
//     lanes of one h), each lane holding one column; per accumulator register there is one running u32 `run` = hits of row
//     acc_row(v, h) in the tiles swept so far, uniform over the row group.
//       pass-through: ineligible, out-of-range (rows >= n_head too) and masked elements become NaN, which fails >= for every cut,
//                     -inf included; then one compare per element, OR-ed into one ballot per tile.
//       hit path:     (wave-uniform branch) per accumulator register one ballot; the popcount of the row group's bits is added to
//                     `run`.  FILL: a lane with a hit reads row_ptr[row] and row_ptr[row + 1] there and then, its slot is
//                     row_ptr[row] + run + popcount(the group's bits on lower lanes), in 64-bit, and it stores its column and
//                     probability with two plain vector stores.  Only a lane with a hit reads row_ptr, and an element of a row
//                     >= n_head never hits, so both entries lie inside row_ptr.
//       end:          count: lane 0 of every row group stores `run` for every row < n_head, rows without a hit included: the result
//                     needs no zeroing.
// Order.  Tiles reach the epilogue in ascending column order -- chunks ascending, tiles ascending inside a chunk, no per-workgroup
// rotation -- and inside a tile register v of accumulator t in lane (r, h) is column tcol0 + 32 t + r: the column rises with the
// lane index r inside the row group, and t = 0 is taken before t = 1.  So a row's hits land in ascending column order and the
// output is canonical CSR, the order torch.nonzero gives on the dense mask.  Sigmoid rounding makes exact ties common (many
// probabilities are exactly 1): >= keeps all of them, and nothing about the order depends on the values.
// Bounded writes (fill).  Slot s of row r is written only if row_ptr[r] >= 0 and row_ptr[r] <= s < row_ptr[r + 1]; a hit past the
// row's end is dropped.  A stale row_ptr gives a truncated or partly unwritten result, never a store outside [row_ptr[r],
// row_ptr[r + 1]).  `run` < n_tail < 2^31 is widened before the add.
// Mask (MASKED instantiations): the words [row block of the wave][columns of the chunk's tiles] are needed once per chunk: two
// plain loads per tile and lane, issued before the last model's T rebuild, whose own loads are waited for anyway.  The unmasked
// instantiations read no mask memory.
// Waits.  Every stage barrier waits vmcnt(0).  In the count pass the only vector-memory operations a wave has in flight there are
// the LDS-DMAs of the tile about to be read.  In the fill pass the stores and row_ptr reads of the PREVIOUS chunk's epilogue may
// still be in flight at the next chunk's first barriers; vmcnt(0) waits for them too, which is correct by construction (vmcnt
// retires in order for loads, and 0 covers everything).  A counted wait would have to bound those stores; the measurement
//  shows no gap between the passes at a sparse cut that would pay for one.
// No atomics, no LDS beyond the stage buffers and the slabs: bit-identical from launch to launch.
#include "ensemble_sweep.h"

namespace {

struct EnsSelArgs : EnsOperands {
  const float* thr;            // [n_labels]
  int* row_counts;             // count pass: [n_labels, n_head]
  const long long* row_ptr;    // fill pass: [n_labels * n_head + 1]
  int* cols;                   // fill pass: [row_ptr[last]]
  float* vals;
  int64_t n_head, n_tail;
  int n_models;
  int eligible;                // mdg_topk_eligible
};

template <bool MASKED> struct EnsSelKArgs : EnsSelArgs {};
template <> struct EnsSelKArgs<true> : EnsSelArgs { PairMask mask; };

// Hit path of one accumulator register: select.hip's select_take<32, FILL>.  Must be called in wave-uniform control flow.  The 32
// lanes of one h share the row whose row_ptr entry is `rp` (FILL; read by lanes with a hit only); `run`: the row's hits so far.
template <bool FILL>
__device__ __forceinline__ void ens_sel_take(const EnsSelArgs& p, unsigned& run, bool hit, float x, int col, const long long* rp, int lane) {
  const unsigned long long m = __ballot(hit);
  const int c = lane & 31, base = lane & ~31;
  const unsigned mine = static_cast<unsigned>(m >> base);             // hits of MY row, one bit per lane of the group
  if constexpr (FILL) {
    if (hit) {
      const int64_t beg = rp[0], end = rp[1];
      const int64_t slot = beg + static_cast<int64_t>(run) + __builtin_popcount(mine & ((1u << c) - 1u));
      if (beg >= 0 && slot < end) {
        p.cols[slot] = col;
        p.vals[slot] = x;
      }
    }
  }
  run += __builtin_popcount(mine);
}

template <int MODE, bool FILL, bool MASKED, int CH>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_select_kernel(const EnsSelKArgs<MASKED> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t l = blockIdx.y;
  const int K = p.n_models, mode = p.eligible;
  const float kf = static_cast<float>(K);
  const float thr = p.thr[l];
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  // LOWER: the last row block sweeps the most column tiles -- it goes first
  const int64_t rbk = mode == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  const int64_t wrow0 = row0 + wave * 32;        // this wave's rows: wrow0 .. wrow0 + 31
  const int nt = sweep_tiles(mode, row0, BM, p.n_head, p.n_tail);
  int64_t zr = wrow0 + (tid & 31);
  zr = zr < p.n_head ? zr : p.n_head - 1;
  auto build = [&](AFrag<MODE>& A, int m) {
    int t_o = tid;
    asm volatile("" : "+v"(t_o));
    const int r = t_o & 31, h = (t_o >> 5) & 1;
    TileSrc wl = pick(p.w, m);
    if constexpr (MODE == MDG_PREC_F32) wl.f32 += l * D * D;
    else { wl.hi += l * D * D; wl.lo += l * D * D; }
    build_t<MODE, NW>(A, pick(p.z_head, m) + zr * D, wl, smem, slab, t_o, r, h);
  };
  const unsigned* mrow = nullptr;                // MASKED: the words of this wave's row block, outcome l
  if constexpr (MASKED) {
    int64_t rb = wrow0 >> 5;
    rb = rb < p.mask.nrb ? rb : p.mask.nrb - 1;  // rows >= n_head only: clamped onto the last block, as the z_head row is
    mrow = p.mask.words + l * p.mask.plane_stride + rb * p.mask.ld;
  }

  unsigned run[16];                              // hits so far of row acc_row(v, h)
#pragma unroll
  for (int v = 0; v < 16; ++v) run[v] = 0u;

  AFrag<MODE> At;
  int par = 0;               // stage buffer of the next stage
  const int nch = (nt + CH - 1) / CH;
  for (int c = 0; c < nch; ++c) {
    const int s0 = c * CH;
    const int nc = nt - s0 < CH ? nt - s0 : CH;
    float psum[CH][2][16];
    unsigned mw[CH][2];      // MASKED: lane (r, h)'s words of the chunk's tiles, columns 64 tile + r and + 32
    for (int m = 0; m < K; ++m) {
      const bool last = (m == K - 1);
      if constexpr (MASKED) {
        if (last) {          // ahead of the rebuild: its loads are waited for before the sweep starts
          int ln = tid & 63;
          asm volatile("" : "+v"(ln));
#pragma unroll
          for (int ci = 0; ci < CH; ++ci) {
            mw[ci][0] = mw[ci][1] = 0u;
            if (ci < nc) {   // tile s0 + ci starts below n_tail, so both words lie inside the padded row (ld = n_tail up to 64)
              const unsigned* q = mrow + static_cast<int64_t>(s0 + ci) * BN + (ln & 31);
              mw[ci][0] = q[0];
              mw[ci][1] = q[32];
            }
          }
        }
      }
      // every (chunk, model): the previous T is dead here, its registers are reused.  One model: T stays resident.
      if (K > 1 || c == 0) build(At, m);
      const TileSrc zt = pick(p.zt, m);
      {
        // the chunk's first tile; the buffer was last read two stages ago, and every wave has passed a barrier since
        int ln = tid & 63;
        asm volatile("" : "+v"(ln));
        stage_dma<MODE>(zt, static_cast<int64_t>(s0) * BN, smem + par * STAGE_BYTES, wave, ln, NW);
      }
#pragma unroll
      for (int ci = 0; ci < CH; ++ci) {
        if (ci < nc) {
          // lane-dependent offsets recomputed per stage (hoisted out of the loops they would hold many VGPRs per unrolled stage)
          int lane = tid & 63;
          asm volatile("" : "+v"(lane));
          const int r = lane & 31, h = lane >> 5;
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's DMAs (fill: and what the last epilogue left in flight)
          __builtin_amdgcn_s_barrier();                                       // ... for every wave; every wave is done with the other buffer
          char* const cur = smem + par * STAGE_BYTES;
          char* const nxt = smem + (par ^ 1) * STAGE_BYTES;
          if (ci + 1 < nc) stage_dma<MODE>(zt, static_cast<int64_t>(s0 + ci + 1) * BN, nxt, wave, lane, NW);
          par ^= 1;
          const int64_t tcol0 = static_cast<int64_t>(s0 + ci) * BN;
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
                psum[ci][t][v] = m == 0 ? sg : psum[ci][t][v] + sg;
                if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four sigmoids' temporaries at a time
              }
          }
        }
      }
    }
    // ---- the chunk's finished tiles, in ascending order, through the selecting epilogue (one copy of the take code: `ci` is a
    // run-time index, the tile's sums are picked out of the register array by wave-uniform selects) ----
    {
      int lane = tid & 63;
      asm volatile("" : "+v"(lane));
      const int r = lane & 31, h = lane >> 5;
      const long long* const rp = p.row_ptr + (l * p.n_head + wrow0 + 4 * h);      // row acc_row(v, h): rp[(v & 3) + 8 * (v >> 2)]
      for (int ci = 0; ci < nc; ++ci) {
        const int64_t tcol0 = static_cast<int64_t>(s0 + ci) * BN;
        if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31) break;              // wave-uniform: this tile and the later ones were skipped
        float pr[2][16];
        unsigned w0 = 0u, w1 = 0u;
#pragma unroll
        for (int c2 = 0; c2 < CH; ++c2)
          if (ci == c2) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) pr[t][v] = psum[c2][t][v];
            if constexpr (MASKED) { w0 = mw[c2][0]; w1 = mw[c2][1]; }
          }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            pr[t][v] = pr[t][v] / kf;                                           // P = sum / K
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
        if constexpr (MASKED) {
          if (__ballot((w0 | w1) != 0u) != 0) {                                // wave-uniform: a tile without a known pair costs this ballot
            const unsigned mh[2] = {w0 >> (4 * h), w1 >> (4 * h)};             // bit acc_row(v, 0) of mh[t] <-> row acc_row(v, h)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) pr[t][v] = pairmask_nan_if(pr[t][v], mh[t], acc_row(v, 0));
          }
        }
        bool any = false;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) any |= pr[t][v] >= thr;
        if (__ballot(any) != 0) {
#pragma unroll
          for (int v = 0; v < 16; ++v)
#pragma unroll
            for (int t = 0; t < 2; ++t)                                        // columns 0..31 of the tile, then 32..63
              ens_sel_take<FILL>(p, run[v], pr[t][v] >= thr, pr[t][v], static_cast<int>(tcol0) + 32 * t + r,
                                 rp + ((v & 3) + 8 * (v >> 2)), lane);
        }
      }
    }
  }
  if constexpr (!FILL) {
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = wrow0 + acc_row(v, h);
      if (r == 0 && row < p.n_head) p.row_counts[l * p.n_head + row] = static_cast<int>(run[v]);
    }
  }
}

template <int MODE, bool FILL, bool MASKED>
int launch_ens_select(EnsSelKArgs<MASKED>& a, const float* const* z_tail, const float* const* w_sym, int64_t n_labels, char* ws,
                      hipStream_t st, const char* fn) {
  const int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, fn);
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * ENS_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL((ensemble_select_kernel<MODE, FILL, MASKED, ENS_CH>), grid, dim3(64 * ENS_NW), ENS_LDS, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

// The checks both entry points share; `outputs`: none of the pass's own pointers is null.  Returns MDG_OK with *launch = false when
// there is nothing to do.
int ens_select_check(const char* fn, const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                     const float* thr, bool outputs, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible,
                     void* workspace, size_t workspace_bytes, bool* launch) {
  *launch = false;
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "%s: n_tail %lld does not fit the int32 column indices", fn, (long long)n_tail);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, thr && outputs, n_tail, n_labels, precision, workspace, workspace_bytes);
  *launch = rc == MDG_OK;
  return rc;
}

template <bool FILL, bool MASKED>
int ens_select_run(const char* fn, const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                   const float* thr, int32_t* row_counts, const int64_t* row_ptr, int32_t* cols, float* vals, int64_t n_head, int64_t n_tail,
                   int64_t n_labels, int precision, int eligible, void* workspace, void* stream, const uint32_t* mask, int64_t plane_stride) {
  EnsSelKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args(fn, a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  ens_fill_operands(a, z_head, n_models, n_tail);
  a.thr = thr;
  a.row_counts = row_counts;
  a.row_ptr = reinterpret_cast<const long long*>(row_ptr);
  a.cols = cols;
  a.vals = vals;
  a.n_head = n_head; a.n_tail = n_tail;
  a.n_models = n_models;
  a.eligible = eligible;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (precision == MDG_PREC_F32) return launch_ens_select<MDG_PREC_F32, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
  return launch_ens_select<MDG_PREC_BF16X3, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
}

}  // namespace

extern "C" size_t mdg_bilinear_ensemble_select_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_models,
                                                               int precision) {
  (void)n_head;
  return ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
}

extern "C" int mdg_bilinear_ensemble_select_count(const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                                                  int n_models, const float* thr, int32_t* row_counts, int64_t n_head, int64_t n_tail,
                                                  int64_t n_labels, int64_t D_, int precision, int eligible, void* workspace,
                                                  size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_ensemble_select_count";
  bool launch;
  const int rc = ens_select_check(fn, z_head, z_tail, w_sym, n_models, thr, row_counts != nullptr, n_head, n_tail, n_labels, D_, precision,
                                  eligible, workspace, workspace_bytes, &launch);
  if (rc != MDG_OK || !launch) return rc;
  if (!mask)
    return ens_select_run<false, false>(fn, z_head, z_tail, w_sym, n_models, thr, row_counts, nullptr, nullptr, nullptr, n_head, n_tail,
                                        n_labels, precision, eligible, workspace, stream, nullptr, 0);
  return ens_select_run<false, true>(fn, z_head, z_tail, w_sym, n_models, thr, row_counts, nullptr, nullptr, nullptr, n_head, n_tail, n_labels,
                                     precision, eligible, workspace, stream, mask, plane_stride);
}

extern "C" int mdg_bilinear_ensemble_select_fill(const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                                                 int n_models, const float* thr, const int64_t* row_ptr, int32_t* cols, float* vals,
                                                 int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible,
                                                 void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                                                 int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_ensemble_select_fill";
  bool launch;
  const int rc = ens_select_check(fn, z_head, z_tail, w_sym, n_models, thr, row_ptr && cols && vals, n_head, n_tail, n_labels, D_, precision,
                                  eligible, workspace, workspace_bytes, &launch);
  if (rc != MDG_OK || !launch) return rc;
  if (!mask)
    return ens_select_run<true, false>(fn, z_head, z_tail, w_sym, n_models, thr, nullptr, row_ptr, cols, vals, n_head, n_tail, n_labels,
                                       precision, eligible, workspace, stream, nullptr, 0);
  return ens_select_run<true, true>(fn, z_head, z_tail, w_sym, n_models, thr, nullptr, row_ptr, cols, vals, n_head, n_tail, n_labels, precision,
                                    eligible, workspace, stream, mask, plane_stride);
}
