// Per-row top-k of the checkpoint-ensembled all-pairs head for gfx950 (mdg_bilinear_ensemble_topk).
//
//   for every outcome l and head row i: the k largest
//       P[l,i,j] = (sum_{m<K} sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])) / K          K = 1..8 checkpoints
//   over the ELIGIBLE tail columns j, with those columns, ordered by (P descending, column ascending).
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614, average the sigmoids
// of the checkpoints; the reference then looks partners up in the stored tensor.)  The mean of K sigmoids is not monotone in any
// one model's logit, so no composition of single-model lists gives this ranking; here nothing of [L,Nh,Nt] is materialised.
//
// Two existing kernels joined:
//   score arithmetic: ensemble.hip's general (non-symmetric) sweep, bit for bit.  A workgroup (4 waves, 128 head rows of one
//     outcome, one wave per SIMD) walks its tail tiles in chunks of CH; for every chunk it rebuilds T_m = z_head_m[rows] . W_sym_m[l]
//     (build_t) for m = 0..K-1 and sweeps the chunk with it (compute_tile_spread), sigmoid 1 / (1 + expf(-s)), the running sums of
//     the chunk (CH x 32 VGPRs) staying in registers across the models, divided once by K.  build_t, pick, sigmoid_head and the
//     layout's constants are ensemble_sweep.h's, shared with ensemble.hip; the two-buffer ring is this file's own text (sharing
//     sweep text has moved hipcc's schedule before).
//     With K = 1 the one T stays resident: it is built for the first chunk only.
//   epilogue: topk.hip's, run on the chunk's finished tiles after its last model, in ascending tile order.  Every wave owns 32 head
//     rows; a row's sorted list lives in its 32 lanes (topk_list.h: lv / li / thr per accumulator register).  Ineligible, out-of-range
//     and masked elements become -inf, then one compare per element against the row's k-th value, and topk_insert for what passes.
//     The tile index of that loop is a run-time value and the tile's sums are picked by wave-uniform selects: ONE copy of the 32
//     inlined inserts (six copies inside the unrolled stage loop kept hipcc from unrolling it, and the sums went to scratch).
// Tie rule: tiles reach the epilogue in ascending column order -- chunks ascending, tiles ascending inside a chunk, no
// per-workgroup rotation (ensemble.hip's `stagger` is not used) -- so a later value equal to the threshold has a larger column
// than every kept entry and rightly fails `x > thr`; inside a tile the insert compares the full key.  Sigmoid rounding makes
// exact ties common (many probabilities are exactly 1), so this is the normal case here, not a corner.
// Mask (MASKED instantiations): the words [row block of the wave][columns of the chunk's tiles] are needed once per chunk, not
// once per model: two plain loads per tile and lane, issued before the last model's T rebuild, whose own loads are waited for
// anyway.  The unmasked instantiations read no mask memory.
// Waits: the kernel stores nothing inside the sweep; per wave the only vector-memory operations in flight at a stage barrier are
// the LDS-DMAs of the tile about to be read, so every stage waits vmcnt(0).  (ensemble.hip's vmcnt(32) counts stores that do not
// exist here.)  No atomics, no memory traffic besides the final k stores per row: bit-identical from launch to launch.
#include "ensemble_sweep.h"
#include "topk_list.h"

namespace {

struct EnsTopkArgs : EnsOperands {
  float* vals;                 // [n_labels, n_head, k]
  int* idx;                    // [n_labels, n_head, k]
  int64_t n_head, n_tail;
  int n_models;
  int k;
  int eligible;                // mdg_topk_eligible
};

template <bool MASKED> struct EnsTopkKArgs : EnsTopkArgs {};
template <> struct EnsTopkKArgs<true> : EnsTopkArgs { PairMask mask; };

__device__ __forceinline__ bool ens_topk_eligible(int mode, int64_t row, int64_t col, int64_t n_tail) {
  return col < n_tail && (mode == MDG_TOPK_ALL || (mode == MDG_TOPK_NOT_SELF ? col != row : col < row));
}

template <int MODE, bool MASKED, int CH>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_topk_kernel(const EnsTopkKArgs<MASKED> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t l = blockIdx.y;
  const int K = p.n_models, mode = p.eligible, k = p.k;
  const float kf = static_cast<float>(K);
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

  float lv[16][1], thr[16];
  int li[16][1];
#pragma unroll
  for (int v = 0; v < 16; ++v) { lv[v][0] = -INFINITY; li[v][0] = -1; thr[v] = -INFINITY; }

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
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's DMAs: all this wave has in flight
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
    // ---- the chunk's finished tiles, in ascending order, through the lists (one copy of the insert code: `ci` is a run-time index,
    // the tile's sums are picked out of the register array by wave-uniform selects) ----
    {
      int lane = tid & 63;
      asm volatile("" : "+v"(lane));
      const int r = lane & 31, h = lane >> 5;
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
        const bool plain = tcol0 + BN <= p.n_tail &&
                           (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
        if (!plain) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v)
              pr[t][v] = ens_topk_eligible(mode, wrow0 + acc_row(v, h), tcol0 + 32 * t + r, p.n_tail) ? pr[t][v] : -INFINITY;
        }
        if constexpr (MASKED) {
          if (__ballot((w0 | w1) != 0u) != 0) {                                // wave-uniform: a tile without a known pair costs this ballot
            const unsigned mh[2] = {w0 >> (4 * h), w1 >> (4 * h)};             // bit acc_row(v, 0) of mh[t] <-> row acc_row(v, h)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) pr[t][v] = (mh[t] >> acc_row(v, 0)) & 1u ? -INFINITY : pr[t][v];
          }
        }
        bool any = false;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) any |= pr[t][v] > thr[v];
        if (__ballot(any) != 0) {
#pragma unroll
          for (int v = 0; v < 16; ++v)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              topk_insert<32>(lv[v], li[v], thr[v], pr[t][v] > thr[v], pr[t][v], static_cast<int>(tcol0) + 32 * t + r, lane, k);
        }
      }
    }
  }
  {
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = wrow0 + acc_row(v, h);
      if (r < k && row < p.n_head) {
        const int64_t o = (l * p.n_head + row) * k + r;
        p.vals[o] = lv[v][0];
        p.idx[o] = li[v][0];
      }
    }
  }
}

template <int MODE, bool MASKED>
int launch_ens_topk(EnsTopkKArgs<MASKED>& a, const float* const* z_tail, const float* const* w_sym, int64_t n_labels, char* ws,
                    hipStream_t st) {
  const char* const fn = "mdg_bilinear_ensemble_topk";
  const int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, "mdg_bilinear_ensemble_topk(operand images)");
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * ENS_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL((ensemble_topk_kernel<MODE, MASKED, ENS_CH>), grid, dim3(64 * ENS_NW), ENS_LDS, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

template <bool MASKED>
int ens_topk_run(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models, float* vals, int32_t* idx,
                 int64_t n_head, int64_t n_tail, int64_t n_labels, int precision, int k, int eligible, void* workspace, void* stream,
                 const uint32_t* mask, int64_t plane_stride) {
  EnsTopkKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args("mdg_bilinear_ensemble_topk", a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  ens_fill_operands(a, z_head, n_models, n_tail);
  a.vals = vals;
  a.idx = idx;
  a.n_head = n_head; a.n_tail = n_tail;
  a.n_models = n_models;
  a.k = k;
  a.eligible = eligible;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (precision == MDG_PREC_F32) return launch_ens_topk<MDG_PREC_F32, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
  return launch_ens_topk<MDG_PREC_BF16X3, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
}

}  // namespace

extern "C" int mdg_bilinear_ensemble_topk_chunk_tiles(void) { return ENS_CH; }

extern "C" size_t mdg_bilinear_ensemble_topk_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_models,
                                                             int precision) {
  (void)n_head;
  return ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
}

extern "C" int mdg_bilinear_ensemble_topk(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                          float* vals, int32_t* idx, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_,
                                          int precision, int k, int eligible, void* workspace, size_t workspace_bytes, void* stream,
                                          const uint32_t* mask, int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_ensemble_topk";
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "mdg_bilinear_ensemble_topk: k must be in 1..%d (got %d)", TOPK_MAX_K, k);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "mdg_bilinear_ensemble_topk: n_tail %lld does not fit the int32 column indices",
                (long long)n_tail);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, vals && idx, n_tail, n_labels, precision, workspace, workspace_bytes);
  if (rc != MDG_OK) return rc;
  if (!mask)
    return ens_topk_run<false>(z_head, z_tail, w_sym, n_models, vals, idx, n_head, n_tail, n_labels, precision, k, eligible, workspace, stream,
                               nullptr, 0);
  return ens_topk_run<true>(z_head, z_tail, w_sym, n_models, vals, idx, n_head, n_tail, n_labels, precision, k, eligible, workspace, stream, mask,
                            plane_stride);
}
