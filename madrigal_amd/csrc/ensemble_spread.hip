// Spread of the checkpoint-ensembled all-pairs head for gfx950: how much the K checkpoints agree (mdg_bilinear_ensemble_spread,
// mdg_bilinear_ensemble_spread_topk).
//
//   p_m[l,i,j]  = sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])                          m = 0..K-1, K = 1..8 checkpoints
//   mean[l,i,j] = (p_0 + ... + p_{K-1}) / K                                              mdg_bilinear_ensemble_sigmoid's P, bit for bit
//   std[l,i,j]  = sqrt((1/K) sum_m (p_m - mean)^2)                                       population standard deviation (ddof = 0)
//   bound       = fmaf(kappa, std, mean)                                                 one rounding
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614, keep every checkpoint's
// score tensor in memory before they average, so there the spread is np.stack(...).std(0) of what is stored; the reference has no
// call of its own for it.)  On this path the per-checkpoint tensors never exist: the sweep holds each model's sigmoid in a register
// when it adds it to the running sum, and the second moment is a recurrence on that register.
//
// The recurrence is Welford's, in fp32, beside the untouched running sum (the mean stays the dense product's, bit for bit):
//   model 0:   mu = p, M2 = 0
//   model n-1: d = p - mu;  mu = mu + d * (1 / n);  M2 = M2 + d * (p - mu)               (each operation rounded, no contraction)
//   finish:    std = sqrtf(M2 / K)
// It does not cancel: M2 is a sum of products of two differences, never a difference of two large sums (sum p^2 - (sum p)^2 / K
// returns noise of the order of 3e-4 where the probabilities round to 1, and goes negative).  M2 >= 0 always: 1 / n <= 1/2, so the
// exact mu + d / n lies between mu and p, rounding is monotone and both ends are fp32 numbers, hence the new mu lies between them
// and p - mu keeps the sign of d (or is zero).  So the square root never sees a negative number, std >= 0 and never NaN for finite
// logits.  K equal values give d == 0 at every step and std == 0.0f exactly; K = 1 gives sqrtf(0 / 1).
// spread_update and spread_finish below are the only text of it: both kernels call them, so their std and bound agree bit for bit.
//
// Score arithmetic, workgroup layout, T rebuild per (chunk, model), the two-buffer LDS-DMA ring and its waits: ensemble_topk.hip's
// (4 waves, one per SIMD, 32 head rows per wave; every stage waits vmcnt(0), nothing is stored inside the sweep).  The sweep text is
// carried here, as every member of the family carries it.  Per element the state is three registers -- running
// sum, mu, M2 -- so the chunk is SPREAD_CH = 2 tiles (2 x 96 VGPRs) where the mean-only products sweep 6; T is rebuilt for as much
// MFMA work as the chunk's own.  (Three tiles fit the dense kernel, 424 - 448 registers, but not the top-k kernel, whose lists are
// another 80: hipcc then spills about 130 registers to scratch.  One width serves both)  With K = 1 the one T
// stays resident.
//
// Dense kernel: after the chunk's last model the finished tiles leave as fp32 rows of any non-null subset of mean / std / bound
// (4-byte buffer stores, lane = column, one common row pitch; ragged rows / columns dropped by the buffer range or a 0xFFFFFFFF
// offset, as ensemble.hip).  The workgroups start at staggered tiles, as there; column order does not matter here.
// Top-k kernel: ensemble_topk.hip's epilogue with `bound` as the key and two payload registers per list entry, the entry's mean
// and std (topk_insert_payload: topk_list.h's insert for G = 32 with two more shuffles per shifted slot).  After the last model
// the chunk's tiles are finished IN PLACE by a compile-time tile index -- sum -> mean, M2 -> std, mu -> bound, ineligible / out of
// range / masked bounds -> -inf -- and then walked by a run-time tile index that picks each element out of the register arrays by
// wave-uniform selects where it is used: one copy of the 32 inlined inserts and no second copy of the tile's 96 values.
// Tie rule: tiles reach the lists in ascending column order (no stagger), so ensemble_topk.hip's argument holds unchanged.
// No atomics; bit-identical from launch to launch.
#include <cmath>

#include "ensemble_sweep.h"
#include "topk_list.h"

namespace {

constexpr int SPREAD_CH = 2;           // tail tiles per chunk: 2 x (sum, mu, M2) x 32 VGPRs beside T and the lists

// ---- the recurrence -----------------------------------------------------------------------------------------------------------
// One model's probability into the element's state; rn = 1 / (models seen, this one included), `first`: this is model 0.
__device__ __forceinline__ void spread_update(bool first, float& sum, float& mu, float& m2, float p, float rn) {
  const float d = p - mu;
  const float mu1 = mu + d * rn;
  const float m21 = m2 + d * (p - mu1);
  sum = first ? p : sum + p;
  mu = first ? p : mu1;
  m2 = first ? 0.f : m21;
}

// The element's three results from its state after the last model.
__device__ __forceinline__ void spread_finish(float sum, float m2, float kf, float kappa, float& mean, float& sd, float& bound) {
  mean = sum / kf;
  sd = __builtin_sqrtf(m2 / kf);
  bound = __builtin_fmaf(kappa, sd, mean);
}

// topk_list.h's topk_insert<32> whose entries carry two payload registers (pa, pb): they ride the shuffles of the index.
__device__ __forceinline__ void topk_insert_payload(float& lv, int& li, float& pa, float& pb, float& thr, bool cand, float x, int col, float a,
                                                    float b, int lane, int k) {
  unsigned long long m = __ballot(cand);
  if (m == 0) return;
  const int c = lane & 31, base = lane & ~31;
  unsigned mine = static_cast<unsigned>(m >> base);                   // candidates of MY row, one bit per lane of the group
  while (m != 0) {
    const bool has = mine != 0;
    const int src = base + (has ? __builtin_ctz(mine) : 0);
    const float cx = __shfl(x, src, 64);
    const int cc = __shfl(col, src, 64);
    const float ca = __shfl(a, src, 64);
    const float cb = __shfl(b, src, 64);
    const bool ahead = lv > cx || (lv == cx && li < cc);              // entries that stay ahead of the candidate (sorted: a prefix)
    const int p = __builtin_popcount(static_cast<unsigned>(__ballot(ahead) >> base));
    const int prev = (lane + 63) & 63;
    const float upv = __shfl(lv, prev, 64);
    const int upi = __shfl(li, prev, 64);
    const float upa = __shfl(pa, prev, 64);
    const float upb = __shfl(pb, prev, 64);
    const bool take_new = has && c == p, take_up = has && c > p;
    lv = take_new ? cx : (take_up ? upv : lv);
    li = take_new ? cc : (take_up ? upi : li);
    pa = take_new ? ca : (take_up ? upa : pa);
    pb = take_new ? cb : (take_up ? upb : pb);
    thr = __shfl(lv, base + ((k - 1) & 31), 64);
    mine &= mine - 1;
    m = __ballot(mine != 0);
  }
}

// a[ci][t][v] for a wave-uniform run-time ci and compile-time t, v (scalar-conditioned selects, no indexing of the registers)
template <int CH>
__device__ __forceinline__ float pick_tile(const float (&a)[CH][2][16], int ci, int t, int v) {
  float x = a[0][t][v];
#pragma unroll
  for (int c2 = 1; c2 < CH; ++c2)
    if (ci == c2) x = a[c2][t][v];
  return x;
}

// ---- dense: mean / std / bound -------------------------------------------------------------------------------------------------
struct EnsSpreadArgs : EnsOperands {
  float* mean;                 // [n_labels, n_head, ldo] each; null: not written
  float* sd;
  float* bound;
  int64_t n_head, n_tail, ldo;
  int n_models;
  float kappa;
};

template <int MODE, int CH>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_spread_kernel(const EnsSpreadArgs p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t l = blockIdx.y, N = p.n_tail, ld = p.ldo;
  const int K = p.n_models;
  const float kf = static_cast<float>(K), kappa = p.kappa;
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int nt = static_cast<int>((N + BN - 1) / BN);
  const int start = static_cast<int>((blockIdx.x * 5u + blockIdx.y * 3u) % static_cast<unsigned>(nt));
  auto tile_of = [&](int s) { const int t = s + start; return t >= nt ? t - nt : t; };
  int64_t zr = row0 + wave * 32 + (tid & 31);
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
  // the workgroup's rows of outcome l in each tensor; rows >= n_head fall outside the range and are dropped
  const int64_t slab_rows = (p.n_head - row0) < BM ? (p.n_head - row0) : BM;
  const int64_t out0 = (l * p.n_head + row0) * ld;
  const int range = static_cast<int>(slab_rows * ld * 4);
  const __amdgpu_buffer_rsrc_t rs_mean = __builtin_amdgcn_make_buffer_rsrc(p.mean ? p.mean + out0 : nullptr, 0, p.mean ? range : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_sd = __builtin_amdgcn_make_buffer_rsrc(p.sd ? p.sd + out0 : nullptr, 0, p.sd ? range : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_bound = __builtin_amdgcn_make_buffer_rsrc(p.bound ? p.bound + out0 : nullptr, 0, p.bound ? range : 0, 0x00020000);

  AFrag<MODE> At;
  int par = 0;               // stage buffer of the next stage
  const int nch = (nt + CH - 1) / CH;
  for (int c = 0; c < nch; ++c) {
    const int s0 = c * CH;
    const int nc = nt - s0 < CH ? nt - s0 : CH;
    float psum[CH][2][16], mu[CH][2][16], m2[CH][2][16];
    for (int m = 0; m < K; ++m) {
      const float rn = 1.0f / static_cast<float>(m + 1);
      // every (chunk, model): the previous T is dead here, its registers are reused.  One model: T stays resident.
      if (K > 1 || c == 0) build(At, m);
      const TileSrc zt = pick(p.zt, m);
      {
        // the chunk's first tile; the buffer was last read two stages ago, and every wave has passed a barrier since
        int ln = tid & 63;
        asm volatile("" : "+v"(ln));
        stage_dma<MODE>(zt, static_cast<int64_t>(tile_of(s0)) * BN, smem + par * STAGE_BYTES, wave, ln, NW);
      }
#pragma unroll
      for (int ci = 0; ci < CH; ++ci) {
        if (ci < nc) {
          // lane-dependent offsets recomputed per stage (hoisted out of the loops they would hold many VGPRs per unrolled stage)
          int lane = tid & 63;
          asm volatile("" : "+v"(lane));
          const int r = lane & 31, h = lane >> 5;
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's DMAs (and the previous chunk's stores)
          __builtin_amdgcn_s_barrier();                                       // ... for every wave; every wave is done with the other buffer
          char* const cur = smem + par * STAGE_BYTES;
          char* const nxt = smem + (par ^ 1) * STAGE_BYTES;
          if (ci + 1 < nc) stage_dma<MODE>(zt, static_cast<int64_t>(tile_of(s0 + ci + 1)) * BN, nxt, wave, lane, NW);
          par ^= 1;
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
              spread_update(m == 0, psum[ci][t][v], mu[ci][t][v], m2[ci][t][v], sigmoid_head(acc[t][v]), rn);
              if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four sigmoids' and updates' temporaries at a time
            }
        }
      }
    }
    // ---- the chunk's finished tiles leave as rows ----
    {
      int lane = tid & 63;
      asm volatile("" : "+v"(lane));
      const int r = lane & 31, h = lane >> 5;
#pragma unroll
      for (int ci = 0; ci < CH; ++ci) {
        if (ci < nc) {
          const int64_t tcol0 = static_cast<int64_t>(tile_of(s0 + ci)) * BN;
          // byte offsets in 32 bits (the slab is < 2^31 bytes): a lane base plus a wave-uniform row step per register
          const unsigned lrow_base = static_cast<unsigned>(((wave * 32 + 4 * h) * ld + tcol0 + r) * 4);
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
              float mean, sd, bd;
              spread_finish(psum[ci][t][v], m2[ci][t][v], kf, kappa, mean, sd, bd);
              const int dv = (v & 3) + 8 * (v >> 2);
              const bool ok = tcol0 + 32 * t + r < N;
              const unsigned off = ok ? lrow_base + static_cast<unsigned>((dv * ld + 32 * t) * 4) : 0xFFFFFFFFu;
              if (p.mean) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, mean), rs_mean, off, 0, 0);
              if (p.sd) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sd), rs_sd, off, 0, 0);
              if (p.bound) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, bd), rs_bound, off, 0, 0);
              if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four elements' temporaries at a time
            }
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- top-k by the bound ---------------------------------------------------------------------------------------------------------
struct EnsSpreadTopkArgs : EnsOperands {
  float* bound;                // [n_labels, n_head, k] each
  int* idx;
  float* mean;
  float* sd;
  int64_t n_head, n_tail;
  int n_models;
  int k;
  int eligible;                // mdg_topk_eligible
  float kappa;
};

template <bool MASKED> struct EnsSpreadTopkKArgs : EnsSpreadTopkArgs {};
template <> struct EnsSpreadTopkKArgs<true> : EnsSpreadTopkArgs { PairMask mask; };

__device__ __forceinline__ bool spread_topk_eligible(int mode, int64_t row, int64_t col, int64_t n_tail) {
  return col < n_tail && (mode == MDG_TOPK_ALL || (mode == MDG_TOPK_NOT_SELF ? col != row : col < row));
}

template <int MODE, bool MASKED, int CH>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_spread_topk_kernel(const EnsSpreadTopkKArgs<MASKED> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t l = blockIdx.y;
  const int K = p.n_models, mode = p.eligible, k = p.k;
  const float kf = static_cast<float>(K), kappa = p.kappa;
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

  // per accumulator register (= head row): this lane's entry of the row's sorted list -- bound, column, mean, std -- and the k-th bound
  float lv[16], lm[16], ls[16], thr[16];
  int li[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) { lv[v] = -INFINITY; li[v] = -1; lm[v] = NAN; ls[v] = NAN; thr[v] = -INFINITY; }

  AFrag<MODE> At;
  int par = 0;               // stage buffer of the next stage
  const int nch = (nt + CH - 1) / CH;
  for (int c = 0; c < nch; ++c) {
    const int s0 = c * CH;
    const int nc = nt - s0 < CH ? nt - s0 : CH;
    float psum[CH][2][16], mu[CH][2][16], m2[CH][2][16];
    unsigned mw[CH][2];      // MASKED: lane (r, h)'s words of the chunk's tiles, columns 64 tile + r and + 32
    for (int m = 0; m < K; ++m) {
      const bool last = (m == K - 1);
      const float rn = 1.0f / static_cast<float>(m + 1);
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
                spread_update(m == 0, psum[ci][t][v], mu[ci][t][v], m2[ci][t][v], sigmoid_head(acc[t][v]), rn);
                if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four sigmoids' and updates' temporaries at a time
              }
          }
        }
      }
    }
    {
      int lane = tid & 63;
      asm volatile("" : "+v"(lane));
      const int r = lane & 31, h = lane >> 5;
      // ---- the chunk's tiles finished in place: psum -> mean, m2 -> std, mu -> bound (-inf where the element may not be kept) ----
#pragma unroll
      for (int ci = 0; ci < CH; ++ci) {
        const int64_t tcol0 = static_cast<int64_t>(s0 + ci) * BN;
        if (ci < nc && !(mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31)) {     // wave-uniform: the tiles that were swept
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
              float mean, sd, bd;
              spread_finish(psum[ci][t][v], m2[ci][t][v], kf, kappa, mean, sd, bd);
              psum[ci][t][v] = mean;
              m2[ci][t][v] = sd;
              mu[ci][t][v] = bd;
              if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four elements' temporaries at a time
            }
          // whole tile eligible for every row of the wave (wave-uniform): no per-element masking
          const bool plain = tcol0 + BN <= p.n_tail &&
                             (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
          if (!plain) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v)
                mu[ci][t][v] = spread_topk_eligible(mode, wrow0 + acc_row(v, h), tcol0 + 32 * t + r, p.n_tail) ? mu[ci][t][v] : -INFINITY;
          }
          if constexpr (MASKED) {
            const unsigned w0 = mw[ci][0], w1 = mw[ci][1];
            if (__ballot((w0 | w1) != 0u) != 0) {                              // wave-uniform: a tile without a known pair costs this ballot
              const unsigned mh[2] = {w0 >> (4 * h), w1 >> (4 * h)};           // bit acc_row(v, 0) of mh[t] <-> row acc_row(v, h)
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) mu[ci][t][v] = (mh[t] >> acc_row(v, 0)) & 1u ? -INFINITY : mu[ci][t][v];
            }
          }
        }
      }
      // ---- ... and through the lists in ascending order (one copy of the insert code: `ci` is a run-time index, every element is
      // picked out of the register arrays by wave-uniform selects where it is used) ----
#pragma nounroll
      for (int ci = 0; ci < nc; ++ci) {
        const int64_t tcol0 = static_cast<int64_t>(s0 + ci) * BN;
        if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31) break;              // wave-uniform: this tile and the later ones were skipped
        bool any = false;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) any |= pick_tile<CH>(mu, ci, t, v) > thr[v];
        if (__ballot(any) != 0) {
#pragma unroll
          for (int v = 0; v < 16; ++v)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const float x = pick_tile<CH>(mu, ci, t, v);
              topk_insert_payload(lv[v], li[v], lm[v], ls[v], thr[v], x > thr[v], x, static_cast<int>(tcol0) + 32 * t + r,
                                  pick_tile<CH>(psum, ci, t, v), pick_tile<CH>(m2, ci, t, v), lane, k);
            }
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
        p.bound[o] = lv[v];
        p.idx[o] = li[v];
        p.mean[o] = lm[v];
        p.sd[o] = ls[v];
      }
    }
  }
}

// ---- launch side ----------------------------------------------------------------------------------------------------------------
template <int MODE>
int launch_ens_spread(EnsSpreadArgs& a, const float* const* z_tail, const float* const* w_sym, int64_t n_labels, char* ws, hipStream_t st) {
  const int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, "mdg_bilinear_ensemble_spread(operand images)");
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * ENS_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL((ensemble_spread_kernel<MODE, SPREAD_CH>), grid, dim3(64 * ENS_NW), ENS_LDS, st, a);
  MDG_CHECK_LAUNCH("mdg_bilinear_ensemble_spread");
  return MDG_OK;
}

template <int MODE, bool MASKED>
int launch_ens_spread_topk(EnsSpreadTopkKArgs<MASKED>& a, const float* const* z_tail, const float* const* w_sym, int64_t n_labels, char* ws,
                           hipStream_t st) {
  const int rc =
      ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, "mdg_bilinear_ensemble_spread_topk(operand images)");
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * ENS_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL((ensemble_spread_topk_kernel<MODE, MASKED, SPREAD_CH>), grid, dim3(64 * ENS_NW), ENS_LDS, st, a);
  MDG_CHECK_LAUNCH("mdg_bilinear_ensemble_spread_topk");
  return MDG_OK;
}

template <bool MASKED>
int ens_spread_topk_run(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models, float kappa, float* bound,
                        int32_t* idx, float* mean, float* sd, int64_t n_head, int64_t n_tail, int64_t n_labels, int precision, int k,
                        int eligible, void* workspace, void* stream, const uint32_t* mask, int64_t plane_stride) {
  EnsSpreadTopkKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args("mdg_bilinear_ensemble_spread_topk", a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  ens_fill_operands(a, z_head, n_models, n_tail);
  a.bound = bound;
  a.idx = idx;
  a.mean = mean;
  a.sd = sd;
  a.n_head = n_head; a.n_tail = n_tail;
  a.n_models = n_models;
  a.k = k;
  a.eligible = eligible;
  a.kappa = kappa;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (precision == MDG_PREC_F32) return launch_ens_spread_topk<MDG_PREC_F32, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
  return launch_ens_spread_topk<MDG_PREC_BF16X3, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
}

}  // namespace

extern "C" int mdg_bilinear_ensemble_spread_chunk_tiles(void) { return SPREAD_CH; }

extern "C" size_t mdg_bilinear_ensemble_spread_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_models,
                                                               int precision) {
  (void)n_head;
  return ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
}

extern "C" int mdg_bilinear_ensemble_spread(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                            float* mean, float* std_, float* bound, float kappa, int64_t ldo, int64_t n_head, int64_t n_tail,
                                            int64_t n_labels, int64_t D_, int precision, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "mdg_bilinear_ensemble_spread";
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, MDG_TOPK_ALL);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(std::isfinite(kappa), "mdg_bilinear_ensemble_spread: kappa must be finite (got %g)", static_cast<double>(kappa));
  MDG_CHECK_ARG(ldo >= n_tail, "mdg_bilinear_ensemble_spread: row pitch %lld < n_tail %lld", (long long)ldo, (long long)n_tail);
  MDG_CHECK_ARG(ldo * 32 * ENS_NW * 4 < (int64_t(1) << 31), "mdg_bilinear_ensemble_spread: row pitch %lld too large", (long long)ldo);
  if (n_head == 0 || n_tail == 0 || n_labels == 0) return MDG_OK;
  rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, mean || std_ || bound, n_tail, n_labels, precision, workspace, workspace_bytes);
  if (rc != MDG_OK) return rc;
  EnsSpreadArgs a{};
  ens_fill_operands(a, z_head, n_models, n_tail);
  a.mean = mean;
  a.sd = std_;
  a.bound = bound;
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.n_models = n_models;
  a.kappa = kappa;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (precision == MDG_PREC_F32) return launch_ens_spread<MDG_PREC_F32>(a, z_tail, w_sym, n_labels, ws, st);
  return launch_ens_spread<MDG_PREC_BF16X3>(a, z_tail, w_sym, n_labels, ws, st);
}

extern "C" int mdg_bilinear_ensemble_spread_topk(const float* const* z_head, const float* const* z_tail, const float* const* w_sym, int n_models,
                                                 float kappa, float* bound, int32_t* idx, float* mean, float* std_, int64_t n_head,
                                                 int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int k, int eligible,
                                                 void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                                                 int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_ensemble_spread_topk";
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(std::isfinite(kappa), "mdg_bilinear_ensemble_spread_topk: kappa must be finite (got %g)", static_cast<double>(kappa));
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "mdg_bilinear_ensemble_spread_topk: k must be in 1..%d (got %d)", TOPK_MAX_K, k);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "mdg_bilinear_ensemble_spread_topk: n_tail %lld does not fit the int32 column indices",
                (long long)n_tail);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, bound && idx && mean && std_, n_tail, n_labels, precision, workspace,
                          workspace_bytes);
  if (rc != MDG_OK) return rc;
  if (!mask)
    return ens_spread_topk_run<false>(z_head, z_tail, w_sym, n_models, kappa, bound, idx, mean, std_, n_head, n_tail, n_labels, precision, k,
                                      eligible, workspace, stream, nullptr, 0);
  return ens_spread_topk_run<true>(z_head, z_tail, w_sym, n_models, kappa, bound, idx, mean, std_, n_head, n_tail, n_labels, precision, k,
                                   eligible, workspace, stream, mask, plane_stride);
}
