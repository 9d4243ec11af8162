// Per-outcome probability counts over the checkpoint-ensembled all-pairs head for gfx950 (mdg_bilinear_ensemble_bincount / _split).
//
//   for every outcome l, given B ascending edges e[l,0..B-1]:
//     counts[l,b] = #{eligible (i,j) : e[l,b-1] <= P[l,i,j] < e[l,b]},  e[l,-1] = -inf, e[l,B] = +inf     (B + 1 int64 per outcome)
//     P[l,i,j]    = (sum_{m<K} sigmoid(z_head_m[i]^T W_sym_m[l] z_tail_m[j])) / K                          K = 1..8 checkpoints
//   = torch.bucketize(P[l], e[l], right=True) followed by a bincount over the eligible pairs.
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614, average the sigmoids
// of the checkpoints; notebooks/normalize_scores.py:36-74 turns that tensor into normalised ranks.)  With the edges at the
// probabilities of screened hits the cumulative counts are the hits' exact ranks among all pairs; with evenly spaced edges they are
// a histogram.  The mean of K sigmoids is not monotone in any one model's logit, so no combination of single-model counts gives
// these; here nothing of [L,N,N] is materialised.
//
// Two existing kernels joined: bincount.hip's epilogue on ensemble_select.hip's count-pass sweep.
//   score arithmetic: ensemble_select.hip's, which is ensemble.hip's general (non-symmetric) sweep bit for bit.  A workgroup (4
//     waves, 128 head rows of one outcome, one wave per SIMD) walks its tail tiles in chunks of CH; for every chunk it rebuilds
//     T_m = z_head_m[rows] . W_sym_m[l] (build_t) for m = 0..K-1 and sweeps the chunk with it, sigmoid 1 / (1 + expf(-s)), the
//     running sums of the chunk (psum, CH x 32 VGPRs) staying in registers across the models, divided once by K; every compare is on
//     that quotient.  With K = 1 the one T is built for the first chunk only.  build_t, pick, sigmoid_head, the eligibility test
//     and the layout's constants are ensemble_sweep.h's, shared by the family; the two-buffer ring is this file's own text
//     (sharing sweep text has moved hipcc's schedule before).
//   epilogue: bincount.hip's, run on the chunk's finished tiles after its last model.  The tile index of that loop is a run-time
//     value and the tile's sums are picked by wave-uniform selects: ONE copy of the counting code (copies inside the
//     unrolled stage loop sent psum to scratch).  One workgroup = one outcome, so the edge table is workgroup-uniform: the B edges
//     and B + 1 u32 counters (SPLIT: two tables) sit in LDS behind the stage buffers and the slabs.
//       fast path: every element is compared with e[0] and e[B-1]; "below all" and "at or above all" are counted by ballot +
//                  popcount into two wave-uniform registers, no memory traffic.
//       slow path: per group of 8 elements and only when some lane of the wave holds a value in [e[0], e[B-1]) (wave-uniform
//                  branch): a branch-free binary search over the LDS edges, the 8 searches level by level, then a non-returning
//                  workgroup-scope LDS add on bin = #{edges <= x} <= B, guarded by x >= e0 && x < elast.
//       end:       the waves add their two fast-path counts to counters 0 and B; the workgroup adds its non-zero counters to the
//                  int64 result with device-scope integer atomics (the entry point zeroes the result on the stream).  Integer sums:
//                  bit-identical from launch to launch whatever the order.
// Elements counted nowhere: select's spelling.  Ineligible and out-of-range elements (rows >= n_head too) become NaN, and so does
// nothing else: a NaN is neither < e[0] nor >= e[B-1], and "inside" is the ballot of x >= e[0] without the ballot of x >= e[B-1],
// which a NaN fails as well -- one more ballot term than bincount.hip, no correction of `below`, and a boundary tile does not take
// the search path because of such elements.  A NaN probability (non-finite operands) is counted nowhere for the same reason.
// Counter width: a workgroup sees at most 128 * n_tail values; the entry point keeps bincount's n_tail < 2^23.
// SPLIT instantiations (DESIGN.md 4x on this sweep): the mask words [row block of the wave][columns of the chunk's tiles] are loaded
// as ensemble_select.hip's MASKED path loads them, two plain loads per tile and lane ahead of the last model's T rebuild.  The bit
// excludes nothing, it picks the table: table 0 the eligible pairs whose bit is clear, table 1 those whose bit is set.  A tile whose
// words are all zero for the wave takes the unsplit path into table 0; otherwise the ballots of the fast path are split by the
// ballot of the bit and the slow path adds to cnt + bit * table stride + bin.  An ineligible element is NaN and reaches neither
// table whatever its bit, which is what forcing its bit clear amounts to.  The unsplit instantiations read no mask memory.
// Waits.  Every stage barrier waits vmcnt(0); the only vector-memory operations a wave has in flight there are the LDS-DMAs of the
// tile about to be read (the LDS adds of the epilogue are counted by lgkmcnt, the global adds come after the last tile).
#include "ensemble_sweep.h"

namespace {

constexpr int ENS_BIN_MAX_EDGES = 1024;     // mdg_bilinear_bincount_max_edges()
constexpr int ENS_BIN_TABLE = ENS_BIN_MAX_EDGES + 4;        // SPLIT: words from table 0 to table 1
// LDS behind the ring and the slabs (ENS_LDS): the edges, then one or two counter tables.
template <bool SPLIT> constexpr int ens_bin_lds = ENS_LDS + ENS_BIN_MAX_EDGES * 4 + (SPLIT ? 2 : 1) * ENS_BIN_TABLE * 4;

struct EnsBinArgs : EnsOperands {
  const float* edges;         // [n_labels, n_edges] ascending per outcome
  unsigned long long* counts;  // [n_labels, n_edges + 1] (SPLIT: two such tables), zeroed on the stream before the launch
  int64_t n_head, n_tail;
  int n_models;
  int n_edges;
  int eligible;                // mdg_topk_eligible
};

template <bool SPLIT> struct EnsBinKArgs : EnsBinArgs {};
template <> struct EnsBinKArgs<true> : EnsBinArgs { PairMask mask; };

// The wave's fast-path counts and the edge / counter tables in LDS.
struct EnsBinState {
  const float* eds;     // LDS: the outcome's B edges
  unsigned* cnt;        // LDS: B + 1 counters (SPLIT: table 1 is ENS_BIN_TABLE words on)
  float e0, elast;      // e[0], e[B-1]
  int B;
  unsigned below, above;       // wave-uniform: values < e[0], values >= e[B-1] (SPLIT: of table 0)
  unsigned below1, above1;     // SPLIT: the same of table 1
};

// Fast path of NE elements: counts below / above, returns whether any lane holds a value inside [e0, elast).  A NaN (an element
// counted nowhere) fails all three compares.
template <int NE>
__device__ __forceinline__ bool ens_bin_classify(EnsBinState& b, const float (&x)[NE]) {
  unsigned long long inside = 0ull;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const unsigned long long lo = __ballot(x[e] < b.e0), hi = __ballot(x[e] >= b.elast);
    b.below += __builtin_popcountll(lo);
    b.above += __builtin_popcountll(hi);
    inside |= __ballot(x[e] >= b.e0) & ~hi;
  }
  return inside != 0;
}

// ens_bin_classify with the two counting ballots split by the ballot of the element's bit: element e owns bit 8 (e >> 2) + (e & 3)
// of `w` (the lane's mask word, shifted to the group's first row).
template <int NE>
__device__ __forceinline__ bool ens_bin_classify_split(EnsBinState& b, const float (&x)[NE], unsigned w) {
  unsigned long long inside = 0ull;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const unsigned long long lo = __ballot(x[e] < b.e0), hi = __ballot(x[e] >= b.elast);
    const unsigned long long kb = __ballot(((w >> (8 * (e >> 2) + (e & 3))) & 1u) != 0u);
    b.below += __builtin_popcountll(lo & ~kb);
    b.below1 += __builtin_popcountll(lo & kb);
    b.above += __builtin_popcountll(hi & ~kb);
    b.above1 += __builtin_popcountll(hi & kb);
    inside |= __ballot(x[e] >= b.e0) & ~hi;
  }
  return inside != 0;
}

// Slow path of a group of NE elements (wave-uniform call): bin = #{edges <= x} by a branch-free binary search, all NE searches
// level by level; lanes whose element is outside [e0, elast) (or NaN) search along and add nothing.  Every index read lies in
// [0, B): base + half - 1 <= base + len - 1 <= B - 1 by the invariant.  SPLIT: the add goes to table `bit` of the element.
template <int NE, bool SPLIT>
__device__ __forceinline__ void ens_bin_search(const EnsBinState& b, const float (&x)[NE], unsigned w) {
  int base[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) base[e] = 0;
  int len = b.B;
  while (len > 1) {                                  // invariant: the bin of x[e] lies in [base[e], base[e] + len], base[e] + len <= B
    const int half = len >> 1;
#pragma unroll
    for (int e = 0; e < NE; ++e) base[e] += b.eds[base[e] + half - 1] <= x[e] ? half : 0;
    len -= half;
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    int bin = base[e] + (b.eds[base[e]] <= x[e] ? 1 : 0);
    if constexpr (SPLIT) bin += static_cast<int>((w >> (8 * (e >> 2) + (e & 3))) & 1u) * ENS_BIN_TABLE;
    if (x[e] >= b.e0 && x[e] < b.elast) __hip_atomic_fetch_add(b.cnt + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

template <int MODE, bool SPLIT, int CH>
__global__ __launch_bounds__(64 * ENS_NW, 1) void ensemble_bincount_kernel(const EnsBinKArgs<SPLIT> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "the ensemble's precisions");
  constexpr int NW = ENS_NW, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t l = blockIdx.y;
  const int K = p.n_models, mode = p.eligible;
  const float kf = static_cast<float>(K);
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  // LOWER: the last row block sweeps the most column tiles -- it goes first
  const int64_t rbk = mode == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  const int64_t wrow0 = row0 + wave * 32;        // this wave's rows: wrow0 .. wrow0 + 31
  const int nt = sweep_tiles(mode, row0, BM, p.n_head, p.n_tail);
  int64_t zr = wrow0 + (tid & 31);
  zr = zr < p.n_head ? zr : p.n_head - 1;

  // Kernel start: the outcome's edges into LDS, the counters to zero.  The barriers of the first build_t order this before the sweep.
  EnsBinState bs;
  {
    float* eds = reinterpret_cast<float*>(smem + ENS_LDS);
    unsigned* cnt = reinterpret_cast<unsigned*>(smem + ENS_LDS + ENS_BIN_MAX_EDGES * 4);
    const float* ge = p.edges + l * p.n_edges;
    for (int i = tid; i < p.n_edges; i += 64 * NW) eds[i] = ge[i];
    for (int i = tid; i <= p.n_edges; i += 64 * NW) cnt[i] = 0u;
    if constexpr (SPLIT)
      for (int i = tid; i <= p.n_edges; i += 64 * NW) cnt[ENS_BIN_TABLE + i] = 0u;
    bs.eds = eds;
    bs.cnt = cnt;
    bs.B = p.n_edges;
    bs.e0 = ge[0];
    bs.elast = ge[p.n_edges - 1];
    bs.below = bs.above = bs.below1 = bs.above1 = 0u;
  }

  auto build = [&](AFrag<MODE>& A, int m) {
    int t_o = tid;
    asm volatile("" : "+v"(t_o));
    const int r = t_o & 31, h = (t_o >> 5) & 1;
    TileSrc wl = pick(p.w, m);
    if constexpr (MODE == MDG_PREC_F32) wl.f32 += l * D * D;
    else { wl.hi += l * D * D; wl.lo += l * D * D; }
    build_t<MODE, NW>(A, pick(p.z_head, m) + zr * D, wl, smem, slab, t_o, r, h);
  };
  const unsigned* mrow = nullptr;                // SPLIT: the words of this wave's row block, outcome l
  if constexpr (SPLIT) {
    int64_t rb = wrow0 >> 5;
    rb = rb < p.mask.nrb ? rb : p.mask.nrb - 1;  // rows >= n_head only: clamped onto the last block, as the z_head row is
    mrow = p.mask.words + l * p.mask.plane_stride + rb * p.mask.ld;
  }

  AFrag<MODE> At;
  int par = 0;               // stage buffer of the next stage
  const int nch = (nt + CH - 1) / CH;
  for (int c = 0; c < nch; ++c) {
    const int s0 = c * CH;
    const int nc = nt - s0 < CH ? nt - s0 : CH;
    float psum[CH][2][16];
    unsigned mw[CH][2];      // SPLIT: lane (r, h)'s words of the chunk's tiles, columns 64 tile + r and + 32
    for (int m = 0; m < K; ++m) {
      const bool last = (m == K - 1);
      if constexpr (SPLIT) {
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
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this tile's DMAs
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
    // ---- the chunk's finished tiles through the counting epilogue (one copy of the counting code: `ci` is a run-time index, the
    // tile's sums are picked out of the register array by wave-uniform selects) ----
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
            if constexpr (SPLIT) { w0 = mw[c2][0]; w1 = mw[c2][1]; }
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
        // SPLIT: a tile without a known pair for the wave (wave-uniform) costs this ballot and goes the unsplit way
        bool mixed = false;
        unsigned mh[2] = {0u, 0u};                                             // bit acc_row(v, 0) of mh[t] <-> row acc_row(v, h)
        if constexpr (SPLIT) {
          mixed = __ballot((w0 | w1) != 0u) != 0;
          mh[0] = w0 >> (4 * h);
          mh[1] = w1 >> (4 * h);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = pr[t][8 * g + e];
            if constexpr (SPLIT) {
              if (mixed) {                                                     // acc_row(8 g + e, 0) = 16 g + 8 (e >> 2) + (e & 3)
                if (ens_bin_classify_split<8>(bs, x, mh[t] >> (16 * g))) ens_bin_search<8, true>(bs, x, mh[t] >> (16 * g));
                continue;
              }
            }
            if (ens_bin_classify<8>(bs, x)) ens_bin_search<8, false>(bs, x, 0u);
          }
      }
    }
  }

  // Kernel end: the waves' fast-path counts into counters 0 and B, the workgroup's non-zero counters into the global result.
  // SPLIT: the same for table 1, whose rows follow the gridDim.y rows of table 0 in the result.
  if ((tid & 63) == 0) {
    if (bs.below) __hip_atomic_fetch_add(bs.cnt, bs.below, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (bs.above) __hip_atomic_fetch_add(bs.cnt + bs.B, bs.above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if constexpr (SPLIT) {
      if (bs.below1) __hip_atomic_fetch_add(bs.cnt + ENS_BIN_TABLE, bs.below1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (bs.above1) __hip_atomic_fetch_add(bs.cnt + ENS_BIN_TABLE + bs.B, bs.above1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  unsigned long long* out = p.counts + l * (p.n_edges + 1);
  for (int i = tid; i <= bs.B; i += 64 * NW) {
    const unsigned cv = bs.cnt[i];
    if (cv) __hip_atomic_fetch_add(out + i, static_cast<unsigned long long>(cv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (SPLIT) {
    unsigned long long* out1 = p.counts + (static_cast<int64_t>(gridDim.y) + l) * (p.n_edges + 1);
    for (int i = tid; i <= bs.B; i += 64 * NW) {
      const unsigned cv = bs.cnt[ENS_BIN_TABLE + i];
      if (cv) __hip_atomic_fetch_add(out1 + i, static_cast<unsigned long long>(cv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int MODE, bool SPLIT>
int launch_ens_bincount(EnsBinKArgs<SPLIT>& a, const float* const* z_tail, const float* const* w_sym, int64_t n_labels, char* ws,
                        hipStream_t st, const char* fn) {
  int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, fn);
  if (rc != MDG_OK) return rc;
  constexpr int lds = ens_bin_lds<SPLIT>;
  rc = mdg_raise_dynamic_lds(reinterpret_cast<const void*>(ensemble_bincount_kernel<MODE, SPLIT, ENS_CH>), lds, fn);
  if (rc != MDG_OK) return rc;
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 32 * ENS_NW)), static_cast<unsigned>(n_labels));
  hipLaunchKernelGGL((ensemble_bincount_kernel<MODE, SPLIT, ENS_CH>), grid, dim3(64 * ENS_NW), lds, st, a);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}

// Both entry points: the checks (the family's, plus n_edges and bincount's n_tail rule), the zeroing of `tables`
// count tables on the stream, the launch.  SPLIT: the sweep keeps two tables by the bit of `mask`; tables == 2 without SPLIT is the
// split entry point without a mask (table 1 stays zero).
template <bool SPLIT>
int ens_bincount_run(const char* fn, int tables, const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                     int n_models, const float* edges, int64_t* counts, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_,
                     int n_edges, int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                     int64_t plane_stride) {
  int rc = ens_check_sizes(fn, n_models, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(n_edges >= 1 && n_edges <= ENS_BIN_MAX_EDGES, "%s: n_edges must be in 1..%d (got %d)", fn, ENS_BIN_MAX_EDGES, n_edges);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 23), "%s: n_tail %lld does not fit the 32-bit workgroup counters (< 2^23)", fn, (long long)n_tail);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t count_bytes = static_cast<size_t>(tables) * n_labels * (n_edges + 1) * sizeof(int64_t);
  auto zero = [&]() -> int {
    if (count_bytes && hipMemsetAsync(counts, 0, count_bytes, st) != hipSuccess) {
      (void)hipGetLastError();
      mdg_set_error("%s: zeroing the counts failed", fn);
      return MDG_ELAUNCH;
    }
    return MDG_OK;
  };
  if (n_head == 0 || n_labels == 0) return counts ? zero() : MDG_OK;        // no pair at all: every count is 0
  rc = ens_check_operands(fn, z_head, z_tail, w_sym, n_models, edges && counts, n_tail, n_labels, precision, workspace, workspace_bytes);
  if (rc != MDG_OK) return rc;
  EnsBinKArgs<SPLIT> a{};
  if constexpr (SPLIT) {
    const int mrc = sweep_mask_args(fn, a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  const int zrc = zero();
  if (zrc != MDG_OK) return zrc;
  ens_fill_operands(a, z_head, n_models, n_tail);
  a.edges = edges;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.n_head = n_head; a.n_tail = n_tail;
  a.n_models = n_models;
  a.n_edges = n_edges;
  a.eligible = eligible;
  char* ws = static_cast<char*>(workspace);
  if (precision == MDG_PREC_F32) return launch_ens_bincount<MDG_PREC_F32, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
  return launch_ens_bincount<MDG_PREC_BF16X3, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
}

}  // namespace

extern "C" size_t mdg_bilinear_ensemble_bincount_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_models,
                                                                 int precision) {
  (void)n_head;
  return ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
}

extern "C" int mdg_bilinear_ensemble_bincount(const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                                              int n_models, const float* edges, int64_t* counts, int64_t n_head, int64_t n_tail,
                                              int64_t n_labels, int64_t D_, int n_edges, int precision, int eligible, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return ens_bincount_run<false>("mdg_bilinear_ensemble_bincount", 1, z_head, z_tail, w_sym, n_models, edges, counts, n_head, n_tail, n_labels,
                                 D_, n_edges, precision, eligible, workspace, workspace_bytes, stream, nullptr, 0);
}

extern "C" int mdg_bilinear_ensemble_bincount_split(const float* const* z_head, const float* const* z_tail, const float* const* w_sym,
                                                    int n_models, const float* edges, int64_t* counts, int64_t n_head, int64_t n_tail,
                                                    int64_t n_labels, int64_t D_, int n_edges, int precision, int eligible,
                                                    void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                                                    int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_ensemble_bincount_split";
  if (!mask)                                              // the unsplit sweep into table 0 of a zeroed result; no mask memory is read
    return ens_bincount_run<false>(fn, 2, z_head, z_tail, w_sym, n_models, edges, counts, n_head, n_tail, n_labels, D_, n_edges, precision,
                                   eligible, workspace, workspace_bytes, stream, nullptr, 0);
  return ens_bincount_run<true>(fn, 2, z_head, z_tail, w_sym, n_models, edges, counts, n_head, n_tail, n_labels, D_, n_edges, precision,
                                eligible, workspace, workspace_bytes, stream, mask, plane_stride);
}
