// Per-outcome score counts of the all-pairs bilinear sweep for gfx950 (mdg_bilinear_bincount).
//
//   for every outcome l, given B ascending edges e[l,0..B-1]:
//     counts[l,b] = #{eligible (i,j) : e[l,b-1] <= S[l,i,j] < e[l,b]},  e[l,-1] = -inf, e[l,B] = +inf     (B + 1 int64 per outcome)
//   = torch.bucketize(S, e[l], right=True) followed by a bincount, S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j].
//
// The histogram part of the reducing epilogue (top-k is topk.hip): nothing of [L,N,N] is materialised.  With the edges at the
// scores of screened hits, the cumulative counts are the hits' exact ranks among all pairs (notebooks/normalize_scores.py:36-74);
// with evenly spaced edges they are a score histogram.  The two kernels below are the row-statistics sweeps of bilinear.hip
// as topk.hip carries them (same prologue, same staging, same MFMA sequence per accumulator element) with the epilogue replaced, so
// every counted score equals the general sweep's bit for bit in f32 / bf16x3 (bf16 / f16: the 16x16x32 regrouping, <= 2e-6 of the
// scale, as for top-k).  The launch side is shared with topk.hip and select.hip (sweep_reduce.h).
//
// Epilogue.  One workgroup = one outcome (blockIdx.y), so the edge table is workgroup-uniform: the B edges and B + 1 u32
// counters sit in LDS behind the three stage buffers (96 KB + 8 KB + 16 B of 160 KB).
//   fast path: every accumulator element is compared with e[0] and e[B-1]; "below all" and "at or above all" are counted by
//              ballot + popcount into two wave-uniform registers -- two compares per element, no memory traffic.  With the
//              edges in the extreme tail (ranks of hits) nearly every score ends here.
//   slow path: elements inside [e[0], e[B-1]) -- taken per group of 8 accumulator elements and only when some lane of the wave has
//              one (wave-uniform branch): a branch-free binary search over the LDS edges, the 8 searches of a group level by
//              level so that their LDS reads overlap (ceil(log2 B) + 1 reads each), then a non-returning LDS add on the bin.
//   end:       the waves add their two fast-path counts to counters 0 and B; the workgroup adds its non-zero counters to the global
//              int64 result with device-scope integer atomics (the entry point zeroes the result on the stream).  Integer sums:
//              the result is bit-identical from launch to launch whatever the order.
// Counter width: a workgroup sees at most BM * n_tail scores (BM = 256, or 512 in the 16-bit sweep), so its u32 counters
// cannot overflow while n_tail < 2^23; the entry point refuses more.  Ineligible elements (and rows past n_head) become -inf
// and are taken out of the "below all" count again; scores are finite by contract (a NaN is counted nowhere).
//
// SPLIT instantiations (mdg_bilinear_bincount_split): the same counts kept in TWO tables, by the element's bit of a
// known-pair bitmap (pairmask.hip) -- table 0: eligible pairs whose bit is clear, table 1: eligible pairs whose bit is set.  Nothing
// is excluded: the two tables sum to the counts above.  The mask slots of the ring sit right behind the stage buffers, the edges and
// the two counter tables behind them.  A (sub-)tile whose words are all zero for the wave takes the path above into table 0; otherwise the ballots of the
// fast path are split by the ballot of the bit and the slow path adds to cnt + bit * stride + bin.  An ineligible element has its
// bit forced clear, so that its -inf and the correction for it both land in table 0.  The SPLIT = false kernels are what they were.
#include "sweep_reduce.h"

namespace {

constexpr int BINCOUNT_MAX_EDGES = 1024;
constexpr int BINCOUNT_TABLE = BINCOUNT_MAX_EDGES + 4;      // SPLIT: words from table 0 to table 1
// LDS behind the ring's (sweep_lds_bytes: the stage buffers, SPLIT: and the mask slots): the edges, then one or two counter tables.
template <bool SPLIT> constexpr int bincount_tables_bytes = BINCOUNT_MAX_EDGES * 4 + (SPLIT ? 2 : 1) * BINCOUNT_TABLE * 4;

struct BincountArgs {
  const float* z_head;
  TileSrc zt;
  TileSrc w;            // W_sym (this call's labels); nrows = D
  const float* edges;   // [n_labels, n_edges] ascending per outcome
  unsigned long long* counts;   // [n_labels, n_edges + 1], zeroed on the stream before the launch
  int64_t n_head, n_tail;
  int n_edges;
  int eligible;         // mdg_topk_eligible
};

// The kernel argument: BincountArgs itself, plus the known-pair bitmap in the SPLIT instantiations (mdg_bilinear_bincount_split,
// whose counts are [2][n_labels][n_edges + 1]).
template <bool SPLIT> struct BincountKArgs : BincountArgs {};
template <> struct BincountKArgs<true> : BincountArgs { PairMask mask; };

__device__ __forceinline__ bool bincount_eligible(int mode, int64_t row, int64_t col, int64_t n_head, int64_t n_tail) {
  const bool pair = mode == MDG_TOPK_NOT_SELF ? col != row : col < row;                 // (bitwise: selects, no branches)
  return (row < n_head) & (col < n_tail) & ((mode == MDG_TOPK_ALL) | pair);
}

// The wave's two fast-path counts and the edge / counter tables in LDS.
struct BinState {
  const float* eds;     // LDS: the outcome's B edges
  unsigned* cnt;        // LDS: B + 1 counters
  float e0, elast;      // e[0], e[B-1]
  int B;
  unsigned below, above;       // wave-uniform: scores < e[0], scores >= e[B-1]
};

// Fast path of NE accumulator elements: counts below / above, returns whether any lane holds a score inside [e0, elast).
// An ineligible element arrives as -inf: it lands in `below`, and bincount_mask took it out of `below` beforehand.
template <int NE>
__device__ __forceinline__ bool bincount_classify(BinState& b, const float (&x)[NE]) {
  unsigned long long outside = ~0ull;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const unsigned long long lo = __ballot(x[e] < b.e0), hi = __ballot(x[e] >= b.elast);
    b.below += __builtin_popcountll(lo);
    b.above += __builtin_popcountll(hi);
    outside &= lo | hi;
  }
  return (~outside & __ballot(true)) != 0;
}

// An element of a tile that is not wholly eligible: the score, or -inf (and one off `below`, where -inf will be counted).
__device__ __forceinline__ float bincount_mask(BinState& b, bool ok, float x) {
  b.below -= __builtin_popcountll(__ballot(!ok));
  return ok ? x : -INFINITY;
}

// Slow path of a group of NE elements (wave-uniform call): bin = #{edges <= x} by a branch-free binary search, all NE
// searches level by level; lanes whose element is outside [e0, elast) (or NaN) search along and add nothing.
template <int NE>
__device__ __forceinline__ void bincount_search(const BinState& b, const float (&x)[NE]) {
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
    const int bin = base[e] + (b.eds[base[e]] <= x[e] ? 1 : 0);
    if (x[e] >= b.e0 && x[e] < b.elast) __hip_atomic_fetch_add(b.cnt + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// SPLIT: the fast-path counts of table 1 (set bits); BinState's own two are table 0's.
struct BinSplit {
  unsigned below1, above1;
};

// bincount_classify with the two ballots split by the ballot of the element's bit: element e owns bit POS(e) = ROWSTEP (e >> 2) +
// (e & 3) of `w` (the lane's mask word, shifted to the group's first row; the bits of ineligible elements already cleared).
template <int NE, int ROWSTEP>
__device__ __forceinline__ bool bincount_classify_split(BinState& b, BinSplit& s, const float (&x)[NE], unsigned w) {
  unsigned long long outside = ~0ull;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const unsigned long long lo = __ballot(x[e] < b.e0), hi = __ballot(x[e] >= b.elast);
    const unsigned long long kb = __ballot(((w >> (ROWSTEP * (e >> 2) + (e & 3))) & 1u) != 0u);
    b.below += __builtin_popcountll(lo & ~kb);
    s.below1 += __builtin_popcountll(lo & kb);
    b.above += __builtin_popcountll(hi & ~kb);
    s.above1 += __builtin_popcountll(hi & kb);
    outside &= lo | hi;
  }
  return (~outside & __ballot(true)) != 0;
}

// bincount_search with the LDS add on cnt + bit * BINCOUNT_TABLE + bin.
template <int NE, int ROWSTEP>
__device__ __forceinline__ void bincount_search_split(const BinState& b, const float (&x)[NE], unsigned w) {
  int base[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) base[e] = 0;
  int len = b.B;
  while (len > 1) {
    const int half = len >> 1;
#pragma unroll
    for (int e = 0; e < NE; ++e) base[e] += b.eds[base[e] + half - 1] <= x[e] ? half : 0;
    len -= half;
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int bit = static_cast<int>((w >> (ROWSTEP * (e >> 2) + (e & 3))) & 1u);
    const int bin = base[e] + (b.eds[base[e]] <= x[e] ? 1 : 0) + bit * BINCOUNT_TABLE;
    if (x[e] >= b.e0 && x[e] < b.elast) __hip_atomic_fetch_add(b.cnt + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// Kernel start: the outcome's edges into LDS, the counters to zero.  The prologue's barriers order this before the sweep.
// `tab`: the edges, then the counter table(s) (SPLIT: two, BINCOUNT_TABLE words apart).
template <bool SPLIT>
__device__ __forceinline__ void bincount_begin(BinState& b, const BincountArgs& p, char* tab, int64_t l, int tid) {
  float* eds = reinterpret_cast<float*>(tab);
  unsigned* cnt = reinterpret_cast<unsigned*>(tab + BINCOUNT_MAX_EDGES * 4);
  const float* ge = p.edges + l * p.n_edges;
  for (int i = tid; i < p.n_edges; i += 512) eds[i] = ge[i];
  for (int i = tid; i <= p.n_edges; i += 512) cnt[i] = 0u;
  if constexpr (SPLIT)
    for (int i = tid; i <= p.n_edges; i += 512) cnt[BINCOUNT_TABLE + i] = 0u;
  b.eds = eds;
  b.cnt = cnt;
  b.B = p.n_edges;
  b.e0 = ge[0];
  b.elast = ge[p.n_edges - 1];
  b.below = 0u;
  b.above = 0u;
}

// Kernel end: the waves' fast-path counts into counters 0 and B, the workgroup's non-zero counters into the global result.
// SPLIT: the same for table 1, whose rows follow the gridDim.y rows of table 0 in the result.
template <bool SPLIT>
__device__ __forceinline__ void bincount_end(const BinState& b, const BinSplit& s, const BincountArgs& p, int64_t l, int tid) {
  if ((tid & 63) == 0) {
    if (b.below) __hip_atomic_fetch_add(b.cnt, b.below, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (b.above) __hip_atomic_fetch_add(b.cnt + b.B, b.above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if constexpr (SPLIT) {
      if (s.below1) __hip_atomic_fetch_add(b.cnt + BINCOUNT_TABLE, s.below1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (s.above1) __hip_atomic_fetch_add(b.cnt + BINCOUNT_TABLE + b.B, s.above1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  unsigned long long* out = p.counts + l * (p.n_edges + 1);
  for (int i = tid; i <= b.B; i += 512) {
    const unsigned c = b.cnt[i];
    if (c) __hip_atomic_fetch_add(out + i, static_cast<unsigned long long>(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (SPLIT) {
    unsigned long long* out1 = p.counts + (static_cast<int64_t>(gridDim.y) + l) * (p.n_edges + 1);
    for (int i = tid; i <= b.B; i += 512) {
      const unsigned c = b.cnt[BINCOUNT_TABLE + i];
      if (c) __hip_atomic_fetch_add(out1 + i, static_cast<unsigned long long>(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The two kernels below carry the sweep itself -- prologue, three-buffer LDS-DMA ring with its hand-counted waits, mask-word DMAs --
// as topk.hip, select.hip and bincount.hip each do: sharing that text between them was tried and measured 0.2 - 2.9 % slower in some
// instantiations whichever way it was spelled, so a change to the ring is made in all three files.
// ---- f32 / bf16x3: bilinear_allpairs_kernel<MODE, ROWSTATS, 8> with the counting epilogue ---------------------------------------
// SPLIT: the 64 words [row block of the wave][columns of the tile] ride with the tile: one more LDS-DMA per wave and tile group into
// a slot of the wave's own, so a group is NDMA + 1 = 5 instructions and the wait keeps 5 in flight.  Lane (r, h) reads words r and
// 32 + r of the slot (its columns for t = 0, 1); its rows are bits acc_row(v, h) of them.
template <int MODE, bool SPLIT>
__global__ __launch_bounds__(512, 1) void bilinear_bincount_kernel(const BincountKArgs<SPLIT> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "32x32 sweep of the fp32-grade modes");
  constexpr int NW = 8, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int64_t l = blockIdx.y;
  // LOWER: the last row block sweeps the most column tiles -- it goes first
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  BinState bs;
  BinSplit sp{0u, 0u};
  bincount_begin<SPLIT>(bs, p, smem + sweep_lds_bytes<SPLIT, 1>, l, tid);

  // ---------------- prologue: T = z_head[rows] . W_sym[l], kept as the A operand (as in bilinear.hip) -------------
  AFrag<MODE> At;
  {
    AFrag<MODE> Az;
    int64_t zr = row0 + wave * 32 + r;
    zr = zr < p.n_head ? zr : p.n_head - 1;
    afrag_from_global<MODE>(Az, p.z_head + zr * D, h);
    TileSrc ws = p.w;
    if constexpr (MODE == MDG_PREC_F32) ws.f32 += l * D * D;
    else { ws.hi += l * D * D; ws.lo += l * D * D; }
    char* const slab = smem + wave * 8192;       // [32 rows][64 cols] fp32, chunk-swizzled
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      u32x4 regs[32 / NW];
      stage_load<MODE, NW>(ws, 64 * st, tid, regs);
      __syncthreads();                            // slabs of the previous half are consumed
      stage_write<MODE, NW>(buf0, tid, regs);
      __syncthreads();
      f32x16 acc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
      compute_tile<MODE>(Az, buf0, r, h, acc);
      __syncthreads();                            // every wave is done reading buf0
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
    }
    __syncthreads();
  }

  // ---------------- sweep: three stage buffers, prefetch distance two, ascending column tiles -------------
  const int nst = sweep_tiles(p.eligible, row0, BM, p.n_head, p.n_tail);
  const int64_t wrow0 = row0 + wave * 32;        // this wave's rows: wrow0 .. wrow0 + 31
  const int mode = p.eligible;
  constexpr int NDMA = 32 / NW;                  // LDS-DMA instructions per wave and tile
  static_assert(NDMA == 4, "vmcnt immediate below");
  // SPLIT: the wave's mask slot of stage buffer b is mslot + b * sweep_mask_stage<1>; every group of DMAs below (tile + words) is
  // issued together, so "the last group in flight" is 5 instructions instead of 4 and nothing else about the chain changes.
  constexpr int MSTAGE = sweep_mask_stage<1>;
  const char* const mslot = smem + 3 * STAGE_BYTES + wave * PAIRMASK_SLOT;
  const unsigned* mplane = nullptr;
  if constexpr (SPLIT) mplane = p.mask.words + l * p.mask.plane_stride;             // workgroup-uniform
  stage_dma<MODE>(p.zt, 0, smem, wave, lane, NW);
  if constexpr (SPLIT) pairmask_dma(p.mask, mplane, wrow0 >> 5, 0, lane, lds_addr(mslot));
  stage_dma<MODE>(p.zt, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, smem + STAGE_BYTES, wave, lane, NW);
  if constexpr (SPLIT) pairmask_dma(p.mask, mplane, wrow0 >> 5, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, lane, lds_addr(mslot + MSTAGE));
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    const int64_t tcol0 = static_cast<int64_t>(s) * BN;
    if constexpr (SPLIT) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");       // = NDMA + 1 mask DMA: group s landed, group s+1 stays in flight
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // = NDMA: tile s landed, tile s+1 stays in flight
    __builtin_amdgcn_s_barrier();      // tile s landed for every wave; every wave finished reading tile s-1
    const int nxt2 = cur == 0 ? 2 : cur - 1;                           // (cur + 2) % 3 = buffer of tile s-1
    const int s2 = s + 2 < nst ? s + 2 : nst - 1;                      // past the end: a copy nobody consumes
    stage_dma<MODE>(p.zt, static_cast<int64_t>(s2) * BN, smem + nxt2 * STAGE_BYTES, wave, lane, NW);
    if constexpr (SPLIT) pairmask_dma(p.mask, mplane, wrow0 >> 5, static_cast<int64_t>(s2) * BN, lane, lds_addr(mslot + nxt2 * MSTAGE));
    const char* lds = smem + cur * STAGE_BYTES;
    const char* const mcur = mslot + cur * MSTAGE;                     // this wave's words of tile s (its own DMA: landed with the wait above)
    cur = cur == 2 ? 0 : cur + 1;
    if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31) continue;       // wave-uniform: no column of this tile is below any of my rows
    unsigned w0 = 0u, w1 = 0u;                                          // SPLIT: read ahead of the MFMAs, whose issue hides the LDS latency
    if constexpr (SPLIT) { w0 = pairmask_word(mcur, r); w1 = pairmask_word(mcur, 32 + r); }
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    compute_tile<MODE>(At, lds, r, h, acc);
    // whole tile eligible for every row of the wave (wave-uniform): no per-element masking
    const bool plain = tcol0 + BN <= p.n_tail && wrow0 + 32 <= p.n_head &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
    // SPLIT: a tile without a known pair for the wave (wave-uniform) costs two reads and this ballot, and goes the unsplit way
    bool mixed = false;
    unsigned mw[2] = {0u, 0u};                                         // bit acc_row(v, 0) of mw[t] <-> row acc_row(v, h)
    if constexpr (SPLIT) {
      mixed = __ballot((w0 | w1) != 0u) != 0;
      mw[0] = w0 >> (4 * h);
      mw[1] = w1 >> (4 * h);
    }
    if (!plain) {
      unsigned okb[2] = {0u, 0u};                                      // SPLIT: an ineligible element has its bit forced clear (table 0)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const bool ok = bincount_eligible(mode, wrow0 + acc_row(v, h), tcol0 + 32 * t + r, p.n_head, p.n_tail);
          acc[t][v] = bincount_mask(bs, ok, acc[t][v]);
          if constexpr (SPLIT) okb[t] |= ok ? 1u << acc_row(v, 0) : 0u;
        }
      if constexpr (SPLIT) { mw[0] &= okb[0]; mw[1] &= okb[1]; }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = acc[t][8 * g + e];
        if constexpr (SPLIT) {
          if (mixed) {                                                 // acc_row(8 g + e, 0) = 16 g + 8 (e >> 2) + (e & 3)
            if (bincount_classify_split<8, 8>(bs, sp, x, mw[t] >> (16 * g))) bincount_search_split<8, 8>(bs, x, mw[t] >> (16 * g));
            continue;
          }
        }
        if (bincount_classify<8>(bs, x)) bincount_search<8>(bs, x);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bincount_end<SPLIT>(bs, sp, p, l, tid);
}

// ---- bf16 / f16: bilinear_rowstats16_kernel (v_mfma_f32_16x16x32, 64 rows per wave) with the counting epilogue -----------------
// SPLIT: the wave's 64 rows are two row blocks of the mask, so two mask DMAs per tile group (2 + 2 = 4 in flight) and eight words per
// lane and tile: word [ct][rt >> 1] holds the rows of acc[rt] at bits 16 (rt & 1) + 4 g4 + i.  Decided per 16-column sub-tile.
template <int MODE, bool SPLIT>
__global__ __launch_bounds__(512, 1) void bilinear_bincount16_kernel(const BincountKArgs<SPLIT> p) {
  static_assert(kSingle16<MODE>, "one rounded 16-bit product per k step");
  constexpr int NW = 8, BM = 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, c16 = lane & 15, g4 = lane >> 4;
  const int64_t l = blockIdx.y;
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  BinState bs;
  BinSplit sp{0u, 0u};
  bincount_begin<SPLIT>(bs, p, smem + sweep_lds_bytes<SPLIT, 2>, l, tid);
  // ---- prologue: T = z_head[rows] . W_sym[l] (32x32x16 products, as every other path), re-laid out for 16x16x32 ----
  bf16x8 A16[4][4];                                  // [row tile of 16][k step of 32]: lane (c16, g4) holds row c16, k = 32 ks + 8 g4 ..+7
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    AFrag<MODE> Az;
    int64_t zr = row0 + (wave * 2 + rb) * 32 + r;
    zr = zr < p.n_head ? zr : p.n_head - 1;
    afrag_from_global<MODE>(Az, p.z_head + zr * D, h);
    TileSrc ws = p.w;
    ws.hi += l * D * D;
    char* const slab = smem + wave * 8192;             // [32 rows][64 cols] fp32, chunk-swizzled
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      u32x4 regs[32 / NW];
      stage_load<MODE, NW>(ws, 64 * st, tid, regs);
      __syncthreads();
      stage_write<MODE, NW>(buf0, tid, regs);
      __syncthreads();
      f32x16 acc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
      compute_tile<MODE>(Az, buf0, r, h, acc);
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = acc_row(v, h), n = 32 * t + r;
          *reinterpret_cast<float*>(slab + tile_off<256>(row, n >> 2) + (n & 3) * 4) = acc[t][v];
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
        for (int ksl = 0; ksl < 2; ++ksl) {
          const int row = 16 * rt2 + c16, chunk = (32 * ksl + 8 * g4) >> 2;         // 4-float chunks of the 64-column half
          const float4 v0 = *reinterpret_cast<const float4*>(slab + tile_off<256>(row, chunk));
          const float4 v1 = *reinterpret_cast<const float4*>(slab + tile_off<256>(row, chunk + 1));
          bf16x8 hi, lo;
          split8<MODE>(v0, v1, hi, lo);
          A16[2 * rb + rt2][2 * st + ksl] = hi;
        }
    }
    __syncthreads();
  }
  // ---- sweep ----
  const int nst = sweep_tiles(p.eligible, row0, BM, p.n_head, p.n_tail);
  const int64_t wrow0 = row0 + wave * 64;            // this wave's rows: wrow0 .. wrow0 + 63
  const int mode = p.eligible;
  constexpr int MSTAGE = sweep_mask_stage<2>;
  const char* const mslot = smem + 3 * STAGE_BYTES + wave * 2 * PAIRMASK_SLOT;
  const unsigned* mplane = nullptr;
  if constexpr (SPLIT) mplane = p.mask.words + l * p.mask.plane_stride;             // workgroup-uniform
  auto mask_dma = [&](int64_t col0, const char* slot) {               // the group's two mask DMAs: row blocks wrow0 / 32 and + 1
    if constexpr (SPLIT) {
      pairmask_dma(p.mask, mplane, wrow0 >> 5, col0, lane, lds_addr(slot));
      pairmask_dma(p.mask, mplane, (wrow0 >> 5) + 1, col0, lane, lds_addr(slot + PAIRMASK_SLOT));
    }
  };
  stage_dma<MODE>(p.zt, 0, smem, wave, lane, NW);
  if constexpr (SPLIT) mask_dma(0, mslot);
  stage_dma<MODE>(p.zt, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, smem + STAGE_BYTES, wave, lane, NW);
  if constexpr (SPLIT) mask_dma(static_cast<int64_t>(1 < nst ? 1 : 0) * BN, mslot + MSTAGE);
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    const int64_t tcol0 = static_cast<int64_t>(s) * BN;
    if constexpr (SPLIT) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // = 2 tile + 2 mask DMAs per group: group s landed, group s+1 stays in flight
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");           // = LDS-DMA instructions per wave and tile: tile s landed, tile s+1 stays in flight
    __builtin_amdgcn_s_barrier();
    const int nxt2 = cur == 0 ? 2 : cur - 1;
    const int s2 = s + 2 < nst ? s + 2 : nst - 1;
    stage_dma<MODE>(p.zt, static_cast<int64_t>(s2) * BN, smem + nxt2 * STAGE_BYTES, wave, lane, NW);
    if constexpr (SPLIT) mask_dma(static_cast<int64_t>(s2) * BN, mslot + nxt2 * MSTAGE);
    const char* lds = smem + cur * STAGE_BYTES;
    const char* const mcur = mslot + cur * MSTAGE;                     // this wave's words of tile s (its own DMAs: landed with the wait above)
    cur = cur == 2 ? 0 : cur + 1;
    if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 63) continue;       // wave-uniform: nothing below the diagonal for my rows
    const bool plain = tcol0 + BN <= p.n_tail && wrow0 + 64 <= p.n_head &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 63));
    unsigned mwd[4][2];                                                // SPLIT: the tile's eight words, read ahead of the MFMAs that hide the LDS latency
    if constexpr (SPLIT) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        mwd[ct][0] = pairmask_word(mcur, 16 * ct + c16);
        mwd[ct][1] = pairmask_word(mcur + PAIRMASK_SLOT, 16 * ct + c16);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4v acc[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(16 * ct + c16, 4 * ks + g4));
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = mma16x16<MODE>(A16[rt][ks], b, acc[rt]);
      }
      const int64_t col = tcol0 + 16 * ct + c16;
      // SPLIT: decided per 16-column sub-tile (wave-uniform); word g holds rows 32 g .. 32 g + 31, i.e. acc[2 g] and acc[2 g + 1]
      bool mixed = false;
      unsigned mw[2] = {0u, 0u};                                       // bit 16 (rt & 1) + i of mw[rt >> 1] <-> row 16 rt + 4 g4 + i
      if constexpr (SPLIT) {
        mixed = __ballot((mwd[ct][0] | mwd[ct][1]) != 0u) != 0;
        mw[0] = mwd[ct][0] >> (4 * g4);
        mw[1] = mwd[ct][1] >> (4 * g4);
      }
      if (!plain) {
        unsigned okb[2] = {0u, 0u};                                    // SPLIT: an ineligible element has its bit forced clear (table 0)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool ok = bincount_eligible(mode, wrow0 + 16 * rt + 4 * g4 + i, col, p.n_head, p.n_tail);
            acc[rt][i] = bincount_mask(bs, ok, acc[rt][i]);
            if constexpr (SPLIT) okb[rt >> 1] |= ok ? 1u << (16 * (rt & 1) + i) : 0u;
          }
        if constexpr (SPLIT) { mw[0] &= okb[0]; mw[1] &= okb[1]; }
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = acc[2 * g + (e >> 2)][e & 3];
        if constexpr (SPLIT) {
          if (mixed) {
            if (bincount_classify_split<8, 16>(bs, sp, x, mw[g])) bincount_search_split<8, 16>(bs, x, mw[g]);
            continue;
          }
        }
        if (bincount_classify<8>(bs, x)) bincount_search<8>(bs, x);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bincount_end<SPLIT>(bs, sp, p, l, tid);
}

template <int MODE, bool SPLIT>
int launch_bincount(BincountKArgs<SPLIT>& a, const float* z_tail, const float* w_sym, int64_t n_labels, char* ws, hipStream_t st, const char* fn) {
  make_head_images<MODE>(a.zt, a.w, z_tail, w_sym, a.n_tail, n_labels, ws, st);
  MDG_CHECK_LAUNCH(fn);
  constexpr int tables = bincount_tables_bytes<SPLIT>;
  if constexpr (kSingle16<MODE>) return sweep_launch<SPLIT, 2>(bilinear_bincount16_kernel<MODE, SPLIT>, a, n_labels, tables, st, fn);
  else return sweep_launch<SPLIT, 1>(bilinear_bincount_kernel<MODE, SPLIT>, a, n_labels, tables, st, fn);
}

// Both entry points: the checks, the zeroing of `tables` count tables on the stream, the launch.  SPLIT: the sweep keeps two tables by
// the bit of `mask`; tables == 2 without SPLIT is the split entry point without a mask (table 1 stays zero).
template <bool SPLIT>
int bincount_run(const char* fn, int tables, const float* z_head, const float* z_tail, const float* w_sym, const float* edges, int64_t* counts,
                 int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_edges, int precision, int eligible, void* workspace,
                 size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride) {
  const int rc = sweep_check_sizes(fn, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(n_edges >= 1 && n_edges <= BINCOUNT_MAX_EDGES, "%s: n_edges must be in 1..%d (got %d)", fn, BINCOUNT_MAX_EDGES, n_edges);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 23), "%s: n_tail %lld does not fit the 32-bit workgroup counters (< 2^23)", fn, (long long)n_tail);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail,
                "%s: NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)", fn, (long long)n_head, (long long)n_tail);
  BincountKArgs<SPLIT> a{};
  if constexpr (SPLIT) {
    const int mrc = sweep_mask_args(fn, a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  if (n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(edges && counts, "%s: null pointer", fn);
  const bool empty = n_head == 0 || n_tail == 0;          // no pair at all: every count is 0
  if (!empty) {
    const int orc = sweep_check_operands(fn, z_head, z_tail, w_sym, true, n_tail, n_labels, precision, workspace, workspace_bytes);
    if (orc != MDG_OK) return orc;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, static_cast<size_t>(tables) * n_labels * (n_edges + 1) * sizeof(int64_t), st) != hipSuccess) {
    (void)hipGetLastError();
    mdg_set_error("%s: zeroing the counts failed", fn);
    return MDG_ELAUNCH;
  }
  if (empty) return MDG_OK;
  a.z_head = z_head;
  a.edges = edges;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.n_head = n_head; a.n_tail = n_tail;
  a.n_edges = n_edges;
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  char* ws = static_cast<char*>(workspace);
  switch (precision) {
    case MDG_PREC_F32: return launch_bincount<MDG_PREC_F32, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
    case MDG_PREC_BF16X3: return launch_bincount<MDG_PREC_BF16X3, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
    case MDG_PREC_BF16: return launch_bincount<MDG_PREC_BF16, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
    default: return launch_bincount<MDG_PREC_F16, SPLIT>(a, z_tail, w_sym, n_labels, ws, st, fn);
  }
}

}  // namespace

extern "C" int mdg_bilinear_bincount_max_edges(void) { return BINCOUNT_MAX_EDGES; }

extern "C" size_t mdg_bilinear_bincount_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_edges, int precision) {
  (void)n_head; (void)n_edges;
  return head_images_workspace_bytes(n_tail, n_labels, D_, precision);
}

extern "C" int mdg_bilinear_bincount(const float* z_head, const float* z_tail, const float* w_sym, const float* edges, int64_t* counts,
                                     int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_edges, int precision, int eligible,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return bincount_run<false>("mdg_bilinear_bincount", 1, z_head, z_tail, w_sym, edges, counts, n_head, n_tail, n_labels, D_, n_edges, precision,
                             eligible, workspace, workspace_bytes, stream, nullptr, 0);
}

extern "C" int mdg_bilinear_bincount_split(const float* z_head, const float* z_tail, const float* w_sym, const float* edges, int64_t* counts,
                                           int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int n_edges, int precision,
                                           int eligible, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                                           int64_t plane_stride) {
  if (!mask)                                              // the twin's sweep into table 0 of a zeroed result
    return bincount_run<false>("mdg_bilinear_bincount_split", 2, z_head, z_tail, w_sym, edges, counts, n_head, n_tail, n_labels, D_, n_edges,
                               precision, eligible, workspace, workspace_bytes, stream, nullptr, 0);
  return bincount_run<true>("mdg_bilinear_bincount_split", 2, z_head, z_tail, w_sym, edges, counts, n_head, n_tail, n_labels, D_, n_edges,
                            precision, eligible, workspace, workspace_bytes, stream, mask, plane_stride);
}
