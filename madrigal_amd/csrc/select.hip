// Threshold selection inside the all-pairs bilinear sweep for gfx950 (mdg_bilinear_select_count / mdg_bilinear_select_fill).
//
//   for every outcome l with its cut thr[l]: all eligible pairs (i, j) with S[l,i,j] >= thr[l], S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j],
//   as CSR over the n_labels * n_head rows (l, i): row_ptr, then per hit its column j and its score.
//
// The set-valued product of the head ("every pair above a cut"): nothing of [L,N,N] is materialised.  The kernels below are
// the row-statistics sweeps of bilinear.hip as topk.hip and bincount.hip carry them (same prologue, same staging, same MFMA sequence
// per accumulator element, same LOWER tile skipping) with the epilogue replaced, so every compared and stored score equals the general
// sweep's bit for bit in f32 / bf16x3 (bf16 / f16: the 16x16x32 regrouping, <= 2e-6 of the scale, as for top-k).  The launch side
// is shared with those two files (sweep_reduce.h).
//
// Two passes over the same sweep (FILL = false / true), because the size of the result is not known beforehand:
//   count: row_counts[l,i] = #{eligible j : S[l,i,j] >= thr[l]}.  The caller's exclusive prefix sum over the flattened counts is
//          row_ptr (int64, n_labels * n_head + 1 entries).
//   fill:  the same sweep again; hit number q of row (l,i) in ascending column order goes to slot row_ptr[l * n_head + i] + q.
// Epilogue.  Every head row belongs to ONE wave, G lanes per row (G = 32 on the 32x32 MFMA, 16 on 16x16x32), each lane holding one
// column; per accumulator register and lane there is one running u32 `run` = hits of that row in the tiles swept so far
// (uniform over the G lanes; 16 registers in either layout).
//   pass-through: one v_cmp per accumulator element (x >= thr), OR-ed into one ballot per tile (per 16-column sub-tile in the
//                 16-bit sweep): a tile without a hit costs what ROWSTATS' add + max costs;
//   hit path:     (wave-uniform branch) per accumulator register one ballot; the popcount of the row group's bits is added to `run`;
//                 FILL: a lane with a hit reads row_ptr[row] and row_ptr[row + 1] there and then (lazily: no per-row state
//                 besides `run`), its slot is row_ptr[row] + run + popcount(the group's ballot bits on lower lanes), and it
//                 stores its column and score with two plain vector stores.
//   end:          count: lane 0 of every group stores `run` -- one store per row, rows without a hit included, so the result
//                 needs no zeroing.  No atomics, no LDS beyond the stage buffers.
// Order.  A workgroup walks its column tiles in ascending order (no per-workgroup rotation), and inside a tile the column rises
// with the lane index inside the row group, in both accumulator layouts:
//   32x32 (f32 / bf16x3): register v of accumulator t in lane (r, h) is row acc_row(v, h), column tcol0 + 32 t + r; the group is
//                  the 32 lanes of one h, r is the lane index inside it, and t = 0 (columns 0..31) is taken before t = 1 (32..63);
//   16x16x32 (bf16 / f16): element i of accumulator rt in lane (c16, g4) is row 16 rt + 4 g4 + i, column tcol0 + 16 ct + c16; the
//                  group is the 16 lanes of one g4, c16 is the lane index inside it, and the sub-tiles ct = 0..3 are taken in turn.
// So the hits of a row land in ascending column order and the whole output is canonical CSR: the order torch.nonzero gives on
// the dense [L, Nh, Nt] mask.  Nothing depends on timing: bit-identical from launch to launch.
// Bounded writes.  The fill pass writes slot s of row r only if row_ptr[r] >= 0 and row_ptr[r] <= s < row_ptr[r + 1]; a hit past
// the row's end is dropped.  A stale or wrong row_ptr (counts of another threshold) therefore gives a truncated or partly
// unwritten result, never a store outside [row_ptr[r], row_ptr[r + 1]) -- inside cols / vals as long as row_ptr's own entries are.
// All slot arithmetic is 64-bit (row_ptr int64, `run` < n_tail < 2^31 widened before the add).
// Ineligible elements (and rows past n_head) become NaN, which fails `x >= thr` for every thr, -inf included; for the same
// reason a NaN score is never selected.
// MASKED instantiations (mdg_bilinear_select_*_masked): a known-pair exclusion bitmap (pairmask.hip) on top of
// `eligible`; a set bit makes its element NaN like an ineligible one, in both passes alike, so order, bounded writes and
// determinism are those described above.
#include "sweep_reduce.h"

namespace {

struct SelectArgs {
  const float* z_head;
  TileSrc zt;
  TileSrc w;                  // W_sym (this call's labels); nrows = D
  const float* thr;           // [n_labels]
  int* row_counts;            // count pass: [n_labels, n_head]
  const long long* row_ptr;   // fill pass: [n_labels * n_head + 1]
  int* cols;                  // fill pass: [row_ptr[last]]
  float* vals;
  int64_t n_head, n_tail;
  int eligible;               // mdg_topk_eligible
};

// The kernel argument: SelectArgs itself, plus the exclusion mask in the MASKED instantiations (mdg_bilinear_select_*_masked).
template <bool MASKED> struct SelectKArgs : SelectArgs {};
template <> struct SelectKArgs<true> : SelectArgs { PairMask mask; };

// Eligibility of the element in row wrow0 + lr, column tcol0 + lc of a tile (0 <= lr, lc < 64) from the tile's 32-bit distances
// (wave-uniform, select_clamp-ed): dcr = tcol0 - wrow0, nr = n_head - wrow0, nc = n_tail - tcol0.  The same test as top-k's and
// bincount's on the 64-bit indices (col - row keeps its sign and its zero through the clamp); a lane's lr and lc differ from
// element to element by compile-time constants only.
__device__ __forceinline__ int select_clamp(int64_t x) {
  return static_cast<int>(x < -(int64_t(1) << 30) ? -(int64_t(1) << 30) : (x > (int64_t(1) << 30) ? (int64_t(1) << 30) : x));
}
__device__ __forceinline__ bool select_eligible(int mode, int lr, int lc, int dcr, int nr, int nc) {
  const int d = dcr + lc - lr;                                                          // column - row
  const bool pair = mode == MDG_TOPK_NOT_SELF ? d != 0 : d < 0;                         // (bitwise: selects, no branches)
  return (lr < nr) & (lc < nc) & ((mode == MDG_TOPK_ALL) | pair);
}

// Hit path of one accumulator register.  Must be called in wave-uniform control flow.  G lanes share the row whose row_ptr entry is
// `rp` (FILL; read by lanes with a hit only -- an ineligible element never hits, so rp[0] and rp[1] lie inside row_ptr); `run`: the
// row's hits so far.
template <int G, bool FILL>
__device__ __forceinline__ void select_take(const SelectArgs& p, unsigned& run, bool hit, float x, int col, const long long* rp, int lane) {
  constexpr unsigned GMASK = G == 32 ? 0xFFFFFFFFu : 0xFFFFu;
  const unsigned long long m = __ballot(hit);
  const int c = lane & (G - 1), base = lane & ~(G - 1);
  const unsigned mine = static_cast<unsigned>(m >> base) & GMASK;    // hits of MY row, one bit per lane of the group
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

// The two kernels below carry the sweep itself -- prologue, three-buffer LDS-DMA ring with its hand-counted waits, mask-word DMAs --
// as topk.hip, select.hip and bincount.hip each do: sharing that text between them was tried and measured 0.2 - 2.9 % slower in some
// instantiations whichever way it was spelled, so a change to the ring is made in all three files.
// ---- f32 / bf16x3: bilinear_allpairs_kernel<MODE, ROWSTATS, 8> with the selecting epilogue ---------------------------------------
// MASKED: an element is eligible when the mode allows it AND its bit of the exclusion mask is clear (it becomes NaN like every
// ineligible element).  The 64 words [row block of the wave][columns of the tile] ride with the tile: one more LDS-DMA per wave and
// tile group into a slot of the wave's own, so a group is NDMA + 1 = 5 instructions and the wait keeps 5 in flight.  Lane (r, h)
// reads words r and 32 + r of the slot (its columns for t = 0, 1); its rows are bits acc_row(v, h) of them.
template <int MODE, bool FILL, bool MASKED>
__global__ __launch_bounds__(512, 1) void bilinear_select_kernel(const SelectKArgs<MASKED> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "32x32 sweep of the fp32-grade modes");
  constexpr int NW = 8, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int64_t l = blockIdx.y;
  // LOWER: the last row block sweeps the most column tiles -- it goes first
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  const float thr = p.thr[l];

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
  unsigned run[16];                              // hits so far of row acc_row(v, h)
  const long long* const rp = p.row_ptr + (l * p.n_head + wrow0 + 4 * h);      // row acc_row(v, h): rp[(v & 3) + 8 * (v >> 2)]
#pragma unroll
  for (int v = 0; v < 16; ++v) run[v] = 0u;
  constexpr int NDMA = 32 / NW;                  // LDS-DMA instructions per wave and tile
  static_assert(NDMA == 4, "vmcnt immediate below");
  // MASKED: the wave's mask slot of stage buffer b is mslot + b * sweep_mask_stage<1>; every group of DMAs below (tile + words) is
  // issued together, so "the last group in flight" is 5 instructions instead of 4 and nothing else about the chain changes.  (The
  // fill pass's stores and row_ptr reads are issued after a group and only make a wait stricter, as before.)
  constexpr int MSTAGE = sweep_mask_stage<1>;
  const char* const mslot = smem + 3 * STAGE_BYTES + wave * PAIRMASK_SLOT;
  const unsigned* mplane = nullptr;
  if constexpr (MASKED) mplane = p.mask.words + l * p.mask.plane_stride;            // workgroup-uniform
  stage_dma<MODE>(p.zt, 0, smem, wave, lane, NW);
  if constexpr (MASKED) pairmask_dma(p.mask, mplane, wrow0 >> 5, 0, lane, lds_addr(mslot));
  stage_dma<MODE>(p.zt, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, smem + STAGE_BYTES, wave, lane, NW);
  if constexpr (MASKED) pairmask_dma(p.mask, mplane, wrow0 >> 5, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, lane, lds_addr(mslot + MSTAGE));
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    const int64_t tcol0 = static_cast<int64_t>(s) * BN;
    if constexpr (MASKED) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");       // = NDMA + 1 mask DMA: group s landed, group s+1 stays in flight
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // = NDMA: tile s landed, tile s+1 stays in flight
    __builtin_amdgcn_s_barrier();      // tile s landed for every wave; every wave finished reading tile s-1
    const int nxt2 = cur == 0 ? 2 : cur - 1;                           // (cur + 2) % 3 = buffer of tile s-1
    const int s2 = s + 2 < nst ? s + 2 : nst - 1;                      // past the end: a copy nobody consumes
    stage_dma<MODE>(p.zt, static_cast<int64_t>(s2) * BN, smem + nxt2 * STAGE_BYTES, wave, lane, NW);
    if constexpr (MASKED) pairmask_dma(p.mask, mplane, wrow0 >> 5, static_cast<int64_t>(s2) * BN, lane, lds_addr(mslot + nxt2 * MSTAGE));
    const char* lds = smem + cur * STAGE_BYTES;
    const char* const mcur = mslot + cur * MSTAGE;                     // this wave's words of tile s (its own DMA: landed with the wait above)
    cur = cur == 2 ? 0 : cur + 1;
    if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 31) continue;       // wave-uniform: no column of this tile is below any of my rows
    unsigned w0 = 0u, w1 = 0u;                                          // MASKED: read ahead of the MFMAs, whose issue hides the LDS latency
    if constexpr (MASKED) { w0 = pairmask_word(mcur, r); w1 = pairmask_word(mcur, 32 + r); }
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    compute_tile<MODE>(At, lds, r, h, acc);
    // whole tile eligible for every row of the wave (wave-uniform): no per-element masking
    const bool plain = tcol0 + BN <= p.n_tail && wrow0 + 32 <= p.n_head &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
    if (!plain) {
      const int dcr = select_clamp(tcol0 - wrow0), nr = select_clamp(p.n_head - wrow0), nc = select_clamp(p.n_tail - tcol0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          acc[t][v] = select_eligible(mode, acc_row(v, h), 32 * t + r, dcr, nr, nc) ? acc[t][v] : __builtin_nanf("");
    }
    if constexpr (MASKED) {
      if (__ballot((w0 | w1) != 0u) != 0) {                            // wave-uniform: a tile without a known pair costs two reads and this ballot
        const unsigned mw[2] = {w0 >> (4 * h), w1 >> (4 * h)};         // bit acc_row(v, 0) of mw[t] <-> row acc_row(v, h)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[t][v] = pairmask_nan_if(acc[t][v], mw[t], acc_row(v, 0));
      }
    }
    bool any = false;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) any |= acc[t][v] >= thr;
    if (__ballot(any) != 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v)
#pragma unroll
        for (int t = 0; t < 2; ++t)                                    // columns 0..31 of the tile, then 32..63
          select_take<32, FILL>(p, run[v], acc[t][v] >= thr, acc[t][v], static_cast<int>(tcol0) + 32 * t + r,
                                rp + ((v & 3) + 8 * (v >> 2)), lane);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (!FILL) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = wrow0 + acc_row(v, h);
      if (r == 0 && row < p.n_head) p.row_counts[l * p.n_head + row] = static_cast<int>(run[v]);
    }
  }
}

// ---- bf16 / f16: bilinear_rowstats16_kernel (v_mfma_f32_16x16x32, 64 rows per wave) with the selecting epilogue -----------------
// MASKED: as above; the wave's 64 rows are two row blocks of the mask, so two mask DMAs per tile group (2 + 2 = 4 in flight) and
// two slots: lane (c16, g4) reads word 16 ct + c16 of each for sub-tile ct; row 16 rt + 4 g4 + i is bit 16 (rt & 1) + 4 g4 + i
// of the word of row block rt >> 1.
template <int MODE, bool FILL, bool MASKED>
__global__ __launch_bounds__(512, 1) void bilinear_select16_kernel(const SelectKArgs<MASKED> p) {
  static_assert(kSingle16<MODE>, "one rounded 16-bit product per k step");
  constexpr int NW = 8, BM = 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, c16 = lane & 15, g4 = lane >> 4;
  const int64_t l = blockIdx.y;
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
  const float thr = p.thr[l];
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
  unsigned run[16];                                  // hits so far of row 16 rt + 4 g4 + i: counter 4 rt + i
  const long long* const rp = p.row_ptr + (l * p.n_head + wrow0 + 4 * g4);     // row 16 rt + 4 g4 + i: rp[16 * rt + i]
#pragma unroll
  for (int q = 0; q < 16; ++q) run[q] = 0u;
  constexpr int MSTAGE = sweep_mask_stage<2>;
  const char* const mslot = smem + 3 * STAGE_BYTES + wave * 2 * PAIRMASK_SLOT;
  const unsigned* mplane = nullptr;
  if constexpr (MASKED) mplane = p.mask.words + l * p.mask.plane_stride;            // workgroup-uniform
  auto mask_dma = [&](int64_t col0, const char* slot) {               // the group's two mask DMAs: row blocks wrow0 / 32 and + 1
    if constexpr (MASKED) {
      pairmask_dma(p.mask, mplane, wrow0 >> 5, col0, lane, lds_addr(slot));
      pairmask_dma(p.mask, mplane, (wrow0 >> 5) + 1, col0, lane, lds_addr(slot + PAIRMASK_SLOT));
    }
  };
  stage_dma<MODE>(p.zt, 0, smem, wave, lane, NW);
  if constexpr (MASKED) mask_dma(0, mslot);
  stage_dma<MODE>(p.zt, static_cast<int64_t>(1 < nst ? 1 : 0) * BN, smem + STAGE_BYTES, wave, lane, NW);
  if constexpr (MASKED) mask_dma(static_cast<int64_t>(1 < nst ? 1 : 0) * BN, mslot + MSTAGE);
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    const int64_t tcol0 = static_cast<int64_t>(s) * BN;
    if constexpr (MASKED) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // = 2 tile + 2 mask DMAs per group: group s landed, group s+1 stays in flight
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");           // = LDS-DMA instructions per wave and tile: tile s landed, tile s+1 stays in flight
    __builtin_amdgcn_s_barrier();
    const int nxt2 = cur == 0 ? 2 : cur - 1;
    const int s2 = s + 2 < nst ? s + 2 : nst - 1;
    stage_dma<MODE>(p.zt, static_cast<int64_t>(s2) * BN, smem + nxt2 * STAGE_BYTES, wave, lane, NW);
    if constexpr (MASKED) mask_dma(static_cast<int64_t>(s2) * BN, mslot + nxt2 * MSTAGE);
    const char* lds = smem + cur * STAGE_BYTES;
    const char* const mcur = mslot + cur * MSTAGE;                     // this wave's words of tile s (its own DMAs: landed with the wait above)
    cur = cur == 2 ? 0 : cur + 1;
    if (mode == MDG_TOPK_LOWER && tcol0 >= wrow0 + 63) continue;       // wave-uniform: nothing below the diagonal for my rows
    const bool plain = tcol0 + BN <= p.n_tail && wrow0 + 64 <= p.n_head &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 63));
    unsigned mwd[4][2];                                                // MASKED: the tile's eight words, read ahead of the MFMAs that hide the LDS latency
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      mwd[ct][0] = mwd[ct][1] = 0u;
      if constexpr (MASKED) { mwd[ct][0] = pairmask_word(mcur, 16 * ct + c16); mwd[ct][1] = pairmask_word(mcur + PAIRMASK_SLOT, 16 * ct + c16); }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {                                   // 16-column sub-tiles in ascending order
      f32x4v acc[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(16 * ct + c16, 4 * ks + g4));
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = mma16x16<MODE>(A16[rt][ks], b, acc[rt]);
      }
      const int col = static_cast<int>(tcol0) + 16 * ct + c16;
      if (!plain) {
        const int dcr = select_clamp(tcol0 - wrow0), nr = select_clamp(p.n_head - wrow0), nc = select_clamp(p.n_tail - tcol0);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[rt][i] = select_eligible(mode, 16 * rt + 4 * g4 + i, 16 * ct + c16, dcr, nr, nc) ? acc[rt][i] : __builtin_nanf("");
      }
      if constexpr (MASKED) {
        if (__ballot((mwd[ct][0] | mwd[ct][1]) != 0u) != 0) {           // wave-uniform, per 16-column sub-tile
          const unsigned mw[2] = {mwd[ct][0] >> (4 * g4), mwd[ct][1] >> (4 * g4)};
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[rt][i] = pairmask_nan_if(acc[rt][i], mw[rt >> 1], 16 * (rt & 1) + i);
        }
      }
      bool any = false;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) any |= acc[rt][i] >= thr;
      if (__ballot(any) != 0) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            select_take<16, FILL>(p, run[4 * rt + i], acc[rt][i] >= thr, acc[rt][i], col, rp + (16 * rt + i), lane);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (!FILL) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = wrow0 + 16 * rt + 4 * g4 + i;
        if (c16 == 0 && row < p.n_head) p.row_counts[l * p.n_head + row] = static_cast<int>(run[4 * rt + i]);
      }
  }
}

template <int MODE, bool FILL, bool MASKED>
int launch_select(SelectKArgs<MASKED>& a, const float* z_tail, const float* w_sym, int64_t n_labels, char* ws, hipStream_t st, const char* fn) {
  make_head_images<MODE>(a.zt, a.w, z_tail, w_sym, a.n_tail, n_labels, ws, st);
  MDG_CHECK_LAUNCH(fn);
  if constexpr (kSingle16<MODE>) return sweep_launch<MASKED, 2>(bilinear_select16_kernel<MODE, FILL, MASKED>, a, n_labels, 0, st, fn);
  else return sweep_launch<MASKED, 1>(bilinear_select_kernel<MODE, FILL, MASKED>, a, n_labels, 0, st, fn);
}

// The checks both entry points share; `outputs`: none of the pass's own pointers is null.  Returns MDG_OK with *launch = false
// when there is nothing to do.
int select_check(const char* fn, const float* z_head, const float* z_tail, const float* w_sym, const float* thr, bool outputs, int64_t n_head,
                 int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible, void* workspace, size_t workspace_bytes,
                 bool* launch) {
  *launch = false;
  const int rc = sweep_check_sizes(fn, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail,
                "%s: eligible NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)", fn, (long long)n_head,
                (long long)n_tail);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "%s: n_tail %lld does not fit the int32 column indices", fn, (long long)n_tail);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(n_tail >= 1, "%s: n_tail must be at least 1", fn);
  const int orc = sweep_check_operands(fn, z_head, z_tail, w_sym, thr && outputs, n_tail, n_labels, precision, workspace, workspace_bytes);
  if (orc != MDG_OK) return orc;
  *launch = true;
  return MDG_OK;
}

template <bool FILL, bool MASKED>
int select_dispatch(SelectKArgs<MASKED>& a, const float* z_tail, const float* w_sym, int64_t n_labels, int precision, void* workspace, void* stream,
                    const char* fn) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  switch (precision) {
    case MDG_PREC_F32: return launch_select<MDG_PREC_F32, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
    case MDG_PREC_BF16X3: return launch_select<MDG_PREC_BF16X3, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
    case MDG_PREC_BF16: return launch_select<MDG_PREC_BF16, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
    default: return launch_select<MDG_PREC_F16, FILL, MASKED>(a, z_tail, w_sym, n_labels, ws, st, fn);
  }
}

}  // namespace

extern "C" size_t mdg_bilinear_select_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision) {
  (void)n_head;
  return head_images_workspace_bytes(n_tail, n_labels, D_, precision);
}

namespace {

template <bool MASKED>
int select_count_run(const char* fn, const float* z_head, const float* z_tail, const float* w_sym, const float* thr, int32_t* row_counts,
                     int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible, void* workspace,
                     size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride) {
  bool launch;
  const int rc = select_check(fn, z_head, z_tail, w_sym, thr, row_counts != nullptr, n_head, n_tail, n_labels, D_, precision, eligible,
                              workspace, workspace_bytes, &launch);
  if (rc != MDG_OK || !launch) return rc;
  SelectKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args(fn, a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  a.z_head = z_head;
  a.thr = thr;
  a.row_counts = row_counts;
  a.n_head = n_head; a.n_tail = n_tail;
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  return select_dispatch<false, MASKED>(a, z_tail, w_sym, n_labels, precision, workspace, stream, fn);
}

template <bool MASKED>
int select_fill_run(const char* fn, const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const int64_t* row_ptr,
                    int32_t* cols, float* vals, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible,
                    void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride) {
  bool launch;
  const int rc = select_check(fn, z_head, z_tail, w_sym, thr, row_ptr && cols && vals, n_head, n_tail, n_labels, D_, precision, eligible,
                              workspace, workspace_bytes, &launch);
  if (rc != MDG_OK || !launch) return rc;
  SelectKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args(fn, a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  a.z_head = z_head;
  a.thr = thr;
  a.row_ptr = reinterpret_cast<const long long*>(row_ptr);
  a.cols = cols;
  a.vals = vals;
  a.n_head = n_head; a.n_tail = n_tail;
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  return select_dispatch<true, MASKED>(a, z_tail, w_sym, n_labels, precision, workspace, stream, fn);
}

}  // namespace

extern "C" int mdg_bilinear_select_count(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, int32_t* row_counts,
                                         int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int eligible,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return select_count_run<false>("mdg_bilinear_select_count", z_head, z_tail, w_sym, thr, row_counts, n_head, n_tail, n_labels, D_, precision,
                                 eligible, workspace, workspace_bytes, stream, nullptr, 0);
}

extern "C" int mdg_bilinear_select_fill(const float* z_head, const float* z_tail, const float* w_sym, const float* thr, const int64_t* row_ptr,
                                        int32_t* cols, float* vals, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_,
                                        int precision, int eligible, void* workspace, size_t workspace_bytes, void* stream) {
  return select_fill_run<false>("mdg_bilinear_select_fill", z_head, z_tail, w_sym, thr, row_ptr, cols, vals, n_head, n_tail, n_labels, D_,
                                precision, eligible, workspace, workspace_bytes, stream, nullptr, 0);
}

extern "C" int mdg_bilinear_select_count_masked(const float* z_head, const float* z_tail, const float* w_sym, const float* thr,
                                                int32_t* row_counts, int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision,
                                                int eligible, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask,
                                                int64_t plane_stride) {
  if (!mask)
    return select_count_run<false>("mdg_bilinear_select_count_masked", z_head, z_tail, w_sym, thr, row_counts, n_head, n_tail, n_labels, D_,
                                   precision, eligible, workspace, workspace_bytes, stream, nullptr, 0);
  return select_count_run<true>("mdg_bilinear_select_count_masked", z_head, z_tail, w_sym, thr, row_counts, n_head, n_tail, n_labels, D_,
                                precision, eligible, workspace, workspace_bytes, stream, mask, plane_stride);
}

extern "C" int mdg_bilinear_select_fill_masked(const float* z_head, const float* z_tail, const float* w_sym, const float* thr,
                                               const int64_t* row_ptr, int32_t* cols, float* vals, int64_t n_head, int64_t n_tail,
                                               int64_t n_labels, int64_t D_, int precision, int eligible, void* workspace, size_t workspace_bytes,
                                               void* stream, const uint32_t* mask, int64_t plane_stride) {
  if (!mask)
    return select_fill_run<false>("mdg_bilinear_select_fill_masked", z_head, z_tail, w_sym, thr, row_ptr, cols, vals, n_head, n_tail, n_labels,
                                  D_, precision, eligible, workspace, workspace_bytes, stream, nullptr, 0);
  return select_fill_run<true>("mdg_bilinear_select_fill_masked", z_head, z_tail, w_sym, thr, row_ptr, cols, vals, n_head, n_tail, n_labels, D_,
                               precision, eligible, workspace, workspace_bytes, stream, mask, plane_stride);
}
