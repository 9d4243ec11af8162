// Per-row top-k of the all-pairs bilinear sweep for gfx950 (mdg_bilinear_topk).
//
//   for every outcome l and head row i: the k largest S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j] over the ELIGIBLE tail
//   columns j, with their column indices, ordered by (score descending, column ascending).
//
// The fourth, reducing product of the head: nothing of [L,N,N] is materialised.  The score arithmetic is the sweep's own -- the two
// kernels below are the row-statistics sweeps of bilinear.hip (same prologue, same staging, same MFMA sequence per accumulator
// element) with the sum / max epilogue replaced, so every score equals the general sweep's bit for bit.  The launch side is shared
// with select.hip and bincount.hip (sweep_reduce.h).
//
// Where the lists live: in registers.  The accumulator layouts give every head row to ONE wave, G lanes per row (G = 32 on
// the 32x32 MFMA, 16 on 16x16x32), each lane holding one column.  Those same G lanes hold the row's sorted list: entry e sits
// in slot e / G of lane e % G (32 entries per row: 16 rows x 1 slot, or 16 rows x 2 slots, per lane).  Per row and lane
// there is also the threshold `thr` = the row's current k-th value (-inf while the list is short), uniform over the G lanes.
//   pass-through: one v_cmp per accumulator element (x > thr), OR-ed into one ballot per tile: the common case costs what
//                 ROWSTATS' add + max costs;
//   insert:       per row with a candidate (wave-uniform branch): the candidates of the row are taken one by one (lowest lane
//                 first); position p = number of entries that beat it (a ballot + popcount per slot), entries behind p move
//                 one lane up (ds_bpermute), lane p takes it, thr is re-read from entry k - 1.  No memory traffic.  A score
//                 passes the threshold about k ln(Nt / k) times per row; the two rows of a register (one per lane group) are
//                 served together, the 16 registers one after the other: this path is what the epilogue costs.
// Tie rule: the sweep visits the column tiles in ascending order (no per-workgroup rotation here), so a later score equal to
// the threshold has a larger column than every kept entry and rightly fails `x > thr`; inside a tile the insert compares the
// full key (score, then column).  No atomics, no memory traffic besides the final k stores per row: bit-reproducible.
// NaN scores never pass `x > thr` and are never kept (scores are finite by contract).
//
// Registers: the workgroup may use 256 per lane (launch bound 1), see DESIGN.md 4m for the measured budget of every instantiation.
//
// MASKED instantiations (mdg_bilinear_topk_masked): a known-pair exclusion bitmap (pairmask.hip) on top of
// `eligible`; a set bit makes its element -inf like an ineligible one, so everything above holds for what remains.
#include "sweep_reduce.h"
#include "topk_list.h"         // TOPK_MAX_K, topk_insert: shared with knn.hip

namespace {

struct TopkArgs {
  const float* z_head;
  TileSrc zt;
  TileSrc w;            // W_sym (this call's labels); nrows = D
  float* vals;          // [n_labels, n_head, k]
  int* idx;             // [n_labels, n_head, k]
  int64_t n_head, n_tail;
  int k;
  int eligible;         // mdg_topk_eligible
};

// The kernel argument: TopkArgs itself, plus the exclusion mask in the MASKED instantiations (mdg_bilinear_topk_masked).
template <bool MASKED> struct TopkKArgs : TopkArgs {};
template <> struct TopkKArgs<true> : TopkArgs { PairMask mask; };

__device__ __forceinline__ bool topk_eligible(int mode, int64_t row, int64_t col, int64_t n_tail) {
  return col < n_tail && (mode == MDG_TOPK_ALL || (mode == MDG_TOPK_NOT_SELF ? col != row : col < row));
}

// The two kernels below carry the sweep itself -- prologue, three-buffer LDS-DMA ring with its hand-counted waits, mask-word DMAs --
// as topk.hip, select.hip and bincount.hip each do: sharing that text between them was tried and measured 0.2 - 2.9 % slower in some
// instantiations whichever way it was spelled, so a change to the ring is made in all three files.
// ---- f32 / bf16x3: bilinear_allpairs_kernel<MODE, ROWSTATS, 8> with the list epilogue ---------------------------------------
// MASKED: an element is eligible when the mode allows it AND its bit of the exclusion mask is clear.  The 64 words
// [row block of the wave][columns of the tile] ride with the tile: one more LDS-DMA per wave and tile group, into a slot of the
// wave's own behind the stage buffers, so the group is NDMA + 1 = 5 instructions and the wait below keeps 5 in flight.  Lane
// (r, h) then reads words r and 32 + r of the slot (its columns for t = 0, 1); its rows are bits acc_row(v, h) of them.
template <int MODE, bool MASKED>
__global__ __launch_bounds__(512, 1) void bilinear_topk_kernel(const TopkKArgs<MASKED> p) {
  static_assert(MODE == MDG_PREC_F32 || MODE == MDG_PREC_BF16X3, "32x32 sweep of the fp32-grade modes");
  constexpr int NW = 8, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int64_t l = blockIdx.y;
  // LOWER: the last row block sweeps the most column tiles -- it goes first
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;

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
  const int mode = p.eligible, k = p.k;
  float lv[16][1], thr[16];
  int li[16][1];
#pragma unroll
  for (int v = 0; v < 16; ++v) { lv[v][0] = -INFINITY; li[v][0] = -1; thr[v] = -INFINITY; }
  constexpr int NDMA = 32 / NW;                  // LDS-DMA instructions per wave and tile
  static_assert(NDMA == 4, "vmcnt immediate below");
  // MASKED: the wave's mask slot of stage buffer b is mslot + b * sweep_mask_stage<1>; every group of DMAs below (tile + words)
  // is issued together, so "the last group in flight" is 5 instructions instead of 4 and nothing else about the chain changes.
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
    const bool plain = tcol0 + BN <= p.n_tail &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 31));
    if (!plain) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          acc[t][v] = topk_eligible(mode, wrow0 + acc_row(v, h), tcol0 + 32 * t + r, p.n_tail) ? acc[t][v] : -INFINITY;
    }
    if constexpr (MASKED) {
      if (__ballot((w0 | w1) != 0u) != 0) {                            // wave-uniform: a tile without a known pair costs two reads and this ballot
        const unsigned mw[2] = {w0 >> (4 * h), w1 >> (4 * h)};         // bit acc_row(v, 0) of mw[t] <-> row acc_row(v, h)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[t][v] = (mw[t] >> acc_row(v, 0)) & 1u ? -INFINITY : acc[t][v];
      }
    }
    bool any = false;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) any |= acc[t][v] > thr[v];
    if (__ballot(any) != 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          topk_insert<32>(lv[v], li[v], thr[v], acc[t][v] > thr[v], acc[t][v], static_cast<int>(tcol0) + 32 * t + r, lane, k);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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

// ---- bf16 / f16: bilinear_rowstats16_kernel (v_mfma_f32_16x16x32, 64 rows per wave) with the list epilogue -----------------
// MASKED: as above; the wave's 64 rows are two row blocks of the mask, so two mask DMAs per tile group (2 + 2 = 4 in flight) and
// two slots: lane (c16, g4) reads word 16 ct + c16 of each for sub-tile ct; row 16 rt + 4 g4 + i is bit 16 (rt & 1) + 4 g4 + i
// of the word of row block rt >> 1.
template <int MODE, bool MASKED>
__global__ __launch_bounds__(512, 1) void bilinear_topk16_kernel(const TopkKArgs<MASKED> p) {
  static_assert(kSingle16<MODE>, "one rounded 16-bit product per k step");
  constexpr int NW = 8, BM = 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, c16 = lane & 15, g4 = lane >> 4;
  const int64_t l = blockIdx.y;
  const int64_t rbk = p.eligible == MDG_TOPK_LOWER ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int64_t row0 = rbk * BM;
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
  const int mode = p.eligible, k = p.k;
  float lv[16][2], thr[16];                          // row 16 rt + 4 g4 + i is list 4 rt + i
  int li[16][2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { lv[q][0] = lv[q][1] = -INFINITY; li[q][0] = li[q][1] = -1; thr[q] = -INFINITY; }
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
    const bool plain = tcol0 + BN <= p.n_tail &&
                       (mode == MDG_TOPK_ALL || tcol0 + BN <= wrow0 || (mode == MDG_TOPK_NOT_SELF && tcol0 > wrow0 + 63));
    unsigned mwd[4][2];                                                // MASKED: the tile's eight words, read ahead of the MFMAs that hide the LDS latency
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      mwd[ct][0] = mwd[ct][1] = 0u;
      if constexpr (MASKED) { mwd[ct][0] = pairmask_word(mcur, 16 * ct + c16); mwd[ct][1] = pairmask_word(mcur + PAIRMASK_SLOT, 16 * ct + c16); }
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
      const int col = static_cast<int>(tcol0) + 16 * ct + c16;
      if (!plain) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[rt][i] = topk_eligible(mode, wrow0 + 16 * rt + 4 * g4 + i, col, p.n_tail) ? acc[rt][i] : -INFINITY;
      }
      if constexpr (MASKED) {
        if (__ballot((mwd[ct][0] | mwd[ct][1]) != 0u) != 0) {           // wave-uniform, per 16-column sub-tile
          const unsigned mw[2] = {mwd[ct][0] >> (4 * g4), mwd[ct][1] >> (4 * g4)};
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[rt][i] = (mw[rt >> 1] >> (16 * (rt & 1) + i)) & 1u ? -INFINITY : acc[rt][i];
        }
      }
      bool any = false;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) any |= acc[rt][i] > thr[4 * rt + i];
      if (__ballot(any) != 0) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            topk_insert<16>(lv[4 * rt + i], li[4 * rt + i], thr[4 * rt + i], acc[rt][i] > thr[4 * rt + i], acc[rt][i], col, lane, k);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = wrow0 + 16 * rt + 4 * g4 + i;
      if (row < p.n_head) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          const int e = 16 * sl + c16;
          if (e < k) {
            const int64_t o = (l * p.n_head + row) * k + e;
            p.vals[o] = lv[4 * rt + i][sl];
            p.idx[o] = li[4 * rt + i][sl];
          }
        }
      }
    }
}

template <int MODE, bool MASKED>
int launch_topk(TopkKArgs<MASKED>& a, const float* z_tail, const float* w_sym, int64_t n_labels, char* ws, hipStream_t st) {
  make_head_images<MODE>(a.zt, a.w, z_tail, w_sym, a.n_tail, n_labels, ws, st);
  MDG_CHECK_LAUNCH("mdg_bilinear_topk(operand images)");
  if constexpr (kSingle16<MODE>) return sweep_launch<MASKED, 2>(bilinear_topk16_kernel<MODE, MASKED>, a, n_labels, 0, st, "mdg_bilinear_topk");
  else return sweep_launch<MASKED, 1>(bilinear_topk_kernel<MODE, MASKED>, a, n_labels, 0, st, "mdg_bilinear_topk");
}

}  // namespace

extern "C" int mdg_bilinear_topk_max_k(void) { return TOPK_MAX_K; }

extern "C" size_t mdg_bilinear_topk_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int k) {
  (void)n_head; (void)k;
  return head_images_workspace_bytes(n_tail, n_labels, D_, precision);
}

namespace {

// Both entry points; MASKED: `mask` is not null.
template <bool MASKED>
int topk_run(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx, int64_t n_head, int64_t n_tail,
             int64_t n_labels, int64_t D_, int precision, int k, int eligible, void* workspace, size_t workspace_bytes, void* stream,
             const uint32_t* mask, int64_t plane_stride) {
  const char* const fn = "mdg_bilinear_topk";
  const int rc = sweep_check_sizes(fn, n_head, n_tail, n_labels, D_, precision, eligible);
  if (rc != MDG_OK) return rc;
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "mdg_bilinear_topk: k must be in 1..%d (got %d)", TOPK_MAX_K, k);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "mdg_bilinear_topk: n_tail %lld does not fit the int32 column indices", (long long)n_tail);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail,
                "mdg_bilinear_topk: NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)", (long long)n_head, (long long)n_tail);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(n_tail >= 1, "mdg_bilinear_topk: n_tail must be at least 1");
  const int orc = sweep_check_operands(fn, z_head, z_tail, w_sym, vals && idx, n_tail, n_labels, precision, workspace, workspace_bytes);
  if (orc != MDG_OK) return orc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  TopkKArgs<MASKED> a{};
  if constexpr (MASKED) {
    const int mrc = sweep_mask_args("mdg_bilinear_topk_masked", a.mask, mask, plane_stride, n_head, n_tail);
    if (mrc != MDG_OK) return mrc;
  }
  a.z_head = z_head;
  a.vals = vals;
  a.idx = idx;
  a.n_head = n_head; a.n_tail = n_tail;
  a.k = k;
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  char* ws = static_cast<char*>(workspace);
  switch (precision) {
    case MDG_PREC_F32: return launch_topk<MDG_PREC_F32, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
    case MDG_PREC_BF16X3: return launch_topk<MDG_PREC_BF16X3, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
    case MDG_PREC_BF16: return launch_topk<MDG_PREC_BF16, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
    default: return launch_topk<MDG_PREC_F16, MASKED>(a, z_tail, w_sym, n_labels, ws, st);
  }
}

}  // namespace

extern "C" int mdg_bilinear_topk(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx, int64_t n_head,
                                 int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int k, int eligible, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return topk_run<false>(z_head, z_tail, w_sym, vals, idx, n_head, n_tail, n_labels, D_, precision, k, eligible, workspace, workspace_bytes,
                         stream, nullptr, 0);
}

extern "C" int mdg_bilinear_topk_masked(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx,
                                        int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int k, int eligible,
                                        void* workspace, size_t workspace_bytes, void* stream, const uint32_t* mask, int64_t plane_stride) {
  if (!mask)
    return topk_run<false>(z_head, z_tail, w_sym, vals, idx, n_head, n_tail, n_labels, D_, precision, k, eligible, workspace, workspace_bytes,
                           stream, nullptr, 0);
  return topk_run<true>(z_head, z_tail, w_sym, vals, idx, n_head, n_tail, n_labels, D_, precision, k, eligible, workspace, workspace_bytes, stream,
                        mask, plane_stride);
}
