// Per-row top-k of the all-pairs bilinear sweep for gfx950 (mdg_bilinear_topk).
//
//   for every outcome l and head row i: the k largest S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j] over the ELIGIBLE tail
//   columns j, with their column indices, ordered by (score descending, column ascending).
//
// The fourth, reducing product of the head: nothing of [L,N,N] is materialised.  The score arithmetic is the sweep's own --
// the two kernels below are the row-statistics sweeps of bilinear.hip (same prologue, same staging, same MFMA sequence per
// accumulator element: `bilinear_allpairs_kernel<MODE, ROWSTATS, 8>` for f32 / bf16x3, `bilinear_rowstats16_kernel` for the
// single-product 16-bit modes) with the sum / max epilogue replaced, so every score equals the general sweep's bit for bit.
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
// LDS: the three stage buffers of the row-statistics sweeps (96 KB, one workgroup per CU -- as ROWSTATS); registers: the
// workgroup may use 256 per lane (launch bound 1), see DESIGN.md 4m for the measured budget of every instantiation.
//
// MASKED instantiations (mdg_bilinear_topk_masked): a known-pair exclusion bitmap (pairmask.hip) on top of
// `eligible`; a set bit makes its element -inf like an ineligible one, so everything above holds for what remains.  The words of a
// tile reach LDS by one or two more LDS-DMAs in the tile's group (pairmask.h); the MASKED = false kernels are what they were.
#include "pairmask.h"
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

// LDS of a MASKED sweep behind the three stage buffers: per stage buffer and wave, NMW slots of 256 bytes -- the mask words of the
// wave's row block(s) for the 64 columns of that buffer's tile (pairmask.h).
template <int NMW> constexpr int topk_mask_stage = 8 * NMW * PAIRMASK_SLOT;
template <bool MASKED, int NMW> constexpr int topk_lds_bytes = 3 * STAGE_BYTES + (MASKED ? 3 * topk_mask_stage<NMW> : 0);

__device__ __forceinline__ bool topk_eligible(int mode, int64_t row, int64_t col, int64_t n_tail) {
  return col < n_tail && (mode == MDG_TOPK_ALL || (mode == MDG_TOPK_NOT_SELF ? col != row : col < row));
}

// column tiles a workgroup with head rows [row0, row0 + BM) has to visit: LOWER needs columns j <= last row - 1 only
__device__ __forceinline__ int topk_tiles(const TopkArgs& p, int64_t row0, int BM) {
  const int nst = static_cast<int>((p.n_tail + BN - 1) / BN);
  if (p.eligible != MDG_TOPK_LOWER) return nst;
  const int64_t last = (row0 + BM < p.n_head ? row0 + BM : p.n_head) - 1;      // columns [0, last) are eligible for some row
  const int need = static_cast<int>((last + BN - 1) / BN);
  return need < 1 ? 1 : (need < nst ? need : nst);
}

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
  const int nst = topk_tiles(p, row0, BM);
  const int64_t wrow0 = row0 + wave * 32;        // this wave's rows: wrow0 .. wrow0 + 31
  const int mode = p.eligible, k = p.k;
  float lv[16][1], thr[16];
  int li[16][1];
#pragma unroll
  for (int v = 0; v < 16; ++v) { lv[v][0] = -INFINITY; li[v][0] = -1; thr[v] = -INFINITY; }
  constexpr int NDMA = 32 / NW;                  // LDS-DMA instructions per wave and tile
  static_assert(NDMA == 4, "vmcnt immediate below");
  // MASKED: the wave's mask slot of stage buffer b is mslot + b * topk_mask_stage<1>; every group of DMAs below (tile + words)
  // is issued together, so "the last group in flight" is 5 instructions instead of 4 and nothing else about the chain changes.
  constexpr int MSTAGE = topk_mask_stage<1>;
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
typedef __attribute__((ext_vector_type(4))) float f32x4v;

template <int MODE>
__device__ __forceinline__ f32x4v topk_mma16x16(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
  if constexpr (MODE == MDG_PREC_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

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
  const int nst = topk_tiles(p, row0, BM);
  const int64_t wrow0 = row0 + wave * 64;            // this wave's rows: wrow0 .. wrow0 + 63
  const int mode = p.eligible, k = p.k;
  float lv[16][2], thr[16];                          // row 16 rt + 4 g4 + i is list 4 rt + i
  int li[16][2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { lv[q][0] = lv[q][1] = -INFINITY; li[q][0] = li[q][1] = -1; thr[q] = -INFINITY; }
  constexpr int MSTAGE = topk_mask_stage<2>;
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
        for (int rt = 0; rt < 4; ++rt) acc[rt] = topk_mma16x16<MODE>(A16[rt][ks], b, acc[rt]);
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

// ---- pre-pass: the 16-bit operand images of z_tail and W_sym (the images mdg_bilinear_allpairs makes) ----------------------
template <int MODE>
__global__ void topk_images_kernel(const float* __restrict__ x, __bf16* __restrict__ hi, __bf16* __restrict__ lo, int64_t n4) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  const float f[4] = {v.x, v.y, v.z, v.w};
  if constexpr (MODE == MDG_PREC_F16) {
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    f16x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = static_cast<_Float16>(f[c]);
    reinterpret_cast<f16x4*>(hi)[i] = o;
  } else {
    bf16x4 hv, lw;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      __bf16 a, b;
      mdg_split_bf16(f[c], a, b);
      hv[c] = a;
      lw[c] = b;
    }
    reinterpret_cast<bf16x4*>(hi)[i] = hv;
    if constexpr (MODE == MDG_PREC_BF16X3) reinterpret_cast<bf16x4*>(lo)[i] = lw;
  }
}

inline size_t topk_align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

template <int MODE, bool MASKED>
int launch_topk(TopkKArgs<MASKED>& a, const float* z_tail, const float* w_sym, int64_t n_labels, char* ws, hipStream_t st) {
  if constexpr (MODE == MDG_PREC_F32) {
    a.zt.f32 = z_tail;
    a.w.f32 = w_sym;
  } else {
    const size_t zb = topk_align256(static_cast<size_t>(a.n_tail) * D * 2), wb = topk_align256(static_cast<size_t>(n_labels) * D * D * 2);
    const bool x3 = MODE == MDG_PREC_BF16X3;
    __bf16* zhi = reinterpret_cast<__bf16*>(ws);
    __bf16* whi = reinterpret_cast<__bf16*>(ws + zb);
    __bf16* zlo = x3 ? reinterpret_cast<__bf16*>(ws + zb + wb) : nullptr;
    __bf16* wlo = x3 ? reinterpret_cast<__bf16*>(ws + 2 * zb + wb) : nullptr;
    const int64_t z4 = a.n_tail * D / 4, w4 = n_labels * D * D / 4;
    hipLaunchKernelGGL(topk_images_kernel<MODE>, dim3(static_cast<unsigned>(mdg_cdiv(z4, 256))), dim3(256), 0, st, z_tail, zhi, zlo, z4);
    hipLaunchKernelGGL(topk_images_kernel<MODE>, dim3(static_cast<unsigned>(mdg_cdiv(w4, 256))), dim3(256), 0, st, w_sym, whi, wlo, w4);
    MDG_CHECK_LAUNCH("mdg_bilinear_topk(operand images)");
    a.zt.hi = zhi; a.zt.lo = zlo;
    a.w.hi = whi; a.w.lo = wlo;
  }
  if constexpr (MASKED) {                         // more dynamic LDS than the unmasked sweeps use: raise the kernel's limit once
    static bool attr_done = false;
    if (!attr_done) {
      if constexpr (kSingle16<MODE>)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bilinear_topk16_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, topk_lds_bytes<true, 2>);
      else
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bilinear_topk_kernel<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, topk_lds_bytes<true, 1>);
      attr_done = true;
    }
  }
  if constexpr (kSingle16<MODE>) {
    const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 512)), static_cast<unsigned>(n_labels));
    hipLaunchKernelGGL((bilinear_topk16_kernel<MODE, MASKED>), grid, dim3(512), (topk_lds_bytes<MASKED, 2>), st, a);
  } else {
    const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 256)), static_cast<unsigned>(n_labels));
    hipLaunchKernelGGL((bilinear_topk_kernel<MODE, MASKED>), grid, dim3(512), (topk_lds_bytes<MASKED, 1>), st, a);
  }
  MDG_CHECK_LAUNCH("mdg_bilinear_topk");
  return MDG_OK;
}

}  // namespace

extern "C" int mdg_bilinear_topk_max_k(void) { return TOPK_MAX_K; }

extern "C" size_t mdg_bilinear_topk_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int k) {
  (void)n_head; (void)k;
  if (precision == MDG_PREC_F32 || n_tail <= 0 || n_labels <= 0 || D_ <= 0) return 0;
  const size_t z = topk_align256(static_cast<size_t>(n_tail) * D_ * 2), w = topk_align256(static_cast<size_t>(n_labels) * D_ * D_ * 2);
  return precision == MDG_PREC_BF16X3 ? 2 * (z + w) : (z + w);
}

namespace {

// Both entry points; MASKED: `mask` is not null.
template <bool MASKED>
int topk_run(const float* z_head, const float* z_tail, const float* w_sym, float* vals, int32_t* idx, int64_t n_head, int64_t n_tail,
             int64_t n_labels, int64_t D_, int precision, int k, int eligible, void* workspace, size_t workspace_bytes, void* stream,
             const uint32_t* mask, int64_t plane_stride) {
  MDG_CHECK_ARG(D_ == D, "mdg_bilinear_topk: D must be %d (got %lld)", D, (long long)D_);
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "mdg_bilinear_topk: k must be in 1..%d (got %d)", TOPK_MAX_K, k);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "mdg_bilinear_topk: negative size");
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - BN, "mdg_bilinear_topk: n_tail %lld does not fit the int32 column indices", (long long)n_tail);
  MDG_CHECK_ARG(n_labels <= 65535, "mdg_bilinear_topk: n_labels %lld > 65535 per call", (long long)n_labels);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || eligible == MDG_TOPK_NOT_SELF || eligible == MDG_TOPK_LOWER,
                "mdg_bilinear_topk: unknown eligible mode %d", eligible);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || n_head == n_tail,
                "mdg_bilinear_topk: NOT_SELF / LOWER need one drug set against itself (n_head %lld != n_tail %lld)", (long long)n_head, (long long)n_tail);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3 || precision == MDG_PREC_BF16 || precision == MDG_PREC_F16,
                "mdg_bilinear_topk: unknown precision %d", precision);
  if (n_head == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(n_tail >= 1, "mdg_bilinear_topk: n_tail must be at least 1");
  MDG_CHECK_ARG(z_head && z_tail && w_sym && vals && idx, "mdg_bilinear_topk: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(z_head) && mdg_aligned16(z_tail) && mdg_aligned16(w_sym),
                "mdg_bilinear_topk: z_head, z_tail and w_sym must be 16-byte aligned");
  if constexpr (MASKED) {
    MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(mask) & 3u) == 0, "mdg_bilinear_topk_masked: mask must be 4-byte aligned");
    MDG_CHECK_ARG(plane_stride == 0 || plane_stride >= mdg_pair_mask_plane_words(n_head, n_tail),
                  "mdg_bilinear_topk_masked: plane_stride %lld is neither 0 (shared plane) nor >= the %lld words of a plane", (long long)plane_stride,
                  (long long)mdg_pair_mask_plane_words(n_head, n_tail));
  }
  const size_t need = mdg_bilinear_topk_workspace_bytes(n_head, n_tail, n_labels, D_, precision, k);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("mdg_bilinear_topk: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  TopkKArgs<MASKED> a{};
  a.z_head = z_head;
  a.vals = vals;
  a.idx = idx;
  a.n_head = n_head; a.n_tail = n_tail;
  a.k = k;
  a.eligible = eligible;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  if constexpr (MASKED) {
    a.mask.words = mask;
    a.mask.plane_stride = plane_stride;
    a.mask.ld = mdg_pair_mask_ld(n_tail);
    a.mask.nrb = mdg_cdiv(n_head, 32);
  }
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
