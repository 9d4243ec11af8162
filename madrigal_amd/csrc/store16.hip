// 16-bit score / probability tensors of the all-pairs bilinear head for gfx950 (mdg_bilinear_allpairs16_ld).
//
//   out[l,i,j] = round16(S[l,i,j])  or  round16(sigmoid(S[l,i,j])),   S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j]
//
// The general sweep of bilinear.hip (bilinear_allpairs_kernel, 8 waves x 32 head rows of one outcome, 64 tail rows per stage by
// LDS-DMA, two LDS buffers, counted waits, early / late wave halves) with a 16-bit epilogue: the fp32 accumulator -- per element the
// MFMA sequence of T = z_head W_sym[l] and of the score is that kernel's in ALL FOUR precisions (same fragments, same k order, T
// rounded to fp32 and then to the operand format) -- is rounded ONCE, to nearest even, to IEEE half or bfloat16, so the tensor is bit
// for bit `mdg_bilinear_allpairs(...).to(16-bit type)` and 2 B per score leave the chip instead of 4 (or 4 + 2 read + 2 written by
// a cast afterwards).  STORE_SIGMOID is 1.0f / (1.0f + expf(-s)), the head's formula, then the same rounding.
//
// Store shape.  In the accumulator layout lane (r, h) holds ONE column of 16 rows, so a 2-byte store per lane would write 64-byte
// half lines.  Which tail row sits in which accumulator column is free, though: an accumulator element is the dot product of one T
// row with one staged tail row whatever its position.  The LDS-DMA here stages tail row  tcol0 + 2 r + t  as LDS row 32 t + r
// (store16_stage_dma: stage_dma with that row permutation on the SOURCE address; the LDS image, its swizzle and compute_tile are
// untouched), so lane (r, h) ends up with columns 2 r (accumulator tile 0) and 2 r + 1 (tile 1) of the same 16 rows: the pair is
// packed in the lane itself -- no DPP, no LDS transpose -- and leaves as one dword.  A wave instruction writes 32 lanes x 4 B = one
// whole 128-byte line in each of two rows: the access shape of the fp32 head's stores, 16 instructions per wave and stage
// instead of 32.
// Alignment.  The dword path needs every row to start on 4 bytes: base % 4 == 0 and an even pitch (`pairs`, decided by the
// launcher).  Otherwise (contiguous rows with an odd n_tail, a view at an odd element offset) every element leaves as a 2-byte
// store.  With `pairs` and an odd n_tail the one pair that straddles the end of a row is dropped from the dword stores and its
// first half written by 16 extra 2-byte stores of the ragged tile: no lane ever writes outside columns [0, n_tail) of its own row.
// Rows past the slab and columns past n_tail get the offset 0xFFFFFFFF / fall outside the descriptor's range (bytes of the
// 16-bit type) and are dropped by the hardware, never skipped.
// Counted waits.  Per stage and wave the vector-memory stream is [LDS-DMA of tile s+1][>= 16 stores]; `s_waitcnt vmcnt(16)` at the
// top of the next stage therefore retires the DMA (loads, stores -- dropped ones included -- and LDS-DMA retire in issue order, see
// bilinear.hip) and leaves the 16 youngest stores in flight.  The 2-byte paths issue MORE than 16 stores per stage, which only
// makes that wait stricter (it then also retires the older stores), never weaker.
// No atomics, one writer per element: bit-identical from launch to launch.  z_head == z_tail takes the same sweep.
#include "bilinear_tiles.h"

namespace {

struct Store16Args {
  const float* z_head;
  TileSrc zt;
  TileSrc w;                  // W_sym (this call's labels); nrows = D
  unsigned short* out;        // [n_labels, n_head, ldo] IEEE half or bfloat16 bits
  int64_t n_head, n_tail, ldo;
  int pairs;                  // every row starts 4-byte aligned: column pairs leave as dwords
};

// stage_dma (bilinear_tiles.h) for all 8 waves with the tail rows of the tile permuted: LDS row 32 t + r <- tail row row0 + 2 r + t
template <int MODE>
__device__ __forceinline__ void store16_stage_dma(const TileSrc& s, int64_t row0, char* lds, int wave, int lane) {
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = wave + 8 * i;
      const int row = 2 * p + (lane >> 5), c = (lane & 31) ^ (row & 15);
      int64_t gr = row0 + 2 * (row & 31) + (row >> 5);
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.f32 + gr * D + c * 4, lds_addr(lds + p * 1024));
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = wave + 8 * i;
      const int row = 4 * p + (lane >> 4), c = (lane & 15) ^ (row & 15);
      int64_t gr = row0 + 2 * (row & 31) + (row >> 5);
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.hi + gr * D + c * 8, lds_addr(lds + p * 1024));
      if constexpr (MODE == MDG_PREC_BF16X3) glds16(s.lo + gr * D + c * 8, lds_addr(lds + LO_OFF + p * 1024));
    }
  }
}

template <int MODE, int EPI, int TY>
__global__ __launch_bounds__(512, 2) void bilinear_store16_kernel(const Store16Args p) {
  constexpr int NW = 8, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const buf0 = smem;
  char* const buf1 = smem + STAGE_BYTES;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int64_t l = blockIdx.y;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;

  // ---------------- prologue: T = z_head[rows] . W_sym[l], kept as the A operand (bilinear_allpairs_kernel's) -------------
  AFrag<MODE> At;
  {
    AFrag<MODE> Az;
    int64_t zr = row0 + wave * 32 + r;
    zr = zr < p.n_head ? zr : p.n_head - 1;
    afrag_from_global<MODE>(Az, p.z_head + zr * D, h);
    TileSrc ws = p.w;
    if constexpr (MODE == MDG_PREC_F32) ws.f32 += l * D * D;
    else { ws.hi += l * D * D; if constexpr (MODE == MDG_PREC_BF16X3) ws.lo += l * D * D; }
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

  // ---------------- sweep over the tail drugs ------------------------------------------------
  const int nst = static_cast<int>((p.n_tail + BN - 1) / BN);
  const int64_t slab_rows = (p.n_head - row0) < BM ? (p.n_head - row0) : BM;
  unsigned short* const out_slab = p.out + (l * p.n_head + row0) * p.ldo;
  // range in bytes of the 16-bit type, up to the last element of the slab's last row (the launcher keeps 256 * ldo * 2 < 2^31)
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(out_slab, 0, static_cast<int>(((slab_rows - 1) * p.ldo + p.n_tail) * 2), 0x00020000);
  const int start = static_cast<int>((blockIdx.x * 5u + blockIdx.y * 3u) % static_cast<unsigned>(nst));   // HBM channel spreading
  auto tile_of = [&](int s) { int t = s + start; return t >= nst ? t - nst : t; };
  const bool pairs = p.pairs != 0;
  const bool odd_end = (p.n_tail & 1) != 0;

  // accumulators -> 16 dwords: low half column 2 r (tile 0), high half column 2 r + 1 (tile 1), row acc_row(v, h)
  auto pack = [&](const f32x16 (&acc)[2], unsigned (&pk)[16]) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      float a = acc[0][v], b = acc[1][v];
      if constexpr (EPI == MDG_EPI_STORE_SIGMOID) {
        a = 1.0f / (1.0f + expf(-a));
        b = 1.0f / (1.0f + expf(-b));
      }
      pk[v] = round16<TY>(a) | (round16<TY>(b) << 16);
    }
  };
  // at least 16 stores per call, whatever is in range (the counted wait depends on it)
  auto store_tile = [&](const unsigned (&pk)[16], int64_t tcol0) {
    const int64_t col = tcol0 + 2 * r;
    if (pairs) {
      const bool both = col + 1 < p.n_tail;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t e = static_cast<int64_t>(wave * 32 + acc_row(v, h)) * p.ldo + col;
        const unsigned off = both ? static_cast<unsigned>(e * 2) : 0xFFFFFFFFu;               // out of range => dropped
        __builtin_amdgcn_raw_buffer_store_b32(pk[v], rsrc, off, 0, 0);
      }
      if (odd_end && tcol0 + BN > p.n_tail) {     // wave-uniform: the pair that straddles the end of the row, first half only
        const bool last = col + 1 == p.n_tail;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t e = static_cast<int64_t>(wave * 32 + acc_row(v, h)) * p.ldo + col;
          const unsigned off = last ? static_cast<unsigned>(e * 2) : 0xFFFFFFFFu;
          __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(pk[v] & 0xFFFFu), rsrc, off, 0, 0);
        }
      }
    } else {                                      // rows at 2-byte alignment: every element on its own
      const bool ok0 = col < p.n_tail, ok1 = col + 1 < p.n_tail;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t e = static_cast<int64_t>(wave * 32 + acc_row(v, h)) * p.ldo + col;
        const unsigned off0 = ok0 ? static_cast<unsigned>(e * 2) : 0xFFFFFFFFu;
        const unsigned off1 = ok1 ? static_cast<unsigned>(e * 2 + 2) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(pk[v] & 0xFFFFu), rsrc, off0, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(pk[v] >> 16), rsrc, off1, 0, 0);
      }
    }
  };

  // The two waves that share a SIMD (w, w + 4) run the same code between the same barriers: the younger half issues the stores of
  // the PREVIOUS tile (16 packed registers) before its MFMAs, so one partner stores while the other computes (as in bilinear.hip).
  const bool late = __builtin_amdgcn_readfirstlane(wave) >= NW / 2;
  unsigned held[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) held[v] = 0u;
  int64_t held_col0 = p.n_tail;                   // first stage of a late wave: 16 (or 32) dropped stores
  store16_stage_dma<MODE>(p.zt, static_cast<int64_t>(tile_of(0)) * BN, buf0, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int s = 0; s < nst; ++s) {
    const int64_t tcol0 = static_cast<int64_t>(tile_of(s)) * BN;
    char* const cur = (s & 1) ? buf1 : buf0;
    char* const nxt = (s & 1) ? buf0 : buf1;
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");   // this wave's DMA pieces of tile s have landed
    __builtin_amdgcn_s_barrier();                       // ... and everybody else's; every wave has finished reading tile s-1
    // past the end the tile index repeats the last one; that copy is never consumed
    store16_stage_dma<MODE>(p.zt, static_cast<int64_t>(tile_of(s + 1 < nst ? s + 1 : s)) * BN, nxt, wave, lane);
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    if (late) {
      store_tile(held, held_col0);
      compute_tile<MODE>(At, cur, r, h, acc);
      pack(acc, held);
      held_col0 = tcol0;
    } else {
      compute_tile<MODE>(At, cur, r, h, acc);
      unsigned pk[16];
      pack(acc, pk);
      store_tile(pk, tcol0);
    }
  }
  if (late) store_tile(held, held_col0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int MODE, int EPI>
int launch_store16_ty(const Store16Args& a, int64_t n_labels, int score_type, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.n_head, 256)), static_cast<unsigned>(n_labels));
  if (score_type == MDG_SCORE_F16) hipLaunchKernelGGL((bilinear_store16_kernel<MODE, EPI, MDG_SCORE_F16>), grid, dim3(512), 2 * STAGE_BYTES, st, a);
  else hipLaunchKernelGGL((bilinear_store16_kernel<MODE, EPI, MDG_SCORE_BF16>), grid, dim3(512), 2 * STAGE_BYTES, st, a);
  MDG_CHECK_LAUNCH("mdg_bilinear_allpairs16_ld");
  return MDG_OK;
}

template <int MODE>
int launch_store16(Store16Args& a, const float* z_tail, const float* w_sym, int64_t n_labels, int epilogue, int score_type, char* ws,
                   hipStream_t st) {
  make_head_images<MODE>(a.zt, a.w, z_tail, w_sym, a.n_tail, n_labels, ws, st);
  MDG_CHECK_LAUNCH("mdg_bilinear_allpairs16_ld(images)");
  return epilogue == MDG_EPI_STORE ? launch_store16_ty<MODE, MDG_EPI_STORE>(a, n_labels, score_type, st)
                                   : launch_store16_ty<MODE, MDG_EPI_STORE_SIGMOID>(a, n_labels, score_type, st);
}

}  // namespace

extern "C" int mdg_bilinear_allpairs16_ld(const float* z_head, const float* z_tail, const float* w_sym, void* out, int64_t ldo,
                                          int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int epilogue,
                                          int score_type, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "mdg_bilinear_allpairs16_ld";
  MDG_CHECK_ARG(D_ == D, "%s: D must be %d (got %lld)", fn, D, (long long)D_);
  MDG_CHECK_ARG(epilogue == MDG_EPI_STORE || epilogue == MDG_EPI_STORE_SIGMOID,
                "%s: epilogue %d has no 16-bit form (MDG_EPI_STORE or MDG_EPI_STORE_SIGMOID)", fn, epilogue);
  MDG_CHECK_ARG(score_type == MDG_SCORE_F16 || score_type == MDG_SCORE_BF16, "%s: unknown score type %d", fn, score_type);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "%s: negative size", fn);
  MDG_CHECK_ARG(ldo >= n_tail, "%s: row pitch %lld < n_tail %lld", fn, (long long)ldo, (long long)n_tail);
  MDG_CHECK_ARG(n_labels <= 65535, "%s: n_labels %lld > 65535 per call", fn, (long long)n_labels);
  MDG_CHECK_ARG(ldo * 256 * 2 < (int64_t(1) << 31), "%s: n_tail / row pitch %lld too large", fn, (long long)ldo);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3 || precision == MDG_PREC_BF16 || precision == MDG_PREC_F16,
                "%s: unknown precision %d", fn, precision);
  if (n_head == 0 || n_tail == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(z_head && z_tail && w_sym && out, "%s: null pointer", fn);
  MDG_CHECK_ARG(mdg_aligned16(z_head) && mdg_aligned16(z_tail) && mdg_aligned16(w_sym), "%s: z_head, z_tail and w_sym must be 16-byte aligned",
                fn);
  MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 1u) == 0, "%s: out must be 2-byte aligned", fn);
  const size_t need = mdg_bilinear_allpairs_workspace_bytes(n_head, n_tail, n_labels, D_, precision);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("%s: workspace of %zu bytes (16-byte aligned) required, got %zu", fn, need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  Store16Args a{};
  a.z_head = z_head;
  a.out = static_cast<unsigned short*>(out);
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.pairs = ((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (ldo & 1) == 0) ? 1 : 0;
  a.zt.nrows = n_tail;
  a.w.nrows = D;
  char* ws = static_cast<char*>(workspace);
  switch (precision) {
    case MDG_PREC_F32: return launch_store16<MDG_PREC_F32>(a, z_tail, w_sym, n_labels, epilogue, score_type, ws, st);
    case MDG_PREC_BF16X3: return launch_store16<MDG_PREC_BF16X3>(a, z_tail, w_sym, n_labels, epilogue, score_type, ws, st);
    case MDG_PREC_BF16: return launch_store16<MDG_PREC_BF16>(a, z_tail, w_sym, n_labels, epilogue, score_type, ws, st);
    default: return launch_store16<MDG_PREC_F16>(a, z_tail, w_sym, n_labels, epilogue, score_type, ws, st);
  }
}
