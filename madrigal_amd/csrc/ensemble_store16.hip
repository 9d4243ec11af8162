// 16-bit probability tensors of the checkpoint ensemble of the all-pairs head for gfx950 (mdg_bilinear_ensemble_sigmoid16).
//
//   out[l,i,j] = round16(P[l,i,j]),   P[l,i,j] = (sum_{k<K} sigmoid(z_head_k[i]^T W_sym_k[l] z_tail_k[j])) / K      K = 1..8
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614.)  This is
// ensemble.hip's sweep (ensemble_sigmoid_kernel: T rebuilt per model and per chunk of ENS_CH tail tiles, running sums of the chunk in
// registers summed in model order, one division by K; K = 1 with 8 waves and T resident, K >= 2 with 4 waves; the general sweep and
// the symmetric one with its mirrored stores and its diagonal-block rule; stagger) with a 16-bit epilogue: P (fp32, after the
// division) is rounded ONCE, to nearest even, to IEEE half or bfloat16 (pack16: round16 of bilinear_tiles.h for a column pair in one
// packed conversion), so the tensor is bit for bit
// `mdg_bilinear_ensemble_sigmoid(same operands).to(16-bit type)` and 2 B per probability leave the chip instead of 4.
//
// Store shape (store16.hip's).  The LDS-DMA stages tail row tcol0 + 2 r + t as LDS row 32 t + r (stage_dma_pairs, ensemble_sweep.h:
// the permutation is on the SOURCE address; LDS image, swizzle and compute_tile_spread untouched).  An accumulator element is the
// dot product of one T row with one staged tail row in the same k order wherever that row sits, so every P has the fp32 kernel's
// bits; lane (r, h) holds columns tcol0 + 2 r (tile 0) and tcol0 + 2 r + 1 (tile 1) of the same 16 rows and packs them into one
// dword: a wave instruction writes a whole 128-byte line in each of two rows, 16 row stores per stage instead of 32.
//
// Mirrored stores (symmetric sweep).  The packed tile goes through the wave's slab as [64 tail rows][32 head rows] of 16-bit values
// (slab row 2 r + t = output row tcol0 + 2 r + t; 8 x 8-byte writes per lane, the 8-byte chunk XORed with (slab row / 2) & 7) and
// leaves as rows of the transposed block: 32 columns = 64 bytes per row, so lane (g, d) = (lane / 16, lane % 16) of instruction q
// writes the dword of columns 2 d, 2 d + 1 of output row tcol0 + 4 q + g -- four whole 64-byte row segments per instruction, 16
// instructions per stage instead of 32.
//
// One writer per element.  As in ensemble.hip, inside the diagonal block only entries with j >= i leave as rows and only j > i are
// mirrored.  A packed pair straddles that boundary where its high column (rows) or its high column (mirrored) is the first / last
// one that path owns; such a pair is dropped from the dword stores and the half the path owns leaves by a 2-byte store:
//   rows,     pair (c, c + 1) of row i:   dword if c >= i;      c + 1 == i: the HIGH half alone (the diagonal element)
//   mirrored, pair (c, c + 1) of row j:   dword if j > c + 1;   j == c + 1: the LOW half alone
// so every element has one writer and every P[l] is exactly symmetric.
//
// Alignment.  The dword paths need every row to start on 4 bytes: base % 4 == 0 and an even pitch (`pairs`, decided by the
// launcher, a template parameter: both store forms in one kernel cost the K >= 2 symmetric kernel its full unrolling); row-store columns tcol0 + 2 r and mirrored columns row0 + 32 wave + 2 d are even.  Otherwise every element leaves as a
// 2-byte store.  With `pairs` and an odd n_tail the pair that straddles the end of a row is dropped from the dword stores and its
// LOW half written by a 2-byte store.  No lane writes outside columns [0, n_tail) of its own row: columns are tested, rows past the
// slab fall outside the descriptor's range (bytes of the 16-bit type, up to the last element of the last row) or get the offset
// 0xFFFFFFFF, and are dropped by the hardware, never skipped.
//
// Counted waits.  Per storing stage and wave the vector-memory stream is [LDS-DMA of the next tile][row stores][mirrored stores]:
//   row stores       pairs: 16 dwords, + 16 2-byte stores in a diagonal tile or in the ragged tile of an odd n_tail;  2-byte path: 32
//   mirrored stores  pairs: 16 dwords, + 16 2-byte stores in a diagonal tile or when the wave's 32 columns reach past an odd N;
//                    2-byte path: 32
// Every one is issued, the dropped ones included.  The fewest operations after the DMA are therefore 16 in the general sweep and
// 32 in the symmetric one, on every path: `s_waitcnt vmcnt(16)` resp. `vmcnt(32)` at the top of the next stage retires the DMA
// (in-order retirement, bilinear.hip) and leaves the youngest stores in flight; the paths that issue more only make the wait
// stricter.  A stage that follows a T rebuild or issued no stores waits vmcnt(0), as in ensemble.hip.
// No atomics: bit-identical from launch to launch.
#include "ensemble_sweep.h"

namespace {

template <bool ONE> constexpr int kWaves16 = ONE ? 8 : ENS_NW;
constexpr int BM_MAX16 = 32 * 8;       // the most head rows per workgroup
template <int NW> constexpr int kLds16 = 2 * STAGE_BYTES + NW * SLAB_BYTES;   // stage buffers + one slab per wave (T halves while rebuilding)

struct Ensemble16Args : EnsOperands {
  unsigned short* out;        // [n_labels, n_head, ldo] IEEE half or bfloat16 bits
  int64_t n_head, n_tail, ldo;
  int n_models;
  int stagger;
};

typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;

// round16 (bilinear_tiles.h) of a column pair as ONE packed conversion (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32, the same rounding to
// nearest even): low half `lo`, high half `hi`
template <int TY>
__device__ __forceinline__ unsigned pack16(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  const f32x2_t v = {lo, hi};
  if constexpr (TY == MDG_SCORE_F16) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
  } else {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
  }
}

// ONE: K == 1 (T built once per row block and held for the whole sweep, no running sums)
// PAIRS: every row starts 4-byte aligned, column pairs leave as dwords (otherwise every element by a 2-byte store)
template <int MODE, bool SYM, bool ONE, int CH, int TY, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves16<ONE>, 1) void ensemble_sigmoid16_kernel(const Ensemble16Args p) {
  constexpr int NW = kWaves16<ONE>, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t l = blockIdx.y, N = p.n_tail, ld = p.ldo;
  const int K = ONE ? 1 : p.n_models;
  const float kf = static_cast<float>(K);
  const bool odd_end = (N & 1) != 0;
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  unsigned short* const out_l = p.out + l * p.n_head * ld;
  const int nst = static_cast<int>((N + BN - 1) / BN);
  const int nb = static_cast<int>((p.n_head + BM - 1) / BM);

  for (int half = 0; half < (SYM ? 2 : 1); ++half) {
    // symmetric: row blocks b and nb-1-b share a workgroup (their tile counts add up to the same total for every pair)
    const int rbk = (SYM && half == 1) ? nb - 1 - static_cast<int>(blockIdx.x) : static_cast<int>(blockIdx.x);
    if (SYM && half == 1 && rbk == static_cast<int>(blockIdx.x)) break;
    const int64_t row0 = static_cast<int64_t>(rbk) * BM;
    const int t0 = SYM ? rbk * (BM / BN) : 0;
    const int t_diag_end = t0 + BM / BN;
    const int nt = nst - t0;
    const int start = p.stagger ? static_cast<int>((blockIdx.x * 5u + blockIdx.y * 3u) % static_cast<unsigned>(nt)) : 0;
    auto tile_of = [&](int s) { int t = s + start; return t0 + (t >= nt ? t - nt : t); };
    const int64_t slab_rows = (p.n_head - row0) < BM ? (p.n_head - row0) : BM;
    // range in bytes of the 16-bit type, up to the last element of the slab's last row (the launcher keeps BM_MAX16 * ldo * 2 < 2^31)
    const __amdgpu_buffer_rsrc_t rs_rows =
        __builtin_amdgcn_make_buffer_rsrc(out_l + row0 * ld, 0, static_cast<int>(((slab_rows - 1) * ld + N) * 2), 0x00020000);
    int64_t zr = row0 + wave * 32 + (lane & 31);
    zr = zr < p.n_head ? zr : p.n_head - 1;
    auto build = [&](AFrag<MODE>& A, int k) {
      int t_o = tid;
      asm volatile("" : "+v"(t_o));
      const int r = t_o & 31, h = (t_o >> 5) & 1;
      TileSrc wl = pick(p.w, k);
      if constexpr (MODE == MDG_PREC_F32) wl.f32 += l * D * D;
      else { wl.hi += l * D * D; wl.lo += l * D * D; }
      build_t<MODE, NW>(A, pick(p.z_head, k) + zr * D, wl, smem, slab, t_o, r, h);
    };
    AFrag<MODE> At;
    if constexpr (ONE) build(At, 0);
    int par = 0;               // stage buffer of the next stage
    bool prefetched = false;   // the next stage's tile is already on its way
    bool stored = false;       // stores were issued after the last LDS-DMA
    const int nch = (nt + CH - 1) / CH;
    for (int c = 0; c < nch; ++c) {
      const int s0 = c * CH;
      const int nc = nt - s0 < CH ? nt - s0 : CH;
      float psum[CH][2][16];
      for (int k = 0; k < K; ++k) {
        if constexpr (!ONE) {                 // every (chunk, model): the previous T is dead here, its registers are reused
          build(At, k);
          prefetched = false;
        }
        const TileSrc zt = pick(p.zt, k);
        if (!prefetched) {
          int lane = tid & 63;
          asm volatile("" : "+v"(lane));
          stage_dma_pairs<MODE, NW>(zt, static_cast<int64_t>(tile_of(s0)) * BN, smem + par * STAGE_BYTES, wave, lane);
          stored = false;
        }
        const bool last = (k == K - 1);
#pragma unroll
        for (int ci = 0; ci < CH; ++ci) {
          if (ci < nc) {
            // lane-dependent offsets recomputed per stage (hoisted out of the loops they would hold ~100 VGPRs per unrolled stage)
            int lane = tid & 63;
            asm volatile("" : "+v"(lane));
            const int r = lane & 31, h = lane >> 5;
            // this tile landed; the youngest stores stay in flight: at least 16 (general) / 32 (symmetric) were issued after its DMA
            if (stored) {
              if constexpr (SYM) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
              else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                                       // ... for every wave; every wave is done with the other buffer
            char* const cur = smem + par * STAGE_BYTES;
            char* const nxt = smem + (par ^ 1) * STAGE_BYTES;
            prefetched = false;
            if (ci + 1 < nc) {
              stage_dma_pairs<MODE, NW>(zt, static_cast<int64_t>(tile_of(s0 + ci + 1)) * BN, nxt, wave, lane);
              prefetched = true;
            } else if (ONE && c + 1 < nch) {       // one model: T stays resident, the sweep runs on into the next chunk
              stage_dma_pairs<MODE, NW>(zt, static_cast<int64_t>(tile_of(s0 + nc)) * BN, nxt, wave, lane);
              prefetched = true;
            }
            stored = false;
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
            // the head's products in the head's order, B fragments fetched one step ahead (no hook: nothing is stored in between)
            compute_tile_spread<MODE>(At, cur, r, h, acc, [](int) {});
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int v = 0; v < 16; ++v) {
                const float sg = sigmoid_head(acc[t][v]);
                psum[ci][t][v] = k == 0 ? sg : psum[ci][t][v] + sg;
                if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);             // four sigmoids' temporaries at a time
              }
            if (last) {
              const int tile = tile_of(s0 + ci);
              const int64_t tcol0 = static_cast<int64_t>(tile) * BN;
              const bool diag = SYM && tile < t_diag_end;
              // P = sum / K, rounded once; pk[v]: low half column tcol0 + 2 r (tile 0), high half column tcol0 + 2 r + 1 (tile 1),
              // row acc_row(v, h) of the wave's 32
              unsigned pk[16];
#pragma unroll
              for (int v = 0; v < 16; ++v)
                pk[v] = pack16<TY>(psum[ci][0][v] / kf, psum[ci][1][v] / kf);
              // byte offsets in 32 bits (the slab is < 2^31 bytes): a lane base plus a wave-uniform row step per register
              const unsigned lrow_base = static_cast<unsigned>(((wave * 32 + 4 * h) * ld + tcol0 + 2 * r) * 2);
              const int diag_d = static_cast<int>(tcol0 + 2 * r - (row0 + wave * 32 + 4 * h));    // low column - row at v = 0
              const bool in_lo = tcol0 + 2 * r < N, in_hi = tcol0 + 2 * r + 1 < N;
              if constexpr (PAIRS) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                  const int dv = (v & 3) + 8 * (v >> 2);
                  const bool ok = in_hi && (!diag || diag_d - dv >= 0);
                  const unsigned off = ok ? lrow_base + static_cast<unsigned>(dv * ld * 2) : 0xFFFFFFFFu;
                  __builtin_amdgcn_raw_buffer_store_b32(pk[v], rs_rows, off, 0, 0);
                }
                if (diag || (odd_end && tcol0 + BN > N)) {       // wave-uniform: the pairs only one half of which is this path's
#pragma unroll
                  for (int v = 0; v < 16; ++v) {
                    const int dv = (v & 3) + 8 * (v >> 2);
                    const bool hi_only = diag && in_hi && diag_d - dv == -1;                      // high column == row: the diagonal element
                    const bool lo_only = in_lo && !in_hi && (!diag || diag_d - dv >= 0);          // the last column of an odd n_tail
                    const unsigned at = lrow_base + static_cast<unsigned>(dv * ld * 2);
                    const unsigned off = hi_only ? at + 2u : (lo_only ? at : 0xFFFFFFFFu);
                    const unsigned val = hi_only ? pk[v] >> 16 : pk[v] & 0xFFFFu;
                    __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(val), rs_rows, off, 0, 0);
                  }
                }
              } else {                                           // rows at 2-byte alignment: every element on its own
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                  const int dv = (v & 3) + 8 * (v >> 2);
                  const bool ok0 = in_lo && (!diag || diag_d - dv >= 0);
                  const bool ok1 = in_hi && (!diag || diag_d + 1 - dv >= 0);
                  const unsigned at = lrow_base + static_cast<unsigned>(dv * ld * 2);
                  __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(pk[v] & 0xFFFFu), rs_rows, ok0 ? at : 0xFFFFFFFFu, 0, 0);
                  __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(pk[v] >> 16), rs_rows, ok1 ? at + 2u : 0xFFFFFFFFu, 0, 0);
                }
              }
              if constexpr (SYM) {
                // the packed tile into the slab: slab row 2 r + t (64 bytes: 32 head rows) = output row tcol0 + 2 r + t; the four rows
                // acc_row(4 g .. 4 g + 3, h) = 8 g + 4 h .. + 3 are 8-byte chunk 2 g + h, XORed with (slab row / 2) & 7 = r & 7
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                  for (int g = 0; g < 4; ++g) {
                    const unsigned sh = 16 * t;
                    const u32x2_t w2 = {((pk[4 * g] >> sh) & 0xFFFFu) | (((pk[4 * g + 1] >> sh) & 0xFFFFu) << 16),
                                        ((pk[4 * g + 2] >> sh) & 0xFFFFu) | (((pk[4 * g + 3] >> sh) & 0xFFFFu) << 16)};
                    *reinterpret_cast<u32x2_t*>(slab + (2 * r + t) * 64 + (((2 * g + h) ^ (r & 7)) << 3)) = w2;
                  }
                const int64_t mrows = (N - tcol0) < BN ? (N - tcol0) : BN;
                const __amdgpu_buffer_rsrc_t rs_m =
                    __builtin_amdgcn_make_buffer_rsrc(out_l + tcol0 * ld, 0, static_cast<int>(((mrows - 1) * ld + N) * 2), 0x00020000);
                const int g4 = lane >> 4, d = lane & 15;
                const int64_t gc = row0 + wave * 32 + 2 * d;                     // output column of the low half
                const unsigned m_base = static_cast<unsigned>((g4 * ld + gc) * 2);
                const int m_d = static_cast<int>(tcol0 + g4 - gc);               // output row - low output column at q = 0
                const bool c_lo = gc < N, c_hi = gc + 1 < N;
                // wave-uniform: pairs only the low half of which is this path's (diagonal tile; the last column of an odd N)
                const bool edge = diag || (odd_end && row0 + wave * 32 + 32 > N);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                  if ((q & 7) == 0) __builtin_amdgcn_sched_barrier(0);         // a few slab reads in flight, not all 16
                  const int R = 4 * q + g4;
                  const unsigned val = *reinterpret_cast<const unsigned*>(slab + R * 64 + ((((d >> 1) ^ (R >> 1)) & 7) << 3) + (d & 1) * 4);
                  const bool ok_lo = c_lo && (!diag || m_d + 4 * q > 0);
                  const bool ok_hi = c_hi && (!diag || m_d + 4 * q > 1);
                  const unsigned at = m_base + static_cast<unsigned>(4 * q * ld * 2);
                  if constexpr (PAIRS) {
                    __builtin_amdgcn_raw_buffer_store_b32(val, rs_m, ok_hi ? at : 0xFFFFFFFFu, 0, 0);
                    if (edge)
                      __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(val & 0xFFFFu), rs_m,
                                                            (ok_lo && !ok_hi) ? at : 0xFFFFFFFFu, 0, 0);
                  } else {
                    __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(val & 0xFFFFu), rs_m, ok_lo ? at : 0xFFFFFFFFu, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b16(static_cast<unsigned short>(val >> 16), rs_m, ok_hi ? at + 2u : 0xFFFFFFFFu, 0, 0);
                  }
                }
              }
              stored = true;
            }
            par ^= 1;
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

template <int MODE, int TY, bool PAIRS>
int launch_ensemble16_ty(const Ensemble16Args& a, bool sym, int64_t n_labels, hipStream_t st) {
  const bool one = a.n_models == 1;
  const int nw = one ? kWaves16<true> : kWaves16<false>;
  const int nb = static_cast<int>(mdg_cdiv(a.n_head, 32 * nw));
  const dim3 block(64 * nw);
  if (sym) {
    const dim3 grid(static_cast<unsigned>((nb + 1) / 2), static_cast<unsigned>(n_labels));
    if (one) hipLaunchKernelGGL((ensemble_sigmoid16_kernel<MODE, true, true, ENS_CH, TY, PAIRS>), grid, block, kLds16<kWaves16<true>>, st, a);
    else hipLaunchKernelGGL((ensemble_sigmoid16_kernel<MODE, true, false, ENS_CH, TY, PAIRS>), grid, block, kLds16<kWaves16<false>>, st, a);
  } else {
    const dim3 grid(static_cast<unsigned>(nb), static_cast<unsigned>(n_labels));
    if (one) hipLaunchKernelGGL((ensemble_sigmoid16_kernel<MODE, false, true, ENS_CH, TY, PAIRS>), grid, block, kLds16<kWaves16<true>>, st, a);
    else hipLaunchKernelGGL((ensemble_sigmoid16_kernel<MODE, false, false, ENS_CH, TY, PAIRS>), grid, block, kLds16<kWaves16<false>>, st, a);
  }
  MDG_CHECK_LAUNCH("mdg_bilinear_ensemble_sigmoid16");
  return MDG_OK;
}

// the models' operand images (the reducing products' layout: ensemble_sweep.h), then the sweep
template <int MODE>
int launch_ensemble16(Ensemble16Args& a, const float* const* z_tail, const float* const* w_sym, bool sym, int64_t n_labels, int score_type,
                      bool pairs, char* ws, hipStream_t st) {
  const int rc = ens_make_images<MODE>(a, z_tail, w_sym, a.n_models, a.n_tail, n_labels, ws, st, "mdg_bilinear_ensemble_sigmoid16(images)");
  if (rc != MDG_OK) return rc;
  if (score_type == MDG_SCORE_F16)
    return pairs ? launch_ensemble16_ty<MODE, MDG_SCORE_F16, true>(a, sym, n_labels, st)
                 : launch_ensemble16_ty<MODE, MDG_SCORE_F16, false>(a, sym, n_labels, st);
  return pairs ? launch_ensemble16_ty<MODE, MDG_SCORE_BF16, true>(a, sym, n_labels, st)
               : launch_ensemble16_ty<MODE, MDG_SCORE_BF16, false>(a, sym, n_labels, st);
}

}  // namespace

extern "C" int mdg_bilinear_ensemble_sigmoid16(const float* const* z_head_host, const float* const* z_tail_host,
                                               const float* const* w_sym_host, int n_models, void* out, int64_t ldo, int64_t n_head,
                                               int64_t n_tail, int64_t n_labels, int64_t D_, int precision, int score_type, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  const char* const fn = "mdg_bilinear_ensemble_sigmoid16";
  MDG_CHECK_ARG(n_models >= 1 && n_models <= MAXK, "%s: n_models must be in 1..%d (got %d)", fn, MAXK, n_models);
  MDG_CHECK_ARG(D_ == D, "%s: D must be %d (got %lld)", fn, D, (long long)D_);
  MDG_CHECK_ARG(score_type == MDG_SCORE_F16 || score_type == MDG_SCORE_BF16, "%s: unknown score type %d (MDG_SCORE_F16 or MDG_SCORE_BF16)", fn,
                score_type);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "%s: negative size", fn);
  MDG_CHECK_ARG(ldo >= n_tail, "%s: row pitch %lld < n_tail %lld", fn, (long long)ldo, (long long)n_tail);
  MDG_CHECK_ARG(n_labels <= 65535, "%s: n_labels %lld > 65535 per call", fn, (long long)n_labels);
  // a workgroup's slab of rows and the 64 rows of a mirrored tile are addressed with 32-bit byte offsets
  MDG_CHECK_ARG(ldo < (int64_t(1) << 31) / (BM_MAX16 * 2), "%s: row pitch %lld too large", fn, (long long)ldo);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3, "%s: precision %d not offered (MDG_PREC_F32 or MDG_PREC_BF16X3)", fn,
                precision);
  const size_t need = ens_workspace_bytes(n_tail, n_labels, D_, n_models, precision);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("%s: workspace of %zu bytes (16-byte aligned) required, got %zu", fn, need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  if (n_head == 0 || n_tail == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(z_head_host && z_tail_host && w_sym_host && out, "%s: null pointer", fn);
  MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 1u) == 0, "%s: out must be 2-byte aligned", fn);
  bool sym = n_head == n_tail;
  for (int k = 0; k < n_models; ++k) {
    MDG_CHECK_ARG(z_head_host[k] && z_tail_host[k] && w_sym_host[k], "%s: null pointer for model %d", fn, k);
    MDG_CHECK_ARG(mdg_aligned16(z_head_host[k]) && mdg_aligned16(z_tail_host[k]) && mdg_aligned16(w_sym_host[k]),
                  "%s: z_head, z_tail and w_sym must be 16-byte aligned (model %d)", fn, k);
    sym = sym && z_head_host[k] == z_tail_host[k];
  }
  Ensemble16Args a{};
  ens_fill_operands(a, z_head_host, n_models, n_tail);
  a.out = static_cast<unsigned short*>(out);
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.n_models = n_models;
  a.stagger = 1;
  // every row starts on 4 bytes: the packed-pair kernels; otherwise the 2-byte ones
  const bool pairs = (reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (ldo & 1) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  if (precision == MDG_PREC_F32) return launch_ensemble16<MDG_PREC_F32>(a, z_tail_host, w_sym_host, sym, n_labels, score_type, pairs, ws, st);
  return launch_ensemble16<MDG_PREC_BF16X3>(a, z_tail_host, w_sym_host, sym, n_labels, score_type, pairs, ws, st);
}
