// GeomCA on the device for gfx950: the epsilon-graph of two [n,128] fp32 embedding sets without an [n,n] matrix or an edge list.
//
// Replaces madrigal/evaluate/GeomCA.py:250-282 (estimate_distance: cdist + np.percentile), :333-352 (get_sparse_pnts: GUDHI's
// sparsify_point_set) and :354-387 / :423-435 (RipsComplex 1-skeleton + networkx connected components).
//
// Every geometric decision is a comparison of d2(x, y) = max(fmaf(-2, g(x,y), n(x) + n(y)), 0) with a threshold, g the gram_step
// chain of gram.h and n(x) = g(x, x) formed BY THAT CHAIN (gc_prep takes the diagonal of 32-row Gram tiles), so d2 is the same bits
// seen from either row and bitwise-equal rows are at d2 == 0 exactly.
//
// gc_sweep<EPI> is the row-persistent sweep of knn.hip: grid (row blocks of 128, column segments), 4 waves, wave w keeps rows
// 32 w .. 32 w + 31 as the A operand in registers, the columns arrive in 64-column fp32 stages by LDS-DMA into two 32 KB buffers
// (one vmcnt(0) + barrier per stage).  The column count may live on the device (the kept array of the sparsifier grows without a
// host read); a segment whose range is empty leaves before its first barrier.  Epilogues:
//   NEAR   flag[row] |= some column has d2 < thr                      (candidates of a chunk against everything kept so far)
//   BITS   bits[row][col / 32]: the chunk x chunk matrix of d2 < thr   (ballots; every word has one writer)
//   LINK   cand[row] = min(cand[row], label[col]) over d2 <= thr, col != row; LINKDEG also deg_same / deg_cross
//   DIGIT  one digit of the radix select on the fp32 bit pattern of d2 > 0 over the pairs with ida[row] != idb[col]: LDS histograms
//          (non-returning adds) for two prefixes, flushed to 64-bit global counters
// Segments combine by integer atomicOr / atomicMin / atomicAdd only: results do not depend on order or on the segment count.
//
// gc_resolve: one workgroup walks a chunk in input order with the drop mask in registers (lane w of wave 0 = word w) and the bit
// matrix in LDS: row i is kept iff its bit is clear (not near a kept earlier point, not dropped by a kept row of the chunk), and
// only a KEPT row drops others.  The kept rows are compacted onto the kept array.
// Components: hooking of each tree's root onto the smallest label any member sees (gc_hook, from a snapshot) + pointer jumping to
// the roots (gc_jump) between LINK sweeps, until a device flag says no vertex saw a smaller label.
//
// Budget (-Rpass-analysis=kernel-resource-usage): 64 KB LDS (DIGIT 80 KB) and under 256 VGPRs, 0 scratch.
#include "bilinear_tiles.h"      // stage_dma, tile_off, acc_row
#include "gram.h"

#include <limits.h>

namespace {

constexpr int GC_BM = 128;               // rows per workgroup: 4 waves x 32
constexpr int GC_THREADS = 256;
constexpr int GC_LDS = 2 * STAGE_BYTES;
constexpr int GC_CUS = 256;              // MI355X
constexpr int GC_BINS = 2048;            // 11 + 11 + 10 bits
constexpr int GC_HIST_LDS = 2 * GC_BINS * 4;
constexpr int GC_CHUNK_MAX = 512;        // gc_resolve keeps the chunk's bit matrix (C x C / 8 bytes) in LDS
constexpr int GC_CHUNK_DEFAULT = 512;
constexpr int GC_MAX_SWEEPS = 128;
static_assert(D == 128 && BN == 64 && GC_LDS == 65536, "two 64-column fp32 stages of 128 k values");

enum { GC_NEAR = 0, GC_BITS = 1, GC_LINK = 2, GC_LINKDEG = 3, GC_DIGIT = 4 };

__device__ __forceinline__ float gc_d2(float g, float na, float nb) { return fmaxf(fmaf(-2.0f, g, na + nb), 0.f); }

// One wave per 32 rows: lane (r, h) holds half h of row r0 + r, which is both the A and the B fragment of the 32 x 32 Gram tile
// of these rows with themselves.  norm[row] = the tile's diagonal.
__global__ __launch_bounds__(GC_THREADS) void gc_prep(const float* __restrict__ x, int n, float* __restrict__ norm, int* __restrict__ status) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int r0 = (blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6)) * 32;
  if (r0 >= n) return;
  const int row = min(r0 + r, n - 1);
  const float* xr = x + static_cast<int64_t>(row) * D + 4 * h;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 a = *reinterpret_cast<const float4*>(xr + 8 * q);
    ok = ok && finite4(a);
    acc = gram_step(a, a, acc);
  }
  // element [row r][col r] sits in lane (r, (r >> 2) & 1), register (r & 3) + 4 (r >> 3)
  const int vsel = (r & 3) + 4 * (r >> 3);
  float dg = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) dg = v == vsel ? acc[v] : dg;
  const bool mine = h == ((r >> 2) & 1);
  const bool valid = r0 + r < n;
  if (valid && (!ok || (mine && !isfinite(dg)))) atomicOr(status, 1);
  if (valid && mine) norm[row] = dg;
}

struct GcArgs {
  const float* a;          // rows [nrow][128]
  TileSrc b;               // f32 = columns; nrows = rows that may be read (>= the column count)
  const float* an;         // [nrow] Gram-chain norms
  const float* bn;
  int nrow, ncol;
  const int* ncol_dev;     // not null: the column count is read from here
  float thr;
  int* flag;               // NEAR [nrow]
  uint32_t* bits;          // BITS [nrow][words]
  int words;
  const int* label;        // LINK [ncol]
  int* cand;               // LINK [nrow]
  int* deg_same;           // LINKDEG [nrow]
  int* deg_cross;
  int n_r;
  const int* ida;          // DIGIT [nrow]
  const int* idb;          // DIGIT [ncol]
  unsigned long long* hist;   // DIGIT [2][GC_BINS]
  unsigned long long* zeros;  // DIGIT, null after the first digit
  int sh_pref, sh_bin;     // prefix = bits >> sh_pref (64-bit shift: 32 = no prefix), bin = (bits >> sh_bin) & bin_mask
  unsigned bin_mask, pref_a, pref_b;
};

template <int EPI>
__global__ __launch_bounds__(GC_THREADS, 2) void gc_sweep(const GcArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nrow = p.nrow;
  const int ncol = p.ncol_dev ? *p.ncol_dev : p.ncol;
  const int st_all = (ncol + BN - 1) / BN;
  const int per = (st_all + static_cast<int>(gridDim.y) - 1) / static_cast<int>(gridDim.y);
  const int st0 = static_cast<int>(blockIdx.y) * per;
  const int nst = min(per, st_all - st0);
  if (nst <= 0) return;                                   // workgroup-uniform, before any barrier
  const int wrow0 = blockIdx.x * GC_BM + wave * 32;
  const bool active = wrow0 < nrow;                       // wave-uniform; an idle wave still stages and meets the barriers

  unsigned* hist = reinterpret_cast<unsigned*>(smem + GC_LDS);
  if constexpr (EPI == GC_DIGIT) {
    for (int i = tid; i < 2 * GC_BINS; i += GC_THREADS) hist[i] = 0u;   // visible after the first stage's barrier
  }

  float4 a[16];
  {
    const float* ar = p.a + static_cast<int64_t>(min(wrow0 + r, nrow - 1)) * D + 4 * h;
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = *reinterpret_cast<const float4*>(ar + 8 * q);
  }
  float rown[16];
  int rida[16], minl[16], dsame[16], dcross[16];
  unsigned hit = 0u;
  unsigned long long zc = 0ull;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = min(wrow0 + acc_row(v, h), nrow - 1);
    rown[v] = p.an[row];
    rida[v] = EPI == GC_DIGIT ? p.ida[row] : 0;
    minl[v] = INT_MAX;
    dsame[v] = 0;
    dcross[v] = 0;
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every load above has landed before the first LDS-DMA is counted
  stage_dma<MDG_PREC_F32>(p.b, static_cast<int64_t>(st0) * BN, smem, wave, lane, GC_THREADS / 64);
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of stage s landed
    __builtin_amdgcn_s_barrier();                         // ... and everyone's; every wave finished reading stage s - 1
    if (s + 1 < nst)
      stage_dma<MDG_PREC_F32>(p.b, static_cast<int64_t>(st0 + s + 1) * BN, smem + (cur ^ 1) * STAGE_BYTES, wave, lane, GC_THREADS / 64);
    const char* lds = smem + cur * STAGE_BYTES;
    cur ^= 1;
    if (!active) continue;
    const int col0 = (st0 + s) * BN;
    float cn[2];
    int cx[2];                                            // per column: its label (LINK) or its drawn index (DIGIT)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int jc = min(col0 + 32 * t + r, ncol - 1);
      cn[t] = p.bn[jc];
      if constexpr (EPI == GC_LINK || EPI == GC_LINKDEG) cx[t] = p.label[jc];
      else if constexpr (EPI == GC_DIGIT) cx[t] = p.idb[jc];
      else cx[t] = 0;
    }
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 b = *reinterpret_cast<const float4*>(lds + tile_off<512>(32 * t + r, 2 * q + h));
        acc[t] = gram_step(a[q], b, acc[t]);
      }
    // lane (r, h) of block t holds column col0 + 32 t + r, rows wrow0 + acc_row(v, h)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = col0 + 32 * t + r;
      const bool in = col < ncol;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float d2 = gc_d2(acc[t][v], rown[v], cn[t]);
        if constexpr (EPI == GC_NEAR) {
          hit |= (in && d2 < p.thr) ? (1u << v) : 0u;
        } else if constexpr (EPI == GC_BITS) {
          const unsigned long long bal = __ballot(in && d2 < p.thr);
          const int row = wrow0 + acc_row(v, h);
          if (r == 0 && row < nrow)
            p.bits[static_cast<int64_t>(row) * p.words + (col0 >> 5) + t] = static_cast<uint32_t>(h ? (bal >> 32) : bal);
        } else if constexpr (EPI == GC_LINK || EPI == GC_LINKDEG) {
          const int row = wrow0 + acc_row(v, h);
          const bool nb = in && d2 <= p.thr && col != row;
          minl[v] = nb ? min(minl[v], cx[t]) : minl[v];
          if constexpr (EPI == GC_LINKDEG) {
            const bool same = (col < p.n_r) == (row < p.n_r);
            dsame[v] += (nb && same) ? 1 : 0;
            dcross[v] += (nb && !same) ? 1 : 0;
          }
        } else {
          if (in && wrow0 + acc_row(v, h) < nrow && rida[v] != cx[t]) {
            const unsigned u = __builtin_bit_cast(unsigned, d2);
            if (u == 0u) {
              zc += 1ull;
            } else {
              const unsigned pref = static_cast<unsigned>(static_cast<unsigned long long>(u) >> p.sh_pref);
              const unsigned bin = (u >> p.sh_bin) & p.bin_mask;
              if (pref == p.pref_a) atomicAdd(&hist[bin], 1u);
              else if (pref == p.pref_b) atomicAdd(&hist[GC_BINS + bin], 1u);
            }
          }
        }
      }
    }
  }

  if constexpr (EPI == GC_NEAR) {
    if (!active) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const unsigned long long bal = __ballot((hit >> v) & 1u);
      const unsigned mine = static_cast<unsigned>(h ? (bal >> 32) : bal);
      const int row = wrow0 + acc_row(v, h);
      if (r == 0 && mine != 0u && row < nrow) atomicOr(p.flag + row, 1);
    }
  } else if constexpr (EPI == GC_LINK || EPI == GC_LINKDEG) {
    if (!active) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      int m = minl[v], s1 = dsame[v], s2 = dcross[v];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) {                 // the 32 lanes of half h share the row
        m = min(m, __shfl_xor(m, o));
        if constexpr (EPI == GC_LINKDEG) {
          s1 += __shfl_xor(s1, o);
          s2 += __shfl_xor(s2, o);
        }
      }
      const int row = wrow0 + acc_row(v, h);
      if (r == 0 && row < nrow) {
        if (m != INT_MAX) atomicMin(p.cand + row, m);
        if constexpr (EPI == GC_LINKDEG) {
          if (s1) atomicAdd(p.deg_same + row, s1);
          if (s2) atomicAdd(p.deg_cross + row, s2);
        }
      }
    }
  } else if constexpr (EPI == GC_DIGIT) {
    __syncthreads();                                      // every wave, idle ones included, is past its last LDS add
    for (int i = tid; i < 2 * GC_BINS; i += GC_THREADS) {
      const unsigned c = hist[i];
      if (c) atomicAdd(p.hist + i, static_cast<unsigned long long>(c));
    }
    if (p.zeros) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) zc += __shfl_xor(zc, o);
      if (lane == 0 && zc) atomicAdd(p.zeros, zc);
    }
  }
}

// One workgroup per chunk: see the top of the file.  cnt rows (<= 32 words), row pitch of `bits` = words.
__global__ __launch_bounds__(GC_THREADS) void gc_resolve(const float* __restrict__ x, const float* __restrict__ xn, int64_t chunk0, int cnt,
                                                         int words, const int* __restrict__ flag, const uint32_t* __restrict__ bits,
                                                         float* __restrict__ kept_x, float* __restrict__ kept_n, int* __restrict__ kept_idx,
                                                         int* __restrict__ count) {
  __shared__ uint32_t sb[GC_CHUNK_MAX * (GC_CHUNK_MAX / 32)];
  __shared__ uint32_t skept[GC_CHUNK_MAX / 32];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < cnt * words; i += GC_THREADS) sb[i] = bits[i];
  __syncthreads();
  if (tid < 64) {
    uint32_t dropped = 0xffffffffu, kept = 0u;
    if (lane < words) {
      dropped = 0u;
      for (int b = 0; b < 32; ++b) {
        const int row = lane * 32 + b;
        if (row >= cnt || flag[row] != 0) dropped |= 1u << b;
      }
    }
    for (int i = 0; i < cnt; ++i) {
      const int w = i >> 5;
      const uint32_t dw = __shfl(dropped, w);             // wave-uniform
      if (((dw >> (i & 31)) & 1u) == 0u) {
        if (lane < words) dropped |= sb[i * words + lane];
        if (lane == w) kept |= 1u << (i & 31);
      }
    }
    if (lane < GC_CHUNK_MAX / 32) skept[lane] = lane < words ? kept : 0u;
  }
  __syncthreads();
  const int base = *count;
  const int g = tid >> 5, l = tid & 31;                   // 32 lanes copy one kept row
  for (int row = g; row < cnt; row += GC_THREADS / 32) {
    const int w = row >> 5, b = row & 31;
    const uint32_t kw = skept[w];
    if (((kw >> b) & 1u) == 0u) continue;
    int pos = base + __popc(kw & ((1u << b) - 1u));
    for (int ww = 0; ww < w; ++ww) pos += __popc(skept[ww]);
    const int64_t src = chunk0 + row;
    reinterpret_cast<float4*>(kept_x + static_cast<int64_t>(pos) * D)[l] = reinterpret_cast<const float4*>(x + src * D)[l];
    if (l == 0) {
      kept_n[pos] = xn[src];
      kept_idx[pos] = static_cast<int>(src);
    }
  }
  __syncthreads();                                        // every thread has read *count
  if (tid == 0) {
    int total = 0;
    for (int ww = 0; ww < words; ++ww) total += __popc(skept[ww]);
    *count = base + total;
  }
}

__global__ __launch_bounds__(GC_THREADS) void gc_iota(int* __restrict__ label, int n) {
  const int i = blockIdx.x * GC_THREADS + threadIdx.x;
  if (i < n) label[i] = i;
}

// label (a snapshot: every entry is a root) and cand are read only; next starts as a copy of label.
__global__ __launch_bounds__(GC_THREADS) void gc_hook(const int* __restrict__ label, const int* __restrict__ cand, int* __restrict__ next,
                                                      int n, int* __restrict__ changed) {
  const int i = blockIdx.x * GC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int l = label[i], c = cand[i];
  if (c < l) {
    atomicMin(next + l, c);
    *changed = 1;
  }
}

// next[x] <= x everywhere, so every chain ends at a root (next[r] == r), and a root is never written here: whatever a racing
// reader sees, old pointer or root, leads to the same root.
__global__ __launch_bounds__(GC_THREADS) void gc_jump(int* next, int n) {
  const int i = blockIdx.x * GC_THREADS + threadIdx.x;
  if (i >= n) return;
  int l = __atomic_load_n(next + i, __ATOMIC_RELAXED);
  for (;;) {
    const int q = __atomic_load_n(next + l, __ATOMIC_RELAXED);
    if (q == l) break;
    l = q;
  }
  __atomic_store_n(next + i, l, __ATOMIC_RELAXED);
}

template <int EPI>
void gc_launch(const GcArgs& a, int64_t row_blocks, int S, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(row_blocks), static_cast<unsigned>(S));
  const int lds = GC_LDS + (EPI == GC_DIGIT ? GC_HIST_LDS : 0);
  if constexpr (EPI == GC_DIGIT) {
    static bool once = false;
    if (!once) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gc_sweep<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      once = true;
    }
  }
  hipLaunchKernelGGL((gc_sweep<EPI>), grid, dim3(GC_THREADS), lds, st, a);
}

int gc_segments(int64_t nrow, int64_t ncol, int segments) {
  const int64_t tiles = mdg_cdiv(ncol, 2 * BN);
  int64_t S = segments;
  if (S < 1) {
    const int64_t blocks = mdg_cdiv(nrow, GC_BM), want = 2 * GC_CUS;
    S = blocks >= want ? 1 : mdg_cdiv(want, blocks);
  }
  if (S > tiles) S = tiles;
  if (S > 65535) S = 65535;
  return static_cast<int>(S < 1 ? 1 : S);
}

GcArgs gc_args(const float* a, const float* an, int64_t nrow, const float* b, const float* bn, int64_t ncol, int64_t bcap, float thr) {
  GcArgs p{};
  p.a = a;
  p.b = TileSrc{b, nullptr, nullptr, bcap};
  p.an = an;
  p.bn = bn;
  p.nrow = static_cast<int>(nrow);
  p.ncol = static_cast<int>(ncol);
  p.thr = thr;
  return p;
}

constexpr int64_t GC_MAX_ROWS = (int64_t(1) << 31) - GC_BM - 1;

size_t gc_align(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

bool gc_chunk_ok(int chunk) { return chunk >= 128 && chunk <= GC_CHUNK_MAX && chunk % 128 == 0; }

}  // namespace

extern "C" int mdg_geomca_default_chunk(void) { return GC_CHUNK_DEFAULT; }

extern "C" int mdg_geomca_default_segments(int64_t nrow, int64_t ncol) {
  if (nrow < 1 || ncol < 1) return 1;
  return gc_segments(nrow, ncol, 0);
}

extern "C" int mdg_geomca_prep(const float* x, int64_t n, int64_t d, float* norms, int* status, void* stream) {
  MDG_CHECK_ARG(d == D, "mdg_geomca_prep: only D = %d is supported (got %lld)", D, (long long)d);
  MDG_CHECK_ARG(n >= 1 && n <= GC_MAX_ROWS, "mdg_geomca_prep: need 1 <= n < 2^31 - 128 (got %lld)", (long long)n);
  MDG_CHECK_ARG(x && norms && status, "mdg_geomca_prep: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(x), "mdg_geomca_prep: x must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_geomca_prep: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  hipLaunchKernelGGL(gc_prep, dim3(static_cast<unsigned>(mdg_cdiv(mdg_cdiv(n, 32), GC_THREADS / 64))), dim3(GC_THREADS), 0, st, x,
                     static_cast<int>(n), norms, status);
  MDG_CHECK_LAUNCH("gc_prep");
  return MDG_OK;
}

// workspace: kept rows [n][128], kept norms [n], near flags [chunk], bit matrix [chunk][chunk / 32]
extern "C" size_t mdg_geomca_sparsify_workspace_bytes(int64_t n, int chunk) {
  if (n < 1 || !gc_chunk_ok(chunk)) return 0;
  return gc_align(static_cast<size_t>(n) * D * 4) + gc_align(static_cast<size_t>(n) * 4) + gc_align(static_cast<size_t>(chunk) * 4) +
         gc_align(static_cast<size_t>(chunk) * (chunk / 32) * 4);
}

extern "C" int mdg_geomca_sparsify(const float* x, int64_t n, int64_t d, const float* norms, float delta2, int chunk, int segments,
                                   int32_t* kept_idx, int* count, void* workspace, size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(d == D, "mdg_geomca_sparsify: only D = %d is supported (got %lld)", D, (long long)d);
  MDG_CHECK_ARG(n >= 1 && n <= GC_MAX_ROWS, "mdg_geomca_sparsify: need 1 <= n < 2^31 - 128 (got %lld)", (long long)n);
  MDG_CHECK_ARG(gc_chunk_ok(chunk), "mdg_geomca_sparsify: chunk must be a multiple of 128 in 128..%d (got %d)", GC_CHUNK_MAX, chunk);
  MDG_CHECK_ARG(segments >= 0, "mdg_geomca_sparsify: segments must be at least 1, or 0 for the default (got %d)", segments);
  MDG_CHECK_ARG(delta2 == delta2 && delta2 >= 0.f, "mdg_geomca_sparsify: delta^2 must be a number >= 0");
  MDG_CHECK_ARG(x && norms && kept_idx && count, "mdg_geomca_sparsify: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(x), "mdg_geomca_sparsify: x must be 16-byte aligned");
  const size_t need = mdg_geomca_sparsify_workspace_bytes(n, chunk);
  if (!workspace || workspace_bytes < need || !mdg_aligned16(workspace)) {
    mdg_set_error("mdg_geomca_sparsify: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  float* kept_x = reinterpret_cast<float*>(w);
  w += gc_align(static_cast<size_t>(n) * D * 4);
  float* kept_n = reinterpret_cast<float*>(w);
  w += gc_align(static_cast<size_t>(n) * 4);
  int* flag = reinterpret_cast<int*>(w);
  w += gc_align(static_cast<size_t>(chunk) * 4);
  uint32_t* bits = reinterpret_cast<uint32_t*>(w);
  const int words = chunk / 32;
  if (hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_geomca_sparsify: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t cnt = n - c0 < chunk ? n - c0 : chunk;
    if (hipMemsetAsync(flag, 0, static_cast<size_t>(chunk) * 4, st) != hipSuccess) {
      mdg_set_error("mdg_geomca_sparsify: hipMemsetAsync failed");
      return MDG_ELAUNCH;
    }
    const int64_t blocks = mdg_cdiv(cnt, GC_BM);
    if (c0 > 0) {                                         // nothing is kept before the first chunk
      GcArgs a = gc_args(x + c0 * D, norms + c0, cnt, kept_x, kept_n, 0, n, delta2);
      a.ncol_dev = count;
      a.flag = flag;
      gc_launch<GC_NEAR>(a, blocks, gc_segments(cnt, c0, segments), st);
    }
    GcArgs b = gc_args(x + c0 * D, norms + c0, cnt, x + c0 * D, norms + c0, cnt, cnt, delta2);
    b.bits = bits;
    b.words = words;
    gc_launch<GC_BITS>(b, blocks, gc_segments(cnt, cnt, segments), st);
    hipLaunchKernelGGL(gc_resolve, dim3(1), dim3(GC_THREADS), 0, st, x, norms, c0, static_cast<int>(cnt), words, flag, bits, kept_x,
                       kept_n, kept_idx, count);
  }
  MDG_CHECK_LAUNCH("mdg_geomca_sparsify");
  return MDG_OK;
}

// workspace: cand [n], next [n], changed [1]
extern "C" size_t mdg_geomca_components_workspace_bytes(int64_t n) {
  if (n < 1) return 0;
  return 2 * gc_align(static_cast<size_t>(n) * 4) + 256;
}

extern "C" int mdg_geomca_components(const float* v, int64_t n, int64_t n_r, int64_t d, const float* norms, float eps2, int segments,
                                     int32_t* label, int32_t* deg_same, int32_t* deg_cross, int* sweeps_host, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(d == D, "mdg_geomca_components: only D = %d is supported (got %lld)", D, (long long)d);
  MDG_CHECK_ARG(n >= 1 && n <= GC_MAX_ROWS, "mdg_geomca_components: need 1 <= n < 2^31 - 128 (got %lld)", (long long)n);
  MDG_CHECK_ARG(n_r >= 0 && n_r <= n, "mdg_geomca_components: need 0 <= n_r <= n (got %lld of %lld)", (long long)n_r, (long long)n);
  MDG_CHECK_ARG(segments >= 0, "mdg_geomca_components: segments must be at least 1, or 0 for the default (got %d)", segments);
  MDG_CHECK_ARG(eps2 == eps2 && eps2 >= 0.f, "mdg_geomca_components: epsilon^2 must be a number >= 0");
  MDG_CHECK_ARG(v && norms && label && deg_same && deg_cross && sweeps_host, "mdg_geomca_components: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(v), "mdg_geomca_components: v must be 16-byte aligned");
  const size_t need = mdg_geomca_components_workspace_bytes(n);
  if (!workspace || workspace_bytes < need || !mdg_aligned16(workspace)) {
    mdg_set_error("mdg_geomca_components: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  int* cand = reinterpret_cast<int*>(w);
  w += gc_align(static_cast<size_t>(n) * 4);
  int* next = reinterpret_cast<int*>(w);
  w += gc_align(static_cast<size_t>(n) * 4);
  int* changed = reinterpret_cast<int*>(w);
  const size_t nb = static_cast<size_t>(n) * 4;
  const unsigned eb = static_cast<unsigned>(mdg_cdiv(n, GC_THREADS));
  const int S = gc_segments(n, n, segments);
  bool okay = hipMemsetAsync(deg_same, 0, nb, st) == hipSuccess && hipMemsetAsync(deg_cross, 0, nb, st) == hipSuccess;
  hipLaunchKernelGGL(gc_iota, dim3(eb), dim3(GC_THREADS), 0, st, label, static_cast<int>(n));
  int sweeps = 0;
  for (;;) {
    okay = okay && hipMemcpyAsync(cand, label, nb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
           hipMemcpyAsync(next, label, nb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
           hipMemsetAsync(changed, 0, sizeof(int), st) == hipSuccess;
    if (!okay) break;
    GcArgs a = gc_args(v, norms, n, v, norms, n, n, eps2);
    a.label = label;
    a.cand = cand;
    a.deg_same = deg_same;
    a.deg_cross = deg_cross;
    a.n_r = static_cast<int>(n_r);
    if (sweeps == 0) gc_launch<GC_LINKDEG>(a, mdg_cdiv(n, GC_BM), S, st);
    else gc_launch<GC_LINK>(a, mdg_cdiv(n, GC_BM), S, st);
    hipLaunchKernelGGL(gc_hook, dim3(eb), dim3(GC_THREADS), 0, st, label, cand, next, static_cast<int>(n), changed);
    hipLaunchKernelGGL(gc_jump, dim3(eb), dim3(GC_THREADS), 0, st, next, static_cast<int>(n));
    int host_changed = 0;
    okay = hipMemcpyAsync(label, next, nb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
           hipMemcpyAsync(&host_changed, changed, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess;
    ++sweeps;
    if (!okay || !host_changed) break;
    if (sweeps >= GC_MAX_SWEEPS) {
      mdg_set_error("mdg_geomca_components: no fixed point after %d sweeps", sweeps);
      return MDG_ELAUNCH;
    }
  }
  if (!okay) {
    mdg_set_error("mdg_geomca_components: a copy, memset or synchronisation failed: %s", hipGetErrorString(hipGetLastError()));
    return MDG_ELAUNCH;
  }
  MDG_CHECK_LAUNCH("mdg_geomca_components");
  *sweeps_host = sweeps;
  return MDG_OK;
}

// workspace: hist [2][GC_BINS] uint64, zeros [1] uint64
extern "C" size_t mdg_geomca_distance_select_workspace_bytes(void) { return (2 * GC_BINS + 1) * sizeof(unsigned long long); }

extern "C" int mdg_geomca_distance_select(const float* x, const float* y, const int32_t* ids_x, const int32_t* ids_y, int64_t mx, int64_t my,
                                          int64_t d, const float* x_norms, const float* y_norms, double percentile, int segments,
                                          int64_t* counts_host, double* values_host, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  MDG_CHECK_ARG(d == D, "mdg_geomca_distance_select: only D = %d is supported (got %lld)", D, (long long)d);
  MDG_CHECK_ARG(mx >= 1 && mx <= GC_MAX_ROWS && my >= 1 && my <= GC_MAX_ROWS, "mdg_geomca_distance_select: need 1 <= rows < 2^31 - 128 (got %lld, %lld)",
                (long long)mx, (long long)my);
  MDG_CHECK_ARG(percentile >= 0.0 && percentile <= 100.0, "mdg_geomca_distance_select: percentile must lie in [0, 100]");
  MDG_CHECK_ARG(segments >= 0, "mdg_geomca_distance_select: segments must be at least 1, or 0 for the default (got %d)", segments);
  MDG_CHECK_ARG(x && y && ids_x && ids_y && x_norms && y_norms && counts_host && values_host, "mdg_geomca_distance_select: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(x) && mdg_aligned16(y), "mdg_geomca_distance_select: x and y must be 16-byte aligned");
  const size_t need = mdg_geomca_distance_select_workspace_bytes();
  if (!workspace || workspace_bytes < need || !mdg_aligned16(workspace)) {
    mdg_set_error("mdg_geomca_distance_select: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* hist = static_cast<unsigned long long*>(workspace);
  unsigned long long* zeros = hist + 2 * GC_BINS;
  static const int SH_BIN[3] = {21, 10, 0}, SH_PREF[3] = {32, 21, 10};
  static const unsigned MASK[3] = {2047u, 2047u, 1023u};
  unsigned long long host[2 * GC_BINS + 1];
  unsigned long long zero_count = 0, M = 0, rank[2] = {0, 0};
  unsigned pref[2] = {0u, 0u};
  double pos = 0.0;
  const int S = gc_segments(mx, my, segments);
  for (int pass = 0; pass < 3; ++pass) {
    if (hipMemsetAsync(hist, 0, need, st) != hipSuccess) {
      mdg_set_error("mdg_geomca_distance_select: hipMemsetAsync failed");
      return MDG_ELAUNCH;
    }
    GcArgs a = gc_args(x, x_norms, mx, y, y_norms, my, my, 0.f);
    a.ida = ids_x;
    a.idb = ids_y;
    a.hist = hist;
    a.zeros = pass == 0 ? zeros : nullptr;
    a.sh_pref = SH_PREF[pass];
    a.sh_bin = SH_BIN[pass];
    a.bin_mask = MASK[pass];
    a.pref_a = pref[0];
    a.pref_b = pref[0] == pref[1] ? 0xffffffffu : pref[1];   // one histogram while both ranks share the prefix (no prefix has 32 bits set)
    gc_launch<GC_DIGIT>(a, mdg_cdiv(mx, GC_BM), S, st);
    MDG_CHECK_LAUNCH("gc_sweep<digit>");
    if (hipMemcpyAsync(host, hist, need, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      mdg_set_error("mdg_geomca_distance_select: reading the histogram failed: %s", hipGetErrorString(hipGetLastError()));
      return MDG_ELAUNCH;
    }
    if (pass == 0) {
      zero_count = host[2 * GC_BINS];
      for (int b = 0; b < GC_BINS; ++b) M += host[b];
      if (M == 0) break;
      pos = percentile / 100.0 * static_cast<double>(M - 1);
      rank[0] = static_cast<unsigned long long>(pos);
      rank[1] = rank[0] + 1 < M ? rank[0] + 1 : M - 1;
    }
    const bool shared = pref[0] == pref[1];
    for (int q = 0; q < 2; ++q) {
      const unsigned long long* hq = host + ((q == 1 && !shared) ? GC_BINS : 0);
      unsigned long long cum = 0;
      unsigned b = 0;
      for (; b <= MASK[pass]; ++b) {
        if (rank[q] < cum + hq[b]) break;
        cum += hq[b];
      }
      if (b > MASK[pass]) {
        mdg_set_error("mdg_geomca_distance_select: rank outside the histogram (digit %d)", pass);
        return MDG_ELAUNCH;
      }
      rank[q] -= cum;
      pref[q] = (pass == 0 ? 0u : pref[q] << (pass == 2 ? 10 : 11)) | b;
    }
  }
  counts_host[0] = static_cast<int64_t>(zero_count);
  counts_host[1] = static_cast<int64_t>(M);
  float lo = 0.f, hi = 0.f;
  if (M) {
    lo = __builtin_bit_cast(float, pref[0]);
    hi = __builtin_bit_cast(float, pref[1]);
  }
  values_host[0] = lo;
  values_host[1] = hi;
  values_host[2] = pos;
  return MDG_OK;
}
