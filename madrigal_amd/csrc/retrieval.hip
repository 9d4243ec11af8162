// Cross-modal retrieval metrics of contrastive pretraining for gfx950: match counts and uniformity.
//
// Replaces the CPU torch metrics of pretraining evaluation (madrigal/evaluate/evaluate.py:406-450 get_inst_dist_topk_accuracy,
// madrigal/evaluate/eval_utils.py:147-156 uniform_loss / alignment_loss, :159-174 stacked_inst_dist_topk_accuracy, :232-247
// foscttm).  Each of them is an all-pairs sweep over [n,128] fp32 embeddings whose epilogue compares an entry with its row's
// or column's true match (the diagonal) or sums a function of it.
//
// mdg_pair_match_counts (X, Y [n,128]):
//   rt_prep      per row: |x|^2, |y|^2, 1/|x|, 1/|y|, the diagonal g_ii = x_i.y_i (computed by the same MFMA chain as the
//                tiles, so a competitor equal to the true match compares equal), the thresholds
//                cthr_i = (g_ii/|x_i|)/|y_i|, drow_i = |y_i|^2 - 2 g_ii, dcol_i = |x_i|^2 - 2 g_ii, the alignment term
//                |x^_i - y^_i|^2, and the NaN / inf / zero-norm status bits
//   rt_tile<0>   G = X Y^T in full, 128 x 128 tiles: cosine and distance tests against the row's and the column's threshold
//   rt_tile<1>   upper triangles of X X^T and Y Y^T: each entry counted for its row and its column (stacked top-k)
//   rt_reduce    sums the per-tile partial counts (a [6][T][n] int32 slab, every entry written once: no atomics)
// mdg_pair_uniformity (X [m,128]):
//   rt_prep<false>, rt_tile<2> (upper triangle, exp(-t (2 - 2 cos)) summed in fp32 per tile, one double per tile),
//   rt_uniform_final (fixed-order fp64 sum, log of the mean).
//
// Numerics: products on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma chain per entry: every entry, the diagonal's
// included, sees the same sequence).  A tile computes g once; cos = (g / |x_i|) / |y_j| as (g * rx_i) * ry_j, and the
// distance test |x_j - y_i|^2 < |x_i - y_i|^2 as fmaf(-2, g_ji, |x_j|^2) < fmaf(-2, g_ii, |x_i|^2) (|y_i|^2 cancels).
// Ties with the true match do not count against it (strict > and <: "ties count as hits"); the true match itself is
// excluded by index.  Counts are integers summed without atomics, so every output is bit-identical from run to run.
#include "gram.h"               // gram_step, norm2_step, finite4: shared with knn.hip

namespace {

constexpr int RT_D = 128;            // embedding width of every shipped config
constexpr int RT_BT = 128;           // tile edge (rows and columns)
constexpr int RT_THREADS = 256;      // 4 waves, 2 x 2 over the tile, 64 x 64 each (2 x 2 MFMA blocks of 32 x 32)
constexpr int RT_NCOUNT = 6;         // cos_row, cos_col, dist_row, dist_col, same_x, same_y

enum { RT_CROSS = 0, RT_SAME = 1, RT_UNIFORM = 2 };

__device__ __forceinline__ int acc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

struct RtParams {   // per-row quantities of the pre-pass, [n] each
  float *rx, *ry, *nx2, *ny2, *cthr, *drow, *dcol;
};

// One wave per 32 rows: lane (r, h) reads half h of row r0 + r.  HAS_Y: X and Y (counts); otherwise X alone (uniformity).
template <bool HAS_Y>
__global__ __launch_bounds__(RT_THREADS) void rt_prep(const float* __restrict__ x, const float* __restrict__ y, int n, RtParams p,
                                                      float* __restrict__ align, int* __restrict__ status) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int r0 = (blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6)) * 32;
  if (r0 >= n) return;
  const int row = min(r0 + r, n - 1);
  const float* xr = x + static_cast<int64_t>(row) * RT_D;
  const float* yr = HAS_Y ? y + static_cast<int64_t>(row) * RT_D : xr;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  float sx = 0.f, sy = 0.f;
  bool ok = true;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const float4 a = *reinterpret_cast<const float4*>(xr + 8 * q + 4 * h);
    ok = ok && finite4(a);
    sx = norm2_step(a, sx);
    if constexpr (HAS_Y) {
      const float4 b = *reinterpret_cast<const float4*>(yr + 8 * q + 4 * h);
      ok = ok && finite4(b);
      sy = norm2_step(b, sy);
      acc = gram_step(a, b, acc);
    }
  }
  const float nx2 = sx + __shfl_xor(sx, 32);            // the same sum in both halves (fp32 addition commutes)
  const float rx = 1.0f / sqrtf(nx2);
  const bool valid = r0 + r < n;
  int bad = (!ok || !isfinite(nx2)) ? 1 : 0;
  if (!(nx2 > 0.f)) bad |= 2;
  float ny2 = 0.f, ry = 0.f, gii = 0.f, al = 0.f;
  if constexpr (HAS_Y) {
    ny2 = sy + __shfl_xor(sy, 32);
    ry = 1.0f / sqrtf(ny2);
    if (!isfinite(ny2)) bad |= 1;
    if (!(ny2 > 0.f)) bad |= 2;
    // g_ii of column c = r sits in lane c + 32 * ((c >> 2) & 1), register (c & 3) + 4 (c >> 3)
    const int vd = (r & 3) + 4 * (r >> 3);
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) d = (v == vd) ? acc[v] : d;
    const float other = __shfl_xor(d, 32);
    gii = (((r >> 2) & 1) == h) ? d : other;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(xr + 8 * q + 4 * h);
      const float4 b = *reinterpret_cast<const float4*>(yr + 8 * q + 4 * h);
      float t;
      t = a.x * rx - b.x * ry; al = fmaf(t, t, al);
      t = a.y * rx - b.y * ry; al = fmaf(t, t, al);
      t = a.z * rx - b.z * ry; al = fmaf(t, t, al);
      t = a.w * rx - b.w * ry; al = fmaf(t, t, al);
    }
    al = al + __shfl_xor(al, 32);
  }
  if (valid && bad) atomicOr(status, bad);
  if (valid && h == 0) {
    p.rx[row] = rx;
    p.nx2[row] = nx2;
    if constexpr (HAS_Y) {
      p.ry[row] = ry;
      p.ny2[row] = ny2;
      p.cthr[row] = (gii * rx) * ry;
      p.drow[row] = fmaf(-2.0f, gii, ny2);
      p.dcol[row] = fmaf(-2.0f, gii, nx2);
      align[row] = al;
    }
  }
}

struct RtTileArgs {
  const float* a;          // row operand (X)
  const float* b;          // column operand (Y for RT_CROSS, else A itself)
  RtParams p;
  int n, T;
  int* slab;               // RT_CROSS / RT_SAME: [6][T][n] int32 partial counts
  double* uslab;           // RT_UNIFORM: [T (T + 1) / 2] per-tile sums
  const float* b_alt;      // RT_SAME: the second matrix (blockIdx.y == 1: Y Y^T with 1/|y|)
  float t;                 // RT_UNIFORM: temperature
};

// (I, J), J >= I, of upper-triangle tile t (row-major over J, then I)
__device__ __forceinline__ void tri_decode(int t, int& I, int& J) {
  int r = static_cast<int>((sqrtf(8.0f * static_cast<float>(t) + 1.0f) - 1.0f) * 0.5f);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  J = r;
  I = t - r * (r + 1) / 2;
}

template <int EPI>
__global__ __launch_bounds__(RT_THREADS, 2) void rt_tile(const RtTileArgs args) {
  __shared__ float4 rowp[RT_BT];                 // per tile row: {scale, cosine threshold, distance threshold, |row|^2}
  __shared__ int red_row[2][2][RT_BT];           // [column half of the wave][count kind][row]
  __shared__ int red_col[2][2][RT_BT];           // [row half of the wave][count kind][column]
  __shared__ float red_u[RT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int n = args.n;
  int I, J;
  if constexpr (EPI == RT_CROSS) {
    I = blockIdx.y;
    J = blockIdx.x;
  } else {
    tri_decode(blockIdx.x, I, J);
  }
  const bool second = EPI == RT_SAME && blockIdx.y == 1;
  const float* A = second ? args.b_alt : args.a;
  const float* B = EPI == RT_CROSS ? args.b : A;
  const float* rscale = second ? args.p.ry : args.p.rx;                  // row side: 1/|x| (or 1/|y|)
  const float* cscale = EPI == RT_CROSS ? args.p.ry : rscale;            // column side
  const int row0 = I * RT_BT, col0 = J * RT_BT;

  if (tid < RT_BT) {
    const int i = min(row0 + tid, n - 1);
    float4 v;
    v.x = rscale[i];
    v.y = EPI == RT_UNIFORM ? 0.f : args.p.cthr[i];
    v.z = EPI == RT_CROSS ? args.p.drow[i] : 0.f;
    v.w = EPI == RT_CROSS ? args.p.nx2[i] : 0.f;
    rowp[tid] = v;
  }

  // ---- G tile: 2 x 2 blocks of 32 x 32 per wave, operands straight from global (L2 / L1), one k step prefetched
  const float* arow[2];
  const float* brow[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    arow[s] = A + static_cast<int64_t>(min(row0 + 64 * wr + 32 * s + r, n - 1)) * RT_D + 4 * h;
    brow[s] = B + static_cast<int64_t>(min(col0 + 64 * wc + 32 * s + r, n - 1)) * RT_D + 4 * h;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
  float4 ca[2], cb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    ca[s] = *reinterpret_cast<const float4*>(arow[s]);
    cb[s] = *reinterpret_cast<const float4*>(brow[s]);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    float4 na[2], nb[2];
    if (q < 15) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        na[s] = *reinterpret_cast<const float4*>(arow[s] + 8 * (q + 1));
        nb[s] = *reinterpret_cast<const float4*>(brow[s] + 8 * (q + 1));
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = gram_step(ca[a], cb[b], acc[a][b]);
    if (q < 15) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        ca[s] = na[s];
        cb[s] = nb[s];
      }
    }
  }
  __syncthreads();                               // rowp is written

  // ---- epilogue.  Lane (r, h) of block (a, b) holds column j = col0 + 64 wc + 32 b + r, rows i = row0 + 64 wr + 32 a + acc_row(v, h).
  int jcol[2];
  float cs[2], cth[2], cd[2], cn2[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    jcol[b] = col0 + 64 * wc + 32 * b + r;
    const int jc = min(jcol[b], n - 1);
    cs[b] = cscale[jc];
    cth[b] = EPI == RT_UNIFORM ? 0.f : args.p.cthr[jc];
    cd[b] = EPI == RT_CROSS ? args.p.dcol[jc] : 0.f;
    cn2[b] = EPI == RT_CROSS ? args.p.ny2[jc] : 0.f;
  }
  if constexpr (EPI == RT_UNIFORM) {
    const float nt = -args.t;
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int li = 64 * wr + 32 * a + acc_row(v, h);
        const int i = row0 + li;
        const float rs = rowp[li].x;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float c = (acc[a][b][v] * rs) * cs[b];
          const float d2 = fmaxf(2.0f - 2.0f * c, 0.0f);
          const float e = expf(nt * d2);
          sum += (i < n && jcol[b] < n && jcol[b] > i) ? e : 0.f;
        }
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) red_u[wave] = sum;
    __syncthreads();
    if (tid == 0) {
      const float tile_sum = (red_u[0] + red_u[1]) + (red_u[2] + red_u[3]);
      args.uslab[blockIdx.x] = static_cast<double>(tile_sum);
    }
    return;
  } else {
    // row counts: ballot per register (lanes 0..31 -> row acc_row(v, 0), lanes 32..63 -> acc_row(v, 1)), lane r < 32 collects row r
    int rc0[2] = {0, 0}, rc1[2] = {0, 0};        // [a]: cosine (or same-view) / distance row counts
    int cc0[2] = {0, 0}, cc1[2] = {0, 0};        // [b]: column counts
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int li = 64 * wr + 32 * a + acc_row(v, h);
        const int i = row0 + li;
        const float4 rp = rowp[li];
        int pc0 = 0, pc1 = 0, pd0 = 0, pd1 = 0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float g = acc[a][b][v];
          const int j = jcol[b];
          const bool ok = EPI == RT_CROSS ? (i < n && j < n && i != j) : (i < n && j < n && j > i);
          const float c = (g * rp.x) * cs[b];
          const bool crow = ok && c > rp.y;      // competitor j beats row i's true match
          const bool ccol = ok && c > cth[b];    // competitor i beats column j's true match
          const uint64_t mr = __ballot(crow);
          pc0 += __popcll(mr & 0xFFFFFFFFull);
          pc1 += __popcll(mr >> 32);
          cc0[b] += ccol ? 1 : 0;
          if constexpr (EPI == RT_CROSS) {
            const bool drw = ok && fmaf(-2.0f, g, cn2[b]) < rp.z;   // |x_i - y_j| < |x_i - y_i|
            const bool dcl = ok && fmaf(-2.0f, g, rp.w) < cd[b];    // |x_i - y_j| < |x_j - y_j|
            const uint64_t md = __ballot(drw);
            pd0 += __popcll(md & 0xFFFFFFFFull);
            pd1 += __popcll(md >> 32);
            cc1[b] += dcl ? 1 : 0;
          }
        }
        const int R0 = acc_row(v, 0), R1 = R0 + 4;
        rc0[a] += (lane == R0) ? pc0 : ((lane == R1) ? pc1 : 0);
        if constexpr (EPI == RT_CROSS) rc1[a] += (lane == R0) ? pd0 : ((lane == R1) ? pd1 : 0);
      }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      cc0[b] += __shfl_xor(cc0[b], 32);
      cc1[b] += __shfl_xor(cc1[b], 32);
    }
    if (lane < 32) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        red_row[wc][0][64 * wr + 32 * a + lane] = rc0[a];
        red_row[wc][1][64 * wr + 32 * a + lane] = rc1[a];
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        red_col[wr][0][64 * wc + 32 * b + lane] = cc0[b];
        red_col[wr][1][64 * wc + 32 * b + lane] = cc1[b];
      }
    }
    __syncthreads();
    // slab kinds: 0 cos_row, 1 cos_col, 2 dist_row, 3 dist_col, 4 same_x, 5 same_y; slab[kind][t][i] with t the other block
    const int64_t nn = n, TT = args.T;
    const int idx = tid & (RT_BT - 1), kind = tid >> 7;
    if constexpr (EPI == RT_CROSS) {
      const int rsum = red_row[0][kind][idx] + red_row[1][kind][idx];
      const int csum = red_col[0][kind][idx] + red_col[1][kind][idx];
      int* s_row = args.slab + (2 * kind) * TT * nn;        // cos_row / dist_row
      int* s_col = args.slab + (2 * kind + 1) * TT * nn;    // cos_col / dist_col
      if (row0 + idx < n) s_row[J * nn + row0 + idx] = rsum;
      if (col0 + idx < n) s_col[I * nn + col0 + idx] = csum;
    } else {
      int* s = args.slab + (second ? 5 : 4) * TT * nn;
      const int rsum = red_row[0][0][idx] + red_row[1][0][idx];
      const int csum = red_col[0][0][idx] + red_col[1][0][idx];
      if (I == J) {
        if (kind == 0 && row0 + idx < n) s[I * nn + row0 + idx] = rsum + csum;
      } else if (kind == 0) {
        if (row0 + idx < n) s[J * nn + row0 + idx] = rsum;
      } else {
        if (col0 + idx < n) s[I * nn + col0 + idx] = csum;
      }
    }
  }
}

__global__ __launch_bounds__(RT_THREADS) void rt_reduce(const int* __restrict__ slab, int n, int T, int* cos_row, int* cos_col,
                                                        int* dist_row, int* dist_col, int* same_x, int* same_y) {
  const int i = blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= n) return;
  int* const outs[RT_NCOUNT] = {cos_row, cos_col, dist_row, dist_col, same_x, same_y};
  const int64_t nn = n;
#pragma unroll
  for (int k = 0; k < RT_NCOUNT; ++k) {
    const int* s = slab + k * static_cast<int64_t>(T) * nn + i;
    int c = 0;
    for (int t = 0; t < T; ++t) c += s[t * nn];
    outs[k][i] = c;
  }
}

__global__ __launch_bounds__(RT_THREADS) void rt_uniform_final(const double* __restrict__ uslab, int n_tiles, int64_t m,
                                                               float* __restrict__ out) {
  __shared__ double red[RT_THREADS];
  double s = 0.0;
  for (int t = threadIdx.x; t < n_tiles; t += RT_THREADS) s += uslab[t];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = RT_THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double pairs = 0.5 * static_cast<double>(m) * static_cast<double>(m - 1);
    out[0] = static_cast<float>(log(red[0] / pairs));
  }
}

struct RtLayout {
  size_t params, slab, total;
};

RtLayout rt_layout(int64_t n, bool counts) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const int64_t T = mdg_cdiv(n, RT_BT);
  RtLayout o;
  o.params = 0;
  size_t off = al(sizeof(float) * 7 * n);
  o.slab = off;
  off += counts ? al(sizeof(int) * RT_NCOUNT * T * n) : al(sizeof(double) * (T * (T + 1) / 2));
  o.total = off;
  return o;
}

RtParams rt_params(char* ws, int64_t n) {
  float* f = reinterpret_cast<float*>(ws);
  return RtParams{f, f + n, f + 2 * n, f + 3 * n, f + 4 * n, f + 5 * n, f + 6 * n};
}

constexpr int64_t RT_MAX_ROWS = 65536;

}  // namespace

extern "C" size_t mdg_pair_match_counts_workspace_bytes(int64_t n) {
  if (n <= 0 || n > RT_MAX_ROWS) return 0;
  return rt_layout(n, true).total;
}

extern "C" int mdg_pair_match_counts(const float* x, const float* y, int64_t n, int64_t d, int* cos_row, int* cos_col, int* same_x,
                                     int* same_y, int* dist_row, int* dist_col, float* align, int* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n >= 1 && n <= RT_MAX_ROWS, "mdg_pair_match_counts: need 1 <= n <= %lld (got %lld)", (long long)RT_MAX_ROWS,
                (long long)n);
  MDG_CHECK_ARG(d == RT_D, "mdg_pair_match_counts: only D = %d is supported (got %lld)", RT_D, (long long)d);
  MDG_CHECK_ARG(x && y && cos_row && cos_col && same_x && same_y && dist_row && dist_col && align && status,
                "mdg_pair_match_counts: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(x) && mdg_aligned16(y), "mdg_pair_match_counts: x and y must be 16-byte aligned");
  const RtLayout lay = rt_layout(n, true);
  if (!workspace || workspace_bytes < lay.total) {
    mdg_set_error("mdg_pair_match_counts: workspace of %zu bytes needed", lay.total);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const RtParams prm = rt_params(ws + lay.params, n);
  const int T = static_cast<int>(mdg_cdiv(n, RT_BT));
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_pair_match_counts: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  const int waves = static_cast<int>(mdg_cdiv(n, 32));
  hipLaunchKernelGGL(rt_prep<true>, dim3(static_cast<unsigned>(mdg_cdiv(waves, RT_THREADS / 64))), dim3(RT_THREADS), 0, st, x, y,
                     static_cast<int>(n), prm, align, status);
  MDG_CHECK_LAUNCH("rt_prep");
  RtTileArgs a{x, y, prm, static_cast<int>(n), T, reinterpret_cast<int*>(ws + lay.slab), nullptr, y, 0.f};
  hipLaunchKernelGGL(rt_tile<RT_CROSS>, dim3(T, T), dim3(RT_THREADS), 0, st, a);
  MDG_CHECK_LAUNCH("rt_tile<cross>");
  hipLaunchKernelGGL(rt_tile<RT_SAME>, dim3(T * (T + 1) / 2, 2), dim3(RT_THREADS), 0, st, a);
  MDG_CHECK_LAUNCH("rt_tile<same>");
  hipLaunchKernelGGL(rt_reduce, dim3(static_cast<unsigned>(mdg_cdiv(n, RT_THREADS))), dim3(RT_THREADS), 0, st,
                     reinterpret_cast<const int*>(ws + lay.slab), static_cast<int>(n), T, cos_row, cos_col, dist_row, dist_col, same_x,
                     same_y);
  MDG_CHECK_LAUNCH("rt_reduce");
  return MDG_OK;
}

extern "C" size_t mdg_pair_uniformity_workspace_bytes(int64_t m) {
  if (m < 2 || m > RT_MAX_ROWS) return 0;
  return rt_layout(m, false).total;
}

extern "C" int mdg_pair_uniformity(const float* x, int64_t m, int64_t d, float t, float* out, int* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(m >= 2 && m <= RT_MAX_ROWS, "mdg_pair_uniformity: need 2 <= m <= %lld (got %lld)", (long long)RT_MAX_ROWS,
                (long long)m);
  MDG_CHECK_ARG(d == RT_D, "mdg_pair_uniformity: only D = %d is supported (got %lld)", RT_D, (long long)d);
  MDG_CHECK_ARG(x && out && status, "mdg_pair_uniformity: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(x), "mdg_pair_uniformity: x must be 16-byte aligned");
  MDG_CHECK_ARG(t == t, "mdg_pair_uniformity: t is NaN");
  const RtLayout lay = rt_layout(m, false);
  if (!workspace || workspace_bytes < lay.total) {
    mdg_set_error("mdg_pair_uniformity: workspace of %zu bytes needed", lay.total);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const RtParams prm = rt_params(ws + lay.params, m);
  const int T = static_cast<int>(mdg_cdiv(m, RT_BT));
  const int n_tiles = T * (T + 1) / 2;
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_pair_uniformity: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  const int waves = static_cast<int>(mdg_cdiv(m, 32));
  hipLaunchKernelGGL(rt_prep<false>, dim3(static_cast<unsigned>(mdg_cdiv(waves, RT_THREADS / 64))), dim3(RT_THREADS), 0, st, x, x,
                     static_cast<int>(m), prm, nullptr, status);
  MDG_CHECK_LAUNCH("rt_prep");
  double* uslab = reinterpret_cast<double*>(ws + lay.slab);
  RtTileArgs a{x, x, prm, static_cast<int>(m), T, nullptr, uslab, x, t};
  hipLaunchKernelGGL(rt_tile<RT_UNIFORM>, dim3(n_tiles), dim3(RT_THREADS), 0, st, a);
  MDG_CHECK_LAUNCH("rt_tile<uniform>");
  hipLaunchKernelGGL(rt_uniform_final, dim3(1), dim3(RT_THREADS), 0, st, uslab, n_tiles, m, out);
  MDG_CHECK_LAUNCH("rt_uniform_final");
  return MDG_OK;
}
