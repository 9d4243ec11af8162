// Per-outcome classification metrics of labelled DDI triples (madrigal/evaluate/metrics.py:60-191: get_metrics_binary once per
// label, sklearn inside), every label in one call.
//
// Layout.  Each triple becomes one 64-bit key: bits 0-31 the order-preserving image of its score (mdg_order_key; -0 folded to +0 so
// equal floats give equal keys), bit 32 its target, bits 33-48 its label.  A stable device-wide LSD radix sort with 8-bit digits
// orders the keys by score (4 passes), then by label (1 or 2 passes, none when L == 1).  Every pass is
//   em_hist     one workgroup per tile of 4096 keys: the tile's 256-bin digit histogram (LDS integer counts), stored digit-major;
//   em_scan     one workgroup per digit: exclusive scan of that digit's per-tile counts (fixed order), and the digit's total;
//   em_scatter  per tile again: each wave ranks its 16 x 64 keys stably (ballot match of the 8 digit bits, a running count per
//               digit and wave), the 4 waves' counts are scanned per digit, and each key goes to
//               digit base + tile offset + wave offset + rank.
// No atomic decides a position: the result is the same permutation on every run.  After the last pass each label is one contiguous
// segment, ascending by score, ties in their original order (em_bounds finds the segments).
//
// em_label_metrics: one workgroup (256 threads) per label walks its segment from the top, in chunks of 2048 keys (8 consecutive
// positions per thread).  A very large label is walked by its one workgroup too (no multi-workgroup path yet: with skewed sizes
// the largest label's walk sets the call's time).  A first sweep counts the positives P and the confusion counts at pred > threshold; the second sweep
// computes, per descending position p (1-based p+1 items above and at it):
//   tp_p, fp_p           block scan of the target bits plus the chunk carry;
//   threshold            p is the last item of its run of equal scores (sklearn's distinct thresholds);
//   previous threshold   exclusive max-scan of (p+1, tp_p) packed in 64 bits over the thresholds (both grow with p);
//   auprc                sum over thresholds of (tp_p/P - tp_prev/P) * tp_p/(p+1), f64 (average_precision_score);
//   auroc                2 x area = sum over thresholds of (fp_p - fp_prev)(tp_p + tp_prev), uint64, divided once by 2 P N in f64;
//   fmax                 max over thresholds of 2 pr / (p + r) (0 where p + r = 0; the curve's final (1, 0) point adds 0);
//   top-k                the first k positions: tp_k, and ap@k = sum over the thresholds inside the top k (position k-1 always
//                        closes one) of (tp_p - tp_prev) * tp_p/(p+1), divided by tp_k.
// Tie rule at the k-th place: descending score, ties in REVERSE original order -- a stable ascending sort read from the top, which is
// np.argsort(pred, kind="stable")[::-1].  (The reference uses np.argsort's unstable default there and when it groups the labels, so
// on a tie at the k-th place its choice is arbitrary.)
// Numerics: integer counts throughout; every f64 partial sum is per thread in position order, reduced across the block in a fixed
// tree: the values are bit-identical from run to run.  No scratch, no float atomics, no global atomics except the status word (OR).
#include "mdg_common.h"

#include <algorithm>

namespace {

constexpr int EM_THREADS = 256;
constexpr int EM_ITEMS = 16;                              // keys per thread and sort pass
constexpr int EM_TILE = EM_THREADS * EM_ITEMS;            // 4096 keys per sort workgroup
constexpr int EM_WALK_ITEMS = 8;                          // consecutive positions per thread in the metric walk
constexpr int EM_CHUNK = EM_THREADS * EM_WALK_ITEMS;      // 2048 positions per walk step
constexpr int EM_N_METRICS = 13;

constexpr uint32_t EM_BAD_PRED = 1u, EM_BAD_LABEL = 2u, EM_BAD_TARGET = 4u, EM_ZERO_K = 8u, EM_BAD_GROUP = 16u;
constexpr int EM_SMALL_GROUP = 32;                        // mdg_group_metrics: groups of at most this many triples take the thread walk

__device__ __forceinline__ uint32_t em_digit(uint64_t key, int shift) { return static_cast<uint32_t>(key >> shift) & 255u; }
__device__ __forceinline__ uint32_t em_score(uint64_t key) { return static_cast<uint32_t>(key); }
__device__ __forceinline__ uint32_t em_target(uint64_t key) { return static_cast<uint32_t>(key >> 32) & 1u; }
__device__ __forceinline__ uint32_t em_label(uint64_t key) { return static_cast<uint32_t>(key >> 33); }

__device__ __forceinline__ uint64_t em_lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// ---- 1. pack + validate -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) em_pack(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const int64_t* __restrict__ label, int64_t T, int64_t L,
                                                       uint64_t* __restrict__ keys, int* __restrict__ status, uint32_t bad_index_bit) {
  uint32_t bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * EM_THREADS) {
    float p = pred[i];
    const float y = target[i];
    const int64_t l = label[i];
    if (!(fabsf(p) <= 3.402823466e38f)) bad |= EM_BAD_PRED;            // NaN or +-inf
    if (l < 0 || l >= L) bad |= bad_index_bit;
    if (!(y == 0.0f || y == 1.0f)) bad |= EM_BAD_TARGET;
    if (p == 0.0f) p = 0.0f;                                            // -0 and +0 are one threshold (np.diff == 0)
    const uint64_t lab = (l >= 0 && l < L) ? static_cast<uint64_t>(l) : 0ull;
    keys[i] = (lab << 33) | (static_cast<uint64_t>(y == 1.0f) << 32) | mdg_order_key(p);
  }
  // one OR per wave that saw a bad value (the ballots are wave-uniform)
  const uint32_t wave_bad = (__ballot(bad & EM_BAD_PRED) ? EM_BAD_PRED : 0u) | (__ballot(bad & bad_index_bit) ? bad_index_bit : 0u) |
                            (__ballot(bad & EM_BAD_TARGET) ? EM_BAD_TARGET : 0u);
  if (wave_bad && (threadIdx.x & 63) == 0) atomicOr(status, static_cast<int>(wave_bad));
}

// ---- 2. one LSD pass: histogram, scan, stable scatter -------------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) em_hist(const uint64_t* __restrict__ keys, int64_t T, int shift,
                                                       uint32_t* __restrict__ hist, int64_t n_tiles) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = blockIdx.x * (int64_t)EM_TILE;
#pragma unroll 4
  for (int it = 0; it < EM_ITEMS; ++it) {
    const int64_t i = base + it * EM_THREADS + threadIdx.x;
    if (i < T) atomicAdd(&cnt[em_digit(keys[i], shift)], 1u);          // an LDS count: order-free
  }
  __syncthreads();
  hist[threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// Block-wide exclusive sum of one uint32 per thread (256 threads); returns the block total in *total.
__device__ __forceinline__ uint32_t em_block_excl_sum_u32(uint32_t v, uint32_t* lds4, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds4[w] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t s = lds4[q];
    before += (q < w) ? s : 0u;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

__global__ void __launch_bounds__(EM_THREADS) em_scan(uint32_t* __restrict__ hist, int64_t n_tiles, uint32_t* __restrict__ totals) {
  __shared__ uint32_t lds4[4];
  uint32_t* row = hist + blockIdx.x * n_tiles;
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < n_tiles; b0 += EM_THREADS) {
    const int64_t b = b0 + threadIdx.x;
    const uint32_t v = b < n_tiles ? row[b] : 0u;
    uint32_t tot;
    const uint32_t ex = em_block_excl_sum_u32(v, lds4, &tot);
    if (b < n_tiles) row[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(EM_THREADS) em_scatter(const uint64_t* __restrict__ keys, uint64_t* __restrict__ out, int64_t T,
                                                          int shift, const uint32_t* __restrict__ hist, int64_t n_tiles,
                                                          const uint32_t* __restrict__ totals) {
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t lds4[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) wcnt[q][threadIdx.x] = 0;
  // digit bases: exclusive scan of the 256 digit totals
  uint32_t dtot;
  const uint32_t dbase = em_block_excl_sum_u32(totals[threadIdx.x], lds4, &dtot);
  const uint32_t tile_off = hist[threadIdx.x * n_tiles + blockIdx.x];
  __syncthreads();

  // wave w owns keys [tile + w*1024, tile + (w+1)*1024), 64 at a time, in index order
  const int64_t base = blockIdx.x * (int64_t)EM_TILE + w * (EM_ITEMS * 64);
  const uint64_t lt = em_lanemask_lt();
  uint64_t k[EM_ITEMS];
  uint32_t rank[EM_ITEMS];
#pragma unroll
  for (int it = 0; it < EM_ITEMS; ++it) {
    const int64_t i = base + it * 64 + lane;
    const bool ok = i < T;
    k[it] = ok ? keys[i] : 0ull;
    const uint32_t d = em_digit(k[it], shift);
    uint64_t peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t ones = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? ones : ~ones;
    }
    const uint32_t before = wcnt[w][d];
    const uint32_t r = static_cast<uint32_t>(__popcll(peers & lt));
    rank[it] = before + r;
    // the highest peer lane advances the running count (after every lane's read: LDS ops of one wave complete in order)
    __builtin_amdgcn_wave_barrier();
    if (ok && (peers >> lane) == 1ull) wcnt[w][d] = before + r + 1u;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    const int d = threadIdx.x;                                   // per digit: offsets of the 4 waves
    uint32_t run = dbase + tile_off;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = wcnt[q][d];
      wcnt[q][d] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < EM_ITEMS; ++it) {
    const int64_t i = base + it * 64 + lane;
    if (i < T) out[wcnt[w][em_digit(k[it], shift)] + rank[it]] = k[it];
  }
}

// ---- 3. label segments of the sorted keys --------------------------------------------------------------------------------
__global__ void __launch_bounds__(EM_THREADS) em_bounds(const uint64_t* __restrict__ keys, int64_t T, int32_t* __restrict__ seg_lo,
                                                         int32_t* __restrict__ seg_hi) {
  for (int64_t i = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * EM_THREADS) {
    const uint32_t l = em_label(keys[i]);
    if (i == 0 || em_label(keys[i - 1]) != l) seg_lo[l] = static_cast<int32_t>(i);
    if (i == T - 1 || em_label(keys[i + 1]) != l) seg_hi[l] = static_cast<int32_t>(i + 1);
  }
}

// ---- 4. the metrics of one label per workgroup ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t em_block_excl_max_u64(uint64_t v, uint64_t* lds4, uint64_t* all_out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x = x > y ? x : y;
  }
  uint64_t ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = 0;
  if (lane == 63) lds4[w] = x;
  __syncthreads();
  uint64_t all = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint64_t s = lds4[q];
    if (q < w) ex = ex > s ? ex : s;
    all = all > s ? all : s;
  }
  __syncthreads();
  *all_out = all;
  return ex;
}

template <typename T, typename Op>
__device__ __forceinline__ T em_block_reduce(T v, T* lds, Op op) {        // fixed tree: lanes, then waves 0..3 in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = op(op(lds[0], lds[1]), op(lds[2], lds[3]));
  __syncthreads();
  return r;
}

// The 13 values of one problem from its walk totals, written to column `col` of values [13, stride] and count / pos / k_eff.
__device__ __forceinline__ void em_finish(int64_t n, int64_t P, int64_t tp_t, int64_t fp_t, uint64_t auc2, double ap, double apk,
                                          double fmax, int64_t k, uint32_t tp_k, double* __restrict__ values, int64_t stride, int64_t col,
                                          int64_t* __restrict__ count, int64_t* __restrict__ pos, int64_t* __restrict__ k_eff_out) {
  const double nan = __builtin_nan("");
  const int64_t N = n - P;
  const double Pd = static_cast<double>(P);
  const double tp = static_cast<double>(tp_t), fp = static_cast<double>(fp_t);
  const double fn = static_cast<double>(P - tp_t), tn = static_cast<double>(N - fp_t);
  const double nd = static_cast<double>(n);
  const double specificity = tn / (tn + fp), recall = tp / (tp + fn), npv = tn / (tn + fn), precision = tp / (tp + fp);
  const double f1 = (2.0 * precision * recall) / (precision + recall);
  const double accuracy = (tp + tn) / (tn + fn + tp + fp);
  // sklearn matthews_corrcoef over the 2 x 2 confusion matrix, in f64
  const double t0 = tn + fp, t1 = fn + tp, q0 = tn + fn, q1 = fp + tp;
  const double cov_ytyp = (tp + tn) * nd - (t0 * q0 + t1 * q1);
  const double cov_ypyp = nd * nd - (q0 * q0 + q1 * q1);
  const double cov_ytyt = nd * nd - (t0 * t0 + t1 * t1);
  const double cyy = cov_ypyp * cov_ytyt;
  const double mcc = cyy == 0.0 ? 0.0 : cov_ytyp / sqrt(cyy);
  const double auroc = (P == 0 || N == 0) ? nan : static_cast<double>(auc2) / static_cast<double>(2 * P * N);
  const double auprc = P == 0 ? 0.0 : ap;
  const bool k_ok = k > 0 && k <= n;
  const double tpk = static_cast<double>(tp_k);
  const double recall_k = k_ok ? tpk / Pd : nan;                       // 0/0 -> NaN when P == 0
  const double precision_k = k_ok ? tpk / static_cast<double>(k) : nan;
  const double ap_k = k_ok ? (tp_k == 0 ? 0.0 : apk / tpk) : nan;
  const double v[EM_N_METRICS] = {P == 0 ? 0.0 : fmax, mcc, auroc, auprc, npv, specificity, f1, recall_k, precision_k, ap_k,
                                   accuracy, precision, recall};
#pragma unroll
  for (int m = 0; m < EM_N_METRICS; ++m) values[m * stride + col] = v[m];
  count[col] = n;
  pos[col] = P;
  k_eff_out[col] = k;
}

// The workgroup walk (256 threads) of one problem: seg[0, n) ascending, n > 0.  Every thread of the block calls it (it holds
// barriers); thread 0 writes the results.
__device__ __forceinline__ void em_walk_block(const uint64_t* __restrict__ seg, int64_t n, int64_t k_int, double k_frac, uint32_t thr_key,
                                              double* __restrict__ values, int64_t stride, int64_t col, int64_t* __restrict__ count,
                                              int64_t* __restrict__ pos, int64_t* __restrict__ k_eff_out, int* __restrict__ status,
                                              uint32_t* lds_u32, uint64_t* lds_u64, double* lds_f64, int64_t* lds_tpk) {
  const int64_t k = k_int > 0 ? k_int : static_cast<int64_t>(k_frac * static_cast<double>(n));   // int(k * n), as Python truncates
  if (k <= 0 && threadIdx.x == 0) atomicOr(status, static_cast<int>(EM_ZERO_K));
  // (seg is ascending; descending position p is seg[n - 1 - p])

  // sweep 1: P and the confusion counts at pred > threshold
  uint32_t c_pos = 0, c_tp = 0, c_fp = 0;
  for (int64_t p = threadIdx.x; p < n; p += EM_THREADS) {
    const uint64_t key = seg[p];
    const uint32_t y = em_target(key), hit = em_score(key) > thr_key;
    c_pos += y;
    c_tp += y & hit;
    c_fp += (1u - y) & hit;
  }
  auto add_u32 = [](uint32_t a, uint32_t b) { return a + b; };
  const int64_t P = em_block_reduce(c_pos, lds_u32, add_u32);
  const int64_t tp_t = em_block_reduce(c_tp, lds_u32, add_u32);
  const int64_t fp_t = em_block_reduce(c_fp, lds_u32, add_u32);
  const double Pd = static_cast<double>(P);

  // sweep 2: the walk from the top
  double ap = 0.0, apk = 0.0, fmax = 0.0;
  uint64_t auc2 = 0;
  uint32_t tp_carry = 0;
  uint64_t thr_carry = 0;                                           // (p+1) << 32 | tp at the last threshold so far
  if (threadIdx.x == 0) *lds_tpk = 0;
  for (int64_t c0 = 0; c0 < n; c0 += EM_CHUNK) {
    const int64_t p0 = c0 + threadIdx.x * EM_WALK_ITEMS;
    uint32_t sc[EM_WALK_ITEMS + 1], yb[EM_WALK_ITEMS];
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < EM_WALK_ITEMS; ++i) {
      const int64_t p = p0 + i;
      const uint64_t key = p < n ? seg[n - 1 - p] : 0ull;
      sc[i] = em_score(key);
      yb[i] = p < n ? em_target(key) : 0u;
      cnt += yb[i];
    }
    sc[EM_WALK_ITEMS] = (p0 + EM_WALK_ITEMS < n) ? em_score(seg[n - 1 - (p0 + EM_WALK_ITEMS)]) : 0u;
    uint32_t chunk_pos;
    uint32_t tp = tp_carry + em_block_excl_sum_u32(cnt, lds_u32, &chunk_pos);
    // thresholds of this thread and the last one at or before each
    uint64_t my_last = 0;
    uint32_t tpi[EM_WALK_ITEMS];
#pragma unroll
    for (int i = 0; i < EM_WALK_ITEMS; ++i) {
      tp += yb[i];
      tpi[i] = tp;
      const int64_t p = p0 + i;
      const bool thr = p < n && (p == n - 1 || sc[i + 1] != sc[i]);
      if (thr) my_last = (static_cast<uint64_t>(p + 1) << 32) | tp;
    }
    uint64_t chunk_last;
    uint64_t prev = em_block_excl_max_u64(my_last, lds_u64, &chunk_last);
    prev = prev > thr_carry ? prev : thr_carry;
#pragma unroll
    for (int i = 0; i < EM_WALK_ITEMS; ++i) {
      const int64_t p = p0 + i;
      if (p >= n) break;
      const uint32_t t = tpi[i];
      if (p == k - 1) *lds_tpk = t;
      const bool thr = p == n - 1 || sc[i + 1] != sc[i];
      const bool thr_k = thr || p == k - 1;                        // the top-k list ends at position k-1
      if (!thr_k) continue;
      const uint32_t prev_n = static_cast<uint32_t>(prev >> 32), prev_tp = static_cast<uint32_t>(prev);
      const double prec = static_cast<double>(t) / static_cast<double>(p + 1);
      if (p < k && thr_k) apk += static_cast<double>(t - prev_tp) * prec;
      if (thr) {
        const int64_t fp = (p + 1) - t, prev_fp = static_cast<int64_t>(prev_n) - prev_tp;
        auc2 += static_cast<uint64_t>(fp - prev_fp) * (static_cast<uint64_t>(t) + prev_tp);
        if (P > 0) {
          const double rec = static_cast<double>(t) / Pd, rec_prev = static_cast<double>(prev_tp) / Pd;
          ap += (rec - rec_prev) * prec;
          const double num = 2.0 * (prec * rec), den = prec + rec;
          const double f = den != 0.0 ? num / den : 0.0;
          fmax = f > fmax ? f : fmax;
        }
        prev = (static_cast<uint64_t>(p + 1) << 32) | t;
      }
    }
    tp_carry += chunk_pos;
    thr_carry = chunk_last > thr_carry ? chunk_last : thr_carry;
  }
  auto add_f64 = [](double a, double b) { return a + b; };
  auto max_f64 = [](double a, double b) { return a > b ? a : b; };
  auto add_u64 = [](uint64_t a, uint64_t b) { return a + b; };
  ap = em_block_reduce(ap, lds_f64, add_f64);
  apk = em_block_reduce(apk, lds_f64, add_f64);
  fmax = em_block_reduce(fmax, lds_f64, max_f64);
  auc2 = em_block_reduce(auc2, lds_u64, add_u64);
  if (threadIdx.x != 0) return;
  em_finish(n, P, tp_t, fp_t, auc2, ap, apk, fmax, k, static_cast<uint32_t>(*lds_tpk), values, stride, col, count, pos, k_eff_out);
}

__global__ void __launch_bounds__(EM_THREADS) em_label_metrics(const uint64_t* __restrict__ keys, const int32_t* __restrict__ seg_lo,
                                                                const int32_t* __restrict__ seg_hi, int64_t L, int64_t k_int, double k_frac,
                                                                uint32_t thr_key, double* __restrict__ values, int64_t* __restrict__ count,
                                                                int64_t* __restrict__ pos, int64_t* __restrict__ k_eff_out,
                                                                int* __restrict__ status) {
  __shared__ uint32_t lds_u32[4];
  __shared__ uint64_t lds_u64[4];
  __shared__ double lds_f64[4];
  __shared__ int64_t lds_tpk;
  const int64_t l = blockIdx.x;
  const int64_t lo = seg_lo[l], hi = seg_hi[l];
  const int64_t n = hi - lo;
  if (n <= 0) {
    if (threadIdx.x < EM_N_METRICS) values[threadIdx.x * L + l] = __builtin_nan("");
    if (threadIdx.x == 0) {
      count[l] = 0;
      pos[l] = 0;
      k_eff_out[l] = 0;
    }
    return;
  }
  em_walk_block(keys + lo, n, k_int, k_frac, thr_key, values, L, l, count, pos, k_eff_out, status, lds_u32, lds_u64, lds_f64, &lds_tpk);
}

// ---- 5. grouped metrics (mdg_group_metrics) ------------------------------------------------------------------------------
// The thread walk: one thread walks one problem seg[0, n) serially from the top, with the workgroup walk's formulas (its f64
// sums run in position order instead of per-thread partials plus a tree: equal to the workgroup walk within rounding).
__device__ __forceinline__ void em_walk_thread(const uint64_t* __restrict__ seg, int64_t n, int64_t k_int, double k_frac, uint32_t thr_key,
                                               double* __restrict__ values, int64_t stride, int64_t col, int64_t* __restrict__ count,
                                               int64_t* __restrict__ pos, int64_t* __restrict__ k_eff_out, int* __restrict__ status) {
  const int64_t k = k_int > 0 ? k_int : static_cast<int64_t>(k_frac * static_cast<double>(n));
  if (k <= 0) atomicOr(status, static_cast<int>(EM_ZERO_K));
  uint32_t P = 0, tp_t = 0, fp_t = 0;
  for (int64_t p = 0; p < n; ++p) {
    const uint64_t key = seg[p];
    const uint32_t y = em_target(key), hit = em_score(key) > thr_key;
    P += y;
    tp_t += y & hit;
    fp_t += (1u - y) & hit;
  }
  const double Pd = static_cast<double>(P);
  double ap = 0.0, apk = 0.0, fmax = 0.0;
  uint64_t auc2 = 0;
  uint32_t tp = 0, tp_k = 0;
  uint32_t prev_n = 0, prev_tp = 0;                                 // the last threshold before p
  uint64_t key = seg[n - 1];
  for (int64_t p = 0; p < n; ++p) {
    const uint64_t next = p + 1 < n ? seg[n - 2 - p] : 0ull;
    const uint32_t sc = em_score(key);
    tp += em_target(key);
    if (p == k - 1) tp_k = tp;
    const bool thr = p == n - 1 || em_score(next) != sc;
    key = next;
    if (!(thr || p == k - 1)) continue;
    const double prec = static_cast<double>(tp) / static_cast<double>(p + 1);
    if (p < k) apk += static_cast<double>(tp - prev_tp) * prec;
    if (thr) {
      const int64_t fp = (p + 1) - tp, prev_fp = static_cast<int64_t>(prev_n) - prev_tp;
      auc2 += static_cast<uint64_t>(fp - prev_fp) * (static_cast<uint64_t>(tp) + prev_tp);
      if (P > 0) {
        const double rec = static_cast<double>(tp) / Pd, rec_prev = static_cast<double>(prev_tp) / Pd;
        ap += (rec - rec_prev) * prec;
        const double num = 2.0 * (prec * rec), den = prec + rec;
        const double f = den != 0.0 ? num / den : 0.0;
        fmax = f > fmax ? f : fmax;
      }
      prev_n = static_cast<uint32_t>(p + 1);
      prev_tp = tp;
    }
  }
  em_finish(n, P, tp_t, fp_t, auc2, ap, apk, fmax, k, tp_k, values, stride, col, count, pos, k_eff_out);
}

// Fixed-order stream compaction of the indices i in [0, n) whose flag is set, in ascending order (no atomics): per tile of
// EM_TILE indices a count (em_flag_count), the exclusive scan of the tile counts (em_scan, one workgroup), and a write pass that
// ranks the flags of its tile by a block scan (em_flag_write; each thread owns EM_ITEMS consecutive indices).  n is n_host, or
// *n_dev when n_dev is given (a count the device produced earlier in the call).
struct EmSegStart {                                        // i starts a group of the sorted keys
  const uint64_t* keys;
  __device__ bool operator()(int64_t i) const { return i == 0 || em_label(keys[i - 1]) != em_label(keys[i]); }
};
struct EmBigGroup {                                        // group j (of n_present) takes the workgroup walk
  const int32_t* start;
  const uint32_t* n_present;
  int64_t T;
  int mode;                                                // 0: by size, 1: none, other: all
  __device__ bool operator()(int64_t j) const {
    if (mode == 1) return false;
    if (mode != 0) return true;
    const int64_t hi = j + 1 < static_cast<int64_t>(*n_present) ? start[j + 1] : T;
    return hi - start[j] > EM_SMALL_GROUP;
  }
};

template <typename Flag>
__global__ void __launch_bounds__(EM_THREADS) em_flag_count(Flag flag, int64_t n_host, const uint32_t* __restrict__ n_dev,
                                                             uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t lds4[4];
  const int64_t n = n_dev ? static_cast<int64_t>(*n_dev) : n_host;
  const int64_t base = blockIdx.x * (int64_t)EM_TILE + threadIdx.x * (int64_t)EM_ITEMS;
  uint32_t c = 0;
  for (int it = 0; it < EM_ITEMS; ++it) {
    const int64_t i = base + it;
    if (i < n) c += flag(i) ? 1u : 0u;
  }
  auto add_u32 = [](uint32_t a, uint32_t b) { return a + b; };
  c = em_block_reduce(c, lds4, add_u32);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}

template <typename Flag>
__global__ void __launch_bounds__(EM_THREADS) em_flag_write(Flag flag, int64_t n_host, const uint32_t* __restrict__ n_dev,
                                                             const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ total,
                                                             int32_t* __restrict__ out, int64_t* __restrict__ n_out) {
  __shared__ uint32_t lds4[4];
  const int64_t n = n_dev ? static_cast<int64_t>(*n_dev) : n_host;
  const int64_t base = blockIdx.x * (int64_t)EM_TILE + threadIdx.x * (int64_t)EM_ITEMS;
  uint32_t bits = 0, c = 0;
  for (int it = 0; it < EM_ITEMS; ++it) {
    const int64_t i = base + it;
    const bool f = i < n && flag(i);
    bits |= (f ? 1u : 0u) << it;
    c += f ? 1u : 0u;
  }
  uint32_t all;
  uint32_t r = tile_off[blockIdx.x] + em_block_excl_sum_u32(c, lds4, &all);
  for (int it = 0; it < EM_ITEMS; ++it)
    if ((bits >> it) & 1u) out[r++] = static_cast<int32_t>(base + it);
  if (n_out && blockIdx.x == 0 && threadIdx.x == 0) n_out[0] = static_cast<int64_t>(*total);
}

// Groups of at most EM_SMALL_GROUP triples (mode 0), every group (mode 1) or none (other modes) by the thread walk, one thread
// per group; every thread also writes its group's id.
__global__ void __launch_bounds__(EM_THREADS) em_group_walk_thread(const uint64_t* __restrict__ keys, int64_t T,
                                                                    const int32_t* __restrict__ start, const uint32_t* __restrict__ n_present,
                                                                    int mode, int64_t cap, int64_t k_int, double k_frac, uint32_t thr_key,
                                                                    int64_t* __restrict__ group_id, double* __restrict__ values,
                                                                    int64_t* __restrict__ count, int64_t* __restrict__ pos,
                                                                    int64_t* __restrict__ k_eff_out, int* __restrict__ status) {
  const int64_t np = static_cast<int64_t>(*n_present);
  for (int64_t j = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; j < np; j += (int64_t)gridDim.x * EM_THREADS) {
    const int64_t lo = start[j], hi = j + 1 < np ? start[j + 1] : T;
    group_id[j] = static_cast<int64_t>(em_label(keys[lo]));
    const bool mine = mode == 1 || (mode == 0 && hi - lo <= EM_SMALL_GROUP);
    if (mine) em_walk_thread(keys + lo, hi - lo, k_int, k_frac, thr_key, values, cap, j, count, pos, k_eff_out, status);
  }
}

// The listed groups by the workgroup walk; each workgroup takes list entries blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ void __launch_bounds__(EM_THREADS) em_group_walk_block(const uint64_t* __restrict__ keys, int64_t T,
                                                                   const int32_t* __restrict__ start, const uint32_t* __restrict__ n_present,
                                                                   const int32_t* __restrict__ big, const uint32_t* __restrict__ n_big,
                                                                   int64_t cap, int64_t k_int, double k_frac, uint32_t thr_key,
                                                                   double* __restrict__ values, int64_t* __restrict__ count,
                                                                   int64_t* __restrict__ pos, int64_t* __restrict__ k_eff_out,
                                                                   int* __restrict__ status) {
  __shared__ uint32_t lds_u32[4];
  __shared__ uint64_t lds_u64[4];
  __shared__ double lds_f64[4];
  __shared__ int64_t lds_tpk;
  const int64_t np = static_cast<int64_t>(*n_present), nb = static_cast<int64_t>(*n_big);
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t j = big[b];
    const int64_t lo = start[j], hi = j + 1 < np ? start[j + 1] : T;
    em_walk_block(keys + lo, hi - lo, k_int, k_frac, thr_key, values, cap, j, count, pos, k_eff_out, status, lds_u32, lds_u64, lds_f64,
                  &lds_tpk);
    __syncthreads();                                               // lds_tpk is read by thread 0 before the next group resets it
  }
}

// Means per outer index o (groups [o * inner, (o + 1) * inner)): one thread per (o, metric) sums that metric over the outer's present
// groups sequentially in f64, ascending group order, and divides once (numpy's mean(axis=0) over the rows of those groups).
__global__ void __launch_bounds__(EM_THREADS) em_outer_means(const int64_t* __restrict__ group_id, const uint32_t* __restrict__ n_present,
                                                              const double* __restrict__ values, int64_t cap, int64_t inner, int64_t n_outer,
                                                              double* __restrict__ outer_values, int64_t* __restrict__ outer_groups) {
  const int64_t np = static_cast<int64_t>(*n_present);
  auto lower = [&](int64_t g) {                                    // first j with group_id[j] >= g
    int64_t a = 0, b = np;
    while (a < b) {
      const int64_t c = (a + b) >> 1;
      if (group_id[c] < g) a = c + 1; else b = c;
    }
    return a;
  };
  for (int64_t t = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; t < n_outer * EM_N_METRICS; t += (int64_t)gridDim.x * EM_THREADS) {
    const int64_t o = t / EM_N_METRICS, m = t - o * EM_N_METRICS;
    const int64_t lo = lower(o * inner), hi = lower((o + 1) * inner);
    const double* row = values + m * cap;
    double s = 0.0;
    for (int64_t j = lo; j < hi; ++j) s += row[j];
    outer_values[m * n_outer + o] = hi > lo ? s / static_cast<double>(hi - lo) : __builtin_nan("");
    if (m == 0) outer_groups[o] = hi - lo;
  }
}

struct EmLayout {
  size_t keys_b, hist, totals, seg_lo, seg_hi, total;
};

EmLayout em_layout(int64_t T, int64_t L) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const int64_t n_tiles = mdg_cdiv(T, EM_TILE);
  EmLayout o;
  size_t off = al(sizeof(uint64_t) * T);                               // keys A at 0
  o.keys_b = off;
  off += al(sizeof(uint64_t) * T);
  o.hist = off;
  off += al(sizeof(uint32_t) * 256 * n_tiles);
  o.totals = off;
  off += al(sizeof(uint32_t) * 256);
  o.seg_lo = off;
  off += al(sizeof(int32_t) * L);
  o.seg_hi = off;
  off += al(sizeof(int32_t) * L);
  o.total = off;
  return o;
}

}  // namespace

extern "C" size_t mdg_label_metrics_workspace_bytes(int64_t n_triples, int64_t n_labels) {
  if (n_triples <= 0 || n_labels <= 0) return 0;
  return em_layout(n_triples, n_labels).total;
}

extern "C" int mdg_label_metrics(const float* pred, const float* target, const int64_t* label, int64_t n_triples, int64_t n_labels,
                                 int64_t k, double k_frac, float threshold, double* values, int64_t* count, int64_t* pos,
                                 int64_t* k_eff, int* status, void* workspace, size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n_triples > 0 && n_triples < (int64_t(1) << 31), "mdg_label_metrics: need 0 < n_triples < 2^31 (got %lld)",
                (long long)n_triples);
  MDG_CHECK_ARG(n_labels > 0 && n_labels <= 65536, "mdg_label_metrics: need 0 < n_labels <= 65536 (got %lld)", (long long)n_labels);
  MDG_CHECK_ARG((k > 0) != (k_frac > 0.0 && k_frac < 1.0), "mdg_label_metrics: give k > 0 or 0 < k_frac < 1, not both");
  MDG_CHECK_ARG(threshold == threshold, "mdg_label_metrics: threshold is NaN");
  MDG_CHECK_ARG(pred && target && label && values && count && pos && k_eff && status, "mdg_label_metrics: null pointer");
  const EmLayout lay = em_layout(n_triples, n_labels);
  if (!workspace || workspace_bytes < lay.total) {
    mdg_set_error("mdg_label_metrics: workspace of %zu bytes needed", lay.total);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  uint64_t* ka = reinterpret_cast<uint64_t*>(ws);
  uint64_t* kb = reinterpret_cast<uint64_t*>(ws + lay.keys_b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  uint32_t* totals = reinterpret_cast<uint32_t*>(ws + lay.totals);
  int32_t* seg_lo = reinterpret_cast<int32_t*>(ws + lay.seg_lo);
  int32_t* seg_hi = reinterpret_cast<int32_t*>(ws + lay.seg_hi);
  const int64_t T = n_triples, L = n_labels, n_tiles = mdg_cdiv(T, EM_TILE);

  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(seg_lo, 0, lay.total - lay.seg_lo, st) != hipSuccess) {          // seg_lo and seg_hi: absent labels = [0, 0)
    mdg_set_error("mdg_label_metrics: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  const int grid_ew = static_cast<int>(std::min<int64_t>(mdg_cdiv(T, EM_THREADS), 256 * 16));
  hipLaunchKernelGGL(em_pack, dim3(grid_ew), dim3(EM_THREADS), 0, st, pred, target, label, T, L, ka, status, EM_BAD_LABEL);
  MDG_CHECK_LAUNCH("em_pack");

  int label_bits = 0;
  while ((int64_t(1) << label_bits) < L) ++label_bits;
  int shifts[6], n_pass = 0;
  for (int s = 0; s < 32; s += 8) shifts[n_pass++] = s;
  for (int s = 0; s < label_bits; s += 8) shifts[n_pass++] = 33 + s;
  uint64_t *src = ka, *dst = kb;
  for (int q = 0; q < n_pass; ++q) {
    hipLaunchKernelGGL(em_hist, dim3(n_tiles), dim3(EM_THREADS), 0, st, src, T, shifts[q], hist, n_tiles);
    MDG_CHECK_LAUNCH("em_hist");
    hipLaunchKernelGGL(em_scan, dim3(256), dim3(EM_THREADS), 0, st, hist, n_tiles, totals);
    MDG_CHECK_LAUNCH("em_scan");
    hipLaunchKernelGGL(em_scatter, dim3(n_tiles), dim3(EM_THREADS), 0, st, src, dst, T, shifts[q], hist, n_tiles, totals);
    MDG_CHECK_LAUNCH("em_scatter");
    uint64_t* t = src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(em_bounds, dim3(grid_ew), dim3(EM_THREADS), 0, st, src, T, seg_lo, seg_hi);
  MDG_CHECK_LAUNCH("em_bounds");
  const float thr = threshold == 0.0f ? 0.0f : threshold;
  const uint32_t thr_key = [&] {
    const uint32_t u = __builtin_bit_cast(uint32_t, thr);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }();
  hipLaunchKernelGGL(em_label_metrics, dim3(L), dim3(EM_THREADS), 0, st, src, seg_lo, seg_hi, L, k, k_frac, thr_key, values, count, pos,
                     k_eff, status);
  MDG_CHECK_LAUNCH("em_label_metrics");
  return MDG_OK;
}

namespace {

struct EgLayout {
  size_t keys_b, hist, totals, tile_cnt, counters, start, big, total;
};

EgLayout eg_layout(int64_t T, int64_t n_groups) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const int64_t n_tiles = mdg_cdiv(T, EM_TILE), cap = std::min(T, n_groups);
  EgLayout o;
  size_t off = al(sizeof(uint64_t) * T);                               // keys A at 0
  o.keys_b = off;
  off += al(sizeof(uint64_t) * T);
  o.hist = off;
  off += al(sizeof(uint32_t) * 256 * n_tiles);
  o.totals = off;
  off += al(sizeof(uint32_t) * 256);
  o.tile_cnt = off;
  off += al(sizeof(uint32_t) * std::max(n_tiles, mdg_cdiv(cap, EM_TILE)));
  o.counters = off;                                                    // [0] groups present, [1] groups of the workgroup walk
  off += al(sizeof(uint32_t) * 2);
  o.start = off;
  off += al(sizeof(int32_t) * cap);
  o.big = off;
  off += al(sizeof(int32_t) * cap);
  o.total = off;
  return o;
}

}  // namespace

extern "C" size_t mdg_group_metrics_workspace_bytes(int64_t n_triples, int64_t n_groups) {
  if (n_triples <= 0 || n_groups <= 0) return 0;
  return eg_layout(n_triples, n_groups).total;
}

extern "C" int mdg_group_metrics(const float* pred, const float* target, const int64_t* group, int64_t n_triples, int64_t n_groups,
                                 int64_t k, double k_frac, float threshold, int64_t inner, int64_t* group_id, double* values,
                                 int64_t* count, int64_t* pos, int64_t* k_eff, int64_t* n_present, double* outer_values,
                                 int64_t* outer_groups, int* status, void* workspace, size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n_triples > 0 && n_triples < (int64_t(1) << 31), "mdg_group_metrics: need 0 < n_triples < 2^31 (got %lld)",
                (long long)n_triples);
  MDG_CHECK_ARG(n_groups > 0 && n_groups <= (int64_t(1) << 31), "mdg_group_metrics: need 0 < n_groups <= 2^31 (got %lld)",
                (long long)n_groups);
  MDG_CHECK_ARG((k > 0) != (k_frac > 0.0 && k_frac < 1.0), "mdg_group_metrics: give k > 0 or 0 < k_frac < 1, not both");
  MDG_CHECK_ARG(threshold == threshold, "mdg_group_metrics: threshold is NaN");
  MDG_CHECK_ARG(inner >= 0, "mdg_group_metrics: inner must be >= 0 (got %lld)", (long long)inner);
  MDG_CHECK_ARG(pred && target && group && group_id && values && count && pos && k_eff && n_present && status,
                "mdg_group_metrics: null pointer");
  MDG_CHECK_ARG(inner == 0 || (outer_values && outer_groups), "mdg_group_metrics: inner > 0 needs outer_values and outer_groups");
  const EgLayout lay = eg_layout(n_triples, n_groups);
  if (!workspace || workspace_bytes < lay.total) {
    mdg_set_error("mdg_group_metrics: workspace of %zu bytes needed", lay.total);
    return MDG_EWORKSPACE;
  }
  static MdgEnvInt walk_sw{"MDG_GROUP_WALK", 0};        // test hook: 0 by size, 1 every group by the thread walk, other: workgroup walk
  const int mode = walk_sw.get();
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  uint64_t* ka = reinterpret_cast<uint64_t*>(ws);
  uint64_t* kb = reinterpret_cast<uint64_t*>(ws + lay.keys_b);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  uint32_t* totals = reinterpret_cast<uint32_t*>(ws + lay.totals);
  uint32_t* tile_cnt = reinterpret_cast<uint32_t*>(ws + lay.tile_cnt);
  uint32_t* n_pres_u32 = reinterpret_cast<uint32_t*>(ws + lay.counters);
  uint32_t* n_big_u32 = n_pres_u32 + 1;
  int32_t* start = reinterpret_cast<int32_t*>(ws + lay.start);
  int32_t* big = reinterpret_cast<int32_t*>(ws + lay.big);
  const int64_t T = n_triples, G = n_groups, cap = std::min(T, G), n_tiles = mdg_cdiv(T, EM_TILE), n_gtiles = mdg_cdiv(cap, EM_TILE);

  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_group_metrics: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  const int grid_ew = static_cast<int>(std::min<int64_t>(mdg_cdiv(T, EM_THREADS), 256 * 16));
  hipLaunchKernelGGL(em_pack, dim3(grid_ew), dim3(EM_THREADS), 0, st, pred, target, group, T, G, ka, status, EM_BAD_GROUP);
  MDG_CHECK_LAUNCH("em_pack");

  int group_bits = 0;
  while ((int64_t(1) << group_bits) < G) ++group_bits;
  int shifts[8], n_pass = 0;
  for (int s = 0; s < 32; s += 8) shifts[n_pass++] = s;
  for (int s = 0; s < group_bits; s += 8) shifts[n_pass++] = 33 + s;
  uint64_t *src = ka, *dst = kb;
  for (int q = 0; q < n_pass; ++q) {
    hipLaunchKernelGGL(em_hist, dim3(n_tiles), dim3(EM_THREADS), 0, st, src, T, shifts[q], hist, n_tiles);
    MDG_CHECK_LAUNCH("em_hist");
    hipLaunchKernelGGL(em_scan, dim3(256), dim3(EM_THREADS), 0, st, hist, n_tiles, totals);
    MDG_CHECK_LAUNCH("em_scan");
    hipLaunchKernelGGL(em_scatter, dim3(n_tiles), dim3(EM_THREADS), 0, st, src, dst, T, shifts[q], hist, n_tiles, totals);
    MDG_CHECK_LAUNCH("em_scatter");
    uint64_t* t = src;
    src = dst;
    dst = t;
  }
  // segment starts of the present groups, compacted in ascending order; n_present
  const EmSegStart seg_flag{src};
  hipLaunchKernelGGL(em_flag_count<EmSegStart>, dim3(n_tiles), dim3(EM_THREADS), 0, st, seg_flag, T, nullptr, tile_cnt);
  MDG_CHECK_LAUNCH("em_flag_count");
  hipLaunchKernelGGL(em_scan, dim3(1), dim3(EM_THREADS), 0, st, tile_cnt, n_tiles, n_pres_u32);
  MDG_CHECK_LAUNCH("em_scan");
  hipLaunchKernelGGL(em_flag_write<EmSegStart>, dim3(n_tiles), dim3(EM_THREADS), 0, st, seg_flag, T, nullptr, tile_cnt, n_pres_u32, start,
                     n_present);
  MDG_CHECK_LAUNCH("em_flag_write");
  // the groups of the workgroup walk, compacted in ascending order
  const EmBigGroup big_flag{start, n_pres_u32, T, mode};
  hipLaunchKernelGGL(em_flag_count<EmBigGroup>, dim3(n_gtiles), dim3(EM_THREADS), 0, st, big_flag, cap, n_pres_u32, tile_cnt);
  MDG_CHECK_LAUNCH("em_flag_count");
  hipLaunchKernelGGL(em_scan, dim3(1), dim3(EM_THREADS), 0, st, tile_cnt, n_gtiles, n_big_u32);
  MDG_CHECK_LAUNCH("em_scan");
  hipLaunchKernelGGL(em_flag_write<EmBigGroup>, dim3(n_gtiles), dim3(EM_THREADS), 0, st, big_flag, cap, n_pres_u32, tile_cnt, n_big_u32,
                     big, nullptr);
  MDG_CHECK_LAUNCH("em_flag_write");

  const float thr = threshold == 0.0f ? 0.0f : threshold;
  const uint32_t thr_key = [&] {
    const uint32_t u = __builtin_bit_cast(uint32_t, thr);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }();
  const int grid_thread = static_cast<int>(std::min<int64_t>(mdg_cdiv(cap, EM_THREADS), 4096));
  hipLaunchKernelGGL(em_group_walk_thread, dim3(grid_thread), dim3(EM_THREADS), 0, st, src, T, start, n_pres_u32, mode, cap, k, k_frac,
                     thr_key, group_id, values, count, pos, k_eff, status);
  MDG_CHECK_LAUNCH("em_group_walk_thread");
  // at most T / (EM_SMALL_GROUP + 1) groups are larger than EM_SMALL_GROUP
  const int64_t big_bound = mode == 1 ? 0 : (mode == 0 ? std::min(cap, T / (EM_SMALL_GROUP + 1)) : cap);
  if (big_bound > 0) {
    hipLaunchKernelGGL(em_group_walk_block, dim3(static_cast<int>(std::min<int64_t>(big_bound, 4096))), dim3(EM_THREADS), 0, st, src, T,
                       start, n_pres_u32, big, n_big_u32, cap, k, k_frac, thr_key, values, count, pos, k_eff, status);
    MDG_CHECK_LAUNCH("em_group_walk_block");
  }
  if (inner > 0) {
    const int64_t n_outer = mdg_cdiv(G, inner);
    const int grid_outer = static_cast<int>(std::min<int64_t>(mdg_cdiv(n_outer * EM_N_METRICS, EM_THREADS), 256 * 64));
    hipLaunchKernelGGL(em_outer_means, dim3(grid_outer), dim3(EM_THREADS), 0, st,
                       group_id, n_pres_u32, values, cap, inner, n_outer, outer_values, outer_groups);
    MDG_CHECK_LAUNCH("em_outer_means");
  }
  return MDG_OK;
}
