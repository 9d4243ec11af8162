// Streaming per-pair top-k over the OUTCOME axis of a score / rank tensor for gfx950 (mdg_outcome_topk_update).
//
// x [Lc, Nh, Nt] (fp32, IEEE half or bfloat16; explicit outcome stride and row pitch) is folded into a running state
// vals fp32 / idx int32 [k, Nh, Nt]: per pair (i, j) the k best (value, outcome id) under ONE total order -- value descending, id
// ascending -- so the state after any sequence of calls does not depend on how the outcomes were split or ordered.
//
// Layout: a lane owns COLS neighbouring tail columns of one head row (16 bytes of x: 4 fp32 or 8 half columns; COLS = 1 on the
// scalar path for odd pitches / unaligned bases) and keeps their k (value, id) lists in registers over the whole Lc loop; the state
// is loaded once and stored once per call.  Every access is coalesced along the tail dimension.  The planes of one pair are
// Nh * pitch elements apart -- each its own DRAM stream -- so OT_DEPTH planes are in flight before the inserts of the current one.
// The insert is a per-lane branch-free compare-and-shift: no cross-lane traffic, no LDS, no atomics.
// `largest = 0` runs the same code on negated values (an exact sign flip on the way in and out of the registers).
#include "mdg_common.h"

namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_DEPTH = 8;               // planes in flight per lane on the main paths
constexpr int OT_MAX_K = 8;
constexpr int OT_NO_ID = 0x7fffffff;      // the id of a value that must not be kept: it loses every tie, also against the sentinel's -1

struct OtF16 { unsigned short u; };
struct OtBf16 { unsigned short u; };

struct OtArgs {
  const void* x;
  int64_t xs, ldx;            // outcome stride and row pitch of x, in elements
  const int32_t* labels;      // [n_labels] or null
  const float* shift;         // [n_labels] or null
  const float* scale;         // [n_labels] or null
  float* vals;
  int32_t* idx;
  int64_t ss, lds;            // plane stride and row pitch of the state, in elements
  int n_tail, n_labels, ncb;  // ncb: column blocks per head row
  int label_base;
  int fresh, lower;
  uint32_t neg;               // 0x80000000 for `largest = 0`, else 0
};

__device__ __forceinline__ float ot_widen(float v) { return v; }
__device__ __forceinline__ float ot_widen(OtF16 v) { return static_cast<float>(__builtin_bit_cast(_Float16, v.u)); }
__device__ __forceinline__ float ot_widen(OtBf16 v) { return __builtin_bit_cast(float, static_cast<uint32_t>(v.u) << 16); }

// one plane's COLS values of a lane: the 16 raw bytes on the vector path, widened floats on the guarded element path
template <typename T, int COLS, bool VEC>
struct OtRaw {
  float f[COLS];
  __device__ __forceinline__ float get(int c) const { return f[c]; }
  __device__ __forceinline__ void load(const T* p, int ncol) {
#pragma unroll
    for (int c = 0; c < COLS; ++c) f[c] = c < ncol ? ot_widen(p[c]) : 0.f;
  }
};
template <typename T, int COLS>
struct OtRaw<T, COLS, true> {
  u32x4 q;
  __device__ __forceinline__ float get(int c) const {
    if constexpr (sizeof(T) == 4) {
      const uint32_t w = q[c];              // (a bit cast of the element expression itself reads element 0)
      return __builtin_bit_cast(float, w);
    } else {
      T h;
      h.u = static_cast<unsigned short>(q[c >> 1] >> (16 * (c & 1)));
      return ot_widen(h);
    }
  }
  __device__ __forceinline__ void load(const T* p, int) { q = *reinterpret_cast<const u32x4*>(p); }
};

// (v, id) into the sorted list: slot s keeps its entry while that entry beats the new one, takes the new one when the slot above
// still beats it, and the slot above's entry otherwise
template <int K>
__device__ __forceinline__ void ot_insert(float (&val)[K], int (&idx)[K], float v, int id) {
  bool beats[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    // val > v, or val == v and the lower id; written on >= and with bitwise operators so that the three compares combine as lane
    // masks on the scalar unit
    beats[s] = static_cast<bool>(static_cast<int>(val[s] > v) | (static_cast<int>(val[s] >= v) & static_cast<int>(idx[s] < id)));
  }
#pragma unroll
  for (int s = K - 1; s > 0; --s) {
    const float tv = beats[s - 1] ? v : val[s - 1];
    const int ti = beats[s - 1] ? id : idx[s - 1];
    val[s] = beats[s] ? val[s] : tv;
    idx[s] = beats[s] ? idx[s] : ti;
  }
  val[0] = beats[0] ? val[0] : v;
  idx[0] = beats[0] ? idx[0] : id;
}

template <typename T, int K, int COLS, bool VEC, int DEPTH>
__device__ __forceinline__ void ot_fold(const OtArgs& a, const T* xp, int ncol, float (&val)[COLS][K], int (&idx)[COLS][K]) {
  const int L = a.n_labels;
  OtRaw<T, COLS, VEC> buf[DEPTH];
#pragma unroll
  for (int p = 0; p < DEPTH; ++p) buf[p].load(xp + static_cast<int64_t>(min(p, L - 1)) * a.xs, ncol);
  for (int l0 = 0; l0 < L; l0 += DEPTH) {
#pragma unroll
    for (int p = 0; p < DEPTH; ++p) {
      const int l = l0 + p;
      if (l >= L) break;                                      // wave-uniform
      const OtRaw<T, COLS, VEC> r = buf[p];
      buf[p].load(xp + static_cast<int64_t>(min(l + DEPTH, L - 1)) * a.xs, ncol);          // (past the end: the last plane again, unused)
      const int id = a.labels ? a.labels[l] : a.label_base + l;
      const float sh = a.shift ? a.shift[l] : 0.f;
      const float sc = a.scale ? a.scale[l] : 1.f;
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        // a subtract, then a multiply, each rounded to fp32 (x - 0 and x * 1 are exact); then the sign flip of `largest = 0`
        const float u = __fmul_rn(__fsub_rn(r.get(c), sh), sc);
        const float v = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, u) ^ a.neg);
        const bool keep = id >= 0 && v == v && v != -INFINITY;          // not a skipped plane, not NaN, not the sentinel value
        ot_insert<K>(val[c], idx[c], keep ? v : -INFINITY, keep ? id : OT_NO_ID);
      }
    }
  }
}

template <typename T, int K, int COLS>
__global__ __launch_bounds__(OT_THREADS) void outcome_topk_kernel(const OtArgs a) {
  const int64_t row = blockIdx.x / a.ncb;
  const int cb = blockIdx.x - static_cast<int>(row) * a.ncb;
  const int64_t c0 = (static_cast<int64_t>(cb) * OT_THREADS + threadIdx.x) * COLS;
  if (c0 >= a.n_tail) return;
  const int ncol = static_cast<int>(min(static_cast<int64_t>(COLS), a.n_tail - c0));
  // eligible columns of the group: all of them, or (LOWER) those below the row index -- a prefix of the group either way
  const int nelig = a.lower ? static_cast<int>(max(static_cast<int64_t>(0), min(static_cast<int64_t>(ncol), row - c0))) : ncol;
  if (nelig == 0 && !a.fresh) return;                         // nothing to fold and nothing to initialise
  const bool full = COLS > 1 && ncol == COLS;                 // the whole group lies inside the row: 16-byte accesses

  float val[COLS][K];
  int idx[COLS][K];
  float* const vp = a.vals + row * a.lds + c0;
  int32_t* const ip = a.idx + row * a.lds + c0;
  if (a.fresh) {
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
#pragma unroll
      for (int s = 0; s < K; ++s) { val[c][s] = -INFINITY; idx[c][s] = -1; }
    }
  } else {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (full) {
#pragma unroll
        for (int g = 0; g < COLS / 4; ++g) {
          const u32x4 v4 = *reinterpret_cast<const u32x4*>(vp + s * a.ss + 4 * g);
          const u32x4 i4 = *reinterpret_cast<const u32x4*>(ip + s * a.ss + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            val[4 * g + e][s] = __builtin_bit_cast(float, v4[e] ^ a.neg);
            idx[4 * g + e][s] = static_cast<int>(i4[e]);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
          val[c][s] = c < ncol ? __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, vp[s * a.ss + c]) ^ a.neg) : -INFINITY;
          idx[c][s] = c < ncol ? ip[s * a.ss + c] : -1;
        }
      }
    }
  }

  if (nelig > 0 && a.n_labels > 0) {
    const T* xp = static_cast<const T*>(a.x) + row * a.ldx + c0;
    if constexpr (COLS == 1) {
      ot_fold<T, K, 1, false, OT_DEPTH>(a, xp, 1, val, idx);
    } else {
      if (full) ot_fold<T, K, COLS, true, OT_DEPTH>(a, xp, ncol, val, idx);
      else ot_fold<T, K, COLS, false, 2>(a, xp, ncol, val, idx);          // the ragged last group of a row: guarded element loads
    }
  }

  // fresh: every entry of the group is written, the ineligible ones as sentinels; otherwise only the eligible prefix
  const int nstore = a.fresh ? ncol : nelig;
#pragma unroll
  for (int c = 0; c < COLS; ++c) {
    if (c >= nelig) {
#pragma unroll
      for (int s = 0; s < K; ++s) { val[c][s] = -INFINITY; idx[c][s] = -1; }
    }
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (full && nstore == COLS) {
#pragma unroll
      for (int g = 0; g < COLS / 4; ++g) {
        u32x4 v4, i4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v4[e] = __builtin_bit_cast(uint32_t, val[4 * g + e][s]) ^ a.neg;
          i4[e] = static_cast<uint32_t>(idx[4 * g + e][s]);
        }
        *reinterpret_cast<u32x4*>(vp + s * a.ss + 4 * g) = v4;
        *reinterpret_cast<u32x4*>(ip + s * a.ss + 4 * g) = i4;
      }
    } else {
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        if (c < nstore) {
          vp[s * a.ss + c] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, val[c][s]) ^ a.neg);
          ip[s * a.ss + c] = idx[c][s];
        }
      }
    }
  }
}

template <typename T, int COLS>
void ot_launch(const OtArgs& a, int k, unsigned grid, hipStream_t st) {
  switch (k) {
    case 1: hipLaunchKernelGGL((outcome_topk_kernel<T, 1, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 2: hipLaunchKernelGGL((outcome_topk_kernel<T, 2, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 3: hipLaunchKernelGGL((outcome_topk_kernel<T, 3, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 4: hipLaunchKernelGGL((outcome_topk_kernel<T, 4, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 5: hipLaunchKernelGGL((outcome_topk_kernel<T, 5, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 6: hipLaunchKernelGGL((outcome_topk_kernel<T, 6, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    case 7: hipLaunchKernelGGL((outcome_topk_kernel<T, 7, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL((outcome_topk_kernel<T, 8, COLS>), dim3(grid), dim3(OT_THREADS), 0, st, a); break;
  }
}

template <typename T>
void ot_launch_type(const OtArgs& a, int k, bool vec, int64_t n_head, hipStream_t st, int64_t* blocks) {
  constexpr int VCOLS = 16 / sizeof(T);
  const int cols = vec ? VCOLS : 1;
  OtArgs b = a;
  b.ncb = static_cast<int>(mdg_cdiv(a.n_tail, static_cast<int64_t>(OT_THREADS) * cols));
  *blocks = n_head * b.ncb;
  if (*blocks > 0x7fffffff) return;
  if (vec) ot_launch<T, VCOLS>(b, k, static_cast<unsigned>(*blocks), st);
  else ot_launch<T, 1>(b, k, static_cast<unsigned>(*blocks), st);
}

}  // namespace

extern "C" int mdg_outcome_topk_update(const void* x, int x_type, int64_t x_outcome_stride, int64_t ldx, const int32_t* labels,
                                       int64_t label_base, const float* shift, const float* scale, float* vals, int32_t* idx,
                                       int64_t state_plane_stride, int64_t lds, int64_t n_head, int64_t n_tail, int64_t n_labels, int k,
                                       int fresh, int largest, int eligible, void* stream) {
  const char* const fn = "mdg_outcome_topk_update";
  MDG_CHECK_ARG(x_type == 0 || x_type == MDG_SCORE_F16 || x_type == MDG_SCORE_BF16, "%s: unknown x_type %d (0 = fp32, MDG_SCORE_F16, MDG_SCORE_BF16)",
                fn, x_type);
  MDG_CHECK_ARG(k >= 1 && k <= OT_MAX_K, "%s: k = %d outside 1..%d", fn, k, OT_MAX_K);
  MDG_CHECK_ARG(eligible == MDG_TOPK_ALL || eligible == MDG_TOPK_LOWER, "%s: eligible must be MDG_TOPK_ALL or MDG_TOPK_LOWER (got %d)", fn, eligible);
  MDG_CHECK_ARG(largest == 0 || largest == 1, "%s: largest must be 0 or 1 (got %d)", fn, largest);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "%s: negative size", fn);
  MDG_CHECK_ARG(n_tail < (int64_t(1) << 31) - 8 * OT_THREADS, "%s: n_tail %lld does not fit the int32 column indices", fn, (long long)n_tail);
  MDG_CHECK_ARG(label_base >= 0 && label_base + n_labels <= 0x7fffffff, "%s: outcome ids [%lld, %lld) leave the int32 range", fn,
                (long long)label_base, (long long)(label_base + n_labels));
  if (n_head == 0 || n_tail == 0 || (n_labels == 0 && !fresh)) return MDG_OK;
  MDG_CHECK_ARG(vals && idx, "%s: null state pointer", fn);
  MDG_CHECK_ARG(lds >= n_tail && (k == 1 || state_plane_stride >= (n_head - 1) * lds + n_tail),
                "%s: state pitch %lld < n_tail %lld, or plane stride %lld inside a plane", fn, (long long)lds, (long long)n_tail,
                (long long)state_plane_stride);
  MDG_CHECK_ARG(((reinterpret_cast<uintptr_t>(vals) | reinterpret_cast<uintptr_t>(idx)) & 3u) == 0, "%s: vals and idx must be 4-byte aligned", fn);
  const size_t esz = x_type == 0 ? 4 : 2;
  if (n_labels > 0) {
    MDG_CHECK_ARG(x, "%s: null x", fn);
    MDG_CHECK_ARG(ldx >= n_tail && x_outcome_stride >= 0, "%s: x pitch %lld < n_tail %lld, or a negative outcome stride", fn, (long long)ldx,
                  (long long)n_tail);
    MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & (esz - 1)) == 0, "%s: x must be aligned to its element size", fn);
  }
  // 16-byte accesses where every row of x and of the state starts on a 16-byte boundary; the element path otherwise
  const bool vec = (n_labels == 0 || (mdg_aligned16(x) && (ldx * esz) % 16 == 0 && (x_outcome_stride * esz) % 16 == 0)) && mdg_aligned16(vals) &&
                   mdg_aligned16(idx) && lds % 4 == 0 && state_plane_stride % 4 == 0;
  OtArgs a{};
  a.x = x; a.xs = x_outcome_stride; a.ldx = ldx;
  a.labels = labels; a.shift = shift; a.scale = scale;
  a.vals = vals; a.idx = idx; a.ss = state_plane_stride; a.lds = lds;
  a.n_tail = static_cast<int>(n_tail); a.n_labels = static_cast<int>(n_labels);
  a.label_base = static_cast<int>(label_base);
  a.fresh = fresh ? 1 : 0;
  a.lower = eligible == MDG_TOPK_LOWER;
  a.neg = largest ? 0u : 0x80000000u;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t blocks = 0;
  if (x_type == 0) ot_launch_type<float>(a, k, vec, n_head, st, &blocks);
  else if (x_type == MDG_SCORE_F16) ot_launch_type<OtF16>(a, k, vec, n_head, st, &blocks);
  else ot_launch_type<OtBf16>(a, k, vec, n_head, st, &blocks);
  MDG_CHECK_ARG(blocks <= 0x7fffffff, "%s: %lld workgroups exceed the grid (split the head rows)", fn, (long long)blocks);
  MDG_CHECK_LAUNCH(fn);
  return MDG_OK;
}
