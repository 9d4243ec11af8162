// Sorted top-k lists held in registers by the lanes that share a row of an MFMA accumulator (topk.hip, knn.hip).
//
// G lanes share a row (32 on the 32x32 accumulator layout, 16 on 16x16), each holding one column; the same G lanes hold the row's
// sorted list: entry e sits in slot e / G of lane e % G, 32 entries at the most.  `thr` is the row's current k-th value (-inf
// while the list is short), uniform over the G lanes.  The order is total: value descending, then column ascending.
#pragma once
#include "mdg_common.h"

namespace {

constexpr int TOPK_MAX_K = 32;      // one entry per lane of the 32 lanes sharing a row on the 32x32 MFMA

// Sorted insert of the candidates (cand, x, col) of one row into its list.  Must be called in wave-uniform control flow.
// G lanes share the row; lv / li: this lane's slots of the list (entry s * G + (lane % G)), thr: the row's k-th value.
// (Measured alternatives at 4096^2 x 896 bf16x3 / 100 352^2 x 64 f16, k = 16: this form 38.0 / 364 ms; candidates and threshold
// by v_readlane, shifts by DPP, overtaken candidates dropped: 44.0 / 431 ms; shifts by DPP only: 37.4 / 418 ms.)
template <int G>
__device__ __forceinline__ void topk_insert(float (&lv)[32 / G], int (&li)[32 / G], float& thr, bool cand, float x, int col, int lane, int k) {
  constexpr int S = 32 / G;
  constexpr unsigned GMASK = G == 32 ? 0xFFFFFFFFu : 0xFFFFu;
  unsigned long long m = __ballot(cand);
  if (m == 0) return;
  const int c = lane & (G - 1), base = lane & ~(G - 1);
  unsigned mine = static_cast<unsigned>(m >> base) & GMASK;          // candidates of MY row, one bit per lane of the group
  while (m != 0) {
    const bool has = mine != 0;
    const int src = base + (has ? __builtin_ctz(mine) : 0);
    const float cx = __shfl(x, src, 64);
    const int cc = __shfl(col, src, 64);
    int p = 0;                                                       // entries that stay ahead of the candidate (the list is sorted: a prefix)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const bool ahead = lv[s] > cx || (lv[s] == cx && li[s] < cc);
      p += __builtin_popcount(static_cast<unsigned>(__ballot(ahead) >> base) & GMASK);
    }
    const int prev = (lane + 63) & 63;
#pragma unroll
    for (int s = S - 1; s >= 0; --s) {                               // slot 1 first: it takes the OLD last entry of slot 0
      float upv = __shfl(lv[s], prev, 64);
      int upi = __shfl(li[s], prev, 64);
      if (s > 0) {
        const float wv = __shfl(lv[s - 1], base + G - 1, 64);
        const int wi = __shfl(li[s - 1], base + G - 1, 64);
        if (c == 0) { upv = wv; upi = wi; }
      }
      const int e = s * G + c;
      const bool take_new = has && e == p, take_up = has && e > p;
      lv[s] = take_new ? cx : (take_up ? upv : lv[s]);
      li[s] = take_new ? cc : (take_up ? upi : li[s]);
    }
    float t = __shfl(lv[0], base + ((k - 1) & (G - 1)), 64);
    if (S > 1) {
      const float t1 = __shfl(lv[S - 1], base + ((k - 1) & (G - 1)), 64);
      if (k > G) t = t1;
    }
    thr = t;
    mine &= mine - 1;
    m = __ballot(mine != 0);
  }
}

}  // namespace
