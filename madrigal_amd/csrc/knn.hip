// k-nearest-neighbour search over [n,128] fp32 embeddings for gfx950 (mdg_knn_topk) and the kNN classifier's vote (mdg_knn_vote).
//
// Replaces the dense similarity / distance matrix + torch.topk of madrigal/evaluate/eval_utils.py:177-229 (knn_classifier) and of
// madrigal/evaluate/evaluate.py:411-418 (the top-k index tensors of get_inst_dist_topk_accuracy): nothing of [nq, nl] is stored.
//
// mdg_knn_topk (Q [nq,128], Lib [nl,128]):
//   knn_prep    per row of Q and of Lib: |x|^2 and 1/|x| (the chain of retrieval.hip's rt_prep: norm2_step), the NaN / inf /
//               zero-norm status bits
//   knn_sweep   grid (row blocks of 128, S column segments).  4 waves; wave w owns query rows 32 w .. 32 w + 31 of the block for the
//               whole sweep: their 128 k values stay in registers as the A operand (16 float4 per lane).  The library is walked in
//               ascending 64-column stages, staged ONCE per workgroup into LDS by LDS-DMA (two 32 KB buffers, the next stage in
//               flight while this one is multiplied; bilinear_tiles.h's swizzled layout), each wave forming its 32 x 64 block of
//               G = Q Lib^T as two 32x32 accumulators with gram_step -- the chain of retrieval.hip, so a value here is bit-equal to
//               the one mdg_pair_match_counts compares.  Each row's k best sit in the 32 lanes that share the row (topk_list.h).
//   knn_merge   S > 1: every (row block, segment) wrote a partial list; one 32-lane group per query row inserts the S lists in
//               ascending segment order.
// Key: value best-first, then library index ascending.  cosine: (g rq_i) rl_j, larger is better; dot: g; euclidean: the list is
// kept on -d2, d2 = (|q_i|^2 - 2 g) + |l_j|^2, and sqrt(max(d2, 0)) is returned.  Columns ascend inside a segment and segments
// ascend in the merge, so a later value equal to the k-th has a larger index than every kept entry and rightly fails `x > thr`;
// inside a stage the insert compares the full key.  No atomics on the outputs: bit-identical from run to run and for every S.
// A column is ineligible (-inf, never kept) past the end of the library or when it is the row's `skip` index.
//
// Budget (-Rpass-analysis=kernel-resource-usage): 64 KB LDS and at most 256 VGPRs -> two workgroups per CU, 0 scratch.
#include "bilinear_tiles.h"      // stage_dma, tile_off, acc_row: the staged [64 rows][128] fp32 tile of the all-pairs head
#include "gram.h"
#include "topk_list.h"

namespace {

constexpr int KNN_BM = 128;              // query rows per workgroup: 4 waves x 32
constexpr int KNN_THREADS = 256;
constexpr int KNN_SEG = 128;             // segments are whole 128-column tiles (two stages of BN = 64)
constexpr int KNN_LDS = 2 * STAGE_BYTES;
constexpr int KNN_CUS = 256;             // MI355X
static_assert(D == 128 && BN == 64 && KNN_LDS == 65536, "two 64-column fp32 stages of 128 k values");

enum { KNN_COSINE = MDG_KNN_COSINE, KNN_DOT = MDG_KNN_DOT, KNN_EUCLIDEAN = MDG_KNN_EUCLIDEAN };

// One wave per 32 rows: lane (r, h) reads half h of row r0 + r.  stat[row] = |x|^2, stat[n + row] = 1 / |x|.
__global__ __launch_bounds__(KNN_THREADS) void knn_prep(const float* __restrict__ x, int n, float* __restrict__ stat, int zero_is_bad,
                                                        int* __restrict__ status) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int r0 = (blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6)) * 32;
  if (r0 >= n) return;
  const int row = min(r0 + r, n - 1);
  const float* xr = x + static_cast<int64_t>(row) * D;
  float s = 0.f;
  bool ok = true;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const float4 a = *reinterpret_cast<const float4*>(xr + 8 * q + 4 * h);
    ok = ok && finite4(a);
    s = norm2_step(a, s);
  }
  const float n2 = s + __shfl_xor(s, 32);               // the same sum in both halves (fp32 addition commutes)
  const float rn = 1.0f / sqrtf(n2);
  int bad = (!ok || !isfinite(n2)) ? 1 : 0;
  if (zero_is_bad && !(n2 > 0.f)) bad |= 2;
  const bool valid = r0 + r < n;
  if (valid && bad) atomicOr(status, bad);
  if (valid && h == 0) {
    stat[row] = n2;
    stat[n + row] = rn;
  }
}

struct KnnArgs {
  const float* q;
  TileSrc lib;             // f32 = Lib, nrows = nl
  const float* qstat;      // [2][nq]
  const float* lstat;      // [2][nl]
  const int* skip;         // [nq] or null
  float* vals;             // S == 1: [nq][k] results; S > 1: [S][nq][k] keys.  LISTS = false: [S][nq] row maxima
  int* idx;
  int nq, nl, k;
  int seg_stages;          // 64-column stages per segment
  int final;               // S == 1
};

// LISTS = false: the same sweep with the list epilogue compiled out (the row maximum of the values is kept instead, so the products
// stay live): what scripts/knn_bench.py measures the lists against.
template <int METRIC, bool LISTS>
__global__ __launch_bounds__(KNN_THREADS, 2) void knn_sweep(const KnnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nq = p.nq, nl = p.nl, k = p.k;
  const int wrow0 = blockIdx.x * KNN_BM + wave * 32;      // this wave's rows: wrow0 .. wrow0 + 31
  const bool active = wrow0 < nq;                         // wave-uniform; an idle wave still stages and meets the barriers
  const int seg = blockIdx.y;
  const int st0 = seg * p.seg_stages;
  const int st_all = (nl + BN - 1) / BN;
  const int nst = min(p.seg_stages, st_all - st0);        // >= 1: the host launches no empty segment

  float4 a[16];                                           // A operand: row wrow0 + r, k = 8 q + 4 h + e
  {
    const float* qr = p.q + static_cast<int64_t>(min(wrow0 + r, nq - 1)) * D + 4 * h;
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = *reinterpret_cast<const float4*>(qr + 8 * q);
  }
  float rowp[16];                                         // per accumulator row: 1/|q| (cosine) or |q|^2 (euclidean)
  int skp[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = min(wrow0 + acc_row(v, h), nq - 1);
    rowp[v] = METRIC == KNN_COSINE ? p.qstat[nq + row] : (METRIC == KNN_EUCLIDEAN ? p.qstat[row] : 0.f);
    skp[v] = p.skip ? p.skip[row] : -1;
  }
  float lv[16][1], thr[16];
  int li[16][1];
#pragma unroll
  for (int v = 0; v < 16; ++v) { lv[v][0] = -INFINITY; li[v][0] = -1; thr[v] = -INFINITY; }

  // every load above has landed before the first LDS-DMA is counted
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  stage_dma<MDG_PREC_F32>(p.lib, static_cast<int64_t>(st0) * BN, smem, wave, lane, KNN_THREADS / 64);
  int cur = 0;
  for (int s = 0; s < nst; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of stage s landed
    __builtin_amdgcn_s_barrier();                         // ... and everyone's; every wave finished reading stage s - 1
    if (s + 1 < nst)
      stage_dma<MDG_PREC_F32>(p.lib, static_cast<int64_t>(st0 + s + 1) * BN, smem + (cur ^ 1) * STAGE_BYTES, wave, lane, KNN_THREADS / 64);
    const char* lds = smem + cur * STAGE_BYTES;
    cur ^= 1;
    if (!active) continue;
    const int col0 = (st0 + s) * BN;
    float cp[2];                                          // per column: 1/|l| (cosine) or |l|^2 (euclidean)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int jc = min(col0 + 32 * t + r, nl - 1);
      cp[t] = METRIC == KNN_COSINE ? p.lstat[nl + jc] : (METRIC == KNN_EUCLIDEAN ? p.lstat[jc] : 0.f);
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
    // values; lane (r, h) of block t holds column col0 + 32 t + r, rows wrow0 + acc_row(v, h)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = col0 + 32 * t + r;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float g = acc[t][v];
        float x;
        if constexpr (METRIC == KNN_COSINE) x = (g * rowp[v]) * cp[t];
        else if constexpr (METRIC == KNN_EUCLIDEAN) x = -((rowp[v] - 2.0f * g) + cp[t]);
        else x = g;
        acc[t][v] = (col < nl && col != skp[v]) ? x : -INFINITY;
      }
    }
    if constexpr (LISTS) {
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
            topk_insert<32>(lv[v], li[v], thr[v], acc[t][v] > thr[v], acc[t][v], col0 + 32 * t + r, lane, k);
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) thr[v] = fmaxf(thr[v], fmaxf(acc[0][v], acc[1][v]));
    }
  }
  if (!active) return;
  if constexpr (LISTS) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = wrow0 + acc_row(v, h);
      if (r < k && row < nq) {
        const int64_t o = (static_cast<int64_t>(p.final ? 0 : seg) * nq + row) * k + r;
        float x = lv[v][0];
        if (METRIC == KNN_EUCLIDEAN && p.final) x = sqrtf(fmaxf(-x, 0.f));
        p.vals[o] = x;
        p.idx[o] = li[v][0];
      }
    }
  } else {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      float m = thr[v];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      const int row = wrow0 + acc_row(v, h);
      if (r == 0 && row < nq) p.vals[static_cast<int64_t>(seg) * nq + row] = m;
    }
  }
}

// One 32-lane group per query row; lane c holds entry c of the list.  The S partial lists arrive in ascending segment order.
__global__ __launch_bounds__(KNN_THREADS) void knn_merge(const float* __restrict__ pv, const int* __restrict__ pi, int nq, int k, int S,
                                                         int euclidean, float* __restrict__ vals, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63, c = lane & 31;
  const int row = (blockIdx.x * KNN_THREADS + threadIdx.x) >> 5;
  const int rr = min(row, nq - 1);
  float lv[1] = {-INFINITY}, thr = -INFINITY;
  int li[1] = {-1};
  const int cc = min(c, k - 1);
  float x = pv[static_cast<int64_t>(rr) * k + cc];
  int i = pi[static_cast<int64_t>(rr) * k + cc];
  for (int s = 0; s < S; ++s) {                           // S is uniform: topk_insert runs in wave-uniform control flow
    float nx = x;
    int ni = i;
    if (s + 1 < S) {
      const int64_t o = (static_cast<int64_t>(s + 1) * nq + rr) * k + cc;
      nx = pv[o];
      ni = pi[o];
    }
    topk_insert<32>(lv, li, thr, c < k && x > thr, x, i, lane, k);
    x = nx;
    i = ni;
  }
  if (row < nq && c < k) {
    const int64_t o = static_cast<int64_t>(row) * k + c;
    vals[o] = euclidean ? sqrtf(fmaxf(-lv[0], 0.f)) : lv[0];
    idx[o] = li[0];
  }
}

// One thread per (query, label column).  Binary (num_classes == 2): p1 = sum_j w_j lab[idx_j, c] for j ascending, p0 = sum_j w_j - p1;
// sums [nq][C][2].  Otherwise (C == 1): per-class sums, sums [nq][num_classes].  Prediction: the largest sum, lowest class on a tie.
__global__ __launch_bounds__(KNN_THREADS) void knn_vote(const float* __restrict__ vals, const int* __restrict__ idx,
                                                        const uint8_t* __restrict__ labels, int64_t nq, int k, int64_t C, int num_classes,
                                                        float T, uint8_t* __restrict__ pred, float* __restrict__ sums) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * KNN_THREADS + threadIdx.x;
  if (t >= nq * C) return;
  const int64_t i = t / C, c = t - i * C;
  const float* v = vals + i * k;
  const int* ix = idx + i * k;
  if (num_classes == 2) {
    float wsum = 0.f, p1 = 0.f;
    for (int j = 0; j < k; ++j) {
      const float w = expf(v[j] / T);
      wsum += w;
      p1 += w * static_cast<float>(labels[static_cast<int64_t>(ix[j]) * C + c]);
    }
    const float p0 = wsum - p1;
    sums[2 * t] = p0;
    sums[2 * t + 1] = p1;
    pred[t] = p1 > p0 ? 1 : 0;
  } else {
    float best = 0.f;
    int arg = 0;
    for (int cls = 0; cls < num_classes; ++cls) {
      float s = 0.f;
      for (int j = 0; j < k; ++j) {
        const float w = expf(v[j] / T);
        s += labels[ix[j]] == cls ? w : 0.f;
      }
      sums[i * num_classes + cls] = s;
      if (cls == 0 || s > best) { best = s; arg = cls; }
    }
    pred[i] = static_cast<uint8_t>(arg);
  }
}

struct KnnPlan {
  int S;                   // segments launched (none is empty)
  int seg_stages;          // 64-column stages per segment
};

KnnPlan knn_plan(int64_t nl, int segments) {
  const int64_t tiles = mdg_cdiv(nl, KNN_SEG);
  int64_t S = segments < 1 ? 1 : segments;
  if (S > tiles) S = tiles;
  const int64_t per = mdg_cdiv(tiles, S);
  return KnnPlan{static_cast<int>(mdg_cdiv(tiles, per)), static_cast<int>(per * (KNN_SEG / BN))};
}

constexpr int64_t KNN_MAX_ROWS = (int64_t(1) << 31) - KNN_BM - 1;

template <int METRIC, bool LISTS>
void knn_launch(const KnnArgs& a, int S, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(mdg_cdiv(a.nq, KNN_BM)), static_cast<unsigned>(S));
  hipLaunchKernelGGL((knn_sweep<METRIC, LISTS>), grid, dim3(KNN_THREADS), KNN_LDS, st, a);
}

}  // namespace

extern "C" int mdg_knn_max_k(void) { return TOPK_MAX_K; }

extern "C" int mdg_knn_default_segments(int64_t nq, int64_t nl) {
  if (nq < 1 || nl < 1) return 1;
  const int64_t blocks = mdg_cdiv(nq, KNN_BM), want = 2 * KNN_CUS, tiles = mdg_cdiv(nl, KNN_SEG);
  if (blocks >= want) return 1;
  const int64_t S = mdg_cdiv(want, blocks);
  return static_cast<int>(S < tiles ? S : tiles);
}

extern "C" size_t mdg_knn_topk_workspace_bytes(int64_t nq, int64_t nl, int k, int segments) {
  if (nq < 1 || nl < 1 || k < 1) return 0;
  const KnnPlan pl = knn_plan(nl, segments);
  if (pl.S == 1) return 0;
  return static_cast<size_t>(pl.S) * nq * k * (sizeof(float) + sizeof(int));
}

extern "C" int mdg_knn_topk(const float* q, const float* lib, int64_t nq, int64_t nl, int64_t d, int k, int metric, const int32_t* skip,
                            int segments, float* q_stats, float* lib_stats, float* vals, int32_t* idx, int* status, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const bool lists = (metric & MDG_KNN_NO_LISTS) == 0;
  metric &= ~MDG_KNN_NO_LISTS;
  MDG_CHECK_ARG(d == D, "mdg_knn_topk: only D = %d is supported (got %lld)", D, (long long)d);
  MDG_CHECK_ARG(nq >= 1 && nq <= KNN_MAX_ROWS && nl >= 1 && nl <= KNN_MAX_ROWS, "mdg_knn_topk: need 1 <= nq, nl < 2^31 - 128 (got %lld, %lld)",
                (long long)nq, (long long)nl);
  MDG_CHECK_ARG(metric == KNN_COSINE || metric == KNN_DOT || metric == KNN_EUCLIDEAN, "mdg_knn_topk: unknown metric %d", metric);
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K && k <= nl - (skip ? 1 : 0), "mdg_knn_topk: need 1 <= k <= min(%d, candidates per row) (got k = %d, nl = %lld%s)",
                TOPK_MAX_K, k, (long long)nl, skip ? ", one skipped" : "");
  MDG_CHECK_ARG(segments >= 1, "mdg_knn_topk: segments must be at least 1 (got %d)", segments);
  MDG_CHECK_ARG(q && lib && q_stats && lib_stats && vals && status && (idx || !lists), "mdg_knn_topk: null pointer");
  MDG_CHECK_ARG(mdg_aligned16(q) && mdg_aligned16(lib), "mdg_knn_topk: q and lib must be 16-byte aligned");
  const KnnPlan pl = knn_plan(nl, segments);
  MDG_CHECK_ARG(pl.S <= 65535, "mdg_knn_topk: %d segments > 65535", pl.S);
  const size_t need = lists ? mdg_knn_topk_workspace_bytes(nq, nl, k, segments) : 0;
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("mdg_knn_topk: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    mdg_set_error("mdg_knn_topk: hipMemsetAsync failed");
    return MDG_ELAUNCH;
  }
  const int zero_is_bad = metric == KNN_COSINE;
  hipLaunchKernelGGL(knn_prep, dim3(static_cast<unsigned>(mdg_cdiv(mdg_cdiv(nq, 32), KNN_THREADS / 64))), dim3(KNN_THREADS), 0, st, q,
                     static_cast<int>(nq), q_stats, zero_is_bad, status);
  hipLaunchKernelGGL(knn_prep, dim3(static_cast<unsigned>(mdg_cdiv(mdg_cdiv(nl, 32), KNN_THREADS / 64))), dim3(KNN_THREADS), 0, st, lib,
                     static_cast<int>(nl), lib_stats, zero_is_bad, status);
  MDG_CHECK_LAUNCH("knn_prep");
  const bool final = pl.S == 1 || !lists;
  float* pv = final ? vals : static_cast<float*>(workspace);
  int* pi = final ? idx : reinterpret_cast<int*>(pv + static_cast<size_t>(pl.S) * nq * k);
  KnnArgs a{q, TileSrc{lib, nullptr, nullptr, nl}, q_stats, lib_stats, skip, pv, pi, static_cast<int>(nq), static_cast<int>(nl), k,
            pl.seg_stages, final ? 1 : 0};
  if (!lists) {                                           // measurement: vals [S][nq] row maxima of the metric's values
    if (metric == KNN_COSINE) knn_launch<KNN_COSINE, false>(a, pl.S, st);
    else if (metric == KNN_DOT) knn_launch<KNN_DOT, false>(a, pl.S, st);
    else knn_launch<KNN_EUCLIDEAN, false>(a, pl.S, st);
    MDG_CHECK_LAUNCH("knn_sweep");
    return MDG_OK;
  }
  if (metric == KNN_COSINE) knn_launch<KNN_COSINE, true>(a, pl.S, st);
  else if (metric == KNN_DOT) knn_launch<KNN_DOT, true>(a, pl.S, st);
  else knn_launch<KNN_EUCLIDEAN, true>(a, pl.S, st);
  MDG_CHECK_LAUNCH("knn_sweep");
  if (!final) {
    hipLaunchKernelGGL(knn_merge, dim3(static_cast<unsigned>(mdg_cdiv(nq * 32, KNN_THREADS))), dim3(KNN_THREADS), 0, st, pv, pi,
                       static_cast<int>(nq), k, pl.S, metric == KNN_EUCLIDEAN ? 1 : 0, vals, idx);
    MDG_CHECK_LAUNCH("knn_merge");
  }
  return MDG_OK;
}

extern "C" int mdg_knn_vote(const float* vals, const int32_t* idx, const uint8_t* labels, int64_t nq, int64_t nl, int k, int64_t n_cols,
                            int num_classes, float T, uint8_t* pred, float* sums, void* stream) {
  MDG_CHECK_ARG(nq >= 0 && nl >= 1 && n_cols >= 1, "mdg_knn_vote: bad size (nq %lld, nl %lld, label columns %lld)", (long long)nq,
                (long long)nl, (long long)n_cols);
  MDG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "mdg_knn_vote: k must be in 1..%d (got %d)", TOPK_MAX_K, k);
  MDG_CHECK_ARG(num_classes >= 2 && num_classes <= 64, "mdg_knn_vote: num_classes must be in 2..64 (got %d)", num_classes);
  MDG_CHECK_ARG(num_classes == 2 || n_cols == 1, "mdg_knn_vote: %lld label columns need binary labels (num_classes = 2, got %d)",
                (long long)n_cols, num_classes);
  MDG_CHECK_ARG(T == T && T != 0.f, "mdg_knn_vote: T must be a non-zero number");
  if (nq == 0) return MDG_OK;
  MDG_CHECK_ARG(vals && idx && labels && pred && sums, "mdg_knn_vote: null pointer");
  hipLaunchKernelGGL(knn_vote, dim3(static_cast<unsigned>(mdg_cdiv(nq * n_cols, KNN_THREADS))), dim3(KNN_THREADS), 0,
                     static_cast<hipStream_t>(stream), vals, idx, labels, nq, k, n_cols, num_classes, T, pred, sums);
  MDG_CHECK_LAUNCH("knn_vote");
  return MDG_OK;
}
