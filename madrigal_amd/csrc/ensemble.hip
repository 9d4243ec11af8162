// Checkpoint ensemble of the all-pairs bilinear head for gfx950.
//
//   P[l,i,j] = (sum_{k<K} sigmoid(z_head_k[i]^T W_sym_k[l] z_tail_k[j])) / K          K = 1..8 checkpoints
//
// (get_twosides_scores_wrapper / get_drugbank_scores_wrapper, madrigal/evaluate/predict.py:466-499, 582-614: sigmoid of the K
// checkpoints' raw scores, stacked and averaged on the host.)  One sweep writes P once: 4 B per probability whatever K is.
//
// Per model, the logit is the head's own arithmetic (bilinear.hip, general kernel): T = z_head[rows] . W_sym[l] on the matrix
// cores, rounded to fp32 and kept as the MFMA A operand, times 64-row tail tiles staged in LDS by LDS-DMA; the same products in
// the same order (compute_tile: three bf16 products per k step in MDG_PREC_BF16X3, 32x32x2f32 in MDG_PREC_F32).  The sigmoid is
// 1 / (1 + expf(-s)) as in MDG_EPI_STORE_SIGMOID; the K sigmoids are summed in fp32 in model order and divided once by K.
//
// Where the K operands live: a resident T is 64 VGPRs per lane, so only one model's T is held at a time.  A workgroup (4 waves,
// 128 head rows of one outcome, one wave per SIMD with 512 VGPRs) walks its tail tiles in chunks of CH tiles; for every chunk it
// rebuilds T_k for k = 0..K-1 and sweeps the chunk with it, the running sum of sigmoids of the chunk (CH x 32 VGPRs) staying in
// registers across the models.
// The last model's stage turns the sum into P and stores it.  Rebuilding T costs 128 / (64 CH) of the chunk's MFMA work
// (K = 1 builds T once per row block and runs 8 waves of 32 rows, like the head).
//
// Symmetric case (z_head_k == z_tail_k for every k): tiles on / right of the block diagonal are computed, each stored as rows and
// as its transpose (mirrored rows through a wave-private LDS slab).  Inside the diagonal block only entries with j >= i leave as
// rows and only j > i are mirrored, so P[l] is exactly symmetric (the single-model sweep writes its diagonal block in full).
//
// Stores are 4-byte buffer stores, lane = column: 128-byte row segments on the pitched layout (ops.empty_scores), any ldo and
// alignment accepted, ragged rows / columns dropped by the buffer range or a 0xFFFFFFFF offset.  Waits: per stage and wave the
// vector-memory stream is [LDS-DMA of the next tile][32 row stores (+ 32 mirrored)], so `s_waitcnt vmcnt(32)` retires the DMA and
// leaves the youngest stores in flight (in-order retirement, see bilinear.hip's main loop); a stage that follows a T rebuild or
// issued no stores waits vmcnt(0).
//
// build_t, pick, sigmoid_head and the constants of the layout live in ensemble_sweep.h, which the four reducing products of this
// sweep (ensemble_topk / _select / _bincount / _profile.hip) include as well.
#include "ensemble_sweep.h"

namespace {

// waves per workgroup: K >= 2 one per SIMD (512 VGPRs: T, the chunk's running sums), K = 1 two per SIMD like the head
template <bool ONE> constexpr int kWaves = ONE ? 8 : ENS_NW;
constexpr int BM_MAX = 32 * 8;         // the most head rows per workgroup
template <int NW> constexpr int kLds = 2 * STAGE_BYTES + NW * SLAB_BYTES;   // stage buffers + one slab per wave

struct EnsembleArgs : EnsOperands {
  float* out;
  int64_t n_head, n_tail, ldo;
  int n_models;
  int stagger;
};

// ONE: K == 1 (T built once per row block and held for the whole sweep, no running sums)
template <int MODE, bool SYM, bool ONE, int CH>
__global__ __launch_bounds__(64 * kWaves<ONE>, 1) void ensemble_sigmoid_kernel(const EnsembleArgs p) {
  constexpr int NW = kWaves<ONE>, BM = 32 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t l = blockIdx.y, N = p.n_tail, ld = p.ldo;
  const int K = ONE ? 1 : p.n_models;
  const float kf = static_cast<float>(K);
  char* const slab = smem + 2 * STAGE_BYTES + wave * SLAB_BYTES;
  float* const out_l = p.out + l * p.n_head * ld;
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
    const __amdgpu_buffer_rsrc_t rs_rows =
        __builtin_amdgcn_make_buffer_rsrc(out_l + row0 * ld, 0, static_cast<int>(slab_rows * ld * 4), 0x00020000);
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
          stage_dma<MODE>(zt, static_cast<int64_t>(tile_of(s0)) * BN, smem + par * STAGE_BYTES, wave, lane, NW);
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
            if (stored) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");      // this tile landed; the youngest 32 stores stay in flight
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                                       // ... for every wave; every wave is done with the other buffer
            char* const cur = smem + par * STAGE_BYTES;
            char* const nxt = smem + (par ^ 1) * STAGE_BYTES;
            prefetched = false;
            if (ci + 1 < nc) {
              stage_dma<MODE>(zt, static_cast<int64_t>(tile_of(s0 + ci + 1)) * BN, nxt, wave, lane, NW);
              prefetched = true;
            } else if (ONE && c + 1 < nch) {       // one model: T stays resident, the sweep runs on into the next chunk
              stage_dma<MODE>(zt, static_cast<int64_t>(tile_of(s0 + nc)) * BN, nxt, wave, lane, NW);
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
              float (&pr)[2][16] = psum[ci];       // in place: P = sum / K
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) pr[t][v] = pr[t][v] / kf;
              // byte offsets in 32 bits (the slab is < 2^31 bytes): a lane base plus a wave-uniform row step per register
              const unsigned lrow_base = static_cast<unsigned>(((wave * 32 + 4 * h) * ld + tcol0 + r) * 4);
              const int diag_d = static_cast<int>(tcol0 + r - (row0 + wave * 32 + 4 * h));    // col - row at v = 0, t = 0
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                  const int dv = (v & 3) + 8 * (v >> 2);
                  const bool ok = tcol0 + 32 * t + r < N && (!diag || diag_d + 32 * t - dv >= 0);
                  const unsigned off = ok ? lrow_base + static_cast<unsigned>((dv * ld + 32 * t) * 4) : 0xFFFFFFFFu;
                  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pr[t][v]), rs_rows, off, 0, 0);
                }
              if constexpr (SYM) {
                // tile column-major in the slab ([64 columns][32 rows]), then tile column 2q + h = output row tcol0 + 2q + h, lane r =
                // output column row0 + 32 wave + r
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                  for (int g = 0; g < 4; ++g) {
                    const f32x4 v4 = {pr[t][4 * g], pr[t][4 * g + 1], pr[t][4 * g + 2], pr[t][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(slab + (32 * t + r) * 128 + (8 * g + 4 * h) * 4) = v4;
                  }
                const int64_t mrows = (N - tcol0) < BN ? (N - tcol0) : BN;
                const __amdgpu_buffer_rsrc_t rs_m =
                    __builtin_amdgcn_make_buffer_rsrc(out_l + tcol0 * ld, 0, static_cast<int>(mrows * ld * 4), 0x00020000);
                const int64_t gi = row0 + wave * 32 + r;
                const unsigned m_base = static_cast<unsigned>((h * ld + gi) * 4);
                const int m_d = static_cast<int>(tcol0 + h - gi);                // output row - output column at q = 0
#pragma unroll
                for (int q = 0; q < 32; ++q) {
                  if ((q & 7) == 0) __builtin_amdgcn_sched_barrier(0);         // a few slab reads in flight, not all 32
                  const float val = *reinterpret_cast<const float*>(slab + (2 * q + h) * 128 + r * 4);
                  const bool ok = gi < N && (!diag || m_d + 2 * q > 0);
                  const unsigned off = ok ? m_base + static_cast<unsigned>(2 * q * ld * 4) : 0xFFFFFFFFu;
                  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rs_m, off, 0, 0);
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

// hi / lo bf16 images of K fp32 operands in one launch (grid.y = model)
struct SplitJobs {
  const float* x[2 * MAXK];
  __bf16* hi[2 * MAXK];
  __bf16* lo[2 * MAXK];
  int64_t n4[2 * MAXK];
};

__global__ void ensemble_split_kernel(const SplitJobs j) {
  const int m = blockIdx.y;
  const float* x = j.x[0];
  __bf16 *hi = j.hi[0], *lo = j.lo[0];
  int64_t n4 = j.n4[0];
#pragma unroll
  for (int i = 1; i < 2 * MAXK; ++i)
    if (m == i) { x = j.x[i]; hi = j.hi[i]; lo = j.lo[i]; n4 = j.n4[i]; }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    bf16x4 hv, lv;
    __bf16 a, b;
    mdg_split_bf16(v.x, a, b); hv[0] = a; lv[0] = b;
    mdg_split_bf16(v.y, a, b); hv[1] = a; lv[1] = b;
    mdg_split_bf16(v.z, a, b); hv[2] = a; lv[2] = b;
    mdg_split_bf16(v.w, a, b); hv[3] = a; lv[3] = b;
    reinterpret_cast<bf16x4*>(hi)[i] = hv;
    reinterpret_cast<bf16x4*>(lo)[i] = lv;
  }
}

inline size_t ens_align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

template <int MODE>
int launch_ensemble(const EnsembleArgs& a, bool sym, int64_t n_labels, hipStream_t st) {
  const bool one = a.n_models == 1;
  const int nw = one ? kWaves<true> : kWaves<false>;
  const int nb = static_cast<int>(mdg_cdiv(a.n_head, 32 * nw));
  const dim3 block(64 * nw);
  if (sym) {
    const dim3 grid(static_cast<unsigned>((nb + 1) / 2), static_cast<unsigned>(n_labels));
    if (one) hipLaunchKernelGGL((ensemble_sigmoid_kernel<MODE, true, true, ENS_CH>), grid, block, kLds<kWaves<true>>, st, a);
    else hipLaunchKernelGGL((ensemble_sigmoid_kernel<MODE, true, false, ENS_CH>), grid, block, kLds<kWaves<false>>, st, a);
  } else {
    const dim3 grid(static_cast<unsigned>(nb), static_cast<unsigned>(n_labels));
    if (one) hipLaunchKernelGGL((ensemble_sigmoid_kernel<MODE, false, true, ENS_CH>), grid, block, kLds<kWaves<true>>, st, a);
    else hipLaunchKernelGGL((ensemble_sigmoid_kernel<MODE, false, false, ENS_CH>), grid, block, kLds<kWaves<false>>, st, a);
  }
  MDG_CHECK_LAUNCH("mdg_bilinear_ensemble_sigmoid");
  return MDG_OK;
}

size_t images_per_model(int64_t n_tail, int64_t n_labels, int64_t D_) {
  return 2 * (ens_align256(static_cast<size_t>(n_tail) * D_ * 2) + ens_align256(static_cast<size_t>(n_labels) * D_ * D_ * 2));
}

}  // namespace

extern "C" size_t mdg_bilinear_ensemble_sigmoid_workspace_bytes(int64_t n_head, int64_t n_tail, int64_t n_labels, int64_t D_,
                                                                int n_models, int precision) {
  (void)n_head;
  if (precision == MDG_PREC_F32 || n_tail <= 0 || n_labels <= 0 || D_ <= 0 || n_models <= 0) return 0;
  return static_cast<size_t>(n_models) * images_per_model(n_tail, n_labels, D_);
}

extern "C" int mdg_bilinear_ensemble_sigmoid(const float* const* z_head_host, const float* const* z_tail_host,
                                             const float* const* w_sym_host, int n_models, float* out, int64_t ldo, int64_t n_head,
                                             int64_t n_tail, int64_t n_labels, int64_t D_, int precision, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n_models >= 1 && n_models <= MAXK, "mdg_bilinear_ensemble_sigmoid: n_models must be in 1..%d (got %d)", MAXK, n_models);
  MDG_CHECK_ARG(D_ == D, "mdg_bilinear_ensemble_sigmoid: D must be %d (got %lld)", D, (long long)D_);
  MDG_CHECK_ARG(n_head >= 0 && n_tail >= 0 && n_labels >= 0, "mdg_bilinear_ensemble_sigmoid: negative size");
  MDG_CHECK_ARG(ldo >= n_tail, "mdg_bilinear_ensemble_sigmoid: row pitch %lld < n_tail %lld", (long long)ldo, (long long)n_tail);
  MDG_CHECK_ARG(n_labels <= 65535, "mdg_bilinear_ensemble_sigmoid: n_labels %lld > 65535 per call", (long long)n_labels);
  MDG_CHECK_ARG(ldo * BM_MAX * 4 < (int64_t(1) << 31), "mdg_bilinear_ensemble_sigmoid: row pitch %lld too large", (long long)ldo);
  MDG_CHECK_ARG(precision == MDG_PREC_F32 || precision == MDG_PREC_BF16X3,
                "mdg_bilinear_ensemble_sigmoid: precision %d not offered (MDG_PREC_F32 or MDG_PREC_BF16X3)", precision);
  const size_t need = mdg_bilinear_ensemble_sigmoid_workspace_bytes(n_head, n_tail, n_labels, D_, n_models, precision);
  if (need && (!workspace || workspace_bytes < need || !mdg_aligned16(workspace))) {
    mdg_set_error("mdg_bilinear_ensemble_sigmoid: workspace of %zu bytes (16-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  if (n_head == 0 || n_tail == 0 || n_labels == 0) return MDG_OK;
  MDG_CHECK_ARG(z_head_host && z_tail_host && w_sym_host && out, "mdg_bilinear_ensemble_sigmoid: null pointer");
  bool sym = n_head == n_tail;
  EnsembleArgs a{};
  for (int k = 0; k < n_models; ++k) {
    MDG_CHECK_ARG(z_head_host[k] && z_tail_host[k] && w_sym_host[k], "mdg_bilinear_ensemble_sigmoid: null pointer for model %d", k);
    MDG_CHECK_ARG(mdg_aligned16(z_head_host[k]) && mdg_aligned16(z_tail_host[k]) && mdg_aligned16(w_sym_host[k]),
                  "mdg_bilinear_ensemble_sigmoid: z_head, z_tail and w_sym must be 16-byte aligned (model %d)", k);
    sym = sym && z_head_host[k] == z_tail_host[k];
  }
  a.out = out;
  a.n_head = n_head; a.n_tail = n_tail; a.ldo = ldo;
  a.n_models = n_models;
  a.stagger = 1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int k = 0; k < MAXK; ++k) {            // unused slots repeat model 0 (never read)
    const int m = k < n_models ? k : 0;
    a.z_head[k] = z_head_host[m];
    a.zt[k].nrows = n_tail;
    a.w[k].nrows = D;
  }
  if (precision == MDG_PREC_F32) {
    for (int k = 0; k < MAXK; ++k) {
      const int m = k < n_models ? k : 0;
      a.zt[k].f32 = z_tail_host[m];
      a.w[k].f32 = w_sym_host[m];
    }
    return launch_ensemble<MDG_PREC_F32>(a, sym, n_labels, st);
  }
  // split-bf16 images of every model's z_tail and W_sym: [zhi | zlo | whi | wlo] per model
  const size_t zb = ens_align256(static_cast<size_t>(n_tail) * D * 2), wb = ens_align256(static_cast<size_t>(n_labels) * D * D * 2);
  char* ws = static_cast<char*>(workspace);
  SplitJobs jobs{};
  int64_t most = 0;
  for (int k = 0; k < n_models; ++k) {
    char* base = ws + static_cast<size_t>(k) * images_per_model(n_tail, n_labels, D);
    __bf16* zhi = reinterpret_cast<__bf16*>(base);
    __bf16* zlo = reinterpret_cast<__bf16*>(base + zb);
    __bf16* whi = reinterpret_cast<__bf16*>(base + 2 * zb);
    __bf16* wlo = reinterpret_cast<__bf16*>(base + 2 * zb + wb);
    jobs.x[2 * k] = z_tail_host[k]; jobs.hi[2 * k] = zhi; jobs.lo[2 * k] = zlo; jobs.n4[2 * k] = n_tail * D / 4;
    jobs.x[2 * k + 1] = w_sym_host[k]; jobs.hi[2 * k + 1] = whi; jobs.lo[2 * k + 1] = wlo; jobs.n4[2 * k + 1] = n_labels * D * D / 4;
    most = jobs.n4[2 * k + 1] > most ? jobs.n4[2 * k + 1] : most;
    most = jobs.n4[2 * k] > most ? jobs.n4[2 * k] : most;
    a.zt[k].hi = zhi; a.zt[k].lo = zlo;
    a.w[k].hi = whi; a.w[k].lo = wlo;
  }
  for (int k = n_models; k < MAXK; ++k) { a.zt[k] = a.zt[0]; a.w[k] = a.w[0]; }
  const int64_t blocks = mdg_cdiv(most, 256) < 4096 ? mdg_cdiv(most, 256) : 4096;
  hipLaunchKernelGGL(ensemble_split_kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(2 * n_models)), dim3(256), 0, st, jobs);
  MDG_CHECK_LAUNCH("mdg_bilinear_ensemble_sigmoid(split)");
  return launch_ensemble<MDG_PREC_BF16X3>(a, sym, n_labels, st);
}
