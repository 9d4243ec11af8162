// Multi-tensor AdamW for the finetune step (train_ddi_batch.py:350, madrigal/utils.py:600-613: torch.optim.AdamW over
// parameter groups with their own lr / weight decay).  One launch updates every parameter tensor: the host passes a
// table of 4096-element chunks (param / grad / exp_avg / exp_avg_sq pointers) and per-tensor hyper-parameters.
//
// The reference's two other optimizers run over the same chunk tables: RAdam (madrigal/utils.py:602, torch.optim.RAdam) in one
// launch, LARS (madrigal/utils.py:628-662, pretrain.py:175-176) in three -- per-chunk norms, per-tensor trust ratio, update.
#include "mdg_common.h"

namespace {

constexpr int OPT_CHUNK = 4096;

// hyper[tensor] = {lr, beta1, beta2, eps, weight_decay, 1/bias_correction1, 1/sqrt(bias_correction2), unused}
__global__ __launch_bounds__(256) void adamw_multi_kernel(const int64_t* __restrict__ ptrs, const int32_t* __restrict__ lens,
                                                          const int32_t* __restrict__ tensor_of_chunk, const float* __restrict__ hyper) {
  const int64_t c = blockIdx.x;
  float* __restrict__ p = reinterpret_cast<float*>(ptrs[4 * c + 0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(ptrs[4 * c + 1]);
  float* __restrict__ m = reinterpret_cast<float*>(ptrs[4 * c + 2]);
  float* __restrict__ v = reinterpret_cast<float*>(ptrs[4 * c + 3]);
  const float* h = hyper + 8 * tensor_of_chunk[c];
  const float lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], ibc1 = h[5], isbc2 = h[6];
  const int n = lens[c];
  for (int i = threadIdx.x; i < n; i += 256) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float pi = p[i] * (1.0f - lr * wd);                       // decoupled weight decay
    p[i] = pi - (lr * ibc1) * mi / (sqrtf(vi) * isbc2 + eps);
  }
}

// hyper[tensor] = {lr, beta1, beta2, eps, weight_decay, 1/bias_correction1, rect * sqrt(bias_correction2) or 0, decoupled}
__global__ __launch_bounds__(256) void radam_multi_kernel(const int64_t* __restrict__ ptrs, const int32_t* __restrict__ lens,
                                                          const int32_t* __restrict__ tensor_of_chunk, const float* __restrict__ hyper) {
  const int64_t c = blockIdx.x;
  float* __restrict__ p = reinterpret_cast<float*>(ptrs[4 * c + 0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(ptrs[4 * c + 1]);
  float* __restrict__ m = reinterpret_cast<float*>(ptrs[4 * c + 2]);
  float* __restrict__ v = reinterpret_cast<float*>(ptrs[4 * c + 3]);
  const float* h = hyper + 8 * tensor_of_chunk[c];
  const float lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], ibc1 = h[5], rect = h[6];
  const bool decoupled = h[7] != 0.0f;
  const float shrink = decoupled ? 1.0f - lr * wd : 1.0f, l2 = decoupled ? 0.0f : wd;
  const int n = lens[c];
  for (int i = threadIdx.x; i < n; i += 256) {
    float pi = p[i];
    const float gi = g[i] + l2 * pi;                                // L2 decay joins the gradient (torch's default)
    pi *= shrink;
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    // rho_t <= 5 (rect == 0): the variance of the adaptive rate is not tractable yet, plain bias-corrected momentum
    const float step = rect > 0.0f ? rect / (sqrtf(vi) + eps) : 1.0f;
    p[i] = pi - (lr * ibc1) * mi * step;
  }
}

// ---- LARS.  A thread owns groups of four consecutive elements (group j of thread t = elements 4 (t + 256 j) ..+3); a group is one
// 16-byte access when the chunk's three bases allow it and four 4-byte ones otherwise, so the order of every sum -- and with it
// every bit of the result -- is the same for aligned and unaligned parameter views.
constexpr int LARS_HYPER = 5;                                        // {lr, weight_decay, momentum, trust_coefficient, scaled}

__device__ __forceinline__ f32x4 lars_load4(const float* __restrict__ x, int i, int n, bool vec) {
  if (vec && i + 4 <= n) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = i + e < n ? x[i + e] : 0.0f;
  return r;
}
__device__ __forceinline__ void lars_store4(float* __restrict__ x, int i, int n, bool vec, f32x4 r) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<f32x4*>(x + i) = r;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) x[i + e] = r[e];
}

// (a) partials[chunk] = {sum p^2, sum (g + wd p)^2} over the chunk, chunks of the scaled (ndim > 1) tensors only
__global__ __launch_bounds__(256) void lars_norm_kernel(const int64_t* __restrict__ ptrs, const int32_t* __restrict__ lens,
                                                        const int32_t* __restrict__ tensor_of_chunk, const float* __restrict__ hyper,
                                                        f32x2* __restrict__ partials) {
  const int64_t c = blockIdx.x;
  const float* h = hyper + LARS_HYPER * tensor_of_chunk[c];
  if (h[4] == 0.0f) return;                                          // block-uniform
  const float wd = h[1];
  const float* __restrict__ p = reinterpret_cast<const float*>(ptrs[3 * c + 0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(ptrs[3 * c + 1]);
  const bool vec = ((ptrs[3 * c + 0] | ptrs[3 * c + 1]) & 15) == 0;
  const int n = lens[c];
  float sp = 0.0f, su = 0.0f;
  for (int i = 4 * threadIdx.x; i < n; i += 1024) {
    const f32x4 pv = lars_load4(p, i, n, vec), gv = lars_load4(g, i, n, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = gv[e] + wd * pv[e];
      sp += pv[e] * pv[e];
      su += u * u;
    }
  }
  sp = mdg_wave_sum(sp);                                             // xor butterfly: every lane ends with the same bits
  su = mdg_wave_sum(su);
  __shared__ f32x2 wave_part[4];
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = f32x2{sp, su};
  __syncthreads();
  if (threadIdx.x == 0) {
    f32x2 s = wave_part[0];
    for (int w = 1; w < 4; ++w) s += wave_part[w];                   // waves 0..3 in order
    partials[c] = s;
  }
}

// (b) one block per tensor: q = trust_coefficient |p| / |u| (1 when a norm is 0, and for the unscaled tensors).  The few hundred
// partials of a tensor are summed in double, thread t taking partials t, t + 256, ..., then the fixed tree.
__global__ __launch_bounds__(256) void lars_trust_kernel(const f32x2* __restrict__ partials, const int32_t* __restrict__ first_chunk,
                                                         const int32_t* __restrict__ n_chunks_of, const float* __restrict__ hyper,
                                                         float* __restrict__ q) {
  const int t = blockIdx.x;
  const float* h = hyper + LARS_HYPER * t;
  if (h[4] == 0.0f) {
    if (threadIdx.x == 0) q[t] = 1.0f;
    return;
  }
  const f32x2* part = partials + first_chunk[t];
  const int n = n_chunks_of[t];
  double sp = 0.0, su = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const f32x2 v = part[i];
    sp += static_cast<double>(v[0]);
    su += static_cast<double>(v[1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sp += __shfl_xor(sp, o, 64);
    su += __shfl_xor(su, o, 64);
  }
  __shared__ double wave_part[4][2];
  if ((threadIdx.x & 63) == 0) {
    wave_part[threadIdx.x >> 6][0] = sp;
    wave_part[threadIdx.x >> 6][1] = su;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      sp += wave_part[w][0];
      su += wave_part[w][1];
    }
    q[t] = (sp > 0.0 && su > 0.0) ? static_cast<float>(static_cast<double>(h[3]) * sqrt(sp) / sqrt(su)) : 1.0f;
  }
}

// (c) u = q (g + wd p) for the scaled tensors, g for the others;  mu <- momentum mu + u;  p <- p - lr mu
__global__ __launch_bounds__(256) void lars_update_kernel(const int64_t* __restrict__ ptrs, const int32_t* __restrict__ lens,
                                                          const int32_t* __restrict__ tensor_of_chunk, const float* __restrict__ hyper,
                                                          const float* __restrict__ q) {
  const int64_t c = blockIdx.x;
  const int t = tensor_of_chunk[c];
  const float* h = hyper + LARS_HYPER * t;
  const float lr = h[0], momentum = h[2];
  const bool scaled = h[4] != 0.0f;
  const float wd = scaled ? h[1] : 0.0f, qt = scaled ? q[t] : 1.0f;
  float* __restrict__ p = reinterpret_cast<float*>(ptrs[3 * c + 0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(ptrs[3 * c + 1]);
  float* __restrict__ mu = reinterpret_cast<float*>(ptrs[3 * c + 2]);
  const bool vec = ((ptrs[3 * c + 0] | ptrs[3 * c + 1] | ptrs[3 * c + 2]) & 15) == 0;
  const int n = lens[c];
  for (int i = 4 * threadIdx.x; i < n; i += 1024) {
    f32x4 pv = lars_load4(p, i, n, vec), mv = lars_load4(mu, i, n, vec);
    const f32x4 gv = lars_load4(g, i, n, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = scaled ? qt * (gv[e] + wd * pv[e]) : gv[e];
      mv[e] = momentum * mv[e] + u;
      pv[e] = pv[e] - lr * mv[e];
    }
    lars_store4(mu, i, n, vec, mv);
    lars_store4(p, i, n, vec, pv);
  }
}

}  // namespace

extern "C" int mdg_adamw_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int mdg_adamw_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                               int64_t n_chunks, void* stream) {
  MDG_CHECK_ARG(n_chunks >= 0 && n_chunks <= 0x7fffffff, "mdg_adamw_multi: bad chunk count");
  if (n_chunks == 0) return MDG_OK;
  MDG_CHECK_ARG(chunk_ptrs && chunk_lens && chunk_tensor && hyper, "mdg_adamw_multi: null table");
  hipLaunchKernelGGL(adamw_multi_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, static_cast<hipStream_t>(stream), chunk_ptrs,
                     chunk_lens, chunk_tensor, hyper);
  MDG_CHECK_LAUNCH("mdg_adamw_multi");
  return MDG_OK;
}

extern "C" int mdg_radam_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                               int64_t n_chunks, void* stream) {
  MDG_CHECK_ARG(n_chunks >= 0 && n_chunks <= 0x7fffffff, "mdg_radam_multi: bad chunk count");
  if (n_chunks == 0) return MDG_OK;
  MDG_CHECK_ARG(chunk_ptrs && chunk_lens && chunk_tensor && hyper, "mdg_radam_multi: null table");
  hipLaunchKernelGGL(radam_multi_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, static_cast<hipStream_t>(stream), chunk_ptrs,
                     chunk_lens, chunk_tensor, hyper);
  MDG_CHECK_LAUNCH("mdg_radam_multi");
  return MDG_OK;
}

// workspace: partials [n_chunks] x {p^2, u^2}, then q [n_tensors]
static size_t lars_partials_bytes(int64_t n_chunks) { return (static_cast<size_t>(n_chunks) * sizeof(f32x2) + 15) & ~static_cast<size_t>(15); }

extern "C" size_t mdg_lars_multi_workspace_bytes(int64_t n_chunks, int64_t n_tensors) {
  if (n_chunks <= 0 || n_tensors <= 0) return 0;
  return lars_partials_bytes(n_chunks) + static_cast<size_t>(n_tensors) * sizeof(float);
}

extern "C" int mdg_lars_multi(const int64_t* chunk_ptrs, const int32_t* chunk_lens, const int32_t* chunk_tensor, const float* hyper,
                              const int32_t* first_chunk, const int32_t* tensor_chunks, int64_t n_chunks, int64_t n_tensors, void* workspace,
                              size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n_chunks >= 0 && n_chunks <= 0x7fffffff, "mdg_lars_multi: bad chunk count");
  MDG_CHECK_ARG(n_tensors >= 0 && n_tensors <= n_chunks, "mdg_lars_multi: bad tensor count (every tensor owns at least one chunk)");
  if (n_chunks == 0) return MDG_OK;
  MDG_CHECK_ARG(n_tensors > 0, "mdg_lars_multi: chunks without tensors");
  MDG_CHECK_ARG(chunk_ptrs && chunk_lens && chunk_tensor && hyper && first_chunk && tensor_chunks, "mdg_lars_multi: null table");
  MDG_CHECK_ARG(workspace && mdg_aligned16(workspace), "mdg_lars_multi: workspace must be a 16-byte aligned device buffer");
  MDG_CHECK_ARG(workspace_bytes >= mdg_lars_multi_workspace_bytes(n_chunks, n_tensors), "mdg_lars_multi: workspace too small (%zu < %zu)",
                workspace_bytes, mdg_lars_multi_workspace_bytes(n_chunks, n_tensors));
  hipStream_t s = static_cast<hipStream_t>(stream);
  f32x2* partials = static_cast<f32x2*>(workspace);
  float* q = reinterpret_cast<float*>(static_cast<char*>(workspace) + lars_partials_bytes(n_chunks));
  hipLaunchKernelGGL(lars_norm_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, s, chunk_ptrs, chunk_lens, chunk_tensor, hyper,
                     partials);
  hipLaunchKernelGGL(lars_trust_kernel, dim3(static_cast<unsigned>(n_tensors)), dim3(256), 0, s, partials, first_chunk, tensor_chunks, hyper, q);
  hipLaunchKernelGGL(lars_update_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, s, chunk_ptrs, chunk_lens, chunk_tensor, hyper,
                     q);
  MDG_CHECK_LAUNCH("mdg_lars_multi");
  return MDG_OK;
}
