// Tile helpers of the all-pairs bilinear head (shared by bilinear.hip and ensemble.hip): the fp32 / split-bf16 / 16-bit
// operand images, the swizzled [64 tail rows][D] LDS tile, its staging by registers or LDS-DMA, the A fragment of T = z W_sym
// and the 32 x 64 product of one stage on the matrix cores.  Layout and k ordering: see the top of bilinear.hip.
#pragma once
#include "mdg_common.h"

namespace {
constexpr int D = 128;
constexpr int BN = 64;             // tail rows per stage
constexpr int STAGE_BYTES = BN * D * 4;   // fp32 tile, or bf16 hi (16 KB) + lo (16 KB)
constexpr int LO_OFF = BN * D * 2;

struct TileSrc {
  const float* f32;
  const __bf16* hi;
  const __bf16* lo;
  int64_t nrows;
};

// 16-bit operand images travel as bf16x8 containers; MDG_PREC_F16 stores IEEE half bits in them and casts at the MFMA.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <int MODE> struct AFrag;
template <> struct AFrag<MDG_PREC_F32> { float a[64]; };
template <> struct AFrag<MDG_PREC_BF16X3> { bf16x8 hi[8]; bf16x8 lo[8]; };
template <> struct AFrag<MDG_PREC_BF16> { bf16x8 hi[8]; };
template <> struct AFrag<MDG_PREC_F16> { bf16x8 hi[8]; };

// one rounded product per k-step (operands rounded to bf16 / fp16 once)
template <int MODE> constexpr bool kSingle16 = (MODE == MDG_PREC_BF16 || MODE == MDG_PREC_F16);

template <int MODE>
__device__ __forceinline__ f32x16 mma16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (MODE == MDG_PREC_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <int ROWB>
__device__ __forceinline__ int tile_off(int row, int chunk) {
  return row * ROWB + ((chunk ^ (row & 15)) << 4);
}

// ---- global -> registers -> LDS staging of one 64-row tile ---------------------------------
template <int MODE, int NW>
__device__ __forceinline__ void stage_load(const TileSrc& s, int64_t row0, int tid, u32x4 (&regs)[32 / NW]) {
  constexpr int NTHREADS = 64 * NW;
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int i = 0; i < 32 / NW; ++i) {
      const int g = tid + NTHREADS * i, row = g >> 5, c = g & 31;
      int64_t gr = row0 + row;
      gr = gr < s.nrows ? gr : s.nrows - 1;
      regs[i] = *reinterpret_cast<const u32x4*>(s.f32 + gr * D + c * 4);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16 / NW; ++i) {
      const int g = tid + NTHREADS * i, row = g >> 4, c = g & 15;
      int64_t gr = row0 + row;
      gr = gr < s.nrows ? gr : s.nrows - 1;
      regs[i] = *reinterpret_cast<const u32x4*>(s.hi + gr * D + c * 8);
      if constexpr (MODE == MDG_PREC_BF16X3) regs[16 / NW + i] = *reinterpret_cast<const u32x4*>(s.lo + gr * D + c * 8);
    }
  }
}

template <int MODE, int NW>
__device__ __forceinline__ void stage_write(char* lds, int tid, const u32x4 (&regs)[32 / NW]) {
  constexpr int NTHREADS = 64 * NW;
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int i = 0; i < 32 / NW; ++i) {
      const int g = tid + NTHREADS * i, row = g >> 5, c = g & 31;
      *reinterpret_cast<u32x4*>(lds + tile_off<512>(row, c)) = regs[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16 / NW; ++i) {
      const int g = tid + NTHREADS * i, row = g >> 4, c = g & 15;
      *reinterpret_cast<u32x4*>(lds + tile_off<256>(row, c)) = regs[i];
      if constexpr (MODE == MDG_PREC_BF16X3) *reinterpret_cast<u32x4*>(lds + LO_OFF + tile_off<256>(row, c)) = regs[16 / NW + i];
    }
  }
}


// ---- global -> LDS staging by LDS-DMA (no staging registers, asynchronous) ------------------
// One wave-instruction moves 1 KiB: LDS destination = wave-uniform base + lane*16 (linear), the
// per-lane SOURCE address carries the chunk swizzle (cdna guide rule 21: linear dest + swizzled
// source + the same swizzle on the read).  Completion is tracked by the issuing wave's vmcnt.
// Issued as inline asm so that hipcc's waitcnt pass does not see it (with the builtin it drains
// vmcnt(0) -- i.e. every score store in flight -- before the next ds_read); the waits are counted
// by hand in the kernel.  M0 carries the LDS base and is restored (cdna guide 5.7).
typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return static_cast<unsigned>(reinterpret_cast<size_t>((lds_void*)p));
}

__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst_uniform) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst_uniform);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(dst)
               : "memory");
}

// `nload` waves (0..nload-1) share the pieces of a tile; the other waves issue nothing.
template <int MODE>
__device__ __forceinline__ void stage_dma(const TileSrc& s, int64_t row0, char* lds, int wave, int lane, int nload) {
  if constexpr (MODE == MDG_PREC_F32) {
    for (int p = wave; p < 32; p += nload) {
      const int row = 2 * p + (lane >> 5), c = (lane & 31) ^ (row & 15);
      int64_t gr = row0 + row;
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.f32 + gr * D + c * 4, lds_addr(lds + p * 1024));
    }
  } else {
    for (int p = wave; p < 16; p += nload) {
      const int row = 4 * p + (lane >> 4), c = (lane & 15) ^ (row & 15);
      int64_t gr = row0 + row;
      gr = gr < s.nrows ? gr : s.nrows - 1;
      glds16(s.hi + gr * D + c * 8, lds_addr(lds + p * 1024));
      if constexpr (MODE == MDG_PREC_BF16X3) glds16(s.lo + gr * D + c * 8, lds_addr(lds + LO_OFF + p * 1024));
    }
  }
}

// ---- A fragment from 8 consecutive fp32 values --------------------------------------------
template <int MODE>
__device__ __forceinline__ void split8(const float4& x0, const float4& x1, bf16x8& hi, bf16x8& lo) {
  const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  if constexpr (MODE == MDG_PREC_F16) {
    f16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = static_cast<_Float16>(v[j]);       // round to nearest even
    hi = __builtin_bit_cast(bf16x8, t);
    lo = hi;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __bf16 a, b;
      mdg_split_bf16(v[j], a, b);
      hi[j] = a;
      lo[j] = b;
    }
  }
}

// rows of z_head straight from global memory (one-time, 512 B per lane)
template <int MODE>
__device__ __forceinline__ void afrag_from_global(AFrag<MODE>& A, const float* row, int h) {
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(row + 8 * q + 4 * h);
      A.a[4 * q + 0] = v.x; A.a[4 * q + 1] = v.y; A.a[4 * q + 2] = v.z; A.a[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float4 v0 = *reinterpret_cast<const float4*>(row + 16 * s + 8 * h);
      const float4 v1 = *reinterpret_cast<const float4*>(row + 16 * s + 8 * h + 4);
      bf16x8 hi, lo;
      split8<MODE>(v0, v1, hi, lo);
      A.hi[s] = hi;
      if constexpr (MODE == MDG_PREC_BF16X3) A.lo[s] = lo;
    }
  }
}

// half of the T fragment (k in [64*st, 64*st+64)) from this wave's [32][64] fp32 slab in LDS
template <int MODE>
__device__ __forceinline__ void afrag_from_slab(AFrag<MODE>& A, const char* slab, int st, int r, int h) {
  if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(slab + tile_off<256>(r, 2 * q + h));
      const int o = 4 * (8 * st + q);
      A.a[o + 0] = v.x; A.a[o + 1] = v.y; A.a[o + 2] = v.z; A.a[o + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float4 v0 = *reinterpret_cast<const float4*>(slab + tile_off<256>(r, 4 * s + 2 * h));
      const float4 v1 = *reinterpret_cast<const float4*>(slab + tile_off<256>(r, 4 * s + 2 * h + 1));
      bf16x8 hi, lo;
      split8<MODE>(v0, v1, hi, lo);
      A.hi[4 * st + s] = hi;
      if constexpr (MODE == MDG_PREC_BF16X3) A.lo[4 * st + s] = lo;
    }
  }
}

// ---- 32 rows (A, registers) x 64 staged tail rows (B, LDS) -> two 32x32 accumulators --------
template <int MODE>
__device__ __forceinline__ void compute_tile(const AFrag<MODE>& A, const char* lds, int r, int h, f32x16 (&acc)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = 32 * t + r;
    if constexpr (MODE == MDG_PREC_F32) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float4 b = *reinterpret_cast<const float4*>(lds + tile_off<512>(j, 2 * q + h));
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 0], b.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 1], b.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 2], b.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 3], b.w, acc[t], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(j, 2 * s + h));
        if constexpr (MODE == MDG_PREC_BF16X3) {
          const bf16x8 bl = *reinterpret_cast<const bf16x8*>(lds + LO_OFF + tile_off<256>(j, 2 * s + h));
          acc[t] = mma16<MODE>(A.lo[s], bh, acc[t]);
          acc[t] = mma16<MODE>(A.hi[s], bl, acc[t]);
        }
        acc[t] = mma16<MODE>(A.hi[s], bh, acc[t]);
      }
    }
  }
}

// The same products with the 32 score stores of the PREVIOUS tile (held in registers by the caller) spread evenly between
// the MFMAs instead of issued as one burst: `store_k(k)`, k = 0..31, issues store k.  B fragments are fetched one step
// ahead by hand because the scheduling barriers that pin the store positions also stop the compiler from hoisting them.
template <int MODE, typename StoreFn>
__device__ __forceinline__ void compute_tile_spread(const AFrag<MODE>& A, const char* lds, int r, int h, f32x16 (&acc)[2],
                                                    StoreFn&& store_k) {
  if constexpr (MODE == MDG_PREC_F32) {
    float4 b = *reinterpret_cast<const float4*>(lds + tile_off<512>(r, h));
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int t = i >> 4, q = i & 15;
      float4 nb = b;
      if (i + 1 < 32) nb = *reinterpret_cast<const float4*>(lds + tile_off<512>(32 * ((i + 1) >> 4) + r, 2 * ((i + 1) & 15) + h));
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 0], b.x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 1], b.y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 2], b.z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a[4 * q + 3], b.w, acc[t], 0, 0, 0);
      store_k(i);
      __builtin_amdgcn_sched_barrier(0);
      b = nb;
    }
  } else {
    bf16x8 bh = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(r, h)), bl = bh;
    if constexpr (MODE == MDG_PREC_BF16X3) bl = *reinterpret_cast<const bf16x8*>(lds + LO_OFF + tile_off<256>(r, h));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = i >> 3, s = i & 7;
      bf16x8 nbh = bh, nbl = bl;
      if (i + 1 < 16) {
        const int j = 32 * ((i + 1) >> 3) + r, c = 2 * ((i + 1) & 7) + h;
        nbh = *reinterpret_cast<const bf16x8*>(lds + tile_off<256>(j, c));
        if constexpr (MODE == MDG_PREC_BF16X3) nbl = *reinterpret_cast<const bf16x8*>(lds + LO_OFF + tile_off<256>(j, c));
      }
      if constexpr (MODE == MDG_PREC_BF16X3) {
        acc[t] = mma16<MODE>(A.lo[s], bh, acc[t]);
        store_k(2 * i);
        acc[t] = mma16<MODE>(A.hi[s], bl, acc[t]);
        store_k(2 * i + 1);
        acc[t] = mma16<MODE>(A.hi[s], bh, acc[t]);
      } else {
        acc[t] = mma16<MODE>(A.hi[s], bh, acc[t]);
        store_k(2 * i);
        store_k(2 * i + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      bh = nbh;
      bl = nbl;
    }
  }
}

// accumulator register v of lane (r,h) is element [row (v&3)+8(v>>2)+4h][col r] of the 32x32 tile
__device__ __forceinline__ int acc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// ---- 16-bit destinations (store16.hip, ensemble_store16.hip): one rounding to nearest even (a plain cast; fp16 overflow becomes
// +-inf) -> the bits of an IEEE half (MDG_SCORE_F16) or a bfloat16 (MDG_SCORE_BF16)
template <int TY>
__device__ __forceinline__ unsigned round16(float x) {
  if constexpr (TY == MDG_SCORE_F16) return __builtin_bit_cast(unsigned short, static_cast<_Float16>(x));
  else return __builtin_bit_cast(unsigned short, static_cast<__bf16>(x));
}

// ---- pre-pass: the 16-bit operand images of z_tail and W_sym (the images mdg_bilinear_allpairs makes) ----------------------
template <int MODE>
__global__ void operand_images_kernel(const float* __restrict__ x, __bf16* __restrict__ hi, __bf16* __restrict__ lo, int64_t n4) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  const float f[4] = {v.x, v.y, v.z, v.w};
  if constexpr (MODE == MDG_PREC_F16) {
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    f16x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = static_cast<_Float16>(f[c]);
    reinterpret_cast<f16x4*>(hi)[i] = o;
  } else {
    bf16x4 hv, lw;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      __bf16 a, b;
      mdg_split_bf16(f[c], a, b);
      hv[c] = a;
      lw[c] = b;
    }
    reinterpret_cast<bf16x4*>(hi)[i] = hv;
    if constexpr (MODE == MDG_PREC_BF16X3) reinterpret_cast<bf16x4*>(lo)[i] = lw;
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// Workspace of the images, laid out zhi | whi | zlo | wlo (the lo halves in bf16x3 only), every part 256-byte aligned; fp32 needs none.
inline size_t head_images_workspace_bytes(int64_t n_tail, int64_t n_labels, int64_t D_, int precision) {
  if (precision == MDG_PREC_F32 || n_tail <= 0 || n_labels <= 0 || D_ <= 0) return 0;
  const size_t z = align256(static_cast<size_t>(n_tail) * D_ * 2), w = align256(static_cast<size_t>(n_labels) * D_ * D_ * 2);
  return precision == MDG_PREC_BF16X3 ? 2 * (z + w) : (z + w);
}

// Points the two operands at what the kernels of MODE read: the caller's fp32 arrays, or their images, made in `ws` on the stream
// (two launches; the caller checks them).
template <int MODE>
void make_head_images(TileSrc& zt, TileSrc& w, const float* z_tail, const float* w_sym, int64_t n_tail, int64_t n_labels, char* ws, hipStream_t st) {
  if constexpr (MODE == MDG_PREC_F32) {
    zt.f32 = z_tail;
    w.f32 = w_sym;
  } else {
    const size_t zb = align256(static_cast<size_t>(n_tail) * D * 2), wb = align256(static_cast<size_t>(n_labels) * D * D * 2);
    const bool x3 = MODE == MDG_PREC_BF16X3;
    __bf16* zhi = reinterpret_cast<__bf16*>(ws);
    __bf16* whi = reinterpret_cast<__bf16*>(ws + zb);
    __bf16* zlo = x3 ? reinterpret_cast<__bf16*>(ws + zb + wb) : nullptr;
    __bf16* wlo = x3 ? reinterpret_cast<__bf16*>(ws + 2 * zb + wb) : nullptr;
    const int64_t z4 = n_tail * D / 4, w4 = n_labels * D * D / 4;
    hipLaunchKernelGGL(operand_images_kernel<MODE>, dim3(static_cast<unsigned>(mdg_cdiv(z4, 256))), dim3(256), 0, st, z_tail, zhi, zlo, z4);
    hipLaunchKernelGGL(operand_images_kernel<MODE>, dim3(static_cast<unsigned>(mdg_cdiv(w4, 256))), dim3(256), 0, st, w_sym, whi, wlo, w4);
    zt.hi = zhi; zt.lo = zlo;
    w.hi = whi; w.lo = wlo;
  }
}

}  // namespace
