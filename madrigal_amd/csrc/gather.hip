// Row gather across several source matrices of one width (mdg_gather_rows_multi): out[i] = row (idx[i] % rows_per_source) of
// source idx[i] / rows_per_source.  Stands for torch.cat(sources).index_select(0, idx) (equal-sized sources) without the
// concatenated copy: the 16 per-cell-line signature matrices of the tx encoder, the [str | kg | cv | tx] stack the uni-modal
// drugs read, the KG rows of a drug batch with the filler table as the second source.  The kernel can also write the gathered
// rows as the packed operand image of the dense block that consumes them (what mdg_pack_operand writes for the same rows).
#include "mdg_common.h"

namespace {

constexpr int MAX_SRC = MDG_GATHER_MAX_SOURCES;

struct GatherArgs {
  const float* src[MAX_SRC];
  int64_t rows[MAX_SRC];        // rows of each source: an index outside its source gathers a zero row
  int64_t ld[MAX_SRC];
  const int64_t* idx;
  int64_t n, rps;
  int n_src;
  int W, Wo, Kp;                // source width | width of the fp32 result (W padded to 4) | inner length of the image
  int groups;                   // 4-element groups per gathered row: max(Wo, Kp) / 4
  float* out; int64_t ldo;
  char* img; int x3;
};

// byte offset of the hi value of (row, k) in a bf16x3 image (linear.hip: per row and block of 32 k, 64 B of hi then 64 B of lo values)
__device__ __forceinline__ int64_t gather_img_off_x3(int64_t row, int64_t k, int64_t Kp) { return row * Kp * 4 + (k >> 5) * 128 + (k & 31) * 2; }

// VEC = floats per load: 4 (W % 4 == 0, rows 16-byte aligned), 2 (W even, rows 8-byte aligned: the 978-wide signatures) or 1.
// One thread per 4 consecutive columns of one gathered row, as in linear.hip's operand pre-pass.
template <int VEC>
__global__ __launch_bounds__(256) void gather_rows_multi_kernel(const GatherArgs a) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (q >= a.n * a.groups) return;
  const int64_t r = q / a.groups;
  const int k = static_cast<int>(q - r * a.groups) * 4;
  const int64_t i = a.idx[r];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i >= 0 && k < a.W) {
    const int64_t s = i / a.rps, row = i - s * a.rps;
    if (s < a.n_src && row < a.rows[s]) {
      const float* p = a.src[s] + row * a.ld[s] + k;
      if constexpr (VEC == 4) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else if constexpr (VEC == 2) {
        const f32x2 lo = *reinterpret_cast<const f32x2*>(p);
        v[0] = lo[0];
        v[1] = lo[1];
        if (k + 2 < a.W) {
          const f32x2 hi = *reinterpret_cast<const f32x2*>(p + 2);
          v[2] = hi[0];
          v[3] = hi[1];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < a.W) v[e] = p[e];
      }
    }
  }
  if (a.out && k < a.Wo) *reinterpret_cast<f32x4*>(a.out + r * a.ldo + k) = v;
  if (a.img && k < a.Kp) {
    bf16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      __bf16 h, l;
      mdg_split_bf16(v[e], h, l);
      hi[e] = h;
      lo[e] = l;
    }
    if (a.x3) {
      char* d = a.img + gather_img_off_x3(r, k, a.Kp);
      *reinterpret_cast<bf16x4*>(d) = hi;
      *reinterpret_cast<bf16x4*>(d + 64) = lo;
    } else {
      *reinterpret_cast<bf16x4*>(a.img + (r * a.Kp + k) * 2) = hi;
    }
  }
}

}  // namespace

extern "C" int mdg_gather_rows_multi(const float* const* sources_host, const int64_t* source_rows_host, const int64_t* source_ld_host,
                                     int n_sources, int64_t rows_per_source, int64_t width, const int64_t* idx, int64_t n, float* out,
                                     int64_t ldo, void* image, size_t image_bytes, int precision, void* stream) {
  MDG_CHECK_ARG(n_sources >= 1 && n_sources <= MAX_SRC, "mdg_gather_rows_multi: 1 to %d sources (got %d)", MAX_SRC, n_sources);
  MDG_CHECK_ARG(sources_host && source_rows_host && source_ld_host, "mdg_gather_rows_multi: null source table");
  MDG_CHECK_ARG(n >= 0 && rows_per_source > 0 && width > 0 && width < (1 << 24), "mdg_gather_rows_multi: bad size");
  MDG_CHECK_ARG(out || image, "mdg_gather_rows_multi: neither fp32 rows nor an image requested");
  if (n == 0) return MDG_OK;
  MDG_CHECK_ARG(idx, "mdg_gather_rows_multi: null index");
  const int64_t Wo = (width + 3) / 4 * 4, Kp = (Wo + 63) / 64 * 64;
  GatherArgs a{};
  unsigned align = 16;
  for (int s = 0; s < n_sources; ++s) {
    const int64_t rows = source_rows_host[s], ld = source_ld_host[s];
    MDG_CHECK_ARG(rows >= 0 && rows <= rows_per_source && ld >= width, "mdg_gather_rows_multi: source %d has %lld rows (ld %lld) for rows_per_source %lld, width %lld",
                  s, (long long)rows, (long long)ld, (long long)rows_per_source, (long long)width);
    MDG_CHECK_ARG(sources_host[s] || rows == 0, "mdg_gather_rows_multi: source %d is null", s);
    MDG_CHECK_ARG((reinterpret_cast<uintptr_t>(sources_host[s]) & 3u) == 0, "mdg_gather_rows_multi: source %d is not 4-byte aligned", s);
    a.src[s] = sources_host[s];
    a.rows[s] = rows;
    a.ld[s] = ld;
    // widest load every row of this source is aligned for
    const uintptr_t base = reinterpret_cast<uintptr_t>(sources_host[s]);
    while (align > 4 && ((base % align) != 0 || (static_cast<uint64_t>(ld) * 4) % align != 0)) align /= 2;
  }
  if (width % 4 != 0 && align > 8) align = 8;
  if (width % 2 != 0) align = 4;
  a.idx = idx; a.n = n; a.rps = rows_per_source; a.n_src = n_sources;
  a.W = static_cast<int>(width); a.Wo = static_cast<int>(Wo); a.Kp = image ? static_cast<int>(Kp) : 0;
  a.groups = static_cast<int>((image ? Kp : Wo) / 4);
  if (out) {
    MDG_CHECK_ARG(ldo >= Wo && ldo % 4 == 0 && mdg_aligned16(out), "mdg_gather_rows_multi: out must be 16-byte aligned with ldo >= width padded to 4, ldo %% 4 == 0");
    a.out = out; a.ldo = ldo;
  }
  if (image) {
    MDG_CHECK_ARG(precision == MDG_PREC_BF16X3 || precision == MDG_PREC_BF16, "mdg_gather_rows_multi: the image exists in the 16-bit operand modes only");
    const size_t need = static_cast<size_t>(n) * static_cast<size_t>(Kp) * (precision == MDG_PREC_BF16X3 ? 4 : 2);
    if (image_bytes < need || !mdg_aligned16(image)) {
      mdg_set_error("mdg_gather_rows_multi: image of %zu bytes (16-byte aligned) required, got %zu", need, image_bytes);
      return MDG_EWORKSPACE;
    }
    a.img = static_cast<char*>(image); a.x3 = precision == MDG_PREC_BF16X3 ? 1 : 0;
  }
  const int64_t blocks = mdg_cdiv(n * a.groups, 256);
  MDG_CHECK_ARG(blocks < (1ll << 31), "mdg_gather_rows_multi: too many rows for one launch");
  const dim3 grid(static_cast<unsigned>(blocks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (align == 16) hipLaunchKernelGGL(gather_rows_multi_kernel<4>, grid, dim3(256), 0, st, a);
  else if (align == 8) hipLaunchKernelGGL(gather_rows_multi_kernel<2>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(gather_rows_multi_kernel<1>, grid, dim3(256), 0, st, a);
  MDG_CHECK_LAUNCH("mdg_gather_rows_multi");
  return MDG_OK;
}
