// Pair-exclusion masks for the in-sweep screening products (mdg_bilinear_topk_masked, mdg_bilinear_select_*_masked): one bit
// per (head row, tail column), set = "this pair is not eligible" -- the known interactions a screening run leaves out.
//
// Layout (the one place its arithmetic lives: mdg_pair_mask_ld / mdg_pair_mask_plane_words):
//   mask [planes][ceil(n_head / 32)][ld] 32-bit words, ld = n_tail rounded up to 64;
//   word [p][i >> 5][j] holds the bit of row i, column j at position i & 31.
// A word is "32 rows of one column", because that is how the sweeps hold scores: a lane owns one column per accumulator and its
// rows lie in one 32-row block, so the lanes of a wave read consecutive words (pairmask.h).  The padding to 64 columns (one
// column tile) and to whole row blocks keeps every tile-wide read inside the plane.
//
// mdg_pair_mask_set: one thread per listed pair, one vector atomicOr per bit.  OR is commutative and idempotent: duplicates and
// any thread order give the same words.  A pair outside the mask is skipped, never stored.
#include "mdg_common.h"

namespace {

__global__ void pair_mask_set_kernel(unsigned* __restrict__ mask, int64_t n_planes, int64_t n_head, int64_t n_tail, int64_t ld,
                                     int64_t plane_words, const long long* __restrict__ heads, const long long* __restrict__ tails,
                                     const long long* __restrict__ planes, int64_t n_pairs, int symmetric) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= n_pairs) return;
  const int64_t h = heads[q], t = tails[q], pl = planes ? planes[q] : 0;
  if (h < 0 || h >= n_head || t < 0 || t >= n_tail || pl < 0 || pl >= n_planes) return;
  unsigned* const plane = mask + pl * plane_words;
  atomicOr(plane + (h >> 5) * ld + t, 1u << (h & 31));
  if (symmetric) atomicOr(plane + (t >> 5) * ld + h, 1u << (t & 31));      // n_head == n_tail (checked by the entry point)
}

}  // namespace

extern "C" int64_t mdg_pair_mask_ld(int64_t n_tail) { return n_tail <= 0 ? 0 : (n_tail + 63) / 64 * 64; }

extern "C" int64_t mdg_pair_mask_plane_words(int64_t n_head, int64_t n_tail) {
  return n_head <= 0 ? 0 : (n_head + 31) / 32 * mdg_pair_mask_ld(n_tail);
}

extern "C" int mdg_pair_mask_set(uint32_t* mask, int64_t n_planes, int64_t n_head, int64_t n_tail, const int64_t* heads,
                                 const int64_t* tails, const int64_t* planes, int64_t n_pairs, int symmetric, void* stream) {
  MDG_CHECK_ARG(n_planes >= 0 && n_head >= 0 && n_tail >= 0 && n_pairs >= 0, "mdg_pair_mask_set: negative size");
  MDG_CHECK_ARG(!symmetric || n_head == n_tail, "mdg_pair_mask_set: symmetric needs one drug set against itself (n_head %lld != n_tail %lld)",
                (long long)n_head, (long long)n_tail);
  MDG_CHECK_ARG(n_pairs < (int64_t(1) << 31) * 256, "mdg_pair_mask_set: too many pairs for one call (%lld)", (long long)n_pairs);
  if (n_pairs == 0 || n_planes == 0 || mdg_pair_mask_plane_words(n_head, n_tail) == 0) return MDG_OK;
  MDG_CHECK_ARG(mask && heads && tails, "mdg_pair_mask_set: null pointer");
  hipLaunchKernelGGL(pair_mask_set_kernel, dim3(static_cast<unsigned>(mdg_cdiv(n_pairs, 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<unsigned*>(mask), n_planes, n_head, n_tail, mdg_pair_mask_ld(n_tail),
                     mdg_pair_mask_plane_words(n_head, n_tail), reinterpret_cast<const long long*>(heads),
                     reinterpret_cast<const long long*>(tails), reinterpret_cast<const long long*>(planes), n_pairs, symmetric);
  MDG_CHECK_LAUNCH("mdg_pair_mask_set");
  return MDG_OK;
}
