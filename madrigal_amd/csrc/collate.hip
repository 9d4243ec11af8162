// On-device batch collation from a device-resident drug store (madrigal_amd/collate.py): what the reference's DrugCLCollator
// does on the host for every batch (madrigal/data/data.py:1479-1501).
//   mdg_collate_offsets   ids -> store rows, exclusive scans of the per-drug atom / edge counts, totals and a status word
//   mdg_collate_molecules the packed molecule batch AND its destination-sorted aggregation plan, one pass over the output rows
//   mdg_collate_rows      exact-width row gathers of stacked equal-shaped tables (16 signature matrices, dosages, cell viability)
// Plain loads and vector stores only; every output element has exactly one writer, so the result is a pure function of the inputs.
#include "mdg_common.h"

namespace {

constexpr int NODE_W = 67, BOND_W = 18, AUG_W = 20;         // floats per atom row (268 B), bond row (72 B), augmented bond row (80 B)
constexpr int SCAN_THREADS = 256, SCAN_PER_THREAD = 4, SCAN_CHUNK = SCAN_THREADS * SCAN_PER_THREAD;     // ids per workgroup

struct ScanPartial {          // one per workgroup of the count pass
  int64_t atoms, edges, bad, first_bad;
};

__device__ __forceinline__ int64_t collate_row_of(const int64_t* ids, int64_t i, const int64_t* id2row, int64_t n_table, int64_t n_mols) {
  const int64_t id = ids[i];
  if (id < 0 || id >= n_table) return -1;
  const int64_t r = id2row[id];
  return (r >= 0 && r < n_mols) ? r : -1;
}

// sum / min of one value per thread over the workgroup (256 threads); every thread receives the result
__device__ __forceinline__ int64_t block_sum(int64_t v, int64_t* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int o = SCAN_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  return sh[0];
}
__device__ __forceinline__ int64_t block_min(int64_t v, int64_t* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int o = SCAN_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] = sh[t + o] < sh[t] ? sh[t + o] : sh[t];
    __syncthreads();
  }
  return sh[0];
}

// pass 1: rows[i] and the workgroup's sums
__global__ __launch_bounds__(SCAN_THREADS) void collate_count_kernel(const int64_t* __restrict__ ids, int64_t n_ids, const int64_t* __restrict__ id2row,
                                                                     int64_t n_table, const int64_t* __restrict__ atom_ptr,
                                                                     const int64_t* __restrict__ edge_ptr, int64_t n_mols, int64_t* __restrict__ rows,
                                                                     ScanPartial* __restrict__ partial) {
  __shared__ int64_t sh[SCAN_THREADS];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * SCAN_CHUNK;
  int64_t atoms = 0, edges = 0, bad = 0, first_bad = INT64_MAX;
#pragma unroll
  for (int k = 0; k < SCAN_PER_THREAD; ++k) {
    const int64_t i = base + k * SCAN_THREADS + threadIdx.x;
    if (i >= n_ids) continue;
    const int64_t r = collate_row_of(ids, i, id2row, n_table, n_mols);
    rows[i] = r;
    if (r < 0) {
      ++bad;
      if (i < first_bad) first_bad = i;
    } else {
      atoms += atom_ptr[r + 1] - atom_ptr[r];
      edges += edge_ptr[r + 1] - edge_ptr[r];
    }
  }
  atoms = block_sum(atoms, sh);
  edges = block_sum(edges, sh);
  bad = block_sum(bad, sh);
  first_bad = block_min(first_bad, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = ScanPartial{atoms, edges, bad, first_bad};
}

// pass 2: workgroup g adds the sums of the workgroups before it to the exclusive scan of its own ids; the last one writes the totals
__global__ __launch_bounds__(SCAN_THREADS) void collate_scan_kernel(const int64_t* __restrict__ rows, int64_t n_ids, const int64_t* __restrict__ atom_ptr,
                                                                    const int64_t* __restrict__ edge_ptr, const ScanPartial* __restrict__ partial,
                                                                    int64_t* __restrict__ out_atom_ptr, int64_t* __restrict__ out_edge_ptr,
                                                                    int64_t* __restrict__ totals) {
  __shared__ int64_t sh[SCAN_THREADS];
  __shared__ int64_t sh_a[SCAN_THREADS], sh_e[SCAN_THREADS];
  const int t = threadIdx.x;
  const int64_t g = blockIdx.x, n_groups = gridDim.x;
  const bool last = g == n_groups - 1;
  int64_t pa = 0, pe = 0, bad = 0, first_bad = INT64_MAX;
  for (int64_t j = t; j < n_groups; j += SCAN_THREADS) {
    const ScanPartial p = partial[j];
    if (j < g) {
      pa += p.atoms;
      pe += p.edges;
    }
    bad += p.bad;
    if (p.first_bad < first_bad) first_bad = p.first_bad;
  }
  pa = block_sum(pa, sh);
  pe = block_sum(pe, sh);
  if (last) {
    bad = block_sum(bad, sh);
    first_bad = block_min(first_bad, sh);
  }
  // thread t owns ids [base + 4 t, base + 4 t + 4)
  const int64_t base = g * SCAN_CHUNK + static_cast<int64_t>(t) * SCAN_PER_THREAD;
  int64_t ca[SCAN_PER_THREAD], ce[SCAN_PER_THREAD], ta = 0, te = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PER_THREAD; ++k) {
    ca[k] = ce[k] = 0;
    const int64_t i = base + k;
    if (i < n_ids) {
      const int64_t r = rows[i];
      if (r >= 0) {
        ca[k] = atom_ptr[r + 1] - atom_ptr[r];
        ce[k] = edge_ptr[r + 1] - edge_ptr[r];
      }
    }
    ta += ca[k];
    te += ce[k];
  }
  // inclusive scan of the threads' sums (Hillis-Steele; a read phase and a write phase per step)
  sh_a[t] = ta;
  sh_e[t] = te;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {
    const int64_t va = t >= o ? sh_a[t - o] : 0, ve = t >= o ? sh_e[t - o] : 0;
    __syncthreads();
    sh_a[t] += va;
    sh_e[t] += ve;
    __syncthreads();
  }
  int64_t xa = pa + sh_a[t] - ta, xe = pe + sh_e[t] - te;      // exclusive prefix of this thread's first id
#pragma unroll
  for (int k = 0; k < SCAN_PER_THREAD; ++k) {
    const int64_t i = base + k;
    if (i < n_ids) {
      out_atom_ptr[i] = xa;
      out_edge_ptr[i] = xe;
    }
    xa += ca[k];
    xe += ce[k];
  }
  if (last && t == SCAN_THREADS - 1) {          // xa / xe of the last thread of the last workgroup: the totals
    out_atom_ptr[n_ids] = xa;
    out_edge_ptr[n_ids] = xe;
    totals[0] = xa;
    totals[1] = xe;
    totals[2] = bad;
    totals[3] = bad ? first_bad : -1;
  }
}

// ------------------------------------------------------------------------------------------------------------------ molecules
struct MolArgs {
  const int64_t *rows, *out_atom_ptr, *out_edge_ptr;
  int64_t n_ids, A, E, atom_tiles;
  const int64_t *atom_ptr, *edge_ptr;
  const float* s_nf;
  const int64_t* s_el;
  const float *s_ef, *s_ew, *s_aug;
  const int64_t* s_rowptr;
  float* nf;
  int64_t *n2g, *el;
  float *ef, *ew;
  int64_t *rowptr, *col;
  float *aug, *w;
};

constexpr int MOL_THREADS = 256;
constexpr int ATOM_TILE = 32;       // atom rows per workgroup: 32 x 67 floats
constexpr int EDGE_TILE = 64;       // edge rows per workgroup

// the drug b of output position x: ptr[b] <= x < ptr[b + 1] (drugs without atoms / edges own no position); ptr has n + 1 entries
__device__ __forceinline__ int64_t collate_owner(const int64_t* __restrict__ ptr, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;             // invariant: ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MOL_THREADS) void collate_molecules_kernel(const MolArgs a) {
  __shared__ int64_t sh_src[EDGE_TILE];        // store row (atom / edge) of each output row of the tile
  __shared__ int64_t sh_delta[EDGE_TILE];      // edge tiles: out_atom_ptr[b] - atom_ptr[row], what rebases an atom index
  const int t = threadIdx.x;
  const int64_t blk = blockIdx.x;
  if (blk == 0 && t == 0) a.rowptr[a.A] = a.E;
  if (blk < a.atom_tiles) {
    const int64_t a0 = blk * ATOM_TILE;
    const int n = static_cast<int>(a.A - a0 < ATOM_TILE ? a.A - a0 : ATOM_TILE);
    if (t < n) {
      const int64_t ao = a0 + t;
      const int64_t b = collate_owner(a.out_atom_ptr, a.n_ids, ao);
      const int64_t row = a.rows[b];
      const int64_t as = ao - a.out_atom_ptr[b] + a.atom_ptr[row];
      sh_src[t] = as;
      a.n2g[ao] = b;
      a.rowptr[ao] = a.s_rowptr[as] - a.edge_ptr[row] + a.out_edge_ptr[b];
    }
    __syncthreads();
    // 268-byte rows: consecutive rows share no alignment above 4 bytes, so one float per lane; the tile's output is contiguous
    float* out = a.nf + a0 * NODE_W;
    for (int j = t; j < n * NODE_W; j += MOL_THREADS) {
      const int r = j / NODE_W, c = j - r * NODE_W;
      out[j] = a.s_nf[sh_src[r] * NODE_W + c];
    }
    return;
  }
  const int64_t e0 = (blk - a.atom_tiles) * EDGE_TILE;
  if (e0 >= a.E) return;
  const int n = static_cast<int>(a.E - e0 < EDGE_TILE ? a.E - e0 : EDGE_TILE);
  if (t < n) {
    const int64_t eo = e0 + t;
    const int64_t b = collate_owner(a.out_edge_ptr, a.n_ids, eo);
    const int64_t row = a.rows[b];
    const int64_t es = eo - a.out_edge_ptr[b] + a.edge_ptr[row];
    const int64_t delta = a.out_atom_ptr[b] - a.atom_ptr[row];
    sh_src[t] = es;
    sh_delta[t] = delta;
    const float wv = a.s_ew[es];
    a.ew[eo] = wv;
    if (a.w) a.w[eo] = wv;
    a.col[eo] = a.s_el[es * 3] + delta;
  }
  __syncthreads();
  // edge_list rows: 3 x int64 (24 B), one 8-byte element per lane
  for (int j = t; j < n * 3; j += MOL_THREADS) {
    const int r = j / 3, c = j - r * 3;
    int64_t v = a.s_el[sh_src[r] * 3 + c];
    if (c < 2) v += sh_delta[r];
    a.el[e0 * 3 + j] = v;
  }
  // bond rows: 72 B = 9 x 8 B (rows are 8-byte aligned, not 16)
  {
    const f32x2* src = reinterpret_cast<const f32x2*>(a.s_ef);
    f32x2* dst = reinterpret_cast<f32x2*>(a.ef) + e0 * (BOND_W / 2);
    for (int j = t; j < n * (BOND_W / 2); j += MOL_THREADS) {
      const int r = j / (BOND_W / 2), c = j - r * (BOND_W / 2);
      dst[j] = src[sh_src[r] * (BOND_W / 2) + c];
    }
  }
  // augmented rows: 80 B = 5 x 16 B
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.s_aug);
    f32x4* dst = reinterpret_cast<f32x4*>(a.aug) + e0 * (AUG_W / 4);
    for (int j = t; j < n * (AUG_W / 4); j += MOL_THREADS) {
      const int r = j / (AUG_W / 4), c = j - r * (AUG_W / 4);
      dst[j] = src[sh_src[r] * (AUG_W / 4) + c];
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- tabular rows
constexpr int MAX_SEG = MDG_COLLATE_MAX_SEGMENTS;
constexpr int ROW_THREADS = 256;

struct RowsArgs {
  const float* src[MAX_SEG];
  float* out[MAX_SEG];
  int64_t n_src[MAX_SEG];
  int width[MAX_SEG];
  int vec[MAX_SEG];           // floats per load: 4, 2 or 1
  int tpr[MAX_SEG];           // threads per row: a power of two <= 256
  const int64_t* rows;
  int64_t n_ids, n_store_rows;
};

template <typename V>
__device__ __forceinline__ void copy_row(const float* __restrict__ s, float* __restrict__ d, int groups, int g0, int step) {
  const V* sv = reinterpret_cast<const V*>(s);
  V* dv = reinterpret_cast<V*>(d);
  for (int g = g0; g < groups; g += step) dv[g] = sv[g];
}

// blockIdx.y = segment; a workgroup owns 256 / tpr consecutive output rows (s, b) of its segment
__global__ __launch_bounds__(ROW_THREADS) void collate_rows_kernel(const RowsArgs a) {
  const int seg = blockIdx.y;
  const int tpr = a.tpr[seg], W = a.width[seg], vec = a.vec[seg];
  const int t = threadIdx.x;
  const int64_t q = static_cast<int64_t>(blockIdx.x) * (ROW_THREADS / tpr) + t / tpr;       // output row: source s, batch position b
  if (q >= a.n_src[seg] * a.n_ids) return;
  const int64_t s = q / a.n_ids, b = q - s * a.n_ids;
  const int64_t r = a.rows[b];
  if (r < 0 || r >= a.n_store_rows) return;
  const float* src = a.src[seg] + (s * a.n_store_rows + r) * W;
  float* dst = a.out[seg] + q * W;
  const int g0 = t & (tpr - 1);
  if (vec == 4) copy_row<f32x4>(src, dst, W / 4, g0, tpr);
  else if (vec == 2) copy_row<f32x2>(src, dst, W / 2, g0, tpr);
  else copy_row<float>(src, dst, W, g0, tpr);
}

}  // namespace

extern "C" size_t mdg_collate_offsets_workspace_bytes(int64_t n_ids) {
  if (n_ids <= 0) return 0;
  return static_cast<size_t>(mdg_cdiv(n_ids, SCAN_CHUNK)) * sizeof(ScanPartial);
}

extern "C" int mdg_collate_offsets(const int64_t* ids, int64_t n_ids, const int64_t* id2row, int64_t n_table, const int64_t* atom_ptr,
                                   const int64_t* edge_ptr, int64_t n_mols, int64_t* rows, int64_t* out_atom_ptr, int64_t* out_edge_ptr,
                                   int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  MDG_CHECK_ARG(n_ids >= 1, "mdg_collate_offsets: no ids");
  MDG_CHECK_ARG(n_table >= 0 && n_mols >= 0, "mdg_collate_offsets: bad store size");
  MDG_CHECK_ARG(ids && (id2row || n_table == 0) && atom_ptr && edge_ptr && rows && out_atom_ptr && out_edge_ptr && totals,
                "mdg_collate_offsets: null pointer");
  const int64_t groups = mdg_cdiv(n_ids, SCAN_CHUNK);
  MDG_CHECK_ARG(groups < (1ll << 31), "mdg_collate_offsets: too many ids for one launch");
  const size_t need = mdg_collate_offsets_workspace_bytes(n_ids);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) {
    mdg_set_error("mdg_collate_offsets: workspace of %zu bytes (8-byte aligned) required, got %zu", need, workspace_bytes);
    return MDG_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  ScanPartial* partial = static_cast<ScanPartial*>(workspace);
  const dim3 grid(static_cast<unsigned>(groups));
  hipLaunchKernelGGL(collate_count_kernel, grid, dim3(SCAN_THREADS), 0, st, ids, n_ids, id2row, n_table, atom_ptr, edge_ptr, n_mols, rows, partial);
  MDG_CHECK_LAUNCH("mdg_collate_offsets (counts)");
  hipLaunchKernelGGL(collate_scan_kernel, grid, dim3(SCAN_THREADS), 0, st, rows, n_ids, atom_ptr, edge_ptr, partial, out_atom_ptr, out_edge_ptr, totals);
  MDG_CHECK_LAUNCH("mdg_collate_offsets (scan)");
  return MDG_OK;
}

extern "C" int mdg_collate_molecules(const int64_t* rows, const int64_t* out_atom_ptr, const int64_t* out_edge_ptr, int64_t n_ids,
                                     int64_t n_atoms, int64_t n_edges, const int64_t* atom_ptr, const int64_t* edge_ptr,
                                     const float* store_node_feature, const int64_t* store_edge_list, const float* store_edge_feature,
                                     const float* store_edge_weight, const float* store_edge_feat_aug, const int64_t* store_rowptr,
                                     float* node_feature, int64_t* node2graph, int64_t* edge_list, float* edge_feature, float* edge_weight,
                                     int64_t* rowptr, int64_t* col, float* edge_feat_aug, float* w, void* stream) {
  MDG_CHECK_ARG(n_ids >= 1 && n_atoms >= 0 && n_edges >= 0, "mdg_collate_molecules: bad size");
  MDG_CHECK_ARG(rows && out_atom_ptr && out_edge_ptr && atom_ptr && edge_ptr && rowptr, "mdg_collate_molecules: null pointer");
  MDG_CHECK_ARG(n_atoms == 0 || (store_node_feature && store_rowptr && node_feature && node2graph), "mdg_collate_molecules: null atom array");
  MDG_CHECK_ARG(n_edges == 0 || (store_edge_list && store_edge_feature && store_edge_weight && store_edge_feat_aug && edge_list &&
                                 edge_feature && edge_weight && col && edge_feat_aug),
                "mdg_collate_molecules: null edge array");
  MDG_CHECK_ARG(n_edges == 0 || n_atoms > 0, "mdg_collate_molecules: edges without atoms");
  MDG_CHECK_ARG(n_edges == 0 || ((reinterpret_cast<uintptr_t>(store_edge_feature) & 7u) == 0 && (reinterpret_cast<uintptr_t>(edge_feature) & 7u) == 0),
                "mdg_collate_molecules: edge_feature arrays must be 8-byte aligned");
  MDG_CHECK_ARG(n_edges == 0 || (mdg_aligned16(store_edge_feat_aug) && mdg_aligned16(edge_feat_aug)),
                "mdg_collate_molecules: edge_feat_aug arrays must be 16-byte aligned");
  MolArgs a{};
  a.rows = rows; a.out_atom_ptr = out_atom_ptr; a.out_edge_ptr = out_edge_ptr;
  a.n_ids = n_ids; a.A = n_atoms; a.E = n_edges; a.atom_tiles = mdg_cdiv(n_atoms, ATOM_TILE);
  a.atom_ptr = atom_ptr; a.edge_ptr = edge_ptr;
  a.s_nf = store_node_feature; a.s_el = store_edge_list; a.s_ef = store_edge_feature; a.s_ew = store_edge_weight;
  a.s_aug = store_edge_feat_aug; a.s_rowptr = store_rowptr;
  a.nf = node_feature; a.n2g = node2graph; a.el = edge_list; a.ef = edge_feature; a.ew = edge_weight;
  a.rowptr = rowptr; a.col = col; a.aug = edge_feat_aug; a.w = w;
  const int64_t blocks = a.atom_tiles + mdg_cdiv(n_edges, EDGE_TILE);
  MDG_CHECK_ARG(blocks < (1ll << 31), "mdg_collate_molecules: too many rows for one launch");
  const dim3 grid(static_cast<unsigned>(blocks > 0 ? blocks : 1));          // an empty batch still writes rowptr[0] = 0
  hipLaunchKernelGGL(collate_molecules_kernel, grid, dim3(MOL_THREADS), 0, static_cast<hipStream_t>(stream), a);
  MDG_CHECK_LAUNCH("mdg_collate_molecules");
  return MDG_OK;
}

extern "C" int mdg_collate_rows(const float* const* src_host, float* const* out_host, const int64_t* n_sources_host,
                                const int64_t* width_host, int n_segments, int64_t n_store_rows, const int64_t* rows, int64_t n_ids,
                                void* stream) {
  MDG_CHECK_ARG(n_segments >= 1 && n_segments <= MAX_SEG, "mdg_collate_rows: 1 to %d segments (got %d)", MAX_SEG, n_segments);
  MDG_CHECK_ARG(src_host && out_host && n_sources_host && width_host, "mdg_collate_rows: null segment table");
  MDG_CHECK_ARG(n_ids >= 1 && n_store_rows >= 1 && rows, "mdg_collate_rows: bad size or null rows");
  RowsArgs a{};
  int64_t blocks = 1;
  for (int g = 0; g < n_segments; ++g) {
    const int64_t S = n_sources_host[g], W = width_host[g];
    MDG_CHECK_ARG(S >= 1 && W >= 1 && W < (1 << 24), "mdg_collate_rows: segment %d has %lld sources of width %lld", g, (long long)S, (long long)W);
    MDG_CHECK_ARG(src_host[g] && out_host[g], "mdg_collate_rows: segment %d has a null pointer", g);
    const uintptr_t both = reinterpret_cast<uintptr_t>(src_host[g]) | reinterpret_cast<uintptr_t>(out_host[g]);
    MDG_CHECK_ARG((both & 3u) == 0, "mdg_collate_rows: segment %d is not 4-byte aligned", g);
    // widest access every row of both arrays is aligned for: rows start at multiples of W floats from the base
    int vec = 1;
    if (W % 4 == 0 && (both & 15u) == 0) vec = 4;
    else if (W % 2 == 0 && (both & 7u) == 0) vec = 2;
    const int64_t groups = W / vec;
    int tpr = 1;
    while (tpr < ROW_THREADS && tpr < groups) tpr *= 2;
    a.src[g] = src_host[g]; a.out[g] = out_host[g]; a.n_src[g] = S;
    a.width[g] = static_cast<int>(W); a.vec[g] = vec; a.tpr[g] = tpr;
    const int64_t need = mdg_cdiv(S * n_ids, ROW_THREADS / tpr);
    if (need > blocks) blocks = need;
  }
  MDG_CHECK_ARG(blocks < (1ll << 31), "mdg_collate_rows: too many rows for one launch");
  a.rows = rows; a.n_ids = n_ids; a.n_store_rows = n_store_rows;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(n_segments));
  hipLaunchKernelGGL(collate_rows_kernel, grid, dim3(ROW_THREADS), 0, static_cast<hipStream_t>(stream), a);
  MDG_CHECK_LAUNCH("mdg_collate_rows");
  return MDG_OK;
}
