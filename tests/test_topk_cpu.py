"""CPU checks of the top-k screening product: the C ABI of mdg_bilinear_topk is declared and exported, and the
merge-and-certify step of pipeline.top_pairs equals brute force over the oracle's scores."""
import ctypes

import numpy as np
import pytest
import torch

NEG = float("-inf")


def test_topk_symbols_are_declared_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    L = _lib.lib()
    for s in ("mdg_bilinear_topk", "mdg_bilinear_topk_workspace_bytes", "mdg_bilinear_topk_max_k"):
        assert s in syms and hasattr(L, s), s
    assert L.mdg_bilinear_topk_max_k() >= 32
    assert L.mdg_abi_version() >= 10


def test_topk_workspace_query_needs_no_gpu():
    from madrigal_amd import _lib
    L = _lib.lib()
    c = ctypes.c_int64
    assert L.mdg_bilinear_topk_workspace_bytes(c(4096), c(4096), c(896), c(128), 0, 16) == 0
    b3 = L.mdg_bilinear_topk_workspace_bytes(c(4096), c(4096), c(896), c(128), 1, 16)
    b1 = L.mdg_bilinear_topk_workspace_bytes(c(4096), c(4096), c(896), c(128), 3, 16)
    assert b3 == 2 * b1 and b1 >= 4096 * 128 * 2 + 896 * 128 * 128 * 2
    # the operand images are those of the dense head
    assert b3 == L.mdg_bilinear_allpairs_workspace_bytes(c(4096), c(4096), c(896), c(128), 1)


def test_topk_refuses_cpu_tensors_and_bad_arguments_without_a_gpu():
    from madrigal_amd import ops
    z = torch.zeros(4, 128)
    w = torch.zeros(1, 128, 128)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_topk(z, z, w, 2)
    assert ops.bilinear_topk_max_k() >= 32
    # the C entry point validates before it touches the device
    from madrigal_amd._lib import lib
    c = ctypes.c_int64
    rc = lib().mdg_bilinear_topk(None, None, None, None, None, c(4), c(4), c(1), c(128), 0, 0, 0, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"k must be" in lib().mdg_last_error()
    rc = lib().mdg_bilinear_topk(None, None, None, None, None, c(4), c(5), c(1), c(128), 0, 2, 2, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"one drug set" in lib().mdg_last_error()


def _row_lists(S, k_row):
    """What the kernel hands over in lower-triangle mode, from dense scores S [L,N,N]: per row its k_row best j < i by
    (score descending, j ascending), padded with -inf / -1."""
    L, N, _ = S.shape
    d = S.clone()
    i = torch.arange(N)[:, None]
    j = torch.arange(N)[None, :]
    d[:, j >= i] = NEG
    sv, si = torch.sort(d, dim=2, descending=True, stable=True)
    sv, si = sv[..., :k_row], si[..., :k_row]
    if sv.shape[2] < k_row:
        pad = k_row - sv.shape[2]
        sv = torch.cat([sv, sv.new_full((L, N, pad), NEG)], 2)
        si = torch.cat([si, si.new_full((L, N, pad), -1)], 2)
    return sv.contiguous(), torch.where(sv == NEG, torch.full_like(si, -1), si).to(torch.int32).contiguous()


def brute_force_pairs(S, K):
    """The K best of the strict lower triangle of S [L,N,N]: stable descending sort in row-major order."""
    L, N, _ = S.shape
    ii, jj = torch.tril_indices(N, N, -1)
    flat = S[:, ii, jj]
    sv, so = torch.sort(flat, dim=1, descending=True, stable=True)
    take = min(K, flat.shape[1])
    v = torch.full((L, K), NEG)
    h = torch.full((L, K), -1, dtype=torch.int64)
    t = torch.full((L, K), -1, dtype=torch.int64)
    v[:, :take], h[:, :take], t[:, :take] = sv[:, :take], ii[so[:, :take]], jj[so[:, :take]]
    return v, h, t


def pair_case(N, hubs, seed=0, L=2):
    """Embeddings and weights of one top_pairs case: rows 5 and 9 are copies of row 3 (exact ties); ``hubs``: two drugs whose
    embeddings are scaled up so that they own most of the top pairs."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((N, 128), generator=g)
    w = torch.randn((L, 128, 128), generator=g) / np.sqrt(128)
    z[5] = z[3]
    z[9] = z[3]
    if hubs:
        z[N - 1] *= 4
        z[N // 2] *= 3
    return z, w


PAIR_CASES = [(700, 200, 16, False), (700, 200, 16, True), (300, 1000, 8, False), (40, 2000, 16, False)]


@pytest.mark.parametrize("N,K,k_row,hubs", PAIR_CASES)
def test_merge_and_certify_equals_brute_force(N, K, k_row, hubs):
    from madrigal_amd.pipeline import merge_row_candidates
    from oracle import madrigal_oracle as O
    z, w = pair_case(N, hubs)
    S = O.bilinear_scores(z, z, w)
    vals, idx = _row_lists(S, k_row)
    info = {}
    v, h, t = merge_row_candidates(vals, idx, K, lambda l, rows: S[l, rows], info)
    bv, bh, bt = brute_force_pairs(S, K)
    assert torch.equal(h, bh) and torch.equal(t, bt) and torch.equal(v, bv)
    if hubs:
        assert min(info["open_rows"]) >= 1, info        # the refinement is really exercised
    assert max(info["open_rows"]) <= max(K // k_row, 1)
    if K > N * (N - 1) // 2:
        assert bool((v[:, N * (N - 1) // 2:] == NEG).all()) and bool((h[:, N * (N - 1) // 2:] == -1).all())


def test_no_row_is_open_when_the_lists_hold_K_entries():
    from madrigal_amd.pipeline import merge_row_candidates
    from oracle import madrigal_oracle as O
    z, w = pair_case(200, True)
    S = O.bilinear_scores(z, z, w)
    vals, idx = _row_lists(S, 16)

    def never(l, rows):
        raise AssertionError("k_row >= K: no row can be open")
    v, h, t = merge_row_candidates(vals, idx, 16, never)
    bv, bh, bt = brute_force_pairs(S, 16)
    assert torch.equal(h, bh) and torch.equal(t, bt) and torch.equal(v, bv)
