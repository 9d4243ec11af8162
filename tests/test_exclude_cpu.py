"""CPU checks of the known-pair exclusion masks of the in-sweep screening products: the C ABI (version 16) declares and exports
the mask builder and the three *_masked entry points, ops.pair_mask_dense inverts the documented layout, and the merge step of
pipeline.top_pairs with a masking ``rescore`` equals brute force over dense scores whose excluded pairs sit at -inf."""
import numpy as np
import pytest
import torch

from test_topk_cpu import PAIR_CASES, _row_lists, brute_force_pairs, pair_case

NEG = float("-inf")
NEW_SYMBOLS = ("mdg_pair_mask_ld", "mdg_pair_mask_plane_words", "mdg_pair_mask_set", "mdg_bilinear_topk_masked",
               "mdg_bilinear_select_count_masked", "mdg_bilinear_select_fill_masked")


def numpy_pack(excl: np.ndarray) -> np.ndarray:
    """The documented layout, written out element by element: bool [P, n_head, n_tail] -> uint32 [P, ceil(n_head/32), ld], ld =
    n_tail rounded up to 64; word [p][i >> 5][j] holds the bit of row i, column j at position i & 31."""
    P, nh, nt = excl.shape
    ld = (nt + 63) // 64 * 64
    out = np.zeros((P, (nh + 31) // 32, ld), dtype=np.uint32)
    p, i, j = np.nonzero(excl)
    np.bitwise_or.at(out, (p, i >> 5, j), np.uint32(1) << (i & 31).astype(np.uint32))
    return out


def as_mask(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(words.view(np.int32).copy())


def test_abi_version_and_the_new_symbols():
    from madrigal_amd import _lib
    L = _lib.lib()
    assert L.mdg_abi_version() >= 16
    syms = _lib.declared_symbols()
    protos = _lib.declared_prototypes()
    for s in NEW_SYMBOLS:
        assert s in syms and s in protos and hasattr(L, s), s
    # a masked entry point takes its twin's arguments plus (mask, plane_stride)
    for twin in ("mdg_bilinear_topk", "mdg_bilinear_select_count", "mdg_bilinear_select_fill"):
        assert len(protos[twin + "_masked"][1]) == len(protos[twin][1]) + 2
        assert protos[twin + "_masked"][1][:-2] == protos[twin][1]


def test_the_layout_arithmetic_lives_in_the_library():
    from madrigal_amd._lib import lib
    L = lib()
    for nh, nt in ((1, 1), (33, 4), (300, 333), (2049, 2049), (100352, 100352), (64, 64), (32, 128)):
        ld = L.mdg_pair_mask_ld(nt)
        assert ld == (nt + 63) // 64 * 64 and ld % 64 == 0 and ld >= nt
        assert L.mdg_pair_mask_plane_words(nh, nt) == (nh + 31) // 32 * ld
    assert L.mdg_pair_mask_ld(0) == 0 and L.mdg_pair_mask_plane_words(0, 5) == 0
    # argument checks run before anything touches a device
    rc = L.mdg_pair_mask_set(None, 1, 4, 5, None, None, None, 3, 1, None)
    assert rc == -1 and b"symmetric" in L.mdg_last_error()


@pytest.mark.parametrize("nh,nt", [(1, 1), (33, 4), (300, 333)])
@pytest.mark.parametrize("P", [1, 3])
def test_pair_mask_dense_inverts_the_numpy_packing(nh, nt, P):
    from madrigal_amd import ops
    rng = np.random.default_rng(nh * 1000 + nt + P)
    excl = rng.random((P, nh, nt)) < 0.4
    excl[:, nh - 1, nt - 1] = True                  # the last row (bit (nh - 1) & 31 of the last row block) and column
    excl[:, 0, 0] = True
    words = numpy_pack(excl)
    assert words.shape == (P, (nh + 31) // 32, (nt + 63) // 64 * 64)
    mask = as_mask(words)
    dense = ops.pair_mask_dense(mask, nh, nt)
    assert dense.dtype == torch.bool and dense.shape == (P, nh, nt)
    assert np.array_equal(dense.numpy(), excl)
    rows = torch.tensor(sorted({0, nh - 1, nh // 2, min(31, nh - 1), min(32, nh - 1)}))
    for p in range(P):
        assert torch.equal(ops.pair_mask_rows(mask, p, rows, nt), dense[p, rows])
    # bits in the pad columns and pad rows are not pairs
    padded = words.copy()
    padded[:, :, nt:] = 0xFFFFFFFF
    if nh % 32:
        padded[:, -1, :] |= np.uint32((0xFFFFFFFF << (nh % 32)) & 0xFFFFFFFF)
    assert np.array_equal(ops.pair_mask_dense(as_mask(padded), nh, nt).numpy(), excl)
    for bad in (mask.long(), mask[:, :, :-1], mask[0]):
        with pytest.raises(ValueError):
            ops.pair_mask_dense(bad, nh, nt)


def _known_network(N, hubs, seed):
    """A symmetric bool [N, N] of "known" pairs: 30 % random, plus -- with ``hubs`` -- every other partner of the two hub drugs
    of pair_case: their rows stay open (they still own most of the best pairs) and half of what is re-scored has to be masked."""
    g = torch.Generator().manual_seed(seed)
    known = torch.rand((N, N), generator=g) < 0.3
    if hubs:
        known[N - 1, ::2] = True
        known[N // 2, 1::2] = True
    known = known | known.T
    known.fill_diagonal_(False)
    return known


@pytest.mark.parametrize("N,K,k_row,hubs", PAIR_CASES)
def test_merge_with_a_masking_rescore_equals_brute_force(N, K, k_row, hubs):
    """What top_pairs(exclude=...) does after the sweep, on the CPU: row lists of the scores with the known pairs at -inf, a
    ``rescore`` that masks the re-scored dense rows with ops.pair_mask_rows of the PACKED mask, merge_row_candidates unchanged."""
    from madrigal_amd import ops
    from madrigal_amd.pipeline import merge_row_candidates
    from oracle import madrigal_oracle as O
    z, w = pair_case(N, hubs)
    S = O.bilinear_scores(z, z, w)
    known = _known_network(N, hubs, seed=N + K)
    mask = as_mask(numpy_pack(known[None].numpy()))
    assert torch.equal(ops.pair_mask_dense(mask, N, N)[0], known)
    S_ex = S.masked_fill(known[None], NEG)
    vals, idx = _row_lists(S_ex, k_row)

    def rescore(l, rows):
        return S[l, rows].masked_fill(ops.pair_mask_rows(mask, 0, rows, N), NEG)

    info = {}
    v, h, t = merge_row_candidates(vals, idx, K, rescore, info)
    bv, bh, bt = brute_force_pairs(S_ex, K)
    gone = bv == NEG                                        # brute force lists excluded pairs at the end: they are padding
    bh, bt = bh.masked_fill(gone, -1), bt.masked_fill(gone, -1)
    assert torch.equal(h, bh) and torch.equal(t, bt) and torch.equal(v, bv)
    assert not bool(known[h.clamp(min=0), t.clamp(min=0)][h >= 0].any())
    if hubs:
        assert min(info["open_rows"]) >= 1, info            # the masked re-score is really exercised
