"""CPU checks of the per-pair outcome profile: mdg_bilinear_profile is declared, typed and exported and refuses bad shapes before it
touches a device, ops.profile_merge of any split of the outcomes equals the unsplit profile, and the dense reference of the GPU
tests agrees with a plain loop in the kernel's order."""
import ctypes
import itertools

import pytest
import torch

from profile_ref import dense_profile, loop_profile, same

NEW = ("mdg_bilinear_profile_workspace_bytes", "mdg_bilinear_profile")
INF = float("inf")


def test_profile_symbols_are_declared_typed_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    protos = _lib.declared_prototypes()
    L = _lib.lib()
    for s in NEW:
        assert s in syms and s in protos and hasattr(L, s), s
    P, I, I64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert protos["mdg_bilinear_profile_workspace_bytes"] == (Z, [I64, I64, I64, I64, I])
    assert protos["mdg_bilinear_profile"] == (I, [P, P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I, I, P, Z, P])
    assert L.mdg_bilinear_profile_workspace_bytes(4096, 4096, 896, 128, 0) == 0
    for nh, nt, nl in ((4096, 4096, 896), (100352, 100352, 64), (7, 333, 3)):
        for prec in (0, 1, 2, 3):                      # the operand images, as for the other sweeps
            assert L.mdg_bilinear_profile_workspace_bytes(nh, nt, nl, 128, prec) == L.mdg_bilinear_select_workspace_bytes(nh, nt, nl, 128, prec)
    header = open(_lib.HEADER).read()
    assert "the reference has no function of this kind; it reads such summaries off its stored score tensor" in " ".join(header.split())


def test_c_entry_refuses_bad_shapes_before_it_touches_a_device():
    from madrigal_amd._lib import lib
    L = lib()
    f = L.mdg_bilinear_profile
    for n_head, n_tail, n_labels, D, ldo, eligible, what in ((4, 4, 1, 128, 4, 7, b"unknown eligible"), (4, 5, 1, 128, 5, 2, b"one drug set"),
                                                             (4, 5, 1, 128, 5, 1, b"one drug set"), (4, 4, 1, 64, 4, 0, b"D must be"),
                                                             (4, 4, 65536, 128, 4, 0, b"n_labels"), (4, 4, 1, 128, 3, 0, b"ldo"),
                                                             (4, 4, 1, 128, 4, 0, b"null output")):
        rc = f(None, None, None, None, None, None, None, None, ldo, n_head, n_tail, n_labels, D, 0, eligible, None, 0, None)
        assert rc == -1 and b"mdg_bilinear_profile" in L.mdg_last_error() and what in L.mdg_last_error(), (what, L.mdg_last_error())
    assert f(None, None, None, None, None, None, None, None, 0, 0, 0, 1, 128, 0, 0, None, 0, None) == 0          # no row: nothing to do


def test_wrapper_validation_without_a_gpu():
    from madrigal_amd import ops
    z, z2, w = torch.zeros(6, 128), torch.zeros(4, 128), torch.zeros(2, 128, 128)
    thr = torch.zeros(2)
    f = ops.bilinear_profile
    with pytest.raises(ValueError, match="NaN"):
        f(z, z, w, torch.tensor([0.0, float("nan")]))
    with pytest.raises(ValueError, match="one cut per outcome"):
        f(z, z, w, torch.zeros(3))
    with pytest.raises(ValueError, match="one drug set"):
        f(z, z2, w, thr, eligible="not_self")
    with pytest.raises(ValueError, match="unknown eligible"):
        f(z, z, w, thr, eligible="upper")
    with pytest.raises(ValueError, match="scale"):
        f(z, z, w, thr, scale=torch.ones(3))
    with pytest.raises(ValueError, match="GPU"):                      # a well-formed call on CPU tensors: no CPU fallback
        f(z, z, w, thr, scale=torch.ones(2))


def _tensor(seed=0):
    """L = 5, 7 x 6: outcome 2 is a copy of outcome 0 (exact ties across outcomes when their cuts and scales agree), one NaN score."""
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn((5, 7, 6), generator=g)
    dense[2] = dense[0]
    dense[1, 3, 2] = float("nan")
    return dense


CUTS = {
    "plain": [0.1, -0.3, 0.1, 0.5, -1.0],
    "left_dead": [INF, INF, 0.1, 0.5, -1.0],          # chunks whose every u is -inf
    "right_dead": [0.1, -0.3, INF, INF, INF],
    "all_dead": [INF] * 5,
    "all_in": [-INF] * 5,
    "mixed": [-INF, 0.0, INF, 0.2, -INF],
}


@pytest.mark.parametrize("eligible", ["all", "lower"])
@pytest.mark.parametrize("name", sorted(CUTS))
def test_profile_merge_of_any_split_equals_the_unsplit_profile(name, eligible):
    from madrigal_amd.ops import profile_merge
    dense = _tensor()
    if eligible == "lower":
        dense = dense[:, :6]
    thr = torch.tensor(CUTS[name])
    for scale in (None, torch.tensor([2.0, 0.5, 2.0, 1.0, 3.0])):            # scale[2] == scale[0]: the tie survives
        whole = dense_profile(dense, thr, scale, eligible)
        if name == "plain":
            assert not bool((whole[1] == 2).any()) and bool((whole[1] == 0).any())          # the tied pair of outcomes resolves to the lower
        for n_cuts in (1, 2):
            for cuts in itertools.combinations(range(1, 5), n_cuts):         # every split into two or three chunks; (1,), (2,) part 0 from 2
                edges = (0,) + cuts + (5,)
                acc = None
                for a, b in zip(edges[:-1], edges[1:]):
                    part = dense_profile(dense[a:b], thr[a:b], None if scale is None else scale[a:b], eligible)
                    before = [t.clone() for t in part]
                    acc = part if acc is None else profile_merge(acc, part, a)
                    assert all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)
                               for x, y in zip(part, before))                 # the arguments are left alone
                assert same(acc, whole), (name, eligible, cuts)
    if name == "all_dead":
        assert bool((whole[1] == -1).all()) and bool((whole[0] == 0).all()) and bool(torch.isinf(whole[2]).all())


def test_profile_merge_out_of_order_keeps_the_lower_global_outcome():
    """Chunks merged in the other order (b's outcomes BELOW a's): equal margins still keep the lower global index."""
    from madrigal_amd.ops import profile_merge
    dense = _tensor()
    thr = torch.tensor(CUTS["plain"])
    whole = dense_profile(dense, thr, None, "all")
    hi = dense_profile(dense[2:], thr[2:], None, "all")
    hi = (hi[0], torch.where(hi[1] >= 0, hi[1] + 2, hi[1]), hi[2])            # already global
    lo = dense_profile(dense[:2], thr[:2], None, "all")
    assert same(profile_merge(hi, lo, 0), whole)


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
def test_reference_agrees_with_a_plain_loop(eligible):
    g = torch.Generator().manual_seed(5)
    nh, nt = (7, 6) if eligible == "all" else (7, 7)
    dense = torch.randn((3, nh, nt), generator=g)
    dense[2] = dense[0]
    dense[1, 2, 1] = float("nan")
    for thr in ([0.0, 0.2, 0.0], [-INF, INF, -INF], [INF, INF, INF], [float(dense[0, 4, 1]), 0.0, float(dense[0, 4, 1])]):
        thr = torch.tensor(thr)
        for scale in (None, torch.tensor([1.5, 0.25, 1.5])):
            ref = dense_profile(dense, thr, scale, eligible)
            assert same(ref, loop_profile(dense, thr, scale, eligible)), (eligible, thr.tolist())
            assert ref[0].dtype == torch.int32 and ref[1].dtype == torch.int32 and ref[2].dtype == torch.float32
    assert same(dense_profile(dense[:0], torch.zeros(0), None, eligible), loop_profile(dense[:0], torch.zeros(0), None, eligible))
