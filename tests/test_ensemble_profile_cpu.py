"""Per-pair outcome profiles over a checkpoint ensemble (mdg_bilinear_ensemble_profile, ops.bilinear_ensemble_profile,
pipeline.ensemble_outcome_profile / ensemble_most_flagged_pairs, most_flagged_pairs(exclude=)): what is decided without a GPU -- the C
ABI as the header declares it, the workspace query, the argument checks that return before any launch (null pointers throughout: a
launch would be an error of its own), the wrappers' ValueErrors, and the row-block walk the two most-flagged functions share, driven
by a pure-torch profile on the CPU against a brute-force sort."""
import ctypes

import pytest
import torch

from profile_ref import dense_profile

NEW = ("mdg_bilinear_ensemble_profile_tiles", "mdg_bilinear_ensemble_profile_workspace_bytes", "mdg_bilinear_ensemble_profile")
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16 = 0, 1, 2, 3
ALL, NOT_SELF, LOWER = 0, 1, 2
INF = float("inf")


def test_the_library_exports_the_symbols_with_the_header_prototypes():
    from madrigal_amd import _lib
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    for s in NEW:
        assert s in _lib.declared_symbols() and hasattr(L, s)
        assert (getattr(L, s).restype, list(getattr(L, s).argtypes)) == (protos[s][0], protos[s][1])
    I, I64, Z, P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
    assert protos[NEW[0]] == (I, [])
    assert protos[NEW[1]] == (Z, [I64, I64, I64, I64, I, I])
    assert protos[NEW[2]] == (I, [P, P, P, I, P, P, P, P, P, I64, I64, I64, I64, I64, I, I, P, Z, P])
    assert L.mdg_abi_version() >= 29
    assert 1 <= L.mdg_bilinear_ensemble_profile_tiles() <= 4


@pytest.mark.parametrize("sizes", [(4096, 4096, 896), (129, 1001, 2), (1, 1, 1), (5, 0, 3)])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_workspace_is_the_ensemble_sweeps(sizes, K):
    from madrigal_amd._lib import lib
    L = lib()
    nh, nt, nl = sizes
    assert L.mdg_bilinear_ensemble_profile_workspace_bytes(nh, nt, nl, 128, K, PREC_F32) == 0
    for prec in (PREC_F32, PREC_BF16X3):
        assert (L.mdg_bilinear_ensemble_profile_workspace_bytes(nh, nt, nl, 128, K, prec)
                == L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(nh, nt, nl, 128, K, prec))
    assert L.mdg_bilinear_ensemble_profile_workspace_bytes(nh, nt, nl, 128, 0, PREC_BF16X3) == 0


def _profile(n_models=2, prec=PREC_F32, eligible=ALL, nh=8, nt=8, nl=2, D=128, ldo=None):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_profile(None, None, None, n_models, None, None, None, None, None, nt if ldo is None else ldo, nh, nt, nl,
                                               D, prec, eligible, None, 0, None)


@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"prec": PREC_F16}, b"not offered"), ({"prec": 7}, b"precision"),
                                     ({"eligible": NOT_SELF, "nt": 9}, b"one drug set against itself"),
                                     ({"eligible": LOWER, "nt": 9}, b"one drug set against itself"), ({"eligible": 9}, b"eligible"),
                                     ({"D": 64}, b"D must be"), ({"nl": 65536}, b"n_labels"), ({"nh": -1}, b"negative"),
                                     ({"nt": (1 << 31) - 64}, b"int32 column indices"), ({"nh": 65535 * 128 + 1}, b"rows per call"),
                                     ({"ldo": 7}, b"ldo")])
def test_bad_arguments_are_refused_before_any_launch(kw, word):
    from madrigal_amd._lib import lib
    assert _profile(**kw) == -1
    msg = lib().mdg_last_error()
    assert b"mdg_bilinear_ensemble_profile" in msg and word in msg, msg


def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass():
    from madrigal_amd._lib import lib
    assert _profile() == -1 and b"mdg_bilinear_ensemble_profile: null output pointer" in lib().mdg_last_error()
    assert _profile(nl=0) == -1 and b"null output pointer" in lib().mdg_last_error()       # no outcome still writes the sentinels
    assert _profile(nh=0) == 0
    assert _profile(nt=0, nh=0) == 0


def test_null_model_pointers_and_the_workspace_are_checked_per_model():
    """Non-null host arrays whose entries are null; then (aligned, never dereferenced) made-up addresses with no workspace."""
    from madrigal_amd._lib import lib
    L = lib()
    some = ctypes.c_void_p(4096)

    def run(arrs, prec):
        return L.mdg_bilinear_ensemble_profile(arrs, arrs, arrs, 2, some, None, some, some, some, 8, 8, 8, 2, 128, prec, ALL, None, 0, None)

    assert run(None, PREC_F32) == -1 and b"null pointer" in L.mdg_last_error()
    assert run((ctypes.c_void_p * 2)(None, None), PREC_F32) == -1
    assert b"mdg_bilinear_ensemble_profile: null pointer for model 0" in L.mdg_last_error()
    assert run((ctypes.c_void_p * 2)(4096, 4100), PREC_F32) == -1 and b"16-byte aligned (model 1)" in L.mdg_last_error()
    assert run((ctypes.c_void_p * 2)(4096, 8192), PREC_BF16X3) == -2      # MDG_EWORKSPACE
    assert b"mdg_bilinear_ensemble_profile" in L.mdg_last_error() and b"workspace" in L.mdg_last_error()


def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


def test_ops_refuses_bad_calls_without_a_device():
    from madrigal_amd import ops
    f = ops.bilinear_ensemble_profile
    z, w = _inputs(2)
    thr = torch.full((3,), 0.5)
    with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
        f(z, z[:1], w, thr)
    with pytest.raises(ValueError, match="2 z_heads, 2 z_tails, 1 w_syms"):
        f(z, z, w[:1], thr)
    with pytest.raises(ValueError, match="1..8"):
        f([], [], [], thr)
    with pytest.raises(ValueError, match="1..8"):
        f((z * 5)[:9], (z * 5)[:9], (w * 5)[:9], thr)       # list repetition: nine models
    with pytest.raises(ValueError, match="precision"):
        f(z, z, w, thr, precision="bf16")
    with pytest.raises(ValueError, match="eligible"):
        f(z, z, w, thr, eligible="upper")
    with pytest.raises(ValueError, match="one cut per outcome"):
        f(z, z, w, torch.zeros(4))
    with pytest.raises(ValueError, match="NaN"):
        f(z, z, w, torch.tensor([0.5, float("nan"), 0.5]))
    with pytest.raises(ValueError, match="one drug set"):
        f(z, [t[:4] for t in z], w, thr, eligible="lower")
    with pytest.raises(ValueError, match="model 1 has"):
        f(z, z, [w[0], w[1][:2]], thr)
    with pytest.raises(ValueError, match="model 1 has"):
        f(z, [z[0], z[1][:4]], w, thr)
    for bad in (torch.ones(4), torch.ones(3, dtype=torch.float64), torch.ones(3, 1), [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="scale"):
            f(z, z, w, thr, scale=bad)
    many = [torch.zeros(1, 128, 128).expand(65536, 128, 128)] * 2           # (a view: no memory behind the 65536 outcomes)
    with pytest.raises(ValueError, match="at most 65535"):
        f(z, z, many, torch.zeros(65536))
    for bad in ((torch.zeros(5, 5, dtype=torch.int32),) * 2, torch.zeros(5, 5), "count"):
        with pytest.raises(ValueError, match="triple"):
            f(z, z, w, thr, out=bad)
    with pytest.raises(ValueError, match="GPU"):                            # a well-formed call on CPU tensors: no CPU fallback
        f(z, z, w, thr, scale=torch.ones(3))


def _plane_per_outcome(N, n_out):
    return torch.zeros((n_out, (N + 31) // 32, (N + 63) // 64 * 64), dtype=torch.int32)


def test_the_pipeline_functions_refuse_bad_calls_without_a_device():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    for fn in (pipeline.ensemble_outcome_profile, lambda m, e, t, **kw: pipeline.ensemble_most_flagged_pairs(m, e, t, 10, **kw)):
        with pytest.raises(ValueError, match="1..8"):
            fn(w, z[:1], 0.9)
        with pytest.raises(ValueError, match="1..8"):
            fn([], [], 0.9)
        with pytest.raises(ValueError, match="1..8"):
            fn((w * 5)[:9], (z * 5)[:9], 0.9)
        with pytest.raises(ValueError, match="GPU"):
            fn(w, z, 0.9)
        with pytest.raises(ValueError, match="out of scope"):
            fn(w, z, 0.9, exclude=_plane_per_outcome(5, 3))
        with pytest.raises(ValueError, match="known_pairs_mask"):
            fn(w, z, 0.9, exclude=torch.zeros(5, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="eligible"):
        pipeline.ensemble_outcome_profile(w, z, 0.9, eligible="upper")
    for bad in (0, 65536, True, 2.0):
        with pytest.raises(ValueError, match="chunk"):
            pipeline.ensemble_outcome_profile(w, z, 0.9, chunk=bad)
    for bad in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="K"):
            pipeline.ensemble_most_flagged_pairs(w, z, 0.9, bad)
    # the single-model twin checks its mask before it looks at the model
    with pytest.raises(ValueError, match="out of scope"):
        pipeline.most_flagged_pairs(None, z[0], 0.9, 10, exclude=_plane_per_outcome(5, 3))
    with pytest.raises(ValueError, match="known_pairs_mask"):
        pipeline.most_flagged_pairs(None, z[0], 0.9, 10, exclude="known")


# ---- the shared row-block walk on the CPU -----------------------------------------------------------------------------------------
def _cpu_setting(N, L, seed, levels=None):
    """A dense [L, N, N] tensor on the CPU, cuts and scales, and the ALL-mode profile callable of its row blocks.  ``levels``: the
    values are drawn from that many distinct numbers, so counts AND margins tie all over the place."""
    g = torch.Generator().manual_seed(seed)
    dense = torch.rand(L, N, N, generator=g)
    if levels:
        dense = torch.floor(dense * levels) / levels
    thr = torch.full((L,), 0.5)
    scale = torch.tensor([1.0, 2.0, 0.5, 4.0][:L])
    calls = []

    def block(r0, r1):
        calls.append((r0, r1))
        return dense_profile(dense[:, r0:r1, :r1].contiguous(), thr, scale, "all")

    return dense, thr, scale, block, calls


def _brute_force(dense, thr, scale, K, lo=0, removed=None):
    count, best, margin = dense_profile(dense, thr, scale, "lower")
    N = count.shape[0]
    pairs = [(i, j) for i in range(N) for j in range(i) if removed is None or not bool(removed[i, j])]
    pairs.sort(key=lambda p: (-int(count[p]), -float(margin[p]), p[0], p[1]))
    pairs = pairs[:K]
    pad = K - len(pairs)
    b = [int(best[p]) for p in pairs]
    return ([int(count[p]) for p in pairs] + [0] * pad, [p[0] for p in pairs] + [-1] * pad, [p[1] for p in pairs] + [-1] * pad,
            [x + lo if x >= 0 else x for x in b] + [-1] * pad, [float(margin[p]) for p in pairs] + [-INF] * pad)


def _lists(res):
    assert [t.dtype for t in res] == [torch.int32, torch.int64, torch.int64, torch.int64, torch.float32]
    return tuple(t.tolist() for t in res)


@pytest.mark.parametrize("rows_per_block", [1, 7, 1000])
@pytest.mark.parametrize("levels", [None, 3])
def test_the_shared_walk_equals_the_brute_force_sort(levels, rows_per_block):
    from madrigal_amd.pipeline import _most_flagged
    N, L = 23, 4
    dense, thr, scale, block, calls = _cpu_setting(N, L, 1, levels)
    for K in (1, 10, 60, N * (N - 1) // 2, N * (N - 1) // 2 + 5):           # the last: padded
        calls.clear()
        got = _lists(_most_flagged(block, N, K, 3, 48 * N * rows_per_block, torch.device("cpu")))
        assert got == _brute_force(dense, thr, scale, K, lo=3), (K, levels)
        assert calls[0][0] == 1 and calls[-1][1] == N and all(a[1] == b[0] for a, b in zip(calls, calls[1:]))
        assert len(calls) == -(-(N - 1) // min(rows_per_block, N))


def test_a_tie_at_the_kth_place_is_broken_by_the_pair_indices():
    """Every pair has the same count and the same margin: the K best are the first K pairs in (i, j) order, whatever the blocks."""
    from madrigal_amd.pipeline import _most_flagged
    N, L = 12, 2
    dense = torch.full((L, N, N), 0.75)
    thr, scale = torch.full((L,), 0.5), None
    block = lambda r0, r1: dense_profile(dense[:, r0:r1, :r1].contiguous(), thr, scale, "all")      # noqa: E731
    for rows in (1, 4, 100):
        c, h, t, b, m = _lists(_most_flagged(block, N, 8, 0, 48 * N * rows, torch.device("cpu")))
        assert list(zip(h, t)) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1)]
        assert c == [L] * 8 and b == [0] * 8 and m == [0.25] * 8
    # two levels: the K-th place falls inside the group of the lower level
    dense[:, 5, 2] = dense[:, 9, 7] = 0.875
    got = _lists(_most_flagged(block, N, 4, 0, 48 * N * 3, torch.device("cpu")))
    assert list(zip(got[1], got[2])) == [(5, 2), (9, 7), (1, 0), (2, 0)] and got == _brute_force(dense, thr, scale, 4)


def _pack(removed: torch.Tensor) -> torch.Tensor:
    """A bool [N, N] plane in the packed layout of ops.pair_mask (bit i & 31 of word [0, i >> 5, j]), built on the CPU."""
    N = removed.shape[0]
    nrb, ld = (N + 31) // 32, (N + 63) // 64 * 64
    padded = torch.zeros((nrb * 32, ld), dtype=torch.int64)
    padded[:N, :N] = removed
    words = (padded.view(nrb, 32, ld) << torch.arange(32)[None, :, None]).sum(1)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)[None]


def test_excluded_pairs_never_enter_the_ranking():
    from madrigal_amd import ops
    from madrigal_amd.pipeline import _most_flagged
    N, L = 40, 3
    dense, thr, scale, block, _ = _cpu_setting(N, L, 2, 3)
    top = _brute_force(dense, thr, scale, 6)
    g = torch.Generator().manual_seed(5)
    heads = torch.cat([torch.randint(0, N, (60,), generator=g), torch.tensor(top[1])])
    tails = torch.cat([torch.randint(0, N, (60,), generator=g), torch.tensor(top[2])])
    removed = torch.zeros((N, N), dtype=torch.bool)
    removed[heads, tails] = True
    removed |= removed.T.clone()                                            # both sides, as known_pairs_mask
    known = _pack(removed)
    assert torch.equal(ops.pair_mask_dense(known, N, N)[0], removed)
    assert all(bool(removed[i, j]) for i, j in zip(top[1], top[2]))
    for rows in (1, 9, 100):
        for K in (6, 50, N * N):
            got = _lists(_most_flagged(block, N, K, 0, 48 * N * rows, torch.device("cpu"), known))
            assert got == _brute_force(dense, thr, scale, K, removed=removed), (rows, K)
            assert not any(bool(removed[i, j]) for i, j in zip(got[1], got[2]) if i >= 0)
    everything = _pack(torch.ones((N, N), dtype=torch.bool))
    got = _lists(_most_flagged(block, N, 5, 0, 1 << 30, torch.device("cpu"), everything))
    assert got[1] == [-1] * 5 and got[0] == [0] * 5 and got[4] == [-INF] * 5
