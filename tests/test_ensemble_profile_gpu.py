"""Per-pair outcome profiles over a checkpoint ensemble on the GPU (ops.bilinear_ensemble_profile, pipeline.ensemble_outcome_profile /
ensemble_most_flagged_pairs, most_flagged_pairs(exclude=)) against the dense ensemble product, exactly.

The reference is always ``tests/profile_ref.py::dense_profile`` of the GENERAL ensemble sweep on the card,
``ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws)`` (the clone on the tail side forces the non-mirrored sweep, whose
values (z_i W) z_j are the ones the profile sees).  Every comparison is ``torch.equal`` on counts and best and on the int32 view of
the margin: no tolerance is involved.

Two input regimes (z ~ N(0,1) * scale, W ~ N(0,1) / sqrt(128), symmetrised):
  scale 0.3: no probability is 0 or 1 -- tests the values and >= on an attained value;
  scale 1.0: several per cent of all probabilities are exactly 1.0 at K = 1, fewer at K = 2 -- exact ties of the margin across
             outcomes, where "the lowest outcome" decides ``best``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from profile_ref import dense_profile, same

pytestmark = pytest.mark.gpu

L = 5
INF = float("inf")
INT_SENTINEL, VAL_SENTINEL = -12345, -777.25
PREC = {"f32": 0, "bf16x3": 1}
ELIGIBLE = {"all": 0, "not_self": 1, "lower": 2}
SCALE = [2.0, 0.37, 5.5, 1.0, 0.0123]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _dense(zh, zt, ws, prec):
    from madrigal_amd import ops
    return ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws, precision=prec).contiguous()


@functools.lru_cache(maxsize=None)
def _case(K, nh, nt, scale, prec, one_set, tied=False, seed=0):
    """Inputs on the card and their dense general-sweep product: (zh, zt, ws, P [L,nh,nt] contiguous).  Shared; never modified.
    ``tied``: outcome 2 has outcome 0's weight in every model."""
    from madrigal_amd import ops
    zh = [_rand((nh, 128), 1000 * seed + 10 * m, scale).cuda() for m in range(K)]
    zt = zh if one_set else [_rand((nt, 128), 1000 * seed + 10 * m + 1, scale).cuda() for m in range(K)]
    ws = []
    for m in range(K):
        w = _rand((L, 128, 128), 1000 * seed + 10 * m + 2, 1 / np.sqrt(128))
        if tied:
            w[2] = w[0]
        ws.append(ops.symmetrize(w.cuda()))
    return zh, zt, ws, _dense(zh, zt, ws, prec)


@functools.lru_cache(maxsize=None)
def _threshold_sets(K, nh, nt, scale, prec, one_set, tied=False):
    """The nine threshold vectors of a case, one cut per outcome each, from its dense product."""
    P = _case(K, nh, nt, scale, prec, one_set, tied)[3]
    dev = P.device
    flat = torch.sort(P.reshape(L, -1), dim=1).values
    n = flat.shape[1]
    attained = P[:, nh - 1, min(3, nt - 1)].contiguous()
    median = flat[:, (n - 1) // 2].contiguous()
    top = flat[:, int(0.999 * (n - 1))].contiguous()                  # about 0.1 % at or above it (an attained value)
    full = lambda v: torch.full((L,), v, device=dev)                 # noqa: E731
    return {"ninf": full(-INF), "pinf": full(INF), "zero": full(0.0), "one": full(1.0), "above": full(1.5), "attained": attained,
            "median": median, "top": top,
            "mixed": torch.stack([full(-INF)[0], attained[1], full(1.0)[2], full(INF)[3], median[4]]).contiguous()}


def _allowed(nh, nt, eligible):
    i = torch.arange(nh, device="cuda")[:, None]
    j = torch.arange(nt, device="cuda")[None, :]
    if eligible == "all":
        return torch.ones((nh, nt), dtype=torch.bool, device="cuda")
    return (j != i) if eligible == "not_self" else (j < i)


def _check_case(K, nh, nt, scale, prec, eligible, one_set):
    from madrigal_amd import ops
    zh, zt, ws, P = _case(K, nh, nt, scale, prec, one_set)
    ok = _allowed(nh, nt, eligible)
    sc = torch.tensor(SCALE, device="cuda")
    for name, thr in _threshold_sets(K, nh, nt, scale, prec, one_set).items():
        for s in (None, sc):
            got = ops.bilinear_ensemble_profile(zh, zt, ws, thr, scale=s, eligible=eligible, precision=prec)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
            assert same(got, dense_profile(P, thr, s, eligible)), (name, s is not None)
            c, b, m = got
            assert bool((c[~ok] == 0).all()) and bool((b[~ok] == -1).all()) and bool((m[~ok] == -INF).all()), name
            if name == "ninf":
                assert bool((c[ok] == L).all()) and bool((b[ok] == 0).all()) and bool((m[ok] == INF).all())
            elif name == "pinf":
                assert bool((c == 0).all()) and bool((b == -1).all()) and bool((m == -INF).all())
            elif name == "zero":
                assert bool((c[ok] == L).all())
            elif name == "above":
                assert bool((c == 0).all()) and bool((b[ok] >= 0).all()) and bool(torch.isfinite(m[ok]).all()) and bool((m[ok] < 0).all())


def _shape(name):
    from madrigal_amd import ops
    G = ops.bilinear_ensemble_profile_tiles()
    return {"1x1": (1, 1), "33x65": (33, 65), "129xG-1": (129, 64 * G - 1), "129xG": (129, 64 * G), "129xG+1": (129, 64 * G + 1),
            "300x333": (300, 333)}[name]


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", ["1x1", "33x65", "129xG-1", "129xG", "129xG+1", "300x333"])
def test_sizes_and_cuts_against_the_dense_product(shape, K, scale, prec):
    """Two drug sets, every pair eligible: one element, a ragged tile, the workgroup's column boundary - 1 / + 0 / + 1 behind a
    second row block, and several row blocks by several column groups."""
    nh, nt = _shape(shape)
    _check_case(K, nh, nt, scale, prec, "all", False)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("N", [129, 300, 513])
def test_one_drug_set_against_itself(N, eligible, K, scale, prec):
    """Squares past a 128-row block that end on a ragged tile; under LOWER some workgroups store the sentinels and leave, others
    sweep fewer tiles than they own, and the tiles on the diagonal are masked element by element."""
    _check_case(K, N, N, scale, prec, eligible, True)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(1, 1.0), (2, 1.0), (5, 0.3)])
def test_equal_outcomes_keep_the_lower_index(K, scale, prec):
    """w[2] = w[0] in every model, thr[2] = thr[0], scale[2] = scale[0]: u_2 == u_0 for every pair, so best is never 2."""
    from madrigal_amd import ops
    nh, nt = 200, 150
    zh, zt, ws, P = _case(K, nh, nt, scale, prec, False, True)
    assert torch.equal(P[2], P[0])
    sets = _threshold_sets(K, nh, nt, scale, prec, False, True)
    sc = torch.tensor([2.0, 0.37, 2.0, 1.0, 0.0123], device="cuda")
    for name in ("median", "attained", "one", "above", "ninf"):
        thr = sets[name].clone()
        thr[2] = thr[0]
        for s in (None, sc):
            got = ops.bilinear_ensemble_profile(zh, zt, ws, thr, scale=s, precision=prec)
            assert same(got, dense_profile(P, thr, s, "all")), name
            assert not bool((got[1] == 2).any()), name
            if s is None and name != "ninf":
                assert bool((got[1] == 0).any()), name                 # outcome 0 (and with it 2) does win somewhere


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("eligible", ["all", "lower"])
def test_saturated_ties_across_outcomes_keep_the_lowest(K, eligible, prec):
    """Saturated inputs, cut 1.0: pairs whose probability is exactly 1.0 for two or more outcomes have margin 0 for each of them;
    best is the lowest such outcome."""
    from madrigal_amd import ops
    N = 513
    z, _, ws, P = _case(K, N, N, 1.0, prec, True)
    ok = _allowed(N, N, eligible)
    ones = (P == 1.0)
    multi = (ones.sum(0) >= 2) & ok
    assert int(multi.sum()) > 0                                         # a condition on the input
    lowest = torch.where(ones, torch.arange(L, device="cuda")[:, None, None], L).min(0).values
    thr = torch.full((L,), 1.0, device="cuda")
    for s in (None, torch.tensor(SCALE, device="cuda")):
        c, b, m = ops.bilinear_ensemble_profile(z, z, ws, thr, scale=s, eligible=eligible, precision=prec)
        assert torch.equal(b[multi].long(), lowest[multi]) and bool((m[multi] == 0).all())
        assert torch.equal(c[multi].long(), ones.sum(0)[multi])
        assert bool((c[multi] >= 2).all())


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_the_counts_sum_to_the_selection_sweeps(eligible, prec):
    """Summed over the pairs of a row, the per-pair counts are the per-outcome row counts of bilinear_ensemble_select_count summed
    over the outcomes."""
    from madrigal_amd import ops
    K, N = 2, 300
    z, _, ws, P = _case(K, N, N, 0.3, prec, True)
    thr = _threshold_sets(K, N, N, 0.3, prec, True)["median"]
    c = ops.bilinear_ensemble_profile(z, z, ws, thr, eligible=eligible, precision=prec)[0]
    rows = ops.bilinear_ensemble_select_count(z, z, ws, thr, eligible=eligible, precision=prec)
    assert int(rows.sum()) > 0 and torch.equal(c.sum(1), rows.sum(0))


@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
def test_two_calls_agree_and_out_is_reused_contiguous_or_pitched(K, scale):
    from madrigal_amd import ops
    nh, nt = 300, 333
    zh, zt, ws, P = _case(K, nh, nt, scale, "bf16x3", False)
    thr = _threshold_sets(K, nh, nt, scale, "bf16x3", False)["median"]
    sc = torch.tensor(SCALE, device="cuda")
    first = ops.bilinear_ensemble_profile(zh, zt, ws, thr, scale=sc)
    keep = tuple(t.clone() for t in first)
    for t in first:
        t.fill_(7)
    again = ops.bilinear_ensemble_profile(zh, zt, ws, thr, scale=sc, out=first)
    assert all(a is b for a, b in zip(again, first)) and same(again, keep)
    dts = (torch.int32, torch.int32, torch.float32)
    whole = tuple(torch.full((nh, nt + 5), 7, dtype=dt, device="cuda") for dt in dts)
    pitched = tuple(t[:, :nt] for t in whole)
    got = ops.bilinear_ensemble_profile(zh, zt, ws, thr, scale=sc, out=pitched)
    assert same(got, keep) and all(bool((t[:, nt:] == 7).all()) for t in whole)
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_ensemble_profile(zh, zt, ws, thr, out=(pitched[0], pitched[1], keep[2]))      # two pitches
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_ensemble_profile(zh, zt, ws, thr, out=(keep[0], keep[1], keep[2].double()))


def _c_profile(zh, zt, ws, thr, scale, prec, eligible, pad=3, n_models=None, n_labels=None, D=128, nt=None, workspace=True):
    """mdg_bilinear_ensemble_profile through the C entry into sentinel-filled outputs with a guard row and `pad` pitch columns
    -> (rc, count, best, margin) with the full padded tensors."""
    from madrigal_amd import ops
    from madrigal_amd._lib import lib
    K = len(zh)
    prec = PREC.get(prec, prec)                                             # a name, or a raw precision code
    nh = zh[0].shape[0]
    nt = zt[0].shape[0] if nt is None else nt
    nl = ws[0].shape[0] if n_labels is None else n_labels
    ldo = nt + pad
    count = torch.full((nh + 1, max(ldo, 1)), INT_SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((nh + 1, max(ldo, 1)), INT_SENTINEL, dtype=torch.int32, device="cuda")
    margin = torch.full((nh + 1, max(ldo, 1)), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    buf, nbytes = (None, 0)
    if workspace:
        buf, nbytes = ops._scratch("mdg_bilinear_ensemble_profile_workspace_bytes", zh[0].device, nh, nt, nl, 128, K, prec)
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    rc = lib().mdg_bilinear_ensemble_profile(arr(zh), arr(zt), arr(ws), K if n_models is None else n_models, thr.data_ptr(),
                                             None if scale is None else scale.data_ptr(), count.data_ptr(), best.data_ptr(),
                                             margin.data_ptr(), ldo, nh, nt, nl, D, prec, ELIGIBLE[eligible],
                                             None if buf is None else buf.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    return rc, count, best, margin


def _untouched(res):
    return bool((res[1] == INT_SENTINEL).all()) and bool((res[2] == INT_SENTINEL).all()) and bool((res[3] == VAL_SENTINEL).all())


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_writes_are_bounded_and_complete(prec, eligible):
    """Sentinel-filled outputs with a guard row and three pitch columns (ldo > n_tail) through the C entry: no sentinel is left
    inside [nh, nt], the result is the reference, the guard row and the pitch padding are untouched."""
    K, N = 2, 513
    z, _, ws, P = _case(K, N, N, 0.3, prec, True)
    thr = _threshold_sets(K, N, N, 0.3, prec, True)["median"]
    sc = torch.tensor(SCALE, device="cuda")
    rc, count, best, margin = _c_profile(z, z, ws, thr, sc, prec, eligible)
    assert rc == 0
    inner = (count[:N, :N], best[:N, :N], margin[:N, :N])
    assert not bool((inner[0] == INT_SENTINEL).any()) and not bool((inner[1] == INT_SENTINEL).any()) and not bool((inner[2] == VAL_SENTINEL).any())
    assert same(inner, dense_profile(P, thr, sc, eligible))
    for t, s in ((count, INT_SENTINEL), (best, INT_SENTINEL), (margin, VAL_SENTINEL)):
        assert bool((t[N] == s).all()) and bool((t[:, N:] == s).all())


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_a_nan_row_of_one_model_blanks_that_row_only(prec):
    from madrigal_amd import ops
    K, nh, nt = 5, 300, 333
    zh, zt, ws, P = _case(K, nh, nt, 0.3, prec, False)
    thr = _threshold_sets(K, nh, nt, 0.3, prec, False)["median"]
    clean = ops.bilinear_ensemble_profile(zh, zt, ws, thr, precision=prec)
    bad = [t.clone() for t in zh]
    bad[3][131] = float("nan")
    c, b, m = ops.bilinear_ensemble_profile(bad, zt, ws, thr, precision=prec)
    assert bool((c[131] == 0).all()) and bool((b[131] == -1).all()) and bool((m[131] == -INF).all())
    rest = torch.arange(nh, device="cuda") != 131
    assert same((c[rest], b[rest], m[rest]), tuple(t[rest] for t in clean))
    assert same((c, b, m), dense_profile(_dense(bad, zt, ws, prec), thr, None, "all"))


def test_no_outcome_writes_the_ineligible_values_and_empty_sets_give_empty_results():
    from madrigal_amd import ops
    z = [torch.randn(200, 128, device="cuda") for _ in range(2)]
    w = [ops.symmetrize(torch.randn(2, 128, 128, device="cuda")) for _ in range(2)]
    thr = torch.zeros(2, device="cuda")
    for eligible in ("all", "lower"):
        c, b, m = ops.bilinear_ensemble_profile(z, z, [t[:0] for t in w], thr[:0], eligible=eligible)
        assert c.shape == (200, 200) and bool((c == 0).all()) and bool((b == -1).all()) and bool((m == -INF).all())
    res = _c_profile(z, z, w, thr, None, "bf16x3", "all", n_labels=0, workspace=False)
    assert res[0] == 0
    assert bool((res[1][:200, :200] == 0).all()) and bool((res[2][:200, :200] == -1).all()) and bool((res[3][:200, :200] == -INF).all())
    assert bool((res[1][200] == INT_SENTINEL).all()) and bool((res[3][:, 200:] == VAL_SENTINEL).all())
    assert ops.bilinear_ensemble_profile([t[:0] for t in z], z, w, thr)[0].shape == (0, 200)
    assert ops.bilinear_ensemble_profile(z, [t[:0] for t in z], w, thr)[2].shape == (200, 0)


def test_c_level_refusals_launch_nothing():
    from madrigal_amd import ops
    from madrigal_amd._lib import lib
    K = 2
    z = [torch.randn(6, 128, device="cuda") for _ in range(K)]
    w = [ops.symmetrize(torch.randn(2, 128, 128, device="cuda")) for _ in range(K)]
    thr = torch.zeros(2, device="cuda")
    one = torch.ones(2, device="cuda")
    err = lambda: lib().mdg_last_error()          # noqa: E731
    name = b"mdg_bilinear_ensemble_profile"
    nan_thr = torch.tensor([0.0, float("nan")], device="cuda")
    res = _c_profile(z, z, w, nan_thr, None, "f32", "all")
    assert res[0] == -1 and name in err() and b"NaN" in err() and _untouched(res)
    for bad in (0.0, -1.0, INF, float("nan")):
        res = _c_profile(z, z, w, thr, torch.tensor([1.0, bad], device="cuda"), "f32", "all")
        assert res[0] == -1 and b"scale[1]" in err() and _untouched(res), bad
    for nm in (0, 9):
        res = _c_profile(z, z, w, thr, one, "f32", "all", n_models=nm)
        assert res[0] == -1 and b"n_models" in err() and _untouched(res)
    res = _c_profile(z, z, w, thr, one, "f32", "all", D=64)
    assert res[0] == -1 and b"D must be" in err() and _untouched(res)
    res = _c_profile(z, z, w, thr, one, "f32", "all", n_labels=65536)
    assert res[0] == -1 and b"n_labels" in err() and _untouched(res)
    res = _c_profile(z, z, w, thr, one, "f32", "all", pad=-1)
    assert res[0] == -1 and b"ldo" in err() and _untouched(res)
    for mode in ("not_self", "lower"):
        res = _c_profile(z, z, w, thr, one, "f32", mode, nt=4)
        assert res[0] == -1 and b"one drug set" in err() and _untouched(res)
    for prec in (2, 3):                                                     # the 16-bit precisions: the ensemble family has none
        res = _c_profile(z, z, w, thr, one, prec, "all", workspace=False)
        assert res[0] == -1 and b"not offered" in err() and _untouched(res)
    res = _c_profile(z, z, w, thr, one, "bf16x3", "all", workspace=False)   # the operand images need a workspace
    assert res[0] == -2 and name in err() and b"workspace" in err() and _untouched(res)
    res = _c_profile(z, z, w, thr, one, "f32", "all")                       # the same call, well-formed, does write
    assert res[0] == 0 and not _untouched(res)
    # the wrapper
    with pytest.raises(ValueError, match="NaN"):
        ops.bilinear_ensemble_profile(z, z, w, nan_thr)
    with pytest.raises(ValueError, match="scale"):
        ops.bilinear_ensemble_profile(z, z, w, thr, scale=torch.tensor([1.0, 0.0], device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_profile([t.cpu() for t in z], [t.cpu() for t in z], [t.cpu() for t in w], thr.cpu())
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_ensemble_profile(z, [t[:4] for t in z], w, thr, eligible="lower")
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_ensemble_profile(z, z, w, thr, out=(torch.empty(6, 6, device="cuda"),) * 3)


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_models():
    """Three configs.build_model checkpoints (drugbank163 layout, 6 outcomes) differing by seed, and the embeddings of 300 drugs
    from generate_embeddings under each (the recipe of tests/test_ensemble_select_gpu.py)."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n, n_out = 300, 6
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = torch.randn((n, 128), generator=torch.Generator().manual_seed(6)).cuda()
    models, zs = [], []
    for seed in (3, 4, 5):
        torch.manual_seed(seed)
        model = configs.build_model("drugbank163", bkg["data"], n_out).cuda().eval()
        with M.precision("bf16x3"):
            z = generate_embeddings(model, b, kgc, kg_filler=filler).contiguous()
        assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
        models.append(model)
        zs.append(z)
    return models, zs


def _same64(got, ref, offset=0):
    """A pipeline triple (best int64, model outcome indices) against a reference triple (best int32, relative to ``offset``)."""
    rb = ref[1].long()
    rb = torch.where(rb >= 0, rb + offset, rb)
    return got[1].dtype == torch.int64 and same(got, (ref[0], rb, ref[2]))


def _brute_force(profile, K, removed=None):
    """The K first lower-triangle pairs of a dense profile under (count descending, margin descending, i ascending, j ascending),
    without the pairs of ``removed`` (bool [N, N]) -> (count, i, j, best int64, margin)."""
    count, best, margin = profile
    N = count.shape[0]
    i, j = torch.tril_indices(N, N, -1, device=count.device)                      # ascending (i, j)
    if removed is not None:
        keep = ~removed[i, j]
        i, j = i[keep], j[keep]
    c, b, m = count[i, j], best[i, j].long(), margin[i, j]
    order = torch.arange(i.numel(), device=count.device)
    order = order[torch.sort(m[order].double(), descending=True, stable=True).indices]
    order = order[torch.sort(c[order], descending=True, stable=True).indices][:K]
    return c[order], i[order], j[order], b[order], m[order]


def _equal5(got, want):
    n = want[0].numel()
    return (torch.equal(got[0][:n], want[0]) and torch.equal(got[1][:n], want[1]) and torch.equal(got[2][:n], want[2])
            and torch.equal(got[3][:n], want[3]) and torch.equal(got[4][:n].view(torch.int32), want[4].view(torch.int32)))


def _padded(got, n):
    return (got[0][n:].tolist() == [0] * (got[0].numel() - n) and bool((got[1][n:] == -1).all()) and bool((got[2][n:] == -1).all())
            and bool((got[3][n:] == -1).all()) and bool((got[4][n:] == -INF).all()))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_pipeline_products_on_three_checkpoints(small_models, prec):
    """ensemble_outcome_profile equals the reference on the dense general sweep: whole, over a label range, over merged chunks of two
    outcomes, and as head_rows blocks; exclude= blanks exactly the known pairs.  ensemble_most_flagged_pairs equals the brute-force
    sort of the dense lower-triangle profile: over several row blocks, in one block, padded, and with the known pairs removed."""
    from madrigal_amd import models as M
    from madrigal_amd import ops
    from madrigal_amd.pipeline import ensemble_all_pairs, ensemble_most_flagged_pairs, ensemble_outcome_profile, known_pairs_mask
    models, zs = small_models
    N, n_out = zs[0].shape[0], 6
    with M.precision(prec), torch.no_grad():
        dense = ensemble_all_pairs(models, zs, drug_2_inds=list(range(N))).contiguous()       # an index list on the tail side: the general sweep
        thr = torch.quantile(dense.reshape(n_out, -1), 0.9, dim=1).contiguous()
        scale = torch.tensor([1.0, 2.5, 0.5, 1.25, 3.0, 0.75], device="cuda")
        for eligible in ("lower", "not_self", "all"):
            ref = dense_profile(dense, thr, scale, eligible)
            assert _same64(ensemble_outcome_profile(models, zs, thr, scale, eligible=eligible), ref), eligible
            assert _same64(ensemble_outcome_profile(models, zs, thr, scale, eligible=eligible, chunk=2), ref), eligible     # three chunks, merged
            part = ensemble_outcome_profile(models, zs, thr[1:5], scale[1:5], label_range=(1, 5), eligible=eligible)
            assert _same64(part, dense_profile(dense[1:5], thr[1:5], scale[1:5], eligible), offset=1), eligible
            part = ensemble_outcome_profile(models, zs, thr[1:6], scale[1:6], label_range=(1, 6), eligible=eligible, chunk=2)
            assert _same64(part, dense_profile(dense[1:6], thr[1:6], scale[1:6], eligible), offset=1), eligible
            blocks = [ensemble_outcome_profile(models, zs, thr, scale, eligible=eligible, head_rows=hr) for hr in ((0, 100), (100, 100), (100, N))]
            assert blocks[1][0].shape == (0, N)
            assert _same64(tuple(torch.cat([b[k] for b in blocks], 0) for k in range(3)), ref), eligible
        one = ensemble_outcome_profile(models, zs, 0.9)                         # one number for every outcome, no scale
        assert _same64(one, dense_profile(dense, torch.full((n_out,), 0.9, device="cuda"), None, "not_self"))
        # the K most flagged pairs
        low = dense_profile(dense, thr, scale, "lower")
        K = 50
        want = _brute_force(low, K)
        got = ensemble_most_flagged_pairs(models, zs, thr, K, scale=scale, max_bytes=48 * N * 70)          # blocks of 70 rows
        assert [t.shape for t in got] == [(K,)] * 5 and got[1].dtype == torch.int64 and got[0].dtype == torch.int32
        assert _equal5(got, want) and bool((got[1] > got[2]).all()) and int(got[0][0]) >= int(got[0][-1]) >= 1
        whole = ensemble_most_flagged_pairs(models, zs, thr, K, scale=scale)    # one block
        assert _equal5(whole, want)
        part = ensemble_most_flagged_pairs(models, zs, thr[2:5], K, scale=scale[2:5], label_range=(2, 5), max_bytes=48 * N * 130)
        w = _brute_force(dense_profile(dense[2:5], thr[2:5], scale[2:5], "lower"), K)
        assert _equal5(part, (w[0], w[1], w[2], torch.where(w[3] >= 0, w[3] + 2, w[3]), w[4]))
        few_z = [z[:4].contiguous() for z in zs]
        few = ensemble_most_flagged_pairs(models, few_z, thr, 10, scale=scale)  # K > N (N - 1) / 2 = 6: padded
        w = _brute_force(dense_profile(dense[:, :4, :4].contiguous(), thr, scale, "lower"), 10)
        assert w[0].numel() == 6 and _equal5(few, w) and _padded(few, 6)
        # the known network: random pairs plus the 20 most flagged ones, as one shared plane
        g = torch.Generator().manual_seed(12)
        kh, kt = torch.randint(0, N, (900,), generator=g), torch.randint(0, N, (900,), generator=g)
        known = known_pairs_mask(N, torch.cat([kh, want[1][:20].cpu()]), torch.cat([kt, want[2][:20].cpu()]))
        removed = ops.pair_mask_dense(known, N, N)[0]
        assert bool(removed[want[1][:20], want[2][:20]].all())
        novel = _brute_force(low, K, removed)
        got = ensemble_most_flagged_pairs(models, zs, thr, K, scale=scale, max_bytes=48 * N * 70, exclude=known)
        assert _equal5(got, novel) and not bool(removed[got[1], got[2]].any())
        for eligible in ("lower", "not_self", "all"):
            ref = dense_profile(dense, thr, scale, eligible)
            ref = (ref[0].masked_fill(removed, 0), ref[1].masked_fill(removed, -1), ref[2].masked_fill(removed, -INF))
            assert _same64(ensemble_outcome_profile(models, zs, thr, scale, eligible=eligible, exclude=known), ref), eligible
            blocks = [ensemble_outcome_profile(models, zs, thr, scale, eligible=eligible, head_rows=hr, exclude=known) for hr in ((0, 170), (170, N))]
            assert _same64(tuple(torch.cat([b[k] for b in blocks], 0) for k in range(3)), ref), eligible
        per_outcome = known_pairs_mask(N, kh, kt, labels=torch.randint(0, n_out, (900,), generator=g), n_labels=n_out)
        with pytest.raises(ValueError, match="out of scope"):
            ensemble_most_flagged_pairs(models, zs, thr, K, exclude=per_outcome)
        with pytest.raises(ValueError, match="out of scope"):
            ensemble_outcome_profile(models, zs, thr, exclude=per_outcome)
    with pytest.raises(ValueError):
        ensemble_outcome_profile(models, zs, thr[:4])
    with pytest.raises(ValueError):
        ensemble_outcome_profile(models, zs, thr, label_range=(0, 7))
    with pytest.raises(ValueError):
        ensemble_most_flagged_pairs(models, zs, thr, 0)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_most_flagged_pairs_of_one_model_without_the_known_pairs(small_models, prec):
    """most_flagged_pairs(exclude=) on one checkpoint against the brute force with the known pairs removed; exclude=None is the call
    without the argument."""
    from madrigal_amd import models as M
    from madrigal_amd import ops
    from madrigal_amd.pipeline import known_pairs_mask, most_flagged_pairs, score_all_pairs
    models, zs = small_models
    model, z = models[0], zs[0]
    N, n_out = z.shape[0], 6
    with M.precision(prec), torch.no_grad():
        dense = torch.cat([score_all_pairs(model, z, head_rows=(0, 150)), score_all_pairs(model, z, head_rows=(150, N))], 1)    # the general sweep
        thr = torch.quantile(dense.reshape(n_out, -1), 0.9, dim=1).contiguous()
        scale = torch.tensor([1.0, 2.5, 0.5, 1.25, 3.0, 0.75], device="cuda")
        low = dense_profile(dense, thr, scale, "lower")
        K = 50
        want = _brute_force(low, K)
        plain = most_flagged_pairs(model, z, thr, K, scale=scale, max_bytes=48 * N * 70)
        assert _equal5(plain, want)
        assert _equal5(most_flagged_pairs(model, z, thr, K, scale=scale, max_bytes=48 * N * 70, exclude=None), want)
        g = torch.Generator().manual_seed(13)
        kh, kt = torch.randint(0, N, (900,), generator=g), torch.randint(0, N, (900,), generator=g)
        known = known_pairs_mask(N, torch.cat([kh, want[1][:20].cpu()]), torch.cat([kt, want[2][:20].cpu()]))
        removed = ops.pair_mask_dense(known, N, N)[0]
        got = most_flagged_pairs(model, z, thr, K, scale=scale, max_bytes=48 * N * 70, exclude=known)
        assert _equal5(got, _brute_force(low, K, removed)) and not bool(removed[got[1], got[2]].any())
        assert not _equal5(got, want)
        per_outcome = known_pairs_mask(N, kh, kt, labels=torch.randint(0, n_out, (900,), generator=g), n_labels=n_out)
        with pytest.raises(ValueError, match="out of scope"):
            most_flagged_pairs(model, z, thr, K, exclude=per_outcome)
