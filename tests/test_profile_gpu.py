"""Per-pair outcome profiles of the all-pairs head on the GPU: mdg_bilinear_profile against the dense reference (profile_ref) over
the project's own dense general sweep -- count, best and the bits of margin exactly, in all four precisions (the kernel runs the
general sweep's own 32x32x16 products in the 16-bit modes too) --, its tie with mdg_bilinear_select_count, bounded writes through the
C entry, the refusals, and the pipeline products built on it (outcome_profile, most_flagged_pairs)."""
import functools

import pytest
import torch

from bincount_ref import eligible_mask, eligible_scores, inputs
from profile_ref import dense_profile, same

pytestmark = pytest.mark.gpu

L = 5
ALL_ONLY = [(1, 1), (33, 4), (300, 333)]
SQUARE = [(300, 300), (513, 513)]          # past a 256-row workgroup, ending on a ragged 64-column tile; LOWER skips tiles
TIED = [(33, 4), (300, 300)]               # shapes that also run with W[2] = W[0]: an exact tie across outcomes
ELIGIBLE = {"all": 0, "not_self": 1, "lower": 2}
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16": 3}
INT_SENTINEL, VAL_SENTINEL = -7, -12345.0
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if (nh, nt) in SQUARE else ["all"]


@functools.lru_cache(maxsize=None)
def _case(prec, nh, nt, tied=False):
    """(zh, zt, ws, dense) on the GPU: the inputs of bincount_ref and the STORE tensor of the general sweep in the same precision,
    computed once per precision and shape and never modified.  ``tied``: outcome 2 is a copy of outcome 0."""
    from madrigal_amd import ops
    zh, zt, w = inputs(nh, nt, L)
    if tied:
        w[2] = w[0]
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    return zh, zt, ws, ops.bilinear_allpairs(zh, zt, ws, precision=prec)


def _threshold_sets(dense, eligible):
    """{name: thr [L]}: -inf (every eligible pair flagged for every outcome), +inf (nothing), the outcome's maximum eligible score,
    the score of (row nh - 1, column 3) -- columns 5, 9 and nt - 2 tie with it exactly where they exist --, the median, the value
    with about 0.1 % of the eligible scores at or above it, and one vector mixing the kinds."""
    vals = eligible_scores(dense, eligible)
    M = vals.shape[1]
    nh, nt = dense.shape[1:]
    dev = dense.device
    sv = torch.sort(vals, dim=1).values
    sets = {"ninf": torch.full((L,), -INF, device=dev), "pinf": torch.full((L,), INF, device=dev), "max": sv[:, -1].clone(),
            "tie": dense[:, nh - 1, min(3, nt - 1)].clone(), "median": sv[:, (M - 1) // 2].clone(),
            "sparse": sv[:, M - max(1, round(0.001 * M))].clone()}
    sets["mixed"] = torch.stack([sets["sparse"][0], sets["ninf"][1], sets["tie"][2], sets["pinf"][3], sets["median"][4]])
    return {k: v.contiguous() for k, v in sets.items()}


def _scales(tied):
    s = torch.tensor([2.0, 0.37, 5.5, 1.0, 0.0123], device="cuda")
    if tied:
        s[2] = s[0]
    return (None, s)


def _check_all(ops, prec, nh, nt, tied):
    zh, zt, ws, dense = _case(prec, nh, nt, tied)
    if tied:
        assert torch.equal(dense[2].view(torch.int32), dense[0].view(torch.int32))
    for eligible in _modes(nh, nt):
        elig = eligible_mask(nh, nt, eligible, "cuda")
        for name, thr in _threshold_sets(dense, eligible).items():
            if tied and name != "mixed":
                assert float(thr[2]) == float(thr[0])
            for scale in _scales(tied):
                what = (prec, (nh, nt), tied, eligible, name, scale is not None)
                ref = dense_profile(dense, thr, scale, eligible)
                got = ops.bilinear_profile(zh, zt, ws, thr, scale=scale, eligible=eligible, precision=prec)
                assert got[0].shape == (nh, nt) and got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
                assert got[0].stride(0) % 4 == 0 and got[0].stride(1) == 1
                assert torch.equal(got[0], ref[0]), what + ("count", int((got[0] != ref[0]).sum()))
                assert torch.equal(got[1], ref[1]), what + ("best", int((got[1] != ref[1]).sum()))
                assert torch.equal(got[2].contiguous().view(torch.int32), ref[2].contiguous().view(torch.int32)), what + ("margin",)
                again = ops.bilinear_profile(zh, zt, ws, thr, scale=scale, eligible=eligible, precision=prec, out=got if scale is None else None)
                assert same(again, ref), what + ("second call",)
                if prec in ("f32", "bf16x3"):            # (the 16-bit select runs the regrouped row-statistics sweep)
                    sel = ops.bilinear_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec)
                    assert torch.equal(got[0].sum(1), sel.sum(0)), what + ("select_count",)
                if name == "ninf":
                    assert bool((got[0][elig] == L).all()) and bool((got[1][elig] == 0).all()) and bool((got[2][elig] == INF).all()), what
                if name == "pinf":
                    assert bool((got[0] == 0).all()) and bool((got[1] == -1).all()) and bool((got[2] == -INF).all()), what
                if tied and name != "mixed":
                    assert not bool((got[1] == 2).any()), what
                assert bool((got[0][~elig] == 0).all()) and bool((got[1][~elig] == -1).all()) and bool((got[2][~elig] == -INF).all()), what


@pytest.mark.parametrize("nh,nt", ALL_ONLY + SQUARE)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_profile_equals_the_dense_reference_bit_for_bit(ops, prec, nh, nt):
    """count, best and the bits of margin == the reference over the dense general sweep for every threshold set, with and without a
    scale vector; a second call (into the first call's tensors) is identical; count.sum(1) == the select sweep's counts summed over
    the outcomes; with outcome 2 a copy of outcome 0, best is never 2."""
    _check_all(ops, prec, nh, nt, False)
    if (nh, nt) in TIED:
        _check_all(ops, prec, nh, nt, True)


@pytest.mark.parametrize("nh,nt", ALL_ONLY + SQUARE)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_profile_of_the_16bit_modes_is_bit_equal_too(ops, prec, nh, nt):
    """The single-product modes run the general sweep's 32x32x16 products here (not the 16x16x32 regrouping of the row-statistics
    sweeps), so the same exact test holds."""
    _check_all(ops, prec, nh, nt, False)
    if (nh, nt) in TIED:
        _check_all(ops, prec, nh, nt, True)


def _c_profile(ops, zh, zt, ws, thr, scale, prec, eligible, pad=3, n_labels=None, D=128, nt=None, workspace=True):
    """mdg_bilinear_profile through the C entry into sentinel-filled outputs with a guard row and `pad` pitch columns
    -> (rc, count, best, margin) with the full padded tensors."""
    from madrigal_amd._lib import lib
    nh = zh.shape[0]
    nt = zt.shape[0] if nt is None else nt
    nl = ws.shape[0] if n_labels is None else n_labels
    ldo = nt + pad
    count = torch.full((nh + 1, ldo), INT_SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((nh + 1, ldo), INT_SENTINEL, dtype=torch.int32, device="cuda")
    margin = torch.full((nh + 1, ldo), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    buf, nbytes = (None, 0)
    if workspace:
        buf, nbytes = ops._scratch("mdg_bilinear_profile_workspace_bytes", zh.device, nh, nt, nl, 128, PREC[prec])
    rc = lib().mdg_bilinear_profile(zh.data_ptr(), zt.data_ptr(), ws.data_ptr(), thr.data_ptr(), None if scale is None else scale.data_ptr(),
                                    count.data_ptr(), best.data_ptr(), margin.data_ptr(), ldo, nh, nt, nl, D, PREC[prec], ELIGIBLE[eligible],
                                    None if buf is None else buf.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    return rc, count, best, margin


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "f16"])
def test_writes_are_bounded_and_complete(ops, prec, eligible):
    """Sentinel-filled outputs with a guard row and three pitch columns (ldo > n_tail) through the C entry: no sentinel is left
    inside [nh, nt], the result is the reference, the guard row and the pitch padding are untouched."""
    nh = nt = 513
    zh, zt, ws, dense = _case(prec, nh, nt)
    thr = _threshold_sets(dense, eligible)["median"]
    scale = _scales(False)[1]
    rc, count, best, margin = _c_profile(ops, zh, zt, ws, thr, scale, prec, eligible)
    assert rc == 0
    inner = (count[:nh, :nt], best[:nh, :nt], margin[:nh, :nt])
    assert not bool((inner[0] == INT_SENTINEL).any()) and not bool((inner[1] == INT_SENTINEL).any()) and not bool((inner[2] == VAL_SENTINEL).any())
    assert same(inner, dense_profile(dense, thr, scale, eligible))
    for t, s in ((count, INT_SENTINEL), (best, INT_SENTINEL), (margin, VAL_SENTINEL)):
        assert bool((t[nh] == s).all()) and bool((t[:, nt:] == s).all())


def test_refusals_launch_nothing(ops):
    from madrigal_amd._lib import lib
    zh, zt, ws, dense = _case("f32", 33, 4)
    z = torch.randn(6, 128, device="cuda")
    w = ops.symmetrize(torch.randn(2, 128, 128, device="cuda"))
    thr = torch.zeros(2, device="cuda")
    one = torch.ones(2, device="cuda")
    err = lambda: lib().mdg_last_error()          # noqa: E731

    def untouched(res):
        return bool((res[1] == INT_SENTINEL).all()) and bool((res[2] == INT_SENTINEL).all()) and bool((res[3] == VAL_SENTINEL).all())

    nan_thr = torch.tensor([0.0, float("nan")], device="cuda")
    res = _c_profile(ops, z, z, w, nan_thr, None, "f32", "all")
    assert res[0] == -1 and b"NaN" in err() and untouched(res)
    for bad in (0.0, -1.0, INF, float("nan")):
        res = _c_profile(ops, z, z, w, thr, torch.tensor([1.0, bad], device="cuda"), "f32", "all")
        assert res[0] == -1 and b"scale[1]" in err() and untouched(res), bad
    res = _c_profile(ops, z, z, w, thr, one, "f32", "all", D=64)
    assert res[0] == -1 and b"D must be" in err() and untouched(res)
    res = _c_profile(ops, z, z, w, thr, one, "f32", "all", n_labels=65536)
    assert res[0] == -1 and b"n_labels" in err() and untouched(res)
    for mode in ("not_self", "lower"):
        res = _c_profile(ops, z, z, w, thr, one, "f32", mode, nt=4)
        assert res[0] == -1 and b"one drug set" in err() and untouched(res)
    for prec in ("bf16x3", "bf16", "f16"):       # the operand images need a workspace: refused before anything is enqueued
        res = _c_profile(ops, z, z, w, thr, one, prec, "all", workspace=False)
        assert res[0] == -2 and b"workspace" in err() and untouched(res)
    res = _c_profile(ops, z, z, w, thr, one, "f32", "all")          # the same call, well-formed, does write
    assert res[0] == 0 and not untouched(res)
    # the wrapper
    with pytest.raises(ValueError, match="NaN"):
        ops.bilinear_profile(z, z, w, nan_thr)
    with pytest.raises(ValueError, match="scale"):
        ops.bilinear_profile(z, z, w, thr, scale=torch.tensor([1.0, 0.0], device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_profile(z.cpu(), z.cpu(), w.cpu(), thr.cpu())
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_profile(z, z[:4], w, thr, eligible="lower")
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_profile(z, z, w, thr, out=(torch.empty(6, 6, device="cuda"),) * 3)
    # no outcome: the ineligible values everywhere; no row or column: empty results
    c, b, m = ops.bilinear_profile(z, z, w[:0], thr[:0])
    assert bool((c == 0).all()) and bool((b == -1).all()) and bool((m == -INF).all()) and c.shape == (6, 6)
    assert ops.bilinear_profile(z[:0], z, w, thr)[0].shape == (0, 6) and ops.bilinear_profile(z, z[:0], w, thr)[2].shape == (6, 0)


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def small_model():
    """A configs.build_model model (drugbank163 layout, 6 outcomes) and the embeddings of 300 drugs from generate_embeddings (the
    recipe of tests/test_select_gpu.py)."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n, n_out = 300, 6
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    torch.manual_seed(3)
    model = configs.build_model("drugbank163", bkg["data"], n_out).cuda().eval()
    filler = torch.randn((n, 128), generator=torch.Generator().manual_seed(6)).cuda()
    with M.precision("bf16x3"):
        z = generate_embeddings(model, b, kgc, kg_filler=filler).contiguous()
    assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
    return model, z


def _same64(got, ref, offset=0):
    """A pipeline triple (best int64, model outcome indices) against a reference triple (best int32, relative to ``offset``)."""
    rb = ref[1].long()
    rb = torch.where(rb >= 0, rb + offset, rb)
    return got[1].dtype == torch.int64 and same(got, (ref[0], rb, ref[2]))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_pipeline_products_on_a_built_model(small_model, prec):
    """outcome_profile over a label range, and over two merged chunks, equals the reference on score_all_pairs' general sweep; the
    head_rows blocks concatenate to the full result; most_flagged_pairs over several row blocks equals the sort of the dense
    profile by (count descending, margin descending, i, j)."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import most_flagged_pairs, outcome_profile, score_all_pairs
    model, z = small_model
    N, n_out = z.shape[0], 6
    with M.precision(prec), torch.no_grad():
        dense = torch.cat([score_all_pairs(model, z, head_rows=(0, 150)), score_all_pairs(model, z, head_rows=(150, N))], 1)    # the general sweep
        thr = torch.quantile(dense.reshape(n_out, -1), 0.9, dim=1).contiguous()
        scale = torch.tensor([1.0, 2.5, 0.5, 1.25, 3.0, 0.75], device="cuda")
        for eligible in ("not_self", "lower", "all"):
            ref = dense_profile(dense, thr, scale, eligible)
            assert _same64(outcome_profile(model, z, thr, scale, eligible=eligible), ref), eligible
            assert _same64(outcome_profile(model, z, thr, scale, eligible=eligible, chunk=3), ref), eligible          # two chunks, merged
            assert _same64(outcome_profile(model, z, thr, scale, eligible=eligible, chunk=1), ref), eligible          # six
            part = outcome_profile(model, z, thr[1:5], scale[1:5], label_range=(1, 5), eligible=eligible)
            assert _same64(part, dense_profile(dense[1:5], thr[1:5], scale[1:5], eligible), offset=1), eligible
            blocks = [outcome_profile(model, z, thr, scale, eligible=eligible, head_rows=hr) for hr in ((0, 100), (100, 100), (100, N))]
            assert blocks[1][0].shape == (0, N)
            assert _same64(tuple(torch.cat([b[k] for b in blocks], 0) for k in range(3)), ref), eligible
        one = outcome_profile(model, z, float(thr.max()))                      # one number for every outcome, no scale
        assert _same64(one, dense_profile(dense, thr.max().expand(n_out).contiguous(), None, "not_self"))
        # most_flagged_pairs: K = 50 over blocks of 70 rows
        K = 50
        count, best, margin = dense_profile(dense, thr, scale, "lower")
        i, j = torch.tril_indices(N, N, -1, device="cuda")                      # ascending (i, j)
        c, b, m = count[i, j], best[i, j].long(), margin[i, j]
        order = torch.arange(i.numel(), device="cuda")
        order = order[torch.sort(m[order].double(), descending=True, stable=True).indices]
        order = order[torch.sort(c[order], descending=True, stable=True).indices][:K]
        got = most_flagged_pairs(model, z, thr, K, scale=scale, max_bytes=48 * N * 70)
        assert [t.shape for t in got] == [(K,)] * 5 and got[1].dtype == torch.int64
        assert torch.equal(got[0], c[order]) and torch.equal(got[1], i[order]) and torch.equal(got[2], j[order])
        assert torch.equal(got[3], b[order]) and torch.equal(got[4].view(torch.int32), m[order].view(torch.int32))
        assert bool((got[1] > got[2]).all()) and int(got[0][0]) >= int(got[0][-1]) >= 1
        whole = most_flagged_pairs(model, z, thr, K, scale=scale)              # one block
        assert all(torch.equal(a, b) for a, b in zip(whole[:4], got[:4])) and torch.equal(whole[4], got[4])
        few = most_flagged_pairs(model, z[:4].contiguous(), thr, 10, scale=scale)          # K > N (N - 1) / 2 = 6: padded
        assert few[1][6:].tolist() == [-1] * 4 and few[0][6:].tolist() == [0] * 4 and bool((few[4][6:] == -INF).all()) and bool((few[1][:6] >= 0).all())
    with pytest.raises(ValueError):
        outcome_profile(model, z, thr[:4])
    with pytest.raises(ValueError):
        outcome_profile(model, z, thr, label_range=(0, 7))
    with pytest.raises(ValueError):
        most_flagged_pairs(model, z, thr, 0)
