"""Top-k screening of the all-pairs head on the GPU: mdg_bilinear_topk against the project's own dense head (exactly, in the
fp32-grade modes) and the CPU oracle, and the two pipeline products built on it (top_partners, top_pairs)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tolerance per arithmetic mode against the oracle: the table of tests/test_head_gpu.py
TOL = {"f32": 2e-5, "bf16x3": 1e-4, "bf16": 3e-2, "f16": 4e-3}
NEG = float("-inf")
SHAPES = [(1, 1), (33, 4), (300, 333), (513, 64), (1100, 130), (700, 700), (2049, 2049)]


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _inputs(nh, nt, L, seed=0):
    """Head / tail embeddings with exact ties: tail rows 5 and 9 (and a late one) are copies of row 3.  nh == nt is ONE drug set
    (z_tail is a separate copy of z_head: with one tensor object the dense head would take the symmetric sweep, whose mirrored
    tiles hold the other association order and are not bit-equal to the general sweep)."""
    w = _rand((L, 128, 128), seed + 3, 1 / np.sqrt(128))
    zt = _rand((nt, 128), seed + 2)
    for dup in (5, 9, nt - 2):
        if 3 < dup < nt:
            zt[dup] = zt[3]
    zh = zt.clone() if nh == nt else _rand((nh, 128), seed + 1)
    return zh, zt, w


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if nh == nt else ["all"]


def _mask(dense, eligible):
    """dense [L,Nh,Nt] with the ineligible columns set to -inf."""
    d = dense.clone()
    nh, nt = d.shape[1:]
    i = torch.arange(nh, device=d.device)[:, None]
    j = torch.arange(nt, device=d.device)[None, :]
    if eligible == "not_self":
        d[:, i == j] = NEG
    elif eligible == "lower":
        d[:, j >= i] = NEG
    return d


def _ref_topk(dense, eligible, k):
    """The first k of the reference order: stable descending sort (ties by ascending column) of the eligible scores,
    padded with -inf / -1."""
    sv, si = torch.sort(_mask(dense, eligible), dim=2, descending=True, stable=True)
    sv, si = sv[..., :k], si[..., :k]
    if sv.shape[2] < k:
        pad = k - sv.shape[2]
        sv = torch.cat([sv, sv.new_full(sv.shape[:2] + (pad,), NEG)], 2)
        si = torch.cat([si, si.new_full(si.shape[:2] + (pad,), -1)], 2)
    si = torch.where(sv == NEG, torch.full_like(si, -1), si)
    return sv, si.to(torch.int32)


def _take(dense, idx):
    """dense[l, i, idx[l, i, :]] with -inf where idx is the padding value."""
    got = torch.gather(dense, 2, idx.clamp(min=0).long())
    return torch.where(idx < 0, torch.full_like(got, NEG), got)


def _check_16bit_rule(vals, idx, dense, eligible, k, bound):
    """idx may differ from the dense order only where the dense scores of the swapped entries are within ``bound``; vals agree
    with the dense order within ``bound``; the entries are eligible and distinct."""
    rv, ri = _ref_topk(dense, eligible, k)
    pad = ri < 0
    assert torch.equal(idx < 0, pad)
    assert bool((vals[pad] == NEG).all())
    dv = torch.where(pad, torch.zeros_like(vals), (vals - rv).abs())
    print("16-bit rule: max |vals - dense order|", float(dv.max()), "bound", bound)
    assert float(dv.max()) < bound
    mine = _take(_mask(dense, eligible), idx)                 # -inf here = an ineligible column was returned
    assert bool(torch.isfinite(mine[~pad]).all())
    ds = torch.where(pad, torch.zeros_like(mine), (mine - rv).abs())
    print("16-bit rule: max |dense[idx] - dense order|", float(ds.max()))
    assert float(ds.max()) < bound
    srt = torch.sort(idx, dim=2).values
    assert bool(((srt[..., 1:] != srt[..., :-1]) | (srt[..., 1:] < 0)).all())


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_topk_equals_the_dense_general_sweep(ops, prec, nh, nt, L):
    """vals and idx are EQUAL to the first k of the stable descending order of the STORE tensor of the general sweep in the same
    precision: same products, same order, every k, every eligibility mode, ties and padded rows included."""
    zh, zt, w = _inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    max_k = ops.bilinear_topk_max_k()
    for eligible in _modes(nh, nt):
        for k in sorted({1, 5, 16, 32, max_k}):
            vals, idx = ops.bilinear_topk(zh, zt, ws, k, eligible=eligible, precision=prec)
            rv, ri = _ref_topk(dense, eligible, k)
            assert vals.shape == (L, nh, k) and idx.shape == (L, nh, k) and idx.dtype == torch.int32
            assert torch.equal(idx, ri), (eligible, k)
            assert torch.equal(vals, rv), (eligible, k)


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_topk_16bit_modes_against_the_dense_general_sweep(ops, prec, nh, nt, L):
    """The single-product modes run the row-statistics sweep (16x16x32: fp32 sums grouped differently from the dense 32x32x16
    sweep), so the order may differ from the dense one where two dense scores are within 2e-6 of the scale."""
    zh, zt, w = _inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    bound = 2e-6 * float(dense.abs().max())
    max_k = ops.bilinear_topk_max_k()
    for eligible in _modes(nh, nt):
        for k in sorted({1, 5, 16, 32, max_k}):
            vals, idx = ops.bilinear_topk(zh, zt, ws, k, eligible=eligible, precision=prec)
            _check_16bit_rule(vals, idx, dense, eligible, k, bound)


def _check_oracle_rule(vals, idx, ref, eligible, k, tol):
    """|vals - ref[l, i, idx]| < tol and the k-th kept value is not below the k-th largest eligible oracle score - tol."""
    pad = idx < 0
    rv, ri = _ref_topk(ref, eligible, k)
    assert torch.equal(pad, ri < 0)
    mine = _take(_mask(ref, eligible), idx)
    assert bool(torch.isfinite(mine[~pad]).all())
    err = torch.where(pad, torch.zeros_like(vals), (vals - mine).abs())
    print("oracle rule: max |vals - ref[idx]|", float(err.max()), "tol", tol)
    assert float(err.max()) < tol
    full = ~pad[..., k - 1]
    short = (vals[..., k - 1] - (rv[..., k - 1] - tol))[full]
    assert bool((short >= 0).all())


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "f16"])
def test_topk_against_the_oracle(ops, prec, nh, nt, L):
    from oracle import madrigal_oracle as O
    zh, zt, w = _inputs(nh, nt, L)
    ref = O.bilinear_scores(zh, zt, w)
    tol = TOL[prec] * max(float(ref.abs().max()), 128 ** 0.5)
    zhc, ztc, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    max_k = ops.bilinear_topk_max_k()
    for eligible in _modes(nh, nt):
        for k in sorted({1, 5, 16, 32, max_k}):
            vals, idx = ops.bilinear_topk(zhc, ztc, ws, k, eligible=eligible, precision=prec)
            _check_oracle_rule(vals.cpu(), idx.cpu(), ref, eligible, k, tol)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("nh,nt", [(300, 333), (1, 1), (513, 64), (1100, 130)])
def test_top1_is_the_rowstats_maximum(ops, prec, nh, nt):
    zh, zt, w = _inputs(nh, nt, 4, seed=10)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    st = ops.bilinear_allpairs(zh, zt, ws, precision=prec, epilogue=ops.EPI_ROWSTATS)
    vals, _ = ops.bilinear_topk(zh, zt, ws, 1, precision=prec)
    assert torch.equal(vals[..., 0], st[..., 1])


@pytest.mark.parametrize("prec", ["bf16x3", "f32", "f16", "bf16"])
@pytest.mark.parametrize("nh,nt,L,eligible", [(4096, 4096, 8, "not_self"), (1000, 3001, 7, "all"), (3000, 3000, 5, "lower")])
def test_repeated_topk_launches_are_bit_identical(ops, prec, nh, nt, L, eligible):
    zh, zt, w = _inputs(nh, nt, L, seed=40)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    first = None
    for it in range(5):
        vals = torch.full((L, nh, 16), float("nan"), device="cuda")
        idx = torch.full((L, nh, 16), -7, dtype=torch.int32, device="cuda")
        ops.bilinear_topk(zh, zt, ws, 16, eligible=eligible, precision=prec, out=(vals, idx))
        assert not bool(torch.isnan(vals).any()) and not bool((idx == -7).any())
        if first is None:
            first = (vals, idx)
        else:
            assert torch.equal(vals, first[0]) and torch.equal(idx, first[1]), f"launch {it} differs from launch 0"


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_cfg5_scale_top_partners_of_every_drug(ops, prec):
    """BASELINE configs[4] (100 352 drugs, 16-bit head): the 16 strongest partners of every drug for a few outcomes.  Every
    row: finite, ordered, indices in range, distinct and not the drug itself; the 96 head rows 70 001 .. 70 096 (ragged against
    the 512-row workgroups) against the dense general sweep of those rows and against the oracle."""
    from oracle import madrigal_oracle as O
    N, L, k = 100_352, 3, 16
    z = _rand((N, 128), 50)
    w = _rand((L, 128, 128), 51, 1 / np.sqrt(128))
    zc, wc = z.cuda(), ops.symmetrize(w.cuda())
    vals, idx = ops.bilinear_topk(zc, zc, wc, k, eligible="not_self", precision=prec)
    assert vals.shape == (L, N, k) and bool(torch.isfinite(vals).all())
    assert bool((vals[..., 1:] <= vals[..., :-1]).all())
    assert bool(((idx >= 0) & (idx < N)).all())
    assert bool((idx != torch.arange(N, device="cuda", dtype=torch.int32)[None, :, None]).all())
    srt = torch.sort(idx, dim=2).values
    assert bool((srt[..., 1:] != srt[..., :-1]).all())
    rows = torch.arange(70_001, 70_097)
    dense = ops.bilinear_allpairs(zc[rows.cuda()], zc, wc, precision=prec)          # general sweep: [L, 96, N]
    dense[:, torch.arange(96), rows] = NEG                                          # the drug itself
    bound = 2e-6 * float(dense[torch.isfinite(dense)].abs().max())
    _check_16bit_rule(vals[:, rows.cuda()], idx[:, rows.cuda()], dense, "all", k, bound)
    ref = O.bilinear_scores(z[rows], z, w)
    tol = TOL[prec] * max(float(ref.abs().max()), 128 ** 0.5)
    ref[:, torch.arange(96), rows] = NEG
    _check_oracle_rule(vals[:, rows.cuda()].cpu(), idx[:, rows.cuda()].cpu(), ref, "all", k, tol)


def test_topk_empty_and_errors(ops):
    z = _rand((6, 128), 0).cuda()
    w = _rand((2, 128, 128), 1).cuda()
    max_k = ops.bilinear_topk_max_k()
    assert max_k >= 32
    v, i = ops.bilinear_topk(z[:0], z, w, 3)
    assert v.shape == (2, 0, 3) and i.shape == (2, 0, 3) and i.dtype == torch.int32
    v, i = ops.bilinear_topk(z, z, w[:0], 3)
    assert v.shape == (0, 6, 3)
    v, i = ops.bilinear_topk(z, z[:0], w, 3)
    assert v.shape == (2, 6, 3) and bool((v == NEG).all()) and bool((i == -1).all())
    for bad_k in (0, max_k + 1, -1, 2.0):
        with pytest.raises(ValueError):
            ops.bilinear_topk(z, z, w, bad_k)
    with pytest.raises(ValueError):
        ops.bilinear_topk(z, z[:4], w, 2, eligible="lower")
    with pytest.raises(ValueError):
        ops.bilinear_topk(z, z[:4], w, 2, eligible="not_self")
    with pytest.raises(ValueError):
        ops.bilinear_topk(z, z, w, 2, eligible="upper")
    with pytest.raises(ValueError):
        ops.bilinear_topk(z, z, w, 2, precision="fp8")
    with pytest.raises(ValueError):
        ops.bilinear_topk(z.cpu(), z, w, 2)
    with pytest.raises(ValueError):
        ops.bilinear_topk(z[:, :64], z, w, 2)
    # the C ABI refuses the same on its own
    import ctypes
    from madrigal_amd._lib import lib
    vals = torch.empty(2, 6, 40, device="cuda")
    idx = torch.empty(2, 6, 40, dtype=torch.int32, device="cuda")
    args = lambda k, nt, el: (ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(w.data_ptr()),
                              ctypes.c_void_p(vals.data_ptr()), ctypes.c_void_p(idx.data_ptr()), ctypes.c_int64(6), ctypes.c_int64(nt),
                              ctypes.c_int64(2), ctypes.c_int64(128), 0, k, el, None, ctypes.c_size_t(0), None)
    for k, nt, el in ((0, 6, 0), (max_k + 1, 6, 0), (2, 4, 2), (2, 6, 5), (2, 2 ** 31, 0)):
        assert lib().mdg_bilinear_topk(*args(k, nt, el)) == -1
        assert b"mdg_bilinear_topk" in lib().mdg_last_error()


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def small_model():
    """A configs.build_model model (drugbank163 layout, 6 outcomes) and the embeddings of 513 drugs from generate_embeddings."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n, L = 513, 6
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    torch.manual_seed(3)
    model = configs.build_model("drugbank163", bkg["data"], L).cuda().eval()
    with M.precision("bf16x3"):
        z = generate_embeddings(model, b, kgc, kg_filler=_rand((n, 128), 6).cuda()).contiguous()
    assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
    return model, z


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_top_partners_equals_the_kernel_level_reference(small_model, prec):
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import top_partners
    model, z = small_model
    N = z.shape[0]
    with M.precision(prec):
        dense = _general_dense(model, z)
        for k in (1, 8, 32):
            vals, idx = top_partners(model, z, k)
            rv, ri = _ref_topk(dense, "not_self", k)
            assert torch.equal(vals, rv) and torch.equal(idx, ri)
        vals, idx = top_partners(model, z, 8, label_range=(2, 5))
        rv, ri = _ref_topk(dense[2:5], "not_self", 8)
        assert torch.equal(vals, rv) and torch.equal(idx, ri)
        rows = [512, 0, 77, 256, 77]
        for budget in (1 << 30, 1):                                   # one chunk; one outcome per chunk
            vals, idx = top_partners(model, z, 8, label_range=(1, 6), drug_rows=rows, max_temp_bytes=budget)
            rv, ri = _ref_topk(dense[1:6], "not_self", 8)
            assert vals.shape == (5, 5, 8) and torch.equal(vals, rv[:, rows]) and torch.equal(idx, ri[:, rows])
        v2, i2 = model.decoder.topk(z, z, 16)
        rv, ri = _ref_topk(dense, "all", 16)
        assert torch.equal(v2, rv) and torch.equal(i2, ri)
    with pytest.raises(ValueError):
        top_partners(model, z, 8, drug_rows=[N])
    with pytest.raises(ValueError):
        top_partners(model, z, 8, label_range=(0, 7))


def _general_dense(model, z):
    """Dense scores [L,N,N] of the GENERAL sweep.  (score_all_pairs(model, z, head_rows=(0, N)) hands the decoder the view
    z[0:N], which is the same memory as z, so the head recognises one drug set and takes the symmetric sweep; a separate copy
    of z as the head operand is what selects the general one.)"""
    with torch.no_grad():
        return model.decoder(z.clone(), z)


def _dense_lower_pairs(model, z, K):
    """Brute force: stable descending sort of the strict lower triangle (row-major) of the general sweep's scores."""
    from test_topk_cpu import brute_force_pairs
    dense = _general_dense(model, z).cpu()
    return dense, brute_force_pairs(dense, K)


def _pair_inputs(N, hubs):
    from test_topk_cpu import pair_case
    z, _ = pair_case(N, hubs)
    return z.cuda()


from test_topk_cpu import PAIR_CASES  # noqa: E402


@pytest.mark.parametrize("N,K,k_row,hubs", PAIR_CASES)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_top_pairs_equals_brute_force_over_the_dense_scores(small_model, prec, N, K, k_row, hubs):
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import top_pairs
    model, _ = small_model
    z = _pair_inputs(N, hubs)
    with M.precision(prec):
        info = {}
        v, h, t = top_pairs(model, z, K, k_row=k_row, info=info)
        dense, (bv, bh, bt) = _dense_lower_pairs(model, z, K)
        assert torch.equal(h.cpu(), bh) and torch.equal(t.cpu(), bt) and torch.equal(v.cpu(), bv)
        if hubs:
            assert min(info["open_rows"]) >= 1, info
        # an outcome shard, one outcome per chunk
        v2, h2, t2 = top_pairs(model, z, K, label_range=(1, 4), k_row=k_row, max_temp_bytes=1)
        assert torch.equal(v2, v[1:4]) and torch.equal(h2, h[1:4]) and torch.equal(t2, t[1:4])


@pytest.mark.parametrize("N,K,k_row,hubs", PAIR_CASES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_top_pairs_16bit_modes(small_model, monkeypatch, prec, N, K, k_row, hubs):
    """The list sweep and the dense sweep group their fp32 sums differently in the single-product modes: pairs may differ from
    the brute-force order only where their dense scores are within 2e-6 of the scale, values agree within the same bound."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import top_pairs
    model, _ = small_model
    z = _pair_inputs(N, hubs)
    monkeypatch.setitem(M._state, "precision", prec)          # (the head runs "f16"; set_precision covers the whole-model modes only)
    info = {}
    v, h, t = top_pairs(model, z, K, k_row=k_row, info=info)
    dense, (bv, bh, bt) = _dense_lower_pairs(model, z, K)
    v, h, t = v.cpu(), h.cpu(), t.cpu()
    bound = 2e-6 * float(dense.abs().max())
    pad = bh < 0
    assert torch.equal(h < 0, pad) and torch.equal(t < 0, pad) and bool((v[pad] == NEG).all())
    assert bool((h > t)[~pad].all())
    dv = torch.where(pad, torch.zeros_like(v), (v - bv).abs())
    mine = dense[torch.arange(dense.shape[0])[:, None], h.clamp(min=0), t.clamp(min=0)]
    ds = torch.where(pad, torch.zeros_like(v), (mine - bv).abs())
    print("top_pairs 16-bit:", float(dv.max()), float(ds.max()), "bound", bound, "open rows", info["open_rows"])
    assert float(dv.max()) < bound and float(ds.max()) < bound
    key = torch.where(pad, -torch.arange(1, K + 1)[None, :].expand_as(h), h * N + t)
    srt = torch.sort(key, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    if hubs:
        assert min(info["open_rows"]) >= 1, info


def test_top_pairs_makes_no_dense_score_tensor():
    """N = 4096, L = 64, K = 1000: the peak allocation during top_pairs stays below one outcome's N^2 * 4 bytes plus the stated
    temporary budget."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import top_pairs, top_partners
    N, L, K, budget = 4096, 64, 1000, 256 << 20
    model = _DecoderOnly(M, L, 0).cuda().eval()
    z = _rand((N, 128), 1).cuda()
    with M.precision("bf16x3"):
        top_pairs(model, z, 10, label_range=(0, 1))               # scratch buffers of the library wrappers exist before measuring
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        v, h, t = top_pairs(model, z, K, max_temp_bytes=budget)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        print("top_pairs peak bytes", peak, "limit", N * N * 4 + budget)
        assert peak < N * N * 4 + budget
        assert v.shape == (L, K) and bool(torch.isfinite(v).all()) and bool((h > t).all())
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        vals, idx = top_partners(model, z, 16)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < L * N * 16 * 8 + N * N * 4                  # the result itself and nothing of the size of a score slab


class _DecoderOnly(torch.nn.Module):
    """Decoder-only stand-in for NovelDDIMultilabel: the screening functions read ``model.decoder`` only."""

    def __init__(self, M, L, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, L)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)
