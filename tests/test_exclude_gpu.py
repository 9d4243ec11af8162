"""Known-pair exclusion masks inside the all-pairs sweep, on the GPU: the mask builder against a numpy packing of the documented
layout; masked top-k and masked selection against the project's own dense general sweep with the ineligible AND the excluded entries
taken out (exactly in the fp32-grade modes, within the regrouping bound in the 16-bit modes); masked selection against unmasked
selection filtered by pair key; determinism; refusals; and the pipeline products (top_partners, top_pairs, pairs_above,
partners_above, partner_counts) with ``exclude=``.

Every mask pattern is built so that it alone stands between the kernel and a wrong answer; every element of every result is
compared (a misplaced wait in the sweep gives stale tiles, not a fault)."""
import functools

import numpy as np
import pytest
import torch

from test_exclude_cpu import numpy_pack
from test_topk_cpu import brute_force_pairs

pytestmark = pytest.mark.gpu

NEG = float("-inf")
SHAPES = [(1, 1), (33, 4), (300, 333), (513, 64), (1100, 130), (700, 700), (2049, 2049)]
PATTERNS = ["empty", "random", "hub", "full_row", "band", "pad_and_diagonal", "ties"]


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _inputs(nh, nt, L, seed=0):
    """The inputs of tests/test_topk_gpu.py: tail rows 5, 9 and nt - 2 are copies of row 3 (exact ties); nh == nt is ONE drug set
    (z_tail a separate copy of z_head, so that the dense head takes the general sweep)."""
    w = _rand((L, 128, 128), seed + 3, 1 / np.sqrt(128))
    zt = _rand((nt, 128), seed + 2)
    for dup in (5, 9, nt - 2):
        if 3 < dup < nt:
            zt[dup] = zt[3]
    zh = zt.clone() if nh == nt else _rand((nh, 128), seed + 1)
    return zh, zt, w


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if nh == nt else ["all"]


@functools.lru_cache(maxsize=4)
def _case(prec, nh, nt, L):
    """(zh, zt, ws, dense) on the GPU: computed once per precision and shape, shared by the tests and never modified."""
    from madrigal_amd import ops
    zh, zt, w = _inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    return zh, zt, ws, ops.bilinear_allpairs(zh, zt, ws, precision=prec)


def _eligible(nh, nt, mode):
    i = torch.arange(nh, device="cuda")[:, None]
    j = torch.arange(nt, device="cuda")[None, :]
    if mode == "not_self":
        return i != j
    if mode == "lower":
        return j < i
    return torch.ones((nh, nt), dtype=torch.bool, device="cuda")


def _pack(excl, extra_pad_bits=False):
    """The documented layout on the GPU, independent of the code under test: bool [P, nh, nt] -> int32 [P, ceil(nh/32), ld];
    word [p][i >> 5][j], bit i & 31.  ``extra_pad_bits``: every bit of the pad columns [nt, ld) and of the pad rows is set too."""
    P, nh, nt = excl.shape
    nrb, ld = (nh + 31) // 32, (nt + 63) // 64 * 64
    full = torch.full((P, nrb * 32, ld), bool(extra_pad_bits), dtype=torch.bool, device=excl.device)
    full[:, :nh, :nt] = excl
    full = full.view(P, nrb, 32, ld)
    words = torch.zeros((P, nrb, ld), dtype=torch.int64, device=excl.device)
    for b in range(32):
        words |= full[:, :, b, :].to(torch.int64) << b
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def _pattern(name, nh, nt, P, mode):
    """bool [P, nh, nt] on the GPU (planes differ from each other where the pattern allows it)."""
    g = torch.Generator().manual_seed(PATTERNS.index(name) * 7919 + nh * 31 + nt * 17 + P)
    ex = torch.zeros((P, nh, nt), dtype=torch.bool)
    elig = _eligible(nh, nt, mode).cpu()
    for p in range(P):
        if name == "random":
            ex[p] = torch.rand((nh, nt), generator=g) < 0.5
        elif name == "hub":
            # a row with all but 3 of its eligible columns excluded: k > what is left, the list ends in padding
            row = nh - 1 - p if nh > p else nh - 1
            cols = elig[row].nonzero()[:, 0]
            keep = cols[torch.randperm(cols.numel(), generator=g)[:3]]
            ex[p, row] = True
            ex[p, row, keep] = False
        elif name == "full_row":
            ex[p, (nh // 2 + 37 * p) % nh] = True
        elif name == "band":
            c0 = 64 * ((p + 1) % max(1, nt // 64)) if nt >= 128 else 0          # one whole 64-column tile
            ex[p, :, c0:c0 + 64] = True
        elif name == "pad_and_diagonal":
            if mode != "all":                                                   # the diagonal is ineligible there already
                ex[p] = torch.eye(nh, nt, dtype=torch.bool)
        elif name == "ties":
            for c in (5, nt - 2) if p % 2 == 0 else (3, 9):                     # some of the tied duplicate columns, not all
                if 3 < c < nt or c == 3 < nt:
                    ex[p, :, c] = True
    return ex.cuda()


@functools.lru_cache(maxsize=None)
def _mask_of(name, nh, nt, P, mode):
    ex = _pattern(name, nh, nt, P, mode)
    return ex, _pack(ex, extra_pad_bits=(name == "pad_and_diagonal"))


def _ref_topk(masked, k):
    sv, si = torch.sort(masked, dim=2, descending=True, stable=True)
    sv, si = sv[..., :k], si[..., :k]
    if sv.shape[2] < k:
        pad = k - sv.shape[2]
        sv = torch.cat([sv, sv.new_full(sv.shape[:2] + (pad,), NEG)], 2)
        si = torch.cat([si, si.new_full(si.shape[:2] + (pad,), -1)], 2)
    si = torch.where(sv == NEG, torch.full_like(si, -1), si)
    return sv, si.to(torch.int32)


def _take(dense, idx):
    got = torch.gather(dense, 2, idx.clamp(min=0).long())
    return torch.where(idx < 0, torch.full_like(got, NEG), got)


def _check_16bit_rule(vals, idx, masked, k, bound):
    """The 16-bit rule of tests/test_topk_gpu.py on dense scores whose ineligible and excluded entries are -inf: idx may differ from
    the dense order only where the dense scores of the swapped entries are within ``bound``; vals agree with the dense order within
    ``bound``; the entries are eligible, not excluded, and distinct."""
    rv, ri = _ref_topk(masked, k)
    pad = ri < 0
    assert torch.equal(idx < 0, pad)
    assert bool((vals[pad] == NEG).all())
    dv = torch.where(pad, torch.zeros_like(vals), (vals - rv).abs())
    assert float(dv.max()) < bound, (float(dv.max()), bound)
    mine = _take(masked, idx)                                  # -inf here = an ineligible or excluded column was returned
    assert bool(torch.isfinite(mine[~pad]).all())
    ds = torch.where(pad, torch.zeros_like(mine), (mine - rv).abs())
    assert float(ds.max()) < bound, (float(ds.max()), bound)
    srt = torch.sort(idx, dim=2).values
    assert bool(((srt[..., 1:] != srt[..., :-1]) | (srt[..., 1:] < 0)).all())


# ------------------------------------------------------------------------------------------------ builder
@pytest.mark.parametrize("nh,nt", SHAPES)
def test_pair_mask_equals_the_numpy_packing(ops, nh, nt):
    """ops.pair_mask == the numpy packing of the documented layout: lists with duplicates, both ``symmetric`` settings, one plane
    and one plane per outcome."""
    rng = np.random.default_rng(nh + nt)
    n = min(5000, 4 * nh * nt)
    h, t = rng.integers(0, nh, n), rng.integers(0, nt, n)
    h, t = np.concatenate([h, h[: n // 3], [nh - 1]]), np.concatenate([t, t[: n // 3], [nt - 1]])       # duplicates; the last bit
    for L in (1, 4):
        lab = rng.integers(0, L, h.size)
        for symmetric in ([False, True] if nh == nt else [False]):
            want = np.zeros((L, nh, nt), dtype=bool)
            want[lab, h, t] = True
            if symmetric:
                want[lab, t, h] = True
            got = ops.pair_mask(h, t, nh, nt, labels=lab, n_labels=L, symmetric=symmetric)
            assert got.dtype == torch.int32 and got.is_cuda and got.shape == (L, (nh + 31) // 32, (nt + 63) // 64 * 64)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), numpy_pack(want))
            assert torch.equal(ops.pair_mask_dense(got, nh, nt).cpu(), torch.from_numpy(want))
            shared = ops.pair_mask(torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda(), nh, nt, symmetric=symmetric)
            assert shared.shape[0] == 1
            assert np.array_equal(shared.cpu().numpy().view(np.uint32), numpy_pack(want.any(0, keepdims=True)))
            assert torch.equal(_pack(torch.from_numpy(want).cuda()), got)                    # the GPU packing the tests below use
    if nh == nt:
        assert torch.equal(ops.pair_mask(h, t, nh), ops.pair_mask(h, t, nh, nt))
    empty = ops.pair_mask([], [], nh, nt)
    assert empty.shape[0] == 1 and not bool(empty.any())


def test_pair_mask_refusals(ops):
    with pytest.raises(ValueError, match="symmetric"):
        ops.pair_mask([0], [1], 5, 7, symmetric=True)
    for h, t, kw in (([5], [0], {}), ([0], [7], {}), ([-1], [0], {}), ([0, 1], [0], {}), ([0], [0], {"labels": [2], "n_labels": 2}),
                     ([0], [0], {"labels": [0]}), ([0], [0], {"n_labels": 2}), ([0.5], [0], {})):
        with pytest.raises(ValueError):
            ops.pair_mask(h, t, 5, 7, **kw)
    # the kernel itself skips what lies outside the mask: the guard words around it stay zero
    from madrigal_amd._lib import call, lib
    words = lib().mdg_pair_mask_plane_words(5, 7)
    buf = torch.zeros(words + 128, dtype=torch.int32, device="cuda")
    h = torch.tensor([0, 5, -1, 4, 2, 1 << 40], device="cuda")
    t = torch.tensor([0, 0, 0, 7, -3, 1], device="cuda")
    pl = torch.tensor([0, 0, 0, 0, 0, 0], device="cuda")
    call("mdg_pair_mask_set", buf.data_ptr() + 64 * 4, 1, 5, 7, h.data_ptr(), t.data_ptr(), pl.data_ptr(), 6, 0, None)
    torch.cuda.synchronize()
    assert int(buf[64]) == 1 and int(buf.count_nonzero()) == 1


# ------------------------------------------------------------------------------------------------ top-k
def _topk_cases(nh, nt, L):
    for mode in _modes(nh, nt):
        elig = _eligible(nh, nt, mode)
        for P in sorted({1, L}):
            for name in PATTERNS:
                ex, mask = _mask_of(name, nh, nt, P, mode)
                yield mode, elig, P, name, ex, mask


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_masked_topk_equals_the_dense_general_sweep(ops, prec, nh, nt, L):
    """vals and idx are EQUAL to the stable descending sort of the dense general sweep with the ineligible and the excluded entries
    at -inf, for k in {1, 16, 32}, every eligible mode, shared and per-outcome planes, every mask pattern."""
    zh, zt, ws, dense = _case(prec, nh, nt, L)
    plain = {}
    for mode, elig, P, name, ex, mask in _topk_cases(nh, nt, L):
        masked = dense.masked_fill(~elig[None] | ex, NEG)
        rv32, ri32 = _ref_topk(masked, 32)
        for k in (1, 16, 32):
            what = (mode, P, name, k)
            vals, idx = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec, exclude=mask)
            assert vals.shape == (L, nh, k) and idx.shape == (L, nh, k) and idx.dtype == torch.int32
            assert torch.equal(idx, ri32[..., :k].contiguous()), what
            assert torch.equal(vals, rv32[..., :k].contiguous()), what
            if name in ("empty", "pad_and_diagonal"):                      # no pair excluded: the unmasked call, bit for bit
                if (mode, k) not in plain:
                    plain[mode, k] = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec)
                assert torch.equal(vals, plain[mode, k][0]) and torch.equal(idx, plain[mode, k][1]), what
            if name == "random" and k == 16:                               # a second launch is bit-identical
                v2, i2 = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec, exclude=mask)
                assert torch.equal(v2, vals) and torch.equal(i2, idx), what
            if name == "hub" and k == 16:                                  # the hub rows really end in padding: 3 entries, 13 pads
                for p in range(P):
                    row = nh - 1 - p if nh > p else nh - 1
                    n_left = int((elig[row] & ~ex[p, row]).sum())
                    sel = slice(None) if P == 1 else p
                    assert bool(((idx[sel, row] >= 0).sum(-1) == min(n_left, k)).all()), what


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_masked_topk_16bit_modes(ops, prec, nh, nt, L):
    """The single-product modes run the 16x16x32 sweep, whose fp32 sums are grouped differently from the dense sweep's: the 16-bit
    rule of tests/test_topk_gpu.py with its bound (2e-6 of the scale), on the dense scores with the excluded entries at -inf.  With
    no pair excluded the result is the unmasked call's, bit for bit."""
    zh, zt, ws, dense = _case(prec, nh, nt, L)
    bound = 2e-6 * float(dense.abs().max())
    plain = {}
    for mode, elig, P, name, ex, mask in _topk_cases(nh, nt, L):
        masked = dense.masked_fill(~elig[None] | ex, NEG)
        for k in (1, 16, 32):
            what = (mode, P, name, k)
            vals, idx = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec, exclude=mask)
            _check_16bit_rule(vals, idx, masked, k, bound)
            if name in ("empty", "pad_and_diagonal"):
                if (mode, k) not in plain:
                    plain[mode, k] = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec)
                assert torch.equal(vals, plain[mode, k][0]) and torch.equal(idx, plain[mode, k][1]), what
            if name == "random" and k == 16:
                v2, i2 = ops.bilinear_topk(zh, zt, ws, k, eligible=mode, precision=prec, exclude=mask)
                assert torch.equal(v2, vals) and torch.equal(i2, idx), what


# ------------------------------------------------------------------------------------------------ select
def _cuts(dense, keep):
    """{name: thr [L]}: -inf, the median and the 99.9th percentile of the scores that remain (``keep`` [L or 1, nh, nt])."""
    L = dense.shape[0]
    out = {"ninf": torch.full((L,), NEG, device="cuda")}
    med, top = [], []
    for l in range(L):
        v = torch.sort(dense[l][keep[l if keep.shape[0] > 1 else 0]]).values
        M = v.numel()
        med.append(v[(M - 1) // 2] if M else dense.new_tensor(0.0))
        top.append(v[M - max(1, round(0.001 * M))] if M else dense.new_tensor(0.0))
    out["median"], out["p999"] = torch.stack(med).contiguous(), torch.stack(top).contiguous()
    return out


def _csr_of(sel, dense):
    """counts, row_ptr, cols, vals of the bool selection ``sel`` [L, nh, nt] in torch.nonzero order."""
    L, nh, _ = sel.shape
    counts = sel.sum(2).to(torch.int32)
    row_ptr = torch.zeros(L * nh + 1, dtype=torch.int64, device=sel.device)
    row_ptr[1:] = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    nz = torch.nonzero(sel)
    return counts, row_ptr, nz[:, 2].to(torch.int32), dense[nz[:, 0], nz[:, 1], nz[:, 2]]


def _rows_of(row_ptr, n_rows):
    return torch.repeat_interleave(torch.arange(n_rows, device=row_ptr.device), row_ptr[1:] - row_ptr[:-1])


def _bits(t):
    return t.view(torch.int32)


def _filtered(ops, zh, zt, ws, thr, mode, prec, ex):
    """Unmasked selection with the excluded entries filtered out by pair key -- no dense score tensor involved."""
    L, nh = ws.shape[0], zh.shape[0]
    rp, cols, vals = ops.bilinear_select(zh, zt, ws, thr, eligible=mode, precision=prec)
    rows = _rows_of(rp, L * nh)
    l, i = rows // nh, rows % nh
    keep = ~ex[l if ex.shape[0] > 1 else torch.zeros_like(l), i, cols.long()]
    counts = torch.zeros(L * nh, dtype=torch.int64, device="cuda").index_add_(0, rows[keep], torch.ones_like(rows[keep]))
    row_ptr = torch.zeros(L * nh + 1, dtype=torch.int64, device="cuda")
    row_ptr[1:] = torch.cumsum(counts, 0)
    return counts.view(L, nh).to(torch.int32), row_ptr, cols[keep], vals[keep]


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_masked_select_equals_nonzero_of_the_dense_general_sweep(ops, prec, nh, nt, L):
    """Counts, row_ptr and cols == torch.nonzero((dense >= thr) & eligible & ~excluded), vals bit-equal; the same result from the
    unmasked selection filtered by pair key; a second call identical."""
    zh, zt, ws, dense = _case(prec, nh, nt, L)
    for mode, elig, P, name, ex, mask in _topk_cases(nh, nt, L):
        keep = elig[None] & ~ex
        for cut, thr in _cuts(dense, keep).items():
            what = (mode, P, name, cut)
            rc, rp, rcol, rval = _csr_of((dense >= thr[:, None, None]) & keep, dense)
            counts = ops.bilinear_select_count(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
            assert counts.dtype == torch.int32 and torch.equal(counts, rc), what
            row_ptr, cols, vals = ops.bilinear_select(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
            assert torch.equal(row_ptr, rp) and torch.equal(cols, rcol) and torch.equal(_bits(vals), _bits(rval)), what
            fc, frp, fcols, fvals = _filtered(ops, zh, zt, ws, thr, mode, prec, ex)
            assert torch.equal(fc, counts) and torch.equal(frp, row_ptr) and torch.equal(fcols, cols), what
            assert torch.equal(_bits(fvals), _bits(vals)), what
            if name == "random" and cut == "median":
                again = ops.bilinear_select(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
                assert torch.equal(again[0], row_ptr) and torch.equal(again[1], cols) and torch.equal(_bits(again[2]), _bits(vals)), what
            if cut == "ninf":
                assert int(row_ptr[-1]) == int(keep.sum()) * (L if P == 1 else 1), what


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("nh,nt", SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_masked_select_16bit_modes(ops, prec, nh, nt, L):
    """The thr +- delta rule of tests/test_select_gpu.py (delta = 2e-6 max|dense|) on what the mask leaves: every remaining pair with
    dense >= thr + delta is selected, none with dense < thr - delta, nothing ineligible or excluded, values within delta; columns
    ascend within a row; and -- exactly, the arithmetic being the unmasked sweep's -- the unmasked selection filtered by pair key."""
    zh, zt, ws, dense = _case(prec, nh, nt, L)
    delta = 2e-6 * float(dense.abs().max())
    for mode, elig, P, name, ex, mask in _topk_cases(nh, nt, L):
        keep = elig[None] & ~ex
        for cut, thr in _cuts(dense, keep).items():
            what = (mode, P, name, cut)
            counts = ops.bilinear_select_count(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
            row_ptr, cols, vals = ops.bilinear_select(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
            rp = torch.zeros(L * nh + 1, dtype=torch.int64, device="cuda")
            rp[1:] = torch.cumsum(counts.reshape(-1), 0)
            assert torch.equal(rp, row_ptr) and cols.numel() == int(rp[-1]), what
            assert bool(((cols >= 0) & (cols < nt)).all()), what
            rows = _rows_of(row_ptr, L * nh)
            l, i = rows // nh, rows % nh
            got = torch.zeros(dense.shape, dtype=torch.bool, device="cuda")
            got[l, i, cols.long()] = True
            assert int(got.sum()) == cols.numel(), what                                  # no column twice in a row
            assert bool((cols[1:] > cols[:-1])[rows[1:] == rows[:-1]].all()), what
            must = (dense >= (thr + delta)[:, None, None]) & keep
            may = (dense >= (thr - delta)[:, None, None]) & keep
            assert not bool((got & ~keep).any()), what
            assert not bool((must & ~got).any()), what
            assert not bool((got & ~may).any()), what
            assert bool(((vals - dense[l, i, cols.long()]).abs() <= delta).all()), what
            fc, frp, fcols, fvals = _filtered(ops, zh, zt, ws, thr, mode, prec, ex)
            assert torch.equal(fc, counts) and torch.equal(frp, row_ptr) and torch.equal(fcols, cols), what
            assert torch.equal(_bits(fvals), _bits(vals)), what
            if name == "random" and cut == "median":
                again = ops.bilinear_select(zh, zt, ws, thr, eligible=mode, precision=prec, exclude=mask)
                assert torch.equal(again[0], row_ptr) and torch.equal(again[1], cols) and torch.equal(_bits(again[2]), _bits(vals)), what


def test_exclude_refusals_happen_before_any_launch(ops):
    """Wrong dtype, device, shape or number of planes -> ValueError, outputs untouched."""
    nh, nt, L = 70, 130, 3
    zh, zt, w = _inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    good = ops.pair_mask([1], [2], nh, nt)
    thr = torch.zeros(L, device="cuda")
    bad = {"dtype": good.long(), "float": good.float(), "device": good.cpu(), "columns": good[:, :, :64].contiguous(),
           "row blocks": good[:, :2].contiguous(), "dims": good[0], "planes": good.expand(2, -1, -1).contiguous(),
           "other shape": ops.pair_mask([1], [2], nt, nh), "not a tensor": [[0]]}
    for name, m in bad.items():
        vals = torch.full((L, nh, 4), 7.0, device="cuda")
        idx = torch.full((L, nh, 4), 7, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="exclude"):
            ops.bilinear_topk(zh, zt, ws, 4, exclude=m, out=(vals, idx))
        assert bool((vals == 7.0).all()) and bool((idx == 7).all()), name
        with pytest.raises(ValueError, match="exclude"):
            ops.bilinear_select_count(zh, zt, ws, thr, exclude=m)
        with pytest.raises(ValueError, match="exclude"):
            ops.bilinear_select(zh, zt, ws, thr, exclude=m)
    with pytest.raises(ValueError, match="symmetric"):
        ops.pair_mask([1], [2], nh, nt, symmetric=True)
    # P = L and P = 1 are both fine; exclude=None is the unmasked call
    per = ops.pair_mask([1, 1], [2, 3], nh, nt, labels=[0, 2], n_labels=L)
    v, i = ops.bilinear_topk(zh, zt, ws, 4, exclude=per)
    v0, i0 = ops.bilinear_topk(zh, zt, ws, 4, exclude=None)
    v1, i1 = ops.bilinear_topk(zh, zt, ws, 4)
    assert torch.equal(v0, v1) and torch.equal(i0, i1) and v.shape == v0.shape
    # the C ABI refuses a plane stride that is neither 0 nor a whole plane, and forwards a null mask to the twin
    from madrigal_amd._lib import lib
    args = (zh.data_ptr(), zt.data_ptr(), ws.data_ptr(), v.data_ptr(), i.data_ptr(), nh, nt, L, 128, 0, 4, 0, None, 0, None)
    assert lib().mdg_bilinear_topk_masked(*args, per.data_ptr(), 5) == -1 and b"plane_stride" in lib().mdg_last_error()
    assert lib().mdg_bilinear_topk_masked(*args, None, 0) == 0
    torch.cuda.synchronize()
    vf, _ = ops.bilinear_topk(zh, zt, ws, 4, precision="f32")
    assert torch.equal(v, vf)


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def small_model():
    """The small model of tests/test_topk_gpu.py (configs.build_model, drugbank163 layout, 6 outcomes) with the embeddings of 700
    drugs from generate_embeddings."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n, L = 700, 6
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    torch.manual_seed(3)
    model = configs.build_model("drugbank163", bkg["data"], L).cuda().eval()
    with M.precision("bf16x3"):
        z = generate_embeddings(model, b, kgc, kg_filler=_rand((n, 128), 6).cuda()).contiguous()
    assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
    return model, z


def _general_dense(model, z):
    """Dense scores [L,N,N] of the GENERAL sweep (a separate copy of z as the head operand selects it)."""
    with torch.no_grad():
        return model.decoder(z.clone(), z)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_top_partners_skips_the_known_partners_of_a_hub(small_model, prec):
    """The case the feature exists for: the 40 highest-scoring partners of drug 5 (per outcome) are known.  With ``exclude`` its 16
    partners are exactly ranks 41-56 of the dense row, bit-equal; the unmasked call returns none of them."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import known_pairs_mask, top_partners
    model, z = small_model
    N, drug, n_known, k = z.shape[0], 5, 40, 16
    with M.precision(prec):
        dense = _general_dense(model, z)
        L = dense.shape[0]
        i = torch.arange(N, device="cuda")
        not_self = dense.masked_fill((i[:, None] == i[None, :])[None], NEG)
        sv, si = torch.sort(not_self[:, drug], dim=1, descending=True, stable=True)          # [L, N]
        known_t = si[:, :n_known]
        labels = torch.arange(L, device="cuda")[:, None].expand(-1, n_known)
        mask = known_pairs_mask(N, torch.full((L * n_known,), drug), known_t.reshape(-1), labels=labels.reshape(-1), n_labels=L)
        assert mask.shape[0] == L
        vals, idx = top_partners(model, z, k, exclude=mask)
        assert torch.equal(idx[:, drug].long(), si[:, n_known:n_known + k])
        assert torch.equal(vals[:, drug], sv[:, n_known:n_known + k])
        plain_v, plain_i = top_partners(model, z, k)
        for l in range(L):
            assert not set(plain_i[l, drug].tolist()) & set(idx[l, drug].tolist())
            assert set(plain_i[l, drug].tolist()) <= set(known_t[l].tolist())
        # every other row: the dense order without the (symmetric) known pairs
        ex = torch.zeros((L, N, N), dtype=torch.bool, device="cuda")
        ex[labels, drug, known_t] = True
        ex |= ex.transpose(1, 2).clone()
        rv, ri = _ref_topk(not_self.masked_fill(ex, NEG), k)
        assert torch.equal(vals, rv) and torch.equal(idx, ri)
        # a sub-range of the outcomes takes its own planes of the per-outcome mask
        v2, i2 = top_partners(model, z, k, label_range=(2, 5), exclude=mask)
        assert torch.equal(v2, vals[2:5]) and torch.equal(i2, idx[2:5])
        v3, i3 = top_partners(model, z, k, label_range=(1, 6), drug_rows=[drug, 0, 699], max_temp_bytes=1, exclude=mask)
        assert torch.equal(v3, vals[1:6][:, [drug, 0, 699]]) and torch.equal(i3, idx[1:6][:, [drug, 0, 699]])
        with pytest.raises(ValueError, match="exclude"):
            top_partners(model, z, k, exclude=mask[:4])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_top_pairs_with_known_pairs_equals_brute_force(small_model, prec):
    """top_pairs(K = 200, k_row = 4, exclude) == brute force over the dense lower triangle with the excluded pairs at -inf.  The mask
    leaves only the pairs that involve one of ten drugs, so the 200 best lie in few rows whose 4-entry lists are too short: open rows,
    i.e. the masked re-score, in every outcome."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import known_pairs_mask, top_pairs
    model, z = small_model
    N, K = z.shape[0], 200
    ii, jj = torch.tril_indices(N - 10, N - 10, -1)                          # every pair among drugs 0 .. N - 11 is known
    shared = known_pairs_mask(N, ii, jj)
    with M.precision(prec):
        dense = _general_dense(model, z)
        L = dense.shape[0]
        known = torch.zeros((N, N), dtype=torch.bool, device="cuda")
        known[ii.cuda(), jj.cuda()] = True
        known |= known.T.clone()
        info = {}
        v, h, t = top_pairs(model, z, K, k_row=4, exclude=shared, info=info)
        bv, bh, bt = brute_force_pairs(dense.masked_fill(known[None], NEG).cpu(), K)
        assert bool(torch.isfinite(bv).all())
        assert torch.equal(h.cpu(), bh) and torch.equal(t.cpu(), bt) and torch.equal(v.cpu(), bv)
        assert max(info["open_rows"]) > 0 and min(info["open_rows"]) > 0, info
        assert bool((h >= N - 10).all())
        # per-outcome planes: outcome l additionally knows the best pair of outcome l found above; one outcome per chunk
        lab = torch.arange(L).repeat_interleave(ii.numel())
        hh, tt = torch.cat([ii.repeat(L), h[:, 0].cpu()]), torch.cat([jj.repeat(L), t[:, 0].cpu()])
        per = known_pairs_mask(N, hh, tt, labels=torch.cat([lab, torch.arange(L)]), n_labels=L)
        ex = known[None].repeat(L, 1, 1)
        ex[torch.arange(L), h[:, 0], t[:, 0]] = True
        info2 = {}
        v2, h2, t2 = top_pairs(model, z, K, label_range=(1, 5), k_row=4, exclude=per, info=info2, max_temp_bytes=1)
        bv, bh, bt = brute_force_pairs(dense.masked_fill(ex, NEG)[1:5].cpu(), K)
        assert torch.equal(h2.cpu(), bh) and torch.equal(t2.cpu(), bt) and torch.equal(v2.cpu(), bv)
        assert torch.equal(v2[:, 0], v[1:5, 1]) and min(info2["open_rows"]) > 0


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_selection_products_without_the_known_pairs(small_model, prec):
    """pairs_above, partners_above and partner_counts with ``exclude`` == their unmasked results with the known pairs removed
    (offsets and row pointers recomputed); a label sub-range of a per-outcome mask uses the right planes."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import csr_rows, known_pairs_mask, pairs_above, partner_counts, partners_above
    model, z = small_model
    N = z.shape[0]
    g = torch.Generator().manual_seed(11)
    with M.precision(prec):
        dense = _general_dense(model, z)
        L = dense.shape[0]
        n = 30000
        kh, kt, kl = torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g), torch.randint(0, L, (n,), generator=g)
        ok = kh != kt
        kh, kt, kl = kh[ok], kt[ok], kl[ok]
        per = known_pairs_mask(N, kh, kt, labels=kl, n_labels=L)
        known = torch.zeros((L, N, N), dtype=torch.bool, device="cuda")
        known[kl.cuda(), kh.cuda(), kt.cuda()] = True
        known |= known.transpose(1, 2).clone()
        low = torch.tril(torch.ones((N, N), dtype=torch.bool, device="cuda"), -1)
        thr = torch.stack([torch.quantile(dense[l][low][:200000], 0.97) for l in range(L)])
        for lo, hi in ((0, L), (2, 5)):
            kn, cut = known[lo:hi], thr[lo:hi]
            # pairs_above
            off0, h0, t0, v0 = pairs_above(model, z, cut, label_range=(lo, hi))
            off, h, t, v = pairs_above(model, z, cut, label_range=(lo, hi), exclude=per)
            l0 = torch.repeat_interleave(torch.arange(hi - lo, device="cuda"), off0[1:] - off0[:-1])
            keep = ~kn[l0, h0, t0]
            assert 0 < int(keep.sum()) < keep.numel()
            assert torch.equal(h, h0[keep]) and torch.equal(t, t0[keep]) and torch.equal(_bits(v), _bits(v0[keep]))
            want_off = torch.zeros(hi - lo + 1, dtype=torch.int64, device="cuda")
            want_off[1:] = torch.cumsum(torch.bincount(l0[keep], minlength=hi - lo), 0)
            assert torch.equal(off, want_off)
            # partners_above and partner_counts
            rp0, c0, pv0 = partners_above(model, z, cut, label_range=(lo, hi))
            rp, c, pv = partners_above(model, z, cut, label_range=(lo, hi), exclude=per)
            ol, oi, _ = csr_rows(rp0, N, total=int(c0.numel()))
            keep = ~kn[ol, oi, c0.long()]
            assert torch.equal(c, c0[keep]) and torch.equal(_bits(pv), _bits(pv0[keep]))
            cnt = torch.bincount((ol * N + oi)[keep], minlength=(hi - lo) * N)
            want_rp = torch.zeros((hi - lo) * N + 1, dtype=torch.int64, device="cuda")
            want_rp[1:] = torch.cumsum(cnt, 0)
            assert torch.equal(rp, want_rp)
            counts = partner_counts(model, z, cut, label_range=(lo, hi), exclude=per)
            assert counts.dtype == torch.int32 and torch.equal(counts.long(), cnt.view(hi - lo, N))
            assert not torch.equal(counts, partner_counts(model, z, cut, label_range=(lo, hi)))
        # a shared plane: known under any outcome
        shared = known_pairs_mask(N, kh, kt)
        any_known = known.any(0)
        off0, h0, t0, v0 = pairs_above(model, z, thr)
        off, h, t, v = pairs_above(model, z, thr, exclude=shared)
        keep = ~any_known[h0, t0]
        assert torch.equal(h, h0[keep]) and torch.equal(t, t0[keep]) and torch.equal(_bits(v), _bits(v0[keep]))
        # the decoder slices a per-outcome mask like the weight
        vals, idx = model.decoder.topk(z, z, 8, (2, 5), eligible="not_self", exclude=per)
        i = torch.arange(N, device="cuda")
        rv, ri = _ref_topk(dense[2:5].masked_fill((i[:, None] == i[None, :])[None] | known[2:5], NEG), 8)
        assert torch.equal(vals, rv) and torch.equal(idx, ri)
