"""Threshold selection over a checkpoint ensemble on the GPU (ops.bilinear_ensemble_select_count / bilinear_ensemble_select,
pipeline.ensemble_partner_counts / ensemble_partners_above / ensemble_pairs_above) against the dense ensemble product, exactly.

The reference is always the GENERAL ensemble sweep on the card: ``ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws)`` (the
clone on the tail side forces the non-mirrored sweep, whose values (z_i W) z_j are the ones the selection sees), then
``torch.nonzero((P >= thr[:, None, None]) & allowed & ~excluded)``: row_ptr from a bincount of l * Nh + i, cols = the third index,
vals = P at the indices.  Every comparison is ``torch.equal`` (values compared as bits): no tolerance is involved.

Two input regimes (z ~ N(0,1) * scale, W ~ N(0,1) / sqrt(128), symmetrised):
  scale 0.3: no probability is 0 or 1 -- tests the values and >= on an attained value;
  scale 1.0: several per cent of all probabilities are exactly 1.0 at K = 1, fewer at K = 2 -- a cut of 1.0 selects a real tie set."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 3
INF = float("inf")
COL_SENTINEL, VAL_SENTINEL = -12345, -777.25
PREC = {"f32": 0, "bf16x3": 1}
ELIGIBLE = {"all": 0, "not_self": 1, "lower": 2}


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _dense(zh, zt, ws, prec):
    from madrigal_amd import ops
    return ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws, precision=prec).contiguous()


@functools.lru_cache(maxsize=None)
def _case(K, nh, nt, scale, prec, same, seed=0):
    """Inputs on the card and their dense general-sweep product: (zh, zt, ws, P [L,nh,nt] contiguous).  Shared; never modified."""
    from madrigal_amd import ops
    zh = [_rand((nh, 128), 1000 * seed + 10 * m, scale).cuda() for m in range(K)]
    zt = zh if same else [_rand((nt, 128), 1000 * seed + 10 * m + 1, scale).cuda() for m in range(K)]
    ws = [ops.symmetrize(_rand((L, 128, 128), 1000 * seed + 10 * m + 2, 1 / np.sqrt(128)).cuda()) for m in range(K)]
    return zh, zt, ws, _dense(zh, zt, ws, prec)


def _allowed(nh, nt, eligible, device="cuda"):
    i = torch.arange(nh, device=device)[:, None]
    j = torch.arange(nt, device=device)[None, :]
    if eligible == "all":
        return torch.ones((nh, nt), dtype=torch.bool, device=device)
    return (j != i) if eligible == "not_self" else (j < i)


def _attained(plane, q=0.99):
    """The value of ``plane`` at its dense q quantile: an attained value, so >= is tested on equality."""
    flat = torch.sort(plane.reshape(-1)).values
    return float(flat[int(q * (flat.numel() - 1))])


def _cuts(P):
    """The three threshold vectors of the issue, one cut per outcome each."""
    dev = P.device
    return {"attained_half_one": torch.tensor([_attained(P[0]), 0.5, 1.0], device=dev),
            "ninf_pinf_above": torch.tensor([-INF, INF, 1.5], device=dev),
            "zero_attained_ninf": torch.tensor([0.0, _attained(P[1]), -INF], device=dev)}


def _dense_csr(P, thr, eligible, excluded=None):
    """(row_counts int32 [L,nh], row_ptr int64 [L*nh+1], cols int32 [T], vals fp32 [T]) of the dense P."""
    nl, nh, nt = P.shape
    m = (P >= thr[:, None, None]) & _allowed(nh, nt, eligible, P.device)[None]
    if excluded is not None:
        m &= ~excluded.expand(nl, nh, nt)
    idx = torch.nonzero(m)
    counts = torch.bincount(idx[:, 0] * nh + idx[:, 1], minlength=nl * nh)
    row_ptr = torch.zeros(nl * nh + 1, dtype=torch.int64, device=P.device)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return counts.reshape(nl, nh).to(torch.int32), row_ptr, idx[:, 2].to(torch.int32), P[idx[:, 0], idx[:, 1], idx[:, 2]]


def _bits(t):
    return t.view(torch.int32)


def _check_csr(got, want, what=()):
    row_ptr, cols, vals = got
    _, rp, rcol, rval = want
    assert row_ptr.dtype == torch.int64 and cols.dtype == torch.int32 and vals.dtype == torch.float32, what
    assert row_ptr.shape == rp.shape and cols.shape == rcol.shape and vals.shape == rval.shape, what + (tuple(cols.shape), tuple(rcol.shape))
    assert torch.equal(row_ptr, rp), what
    assert torch.equal(cols, rcol), what
    assert torch.equal(_bits(vals), _bits(rval)), what


def _check_both(zh, zt, ws, P, thr, eligible, prec, exclude=None, excluded=None, what=()):
    """count alone against the row sizes, select against the whole CSR; returns the selection."""
    from madrigal_amd import ops
    want = _dense_csr(P, thr, eligible, excluded)
    counts = ops.bilinear_ensemble_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec, exclude=exclude)
    assert counts.dtype == torch.int32 and counts.shape == want[0].shape, what
    assert torch.equal(counts, want[0]), what + (int((counts != want[0]).sum()),)
    got = ops.bilinear_ensemble_select(zh, zt, ws, thr, eligible=eligible, precision=prec, exclude=exclude)
    _check_csr(got, want, what)
    return got


def _shape(name):
    from madrigal_amd import ops
    chunk = 64 * ops.bilinear_ensemble_topk_chunk_tiles()
    return {"1x1": (1, 1), "33x65": (33, 65), "129x130": (129, 130), "chunk-1": (129, chunk - 1), "chunk": (129, chunk),
            "chunk+1": (129, chunk + 1), "300x1001": (300, 1001)}[name]


# ---- sizes and cuts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", ["1x1", "33x65", "129x130", "chunk-1", "chunk", "chunk+1", "300x1001"])
def test_sizes_and_cuts_against_the_dense_product(shape, K, scale, prec):
    nh, nt = _shape(shape)
    zh, zt, ws, P = _case(K, nh, nt, scale, prec, False)
    for name, thr in _cuts(P).items():
        rp, cols, vals = _check_both(zh, zt, ws, P, thr, "all", prec, what=(name,))
        sizes = (rp[1:] - rp[:-1]).reshape(L, nh)
        if name == "ninf_pinf_above":                  # every column of every row; nothing; nothing (no probability exceeds 1)
            assert bool((sizes[0] == nt).all()) and int(sizes[1:].sum()) == 0
        if name == "zero_attained_ninf":               # a probability is never negative: 0.0 and -inf both select full rows
            assert bool((sizes[0] == nt).all()) and bool((sizes[2] == nt).all())
            assert 0 < int(sizes[1].sum()) < nh * nt or nh * nt == 1


def test_the_two_regimes_are_what_the_docstring_says():
    """Scale 1.0: a cut of 1.0 selects a non-trivial tie set at K = 1 and K = 2, next to nothing at K = 5 and nothing at K = 8;
    scale 0.3: no probability is 0 or 1 for any K; the attained 0.99 cut leaves short rows, some of them empty at K = 1."""
    from madrigal_amd import ops
    one = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    for K, lo in ((1, 0.01), (2, 0.0005)):
        zh, zt, ws, P = _case(K, 300, 1001, 1.0, "bf16x3", False)
        assert float((P == 1.0).float().mean()) > lo
        assert int(ops.bilinear_ensemble_select_count(zh, zt, ws, one).sum()) == int((P == 1.0).sum())
    zh, zt, ws, P = _case(5, 300, 1001, 1.0, "bf16x3", False)      # five sigmoids that all round to 1: a handful of pairs at most
    assert int(ops.bilinear_ensemble_select_count(zh, zt, ws, one).sum()) == int((P == 1.0).sum()) < 100
    zh, zt, ws, P = _case(8, 300, 1001, 1.0, "bf16x3", False)
    assert int(ops.bilinear_ensemble_select_count(zh, zt, ws, one).sum()) == int((P == 1.0).sum()) == 0
    for K in (1, 2, 5, 8):
        P = _case(K, 300, 1001, 0.3, "bf16x3", False)[3]
        assert not bool(((P == 0.0) | (P == 1.0)).any())
    zh, zt, ws, P = _case(1, 300, 1001, 0.3, "bf16x3", False)
    c = ops.bilinear_ensemble_select_count(zh, zt, ws, _cuts(P)["attained_half_one"])[0]
    assert int(c.min()) == 0 and 8 < int(c.max()) < 64


# ---- eligibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0), (2, 1.0)])
@pytest.mark.parametrize("eligible", ["not_self", "lower"])
@pytest.mark.parametrize("N", [1, 2, 129, 300])
def test_one_drug_set_against_itself(N, eligible, K, scale, prec):
    z, _, ws, P = _case(K, N, N, scale, prec, True)
    for name, thr in _cuts(P).items():
        rp, cols, vals = _check_both(z, z, ws, P, thr, eligible, prec, what=(name,))
        sizes = (rp[1:] - rp[:-1]).reshape(L, N)
        if eligible == "lower":                       # row 0 has no eligible column, row 5 has five
            assert int(sizes[:, 0].sum()) == 0
            if N > 5:
                assert int(sizes[:, 5].max()) <= 5
                if name == "ninf_pinf_above":
                    assert int(sizes[0, 5]) == 5 and cols[int(rp[5]):int(rp[6])].tolist() == [0, 1, 2, 3, 4]
        elif name == "ninf_pinf_above":
            assert bool((sizes[0] == N - 1).all())


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def _random_pairs(N, frac, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(N * N * frac)
    return torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
@pytest.mark.parametrize("planes", ["shared", "per_outcome"])
@pytest.mark.parametrize("eligible", ["not_self", "lower"])
def test_exclusion_masks(eligible, planes, K, scale, prec):
    """1 % of the pairs at random plus every bit of row 7: the masked selection is the dense one minus those pairs, and (shared
    plane) row 7 is empty under every cut, -inf included."""
    from madrigal_amd import ops
    N = 300
    z, _, ws, P = _case(K, N, N, scale, prec, True)
    h, t = _random_pairs(N, 0.01, 5)
    h = torch.cat([h, torch.full((N,), 7)])
    t = torch.cat([t, torch.arange(N)])
    sym = eligible == "not_self"
    if planes == "shared":
        mask = ops.pair_mask(h, t, N, symmetric=sym, device="cuda")
    else:
        mask = ops.pair_mask(h, t, N, labels=torch.arange(h.numel()) % L, n_labels=L, symmetric=sym, device="cuda")
    excluded = ops.pair_mask_dense(mask, N, N)
    for name, thr in _cuts(P).items():
        rp, cols, vals = _check_both(z, z, ws, P, thr, eligible, prec, exclude=mask, excluded=excluded, what=(name,))
        if planes == "shared":
            sizes = (rp[1:] - rp[:-1]).reshape(L, N)
            assert int(sizes[:, 7].sum()) == 0


@pytest.mark.parametrize("eligible", ["not_self", "lower"])
def test_an_empty_mask_equals_the_unmasked_call_and_a_mask_of_the_hits_selects_nothing(eligible):
    from madrigal_amd import ops
    from madrigal_amd.pipeline import csr_rows
    N = 300
    z, _, ws, P = _case(5, N, N, 0.3, "bf16x3", True)
    thr = _cuts(P)["attained_half_one"]
    none = ops.bilinear_ensemble_select(z, z, ws, thr, eligible=eligible)
    assert int(none[0][-1]) > 0
    for planes in (1, L):
        zero = torch.zeros((planes, (N + 31) // 32, 320), dtype=torch.int32, device="cuda")
        got = ops.bilinear_ensemble_select(z, z, ws, thr, eligible=eligible, exclude=zero)
        assert all(torch.equal(a, b) for a, b in zip(got, none))
        assert torch.equal(ops.bilinear_ensemble_select_count(z, z, ws, thr, eligible=eligible, exclude=zero),
                           ops.bilinear_ensemble_select_count(z, z, ws, thr, eligible=eligible))
    lab, head, _ = csr_rows(none[0], N)
    hits = ops.pair_mask(head, none[1].long(), N, labels=lab, n_labels=L, device="cuda")      # exactly the hits, outcome by outcome
    rp, cols, vals = ops.bilinear_ensemble_select(z, z, ws, thr, eligible=eligible, exclude=hits)
    assert int(rp[-1]) == 0 and cols.numel() == 0 and vals.numel() == 0 and not bool(rp.any())
    assert not bool(ops.bilinear_ensemble_select_count(z, z, ws, thr, eligible=eligible, exclude=hits).any())
    # one bit fewer in the mask: exactly that pair comes back
    keep = int(none[1].numel()) // 2
    sel = torch.ones(none[1].numel(), dtype=torch.bool, device="cuda")
    sel[keep] = False
    almost = ops.pair_mask(head[sel], none[1].long()[sel], N, labels=lab[sel], n_labels=L, device="cuda")
    rp, cols, vals = ops.bilinear_ensemble_select(z, z, ws, thr, eligible=eligible, exclude=almost)
    assert int(rp[-1]) == 1 and int(cols[0]) == int(none[1][keep]) and torch.equal(_bits(vals), _bits(none[2][keep:keep + 1]))
    assert int(rp[int(lab[keep]) * N + int(head[keep]) + 1]) == 1 and int(rp[int(lab[keep]) * N + int(head[keep])]) == 0


# ---- out, determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
def test_two_calls_agree_and_out_is_written_everywhere(K, scale):
    from madrigal_amd import ops
    zh, zt, ws, P = _case(K, 300, 1001, scale, "bf16x3", False)
    for name, thr in _cuts(P).items():
        a = ops.bilinear_ensemble_select(zh, zt, ws, thr)
        b = ops.bilinear_ensemble_select(zh, zt, ws, thr)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2])), name
        out = torch.full((L, 300), -7, dtype=torch.int32, device="cuda")
        back = ops.bilinear_ensemble_select_count(zh, zt, ws, thr, out=out)
        assert back is out and not bool((out == -7).any())
        assert torch.equal(out, _dense_csr(P, thr, "all")[0]), name
        if name == "ninf_pinf_above":
            assert bool((out[1:] == 0).all())         # zeros are written, not left
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_ensemble_select_count(zh, zt, ws, thr, out=torch.zeros((L, 299), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.bilinear_ensemble_select_count(zh, zt, ws, thr, out=torch.zeros((L, 300), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_ensemble_select(zh, zt, ws, thr, eligible="not_self")


# ---- bounded writes ---------------------------------------------------------------------------------------------------------------
def _c_fill(zh, zt, ws, thr, row_ptr, size, prec, eligible):
    """mdg_bilinear_ensemble_select_fill through the C entry into sentinel-filled cols / vals of `size` entries (and one guard entry
    behind them, which must stay untouched)."""
    import ctypes
    from madrigal_amd import ops
    from madrigal_amd._lib import call
    K, nh, nt = len(zh), zh[0].shape[0], zt[0].shape[0]
    cols = torch.full((size + 1,), COL_SENTINEL, dtype=torch.int32, device="cuda")
    vals = torch.full((size + 1,), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    buf, nbytes = ops._scratch("mdg_bilinear_ensemble_select_workspace_bytes", zh[0].device, nh, nt, L, 128, K, PREC[prec])
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    call("mdg_bilinear_ensemble_select_fill", arr(zh), arr(zt), arr(ws), K, thr.data_ptr(), row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(),
         nh, nt, L, 128, PREC[prec], ELIGIBLE[eligible], None if buf is None else buf.data_ptr(), nbytes, None, None, 0)
    torch.cuda.synchronize()
    assert int(cols[size]) == COL_SENTINEL and float(vals[size]) == VAL_SENTINEL
    return cols[:size], vals[:size]


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_fill_never_writes_outside_its_rows_ranges(prec, eligible):
    """The fill pass at the 0.5 cut, handed the row_ptr of the (higher) attained-value cut and sentinel-filled outputs of the full
    eligible size: every row holds its first row_counts hits in column order, everything behind row_ptr[-1] is untouched."""
    from madrigal_amd import ops
    N, K = 513, 2
    z, _, ws, P = _case(K, N, N, 0.3, prec, True)
    high = torch.tensor([_attained(P[l]) for l in range(L)], device="cuda")
    half = torch.full((L,), 0.5, device="cuda")
    few = ops.bilinear_ensemble_select_count(z, z, ws, high, eligible=eligible, precision=prec).reshape(-1).long()
    m_rp, m_cols, m_vals = ops.bilinear_ensemble_select(z, z, ws, half, eligible=eligible, precision=prec)
    many = m_rp[1:] - m_rp[:-1]
    assert bool((many >= few).all()) and int(many.sum()) > 10 * int(few.sum()) > 0
    row_ptr = torch.zeros(L * N + 1, dtype=torch.int64, device="cuda")
    row_ptr[1:] = torch.cumsum(few, 0)
    Ts = int(row_ptr[-1])
    full = L * int(_allowed(N, N, eligible).sum())
    cols, vals = _c_fill(z, z, ws, half, row_ptr, full, prec, eligible)
    rows = torch.repeat_interleave(torch.arange(L * N, device="cuda"), many)
    first = (torch.arange(m_cols.numel(), device="cuda") - m_rp[rows]) < few[rows]            # the first few[r] hits of every row
    assert int(first.sum()) == Ts
    assert torch.equal(cols[:Ts], m_cols[first]) and torch.equal(_bits(vals[:Ts]), _bits(m_vals[first]))
    assert bool((cols[Ts:] == COL_SENTINEL).all()) and bool((vals[Ts:] == VAL_SENTINEL).all())
    # the matching row_ptr leaves no sentinel
    cols, vals = _c_fill(z, z, ws, half, m_rp, int(m_rp[-1]), prec, eligible)
    assert torch.equal(cols, m_cols) and torch.equal(_bits(vals), _bits(m_vals))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_c_level_refusals_launch_nothing():
    import ctypes
    from madrigal_amd import ops
    from madrigal_amd._lib import lib
    K = 2
    z = [torch.randn(6, 128, device="cuda") for _ in range(K)]
    w = [torch.randn(2, 128, 128, device="cuda") for _ in range(K)]
    thr = torch.zeros(2, device="cuda")
    counts = torch.full((2, 6), -7, dtype=torch.int32, device="cuda")
    row_ptr = torch.arange(13, dtype=torch.int64, device="cuda")
    cols = torch.full((12,), COL_SENTINEL, dtype=torch.int32, device="cuda")
    vals = torch.full((12,), VAL_SENTINEL, device="cuda")
    mask = torch.zeros((1, 1, 64), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    a_z, a_w = arr(z), arr(w)

    def count(nm, nt, nl, D, prec, el, m=None, ms=0):
        return lib().mdg_bilinear_ensemble_select_count(a_z, a_z, a_w, nm, p(thr), p(counts), 6, nt, nl, D, prec, el, None, 0, None, m, ms)

    def fill(nm, nt, nl, D, prec, el, m=None, ms=0):
        return lib().mdg_bilinear_ensemble_select_fill(a_z, a_z, a_w, nm, p(thr), p(row_ptr), p(cols), p(vals), 6, nt, nl, D, prec, el, None, 0,
                                                       None, m, ms)

    for fn, name in ((count, b"mdg_bilinear_ensemble_select_count"), (fill, b"mdg_bilinear_ensemble_select_fill")):
        for nm, nt, nl, D, prec, el, what in ((0, 6, 2, 128, 0, 0, b"n_models"), (9, 6, 2, 128, 0, 0, b"n_models"), (2, 6, 2, 128, 0, 9, b"eligible"),
                                              (2, 4, 2, 128, 0, 2, b"one drug set"), (2, 4, 2, 128, 0, 1, b"one drug set"),
                                              (2, 6, 2, 64, 0, 0, b"D must be"), (2, 6, 65536, 128, 0, 0, b"n_labels"),
                                              (2, 6, 2, 128, 2, 0, b"not offered"), (2, 6, 2, 128, 3, 0, b"not offered")):
            rc = fn(nm, nt, nl, D, prec, el)
            assert rc == -1 and name in lib().mdg_last_error() and what in lib().mdg_last_error(), (name, what, lib().mdg_last_error())
        rc = fn(2, 6, 2, 128, 1, 0)     # the operand images need a workspace: refused before anything is enqueued
        assert rc == -2 and name in lib().mdg_last_error() and b"workspace" in lib().mdg_last_error()
        rc = fn(2, 6, 2, 128, 0, 0, p(mask), 5)     # a plane stride that is neither 0 nor a whole plane
        assert rc == -1 and name in lib().mdg_last_error() and b"plane_stride" in lib().mdg_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((cols == COL_SENTINEL).all()) and bool((vals == VAL_SENTINEL).all())
    # the wrapper
    for f in (ops.bilinear_ensemble_select_count, ops.bilinear_ensemble_select):
        with pytest.raises(ValueError, match="NaN"):
            f(z, z, w, torch.tensor([0.0, float("nan")], device="cuda"))
        with pytest.raises(ValueError, match="one cut per outcome"):
            f(z, z, w, torch.zeros(3, device="cuda"))
        with pytest.raises(ValueError, match="GPU"):
            f([t.cpu() for t in z], [t.cpu() for t in z], [t.cpu() for t in w], thr.cpu())
        with pytest.raises(ValueError, match="one drug set"):
            f(z, [t[:4] for t in z], w, thr, eligible="lower")
    low = torch.full((2,), -INF, device="cuda")
    with pytest.raises(ValueError, match=r"T = 60\b"):                     # 2 outcomes x 6 x 5 pairs, 480 bytes
        ops.bilinear_ensemble_select(z, z, w, low, eligible="not_self", max_bytes=479)
    assert ops.bilinear_ensemble_select(z, z, w, low, eligible="not_self", max_bytes=480)[1].numel() == 60
    # empty L, empty Nh, empty Nt
    rp, c, v = ops.bilinear_ensemble_select(z, z, [t[:0] for t in w], thr[:0])
    assert rp.tolist() == [0] and c.shape == (0,) and v.shape == (0,) and rp.dtype == torch.int64 and c.dtype == torch.int32
    rp, c, v = ops.bilinear_ensemble_select([t[:0] for t in z], z, w, thr)
    assert rp.tolist() == [0] and c.shape == (0,) and v.shape == (0,)
    rp, c, v = ops.bilinear_ensemble_select(z, [t[:0] for t in z], w, low)
    assert rp.tolist() == [0] * 13 and c.shape == (0,)
    assert ops.bilinear_ensemble_select_count(z, z, [t[:0] for t in w], thr[:0]).shape == (0, 6)
    assert ops.bilinear_ensemble_select_count([t[:0] for t in z], z, w, thr).shape == (2, 0)
    assert not bool(ops.bilinear_ensemble_select_count(z, [t[:0] for t in z], w, low).any())


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_models():
    """Three configs.build_model checkpoints (drugbank163 layout, 6 outcomes) differing by seed, and the embeddings of 300 drugs
    from generate_embeddings under each."""
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


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_pipeline_products_on_three_checkpoints(small_models, prec):
    """ensemble_pairs_above at the 50th value of ensemble_top_pairs(K = 50): its best 50 per outcome are ensemble_top_pairs' pairs with
    the same probabilities bit for bit, and nothing lies below the cut; it equals the dense lower-triangle CSR; ensemble_partner_counts
    == the row sums of the dense not_self mask; ensemble_partners_above == the dense not_self CSR and lists every unordered pair from
    both sides; exclude= removes exactly the known pairs."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import (csr_rows, ensemble_all_pairs, ensemble_pairs_above, ensemble_partner_counts, ensemble_partners_above,
                                       ensemble_top_pairs, known_pairs_mask)
    from madrigal_amd import ops
    models, zs = small_models
    N, n_out = zs[0].shape[0], 6
    with M.precision(prec), torch.no_grad():
        dense = ensemble_all_pairs(models, zs, drug_2_inds=list(range(N))).contiguous()       # an index list on the tail side: the general sweep
        tv, th, tt = ensemble_top_pairs(models, zs, 50)
        cut = tv[:, -1].contiguous()
        offsets, head, tail, vals = ensemble_pairs_above(models, zs, cut)
        assert offsets.shape == (n_out + 1,) and offsets.dtype == torch.int64 and head.dtype == torch.int64 and tail.dtype == torch.int64
        assert vals.dtype == torch.float32 and int(offsets[0]) == 0 and int(offsets[-1]) == vals.numel()
        want = _dense_csr(dense, cut, "lower")
        lab, h_want, off_want = csr_rows(want[1], N)
        assert torch.equal(offsets, off_want) and torch.equal(head, h_want) and torch.equal(tail, want[2].long())
        assert torch.equal(_bits(vals), _bits(want[3]))
        for l in range(n_out):
            s, e = int(offsets[l]), int(offsets[l + 1])
            assert e - s >= 50 and bool((vals[s:e] >= cut[l]).all())
            assert bool((head[s:e] > tail[s:e]).all())
            # the best 50 in ensemble_top_pairs' order: (P descending, head ascending, tail ascending) = a stable sort of the CSR order
            order = torch.sort(vals[s:e], descending=True, stable=True).indices[:50]
            assert torch.equal(_bits(vals[s:e][order]), _bits(tv[l])) and torch.equal(head[s:e][order], th[l]) and torch.equal(tail[s:e][order], tt[l])
        # a label range, and a number as the cut
        o2, h2, t2, v2 = ensemble_pairs_above(models, zs, cut[2:5], label_range=(2, 5))
        s, e = int(offsets[2]), int(offsets[5])
        assert torch.equal(o2, offsets[2:6] - offsets[2]) and torch.equal(h2, head[s:e]) and torch.equal(t2, tail[s:e]) and torch.equal(_bits(v2), _bits(vals[s:e]))
        num = float(cut.max())
        o3, h3, t3, v3 = ensemble_pairs_above(models, zs, num)
        w3 = _dense_csr(dense, torch.full((n_out,), num, device="cuda"), "lower")
        assert torch.equal(t3, w3[2].long()) and torch.equal(_bits(v3), _bits(w3[3]))
        # degrees and neighbourhoods
        ns = _dense_csr(dense, cut, "not_self")
        counts = ensemble_partner_counts(models, zs, cut)
        assert counts.dtype == torch.int32 and torch.equal(counts, ns[0])
        assert torch.equal(counts.long(), ((dense >= cut[:, None, None]) & _allowed(N, N, "not_self")[None]).sum(2))
        _check_csr(ensemble_partners_above(models, zs, cut), ns)
        # every unordered pair of ensemble_pairs_above whose mirrored entry also passes is listed from both sides
        rp, pc, pv = ensemble_partners_above(models, zs, cut)
        pl, ph, _ = csr_rows(rp, N)
        listed = torch.zeros((n_out, N, N), dtype=torch.bool, device="cuda")
        listed[pl, ph, pc.long()] = True
        lab_low = torch.repeat_interleave(torch.arange(n_out, device="cuda"), offsets[1:] - offsets[:-1])
        assert bool(listed[lab_low, head, tail].all())
        mirrored = dense[lab_low, tail, head] >= cut[lab_low]
        # (P[l,i,j] and P[l,j,i] differ in their last bits only, so only a pair within rounding distance of the cut can be one-sided)
        assert torch.equal(listed[lab_low, tail, head], mirrored) and float(mirrored.float().mean()) > 0.5
        # the known network
        g = torch.Generator().manual_seed(12)
        kh, kt = torch.randint(0, N, (900,), generator=g), torch.randint(0, N, (900,), generator=g)
        known = known_pairs_mask(N, torch.cat([kh, head[:20].cpu()]), torch.cat([kt, tail[:20].cpu()]))
        excluded = ops.pair_mask_dense(known, N, N)
        assert bool(excluded[0, head[:20], tail[:20]].all())
        wx = _dense_csr(dense, cut, "lower", excluded)
        ox, hx, tx, vx = ensemble_pairs_above(models, zs, cut, exclude=known)
        assert int(ox[-1]) < int(offsets[-1])
        assert torch.equal(tx, wx[2].long()) and torch.equal(_bits(vx), _bits(wx[3])) and torch.equal(hx, csr_rows(wx[1], N)[1])
        assert torch.equal(ensemble_partner_counts(models, zs, cut, exclude=known), _dense_csr(dense, cut, "not_self", excluded)[0])
        _check_csr(ensemble_partners_above(models, zs, cut, exclude=known), _dense_csr(dense, cut, "not_self", excluded))
        with pytest.raises(ValueError, match=r"T = \d+ selected pairs"):
            ensemble_pairs_above(models, zs, cut, max_bytes=8 * int(offsets[-1]) - 1)
        assert ensemble_pairs_above(models, zs, cut, max_bytes=8 * int(offsets[-1]))[3].numel() == int(offsets[-1])
