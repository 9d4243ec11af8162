"""Threshold selection inside the all-pairs head on the GPU: mdg_bilinear_select_count / mdg_bilinear_select_fill against
torch.nonzero of (dense >= thr) & eligible over the project's own dense general sweep (exactly, values bit for bit, in the fp32-grade
modes; within the regrouping bound in the 16-bit modes), the bounded-write guard of the fill pass, the refusals, and the pipeline
products built on it (pairs_above, partner_counts, partners_above)."""
import functools

import pytest
import torch

from bincount_ref import eligible_mask, eligible_scores, inputs
from select_ref import dense_csr, dense_mask

pytestmark = pytest.mark.gpu

L = 3
ALL_ONLY = [(1, 1), (33, 4), (300, 333)]
SQUARE = [(300, 300), (513, 513)]          # past a 256-row and a 512-row workgroup, ending on a ragged 64-column tile; LOWER skips tiles
ELIGIBLE = {"all": 0, "not_self": 1, "lower": 2}
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16": 3}
COL_SENTINEL, VAL_SENTINEL = -7, -12345.0


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if (nh, nt) in SQUARE else ["all"]


@functools.lru_cache(maxsize=None)
def _case(prec, nh, nt):
    """(zh, zt, ws, dense) on the GPU: the inputs of bincount_ref and the STORE tensor of the general sweep, computed once per
    precision and shape and never modified."""
    from madrigal_amd import ops
    zh, zt, w = inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    return zh, zt, ws, ops.bilinear_allpairs(zh, zt, ws, precision=prec)


def _threshold_sets(dense, eligible):
    """{name: thr [L]}: -inf (every eligible pair; rows with more than 64 hits across tiles), +inf (nothing), the outcome's maximum
    eligible score, the score of (row nh - 1, column 3) -- columns 5, 9 and nt - 2 tie with it exactly where they exist --, the
    median, the value with about 0.1 % of the eligible scores at or above it, and one vector mixing the kinds."""
    vals = eligible_scores(dense, eligible)
    M = vals.shape[1]
    nh, nt = dense.shape[1:]
    dev = dense.device
    sv = torch.sort(vals, dim=1).values
    sets = {"ninf": torch.full((L,), float("-inf"), device=dev), "pinf": torch.full((L,), float("inf"), device=dev), "max": sv[:, -1].clone(),
            "tie": dense[:, nh - 1, min(3, nt - 1)].clone(), "median": sv[:, (M - 1) // 2].clone(),
            "sparse": sv[:, M - max(1, round(0.001 * M))].clone()}
    sets["mixed"] = torch.stack([sets["sparse"][0], sets["ninf"][1], sets["tie"][2]])
    return {k: v.contiguous() for k, v in sets.items()}


def _c_fill(ops, zh, zt, ws, thr, row_ptr, size, prec, eligible):
    """mdg_bilinear_select_fill through the C entry into sentinel-filled cols / vals of `size` entries (and one guard entry behind
    them, which must stay untouched)."""
    from madrigal_amd._lib import call
    cols = torch.full((size + 1,), COL_SENTINEL, dtype=torch.int32, device="cuda")
    vals = torch.full((size + 1,), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    nh, nt = zh.shape[0], zt.shape[0]
    buf, nbytes = ops._scratch("mdg_bilinear_select_workspace_bytes", zh.device, nh, nt, L, 128, PREC[prec])
    call("mdg_bilinear_select_fill", zh.data_ptr(), zt.data_ptr(), ws.data_ptr(), thr.data_ptr(), row_ptr.data_ptr(), cols.data_ptr(),
         vals.data_ptr(), nh, nt, L, 128, PREC[prec], ELIGIBLE[eligible], None if buf is None else buf.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert int(cols[size]) == COL_SENTINEL and float(vals[size]) == VAL_SENTINEL
    return cols[:size], vals[:size]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("nh,nt", ALL_ONLY + SQUARE)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_select_equals_nonzero_of_the_dense_general_sweep(ops, prec, nh, nt):
    """Counts, row_ptr, cols and vals == the CSR torch.nonzero gives on (dense >= thr) & eligible, vals bit-equal to dense[l,i,j];
    a second call is identical; row_ptr[-1] == T; the fill pass through the C entry leaves no sentinel."""
    zh, zt, ws, dense = _case(prec, nh, nt)
    for eligible in _modes(nh, nt):
        sets = _threshold_sets(dense, eligible)
        if (nh, nt) in SQUARE:                                             # the tie set tests >= on real ties
            row = dense[:, nh - 1]
            assert all(torch.equal(row[:, c], row[:, 3]) for c in (5, 9, nt - 2))
        for name, thr in sets.items():
            rc, rp, rcol, rval = dense_csr(dense, thr, eligible)
            T = int(rp[-1])
            what = (eligible, name, T)
            counts = ops.bilinear_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec)
            assert counts.shape == (L, nh) and counts.dtype == torch.int32
            assert torch.equal(counts, rc), what + (int((counts != rc).sum()),)
            row_ptr, cols, vals = ops.bilinear_select(zh, zt, ws, thr, eligible=eligible, precision=prec)
            assert row_ptr.dtype == torch.int64 and cols.dtype == torch.int32 and vals.dtype == torch.float32
            assert row_ptr.shape == (L * nh + 1,) and int(row_ptr[-1]) == T and cols.shape == (T,) and vals.shape == (T,), what
            assert torch.equal(row_ptr, rp), what
            assert torch.equal(cols, rcol), what
            assert torch.equal(_bits(vals), _bits(rval)), what
            again = ops.bilinear_select(zh, zt, ws, thr, eligible=eligible, precision=prec)
            assert torch.equal(again[0], row_ptr) and torch.equal(again[1], cols) and torch.equal(_bits(again[2]), _bits(vals)), what
            ccols, cvals = _c_fill(ops, zh, zt, ws, thr, rp, T, prec, eligible)
            assert not bool((ccols == COL_SENTINEL).any()) and torch.equal(ccols, rcol) and torch.equal(_bits(cvals), _bits(rval)), what
            if name == "ninf":
                assert T == L * int(eligible_mask(nh, nt, eligible).sum())
            if name == "pinf":
                assert T == 0
            if name == "tie" and (nh, nt) in SQUARE:
                mine = cols[int(row_ptr[nh - 1]):int(row_ptr[nh])].tolist()            # outcome 0, row nh - 1
                assert all(c in mine for c in (3, 5, 9, nt - 2)), what


def _scatter_mask(row_ptr, cols, shape):
    from madrigal_amd.pipeline import csr_rows
    l, i, _ = csr_rows(row_ptr, shape[1])
    got = torch.zeros(shape, dtype=torch.bool, device=cols.device)
    got[l, i, cols.long()] = True
    return got, l, i


@pytest.mark.parametrize("nh,nt", SQUARE)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_select_of_the_16bit_sweeps_is_within_the_regrouping_bound(ops, prec, nh, nt):
    """The single-product modes run the row-statistics sweep (16x16x32: fp32 sums grouped differently from the dense 32x32x16
    sweep, <= 2e-6 of the scale).  With delta = 2e-6 max|dense|: every eligible pair with dense >= thr + delta is selected, none with
    dense < thr - delta is, every returned value is within delta of its dense entry; count and fill agree (no sentinel left, columns
    strictly ascending within a row); the -inf / +inf sets are exact."""
    zh, zt, ws, dense = _case(prec, nh, nt)
    delta = 2e-6 * float(dense.abs().max())
    for eligible in _modes(nh, nt):
        elig = eligible_mask(nh, nt, eligible, "cuda")[None]
        for name, thr in _threshold_sets(dense, eligible).items():
            what = (eligible, name)
            counts = ops.bilinear_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec)
            row_ptr = torch.zeros(L * nh + 1, dtype=torch.int64, device="cuda")
            row_ptr[1:] = torch.cumsum(counts.reshape(-1), 0)
            T = int(row_ptr[-1])
            cols, vals = _c_fill(ops, zh, zt, ws, thr, row_ptr, T, prec, eligible)
            assert not bool((cols == COL_SENTINEL).any()) and not bool((vals == VAL_SENTINEL).any()), what
            assert bool(((cols >= 0) & (cols < nt)).all()), what
            got, l, i = _scatter_mask(row_ptr, cols, dense.shape)
            assert int(got.sum()) == T, what                                          # no column twice in a row
            same_row = (l[1:] == l[:-1]) & (i[1:] == i[:-1])
            assert bool((cols[1:] > cols[:-1])[same_row].all()), what
            o_rp, o_cols, o_vals = ops.bilinear_select(zh, zt, ws, thr, eligible=eligible, precision=prec)
            assert torch.equal(o_rp, row_ptr) and torch.equal(o_cols, cols) and torch.equal(_bits(o_vals), _bits(vals)), what
            must = dense_mask(dense, thr + delta, eligible)
            may = dense_mask(dense, thr - delta, eligible)
            band = int((may & ~must).sum())
            print(prec, (nh, nt), eligible, name, "selected", T, "inside the band", band, "of them selected", int((got & may & ~must).sum()),
                  "max |val - dense|", float((vals - dense[l, i, cols.long()]).abs().max()) if T else 0.0, "delta", delta)
            assert not bool((got & ~elig).any()), what
            assert not bool((must & ~got).any()), what
            assert not bool((got & ~may).any()), what
            assert bool(((vals - dense[l, i, cols.long()]).abs() <= delta).all()), what
            if name in ("ninf", "pinf"):
                rc, rp, rcol, _ = dense_csr(dense, thr, eligible)
                assert torch.equal(counts, rc) and torch.equal(row_ptr, rp) and torch.equal(cols, rcol), what


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "f16"])
def test_fill_never_writes_outside_its_rows_ranges(ops, prec, eligible):
    """The fill pass at the median cut, handed the row_ptr of the (higher) 0.1 % cut and sentinel-filled outputs of the full -inf
    size: every row holds its first row_counts hits in column order, everything behind row_ptr[-1] is untouched."""
    nh = nt = 513
    zh, zt, ws, dense = _case(prec, nh, nt)
    sets = _threshold_sets(dense, eligible)
    few = ops.bilinear_select_count(zh, zt, ws, sets["sparse"], eligible=eligible, precision=prec).reshape(-1).long()
    m_rp, m_cols, m_vals = ops.bilinear_select(zh, zt, ws, sets["median"], eligible=eligible, precision=prec)
    many = m_rp[1:] - m_rp[:-1]
    assert bool((many >= few).all()) and int(many.sum()) > 10 * int(few.sum()) > 0
    row_ptr = torch.zeros(L * nh + 1, dtype=torch.int64, device="cuda")
    row_ptr[1:] = torch.cumsum(few, 0)
    Ts = int(row_ptr[-1])
    full = L * int(eligible_mask(nh, nt, eligible).sum())
    cols, vals = _c_fill(ops, zh, zt, ws, sets["median"], row_ptr, full, prec, eligible)
    rows = torch.repeat_interleave(torch.arange(L * nh, device="cuda"), many)
    first = (torch.arange(m_cols.numel(), device="cuda") - m_rp[rows]) < few[rows]            # the first few[r] hits of every row
    assert int(first.sum()) == Ts
    assert torch.equal(cols[:Ts], m_cols[first]) and torch.equal(_bits(vals[:Ts]), _bits(m_vals[first]))
    assert bool((cols[Ts:] == COL_SENTINEL).all()) and bool((vals[Ts:] == VAL_SENTINEL).all())


def test_c_level_refusals_launch_nothing(ops):
    from madrigal_amd._lib import lib
    z = torch.randn(6, 128, device="cuda")
    w = torch.randn(2, 128, 128, device="cuda")
    thr = torch.zeros(2, device="cuda")
    counts = torch.full((2, 6), -7, dtype=torch.int32, device="cuda")
    row_ptr = torch.arange(13, dtype=torch.int64, device="cuda")
    cols = torch.full((12,), COL_SENTINEL, dtype=torch.int32, device="cuda")
    vals = torch.full((12,), VAL_SENTINEL, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731

    def count(nt, nl, D, prec, el):
        return lib().mdg_bilinear_select_count(p(z), p(z), p(w), p(thr), p(counts), 6, nt, nl, D, prec, el, None, 0, None)

    def fill(nt, nl, D, prec, el):
        return lib().mdg_bilinear_select_fill(p(z), p(z), p(w), p(thr), p(row_ptr), p(cols), p(vals), 6, nt, nl, D, prec, el, None, 0, None)

    for fn, name in ((count, b"mdg_bilinear_select_count"), (fill, b"mdg_bilinear_select_fill")):
        for nt, nl, D, el, what in ((6, 2, 128, 9, b"eligible"), (4, 2, 128, 2, b"one drug set"), (4, 2, 128, 1, b"one drug set"),
                                    (6, 2, 64, 0, b"D must be"), (6, 65536, 128, 0, b"n_labels")):
            rc = fn(nt, nl, D, 0, el)
            assert rc == -1 and name in lib().mdg_last_error() and what in lib().mdg_last_error(), (name, what, lib().mdg_last_error())
        for prec in (1, 2, 3):      # the operand images need a workspace: refused before anything is enqueued
            rc = fn(6, 2, 128, prec, 0)
            assert rc == -2 and name in lib().mdg_last_error() and b"workspace" in lib().mdg_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((cols == COL_SENTINEL).all()) and bool((vals == VAL_SENTINEL).all())
    # the wrapper
    for f in (ops.bilinear_select_count, ops.bilinear_select):
        with pytest.raises(ValueError, match="NaN"):
            f(z, z, w, torch.tensor([0.0, float("nan")], device="cuda"))
        with pytest.raises(ValueError, match="one cut per outcome"):
            f(z, z, w, torch.zeros(3, device="cuda"))
        with pytest.raises(ValueError, match="GPU"):
            f(z.cpu(), z.cpu(), w.cpu(), thr.cpu())
        with pytest.raises(ValueError, match="one drug set"):
            f(z, z[:4], w, thr, eligible="lower")
    low = torch.full((2,), float("-inf"), device="cuda")
    with pytest.raises(ValueError, match=r"T = 60\b"):                     # 2 outcomes x 6 x 5 pairs, 480 bytes
        ops.bilinear_select(z, z, w, low, eligible="not_self", max_bytes=479)
    assert ops.bilinear_select(z, z, w, low, eligible="not_self", max_bytes=480)[1].numel() == 60
    # empty L, empty Nh
    rp, c, v = ops.bilinear_select(z, z, w[:0], thr[:0])
    assert rp.tolist() == [0] and c.shape == (0,) and v.shape == (0,) and rp.dtype == torch.int64 and c.dtype == torch.int32
    rp, c, v = ops.bilinear_select(z[:0], z, w, thr)
    assert rp.tolist() == [0] and c.shape == (0,) and v.shape == (0,)
    assert ops.bilinear_select_count(z, z, w[:0], thr[:0]).shape == (0, 6)
    assert ops.bilinear_select_count(z[:0], z, w, thr).shape == (2, 0)


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def small_model():
    """A configs.build_model model (drugbank163 layout, 6 outcomes) and the embeddings of 300 drugs from generate_embeddings."""
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


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_pipeline_products_on_a_built_model(small_model, prec):
    """pairs_above at the 50th value of top_pairs(K = 50): its best 50 per outcome are top_pairs' pairs with the same values bit
    for bit, and nothing lies below the cut; it equals the dense lower-triangle CSR; partner_counts == the row sums of the dense
    not_self mask; partners_above == the dense not_self CSR."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import csr_rows, pairs_above, partner_counts, partners_above, top_pairs
    model, z = small_model
    N, n_out = z.shape[0], 6
    with M.precision(prec), torch.no_grad():
        dense = model.decoder(z.clone(), z)                               # the general sweep
        tv, th, tt = top_pairs(model, z, 50)
        cut = tv[:, -1].contiguous()
        offsets, head, tail, vals = pairs_above(model, z, cut)
        assert offsets.shape == (n_out + 1,) and offsets.dtype == torch.int64 and head.dtype == torch.int64 and tail.dtype == torch.int64
        assert int(offsets[0]) == 0 and int(offsets[-1]) == head.numel() == tail.numel() == vals.numel()
        rc, rp, rcol, rval = dense_csr(dense, cut, "lower")
        rl, rh, roff = csr_rows(rp, N)
        assert torch.equal(offsets, roff) and torch.equal(head, rh) and torch.equal(tail, rcol.long()) and torch.equal(_bits(vals), _bits(rval))
        assert bool((head > tail).all())
        for l in range(n_out):
            s, e = int(offsets[l]), int(offsets[l + 1])
            assert e - s >= 50 and bool((vals[s:e] >= cut[l]).all())                 # nothing below the cut
            best = torch.sort(vals[s:e], descending=True, stable=True)
            first = best.indices[:50]
            assert torch.equal(_bits(best.values[:50]), _bits(tv[l]))
            if e - s == 50 or float(best.values[50]) < float(cut[l]):                # no tie across the 50th place: the same pairs
                assert set(zip(head[s:e][first].tolist(), tail[s:e][first].tolist())) == set(zip(th[l].tolist(), tt[l].tolist()))
        o2, h2, t2, v2 = pairs_above(model, z, cut[2:5], label_range=(2, 5))
        s, e = int(offsets[2]), int(offsets[5])
        assert torch.equal(o2, offsets[2:6] - s) and torch.equal(h2, head[s:e]) and torch.equal(t2, tail[s:e]) and torch.equal(v2, vals[s:e])
        one = pairs_above(model, z, float(cut.max()))                                 # one number for every outcome
        assert torch.equal(one[0], csr_rows(dense_csr(dense, cut.max().expand(n_out), "lower")[1], N)[2])
        # degrees and neighbourhoods in the not_self network, at a cut that keeps about 1 % of the entries
        deg_cut = torch.quantile(dense.reshape(n_out, -1), 0.99, dim=1).contiguous()
        nc, nrp, ncol, nval = dense_csr(dense, deg_cut, "not_self")
        deg = partner_counts(model, z, deg_cut)
        assert deg.shape == (n_out, N) and deg.dtype == torch.int32 and torch.equal(deg, nc)
        assert torch.equal(partner_counts(model, z, deg_cut[1:3], label_range=(1, 3)), nc[1:3])
        prp, pcol, pval = partners_above(model, z, deg_cut)
        assert torch.equal(prp, nrp) and torch.equal(pcol, ncol) and torch.equal(_bits(pval), _bits(nval))
        with pytest.raises(ValueError, match="T = "):
            partners_above(model, z, deg_cut, max_bytes=8)
    with pytest.raises(ValueError):
        pairs_above(model, z, cut[:4])
    with pytest.raises(ValueError):
        pairs_above(model, z, cut, label_range=(0, 7))
