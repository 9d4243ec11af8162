"""The in-sweep products agree with each other bit for bit, in every precision.

Top-k, threshold selection and the score histograms promise "the same MFMA sequence per accumulator element" (the headers of csrc/topk.hip, select.hip and bincount.hip),
so what one of them reports about a score the others must report too -- exactly, also in bf16 / f16, where their own tests only
hold them to 2e-6 of the scale against the dense sweep and a changed summation order in ONE product would pass.  No reference and
no tolerance here: per precision, ``eligible`` mode and with / without a pair mask

  top-k (k = 8)  ->  thr[l] = the smallest 8th value over the rows of outcome l with a full list
  selection at thr, re-sorted per row by (score descending, column ascending): its first 8 entries ARE the row's list, values and
      columns, in every row whose 8th value reaches thr[l]
  select_count = the row lengths of that CSR
  bincount(edges = thr)[l, 1] = select_count[l].sum()
  split = mask: the two classes sum to the unsplit counts, class 0 = the count of the masked selection

Shapes: one set of 577 drugs (three 256-row blocks with a one-row last wave, two 512-row blocks in the 16-bit layout, ten column
tiles the last of which holds one column, the diagonal crossing partial tiles) and 130 x 200 for two sets."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 8
L = 2
PRECISIONS = ["f32", "bf16x3", "bf16", "f16"]
CASES = [(577, 577, "all"), (577, 577, "not_self"), (577, 577, "lower"), (130, 200, "all")]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=2)
def _inputs(nh, nt):
    """(zh, zt, ws, mask) on the GPU, shared and never modified.  Tail rows 5 and 9 copy row 3 (exact ties); the mask has about 3 % random
    bits plus one full row and one full column."""
    from madrigal_amd import ops
    zt = _rand((nt, 128), 2)
    zt[5] = zt[9] = zt[3]
    zh = zt.clone() if nh == nt else _rand((nh, 128), 1)
    ws = ops.symmetrize((_rand((L, 128, 128), 3, 1 / np.sqrt(128))).cuda())
    g = torch.Generator().manual_seed(7)
    bits = torch.rand((nh, nt), generator=g) < 0.03
    bits[nh // 3, :] = True
    bits[:, nt - 7] = True
    hs, ts = torch.nonzero(bits, as_tuple=True)
    return zh.cuda(), zt.cuda(), ws, ops.pair_mask(hs, ts, nh, nt)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("nh,nt,mode", CASES, ids=[f"{a}x{b}-{m}" for a, b, m in CASES])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_topk_selection_and_counts_see_the_same_scores(prec, nh, nt, mode, masked):
    from madrigal_amd import ops
    zh, zt, ws, mask = _inputs(nh, nt)
    ex = mask if masked else None
    kw = dict(eligible=mode, precision=prec)
    vals, idx = ops.bilinear_topk(zh, zt, ws, K, exclude=ex, **kw)
    kth = vals[..., K - 1]
    full = kth > float("-inf")
    assert bool(full.any(dim=1).all()), "every outcome needs a row with a full list"
    thr = torch.where(full, kth, torch.full_like(kth, float("inf"))).amin(dim=1)
    assert bool(torch.isfinite(thr).all())

    row_ptr, cols, sv = ops.bilinear_select(zh, zt, ws, thr, exclude=ex, **kw)
    counts = ops.bilinear_select_count(zh, zt, ws, thr, exclude=ex, **kw)
    lens = (row_ptr[1:] - row_ptr[:-1]).reshape(L, nh)
    assert torch.equal(counts.to(torch.int64), lens)

    # the selection of every row re-sorted by (score descending, column ascending); its first K entries against the row's list
    rp, c, v = row_ptr.cpu().numpy(), cols.cpu().numpy(), sv.cpu().numpy()
    rows = np.repeat(np.arange(L * nh), np.diff(rp))
    order = np.lexsort((c, -v, rows))
    c, v = c[order], v[order]
    take = np.nonzero((kth >= thr[:, None]).reshape(-1).cpu().numpy())[0]
    assert take.size >= L and bool((np.diff(rp)[take] >= K).all())
    at = rp[take][:, None] + np.arange(K)[None, :]
    assert np.array_equal(v[at], vals.reshape(L * nh, K).cpu().numpy()[take])
    assert np.array_equal(c[at], idx.reshape(L * nh, K).cpu().numpy()[take])

    edges = thr[:, None].contiguous()
    hist = ops.bilinear_bincount(zh, zt, ws, edges, **kw)
    if not masked:
        assert torch.equal(hist[:, 1], counts.to(torch.int64).sum(dim=1))
    else:
        both = ops.bilinear_bincount(zh, zt, ws, edges, split=mask, **kw)
        assert torch.equal(both.sum(dim=0), hist)
        unmasked = ops.bilinear_select_count(zh, zt, ws, thr, **kw)          # the unsplit counts against selection at these same cuts
        assert torch.equal(hist[:, 1], unmasked.to(torch.int64).sum(dim=1))
        assert torch.equal(both[0][:, 1], counts.to(torch.int64).sum(dim=1))
