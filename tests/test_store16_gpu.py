"""16-bit destinations of the all-pairs head (mdg_bilinear_allpairs16_ld) on the GPU.

Every comparison is exact: the 16-bit tensor must be bit-equal to the fp32 tensor of the GENERAL sweep cast afterwards
(``ops.bilinear_allpairs(z_head, z_tail.clone(), w).to(dtype)``; the clone keeps the fp32 launcher off its symmetric sweep, which
associates differently -- tests/test_ensemble_gpu.py) -- same accumulator bits, same sigmoid formula, one rounding to nearest
even -- for every shape at the kernel's edges (256-row slabs, 64-column stages, 32 x 32 tiles, column pairs, 64-element lines),
precision mode, epilogue, 16-bit type and layout (pitched, contiguous, a view at an odd element offset).  The storage around
the tensor is filled with a pattern first and must still hold it afterwards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A
SHAPES = [(1, 1, 1), (33, 31, 2), (256, 64, 1), (257, 65, 2), (300, 129, 3), (511, 130, 2), (40, 1001, 1), (1001, 300, 2),
          (257, 257, 2)]
CASES = [(s, False) for s in SHAPES] + [((257, 257, 2), True)]          # (shape, z_head is z_tail)
PRECISIONS = ["f32", "bf16x3", "bf16", "f16"]
DTYPES = [torch.float16, torch.bfloat16]
GUARD = 67                                                             # elements before the view (odd) and after it

_inputs = {}
_refs = {}


def _ops():
    from madrigal_amd import ops
    return ops


def _make_inputs(shape, same, scale=1.0):
    """z ~ N(0,1) * scale, W ~ N(0,1) / sqrt(128) symmetrised; seeded, made once per case and never modified."""
    key = (shape, same, scale)
    if key not in _inputs:
        Nh, Nt, L = shape
        g = torch.Generator().manual_seed(1000 * Nh + 10 * Nt + L)
        zh = (torch.randn(Nh, 128, generator=g) * scale).cuda()
        zt = zh if same else (torch.randn(Nt, 128, generator=g) * scale).cuda()
        w = _ops().symmetrize((torch.randn(L, 128, 128, generator=g) / 128 ** 0.5).cuda())
        _inputs[key] = (zh, zt, w)
    return _inputs[key]


def _ref32(shape, same, prec, epi, scale=1.0):
    """The parent's fp32 tensor of the general sweep, computed once per (case, precision, epilogue)."""
    key = (shape, same, prec, epi, scale)
    if key not in _refs:
        zh, zt, w = _make_inputs(shape, same, scale)
        _refs[key] = _ops().bilinear_allpairs(zh, zt.clone(), w, precision=prec, epilogue=epi)
    return _refs[key]


def _bits(t):
    return t.view(torch.int16)


def _filled(n, dtype):
    buf = torch.empty(n, dtype=dtype, device="cuda")
    _bits(buf).fill_(PATTERN)
    return buf


def _layouts(L, Nh, Nt, dtype):
    """(name, out tensor, check(): the storage outside the tensor still holds the pattern)."""
    ops = _ops()
    pitched = ops.empty_scores(L, Nh, Nt, "cuda", dtype=dtype)
    store = pitched._base if pitched._base is not None else pitched
    _bits(store).fill_(PATTERN)
    pitch = store.shape[2]
    assert pitch % 64 == 0 and pitched.stride(1) == pitch

    def pad_ok():
        return bool((_bits(store)[:, :, Nt:] == PATTERN).all())

    contig = _filled(L * Nh * Nt, dtype).view(L, Nh, Nt)
    n = L * Nh * Nt
    buf = _filled(GUARD + n + GUARD, dtype)
    view = buf[GUARD:GUARD + n].view(L, Nh, Nt)
    assert view.data_ptr() % 4 == 2                                    # an odd element offset: rows at 2-byte alignment

    def guard_ok():
        b = _bits(buf)
        return bool((b[:GUARD] == PATTERN).all()) and bool((b[GUARD + n:] == PATTERN).all())

    return [("pitched", pitched, pad_ok), ("contiguous", contig, lambda: True), ("odd_offset", view, guard_ok)]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + ("_same" if c[1] else ""))
def test_16bit_tensor_is_the_fp32_tensor_cast(case, prec):
    ops = _ops()
    (Nh, Nt, L), same = case
    zh, zt, w = _make_inputs((Nh, Nt, L), same)
    for epi in (ops.EPI_STORE, ops.EPI_STORE_SIGMOID):
        ref = _ref32((Nh, Nt, L), same, prec, epi)
        for dtype in DTYPES:
            want = ref.to(dtype)
            for name, out, untouched in _layouts(L, Nh, Nt, dtype):
                got = ops.bilinear_allpairs(zh, zt, w, precision=prec, epilogue=epi, out=out)
                assert got is out
                what = f"{name} {dtype} epilogue {epi}"
                assert torch.equal(_bits(got), _bits(want)), what
                assert untouched(), what + ": wrote outside the tensor"
            # out_dtype alone: the pitched layout, same bits
            got = ops.bilinear_allpairs(zh, zt, w, precision=prec, epilogue=epi, out_dtype=dtype)
            assert got.dtype == dtype and got.stride(1) % 64 == 0
            assert torch.equal(_bits(got), _bits(want)), f"out_dtype {dtype} epilogue {epi}"


def test_fp16_overflow_becomes_inf_and_bfloat16_stays_finite():
    ops = _ops()
    shape = (300, 129, 3)
    zh, zt, w = _make_inputs(shape, False, 64.0)
    ref = _ref32(shape, False, "bf16x3", ops.EPI_STORE, 64.0)
    # the premise: entries beyond the half range as well as finite ones
    assert bool((ref.abs() > 65504).any()) and bool((ref.abs() < 60000).any()) and bool(torch.isfinite(ref).all())
    h = ops.bilinear_allpairs(zh, zt, w, precision="bf16x3", out_dtype=torch.float16)
    assert torch.equal(_bits(h), _bits(ref.to(torch.float16)))
    assert bool(torch.isinf(h).any()) and bool(torch.isfinite(h).any())
    b = ops.bilinear_allpairs(zh, zt, w, precision="bf16x3", out_dtype=torch.bfloat16)
    assert bool(torch.isfinite(b).all())
    assert torch.equal(_bits(b), _bits(ref.to(torch.bfloat16)))


class _Scorer(torch.nn.Module):
    """Decoder-only stand-in for NovelDDIMultilabel: score_all_pairs reads ``model.decoder`` only."""

    def __init__(self, M, L, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, L)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)


def test_scorer_forward_passes_out_dtype_through():
    from madrigal_amd import models as M
    model = _Scorer(M, 7, 0).cuda().eval()
    g = torch.Generator().manual_seed(3)
    z, z2 = torch.randn(70, 128, generator=g).cuda(), torch.randn(45, 128, generator=g).cuda()
    with torch.no_grad(), M.precision("bf16x3"):
        want = model.decoder(z, z2, (2, 6)).to(torch.float16)
        got = model.decoder(z, z2, (2, 6), out_dtype=torch.float16)
    assert got.dtype == torch.float16 and tuple(got.shape) == (4, 70, 45)
    assert torch.equal(_bits(got), _bits(want))


def test_score_all_pairs_16bit_host_and_row_sharded_destinations():
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import score_all_pairs
    ops = _ops()
    N, L = 300, 5
    model = _Scorer(M, L, 1).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad(), M.precision("bf16x3"):
        want = model.decoder(z, z.clone()).to(torch.float16)               # the general fp32 sweep, cast
        dev = score_all_pairs(model, z, out_dtype=torch.float16)
        assert dev.dtype == torch.float16 and torch.equal(_bits(dev), _bits(want))
        host = np.empty((L, N, N), np.float16)
        got = score_all_pairs(model, z, out=host, host_chunk=2)
        assert got is host
        assert np.array_equal(host.view(np.int16), dev.cpu().numpy().view(np.int16))
        rows = ops.empty_scores(L, 200 - 37, N, "cuda", dtype=torch.float16)
        got = score_all_pairs(model, z, head_rows=(37, 200), out=rows)
        assert got is rows and torch.equal(_bits(rows), _bits(want[:, 37:200]))
        rows2 = score_all_pairs(model, z, (1, 3), head_rows=(37, 200), out_dtype=torch.bfloat16)
        assert rows2.dtype == torch.bfloat16
        assert torch.equal(_bits(rows2), _bits(model.decoder(z, z.clone(), (1, 3)).to(torch.bfloat16)[:, 37:200]))
        with pytest.raises(ValueError):
            score_all_pairs(model, z, out=np.empty((L, N, N), np.float16), out_dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            score_all_pairs(model, z, out=np.empty((L, N, N), np.float32), out_dtype=torch.float16)


def test_refusals():
    ops = _ops()
    zh, zt, w = _make_inputs((33, 31, 2), False)
    z = zh
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(z, z, w, epilogue=ops.EPI_TRIKEYS, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(zh, zt, w, epilogue=ops.EPI_ROWSTATS, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(zh, zt, w, out_dtype=torch.float16, out=torch.empty(2, 33, 31, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(zh, zt, w, out_dtype=torch.float16, out=torch.empty(2, 33, 31, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(zh, zt, w, out_dtype=torch.float32, out=torch.empty(2, 33, 31, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        ops.bilinear_allpairs(zh, zt, w, out=torch.empty(2, 33, 32, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        ops.rank_normalize(torch.zeros(2, 33, 33, dtype=torch.float16, device="cuda"))
    from madrigal_amd import _lib
    # the C entry point itself: an epilogue without a 16-bit form is MDG_EINVAL with a message
    out = torch.empty(2, 33, 31, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="16-bit"):
        _lib.call("mdg_bilinear_allpairs16_ld", zh.data_ptr(), zt.data_ptr(), w.data_ptr(), out.data_ptr(), 31, 33, 31, 2, 128, ops.PREC_F32,
                  ops.EPI_ROWSTATS, 1, None, 0, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_extents_return_an_empty_tensor(dtype):
    ops = _ops()
    z = torch.randn(5, 128).cuda()
    none = torch.empty(0, 128, device="cuda")
    w = ops.symmetrize(torch.randn(2, 128, 128).cuda())
    for zh, zt, ww, shape in ((z, z, w[:0], (0, 5, 5)), (none, z, w, (2, 0, 5)), (z, none, w, (2, 5, 0))):
        got = ops.bilinear_allpairs(zh, zt, ww, out_dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == shape and got.numel() == 0
