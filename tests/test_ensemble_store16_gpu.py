"""16-bit probability tensors of the checkpoint-ensemble sweep (mdg_bilinear_ensemble_sigmoid16) on the GPU.

Every comparison is exact: the 16-bit tensor must be bit-equal to the fp32 tensor of the SAME call (same lists, same identity of
z_heads / z_tails, so the symmetric sweep is compared with the symmetric sweep) cast afterwards -- same accumulator bits, same
sigmoids summed in model order, one division, one rounding to nearest even -- for every shape at the kernel's edges (128- and
256-row blocks, 64-column tiles, chunks of 6 tiles, column pairs, the diagonal blocks of the symmetric sweep), K = 1 / 2 / 5, both
precisions, both 16-bit types and three layouts (pitched, contiguous, a view at an odd element offset).  The storage around the
tensor is filled with a pattern first and must still hold it afterwards."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A
GENERAL = [(1, 1, 1), (33, 31, 2), (128, 64, 1),
           (129, 65, 2),            # a second row block at K >= 2
           (257, 385, 1),           # 385 = one chunk of 6 tiles + 1 column; a second row block at K = 1
           (40, 1001, 1),           # several chunks, odd ragged end
           (300, 129, 3)]
SYMMETRIC = [1, 2, 33, 129,
             257,                   # odd N, three 128-row blocks: the middle one pairs with itself
             385, 449]
CASES = [(s, False) for s in GENERAL] + [((n, n, 2 if n < 300 else 1), True) for n in SYMMETRIC]      # (shape, z_tails[k] is z_heads[k])
KS = [1, 2, 5]
PRECISIONS = ["f32", "bf16x3"]
DTYPES = [torch.float16, torch.bfloat16]
GUARD = 67                                                             # elements before the view (odd) and after it

_inputs = {}
_refs = {}


def _ops():
    from madrigal_amd import ops
    return ops


def _case_id(c):
    return "x".join(map(str, c[0])) + ("_same" if c[1] else "")


def _make_inputs(shape, K, same, scale=1.0):
    """Per model k: z ~ N(0,1) * scale, W ~ N(0,1) / sqrt(128) symmetrised, its own seed; made once per case and never modified."""
    key = (shape, K, same, scale)
    if key not in _inputs:
        Nh, Nt, L = shape
        zhs, zts, ws = [], [], []
        for k in range(K):
            g = torch.Generator().manual_seed(1000 * Nh + 10 * Nt + L + 100003 * k)
            zh = (torch.randn(Nh, 128, generator=g) * scale).cuda()
            zt = zh if same else (torch.randn(Nt, 128, generator=g) * scale).cuda()
            zhs.append(zh)
            zts.append(zt)
            ws.append(_ops().symmetrize((torch.randn(L, 128, 128, generator=g) / 128 ** 0.5).cuda()))
        _inputs[key] = (zhs, zts, ws)
    return _inputs[key]


def _ref32(shape, K, same, prec, scale=1.0):
    """The fp32 product of the same lists (the symmetric sweep where the 16-bit call takes it), computed once and left unchanged."""
    key = (shape, K, same, prec, scale)
    if key not in _refs:
        zhs, zts, ws = _make_inputs(shape, K, same, scale)
        _refs[key] = _ops().bilinear_ensemble_sigmoid(zhs, zts, ws, precision=prec)
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

    n = L * Nh * Nt
    cbuf = _filled(n + GUARD, dtype)
    contig = cbuf[:n].view(L, Nh, Nt)

    def tail_ok():
        return bool((_bits(cbuf)[n:] == PATTERN).all())

    buf = _filled(GUARD + n + GUARD, dtype)
    view = buf[GUARD:GUARD + n].view(L, Nh, Nt)
    assert view.data_ptr() % 4 == 2                                    # an odd element offset: rows at 2-byte alignment

    def guard_ok():
        b = _bits(buf)
        return bool((b[:GUARD] == PATTERN).all()) and bool((b[GUARD + n:] == PATTERN).all())

    return [("pitched", pitched, pad_ok), ("contiguous", contig, tail_ok), ("odd_offset", view, guard_ok)]


def _compare_all(shape, K, same, prec, scale=1.0):
    ops = _ops()
    Nh, Nt, L = shape
    zhs, zts, ws = _make_inputs(shape, K, same, scale)
    ref = _ref32(shape, K, same, prec, scale)
    for dtype in DTYPES:
        want = ref.to(dtype)
        for name, out, untouched in _layouts(L, Nh, Nt, dtype):
            got = ops.bilinear_ensemble_sigmoid(zhs, zts, ws, precision=prec, out=out)
            assert got is out
            what = f"{name} {dtype}"
            assert torch.equal(_bits(got), _bits(want)), what
            assert untouched(), what + ": wrote outside the tensor"
            if same:
                # exactly symmetric, and the same bits from a second launch
                assert torch.equal(_bits(got), _bits(got.transpose(1, 2))), what + ": not symmetric"
                first = got.clone()
                again = ops.bilinear_ensemble_sigmoid(zhs, zts, ws, precision=prec, out=out)
                assert torch.equal(_bits(again), _bits(first)), what + ": a second launch differs"
        # out_dtype alone: the pitched layout, same bits
        got = ops.bilinear_ensemble_sigmoid(zhs, zts, ws, precision=prec, out_dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == (L, Nh, Nt) and got.stride(1) % 64 == 0
        assert torch.equal(_bits(got), _bits(want)), f"out_dtype {dtype}"


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_16bit_tensor_is_the_fp32_tensor_cast(case, K, prec):
    shape, same = case
    if same:
        ref = _ref32(shape, K, same, prec)
        assert torch.equal(ref, ref.transpose(1, 2))                   # the premise: the fp32 product took its symmetric sweep
    _compare_all(shape, K, same, prec)


@pytest.mark.parametrize("K", [1, 2])
def test_every_rounding_regime_is_hit(K):
    """Checked on the fp32 reference before the comparison: probabilities in the middle, ones whose half is subnormal, ones whose
    half is exactly 1.0 (and, for what it is worth, exact zeros)."""
    shape = (300, 129, 3)
    ref = _ref32(shape, K, False, "bf16x3")
    h = ref.to(torch.float16)
    assert float(((ref > 0.05) & (ref < 0.95)).float().mean()) >= 0.10
    assert int(((h != 0) & (h.abs() < 2.0 ** -14)).sum()) >= 100
    assert int((h == 1.0).sum()) >= 100
    _compare_all(shape, K, False, "bf16x3")


@pytest.mark.parametrize("shape,K,same", [((300, 129, 3), 2, False), ((129, 129, 2), 5, True)])
def test_unsaturated_probabilities(shape, K, same):
    """scale 0.25: every probability inside (0.05, 0.95), where neighbouring halves are 2^-11 .. 2^-15 apart."""
    ref = _ref32(shape, K, same, "bf16x3", 0.25)
    assert float(ref.min()) > 0.05 and float(ref.max()) < 0.95
    _compare_all(shape, K, same, "bf16x3", 0.25)


def test_more_outcomes_and_eight_models():
    """K = 8 (the most) and enough outcomes that the staggered tile order takes several starting points."""
    _compare_all((129, 200, 7), 8, False, "bf16x3")
    _compare_all((200, 200, 7), 8, True, "f32")


def test_refusals_on_the_device():
    ops = _ops()
    zhs, zts, ws = _make_inputs((33, 31, 2), 2, False)
    f = ops.bilinear_ensemble_sigmoid
    with pytest.raises(ValueError):
        f(zhs, zts, ws, out_dtype=torch.float16, out=torch.empty(2, 33, 31, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        f(zhs, zts, ws, out_dtype=torch.float16, out=torch.empty(2, 33, 31, device="cuda"))
    with pytest.raises(ValueError):
        f(zhs, zts, ws, out=torch.empty(2, 33, 32, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        f(zhs, zts, ws, out=torch.empty(2, 33, 64, dtype=torch.float16, device="cuda")[:, :, ::2][:, :, :31])
    with pytest.raises(ValueError):
        f(zhs, zts, ws, out=torch.empty(2, 33, 31, dtype=torch.float16))
    from madrigal_amd import _lib
    import ctypes
    out = torch.empty(2, 33, 31, dtype=torch.float16, device="cuda")
    arr = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])    # noqa: E731
    with pytest.raises(ValueError, match="score type"):
        _lib.call("mdg_bilinear_ensemble_sigmoid16", arr(zhs), arr(zts), arr(ws), 2, out.data_ptr(), 31, 33, 31, 2, 128, ops.PREC_F32, 3,
                  None, 0, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_extents_return_an_empty_tensor(dtype):
    ops = _ops()
    z = torch.randn(5, 128).cuda()
    none = torch.empty(0, 128, device="cuda")
    w = ops.symmetrize(torch.randn(2, 128, 128).cuda())
    for zh, zt, ww, shape in ((z, z, w[:0], (0, 5, 5)), (none, z, w, (2, 0, 5)), (z, none, w, (2, 5, 0))):
        got = ops.bilinear_ensemble_sigmoid([zh, zh], [zt, zt], [ww, ww], out_dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == shape and got.numel() == 0


def _weights_and_embeddings(K, N, L, seed):
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(L, 128, 128, generator=g) / 128 ** 0.5).cuda() for _ in range(K)]
    zs = [torch.randn(N, 128, generator=g).cuda() for _ in range(K)]
    return ws, zs


def test_pipeline_hbm_destinations_with_and_without_index_lists():
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import ensemble_all_pairs, highest_outcomes_of
    ops = _ops()
    K, N, L = 3, 150, 9
    ws, zs = _weights_and_embeddings(K, N, L, 5)
    oi = [7, 2, 2, 8, 0, 5]
    di = [149, 3, 3, 75, 0, 77, 101, 101, 42]
    d2 = [5, 5, 148, 1, 100, 100, 7]
    with M.precision("bf16x3"):
        for kw in ({}, {"drug_inds": di, "outcome_inds": oi}, {"drug_inds": di, "drug_2_inds": d2, "outcome_inds": oi}, {"drug_2_inds": d2}):
            want = ensemble_all_pairs(ws, zs, **kw)
            assert want.dtype == torch.float32
            for dtype in DTYPES:
                got = ensemble_all_pairs(ws, zs, out_dtype=dtype, **kw)
                assert got.dtype == dtype and got.shape == want.shape and got.stride(1) % 64 == 0
                assert torch.equal(_bits(got), _bits(want.to(dtype))), (kw.keys(), dtype)
                into = ops.empty_scores(*want.shape, "cuda", dtype=dtype)
                assert ensemble_all_pairs(ws, zs, out=into, **kw) is into
                assert torch.equal(_bits(into), _bits(got))
        # the 16-bit tensor feeds the "highest-5 mean" path as it is
        p16 = ensemble_all_pairs(ws, zs, out_dtype=torch.float16)
        vals, idx, mean = highest_outcomes_of(p16, 5)
        v32, i32, m32 = highest_outcomes_of(p16.float(), 5)
        assert torch.equal(vals, v32) and torch.equal(idx, i32) and torch.equal(mean, m32)
        with pytest.raises(ValueError):
            ensemble_all_pairs(ws, zs, out=torch.empty(L, N, N, device="cuda"), out_dtype=torch.float16)


@pytest.mark.parametrize("sym", [True, False])
def test_float16_memmap_destination_equals_the_hbm_result(tmp_path, sym):
    """Host destination in 16 bits: outcome chunks of host_chunk (smaller than L, not dividing it) through 16-bit device and pinned
    staging buffers: the bits of the HBM result."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import ensemble_all_pairs
    K, N, L = 2, 131, 11
    ws, zs = _weights_and_embeddings(K, N, L, 9)
    d2 = None if sym else list(range(N - 1, -1, -2))
    with M.precision("bf16x3"):
        dense = ensemble_all_pairs(ws, zs, drug_2_inds=d2, out_dtype=torch.float16)
        assert torch.equal(_bits(dense), _bits(ensemble_all_pairs(ws, zs, drug_2_inds=d2).to(torch.float16)))
        path = os.path.join(tmp_path, "probs16.mmap")
        mm = np.memmap(path, dtype=np.float16, mode="w+", shape=tuple(dense.shape))
        got = ensemble_all_pairs(ws, zs, drug_2_inds=d2, out=mm, host_chunk=4)
        mm.flush()
        assert got is mm
        back = np.memmap(path, dtype=np.float16, mode="r", shape=tuple(dense.shape))
        assert np.array_equal(np.asarray(back).view(np.int16), dense.cpu().numpy().view(np.int16))
        arr = np.empty(tuple(dense.shape), np.float16)
        assert ensemble_all_pairs(ws, zs, drug_2_inds=d2, out=arr, host_chunk=4, out_dtype=torch.float16) is arr
        assert np.array_equal(arr.view(np.int16), dense.cpu().numpy().view(np.int16))
        with pytest.raises(ValueError):
            ensemble_all_pairs(ws, zs, drug_2_inds=d2, out=arr, out_dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            ensemble_all_pairs(ws, zs, drug_2_inds=d2, out=np.empty(tuple(dense.shape), np.float32), out_dtype=torch.float16)
        with pytest.raises(ValueError):
            ensemble_all_pairs(ws, zs, drug_2_inds=d2, out=np.empty((L, N, dense.shape[2] + 1), np.float16))
