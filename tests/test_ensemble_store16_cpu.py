"""16-bit probability tensors of the checkpoint-ensemble sweep (mdg_bilinear_ensemble_sigmoid16, ops.bilinear_ensemble_sigmoid(out_dtype=),
pipeline.ensemble_all_pairs(out_dtype=)): what is decided without a GPU -- the C ABI as the header declares it, the argument checks
that return before any launch (null or made-up pointers throughout: a launch would be an error of its own) and the wrappers'
refusals."""
import ctypes

import numpy as np
import pytest
import torch

NEW = "mdg_bilinear_ensemble_sigmoid16"
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16 = 0, 1, 2, 3
F16, BF16 = 1, 2


def test_the_library_exports_the_symbol_with_the_header_prototype():
    from madrigal_amd import _lib, ops
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    assert NEW in _lib.declared_symbols() and hasattr(L, NEW)
    assert (getattr(L, NEW).restype, list(getattr(L, NEW).argtypes)) == (protos[NEW][0], protos[NEW][1])
    I, I64, Z, P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
    # z_head_host, z_tail_host, w_sym_host, n_models, out, ldo, n_head, n_tail, n_labels, D, precision, score_type, workspace, bytes, stream
    assert protos[NEW] == (I, [P, P, P, I, P, I64, I64, I64, I64, I64, I, I, P, Z, P])
    assert L.mdg_abi_version() >= 30
    assert ops.SCORE_TYPES == {torch.float16: F16, torch.bfloat16: BF16}


def _call(n_models=2, prec=PREC_F32, ty=F16, nh=8, nt=8, nl=2, D=128, ldo=None, ws=None, ws_bytes=0):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_sigmoid16(None, None, None, n_models, None, nt if ldo is None else ldo, nh, nt, nl, D, prec, ty, ws,
                                                 ws_bytes, None)


@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"prec": PREC_F16}, b"not offered"), ({"ty": 0}, b"score type"), ({"ty": 3}, b"score type"),
                                     ({"ldo": 7}, b"row pitch 7 < n_tail 8"), ({"ldo": 1 << 22}, b"too large"),
                                     ({"nh": 1 << 22, "nt": 1 << 22}, b"too large"), ({"D": 64}, b"D must be"),
                                     ({"nl": 65536}, b"n_labels"), ({"nh": -1}, b"negative")])
def test_bad_arguments_are_refused_before_any_launch(kw, word):
    from madrigal_amd._lib import lib
    assert _call(**kw) == -1
    msg = lib().mdg_last_error()
    assert msg.startswith(NEW.encode() + b":") and word in msg, msg


def test_the_largest_pitch_whose_slab_stays_below_2_31_bytes_is_accepted():
    """256 rows x ldo x 2 bytes < 2^31: ldo = 2^22 - 1 passes the size checks (and stops at the null pointers), 2^22 does not."""
    from madrigal_amd._lib import lib
    assert _call(ldo=(1 << 22) - 1) == -1 and b"null pointer" in lib().mdg_last_error()
    assert _call(ldo=1 << 22) == -1 and b"too large" in lib().mdg_last_error()


def test_a_missing_short_or_misaligned_workspace_is_refused_in_bf16x3():
    from madrigal_amd._lib import lib
    L = lib()
    need = L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(8, 8, 2, 128, 2, PREC_BF16X3)
    assert need > 0
    some = ctypes.c_void_p(4096)
    for ws, nbytes in ((None, 0), (some, need - 1), (ctypes.c_void_p(4100), need), (None, need)):
        assert _call(prec=PREC_BF16X3, ws=ws, ws_bytes=nbytes) == -2          # MDG_EWORKSPACE
        assert L.mdg_last_error().startswith(NEW.encode() + b":") and b"workspace" in L.mdg_last_error()
    # the right size passes the workspace check; fp32 needs none
    assert _call(prec=PREC_BF16X3, ws=some, ws_bytes=need) == -1 and b"null pointer" in L.mdg_last_error()
    assert L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(8, 8, 2, 128, 2, PREC_F32) == 0


def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass():
    from madrigal_amd._lib import lib
    L = lib()
    for kw in ({}, {"ty": BF16}, {"n_models": 1}, {"n_models": 8}, {"nl": 65535}, {"ldo": 64}, {"ldo": 9}):
        assert _call(**kw) == -1 and L.mdg_last_error().startswith(NEW.encode() + b":") and b"null pointer" in L.mdg_last_error(), kw
    assert _call(nh=0) == 0
    assert _call(nt=0) == 0
    assert _call(nl=0) == 0
    assert _call(nh=0, ty=7) == -1                 # the enum rules hold for an empty call too


def test_null_model_pointers_alignment_and_an_odd_out_are_checked():
    """Non-null host arrays whose entries are null; then (never dereferenced) made-up addresses: misaligned operands and an ``out``
    at an odd byte address, all of which return before anything is enqueued."""
    from madrigal_amd._lib import lib
    L = lib()
    some = ctypes.c_void_p(4096)
    tail = (8, 8, 8, 2, 128, PREC_F32, F16, None, 0, None)
    null = (ctypes.c_void_p * 2)(None, None)
    assert L.mdg_bilinear_ensemble_sigmoid16(null, null, null, 2, some, *tail) == -1
    assert b"null pointer for model 0" in L.mdg_last_error()
    half = (ctypes.c_void_p * 2)(4096, None)
    assert L.mdg_bilinear_ensemble_sigmoid16(half, half, half, 2, some, *tail) == -1
    assert b"null pointer for model 1" in L.mdg_last_error()
    ok = (ctypes.c_void_p * 2)(4096, 8192)
    assert L.mdg_bilinear_ensemble_sigmoid16(ok, ok, ok, 2, None, *tail) == -1
    assert b"null pointer" in L.mdg_last_error()
    assert L.mdg_bilinear_ensemble_sigmoid16(ok, ok, ok, 2, ctypes.c_void_p(4097), *tail) == -1
    assert b"2-byte aligned" in L.mdg_last_error()
    odd = (ctypes.c_void_p * 2)(4096, 4100)
    for lists in ((odd, ok, ok), (ok, odd, ok), (ok, ok, odd)):
        assert L.mdg_bilinear_ensemble_sigmoid16(*lists, 2, some, *tail) == -1
        assert b"16-byte aligned (model 1)" in L.mdg_last_error()


def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


def test_ops_refuses_a_bad_out_dtype_and_a_mismatch_before_any_device_work():
    from madrigal_amd import ops
    f = ops.bilinear_ensemble_sigmoid
    z, w = _inputs(2)
    for bad in (torch.int8, torch.float64, "float16"):
        with pytest.raises(ValueError, match="out_dtype"):
            f(z, z, w, out_dtype=bad)
    with pytest.raises(ValueError, match="does not match"):
        f(z, z, w, out_dtype=torch.float16, out=torch.zeros(3, 5, 5, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="does not match"):
        f(z, z, w, out_dtype=torch.bfloat16, out=torch.zeros(3, 5, 5))
    with pytest.raises(ValueError, match="does not match"):
        f(z, z, w, out_dtype=torch.float32, out=torch.zeros(3, 5, 5, dtype=torch.float16))
    # the lists are still checked, and CPU tensors still refused, in either 16-bit type
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
            f(z, z[:1], w, out_dtype=dtype)
        with pytest.raises(ValueError, match="precision"):
            f(z, z, w, out_dtype=dtype, precision="bf16")
        with pytest.raises(ValueError, match="GPU"):
            f(z, z, w, out_dtype=dtype)
        with pytest.raises(ValueError, match="GPU"):
            f(z, z, w, out=torch.zeros(3, 5, 5, dtype=dtype))


def test_the_pipeline_refuses_bad_destinations_before_any_device_work():
    from madrigal_amd import pipeline
    f = pipeline.ensemble_all_pairs
    z, w = _inputs(2)
    for bad in (torch.int8, torch.float64):
        with pytest.raises(ValueError, match="out_dtype"):
            f(w, z, out_dtype=bad)
    with pytest.raises(ValueError, match="numpy has no bfloat16"):
        f(w, z, out=np.empty((3, 5, 5), np.float16), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="numpy has no bfloat16"):
        f(w, z, out=np.empty((3, 5, 5), np.float32), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="float32 / float16"):
        f(w, z, out=np.empty((3, 5, 5), np.float64))
    with pytest.raises(ValueError, match="float32 / float16"):
        f(w, z, out=np.empty((3, 5, 5), np.int16), out_dtype=torch.float16)
    with pytest.raises(ValueError, match="does not match"):
        f(w, z, out=np.empty((3, 5, 5), np.float32), out_dtype=torch.float16)
    with pytest.raises(ValueError, match="does not match"):
        f(w, z, out=np.empty((3, 5, 5), np.float16), out_dtype=torch.float32)
    with pytest.raises(ValueError, match="does not match"):
        f(w, z, out=torch.zeros(3, 5, 5), out_dtype=torch.float16)
    # a good 16-bit destination gets as far as the embeddings' device
    with pytest.raises(ValueError, match="GPU"):
        f(w, z, out=np.empty((3, 5, 5), np.float16))
    with pytest.raises(ValueError, match="GPU"):
        f(w, z, out_dtype=torch.bfloat16)
