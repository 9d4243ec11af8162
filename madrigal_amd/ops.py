"""Python wrappers of the C ABI: validate tensors, pass their addresses, sizes and the current HIP stream as plain values
(the header types every entry point, see _lib.py; ``call`` checks the returned status).

torch is used for device memory and streams only; all arithmetic is in libmadrigal_hip.so.
Every wrapper raises ``ValueError`` for bad shapes/dtypes/devices (the reference raises
assertion errors in the same situations) and ``MadrigalHipError`` if the library is missing.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import os
from typing import Optional

import torch

from ._lib import call, lib

PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16 = 0, 1, 2, 3
PRECISIONS = {"f32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16": PREC_BF16}
HEAD_PRECISIONS = dict(PRECISIONS, f16=PREC_F16)          # the all-pairs head also runs on the fp16 matrix cores
EPI_STORE, EPI_STORE_SIGMOID, EPI_ROWSTATS, EPI_TRIKEYS = 0, 1, 2, 3


def _prec(p, names=PRECISIONS) -> int:
    if isinstance(p, str):
        if p not in names:
            raise ValueError(f"unknown precision {p!r}; expected one of {sorted(names)}")
        return names[p]
    return int(p)


_raw_stream_of = torch._C._cuda_getCurrentRawStream      # the current stream's handle without building a torch.cuda.Stream (~1 000 lookups per training step)


def _stream_handle(device) -> int:
    idx = device.index
    return _raw_stream_of(torch.cuda.current_device() if idx is None else idx)


def _stream(t: torch.Tensor) -> int:
    return _stream_handle(t.device)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _f32_cuda(t: torch.Tensor, name: str, ndim: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


_ws_cache = {}


def _workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Per-device grow-only scratch buffer (the C ABI never allocates)."""
    if nbytes == 0:
        return None
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture: scratch from the graph's own pool (a cached buffer would be shared between the replays and
        # whatever eager op later lands on a stream with the same handle)
        return torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
    # one scratch buffer per (device, stream): ops enqueued on different streams may run concurrently
    key = (device.type, device.index, _stream_handle(device))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _scratch(query: str, device, *dims):
    """(scratch buffer | None, its size in bytes) for the launch whose ``*_workspace_bytes`` query is ``query(*dims)``."""
    nbytes = getattr(lib(), query)(*dims)
    return _workspace(nbytes, device), nbytes


# ------------------------------------------------------------------------------- head
def symmetrize(w_original: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """triu(W) + triu(W,1)^T per outcome (madrigal/models/models.py:522-524)."""
    w = _f32_cuda(w_original, "w_original", 3)
    if w.shape[1] != w.shape[2]:
        raise ValueError(f"w_original: expected [L,D,D], got {tuple(w.shape)}")
    out = torch.empty_like(w) if out is None else _f32_cuda(out, "out", 3)
    if out.shape != w.shape:
        raise ValueError("out: shape mismatch")
    call("mdg_symmetrize", _ptr(w), _ptr(out), w.shape[0], w.shape[1], _stream(w))
    return out


SCORE_TYPES = {torch.float16: 1, torch.bfloat16: 2}      # enum mdg_score_type


# ---- what the wrappers of the all-pairs sweeps share, the single-model family and the checkpoint ensemble's alike ----
def _f32_dims(t, name: str, nd: int) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != nd:
        raise ValueError(f"{name}: expected a float32 tensor with {nd} dims, got "
                         f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")


def _eligible_arg(eligible, Nh: int, Nt: int) -> None:
    if eligible not in TOPK_ELIGIBLE:
        raise ValueError(f"unknown eligible {eligible!r}; expected one of {sorted(TOPK_ELIGIBLE)}")
    if eligible != "all" and Nh != Nt:
        raise ValueError(f"eligible={eligible!r} needs one drug set against itself (Nh {Nh} != Nt {Nt})")


_HEAD_OPERANDS = ("z_head", "z_tail", "w_sym")


def _head_models(z_head, z_tail, w_sym, precision, eligible="all", own=()) -> int:
    """What every single-model sweep wrapper checks about its operands, shapes first, on whatever device the tensors live: float32
    tensors of the right rank (the three operands and the product's ``own``: ``(tensor, name, ndim)`` each), one feature dim, the
    eligible and precision names, one drug set under a restricted ``eligible`` -> the precision code.  (``_ensemble_models`` is the
    ensemble's.)"""
    for t, name, nd in (*zip((z_head, z_tail, w_sym), _HEAD_OPERANDS, (2, 2, 3)), *own):
        _f32_dims(t, name, nd)
    D = z_head.shape[1]
    if z_tail.shape[1] != D or w_sym.shape[1] != D or w_sym.shape[2] != D:
        raise ValueError(f"feature dims disagree: z_head {tuple(z_head.shape)}, z_tail {tuple(z_tail.shape)}, w {tuple(w_sym.shape)}")
    _eligible_arg(eligible, z_head.shape[0], z_tail.shape[0])
    return _prec(precision, HEAD_PRECISIONS)


def _head_on_gpu(z_head, z_tail, w_sym, *own):
    """The operands of ``_head_models`` and the product's ``own`` as contiguous fp32 GPU tensors on one device -> [zh, zt, w, *own]."""
    names = (*_HEAD_OPERANDS, *(name for _, name, _ in own))
    ts = [_f32_cuda(t, name, nd) for t, name, nd in (*zip((z_head, z_tail, w_sym), _HEAD_OPERANDS, (2, 2, 3)), *own)]
    if any(t.device != ts[0].device for t in ts):
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} must be on the same device")
    return ts


def _head_calls(product, zh, zt, w, one_call, *query) -> None:
    """All outcomes through a single-model entry point of ``product`` (allpairs, topk, bincount, select), 65 535 per call: the grid's
    y extent.  ``one_call(lo, n, operands, scratch)`` makes the call for the ``n`` outcomes from ``lo`` on; ``operands`` = the three
    pointers, the entry point's first arguments, ``scratch`` = workspace, its size and the stream; ``query``: what the product's
    workspace query takes after D.  (``_ensemble_calls`` is the ensemble's.)"""
    L, D, Nh, Nt = w.shape[0], w.shape[1], zh.shape[0], zt.shape[0]
    for lo in range(0, L, 65535):
        n = min(L, lo + 65535) - lo
        ws, nbytes = _scratch(f"mdg_bilinear_{product}_workspace_bytes", zh.device, Nh, Nt, n, D, *query)
        one_call(lo, n, (_ptr(zh), _ptr(zt), w.data_ptr() + lo * D * D * 4), (_ptr(ws), nbytes, _stream(zh)))


def _call_masked(entry: str, args, mask, mstride: int, lo: int) -> None:
    """``entry``, or ``entry_masked`` with the planes of the outcomes from ``lo`` on (single-model family: two entry points)."""
    if mask is None:
        call(entry, *args)
    else:
        call(entry + "_masked", *args, mask.data_ptr() + lo * mstride * 4, mstride)


def _row_pitched(t: torch.Tensor, Nh: int, Nt: int) -> bool:
    """[L, Nh, Nt] contiguous, or a view of row-padded storage (``empty_scores``): unit inner stride and one pitch for every row."""
    return t.numel() == 0 or (t.stride(2) == 1 and t.stride(1) >= Nt and t.stride(0) == Nh * t.stride(1))


def _topk_k(k) -> None:
    max_k = bilinear_topk_max_k()
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= max_k:
        raise ValueError(f"k: expected an int in 1..{max_k}, got {k!r}")


_TOPK_OUT = (("vals", torch.float32, float("-inf")), ("idx", torch.int32, -1))          # (name, dtype, padding) of a per-row top-k's results


def _topk_out_shapes(out, kinds, shape) -> None:
    """The caller's ``out`` of a per-row top-k, on whatever device it lives: one contiguous tensor of ``shape`` per entry of ``kinds``."""
    if out is None:
        return
    if not (isinstance(out, (tuple, list)) and len(out) == len(kinds)):
        raise ValueError(f"out: expected a ({', '.join(name for name, _, _ in kinds)}) tuple")
    for n, (t, (name, dt, _)) in enumerate(zip(out, kinds)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError(f"out[{n}] ({name}): expected a contiguous {dt} tensor of shape {shape}")


def _topk_results(out, kinds, shape, Nt: int, device):
    """The result tensors of a per-row top-k -- fresh, or the ``out`` that passed ``_topk_out_shapes`` -- on ``device`` ->
    (tensors, done); done: nothing is left to sweep (no entry, or no column at all: every row is padding, written here)."""
    if out is None:
        res = tuple(torch.empty(shape, dtype=dt, device=device) for _, dt, _ in kinds)
    else:
        res = tuple(out)
        for n, t in enumerate(res):
            if not (t.is_cuda and t.device == device):
                raise ValueError(f"out[{n}] ({kinds[n][0]}): must live on the device of the embeddings ({device})")
    if res[0].numel() and Nt == 0:
        for t, (_, _, pad) in zip(res, kinds):
            t.fill_(pad)
    return res, res[0].numel() == 0 or Nt == 0


def _edges_arg(edges: torch.Tensor, L: int, Nt: int, z_tail: str) -> int:
    """``edges`` [L, B] of the counting sweeps, on whatever device they live: their number, the ``z_tail`` rows the 32-bit counters
    hold, finite and ascending values -> B."""
    B, max_edges = edges.shape[1], bilinear_bincount_max_edges()
    if edges.shape[0] != L:
        raise ValueError(f"edges: expected [{L}, B] (one row per outcome), got {tuple(edges.shape)}")
    if not 1 <= B <= max_edges:
        raise ValueError(f"edges: expected 1..{max_edges} edges per outcome, got {B}")
    if Nt >= 1 << 23:
        raise ValueError(f"{z_tail}: {Nt} rows; the 32-bit workgroup counters hold fewer than 2^23")
    if L and not bool(torch.isfinite(edges).all()):
        raise ValueError("edges: must be finite")
    if L and not bool((edges[:, 1:] >= edges[:, :-1]).all()):
        raise ValueError("edges: must be ascending within every outcome (unsorted edges give unspecified counts)")
    return B


def _bincount_call(entry: str, e, counts, mask, mstride: int, Nh: int, Nt: int, D: int, prec: int, eligible: str):
    """``one_call`` of ``_head_calls`` / ``_ensemble_calls`` for the counting sweep ``entry`` over the edges ``e`` [L, B] into
    ``counts`` [L, B+1], or with a ``mask`` ``entry_split`` into ``counts`` [2, L, B+1]."""
    L, B = e.shape

    def one_call(lo, n, operands, scratch):
        sizes = (Nh, Nt, n, D, B, prec, TOPK_ELIGIBLE[eligible])
        if mask is None:
            call(entry, *operands, e.data_ptr() + lo * B * 4, counts.data_ptr() + lo * (B + 1) * 8, *sizes, *scratch)
            return
        part = counts if n == L else torch.empty((2, n, B + 1), dtype=torch.int64, device=e.device)   # [2][this call's outcomes]
        call(entry + "_split", *operands, e.data_ptr() + lo * B * 4, _ptr(part), *sizes, *scratch, mask.data_ptr() + lo * mstride * 4, mstride)
        if part is not counts:
            counts[:, lo:lo + n] = part

    return one_call


_SELECT_NAN = "thresholds: NaN (use -inf to select every eligible pair, +inf to select none)"


def _cuts_own(thresholds, scale):
    return ((thresholds, "thresholds", 1),) + (() if scale is None else ((scale, "scale", 1),))


def _cuts_arg(thresholds, scale, L: int, Nt: int, z_tail: str, w_sym: str, nan_check_on_device: bool, one_call: bool) -> None:
    """``thresholds`` [L] of the selecting sweeps (and the profile's ``scale`` [L]; ``one_call``: its limit of outcomes), on whatever
    device they live.  ``nan_check_on_device=False``: the caller reads the NaN flag of GPU thresholds itself, together with another
    value (one synchronisation instead of two), or leaves it to the library."""
    if one_call and L > 65535:
        raise ValueError(f"{w_sym}: {L} outcomes; one call takes at most 65535 (merge chunks with profile_merge)")
    if thresholds.shape[0] != L:
        raise ValueError(f"thresholds: expected [{L}] (one cut per outcome), got {tuple(thresholds.shape)}")
    if scale is not None and scale.shape[0] != L:
        raise ValueError(f"scale: expected a float32 tensor [{L}] (one per outcome)")
    if Nt >= (1 << 31) - 64:
        raise ValueError(f"{z_tail}: {Nt} rows do not fit the int32 column indices")
    if L and (nan_check_on_device or not thresholds.is_cuda) and bool(torch.isnan(thresholds).any()):
        raise ValueError(_SELECT_NAN)


def _select_counts(L: int, Nh: int, Nt: int, device, out=None):
    """int32 [L, Nh] for a counting sweep, fresh or the caller's ``out`` -> (counts, done); done: nothing is left to sweep (no entry,
    or no column at all: zeros, written here)."""
    if out is None:
        out = torch.empty((L, Nh), dtype=torch.int32, device=device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == device and out.dtype == torch.int32
              and tuple(out.shape) == (L, Nh) and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous int32 GPU tensor of shape {(L, Nh)}")
    if out.numel() and Nt == 0:
        out.zero_()
    return out, out.numel() == 0 or Nt == 0


def _select_csr(what: str, counts: torch.Tensor, thr: torch.Tensor, max_bytes: int, fill):
    """From the counting sweep's ``counts`` [L, Nh] to the CSR of a selection: ``torch.cumsum``, the one host read -- the total ``T``
    and the NaN flag of the thresholds with it --, the ``max_bytes`` refusal, the allocation, and ``fill(row_ptr, cols, vals)``, the
    filling sweep, where anything was selected -> (row_ptr, cols, vals)."""
    dev = counts.device
    row_ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    T = 0
    if counts.shape[0]:
        row_ptr[1:] = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
        T, bad = torch.stack([row_ptr[-1], torch.isnan(thr).any().to(torch.int64)]).tolist()          # the one host read
        if bad:
            raise ValueError(_SELECT_NAN)
    if 8 * T > int(max_bytes):
        raise ValueError(f"{what}: T = {T} selected pairs need {8 * T} bytes, more than max_bytes = {int(max_bytes)}; "
                         "raise the thresholds, pass fewer outcomes per call, or raise max_bytes")
    cols = torch.empty(T, dtype=torch.int32, device=dev)
    vals = torch.empty(T, dtype=torch.float32, device=dev)
    if T:
        fill(row_ptr, cols, vals)
    return row_ptr, cols, vals


def bilinear_allpairs(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, *, precision="bf16x3",
                      epilogue: int = EPI_STORE, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """All-pairs scores S[l,i,j] = z_head[i]^T W_sym[l] z_tail[j]  -> [L,Nh,Nt] fp32
    (or [L,Nh,2] row statistics with ``EPI_ROWSTATS``).  madrigal/models/models.py:537-547.

    ``EPI_TRIKEYS`` (one drug set against itself, ``z_head is z_tail``): an int32 tensor whose strict lower triangle holds the
    order keys of the scores, for ``rank_normalize`` (which reads nothing else); everything above the diagonal blocks is left
    unwritten -- half the store stream of ``EPI_STORE``.

    ``out_dtype`` = ``torch.float16`` / ``torch.bfloat16`` (or an ``out`` of that dtype; ``EPI_STORE`` / ``EPI_STORE_SIGMOID`` only):
    the tensor in 16 bits, rounded once to nearest even inside the head's epilogue -- bit for bit the fp32 result of the general
    sweep ``.to(out_dtype)`` (fp16 overflow becomes +-inf), half the bytes written and no fp32 tensor next to it.  Without ``out``
    it comes in the ``empty_scores(dtype=...)`` layout.  ``z_head is z_tail`` takes the general sweep here (no mirrored store)."""
    if out_dtype is None:
        out_dtype = out.dtype if (isinstance(out, torch.Tensor) and out.dtype in SCORE_TYPES) else torch.float32
    if out_dtype != torch.float32 and out_dtype not in SCORE_TYPES:
        raise ValueError(f"out_dtype: expected torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    narrow = out_dtype in SCORE_TYPES                       # the 16-bit destination (mdg_bilinear_allpairs16_ld)
    if narrow and epilogue not in (EPI_STORE, EPI_STORE_SIGMOID):
        raise ValueError(f"out_dtype {out_dtype}: only EPI_STORE and EPI_STORE_SIGMOID have a 16-bit form (row statistics and "
                         "lower-triangle keys are fp32 / int32 products)")
    if narrow and isinstance(out, torch.Tensor) and out.dtype != out_dtype:
        raise ValueError(f"out: dtype {out.dtype} does not match out_dtype {out_dtype}")
    prec = _head_models(z_head, z_tail, w_sym, precision)
    zh, zt, w = _head_on_gpu(z_head, z_tail, w_sym)
    L, Nh, Nt, D = w.shape[0], zh.shape[0], zt.shape[0], zh.shape[1]
    shape = (L, Nh, 2) if epilogue == EPI_ROWSTATS else (L, Nh, Nt)
    if epilogue == EPI_TRIKEYS:
        out_dtype = torch.int32
    if out is None:
        if narrow:
            out = empty_scores(L, Nh, Nt, zh.device, dtype=out_dtype)
        elif epilogue == EPI_TRIKEYS:
            out = empty_scores(L, Nh, Nt, zh.device).view(torch.int32)
        else:
            out = torch.empty(shape, dtype=torch.float32, device=zh.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == out_dtype):
        raise ValueError(f"out: expected a {out_dtype} GPU tensor")
    elif tuple(out.shape) != shape or not _row_pitched(out, shape[1], shape[2]):
        raise ValueError(f"out: expected {shape}, contiguous or row-pitched (empty_scores), got {tuple(out.shape)} strides {tuple(out.stride())}")
    if narrow and not out.numel():
        return out
    ldo = out.stride(1) if out.numel() else shape[2]
    # the two entry points share the workspace query; the 16-bit one takes the score type too, and its pointer steps in 2-byte elements
    entry, what, elem, kind = (("mdg_bilinear_allpairs16_ld", "", 2, (SCORE_TYPES[out_dtype],)) if narrow else
                               ("mdg_bilinear_allpairs_ld", "mdg_bilinear_allpairs", 4, ()))
    _head_calls("allpairs", zh, zt, w, lambda lo, n, operands, scratch: call(
        entry, *operands, out.data_ptr() + lo * out.stride(0) * elem, ldo, Nh, Nt, n, D, prec, int(epilogue), *kind, *scratch, what=what), prec)
    return out


TOPK_ELIGIBLE = {"all": 0, "not_self": 1, "lower": 2}


# ---- known-pair exclusion masks of the in-sweep products (include/madrigal_hip.h, "Known-pair exclusion masks") ----
def _pair_list(x, name: str, n: int, what: str) -> torch.Tensor:
    """int64 CPU/GPU vector from an index list, every entry in [0, n)."""
    import numpy as np
    if not isinstance(x, torch.Tensor):
        arr = np.asarray(x)
        if arr.size and arr.dtype.kind not in "iu":
            raise ValueError(f"{name}: expected integer indices, got {arr.dtype}")
        x = torch.as_tensor(arr.astype(np.int64))
    t = x
    if t.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"{name}: expected integer indices, got {t.dtype}")
    t = t.long().reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise ValueError(f"{name}: {what} must lie in [0, {n}), got [{int(t.min())}, {int(t.max())}]")
    return t


def pair_mask(heads, tails, n_head: int, n_tail: Optional[int] = None, *, labels=None, n_labels: Optional[int] = None,
              symmetric: bool = False, device=None) -> torch.Tensor:
    """Exclusion mask of the listed pairs for ``bilinear_topk`` / ``bilinear_select_count`` / ``bilinear_select`` (``exclude=``)
    -> int32 GPU tensor ``[P, ceil(n_head / 32), ld]``, ``ld`` = ``n_tail`` rounded up to 64: bit ``i & 31`` of word
    ``[p, i >> 5, j]`` is set when (head row i, tail column j) is listed, and a set bit takes the pair out of the sweep's results.

    ``heads`` / ``tails``: index lists of one length (any order, duplicates allowed; every index is checked here).  ``n_tail``
    defaults to ``n_head`` (one drug set).  ``labels`` (with ``n_labels``): the outcome of every pair -> one plane per outcome,
    ``P = n_labels``; without it ``P = 1``, one plane for all outcomes.  ``symmetric``: (t, h) is excluded with (h, t); needs
    ``n_head == n_tail``.  The bits are set on the device with integer ORs: the result does not depend on the order of the list.
    ``device``: where to build it (default: the lists' device if they are GPU tensors, else the current GPU)."""
    n_tail = n_head if n_tail is None else n_tail
    for v, name in ((n_head, "n_head"), (n_tail, "n_tail")):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name}: expected a non-negative int, got {v!r}")
    if symmetric and n_head != n_tail:
        raise ValueError(f"symmetric=True needs one drug set against itself (n_head {n_head} != n_tail {n_tail})")
    if (labels is None) != (n_labels is None):
        raise ValueError("labels and n_labels go together (one plane per outcome) or are both omitted (one shared plane)")
    P = 1
    if n_labels is not None:
        if isinstance(n_labels, bool) or not isinstance(n_labels, int) or n_labels < 1:
            raise ValueError(f"n_labels: expected a positive int, got {n_labels!r}")
        P = n_labels
    h = _pair_list(heads, "heads", n_head, "head rows")
    t = _pair_list(tails, "tails", n_tail, "tail columns")
    pl = None if labels is None else _pair_list(labels, "labels", P, "outcomes")
    if h.numel() != t.numel() or (pl is not None and pl.numel() != h.numel()):
        raise ValueError("heads, tails (and labels): index lists of one length")
    if device is None:
        device = next((x.device for x in (heads, tails, labels) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda"))
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"device: the mask is built on the GPU, got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    L = lib()
    ld, nrb = L.mdg_pair_mask_ld(n_tail), (n_head + 31) // 32
    mask = torch.zeros((P, nrb, ld), dtype=torch.int32, device=device)
    if h.numel() and mask.numel():
        h, t = h.to(device).contiguous(), t.to(device).contiguous()
        pl = None if pl is None else pl.to(device).contiguous()
        with torch.cuda.device(device):
            call("mdg_pair_mask_set", _ptr(mask), P, n_head, n_tail, _ptr(h), _ptr(t), _ptr(pl), h.numel(), int(bool(symmetric)), _stream(mask))
    return mask


def _mask_planes(mask: torch.Tensor, n_head: int, n_tail: int) -> int:
    """Shape and dtype check of a packed mask against (n_head, n_tail) -> its number of planes.  A pure check (CPU or GPU tensors)."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32:
        raise ValueError(f"exclude: expected an int32 mask from ops.pair_mask, got "
                         f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
    want = ((n_head + 31) // 32, (n_tail + 63) // 64 * 64 if n_tail > 0 else 0)
    if mask.dim() != 3 or tuple(mask.shape[1:]) != want:
        raise ValueError(f"exclude: expected [P, {want[0]}, {want[1]}] for {n_head} head rows and {n_tail} tail columns, got {tuple(mask.shape)}")
    return mask.shape[0]


def pair_mask_dense(mask: torch.Tensor, n_head: int, n_tail: int) -> torch.Tensor:
    """A packed exclusion mask unpacked -> bool ``[P, n_head, n_tail]``, True where the pair is excluded (for re-scoring dense
    rows and for tests).  A pure tensor function (CPU or GPU)."""
    P = _mask_planes(mask, n_head, n_tail)
    shifts = torch.arange(32, dtype=torch.int32, device=mask.device)
    bits = (mask[:, :, None, :] >> shifts[None, None, :, None]) & 1                 # [P, row blocks, 32, ld]
    return bits.reshape(P, -1, mask.shape[2])[:, :n_head, :n_tail].bool()


def pair_mask_rows(mask: torch.Tensor, plane: int, rows: torch.Tensor, n_tail: int) -> torch.Tensor:
    """Rows ``rows`` (int64 indices) of plane ``plane`` of a packed mask -> bool ``[len(rows), n_tail]``: the rows
    ``pair_mask_dense(mask, ...)[plane, rows]`` holds, without unpacking the plane.  A pure tensor function (CPU or GPU)."""
    words = mask[plane].index_select(0, rows >> 5)[:, :n_tail]
    return ((words >> (rows & 31).to(torch.int32)[:, None]) & 1).bool()


def _exclude_args(exclude, zh: torch.Tensor, Nh: int, Nt: int, L: int):
    """``exclude=`` of the in-sweep products -> (contiguous mask | None, plane stride in words)."""
    if exclude is None:
        return None, 0
    P = _mask_planes(exclude, Nh, Nt)
    if not exclude.is_cuda or exclude.device != zh.device:
        raise ValueError(f"exclude: must live on the device of the embeddings ({zh.device}), got {exclude.device}")
    if P != 1 and P != L:
        raise ValueError(f"exclude: {P} planes; expected 1 (shared by all outcomes) or one per outcome ({L})")
    m = exclude if exclude.is_contiguous() else exclude.contiguous()
    return m, (0 if P == 1 else m.shape[1] * m.shape[2])


def bilinear_topk_max_k() -> int:
    """Largest ``k`` of ``bilinear_topk`` (at least 32)."""
    return lib().mdg_bilinear_topk_max_k()


def bilinear_topk(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, k: int, *, eligible: str = "all",
                  precision="bf16x3", out=None, exclude: Optional[torch.Tensor] = None):
    """Per-row top-k of the all-pairs sweep: ``(vals [L,Nh,k] fp32, idx [L,Nh,k] int32)``, for every outcome and head row the
    ``k`` largest scores ``z_head[i]^T W_sym[l] z_tail[j]`` over the eligible tail columns and those columns, ordered by
    (score descending, column ascending); rows with fewer than ``k`` eligible columns are padded with ``-inf`` / ``-1``.
    Nothing of [L,Nh,Nt] is materialised.

    ``eligible``: ``"all"`` (two drug sets), ``"not_self"`` (``j != i``), ``"lower"`` (``j < i``, the strict lower triangle the
    rank normalisation reads; tiles on or above the diagonal are not computed); the last two need ``Nh == Nt``.  The scores
    are those of ``bilinear_allpairs``'s general sweep in the same ``precision`` ("f32" / "bf16x3": bit for bit; "bf16" / "f16":
    the row-statistics sweep, fp32 sums grouped differently, <= 2e-6 of the scale).  ``out``: optional ``(vals, idx)`` pair.

    ``exclude``: a mask from ``pair_mask`` (``[1, ...]`` shared by all outcomes or ``[L, ...]``, one plane per outcome): a pair
    whose bit is set is not eligible, on top of ``eligible`` -- the known interactions of a screening run.  The scores that remain
    and their order are those of the call without it."""
    prec = _head_models(z_head, z_tail, w_sym, precision, eligible)
    _topk_k(k)
    _topk_out_shapes(out, _TOPK_OUT, (w_sym.shape[0], z_head.shape[0], k))
    zh, zt, w = _head_on_gpu(z_head, z_tail, w_sym)
    L, Nh, Nt, D = w.shape[0], zh.shape[0], zt.shape[0], zh.shape[1]
    mask, mstride = _exclude_args(exclude, zh, Nh, Nt, L)
    (vals, idx), done = _topk_results(out, _TOPK_OUT, (L, Nh, k), Nt, zh.device)
    if not done:
        _head_calls("topk", zh, zt, w, lambda lo, n, operands, scratch: _call_masked("mdg_bilinear_topk", (
            *operands, vals.data_ptr() + lo * Nh * k * 4, idx.data_ptr() + lo * Nh * k * 4, Nh, Nt, n, D, prec, int(k), TOPK_ELIGIBLE[eligible],
            *scratch), mask, mstride, lo), prec, int(k))
    return vals, idx


def bilinear_bincount_max_edges() -> int:
    """Largest number of edges per outcome of ``bilinear_bincount`` (at least 1024)."""
    return lib().mdg_bilinear_bincount_max_edges()


def bilinear_bincount(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, edges: torch.Tensor, *, eligible: str = "all",
                      precision="bf16x3", split: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-outcome counts of the all-pairs sweep's scores between edges -> int64 [L, B+1]: with ``edges`` [L, B] fp32, finite and
    ascending per outcome, ``counts[l, b]`` is the number of eligible pairs (i, j) with ``edges[l, b-1] <= S[l,i,j] < edges[l, b]``
    (``edges[l, -1] = -inf``, ``edges[l, B] = +inf``): ``torch.bucketize(S[l], edges[l], right=True)`` followed by a bincount, with
    nothing of [L,Nh,Nt] materialised.  Equal neighbouring edges give an empty bin; every row sums to the number of eligible pairs.

    ``eligible`` and the score arithmetic are those of ``bilinear_topk`` ("f32" / "bf16x3": the general sweep's scores bit for bit;
    "bf16" / "f16": the row-statistics sweep, <= 2e-6 of the scale).  ``1 <= B <= bilinear_bincount_max_edges()``; Nt < 2^23.
    Integer sums: bit-identical from launch to launch.

    ``split``: a mask from ``pair_mask`` (``[1, ...]`` shared by all outcomes or ``[L, ...]``, one plane per outcome) -> int64
    [2, L, B+1]: the same sweep with the two classes counted separately -- ``[0]`` the eligible pairs whose bit is clear, ``[1]``
    those whose bit is set (the known pairs); a bit of an ineligible pair changes nothing.  Nothing is excluded: ``result.sum(0)`` is
    the call without ``split``, exactly, in every precision."""
    # shapes and edge values first (on whatever device the tensors live), then the device: a bad call says what is wrong with it
    own = (edges, "edges", 2)
    prec = _head_models(z_head, z_tail, w_sym, precision, eligible, (own,))
    L, Nh, Nt, D = w_sym.shape[0], z_head.shape[0], z_tail.shape[0], z_head.shape[1]
    B = _edges_arg(edges, L, Nt, "z_tail")
    zh, zt, w, e = _head_on_gpu(z_head, z_tail, w_sym, own)
    mask, mstride = _exclude_args(split, zh, Nh, Nt, L)
    counts = torch.empty((L, B + 1) if split is None else (2, L, B + 1), dtype=torch.int64, device=zh.device)
    _head_calls("bincount", zh, zt, w, _bincount_call("mdg_bilinear_bincount", e, counts, mask, mstride, Nh, Nt, D, prec, eligible), B, prec)
    return counts


def _select_args(z_head, z_tail, w_sym, thresholds, eligible, precision, nan_check_on_device=True, scale=None, one_call=False):
    """Validation shared by ``bilinear_select_count``, ``bilinear_select`` and ``bilinear_profile`` (its ``scale`` and ``one_call``
    limit): shapes and threshold values first (on whatever device the tensors live, ``_cuts_arg``), then the device -> (zh, zt, w,
    thr, scale, precision code)."""
    own = _cuts_own(thresholds, scale)
    prec = _head_models(z_head, z_tail, w_sym, precision, eligible, own)
    forward_only(z_head, z_tail, w_sym, thresholds)
    _cuts_arg(thresholds, scale, w_sym.shape[0], z_tail.shape[0], "z_tail", "w_sym", nan_check_on_device, one_call)
    zh, zt, w, thr, *sc = _head_on_gpu(z_head, z_tail, w_sym, *own)
    return zh, zt, w, thr, (sc[0] if sc else None), prec


def _select_sweep(entry, zh, zt, w, thr, prec, eligible, mask, mstride, outputs) -> None:
    """One pass (``entry``: mdg_bilinear_select_count / _fill) over all outcomes.  ``outputs(lo)``: the pass's own pointer arguments
    for the outcomes from ``lo`` on."""
    Nh, Nt, D = zh.shape[0], zt.shape[0], zh.shape[1]
    _head_calls("select", zh, zt, w, lambda lo, n, operands, scratch: _call_masked(entry, (
        *operands, thr.data_ptr() + lo * 4, *outputs(lo), Nh, Nt, n, D, prec, TOPK_ELIGIBLE[eligible], *scratch), mask, mstride, lo), prec)


def _select_count(zh, zt, w, thr, prec, eligible, mask=None, mstride=0) -> torch.Tensor:
    Nh = zh.shape[0]
    counts, done = _select_counts(w.shape[0], Nh, zt.shape[0], zh.device)
    if not done:
        _select_sweep("mdg_bilinear_select_count", zh, zt, w, thr, prec, eligible, mask, mstride, lambda lo: (counts.data_ptr() + lo * Nh * 4,))
    return counts


def bilinear_select_count(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, thresholds: torch.Tensor, *,
                          eligible: str = "all", precision="bf16x3", exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row sizes of ``bilinear_select`` -> int32 [L, Nh]: ``counts[l, i]`` is the number of eligible tail columns j with
    ``S[l,i,j] >= thresholds[l]``, counted inside the all-pairs sweep (nothing of [L,Nh,Nt] is materialised).  With one drug set and
    ``eligible="not_self"`` this is the degree of drug i in the outcome's predicted network.  ``thresholds``: fp32 [L], no NaN;
    ``-inf`` counts every eligible column, ``+inf`` none.  ``eligible`` and the score arithmetic are those of ``bilinear_topk``.
    ``exclude``: a mask from ``pair_mask`` (one plane or one per outcome); a pair whose bit is set is not counted.
    Deterministic: no atomics."""
    zh, zt, w, thr, _, prec = _select_args(z_head, z_tail, w_sym, thresholds, eligible, precision)
    mask, mstride = _exclude_args(exclude, zh, zh.shape[0], zt.shape[0], w.shape[0])
    return _select_count(zh, zt, w, thr, prec, eligible, mask, mstride)


def bilinear_select(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, thresholds: torch.Tensor, *, eligible: str = "all",
                    precision="bf16x3", max_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """Every eligible pair at or above a per-outcome cut, as CSR -> ``(row_ptr int64 [L*Nh + 1], cols int32 [T], vals fp32 [T])``:
    row ``l * Nh + i`` holds, at ``[row_ptr[r], row_ptr[r + 1])``, the tail columns j with ``S[l,i,j] >= thresholds[l]`` in ascending
    order and those scores.  This is ``torch.nonzero((S >= thresholds[:, None, None]) & eligible_mask)`` of the dense scores, in that
    order, with nothing of [L,Nh,Nt] materialised: a counting sweep (``bilinear_select_count``), ``torch.cumsum``, one host read of the
    total ``T`` to size the result (the thresholds' NaN flag travels with it) -- the only synchronisation -- and a filling sweep.

    ``thresholds``: fp32 [L], no NaN; ``-inf`` selects every eligible pair, ``+inf`` none; the rule is ``>=``, so a cut at the K-th
    best value (``top_pairs``) includes that value, and an edge of ``score_histogram`` selects the bins at and above it.
    ``eligible`` and the score arithmetic are those of ``bilinear_topk`` ("f32" / "bf16x3": the general sweep's scores bit for bit;
    "bf16" / "f16": the row-statistics sweep, <= 2e-6 of the scale).  ``max_bytes``: if the result's 8 T bytes exceed it a ValueError
    naming ``T`` is raised before anything is allocated or filled.  Deterministic: no atomics; bit-identical from call to call.

    ``exclude``: a mask from ``pair_mask`` (one plane or one per outcome); a pair whose bit is set is not eligible, so the known
    network is neither counted nor stored.  What remains is what the call without it returns, minus those pairs."""
    zh, zt, w, thr, _, prec = _select_args(z_head, z_tail, w_sym, thresholds, eligible, precision, nan_check_on_device=False)
    Nh = zh.shape[0]
    mask, mstride = _exclude_args(exclude, zh, Nh, zt.shape[0], w.shape[0])
    counts = _select_count(zh, zt, w, thr, prec, eligible, mask, mstride)          # (a NaN cut selects nothing: harmless until it is refused)
    return _select_csr("bilinear_select", counts, thr, max_bytes, lambda row_ptr, cols, vals: _select_sweep(
        "mdg_bilinear_select_fill", zh, zt, w, thr, prec, eligible, mask, mstride, lambda lo: (row_ptr.data_ptr() + lo * Nh * 8, _ptr(cols), _ptr(vals))))


def _profile_out(out, Nh: int, Nt: int, device):
    """The (count, best, margin) triple of ``bilinear_profile``: fresh row-pitched tensors, or the caller's, checked."""
    dtypes = (torch.int32, torch.int32, torch.float32)
    if out is None:
        pitch = (Nt + 31) // 32 * 32                  # rows on 128-byte lines, as empty_scores (a multiple of 4 elements)
        return tuple(torch.empty((Nh, pitch), dtype=dt, device=device)[:, :Nt] for dt in dtypes)
    if not (isinstance(out, (tuple, list)) and len(out) == 3):
        raise ValueError("out: expected a (count, best, margin) triple")
    for t, dt, name in zip(out, dtypes, ("count", "best", "margin")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == dt and tuple(t.shape) == (Nh, Nt)):
            raise ValueError(f"out: {name} must be a {dt} GPU tensor of shape {(Nh, Nt)} on {device}")
        if t.numel() and (t.stride(1) != 1 or t.stride(0) < Nt or t.stride(0) != out[0].stride(0)):
            raise ValueError(f"out: {name} must be contiguous or row-pitched, with one pitch for all three (strides {tuple(t.stride())})")
    return tuple(out)


def bilinear_profile(z_head: torch.Tensor, z_tail: torch.Tensor, w_sym: torch.Tensor, thresholds: torch.Tensor, *,
                     scale: Optional[torch.Tensor] = None, eligible: str = "all", precision="bf16x3", out=None):
    """Per-pair outcome profile of the all-pairs head -> ``(count int32, best int32, margin fp32)``, each [Nh, Nt]: over the L
    outcomes of ``w_sym``, ``count[i, j]`` = #{l : S[l,i,j] >= thresholds[l]}, ``margin[i, j]`` = max_l (S[l,i,j] - thresholds[l]) *
    scale[l] (a subtract, then a multiply, in fp32) and ``best[i, j]`` the lowest l attaining it -- the sweep reduced over the
    OUTCOMES, with nothing of [L,Nh,Nt] materialised (``mdg_bilinear_profile``: a workgroup holds a tile of pairs and walks l).
    ``scale``: fp32 [L], finite and > 0 (None: ones).  ``thresholds``: fp32 [L], no NaN; with ``-inf`` every eligible pair counts
    and its margin is +inf, with ``+inf`` none does; a pair no outcome moves off ``-inf`` keeps ``best = -1``.  Ineligible pairs
    (``eligible`` as in ``bilinear_topk``) get 0 / -1 / -inf; every entry is written.  The scores are the general sweep's
    (``bilinear_allpairs``) bit for bit in all four precisions.  L <= 65535 per call: merge chunks with ``profile_merge``.
    ``out``: an optional (count, best, margin) triple to reuse, contiguous or with one common row pitch.  The values of
    ``thresholds`` and ``scale`` are checked by the library, which synchronises the stream once.  Deterministic: no atomics."""
    zh, zt, w, thr, sc, prec = _select_args(z_head, z_tail, w_sym, thresholds, eligible, precision, nan_check_on_device=False,
                                            scale=scale, one_call=True)
    L, Nh, Nt, D = w.shape[0], zh.shape[0], zt.shape[0], zh.shape[1]
    res = _profile_out(out, Nh, Nt, zh.device)
    if Nh == 0 or Nt == 0:
        return res
    ws, nbytes = _scratch("mdg_bilinear_profile_workspace_bytes", zh.device, Nh, Nt, L, D, prec)
    call("mdg_bilinear_profile", _ptr(zh), _ptr(zt), _ptr(w), _ptr(thr), _ptr(sc), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]),
         res[0].stride(0), Nh, Nt, L, D, prec, TOPK_ELIGIBLE[eligible], _ptr(ws), nbytes, _stream(zh))
    return res


def profile_merge(a, b, label_offset_b: int):
    """Merge the ``bilinear_profile`` results of two DISJOINT outcome chunks over the same pairs -> ``(count, best, margin)``:
    counts add, the larger margin wins, equal margins keep the lower global outcome.  ``a``'s ``best`` already holds global
    outcome indices; ``b``'s are local to its chunk, whose first outcome is ``label_offset_b``; ``best = -1`` (no outcome moved the
    pair off -inf) stays -1 and never wins a tie.  Pure torch, any device; the arguments are left unchanged."""
    ca, ba, ma = a
    cb, bb, mb = b
    gb = torch.where(bb >= 0, bb + int(label_offset_b), bb)
    take_b = (mb > ma) | ((mb == ma) & (gb >= 0) & ((ba < 0) | (gb < ba)))
    return ca + cb, torch.where(take_b, gb, ba), torch.where(take_b, mb, ma)


OUTCOME_TOPK_MAX_K = 8
_X_TYPES = {torch.float32: 0, **SCORE_TYPES}                # x_type of mdg_outcome_topk_update


def _byte_span(t: torch.Tensor):
    """[first, past-the-last) byte address a strided tensor can touch."""
    last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    if not (a.numel() and b.numel()):
        return False
    (a0, a1), (b0, b1) = _byte_span(a), _byte_span(b)
    return a0 < b1 and b0 < a1


def _per_outcome(t, name: str, Lc: int, device) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (Lc,):
        raise ValueError(f"{name}: expected a float32 tensor [{Lc}] (one per outcome of x)")
    if not t.is_cuda or t.device != device:
        raise ValueError(f"{name}: must live on the device of x ({device}), got {t.device}")
    return t.contiguous()


def outcome_topk(x: torch.Tensor, k: int, *, labels=None, label_base: int = 0, shift: Optional[torch.Tensor] = None,
                 scale: Optional[torch.Tensor] = None, largest: bool = True, eligible: str = "all", state=None):
    """Per-pair top-k over the OUTCOME axis, streamed -> ``(vals fp32, idx int32)``, each [k, Nh, Nt]: the chunk ``x`` [Lc, Nh, Nt]
    (float32, float16 or bfloat16; contiguous, row-pitched as from ``empty_scores``, or any view with unit inner stride -- nothing is
    copied) is folded into a running per-pair sorted list of the k best (value, outcome id).  Slot s of pair (i, j) holds the s-th
    element of everything folded so far under one total order: value descending, then outcome id ascending (``largest=False``:
    value ascending, then id ascending); empty slots hold (-inf, -1) ((+inf, -1)).  The result does not depend on how the outcomes
    are split into calls nor on the order of the calls, and the values are copies: compare with ``torch.equal``.  This is the
    reference's ``np.partition(lst, len(lst)-5)[-5:]`` per drug pair (notebooks/fig5/fig5_t2d_mash.ipynb:1442-1448, 2034-2039) with
    the outcomes attaining it, in ``k * Nh * Nt * 8`` bytes of state plus one chunk.

    ``state``: None -- fresh row-pitched tensors are allocated and ``[:, :, :Nt]`` views returned; or the ``(vals, idx)`` of an
    earlier call, updated in place and returned (its ``k`` must be ``k``).  ``labels``: int32 [Lc] (a list or an int64 tensor is
    converted), the global outcome id of each plane, in any order; a negative label skips the plane.  Without it plane l has id
    ``label_base + l``.  ``shift`` / ``scale``: fp32 [Lc], each optional; the value folded is ``(x - shift[l]) * scale[l]``, a
    subtract, then a multiply, in fp32 (16-bit inputs are widened exactly first).  ``shift`` must be finite and ``scale`` finite and
    > 0: checking that reads two flags back, ONE host synchronisation per call that passes either.  A NaN value is never kept, nor
    is a value equal to the sentinel value.  ``eligible``: ``"all"`` or ``"lower"`` (only i > j; a fresh state gets the sentinels
    elsewhere, an updated state is left untouched there).  Empty Nh, Nt or Lc launches nothing.  Deterministic: no atomics.
    Merge the states of disjoint outcome shards with ``outcome_topk_merge``."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= OUTCOME_TOPK_MAX_K:
        raise ValueError(f"k: expected an int in 1..{OUTCOME_TOPK_MAX_K}, got {k!r}")
    if not isinstance(x, torch.Tensor):
        raise ValueError("x: expected a torch.Tensor")
    if not x.is_cuda:
        raise ValueError(f"x: must live on the GPU (got {x.device}); the HIP path has no CPU fallback")
    if x.dtype not in _X_TYPES:
        raise ValueError(f"x: expected float32, float16 or bfloat16, got {x.dtype}")
    if x.dim() != 3:
        raise ValueError(f"x: expected [Lc, Nh, Nt], got shape {tuple(x.shape)}")
    if eligible not in ("all", "lower"):
        raise ValueError(f"unknown eligible {eligible!r}; expected 'all' or 'lower'")
    Lc, Nh, Nt = x.shape
    if x.numel() and (x.stride(2) != 1 or x.stride(1) < Nt or x.stride(0) < 0):
        raise ValueError(f"x: expected unit inner stride and a row pitch >= Nt (contiguous or row-pitched), got strides {tuple(x.stride())}")
    if isinstance(label_base, bool) or not isinstance(label_base, int) or label_base < 0 or label_base + Lc > 2 ** 31 - 1:
        raise ValueError(f"label_base: outcome ids [{label_base!r}, {label_base!r} + {Lc}) must lie in the int32 range")
    lab = None
    if labels is not None:
        lab = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(labels)
        if lab.dtype not in (torch.int32, torch.int64) or tuple(lab.shape) != (Lc,):
            raise ValueError(f"labels: expected {Lc} integer outcome ids (int32 [Lc]), got {lab.dtype} {tuple(lab.shape)}")
        if lab.dtype == torch.int64:
            if lab.numel() and int(lab.max()) > 2 ** 31 - 1:
                raise ValueError("labels: outcome ids over the int32 range")
            lab = lab.clamp(min=-1).to(torch.int32)
        lab = lab.to(x.device).contiguous()
    sh, sc = _per_outcome(shift, "shift", Lc, x.device), _per_outcome(scale, "scale", Lc, x.device)
    if Lc and (sh is not None or sc is not None):
        ok = [torch.isfinite(t).all() if t is sh else (torch.isfinite(t) & (t > 0)).all() for t in (sh, sc) if t is not None]
        ok = torch.stack(ok).tolist()                      # the one host read
        if sh is not None and not ok[0]:
            raise ValueError("shift: every entry must be finite")
        if sc is not None and not ok[-1]:
            raise ValueError("scale: every entry must be finite and > 0")
    fresh = state is None
    if fresh:
        pitch = (Nt + 31) // 32 * 32                       # rows on 128-byte lines: the pitch rule of _profile_out
        if Lc == 0:
            vals = torch.full((k, Nh, pitch), float("-inf") if largest else float("inf"), dtype=torch.float32, device=x.device)[:, :, :Nt]
            idx = torch.full((k, Nh, pitch), -1, dtype=torch.int32, device=x.device)[:, :, :Nt]
            return vals, idx
        vals = torch.empty((k, Nh, pitch), dtype=torch.float32, device=x.device)[:, :, :Nt]
        idx = torch.empty((k, Nh, pitch), dtype=torch.int32, device=x.device)[:, :, :Nt]
    else:
        if not (isinstance(state, (tuple, list)) and len(state) == 2):
            raise ValueError("state: expected the (vals, idx) pair of an earlier call")
        vals, idx = state
        for t, dt, name in ((vals, torch.float32, "vals"), (idx, torch.int32, "idx")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == x.device and t.dtype == dt and tuple(t.shape) == (k, Nh, Nt)):
                raise ValueError(f"state: {name} must be a {dt} GPU tensor of shape {(k, Nh, Nt)} on {x.device}")
            if t.numel() and (t.stride(2) != 1 or t.stride(1) < Nt or (k > 1 and t.stride(0) < Nh * t.stride(1))):
                raise ValueError(f"state: {name} must be contiguous or row-pitched (strides {tuple(t.stride())})")
        if vals.numel() and vals.stride() != idx.stride():
            raise ValueError(f"state: vals and idx must share one plane stride and one row pitch (strides {tuple(vals.stride())} and "
                             f"{tuple(idx.stride())})")
        if _overlap(vals, x) or _overlap(idx, x) or _overlap(vals, idx):
            raise ValueError("state: vals and idx must not alias x or each other")
    if Nh == 0 or Nt == 0 or Lc == 0:
        return vals, idx
    call("mdg_outcome_topk_update", _ptr(x), _X_TYPES[x.dtype], x.stride(0), x.stride(1), _ptr(lab), label_base, _ptr(sh), _ptr(sc),
         _ptr(vals), _ptr(idx), vals.stride(0), vals.stride(1), Nh, Nt, Lc, k, int(fresh), int(bool(largest)), TOPK_ELIGIBLE[eligible],
         _stream(x))
    return vals, idx


def outcome_topk_merge(a, b, *, largest: bool = True):
    """Merge two ``outcome_topk`` states over DISJOINT outcome sets and the same pairs -> ``(vals, idx)`` [k, Nh, Nt], k that of
    ``a`` (and ``b``): the k best of both under the same total order (value descending -- ascending with ``largest=False``, which must
    be the direction both states were built with --, then outcome id ascending; sentinels last).  For outcome-sharded ranks.
    Pure torch, any device; the arguments are left unchanged."""
    (va, ia), (vb, ib) = a, b
    if va.shape != ia.shape or vb.shape != ib.shape or va.shape != vb.shape:
        raise ValueError(f"outcome_topk_merge: two (vals, idx) states of one shape, got {tuple(va.shape)} / {tuple(ia.shape)} and "
                         f"{tuple(vb.shape)} / {tuple(ib.shape)}")
    k = va.shape[0]
    v, i = torch.cat([va, vb], 0), torch.cat([ia, ib], 0)
    by_id = torch.sort(torch.where(i < 0, torch.full_like(i, 2 ** 31 - 1), i), dim=0, stable=True).indices
    v, i = v.gather(0, by_id), i.gather(0, by_id)
    by_val = torch.sort(v, dim=0, descending=bool(largest), stable=True).indices[:k]
    return v.gather(0, by_val), i.gather(0, by_val)


ENSEMBLE_PRECISIONS ={"f32": PREC_F32, "bf16x3": PREC_BF16X3}


def _ensemble_models(what, z_heads, z_tails, w_syms, precision, eligible="all", own=()):
    """What every ``bilinear_ensemble_*`` wrapper checks about its model lists, shapes first, on whatever device the tensors live:
    1..8 models, three lists of one length, the precision and eligible names, float32 tensors of the right rank (model 0's and the
    product's ``own``: ``(tensor, name, ndim)`` each), every model shaped as model 0, one drug set under a restricted ``eligible``
    -> (zh, zt, ws) as lists."""
    zh, zt, ws = list(z_heads), list(z_tails), list(w_syms)
    K = len(zh)
    if not 1 <= K <= 8:
        raise ValueError(f"{what}: 1..8 models, got {K}")
    if len(zt) != K or len(ws) != K:
        raise ValueError(f"{what}: {K} z_heads, {len(zt)} z_tails, {len(ws)} w_syms")
    if precision not in ENSEMBLE_PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; expected one of {sorted(ENSEMBLE_PRECISIONS)}")
    for t, name, nd in ((zh[0], "z_heads[0]", 2), (zt[0], "z_tails[0]", 2), (ws[0], "w_syms[0]", 3), *own):
        _f32_dims(t, name, nd)
    L, D = ws[0].shape[0], ws[0].shape[1]
    Nh, Nt = zh[0].shape[0], zt[0].shape[0]
    for m in range(K):
        if tuple(zh[m].shape) != (Nh, D) or tuple(zt[m].shape) != (Nt, D) or tuple(ws[m].shape) != (L, D, D):
            raise ValueError(f"{what}: model {m} has z_head {tuple(zh[m].shape)}, z_tail {tuple(zt[m].shape)}, "
                             f"w_sym {tuple(ws[m].shape)}; model 0 has {(Nh, D)}, {(Nt, D)}, {(L, D, D)}")
    _eligible_arg(eligible, Nh, Nt)
    return zh, zt, ws


def _ensemble_on_gpu(what, zh, zt, ws, *own):
    """The lists of ``_ensemble_models`` and the product's ``own`` ``(tensor, name, ndim)`` as contiguous fp32 GPU tensors on one
    device -> (zh, zt, ws, *own)."""
    zh = [_f32_cuda(t, f"z_heads[{m}]", 2) for m, t in enumerate(zh)]
    zt = [_f32_cuda(t, f"z_tails[{m}]", 2) for m, t in enumerate(zt)]
    ws = [_f32_cuda(t, f"w_syms[{m}]", 3) for m, t in enumerate(ws)]
    own = [_f32_cuda(t, name, nd) for t, name, nd in own]
    dev = zh[0].device
    if any(t.device != dev for t in (*zh, *zt, *ws, *own)):
        raise ValueError(f"{what}: every tensor must be on the same device")
    return (zh, zt, ws, *own)


def _ensemble_calls(product, zh, zt, ws, prec, one_call) -> None:
    """All outcomes through an entry point of ``product`` (sigmoid, topk, select, bincount), 65 535 per call: the grid's y extent.
    ``one_call(lo, n, models, scratch)`` makes the call for the ``n`` outcomes from ``lo`` on; ``models`` = the three pointer
    arrays and K, the entry point's first arguments, ``scratch`` = workspace, its size and the stream, the ones after ``precision``
    (and ``eligible``)."""
    K, L, D, Nh, Nt = len(zh), ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    dev = zh[0].device
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    a_h, a_t = arr(zh), arr(zt)
    for lo in range(0, L, 65535):
        n = min(L, lo + 65535) - lo
        wsp, nbytes = _scratch(f"mdg_bilinear_ensemble_{product}_workspace_bytes", dev, Nh, Nt, n, D, K, prec)
        a_w = (ctypes.c_void_p * K)(*[w.data_ptr() + lo * D * D * 4 for w in ws])
        one_call(lo, n, (a_h, a_t, a_w, K), (_ptr(wsp), nbytes, _stream(zh[0])))


def bilinear_ensemble_sigmoid(z_heads, z_tails, w_syms, *, precision="bf16x3", out: Optional[torch.Tensor] = None,
                              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Checkpoint ensemble of the all-pairs head: P[l,i,j] = mean_k sigmoid(z_heads[k][i]^T w_syms[k][l] z_tails[k][j]) -> [L,Nh,Nt]
    fp32 (madrigal/evaluate/predict.py:466-499, 582-614), K = len(z_heads) in 1..8, one launch.  Per model the logit is
    ``bilinear_allpairs``'s own arithmetic in ``precision`` ("f32" or "bf16x3"); the sigmoids are summed in model order and divided
    once by K.  When ``z_heads[k] is z_tails[k]`` for every k (one drug set against itself) the symmetric sweep runs and every
    P[l] is exactly symmetric.  ``out``: None (an ``empty_scores`` tensor) or a contiguous / row-pitched GPU tensor.

    ``out_dtype`` = ``torch.float16`` / ``torch.bfloat16`` (or an ``out`` of that dtype): the tensor in 16 bits, rounded once to
    nearest even inside the sweep (mdg_bilinear_ensemble_sigmoid16) -- bit for bit the fp32 result of the same call
    ``.to(out_dtype)``, symmetric sweep and exact symmetry included, with half the bytes written and no fp32 tensor next to it.
    Without ``out`` it comes in the ``empty_scores(dtype=...)`` layout; a view at an odd element offset or with an odd pitch is
    written correctly by 2-byte stores, slower."""
    what = "bilinear_ensemble_sigmoid"
    if out_dtype is None:
        out_dtype = out.dtype if (isinstance(out, torch.Tensor) and out.dtype in SCORE_TYPES) else torch.float32
    if out_dtype != torch.float32 and out_dtype not in SCORE_TYPES:
        raise ValueError(f"out_dtype: expected torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    if isinstance(out, torch.Tensor) and out.dtype != out_dtype:
        raise ValueError(f"out: dtype {out.dtype} does not match out_dtype {out_dtype}")
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision)
    sym = all(a is b for a, b in zip(zh, zt))
    zh, zt, ws = _ensemble_on_gpu(what, zh, zt, ws)
    if sym:
        zt = zh                                    # the library tells the symmetric sweep by the pointers
    L, D, Nh, Nt = ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    dev = zh[0].device
    shape = (L, Nh, Nt)
    if out is None:
        out = empty_scores(L, Nh, Nt, dev, dtype=out_dtype)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == out_dtype and tuple(out.shape) == shape
              and _row_pitched(out, Nh, Nt)):
        raise ValueError(f"out: expected a {str(out_dtype).replace('torch.', '')} GPU tensor {shape}, contiguous or row-pitched (empty_scores)")
    ldo = out.stride(1) if out.numel() else Nt
    prec = ENSEMBLE_PRECISIONS[precision]
    if out_dtype == torch.float32:
        _ensemble_calls("sigmoid", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
            "mdg_bilinear_ensemble_sigmoid", *models, out.data_ptr() + lo * out.stride(0) * 4, ldo, Nh, Nt, n, D, prec, *scratch))
    else:                                          # the same workspace query; the pointer steps in bytes of the 16-bit type
        _ensemble_calls("sigmoid", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
            "mdg_bilinear_ensemble_sigmoid16", *models, out.data_ptr() + lo * out.stride(0) * 2, ldo, Nh, Nt, n, D, prec,
            SCORE_TYPES[out_dtype], *scratch))
    return out


def bilinear_ensemble_topk_chunk_tiles() -> int:
    """The 64-column tail tiles ``bilinear_ensemble_topk`` sweeps between two rebuilds of the models' z_head . W_sym products."""
    return lib().mdg_bilinear_ensemble_topk_chunk_tiles()


def bilinear_ensemble_topk(z_heads, z_tails, w_syms, k: int, *, eligible: str = "all", precision="bf16x3", out=None,
                           exclude: Optional[torch.Tensor] = None):
    """Per-row top-k of the checkpoint ensemble: ``(vals [L,Nh,k] fp32, idx [L,Nh,k] int32)``, for every outcome and head row the
    ``k`` largest P[l,i,j] = mean_m sigmoid(z_heads[m][i]^T w_syms[m][l] z_tails[m][j]) over the eligible tail columns and those
    columns, ordered by (P descending, column ascending); rows with fewer than ``k`` eligible columns are padded with ``-inf`` /
    ``-1``.  Nothing of [L,Nh,Nt] is materialised (madrigal/evaluate/predict.py:466-499, 582-614 average the sigmoids; the mean is
    not monotone in any one model's logit, so ``bilinear_topk`` per model cannot give this ranking).

    K = len(z_heads) in 1..8.  P is bit for bit what ``bilinear_ensemble_sigmoid``'s general sweep writes in the same
    ``precision`` ("f32" or "bf16x3") -- the sweep it runs when the head is not the tail object, e.g. a row subset.  ``eligible``,
    ``k``, ``out`` and ``exclude`` as ``bilinear_topk``."""
    what = "bilinear_ensemble_topk"
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision, eligible)
    _topk_k(k)
    L, D, Nh, Nt = ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    _topk_out_shapes(out, _TOPK_OUT, (L, Nh, k))
    zh, zt, ws = _ensemble_on_gpu(what, zh, zt, ws)
    mask, mstride = _exclude_args(exclude, zh[0], Nh, Nt, L)
    (vals, idx), done = _topk_results(out, _TOPK_OUT, (L, Nh, k), Nt, zh[0].device)
    if not done:
        prec = ENSEMBLE_PRECISIONS[precision]
        _ensemble_calls("topk", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
            "mdg_bilinear_ensemble_topk", *models, vals.data_ptr() + lo * Nh * k * 4, idx.data_ptr() + lo * Nh * k * 4, Nh, Nt, n, D, prec, int(k),
            TOPK_ELIGIBLE[eligible], *scratch, None if mask is None else mask.data_ptr() + lo * mstride * 4, mstride))
    return vals, idx


def bilinear_ensemble_spread_chunk_tiles() -> int:
    """The 64-column tail tiles ``bilinear_ensemble_spread`` and ``bilinear_ensemble_spread_topk`` sweep between two rebuilds of the
    models' z_head . W_sym products (fewer than ``bilinear_ensemble_topk_chunk_tiles``: three registers of state per element)."""
    return lib().mdg_bilinear_ensemble_spread_chunk_tiles()


def _kappa(kappa, what: str) -> float:
    """``kappa`` of the confidence bound as a Python float: a finite Python or numpy real that stays finite in fp32."""
    if isinstance(kappa, bool) or not isinstance(kappa, numbers.Real) or not math.isfinite(kappa) or abs(float(kappa)) > 3.4028234663852886e38:
        raise ValueError(f"{what}: kappa must be a finite real number (fp32 range), got {kappa!r}")
    return float(kappa)


def bilinear_ensemble_spread(z_heads, z_tails, w_syms, *, kappa=None, precision="bf16x3", out=None):
    """Mean and spread of the checkpoint ensemble -> ``(mean, std)``, or ``(mean, std, bound)`` when ``kappa`` is given, each
    [L,Nh,Nt] fp32: over the K = len(z_heads) in 1..8 probabilities p_m = sigmoid(z_heads[m][i]^T w_syms[m][l] z_tails[m][j]),
    ``mean`` = their mean, ``std`` = their population standard deviation (ddof = 0, ``np.stack(...).std(0)``) and ``bound`` =
    fmaf(kappa, std, mean), one rounding.  madrigal/evaluate/predict.py:466-499, 582-614 keep every checkpoint's tensor before they
    average; the reference has no std call of its own, one takes it from those stored tensors.  Here they never exist: one sweep,
    the second moment kept in registers beside the running sum (``mdg_bilinear_ensemble_spread``).

    ``mean`` is bit for bit ``bilinear_ensemble_sigmoid``'s general-sweep tensor in ``precision`` ("f32" or "bf16x3"); this product
    always runs the general sweep.  ``std`` comes from Welford's recurrence in fp32, which does not cancel: >= 0, never NaN for
    finite logits, exactly 0 for K = 1 and for K equal probabilities.  ``out``: None (``empty_scores`` tensors) or a tuple
    (mean, std) / (mean, std, bound) to reuse -- contiguous or row-pitched fp32 GPU tensors with ONE common pitch; a ``None`` entry
    skips that tensor (it is returned as None), at least one must be given."""
    what = "bilinear_ensemble_spread"
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision)
    n_out = 2 if kappa is None else 3
    kap = 0.0 if kappa is None else _kappa(kappa, what)
    L, D, Nh, Nt = ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    shape = (L, Nh, Nt)
    names = ("mean", "std", "bound")[:n_out]
    if out is not None:
        if not (isinstance(out, (tuple, list)) and len(out) == n_out):
            raise ValueError(f"out: expected a ({', '.join(names)}) tuple")
        if all(t is None for t in out):
            raise ValueError("out: at least one tensor must be given")
        for t, name in zip(out, names):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape):
                raise ValueError(f"out ({name}): expected a float32 tensor of shape {shape}")
    zh, zt, ws = _ensemble_on_gpu(what, zh, zt, ws)
    dev = zh[0].device
    if out is None:
        res = [empty_scores(L, Nh, Nt, dev) for _ in names]
    else:
        res = list(out)
        for t, name in zip(res, names):
            if t is not None and not (t.is_cuda and t.device == dev and _row_pitched(t, Nh, Nt)):
                raise ValueError(f"out ({name}): expected a GPU tensor on {dev}, contiguous or row-pitched (empty_scores)")
    given = [t for t in res if t is not None]
    if given[0].numel() and any(t.stride(1) != given[0].stride(1) for t in given):
        raise ValueError("out: the tensors must share one row pitch")
    if given[0].numel() == 0:
        return tuple(res)
    ldo, s0 = given[0].stride(1), given[0].stride(0)
    prec = ENSEMBLE_PRECISIONS[precision]
    at = lambda t, lo: None if t is None else t.data_ptr() + lo * s0 * 4    # noqa: E731
    _ensemble_calls("spread", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
        "mdg_bilinear_ensemble_spread", *models, at(res[0], lo), at(res[1], lo), at(res[2], lo) if n_out == 3 else None, kap, ldo, Nh, Nt, n, D,
        prec, *scratch))
    return tuple(res)


def bilinear_ensemble_spread_topk(z_heads, z_tails, w_syms, k: int, kappa, *, eligible: str = "all", precision="bf16x3", out=None,
                                  exclude: Optional[torch.Tensor] = None):
    """Per-row top-k of the checkpoint ensemble under a confidence bound -> ``(bound [L,Nh,k] fp32, idx [L,Nh,k] int32, mean
    [L,Nh,k] fp32, std [L,Nh,k] fp32)``: for every outcome and head row the ``k`` eligible tail columns with the largest
    bound = fmaf(kappa, std, mean) of ``bilinear_ensemble_spread``, ordered by (bound descending, column ascending), with each kept
    column's own mean and std; rows with fewer than ``k`` eligible columns are padded with ``-inf`` / ``-1`` / NaN / NaN.
    ``kappa < 0`` ranks by a lower confidence bound (hits the seeds agree on), ``kappa > 0`` by an upper bound (contested pairs),
    ``kappa = 0`` gives ``bilinear_ensemble_topk``'s lists bit for bit.  The bound is not monotone in the mean, so no composition
    of the mean's lists gives this ranking; nothing of [L,Nh,Nt] is materialised (``mdg_bilinear_ensemble_spread_topk``; the
    per-checkpoint tensors of madrigal/evaluate/predict.py:466-499, 582-614, from which the reference's users take a std, never
    exist here).

    Bound, mean and std are bit for bit the dense product's at ``idx``.  ``eligible``, ``k``, ``out`` (a 4-tuple to reuse) and
    ``exclude`` as ``bilinear_ensemble_topk``."""
    what = "bilinear_ensemble_spread_topk"
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision, eligible)
    _topk_k(k)
    kap = _kappa(kappa, what)
    L, D, Nh, Nt = ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    nan = float("nan")
    kinds = (("bound", torch.float32, float("-inf")), ("idx", torch.int32, -1), ("mean", torch.float32, nan), ("std", torch.float32, nan))
    _topk_out_shapes(out, kinds, (L, Nh, k))
    zh, zt, ws = _ensemble_on_gpu(what, zh, zt, ws)
    mask, mstride = _exclude_args(exclude, zh[0], Nh, Nt, L)
    res, done = _topk_results(out, kinds, (L, Nh, k), Nt, zh[0].device)
    if not done:
        bound, idx, mean, std = res
        prec = ENSEMBLE_PRECISIONS[precision]
        step = Nh * k * 4
        _ensemble_calls("spread", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
            "mdg_bilinear_ensemble_spread_topk", *models, kap, bound.data_ptr() + lo * step, idx.data_ptr() + lo * step,
            mean.data_ptr() + lo * step, std.data_ptr() + lo * step, Nh, Nt, n, D, prec, int(k), TOPK_ELIGIBLE[eligible], *scratch,
            None if mask is None else mask.data_ptr() + lo * mstride * 4, mstride))
    return res


def _ensemble_select_args(what, z_heads, z_tails, w_syms, thresholds, eligible, precision, nan_check_on_device=True, scale=None, one_call=False):
    """``_select_args`` of the ensemble, for ``bilinear_ensemble_select_count``, ``bilinear_ensemble_select`` and
    ``bilinear_ensemble_profile`` -> (zh, zt, ws, thr, scale, precision code)."""
    own = _cuts_own(thresholds, scale)
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision, eligible, own)
    forward_only(*zh, *zt, *ws, thresholds)
    _cuts_arg(thresholds, scale, ws[0].shape[0], zt[0].shape[0], "z_tails", "w_syms", nan_check_on_device, one_call)
    zh, zt, ws, thr, *sc = _ensemble_on_gpu(what, zh, zt, ws, *own)
    return zh, zt, ws, thr, (sc[0] if sc else None), ENSEMBLE_PRECISIONS[precision]


def _ensemble_select_sweep(entry, zh, zt, ws, thr, prec, eligible, mask, mstride, outputs) -> None:
    """``_select_sweep`` of the ensemble (``entry``: mdg_bilinear_ensemble_select_count / _fill; one entry point, the mask optional)."""
    Nh, Nt, D = zh[0].shape[0], zt[0].shape[0], ws[0].shape[1]
    _ensemble_calls("select", zh, zt, ws, prec, lambda lo, n, models, scratch: call(
        entry, *models, thr.data_ptr() + lo * 4, *outputs(lo), Nh, Nt, n, D, prec, TOPK_ELIGIBLE[eligible], *scratch,
        None if mask is None else mask.data_ptr() + lo * mstride * 4, mstride))


def _ensemble_select_count(zh, zt, ws, thr, prec, eligible, mask, mstride, out=None) -> torch.Tensor:
    Nh = zh[0].shape[0]
    counts, done = _select_counts(ws[0].shape[0], Nh, zt[0].shape[0], zh[0].device, out)
    if not done:
        _ensemble_select_sweep("mdg_bilinear_ensemble_select_count", zh, zt, ws, thr, prec, eligible, mask, mstride,
                               lambda lo: (counts.data_ptr() + lo * Nh * 4,))
    return counts


def bilinear_ensemble_select_count(z_heads, z_tails, w_syms, thresholds: torch.Tensor, *, eligible: str = "all", precision="bf16x3",
                                   exclude: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row sizes of ``bilinear_ensemble_select`` -> int32 [L, Nh]: ``counts[l, i]`` is the number of eligible tail columns j with
    P[l,i,j] = mean_m sigmoid(z_heads[m][i]^T w_syms[m][l] z_tails[m][j]) ``>= thresholds[l]``, counted inside the ensemble's
    all-pairs sweep (nothing of [L,Nh,Nt] is materialised; madrigal/evaluate/predict.py:466-499, 582-614 average the sigmoids).
    With one drug set and ``eligible="not_self"`` this is the degree of drug i in the network the ensemble predicts for the outcome.

    K = len(z_heads) in 1..8; P is bit for bit ``bilinear_ensemble_sigmoid``'s general sweep in ``precision`` ("f32" or "bf16x3").
    ``thresholds``: fp32 [L] probabilities, no NaN; ``-inf`` (or 0.0) counts every eligible column, ``+inf`` none.  ``eligible`` and
    ``exclude`` as ``bilinear_select_count``.  ``out``: optional contiguous int32 [L, Nh] GPU tensor; every entry is written, zeros
    included.  Deterministic: no atomics."""
    zh, zt, ws, thr, _, prec = _ensemble_select_args("bilinear_ensemble_select_count", z_heads, z_tails, w_syms, thresholds, eligible, precision)
    mask, mstride = _exclude_args(exclude, zh[0], zh[0].shape[0], zt[0].shape[0], ws[0].shape[0])
    return _ensemble_select_count(zh, zt, ws, thr, prec, eligible, mask, mstride, out)


def bilinear_ensemble_select(z_heads, z_tails, w_syms, thresholds: torch.Tensor, *, eligible: str = "all", precision="bf16x3",
                             max_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """Every eligible pair the checkpoint ensemble rates at or above a per-outcome probability cut, as CSR -> ``(row_ptr int64
    [L*Nh + 1], cols int32 [T], vals fp32 [T])``: row ``l * Nh + i`` holds, at ``[row_ptr[r], row_ptr[r + 1])``, the tail columns j
    with P[l,i,j] = mean_m sigmoid(z_heads[m][i]^T w_syms[m][l] z_tails[m][j]) ``>= thresholds[l]`` in ascending order and those
    probabilities.  This is ``torch.nonzero((P >= thresholds[:, None, None]) & eligible_mask)`` of ``bilinear_ensemble_sigmoid``'s
    dense result, in that order, with nothing of [L,Nh,Nt] materialised: ``bilinear_select``'s flow -- a counting sweep,
    ``torch.cumsum``, one host read of the total ``T`` (the thresholds' NaN flag travels with it), a filling sweep.  The mean of K
    sigmoids is not monotone in any one model's logit, so no combination of ``bilinear_select`` results per model gives this set.

    K = len(z_heads) in 1..8; P is bit for bit the general sweep's of ``bilinear_ensemble_sigmoid`` in ``precision`` ("f32" or
    "bf16x3").  ``thresholds``: fp32 [L], no NaN; the rule is ``>=``, so a cut at the K-th best probability includes every tie with
    it (at saturated inputs many probabilities are exactly 1.0).  ``eligible``, ``max_bytes`` and ``exclude`` as ``bilinear_select``.
    Deterministic: no atomics; bit-identical from call to call."""
    what = "bilinear_ensemble_select"
    zh, zt, ws, thr, _, prec = _ensemble_select_args(what, z_heads, z_tails, w_syms, thresholds, eligible, precision, nan_check_on_device=False)
    Nh = zh[0].shape[0]
    mask, mstride = _exclude_args(exclude, zh[0], Nh, zt[0].shape[0], ws[0].shape[0])
    counts = _ensemble_select_count(zh, zt, ws, thr, prec, eligible, mask, mstride)      # (a NaN cut selects nothing: harmless until it is refused)
    return _select_csr(what, counts, thr, max_bytes, lambda row_ptr, cols, vals: _ensemble_select_sweep(
        "mdg_bilinear_ensemble_select_fill", zh, zt, ws, thr, prec, eligible, mask, mstride,
        lambda lo: (row_ptr.data_ptr() + lo * Nh * 8, _ptr(cols), _ptr(vals))))


def bilinear_ensemble_bincount(z_heads, z_tails, w_syms, edges: torch.Tensor, *, eligible: str = "all", precision="bf16x3",
                               split: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-outcome counts of the checkpoint ensemble's probabilities between edges -> int64 [L, B+1]: with ``edges`` [L, B] fp32,
    finite and ascending per outcome, ``counts[l, b]`` is the number of eligible pairs (i, j) with ``edges[l, b-1] <= P[l,i,j] <
    edges[l, b]`` (``edges[l, -1] = -inf``, ``edges[l, B] = +inf``), P[l,i,j] = mean_m sigmoid(z_heads[m][i]^T w_syms[m][l]
    z_tails[m][j]): ``torch.bucketize(P[l], edges[l], right=True)`` followed by a bincount, counted inside the ensemble's all-pairs
    sweep with nothing of [L,Nh,Nt] materialised (madrigal/evaluate/predict.py:466-499, 582-614 average the sigmoids;
    notebooks/normalize_scores.py:36-74 ranks that tensor).  Equal neighbouring edges give an empty bin; every row sums to the number
    of eligible pairs.  The mean of K sigmoids is not monotone in any one model's logit, so no combination of ``bilinear_bincount``
    results per model gives these counts.

    K = len(z_heads) in 1..8; P is bit for bit ``bilinear_ensemble_sigmoid``'s general sweep in ``precision`` ("f32" or "bf16x3"),
    the value ``bilinear_ensemble_topk`` and ``bilinear_ensemble_select`` return, so their values can serve as edges.  ``eligible``
    as ``bilinear_topk``; ``1 <= B <= bilinear_bincount_max_edges()``; Nt < 2^23.  Integer sums: bit-identical from launch to launch.

    ``split``: a mask from ``pair_mask`` (``[1, ...]`` shared by all outcomes or ``[L, ...]``, one plane per outcome) -> int64
    [2, L, B+1]: the same sweep with the two classes counted separately -- ``[0]`` the eligible pairs whose bit is clear, ``[1]``
    those whose bit is set (the known pairs); a bit of an ineligible pair changes nothing.  Nothing is excluded: ``result.sum(0)`` is
    the call without ``split``, exactly."""
    what = "bilinear_ensemble_bincount"
    # shapes and edge values first (on whatever device the tensors live), then the device: a bad call says what is wrong with it
    own = (edges, "edges", 2)
    zh, zt, ws = _ensemble_models(what, z_heads, z_tails, w_syms, precision, eligible, (own,))
    forward_only(*zh, *zt, *ws, edges)
    L, D, Nh, Nt = ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    B = _edges_arg(edges, L, Nt, "z_tails")
    zh, zt, ws, e = _ensemble_on_gpu(what, zh, zt, ws, own)
    prec = ENSEMBLE_PRECISIONS[precision]
    mask, mstride = _exclude_args(split, zh[0], Nh, Nt, L)
    counts = torch.empty((L, B + 1) if split is None else (2, L, B + 1), dtype=torch.int64, device=zh[0].device)
    if counts.numel() == 0:
        return counts
    if Nh == 0 or Nt == 0:                       # no pair at all
        return counts.zero_()
    _ensemble_calls("bincount", zh, zt, ws, prec, _bincount_call("mdg_bilinear_ensemble_bincount", e, counts, mask, mstride, Nh, Nt, D, prec, eligible))
    return counts


def bilinear_ensemble_profile_tiles() -> int:
    """The 64-column tail tiles a workgroup of ``bilinear_ensemble_profile`` owns (its column groups are this many tiles wide)."""
    return lib().mdg_bilinear_ensemble_profile_tiles()


def bilinear_ensemble_profile(z_heads, z_tails, w_syms, thresholds: torch.Tensor, *, scale: Optional[torch.Tensor] = None,
                              eligible: str = "all", precision="bf16x3", out=None):
    """Per-pair outcome profile of the checkpoint ensemble -> ``(count int32, best int32, margin fp32)``, each [Nh, Nt]: over the L
    outcomes, with P[l,i,j] = mean_m sigmoid(z_heads[m][i]^T w_syms[m][l] z_tails[m][j]), ``count[i, j]`` = #{l : P[l,i,j] >=
    thresholds[l]}, ``margin[i, j]`` = max_l (P[l,i,j] - thresholds[l]) * scale[l] (a subtract, then a multiply, in fp32) and
    ``best[i, j]`` the lowest l attaining it -- ``bilinear_profile``'s contract on the probability madrigal/evaluate/predict.py:
    466-499, 582-614 average over the checkpoints, reduced over the OUTCOMES inside the ensemble's sweep with nothing of [L,Nh,Nt]
    materialised (``mdg_bilinear_ensemble_profile``).  The mean of K sigmoids is not monotone in any one model's logit, so K
    ``bilinear_profile`` results cannot be merged into this.

    K = len(z_heads) in 1..8; P is bit for bit ``bilinear_ensemble_sigmoid``'s general sweep in ``precision`` ("f32" or "bf16x3").
    ``thresholds``: fp32 [L] probabilities, no NaN (``-inf`` flags every eligible pair with margin +inf, ``+inf`` none); ``scale``:
    fp32 [L], finite and > 0 (None: ones).  Exact ties of the margin are common -- many probabilities round to exactly 1 -- and keep
    the lowest outcome; a pair no outcome moves off ``-inf`` keeps ``best = -1``.  Ineligible pairs (``eligible`` as in
    ``bilinear_topk``) get 0 / -1 / -inf; every entry is written.  L <= 65535 per call: merge chunks with ``profile_merge``.
    ``out``: an optional (count, best, margin) triple to reuse, contiguous or with one common row pitch.  The values of
    ``thresholds`` and ``scale`` are checked by the library, which synchronises the stream once.  Deterministic: no atomics."""
    what = "bilinear_ensemble_profile"
    if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 3):
        raise ValueError("out: expected a (count, best, margin) triple")
    zh, zt, ws, thr, sc, prec = _ensemble_select_args(what, z_heads, z_tails, w_syms, thresholds, eligible, precision, nan_check_on_device=False,
                                                      scale=scale, one_call=True)
    K, L, D, Nh, Nt = len(zh), ws[0].shape[0], ws[0].shape[1], zh[0].shape[0], zt[0].shape[0]
    dev = zh[0].device
    res = _profile_out(out, Nh, Nt, dev)
    if Nh == 0 or Nt == 0:
        return res
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    wsp, nbytes = _scratch("mdg_bilinear_ensemble_profile_workspace_bytes", dev, Nh, Nt, L, D, K, prec)
    call("mdg_bilinear_ensemble_profile", arr(zh), arr(zt), arr(ws), K, _ptr(thr), _ptr(sc), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]),
         res[0].stride(0), Nh, Nt, L, D, prec, TOPK_ELIGIBLE[eligible], _ptr(wsp), nbytes, _stream(zh[0]))
    return res


def empty_scores(L: int, Nh: int, Nt: int, device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """An uninitialised [L,Nh,Nt] fp32 score (or rank) tensor in the layout the head writes fastest: rows padded to a multiple of
    32 floats, so that every row starts on a 128-byte line whatever Nt is (the real drug counts -- 11 607 in
    generate_embeddings.ipynb -- are not multiples of anything).  For Nt % 32 == 0 this is a plain contiguous tensor; otherwise a
    [:, :, :Nt] view of the padded storage: same values and indexing, ``.contiguous()`` compacts it.

    ``dtype`` = ``torch.float16`` / ``torch.bfloat16`` (the 16-bit destinations of ``bilinear_allpairs`` and
    ``bilinear_ensemble_sigmoid``): the pitch unit is 64 elements, still one 128-byte line."""
    if dtype != torch.float32 and dtype not in SCORE_TYPES:
        raise ValueError(f"dtype: expected torch.float32, torch.float16 or torch.bfloat16, got {dtype}")
    unit = 32 if dtype == torch.float32 else 64                   # elements: one 128-byte line (scripts/head_ragged_bench.py compared 4 .. 64 floats)
    pitch = (Nt + unit - 1) // unit * unit
    return torch.empty((L, Nh, pitch), dtype=dtype, device=device)[:, :, :Nt]


# ------------------------------------------------------------------------------- dense blocks
ACTS = {None: 0, "none": 0, "relu": 1, "gelu": 2, "sigmoid": 3, "tanh": 4, "leakyrelu": 5, "softplus": 6, "selu": 7}

_pad_cache = {}


def forward_only(*tensors) -> None:
    """The raw wrappers of this module are forward-only: refuse to run under autograd rather than silently return
    tensors that do not carry gradients.  The differentiable entry points are in madrigal_amd.autograd (each node
    calls these wrappers for its forward and its backward pass with autograd switched off)."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError("madrigal_amd.ops wrappers are forward-only: use madrigal_amd.autograd (or the model classes) "
                           "to record a gradient, or call under torch.no_grad()")


def _pad_last(t: torch.Tensor, mult: int = 4) -> torch.Tensor:
    k = t.shape[-1]
    if k % mult == 0:
        return t
    return torch.nn.functional.pad(t, (0, mult - k % mult))


def _wkey(w: torch.Tensor):
    return (w.data_ptr(), tuple(w.shape), tuple(w.stride()), str(w.device))


def padded_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [N,K] with K zero-padded to a multiple of 4.  Cached per storage address and in-place
    version; the entry keeps the source tensor alive, so the address cannot be recycled under the cache."""
    if w.shape[-1] % 4 == 0 and w.is_contiguous():
        return w.detach()
    k = _wkey(w)
    hit = _pad_cache.get(k)
    if hit is not None and hit[0] == w._version:
        return hit[1]
    p = _pad_last(w.detach()).contiguous()
    _pad_cache[k] = (w._version, p, w)
    return p


_pack_cache = {}


def packed_weight_image(w: torch.Tensor, prec: int):
    """Operand image of a (padded) nn.Linear weight for mdg_linear, built once per (storage, version, precision)."""
    N, K = w.shape
    nbytes = lib().mdg_pack_operand_bytes(N, K, prec)
    if nbytes == 0:
        return None
    k = _wkey(w) + (prec,)
    hit = _pack_cache.get(k)
    if hit is not None and hit[0] == w._version:
        return hit[1]
    img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call("mdg_pack_operand", _ptr(w), w.stride(0), N, K, prec, _ptr(img), nbytes, _stream(w))
    _pack_cache[k] = (w._version, img, w)
    return img


def pack_operand(x: torch.Tensor, precision="bf16x3") -> Optional[torch.Tensor]:
    """Operand image of a 2-D fp32 activation for ``linear_packed`` (what mdg_linear's own pre-pass writes); None where the
    arithmetic mode takes the tensor as it is."""
    x = _f32_cuda(x, "x", 2)
    M, K = x.shape
    if K % 4 or x.stride(1) != 1 or x.stride(0) % 4:
        x = _pad_last(x).contiguous()
        K = x.shape[1]
    prec = _prec(precision)
    nbytes = lib().mdg_pack_operand_bytes(M, K, prec)
    if nbytes == 0:
        return None
    img = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    call("mdg_pack_operand", _ptr(x), x.stride(0), M, K, prec, _ptr(img), nbytes, _stream(x))
    return img


GATHER_MAX_SOURCES = 19


def gather_rows_multi(sources, idx: torch.Tensor, rows_per_source: Optional[int] = None, *, pad4: bool = False, image=None,
                      want_fp32: bool = True):
    """``torch.cat(sources).index_select(0, idx)`` for 1..19 fp32 matrices of one width without the concatenated copy
    (mdg_gather_rows_multi): row ``idx[i] % rows_per_source`` of source ``idx[i] // rows_per_source``.  ``rows_per_source``
    defaults to the sources' common row count (then the result equals the cat + index_select bit for bit); with a larger value
    the sources may be shorter, and an index that is negative or outside its source gathers a zero row.

    ``pad4``: the result is [n, width rounded up to 4] with zero columns behind ``width`` (what ``linear`` pads a 978-wide
    input to), else [n, width].  ``image`` (a precision): also return the rows as the packed operand of ``linear_packed``, the
    bytes of ``pack_operand`` on them; None where the mode takes none.  -> rows, or (rows | None, image | None) with ``image``."""
    srcs = list(sources)
    if not 1 <= len(srcs) <= GATHER_MAX_SOURCES:
        raise ValueError(f"gather_rows_multi: 1 to {GATHER_MAX_SOURCES} sources, got {len(srcs)}")
    dev, W = srcs[0].device, srcs[0].shape[-1]
    for j, t in enumerate(srcs):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == W and t.device == dev):
            raise ValueError(f"gather_rows_multi: sources[{j}] must be an fp32 cuda matrix of width {W} on {dev}")
        if t.shape[0] and t.stride(1) != 1:
            srcs[j] = t.contiguous()
    forward_only(*srcs)
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1 and idx.device == dev):
        raise ValueError("gather_rows_multi: idx must be a 1-D int64 cuda tensor on the sources' device")
    idx = idx if idx.is_contiguous() else idx.contiguous()
    rps = max(t.shape[0] for t in srcs) if rows_per_source is None else int(rows_per_source)
    if rows_per_source is None and any(t.shape[0] != rps for t in srcs):
        raise ValueError("gather_rows_multi: sources of different row counts need an explicit rows_per_source")
    if rps < max(t.shape[0] for t in srcs):
        raise ValueError("gather_rows_multi: rows_per_source smaller than a source")
    n, Wo = idx.numel(), _ceil4(W)
    prec = None if image is None else _prec(image)
    nbytes = 0 if prec is None or prec == PREC_F32 else lib().mdg_pack_operand_bytes(n, Wo, prec)
    img = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    out = None
    if want_fp32 or img is None:
        out = torch.empty((n, Wo if pad4 or W % 4 else W), dtype=torch.float32, device=dev)
    if n and W and rps:
        K = len(srcs)
        a_p = (ctypes.c_void_p * K)(*[t.data_ptr() for t in srcs])
        a_r = (ctypes.c_int64 * K)(*[t.shape[0] for t in srcs])
        a_l = (ctypes.c_int64 * K)(*[t.stride(0) if t.shape[0] > 1 else W for t in srcs])
        call("mdg_gather_rows_multi", a_p, a_r, a_l, K, rps, W, _ptr(idx), n, _ptr(out), 0 if out is None else out.stride(0), _ptr(img), nbytes,
             0 if prec is None else prec, _stream(idx))
    elif out is not None:
        out.zero_()
    if out is not None and out.shape[1] != W and not pad4:
        out = out[:, :W]
    return out if image is None else (out, img)


def _rows2d(x: torch.Tensor, name: str):
    """[..., K] fp32 cuda tensor -> (2-D view/copy with unit inner stride and ld % 4 == 0, leading shape)."""
    x = _f32_cuda(x, name)
    lead = tuple(x.shape[:-1])
    return x.reshape(-1, x.shape[-1]), lead


class PackedWeight:
    """A dense block's weight that exists only as its operand image (``shape`` = [rows N, inner K] of the fp32 tensor it stands for):
    accepted by ``linear`` / ``linear_packed`` in place of the tensor.  ``transposed_weight_image`` makes W^T this way in the 16-bit
    modes -- the backward pass never needs W^T itself, only its image."""
    __slots__ = ("shape", "image", "device")

    def __init__(self, shape, image):
        self.shape, self.image, self.device = tuple(int(v) for v in shape), image, image.device


def linear_tile(M: int, N: int, precision="bf16x3") -> int:
    """Edge of the output tile the dense block runs an [M, N] product on, 256 or 128 (mdg_linear_tile: the launch path's own
    decision by shape, mode and MDG_LINEAR_TILE; no launch, no device)."""
    return int(lib().mdg_linear_tile(int(M), int(N), _prec(precision)))


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, scale=None, shift=None,
           act=None, residual: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 1.0,
           precision="bf16x3", out: Optional[torch.Tensor] = None, cache_weight: bool = True,
           weight_image: Optional[torch.Tensor] = None, dropout_p: float = 0.0, dropout_seed: int = 0) -> torch.Tensor:
    """y = alpha * act((x W^T + b) * scale + shift) + beta * residual   (nn.Linear layout W [N,K]).

    ``x`` may be a strided 2-D view (row stride a multiple of 4); ``residual`` may be [N] / [1,N]
    (broadcast over rows) or [M,N].  ``cache_weight``: keep the packed image of ``weight`` (hi/lo bf16 planes, K
    padded) and reuse it while the tensor is unchanged; pass False for one-shot "weights" (e.g. InfoNCE's F F^T).
    ``weight_image``: the (padded) weight's image when the caller keeps one (transposed_weight_image).
    ``dropout_p`` > 0 (training): y = dropout(act(x W^T + b)) + beta * residual, the mask of ``dropout(.., p, seed)`` on the contiguous
    result applied inside the epilogue (mdg_linear_dropout; no scale / shift, alpha = 1)."""
    forward_only(x, weight, bias, residual)
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.shape[1] % 4 == 0 and x.data_ptr() % 16 == 0 \
            and x.is_cuda and x.dtype == torch.float32:
        x2, lead = x, (x.shape[0],)
    else:
        x2, lead = _rows2d(x, "x")
        if x2.shape[1] % 4:
            x2 = _pad_last(x2)
    if isinstance(weight, PackedWeight):
        w, weight_image, w_ld = None, weight.image, 0
        wshape = weight.shape
    else:
        w = padded_weight(_f32_cuda(weight, "weight", 2))
        wshape, w_ld = tuple(w.shape), w.stride(0)
    M, K, N = x2.shape[0], x2.shape[1], wshape[0]
    if wshape[1] != K:
        raise ValueError(f"linear: x has inner dim {x.shape[-1]} but weight is {tuple(weight.shape)}")
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x2.device)
    elif out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"out: expected fp32 cuda [{M},{N}] with unit inner stride")
    ldr = 0
    if residual is not None:
        residual = _f32_cuda(residual, "residual") if residual.is_contiguous() else residual
        if residual.numel() == N:
            ldr = 0
        else:
            if residual.dim() != 2:
                residual = residual.reshape(-1, N)
            if residual.shape != (M, N) or residual.stride(1) != 1:
                raise ValueError(f"residual: expected [{M},{N}] or [{N}], got {tuple(residual.shape)}")
            ldr = residual.stride(0)
    for nm, t in (("bias", bias), ("scale", scale), ("shift", shift)):
        if t is not None and (t.numel() != N or not t.is_cuda or t.dtype != torch.float32):
            raise ValueError(f"{nm}: expected fp32 cuda [{N}]")
    prec = _prec(precision)
    wimg = weight_image if weight_image is not None else (packed_weight_image(w, prec) if cache_weight else None)
    if w is None and (wimg is None or prec == PREC_F32):
        raise ValueError("linear: a PackedWeight needs its image and a 16-bit arithmetic mode")
    ws, nbytes = _scratch("mdg_linear_workspace_bytes", x2.device, M, N, K, prec, 1 if wimg is not None else 0)
    if dropout_p > 0.0:
        if scale is not None or shift is not None or alpha != 1.0 or not out.is_contiguous():
            raise ValueError("linear: the dropout epilogue takes no scale / shift / alpha and a contiguous result")
        call("mdg_linear_dropout", _ptr(x2), x2.stride(0), _ptr(w), w_ld, _ptr(wimg), _ptr(out), out.stride(0), M, N, K,
             _ptr(None if bias is None else bias.detach().contiguous()), ACTS[act], _ptr(residual), ldr, beta, dropout_p,
             dropout_seed & (2 ** 64 - 1), prec, _ptr(ws), nbytes, _stream(x2))
        return out.view(*lead, N) if len(lead) != 1 or lead[0] != M else out
    call("mdg_linear", _ptr(x2), x2.stride(0), _ptr(w), w_ld, _ptr(wimg), _ptr(out), out.stride(0), M, N, K,
         _ptr(None if bias is None else bias.detach().contiguous()), _ptr(None if scale is None else scale.contiguous()),
         _ptr(None if shift is None else shift.contiguous()), ACTS[act], _ptr(residual), ldr, alpha, beta, prec, _ptr(ws), nbytes, _stream(x2))
    return out.view(*lead, N) if len(lead) != 1 or lead[0] != M else out


def linear_chain(x: torch.Tensor, weights, biases, *, edge: Optional[torch.Tensor] = None, edge_weight: Optional[torch.Tensor] = None,
                 scale=None, shift=None, act=None, precision="bf16x3", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch for a chain of 128-wide dense blocks (mdg_linear_chain128), bit-identical to the ``linear`` calls it stands for:

        u = linear(edge, edge_weight, residual=x)          (only with ``edge``; edge_weight [K, K_e], x [M, K])
        for W, b in zip(weights, biases): u = linear(u, W, b, act=act)     (scale / shift join the LAST one)

    ``weights``: 1 to 3 fp32 matrices, the first [128, K] with K <= 128 (a multiple of 4), the others [128, 128]; ``biases``: one
    entry per weight, each [128] or None.  bf16x3 / bf16 only; the weights' operand images are cached like ``linear``'s."""
    forward_only(x, edge, edge_weight, scale, shift, *weights, *[b for b in biases if b is not None])
    prec = _prec(precision)
    x = _f32_cuda(x, "x", 2) if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1) else x
    M, K = x.shape
    n = len(weights)
    if len(biases) != n:
        raise ValueError("linear_chain: one bias entry (or None) per weight")
    ws = [padded_weight(_f32_cuda(w, "weight", 2)) for w in weights]
    N = ws[-1].shape[0] if n else 0
    for j, w in enumerate(ws):
        if tuple(w.shape) != (N, K if j == 0 else N):
            raise ValueError(f"linear_chain: weight {j} is {tuple(w.shape)}, expected {(N, K if j == 0 else N)}")
    for nm, t in [("bias", b) for b in biases] + [("scale", scale), ("shift", shift)]:
        if t is not None and (t.numel() != N or not t.is_cuda or t.dtype != torch.float32):
            raise ValueError(f"{nm}: expected fp32 cuda [{N}]")
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    e_ptr, lde, k_e, we_img = None, 0, 0, None
    if edge is not None:
        edge = _f32_cuda(edge, "edge", 2) if not (edge.is_cuda and edge.dtype == torch.float32 and edge.dim() == 2 and edge.stride(1) == 1) else edge
        we = padded_weight(_f32_cuda(edge_weight, "edge_weight", 2))
        if edge.shape[0] != M or tuple(we.shape) != (K, edge.shape[1]):
            raise ValueError(f"linear_chain: edge {tuple(edge.shape)} / edge_weight {tuple(we.shape)} do not fit x {tuple(x.shape)}")
        e_ptr, lde, k_e = edge, edge.stride(0), edge.shape[1]
        we_img = packed_weight_image(we, prec) if prec != PREC_F32 else None
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    elif out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"out: expected fp32 cuda [{M},{N}] with unit inner stride")
    imgs = [packed_weight_image(w, prec) if prec != PREC_F32 else None for w in ws] + [None] * (3 - n)
    bs = [None if b is None else b.detach().contiguous() for b in biases] + [None] * (3 - n)
    call("mdg_linear_chain128", _ptr(x), x.stride(0), K, _ptr(e_ptr), lde, k_e, _ptr(we_img), n, _ptr(imgs[0]), _ptr(imgs[1]), _ptr(imgs[2]),
         _ptr(bs[0]), _ptr(bs[1]), _ptr(bs[2]), _ptr(None if scale is None else scale.contiguous()),
         _ptr(None if shift is None else shift.contiguous()), ACTS[act], _ptr(out), out.stride(0), M, N, prec, _stream(x))
    return out


def layernorm_packed(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, precision, want_fp32: bool = True):
    """LayerNorm of a 2-D ``x`` -> (y, image): ``image`` is y as the packed operand of the dense block that consumes it
    (linear_packed), written by the same kernel; None where the arithmetic mode or the width takes no image (then the
    consumer is the ordinary linear).  ``want_fp32=False``: y is None when the image exists (nothing else reads y)."""
    forward_only(x, weight, bias)
    x2 = x if (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.is_cuda and x.dtype == torch.float32) else _rows2d(x, "x")[0]
    R, d = x2.shape
    prec = _prec(precision)
    if prec == PREC_F32 or d % 64 or R == 0:
        return layernorm(x2, weight, bias, eps), None
    y = torch.empty((R, d), dtype=torch.float32, device=x2.device) if want_fp32 else None      # image only: y itself is never written
    nbytes = lib().mdg_pack_operand_bytes(R, d, prec)
    img = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
    call("mdg_layernorm_packed", _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()), _ptr(y), d, R, d, eps,
         prec, _ptr(img), nbytes, _stream(x2))
    return y, img


def layernorm_packed_kept(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, precision, q_slot: torch.Tensor, n_keep: int):
    """``layernorm_packed(.., want_fp32=False)`` of a 2-D ``x`` [R, d] whose kernel writes the rows that continue a second time, as a compact
    image of ``n_keep`` rows -> (image, kept_image).  ``q_slot`` [R] int32: the compact index of a kept row, negative elsewhere;
    ``kept_image`` is ``pack_operand`` of the kept fp32 rows in slot order, bit for bit.  None where the arithmetic mode or the width takes
    no image (the caller keeps its other path)."""
    forward_only(x, weight, bias)
    x2 = x if (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.is_cuda and x.dtype == torch.float32) else _rows2d(x, "x")[0]
    R, d = x2.shape
    prec = _prec(precision)
    if prec == PREC_F32 or d % 64 or R == 0:
        return None
    if not (q_slot.is_cuda and q_slot.dtype == torch.int32 and q_slot.dim() == 1 and q_slot.numel() == R and q_slot.is_contiguous()
            and q_slot.device == x2.device):
        raise ValueError(f"q_slot: expected a contiguous int32 cuda [{R}] on {x2.device}")
    n_keep = int(n_keep)
    nbytes, kbytes = lib().mdg_pack_operand_bytes(R, d, prec), lib().mdg_pack_operand_bytes(n_keep, d, prec)
    img = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
    kept = torch.empty(kbytes, dtype=torch.uint8, device=x2.device)
    call("mdg_layernorm_packed_kept", _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()), R, d, eps,
         prec, _ptr(img), nbytes, _ptr(q_slot), n_keep, _ptr(kept), kbytes, _stream(x2))
    return img, kept


def layernorm_logits(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, G: torch.Tensor, precision):
    """``layernorm_packed`` of a 2-D ``x`` [R, d] plus logits [R, H] = LN(x) G^T, formed from the normalised fp32 rows inside the
    norm kernel (G [H, d] fp32, H <= 64) -> (y, image, logits).  As in ``layernorm_packed(.., want_fp32=False)``: y is None when the
    image exists, image is None where the arithmetic mode or the width takes none (then y holds the rows)."""
    forward_only(x, weight, bias, G)
    x2 = x if (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.is_cuda and x.dtype == torch.float32) else _rows2d(x, "x")[0]
    R, d = x2.shape
    G = _f32_cuda(G, "G", 2)
    if G.shape[1] != d or not 1 <= G.shape[0] <= 64:
        raise ValueError(f"layernorm_logits: G must be [H <= 64, {d}], got {tuple(G.shape)}")
    H = G.shape[0]
    prec = _prec(precision)
    logits = torch.empty((R, H), dtype=torch.float32, device=x2.device)
    if prec == PREC_F32 or d % 64:
        y, img, nbytes = torch.empty((R, d), dtype=torch.float32, device=x2.device), None, 0
    else:
        nbytes = lib().mdg_pack_operand_bytes(R, d, prec)
        y, img = None, torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
    if R == 0:
        return y, img, logits
    call("mdg_layernorm_logits", _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()), _ptr(y), d, R, d, eps,
         prec, _ptr(img), nbytes, _ptr(G), H, _ptr(logits), _stream(x2))
    return y, img, logits


def linear_packed(x_img: torch.Tensor, M: int, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act=None,
                  residual: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 1.0, precision="bf16x3",
                  out: Optional[torch.Tensor] = None, weight_image: Optional[torch.Tensor] = None, cache_weight: bool = True) -> torch.Tensor:
    """linear() on an input that already exists as an operand image (layernorm_packed, linear_backward_pack): no pre-pass over x.
    ``weight_image``: the weight's own image if the caller keeps one (transposed_weight_image); ``cache_weight=False``: pack the
    weight inside the call (a one-shot tensor must not enter the per-storage image cache)."""
    if isinstance(weight, PackedWeight):
        w, weight_image, w_ld = None, weight.image, 0
        N, K = weight.shape
    else:
        w = padded_weight(_f32_cuda(weight, "weight", 2))
        N, K = w.shape
        w_ld = w.stride(0)
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    prec = _prec(precision)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x_img.device)
    elif out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"out: expected fp32 cuda [{M},{N}] with unit inner stride")
    ldr = 0
    if residual is not None:
        if residual.numel() != N:
            if residual.dim() != 2 or residual.shape != (M, N) or residual.stride(1) != 1:
                raise ValueError(f"residual: expected [{M},{N}] or [{N}]")
            ldr = residual.stride(0)
    wimg = weight_image if weight_image is not None else (packed_weight_image(w, prec) if cache_weight else None)
    ws, nbytes = _scratch("mdg_linear_packed_x_workspace_bytes", x_img.device, M, N, K, prec, 1 if wimg is not None else 0)    # (+ the stream-K slots of the 256-tile kernel)
    call("mdg_linear_packed_x", _ptr(x_img), M, K, _ptr(w), w_ld, _ptr(wimg), _ptr(out), out.stride(0), N,
         _ptr(None if bias is None else bias.detach().contiguous()), ACTS[act], _ptr(residual), ldr, alpha, beta, prec, _ptr(ws), nbytes,
         _stream(x_img))
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-wise LayerNorm over the last dim; ``x`` / ``out`` may be strided 2-D views (row stride % 4 == 0)."""
    forward_only(x, weight, bias)
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.is_cuda and x.dtype == torch.float32:
        x2, lead = x, None
    else:
        x2, lead = _rows2d(x, "x")
    R, d = x2.shape
    if out is None:
        out = torch.empty((R, d), dtype=torch.float32, device=x2.device)
    call("mdg_layernorm", _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()), _ptr(out), out.stride(0), R,
         d, eps, _stream(x2))
    return out.view(*lead, d) if lead is not None and out.is_contiguous() else out


def row_rstd(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm's per-row factor 1 / sqrt(var + eps) of a 2-D ``x`` [R, d] -> [R] (the factor ``layernorm`` applies, bit for bit)."""
    forward_only(x)
    x2 = x if (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.is_cuda and x.dtype == torch.float32) else _rows2d(x, "x")[0]
    R, d = x2.shape
    out = torch.empty(R, dtype=torch.float32, device=x2.device)
    call("mdg_row_rstd", _ptr(x2), x2.stride(0), _ptr(out), R, d, eps, _stream(x2))
    return out


def linear_rowscaled(x: torch.Tensor, weight: torch.Tensor, row_scale: torch.Tensor, bias_pre: Optional[torch.Tensor] = None,
                     bias: Optional[torch.Tensor] = None, *, precision="bf16x3", weight_image: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[m] = row_scale[m] * (x[m] W^T + bias_pre) + bias on the 128-tile dense block (short K; nn.Linear layout W [N,K]).
    ``weight_image``: the weight's operand image when the caller keeps one, else the per-storage cache of ``linear``."""
    forward_only(x, weight, row_scale, bias_pre, bias)
    x2, lead = _rows2d(x, "x")
    if x2.shape[1] % 4:
        x2 = _pad_last(x2)
    w = padded_weight(_f32_cuda(weight, "weight", 2))
    M, K, N = x2.shape[0], x2.shape[1], w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_rowscaled: x has inner dim {x.shape[-1]} but weight is {tuple(weight.shape)}")
    if row_scale.numel() != M or not row_scale.is_cuda or row_scale.dtype != torch.float32:
        raise ValueError(f"row_scale: expected fp32 cuda [{M}]")
    for nm, t in (("bias_pre", bias_pre), ("bias", bias)):
        if t is not None and (t.numel() != N or not t.is_cuda or t.dtype != torch.float32):
            raise ValueError(f"{nm}: expected fp32 cuda [{N}]")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x2.device)
    elif out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"out: expected fp32 cuda [{M},{N}] with unit inner stride")
    prec = _prec(precision)
    wimg = weight_image if weight_image is not None else packed_weight_image(w, prec)
    ws, nbytes = _scratch("mdg_linear_workspace_bytes", x2.device, M, N, K, prec, 1 if wimg is not None else 0)
    call("mdg_linear_rowscaled", _ptr(x2), x2.stride(0), _ptr(w), w.stride(0), _ptr(wimg), _ptr(out), out.stride(0), M, N, K,
         _ptr(row_scale.contiguous()), _ptr(None if bias_pre is None else bias_pre.detach().contiguous()),
         _ptr(None if bias is None else bias.detach().contiguous()), prec, _ptr(ws), nbytes, _stream(x2))
    return out.view(*lead, N) if len(lead) != 1 or lead[0] != M else out


# ------------------------------------------------------------------------------- fusion
def mask_bits(mask: torch.Tensor) -> torch.Tensor:
    """bool [..., S] (True = masked) -> uint32-valued int32 [...] bit field, bit j = mask[..., j]."""
    S = mask.shape[-1]
    if S > 32:
        raise ValueError("at most 32 tokens")
    w = (torch.ones(S, dtype=torch.int64, device=mask.device) << torch.arange(S, device=mask.device))
    return (mask.to(torch.int64) * w).sum(-1).to(torch.int32).contiguous()     # two's complement keeps bit 31


def assemble_tokens(str_emb, kg_emb, cv_emb, tx_emb, *, bottleneck=None, cls=None, pe=None, rows=None,
                    normalize=False, token_index=None) -> torch.Tensor:
    """[n, S, 128] token sequence (see mdg_assemble_tokens).  tx_emb is [16*n_src,128], cell-line major.
    ``token_index`` (int64 [R], values drug*S + s of the live tokens): emit only those rows -> [R,128]."""
    forward_only(str_emb, kg_emb, cv_emb, tx_emb, bottleneck, cls, pe)
    s, k, c, t = (_f32_cuda(a, nm, 2) for a, nm in ((str_emb, "str"), (kg_emb, "kg"), (cv_emb, "cv"), (tx_emb, "tx")))
    n_src = s.shape[0]
    if k.shape != s.shape or c.shape != s.shape or t.shape != (16 * n_src, s.shape[1]):
        raise ValueError("assemble_tokens: modality embeddings disagree in shape")
    n = n_src if rows is None else int(rows.numel())
    nb = 0 if bottleneck is None else int(bottleneck.shape[0])
    pe2 = None if pe is None else _f32_cuda(pe.detach().reshape(-1, pe.shape[-1]), "pe")
    S = (1 if cls is not None else 0) + 3 + nb + 16
    if token_index is None:
        seq = torch.empty((n, S, s.shape[1]), dtype=torch.float32, device=s.device)
        n_tok = 0
    else:
        if token_index.dtype != torch.int64 or not token_index.is_cuda:
            raise ValueError("token_index: int64 cuda tensor")
        n_tok = int(token_index.numel())
        seq = torch.empty((n_tok, s.shape[1]), dtype=torch.float32, device=s.device)
    call("mdg_assemble_tokens", _ptr(s), _ptr(k), _ptr(c), _ptr(t), _ptr(None if bottleneck is None else bottleneck.detach().contiguous()),
         _ptr(None if cls is None else cls.detach().contiguous()), _ptr(pe2), _ptr(None if rows is None else rows.contiguous()),
         _ptr(None if token_index is None else token_index.contiguous()), n_tok, _ptr(seq), n, n_src, nb, 0 if cls is None else 1,
         0 if pe2 is None else pe2.shape[0], 1 if normalize else 0, s.shape[1], _stream(s))
    return seq


def fusion_attention(qkv: torch.Tensor, n: int, S: int, H: int, dh: int, kpm_bits=None, src_bits=None,
                     want_probs: bool = False, row_start: Optional[torch.Tensor] = None,
                     row_bits: Optional[torch.Tensor] = None, p_drop: float = 0.0, seed: int = 0):
    """Self-attention core over q|k|v rows -> (attention output rows, probs [n,H,S,S] | None).
    Dense: qkv [n*S, 3*H*dh].  Compact (``row_start`` [n+1] int64): qkv holds only live token rows."""
    qkv = _f32_cuda(qkv, "qkv", 2)
    d = H * dh
    rows = n * S if row_start is None else qkv.shape[0]
    if qkv.shape != (rows, 3 * d):
        raise ValueError(f"qkv: expected [{rows},{3 * d}], got {tuple(qkv.shape)}")
    if row_start is not None and (row_start.dtype != torch.int64 or row_start.numel() != n + 1 or want_probs):
        raise ValueError("row_start: int64 [n+1]; attention weights need the dense layout")
    out = torch.empty((rows, d), dtype=torch.float32, device=qkv.device)
    probs = torch.empty((n, H, S, S), dtype=torch.float32, device=qkv.device) if want_probs else None
    call("mdg_fusion_attention_dropout", _ptr(qkv), qkv.stride(0), _ptr(out), d, _ptr(kpm_bits), _ptr(src_bits), _ptr(probs), _ptr(row_start),
         _ptr(row_bits), n, S, H, dh, p_drop, seed & (2 ** 64 - 1), _stream(qkv), what="mdg_fusion_attention")
    return out, probs


def fusion_attention_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n: int, S: int, H: int, ds: int, dv: int, *, hq: int, hk: int,
                         hv: int, out: Optional[torch.Tensor] = None, ho: Optional[int] = None, kpm_bits=None, src_bits=None,
                         row_start: Optional[torch.Tensor] = None, row_bits: Optional[torch.Tensor] = None,
                         qscale: float = 1.0) -> torch.Tensor:
    """``fusion_attention``'s forward pass on three operands of their own (2-D fp32 views with unit inner stride): ``hq`` / ``hk`` /
    ``hv`` the column step from one head to the next (0: the operand's first columns serve every head), ``ds`` columns in the score
    product and ``dv`` in the value product.  ``out`` (view, head step ``ho`` >= dv) defaults to a fresh [rows, H*dv]."""
    forward_only(q, k, v)
    rows = q.shape[0]
    for nm, t in (("q", q), ("k", k), ("v", v)) + ((("out", out),) if out is not None else ()):
        if t.dim() != 2 or t.shape[0] != rows or t.stride(1) != 1 or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{nm}: expected a 2-D fp32 cuda tensor of {rows} rows with unit inner stride")
    if row_start is None and rows != n * S:
        raise ValueError(f"q: expected {n * S} rows, got {rows}")
    if row_start is not None and (row_start.dtype != torch.int64 or row_start.numel() != n + 1):
        raise ValueError("row_start: int64 [n+1]")
    for nm, t, step, w in (("q", q, hq, ds), ("k", k, hk, ds), ("v", v, hv, dv)):
        if t.shape[1] < (H - 1) * step + w:
            raise ValueError(f"{nm}: {t.shape[1]} columns do not hold {H} heads of step {step} and width {w}")
    if out is None:
        ho = dv if ho is None else ho
        out = torch.empty((rows, (H - 1) * ho + dv), dtype=torch.float32, device=q.device)
    elif ho is None or out.shape[1] < (H - 1) * ho + dv:
        raise ValueError("out: give its head step ho, and columns for H heads of it")
    call("mdg_fusion_attention_qkv", _ptr(q), q.stride(0), hq, _ptr(k), k.stride(0), hk, _ptr(v), v.stride(0), hv, _ptr(out), out.stride(0), ho,
         _ptr(kpm_bits), _ptr(src_bits), _ptr(row_start), _ptr(row_bits), n, S, H, ds, dv, qscale, _stream(q))
    return out


def fusion_attention_kept(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_tiles: int, H: int, dh: int, row_start: torch.Tensor,
                          row_bits: Optional[torch.Tensor], q_slot: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Compact-mode ``fusion_attention`` where only the kept rows have a query and an output: ``q`` [n_keep, H*dh] and the result
    [n_keep, H*dh] hold the kept rows in slot order, ``k`` / ``v`` are [R, H*dh] views of one row stride (e.g. the halves of a K|V
    block), ``q_slot`` [R] int32 gives a kept row's slot and is negative elsewhere.  Row ``q_slot[r]`` of the result equals row r of
    ``fusion_attention``'s, bit for bit; the queries of the other rows are never read."""
    forward_only(q, k, v)
    d, R, n_keep = H * dh, k.shape[0], q.shape[0]
    for nm, t, rows in (("q", q, n_keep), ("k", k, R), ("v", v, R)) + ((("out", out, n_keep),) if out is not None else ()):
        if t.dim() != 2 or t.shape != (rows, d) or t.stride(1) != 1 or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{nm}: expected an fp32 cuda [{rows},{d}] tensor with unit inner stride")
    if R and k.stride(0) != v.stride(0):
        raise ValueError("k and v: one row stride for both")
    if row_start.dtype != torch.int64 or row_start.numel() != n_tiles + 1 or not row_start.is_contiguous():
        raise ValueError("row_start: contiguous int64 [n_tiles+1]")
    if q_slot.dtype != torch.int32 or q_slot.dim() != 1 or q_slot.numel() != R or not q_slot.is_contiguous() or not q_slot.is_cuda:
        raise ValueError(f"q_slot: expected a contiguous int32 cuda [{R}]")
    if row_bits is not None and (row_bits.numel() != R or not row_bits.is_contiguous()):
        raise ValueError(f"row_bits: expected a contiguous [{R}]")
    if out is None:
        out = torch.empty((n_keep, d), dtype=torch.float32, device=q.device)
    call("mdg_fusion_attention_kept", _ptr(q), q.stride(0), _ptr(k), _ptr(v), k.stride(0), _ptr(out), out.stride(0), _ptr(row_start),
         _ptr(row_bits), _ptr(q_slot), n_keep, n_tiles, H, dh, _stream(k))
    return out


def token_scaled_rows(tokens: torch.Tensor, rf: torch.Tensor, d: int, eps: float, tail: torch.Tensor):
    """Token rows T [R, 128] -> (X [R, 132] = r * [T, 1, 0, 0, 0], r [R]) with r = 1 / sqrt(|rf [T; 1]|^2 / d + eps) (``rf`` [nr <= 132, 132]:
    the triangular factor of the centred embed2latent, so r is norm1's factor of h = embed2latent(T)); T is also copied into
    ``tail`` (a [R, 128] view, e.g. the last columns of the out_proj block's input)."""
    forward_only(tokens, rf)
    t = tokens if (tokens.dim() == 2 and tokens.stride(1) == 1 and tokens.stride(0) % 4 == 0 and tokens.is_cuda
                   and tokens.dtype == torch.float32) else _f32_cuda(tokens, "tokens", 2)
    R, D = t.shape
    rf = _f32_cuda(rf, "rf", 2)
    Dp = (D + 4) // 4 * 4
    if rf.shape[1] != Dp or rf.shape[0] > Dp:
        raise ValueError(f"rf: expected [<= {Dp}, {Dp}], got {tuple(rf.shape)}")
    if tail.shape != (R, D) or tail.stride(1) != 1 or tail.dtype != torch.float32 or not tail.is_cuda:
        raise ValueError(f"tail: expected an fp32 cuda [{R},{D}] view with unit inner stride")
    X = torch.empty((R, Dp), dtype=torch.float32, device=t.device)
    r = torch.empty(R, dtype=torch.float32, device=t.device)
    call("mdg_token_scaled_rows", _ptr(t), t.stride(0), _ptr(rf), rf.shape[0], D, d, eps, _ptr(X), Dp, _ptr(tail), tail.stride(0), _ptr(r), R,
         _stream(t))
    return X, r


def fusion_attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, n: int, S: int, H: int, dh: int, kpm_bits=None, src_bits=None,
                         row_start=None, row_bits=None, p_drop: float = 0.0, seed: int = 0) -> torch.Tensor:
    """Gradient of the q|k|v rows given the gradient of the attention output (weights recomputed, mask replayed)."""
    qkv, dout = _f32_cuda(qkv, "qkv", 2), _f32_cuda(dout, "dout", 2)
    d = H * dh
    if qkv.shape[1] != 3 * d or dout.shape != (qkv.shape[0], d):
        raise ValueError("fusion_attention_bwd: shape mismatch")
    # rows outside every tile (none in practice) would stay unwritten: start from zeros only in that case
    dqkv = torch.empty_like(qkv)
    call("mdg_fusion_attention_bwd", _ptr(qkv), qkv.stride(0), _ptr(dout), d, _ptr(dqkv), 3 * d, _ptr(kpm_bits), _ptr(src_bits), _ptr(row_start),
         _ptr(row_bits), n, S, H, dh, p_drop, seed & (2 ** 64 - 1), _stream(qkv))
    return dqkv


def xattn_pool(q_proj: torch.Tensor, kv_proj: torch.Tensor, n: int, Tk: int, H: int, dh: int, p_drop: float = 0.0,
               seed: int = 0) -> torch.Tensor:
    q = _f32_cuda(q_proj.reshape(-1), "q_proj", 1)
    kv = _f32_cuda(kv_proj, "kv_proj", 2)
    d = H * dh
    if q.numel() != d or kv.shape != (n * Tk, 2 * d):
        raise ValueError(f"xattn_pool: expected q [{d}] and kv [{n * Tk},{2 * d}]")
    out = torch.empty((n, d), dtype=torch.float32, device=kv.device)
    call("mdg_xattn_pool_dropout", _ptr(q), _ptr(kv), kv.stride(0), _ptr(out), d, n, Tk, H, dh, p_drop, seed & (2 ** 64 - 1), _stream(kv),
         what="mdg_xattn_pool")
    return out


def xattn_fold_pool(P: torch.Tensor, logits: torch.Tensor, c_z: torch.Tensor, n: int, Tk: int) -> torch.Tensor:
    """Folded cross-attention pooling (mdg_xattn_fold_pool): P [n*Tk, H*D] (key rows through V, out_proj and latent2embed, head-major
    column blocks), logits [n*Tk, H], c_z [D] -> z [n, D] = sum_h sum_t softmax_t(logits[., h]) P[., h*D:(h+1)*D] + c_z."""
    P, logits, c_z = _f32_cuda(P, "P", 2), _f32_cuda(logits, "logits", 2), _f32_cuda(c_z.reshape(-1), "c_z", 1)
    D = c_z.numel()
    H = logits.shape[1]
    if P.shape != (n * Tk, H * D) or logits.shape[0] != n * Tk:
        raise ValueError(f"xattn_fold_pool: expected P [{n * Tk},{H * D}] and logits [{n * Tk},{H}], got {tuple(P.shape)} and {tuple(logits.shape)}")
    if P.device != logits.device or P.device != c_z.device:
        raise ValueError("xattn_fold_pool: P, logits and c_z must be on one device")
    if P.stride(0) % 2 or P.data_ptr() % 8:
        P = P.contiguous()
    z = torch.empty((n, D), dtype=torch.float32, device=P.device)
    call("mdg_xattn_fold_pool", _ptr(P), P.stride(0), _ptr(logits), logits.stride(0), _ptr(c_z), _ptr(z), D, n, Tk, H, D, _stream(P))
    return z


def xattn_pool_bwd(q_proj: torch.Tensor, kv_proj: torch.Tensor, dout: torch.Tensor, n: int, Tk: int, H: int, dh: int,
                   p_drop: float = 0.0, seed: int = 0):
    """-> (dq_proj [d], dkv [n*Tk, 2d])."""
    q = _f32_cuda(q_proj.reshape(-1), "q_proj", 1)
    kv, dout = _f32_cuda(kv_proj, "kv_proj", 2), _f32_cuda(dout, "dout", 2)
    d = H * dh
    if q.numel() != d or kv.shape != (n * Tk, 2 * d) or dout.shape != (n, d):
        raise ValueError("xattn_pool_bwd: shape mismatch")
    dkv = torch.empty_like(kv)
    dq_part = torch.empty((n, d), dtype=torch.float32, device=kv.device)
    call("mdg_xattn_pool_bwd", _ptr(q), _ptr(kv), kv.stride(0), _ptr(dout), d, _ptr(dkv), 2 * d, _ptr(dq_part), n, Tk, H, dh, p_drop,
         seed & (2 ** 64 - 1), _stream(kv))
    return colsum(dq_part), dkv


# ------------------------------------------------------------------------------- graphs
# ------------------------------------------------------------------------------- grouped dense block
GROUP_TILE = 128          # output tile edge of mdg_linear_grouped


def group_tile_table(groups, device) -> torch.Tensor:
    """Tile descriptors of a grouped launch (include/madrigal_hip.h: mdg_linear_grouped) -> int64 [n_tiles, words] on
    ``device``.  ``groups``: dicts with m_base, rows (the group's rows in the stacked x), n_base, n (its rows in the stacked W),
    y_off, ldy (float offset of its output block in y and that block's row stride) and optionally res_off, ldr, alpha, beta."""
    import struct
    words = lib().mdg_linear_group_tile_words()
    rows = []
    for g in groups:
        for v in (g["n_base"], g["y_off"], g["ldy"], g.get("res_off", 0) or 0, g.get("ldr", 0)):
            if v % 4:
                raise ValueError("group_tile_table: offsets and row strides must be multiples of 4 floats")
        ab = struct.unpack("<q", struct.pack("<ff", float(g.get("alpha", 1.0)), float(g.get("beta", 1.0))))[0]
        has_res = "res_off" in g and g["res_off"] is not None
        for ty in range((g["rows"] + GROUP_TILE - 1) // GROUP_TILE):
            for tx in range((g["n"] + GROUP_TILE - 1) // GROUP_TILE):
                e = [g["m_base"] + ty * GROUP_TILE, g["m_base"] + g["rows"], g["n_base"] + tx * GROUP_TILE, g["n_base"] + g["n"],
                     g["m_base"], g["n_base"], g["y_off"], g["ldy"], g["res_off"] if has_res else -1, g.get("ldr", 0) if has_res else 0, ab, 0]
                rows.append(e + [0] * (words - len(e)))
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, words) if rows else torch.zeros((0, words), dtype=torch.int64)
    return t.to(device)


def linear_grouped(x: torch.Tensor, w_all: torch.Tensor, bias_all: Optional[torch.Tensor], tiles: torch.Tensor, y: torch.Tensor,
                   residual: Optional[torch.Tensor] = None, act=None, precision="bf16x3") -> torch.Tensor:
    """G products y_g = alpha_g act(x_g W_g^T + b_g) + beta_g r_g in one launch: ``x`` [rows_total, K] and ``w_all``
    [w_rows_total, K] hold the groups' rows stacked, ``tiles`` = group_tile_table(...), ``y`` / ``residual`` the buffers its
    offsets address.  The packed image of ``w_all`` is kept while the tensor is unchanged (as for linear)."""
    forward_only(x, w_all, bias_all, residual)
    x, w_all = _f32_cuda(x, "x", 2), _f32_cuda(w_all, "w_all", 2)
    if x.stride(1) != 1 or w_all.shape[1] != x.shape[1] or not w_all.is_contiguous() or x.shape[1] % 4 or x.stride(0) % 4:
        raise ValueError("linear_grouped: x [rows,K] (unit inner stride, K and row stride multiples of 4), w_all [w_rows,K] contiguous")
    if not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous() or (residual is not None and not residual.is_contiguous()):
        raise ValueError("linear_grouped: y / residual must be contiguous fp32 cuda buffers")
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    prec = _prec(precision)
    K = x.shape[1]
    wimg = packed_weight_image(w_all, prec)
    ws, nbytes = _scratch("mdg_linear_grouped_workspace_bytes", x.device, x.shape[0], K, prec)
    call("mdg_linear_grouped", _ptr(x), x.stride(0), x.shape[0], K, _ptr(w_all), w_all.stride(0), _ptr(wimg), w_all.shape[0],
         _ptr(None if bias_all is None else bias_all.detach().contiguous()), _ptr(tiles), tiles.shape[0], _ptr(y), _ptr(residual), ACTS[act], prec,
         _ptr(ws), nbytes, _stream(x))
    return y


def csr_aggregate(x: torch.Tensor, rowptr: torch.Tensor, col: Optional[torch.Tensor] = None, *, edge_weight=None,
                  x_self: Optional[torch.Tensor] = None, self_coef_dev: Optional[torch.Tensor] = None,
                  self_coef_add: float = 0.0, mean: bool = False) -> torch.Tensor:
    """out[v] = (self_coef_add + self_coef_dev[0]) * x_self[v] + sum_{e in row v} w[e] * x[col[e]]  (see the C header)."""
    forward_only(x, x_self)
    x = _f32_cuda(x, "x", 2)
    if x.shape[1] % 4:
        x = _pad_last(x)
    if x.shape[0] == 0:                       # no source rows (hence no edges): a valid pointer for the C side all the same
        x = torch.zeros((1, x.shape[1]), dtype=torch.float32, device=x.device)
    F = x.shape[1]
    n_dst = int(rowptr.numel()) - 1
    if rowptr.dtype != torch.int64 or (col is not None and col.dtype != torch.int64):
        raise ValueError("rowptr / col must be int64")
    if x_self is not None:
        x_self = _f32_cuda(x_self, "x_self", 2)
        if x_self.shape[1] % 4:
            x_self = _pad_last(x_self)
        if x_self.shape != (n_dst, F):
            raise ValueError("x_self: shape mismatch")
    out = torch.empty((n_dst, F), dtype=torch.float32, device=x.device)
    call("mdg_csr_aggregate", _ptr(x), x.stride(0), _ptr(rowptr.contiguous()), _ptr(None if col is None else col.contiguous()),
         _ptr(None if edge_weight is None else edge_weight.contiguous()), _ptr(x_self), 0 if x_self is None else x_self.stride(0),
         _ptr(self_coef_dev), self_coef_add, 1 if mean else 0, _ptr(out), F, n_dst, F, _stream(x))
    return out


def hgt_attention(q: torch.Tensor, kv: torch.Tensor, plan: dict, heads: int, apply_gelu: bool = True,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Edge softmax + aggregation for one destination node type.  ``q`` may be a column-slice view
    [n_dst,128] of the k|q|v projection; ``plan`` holds col / item_* / item_ptr (see graph_plans).  ``out``: contiguous
    [n_dst,128] rows to write (a row block of a buffer shared by all destination types)."""
    n_dst = q.shape[0]
    if q.dim() != 2 or q.shape[1] != 128 or q.stride(1) != 1 or not q.is_cuda or q.dtype != torch.float32:
        raise ValueError("q: expected fp32 cuda [n_dst,128] with unit inner stride")
    if out is None:
        out = torch.empty((n_dst, 128), dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (n_dst, 128) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != q.device:
        raise ValueError("out: expected contiguous fp32 [n_dst,128] on q's device")
    n_items = int(plan["item_dst"].numel())
    ws, nbytes = _scratch("mdg_hgt_attention_workspace_bytes", q.device, n_items, heads)
    call("mdg_hgt_attention", _ptr(q), q.stride(0), _ptr(kv), 0 if kv is None else kv.stride(0), _ptr(plan["col"]), _ptr(plan["item_dst"]),
         _ptr(plan["item_begin"]), _ptr(plan["item_end"]), n_items, _ptr(plan["item_ptr"]), _ptr(out), 128, n_dst, heads, 128, 1 if apply_gelu else 0,
         _ptr(ws), nbytes, _stream(q))
    return out


def hgt_attention_rows(buf: torch.Tensor, plan_all: dict, heads: int, out: torch.Tensor, apply_gelu: bool = True) -> torch.Tensor:
    """Edge attention of ALL destination types of a conv in one launch (inference).  ``buf``: the flat projection buffer (queries,
    keys and values); ``plan_all``: the destination types' plans concatenated (models.HGTConv._forward_grouped): q_off [n_dst] float
    offsets of the query rows in ``buf``, col / item_* / item_ptr with destinations numbered across the types; ``out`` [n_dst,128]."""
    n_dst = int(plan_all["q_off"].numel())
    if tuple(out.shape) != (n_dst, 128) or not out.is_contiguous() or out.dtype != torch.float32 or not buf.is_contiguous():
        raise ValueError("hgt_attention_rows: out must be contiguous fp32 [n_dst,128], buf contiguous")
    n_items = int(plan_all["item_dst"].numel())
    ws, nbytes = _scratch("mdg_hgt_attention_workspace_bytes", buf.device, n_items, heads)
    kv = buf.view(-1, 128)
    call("mdg_hgt_attention_rows", _ptr(buf), _ptr(plan_all["q_off"]), _ptr(kv), 128, _ptr(plan_all["col"]), _ptr(plan_all["item_dst"]),
         _ptr(plan_all["item_begin"]), _ptr(plan_all["item_end"]), n_items, _ptr(plan_all["item_ptr"]), _ptr(out), 128, n_dst, heads,
         1 if apply_gelu else 0, _ptr(ws), nbytes, _stream(buf))
    return out


HGT_FEAT_ROW = 132       # floats per (destination, relation, head) row of the feature-space blocks: 128 | 1 | 3 zeros


def hgt_attention_feat(x: torch.Tensor, ut: torch.Tensor, plan: dict, heads: int = 4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Edge attention in node-feature space (inference).  ``x`` [n_rows, 128]: the stacked feature rows the plan's
    ``src`` indexes; ``ut`` [n_dst, R, 4, 132] = [K^T q | q . kappa | 0 0 0]; ``plan``: graph_plans.hgt_feat_plan.  Returns the
    relation-major S~ [R, n_dst, 4, 132] = [sum_e p_h(e) x_src(e) | sum_e p_h(e) | 0 0 0], p the softmax over all in-edges."""
    n_dst, R = int(plan["n_dst"]), int(plan["n_rel"])
    if x.dim() != 2 or x.shape[1] != 128 or x.stride(1) != 1 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("hgt_attention_feat: x must be fp32 cuda [n_rows,128] with unit inner stride")
    if x.shape[0] != plan["n_rows"]:
        raise ValueError(f"hgt_attention_feat: the plan indexes {plan['n_rows']} feature rows, x has {x.shape[0]}")
    if heads != 4 or tuple(ut.shape) != (n_dst, R, 4, HGT_FEAT_ROW) or not ut.is_contiguous() or ut.dtype != torch.float32 or ut.device != x.device:
        raise ValueError(f"hgt_attention_feat: ut must be contiguous fp32 [{n_dst},{R},4,{HGT_FEAT_ROW}] on x's device (4 heads)")
    if out is None:
        out = torch.empty((R, n_dst, 4, HGT_FEAT_ROW), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (R, n_dst, 4, HGT_FEAT_ROW) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError(f"hgt_attention_feat: out must be contiguous fp32 [{R},{n_dst},4,{HGT_FEAT_ROW}] on x's device")
    n_items = int(plan["item_dst"].numel())
    ws, nbytes = _scratch("mdg_hgt_attention_feat_workspace_bytes", x.device, n_items)
    call("mdg_hgt_attention_feat", _ptr(x), x.stride(0), x.shape[0], _ptr(ut), _ptr(plan["src"]), int(plan["src"].numel()), _ptr(plan["item_dst"]),
         _ptr(plan["item_rel"]), _ptr(plan["item_begin"]), _ptr(plan["item_end"]), n_items, _ptr(plan["rel_ptr"]), _ptr(out), n_dst, R, heads,
         _ptr(ws), nbytes, _stream(x))
    return out


def hgt_sum_relations(part: torch.Tensor, apply_gelu: bool = True) -> torch.Tensor:
    """act(sum_r part[r]) of ``part`` [R, n, 128], slabs added in order; act = the erf GELU of the dense blocks, or none."""
    if part.dim() != 3 or part.shape[0] < 1 or part.shape[2] != 128 or not part.is_contiguous() or not part.is_cuda or part.dtype != torch.float32:
        raise ValueError("hgt_sum_relations: part must be contiguous fp32 cuda [R,n,128]")
    out = torch.empty((part.shape[1], 128), dtype=torch.float32, device=part.device)
    call("mdg_hgt_sum_relations", _ptr(part), part.shape[1], part.shape[0], 1 if apply_gelu else 0, _ptr(out), _stream(part))
    return out


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    """F.normalize(x, p=2, dim=-1)."""
    forward_only(x)
    x2, lead = _rows2d(x, "x")
    if x2.shape[1] % 4:
        raise ValueError("l2_normalize: last dim must be a multiple of 4")
    y = torch.empty_like(x2)
    call("mdg_l2_normalize", _ptr(x2), x2.stride(0), _ptr(y), y.stride(0), x2.shape[0], x2.shape[1], _stream(x2))
    return y.view(*lead, x2.shape[1])


def token_pool(tokens: torch.Tensor, bits: Optional[torch.Tensor], mode: str) -> torch.Tensor:
    """Masked mean / sum / max over the token axis of [n,S,128]."""
    forward_only(tokens)
    t = _f32_cuda(tokens, "tokens", 3)
    n, S, D = t.shape
    out = torch.empty((n, D), dtype=torch.float32, device=t.device)
    call("mdg_token_pool", _ptr(t), _ptr(bits), _ptr(out), n, S, D, {"mean": 0, "sum": 1, "max": 2}[mode], _stream(t))
    return out


# ------------------------------------------------------------------------------- losses
def info_nce(aug1: torch.Tensor, aug2: torch.Tensor, too_hard_neg: Optional[torch.Tensor], temperature: float,
             precision="bf16x3", want_logits: bool = True):
    """(logits [2B,2B-1], labels [2B,2B-1], loss) of SimCLR_NovelDDI.contrastive_loss (simclr.py:74-108)."""
    forward_only(aug1, aug2)
    a1, a2 = _f32_cuda(aug1, "aug1", 2), _f32_cuda(aug2, "aug2", 2)
    if a1.shape != a2.shape:
        raise ValueError("aug1 / aug2 shapes differ")
    B = a1.shape[0]
    f = l2_normalize(torch.cat([a1, a2], dim=0))
    sim = linear(f, f, None, precision=precision, cache_weight=False)
    hard = None
    if too_hard_neg is not None:
        if too_hard_neg.shape != (B, B):
            raise ValueError("too_hard_neg: expected [B,B]")
        hard = too_hard_neg.to(device=a1.device, dtype=torch.uint8).contiguous()
    logits = torch.empty((2 * B, 2 * B - 1), dtype=torch.float32, device=a1.device) if want_logits else None
    labels = torch.empty_like(logits) if want_logits else None
    row = torch.empty(2 * B, dtype=torch.float32, device=a1.device)
    loss = torch.empty(1, dtype=torch.float32, device=a1.device)
    call("mdg_infonce_finish", _ptr(sim), _ptr(hard), _ptr(logits), _ptr(labels), _ptr(row), _ptr(loss), B, temperature, _stream(a1))
    return logits, labels, loss[0]


def gather_bce(scores: torch.Tensor, labels: torch.Tensor, heads: torch.Tensor, tails: torch.Tensor,
               target: Optional[torch.Tensor] = None, apply_sigmoid: bool = True):
    """pred = sigmoid?(scores)[labels, heads, tails]; loss = BCELoss(pred, target)  (train_ddi_batch.py:285-288)."""
    s = _f32_cuda(scores, "scores", 3)
    n = int(labels.numel())
    for nm, t in (("labels", labels), ("heads", heads), ("tails", tails)):
        if t.dtype != torch.int64 or not t.is_cuda or t.numel() != n:
            raise ValueError(f"{nm}: expected int64 cuda [{n}]")
    if n:
        # torch's advanced indexing (train_ddi_batch.py:286) raises on an index outside the tensor; the kernel would read out of
        # bounds instead, so the ranges are checked here (one small reduction + host read per call; negative indices, which
        # torch would wrap around, never occur in the collator's triples and are refused as well)
        lim = torch.stack([labels.min(), labels.max(), heads.min(), heads.max(), tails.min(), tails.max()]).tolist()
        for (lo, hi), size, nm in zip(((lim[0], lim[1]), (lim[2], lim[3]), (lim[4], lim[5])), s.shape, ("labels", "heads", "tails")):
            if lo < 0 or hi >= size:
                raise IndexError(f"{nm}: index {lo if lo < 0 else hi} is out of bounds for dimension of size {size}")
    pred = torch.empty(n, dtype=torch.float32, device=s.device)
    term = loss = None
    if target is not None:
        target = _f32_cuda(target, "target", 1)
        term = torch.empty(n, dtype=torch.float32, device=s.device)
        loss = torch.zeros(1, dtype=torch.float32, device=s.device)
    call("mdg_gather_bce", _ptr(s), s.shape[0], s.shape[1], s.shape[2], _ptr(labels.contiguous()), _ptr(heads.contiguous()), _ptr(tails.contiguous()),
         _ptr(target), _ptr(pred), _ptr(term), _ptr(loss), n, 1 if apply_sigmoid else 0, _stream(s))
    return pred, (None if loss is None else loss[0])


# ------------------------------------------------------------------------------- rank normalisation
def _scores3(t: torch.Tensor, name: str) -> torch.Tensor:
    """[L,N,N] fp32 GPU tensor, contiguous or row-pitched (empty_scores); anything else is made contiguous."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        return _f32_cuda(t, name, 3)
    if t.numel() and (t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) != t.shape[1] * t.stride(1)):
        return t.contiguous()
    return t


def rank_normalize(scores: torch.Tensor, out: Optional[torch.Tensor] = None, max_workspace_bytes: int = 8 << 30,
                   fallback_flags: Optional[list] = None) -> torch.Tensor:
    """Normalised ranks per outcome (notebooks/normalize_scores.py:36-74): [L,N,N] fp32 -> [L,N,N] fp32.
    Outcomes are processed in chunks sized to ``max_workspace_bytes`` of sort scratch.  ``scores`` / ``out`` may be row-pitched
    (``empty_scores``); without ``out`` the result has the layout of ``scores``.

    ``scores`` of dtype int32 = the lower-triangle order keys of ``bilinear_allpairs(..., epilogue=EPI_TRIKEYS)``: same ranks,
    and without ``out`` they are written over the keys (the returned fp32 tensor shares the keys' memory).

    16-bit scores (``bilinear_allpairs(..., out_dtype=torch.float16 / torch.bfloat16)``) are refused with a ``ValueError``: rounding
    to 11 or 8 significant bits makes scores tie that differ in fp32, and tied scores share a rank here, so the ranks of a 16-bit
    tensor are not the ranks of the model ("Ties in rank normalisation").  Ranks come from fp32 scores or their keys.

    ``fallback_flags`` (diagnostics): a list that receives, per chunk that took the MSD fast path, an int32 tensor with one entry
    per outcome -- non-zero where the fast path handed the outcome to the four-pass LSD sort (same ranks either way)."""
    from_keys = isinstance(scores, torch.Tensor) and scores.dtype == torch.int32
    if from_keys:
        if not (scores.is_cuda and scores.dim() == 3 and (scores.numel() == 0 or (scores.stride(2) == 1 and scores.stride(1) >= scores.shape[2]
                                                                                  and scores.stride(0) == scores.shape[1] * scores.stride(1)))):
            raise ValueError("keys: expected the int32 GPU tensor bilinear_allpairs(..., epilogue=EPI_TRIKEYS) returned")
        s = scores.view(torch.float32)
    else:
        s = _scores3(scores, "scores")
    L, N, N2 = s.shape
    if N != N2:
        raise ValueError("scores: expected [L,N,N]")
    if out is None:
        if from_keys:
            out = s
        else:
            out = empty_scores(L, N, N, s.device) if (N and s.stride(1) != N) else torch.empty((L, N, N), dtype=torch.float32, device=s.device)
    else:
        o2 = _scores3(out, "out")
        if o2 is not out or out.shape != s.shape or (out.data_ptr() == s.data_ptr() and not from_keys):
            raise ValueError("out: an fp32 GPU tensor of the shape of scores (contiguous or row-pitched), not aliasing it")
    if L == 0 or N == 0:
        return out
    entry = "mdg_rank_normalize_keys_ld" if from_keys else "mdg_rank_normalize_ld"
    per = max(lib().mdg_rank_normalize_workspace_bytes(1, N), 1)
    chunk = int(max(1, min(L, 65535, max_workspace_bytes // per)))
    if chunk > 8:
        chunk -= chunk % 8                   # whole launch groups of the MSD path (8 outcomes each): no ragged group at the end of every chunk
    for lo in range(0, L, chunk):
        hi = min(L, lo + chunk)
        ws, nbytes = _scratch("mdg_rank_normalize_workspace_bytes", s.device, hi - lo, N)
        call(entry, s.data_ptr() + lo * s.stride(0) * 4, s.stride(1), out.data_ptr() + lo * out.stride(0) * 4, out.stride(1), hi - lo, N, _ptr(ws),
             nbytes, _stream(s), what="mdg_rank_normalize")
        if fallback_flags is not None and lib().mdg_rank_normalize_fast_path(hi - lo, N):
            fallback_flags.append(ws[: 4 * (hi - lo)].view(torch.int32).clone())
    return out


def _hgt_composite_args(ptrs, k_rel, v_rel, meta):
    nt, R = meta["n_types"], meta["n_edge_types"]
    base = ptrs.data_ptr()
    return (base, base + 8 * nt, _ptr(k_rel), _ptr(v_rel), base + 16 * nt, _ptr(meta["rel_r"]), _ptr(meta["rel_src"]), _ptr(meta["rel_row"]),
            meta["n_rel"], _ptr(meta["type_row"]), nt)


def hgt_composite(ptrs: torch.Tensor, k_rel, v_rel, meta: dict, big_w, big_b) -> None:
    """mdg_hgt_composite_fwd (autograd._HgtComposite): ``ptrs`` = device int64 table [kqv weights | kqv biases | p_rel of every edge type]."""
    call("mdg_hgt_composite_fwd", *_hgt_composite_args(ptrs, k_rel, v_rel, meta), _ptr(big_w), _ptr(big_b), meta["cin"], meta["H"],
         meta["n_edge_types"], meta["F"], _stream(big_w))


def hgt_composite_bwd(ptrs: torch.Tensor, k_rel, v_rel, meta: dict, dbig_w, dbig_b, grads) -> None:
    call("mdg_hgt_composite_bwd", *_hgt_composite_args(ptrs, k_rel, v_rel, meta), _ptr(dbig_w), _ptr(dbig_b), _ptr(grads), meta["cin"], meta["H"],
         meta["n_edge_types"], meta["F"], _stream(grads))


def gmean(tensors) -> torch.Tensor:
    """Elementwise geometric mean of up to 8 equally shaped fp32 tensors (5-seed rank ensembling).  Row-pitched rank tensors
    (``empty_scores``) of one pitch are averaged in place of their padded storage: the result has the same layout."""
    ts = list(tensors)
    if not 1 <= len(ts) <= 8 or any(t.shape != ts[0].shape for t in ts):
        raise ValueError("gmean: 1..8 tensors of identical shape")
    t0 = ts[0]
    pitched = (t0.dim() == 3 and t0.is_cuda and t0.dtype == torch.float32 and t0.numel() > 0 and t0.stride(2) == 1 and t0.stride(1) > t0.shape[2]
               and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.stride() == t0.stride() for t in ts)
               and t0.stride(0) == t0.shape[1] * t0.stride(1))
    if pitched:
        L, N, _ = t0.shape
        P = t0.stride(1)
        full = [t.as_strided((L, N, P), (N * P, P, 1)) for t in ts]          # the padded storage itself: contiguous, n % 4 == 0
        out_full = torch.empty((L, N, P), dtype=torch.float32, device=t0.device)
        arr = (ctypes.c_void_p * len(full))(*[t.data_ptr() for t in full])
        call("mdg_gmean", arr, len(full), _ptr(out_full), L * N * P, _stream(out_full))
        return out_full[:, :, :t0.shape[2]]
    ts = [_f32_cuda(t, f"tensors[{i}]") for i, t in enumerate(ts)]
    out = torch.empty_like(ts[0])
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    call("mdg_gmean", arr, len(ts), _ptr(out), ts[0].numel(), _stream(out))
    return out


def ensemble_ranks(rank_tensors, max_workspace_bytes: int = 8 << 30) -> torch.Tensor:
    """Seed ensembling of the reference (generate_embeddings.ipynb cells 18-20): geometric mean of the seeds'
    normalised-rank tensors, then rank-normalised again per outcome."""
    return rank_normalize(gmean(rank_tensors), max_workspace_bytes=max_workspace_bytes)


# ------------------------------------------------------------------------------- backward building blocks
def _ceil4(n: int) -> int:
    return (n + 3) // 4 * 4


def transpose(x: torch.Tensor, pad_inner: bool = True) -> torch.Tensor:
    """[R, C] (unit inner stride) -> [C, R']; R' = R rounded up to 4 with zero padding when ``pad_inner`` so that the
    result can be an mdg_linear operand as is."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
        x = _f32_cuda(x, "x", 2)
    R, C = x.shape
    Rp = _ceil4(R) if pad_inner else R
    out = (torch.zeros if Rp != R else torch.empty)((C, Rp), dtype=torch.float32, device=x.device)
    call("mdg_transpose", _ptr(x), x.stride(0), _ptr(out), Rp, R, C, _stream(x))
    return out


_wt_cache = {}


def weight_transposed(w: torch.Tensor) -> torch.Tensor:
    """``transpose(w)`` of a parameter, kept per (storage, in-place version): a step differentiates every layer once per
    side / view, so each weight's transpose is needed two or three times between two optimizer updates (which bump the
    version).  The entry keeps ``w`` alive, so its address cannot be recycled under the cache; a new version of the same
    parameter replaces the old entry (memory: one transposed copy per Linear weight)."""
    if w.is_cuda and torch.cuda.is_current_stream_capturing():
        return transpose(w.detach())            # a captured pass must contain the transpose itself: replays see newer weights
    k = (w.data_ptr(), tuple(w.shape), str(w.device))
    hit = _wt_cache.get(k)
    if hit is not None and hit[0] == w._version:
        return hit[1]
    t = transpose(w.detach())
    _wt_cache[k] = (w._version, t, w)
    return t


_wt_img_cache = {}
_param_img_cache = {}


def parameter_images(w: torch.Tensor, precision):
    """(operand image of W, PackedWeight of W^T) of a parameter [N,K] from ONE pass over it (mdg_linear_backward_pack: the kernel that
    packs a gradient both ways), kept per (storage, in-place version, mode): a training step needs both -- W for the forward block,
    W^T for dx -- once per optimizer update.  None in the modes / shapes that take the tensor as it is (callers fall back to the
    separate packs)."""
    prec = _prec(precision)
    if prec == PREC_F32 or w.dim() != 2 or not w.is_contiguous() or w.shape[1] % 4 or w.data_ptr() % 16 or \
            (w.is_cuda and torch.cuda.is_current_stream_capturing()):
        return None
    k = (w.data_ptr(), tuple(w.shape), str(w.device), prec)
    hit = _param_img_cache.get(k)
    if hit is not None and hit[0] == w._version:
        return hit[1], hit[2]
    N, K = w.shape
    rb = lib().mdg_linear_backward_pack_bytes(N, K, prec, 0)
    tb = lib().mdg_linear_backward_pack_bytes(N, K, prec, 1)
    img = torch.empty(rb, dtype=torch.uint8, device=w.device)
    timg = torch.empty(tb, dtype=torch.uint8, device=w.device)
    wd = w.detach()
    call("mdg_linear_backward_pack", _ptr(wd), K, N, K, prec, _ptr(img), _ptr(timg), None, 0.0, 0, None, 0, _stream(wd))
    wt = PackedWeight((K, _ceil4(N)), timg)
    _param_img_cache[k] = (w._version, img, wt, w)
    return img, wt


def transposed_weight_image(w: torch.Tensor, precision):
    """(transpose(w), its operand image) of a parameter, kept per (storage, in-place version, arithmetic mode) like
    ``weight_transposed``: both sides / views of a step multiply their output gradients by the same W.  Image None where the mode
    takes the tensor as it is."""
    prec = _prec(precision)
    if w.is_cuda and torch.cuda.is_current_stream_capturing():
        return transpose(w.detach()), None
    k = (w.data_ptr(), tuple(w.shape), str(w.device), prec)
    hit = _param_img_cache.get(k)
    if hit is not None and hit[0] == w._version:           # made together with W's own image by the forward pass
        return hit[2], hit[2].image
    hit = _wt_img_cache.get(k)
    if hit is not None and hit[0] == w._version:
        return hit[1], hit[2]
    if prec != PREC_F32 and w.is_contiguous():
        # 16-bit modes: W^T is only ever read as an operand image: one transposing pack of W, no fp32 transpose
        N, K = w.shape
        nbytes = lib().mdg_pack_operand_bytes(K, _ceil4(N), prec)
        img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        wd = w.detach()
        call("mdg_pack_operand_transposed", _ptr(wd), wd.stride(0), N, K, prec, _ptr(img), nbytes, _stream(wd))
        wt = PackedWeight((K, _ceil4(N)), img)
        _wt_img_cache[k] = (w._version, wt, img, w)
        return wt, img
    wt = weight_transposed(w)
    nbytes = lib().mdg_pack_operand_bytes(wt.shape[0], wt.shape[1], prec)
    img = None
    if nbytes:
        img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        call("mdg_pack_operand", _ptr(wt), wt.stride(0), wt.shape[0], wt.shape[1], prec, _ptr(img), nbytes, _stream(wt))
    _wt_img_cache[k] = (w._version, wt, img, w)
    return wt, img


def wide_weight_gradient(N: int, K: int) -> bool:
    """dW [N,K] with >= 96 tiles of 128 x 128 fills the chip tile-wise: the 16-bit modes run it as a tile GEMM on transposed images."""
    return ((N + 127) // 128) * ((K + 127) // 128) >= 96


def linear_backward_pack(g: torch.Tensor, precision, want_bias: bool = False, want_row_image: bool = True, dropout_p: float = 0.0,
                         dropout_seed: int = 0):
    """One pass over g = dL/dy [M,N] (contiguous rows, 16-bit operand mode) -> (operand image of g | None, image of g^T, column sums
    of g | None): what the dx GEMM, the dW GEMM and the bias gradient of a wide dense block read (mdg_linear_backward_pack).
    ``dropout_p`` > 0: g is the incoming gradient of a block that ended in dropout(p, seed); the mask is applied while g is read."""
    if g.dim() != 2 or not g.is_cuda or g.dtype != torch.float32 or g.stride(1) != 1:
        raise ValueError("linear_backward_pack: g must be a 2-D fp32 cuda tensor with unit inner stride")
    prec = _prec(precision)
    M, N = g.shape
    rb = lib().mdg_linear_backward_pack_bytes(M, N, prec, 0)
    tb = lib().mdg_linear_backward_pack_bytes(M, N, prec, 1)
    if tb == 0:
        raise ValueError("linear_backward_pack: a 16-bit operand mode (bf16 / bf16x3) and a non-empty g")
    row_img = torch.empty(rb, dtype=torch.uint8, device=g.device) if want_row_image else None
    t_img = torch.empty(tb, dtype=torch.uint8, device=g.device)
    db = torch.empty(N, dtype=torch.float32, device=g.device) if want_bias else None
    nbytes = lib().mdg_linear_backward_pack_bytes(M, N, prec, 2) if want_bias else 0
    ws = _workspace(nbytes, g.device)
    if dropout_p > 0.0 and g.stride(0) != N:
        raise ValueError("linear_backward_pack: the dropout mask is indexed by the contiguous [M,N] position")
    call("mdg_linear_backward_pack", _ptr(g), g.stride(0), M, N, prec, _ptr(row_img), _ptr(t_img), _ptr(db), dropout_p, dropout_seed & (2 ** 64 - 1),
         _ptr(ws), nbytes, _stream(g))
    return row_img, t_img, db


def linear_tn_packed_g(gt_img: torch.Tensor, x: torch.Tensor, N: int, precision, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW [N,K] = g^T x from the image of g^T (linear_backward_pack) and the layer input x [M,K]."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError("linear_tn_packed_g: x must be a 2-D fp32 cuda tensor with unit inner stride")
    M, K = x.shape
    prec = _prec(precision)
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device) if out is None else out
    if tuple(dw.shape) != (N, K) or not dw.is_contiguous() or dw.dtype != torch.float32:
        raise ValueError("linear_tn_packed_g: out must be contiguous fp32 [N,K]")
    ws, nbytes = _scratch("mdg_linear_tn_packed_g_workspace_bytes", x.device, M, N, K, prec)
    call("mdg_linear_tn_packed_g", _ptr(gt_img), _ptr(x), x.stride(0), _ptr(dw), K, M, N, K, prec, _ptr(ws), nbytes, _stream(x))
    return dw


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, beta: float = 0.0) -> torch.Tensor:
    """Column sums of a 2-D tensor (fixed summation order): out = beta * out + x.sum(0)."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
        x = _f32_cuda(x, "x", 2)
    R, C = x.shape
    if out is None:
        out, beta = torch.empty(C, dtype=torch.float32, device=x.device), 0.0
    ws, nbytes = _scratch("mdg_colsum_workspace_bytes", x.device, R, C)
    call("mdg_colsum", _ptr(x), x.stride(0), _ptr(out), R, C, beta, _ptr(ws), nbytes, _stream(x))
    return out


def activation_fwd(pre: torch.Tensor, act) -> torch.Tensor:
    pre = _f32_cuda(pre, "pre")
    y = torch.empty_like(pre)
    call("mdg_activation_fwd", _ptr(pre), _ptr(y), pre.numel(), ACTS[act], _stream(pre))
    return y


def activation_bwd(dy: torch.Tensor, pre: torch.Tensor, act) -> torch.Tensor:
    """dy * act'(pre); for relu ``pre`` may be the activation output itself."""
    dy, pre = _f32_cuda(dy, "dy"), _f32_cuda(pre, "pre")
    if dy.shape != pre.shape:
        raise ValueError("activation_bwd: shape mismatch")
    dx = torch.empty_like(dy)
    call("mdg_activation_bwd", _ptr(dy), _ptr(pre), _ptr(dx), dy.numel(), ACTS[act], _stream(dy))
    return dx


def dropout(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """Inverted dropout with a counter-based mask: the same (seed, p) applied to a gradient is the backward pass."""
    x = _f32_cuda(x, "x")
    y = torch.empty_like(x)
    call("mdg_dropout", _ptr(x), _ptr(y), x.numel(), p, seed & (2 ** 64 - 1), _stream(x))
    return y


def activation_dropout_fwd(pre: torch.Tensor, act, p: float, seed: int) -> torch.Tensor:
    """dropout(act(pre), p, seed) in one pass (same mask as ``dropout``)."""
    pre = _f32_cuda(pre, "pre")
    y = torch.empty_like(pre)
    call("mdg_activation_dropout_fwd", _ptr(pre), _ptr(y), pre.numel(), ACTS[act], p, seed & (2 ** 64 - 1), _stream(pre))
    return y


def activation_dropout_bwd(dy: torch.Tensor, pre: torch.Tensor, act, p: float, seed: int) -> torch.Tensor:
    """act'(pre) * dropout-backward(dy) in one pass."""
    dy, pre = _f32_cuda(dy, "dy"), _f32_cuda(pre, "pre")
    if dy.shape != pre.shape:
        raise ValueError("activation_dropout_bwd: shape mismatch")
    dx = torch.empty_like(dy)
    call("mdg_activation_dropout_bwd", _ptr(dy), _ptr(pre), _ptr(dx), dy.numel(), ACTS[act], p, seed & (2 ** 64 - 1), _stream(dy))
    return dx


def batchnorm_train_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, eps: float, momentum: float, act=None):
    """-> (y, stats[5N]); updates the running statistics in place (nn.BatchNorm1d training semantics)."""
    x = _f32_cuda(x, "x", 2)
    R, C = x.shape
    if R < 2:
        raise ValueError("Expected more than 1 value per channel when training")      # torch's message
    y = torch.empty_like(x)
    stats = torch.empty(5 * C, dtype=torch.float32, device=x.device)
    ws, nbytes = _scratch("mdg_batchnorm_workspace_bytes", x.device, R, C)
    call("mdg_batchnorm_train_fwd", _ptr(x), C, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(y), C, _ptr(stats), R, C, eps,
         momentum, ACTS[act], _ptr(ws), nbytes, _stream(x))
    return y, stats


def batchnorm_replay_update(stats: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor, rows: int, eps: float, momentum: float) -> None:
    """A further momentum update of the running statistics from the batch statistics of an earlier training-mode forward."""
    C = running_mean.numel()
    call("mdg_batchnorm_replay_update", _ptr(stats), _ptr(running_mean), _ptr(running_var), rows, C, eps, momentum, _stream(stats))


def batchnorm_train_bwd(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor):
    """-> (dx, dgamma, dbeta) for the gradient ``dy`` at the BatchNorm output (before any activation)."""
    dy, x = _f32_cuda(dy, "dy", 2), _f32_cuda(x, "x", 2)
    R, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    ws, nbytes = _scratch("mdg_batchnorm_workspace_bytes", x.device, R, C)
    call("mdg_batchnorm_train_bwd", _ptr(dy), _ptr(x), _ptr(stats), _ptr(dx), _ptr(dg), _ptr(db), R, C, _ptr(ws), nbytes, _stream(x))
    return dx, dg, db


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5, extra: Optional[torch.Tensor] = None):
    """-> (dx, dweight, dbias); ``x`` is the LayerNorm input (statistics are recomputed).  ``extra``: a gradient of ``x`` that arrives
    through another consumer (the residual connection of a pre-norm block): dx = LayerNorm-backward(dy) + extra in the same pass."""
    d = x.shape[-1]
    x2 = x.reshape(-1, d) if x.stride(-1) == 1 and x.dim() == 2 else _f32_cuda(x, "x").reshape(-1, d)
    dy2 = dy.reshape(-1, d) if dy.stride(-1) == 1 and dy.dim() == 2 else _f32_cuda(dy, "dy").reshape(-1, d)
    R = x2.shape[0]
    dx = torch.empty((R, d), dtype=torch.float32, device=x2.device)
    dg = torch.empty(d, dtype=torch.float32, device=x2.device)
    db = torch.empty_like(dg)
    ws, nbytes = _scratch("mdg_layernorm_bwd_workspace_bytes", x2.device, R, d)
    if extra is not None:
        e2 = extra.reshape(-1, d) if extra.stride(-1) == 1 and extra.dim() == 2 else _f32_cuda(extra, "extra").reshape(-1, d)
        if e2.shape[0] != R:
            raise ValueError("layernorm_bwd: extra must have the shape of x")
        call("mdg_layernorm_bwd_add", _ptr(dy2), dy2.stride(0), _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(e2), e2.stride(0),
             _ptr(dx), d, _ptr(dg), _ptr(db), R, d, eps, _ptr(ws), nbytes, _stream(x2))
        return dx.view(x.shape), dg, db
    call("mdg_layernorm_bwd", _ptr(dy2), dy2.stride(0), _ptr(x2), x2.stride(0), _ptr(weight.detach().contiguous()), _ptr(dx), d, _ptr(dg), _ptr(db),
         R, d, eps, _ptr(ws), nbytes, _stream(x2))
    return dx.view(x.shape), dg, db


def affine_act(x: torch.Tensor, scale: torch.Tensor, shift: Optional[torch.Tensor] = None, act=None) -> torch.Tensor:
    """act(x * scale + shift) with per-column scale / shift."""
    x = _f32_cuda(x, "x", 2)
    y = torch.empty_like(x)
    call("mdg_affine_act", _ptr(x), x.stride(0), _ptr(scale.contiguous()), _ptr(None if shift is None else shift.contiguous()), _ptr(y), y.stride(0),
         x.shape[0], x.shape[1], ACTS[act], _stream(x))
    return y


def axpby(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0, beta: float = 1.0) -> torch.Tensor:
    """alpha * a + beta * b; ``b`` may be a trailing-dims broadcast of ``a`` (numel(b) divides numel(a))."""
    a, b = _f32_cuda(a, "a"), _f32_cuda(b, "b")
    if a.numel() % max(b.numel(), 1) or (b.numel() != a.numel() and tuple(a.shape[a.dim() - b.dim():]) != tuple(b.shape)):
        raise ValueError(f"axpby: cannot broadcast {tuple(b.shape)} over {tuple(a.shape)}")
    out = torch.empty_like(a)
    call("mdg_axpby", _ptr(a), _ptr(b), _ptr(out), a.numel(), b.numel(), alpha, beta, _stream(a))
    return out


def assemble_tokens_bwd(dseq: torch.Tensor, str_emb, kg_emb, cv_emb, tx_emb, *, bottleneck=None, cls=None, pe_len: int = 0,
                        normalize: bool = False, token_index=None):
    """Gradients of mdg_assemble_tokens (rows=None) -> dict(str, kg, cv, tx, bottleneck, cls, pe)."""
    s, k, c, t = (_f32_cuda(a, nm, 2) for a, nm in ((str_emb, "str"), (kg_emb, "kg"), (cv_emb, "cv"), (tx_emb, "tx")))
    n, D = s.shape
    nb = 0 if bottleneck is None else int(bottleneck.shape[0])
    has_cls = cls is not None
    S = (1 if has_cls else 0) + 3 + nb + 16
    dseq = _f32_cuda(dseq, "dseq").reshape(-1, D)
    n_tok = 0 if token_index is None else int(token_index.numel())
    if dseq.shape[0] != (n * S if token_index is None else n_tok):
        raise ValueError("assemble_tokens_bwd: dseq rows disagree with the token list")
    dev = s.device
    # non-emitted tokens leave zero gradient; dense scratch for the shared tokens is summed over drugs below
    dstr, dkg, dcv = (torch.zeros((n, D), dtype=torch.float32, device=dev) for _ in range(3))
    dtx = torch.zeros((16 * n, D), dtype=torch.float32, device=dev)
    dlearned = torch.zeros((n, S, D), dtype=torch.float32, device=dev) if (nb or has_cls) else None
    dpe = torch.zeros((n, S, D), dtype=torch.float32, device=dev) if pe_len else None
    call("mdg_assemble_tokens_bwd", _ptr(dseq), _ptr(s), _ptr(k), _ptr(c), _ptr(t),
         _ptr(None if bottleneck is None else bottleneck.detach().contiguous()), _ptr(None if cls is None else cls.detach().contiguous()),
         _ptr(None if token_index is None else token_index.contiguous()), n_tok, _ptr(dstr), _ptr(dkg), _ptr(dcv), _ptr(dtx), _ptr(dlearned),
         _ptr(dpe), n, nb, 1 if has_cls else 0, pe_len, 1 if normalize else 0, D, _stream(s))
    out = {"str": dstr, "kg": dkg, "cv": dcv, "tx": dtx, "bottleneck": None, "cls": None, "pe": None}
    if dlearned is not None:
        tot = colsum(dlearned.view(n, S * D)).view(S, D)
        off = 1 if has_cls else 0
        if has_cls:
            out["cls"] = tot[0]
        if nb:
            out["bottleneck"] = tot[off + 3: off + 3 + nb]
    if dpe is not None:
        out["pe"] = colsum(dpe.view(n, S * D)).view(S, D)[:pe_len]
    return out


def l2_normalize_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    dy, x = _f32_cuda(dy, "dy", 2), _f32_cuda(x, "x", 2)
    if x.shape[1] % 4:
        raise ValueError("l2_normalize_bwd: feature dim must be a multiple of 4")
    dx = torch.empty_like(x)
    call("mdg_l2_normalize_bwd", _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dx), dx.stride(0), x.shape[0], x.shape[1], _stream(x))
    return dx


# ------------------------------------------------------------------------------- gathered head (finetune step)
def triple_plan(labels: torch.Tensor, heads: torch.Tensor, tails: torch.Tensor, n_labels: int, n_head: int, n_tail: int) -> dict:
    """Index plumbing for the gathered head: triples sorted by label (and by head drug inside a label), cut into tiles of <= 32 and
    chunks of <= 256 triples of one label; CSR lists of the sorted triples per head drug and per tail drug for the gradient row sums;
    the table of (label, head drug) PAIRS (the batch holds more labelled triples than pairs, and every 128 x 128 product of the head
    depends on the pair only: bilinear_gather_pairs / _bwd).  The reference feeds a new batch of triples to every step
    (train_ddi_batch.py:231-354), so this runs per step: the three sorts are rocprim's (torch.sort), everything between them is the
    mdg_plan_* kernels (csrc/plan.hip) -- ~45 launches and two host reads of a few sizes, where index / scan / repeat_interleave calls
    took ~300 launches and 5 ms of wall time.  tests/helpers.triple_plan_torch is that earlier construction, kept as the checker."""
    T = int(labels.numel())
    dev = labels.device
    for nm, t in (("labels", labels), ("heads", heads), ("tails", tails)):
        if t.dtype != torch.int64 or not t.is_cuda or t.numel() != T or t.dim() != 1:
            raise ValueError(f"{nm}: expected int64 cuda [{T}]")
    st = _stream(labels)
    labels, heads, tails = labels.contiguous(), heads.contiguous(), tails.contiguous()
    i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=dev)

    def bounds(vals, n_vals, scale, n_bounds):
        out = i64(n_bounds)
        call("mdg_plan_lower_bounds", _ptr(vals), vals.element_size(), n_vals, scale, n_bounds, _ptr(out), st)
        return out

    def by_drug(idx, n):
        """CSR pointer over the drugs + the stable order of the entries by drug (16-bit keys when they fit: half the radix passes)."""
        cast = torch.int16 if n <= 32767 else (torch.int32 if n < 2 ** 31 else torch.int64)
        vals, order = torch.sort(idx.to(cast), stable=True)
        return bounds(vals, idx.numel(), 1, n + 1), order

    def cut_count(ptr, n, size, totals_row):
        first = i64(n + 1)
        call("mdg_plan_cut_count", _ptr(ptr), n, size, _ptr(first), _ptr(totals_row), st)
        return first

    def cut_fill(ptr, first, n, size, total, want_which=True):
        which = i64(total) if want_which else None
        start = i64(total + 1)
        call("mdg_plan_cut_fill", _ptr(ptr), _ptr(first), n, size, total, _ptr(which), _ptr(start), st)
        return which, start

    # ONE sort serves the label order and the (label, head drug) pair order: by label, then by head inside a label (any
    # label-sorted order will do for the tiles; a pair's triples must be consecutive for the pair-compressed head).
    # int32 keys when they fit (twice the radix-sort rate).
    big = n_labels * max(n_head, 1) >= 2 ** 31
    key = labels * n_head + heads
    perm = torch.argsort(key if big else key.to(torch.int32), stable=True)
    hs, ts, skey, inv = i64(T), i64(T), i64(T), i64(T)
    sizes = torch.zeros((8, 2), dtype=torch.int64, device=dev)          # rows: tiles | chunks | head pieces | tail pieces | P | status
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    call("mdg_plan_gather", _ptr(perm), _ptr(labels), _ptr(heads), _ptr(tails), T, n_labels, n_head, n_tail, _ptr(hs), _ptr(ts), _ptr(skey),
         _ptr(inv), _ptr(status), st)
    label_ptr = bounds(skey, T, n_head, n_labels + 1)
    head_ptr, head_rows = by_drug(hs, n_head)
    tail_ptr, tail_rows = by_drug(ts, n_tail)
    tile_first = cut_count(label_ptr, n_labels, 32, sizes[0])
    chunk_first = cut_count(label_ptr, n_labels, 256, sizes[1])
    hp_first = cut_count(head_ptr, n_head, 64, sizes[2])
    tp_first = cut_count(tail_ptr, n_tail, 64, sizes[3])
    pair_of = None
    if T:
        flag = i64(T)
        call("mdg_plan_pair_flags", _ptr(skey), T, _ptr(flag), st)
        pair_of = torch.cumsum(flag, 0)                               # sorted triple -> its pair
        sizes[4, 0].copy_(pair_of[T - 1])
    sizes[5, 0].copy_(status[0])
    host = sizes.cpu()                                                # the first of two host reads
    if int(host[5, 0]) & 1:
        raise ValueError("labels: value outside [0, n_labels)")
    if int(host[5, 0]) & 2:
        raise ValueError("heads / tails: index outside the embedding tables")
    n_tiles, n_chunks = int(host[0, 0]), int(host[1, 0])
    tile_label, tile_start = cut_fill(label_ptr, tile_first, n_labels, 32, n_tiles)
    _, chunk_start = cut_fill(label_ptr, chunk_first, n_labels, 256, n_chunks, want_which=False)

    def pieces(ptr, first, n, total, longest):
        """A drug's list can hold thousands of entries while mdg_csr_aggregate gives a row to one group of lanes: every list cut into
        pieces of <= 64 entries -> (piece_ptr over the entries, row_ptr over the pieces) for a two-level sum (_sum_rows); None when
        no list is long enough to matter."""
        if n == 0 or longest <= 256:
            return None
        return cut_fill(ptr, first, n, 64, total, want_which=False)[1], first
    head_pieces = pieces(head_ptr, hp_first, n_head, int(host[2, 0]), int(host[2, 1]))
    tail_pieces = pieces(tail_ptr, tp_first, n_tail, int(host[3, 0]), int(host[3, 1]))
    # ---- (label, head drug) PAIRS: the plan's triple order IS the pair order; pair p owns the triples pair_ptr[p] .. pair_ptr[p+1]
    pairs = None
    if T:
        P = int(host[4, 0]) + 1
        pair_ptr, pair_drug = i64(P + 1), i64(P)
        call("mdg_plan_pair_table", _ptr(skey), _ptr(pair_of), T, n_head, P, _ptr(pair_ptr), _ptr(pair_drug), st)
        plabel_ptr = i64(n_labels + 1)                                  # first pair of every label (= the pair of its first triple)
        call("mdg_plan_take", _ptr(pair_of), _ptr(label_ptr), n_labels + 1, T, P, _ptr(plabel_ptr), st)
        psizes = torch.zeros((4, 2), dtype=torch.int64, device=dev)     # rows: pair tiles | pair chunks | drug pieces
        ptile_first = cut_count(plabel_ptr, n_labels, 32, psizes[0])
        pchunk_first = cut_count(plabel_ptr, n_labels, 512, psizes[1])  # (256: 0.82 ms, 512 / 1024: 0.75 ms, 2048: 1.05 ms for the 2.4e6 pairs of the bench step)
        drug_ptr, drug_rows = by_drug(pair_drug, n_head)
        dp_first = cut_count(drug_ptr, n_head, 64, psizes[2])
        of_triple_by_tail = pair_of[tail_rows]
        phost = psizes.cpu()                                            # the second host read
        pn_tiles, pn_chunks = int(phost[0, 0]), int(phost[1, 0])
        ptile_label, ptile_start = cut_fill(plabel_ptr, ptile_first, n_labels, 32, pn_tiles)
        _, pchunk_start = cut_fill(plabel_ptr, pchunk_first, n_labels, 512, pn_chunks, want_which=False)
        pairs = {"P": P, "drug": pair_drug, "ptr": pair_ptr, "tails_by_pair": ts,
                 "of_triple": pair_of, "tile_start": ptile_start, "tile_label": ptile_label, "n_tiles": pn_tiles,
                 "chunk_start": pchunk_start, "n_chunks": pn_chunks, "label_chunk_ptr": pchunk_first, "drug_ptr": drug_ptr, "drug_rows": drug_rows,
                 "of_triple_by_tail": of_triple_by_tail, "drug_pieces": pieces(drug_ptr, dp_first, n_head, int(phost[2, 0]), int(phost[2, 1]))}
    return {"T": T, "L": n_labels, "n_head": n_head, "n_tail": n_tail, "perm": perm, "inv_perm": inv, "heads": hs, "tails": ts, "pairs": pairs,
            "tile_start": tile_start, "tile_label": tile_label, "n_tiles": n_tiles, "chunk_start": chunk_start,
            "n_chunks": n_chunks, "label_chunk_ptr": chunk_first, "head_ptr": head_ptr,
            "head_rows": head_rows, "tail_ptr": tail_ptr, "tail_rows": tail_rows, "head_pieces": head_pieces,
            "tail_pieces": tail_pieces}


def _sum_rows(x, ptr, rows, pieces, edge_weight=None):
    """csr_aggregate(x, ptr, rows) with the long lists cut into the plan's pieces: piece sums first (many short rows), then
    the pieces of a drug in order.  Same fixed order of additions from run to run."""
    if pieces is None:
        return csr_aggregate(x, ptr, rows, edge_weight=edge_weight)
    part = csr_aggregate(x, pieces[0], rows, edge_weight=edge_weight)
    return csr_aggregate(part, pieces[1], None)


def bilinear_gather(z_head: torch.Tensor, z_tail: torch.Tensor, w: torch.Tensor, plan: dict) -> torch.Tensor:
    """score[t] = z_head[h_t]^T w[l_t] z_tail[t_t] for the plan's triples, in the plan's (label-sorted) order."""
    zh, zt, w = _f32_cuda(z_head, "z_head", 2), _f32_cuda(z_tail, "z_tail", 2), _f32_cuda(w, "w", 3)
    if zh.shape != (plan["n_head"], 128) or zt.shape != (plan["n_tail"], 128) or w.shape != (plan["L"], 128, 128):
        raise ValueError("bilinear_gather: operands disagree with the plan (D must be 128)")
    score = torch.empty(plan["T"], dtype=torch.float32, device=zh.device)
    call("mdg_bilinear_gather", _ptr(zh), _ptr(zt), _ptr(w), _ptr(plan["heads"]), _ptr(plan["tails"]), _ptr(plan["tile_start"]),
         _ptr(plan["tile_label"]), plan["n_tiles"], _ptr(score), 128, _stream(zh))
    return score


def bilinear_gather_bwd(z_head, z_tail, w, plan: dict, dscore: torch.Tensor, w_t: Optional[torch.Tensor] = None, need_dw: bool = True):
    """-> (dz_head [Nh,128], dz_tail [Nt,128], dw [L,128,128] | None).  ``w_t``: per-label transpose of ``w`` (omit when
    ``w`` is symmetric)."""
    zh, zt, w = _f32_cuda(z_head, "z_head", 2), _f32_cuda(z_tail, "z_tail", 2), _f32_cuda(w, "w", 3)
    ds = _f32_cuda(dscore, "dscore", 1)
    T, L, dev = plan["T"], plan["L"], zh.device
    if ds.numel() != T:
        raise ValueError("dscore: one entry per triple expected")
    wt = w if w_t is None else _f32_cuda(w_t, "w_t", 3)
    gh = torch.empty((T, 128), dtype=torch.float32, device=dev)
    gt = torch.empty((T, 128), dtype=torch.float32, device=dev)
    dw = torch.empty((L, 128, 128), dtype=torch.float32, device=dev) if need_dw else None
    part = torch.empty((max(plan["n_chunks"], 1), 128, 128), dtype=torch.float32, device=dev) if need_dw else None
    call("mdg_bilinear_gather_bwd", _ptr(zh), _ptr(zt), _ptr(w), _ptr(wt), _ptr(plan["heads"]), _ptr(plan["tails"]), _ptr(plan["tile_start"]),
         _ptr(plan["tile_label"]), plan["n_tiles"], _ptr(plan["chunk_start"]), plan["n_chunks"], _ptr(plan["label_chunk_ptr"]), L, _ptr(ds), _ptr(gh),
         _ptr(gt), _ptr(part), _ptr(dw), 128, _stream(zh))
    dzh = _sum_rows(gh, plan["head_ptr"], plan["head_rows"], plan.get("head_pieces"))
    dzt = _sum_rows(gt, plan["tail_ptr"], plan["tail_rows"], plan.get("tail_pieces"))
    return dzh, dzt, dw


def _matvec_rows(z, w, row_index, pp, out, precision):
    """rows[p] = W[label of p] z[row_index[p]] per (label, drug) pair, in the step's arithmetic mode (exact fp32 / split-bf16 matrix cores)."""
    prec = _prec(precision)
    ws, nbytes = _scratch("mdg_bilinear_matvec_rows_workspace_bytes", z.device, w.shape[0], prec)
    call("mdg_bilinear_matvec_rows_prec", _ptr(z), _ptr(w), w.shape[0], _ptr(row_index), _ptr(pp["tile_start"]), _ptr(pp["tile_label"]),
         pp["n_tiles"], _ptr(out), 128, prec, _ptr(ws), nbytes, _stream(z), what="mdg_bilinear_matvec_rows")


def bilinear_gather_pairs(z_head: torch.Tensor, z_tail: torch.Tensor, w: torch.Tensor, plan: dict, w_t: Optional[torch.Tensor] = None,
                          precision="f32"):
    """The scores of bilinear_gather through the (label, head drug) pairs: V[p] = W[l_p]^T z_head[i_p] once per pair (the 128 x 128
    product), then score[t] = V[pair(t)] . z_tail[t_t].  -> (score [T] in the plan's order, V [P,128] for the backward pass)."""
    zh, zt, w = _f32_cuda(z_head, "z_head", 2), _f32_cuda(z_tail, "z_tail", 2), _f32_cuda(w, "w", 3)
    if zh.shape != (plan["n_head"], 128) or zt.shape != (plan["n_tail"], 128) or w.shape != (plan["L"], 128, 128):
        raise ValueError("bilinear_gather_pairs: operands disagree with the plan (D must be 128)")
    pp = plan["pairs"]
    score = torch.empty(plan["T"], dtype=torch.float32, device=zh.device)
    if pp is None:
        return score, torch.empty((0, 128), dtype=torch.float32, device=zh.device)
    wt = w if w_t is None else _f32_cuda(w_t, "w_t", 3)
    V = torch.empty((pp["P"], 128), dtype=torch.float32, device=zh.device)
    _matvec_rows(zh, wt, pp["drug"], pp, V, precision)
    call("mdg_gather_rowdot", _ptr(V), _ptr(pp["of_triple"]), _ptr(zt), _ptr(plan["tails"]), _ptr(score), plan["T"], 128, _stream(zh))
    return score, V


def bilinear_gather_pairs_bwd(z_head, z_tail, w, plan: dict, dscore: torch.Tensor, V: torch.Tensor, need_dw: bool = True, precision="f32"):
    """Backward of bilinear_gather_pairs -> (dz_head, dz_tail, dw | None), one 128 x 128 product per PAIR:
        dz_tail[j]  = sum_{t: tail = j} ds_t V[pair(t)]                      (V = W^T z_head: saved by the forward pass)
        u[p]        = sum_{t in pair p} ds_t z_tail[t_t]
        dz_head[i]  = sum_{p: drug = i} W[l_p] u[p]
        dW[l]       = sum_{p: label = l} z_head[i_p] u[p]^T
    Sums run in fixed (sorted) order, no atomics."""
    zh, zt, w = _f32_cuda(z_head, "z_head", 2), _f32_cuda(z_tail, "z_tail", 2), _f32_cuda(w, "w", 3)
    ds = _f32_cuda(dscore, "dscore", 1)
    T, L, dev = plan["T"], plan["L"], zh.device
    if ds.numel() != T:
        raise ValueError("dscore: one entry per triple expected")
    pp = plan["pairs"]
    if pp is None:
        z = torch.zeros
        return z((plan["n_head"], 128), device=dev), z((plan["n_tail"], 128), device=dev), (z((L, 128, 128), device=dev) if need_dw else None)
    dzt = _sum_rows(V, plan["tail_ptr"], pp["of_triple_by_tail"], plan.get("tail_pieces"), edge_weight=ds.index_select(0, plan["tail_rows"]))
    u = csr_aggregate(zt, pp["ptr"], pp["tails_by_pair"], edge_weight=ds)
    R = torch.empty((pp["P"], 128), dtype=torch.float32, device=dev)
    _matvec_rows(u, w, None, pp, R, precision)
    dzh = _sum_rows(R, pp["drug_ptr"], pp["drug_rows"], pp.get("drug_pieces"))
    dw = None
    if need_dw:
        dw = torch.empty((L, 128, 128), dtype=torch.float32, device=dev)
        part = torch.empty((max(pp["n_chunks"], 1), 128, 128), dtype=torch.float32, device=dev)
        call("mdg_bilinear_gather_bwd_prec", _ptr(zh), _ptr(u), _ptr(w), _ptr(w), _ptr(pp["drug"]), None, None, None, 0,
             _ptr(pp["chunk_start"]), pp["n_chunks"], _ptr(pp["label_chunk_ptr"]), L, None, None, None, _ptr(part), _ptr(dw), 128,
             _prec(precision), _stream(zh), what="mdg_bilinear_gather_bwd")
    return dzh[:, :128], dzt[:, :128], dw


def bce_logits(score: torch.Tensor, target: torch.Tensor, want_term: bool = True, grad_scale: Optional[float] = None):
    """-> (term | None, dscore | None): nn.BCELoss(sigmoid(score), target) per element and its logit gradient * grad_scale."""
    s, y = _f32_cuda(score, "score", 1), _f32_cuda(target, "target", 1)
    if s.shape != y.shape:
        raise ValueError("bce_logits: shape mismatch")
    term = torch.empty_like(s) if want_term else None
    ds = torch.empty_like(s) if grad_scale is not None else None
    call("mdg_bce_logits", _ptr(s), _ptr(y), _ptr(term), _ptr(ds), s.numel(), grad_scale or 0.0, _stream(s))
    return term, ds


def symmetrize_bwd(dw_sym: torch.Tensor) -> torch.Tensor:
    dws = _f32_cuda(dw_sym, "dw_sym", 3)
    out = torch.empty_like(dws)
    call("mdg_symmetrize_bwd", _ptr(dws), _ptr(out), dws.shape[0], dws.shape[1], _stream(dws))
    return out


def mul_device_scalar(x: torch.Tensor, scalar: torch.Tensor) -> torch.Tensor:
    x = _f32_cuda(x, "x")
    s = _f32_cuda(scalar.reshape(1), "scalar", 1)
    out = torch.empty_like(x)
    call("mdg_mul_device_scalar", _ptr(x), _ptr(s), _ptr(out), x.numel(), _stream(x))
    return out


# ------------------------------------------------------------------------------- HGT attention, training
def f32_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 mirror (round to nearest even) of a contiguous fp32 tensor whose element count is a multiple of 8 (mdg_f32_to_bf16)."""
    x = _f32_cuda(x, "x")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("mdg_f32_to_bf16", _ptr(x), _ptr(y), x.numel(), _stream(x))
    return y


def _kv16_ok(kv: torch.Tensor, kv16: Optional[torch.Tensor]) -> None:
    if kv16 is not None and (kv16.dtype != torch.bfloat16 or kv16.shape != kv.shape or not kv16.is_contiguous() or kv16.device != kv.device or
                             kv.stride(0) != 128):
        raise ValueError("kv16: the bf16 mirror of kv (same [rows,128] shape, contiguous, same device)")


def hgt_attention_stats(q: torch.Tensor, kv: torch.Tensor, plan: dict, heads: int, kv16: Optional[torch.Tensor] = None):
    """mdg_hgt_attention without the activation -> (out_pre [n_dst,128], stats [n_dst,heads,2]).  ``kv16``: bf16 mirror of ``kv``
    (f32_to_bf16) to gather the k' | v' rows from -- the reduced-precision mode's half-size rows."""
    n_dst = q.shape[0]
    _kv16_ok(kv, kv16)
    if q.dim() != 2 or q.shape[1] != 128 or q.stride(1) != 1 or not q.is_cuda or q.dtype != torch.float32:
        raise ValueError("q: expected fp32 cuda [n_dst,128] with unit inner stride")
    out = torch.empty((n_dst, 128), dtype=torch.float32, device=q.device)
    stats = torch.empty((n_dst, heads, 2), dtype=torch.float32, device=q.device)
    n_items = int(plan["item_dst"].numel())
    ws, nbytes = _scratch("mdg_hgt_attention_workspace_bytes", q.device, n_items, heads)
    call("mdg_hgt_attention_stats", _ptr(q), q.stride(0), _ptr(kv), 0 if kv is None else kv.stride(0), _ptr(plan["col"]), _ptr(plan["item_dst"]),
         _ptr(plan["item_begin"]), _ptr(plan["item_end"]), n_items, _ptr(plan["item_ptr"]), _ptr(out), 128, n_dst, heads, 128, 0, _ptr(stats),
         _ptr(kv16), _ptr(ws), nbytes, _stream(q))
    return out, stats


def hgt_attention_bwd(q: torch.Tensor, kv: torch.Tensor, plan: dict, rev: dict, heads: int, dout: torch.Tensor, out_pre: torch.Tensor,
                      stats: torch.Tensor, dkv: torch.Tensor, dq_out: Optional[torch.Tensor] = None,
                      kv16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dq [n_dst,128]; writes this destination type's key / value gradient rows into ``dkv`` (layout of ``kv``).
    ``dq_out``: write dq there instead (a [n_dst,128] view with unit inner stride, e.g. the query slots of ``dkv`` itself).
    ``kv16``: the bf16 mirror the forward pass gathered from (the same rounded rows enter dq and the softmax gradient)."""
    n_dst = q.shape[0]
    _kv16_ok(kv, kv16)
    dout = _f32_cuda(dout, "dout", 2)
    if kv.dim() != 2 or kv.shape[1] != 128 or not kv.is_contiguous() or dkv.shape != kv.shape or not dkv.is_contiguous():
        raise ValueError("hgt_attention_bwd: kv / dkv must be contiguous [rows,128] (value rows follow key rows)")
    if dq_out is None:
        dq = torch.empty((n_dst, 128), dtype=torch.float32, device=q.device)
    else:
        dq = dq_out
        if dq.shape != (n_dst, 128) or dq.stride(1) != 1 or dq.stride(0) % 4 or dq.dtype != torch.float32 or not dq.is_cuda:
            raise ValueError("hgt_attention_bwd: dq_out must be an fp32 cuda [n_dst,128] view with unit inner stride")
    nnz, n_items = int(plan["col"].numel()), int(plan["item_dst"].numel())
    ws, nbytes = _scratch("mdg_hgt_attention_bwd_workspace_bytes", q.device, nnz, n_items, rev["n_items"], heads)
    call("mdg_hgt_attention_bwd", _ptr(q), q.stride(0), _ptr(kv), 128, _ptr(plan["col"]), nnz, _ptr(plan["item_dst"]), _ptr(plan["item_begin"]),
         _ptr(plan["item_end"]), n_items, _ptr(plan["item_ptr"]), n_dst, _ptr(dout), dout.stride(0), _ptr(out_pre), out_pre.stride(0), _ptr(stats),
         heads, _ptr(rev["t_edge"]), _ptr(rev["t_dst"]), _ptr(rev["item_begin"]), _ptr(rev["item_end"]), rev["n_items"], _ptr(rev["item_ptr"]),
         _ptr(rev["rows"]), rev["n_rows"], _ptr(rev.get("item_row")), _ptr(dq), dq.stride(0), _ptr(dkv), 128, _ptr(kv16), _ptr(ws), nbytes,
         _stream(q))
    return dq


def gated_residual(o: torch.Tensor, x: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    """sigmoid(skip) * o + (1 - sigmoid(skip)) * x, the gate read on the device."""
    o, x = _f32_cuda(o, "o", 2), _f32_cuda(x, "x", 2)
    if o.shape != x.shape:
        raise ValueError("gated_residual: shape mismatch")
    out = torch.empty_like(o)
    call("mdg_gated_residual", _ptr(o), _ptr(x), _ptr(_f32_cuda(skip.reshape(1), "skip", 1)), _ptr(out), o.numel(), _stream(o))
    return out


def gated_residual_bwd(dout: torch.Tensor, o: torch.Tensor, x: torch.Tensor, skip: torch.Tensor):
    """-> (d_o, d_x, d_skip [1])."""
    dout, o, x = _f32_cuda(dout, "dout", 2), _f32_cuda(o, "o", 2), _f32_cuda(x, "x", 2)
    d_o, d_x = torch.empty_like(o), torch.empty_like(o)
    rowdot = torch.empty(o.shape[0], dtype=torch.float32, device=o.device)
    call("mdg_gated_residual_bwd", _ptr(dout), _ptr(o), _ptr(x), _ptr(_f32_cuda(skip.reshape(1), "skip", 1)), _ptr(d_o), _ptr(d_x), _ptr(rowdot),
         o.shape[0], o.shape[1], _stream(o))
    return d_o, d_x, colsum(rowdot.view(-1, 1))


def grad_weight(g: torch.Tensor, x: torch.Tensor, precision="f32", want_bias: bool = False, out=None):
    """dW [N,K] = g^T x for g [M,N], x [M,K] (row-major, unit inner stride; rows may be strided); with ``want_bias`` also
    db [N] = column sums of g -> (dW, db).

    Small outputs (the usual case: 128..512-wide layers over 10^4..10^6 rows) run a split-reduction kernel, which produces the bias
    gradient on the side: exact fp32 matrix cores for "f32", operands rounded (bf16) / split (bf16x3) while staged for the 16-bit
    modes (mdg_grad_weight_prec).  Outputs with >= 96 tiles of 128x128 (the 2048-wide fusion transformer)
    already fill the chip tile-wise: in the bf16 modes they go through the forward GEMM kernel on transposed operands,
    ~5x the fp32 matrix-core rate."""
    if out is not None:                         # (dW, db | None): contiguous fp32 tensors to write into (row blocks of a stacked gradient)
        ow, ob = out
        if tuple(ow.shape) != (g.shape[1], x.shape[1]) or not ow.is_contiguous() or ow.dtype != torch.float32 or \
                (want_bias and (ob is None or ob.numel() != g.shape[1] or not ob.is_contiguous())):
            raise ValueError("grad_weight: out must be contiguous fp32 (dW [N,K], db [N])")
    if g.dim() == 2 and x.dim() == 2 and g.shape[0] == 0 and x.shape[0] == 0:          # no rows: exact zeros
        if out is not None:
            out[0].zero_()
            if want_bias:
                out[1].zero_()
            return out if want_bias else out[0]
        dw = torch.zeros((g.shape[1], x.shape[1]), dtype=torch.float32, device=g.device)
        return (dw, torch.zeros(g.shape[1], dtype=torch.float32, device=g.device)) if want_bias else dw
    for nm, v in (("g", g), ("x", x)):
        if v.dim() != 2 or not v.is_cuda or v.dtype != torch.float32 or v.stride(1) != 1:
            raise ValueError(f"grad_weight: {nm} must be a 2-D fp32 cuda tensor with unit inner stride")
    if g.shape[0] != x.shape[0]:
        raise ValueError("grad_weight: g and x disagree in the number of rows")
    M, N, K = g.shape[0], g.shape[1], x.shape[1]
    if _prec(precision) != PREC_F32 and wide_weight_gradient(N, K):
        prec = _prec(precision)
        dw = torch.empty((N, K), dtype=torch.float32, device=g.device) if out is None else out[0]
        ws, nbytes = _scratch("mdg_linear_tn_workspace_bytes", g.device, M, N, K, prec)
        call("mdg_linear_tn", _ptr(g), g.stride(0), _ptr(x), x.stride(0), _ptr(dw), K, M, N, K, prec, _ptr(ws), nbytes, _stream(g))
        if not want_bias:
            return dw
        if out is None:
            return dw, colsum(g)
        out[1].copy_(colsum(g))
        return dw, out[1]
    dw = torch.empty((N, K), dtype=torch.float32, device=g.device) if out is None else out[0]
    db = (torch.empty(N, dtype=torch.float32, device=g.device) if out is None else out[1]) if want_bias else None
    ws, nbytes = _scratch("mdg_grad_weight_workspace_bytes", g.device, M, N, K)
    call("mdg_grad_weight_prec", _ptr(g), g.stride(0), _ptr(x), x.stride(0), _ptr(dw), _ptr(db), M, N, K, _prec(precision), _ptr(ws), nbytes,
         _stream(g), what="mdg_grad_weight")
    return (dw, db) if want_bias else dw


def info_nce_bwd(sim: torch.Tensor, too_hard_neg: Optional[torch.Tensor], dloss: torch.Tensor, temperature: float) -> torch.Tensor:
    """d loss / d sim for the InfoNCE finish (sim = F F^T [2B,2B]); ``dloss`` is a device scalar."""
    sim = _f32_cuda(sim, "sim", 2)
    B = sim.shape[0] // 2
    hard = None if too_hard_neg is None else too_hard_neg.to(device=sim.device, dtype=torch.uint8).contiguous()
    dsim = torch.empty_like(sim)
    call("mdg_infonce_bwd", _ptr(sim), _ptr(hard), _ptr(_f32_cuda(dloss.reshape(1), "dloss", 1)), _ptr(dsim), B, temperature, _stream(sim))
    return dsim


# ------------------------------------------------------------------------------- SyncBatchNorm (phased BatchNorm)
def _col_reduce(x, y, center, rstd, mode: int) -> torch.Tensor:
    R, C = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws, nbytes = _scratch("mdg_batchnorm_workspace_bytes", x.device, max(R, 1), C)
    call("mdg_col_reduce", _ptr(x), x.stride(0), _ptr(y), 0 if y is None else y.stride(0), _ptr(center), _ptr(rstd), _ptr(out), R, C, mode, _ptr(ws),
         nbytes, _stream(x))
    return out


def sync_batchnorm_train_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, eps: float, momentum: float, act, reduce_):
    """BatchNorm1d training forward with statistics over all ranks: ``reduce_(t)`` sums a small device tensor over ranks
    in place.  The total row count stays on the device (no host read inside the step).  -> (y, stats[5C], count_dev[1])."""
    x = _f32_cuda(x, "x", 2)
    R, C = x.shape
    cnt = torch.tensor([float(R)], dtype=torch.float64).to(x.device, non_blocking=True)
    s = _col_reduce(x, None, None, None, 0)
    reduce_(s)
    reduce_(cnt)
    stats = torch.empty(5 * C, dtype=torch.float32, device=x.device)
    tail = (_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(stats), 0.0, _ptr(cnt), C, eps, momentum)
    call("mdg_batchnorm_finalize", _ptr(s), None, *tail, 0, _stream(x))
    q = _col_reduce(x, None, stats, None, 1)
    reduce_(q)
    call("mdg_batchnorm_finalize", _ptr(s), _ptr(q), *tail, 1, _stream(x))
    y = affine_act(x, stats[2 * C:3 * C], stats[3 * C:4 * C], act)
    return y, stats, cnt


def sync_batchnorm_train_bwd(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, count: torch.Tensor, reduce_):
    """-> (dx, dgamma_local, dbeta_local): dx uses the sums over ALL ranks, the parameter gradients stay local partial sums
    (they are summed over ranks with every other parameter gradient)."""
    dy, x = _f32_cuda(dy, "dy", 2), _f32_cuda(x, "x", 2)
    R, C = x.shape
    db = _col_reduce(dy, None, None, None, 0)
    dg = _col_reduce(dy, x, stats[0:C], stats[C:2 * C], 2)
    both = torch.cat([db, dg])
    reduce_(both)
    dx = torch.empty_like(x)
    call("mdg_batchnorm_bwd_apply", _ptr(dy), _ptr(x), _ptr(stats), _ptr(both[:C].contiguous()), _ptr(both[C:].contiguous()), _ptr(dx), R, C, 0.0,
         _ptr(count), _stream(x))
    return dx, dg, db


# ------------------------------------------------------------------------------- evaluation metrics
LABEL_METRIC_NAMES = ("fmax", "mcc", "auroc", "auprc", "npv", "specificity", "f1", "recall@k", "precision@k", "ap@k",
                      "accuracy", "precision", "recall")
_LABEL_METRIC_STATUS = ((1, "pred holds a NaN or infinite value"), (2, "a label is outside [0, n_labels)"),
                        (4, "target holds a value other than 0 and 1"), (8, "k resolves to 0 for a label (k * n_label < 1)"))


def label_metrics(pred: torch.Tensor, target: torch.Tensor, label: torch.Tensor, n_labels: int, k=50, threshold: float = 0.5) -> dict:
    """Per-label metrics of get_metrics_binary (madrigal/evaluate/metrics.py:60-118) for every label at once (csrc/eval_metrics.hip).

    pred / target fp32 [T] (target 0 or 1), label int64 [T] in [0, n_labels).  ``k`` is an int > 0, or a float in (0, 1) resolved per
    label to int(k * n_label).  Returns device tensors: ``values`` float64 [13, n_labels] in the order of LABEL_METRIC_NAMES (NaN
    columns for labels without triples), ``count`` / ``pos`` / ``k_eff`` int64 [n_labels].  One host read (the status word): raises
    ValueError on a NaN / infinite pred, a label out of range, a target other than 0/1, or k resolving to 0."""
    pred, target = _f32_cuda(pred, "pred", 1), _f32_cuda(target, "target", 1)
    T = int(pred.numel())
    if not (isinstance(label, torch.Tensor) and label.is_cuda and label.dtype == torch.int64 and label.dim() == 1 and label.numel() == T):
        raise ValueError(f"label: expected int64 cuda [{T}]")
    if target.numel() != T or pred.device != target.device or pred.device != label.device:
        raise ValueError("label_metrics: pred, target and label must be [T] on one device")
    if not 0 < T < 2 ** 31:
        raise ValueError(f"label_metrics: need 0 < T < 2^31 triples, got {T}")
    n_labels = int(n_labels)
    if not 0 < n_labels <= 65536:
        raise ValueError(f"label_metrics: need 0 < n_labels <= 65536, got {n_labels}")
    if isinstance(k, bool) or not isinstance(k, (int, float)):
        raise ValueError(f"label_metrics: k must be an int or a float in (0, 1), got {k!r}")
    if isinstance(k, float):
        if not 0.0 < k < 1.0:
            raise ValueError(f"label_metrics: a float k must lie in (0, 1), got {k}")
        k_int, k_frac = 0, float(k)
    else:
        if k <= 0:
            raise ValueError(f"label_metrics: k must be positive, got {k}")
        k_int, k_frac = int(k), 0.0
    dev, L = pred.device, n_labels
    label = label.contiguous()
    values = torch.empty(13, L, dtype=torch.float64, device=dev)
    count, pos, k_eff = (torch.empty(L, dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch("mdg_label_metrics_workspace_bytes", dev, T, L)
    call("mdg_label_metrics", _ptr(pred), _ptr(target), _ptr(label), T, L, k_int, k_frac, threshold, _ptr(values), _ptr(count), _ptr(pos),
         _ptr(k_eff), _ptr(status), _ptr(ws), nbytes, _stream(pred))
    st = int(status.item())
    if st:
        raise ValueError("label_metrics: " + "; ".join(msg for bit, msg in _LABEL_METRIC_STATUS if st & bit))
    return {"values": values, "count": count, "pos": pos, "k_eff": k_eff}


_GROUP_METRIC_STATUS = ((1, "pred holds a NaN or infinite value"), (16, "a group id is outside [0, n_groups)"),
                        (4, "target holds a value other than 0 and 1"), (8, "k resolves to 0 for a group (k * n_group < 1)"))


def group_metrics(pred: torch.Tensor, target: torch.Tensor, group: torch.Tensor, n_groups: int, k=50, threshold: float = 0.5,
                  inner: Optional[int] = None) -> dict:
    """The metrics of ``label_metrics`` per group, for group ids in [0, n_groups) with n_groups up to 2^31 (csrc/eval_metrics.hip,
    mdg_group_metrics): only the groups present are reported, ascending by id.

    pred / target fp32 [T] (target 0 or 1), group int64 [T]; ``k`` as in ``label_metrics`` (a float resolves per group).  Returns
    device tensors sliced to the n_present groups: ``group_id`` int64, ``values`` float64 [13, n_present] in the order of
    LABEL_METRIC_NAMES, ``count`` / ``pos`` / ``k_eff`` int64.  With ``inner`` (an int > 0) also ``outer_values`` float64
    [13, ceil(n_groups / inner)], the mean of each metric over the present groups of outer index group // inner (bit-equal to
    numpy's mean(axis=0) over those columns; NaN where an outer has none) and ``outer_groups`` int64, the number of groups
    averaged.  One host read (status and n_present): raises ValueError on a NaN / infinite pred, a group id out of range, a
    target other than 0/1, or k resolving to 0."""
    pred, target = _f32_cuda(pred, "pred", 1), _f32_cuda(target, "target", 1)
    T = int(pred.numel())
    if not (isinstance(group, torch.Tensor) and group.is_cuda and group.dtype == torch.int64 and group.dim() == 1 and group.numel() == T):
        raise ValueError(f"group: expected int64 cuda [{T}]")
    if target.numel() != T or pred.device != target.device or pred.device != group.device:
        raise ValueError("group_metrics: pred, target and group must be [T] on one device")
    if not 0 < T < 2 ** 31:
        raise ValueError(f"group_metrics: need 0 < T < 2^31 triples, got {T}")
    n_groups = int(n_groups)
    if not 0 < n_groups <= 2 ** 31:
        raise ValueError(f"group_metrics: need 0 < n_groups <= 2^31, got {n_groups}")
    if isinstance(k, bool) or not isinstance(k, (int, float)):
        raise ValueError(f"group_metrics: k must be an int or a float in (0, 1), got {k!r}")
    if isinstance(k, float):
        if not 0.0 < k < 1.0:
            raise ValueError(f"group_metrics: a float k must lie in (0, 1), got {k}")
        k_int, k_frac = 0, float(k)
    else:
        if k <= 0:
            raise ValueError(f"group_metrics: k must be positive, got {k}")
        k_int, k_frac = int(k), 0.0
    if inner is not None and (isinstance(inner, bool) or not isinstance(inner, int) or inner <= 0):
        raise ValueError(f"group_metrics: inner must be a positive int or None, got {inner!r}")
    dev, cap = pred.device, min(T, n_groups)
    group = group.contiguous()
    group_id = torch.empty(cap, dtype=torch.int64, device=dev)
    values = torch.empty(13, cap, dtype=torch.float64, device=dev)
    count, pos, k_eff = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(3))
    meta = torch.zeros(2, dtype=torch.int64, device=dev)             # [0]: the status word (low 32 bits), [1]: n_present
    outer_values = outer_groups = None
    if inner is not None:
        n_outer = -(-n_groups // inner)
        outer_values = torch.empty(13, n_outer, dtype=torch.float64, device=dev)
        outer_groups = torch.empty(n_outer, dtype=torch.int64, device=dev)
    ws, nbytes = _scratch("mdg_group_metrics_workspace_bytes", dev, T, n_groups)
    call("mdg_group_metrics", _ptr(pred), _ptr(target), _ptr(group), T, n_groups, k_int, k_frac, threshold, inner or 0, _ptr(group_id), _ptr(values),
         _ptr(count), _ptr(pos), _ptr(k_eff), meta.data_ptr() + 8, _ptr(outer_values), _ptr(outer_groups), _ptr(meta), _ptr(ws), nbytes,
         _stream(pred))
    m = meta.cpu()
    st, n_present = int(m.view(torch.int32)[0]), int(m[1])
    if st:
        raise ValueError("group_metrics: " + "; ".join(msg for bit, msg in _GROUP_METRIC_STATUS if st & bit))
    out = {"group_id": group_id[:n_present], "values": values[:, :n_present], "count": count[:n_present], "pos": pos[:n_present],
           "k_eff": k_eff[:n_present]}
    if inner is not None:
        out["outer_values"], out["outer_groups"] = outer_values, outer_groups
    return out


# ------------------------------------------------------------------------------- pretraining retrieval metrics
PAIR_MATCH_COUNT_NAMES = ("cos_row", "cos_col", "same_x", "same_y", "dist_row", "dist_col")
_PAIR_STATUS = ((1, "holds a NaN or infinite value"), (2, "has a zero-norm row (its cosines would be NaN)"))


def _embeds_128(x: torch.Tensor, name: str) -> torch.Tensor:
    x = _f32_cuda(x, name, 2)
    if x.shape[1] != 128:
        raise ValueError(f"{name}: expected [n,128] embeddings, got shape {tuple(x.shape)}")
    return x


def _pair_status(status: torch.Tensor, what: str) -> None:
    st = int(status.item())
    if st:
        raise ValueError(f"{what}: input " + "; ".join(msg for bit, msg in _PAIR_STATUS if st & bit))


def pair_match_counts(x: torch.Tensor, y: torch.Tensor) -> dict:
    """Retrieval counts of two views of the same n drugs (csrc/retrieval.hip, mdg_pair_match_counts): row i of x and of y is
    drug i, and column i is row i's true match.  x, y fp32 [n,128] on the GPU, 1 <= n <= 65536.

    Returns device tensors: int32 [n] ``cos_row`` / ``cos_col`` (competitors with a strictly higher cosine than the true match,
    per row of x / per row of y), ``same_x`` / ``same_y`` (same-view competitors of the stacked top-k), ``dist_row`` /
    ``dist_col`` (FOSCTTM counts of strictly closer raw embeddings), and fp32 [n] ``align`` = |x^_i - y^_i|^2.  Ties count as
    hits: a competitor equal to the true match is not counted, and the true match itself is excluded by index.  One host read
    (the status word): raises ValueError for NaN / inf entries and zero-norm rows."""
    x, y = _embeds_128(x, "x"), _embeds_128(y, "y")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"pair_match_counts: x and y must have one shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")
    n = int(x.shape[0])
    if not 1 <= n <= 65536:
        raise ValueError(f"pair_match_counts: need 1 <= n <= 65536 rows, got {n}")
    dev = x.device
    out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in PAIR_MATCH_COUNT_NAMES}
    out["align"] = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch("mdg_pair_match_counts_workspace_bytes", dev, n)
    call("mdg_pair_match_counts", _ptr(x), _ptr(y), n, 128, *(_ptr(out[k]) for k in PAIR_MATCH_COUNT_NAMES), _ptr(out["align"]), _ptr(status),
         _ptr(ws), nbytes, _stream(x))
    _pair_status(status, "pair_match_counts")
    return out


def pair_uniformity(x: torch.Tensor, t: float = 2.0) -> torch.Tensor:
    """uniform_loss of madrigal/evaluate/eval_utils.py:147-150 (csrc/retrieval.hip, mdg_pair_uniformity): 0-dim fp32 device tensor
    log(mean_{i<j} exp(-t |x^_i - x^_j|^2)) over x fp32 [m,128] on the GPU, 2 <= m <= 65536.  fp32 tile sums, fp64 across tiles in
    a fixed order: bit-identical from run to run.  One host read (the status word): raises ValueError for NaN / inf entries and
    zero-norm rows."""
    x = _embeds_128(x, "x")
    m = int(x.shape[0])
    if not 2 <= m <= 65536:
        raise ValueError(f"pair_uniformity: need 2 <= m <= 65536 rows, got {m}")
    t = float(t)
    if t != t:
        raise ValueError("pair_uniformity: t is NaN")
    dev = x.device
    out = torch.empty((), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch("mdg_pair_uniformity_workspace_bytes", dev, m)
    call("mdg_pair_uniformity", _ptr(x), m, 128, t, _ptr(out), _ptr(status), _ptr(ws), nbytes, _stream(x))
    _pair_status(status, "pair_uniformity")
    return out


# ------------------------------------------------------------------------------- k-nearest neighbours
KNN_METRICS = {"cosine": 0, "dot": 1, "euclidean": 2}
_KNN_NO_LISTS = 256


def knn_max_k() -> int:
    """Largest k of ``knn_topk`` (32: one list entry per lane of the 32 lanes that share a query row)."""
    return int(lib().mdg_knn_max_k())


def knn_default_segments(nq: int, nl: int) -> int:
    """Column segments ``knn_topk`` uses when none are given (host only): 1 when the blocks of 128 query rows alone give every
    CU two workgroups, otherwise enough segments to get there, at most ceil(nl / 128)."""
    return int(lib().mdg_knn_default_segments(int(nq), int(nl)))


def _knn_args(q, lib_, k, metric, skip, segments, what):
    q, lib_ = _embeds_128(q, "q"), _embeds_128(lib_, "lib")
    if q.device != lib_.device:
        raise ValueError(f"{what}: q and lib must live on one device, got {q.device} and {lib_.device}")
    if metric not in KNN_METRICS:
        raise ValueError(f"{what}: unknown metric {metric!r}; expected one of {sorted(KNN_METRICS)}")
    nq, nl = int(q.shape[0]), int(lib_.shape[0])
    if nq < 1 or nl < 1:
        raise ValueError(f"{what}: need at least one query and one library row, got {nq} and {nl}")
    if skip is not None:
        if not isinstance(skip, torch.Tensor) or not skip.is_cuda or skip.dtype != torch.int32 or skip.shape != (nq,):
            raise ValueError(f"{what}: skip must be an int32 GPU tensor of shape [{nq}]")
        skip = skip.contiguous()
    k = int(k)
    cand = nl - (1 if skip is not None else 0)
    if not 1 <= k <= min(knn_max_k(), cand):
        raise ValueError(f"{what}: need 1 <= k <= min({knn_max_k()}, {cand} candidates per row), got k = {k} (torch.topk raises for "
                         "k above the candidates)")
    if segments is None:
        segments = knn_default_segments(nq, nl)
    segments = int(segments)
    if segments < 1:
        raise ValueError(f"{what}: segments must be at least 1, got {segments}")
    return q, lib_, nq, nl, k, skip, segments


def knn_topk(q: torch.Tensor, lib_: torch.Tensor, k: int, *, metric: str = "cosine", skip: Optional[torch.Tensor] = None,
             segments: Optional[int] = None):
    """The k nearest rows of ``lib_`` fp32 [nl,128] for every row of ``q`` fp32 [nq,128], both on the GPU (csrc/knn.hip,
    mdg_knn_topk) -> ``(vals fp32 [nq,k], idx int32 [nq,k])`` ordered by (value best-first, library index ascending).

    metric: 'cosine' (larger is better; the value ``pair_match_counts`` compares, bit for bit), 'dot', or 'euclidean' (ranked on the
    fp32 squared distance, the distance is returned).  skip int32 [nq]: the library row query i must not return (-1: none).
    segments: column segments of the sweep (default ``knn_default_segments``); the result is the same bits for every value.
    1 <= k <= min(32, nl - (1 if skip is given else 0)).  One host read (the status word): raises ValueError for NaN / inf entries
    and, for 'cosine', zero-norm rows."""
    q, lib_, nq, nl, k, skip, segments = _knn_args(q, lib_, k, metric, skip, segments, "knn_topk")
    dev = q.device
    vals = torch.empty((nq, k), dtype=torch.float32, device=dev)
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    qstat = torch.empty((2, nq), dtype=torch.float32, device=dev)
    lstat = torch.empty((2, nl), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch("mdg_knn_topk_workspace_bytes", dev, nq, nl, k, segments)
    call("mdg_knn_topk", _ptr(q), _ptr(lib_), nq, nl, 128, k, KNN_METRICS[metric], _ptr(skip), segments, _ptr(qstat), _ptr(lstat), _ptr(vals),
         _ptr(idx), _ptr(status), _ptr(ws), nbytes, _stream(q))
    _pair_status(status, "knn_topk")
    return vals, idx


def knn_sweep_rowmax(q: torch.Tensor, lib_: torch.Tensor, *, metric: str = "cosine", segments: Optional[int] = None) -> torch.Tensor:
    """Measurement aid (scripts/knn_bench.py): the sweep of ``knn_topk`` with the list epilogue compiled out -> fp32
    [segments used, nq], each segment's largest value per query (for 'euclidean', of the negated squared distance).  Pre-pass,
    status word and its host read are ``knn_topk``'s, so the difference of the two is the lists and their merge."""
    q, lib_, nq, nl, _, _, segments = _knn_args(q, lib_, 1, metric, None, segments, "knn_sweep_rowmax")
    dev = q.device
    tiles = -(-nl // 128)
    per = -(-tiles // min(segments, tiles))
    out = torch.empty((-(-tiles // per), nq), dtype=torch.float32, device=dev)        # ceil(tiles / per): no segment is empty
    qstat = torch.empty((2, nq), dtype=torch.float32, device=dev)
    lstat = torch.empty((2, nl), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    call("mdg_knn_topk", _ptr(q), _ptr(lib_), nq, nl, 128, 1, KNN_METRICS[metric] | _KNN_NO_LISTS, None, segments, _ptr(qstat), _ptr(lstat),
         _ptr(out), None, _ptr(status), None, 0, _stream(q))
    _pair_status(status, "knn_sweep_rowmax")                                       # the same host read as knn_topk's
    return out


def knn_vote(vals: torch.Tensor, idx: torch.Tensor, labels: torch.Tensor, T: float, num_classes: int):
    """The kNN classifier's vote on the lists of ``knn_topk`` (csrc/knn.hip, mdg_knn_vote): weights exp(vals / T) in fp32.
    labels uint8 on the GPU: [nl] class ids (< num_classes <= 64), or [nl, C] binary columns with num_classes == 2.
    -> ``(pred uint8, sums fp32)``: [nq] and [nq, num_classes] for a label vector, [nq, C] and [nq, C, 2] for label columns.  With
    num_classes == 2 the sums are p1 = sum_j w_j label_j (j ascending) and p0 = sum_j w_j - p1; otherwise one sum per class.  The
    prediction is the class with the largest sum, the lowest class on a tie."""
    vals = _f32_cuda(vals, "vals", 2)
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.int32 or idx.shape != vals.shape:
        raise ValueError(f"knn_vote: idx must be an int32 GPU tensor of vals' shape {tuple(vals.shape)}")
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.uint8 or labels.dim() not in (1, 2):
        raise ValueError("knn_vote: labels must be a uint8 GPU tensor of shape [nl] or [nl, C]")
    num_classes = int(num_classes)
    if not 2 <= num_classes <= 64:
        raise ValueError(f"knn_vote: num_classes must be in 2..64, got {num_classes}")
    if labels.dim() == 2 and num_classes != 2:
        raise ValueError(f"knn_vote: [nl, C] label columns are binary (num_classes = 2), got num_classes = {num_classes}")
    T = float(T)
    if T != T or T == 0.0:
        raise ValueError("knn_vote: T must be a non-zero number")
    idx, labels = idx.contiguous(), labels.contiguous()
    nq, k = int(vals.shape[0]), int(vals.shape[1])
    nl = int(labels.shape[0])
    C = int(labels.shape[1]) if labels.dim() == 2 else 1
    if nl < 1 or C < 1 or not 1 <= k <= knn_max_k():
        raise ValueError(f"knn_vote: need labels for at least one row and 1 <= k <= {knn_max_k()}, got {tuple(labels.shape)} and k = {k}")
    dev = vals.device
    cols = (C,) if labels.dim() == 2 else ()
    pred = torch.empty((nq,) + cols, dtype=torch.uint8, device=dev)
    sums = torch.empty((nq,) + cols + (2 if num_classes == 2 else num_classes,), dtype=torch.float32, device=dev)
    call("mdg_knn_vote", _ptr(vals), _ptr(idx), _ptr(labels), nq, nl, k, C, num_classes, T, _ptr(pred), _ptr(sums), _stream(vals))
    return pred, sums


# ------------------------------------------------------------------------------- GeomCA
def geomca_default_chunk() -> int:
    """Candidates ``geomca_sparsify`` resolves per step when ``chunk`` is not given (host only)."""
    return int(lib().mdg_geomca_default_chunk())


def geomca_default_segments(nrow: int, ncol: int) -> int:
    """Column segments a GeomCA sweep of ``nrow`` rows over ``ncol`` columns uses when none are given (host only)."""
    return int(lib().mdg_geomca_default_segments(int(nrow), int(ncol)))


def _geomca_segments(segments, what: str) -> int:
    if segments is None:
        return 0
    segments = int(segments)
    if segments < 1:
        raise ValueError(f"{what}: segments must be at least 1, got {segments}")
    return segments


def _geomca_threshold(value, name: str, what: str) -> float:
    """float32(value * value), the product formed in float64: the threshold the kernels compare the fp32 d2 with."""
    value = float(value)
    if not (value == value and 0.0 <= value < float("inf")):
        raise ValueError(f"{what}: {name} must be a finite number >= 0, got {value}")
    thr = float(torch.tensor(value * value, dtype=torch.float64).to(torch.float32))     # round to nearest even
    if thr == float("inf"):
        raise ValueError(f"{what}: {name}^2 = {value * value} does not fit float32")
    return thr


def _geomca_ids(ids, m: int, name: str, device) -> torch.Tensor:
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.dtype not in (torch.int32, torch.int64) or ids.shape != (m,):
        raise ValueError(f"geomca_distance_select: {name} must be an int32 or int64 GPU tensor of shape [{m}]")
    return ids.to(device=device, dtype=torch.int32).contiguous()


def geomca_prep(x: torch.Tensor, what: str = "geomca_prep") -> torch.Tensor:
    """fp32 [n] Gram-chain squared norms n(x) = g(x, x) of x fp32 [n,128] on the GPU (csrc/geomca.hip, mdg_geomca_prep): the
    diagonal of the same MFMA chain that forms g(x, y), so d2(x, y) = max(fmaf(-2, g, n(x) + n(y)), 0) is exactly 0 for bitwise
    equal rows.  One host read (the status word): raises ValueError for NaN / inf entries."""
    x = _embeds_128(x, "x")
    n = int(x.shape[0])
    if n < 1:
        raise ValueError(f"{what}: need at least one row")
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    status = torch.empty(1, dtype=torch.int32, device=x.device)
    call("mdg_geomca_prep", _ptr(x), n, 128, _ptr(norms), _ptr(status), _stream(x))
    _pair_status(status, what)
    return norms


def geomca_sparsify(x: torch.Tensor, delta: float, *, chunk: Optional[int] = None, segments: Optional[int] = None) -> torch.Tensor:
    """GeomCA's geometric sparsification (GeomCA.py:333-352, GUDHI's sparsify_point_set) of x fp32 [n,128] on the GPU
    (csrc/geomca.hip, mdg_geomca_sparsify) -> int64 [kept], the kept input rows, ascending.  Walking the rows in input order, row
    i is kept iff no KEPT row j < i has d2(i, j) < float32(delta^2): the lexicographically first delta-separated subset; a dropped
    row never drops anyone.  chunk: candidates resolved per step (a multiple of 128 in 128..512, default
    ``geomca_default_chunk()``); segments: column segments of the sweeps; the result is the same for every value of both.  Two
    host reads (the status word, the kept count).  Raises ValueError for NaN / inf entries."""
    x = _embeds_128(x, "x")
    n = int(x.shape[0])
    if n < 1:
        raise ValueError("geomca_sparsify: need at least one row")
    thr = _geomca_threshold(delta, "delta", "geomca_sparsify")
    chunk = geomca_default_chunk() if chunk is None else int(chunk)
    if chunk < 128 or chunk > 512 or chunk % 128:
        raise ValueError(f"geomca_sparsify: chunk must be a multiple of 128 in 128..512, got {chunk}")
    segments = _geomca_segments(segments, "geomca_sparsify")
    norms = geomca_prep(x, "geomca_sparsify")
    dev = x.device
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch("mdg_geomca_sparsify_workspace_bytes", dev, n, chunk)
    call("mdg_geomca_sparsify", _ptr(x), n, 128, _ptr(norms), thr, chunk, segments, _ptr(kept), _ptr(count), _ptr(ws), nbytes, _stream(x))
    return kept[:int(count.item())].long()


def geomca_components(v: torch.Tensor, n_r: int, epsilon: float, *, segments: Optional[int] = None):
    """Connected components and degrees of the epsilon-graph on the vertices v fp32 [n,128] (the first ``n_r`` are the R set) on
    the GPU (csrc/geomca.hip, mdg_geomca_components; GeomCA.py:354-387, :423-435) -> ``(label int32 [n], deg_same int32 [n],
    deg_cross int32 [n], sweeps)``.  Edge {i, j}, i != j, iff d2(i, j) <= float32(epsilon^2).  label[i]: the smallest vertex index
    of i's component; deg_same / deg_cross: i's neighbours in its own / in the other set; sweeps: link sweeps run (hooking and
    pointer jumping in between; the last sweep finds nothing to change).  The result is the same for every ``segments``.  Raises
    ValueError for NaN / inf entries."""
    v = _embeds_128(v, "v")
    n, n_r = int(v.shape[0]), int(n_r)
    if n < 1 or not 0 <= n_r <= n:
        raise ValueError(f"geomca_components: need at least one vertex and 0 <= n_r <= n, got n = {n}, n_r = {n_r}")
    thr = _geomca_threshold(epsilon, "epsilon", "geomca_components")
    segments = _geomca_segments(segments, "geomca_components")
    norms = geomca_prep(v, "geomca_components")
    dev = v.device
    label, deg_same, deg_cross = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    sweeps = ctypes.c_int(0)
    ws, nbytes = _scratch("mdg_geomca_components_workspace_bytes", dev, n)
    call("mdg_geomca_components", _ptr(v), n, n_r, 128, _ptr(norms), thr, segments, _ptr(label), _ptr(deg_same), _ptr(deg_cross),
         ctypes.addressof(sweeps), _ptr(ws), nbytes, _stream(v))
    return label, deg_same, deg_cross, int(sweeps.value)


def geomca_distance_select(x: torch.Tensor, y: torch.Tensor, ids_x: torch.Tensor, ids_y: torch.Tensor, percentile: float, *,
                           segments: Optional[int] = None):
    """The order statistics GeomCA's epsilon estimate needs (GeomCA.py:250-282: cdist, distances > 0, np.percentile) without the
    distance matrix (csrc/geomca.hip, mdg_geomca_distance_select).  x fp32 [mx,128], y fp32 [my,128]: the drawn rows; ids_x, ids_y:
    the input rows they were drawn from.  Over the pairs with ids_x[a] != ids_y[b] -> ``(zeros, M, d2_lo, d2_hi, pos)``: the pairs
    at d2 == 0, the pairs at d2 > 0, and the exact order statistics D[k], D[k + 1] (k + 1 clamped to M - 1) of the positive fp32 d2
    values at numpy's linear-interpolation position pos = percentile / 100 * (M - 1), k = floor(pos).  A radix select on the fp32
    bit pattern: three sweeps, three small host reads.  M == 0 returns zeros for the values.  Raises ValueError for NaN / inf."""
    x, y = _embeds_128(x, "x"), _embeds_128(y, "y")
    if x.device != y.device:
        raise ValueError(f"geomca_distance_select: x and y must live on one device, got {x.device} and {y.device}")
    mx, my = int(x.shape[0]), int(y.shape[0])
    if mx < 1 or my < 1:
        raise ValueError(f"geomca_distance_select: need at least one row on each side, got {mx} and {my}")
    percentile = float(percentile)
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"geomca_distance_select: percentile must lie in [0, 100], got {percentile}")
    segments = _geomca_segments(segments, "geomca_distance_select")
    dev = x.device
    ids_x, ids_y = _geomca_ids(ids_x, mx, "ids_x", dev), _geomca_ids(ids_y, my, "ids_y", dev)
    xn = geomca_prep(x, "geomca_distance_select")
    yn = xn if y.data_ptr() == x.data_ptr() and mx == my else geomca_prep(y, "geomca_distance_select")
    counts = (ctypes.c_int64 * 2)()
    values = (ctypes.c_double * 3)()
    ws, nbytes = _scratch("mdg_geomca_distance_select_workspace_bytes", dev)
    call("mdg_geomca_distance_select", _ptr(x), _ptr(y), _ptr(ids_x), _ptr(ids_y), mx, my, 128, _ptr(xn), _ptr(yn), percentile, segments,
         ctypes.addressof(counts), ctypes.addressof(values), _ptr(ws), nbytes, _stream(x))
    return int(counts[0]), int(counts[1]), float(values[0]), float(values[1]), float(values[2])


# ------------------------------------------------------------------------------- on-device batch collation (csrc/collate.hip)
COLLATE_MAX_SEGMENTS = 4


def _i64_cuda(t: torch.Tensor, name: str, dev) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.device == dev):
        raise ValueError(f"{name}: expected a 1-D int64 cuda tensor on {dev}")
    return t if t.is_contiguous() else t.contiguous()


def collate_offsets(ids: torch.Tensor, id2row: torch.Tensor, atom_ptr: torch.Tensor, edge_ptr: torch.Tensor):
    """ids [B] -> ``(rows [B], out_atom_ptr [B+1], out_edge_ptr [B+1], totals [4])`` (mdg_collate_offsets): the store row of
    every id (-1 outside the store), the exclusive scans of the per-drug atom / edge counts, and atoms | edges | ids outside
    the store | position of the first of them.  All int64 on the device: two launches, no host read."""
    dev = ids.device
    ids, id2row = _i64_cuda(ids, "collate_offsets: ids", dev), _i64_cuda(id2row, "collate_offsets: id2row", dev)
    atom_ptr, edge_ptr = _i64_cuda(atom_ptr, "collate_offsets: atom_ptr", dev), _i64_cuda(edge_ptr, "collate_offsets: edge_ptr", dev)
    B, M = int(ids.numel()), int(atom_ptr.numel()) - 1
    if B < 1 or M < 0 or edge_ptr.numel() != M + 1:
        raise ValueError(f"collate_offsets: {B} ids, atom_ptr of {atom_ptr.numel()} and edge_ptr of {edge_ptr.numel()} entries")
    buf = torch.empty(3 * B + 6, dtype=torch.int64, device=dev)
    rows, out_atom_ptr, out_edge_ptr, totals = buf[:B], buf[B:2 * B + 1], buf[2 * B + 1:3 * B + 2], buf[3 * B + 2:]
    ws, nbytes = _scratch("mdg_collate_offsets_workspace_bytes", dev, B)
    call("mdg_collate_offsets", _ptr(ids), B, _ptr(id2row), id2row.numel(), _ptr(atom_ptr), _ptr(edge_ptr), M, _ptr(rows),
         _ptr(out_atom_ptr), _ptr(out_edge_ptr), _ptr(totals), _ptr(ws), nbytes, _stream(ids))
    return rows, out_atom_ptr, out_edge_ptr, totals


def collate_molecules(rows, out_atom_ptr, out_edge_ptr, n_atoms: int, n_edges: int, atom_ptr, edge_ptr, node_feature, edge_list,
                      edge_feature, edge_weight, edge_feat_aug, rowptr, want_w: bool) -> dict:
    """The packed molecules of store rows ``rows`` and their aggregation plan in one launch (mdg_collate_molecules).  The
    ``out_*`` arrays and the sizes come from ``collate_offsets``; the rest is the store (edges sorted by destination atom).
    -> fresh tensors ``node_feature node2graph edge_list edge_feature edge_weight rowptr col edge_feat_aug w`` (w None
    unless ``want_w``)."""
    dev = rows.device
    B, A, E = int(rows.numel()), int(n_atoms), int(n_edges)
    nf, ef, ew, aug = (_f32_cuda(x, "collate_molecules: " + n) for x, n in
                       ((node_feature, "node_feature"), (edge_feature, "edge_feature"), (edge_weight, "edge_weight"), (edge_feat_aug, "edge_feat_aug")))
    if nf.dim() != 2 or nf.shape[1] != 67 or ef.shape[1:] != (18,) or aug.shape[1:] != (20,) or edge_list.shape[1:] != (3,) or \
            not (ef.shape[0] == aug.shape[0] == ew.shape[0] == edge_list.shape[0]) or rowptr.numel() != nf.shape[0] + 1:
        raise ValueError("collate_molecules: the store's arrays do not fit together")
    if edge_list.dtype != torch.int64 or not edge_list.is_contiguous() or edge_list.device != dev:
        raise ValueError("collate_molecules: edge_list must be a contiguous int64 [E,3] tensor on the store's device")
    out = {"node_feature": torch.empty((A, 67), dtype=torch.float32, device=dev),
           "node2graph": torch.empty(A, dtype=torch.int64, device=dev),
           "edge_list": torch.empty((E, 3), dtype=torch.int64, device=dev),
           "edge_feature": torch.empty((E, 18), dtype=torch.float32, device=dev),
           "edge_weight": torch.empty(E, dtype=torch.float32, device=dev),
           "rowptr": torch.empty(A + 1, dtype=torch.int64, device=dev),
           "col": torch.empty(E, dtype=torch.int64, device=dev),
           "edge_feat_aug": torch.empty((E, 20), dtype=torch.float32, device=dev),
           "w": torch.empty(E, dtype=torch.float32, device=dev) if want_w else None}
    call("mdg_collate_molecules", _ptr(rows), _ptr(out_atom_ptr), _ptr(out_edge_ptr), B, A, E,
         _ptr(_i64_cuda(atom_ptr, "collate_molecules: atom_ptr", dev)), _ptr(_i64_cuda(edge_ptr, "collate_molecules: edge_ptr", dev)),
         _ptr(nf), _ptr(edge_list), _ptr(ef), _ptr(ew), _ptr(aug), _ptr(_i64_cuda(rowptr, "collate_molecules: rowptr", dev)),
         *[_ptr(out[k]) for k in ("node_feature", "node2graph", "edge_list", "edge_feature", "edge_weight", "rowptr", "col", "edge_feat_aug", "w")],
         _stream(rows))
    return out


def collate_rows(tables, rows: torch.Tensor) -> list:
    """``[t[:, rows, :] for t in tables]`` in one launch (mdg_collate_rows): every table is a dense fp32 [S, M, W] stack of S
    equal-shaped sources over the same M store rows (up to 4 tables, any S and W); the results are dense [S, B, W], exact width.
    A negative row leaves its output rows unwritten (the caller checks the ids before it uses them)."""
    tables = list(tables)
    if not 1 <= len(tables) <= COLLATE_MAX_SEGMENTS:
        raise ValueError(f"collate_rows: 1 to {COLLATE_MAX_SEGMENTS} tables, got {len(tables)}")
    dev = rows.device
    rows = _i64_cuda(rows, "collate_rows: rows", dev)
    B, M = int(rows.numel()), int(tables[0].shape[1]) if tables[0].dim() == 3 else -1
    for j, t in enumerate(tables):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()
                and t.device == dev and t.shape[1] == M and t.shape[0] >= 1 and t.shape[2] >= 1):
            raise ValueError(f"collate_rows: tables[{j}] must be a contiguous fp32 cuda [S, {M}, W] tensor on {dev}")
    if B < 1 or M < 1:
        raise ValueError(f"collate_rows: {B} rows of {M} store rows")
    outs = [torch.empty((t.shape[0], B, t.shape[2]), dtype=torch.float32, device=dev) for t in tables]
    K = len(tables)
    a_s = (ctypes.c_void_p * K)(*[t.data_ptr() for t in tables])
    a_o = (ctypes.c_void_p * K)(*[o.data_ptr() for o in outs])
    a_n = (ctypes.c_int64 * K)(*[t.shape[0] for t in tables])
    a_w = (ctypes.c_int64 * K)(*[t.shape[2] for t in tables])
    call("mdg_collate_rows", a_s, a_o, a_n, a_w, K, M, _ptr(rows), B, _stream(rows))
    return outs
