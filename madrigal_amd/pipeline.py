"""All-pairs inference: encode every drug once -> (all-gather) -> score every (head, tail, outcome).

MI355X-native counterpart of ``notebooks/generate_embeddings.ipynb`` cells 9-10 and
``get_*_scores_for_all_pairs_among_drugs`` (madrigal/evaluate/predict.py:381-463, 502-579): the
reference encodes once (``model.encoder(...)``), then loops over chunks of 10-30 outcomes calling
``model.decoder(z, z, (start, end)).cpu().numpy()`` into an ``np.memmap``.  Here the head writes the
[L,N,N] tensor straight into HBM (288 GB holds the reference's whole 80 GB tensor) or, when the caller
wants it on the host / in a memmap, streams outcome chunks through two pinned buffers on a copy stream
so that the D2H copy of chunk k overlaps the kernel of chunk k+1.

Multi-GPU (one process per GPU): encode+fuse is independent per drug, so rank r encodes a contiguous
block of drugs (the KG encoder, which is per-graph rather than per-drug, runs destination-partitioned:
every rank computes its block of every node type and one all-gather per conv reassembles them); one
all-gather of the [N/G,128] blocks over RCCL gives every rank z[N,128]; the head is sharded by
outcome (``label_range``: rank-local rank normalisation afterwards; what bench.py and the rank pipeline use)
or by head row (``head_rows``: BASELINE configs[3]'s "row-sharded" -- rank r owns S[:, rows_r, :]; the rank
normalisation of a row-sharded tensor would need a global sort, so it is for callers that want raw scores).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from .data import MoleculeBatch
from .parallel import all_gather_rows, shard_range
from .retrieval import nearest_neighbors


def slice_molecules(mols: MoleculeBatch, lo: int, hi: int) -> MoleculeBatch:
    """Graphs [lo,hi) of a packed molecule batch as a new packed batch (atoms / bonds re-indexed)."""
    n2g = mols.node2graph
    a0 = int(torch.searchsorted(n2g, torch.tensor(lo, device=n2g.device)))
    a1 = int(torch.searchsorted(n2g, torch.tensor(hi, device=n2g.device)))
    keep = (mols.edge_list[:, 1] >= a0) & (mols.edge_list[:, 1] < a1)
    el = mols.edge_list[keep].clone()
    el[:, :2] -= a0
    return MoleculeBatch(mols.node_feature[a0:a1], el, mols.edge_feature[keep], n2g[a0:a1] - lo, hi - lo,
                         mols.edge_weight[keep])


def slice_batch(batch: dict, lo: int, hi: int) -> dict:
    """Drugs [lo,hi) of a reference-format batch dict."""
    tx = {c: {"sigs": v["sigs"][lo:hi], "drugs": v["drugs"][lo:hi], "dosages": v["dosages"][lo:hi],
              "cell_lines": v["cell_lines"][lo:hi]} for c, v in batch["tx"].items()}
    return {"drugs": batch["drugs"][lo:hi], "strs": slice_molecules(batch["strs"], lo, hi), "cv": batch["cv"][lo:hi],
            "tx": tx, "masks": batch["masks"][lo:hi]}


@torch.no_grad()
def generate_embeddings(model, batch: dict, batch_kg: dict, masks: Optional[torch.Tensor] = None, rank: int = 0,
                        world: int = 1, kg_filler: Optional[torch.Tensor] = None, on_encoded=None) -> torch.Tensor:
    """z[N,128] for every drug of ``batch`` (``model.encoder`` on all drugs, generate_embeddings.ipynb raw
    line 226).  With ``world > 1`` each rank encodes its block and the blocks are all-gathered.  ``on_encoded``: called
    (no arguments) between the rank's own encode+fuse and the exchange step -- bench.py records a HIP event there."""
    masks = batch["masks"] if masks is None else masks
    n = int(batch["drugs"].shape[0])
    if world == 1:
        z = model.encoder(batch["drugs"], masks, batch["strs"], batch_kg, batch["cv"], batch["tx"], kg_filler=kg_filler)
        if on_encoded is not None:
            on_encoded()
        return z
    lo, hi = shard_range(n, rank, world)
    local = batch.get("_shards", {}).get((lo, hi))
    if local is None:
        local = slice_batch(batch, lo, hi)
        batch.setdefault("_shards", {})[(lo, hi)] = local
    # the KG encoder is per graph, not per drug: its convs run destination-partitioned over the ranks (HGTConv.forward) instead
    # of replicated (MDG_SHARD_KG=0 keeps it replicated)
    import os
    kg_shard = (rank, world, None) if os.environ.get("MDG_SHARD_KG", "1") != "0" else None
    z_local = model.encoder(local["drugs"], masks[lo:hi], local["strs"], batch_kg, local["cv"], local["tx"], kg_filler=kg_filler,
                            kg_shard=kg_shard)
    if on_encoded is not None:
        on_encoded()
    return all_gather_rows(z_local.contiguous(), n, rank, world)


@torch.no_grad()
def score_all_pairs(model, z: torch.Tensor, label_range: Optional[Tuple[int, int]] = None, out=None,
                    host_chunk: int = 16, epilogue: int = ops.EPI_STORE, head_rows: Optional[Tuple[int, int]] = None,
                    out_dtype=None):
    """Scores of every ordered drug pair for outcomes ``label_range`` (default: all) -> [L',N,N] fp32.

    ``out_dtype`` = ``torch.float16`` / ``torch.bfloat16`` (or an ``out`` of a 16-bit type): the tensor in 16 bits, rounded once inside
    the head (``ops.bilinear_allpairs``) -- half the HBM and, with a host destination (a ``np.float16`` array or memmap; numpy has
    no bfloat16), half the PCIe and disk bytes: the staging buffers and copies are 16-bit too.

    ``head_rows`` = (r0, r1): the row-sharded head -- only head drugs [r0, r1) against ALL tail drugs -> [L', r1 - r0, N]
    (``decoder(z[r0:r1], z, ...)``, the general sweep; HBM destination only).  ``shard_range(N, rank, world)`` gives a rank's rows;
    the row blocks of the ranks concatenate along dim 1 to the full tensor (no collective touches the scores).

    ``out`` None / a CUDA tensor: one head launch writes the whole tensor into HBM.
    ``out`` a numpy array or ``np.memmap`` (the reference's destination, predict.py:410-429): outcome chunks
    of ``host_chunk`` are produced on the GPU and copied out through two pinned staging buffers."""
    dec = model.decoder
    lo, hi = (0, _n_outcomes(model)) if label_range is None else label_range
    N = z.shape[0]
    if out_dtype is not None and out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"out_dtype: expected torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    dtype = torch.float32 if out_dtype is None else out_dtype          # of a tensor allocated here
    kw = {} if out_dtype is None else {"out_dtype": out_dtype}
    if head_rows is not None:
        r0, r1 = head_rows
        if not (0 <= r0 <= r1 <= N):
            raise ValueError(f"head_rows {head_rows} outside [0, {N}]")
        if out is None:
            out = ops.empty_scores(hi - lo, r1 - r0, N, z.device, dtype=dtype)
        if not isinstance(out, torch.Tensor):
            raise ValueError("head_rows: HBM destination only")
        if r1 == r0:
            return out
        return dec(z[r0:r1], z, (lo, hi), epilogue=epilogue, out=out, **kw)
    if out is None:
        out = ops.empty_scores(hi - lo, N, N, z.device, dtype=dtype)      # rows on 128-byte lines whatever N is (a [:, :, :N] view when N % 32 (64) != 0)
    if isinstance(out, torch.Tensor):
        return dec(z, z, (lo, hi), epilogue=epilogue, out=out, **kw)
    if out_dtype == torch.bfloat16:
        raise ValueError("out_dtype torch.bfloat16 needs an HBM destination: numpy has no bfloat16 (use torch.float16 for a host array / memmap)")
    host_dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}.get(out.dtype)
    if tuple(out.shape) != (hi - lo, N, N) or host_dtype is None:
        raise ValueError(f"out: expected a float32 or float16 array of shape {(hi - lo, N, N)}")
    if out_dtype is not None and out_dtype != host_dtype:
        raise ValueError(f"out: dtype {out.dtype} does not match out_dtype {out_dtype}")
    copy_stream = torch.cuda.Stream(device=z.device)
    dev_buf = [ops.empty_scores(host_chunk, N, N, z.device, dtype=host_dtype) for _ in range(2)]     # row-pitched on the device, compacted by the copy
    pin_buf = [torch.empty((host_chunk, N, N), dtype=host_dtype, pin_memory=True) for _ in range(2)]
    done = [None, None]
    pending = [None, None]
    k = 0
    for s in range(lo, hi, host_chunk):
        e = min(hi, s + host_chunk)
        b = k & 1
        if done[b] is not None:                        # staging pair b is free once its last copy has landed
            done[b].synchronize()
            ps, pe = pending[b]
            out[ps - lo:pe - lo] = pin_buf[b][: pe - ps].numpy()
        dec(z, z, (s, e), epilogue=epilogue, out=dev_buf[b][: e - s])
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(z.device))
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            pin_buf[b][: e - s].copy_(dev_buf[b][: e - s], non_blocking=True)
            done[b] = torch.cuda.Event()
            done[b].record(copy_stream)
        pending[b] = (s, e)
        k += 1
    for b in range(2):
        if done[b] is not None:
            done[b].synchronize()
            ps, pe = pending[b]
            out[ps - lo:pe - lo] = pin_buf[b][: pe - ps].numpy()
    return out


@torch.no_grad()
def rank_all_pairs(model, z: torch.Tensor, label_range: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                   max_workspace_bytes: int = 8 << 30) -> torch.Tensor:
    """Normalised ranks of every drug pair per outcome -> [L',N,N] fp32, for callers whose product is the ranks (the reference
    materialises the raw scores into a memmap, predict.py:410-429, and ranks them afterwards on the CPU, notebooks/normalize_scores.py:
    36-85).  The head writes only the order keys of the strict lower triangle -- all the rank normalisation reads -- and the sort puts
    the ranks over them: half the head's store stream and no score tensor next to the rank tensor.  Bit-identical to
    ``ops.rank_normalize(score_all_pairs(...))``."""
    dec = model.decoder
    lo, hi = (0, _n_outcomes(model)) if label_range is None else label_range
    N = z.shape[0]
    if out is None:
        out = ops.empty_scores(hi - lo, N, N, z.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (hi - lo, N, N)):
        raise ValueError(f"out: expected a float32 GPU tensor of shape {(hi - lo, N, N)} (ops.empty_scores)")
    pitch = out.stride(1) if out.numel() else N
    if N * pitch * 4 >= 2 ** 32 or pitch % 4:
        # beyond the symmetric sweep's 32-bit slab offsets (N > 32 767) or on an unpadded tensor: scores first, ranks over them in place of
        # a second tensor is not possible (rank_normalize reads what it overwrites) -- one outcome chunk of scores at a time
        chunk = max(1, min(hi - lo, (8 << 30) // max(N * pitch * 4, 1)))
        tmp = ops.empty_scores(chunk, N, N, z.device)
        for s in range(lo, hi, chunk):
            e = min(hi, s + chunk)
            dec(z, z, (s, e), out=tmp[: e - s])
            ops.rank_normalize(tmp[: e - s], out=out[s - lo: e - lo], max_workspace_bytes=max_workspace_bytes)
        return out
    keys = dec(z, z, (lo, hi), epilogue=ops.EPI_TRIKEYS, out=out.view(torch.int32))
    return ops.rank_normalize(keys, max_workspace_bytes=max_workspace_bytes)


def known_pairs_mask(N: int, heads, tails, labels=None, n_labels: Optional[int] = None, device=None) -> torch.Tensor:
    """Exclusion mask of the KNOWN interactions of one drug set, for the ``exclude=`` of the screening products below: the pairs
    {heads[q], tails[q]} (indices into z; any order, duplicates allowed) are taken out from both sides -- (h, t) and (t, h) --
    -> int32 ``[P, ceil(N / 32), N rounded up to 64]`` on the GPU (``ops.pair_mask``, symmetric).  Without ``labels`` the pairs are
    excluded under every outcome (P = 1: "any known interaction"); with ``labels`` (the outcome of every pair, indices into ALL
    ``n_labels`` outcomes of the head) each outcome has its own plane, which the products slice by their ``label_range``.
    One plane of 100 352 drugs is 1.26 GB (N^2 / 8 bytes), so at that scale the shared plane is the practical form."""
    if isinstance(N, bool) or not isinstance(N, int) or N < 0:
        raise ValueError(f"N: expected the number of drugs, got {N!r}")
    return ops.pair_mask(heads, tails, N, N, labels=labels, n_labels=n_labels, symmetric=True, device=device)


def _n_outcomes(model) -> int:
    dec = model.decoder
    return dec.parametrizations.weight.original.shape[0] if hasattr(dec, "parametrizations") else dec.weight.shape[0]


def _mask3(mask, name: str):
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3:
        raise ValueError(f"{name}: expected a mask from known_pairs_mask / ops.pair_mask")
    return mask


def _planes(excl, s: int, e: int):
    """The planes of outcomes [s, e) of an exclusion mask (a shared plane serves every range)."""
    return None if excl is None else (excl if excl.shape[0] == 1 else excl[s:e])


# ---- what scores all pairs of one drug set: one model, or a checkpoint ensemble.  Every screen below is written once, over a head ----
class _Head:
    """The sweeps of one drug set against itself, as the screen bodies (``_top_pairs`` ...) call them: ``N`` drugs on ``device``,
    ``n_outcomes`` in the whole head, and per product one method over the outcomes [s, e) -- ``topk``, ``select_count``, ``select``,
    ``bincount``, ``profile`` (of the drug slices ``rows`` x ``cols``, None = all) and ``dense_rows`` (the general sweep's values
    [e - s, len(rows), N]), with the contracts of the ``ops`` wrappers they end in.  ``exclude`` / ``split`` arrive as
    ``exclusion`` returned them and the head takes the planes of [s, e) itself.  ``scores``: what the values are called in messages.
    Constructing a head looks at nothing: the operands are checked when a body first reads one of these attributes, which it does
    after it has checked its own plain arguments, so a bad ``K`` is reported whatever is wrong with the embeddings."""
    scores = "scores"

    def outcomes(self, label_range) -> Tuple[int, int]:
        lo, hi = (0, self.n_outcomes) if label_range is None else label_range
        if not (0 <= lo <= hi <= self.n_outcomes):
            raise ValueError(f"label_range {label_range} outside [0, {self.n_outcomes}]")
        return lo, hi

    def exclusion(self, mask, name: str = "exclude") -> Optional[torch.Tensor]:
        """``exclude`` / ``known`` of the screens, checked against the head: one shared plane, or one plane per outcome of the WHOLE
        head (sliced by the outcome range of each sweep, like the weight)."""
        if mask is None:
            return None
        _mask3(mask, name)
        if mask.shape[0] not in (1, self.n_outcomes):
            raise ValueError(f"{name}: {mask.shape[0]} planes; expected 1 or one per outcome of the head ({self.n_outcomes})")
        return mask


class _ModelHead(_Head):
    """One model and its embeddings ``z``: every product through ``model.decoder``'s methods, looked up at call time (the decoder
    slices weight and mask planes by the range)."""

    def __init__(self, model, z: torch.Tensor):
        self.model, self.z, self.N, self.device = model, z, z.shape[0], z.device

    n_outcomes = property(lambda self: _n_outcomes(self.model))

    def topk(self, k, s, e, eligible, exclude):
        return self.model.decoder.topk(self.z, self.z, k, (s, e), eligible=eligible, exclude=exclude)

    def dense_rows(self, rows, s, e):
        return self.model.decoder(self.z[rows].contiguous(), self.z, (s, e))

    def select_count(self, thr, s, e, eligible, exclude):
        return self.model.decoder.select_count(self.z, self.z, thr, (s, e), eligible=eligible, exclude=exclude)

    def select(self, thr, s, e, eligible, max_bytes, exclude):
        return self.model.decoder.select(self.z, self.z, thr, (s, e), eligible=eligible, max_bytes=max_bytes, exclude=exclude)

    def bincount(self, edges, s, e, eligible, split):
        return self.model.decoder.bincount(self.z, self.z, edges, (s, e), eligible=eligible, split=split)

    def profile(self, rows, cols, thr, scale, s, e, eligible):
        z = self.z
        return self.model.decoder.profile(z if rows is None else z[rows], z if cols is None else z[cols], thr, scale, (s, e), eligible=eligible)


class _EnsembleHead(_Head):
    """Checkpoints ``models`` (``_ensemble_weight`` says what one may be) and their embeddings ``zs`` of the same drugs: every product
    through ``ops.bilinear_ensemble_*`` on the W_sym slices, in the precision of ``models.precision(...)``.  ``what``: the public
    function, for the messages."""
    scores = "probs"

    def __init__(self, models, zs, what: str):
        self.models, self.zs, self.what = list(models), list(zs), what

    def __getattr__(self, name):
        """``ws`` (W_sym per checkpoint), ``n_outcomes``, ``N``, ``device``, ``prec``: set by the operand checks, at the first read of one."""
        from .models import get_precision
        if name not in ("ws", "n_outcomes", "N", "device", "prec"):
            raise AttributeError(name)
        zs, what = self.zs, self.what
        K = len(self.models)
        if not 1 <= K <= 8 or len(zs) != K:
            raise ValueError(f"{what}: 1..8 models with one embedding matrix each, got {K} models and {len(zs)} embeddings")
        z0 = zs[0]
        if not (isinstance(z0, torch.Tensor) and z0.is_cuda):
            raise ValueError("zs: embeddings must be GPU tensors")
        ws = [_ensemble_weight(m) for m in self.models]
        for k in range(K):
            if zs[k].shape != z0.shape or ws[k].shape[0] != ws[0].shape[0]:
                raise ValueError(f"{what}: checkpoint {k} has z {tuple(zs[k].shape)} and {ws[k].shape[0]} outcomes; "
                                 f"checkpoint 0 has {tuple(z0.shape)} and {ws[0].shape[0]}")
        self.ws, self.n_outcomes, self.N, self.device, self.prec = ws, ws[0].shape[0], z0.shape[0], z0.device, get_precision()
        return self.__dict__[name]

    def w(self, s, e):
        return [w[s:e] for w in self.ws]

    def topk(self, k, s, e, eligible, exclude):
        return ops.bilinear_ensemble_topk(self.zs, self.zs, self.w(s, e), k, eligible=eligible, precision=self.prec, exclude=_planes(exclude, s, e))

    def dense_rows(self, rows, s, e):       # a row subset is not the tail object: the general sweep, bit for bit what the lists saw
        return ops.bilinear_ensemble_sigmoid([z[rows] for z in self.zs], self.zs, self.w(s, e), precision=self.prec)

    def select_count(self, thr, s, e, eligible, exclude):
        return ops.bilinear_ensemble_select_count(self.zs, self.zs, self.w(s, e), thr, eligible=eligible, precision=self.prec,
                                                  exclude=_planes(exclude, s, e))

    def select(self, thr, s, e, eligible, max_bytes, exclude):
        return ops.bilinear_ensemble_select(self.zs, self.zs, self.w(s, e), thr, eligible=eligible, precision=self.prec, max_bytes=max_bytes,
                                            exclude=_planes(exclude, s, e))

    def bincount(self, edges, s, e, eligible, split):
        return ops.bilinear_ensemble_bincount(self.zs, self.zs, self.w(s, e), edges, eligible=eligible, precision=self.prec,
                                              split=_planes(split, s, e))

    def profile(self, rows, cols, thr, scale, s, e, eligible):
        zh = self.zs if rows is None else [z[rows] for z in self.zs]
        zt = self.zs if cols is None else [z[cols] for z in self.zs]
        return ops.bilinear_ensemble_profile(zh, zt, self.w(s, e), thr, scale=scale, eligible=eligible, precision=self.prec)


def _top_partners(head: _Head, k, label_range, drug_rows, max_temp_bytes, exclude):
    lo, hi = head.outcomes(label_range)
    N, dev = head.N, head.device
    rows = _index(drug_rows, N, "drug_rows", dev)
    excl = head.exclusion(exclude)
    if rows is None:
        return head.topk(k, lo, hi, "not_self", excl)
    n = int(rows.numel())
    vals = torch.empty((hi - lo, n, k), dtype=torch.float32, device=dev)
    idx = torch.empty((hi - lo, n, k), dtype=torch.int32, device=dev)
    chunk = max(1, int(max_temp_bytes) // max(N * k * 8, 1))
    for s in range(lo, hi, chunk):
        e = min(hi, s + chunk)
        v, i = head.topk(k, s, e, "not_self", excl)
        vals[s - lo:e - lo] = v[:, rows]
        idx[s - lo:e - lo] = i[:, rows]
    return vals, idx


@torch.no_grad()
def top_partners(model, z: torch.Tensor, k: int, label_range: Optional[Tuple[int, int]] = None, drug_rows=None,
                 max_temp_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """The ``k`` highest-scoring partners of every drug per outcome -> ``(vals, idx)`` [L', n, k] (fp32, int32): row i of
    outcome l holds the k largest S[l, i, j] over j != i and those j, ordered by (score descending, j ascending); padded with
    -inf / -1 when k > N - 1.  What the reference looks up in its stored [L,N,N] tensor (notebooks/quick_predictions.ipynb cell 8),
    without that tensor: ``decoder.topk`` keeps the lists inside the sweep.  ``z`` from ``generate_embeddings``.

    ``drug_rows``: only these drugs (indices into z; n = their number) -- the sweep still visits every drug, and the lists of
    ``drug_rows`` are picked from outcome chunks whose temporaries ([c, N, k] values and indices) stay under ``max_temp_bytes``.
    Without ``drug_rows`` the kernel writes straight into the result and there is no temporary.  The result itself is the
    caller's: L' * n * k * 8 bytes (1 024 outcomes x 100 352 drugs x k = 8: 6.6 GB).
    ``exclude``: a ``known_pairs_mask``; its pairs are skipped INSIDE the sweep, so the k partners are the k best NOVEL ones --
    for a drug with hundreds of known partners the lists would otherwise hold nothing else, and no post-filter can bring back
    what the sweep dropped.  A row with fewer than k partners left is padded.
    Multi-GPU: pass the outcome shard the rank owns as ``label_range``; no collective is involved."""
    return _top_partners(_ModelHead(model, z), k, label_range, drug_rows, max_temp_bytes, exclude)


@torch.no_grad()
def similar_drugs(z: torch.Tensor, k: int, rows=None, metric: str = "cosine"):
    """The ``k`` nearest OTHER drugs of every drug in embedding space -> ``(values fp32 [n, k], indices int64 [n, k])``, ordered by
    (value best-first, index ascending); ``z`` [N,128] from ``generate_embeddings``.  ``rows``: only these drugs (indices into z;
    n = their number) -- unlike ``top_partners`` the sweep then visits only their rows.  The drug itself is skipped inside the
    sweep (``ops.knn_topk``'s ``skip``), so 1 <= k <= min(32, N - 1).  metric: 'cosine', 'dot' or 'euclidean' (``retrieval.
    nearest_neighbors``); nothing of [n, N] is stored."""
    z = z.detach().float()
    N = z.shape[0]
    sel = _index(rows, N, "rows", z.device)
    skip = (torch.arange(N, device=z.device) if sel is None else sel).to(torch.int32)
    return nearest_neighbors(z if sel is None else z[sel], z, k, metric=metric, skip=skip)


def _best_pairs(v: torch.Tensor, i: torch.Tensor, j: torch.Tensor, K: int, N: int):
    """The first K of flat candidates (v, i, j) in the order (score descending, i ascending, j ascending)."""
    by_pair = torch.argsort(i * N + j)
    sv, o = torch.sort(v[by_pair], descending=True, stable=True)
    o = by_pair[o[:K]]
    return v[o], i[o], j[o]


def merge_row_candidates(vals: torch.Tensor, idx: torch.Tensor, K: int, rescore, info: Optional[dict] = None):
    """Step 2 and 3 of ``top_pairs`` on any device: from the per-row lists ``vals`` / ``idx`` [L, N, k_row] of the strict lower
    triangle (row i: its k_row best S[l, i, j], j < i, ordered by (score descending, j ascending), padded with -inf / -1) to the
    K best pairs of every outcome, exactly -> ``(vals [L, K] fp32, head [L, K] int64, tail [L, K] int64)`` ordered by (score
    descending, head ascending, tail ascending), padded with -inf / -1.

    The K best of the N * k_row candidates are taken first.  A pair the lists dropped sits behind its row's last entry in that
    order, so it can only belong to the answer if that entry lies strictly inside the K best (before their last place).  Rows
    that are truncated (i > k_row) and whose last entry does are "open" -- at most K / k_row per outcome; ``rescore(l, rows)``
    returns their dense scores [len(rows), N] (rows: ascending int64 indices), the lower-triangle part of which replaces their
    candidates, and the K best are taken again.  One round suffices: the K-th score only rises, so every other row stays
    closed and only its entries among the first K best can remain.  ``info["open_rows"]`` receives the open rows per outcome."""
    L, N, kr = vals.shape
    dev = vals.device
    out_v = torch.full((L, K), float("-inf"), dtype=torch.float32, device=dev)
    out_h = torch.full((L, K), -1, dtype=torch.int64, device=dev)
    out_t = torch.full((L, K), -1, dtype=torch.int64, device=dev)
    if info is not None:
        info["open_rows"] = [0] * L
    if L == 0 or K == 0 or N * kr == 0:
        return out_v, out_h, out_t
    take = min(K, N * kr)
    # row-major candidates are already in (i ascending, then the row's own order): a stable sort by score is the pair order
    sv, sp = torch.sort(vals.reshape(L, N * kr), dim=1, descending=True, stable=True)
    sv, sp = sv[:, :take], sp[:, :take]
    tail = torch.gather(idx.reshape(L, N * kr), 1, sp).long()
    head = torch.where(tail >= 0, sp // kr, torch.full_like(sp, -1))
    out_v[:, :take], out_h[:, :take], out_t[:, :take] = sv, head, tail
    inside = torch.arange(take, device=dev)[None, :] < K - 1
    opened = (tail >= 0) & (sp % kr == kr - 1) & (head > kr) & inside
    hits = opened.nonzero()
    if hits.numel() == 0:
        return out_v, out_h, out_t
    cols = torch.arange(N, device=dev)
    for l in torch.unique(hits[:, 0]).tolist():
        rows = torch.sort(head[l][opened[l]]).values
        if info is not None:
            info["open_rows"][l] = int(rows.numel())
        dense = rescore(l, rows).to(torch.float32)
        dense = torch.where(cols[None, :] < rows[:, None], dense, torch.full_like(dense, float("-inf")))
        closed = (tail[l] >= 0) & ~torch.isin(head[l], rows)
        v = torch.cat([sv[l][closed], dense.reshape(-1)])
        i = torch.cat([head[l][closed], rows[:, None].expand(-1, N).reshape(-1)])
        j = torch.cat([tail[l][closed], cols[None, :].expand(rows.numel(), -1).reshape(-1)])
        live = v > float("-inf")
        bv, bi, bj = _best_pairs(v[live], i[live], j[live], K, N)
        n = int(bv.numel())
        out_v[l].fill_(float("-inf"))
        out_h[l].fill_(-1)
        out_t[l].fill_(-1)
        out_v[l, :n], out_h[l, :n], out_t[l, :n] = bv, bi, bj
    return out_v, out_h, out_t


def _positive_int(K, name: str = "K") -> None:
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"{name}: expected a positive int, got {K!r}")


def _top_pairs(head: _Head, K, label_range, k_row, max_temp_bytes, info, exclude):
    max_k = ops.bilinear_topk_max_k()
    _positive_int(K)
    k_row = min(K, 16) if k_row is None else k_row
    if isinstance(k_row, bool) or not isinstance(k_row, int) or not 1 <= k_row <= max_k:
        raise ValueError(f"k_row: expected an int in 1..{max_k}, got {k_row!r}")
    lo, hi = head.outcomes(label_range)
    N, dev = head.N, head.device
    excl = head.exclusion(exclude)
    out_v = torch.empty((hi - lo, K), dtype=torch.float32, device=dev)
    out_h = torch.empty((hi - lo, K), dtype=torch.int64, device=dev)
    out_t = torch.empty((hi - lo, K), dtype=torch.int64, device=dev)
    opened = []
    chunk = max(1, int(max_temp_bytes) // max(N * k_row * 48, 1))
    for s in range(lo, hi, chunk):
        e = min(hi, s + chunk)
        vals, idx = head.topk(k_row, s, e, "lower", excl)
        part = {}

        def rescore(l, rows, s=s):
            dense = head.dense_rows(rows, s + l, s + l + 1)[0]
            if excl is not None:
                dense.masked_fill_(ops.pair_mask_rows(excl, 0 if excl.shape[0] == 1 else s + l, rows, N), float("-inf"))
            return dense

        v, h, t = merge_row_candidates(vals, idx, K, rescore, part)
        out_v[s - lo:e - lo], out_h[s - lo:e - lo], out_t[s - lo:e - lo] = v, h, t
        opened += part["open_rows"]
        del vals, idx, v, h, t
    if info is not None:
        info["open_rows"] = opened
    return out_v, out_h, out_t


@torch.no_grad()
def top_pairs(model, z: torch.Tensor, K: int, label_range: Optional[Tuple[int, int]] = None, k_row: Optional[int] = None,
              max_temp_bytes: int = 1 << 30, info: Optional[dict] = None, exclude: Optional[torch.Tensor] = None):
    """The ``K`` highest-scoring unordered drug pairs of every outcome -> ``(vals [L', K] fp32, head [L', K], tail [L', K]
    int64)``: the pair {i, j} is scored as S[l, i, j] with i > j (the strict lower triangle the rank normalisation reads,
    notebooks/normalize_scores.py:39-46; the value is the general sweep's (z_i W) z_j), ordered by (score descending, i ascending,
    j ascending), padded with -inf / -1 when K > N (N - 1) / 2.  Exact for every K, and no [L', N, N] tensor is made:
      1. ``decoder.topk`` in lower-triangle mode keeps the ``k_row`` best of every row inside the sweep (default min(K, 16), at most
         ``ops.bilinear_topk_max_k()``);
      2. the K best of the N * k_row candidates of an outcome (a sort on the device);
      3. the rows whose list was cut short AND whose last entry lies inside those K best are re-scored densely with the general
         sweep and merged (``merge_row_candidates``): at most K / k_row rows per outcome, none when k_row >= K.
    In "f32" / "bf16x3" the re-scored rows are bit-identical to what the sweep of step 1 saw.  In the 16-bit modes ("bf16" /
    "f16") the two sweeps group their fp32 sums differently (<= 2e-6 of the score scale): re-scored rows carry the dense sweep's
    values, so pairs closer than that may swap places against a brute-force ranking of either sweep.
    Temporaries: outcome chunks sized so that the candidate lists and their sort stay under ``max_temp_bytes`` (48 bytes per
    candidate), plus, per open outcome, the dense rows ([<= K / k_row, N] fp32).  Multi-GPU: pass the rank's outcome shard as
    ``label_range``.  ``info["open_rows"]``: open rows per outcome.
    ``exclude``: a ``known_pairs_mask``; the K best pairs NOT in it.  The row lists skip its pairs inside the sweep and the re-scored
    rows get -inf at their excluded columns (``ops.pair_mask_rows``), so the result is exact as before: a row is open under the
    same condition (removing columns only shortens what lies behind a row's last entry)."""
    return _top_pairs(_ModelHead(model, z), K, label_range, k_row, max_temp_bytes, info, exclude)


def _score_histogram(head: _Head, edges, label_range, eligible, known):
    split = head.exclusion(known, "known")
    lo, hi = head.outcomes(label_range)
    e = torch.as_tensor(edges, dtype=torch.float32, device=head.device)
    if e.dim() == 1:
        e = e[None, :].expand(hi - lo, -1)
    if e.dim() != 2 or e.shape[0] != hi - lo:
        raise ValueError(f"edges: expected [B] or [{hi - lo}, B], got {tuple(e.shape)}")
    return head.bincount(e.contiguous(), lo, hi, eligible, split)


@torch.no_grad()
def score_histogram(model, z: torch.Tensor, edges: torch.Tensor, label_range: Optional[Tuple[int, int]] = None,
                    eligible: str = "lower", known: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-outcome histogram of the all-pairs scores -> int64 [L', B+1]: ``counts[l, b]`` is the number of eligible pairs whose
    score lies in ``[edges[l, b-1], edges[l, b])`` (-inf below the first edge, +inf above the last), counted inside the sweep
    (``decoder.bincount``) -- no [L', N, N] tensor at any N.  ``edges``: ``[B]`` shared by all outcomes or ``[L', B]``, fp32,
    finite and ascending, 1 <= B <= ``ops.bilinear_bincount_max_edges()``.  ``eligible``: ``"lower"`` (the unordered pairs
    i > j the rank normalisation reads, the default), ``"not_self"`` or ``"all"``.  Cumulative sums of a row are the
    distribution function of the outcome's scores at the edges, from which quantiles follow.
    ``known``: a ``known_pairs_mask`` -> int64 [2, L', B+1]: the same sweep with the novel pairs (``[0]``, bit clear) and the known
    pairs (``[1]``, bit set) counted separately; nothing is excluded, ``result.sum(0)`` is the histogram without ``known``
    (``auroc_bounds_from_counts`` reads this form).
    Multi-GPU: pass the rank's outcome shard as ``label_range``; no collective is involved."""
    return _score_histogram(_ModelHead(model, z), edges, label_range, eligible, known)


def _cuts(thresholds, n_out: int, device) -> torch.Tensor:
    """fp32 [L'] on ``device`` from a number (one cut for every outcome) or one cut per outcome."""
    t = torch.as_tensor(thresholds, dtype=torch.float32, device=device)
    if t.dim() == 0:
        t = t.expand(n_out)
    if t.dim() != 1 or t.shape[0] != n_out:
        raise ValueError(f"thresholds: expected a number or [{n_out}] (one cut per outcome), got {tuple(t.shape)}")
    return t.contiguous()


def csr_rows(row_ptr: torch.Tensor, n_head: int, total: Optional[int] = None):
    """The (outcome, head) of every entry of a CSR over ``L * n_head`` rows numbered ``l * n_head + i`` (``ops.bilinear_select``'s
    ``row_ptr``, int64 [L * n_head + 1]) -> ``(outcome int64 [T], head int64 [T], offsets int64 [L + 1])``; ``offsets[l]`` is where
    outcome l's entries begin (``row_ptr[l * n_head]``).  Empty rows and empty outcomes contribute nothing.  ``total``: T =
    ``row_ptr[-1]`` where the caller knows it (on a GPU the expansion then needs no host read).  A pure tensor function (CPU or GPU)."""
    if row_ptr.dim() != 1 or row_ptr.numel() < 1 or n_head < 0 or (n_head == 0 and row_ptr.numel() != 1) or \
            (n_head > 0 and (row_ptr.numel() - 1) % n_head):
        raise ValueError(f"row_ptr: expected [L * {n_head} + 1], got {tuple(row_ptr.shape)}")
    rp = row_ptr.to(torch.int64)
    n_rows = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_rows, device=rp.device), rp[1:] - rp[:-1], output_size=total)
    if n_head == 0:
        return rows, rows.clone(), rp.clone()
    return rows // n_head, rows % n_head, rp[::n_head].clone()


def _partner_counts(head: _Head, thresholds, label_range, exclude):
    lo, hi = head.outcomes(label_range)
    return head.select_count(_cuts(thresholds, hi - lo, head.device), lo, hi, "not_self", head.exclusion(exclude))


def _select_above(head: _Head, thresholds, label_range, eligible, max_bytes, exclude):
    lo, hi = head.outcomes(label_range)
    return head.select(_cuts(thresholds, hi - lo, head.device), lo, hi, eligible, max_bytes, head.exclusion(exclude))


def _pairs_above(head: _Head, thresholds, label_range, max_bytes, exclude):
    row_ptr, cols, vals = _select_above(head, thresholds, label_range, "lower", max_bytes, exclude)
    _, pair_head, offsets = csr_rows(row_ptr, head.N, total=int(cols.numel()))
    if head.N == 0:
        lo, hi = head.outcomes(label_range)
        offsets = torch.zeros(hi - lo + 1, dtype=torch.int64, device=head.device)
    return offsets, pair_head, cols.long(), vals


@torch.no_grad()
def partner_counts(model, z: torch.Tensor, thresholds, label_range: Optional[Tuple[int, int]] = None,
                   exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How many partners j != i of every drug score at or above the outcome's cut -> int32 [L', N]: ``counts[l, i]`` =
    #{j != i : S[l, i, j] >= thresholds[l]}, the degree of drug i in outcome l's predicted interaction network, counted inside the
    sweep (``decoder.select_count``, ``not_self`` mode) -- no [L', N, N] tensor at any N.  ``thresholds``: a number or [L'], no NaN.
    ``exclude``: a ``known_pairs_mask``; its pairs are not counted (the degree in the NOVEL predicted network).
    Multi-GPU: pass the rank's outcome shard as ``label_range``; no collective is involved."""
    return _partner_counts(_ModelHead(model, z), thresholds, label_range, exclude)


@torch.no_grad()
def partners_above(model, z: torch.Tensor, thresholds, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 1 << 30,
                   exclude: Optional[torch.Tensor] = None):
    """ALL partners of every drug at or above the outcome's cut, as CSR -> ``(row_ptr int64 [L' * N + 1], cols int32 [T], vals fp32
    [T])``: row ``l * N + i`` lists the j != i with S[l, i, j] >= thresholds[l] in ascending order and those scores (``decoder.select``,
    ``not_self`` mode; ``csr_rows(row_ptr, N)`` gives every entry's outcome and drug).  Where ``top_partners`` returns the k best of a
    drug, this returns its whole neighbourhood in the predicted network; every unordered pair appears from both sides, with
    S[l, i, j] and S[l, j, i] (equal up to the last bits).  The result's size is known only after the counting sweep: more than
    ``max_bytes`` (8 bytes per entry) raises a ValueError naming the size.  ``thresholds``: a number or [L'], no NaN.
    ``exclude``: a ``known_pairs_mask``; its pairs are neither counted nor stored."""
    return _select_above(_ModelHead(model, z), thresholds, label_range, "not_self", max_bytes, exclude)


@torch.no_grad()
def pairs_above(model, z: torch.Tensor, thresholds, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 1 << 30,
                exclude: Optional[torch.Tensor] = None):
    """ALL unordered drug pairs of every outcome that score at or above its cut -- the outcome's predicted interaction network --
    -> ``(offsets int64 [L' + 1], head int64 [T], tail int64 [T], vals fp32 [T])``: outcome l owns the entries
    ``offsets[l]:offsets[l + 1]``.  The pair {i, j} is scored as S[l, i, j] with i > j, the strict-lower-triangle entry ``top_pairs``,
    ``pair_ranks`` and the rank normalisation use (notebooks/normalize_scores.py:39-46), and is selected when that score is
    ``>= thresholds[l]``; the entries are ordered by (outcome, head, tail) ascending.  Nothing of [L', N, N] is materialised
    (``decoder.select``, ``lower`` mode: a counting and a filling sweep); ``head`` is expanded from the sweep's row pointers
    (``csr_rows``).  More than ``max_bytes`` (8 bytes per pair in the sweep's result) raises a ValueError naming the size.

    Where a cut comes from (``thresholds``: a number or [L'], no NaN):
      * the K-th value of ``top_pairs``: ``pairs_above(model, z, top_pairs(model, z, K)[0][:, -1])`` holds those K pairs and every
        pair tied with the last of them (the rule is ``>=``);
      * an edge of ``score_histogram``: the pairs of the bins at and above it, whose number the histogram already told.
    ``normalized_ranks_of(model, z, vals)`` -- per outcome, e.g. on ``vals[offsets[l]:offsets[l + 1]][None, :]`` with
    ``label_range=(l, l + 1)`` -- gives the normalised ranks of what was selected.
    ``exclude``: a ``known_pairs_mask``; the known network is neither counted nor stored, so a cut low enough to be interesting
    returns (and sizes ``max_bytes`` by) the novel pairs alone.  Ranks stay those over ALL pairs (``normalized_ranks_of``).
    Multi-GPU: pass the rank's outcome shard as ``label_range``; no collective is involved."""
    return _pairs_above(_ModelHead(model, z), thresholds, label_range, max_bytes, exclude)


@torch.no_grad()
def count_below(model, z: torch.Tensor, scores: torch.Tensor, label_range: Optional[Tuple[int, int]] = None,
                known: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For every query ``scores[l, q]`` the number of strict-lower-triangle pairs (i > j) of outcome l that score strictly less
    -> int64 [L', Q].  Any Q; the queries may be unsorted and repeated.  Per outcome they are sorted and deduplicated, the
    counting sweep (``decoder.bincount``, lower-triangle mode) runs once per chunk of at most ``ops.bilinear_bincount_max_edges()``
    edges, the cumulative sum of a chunk's counts is the answer for its edges (chunks are independent: bin 0 of every chunk
    already holds everything below its first edge), and the answers are scattered back to the queries' places.
    ``known``: a ``known_pairs_mask`` -> int64 [2, L', Q]: the novel pairs (``[0]``) and the known pairs (``[1]``) below every query,
    counted separately in the same sweeps; ``result.sum(0)`` is the answer without ``known``.
    Multi-GPU: pass the rank's outcome shard as ``label_range``."""
    return _count_below(_ModelHead(model, z), scores, label_range, known)[0]


def _count_below(head: _Head, scores, label_range, known, name: Optional[str] = None):
    """``count_below`` -> (its result, the row sums of the first chunk's count table(s): the number of eligible pairs per outcome
    [L'], or per class and outcome [2, L']; None when no sweep ran).  ``name``: what the queries are called in messages."""
    split = head.exclusion(known, "known")
    lo, hi = head.outcomes(label_range)
    s = torch.as_tensor(scores, dtype=torch.float32, device=head.device)
    if s.dim() != 2 or s.shape[0] != hi - lo:
        raise ValueError(f"{name or head.scores}: expected [{hi - lo}, Q], got {tuple(s.shape)}")
    return _count_below_sweeps(lambda edges: head.bincount(edges, lo, hi, "lower", split), s, split is not None)


def _count_below_sweeps(counting, s: torch.Tensor, split: bool):
    """The sort / dedup / chunk / scatter of ``count_below`` and ``ensemble_count_below`` around a counting sweep: ``counting(edges)``
    -> the lower-triangle counts int64 [L', B+1] (``split``: [2, L', B+1]) of contiguous fp32 ``edges`` [L', B], B <=
    ``ops.bilinear_bincount_max_edges()``.  ``s``: the queries, fp32 [L', Q] on the sweep's device -> (less, totals) as ``_count_below``."""
    L, Q = s.shape
    less = torch.zeros((2, L, Q) if split else (L, Q), dtype=torch.int64, device=s.device)
    if L == 0 or Q == 0:
        return less, None
    if not bool(torch.isfinite(s).all()):
        raise ValueError("scores: queries must be finite")
    sv, order = torch.sort(s, dim=1)
    new = torch.ones_like(sv, dtype=torch.bool)
    new[:, 1:] = sv[:, 1:] != sv[:, :-1]
    pos = torch.cumsum(new, 1) - 1                              # place of every sorted query among its outcome's distinct values
    U = int(pos.max()) + 1
    uniq = sv[:, -1:].expand(L, U).clone()                      # outcomes with fewer distinct values: the largest one repeated (empty bins)
    uniq.scatter_(1, pos, sv)
    below = torch.empty(less.shape[:-1] + (U,), dtype=torch.int64, device=s.device)
    step = ops.bilinear_bincount_max_edges()
    totals = None
    for c0 in range(0, U, step):
        c1 = min(U, c0 + step)
        counts = counting(uniq[:, c0:c1].contiguous())
        below[..., c0:c1] = torch.cumsum(counts, -1)[..., : c1 - c0]
        totals = counts.sum(-1) if totals is None else totals
    if not split:
        less.scatter_(1, order, torch.gather(below, 1, pos))
    else:
        less.scatter_(2, order.expand(2, -1, -1), torch.gather(below, 2, pos.expand(2, -1, -1)))
    return less, totals


def recovery_from_counts(less_all: torch.Tensor, less_known: torch.Tensor, total, n_known) -> dict:
    """How well a score cut recovers the known network, from counts -> dict of ``selected``, ``hits`` (int64) and ``precision``,
    ``recall``, ``enrichment`` (float64), all of ``less_all``'s shape.  ``less_all`` / ``less_known``: the number of all / of the known
    pairs scoring strictly below the cut (``count_below(known=)``: ``[0] + [1]`` and ``[1]``); ``total`` / ``n_known``: the number of
    all / of the known pairs (ints or tensors that broadcast, e.g. ``[L', 1]``).
      selected = total - less_all            pairs at or above the cut
      hits = n_known - less_known            known pairs among them
      precision = hits / selected            (NaN where nothing is selected)
      recall = hits / n_known                (NaN where nothing is known)
      enrichment = precision / (n_known / total)       over the base rate of known pairs
    A pure tensor function (CPU or GPU)."""
    la, lk = torch.as_tensor(less_all).to(torch.int64), torch.as_tensor(less_known).to(torch.int64)
    tot = torch.as_tensor(total, device=la.device).to(torch.int64)
    nk = torch.as_tensor(n_known, device=la.device).to(torch.int64)
    selected = tot - la
    hits = nk - lk
    selected, hits, tot_b, nk_b = torch.broadcast_tensors(selected, hits, tot, nk)
    nan = torch.full(selected.shape, float("nan"), dtype=torch.float64, device=la.device)
    precision = torch.where(selected == 0, nan, hits.double() / selected.double())
    recall = torch.where(nk_b == 0, nan, hits.double() / nk_b.double())
    enrichment = precision / (nk_b.double() / tot_b.double())
    return {"selected": selected.contiguous(), "hits": hits.contiguous(), "precision": precision, "recall": recall, "enrichment": enrichment}


def _need_known(known) -> None:
    if known is None:
        raise ValueError("known: expected a mask from known_pairs_mask")


def _recovery_at_cuts(head: _Head, known, cuts, label_range):
    _need_known(known)
    less, totals = _count_below(head, cuts, label_range, known, "cuts")
    if totals is None:                                          # no outcome or no cut: nothing was swept
        totals = torch.zeros((2, less.shape[1]), dtype=torch.int64, device=less.device)
    return recovery_from_counts(less[0] + less[1], less[1], (totals[0] + totals[1])[:, None], totals[1][:, None])


@torch.no_grad()
def recovery_at_cuts(model, z: torch.Tensor, known: torch.Tensor, cuts: torch.Tensor, label_range: Optional[Tuple[int, int]] = None) -> dict:
    """How well the ranking of ALL N (N - 1) / 2 pairs recovers the known network -> the dict of ``recovery_from_counts``, every entry
    [L', B]: for each cut ``cuts[l, b]`` (any order, repeats allowed) the pairs of the strict lower triangle scoring at or above it
    (``selected``), the known ones among them (``hits``) and the exact precision, recall and enrichment -- over every pair, not over
    sampled negatives, with no [L', N, N] tensor.  ``known``: a ``known_pairs_mask``.  ``count_below(known=)`` followed by
    ``recovery_from_counts``; the number of known pairs per outcome is read from the same sweeps (the row sum of a count table is
    its class's size), so a per-outcome mask needs no side information.  A known pair is scored with the sweep's own arithmetic: it
    cannot fall on the wrong side of a cut taken from ``top_pairs`` / ``score_histogram``."""
    return _recovery_at_cuts(_ModelHead(model, z), known, cuts, label_range)


def auroc_bounds_from_counts(counts: torch.Tensor):
    """Bounds on the AUROC of ranking all eligible pairs with the known ones as positives, from the split counts [2, L', B+1] of
    ``score_histogram(known=)`` -> ``(lower, upper)`` float64 [L'].  With u = counts[0] (novel), k = counts[1] (known), U = sum u,
    K = sum k:
      lower = sum_b k[b] (sum_{b' < b} u[b']) / (K U)        the (known, novel) pairs the bins already order correctly
      upper = lower + sum_b k[b] u[b] / (K U)                plus those that share a bin
    The exact AUROC (ties counted 1/2) lies in [lower, upper]; an edge between every two distinct scores makes them meet it where no
    known and novel pair tie.  The sums are int64 (exact below 2^63: every shape the sweep accepts), then one float64 divide; NaN where
    K == 0 or U == 0.  A pure tensor function (CPU or GPU)."""
    c = torch.as_tensor(counts)
    if c.dim() != 3 or c.shape[0] != 2:
        raise ValueError(f"counts: expected [2, L', B + 1], got {tuple(c.shape)}")
    u, k = c[0].to(torch.int64), c[1].to(torch.int64)
    U, K = u.sum(1), k.sum(1)
    u_below = torch.cumsum(u, 1) - u                           # novel pairs in lower bins
    sure = (k * u_below).sum(1)
    tied = (k * u).sum(1)
    den = (K * U).double()
    nan = torch.full_like(den, float("nan"))
    bad = (K == 0) | (U == 0)
    lower = torch.where(bad, nan, sure.double() / den)
    upper = torch.where(bad, nan, (sure + tied).double() / den)
    return lower, upper


def _auroc_bounds(head: _Head, known, edges, label_range):
    _need_known(known)
    return auroc_bounds_from_counts(_score_histogram(head, edges, label_range, "lower", known))


@torch.no_grad()
def auroc_bounds(model, z: torch.Tensor, known: torch.Tensor, edges: torch.Tensor, label_range: Optional[Tuple[int, int]] = None):
    """Per-outcome AUROC bounds of the model's ranking of ALL strict-lower-triangle pairs against the known network ->
    ``(lower, upper)`` float64 [L']: ``score_histogram(known=)`` followed by ``auroc_bounds_from_counts`` -- one sweep, no [L', N, N]
    tensor, no sampled negatives.  More (or better placed) ``edges`` tighten the interval; up to
    ``ops.bilinear_bincount_max_edges()`` per sweep."""
    return _auroc_bounds(_ModelHead(model, z), known, edges, label_range)


PROFILE_CHUNK = 65535          # outcomes per call of the profile sweep (count and best share a register there)


def _profile_chunks(head: _Head, rows, cols, thr, scale, lo, hi, eligible, chunk):
    """``head.profile`` of the drug slices ``rows`` x ``cols`` over the outcomes [lo, hi) in chunks, merged -> (count, best, margin),
    ``best`` relative to ``lo``."""
    res = None
    for s in range(lo, max(hi, lo + 1), chunk):
        e = min(hi, s + chunk)
        part = head.profile(rows, cols, thr[s - lo:e - lo], None if scale is None else scale[s - lo:e - lo], s, e, eligible)
        res = part if res is None else ops.profile_merge(res, part, s - lo)
    return res


def _outcome_profile(head: _Head, thresholds, scale, label_range, eligible, head_rows, chunk, exclude=None):
    if eligible not in ops.TOPK_ELIGIBLE:
        raise ValueError(f"unknown eligible {eligible!r}; expected one of {sorted(ops.TOPK_ELIGIBLE)}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= PROFILE_CHUNK:
        raise ValueError(f"chunk: expected an int in 1..{PROFILE_CHUNK}, got {chunk!r}")
    excl = _shared_plane(exclude)
    lo, hi = head.outcomes(label_range)
    N, dev = head.N, head.device
    thr = _cuts(thresholds, hi - lo, dev)
    sc = None if scale is None else _cuts(scale, hi - lo, dev)
    out = None                                  # the entries to blank afterwards
    if head_rows is None:
        r0, r1 = 0, N
        count, best, margin = _profile_chunks(head, None, None, thr, sc, lo, hi, eligible, chunk)
    else:
        r0, r1 = head_rows
        if not (0 <= r0 <= r1 <= N):
            raise ValueError(f"head_rows {head_rows} outside [0, {N}]")
        # a rectangle: the sweep runs in "all" mode and the block's self / upper entries are blanked here
        count, best, margin = _profile_chunks(head, slice(r0, r1), None, thr, sc, lo, hi, "all", chunk)
        if eligible != "all":
            i = torch.arange(r0, r1, device=dev)[:, None]
            j = torch.arange(N, device=dev)[None, :]
            out = (j == i) if eligible == "not_self" else (j >= i)
    if excl is not None:
        known = ops.pair_mask_rows(excl, 0, torch.arange(r0, r1, device=dev), N)
        out = known if out is None else (out | known)
    if out is not None:
        count = count.masked_fill(out, 0)
        best = best.masked_fill(out, -1)
        margin = margin.masked_fill(out, float("-inf"))
    best = best.long()
    return count, torch.where(best >= 0, best + lo, best), margin


@torch.no_grad()
def outcome_profile(model, z: torch.Tensor, thresholds, scale=None, label_range: Optional[Tuple[int, int]] = None,
                    eligible: str = "not_self", head_rows: Optional[Tuple[int, int]] = None, chunk: int = PROFILE_CHUNK):
    """The screen seen per PAIR instead of per outcome -> ``(count int32, best int64, margin fp32)``, each [N, N] (or [r1 - r0, N]
    with ``head_rows``): for the pair (i, j), over the outcomes ``label_range`` (default: all), ``count`` is the number of outcomes
    with S[l, i, j] >= thresholds[l] -- for how many interaction types the pair is flagged --, ``margin`` the largest
    ``(S[l, i, j] - thresholds[l]) * scale[l]`` and ``best`` the MODEL's index of the lowest outcome attaining it (-1 where no
    outcome moved the pair off -inf).  Nothing of [L', N, N] is materialised (``decoder.profile``: one sweep per ``chunk`` <= 65535
    outcomes, merged with ``ops.profile_merge``).  ``thresholds``: a number or [L'], no NaN (cuts come from ``top_pairs``,
    ``score_histogram`` or ``count_below``); ``scale``: None, a positive number or [L'] (e.g. one over an outcome's score spread, to
    compare margins across outcomes).  ``eligible``: ``"not_self"`` (default), ``"lower"`` (j < i) or ``"all"``; ineligible entries
    hold 0 / -1 / -inf.  ``head_rows`` = (r0, r1): only drugs [r0, r1) against all drugs, with the same eligibility in the
    coordinates of the full matrix; the row blocks concatenate to the full result (row sharding across ranks or over time).
    Multi-GPU over outcomes: pass the rank's shard as ``label_range`` and merge the shards with ``ops.profile_merge``."""
    return _outcome_profile(_ModelHead(model, z), thresholds, scale, label_range, eligible, head_rows, chunk)


def _profile_keys(count: torch.Tensor, margin: torch.Tensor) -> torch.Tensor:
    """int64 keys whose descending order is (count descending, margin descending); -0.0 and +0.0 compare equal."""
    b = (margin + 0.0).contiguous().view(torch.int32).long()
    mkey = torch.where(b < 0, -(b & 0x7FFFFFFF) - 1, b) + (1 << 31)              # ascending with the float, in [0, 2^32)
    return (count.long() << 32) | mkey


def _shared_plane(exclude) -> Optional[torch.Tensor]:
    """``exclude`` of the per-pair products: ONE plane from ``known_pairs_mask``, applied to the finished profile (exact, since a
    pair is excluded under every outcome or under none).  A plane per outcome would change the counts outcome by outcome, inside
    the sweep: out of scope."""
    if exclude is not None and _mask3(exclude, "exclude").shape[0] != 1:
        raise ValueError(f"exclude: {exclude.shape[0]} planes; the per-pair profiles take one shared plane (known_pairs_mask without "
                         f"labels) -- a plane per outcome changes the counts inside the sweep and is out of scope")
    return exclude


def _most_flagged(profile_block, N: int, K: int, lo: int, max_bytes: int, dev, exclude: Optional[torch.Tensor] = None):
    """The row-block walk, key construction and running best K that ``most_flagged_pairs`` and ``ensemble_most_flagged_pairs`` share.
    ``profile_block(r0, r1)`` -> the ALL-mode profile (count int32, best, margin fp32), each [r1 - r0, r1], of rows [r0, r1) against
    the drugs [0, r1), ``best`` relative to ``lo``.  ``exclude``: one shared plane; its pairs never enter the ranking."""
    rows = max(1, int(max_bytes) // max(48 * N, 1))
    if rows >= 256:
        rows -= rows % 256                      # whole workgroups of the sweep
    run = None                                  # (key, count, head, tail, best, margin) of the best K so far, in result order
    for r0 in range(1, N, rows):                # row 0 has no column below it
        r1 = min(N, r0 + rows)
        count, best, margin = profile_block(r0, r1)
        i = torch.arange(r0, r1, device=dev)[:, None]
        j = torch.arange(r1, device=dev)[None, :]
        key = _profile_keys(count, margin).masked_fill_(j >= i, -1)
        if exclude is not None:
            key.masked_fill_(ops.pair_mask_rows(exclude, 0, torch.arange(r0, r1, device=dev), r1), -1)
        key = key.reshape(-1)
        k = min(K, key.numel())
        kth = torch.topk(key, k, sorted=True).values[-1].clamp_(min=0)          # (>= 0: ineligible entries never enter)
        flat = torch.nonzero(key >= kth).reshape(-1)                           # ascending (i, j)
        ci, cj = flat // r1, flat % r1
        cand = (key[flat], count[ci, cj], ci + r0, cj, best[ci, cj].long(), margin[ci, cj])
        if run is not None:
            cand = tuple(torch.cat([a, b]) for a, b in zip(run, cand))          # earlier rows first
        order = torch.sort(cand[0], descending=True, stable=True).indices[:K]
        run = tuple(t[order] for t in cand)
        del count, best, margin, key, flat
    out_c = torch.zeros(K, dtype=torch.int32, device=dev)
    out_h = torch.full((K,), -1, dtype=torch.int64, device=dev)
    out_t = torch.full((K,), -1, dtype=torch.int64, device=dev)
    out_b = torch.full((K,), -1, dtype=torch.int64, device=dev)
    out_m = torch.full((K,), float("-inf"), dtype=torch.float32, device=dev)
    if run is not None:
        n = run[0].numel()
        out_c[:n], out_h[:n], out_t[:n], out_m[:n] = run[1], run[2], run[3], run[5]
        out_b[:n] = torch.where(run[4] >= 0, run[4] + lo, run[4])
    return out_c, out_h, out_t, out_b, out_m


def _most_flagged_pairs(head: _Head, thresholds, K, scale, label_range, max_bytes, exclude):
    excl = _shared_plane(exclude)
    _positive_int(K)
    lo, hi = head.outcomes(label_range)
    thr = _cuts(thresholds, hi - lo, head.device)
    sc = None if scale is None else _cuts(scale, hi - lo, head.device)
    return _most_flagged(lambda r0, r1: _profile_chunks(head, slice(r0, r1), slice(0, r1), thr, sc, lo, hi, "all", PROFILE_CHUNK), head.N, K, lo,
                         max_bytes, head.device, excl)


@torch.no_grad()
def most_flagged_pairs(model, z: torch.Tensor, thresholds, K: int, scale=None, label_range: Optional[Tuple[int, int]] = None,
                       max_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """The ``K`` unordered drug pairs flagged for the most outcomes -> ``(count int32 [K], head int64 [K], tail int64 [K], best
    int64 [K], margin fp32 [K])``: the pair {i, j} is profiled as (i, j) with i > j (the strict lower triangle ``top_pairs`` uses),
    ordered by (count descending, margin descending, i ascending, j ascending); ``count``, ``best`` and ``margin`` are those of
    ``outcome_profile``.  Padded with 0 / -1 / -1 / -1 / -inf when K > N (N - 1) / 2.  Streams over row blocks -- rows [r0, r1)
    against the drugs [0, r1), the rest of the block being the upper triangle -- sized so that a block's profile and its selection
    temporaries (about 48 bytes per pair) stay under ``max_bytes``, and keeps a running best K: no [N, N] tensor either, so it
    runs at any N.  Exact: a tie at the K-th place is broken by (i, j) like every other.  ``exclude``: ONE shared plane from
    ``known_pairs_mask`` (no ``labels``); its pairs are left out of the ranking, so the result lists novel pairs only (a plane per
    outcome is refused: it would change the counts inside the sweep)."""
    return _most_flagged_pairs(_ModelHead(model, z), thresholds, K, scale, label_range, max_bytes, exclude)


# ---- per-pair highest outcomes of a rank or score tensor, streamed (ops.outcome_topk) ----
HOST_OUTCOME_CHUNK = 16          # outcomes per staged chunk of a host tensor, as score_all_pairs' host_chunk


def _kept_labels(keep, n_all: int, lo: int, hi: int) -> torch.Tensor:
    """int64 CPU [hi - lo]: the model's outcome id of each outcome of [lo, hi), -1 where ``keep`` (ids or a bool mask over all
    ``n_all`` outcomes; None keeps everything) drops it."""
    ids = torch.arange(lo, hi)
    if keep is None:
        return ids
    kp = torch.as_tensor(keep).cpu()
    if kp.dtype == torch.bool:
        if tuple(kp.shape) != (n_all,):
            raise ValueError(f"keep: a bool mask must have one entry per outcome of the head ([{n_all}]), got {tuple(kp.shape)}")
        mask = kp
    else:
        if kp.dtype not in (torch.int32, torch.int64) or kp.dim() != 1:
            raise ValueError(f"keep: expected outcome ids or a bool mask, got {kp.dtype} {tuple(kp.shape)}")
        if kp.numel() and (int(kp.min()) < 0 or int(kp.max()) >= n_all):
            raise ValueError(f"keep: outcome ids must lie in [0, {n_all})")
        mask = torch.zeros(n_all, dtype=torch.bool)
        mask[kp.long()] = True
    return torch.where(mask[lo:hi], ids, torch.full_like(ids, -1))


def _with_mean(state, k: int, Nh: int, Nt: int, device, largest: bool):
    if state is None:                                    # nothing was folded: the sentinels
        state = ops.outcome_topk(torch.empty((0, Nh, Nt), dtype=torch.float32, device=device), k, largest=largest)
    return state[0], state[1], state[0].mean(0)


@torch.no_grad()
def highest_outcomes_of(x, k: int = 5, *, labels=None, largest: bool = True, eligible: str = "all", chunk: Optional[int] = None,
                        max_bytes: int = 8 << 30):
    """The k highest values over the OUTCOMES of a stored rank or score tensor ``x`` [L, N, N], per drug pair ->
    ``(vals fp32 [k,N,N], idx int32 [k,N,N], mean fp32 [N,N])``: the reference's ``highest_5_scores``, ``highest_5_ddi_classes`` and
    ``highest_5_mean`` (notebooks/fig5/fig5_t2d_mash.ipynb:2034-2039; ``np.mean(np.partition(lst, len(lst)-5)[-5:])`` at :1442-1448)
    for every pair at once, ordered (value descending, outcome ascending); ``largest=False`` gives the lowest k (:2050).
    ``mean = vals.mean(0)``: -inf (+inf) where fewer than k outcomes were kept.

    ``x``: a CUDA tensor (float32 / float16 / bfloat16, contiguous or row-pitched) -- folded where it lies, nothing is copied
    (``chunk``: outcomes per fold, default all in one call) -- or a numpy array / ``np.memmap`` of float32 or float16, the
    reference's ``np.load(..., mmap_mode="r")`` rank file: chunks of ``chunk`` outcomes (default 16, fewer if two device chunks
    exceed ``max_bytes``) go host -> pinned staging -> device on a copy stream while the previous chunk is folded.
    ``labels``: the outcome id of each plane of ``x`` (default 0..L-1); a negative id drops the plane (the reference's
    ``to_delete_classes``), and a host chunk with nothing kept is not copied.  ``eligible``: ``"all"`` or ``"lower"`` (i > j)."""
    on_gpu = isinstance(x, torch.Tensor)
    if on_gpu and not x.is_cuda:
        raise ValueError("x: a torch tensor must live on the GPU (pass host data as a numpy array or np.memmap)")
    if not on_gpu and not (isinstance(x, np.ndarray) and x.dtype in (np.float32, np.float16)):
        raise ValueError("x: expected a CUDA tensor, or a float32 / float16 numpy array or memmap")
    if x.ndim != 3:
        raise ValueError(f"x: expected [L, Nh, Nt], got shape {tuple(x.shape)}")
    L, Nh, Nt = x.shape
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"chunk: expected a positive int, got {chunk!r}")
    lab = None
    if labels is not None:
        lab = torch.as_tensor(labels).cpu()
        if lab.dtype not in (torch.int32, torch.int64) or tuple(lab.shape) != (L,):
            raise ValueError(f"labels: expected {L} integer outcome ids, got {lab.dtype} {tuple(lab.shape)}")
    if on_gpu:
        dev = x.device
        step = max(L, 1) if chunk is None else chunk
        state = None
        for s in range(0, L, step):
            e = min(L, s + step)
            kw = {"label_base": s} if lab is None else {"labels": lab[s:e].to(dev)}
            state = ops.outcome_topk(x[s:e], k, largest=largest, eligible=eligible, state=state, **kw)
        return _with_mean(state, k, Nh, Nt, dev, largest)
    dev = torch.device("cuda", torch.cuda.current_device())
    dtype = torch.float32 if x.dtype == np.float32 else torch.float16
    pitch = ops.empty_scores(0, Nh, Nt, dev, dtype=dtype).stride(1) if Nt else 1
    step = HOST_OUTCOME_CHUNK if chunk is None else chunk
    step = max(1, min(step, max(L, 1), int(max_bytes) // max(2 * Nh * pitch * x.dtype.itemsize, 1)))
    cur, copy_stream = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)
    dev_buf = [ops.empty_scores(step, Nh, Nt, dev, dtype=dtype) for _ in range(2)]          # row-pitched on the device, spread by the copy
    pin_buf = [torch.empty((step, Nh, Nt), dtype=dtype, pin_memory=True) for _ in range(2)]
    copy_stream.wait_stream(cur)                           # the device chunks come from this stream's pool
    folded = [None, None]
    state, n = None, 0
    for s in range(0, L, step):
        e = min(L, s + step)
        if lab is not None and not bool((lab[s:e] >= 0).any()):
            continue
        b = n & 1
        n += 1
        if folded[b] is not None:                          # staging pair b is free once the fold that read it has finished
            folded[b].synchronize()
        pin_buf[b][: e - s].numpy()[...] = x[s:e]          # host read of chunk n overlaps the copy and the fold of chunk n - 1
        with torch.cuda.stream(copy_stream):
            dev_buf[b][: e - s].copy_(pin_buf[b][: e - s], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(copy_stream)
        cur.wait_event(ready)
        kw = {"label_base": s} if lab is None else {"labels": lab[s:e].to(dev)}
        state = ops.outcome_topk(dev_buf[b][: e - s], k, largest=largest, eligible=eligible, state=state, **kw)
        folded[b] = torch.cuda.Event()
        folded[b].record(cur)
    copy_stream.synchronize()
    return _with_mean(state, k, Nh, Nt, dev, largest)


def _outcome_chunks(lab: torch.Tensor, lo: int, hi: int, chunk: int):
    """(s, e, labels int32 CPU) of every outcome chunk of [lo, hi) that keeps at least one outcome."""
    for s in range(lo, hi, chunk):
        e = min(hi, s + chunk)
        part = lab[s - lo:e - lo]
        if bool((part >= 0).any()):
            yield s, e, part.to(torch.int32)


@torch.no_grad()
def highest_outcomes(model, z: torch.Tensor, k: int = 5, *, of: str = "ranks", keep=None, label_range: Optional[Tuple[int, int]] = None,
                     scale=None, shift=None, largest: bool = True, max_bytes: int = 8 << 30):
    """The k highest outcomes of every drug pair, straight from the model -> ``(vals fp32 [k,N,N], idx int32 [k,N,N], mean fp32
    [N,N])``, ``idx`` the MODEL's outcome indices: ``highest_outcomes_of`` without the [L,N,N] tensor ever existing.  Per outcome
    chunk the tensor is produced and folded into the per-pair lists (``ops.outcome_topk``), so memory is ``16 k N^2`` bytes of
    state (8 k stored, read and written once per chunk) plus one chunk.

    ``of="ranks"``: the normalised ranks of ``rank_all_pairs`` (ranks are per outcome, so chunking over outcomes is exact) -- the
    reference's highest-5 mean of one seed.  ``of="scores"``: the head's fp32 scores, folded as ``(S - shift[l]) * scale[l]``
    (``shift`` / ``scale``: None, a number or [L'], e.g. an outcome's mean and one over its spread, to make logits comparable
    across outcomes; ``scale`` finite and > 0).  ``keep``: outcome ids or a bool mask over all outcomes of the head; dropped
    outcomes (the reference's ``to_delete_classes``) never enter a list, and a chunk with nothing kept is not computed at all.
    ``label_range``: only these outcomes (an outcome shard; merge shards with ``ops.outcome_topk_merge``).

    The chunk holds as many outcomes as ``max_bytes`` (default 8 GiB, as elsewhere here) allows.  Every fold reads and writes the
    state, ``16 k`` bytes per pair per call against ``4`` bytes per pair per outcome, so small chunks are dominated by state
    traffic: leave room for >= 64 outcomes per chunk when memory allows."""
    if of not in ("ranks", "scores"):
        raise ValueError(f"of: expected 'ranks' or 'scores', got {of!r}")
    if of == "ranks" and (scale is not None or shift is not None):
        raise ValueError("shift / scale apply to of='scores' (normalised ranks are comparable across outcomes as they are)")
    head = _ModelHead(model, z)
    lo, hi = head.outcomes(label_range)
    N, dev = head.N, head.device
    lab = _kept_labels(keep, head.n_outcomes, lo, hi)
    sh = None if shift is None else _cuts(shift, hi - lo, dev)
    sc = None if scale is None else _cuts(scale, hi - lo, dev)
    plane = N * ops.empty_scores(0, N, N, dev).stride(1) * 4 if N else 1
    chunk = max(1, min(max(hi - lo, 1), int(max_bytes) // plane))
    buf = ops.empty_scores(chunk, N, N, dev)
    state = None
    for s, e, part in _outcome_chunks(lab, lo, hi, chunk):
        if of == "ranks":
            x = rank_all_pairs(model, z, (s, e), out=buf[: e - s])
        else:
            x = score_all_pairs(model, z, (s, e), out=buf[: e - s])
        state = ops.outcome_topk(x, k, labels=part.to(dev), shift=None if sh is None else sh[s - lo:e - lo],
                                 scale=None if sc is None else sc[s - lo:e - lo], largest=largest, state=state)
    return _with_mean(state, k, N, N, dev, largest)


@torch.no_grad()
def ensemble_highest_outcomes(models, zs, k: int = 5, *, keep=None, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 8 << 30):
    """The paper's ranking of candidate combinations, end to end -> ``(vals, idx, mean)`` as ``highest_outcomes``: per outcome
    chunk the normalised ranks of every seed (``rank_all_pairs``), their geometric mean re-ranked (``ops.ensemble_ranks``,
    generate_embeddings.ipynb cells 18-20), folded into the per-pair highest-k lists -- the ``highest_5_mean`` of
    notebooks/fig5/fig5_t2d_mash.ipynb:2034-2039 over the seed-ensembled rank tensor, which at 11 607 drugs x 158 outcomes does not
    fit next to its inputs.  ``models`` / ``zs``: the seeds' models and embeddings of the same drugs.  A chunk holds one rank tensor
    per seed, their geometric mean and its ranks within ``max_bytes`` (the note on small chunks in ``highest_outcomes`` applies).
    A pure composition of public functions."""
    models, zs = list(models), list(zs)
    if not models or len(models) != len(zs):
        raise ValueError(f"ensemble_highest_outcomes: {len(models)} models and {len(zs)} embeddings")
    head = _ModelHead(models[0], zs[0])                   # the seeds are ranked one model at a time: the first one's head stands for all
    lo, hi = head.outcomes(label_range)
    N, dev = head.N, head.device
    for m, zz in zip(models, zs):
        if _n_outcomes(m) != head.n_outcomes or zz.shape[0] != N:
            raise ValueError("ensemble_highest_outcomes: every seed needs the same outcomes and the same drugs")
    lab = _kept_labels(keep, head.n_outcomes, lo, hi)
    plane = N * ops.empty_scores(0, N, N, dev).stride(1) * 4 if N else 1
    chunk = max(1, min(max(hi - lo, 1), int(max_bytes) // ((len(models) + 2) * plane)))          # the seeds' ranks, their gmean, its ranks
    state = None
    for s, e, part in _outcome_chunks(lab, lo, hi, chunk):
        ens = ops.ensemble_ranks([rank_all_pairs(m, zz, (s, e)) for m, zz in zip(models, zs)])
        state = ops.outcome_topk(ens, k, labels=part.to(dev), state=state)
        del ens
    return _with_mean(state, k, N, N, dev, True)


def ranks_from_counts(less: torch.Tensor, N: int) -> torch.Tensor:
    """Normalised rank of a pair with ``less`` pairs of its outcome scoring below it, among the N (N - 1) / 2 pairs of N drugs
    -> float32: ``(less + 1) / (N (N - 1) / 2)``, divided in float64 and rounded to float32 once -- the arithmetic of
    notebooks/normalize_scores.py:46-57 (1-based integer rank over a float64 count, stored into a float32 memmap).  A pure
    tensor function (CPU or GPU); the one place that arithmetic is restated."""
    return ((less.to(torch.float64) + 1.0) / (N * (N - 1) / 2)).to(torch.float32)


@torch.no_grad()
def normalized_ranks_of(model, z: torch.Tensor, scores: torch.Tensor, label_range: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The normalised rank of the scores ``scores[l, q]`` within their outcomes -> float32 [L', Q]: the value the reference's
    rank tensor (notebooks/normalize_scores.py:36-74) holds where the pair scoring ``scores[l, q]`` sits, without the [L', N, N]
    score tensor, its sort, or any limit on N: ``ranks_from_counts(count_below(...), N)``.

    Tie rule: for a score value shared by several pairs this is the LOWEST rank of the tie group.  ``ops.rank_normalize`` spreads
    the group over consecutive ranks by its stable tie-break and the reference's order inside a group is arbitrary (argsort is
    not stable there), so tied pairs agree with either only up to the size of their group."""
    return ranks_from_counts(count_below(model, z, scores, label_range), z.shape[0])


@torch.no_grad()
def pair_ranks(model, z: torch.Tensor, heads, tails, label_range: Optional[Tuple[int, int]] = None, max_temp_bytes: int = 1 << 30):
    """Scores and normalised ranks of P given drug pairs -> ``(scores [L', P] fp32, ranks [L', P] fp32)``.  The pair {i, j} is
    scored as ``S[l, max(i, j), min(i, j)]``, the strict-lower-triangle entry the rank normalisation reads (the dense head is not
    bit-symmetric: S[l, i, j] and S[l, j, i] may differ in the last bits); i == j is refused.  This is what turns a
    ``top_partners`` hit list -- whose values are S[l, i, j] with j on either side of i -- into normalised ranks.

    The scores come from the dense general sweep over the rows that occur (``decoder(z[rows].contiguous(), z, ...)``, as
    ``top_pairs`` re-scores its open rows), in row and outcome chunks whose temporaries stay under ``max_temp_bytes``: in "f32" /
    "bf16x3" they are bit for bit what the counting sweep sees.  The ranks are ``normalized_ranks_of`` those scores (its tie rule
    applies).  Multi-GPU: pass the rank's outcome shard as ``label_range``."""
    head = _ModelHead(model, z)
    lo, hi = head.outcomes(label_range)
    N = head.N
    h, t = _index(heads, N, "heads", head.device), _index(tails, N, "tails", head.device)
    if h is None or t is None or h.numel() != t.numel():
        raise ValueError("heads / tails: two index lists of one length")
    if bool((h == t).any()):
        raise ValueError("heads / tails: a drug paired with itself has no rank (the strict lower triangle holds i > j)")
    big, small = torch.maximum(h, t), torch.minimum(h, t)
    P = int(big.numel())
    scores = torch.empty((hi - lo, P), dtype=torch.float32, device=z.device)
    if P and hi > lo:
        rows, where = torch.unique(big, return_inverse=True)            # ascending rows; where[p]: the place of pair p's row
        rb = max(1, min(int(rows.numel()), int(max_temp_bytes) // (N * 4)))
        chunk = max(1, int(max_temp_bytes) // (rb * N * 4))
        for r0 in range(0, int(rows.numel()), rb):
            r1 = min(int(rows.numel()), r0 + rb)
            mine = ((where >= r0) & (where < r1)).nonzero()[:, 0]
            for s in range(lo, hi, chunk):
                e = min(hi, s + chunk)
                dense = head.dense_rows(rows[r0:r1], s, e)
                scores[s - lo:e - lo, mine] = dense[:, where[mine] - r0, small[mine]]
                del dense
    return scores, ranks_from_counts(_count_below(head, scores, (lo, hi), None)[0], N)


@torch.no_grad()
def ensemble_pair_ranks(models, zs, heads, tails, label_range: Optional[Tuple[int, int]] = None, max_temp_bytes: int = 1 << 30):
    """Normalised ranks of P given pairs under K checkpoints and their geometric mean -> ``(per_model [K, L', P], gmean [L', P])``:
    ``pair_ranks`` with every checkpoint's model and embeddings, then ``ops.gmean`` over the K rank matrices (the 5-seed ensembling
    of the normalisation notebook, cell 18).  The notebook's re-ranking of the ensembled tensor (cell 20) ranks the geometric
    means of ALL pairs against each other, which needs every pair's value: out of scope here."""
    K = len(models)
    if not 1 <= K <= 8 or len(zs) != K:
        raise ValueError(f"ensemble_pair_ranks: 1..8 models with one embedding matrix each, got {K} models and {len(zs)} embeddings")
    ranks = [pair_ranks(m, z, heads, tails, label_range, max_temp_bytes)[1] for m, z in zip(models, zs)]
    return torch.stack(ranks), ops.gmean(ranks)


def _ensemble_weight(m) -> torch.Tensor:
    """W_sym [L,128,128] of one checkpoint: a NovelDDIMultilabel, its BilinearDDIScorer, or an original [L,D,D] weight."""
    if isinstance(m, torch.Tensor):
        if m.dim() != 3 or m.shape[1] != m.shape[2]:
            raise ValueError(f"models: a weight must be [L,D,D], got {tuple(m.shape)}")
        return ops.symmetrize(m.detach())
    dec = getattr(m, "decoder", m)
    if not hasattr(dec, "symmetric_weight"):
        raise ValueError(f"models: expected NovelDDIMultilabel, BilinearDDIScorer or an [L,D,D] weight, got {type(m).__name__}")
    return dec.symmetric_weight()


def _index(inds, n: int, name: str, device) -> Optional[torch.Tensor]:
    if inds is None:
        return None
    t = torch.as_tensor(np.asarray(inds, dtype=np.int64) if not isinstance(inds, torch.Tensor) else inds).long().reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise ValueError(f"{name}: indices must lie in [0, {n}), got [{int(t.min())}, {int(t.max())}]")
    return t.to(device)


@torch.no_grad()
def ensemble_all_pairs(models, zs, drug_inds=None, drug_2_inds=None, outcome_inds=None, out=None, host_chunk: int = 16,
                       out_dtype=None):
    """Mean interaction probability over checkpoints for every drug pair: P[o, a, b] = mean_k sigmoid(S_k[outcome_inds[o],
    drug_inds[a], drug_2_inds[b]]) -> [O, A, B] fp32 (or 16-bit: ``out_dtype``), in one sweep of ``ops.bilinear_ensemble_sigmoid``.  Replaces
    get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614), which write K raw-score
    memmaps and stack, sigmoid and average them on the host.

    ``models[k]``: checkpoint k's NovelDDIMultilabel, its BilinearDDIScorer or its original [L,128,128] head weight (symmetrised
    here); ``zs[k]``: checkpoint k's [N,128] embeddings (all_drug_embeddings_full_{epoch}.pt).  ``drug_inds`` / ``drug_2_inds`` /
    ``outcome_inds``: any index lists (unsorted, repeated) -- gathers of z rows and W_sym outcomes before the sweep.
    ``drug_2_inds=None`` is the same drug set on both sides: the symmetric sweep, P[o] exactly symmetric.  Precision follows
    ``models.precision(...)`` as the single-model head does.

    ``out``: None / a CUDA tensor (one launch into HBM) or a numpy array / ``np.memmap`` (outcome chunks of ``host_chunk`` streamed
    through two pinned buffers, as ``score_all_pairs`` does).  Multi-GPU: give each rank its slice of ``outcome_inds``; the slices
    are independent and no collective is involved.

    ``out_dtype`` = ``torch.float16`` / ``torch.bfloat16`` (or an ``out`` of a 16-bit type): the tensor in 16 bits, rounded once inside
    the sweep (``ops.bilinear_ensemble_sigmoid``), bit for bit the fp32 tensor cast afterwards -- half the HBM and, with a host
    destination (a ``np.float16`` array or memmap; numpy has no bfloat16), half the PCIe and disk bytes: the staging buffers and
    copies are 16-bit too."""
    if out_dtype is not None and out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"out_dtype: expected torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    if isinstance(out, torch.Tensor):
        if out_dtype is not None and out.dtype != out_dtype:
            raise ValueError(f"out: dtype {out.dtype} does not match out_dtype {out_dtype}")
    elif out is not None:
        if out_dtype == torch.bfloat16:
            raise ValueError("out_dtype torch.bfloat16 needs an HBM destination: numpy has no bfloat16 (use torch.float16 for a host array / memmap)")
        host_dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}.get(getattr(out, "dtype", None))
        if host_dtype is None:
            raise ValueError("out: expected a CUDA tensor, or a float32 / float16 numpy array or memmap")
        if out_dtype is not None and out_dtype != host_dtype:
            raise ValueError(f"out: dtype {out.dtype} does not match out_dtype {out_dtype}")
    head = _EnsembleHead(models, zs, "ensemble_all_pairs")
    zs, ws, N, dev, prec = head.zs, head.ws, head.N, head.device, head.prec
    oi = _index(outcome_inds, head.n_outcomes, "outcome_inds", dev)
    di = _index(drug_inds, N, "drug_inds", dev)
    d2 = _index(drug_2_inds, N, "drug_2_inds", dev)
    heads = [z if di is None else z.index_select(0, di) for z in zs]
    tails = heads if d2 is None else [z.index_select(0, d2) for z in zs]
    wsel = ws if oi is None else [w.index_select(0, oi) for w in ws]
    L, A, B = wsel[0].shape[0], heads[0].shape[0], tails[0].shape[0]
    if out is None or isinstance(out, torch.Tensor):
        return ops.bilinear_ensemble_sigmoid(heads, tails, wsel, precision=prec, out=out, out_dtype=out_dtype)
    if tuple(out.shape) != (L, A, B):
        raise ValueError(f"out: expected a float32 or float16 array of shape {(L, A, B)}")
    copy_stream = torch.cuda.Stream(device=dev)
    dev_buf = [ops.empty_scores(host_chunk, A, B, dev, dtype=host_dtype) for _ in range(2)]     # row-pitched on the device, compacted by the copy
    pin_buf = [torch.empty((host_chunk, A, B), dtype=host_dtype, pin_memory=True) for _ in range(2)]
    done = [None, None]
    pending = [None, None]
    for k, s in enumerate(range(0, L, host_chunk)):
        e = min(L, s + host_chunk)
        b = k & 1
        if done[b] is not None:                        # staging pair b is free once its last copy has landed
            done[b].synchronize()
            ps, pe = pending[b]
            out[ps:pe] = pin_buf[b][: pe - ps].numpy()
        ops.bilinear_ensemble_sigmoid(heads, tails, [w[s:e] for w in wsel], precision=prec, out=dev_buf[b][: e - s])
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            pin_buf[b][: e - s].copy_(dev_buf[b][: e - s], non_blocking=True)
            done[b] = torch.cuda.Event()
            done[b].record(copy_stream)
        pending[b] = (s, e)
    for b in range(2):
        if done[b] is not None:
            done[b].synchronize()
            ps, pe = pending[b]
            out[ps:pe] = pin_buf[b][: pe - ps].numpy()
    return out


@torch.no_grad()
def ensemble_top_partners(models, zs, k: int, label_range: Optional[Tuple[int, int]] = None, drug_rows=None,
                          max_temp_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """``top_partners`` over a checkpoint ensemble -> ``(vals, idx)`` [L', n, k] (fp32, int32): row i of outcome l holds the k
    largest P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) over j != i and those j, ordered by (P descending, j ascending), padded with
    -inf / -1 -- the partners the five-seed ensemble of get_twosides_scores_wrapper / get_drugbank_scores_wrapper
    (madrigal/evaluate/predict.py:466-499, 582-614) rates highest, without its [L,N,N] tensor (``ops.bilinear_ensemble_topk``).
    The single-model lists cannot be combined into these: the mean of sigmoids is not monotone in any one model's score.

    ``models[m]``: checkpoint m's NovelDDIMultilabel, its BilinearDDIScorer or its original [L,128,128] head weight; ``zs[m]``: its
    [N,128] embeddings of the same drugs.  ``label_range`` slices every checkpoint's W_sym; ``drug_rows``, ``max_temp_bytes`` and
    ``exclude`` as ``top_partners``.  Precision follows ``models.precision(...)``; P is bit for bit the general sweep's of
    ``ops.bilinear_ensemble_sigmoid``."""
    return _top_partners(_EnsembleHead(models, zs, "ensemble_top_partners"), k, label_range, drug_rows, max_temp_bytes, exclude)


@torch.no_grad()
def ensemble_spread_all_pairs(models, zs, label_range: Optional[Tuple[int, int]] = None, kappa=None, out=None):
    """Mean and spread of a checkpoint ensemble for one drug set against itself -> ``(mean, std)``, or ``(mean, std, bound)`` when
    ``kappa`` is given, each [L', N, N] fp32 over the outcomes of ``label_range``: mean and population standard deviation of the K
    probabilities sigmoid(S_m[l, i, j]) and bound = fmaf(kappa, std, mean) (``ops.bilinear_ensemble_spread``).
    get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) keep every
    checkpoint's tensor before they average, so there the spread is ``.std(0)`` of what is stored; here those tensors never exist.

    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``; ``out`` as ``ops.bilinear_ensemble_spread``.  ``mean`` is bit
    for bit the general sweep's of ``ops.bilinear_ensemble_sigmoid``: (z_i W) z_j, not mirrored, so it is symmetric only up to
    rounding.  Precision follows ``models.precision(...)``."""
    head = _EnsembleHead(models, zs, "ensemble_spread_all_pairs")
    lo, hi = head.outcomes(label_range)
    return ops.bilinear_ensemble_spread(head.zs, head.zs, head.w(lo, hi), kappa=kappa, precision=head.prec, out=out)


@torch.no_grad()
def ensemble_confident_partners(models, zs, k: int, kappa=-1.0, label_range: Optional[Tuple[int, int]] = None, drug_rows=None,
                                eligible: str = "not_self", exclude: Optional[torch.Tensor] = None):
    """``ensemble_top_partners`` under a confidence bound -> ``(bound, partner, mean, std)``, each [L', rows, k] (fp32, int32, fp32,
    fp32): row i of outcome l holds the k eligible partners j with the largest bound = fmaf(kappa, std, mean) -- mean and std over
    the K checkpoints' probabilities sigmoid(S_m[l, i, j]) -- ordered by (bound descending, j ascending), with each partner's own
    mean and std, padded with -inf / -1 / NaN / NaN (``ops.bilinear_ensemble_spread_topk``).  The default ``kappa = -1`` ranks by
    mean - std: partners the seeds agree on, which a list ranked by the mean cannot tell from two seeds at 1.0 and three at 0.88;
    ``kappa > 0`` lists contested pairs, ``kappa = 0`` is ``ensemble_top_partners`` bit for bit.  Nothing of [L', N, N] and none of
    the per-checkpoint tensors of madrigal/evaluate/predict.py:466-499, 582-614 is materialised.

    ``models`` / ``zs`` / ``label_range`` / ``drug_rows`` / ``exclude`` as ``ensemble_top_partners``; ``eligible``: "not_self"
    (j != i), "lower" (j < i) or "all"."""
    head = _EnsembleHead(models, zs, "ensemble_confident_partners")
    lo, hi = head.outcomes(label_range)
    rows = _index(drug_rows, head.N, "drug_rows", head.device)
    excl = head.exclusion(exclude)
    res = ops.bilinear_ensemble_spread_topk(head.zs, head.zs, head.w(lo, hi), k, kappa, eligible=eligible, precision=head.prec,
                                            exclude=_planes(excl, lo, hi))
    return res if rows is None else tuple(t[:, rows] for t in res)


@torch.no_grad()
def ensemble_top_pairs(models, zs, K: int, label_range: Optional[Tuple[int, int]] = None, k_row: Optional[int] = None,
                       max_temp_bytes: int = 1 << 30, info: Optional[dict] = None, exclude: Optional[torch.Tensor] = None):
    """``top_pairs`` over a checkpoint ensemble -> ``(vals [L', K] fp32, head [L', K], tail [L', K] int64)``: the ``K`` unordered
    drug pairs with the highest mean probability P[l, i, j] = mean_m sigmoid(S_m[l, i, j]), i > j, ordered by (P descending, i
    ascending, j ascending), padded with -inf / -1.  Exact for every K and without the [L', N, N] tensor: the lower-triangle lists of
    ``ops.bilinear_ensemble_topk`` (``k_row`` per row, default min(K, 16)), the K best candidates, and the open rows re-scored with
    ``ops.bilinear_ensemble_sigmoid`` over those rows -- a row subset is not the tail object, so the general sweep runs and the
    re-scored probabilities are bit for bit what the lists saw -- merged by ``merge_row_candidates``.  Probabilities tie often (many
    round to exactly 1), so open rows are common with a small ``k_row``; the result stays exact.
    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``; ``max_temp_bytes``, ``info`` and ``exclude`` as ``top_pairs``."""
    return _top_pairs(_EnsembleHead(models, zs, "ensemble_top_pairs"), K, label_range, k_row, max_temp_bytes, info, exclude)


@torch.no_grad()
def ensemble_partner_counts(models, zs, thresholds, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 1 << 30,
                            exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``partner_counts`` over a checkpoint ensemble -> int32 [L', N]: ``counts[l, i]`` = #{j != i : P[l, i, j] >= thresholds[l]},
    P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) -- the degree of drug i in the network the ensemble of get_twosides_scores_wrapper /
    get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) predicts for outcome l, counted inside the sweep
    (``ops.bilinear_ensemble_select_count``, ``not_self`` mode): no [L', N, N] tensor at any N.

    ``thresholds``: a PROBABILITY cut, a number such as 0.9 or [L'] (no NaN), e.g. ``ensemble_top_pairs(models, zs, K)[0][:, -1]``;
    the rule is ``>=``, so ties with the K-th pair are counted, and at saturated inputs many probabilities are exactly 1.0.  A cut on
    the ensemble's probability needs no calibration per outcome, unlike a cut on one model's logit.  Normalised ranks under the
    ensemble: ``ensemble_normalized_ranks_of``.  ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``; ``exclude`` as
    ``partner_counts``; ``max_bytes`` is accepted for symmetry with ``ensemble_partners_above`` (the result is 4 L' N bytes)."""
    return _partner_counts(_EnsembleHead(models, zs, "ensemble_partner_counts"), thresholds, label_range, exclude)


@torch.no_grad()
def ensemble_partners_above(models, zs, thresholds, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 1 << 30,
                            exclude: Optional[torch.Tensor] = None):
    """``partners_above`` over a checkpoint ensemble, as CSR -> ``(row_ptr int64 [L' * N + 1], cols int32 [T], vals fp32 [T])``: row
    ``l * N + i`` lists ALL j != i with P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) >= thresholds[l] in ascending order and those
    probabilities (``ops.bilinear_ensemble_select``, ``not_self`` mode; ``csr_rows(row_ptr, N)`` gives every entry's outcome and
    drug).  Where ``ensemble_top_partners`` returns at most 32 partners of a drug, this returns its whole neighbourhood -- a hub has
    hundreds; every unordered pair appears from both sides, with P[l, i, j] and P[l, j, i] (equal up to the last bits).  More than
    ``max_bytes`` (8 bytes per entry) raises a ValueError naming the size before anything is allocated.

    ``thresholds``: a PROBABILITY cut, a number such as 0.9 or [L'] (no NaN), e.g. ``ensemble_top_pairs(models, zs, K)[0][:, -1]``;
    the rule is ``>=``, so ties with the K-th pair are included, and at saturated inputs many probabilities are exactly 1.0.
    Normalised ranks under the ensemble: ``ensemble_normalized_ranks_of``.  ``models`` / ``zs`` / ``label_range`` as
    ``ensemble_top_partners``; ``exclude`` as ``partners_above``."""
    return _select_above(_EnsembleHead(models, zs, "ensemble_partners_above"), thresholds, label_range, "not_self", max_bytes, exclude)


@torch.no_grad()
def ensemble_pairs_above(models, zs, thresholds, label_range: Optional[Tuple[int, int]] = None, max_bytes: int = 1 << 30,
                         exclude: Optional[torch.Tensor] = None):
    """``pairs_above`` over a checkpoint ensemble -- "every pair the five-seed ensemble calls an interaction with P >= 0.9", the
    outcome's predicted network -- -> ``(offsets int64 [L' + 1], head int64 [T], tail int64 [T], vals fp32 [T])``: outcome l owns the
    entries ``offsets[l]:offsets[l + 1]``.  The pair {i, j} is rated P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) with i > j, the
    strict-lower-triangle entry ``ensemble_top_pairs`` uses, and is selected when that probability is ``>= thresholds[l]``; the
    entries are ordered by (outcome, head, tail) ascending.  Nothing of [L', N, N] is materialised (``ops.bilinear_ensemble_select``,
    ``lower`` mode: a counting and a filling sweep); ``head`` is expanded from the sweep's row pointers (``csr_rows``).  The mean of
    sigmoids is not monotone in any one model's score, so no union or intersection of ``pairs_above`` per checkpoint gives this set.
    More than ``max_bytes`` (8 bytes per pair in the sweep's result) raises a ValueError naming the size.

    Where a cut comes from (``thresholds``: a PROBABILITY, a number or [L'], no NaN):
      * a number such as 0.9: the same cut means the same thing for every outcome, no calibration per outcome;
      * the K-th value of ``ensemble_top_pairs``: ``ensemble_pairs_above(models, zs, ensemble_top_pairs(models, zs, K)[0][:, -1])``
        holds those K pairs and every pair tied with the last of them (the rule is ``>=``).  At saturated inputs many probabilities
        are exactly 1.0, so such a tie set can be large: ``max_bytes`` bounds it.
    The returned probabilities can go straight into ``ensemble_normalized_ranks_of`` (``normalized_ranks_of`` ranks one model's scores).
    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``; ``exclude`` as ``pairs_above``."""
    return _pairs_above(_EnsembleHead(models, zs, "ensemble_pairs_above"), thresholds, label_range, max_bytes, exclude)


@torch.no_grad()
def ensemble_score_histogram(models, zs, edges: torch.Tensor, label_range: Optional[Tuple[int, int]] = None, eligible: str = "lower",
                             known: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``score_histogram`` over a checkpoint ensemble -> int64 [L', B+1]: ``counts[l, b]`` is the number of eligible pairs whose
    mean probability P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) -- the value get_twosides_scores_wrapper / get_drugbank_scores_wrapper
    (madrigal/evaluate/predict.py:466-499, 582-614) predict from -- lies in ``[edges[l, b-1], edges[l, b])`` (-inf below the first
    edge, +inf above the last), counted inside the ensemble's sweep (``ops.bilinear_ensemble_bincount``): no [L', N, N] tensor at any
    N.  ``edges``: ``[B]`` shared by all outcomes or ``[L', B]``, fp32 PROBABILITIES, finite and ascending, 1 <= B <=
    ``ops.bilinear_bincount_max_edges()``; ``eligible`` as ``score_histogram``.  Cumulative sums of a row are the distribution
    function of the outcome's probabilities at the edges, from which quantiles follow.  Saturated probabilities tie exactly (many
    are exactly 1.0): an edge at 1.0 puts that whole tie group into the last bin.
    ``known``: a ``known_pairs_mask`` -> int64 [2, L', B+1]: the novel pairs (``[0]``) and the known pairs (``[1]``) counted
    separately in the same sweep; ``result.sum(0)`` is the histogram without ``known``.
    Edges taken from ``ensemble_top_pairs`` / ``ensemble_pairs_above`` can be fed straight in (the same arithmetic, bit for bit): the
    cumulative counts below such an edge are that pair's rank, the lowest of its tie group (``ensemble_normalized_ranks_of``; not
    ``ensemble_pair_ranks``, which is the geometric mean of per-model ranks).
    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``.  Multi-GPU: pass the rank's outcome shard as ``label_range``."""
    return _score_histogram(_EnsembleHead(models, zs, "ensemble_score_histogram"), edges, label_range, eligible, known)


@torch.no_grad()
def ensemble_count_below(models, zs, probs: torch.Tensor, label_range: Optional[Tuple[int, int]] = None,
                         known: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``count_below`` over a checkpoint ensemble -> int64 [L', Q]: for every query ``probs[l, q]`` the number of
    strict-lower-triangle pairs (i > j) of outcome l whose mean probability P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) is strictly
    less.  Any Q; the queries may be unsorted and repeated: per outcome they are sorted and deduplicated and the counting sweep
    (``ops.bilinear_ensemble_bincount``, lower-triangle mode) runs once per chunk of at most ``ops.bilinear_bincount_max_edges()``
    distinct values, exactly as ``count_below`` does around the single-model sweep.  Strictly less: a query that ties with many
    pairs -- saturated probabilities are exactly 1.0 -- counts none of its tie group.
    The probabilities ``ensemble_top_pairs`` / ``ensemble_pairs_above`` return can be fed straight in: they come from the same
    arithmetic, bit for bit, so a pair is never counted below itself.  The counts are over the MEAN probability; ``ensemble_pair_ranks``
    is a different quantity, the geometric mean of every checkpoint's own rank of the pair.
    ``known``: a ``known_pairs_mask`` -> int64 [2, L', Q]: the novel (``[0]``) and the known pairs (``[1]``) below every query.
    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``."""
    return _count_below(_EnsembleHead(models, zs, "ensemble_count_below"), probs, label_range, known)[0]


@torch.no_grad()
def ensemble_normalized_ranks_of(models, zs, probs: torch.Tensor, label_range: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The normalised rank of the ensemble probabilities ``probs[l, q]`` within their outcomes -> float32 [L', Q]: where a pair with
    mean probability ``probs[l, q]`` sits among all N (N - 1) / 2 pairs ranked by P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) -- the
    value notebooks/normalize_scores.py:36-74 computes from the stored ensemble tensor -- without that tensor or its sort:
    ``ranks_from_counts(ensemble_count_below(...), N)``.

    Tie rule: for a probability shared by several pairs this is the LOWEST rank of the tie group, and exact ties are the rule for
    saturated probabilities (at N(0,1) inputs about 7 % of one model's probabilities are exactly 1.0): all of them get the rank of
    the first of them.
    This is NOT ``ensemble_pair_ranks``: that is the geometric mean of every checkpoint's own rank of the pair; this is the rank of
    the mean probability.  The two orderings differ, because the mean of sigmoids is not monotone in any one model's score.
    The values ``ensemble_top_pairs`` / ``ensemble_pairs_above`` return can be fed straight in (the same arithmetic, bit for bit)."""
    zs = list(zs)
    less = ensemble_count_below(models, zs, probs, label_range)
    return ranks_from_counts(less, zs[0].shape[0])


@torch.no_grad()
def ensemble_recovery_at_cuts(models, zs, known: torch.Tensor, cuts: torch.Tensor, label_range: Optional[Tuple[int, int]] = None) -> dict:
    """``recovery_at_cuts`` over a checkpoint ensemble -> the dict of ``recovery_from_counts``, every entry [L', B]: for each
    PROBABILITY cut ``cuts[l, b]`` (any order, repeats allowed) the strict-lower-triangle pairs the ensemble rates at or above it
    (``selected``, P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) >= cut), the known ones among them (``hits``) and the exact precision,
    recall and enrichment over all N (N - 1) / 2 pairs, with no [L', N, N] tensor.  ``known``: a ``known_pairs_mask``; the class
    sizes are read from the same sweeps.  The rule is ``>=`` and ties are exact: a cut at 1.0 selects the whole saturated tie group.
    Cuts taken from ``ensemble_top_pairs`` / ``ensemble_pairs_above`` can be fed straight in (the same arithmetic, bit for bit)."""
    return _recovery_at_cuts(_EnsembleHead(models, zs, "ensemble_recovery_at_cuts"), known, cuts, label_range)


@torch.no_grad()
def ensemble_auroc_bounds(models, zs, known: torch.Tensor, edges: torch.Tensor, label_range: Optional[Tuple[int, int]] = None):
    """``auroc_bounds`` over a checkpoint ensemble -> ``(lower, upper)`` float64 [L']: bounds on the AUROC of ranking ALL
    strict-lower-triangle pairs by the mean probability P[l, i, j] = mean_m sigmoid(S_m[l, i, j]) against the known network:
    ``ensemble_score_histogram(known=)`` followed by ``auroc_bounds_from_counts`` -- one sweep, no sampled negatives.  Pairs that
    share a bin count towards the gap between the bounds; exactly tied probabilities (the saturated group at 1.0) share a bin
    whatever the edges, and the exact AUROC counts them 1/2, inside the interval."""
    return _auroc_bounds(_EnsembleHead(models, zs, "ensemble_auroc_bounds"), known, edges, label_range)


# ---- per-pair outcome profiles of the checkpoint ensemble (ops.bilinear_ensemble_profile) ----
@torch.no_grad()
def ensemble_outcome_profile(models, zs, thresholds, scale=None, label_range: Optional[Tuple[int, int]] = None,
                             eligible: str = "not_self", head_rows: Optional[Tuple[int, int]] = None, chunk: int = PROFILE_CHUNK,
                             exclude: Optional[torch.Tensor] = None):
    """``outcome_profile`` over a checkpoint ensemble -> ``(count int32, best int64, margin fp32)``, each [N, N] (or [r1 - r0, N]
    with ``head_rows``): for the pair (i, j), over the outcomes ``label_range`` (default: all), with P[l, i, j] = mean_m
    sigmoid(S_m[l, i, j]), ``count`` is the number of outcomes with P[l, i, j] >= thresholds[l] -- for how many interaction types
    the ensemble of get_twosides_scores_wrapper / get_drugbank_scores_wrapper (madrigal/evaluate/predict.py:466-499, 582-614) flags
    the pair --, ``margin`` the largest ``(P[l, i, j] - thresholds[l]) * scale[l]`` and ``best`` the MODELS' index of the lowest
    outcome attaining it (-1 where no outcome moved the pair off -inf; ties are common, many probabilities round to exactly 1).
    Nothing of [L', N, N] is materialised (``ops.bilinear_ensemble_profile``: one sweep per ``chunk`` <= 65535 outcomes, merged with
    ``ops.profile_merge``).  The single-model profiles cannot be combined into this: the mean of sigmoids is not monotone in any one
    model's score.

    ``thresholds``: a PROBABILITY cut, a number such as 0.9 or [L'] (no NaN) -- it needs no calibration per outcome; ``scale``:
    None, a positive number or [L'].  ``eligible`` and ``head_rows`` as ``outcome_profile``.  ``exclude``: ONE shared plane from
    ``known_pairs_mask`` (no ``labels``); its pairs are blanked to 0 / -1 / -inf like ineligible ones (a plane per outcome is
    refused: it would change the counts inside the sweep).  ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``."""
    return _outcome_profile(_EnsembleHead(models, zs, "ensemble_outcome_profile"), thresholds, scale, label_range, eligible, head_rows, chunk, exclude)


@torch.no_grad()
def ensemble_most_flagged_pairs(models, zs, thresholds, K: int, scale=None, label_range: Optional[Tuple[int, int]] = None,
                                max_bytes: int = 1 << 30, exclude: Optional[torch.Tensor] = None):
    """``most_flagged_pairs`` over a checkpoint ensemble -> ``(count int32 [K], head int64 [K], tail int64 [K], best int64 [K],
    margin fp32 [K])``: the ``K`` unordered drug pairs {i, j}, i > j, the ensemble flags for the most outcomes at the probability
    cut ``thresholds`` (e.g. 0.9), ordered by (count descending, margin descending, i ascending, j ascending); ``count``, ``best``
    and ``margin`` are those of ``ensemble_outcome_profile``.  Padding, the row-block streaming under ``max_bytes`` and the exact
    tie rule at the K-th place are ``most_flagged_pairs``'s (one shared walk); no [N, N] and no [L', N, N] tensor, so it runs at
    any N.  ``exclude``: ONE shared plane from ``known_pairs_mask``; its pairs are left out of the ranking (novel pairs only).
    ``models`` / ``zs`` / ``label_range`` as ``ensemble_top_partners``."""
    return _most_flagged_pairs(_EnsembleHead(models, zs, "ensemble_most_flagged_pairs"), thresholds, K, scale, label_range, max_bytes, exclude)
