"""Classification metrics of labelled DDI triples (madrigal/evaluate/metrics.py).

``get_metrics`` is the drop-in for the reference's ``get_metrics`` (metrics.py:129-191): the 13 metrics of
``get_metrics_binary`` (metrics.py:60-118) for every outcome in one call of ``ops.label_metrics`` (csrc/eval_metrics.hip),
then the reference's averaging on the host over [13, L] numbers.
``average_precision`` / ``macro_auprc`` are the earlier acceptance check of the path: AUPRC alone with torch sorts and
prefix sums, kept as an independent statement of the same quantity; sklearn is the checker in tests/."""
from __future__ import annotations

from typing import Any, Optional, Tuple

import numpy as np
import torch


def average_precision(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """sklearn.metrics.average_precision_score(target, pred) for one binary problem: sum over the DISTINCT thresholds of
    (recall_k - recall_{k-1}) * precision_k, scores sorted descending.  Returns a 0-dim float64 tensor (NaN without positives)."""
    if pred.shape != target.shape or pred.dim() != 1:
        raise ValueError("average_precision: 1-D pred / target of the same length")
    order = torch.argsort(pred, descending=True, stable=True)
    p, y = pred[order], target[order].to(torch.float64)
    tp = torch.cumsum(y, 0)
    n_pos = tp[-1] if y.numel() else torch.zeros((), dtype=torch.float64, device=pred.device)
    last = torch.ones_like(p, dtype=torch.bool)                 # last element of each run of equal scores = one threshold
    if p.numel() > 1:
        last[:-1] = p[1:] != p[:-1]
    tp_k = tp[last]
    k = torch.nonzero(last).flatten().to(torch.float64) + 1.0
    precision = tp_k / k
    recall = tp_k / n_pos
    prev = torch.cat([torch.zeros(1, dtype=torch.float64, device=pred.device), recall[:-1]])
    return ((recall - prev) * precision).sum()


def macro_auprc(pred: torch.Tensor, target: torch.Tensor, labels: torch.Tensor, n_labels: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-outcome AUPRC of labelled samples (pred / target / labels all [T]) and its mean over the outcomes that have
    both classes (get_metrics, metrics.py:129-191) -> (macro, per_label [L] with NaN where undefined)."""
    L = int(labels.max().item()) + 1 if n_labels is None else n_labels
    out = torch.full((L,), float("nan"), dtype=torch.float64, device=pred.device)
    order = torch.argsort(labels, stable=True)
    ls, ps, ys = labels[order], pred[order], target[order]
    counts = torch.bincount(ls, minlength=L)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=pred.device), torch.cumsum(counts, 0)]).tolist()
    for l in range(L):
        lo, hi = ptr[l], ptr[l + 1]
        if hi > lo:
            y = ys[lo:hi]
            s = float(y.sum())
            if 0 < s < hi - lo:
                out[l] = average_precision(ps[lo:hi], y)
    return torch.nanmean(out), out


_AVERAGES = (None, "macro", "weighted", "micro")
_TASKS = ("binary", "multilabel", "multiclass")


def _metric_names(k_name) -> tuple:
    return ("fmax", "mcc", "auroc", "auprc", "npv", "specificity", "f1", f"recall@{k_name}", f"precision@{k_name}", f"ap@{k_name}",
            "accuracy", "precision", "recall")


def _print_metrics(names, vals, logger):
    line = ", ".join(f"{n} = {v:.4f}" for n, v in zip(names, vals))
    if logger is None:
        print(line)
    else:
        logger.info(line)


def get_metrics(preds, ys, labels, k=50, task: str = "multilabel", logger: Any = None, average: Optional[str] = "macro",
                verbose: bool = True):
    """madrigal/evaluate/metrics.py:get_metrics on the device -> (metrics dict with the reference's keys in order, pos_samples).

    preds / ys / labels: numpy arrays or CUDA tensors of T triples (numpy input goes to the current device); preds are
    probabilities (predicted positive <=> pred > 0.5, np.round's rule on [0, 1]).  ``task="binary"`` and ``average="micro"`` score
    all triples as one problem; otherwise each label present is one problem and ``average`` is "macro" (plain mean: NaN
    propagates), "weighted" (by positives) or None (arrays over the labels present, ascending).  Values are numpy float64.

    Mirrored quirks of the reference: with a fractional k the names ``recall@{k}`` etc. carry the resolved k of the LAST label
    present (its loop leaves the last label's names); a problem whose targets and rounded preds are all one class raises
    ValueError (the reference's ``confusion_matrix(...).ravel()`` unpack fails there), as does a pred that rounds outside {0, 1}.
    Top-k ties are broken by reverse original order (np.argsort(pred, kind="stable")[::-1]), where the reference's unstable
    argsort leaves them arbitrary."""
    from . import ops
    if average not in _AVERAGES:
        raise ValueError(f"average must be one of {_AVERAGES}, got {average!r}")
    if task not in _TASKS:
        raise ValueError(f"task must be one of {_TASKS}, got {task!r}")
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise ValueError(f"k must be an int or a float in (0, 1), got {k!r}")
    if isinstance(k, (float, np.floating)):
        if not 0.0 < float(k) < 1.0:
            raise ValueError(f"a float k must lie in (0, 1), got {k}")
        k = float(k)
    else:
        k = int(k)
        if k <= 0:
            raise ValueError(f"k must be positive, got {k}")
    n = len(preds)
    if len(ys) != n or len(labels) != n or n == 0:
        raise ValueError(f"preds, ys and labels must be non-empty and of one length (got {n}, {len(ys)}, {len(labels)})")
    ys_dtype = ys.dtype if isinstance(ys, np.ndarray) else torch.empty(0, dtype=ys.dtype).numpy().dtype

    def dev(x, dtype):
        if isinstance(x, torch.Tensor):
            if not x.is_cuda:
                raise ValueError("get_metrics: tensors must live on the GPU (or pass numpy arrays)")
            return x.reshape(-1).to(dtype)
        return torch.as_tensor(np.ascontiguousarray(x).reshape(-1)).to(device=torch.device("cuda", torch.cuda.current_device()), dtype=dtype)

    pred, tgt = dev(preds, torch.float32), dev(ys, torch.float32)
    lab = dev(labels, torch.int64)
    if pred.device != tgt.device or pred.device != lab.device:
        raise ValueError("get_metrics: preds, ys and labels must be on one device")
    single = task == "binary" or average == "micro"
    micro_pos = None
    if single:
        if task != "binary":                                            # micro: pos_samples stay per label
            if int(lab.min()) < 0:
                raise ValueError("labels must be non-negative")
            cnt = torch.bincount(lab)
            micro_pos = torch.bincount(lab, weights=tgt.double())[cnt > 0].cpu().numpy()
        lab, L = torch.zeros_like(lab), 1
    else:
        lo_hi = torch.stack([lab.min(), lab.max()]).tolist()
        if lo_hi[0] < 0:
            raise ValueError(f"labels must be non-negative, got {lo_hi[0]}")
        L = lo_hi[1] + 1
    p_lo, p_hi = torch.aminmax(pred)
    r = ops.label_metrics(pred, tgt, lab, L, k=k, threshold=0.5)
    if not (float(p_lo) >= -0.5 and float(p_hi) < 1.5):
        raise ValueError("get_metrics: a pred rounds outside {0, 1} (the reference's confusion_matrix unpack fails)")
    values, count, pos, k_eff = (r[x].cpu().numpy() for x in ("values", "count", "pos", "k_eff"))
    present = np.flatnonzero(count > 0)
    one_class = ((pos[present] == 0) | (pos[present] == count[present])) & (values[10, present] == 1.0)
    if one_class.any():
        raise ValueError(f"label {int(present[np.argmax(one_class)])}: targets and rounded preds are all one class "
                         "(the reference's confusion_matrix(...).ravel() unpack fails)")
    k_name = int(k_eff[present[-1]]) if isinstance(k, float) else k
    names = _metric_names(k_name)
    if single:
        vals = values[:, 0]
        pos_samples = ys_dtype.type(pos[0]) if task == "binary" else micro_pos.astype(ys_dtype)
        if task == "binary":
            if verbose:
                _print_metrics(names, vals, logger)
            return dict(zip(names, vals)), pos_samples
    else:
        per = np.ascontiguousarray(values[:, present].T)                # [n_present, 13], as the reference stacks its rows
        pos_samples = pos[present].astype(ys_dtype)
        if average == "macro":
            vals = per.mean(axis=0)
        elif average == "weighted":
            vals = per.T @ pos_samples / pos_samples.sum()
        else:
            vals = per.T
    if verbose and average is not None:
        _print_metrics(names, vals, logger)
    return dict(zip(names, vals)), pos_samples


_DRUG_MODES = ("test_between", "test_between_train")


def drug_specific_metrics(preds, heads, tails, labels, pos_neg, n_head: int, mode: str = "test_between"):
    """The metric part of madrigal/evaluate/predict.py:get_drug_specific_scores on the device -> (metrics, owners): ``metrics`` maps
    the reference's names (k = 50, get_metrics order) to one np.float64 per drug of interest; ``owners`` (int64 numpy) are the
    drugs' indices, all head indices (``test_between``) or the sorted tail indices of the positives (``test_between_train``).

    preds: probabilities, and heads / tails / labels / pos_neg: the labelled triples, all CUDA tensors of one length T, in the
    collator's val/test layout: positive i owns the negatives i and i + n_pos of the negative list (each keeps its own label).  A
    drug's problems are its (drug, label) groups of positives, first negatives and second negatives, each macro-averaged over
    labels with NaN propagating, as get_metrics(task="multiclass", average="macro", k=50) does per drug; one
    ``ops.group_metrics`` call computes all of them (group id = owner rank * L + label, L = labels.max() + 1).
    Raises ValueError where the reference fails: fewer than 2 * n_pos negatives (an IndexError there), a drug of interest
    without positives, or a (drug, label) problem whose targets and rounded preds are all one class."""
    from . import ops
    if mode not in _DRUG_MODES:
        raise NotImplementedError(f"drug_specific_metrics: mode must be one of {_DRUG_MODES}, got {mode!r}")
    ts = (preds, heads, tails, labels, pos_neg)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise ValueError("drug_specific_metrics: preds, heads, tails, labels and pos_neg must be CUDA tensors")
    T = int(preds.numel())
    if any(int(t.numel()) != T for t in ts) or T == 0:
        raise ValueError("drug_specific_metrics: preds, heads, tails, labels and pos_neg must be non-empty and of one length")
    dev = preds.device
    n_head = int(n_head)
    is_pos = pos_neg.reshape(-1).bool()
    pos_idx, neg_idx = torch.nonzero(is_pos).flatten(), torch.nonzero(~is_pos).flatten()
    heads, tails, labels = (t.reshape(-1).to(torch.int64) for t in (heads, tails, labels))
    owner = (heads if mode == "test_between" else tails)[pos_idx]
    n_pos, n_neg = int(pos_idx.numel()), int(neg_idx.numel())
    l_hi = int(labels.max()) if T else 0
    L = l_hi + 1
    if mode == "test_between":
        drugs = np.arange(n_head, dtype=np.int64)
        if n_pos and not bool(((owner >= 0) & (owner < n_head)).all()):
            raise ValueError(f"drug_specific_metrics: a positive's head index lies outside [0, {n_head})")
        rank = owner
    else:
        uniq, rank = torch.unique(owner, sorted=True, return_inverse=True)
        drugs = uniq.cpu().numpy().astype(np.int64)
    n_drugs = int(drugs.size)
    if n_pos == 0:
        if mode == "test_between_train":                              # no drug of interest: the reference's loop runs zero times
            return {}, drugs
        raise ValueError(f"drug {int(drugs[0]) if n_drugs else 0}: no positive triples (the reference's confusion_matrix(...).ravel() "
                         "unpack fails on the empty problem)")
    if n_neg < 2 * n_pos:                                             # the reference's negative gather runs off the end
        short = rank[n_neg - n_pos:] if n_neg >= n_pos else rank
        first = int(short.min())
        raise ValueError(f"drug {int(drugs[first])}: its positives lack negatives ({n_neg} negatives for {n_pos} positives; "
                         "the collator's layout has 2 per positive)")
    if n_drugs * L > 2 ** 31:
        raise ValueError(f"drug_specific_metrics: {n_drugs} drugs x {L} labels exceed 2^31 (drug, label) groups")
    order = torch.cat([pos_idx, neg_idx[:2 * n_pos]])                 # positives, negative block 1, negative block 2
    pred = preds.reshape(-1)[order].to(torch.float32)
    target = torch.cat([torch.ones(n_pos, device=dev), torch.zeros(2 * n_pos, device=dev)])
    group = rank.repeat(3) * L + labels[order]
    r = ops.group_metrics(pred, target, group, n_drugs * L, k=50, threshold=0.5, inner=L)
    n_groups = r["outer_groups"].cpu().numpy()
    gid, pos, cnt = (r[x].cpu().numpy() for x in ("group_id", "pos", "count"))
    acc = r["values"][10].cpu().numpy()
    one_class = ((pos == 0) | (pos == cnt)) & (acc == 1.0)
    bad_drug = np.flatnonzero(n_groups == 0)
    first_empty = int(bad_drug[0]) if bad_drug.size else n_drugs
    first_one = int(gid[np.argmax(one_class)] // L) if one_class.any() else n_drugs
    if first_empty < n_drugs and first_empty <= first_one:
        raise ValueError(f"drug {int(drugs[first_empty])}: no positive triples (the reference's confusion_matrix(...).ravel() "
                         "unpack fails on the empty problem)")
    if first_one < n_drugs:
        j = int(np.argmax(one_class))
        raise ValueError(f"drug {int(drugs[first_one])}, label {int(gid[j] % L)}: targets and rounded preds are all one class "
                         "(the reference's confusion_matrix(...).ravel() unpack fails)")
    vals = r["outer_values"].cpu().numpy()
    names = _metric_names(50)
    return {nm: [np.float64(v) for v in vals[m]] for m, nm in enumerate(names)}, drugs
