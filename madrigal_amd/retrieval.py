"""Pretraining retrieval metrics on the device: drop-ins for madrigal/evaluate/eval_utils.py:147-156 (uniform_loss,
alignment_loss), :232-247 (foscttm) and madrigal/evaluate/evaluate.py:406-450 (get_inst_dist_topk_accuracy, with the stacked
top-k of eval_utils.py:159-174).

The reference builds an n x n cosine matrix and a [2n, 2n-1] stacked one on the CPU and calls ``torch.topk``, loops over rows in
Python for FOSCTTM and runs ``torch.pdist`` for uniformity.  Here one sweep (``ops.pair_match_counts``, csrc/retrieval.hip) counts,
for every row and column, the competitors that beat the true match; top-k accuracy at any k is the share of counts below k.
``ops.pair_uniformity`` is the upper triangle of X^ X^T with an exp-sum epilogue.

Ties: a competitor exactly as close as the true match does not count against it ("ties count as hits").  ``torch.topk`` breaks
such ties in an unspecified order; they do not arise with real-valued embeddings.  The accuracies are computed in fp32 with the
reference's own expressions, so they equal its numbers exactly whenever the counts agree.

CPU tensors are moved to the current CUDA device (as ``metrics.get_metrics`` does with numpy input)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

STACKED_TOPK = (1, 5, 20)       # stacked_inst_dist_topk_accuracy's default topk


def _dev(x) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    return x if x.is_cuda else x.to(torch.device("cuda", torch.cuda.current_device()))


def _need_k(k: int, n: int, what: str) -> None:
    if k > n:
        raise ValueError(f"{what}: top-{k} needs at least {k} candidates per row, got {n} (torch.topk raises here)")


def topk_fraction(hits: torch.Tensor, total: int) -> torch.Tensor:
    """hits / total as the reference forms it on the CPU: an fp32 sum divided by an int, correctly rounded in fp32.  The divisor
    is a tensor: on the GPU, division by a Python scalar multiplies by its reciprocal, which can round the other way."""
    return hits.to(torch.float32) / torch.tensor(float(total), dtype=torch.float32, device=hits.device)


def pair_counts(embeds1, embeds2) -> dict:
    """``ops.pair_match_counts`` on device copies of the two views (see there for the definitions)."""
    return ops.pair_match_counts(_dev(embeds1), _dev(embeds2))


def topk_from_counts(counts: dict, ks) -> dict:
    """One-side and stacked top-k accuracies of counts from ``pair_counts`` -> {('one', k) | ('both', k): 0-dim fp32 device
    tensor}.  One-side (get_inst_dist_topk_accuracy's ``topk_acc``): 1 - misses / 2n over rows and columns.  Stacked: the true
    match of drug i's view in X ranks cos_row[i] + same_x[i] among the 2n - 1 others, in Y cos_col[i] + same_y[i]; hits / 2n."""
    n = int(counts["cos_row"].numel())
    out = {}
    for kind, k in ks:
        if kind == "one":
            _need_k(k, n, "get_inst_dist_topk_accuracy")
            miss = (counts["cos_row"] >= k).sum() + (counts["cos_col"] >= k).sum()
            out[(kind, k)] = 1 - topk_fraction(miss, 2 * n)
        else:
            _need_k(max(STACKED_TOPK), 2 * n - 1, "stacked_inst_dist_topk_accuracy")
            hit = ((counts["cos_row"] + counts["same_x"]) < k).sum() + ((counts["cos_col"] + counts["same_y"]) < k).sum()
            out[(kind, k)] = topk_fraction(hit, 2 * n)
    return out


def get_inst_dist_topk_accuracy(embeds1, embeds2, k: int, metric: str = "cosine"):
    """evaluate.py:406-450 -> ``(topk_acc, top20, top5, top1, None, None)`` as Python floats.  The reference's last two values
    are the top-k index tensors of the rows and columns; its only caller discards them, and producing them would need a real
    top-k, so they are None here.  ``metric='euclidean'`` raises NotImplementedError (no caller uses it); k > n raises
    ValueError where ``torch.topk`` raises."""
    if metric == "euclidean":
        raise NotImplementedError("get_inst_dist_topk_accuracy: metric='euclidean' is not implemented on the HIP path")
    if metric != "cosine":
        raise NotImplementedError(f"get_inst_dist_topk_accuracy: unknown metric {metric!r}")
    counts = pair_counts(embeds1, embeds2)
    acc = topk_from_counts(counts, [("one", int(k))] + [("both", kk) for kk in (20, 5, 1)])
    vals = torch.stack([acc[("one", int(k))], acc[("both", 20)], acc[("both", 5)], acc[("both", 1)]]).tolist()
    return vals[0], vals[1], vals[2], vals[3], None, None


def foscttm_from_counts(closer: torch.Tensor):
    """(mu, std) of closer / n as 0-dim fp32 CPU tensors: mean and unbiased std, as foscttm's torch.mean / torch.std."""
    vec = topk_fraction(closer, closer.numel())
    mu_std = torch.stack([vec.mean(), vec.std()]).cpu()
    return mu_std[0], mu_std[1]


def foscttm(R, E):
    """eval_utils.py:232-247 -> (mu, std), 0-dim fp32 CPU tensors: for each row i of E, the share of rows of R strictly closer to
    E[i] than R[i] (Euclidean, raw embeddings).  Prints the reference's line."""
    counts = pair_counts(R, E)
    mu, std = foscttm_from_counts(counts["dist_col"])
    print(f"FOSCTTM Metrics, Mean: {mu}, std: {std}")
    return mu, std


def uniform_loss(x, t=2):
    """eval_utils.py:147-150: log(mean_{i<j} exp(-t |x^_i - x^_j|^2)) -> 0-dim fp32 device tensor (``ops.pair_uniformity``)."""
    return ops.pair_uniformity(_dev(x), float(t))


def alignment_loss(x1, x2, alpha=2):
    """eval_utils.py:153-156: mean_i |x^1_i - x^2_i|^alpha -> 0-dim fp32 device tensor (per-row terms of ``ops.pair_match_counts``)."""
    align = pair_counts(x1, x2)["align"]
    return align.mean() if alpha == 2 else align.sqrt().pow(alpha).mean()
