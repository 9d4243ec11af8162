"""fp64 numpy restatement of the reference's pretraining-evaluation metrics (madrigal/evaluate/evaluate.py:406-450
get_inst_dist_topk_accuracy, madrigal/evaluate/eval_utils.py:147-174 uniform_loss / alignment_loss /
stacked_inst_dist_topk_accuracy, :232-247 foscttm): the checker of the GPU tests of csrc/retrieval.hip.

Counts follow the HIP path's definitions (the true match of row i is column i, strict comparisons: ties count as hits).  Each
count comes with the number of its comparisons that lie within ``rel`` of the threshold on the compared quantity's scale
(``amb_*``): fp32 rounding may decide those either way.  Accuracies are formed in fp32 the way the reference forms them (an fp32
sum of hits divided by an int), so they equal the reference's numbers exactly when the counts agree."""
from __future__ import annotations

import numpy as np

COUNT_NAMES = ("cos_row", "cos_col", "same_x", "same_y", "dist_row", "dist_col")


def _unit(a: np.ndarray) -> np.ndarray:
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def counts(X, Y, rel: float = 1e-5) -> dict:
    """Six int64 [n] counts, the matching ``amb_<name>`` counts of near-ties and ``align`` = |x^_i - y^_i|^2 (fp64)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n = X.shape[0]
    xh, yh = _unit(X), _unit(Y)
    off = ~np.eye(n, dtype=bool)
    C = xh @ yh.T
    c = np.diag(C).copy()
    out = {}

    def put(name, val, thr, scale, axis, strict_gt):
        diff = (val - thr) if strict_gt else (thr - val)
        out[name] = ((diff > 0) & off).sum(axis=axis)
        out["amb_" + name] = ((np.abs(diff) <= rel * scale) & off).sum(axis=axis)

    put("cos_row", C, c[:, None], 1.0, 1, True)
    put("cos_col", C, c[None, :], 1.0, 0, True)
    put("same_x", xh @ xh.T, c[:, None], 1.0, 1, True)
    put("same_y", yh @ yh.T, c[:, None], 1.0, 1, True)
    nx, ny = np.linalg.norm(X, axis=1), np.linalg.norm(Y, axis=1)
    D2 = (X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :] - 2.0 * (X @ Y.T)
    d = np.diag(D2).copy()
    pair = (nx[:, None] + ny[None, :]) ** 2
    put("dist_row", D2, d[:, None], pair + ((nx + ny) ** 2)[:, None], 1, False)      # |x_i - y_j| < |x_i - y_i|
    put("dist_col", D2, d[None, :], pair + ((nx + ny) ** 2)[None, :], 0, False)      # |x_i - y_j| < |x_j - y_j|
    out["align"] = ((xh - yh) ** 2).sum(1)
    return out


def fp32_fraction(hits: int, total: int) -> float:
    return float(np.float32(hits) / np.float32(total))


def one_side_acc(cnt: dict, k: int) -> float:
    """get_inst_dist_topk_accuracy's topk_acc: 1 - misses / 2n (fp32)."""
    n = len(cnt["cos_row"])
    miss = int((cnt["cos_row"] >= k).sum() + (cnt["cos_col"] >= k).sum())
    return float(np.float32(1) - np.float32(miss) / np.float32(2 * n))


def stacked_acc(cnt: dict, k: int) -> float:
    """stacked_inst_dist_topk_accuracy on the [2n, 2n-1] stacked cosines: hits / 2n (fp32)."""
    n = len(cnt["cos_row"])
    hit = int(((cnt["cos_row"] + cnt["same_x"]) < k).sum() + ((cnt["cos_col"] + cnt["same_y"]) < k).sum())
    return fp32_fraction(hit, 2 * n)


def foscttm(closer) -> tuple:
    """(mean, unbiased std) of closer / n in fp64.  foscttm(R=X, E=Y) uses dist_col, foscttm(R=Y, E=X) dist_row."""
    v = np.asarray(closer, dtype=np.float64) / len(closer)
    return float(v.mean()), float(v.std(ddof=1))


def uniform_loss(X, t: float = 2.0) -> float:
    xh = _unit(np.asarray(X, dtype=np.float64))
    iu = np.triu_indices(xh.shape[0], 1)
    d2 = np.maximum(2.0 - 2.0 * (xh @ xh.T), 0.0)[iu]                   # fp64: the cancellation costs ~1e-16
    return float(np.log(np.mean(np.exp(-t * d2))))


def alignment_loss(X, Y, alpha: float = 2.0) -> float:
    xh, yh = _unit(np.asarray(X, dtype=np.float64)), _unit(np.asarray(Y, dtype=np.float64))
    return float((np.linalg.norm(xh - yh, axis=1) ** alpha).mean())


def subset_tuple(cnt_embed: dict, cnt_head: dict, loss: float) -> tuple:
    """evaluate_pretrain_subsets' 14-tuple from the counts of the embeddings and of the CL-head outputs (loss given)."""
    one = [one_side_acc(c, k) for c in (cnt_embed, cnt_head) for k in (20, 5, 1)]
    both = [stacked_acc(c, k) for c in (cnt_embed, cnt_head) for k in (20, 5, 1)]
    mu = (np.float32(foscttm(cnt_embed["dist_col"])[0]) + np.float32(foscttm(cnt_embed["dist_row"])[0])) / np.float32(2)
    return tuple(one + both) + (loss, float(mu))
