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

Which rows are nearest -- the reference's ``knn_classifier`` (eval_utils.py:177-229) and the index tensors of
``get_inst_dist_topk_accuracy`` -- is a second sweep (``ops.knn_topk``, csrc/knn.hip) that keeps each query's k best in registers:
``nearest_neighbors``, ``inst_dist_topk_indices``, ``knn_predict`` / ``knn_classifier``.  Its similarities are the counting sweep's
bit for bit, and equal values are ordered by ascending index.

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


def nearest_neighbors(queries, library, k: int, metric: str = "cosine", skip=None):
    """The ``k`` rows of ``library`` [nl,128] nearest to every row of ``queries`` [nq,128] -> ``(values fp32 [nq,k], indices int64
    [nq,k])`` on the device, ordered by (value best-first, library index ascending).  metric: 'cosine' or 'dot' (similarities,
    largest first) or 'euclidean' (distances, smallest first).  ``skip`` [nq]: the library row each query must not return (-1:
    none), for queries that are themselves in the library.  One sweep (``ops.knn_topk``, csrc/knn.hip): no [nq,nl] matrix exists,
    so 100 000 queries against 100 000 rows need the two inputs and the result, not 40 GB.  1 <= k <= 32."""
    q, lib = _dev(queries).float(), _dev(library).float()
    if skip is not None:
        skip = _dev(skip).to(device=q.device, dtype=torch.int32).reshape(-1)
    vals, idx = ops.knn_topk(q, lib.to(q.device), int(k), metric=metric, skip=skip)
    return vals, idx.long()


def inst_dist_topk_indices(embeds1, embeds2, k: int):
    """evaluate.py:417-418 -> ``(topk_rows, topk_cols)`` int64 [n,k] on the device: the two values ``get_inst_dist_topk_accuracy``
    leaves out.  Row i of ``topk_rows`` holds the k rows of embeds2 most cosine-similar to embeds1[i], row j of ``topk_cols`` the k
    rows of embeds1 most similar to embeds2[j], most similar first and, unlike ``torch.topk``, equal similarities by ascending
    index.  The similarities are the ones ``pair_counts`` compares, bit for bit: index i sits at position cos_row[i] of row i
    whenever cos_row[i] < k (no competitor ties with the true match)."""
    x, y = _dev(embeds1).float(), _dev(embeds2).float()
    _need_k(int(k), int(y.shape[0]), "inst_dist_topk_indices")
    return nearest_neighbors(x, y, k)[1], nearest_neighbors(y, x, k)[1]


def _labels_u8(labels, num_classes: int, what: str) -> torch.Tensor:
    lab = _dev(labels)
    if lab.dim() not in (1, 2) or lab.is_floating_point() and bool((lab != lab.round()).any()):
        raise ValueError(f"{what}: labels must be integers of shape [n] or [n, C], got {tuple(lab.shape)} {lab.dtype}")
    if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= num_classes):
        raise ValueError(f"{what}: labels must lie in [0, {num_classes}), got [{int(lab.min())}, {int(lab.max())}]")
    return lab.to(torch.uint8).contiguous()


def knn_predict(train_features, train_labels, test_features, metric: str = "cosine", k: int = 5, T: float = 1, num_classes: int = 2):
    """The kNN classifier of eval_utils.py:177-229 without the scoring -> ``(predictions uint8, class sums fp32)`` on the device:
    [n_test] and [n_test, num_classes] for a label vector, [n_test, C] and [n_test, C, 2] for [n_train, C] binary labels (one
    neighbour search serves every column).  Neighbours by ``nearest_neighbors`` ('cosine' or 'euclidean'), weights
    exp(value / T) -- for 'euclidean' too, as the reference has it -- and the class with the largest weight sum, the lowest class
    on a tie (the reference's sort leaves ties open)."""
    if metric not in ("cosine", "euclidean"):
        raise NotImplementedError(f"knn_classifier: unknown metric {metric!r}")
    lab = _labels_u8(train_labels, int(num_classes), "knn_classifier")
    train = _dev(train_features).float()
    if lab.shape[0] != train.shape[0]:
        raise ValueError(f"knn_classifier: {train.shape[0]} training rows but {lab.shape[0]} labels")
    _need_k(int(k), int(train.shape[0]), "knn_classifier")
    q = _dev(test_features).float()
    vals, idx = ops.knn_topk(q, train.to(q.device), int(k), metric=metric)
    return ops.knn_vote(vals, idx, lab.to(q.device), float(T), int(num_classes))


def knn_classifier(train_features, train_labels, test_features, test_labels, metric='cosine', k=5, T=1, num_classes=2):
    """eval_utils.py:177-229 (kNN ATC classification of the pretrained embeddings) -> top-1 accuracy as a Python float.  With
    [n, C] binary labels: an fp32 [C] device tensor of per-label accuracies from ONE neighbour search (the reference's docstring
    asks for per-label reporting and pays for it with C calls).  See ``knn_predict``."""
    pred, _ = knn_predict(train_features, train_labels, test_features, metric=metric, k=k, T=T, num_classes=num_classes)
    target = _labels_u8(test_labels, int(num_classes), "knn_classifier").to(pred.device)
    if target.shape != pred.shape:
        raise ValueError(f"knn_classifier: test labels of shape {tuple(target.shape)} for predictions of shape {tuple(pred.shape)}")
    correct = (pred == target).sum(0)
    n = int(pred.shape[0])
    return int(correct) / n if pred.dim() == 1 else topk_fraction(correct, n)


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


# ------------------------------------------------------------------------------------------------- GeomCA
# madrigal/evaluate/GeomCA.py with the parameters of get_alignment_metrics (evaluate.py:481-496; random_seed = SEED = 42).  The
# reference copies the embeddings to the host and goes through GUDHI (k-d tree sparsification, Rips complex) and networkx; here the
# geometry is three kinds of sweeps over squared distances (ops.geomca_*, csrc/geomca.hip) and only O(n) index arrays reach the host.
GEOMCA_DEFAULTS = dict(Rdist_ratio=1.0, Rdist_percentile=5, gamma=1, reduceR=True, reduceE=True, sparsify=True, n_Rsamples=None,
                       n_Esamples=None, comp_consistency_threshold=0.0, comp_quality_threshold=0.0, random_seed=42)
_GEOMCA_IGNORED = ("experiment_path", "experiment_filename_prefix", "subfolder", "log_reduced")      # nothing is written


def geomca_epsilon(R: torch.Tensor, Rdist_ratio: float, Rdist_percentile: float) -> float:
    """GeomCA.estimate_distance (GeomCA.py:250-282): m = int(nR * Rdist_ratio) rows drawn twice with ``np.random.choice`` from
    numpy's global generator, in the reference's order; the percentile of the positive distances among the m x m pairs, by numpy's
    linear interpolation between two exact order statistics of the fp32 squared distances (``ops.geomca_distance_select``).  Pairs
    whose two draws are the same row are left out (their distance is 0 in the reference)."""
    n = int(R.shape[0])
    m = int(n * Rdist_ratio)
    if m < 1:
        raise ValueError(f"geomca: Rdist_ratio = {Rdist_ratio} leaves no estimation points of {n} rows")
    i1 = torch.from_numpy(np.random.choice(n, m)).to(R.device)
    i2 = torch.from_numpy(np.random.choice(n, m)).to(R.device)
    _, M, lo, hi, pos = ops.geomca_distance_select(R.index_select(0, i1), R.index_select(0, i2), i1, i2, float(Rdist_percentile))
    if M == 0:
        raise ValueError("geomca: every estimation pair is at distance 0; epsilon cannot be estimated (np.percentile of an empty array)")
    a, b = float(np.sqrt(lo)), float(np.sqrt(hi))
    return a + (b - a) * (pos - float(np.floor(pos)))


def geomca_scores(label, deg_same, deg_cross, n_r: int, comp_consistency_threshold: float = 0.0, comp_quality_threshold: float = 0.0):
    """Component and network scores (GeomCA.py:392-471, :215-223) from the arrays of ``ops.geomca_components`` ->
    ``(comp_stats, network_stats)``.  Components by size descending, then smallest vertex ascending."""
    label, ds, dc = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64) for t in (label, deg_same, deg_cross))
    n = label.size
    n_e = n - n_r
    roots, inv, sizes = np.unique(label, return_inverse=True, return_counts=True)           # roots ascend
    inv = inv.reshape(-1)
    is_r = np.arange(n) < n_r
    r_cnt = np.bincount(inv, weights=is_r, minlength=roots.size).astype(np.int64)
    e_cnt = sizes - r_cnt
    deg2 = np.bincount(inv, weights=ds + dc, minlength=roots.size).astype(np.int64)       # every edge counted from both ends
    cross2 = np.bincount(inv, weights=dc, minlength=roots.size).astype(np.int64)
    if (deg2 % 2).any() or (cross2 % 2).any():
        raise RuntimeError("geomca: the degree sums of a component are odd (the neighbour relation is not symmetric)")
    members = np.split(np.argsort(inv, kind="stable"), np.cumsum(sizes)[:-1])
    comp_stats = {}
    net = {"num_R_points_in_qualitycomp": 0, "num_E_points_in_qualitycomp": 0, "precision": None, "recall": None,
           "network_consistency": None, "network_quality": None}
    for ci, c in enumerate(np.lexsort((roots, -sizes))):
        r, e, edges, cross = int(r_cnt[c]), int(e_cnt[c]), int(deg2[c] // 2), int(cross2[c] // 2)
        consistency = 1 - abs(r - e) / (r + e)
        quality = cross / edges if edges != 0 else 0
        mem = members[c]
        comp_stats[ci] = {"Ridx": mem[:r], "Eidx": mem[r:] - n_r, "comp_consistency": consistency, "comp_quality": quality,
                          "num_edges": edges, "num_RE_edges": cross}
        if consistency > comp_consistency_threshold and quality > comp_quality_threshold:
            net["num_R_points_in_qualitycomp"] += r
            net["num_E_points_in_qualitycomp"] += e
    edges, cross = int(deg2.sum() // 2), int(cross2.sum() // 2)
    net["precision"] = net["num_E_points_in_qualitycomp"] / n_e
    net["recall"] = net["num_R_points_in_qualitycomp"] / n_r
    net["network_consistency"] = 1 - abs(n_r - n_e) / (n_r + n_e)
    net["network_quality"] = cross / edges if edges != 0 else 0
    return comp_stats, net


def geomca(R, E, **parameters):
    """``GeomCA(R, E, param_dict).get_connected_components()`` (madrigal/evaluate/GeomCA.py) on the device ->
    ``(comp_stats, network_stats, network_params)`` with the reference's keys.  R [nR,128], E [nE,128]; parameters as in the
    reference's ``param_dict`` (defaults ``GEOMCA_DEFAULTS``: those of get_alignment_metrics); ``epsilon`` given skips the estimate.

    comp_stats[i] (components by size descending, then smallest vertex): ``Ridx``, ``Eidx`` (indices into the sparse sets, ascending),
    ``comp_consistency``, ``comp_quality`` and, in place of the networkx ``comp_graph``, ``num_edges`` / ``num_RE_edges``.
    network_stats: ``num_R_points_in_qualitycomp``, ``num_E_points_in_qualitycomp``, ``precision``, ``recall``,
    ``network_consistency``, ``network_quality``.  network_params: the reference's seven entries and ``sparseR_index`` /
    ``sparseE_index``, the kept input rows (int64 numpy).  The path parameters are accepted and nothing is written.  The random
    draws (the estimate's two, then R's and E's samples when ``sparsify`` is False) come from numpy's global generator after
    ``np.random.seed(random_seed)``, as in the reference.  An empty reduced set raises ValueError (the reference divides by zero)."""
    unknown = set(parameters) - set(GEOMCA_DEFAULTS) - set(_GEOMCA_IGNORED) - {"epsilon"}
    if unknown:
        raise ValueError(f"geomca: unknown parameters {sorted(unknown)}")
    p = dict(GEOMCA_DEFAULTS, **parameters)
    R, E = _dev(R).float().contiguous(), _dev(E).float().contiguous()
    E = E.to(R.device)
    np.random.seed(p["random_seed"])
    if p.get("epsilon") is not None:
        epsilon = float(p["epsilon"])
    else:
        epsilon = geomca_epsilon(R, p["Rdist_ratio"], p["Rdist_percentile"])
    delta = epsilon * p["gamma"]

    def reduce_(X, flag, n_samples):
        if not flag:
            return torch.arange(X.shape[0], device=X.device)
        if p["sparsify"]:
            return ops.geomca_sparsify(X, delta)
        if n_samples is None:
            raise ValueError("geomca: sparsify=False needs n_Rsamples / n_Esamples")
        return torch.from_numpy(np.random.choice(np.arange(X.shape[0]), n_samples)).to(X.device)

    ri = reduce_(R, p["reduceR"], p["n_Rsamples"])
    ei = reduce_(E, p["reduceE"], p["n_Esamples"])
    n_r, n_e = int(ri.numel()), int(ei.numel())
    if n_r == 0 or n_e == 0:
        raise ValueError(f"geomca: an empty reduced set ({n_r} R points, {n_e} E points)")
    V = torch.cat([R.index_select(0, ri), E.index_select(0, ei)])
    label, deg_same, deg_cross, _ = ops.geomca_components(V, n_r, epsilon)
    comp_stats, network_stats = geomca_scores(label, deg_same, deg_cross, n_r, p["comp_consistency_threshold"], p["comp_quality_threshold"])
    network_params = {"num_R_points": n_r, "num_E_points": n_e, "num_RE_points": n_r + n_e, "epsilon": epsilon, "gamma": p["gamma"],
                      "comp_consistency_threshold": p["comp_consistency_threshold"],
                      "comp_quality_threshold": p["comp_quality_threshold"],
                      "sparseR_index": ri.cpu().numpy().astype(np.int64), "sparseE_index": ei.cpu().numpy().astype(np.int64)}
    return comp_stats, network_stats, network_params
