"""fp64 numpy restatement of the k-nearest-neighbour search and the kNN classifier's vote (csrc/knn.hip), written from their
definitions:

  value of (query i, library row j), g = q_i . l_j:  cosine g / (|q_i| |l_j|), larger is better;  dot g, larger is better;
  euclidean: ranked on d2 = |q_i|^2 - 2 g + |l_j|^2, smaller is better, reported as sqrt(max(d2, 0)).
  Order: value best-first, then library index ascending (a stable sort).  skip[i]: the library row query i must not return.

Tolerances of an fp32 result against these: a 128-term fp32 dot product is off by at most 128 * 2^-24 ~ 7.6e-6 of |q||l|, so
cosine 1e-5, dot 1e-5 |q||l|, d2 1e-5 (|q| + |l|)^2 (``scale`` below times 1e-5).
"""
import numpy as np

METRICS = ("cosine", "dot", "euclidean")
TOL = 1e-5


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def keys(Q, L, metric):
    """[nq, nl] fp64 ranking keys, SMALLER is better: -cosine, -dot, d2."""
    Q, L = _f64(Q), _f64(L)
    G = Q @ L.T
    if metric == "dot":
        return -G
    q2, l2 = (Q * Q).sum(1), (L * L).sum(1)
    if metric == "cosine":
        with np.errstate(divide="ignore", invalid="ignore"):
            return -(G / np.sqrt(q2)[:, None] / np.sqrt(l2)[None, :])
    if metric == "euclidean":
        return q2[:, None] - 2.0 * G + l2[None, :]
    raise ValueError(metric)


def scale(Q, L, metric):
    """[nq, nl] (or a scalar 1 for cosine): what the tolerance of a key is relative to."""
    if metric == "cosine":
        return np.float64(1.0)
    Q, L = _f64(Q), _f64(L)
    nq, nl = np.sqrt((Q * Q).sum(1)), np.sqrt((L * L).sum(1))
    return nq[:, None] * nl[None, :] if metric == "dot" else (nq[:, None] + nl[None, :]) ** 2


def reported(key, metric):
    """The value the search reports for a ranking key."""
    return np.sqrt(np.maximum(key, 0.0)) if metric == "euclidean" else -key


def _skipped(K, skip):
    if skip is not None:
        skip = np.asarray(skip)
        rows = np.flatnonzero(skip >= 0)
        K = K.copy()
        K[rows, skip[rows]] = np.inf
    return K


class Ranked:
    """The keys of (Q, L, metric, skip) sorted once by a stable sort on (key, index); the first ``keep`` of every row are kept."""

    def __init__(self, Q, L, metric, skip=None, keep=33):
        self.metric = metric
        self.K = _skipped(keys(Q, L, metric), skip)                              # [nq, nl]
        self.S = np.broadcast_to(scale(Q, L, metric), self.K.shape)
        self.idx = np.argsort(self.K, axis=1, kind="stable")[:, :keep].astype(np.int64)
        self.keys = np.take_along_axis(self.K, self.idx, 1)
        self.scales = np.take_along_axis(self.S, self.idx, 1)

    def topk(self, k):
        """(values fp64 [nq, k], indices int64 [nq, k])."""
        return reported(self.keys[:, :k], self.metric), self.idx[:, :k]

    def margins(self, k, tol):
        """[nq, nl] fp64: (key - the row's k-th key) in units of the pair's tolerance: < -1 beats the k-th by more than tol, > 1
        loses by more than tol, within [-1, 1] is ambiguous."""
        kth, skth = self.keys[:, k - 1:k], self.scales[:, k - 1:k]
        with np.errstate(invalid="ignore"):
            return (self.K - kth) / (tol * np.maximum(self.S, skth))

    def ambiguous(self, k, tol, order=False):
        """Queries (indices) where some value other than the k-th lies within ``tol`` (times ``scale``) of the k-th: their
        k-nearest SET depends on rounding.  order=True: also the queries where two of the first k + 1 values lie that close to
        each other, so that the ORDER of the list depends on rounding."""
        bad = (np.abs(self.margins(k, tol)) <= 1.0).sum(1) > 1                   # the k-th itself is one
        if order:
            m = min(k + 1, self.keys.shape[1])
            with np.errstate(invalid="ignore"):
                gap = np.abs(np.diff(self.keys[:, :m], axis=1)) <= tol * np.maximum(self.scales[:, 1:m], self.scales[:, :m - 1])
            bad |= gap.any(1)
        return np.flatnonzero(bad)


def topk(Q, L, k, metric, skip=None):
    """(values fp64 [nq, k], indices int64 [nq, k]) by a stable sort on (key, index)."""
    return Ranked(Q, L, metric, skip, keep=k).topk(k)


def ambiguous(Q, L, k, metric, tol, skip=None, order=False):
    """See ``Ranked.ambiguous``."""
    return Ranked(Q, L, metric, skip, keep=k + 1).ambiguous(k, tol, order)


def vote(vals, idx, labels, T, num_classes):
    """The classifier's epilogue -> (pred uint8, sums fp64, margin fp64).  Weights w_j = exp(vals_j / T), for both metrics.
    labels [nl] with num_classes > 2: per-class sums [nq, num_classes].  num_classes == 2, labels [nl] or [nl, C]: p1 = sum_j w_j
    label_j, p0 = sum_j w_j - p1; sums [nq, 2] or [nq, C, 2].  pred: the largest sum, the lowest class on a tie.  margin: (best -
    second best) / sum_j w_j, per prediction."""
    vals, idx, labels = _f64(vals), np.asarray(idx), np.asarray(labels)
    w = np.exp(vals / float(T))                                                   # [nq, k]
    wsum = w.sum(1)
    if num_classes == 2:
        lab = labels[idx] if labels.ndim == 1 else np.moveaxis(labels[idx], 2, 1)  # [nq, k] or [nq, C, k]
        wj = w if labels.ndim == 1 else w[:, None, :]
        ws = wsum if labels.ndim == 1 else wsum[:, None]
        p1 = np.zeros(lab.shape[:-1])
        for j in range(w.shape[1]):                                               # j ascending
            p1 = p1 + wj[..., j] * lab[..., j]
        sums = np.stack([ws - p1, p1], -1)
    else:
        assert labels.ndim == 1
        lab = labels[idx]
        sums = np.zeros((w.shape[0], num_classes))
        for j in range(w.shape[1]):
            sums[np.arange(w.shape[0]), lab[:, j]] += w[:, j]
        ws = wsum
    pred = sums.argmax(-1).astype(np.uint8)
    srt = np.sort(sums, -1)
    margin = (srt[..., -1] - srt[..., -2]) / ws
    return pred, sums, margin
