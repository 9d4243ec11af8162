"""CPU checks of the evaluation metrics (madrigal/evaluate/metrics.py:60-191): the C-ABI entry point is declared and exported, a short
sklearn restatement of get_metrics reproduces tests/golden/eval_metrics.npz (recorded from the reference by
scripts/gen_eval_metrics_golden.py), and metrics.get_metrics refuses bad arguments before touching a device.

The restatement (``restate_binary`` / ``restate_get_metrics``) is also the checker of tests/test_eval_metrics_gpu.py."""
import os
import warnings

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "eval_metrics.npz")
BASE_NAMES = ("fmax", "mcc", "auroc", "auprc", "npv", "specificity", "f1", "recall@", "precision@", "ap@", "accuracy", "precision", "recall")


def restate_binary(preds, ys, k):
    """The 13 numbers of get_metrics_binary for one problem, with sklearn; top-k ties by np.argsort(kind="stable")[::-1].
    Never raises on a one-class problem (the confusion matrix is taken over the labels {0, 1})."""
    from sklearn.metrics import average_precision_score, confusion_matrix, matthews_corrcoef, precision_recall_curve, roc_auc_score
    n = len(ys)
    kk = int(k * n) if isinstance(k, float) else k
    hard = (preds > 0.5).astype(np.float64)
    tn, fp, fn, tp = confusion_matrix(ys, hard, labels=[0, 1]).ravel()
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec, rec, npv, prec = tn / (tn + fp), tp / (tp + fn), tn / (tn + fn), tp / (tp + fp)
        f1 = 2 * prec * rec / (prec + rec)
        acc = (tp + tn) / n
        p, r, _ = precision_recall_curve(ys, preds)
        num, den = 2 * p * r, p + r
        fmax = float(np.max(np.where(den != 0, num / np.where(den != 0, den, 1), 0.0)))
        order = np.argsort(preds, kind="stable")[::-1]
        top = order[:kk]
        if kk > n:
            rk = pk = apk = np.nan
        else:
            rk, pk = ys[top].sum() / ys.sum(), ys[top].sum() / kk
            apk = average_precision_score(ys[top], preds[top])
        auroc = roc_auc_score(ys, preds)
        auprc = average_precision_score(ys, preds)
        mcc = matthews_corrcoef(ys, hard)
    return np.array([fmax, mcc, auroc, auprc, npv, spec, f1, rk, pk, apk, acc, prec, rec], dtype=np.float64), kk


def restate_get_metrics(preds, ys, labels, k=50, task="multilabel", average="macro"):
    """get_metrics (metrics.py:129-191) over restate_binary -> (names, values, pos_samples); raises ValueError where the reference's
    confusion_matrix unpack fails (targets and rounded preds of one problem all one class)."""
    def one(p, y):
        if len(np.unique(np.concatenate([y, np.round(p)]))) < 2:
            raise ValueError("one class")
        return restate_binary(p, y, k)
    if task == "binary" or average == "micro":
        v, kk = one(preds, ys)
        pos = ys.sum() if task == "binary" else np.array([ys[labels == l].sum() for l in np.unique(labels)])
        return [n + str(kk) if n.endswith("@") else n for n in BASE_NAMES], v, pos
    rows, pos = [], []
    for l in np.unique(labels):
        m = labels == l
        v, kk = one(preds[m], ys[m])
        rows.append(v)
        pos.append(ys[m].sum())
    rows, pos = np.array(rows), np.array(pos)
    names = [n + str(kk) if n.endswith("@") else n for n in BASE_NAMES]
    if average == "macro":
        return names, rows.mean(axis=0), pos
    if average == "weighted":
        return names, rows.T @ pos / pos.sum(), pos
    return names, rows.T, pos


def golden_runs():
    z = np.load(GOLDEN)
    for key in z.files:
        if key.endswith("/names"):
            name, task, avg = key.split("/")[:3]
            k = z[f"{name}/k"].item()
            yield (name, task, None if avg == "None" else avg, k, z[f"{name}/preds"], z[f"{name}/ys"], z[f"{name}/labels"].astype(np.int64),
                   [str(s) for s in z[key]], z[f"{name}/{task}/{avg}/values"], z[f"{name}/{task}/{avg}/pos"])


def test_label_metrics_symbol_is_declared_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    assert "mdg_label_metrics" in syms and "mdg_label_metrics_workspace_bytes" in syms
    L = _lib.lib()
    assert hasattr(L, "mdg_label_metrics")
    b = L.mdg_label_metrics_workspace_bytes(6_000_000, 896)
    assert b >= 16 * 6_000_000 and L.mdg_label_metrics_workspace_bytes(0, 896) == 0


def test_restatement_reproduces_the_reference_golden():
    pytest.importorskip("sklearn")
    runs = list(golden_runs())
    assert {r[1:3] for r in runs} >= {("multilabel", None), ("multilabel", "macro"), ("multilabel", "weighted"), ("multilabel", "micro"),
                                     ("binary", "macro")}
    for name, task, avg, k, preds, ys, labels, want_names, want, want_pos in runs:
        names, got, pos = restate_get_metrics(preds, ys, labels, k=k, task=task, average=avg)
        assert names == want_names, (name, avg)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{name}/{avg}")
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, equal_nan=True, err_msg=f"{name}/{avg}")
        f64 = np.ones(13, dtype=bool)
        f64[7:9] = False                                            # recall@k, precision@k: float32 in the reference
        np.testing.assert_allclose(got[f64], want[f64], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{name}/{avg}")
        np.testing.assert_allclose(np.asarray(pos, np.float64), want_pos, rtol=0, atol=0)


@pytest.mark.parametrize("kw, msg", [(dict(average="median"), "average"), (dict(task="regression"), "task"), (dict(k=0), "k must be"),
                                     (dict(k=1.5), "float k"), (dict(k=-3), "k must be"), (dict(k="50"), "k must be")])
def test_get_metrics_refuses_bad_arguments_without_a_device(kw, msg):
    from madrigal_amd import metrics
    p, y, l = np.full(4, 0.7, np.float32), np.array([0, 1, 0, 1], np.float32), np.zeros(4, np.int64)
    with pytest.raises(ValueError, match=msg):
        metrics.get_metrics(p, y, l, **kw)


def test_get_metrics_refuses_mismatched_lengths_without_a_device():
    from madrigal_amd import metrics
    with pytest.raises(ValueError, match="one length"):
        metrics.get_metrics(np.zeros(4, np.float32), np.zeros(3, np.float32), np.zeros(4, np.int64))
