"""CPU checks of the drug-stratified evaluation (madrigal/evaluate/predict.py:274-355, get_drug_specific_scores): the C-ABI entry
point is declared and exported, a short sklearn restatement reproduces tests/golden/drug_metrics.npz (recorded from the reference
by scripts/gen_drug_metrics_golden.py) in both modes and fails where the reference fails, and the Python layer refuses bad
arguments before touching a device.

The restatement (``restate_drug_scores``) is also the checker of tests/test_drug_metrics_gpu.py."""
import os

import numpy as np
import pytest
import torch

from test_eval_metrics_cpu import restate_get_metrics

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "drug_metrics.npz")


def restate_drug_scores(preds, heads, tails, labels, pos_neg, n_head, mode):
    """get_drug_specific_scores over restate_get_metrics -> (names, values [13, n_drugs], drug indices); ValueError where the
    reference fails (no positives, a one-class problem, negatives missing)."""
    pos = pos_neg.astype(bool)
    pi, ni = np.flatnonzero(pos), np.flatnonzero(~pos)
    n_pos = pi.size
    owner = (heads if mode == "test_between" else tails)[pi]
    drugs = np.arange(n_head) if mode == "test_between" else np.unique(owner)
    names, cols = None, []
    for d in drugs:
        idx = np.flatnonzero(owner == d)
        if idx.size == 0:
            raise ValueError(f"drug {d}: no positives")
        if (idx + n_pos >= ni.size).any():
            raise ValueError(f"drug {d}: negatives missing")
        sel = np.concatenate([pi[idx], ni[idx], ni[idx + n_pos]])
        names, v, _ = restate_get_metrics(preds[sel], pos_neg[sel].astype(np.float32), labels[sel], k=50, task="multiclass",
                                          average="macro")
        cols.append(v)
    return names, np.array(cols).T, drugs


def golden_cases():
    z = np.load(GOLDEN)
    for key in z.files:
        if key.endswith("/mode"):
            name = key[:-5]
            g = lambda x: z[f"{name}/{x}"]  # noqa: E731
            n_head, n_tail = (int(v) for v in g("n_head_tail"))
            want = {"exception": str(g("exception"))} if f"{name}/exception" in z.files else \
                {"names": [str(s) for s in g("names")], "values": g("values"), "drugs": g("drugs")}
            yield (name, str(g("mode")), n_head, n_tail, g("preds"), g("heads").astype(np.int64), g("tails").astype(np.int64),
                   g("labels").astype(np.int64), g("pos_neg").astype(np.float32), want)


def check_values(got, want, what, rtol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    f64 = np.ones(13, dtype=bool)
    f64[7:9] = False                                                # recall@k, precision@k: float32 in the reference
    np.testing.assert_allclose(got[f64], want[f64], rtol=rtol, atol=1e-15, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(got[~f64], want[~f64], rtol=1e-6, atol=0, equal_nan=True, err_msg=what)


def test_group_metrics_symbol_is_declared_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    assert "mdg_group_metrics" in syms and "mdg_group_metrics_workspace_bytes" in syms
    L = _lib.lib()
    assert hasattr(L, "mdg_group_metrics")
    b = L.mdg_group_metrics_workspace_bytes(3_000_000, 4096 * 896)
    assert b >= 16 * 3_000_000 + 8 * 3_000_000 and L.mdg_group_metrics_workspace_bytes(0, 10) == 0


def test_restatement_reproduces_the_reference_golden():
    pytest.importorskip("sklearn")
    seen = set()
    for name, mode, n_head, n_tail, preds, heads, tails, labels, pos_neg, want in golden_cases():
        seen.add((name, mode))
        if "exception" in want:
            continue
        names, got, drugs = restate_drug_scores(preds, heads, tails, labels, pos_neg, n_head, mode)
        assert names == want["names"], name
        offset = 10_000 if mode == "test_between" else 20_000
        np.testing.assert_array_equal(drugs + offset, want["drugs"], err_msg=name)
        check_values(got, want["values"], name)
    assert {m for _, m in seen} == {"test_between", "test_between_train"} and len(seen) == 7


def test_restatement_fails_where_the_reference_fails():
    pytest.importorskip("sklearn")
    n = 0
    for name, mode, n_head, n_tail, preds, heads, tails, labels, pos_neg, want in golden_cases():
        if "exception" not in want:
            continue
        assert want["exception"] in ("ValueError", "IndexError"), name
        with pytest.raises(ValueError):
            restate_drug_scores(preds, heads, tails, labels, pos_neg, n_head, mode)
        n += 1
    assert n == 3


def test_mixed_case_has_defined_top_k_metrics():
    z = {c[0]: c for c in golden_cases()}
    v = z["mixed"][-1]["values"]
    assert np.isfinite(v[7:10, 1]).all() and np.isnan(v[7:10, 0]).all()   # drug 1: groups of 51+ triples; drug 0 mixes sizes


def test_drug_specific_metrics_refuses_cpu_tensors_and_unknown_modes():
    from madrigal_amd import metrics, predict
    t = torch.zeros(6)
    with pytest.raises(ValueError, match="CUDA"):
        metrics.drug_specific_metrics(t, t.long(), t.long(), t.long(), t, 2, "test_between")
    with pytest.raises(NotImplementedError):
        metrics.drug_specific_metrics(t, t.long(), t.long(), t.long(), t, 2, "val_within")
    with pytest.raises(NotImplementedError):
        predict.get_drug_specific_scores(None, {}, "full_full", "str_str+random_sample", "cpu", force_ori_modalities=True)
    with pytest.raises(NotImplementedError):
        predict.get_drug_specific_scores(None, {}, "full_full", "str_str+random_sample", "cpu", mode="train")


def test_make_eval_triples_layout():
    from madrigal_amd import data as D
    lab, h, t, pn = D.make_eval_triples(50, 70, 9, 400, 3)
    n = 400
    assert lab.shape == (3 * n,) and pn.dtype == torch.float32 and float(pn[:n].sum()) == n and float(pn[n:].sum()) == 0
    assert torch.equal(lab[:n], lab[n:2 * n]) and torch.equal(lab[:n], lab[2 * n:])
    assert torch.equal(h[:n], h[n:2 * n]) and torch.equal(h[:n], h[2 * n:])
    assert set(h[:n].tolist()) == set(range(50)) and int(t.max()) < 70
    lab2, h2, t2, _ = D.make_eval_triples(50, 70, 9, 400, 3, between=False)
    assert torch.equal(t2[:n], t2[2 * n:]) and torch.equal(h2[:n], h2[n:2 * n])
    with pytest.raises(ValueError):
        D.make_eval_triples(50, 70, 9, 40, 3)
