"""CPU checks of the pretraining-evaluation checker: the fp64 restatement (tests/pretrain_eval_ref.py) reproduces the reference's
own recorded outputs (tests/golden/pretrain_eval.npz, scripts/gen_pretrain_eval_golden.py), and evaluate_pt's report keys."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pretrain_eval_ref as R                                    # noqa: E402


def _case(g, n):
    return g[f"n{n}_x"].astype(np.float32), g[f"n{n}_y"].astype(np.float32)


@pytest.mark.parametrize("n", [20, 257, 1000])
def test_restatement_reproduces_reference_outputs(golden, n):
    g = golden("pretrain_eval")
    X, Y = _case(g, n)
    c = R.counts(X, Y, rel=1e-4)
    for name in R.COUNT_NAMES:
        assert c["amb_" + name].sum() == 0, name                 # the fixture keeps every decision clear of its threshold
    assert [R.one_side_acc(c, k) for k in (1, 5, 20)] == list(g[f"n{n}_acc_k1_5_20"])
    assert [R.stacked_acc(c, k) for k in (20, 5, 1)] == list(g[f"n{n}_stacked_top20_5_1"])
    assert 0.0 < R.one_side_acc(c, 1) < 1.0
    np.testing.assert_allclose(R.foscttm(c["dist_col"]), g[f"n{n}_foscttm_xy"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(R.foscttm(c["dist_row"]), g[f"n{n}_foscttm_yx"], rtol=0, atol=1e-6)
    np.testing.assert_allclose([R.uniform_loss(X), R.uniform_loss(Y)], g[f"n{n}_uniform_x_y"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(R.alignment_loss(X, Y), g[f"n{n}_alignment"][0], rtol=0, atol=1e-6)


def test_evaluate_pt_report_keys():
    from madrigal_amd import evaluate as E
    keys = E.pretrain_log_keys("val")
    report = keys[0]
    assert len(report) == 5 * 14 and len(set(report)) == len(report)
    assert report[:3] == ["val top20 acc str v kg embed one-side (cosine)", "val top5 acc str v kg embed one-side (cosine)",
                          "val top1 acc str v kg embed one-side (cosine)"]
    assert report[3] == "val top20 acc str v kg CL-head one-side (cosine)"
    assert report[6] == "val top20 acc str v kg embed both-side (cosine)"
    assert report[12:14] == ["val loss str v kg", "val foscttm mu str v kg"]
    assert report[14 * 2] == "val top20 acc str v tx_mcf7 embed one-side (cosine)"
    assert [k[0] for k in keys[1:7]] == [f"val uniformity loss {m}" for m in ("str", "kg", "cv", "tx_mcf7", "tx_pc3", "tx_vcap")]
    assert [k[0] for k in keys[7:]] == [f"val alignment loss str v {m}" for m in ("kg", "cv", "tx_mcf7", "tx_pc3", "tx_vcap")]
    assert [E.MODALITY2NUMBER_LIST[m][0] for m in E.PT_UNIFORMITY_MODALITIES] == [0, 1, 2, 13, 15, 17]


def test_from_indices_to_tensor_matches_the_reference_mask():
    from madrigal_amd import evaluate as E
    m = E.from_indices_to_tensor([0], 19)
    assert m.shape == (19,) and m[0] == 0 and m[1:].eq(1).all()
