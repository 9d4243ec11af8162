"""CPU checks of the k-nearest-neighbour feature: the fp64 restatement tests/knn_ref.py against the reference's recorded
accuracies (tests/golden/knn.npz, scripts/gen_knn_golden.py), and the host-only queries of csrc/knn.hip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as R                                              # noqa: E402

KS, METRICS, TS, CLASSES = (1, 5, 20), ("cosine", "euclidean"), (0.07, 1.0), (2, 4)


def case_key(ntr, k, metric, T, nc):
    return f"n{ntr}_k{k}_{metric}_T{T:g}_c{nc}"


@pytest.mark.parametrize("ntr,nte", [(300, 77), (1000, 257)])
def test_restatement_reproduces_recorded_accuracies(golden, ntr, nte):
    g = golden("knn")
    assert [ntr, nte] in g["sizes"].tolist() and os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "knn.npz")) < 200_000
    train, test = g[f"n{ntr}_train"].astype(np.float32), g[f"n{ntr}_test"].astype(np.float32)
    assert train.shape == (ntr, 128) and test.shape == (nte, 128)
    for metric in METRICS:
        for k in KS:
            assert R.ambiguous(test, train, k, metric, 1e-4).size == 0          # the generator's condition on the inputs
            vals, idx = R.topk(test, train, k, metric)
            for nc in CLASSES:
                lab, want = g[f"n{ntr}_train_labels_c{nc}"], g[f"n{ntr}_test_labels_c{nc}"]
                for T in TS:
                    pred, _, margin = R.vote(vals, idx, lab, T, nc)
                    assert margin.min() >= 1e-3
                    assert float((pred == want).sum()) / nte == float(g[case_key(ntr, k, metric, T, nc)]), (metric, k, nc, T)


def test_restatement_orders_ties_by_index_and_skips():
    L = np.zeros((6, 128))
    L[:, 0] = [1, 2, 2, 3, 2, 1]
    Q = np.zeros((2, 128))
    Q[:, 0] = [1, 2]
    vals, idx = R.topk(Q, L, 4, "dot")
    assert idx.tolist() == [[3, 1, 2, 4], [3, 1, 2, 4]] and vals[1].tolist() == [6, 4, 4, 4]
    vals, idx = R.topk(Q, L, 3, "euclidean", skip=np.array([0, -1]))
    assert idx.tolist() == [[5, 1, 2], [1, 2, 4]] and vals.tolist() == [[0, 1, 1], [0, 0, 0]]
    assert R.ambiguous(Q, L, 1, "dot", 1e-5).tolist() == [] and R.ambiguous(Q, L, 2, "dot", 1e-5).tolist() == [0, 1]
    assert R.ambiguous(Q, L, 4, "dot", 1e-5).tolist() == [0, 1]                 # entries 1, 2 tie with the 4th
    pred, sums, _ = R.vote(np.zeros((1, 4)), np.array([[0, 1, 2, 3]]), np.array([1, 0, 1, 0], dtype=np.uint8), 1.0, 2)
    assert pred.tolist() == [0] and sums.tolist() == [[2.0, 2.0]]               # a tie goes to the lowest class


def test_host_only_queries_need_no_gpu():
    from madrigal_amd import _lib, ops
    L = _lib.lib()
    assert L.mdg_abi_version() >= 21
    assert L.mdg_knn_max_k() == 32 == ops.knn_max_k()
    for nq, nl in ((1, 1), (77, 300), (77, 20000), (4096, 100352), (65535, 129), (65536, 100352), (100352, 100352), (128, 10 ** 7)):
        s = L.mdg_knn_default_segments(nq, nl)
        tiles, blocks = -(-nl // 128), -(-nq // 128)
        assert 1 <= s <= tiles, (nq, nl, s)
        assert s == 1 if blocks >= 512 else (s == tiles or blocks * s >= 512), (nq, nl, s)      # two workgroups for each of 256 CUs
        assert s == L.mdg_knn_default_segments(nq, nl) == ops.knn_default_segments(nq, nl)
    assert L.mdg_knn_default_segments(100352, 100352) == 1
    assert L.mdg_knn_default_segments(77, 20000) > 1
    assert L.mdg_knn_default_segments(4096, 100352) == 16
    sizes = [L.mdg_knn_topk_workspace_bytes(77, 1000, 20, s) for s in (1, 2, 4, 8)]
    assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] == 2 * 77 * 20 * 8
    assert L.mdg_knn_topk_workspace_bytes(77, 1000, 20, 64) == sizes[3]          # at most ceil(1000 / 128) = 8 segments are used
    assert L.mdg_knn_topk_workspace_bytes(100352, 100352, 32, 784) > 2 ** 32     # full width


def test_knn_ops_refuse_cpu_tensors():
    import torch
    from madrigal_amd import ops
    z = torch.zeros(4, 128)
    with pytest.raises(ValueError, match="GPU"):
        ops.knn_topk(z, z, 1)
    with pytest.raises(ValueError, match="GPU"):
        ops.knn_vote(torch.zeros(4, 1), torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), 1.0, 2)
