"""CPU checks of the GeomCA feature: the fp64 restatement tests/geomca_ref.py against the values recorded from the reference's own
GeomCA class (tests/golden/geomca.npz, scripts/gen_geomca_golden.py), the two tie rules, and the host-only queries of
csrc/geomca.hip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geomca_ref as G                                           # noqa: E402

MARGIN = 2.0 ** -13
SCORE_KEYS = ("precision", "recall", "network_consistency", "network_quality")


def golden_case(g, ci):
    """(R fp32, E fp32, gamma, percentile, record dict) of case ``ci``."""
    rec = {k[len(f"c{ci}_"):]: g[k] for k in g.files if k.startswith(f"c{ci}_")}
    return rec["R"].astype(np.float32), rec["E"].astype(np.float32), float(rec["gamma"]), float(rec["percentile"]), rec


def line(coords):
    X = np.zeros((len(coords), 128), dtype=np.float32)
    X[:, 0] = coords
    return X


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_restatement_reproduces_the_recorded_reference(golden, ci):
    g = golden("geomca")
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "geomca.npz")) < 300_000
    assert g["cases"].shape == (3, 3) and len({tuple(c[:2]) for c in g["cases"].tolist()}) >= 2 and (g["cases"][:, 2] < 1).any()
    R, E, gamma, pct, rec = golden_case(g, ci)
    assert R.shape == (int(g["cases"][ci, 0]), 128) and E.shape == (int(g["cases"][ci, 1]), 128) and R.shape[0] != E.shape[0]
    assert (R * 64 == np.round(R * 64)).all() and np.abs(R).max() <= 2 and (E * 64 == np.round(E * 64)).all() and np.abs(E).max() <= 2
    eps = float(rec["epsilon"])
    V = np.concatenate([R, E])
    dd = G.d2(V, V)
    assert (dd * 4096 == np.round(dd * 4096)).all() and dd.max() < 2 ** 10       # fp32 arithmetic on these inputs is exact
    for thr in ((eps * gamma) ** 2, eps ** 2):
        assert np.abs(dd - thr).min() >= MARGIN                                    # the generator's condition on the inputs
    for thr in (G.threshold(eps * gamma), G.threshold(eps)):                      # ... which the float32 rounding leaves standing
        assert np.abs(dd - thr).min() >= MARGIN * (1 - 1e-4)
    comp, net, par = G.geomca(R, E, Rdist_percentile=pct, gamma=gamma)
    assert abs(par["epsilon"] - eps) <= 1e-12 * eps
    assert par["sparseR_index"].tolist() == rec["sparseR_index"].tolist()
    assert par["sparseE_index"].tolist() == rec["sparseE_index"].tolist()
    assert np.array_equal(np.array(G.comp_table(comp)), rec["components"])
    assert [net[k] for k in SCORE_KEYS] == rec["scores"].tolist()
    assert sum(v["num_edges"] for v in comp.values()) == int(rec["edges"])
    sizes = [len(v["Ridx"]) + len(v["Eidx"]) for _, v in sorted(comp.items())]
    firsts = [min(list(v["Ridx"]) + list(v["Eidx"] + par["num_R_points"])) for _, v in sorted(comp.items())]
    assert all(a > b or (a == b and fa < fb) for a, b, fa, fb in zip(sizes, sizes[1:], firsts, firsts[1:]))


def test_tie_rules_on_a_line_at_unit_spacing():
    X = line([0, 1, 2, 3, 4])
    kept = G.sparsify(X, 2.0)                                                    # delta^2 = 4
    assert kept.tolist() == [0, 2, 4]                                            # d2 == delta^2 does not drop
    A = G.adjacency(X[kept], 2.0)                                                # epsilon^2 = 4
    assert sorted(map(tuple, np.argwhere(np.triu(A)).tolist())) == [(0, 1), (1, 2)]      # d2 == epsilon^2 links {0,2}, {2,4}
    label, same, cross, _ = G.components(X[kept], 2, 2.0)
    assert label.tolist() == [0, 0, 0] and same.tolist() == [1, 1, 0] and cross.tolist() == [0, 1, 1]
    assert G.sparsify(X, np.nextafter(2.0, 3.0) * (1 + 1e-6)).tolist() == [0, 3]
    assert not G.adjacency(X[kept], 2.0 * (1 - 1e-6)).any()


def test_a_dropped_point_does_not_drop_its_successor():
    X = line([0, 1.5, 3, 4.5, 6])
    assert G.sparsify(X, 2.0).tolist() == [0, 2, 4]                              # 1 is within delta of 2, but 1 was dropped by 0
    assert G.sparsify(line([0, 1.5, 1.5, 3]), 2.0).tolist() == [0, 3]


def test_scores_order_and_thresholds():
    # vertices: R = {0, 1, 2}, E = {3, 4}; components {0, 3, 4} (two cross edges, one E edge), {1}, {2}
    V = line([0, 10, 20, 0.5, 1.0])
    label, same, cross, Gr = G.components(V, 3, 0.6)
    assert label.tolist() == [0, 1, 2, 0, 0] and same.tolist() == [0, 0, 0, 1, 1] and cross.tolist() == [1, 0, 0, 1, 0]
    comp, net = G.scores(Gr, 3, 2)
    assert G.comp_table(comp) == [(1, 2, 1 - 1 / 3, 0.5), (1, 0, 0.0, 0.0), (1, 0, 0.0, 0.0)]
    assert comp[1]["Ridx"].tolist() == [1] and comp[2]["Ridx"].tolist() == [2] and comp[0]["Eidx"].tolist() == [0, 1]
    assert net["precision"] == 1.0 and net["recall"] == 1 / 3 and net["network_consistency"] == 0.8 and net["network_quality"] == 0.5
    assert G.scores(Gr, 3, 2, quality_threshold=0.5)[1]["precision"] == 0.0


def test_host_only_queries_need_no_gpu():
    from madrigal_amd import _lib, ops
    L = _lib.lib()
    assert L.mdg_abi_version() >= 22
    C = L.mdg_geomca_default_chunk()
    assert C == ops.geomca_default_chunk() and 128 <= C <= 1024 and C % 128 == 0
    for nrow, ncol in ((1, 1), (128, 100352), (512, 4096), (100352, 100352), (4096, 129)):
        s = L.mdg_geomca_default_segments(nrow, ncol)
        tiles, blocks = -(-ncol // 128), -(-nrow // 128)
        assert 1 <= s <= tiles and s == ops.geomca_default_segments(nrow, ncol)
        assert s == 1 if blocks >= 512 else (s == tiles or blocks * s >= 512)
    per_row = 128 * 4 + 4
    small, big = L.mdg_geomca_sparsify_workspace_bytes(1000, C), L.mdg_geomca_sparsify_workspace_bytes(100352, C)
    assert small >= 1000 * per_row + C * C // 8 and big - small >= (100352 - 1000) * per_row - 1024     # O(n) + the chunk's bits
    assert big < 100352 * per_row + C * C // 8 + C * 4 + 4096
    assert L.mdg_geomca_sparsify_workspace_bytes(1000, 100) == 0                  # not a chunk size
    assert 2 * 4 * 1000 <= L.mdg_geomca_components_workspace_bytes(1000) <= 2 * 4 * 1000 + 1024
    assert L.mdg_geomca_distance_select_workspace_bytes() == (2 * 2048 + 1) * 8


def test_geomca_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from madrigal_amd import ops
    z = torch.zeros(4, 128)
    ids = torch.zeros(4, dtype=torch.int64)
    for fn in (lambda: ops.geomca_sparsify(z, 1.0), lambda: ops.geomca_components(z, 2, 1.0),
               lambda: ops.geomca_distance_select(z, z, ids, ids, 5.0), lambda: ops.geomca_prep(z)):
        with pytest.raises(ValueError, match="GPU"):
            fn()
