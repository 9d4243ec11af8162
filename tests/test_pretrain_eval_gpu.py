"""On-device pretraining evaluation (csrc/retrieval.hip, ops.pair_match_counts / pair_uniformity, madrigal_amd.retrieval,
evaluate.evaluate_pretrain_subsets / evaluate_pt) against the reference's recorded outputs and the fp64 restatement
tests/pretrain_eval_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pretrain_eval_ref as R                                    # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = ("cos_row", "cos_col", "same_x", "same_y", "dist_row", "dist_col")


def _views(n, seed, sigma=2.0, scale=1.0):
    rng = np.random.default_rng([seed, 77])
    X = rng.standard_normal((n, 128)) * scale
    Y = X + sigma * scale * rng.standard_normal((n, 128))
    return X.astype(np.float32), Y.astype(np.float32)


def _gpu_counts(X, Y):
    from madrigal_amd import ops
    out = ops.pair_match_counts(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_counts(got, ref):
    for k in COUNTS:
        assert got[k].dtype == np.int32
        d = np.abs(got[k].astype(np.int64) - ref[k])
        assert (d <= ref["amb_" + k]).all(), (k, np.flatnonzero(d > ref["amb_" + k])[:5])


# ---------------------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("n", [20, 257, 1000])
def test_dropins_reproduce_reference_outputs(golden, n):
    from madrigal_amd import retrieval as RT
    g = golden("pretrain_eval")
    X = torch.from_numpy(g[f"n{n}_x"].astype(np.float32)).cuda()
    Y = torch.from_numpy(g[f"n{n}_y"].astype(np.float32)).cuda()
    for k, want in zip((1, 5, 20), g[f"n{n}_acc_k1_5_20"]):
        acc, t20, t5, t1, ir, ic = RT.get_inst_dist_topk_accuracy(X, Y, k, "cosine")
        assert acc == want and ir is None and ic is None
        assert [t20, t5, t1] == list(g[f"n{n}_stacked_top20_5_1"])
    for (r, e), key in (((X, Y), "xy"), ((Y, X), "yx")):
        mu, std = RT.foscttm(r, e)
        assert mu.dim() == 0 and mu.device.type == "cpu"
        np.testing.assert_allclose([float(mu), float(std)], g[f"n{n}_foscttm_{key}"], rtol=0, atol=1e-6)
    u = [float(RT.uniform_loss(X)), float(RT.uniform_loss(Y.cpu()))]          # CPU input goes to the current device
    np.testing.assert_allclose(u, g[f"n{n}_uniform_x_y"], rtol=1e-5)
    np.testing.assert_allclose(float(RT.alignment_loss(X, Y)), g[f"n{n}_alignment"][0], rtol=1e-5)


# ------------------------------------------------------------------------------------------- 2. counts against fp64
@pytest.mark.parametrize("n", [1, 2, 20, 31, 33, 128, 1000, 4099])
def test_counts_against_fp64(n):
    X, Y = _views(n, n, sigma=6.0 if n < 1000 else 1.5, scale=0.3 + (n % 7))
    got = _gpu_counts(X, Y)
    ref = R.counts(X, Y, rel=1e-5)
    _check_counts(got, ref)
    np.testing.assert_allclose(got["align"], ref["align"], rtol=1e-5, atol=1e-6)
    if n >= 1000:
        assert 0 < (got["cos_row"] == 0).mean() < 1                   # a case with hits and misses


# ------------------------------------------------------------------------------------------------- 3. ties and duplicates
def test_ties_count_as_hits_and_diagonal_by_index():
    X, Y = _views(64, 5)
    Y[7] = Y[3]                      # row 3's competitor 7 equals its true match, and row 7's competitor 3 equals its own
    Y[11] = X[9] * 2.0               # a strictly better competitor of row 9 (cosine 1, not a tie)
    got = _gpu_counts(X, Y)
    ref = R.counts(X, Y, rel=1e-6)
    _check_counts(got, ref)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    xh, yh = X64 / np.linalg.norm(X64, axis=1, keepdims=True), Y64 / np.linalg.norm(Y64, axis=1, keepdims=True)
    for i, tie in ((3, 7), (7, 3)):  # the tied competitor is not counted: the counts over the other columns, exactly
        others = [j for j in range(64) if j not in (i, tie)]
        assert got["cos_row"][i] == int((xh[i] @ yh[others].T > xh[i] @ yh[i]).sum())
        assert got["dist_row"][i] == int((np.linalg.norm(X64[i] - Y64[others], axis=1) < np.linalg.norm(X64[i] - Y64[i])).sum())
    assert got["cos_row"][9] >= 1
    # X == Y with duplicated rows: every competitor ties with or loses to the true match -> every count is 0
    Z = _views(64, 6)[0]
    Z[5] = Z[2]
    Z[40] = Z[2]
    got = _gpu_counts(Z, Z.copy())
    for k in COUNTS:
        assert (got[k] == 0).all(), k


# ------------------------------------------------------------------------------------------------------- 4. determinism
def test_bitwise_deterministic():
    from madrigal_amd import ops
    X, Y = (torch.from_numpy(a).cuda() for a in _views(1000, 3))
    a, b = ops.pair_match_counts(X, Y), ops.pair_match_counts(X, Y)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    u1, u2 = ops.pair_uniformity(X), ops.pair_uniformity(X)
    assert u1.view(torch.int32).item() == u2.view(torch.int32).item()


# -------------------------------------------------------------------------------------------------------------- 5. size
def _counts_fp64_torch(X, Y, rel=1e-5, chunk=1024):
    """R.counts in chunked torch fp64 on the GPU (the all-drugs size)."""
    X, Y = X.double(), Y.double()
    n = X.shape[0]
    xh, yh = X / X.norm(dim=1, keepdim=True), Y / Y.norm(dim=1, keepdim=True)
    c = (xh * yh).sum(1)
    nx2, ny2 = (X * X).sum(1), (Y * Y).sum(1)
    nx, ny = nx2.sqrt(), ny2.sqrt()
    d = nx2 + ny2 - 2 * (X * Y).sum(1)
    out = {k: torch.zeros(n, dtype=torch.int64, device=X.device) for k in COUNTS}
    out.update({"amb_" + k: torch.zeros(n, dtype=torch.int64, device=X.device) for k in COUNTS})
    ar = torch.arange(n, device=X.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        off = ar[lo:hi, None] != ar[None, :]
        C = xh[lo:hi] @ yh.T
        D2 = nx2[lo:hi, None] + ny2[None, :] - 2 * (X[lo:hi] @ Y.T)
        pair = (nx[lo:hi, None] + ny[None, :]) ** 2

        def put(name, diff, scale, dim, rows):
            cnt = ((diff > 0) & off).sum(dim)
            amb = ((diff.abs() <= rel * scale) & off).sum(dim)
            if rows:
                out[name][lo:hi] += cnt
                out["amb_" + name][lo:hi] += amb
            else:
                out[name] += cnt
                out["amb_" + name] += amb
        put("cos_row", C - c[lo:hi, None], 1.0, 1, True)
        put("cos_col", C - c[None, :], 1.0, 0, False)
        put("same_x", xh[lo:hi] @ xh.T - c[lo:hi, None], 1.0, 1, True)
        put("same_y", yh[lo:hi] @ yh.T - c[lo:hi, None], 1.0, 1, True)
        put("dist_row", d[lo:hi, None] - D2, pair + ((nx + ny) ** 2)[lo:hi, None], 1, True)
        put("dist_col", d[None, :] - D2, pair + ((nx + ny) ** 2)[None, :], 0, False)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_all_drugs_size():
    from madrigal_amd import ops
    n = 11607
    X, Y = (torch.from_numpy(a).cuda() for a in _views(n, 11, sigma=3.0, scale=0.1))
    got = {k: v.cpu().numpy() for k, v in ops.pair_match_counts(X, Y).items()}
    ref = _counts_fp64_torch(X, Y)
    _check_counts(got, ref)
    xh = X.double() / X.double().norm(dim=1, keepdim=True)
    s = torch.zeros((), dtype=torch.float64, device="cuda")
    for lo in range(0, n, 1024):
        G = xh[lo:lo + 1024] @ xh.T
        keep = torch.arange(lo, min(n, lo + 1024), device="cuda")[:, None] < torch.arange(n, device="cuda")[None, :]
        s += torch.exp(-2.0 * (2.0 - 2.0 * G).clamp_min(0))[keep].sum()
    want = float(torch.log(s / (n * (n - 1) / 2)))
    got_u = float(ops.pair_uniformity(X))
    assert abs(got_u - want) <= 1e-6 * abs(want), (got_u, want)


# ------------------------------------------------------------------------------- 6. evaluate_pretrain_subsets, 7. evaluate_pt
def _gather_mols(m, ids):
    from madrigal_amd.data import MoleculeBatch
    from madrigal_amd.pipeline import slice_molecules
    parts = [slice_molecules(m, int(i), int(i) + 1) for i in ids]
    nodes, el, ef, ew, n2g, base = [], [], [], [], [], 0
    for g, p in enumerate(parts):
        e = p.edge_list.clone()
        e[:, :2] += base
        nodes.append(p.node_feature)
        el.append(e)
        ef.append(p.edge_feature)
        ew.append(p.edge_weight)
        n2g.append(torch.full((p.num_node,), g, dtype=torch.int64, device=p.node2graph.device))
        base += p.num_node
    return MoleculeBatch(torch.cat(nodes), torch.cat(el), torch.cat(ef), torch.cat(n2g), len(parts), torch.cat(ew))


class Collator:
    """collator([drug_array]) -> (drugs, (mols, kg, cv, tx)): rows of one make_batch batch gathered by drug id."""

    def __init__(self, batch, kgc):
        self.b, self.kgc = batch, kgc

    def __call__(self, arg):
        ids = torch.as_tensor(np.asarray(arg[0]), dtype=torch.int64)
        b = self.b
        tx = {c: {"sigs": v["sigs"][ids], "drugs": v["drugs"][ids], "dosages": v["dosages"][ids],
                  "cell_lines": v["cell_lines"][ids.numpy()]} for c, v in b["tx"].items()}
        return ids, (_gather_mols(b["strs"], ids), self.kgc, b["cv"][ids], tx)


@pytest.fixture(scope="module")
def setup():
    from madrigal_amd import data as D, models as M
    from oracle.params import det_state_dict
    from test_pretrain_gpu import _build
    n, seed = 120, 31
    masks = D.make_masks(n, seed, p_kg=0.7, p_cv=0.7, p_tx=0.5)
    batch, bkg = D.make_batch(n, seed, kg_nodes=600, kg_edges=6000, masks=masks)
    model = _build(M, bkg["data"], False, True, mlp_dim=256, T=0.5)
    sd = model.state_dict()
    model.load_state_dict(det_state_dict(seed, {k: tuple(v.shape) for k, v in sd.items()}))
    model = model.cuda().eval()
    kgc = {"data": bkg["data"], "drug_index_map": bkg["drug_index_map"]}
    hard = torch.from_numpy(np.random.default_rng(seed).random((n, n)) < 0.02)
    hard.fill_diagonal_(False)
    return dict(model=model, drugs=np.arange(n), masks=masks.numpy().astype(np.int64), collator=Collator(batch, kgc), hard=hard)


def _restated(s, sub1, sub2, max_drugs, rng_seed):
    """The reference's sequence (evaluate.py:364-397) with the same model on the GPU, checked by the fp64 restatement."""
    from madrigal_amd import evaluate as E
    drugs, masks, model = s["drugs"], s["masks"], s["model"]
    cols = np.unique(sub1 + sub2)
    valid = drugs[(1 - masks[drugs, :][:, cols]).sum(axis=1) == len(cols)]
    np.random.seed(rng_seed)
    if max_drugs is not None:
        valid = np.random.choice(valid, size=min(max_drugs, valid.shape[0]), replace=False)
    state = np.random.get_state()
    ids = torch.from_numpy(valid.astype(np.int64))
    _, data = s["collator"]([ids])
    data = E._to(data, "cuda")
    m1 = E.from_indices_to_tensor(sub1, 19).repeat(len(ids), 1).bool().cuda()
    m2 = E.from_indices_to_tensor(sub2, 19).repeat(len(ids), 1).bool().cuda()
    with torch.no_grad():
        e1 = model.base_encoder(ids.cuda(), m1, *data, raw_encoder_output=model.raw_encoder_output)
        e2 = model.base_encoder(ids.cuda(), m2, *data, raw_encoder_output=model.raw_encoder_output)
        a1, a2, (_, _, loss) = model(ids.cuda(), m1, m2, s["hard"][ids][:, ids].cuda(), data, None, None)
    ce = R.counts(e1.cpu().numpy(), e2.cpu().numpy())
    ch = R.counts(a1.cpu().numpy(), a2.cpu().numpy())
    slack = [sum(int(c["amb_" + k].sum()) for k in COUNTS) / (2 * len(ids)) for c in (ce, ch)]
    return R.subset_tuple(ce, ch, float(loss)), state, slack, len(ids)


def _check_tuple(got, want, slack):
    assert len(got) == 14
    assert all(isinstance(v, float) for v in got[:12])
    for i, (g, w) in enumerate(zip(got[:12], want[:12])):
        assert abs(g - w) <= slack[(i // 3) % 2], (i, g, w)          # exact unless a comparison lies within 1e-5 of its threshold
    assert got[12].dim() == 0 and got[12].device.type == "cpu" and got[13].dim() == 0 and got[13].device.type == "cpu"
    assert abs(float(got[12]) - want[12]) <= 1e-5 * abs(want[12])
    assert abs(float(got[13]) - want[13]) <= 1e-6


@pytest.mark.parametrize("sub2,max_drugs", [([1], 40), ([2], 1000), ([13], None)])
def test_evaluate_pretrain_subsets(setup, sub2, max_drugs):
    from madrigal_amd import evaluate as E
    s = setup
    want, state, slack, n_used = _restated(s, [0], sub2, max_drugs, 5)
    np.random.seed(5)
    got = E.evaluate_pretrain_subsets(s["model"], s["drugs"], s["masks"], s["hard"], s["collator"], [0], sub2, "cuda",
                                      max_drugs=max_drugs)
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    _check_tuple(got, want, slack)
    valid = ((1 - s["masks"][:, [0] + sub2]).sum(1) == 2).sum()
    assert n_used == (valid if max_drugs is None else min(max_drugs, valid))


class FakeWandb:
    def __init__(self):
        self.calls = []

    def log(self, d, step=None):
        self.calls.append((dict(d), step))


def test_evaluate_pt_logs_the_reference_keys(setup):
    from madrigal_amd import evaluate as E
    s = setup
    split, epoch = "val", 7
    wb = FakeWandb()
    np.random.seed(9)
    all_embeds = E.evaluate_pt(s["model"], s["drugs"], s["masks"], None, s["collator"], split, wb, None, "cuda", epoch, max_drugs=30)
    pairs = ["str v kg", "str v cv", "str v tx_mcf7", "str v tx_pc3", "str v tx_vcap"]
    want_report = []
    for comp_pair in pairs:                                       # evaluate.py:266-277
        for side_type in ["one-side", "both-side"]:
            for embed_type in ["embed", "CL-head"]:
                for topk in ["top20", "top5", "top1"]:
                    want_report.append(f"{split} {topk} acc {comp_pair} {embed_type} {side_type} (cosine)")
        want_report += [f"{split} loss {comp_pair}", f"{split} foscttm mu {comp_pair}"]
    want_calls = [want_report] + [[f"{split} uniformity loss {m}"] for m in ["str", "kg", "cv", "tx_mcf7", "tx_pc3", "tx_vcap"]] + \
                 [[f"{split} alignment loss {p}"] for p in pairs]
    assert [list(d.keys()) for d, _ in wb.calls] == want_calls
    assert all(step == epoch for _, step in wb.calls)
    # the report's values: the same seeded sequence of evaluate_pretrain_subsets calls
    np.random.seed(9)
    for p, sub2 in zip(pairs, ([1], [2], [13], [15], [17])):
        vals = E.evaluate_pretrain_subsets(s["model"], s["drugs"], s["masks"], None, s["collator"], [0], sub2, "cuda", max_drugs=30)
        for key, v in zip(want_report[pairs.index(p) * 14:(pairs.index(p) + 1) * 14], vals):
            assert float(wb.calls[0][0][key]) == float(v), key
    assert sorted(all_embeds) == sorted(["0", "1", "2", "13", "15", "17"])
    for col, ent in all_embeds.items():
        valid = np.flatnonzero(s["masks"][:, int(col)] == 0)
        assert isinstance(ent["drugs"], np.ndarray) and np.array_equal(ent["drugs"], valid)
        assert ent["embeds"].device.type == "cpu" and tuple(ent["embeds"].shape) == (len(valid), 128)
        u = wb.calls[1 + ["0", "1", "2", "13", "15", "17"].index(col)][0]
        assert abs(float(next(iter(u.values()))) - R.uniform_loss(ent["embeds"].numpy())) <= 1e-5 * 4
    e0 = all_embeds["0"]
    for i, col in enumerate(["1", "2", "13", "15", "17"]):
        e = all_embeds[col]
        shared = np.intersect1d(e0["drugs"], e["drugs"])
        a = e0["embeds"].numpy()[np.searchsorted(e0["drugs"], shared)]
        b = e["embeds"].numpy()[np.searchsorted(e["drugs"], shared)]
        got = float(next(iter(wb.calls[7 + i][0].values())))
        assert abs(got - R.alignment_loss(a, b)) <= 1e-5 * abs(R.alignment_loss(a, b)) + 1e-7


# ------------------------------------------------------------------------------------------------------------ 8. errors
def test_errors(setup):
    from madrigal_amd import evaluate as E, ops, retrieval as RT
    X, Y = (torch.from_numpy(a).cuda() for a in _views(32, 1))
    with pytest.raises(ValueError, match="GPU"):
        ops.pair_match_counts(X.cpu(), Y.cpu())
    with pytest.raises(ValueError, match="GPU"):
        ops.pair_uniformity(X.cpu())
    with pytest.raises(ValueError):
        ops.pair_match_counts(X.double(), Y.double())
    with pytest.raises(ValueError):
        ops.pair_match_counts(X[:, :64].contiguous(), Y[:, :64].contiguous())
    with pytest.raises(ValueError):
        ops.pair_uniformity(X[:, :64].contiguous())
    with pytest.raises(ValueError):
        ops.pair_match_counts(X, Y[:31])
    for bad in (float("nan"), float("inf")):
        Z = Y.clone()
        Z[4, 7] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            ops.pair_match_counts(X, Z)
        with pytest.raises(ValueError, match="NaN or infinite"):
            ops.pair_uniformity(Z)
    Z = X.clone()
    Z[3] = 0
    with pytest.raises(ValueError, match="zero-norm"):
        ops.pair_match_counts(Z, Y)
    with pytest.raises(ValueError, match="zero-norm"):
        ops.pair_uniformity(Z)
    with pytest.raises(NotImplementedError):
        RT.get_inst_dist_topk_accuracy(X, Y, 5, "euclidean")
    with pytest.raises(ValueError):
        RT.get_inst_dist_topk_accuracy(X[:10].contiguous(), Y[:10].contiguous(), 20)
    s = setup
    few = s["masks"].copy()
    few[20:, 13] = 1                                                # tx_mcf7 (column 13) only among drugs 12..19: fewer than 20
    few[:12, 13] = 1
    with pytest.raises(ValueError, match="at least 20"):
        E.evaluate_pretrain_subsets(s["model"], s["drugs"], few, None, s["collator"], [0], [13], "cuda")
