"""On-device batch collation (madrigal_amd/collate.py, csrc/collate.hip) against a per-drug host gather from the original,
unsorted batch (tests/collate_ref.py): a store of 64 synthetic drugs plus a 1-atom molecule without edges and a 300-atom
molecule, with unit and with non-unit edge weights.  Everything is compared with torch.equal: the kernels only move data."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collate_ref as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 23
_rng = np.random.default_rng(SEED)
ID_LISTS = {
    "first": [0], "last_of_64": [63], "one_atom": [64], "atoms_300": [65],
    "descending_7": [65, 64, 50, 41, 30, 12, 3],
    "all_66": list(range(66)),
    "dup_130": _rng.integers(0, 66, size=130).tolist(),
    "dup_2500": _rng.integers(0, 66, size=2500).tolist(),          # three workgroups of the offset scan (1024 ids each)
}


@pytest.fixture(scope="module")
def env():
    from madrigal_amd import data as D
    from madrigal_amd.collate import DeviceCollator, DrugStore
    out = {}
    for weighted in (False, True):
        batch, bkg = R.make_store_batch(SEED, weighted=weighted)
        kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
        store = DrugStore.from_batch(D.batch_to(batch, "cuda"), kgc)
        out[weighted] = dict(batch=batch, kgc=kgc, store=store, collate=DeviceCollator(store), host=R.HostCollator(batch, kgc), ref={})
    return out


def _host(e, name):
    """The host gather of one id list: computed once, shared, never modified."""
    if name not in e["ref"]:
        e["ref"][name] = e["host"]([torch.tensor(ID_LISTS[name], dtype=torch.int64)])
    return e["ref"][name]


def _check(e, name):
    from madrigal_amd.data import CELL_LINES, MoleculeBatch
    from madrigal_amd.graph_plans import molecule_plan
    ids = torch.tensor(ID_LISTS[name], dtype=torch.int64)
    B = ids.numel()
    got_ids, (mols, kg, cv, tx) = e["collate"]([ids])
    _, (hm, _, hcv, htx) = _host(e, name)
    assert got_ids.is_cuda and got_ids.dtype == torch.int64 and torch.equal(got_ids.cpu(), ids)
    assert kg is e["store"].kg and kg is e["kgc"]
    assert mols.batch_size == B and mols.node_feature.shape == (hm.num_node, 67) and mols.edge_list.shape == (hm.num_edge, 3)
    assert torch.equal(mols.node_feature.cpu(), hm.node_feature)
    assert mols.node2graph.dtype == torch.int64 and torch.equal(mols.node2graph.cpu(), hm.node2graph)
    assert cv.shape == (B, 559) and cv.is_contiguous() and torch.equal(cv.cpu(), hcv)
    assert list(tx) == CELL_LINES
    base = tx[CELL_LINES[0]]["sigs"].data_ptr()
    for k, c in enumerate(CELL_LINES):
        v, h = tx[c], htx[c]
        assert v["sigs"].shape == (B, 978) and v["sigs"].is_contiguous() and v["sigs"].data_ptr() == base + k * B * 978 * 4     # one [16,B,978] buffer
        assert torch.equal(v["sigs"].cpu(), h["sigs"]), c
        assert v["dosages"].shape == (B,) and torch.equal(v["dosages"].cpu(), h["dosages"]), c
        assert torch.equal(v["drugs"].cpu(), h["drugs"]), c
        assert isinstance(v["cell_lines"], np.ndarray) and np.array_equal(v["cell_lines"], h["cell_lines"]), c
    el, ef, ew = R.sorted_by_destination(hm)
    assert mols.edge_list.dtype == torch.int64 and torch.equal(mols.edge_list.cpu(), el)
    assert torch.equal(mols.edge_feature.cpu(), ef) and torch.equal(mols.edge_weight.cpu(), ew)
    plan = mols._mdg_plan
    R.assert_plans_equal(plan, molecule_plan(hm.to("cuda")))
    bare = MoleculeBatch(mols.node_feature, mols.edge_list, mols.edge_feature, mols.node2graph, mols.batch_size, mols.edge_weight)
    R.assert_plans_equal(plan, molecule_plan(bare))
    assert molecule_plan(mols) is plan                                        # the encoder finds the attached plan
    assert mols.to("cuda") is mols and mols.to(torch.device("cuda", 0))._mdg_plan is plan
    return plan


@pytest.mark.parametrize("name", list(ID_LISTS))
def test_collated_batch_equals_host_gather(env, name):
    plan = _check(env[False], name)
    assert plan["w"] is None                                                  # every weight of the store is 1


@pytest.mark.parametrize("name", ["one_atom", "descending_7", "all_66", "dup_2500"])
def test_collated_batch_equals_host_gather_weighted(env, name):
    plan = _check(env[True], name)
    if name == "one_atom":
        assert plan["w"] is None and plan["col"].numel() == 0                 # no edges: molecule_plan reports no weights either
    else:
        assert plan["w"] is not None and plan["w"].shape == (plan["col"].shape[0],)


def test_sparse_ids_and_id_list_forms(env):
    """Drug ids that are not row numbers: the id -> row table decides; every accepted spelling of the id list gives one batch."""
    from madrigal_amd import data as D
    from madrigal_amd.collate import DeviceCollator, DrugStore
    e = env[False]
    drugs = torch.arange(66) * 3 + 2
    drugs[[0, 65]] = drugs[[65, 0]]
    store = DrugStore.from_batch(D.batch_to(dict(e["batch"], drugs=drugs), "cuda"), e["kgc"])
    collate = DeviceCollator(store)
    rows = torch.tensor([65, 0, 17, 17, 64, 3])
    ids = drugs[rows]
    _, (hm, _, hcv, htx) = e["host"]([rows])
    forms = [[ids], [ids.numpy()], ids.tolist(), [(int(i),) for i in ids], ids, ids.cuda(), [ids.int().cuda()]]
    for f in forms:
        got_ids, (mols, _, cv, tx) = collate(f)
        assert torch.equal(got_ids.cpu(), ids)
        assert torch.equal(mols.node_feature.cpu(), hm.node_feature) and torch.equal(mols.node2graph.cpu(), hm.node2graph)
        assert torch.equal(mols.edge_list.cpu(), R.sorted_by_destination(hm)[0])
        assert torch.equal(cv.cpu(), hcv) and torch.equal(tx["pc3"]["sigs"].cpu(), htx["pc3"]["sigs"])
        assert torch.equal(tx["pc3"]["drugs"].cpu(), ids)
    for bad in ([3], [0], [int(drugs.max()) + 1], [2, 5, 1]):                  # inside the table but absent, and outside it
        with pytest.raises(ValueError, match="not in the store"):
            collate([torch.tensor(bad)])


def test_encoder_and_loss_bit_equal_in_f32(env):
    """Eval mode, f32 arithmetic: the encoder's output and one SimCLR_NovelDDI forward loss on the collated batch are bit-equal
    to those on the host-gathered batch (same plan, same rows; the edge order inside the batch object is all that differs)."""
    from madrigal_amd import evaluate as E, models as M
    from oracle.params import det_state_dict
    from test_pretrain_gpu import _build
    e = env[False]
    model = _build(M, e["kgc"]["data"], False, True, mlp_dim=256, T=0.5)
    sd = model.state_dict()
    model.load_state_dict(det_state_dict(SEED, {k: tuple(v.shape) for k, v in sd.items()}))
    model = model.cuda().eval()
    e["model"] = model
    name = "dup_130"
    ids = torch.tensor(ID_LISTS[name], dtype=torch.int64)
    dev_ids, dev_data = e["collate"]([ids])
    _, host_data = _host(e, name)
    host_data = E._to(host_data, "cuda")
    masks = e["batch"]["masks"][ids].cuda()
    m1, m2 = E._subset_masks([0], ids.numel(), 19, "cuda"), E._subset_masks([2], ids.numel(), 19, "cuda")
    outs = []
    with torch.no_grad(), M.precision("f32"):
        for i, data in ((dev_ids, dev_data), (ids.cuda(), host_data)):
            raw = model.base_encoder(i, masks, *data, raw_encoder_output=True)
            _, _, (_, _, loss) = model(i, m1, m2, None, data, None, None)
            outs.append((raw, loss))
    assert outs[0][0].shape == outs[1][0].shape and outs[0][0].shape[0] >= ids.numel() and outs[0][0].shape[1] == 128
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and bool(torch.isfinite(outs[0][1]))


def test_evaluate_pretrain_subsets_same_values(env):
    from madrigal_amd import evaluate as E, models as M
    from oracle.params import det_state_dict
    from test_pretrain_gpu import _build
    e = env[False]
    model = e.get("model")
    if model is None:
        model = _build(M, e["kgc"]["data"], False, True, mlp_dim=256, T=0.5)
        sd = model.state_dict()
        model.load_state_dict(det_state_dict(SEED, {k: tuple(v.shape) for k, v in sd.items()}))
        model = model.cuda().eval()
    drugs, masks = np.arange(66), e["batch"]["masks"].numpy().astype(np.int64)
    hard = torch.from_numpy(np.random.default_rng(SEED).random((66, 66)) < 0.02)
    hard.fill_diagonal_(False)
    vals = []
    for collator in (e["collate"], e["host"]):
        np.random.seed(5)
        vals.append(E.evaluate_pretrain_subsets(model, drugs, masks, hard, collator, [0], [2], "cuda", max_drugs=1000))
    got, want = vals
    assert len(got) == len(want) == 14
    assert list(got[:12]) == list(want[:12])
    assert torch.equal(got[12], want[12]) and torch.equal(got[13], want[13])


def test_every_call_returns_new_tensors(env):
    e = env[True]
    ids = torch.tensor(ID_LISTS["descending_7"], dtype=torch.int64)
    a_ids, (am, akg, acv, atx) = e["collate"]([ids])
    b_ids, (bm, bkg, bcv, btx) = e["collate"]([ids])
    assert akg is bkg and am is not bm and atx is not btx and am._mdg_plan is not bm._mdg_plan
    pairs = [(acv, bcv), (a_ids, b_ids)] + [(getattr(am, k), getattr(bm, k)) for k in ("node_feature", "edge_list", "edge_feature", "node2graph", "edge_weight")]
    pairs += [(am._mdg_plan[k], bm._mdg_plan[k]) for k in ("rowptr", "col", "w", "edge_feat_aug", "graph_rowptr")]
    pairs += [(atx[c][k], btx[c][k]) for c in atx for k in ("sigs", "dosages")]
    for x, y in pairs:
        assert x is not y and x.data_ptr() != y.data_ptr() and torch.equal(x, y)
    assert all(atx[c] is not btx[c] and atx[c]["cell_lines"] is not btx[c]["cell_lines"] for c in atx)


def test_bad_id_lists_raise(env):
    collate = env[False]["collate"]
    for bad in ([torch.tensor([66])], [torch.tensor([-1])], [torch.tensor([3, 10 ** 12])], [3, 700, 2], [torch.arange(2500) % 67],
                [], [torch.zeros(0, dtype=torch.int64)], [np.zeros(0, dtype=np.int64)],
                [torch.tensor([1.0, 2.0])], [np.array([1.0, 2.0])], torch.tensor([1.0]).cuda(),
                [torch.tensor([[1, 2], [3, 4]])], torch.tensor([[1, 2]]).cuda()):
        with pytest.raises(ValueError):
            collate(bad)
    with pytest.raises(ValueError, match="2 of 4 drug ids are not in the store .*id 99 at position 1"):
        collate([5, 99, 6, -4])
    ids, _ = collate([5, 6])                                                   # a refused call leaves the collator usable
    assert ids.tolist() == [5, 6]


def test_store_batch_is_the_finetune_side_dict(env):
    e = env[False]
    store, batch = e["store"], e["batch"]
    ids = torch.tensor([65, 3, 3, 40, 64])
    b = store.batch(ids)
    assert sorted(b) == ["cv", "drugs", "masks", "strs", "tx"]
    assert b["masks"].dtype == torch.bool and torch.equal(b["masks"].cpu(), batch["masks"][ids])
    assert torch.equal(b["drugs"].cpu(), ids) and torch.equal(b["cv"].cpu(), batch["cv"][ids]) and b["strs"].batch_size == 5
    assert torch.equal(b["tx"]["a375"]["sigs"].cpu(), batch["tx"]["a375"]["sigs"][ids])


def test_generate_embeddings_on_a_subset(env):
    """``store.batch(ids)`` feeds the finetune-side entry points: the embeddings of a subset equal those of the host-built dict."""
    from madrigal_amd import configs, data as D
    from madrigal_amd.pipeline import generate_embeddings
    from oracle.params import det_state_dict
    e = env[False]
    model = configs.build_model("drugbank163", e["kgc"]["data"], 5)
    sd = model.state_dict()
    skip = [k for k in sd if k.endswith("pos_encoder.pe")]
    model.load_state_dict({**sd, **det_state_dict(SEED, {k: tuple(v.shape) for k, v in sd.items()}, skip)})
    model = model.cuda().eval()
    name = "descending_7"
    ids = torch.tensor(ID_LISTS[name], dtype=torch.int64)
    _, (hm, _, hcv, htx) = _host(e, name)
    host_batch = D.batch_to({"drugs": ids, "strs": hm, "cv": hcv, "tx": htx, "masks": e["batch"]["masks"][ids]}, "cuda")
    filler = torch.randn(66, 128, generator=torch.Generator().manual_seed(1)).cuda()
    z_dev = generate_embeddings(model, e["store"].batch(ids), e["kgc"], kg_filler=filler)
    z_host = generate_embeddings(model, host_batch, e["kgc"], kg_filler=filler)
    assert z_dev.shape == (7, 128) and bool(torch.isfinite(z_dev).all()) and torch.equal(z_dev, z_host)
