"""Feature-space HGT attention (``ops.hgt_attention_feat``, ``HGTConv.attend_in_feature_space``): the kernels at op level against
fp64 torch on one small graph that holds every path of the two kernels, and the two-conv encoder with the switch on against off."""
import pytest
import torch

from madrigal_amd import data, graph_plans, models as M, ops

pytestmark = pytest.mark.gpu

H, D, F, P = 4, 32, 128, 132
N_SRC, N_DST, R = 300, 8, 3
# in-edges of each destination per relation: none; 1; 2; 127 / 128 / 129 in ONE relation (one edge short of, at and past the
# 128-edge work item); ~300 over all three; a hub of 2 200 edges, 17 work items of them in one relation (> HGT_COOP = 16: the
# cooperative merge of a relation)
DEGREES = [(0, 0, 0), (0, 1, 0), (1, 0, 1), (127, 0, 0), (0, 128, 0), (0, 0, 129), (90, 110, 100), (2100, 60, 40)]


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N_SRC, F, generator=g)                                   # fp32 rows, exact in fp64
    q = torch.randn(N_DST, F, generator=g)
    K = 0.3 * torch.randn(R, H, D, F, dtype=torch.float64, generator=g)      # logits q . (K x + kappa): std ~ 20, spread about +-60
    kap = torch.randn(R, H, D, dtype=torch.float64, generator=g)
    V = 0.1 * torch.randn(R, H, D, F, dtype=torch.float64, generator=g)
    nu = torch.randn(R, H, D, dtype=torch.float64, generator=g)
    edges = []
    for r in range(R):
        src, dst = [], []
        for d, deg in enumerate(DEGREES):
            src.append(torch.randint(0, N_SRC, (deg[r],), generator=g))
            dst.append(torch.full((deg[r],), d, dtype=torch.int64))
        src, dst = torch.cat(src), torch.cat(dst)
        perm = torch.randperm(src.numel(), generator=g)                       # edge lists arrive unsorted
        edges.append((src[perm], dst[perm]))
    xd, qd = x.double(), q.double().view(N_DST, H, D)
    kp = torch.einsum("rhdf,sf->rshd", K, xd) + kap.unsqueeze(1)             # [R, S, H, D]
    vp = torch.einsum("rhdf,sf->rshd", V, xd) + nu.unsqueeze(1)
    # fp64 reference: softmax over ALL in-edges of a destination, weighted v' sum, erf GELU
    ref = torch.zeros(N_DST, H, D, dtype=torch.float64)
    spread = 0.0
    for d in range(N_DST):
        lg, vv = [], []
        for r, (src, dst) in enumerate(edges):
            s = src[dst == d]
            lg.append(torch.einsum("hd,shd->sh", qd[d], kp[r, s]))
            vv.append(vp[r, s])
        lg, vv = torch.cat(lg), torch.cat(vv)
        if lg.numel():
            spread = max(spread, float(lg.max() - lg.min()))
            ref[d] = torch.einsum("sh,shd->hd", torch.softmax(lg, 0), vv)
    ref = torch.nn.functional.gelu(ref.view(N_DST, F))
    # destination-side block and the V~ block, fp64
    ut = torch.zeros(N_DST, R, H, P, dtype=torch.float64)
    ut[..., :F] = torch.einsum("rhdf,nhd->nrhf", K, qd)
    ut[..., F] = torch.einsum("rhd,nhd->nrh", kap, qd)
    Wv = torch.zeros(F, R, H, P, dtype=torch.float64)
    for h in range(H):
        Wv[h * D:(h + 1) * D, :, h, :F] = V[:, h].permute(1, 0, 2)
        Wv[h * D:(h + 1) * D, :, h, F] = nu[:, h].t()
    return dict(x=x, q=q, kp=kp, vp=vp, edges=edges, ref=ref, ut=ut, Wv=Wv.view(F, -1), spread=spread)


def _run_feat(case):
    dev = torch.device("cuda")
    plan = graph_plans.hgt_feat_plan(case["edges"], N_DST, N_SRC, dev)
    st = ops.hgt_attention_feat(case["x"].to(dev), case["ut"].float().to(dev).contiguous(), plan)
    return plan, st


def test_plan_items_are_relation_pure(case):
    plan, _ = _run_feat(case)
    n_items = sum((deg + 127) // 128 for degs in DEGREES for deg in degs)
    assert plan["item_dst"].numel() == n_items == int(plan["rel_ptr"][-1])
    assert plan["src"].dtype == torch.int32 and plan["item_rel"].dtype == torch.int32
    assert int((plan["item_end"] - plan["item_begin"]).max()) == 128 and int((plan["item_end"] - plan["item_begin"]).min()) >= 1
    cnt = (plan["rel_ptr"][1:] - plan["rel_ptr"][:-1]).view(N_DST, R).cpu()
    assert cnt.tolist() == [[(deg + 127) // 128 for deg in degs] for degs in DEGREES]
    assert int(plan["item_ptr"][-1] - plan["item_ptr"][-2]) == 19 and cnt[-1, 0] == 17 > 16
    key = plan["item_dst"] * R + plan["item_rel"]
    assert bool((key[1:] >= key[:-1]).all())


def test_op_against_fp64_and_the_projected_kernel(case):
    dev = torch.device("cuda")
    assert case["spread"] > 100.0                                            # the softmax range is exercised
    _, st = _run_feat(case)
    assert tuple(st.shape) == (R, N_DST, H, P)                               # relation-major
    st64 = st.double().cpu().permute(1, 0, 2, 3).contiguous()
    new = torch.nn.functional.gelu(st64.view(N_DST, -1) @ case["Wv"].t())
    # today's kernel on the same case: k' | v' rows of every (relation, source) in the projection layout of hgt_plan
    sizes = {"src": N_SRC, "dst": N_DST}
    ets = [("src", f"rel{r}", "dst") for r in range(R)]
    eid = {et: torch.stack(case["edges"][r]) for r, et in enumerate(ets)}
    hp = graph_plans.hgt_plan(eid, ets, sizes, dev)
    buf = torch.zeros(N_SRC, 1 + 2 * R, F, dtype=torch.float64)
    for r in range(R):
        buf[:, 1 + 2 * r] = case["kp"][r].reshape(N_SRC, F)
        buf[:, 2 + 2 * r] = case["vp"][r].reshape(N_SRC, F)
    old = ops.hgt_attention(case["q"].to(dev), buf.float().to(dev).view(-1, F), hp["per_dst"]["dst"], H, apply_gelu=True).double().cpu()
    ref = case["ref"]
    scale = float(ref.abs().max())
    err_new, err_old = float((new - ref).abs().max()) / scale, float((old - ref).abs().max()) / scale
    print(f"feature-space error {err_new:.3e}, projected-kernel error {err_old:.3e} (of the output scale {scale:.3f})")
    assert err_old < 1e-4                                                    # the yardstick itself is sound
    assert err_new <= 4.0 * err_old
    # structure of S~: zero rows where a relation or the destination has no edge, zero padding, masses summing to one
    s5 = st64.view(N_DST, R, H, P)
    for d, degs in enumerate(DEGREES):
        for r, deg in enumerate(degs):
            if deg == 0:
                assert float(s5[d, r].abs().max()) == 0.0
        if sum(degs):
            assert float((s5[d, :, :, F].sum(0) - 1.0).abs().max()) < 1e-5
    assert float(s5[..., F + 1:].abs().max()) == 0.0


def test_op_is_deterministic(case):
    _, a = _run_feat(case)
    _, b = _run_feat(case)
    assert torch.equal(a, b)


def test_op_refuses_what_it_was_not_built_for(case):
    dev = torch.device("cuda")
    plan = graph_plans.hgt_feat_plan(case["edges"], N_DST, N_SRC, dev)
    ut = case["ut"].float().to(dev).contiguous()
    with pytest.raises(ValueError):
        ops.hgt_attention_feat(case["x"][:-1].to(dev), ut, plan)             # fewer rows than the plan indexes
    with pytest.raises(ValueError):
        ops.hgt_attention_feat(case["x"].to(dev), ut[:, :2].contiguous(), plan)
    with pytest.raises(ValueError):
        graph_plans.hgt_feat_plan([(torch.tensor([N_SRC]), torch.tensor([0]))], N_DST, N_SRC, dev)


# ------------------------------------------------------------------------------------------ conv level

@pytest.fixture(scope="module")
def encoder():
    torch.manual_seed(7)
    kg = data.make_kg(60, seed=4, n_nodes=2000, n_edges=20000)
    m = M.HGT(128, 128, 128, 2, H, kg.metadata())
    with torch.no_grad():                                                    # non-trivial gates and relation priors
        for conv in m.convs:
            for p_ in conv.skip.values():
                p_.copy_(torch.randn(1) * 0.5)
            for p_ in conv.p_rel.values():
                p_.copy_(1.0 + 0.3 * torch.randn(1, H))
    return m.cuda().eval(), kg.to("cuda")


def _drug_rows(encoder, monkeypatch, precision, on, min_edges=0):
    m, kg = encoder
    calls = []
    real = ops.hgt_attention_feat
    monkeypatch.setattr(ops, "hgt_attention_feat", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for conv in m.convs:
        monkeypatch.setattr(conv, "attend_in_feature_space", on, raising=False)
        monkeypatch.setattr(conv, "feature_space_min_edges_per_row", min_edges, raising=False)
    with torch.no_grad(), M.precision(precision):
        out = m(kg.x_dict, kg.edge_index_dict, only_types=["drug"])["drug"]
    return out.clone(), len(calls)


@pytest.mark.parametrize("precision,bound", [("f32", 1e-5), ("bf16x3", 1e-4)])
def test_conv_switch_on_against_off(encoder, monkeypatch, precision, bound):
    off, n_off = _drug_rows(encoder, monkeypatch, precision, on=False)
    on, n_on = _drug_rows(encoder, monkeypatch, precision, on=True)
    assert (n_off, n_on) == (0, 1)                                           # the last conv only: conv 0 has several destination types
    scale = float(off.abs().max())
    err = float((on - off).abs().max()) / scale
    print(f"{precision}: switch on against off {err:.3e} of the output scale {scale:.3f}")
    assert err <= bound
    again, _ = _drug_rows(encoder, monkeypatch, precision, on=True)
    assert torch.equal(on, again)


def test_guard_miss_keeps_todays_bits(encoder, monkeypatch):
    off, _ = _drug_rows(encoder, monkeypatch, "bf16x3", on=False)
    sparse, n_sparse = _drug_rows(encoder, monkeypatch, "bf16x3", on=True, min_edges=64)      # the size rule: too few edges per row here
    assert n_sparse == 0 and torch.equal(off, sparse)
    off16, _ = _drug_rows(encoder, monkeypatch, "bf16", on=False)
    on16, n16 = _drug_rows(encoder, monkeypatch, "bf16", on=True)                             # the 16-bit mode keeps its mirror
    assert n16 == 0 and torch.equal(off16, on16)
