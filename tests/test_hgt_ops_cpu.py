"""The float64 references of hgt_ref.py checked without a GPU: the vectorised edge attention against a plain loop over the raw edges,
the whole reference pipeline against the oracle's one-conv forward, the share of the bound a float32 evaluation of each reference
uses (the condition test_hgt_ops_gpu.py's bound rests on), the ladder's work-item counts, and the destination-partitioned plans."""
import pytest
import torch

import hgt_ref as R


def _gp():
    from madrigal_amd import graph_plans
    return graph_plans


def _share(what, f32, f64):
    """float32 reference against float64 reference, as a share of the bound of the float64 one."""
    err, b = float((f32.double() - f64).abs().max()), R.bound(f64)
    print(f"[hgt-ref] {what}: float32 reference err {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
    assert err <= R.REF_SHARE * b, (what, err, b)
    return err / b


# ------------------------------------------------------------------------------------ 1. the attention reference against a loop
@pytest.mark.parametrize("t", R.DST_TYPES)
@pytest.mark.parametrize("heads", R.HEADS)
def test_edge_attention_ref_matches_the_edge_loop(heads, t):
    ei, plan = R.ladder(_gp())
    flat = R.ladder_flat(1.0).double()
    q_scale = 3.0 if heads == 4 else 1.0
    pre, m, den = R.edge_attention_ref(flat, plan, t, heads, q_scale)
    pre2, m2, den2 = R.edge_attention_loop(flat, plan, ei, t, heads, q_scale)
    assert float((pre - pre2).abs().max()) <= 1e-12
    assert torch.equal(m, m2)
    assert float(((den - den2).abs() / den2).max()) <= 1e-12
    empty = (plan["per_dst"][t]["rowptr"][1:] == plan["per_dst"][t]["rowptr"][:-1]).nonzero().flatten()
    assert (t == "a") == (empty.numel() == 0)
    for i in empty.tolist():                                   # a destination without edges: a zero row, max -inf, denominator 1e-16
        assert float(pre[i].abs().max()) == 0.0 and bool((m[i] == float("-inf")).all()) and bool((den[i] == 1e-16).all())


@pytest.mark.parametrize("heads", R.HEADS)
def test_edge_attention_ref_matches_the_merge_of_work_item_partials(heads):
    """The plan's work items (every edge of a destination in exactly one item, in order) merged as an online softmax give the
    plain formula: the 1-, 2-, 16-, 17- and 24-item destinations of `b` and the 2-item one of `c`."""
    _, plan = R.ladder(_gp())
    flat = R.ladder_flat(3.0 if heads == 4 else 1.0).double()
    for t in ("b", "c"):
        pre, m, den = R.edge_attention_ref(flat, plan, t, heads)
        pre2, m2, den2 = R.edge_attention_items(flat, plan, t, heads)
        assert float((pre - pre2).abs().max()) <= 1e-12 and torch.equal(m, m2)
        assert float(((den - den2).abs() / den2).max()) <= 1e-12


def test_query_scale_is_the_scaled_buffer():
    """The GPU tests hand the kernels a buffer whose query slots are already scaled and differentiate the reference in that buffer:
    the same function as ``q_scale`` on the unscaled one, its query-slot gradient ``q_scale`` times smaller."""
    _, plan = R.ladder(_gp())
    flat, heads, s = R.ladder_flat(1.0).double(), 4, 3.0
    douts = R.ladder_douts()
    outs, grad = R.attention_grads_ref(R.scale_queries(flat.view(-1), s).view(-1, 128), plan, heads, douts)
    leaf = flat.clone().requires_grad_(True)
    loss = 0.0
    for t in R.DST_TYPES:
        pre, m, den = R.edge_attention_ref(leaf, plan, t, heads, s)
        assert float((pre.detach() - outs[t][0]).abs().max()) <= 1e-12 and torch.equal(m, outs[t][1])
        loss = loss + (pre * douts[t].double()).sum()
    loss.backward()
    want = leaf.grad.view(404, 640).clone()
    want[:, :128] /= s
    assert float((grad.reshape(404, 640) - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


# ------------------------------------------------------------------------------------ 2. the reference pipeline against the oracle
@pytest.mark.parametrize("heads", R.HEADS)
def test_reference_pipeline_matches_the_oracle_conv(heads):
    from oracle import madrigal_oracle as O
    ei, plan = R.ladder(_gp())
    types, F = list(R.SIZES), 128
    meta = R.composite_meta(types, plan["used"], R.EDGE_TYPES, heads, F)
    p = {k: ([t.double() for t in v] if isinstance(v, list) else v.double())
         for k, v in R.composite_params(heads, F, n_types=3, n_edge_types=len(R.EDGE_TYPES), seed=70 + heads).items()}
    x = {t: R.rand((R.SIZES[t], F), 80 + i).double() for i, t in enumerate(types)}
    out_w = {t: R.rand((F, F), 90 + i, F ** -0.5).double() for i, t in enumerate(types)}
    out_b = {t: R.rand((F,), 95 + i, 0.3).double() for i, t in enumerate(types)}
    skip = {"a": torch.tensor([0.4]).double(), "b": torch.tensor([-1.3]).double(), "c": torch.tensor([2.0]).double()}
    # composite -> one product per node type into the flat buffer -> edge attention -> GELU -> out_lin -> gate
    big_w, big_b = R.composite_ref(p, meta)
    flat = torch.zeros(plan["total_floats"], dtype=torch.float64)
    row = 0
    for t in types:
        w = plan["width"][t]
        flat[plan["base"][t]: plan["base"][t] + R.SIZES[t] * w] = (x[t] @ big_w[row:row + w].t() + big_b[row:row + w]).flatten()
        row += w
    assert row == big_w.shape[0] == R.composite_rows(meta)
    got = {}
    for t in R.DST_TYPES:
        pre, _, _ = R.edge_attention_ref(flat, plan, t, heads)
        got[t] = R.gated_residual_ref(O._act("gelu", pre) @ out_w[t].t() + out_b[t], x[t], skip[t])
    op = {"k_rel.weight": p["k_rel"], "v_rel.weight": p["v_rel"]}
    for i, t in enumerate(types):
        op.update({f"kqv_lin.lins.{t}.weight": p["w"][i], f"kqv_lin.lins.{t}.bias": p["b"][i], f"out_lin.lins.{t}.weight": out_w[t],
                   f"out_lin.lins.{t}.bias": out_b[t], f"skip.{t}": skip[t]})
    for r, et in enumerate(R.EDGE_TYPES):
        op["p_rel." + "__".join(et)] = p["p"][r]
    want = O.hgt_conv_forward(op, x, ei, types, R.EDGE_TYPES, heads, F)
    assert set(want) == set(got)
    for t in R.DST_TYPES:
        err = float((got[t] - want[t]).abs().max())
        print(f"[hgt-ref] pipeline heads={heads} type {t}: max err against the oracle {err:.3e}")
        assert err <= 1e-9, (t, err)


# ------------------------------------------------------------------------------------ 3. the bound is fair
@pytest.mark.parametrize("q_scale", R.Q_SCALES)
@pytest.mark.parametrize("heads", R.HEADS)
def test_float32_attention_reference_stays_within_half_the_bound(heads, q_scale):
    _, plan = R.ladder(_gp())
    flat, douts = R.ladder_flat(q_scale), R.ladder_douts()
    outs64, grad64 = R.ladder_reference(_gp(), heads, q_scale)
    outs32, grad32 = R.attention_grads_ref(flat, plan, heads, douts, dtype=torch.float32)
    what = f"heads={heads} q_scale={q_scale:g}"
    for t in R.DST_TYPES:
        _share(f"{what} {t} pre", outs32[t][0], outs64[t][0])
        fin = torch.isfinite(outs64[t][1])
        assert torch.equal(fin, torch.isfinite(outs32[t][1]))
        _share(f"{what} {t} max", outs32[t][1][fin], outs64[t][1][fin])
        rel = float(((outs32[t][2].double() - outs64[t][2]).abs() / outs64[t][2]).max())
        print(f"[hgt-ref] {what} {t} denominator: float32 reference relative err {rel:.3e}, bound {R.TOL:.3e}, ratio {rel / R.TOL:.3f}")
        # (the denominator moves by the float32 error of the logits themselves, |a| * 2^-24 per product term: the reference alone
        # uses more of 2e-5 here than of the outputs' bound; it is held to the bound, the outputs and gradients to half of theirs)
        assert rel <= R.TOL
    if (heads, q_scale) in R.BWD_CASES:                             # the cases the backward kernels are run at
        _share(f"{what} gradient buffer", grad32, grad64)
        for t in R.DST_TYPES:
            _share(f"{what} {t} dq", R.query_rows(grad32, plan, t), R.query_rows(grad64, plan, t))


@pytest.mark.parametrize("heads", [1, 2])
def test_bf16_rounding_of_the_rows_stays_within_the_mirror_bound(heads):
    """The bf16 mirror case of the GPU tests: float64 on the rounded key | value rows against float64 on the rows themselves stays
    within 3e-2 * max(max|ref|, 1) for the outputs, the statistics and the gradient buffer -- the distance the rounding of the
    inputs alone sets.  (One type's query gradients taken by their own scale do not: `c` at two heads is at 1.01 of that bound before
    any kernel runs, so the GPU test compares the mirror's gradient buffer as one tensor and holds each part to the fp32 bound
    against float64 on the rounded rows instead.)"""
    _, plan = R.ladder(_gp())
    flat = R.ladder_flat(1.0)
    outs, grad = R.ladder_reference(_gp(), heads, 1.0)
    outs_r, grad_r = R.attention_grads_ref(flat, plan, heads, R.ladder_douts(), kv=R.bf16_rows(flat))

    def within(what, a, b, relative=False):
        err = float(((a - b).abs() / b).max()) if relative else float((a - b).abs().max())
        lim = 3e-2 if relative else 3e-2 * max(float(b.abs().max()), 1.0)
        print(f"[hgt-ref] bf16 rows heads={heads} {what}: rounded against unrounded float64 {err:.3e}, bound {lim:.3e}, "
              f"ratio {err / lim:.3f}")
        assert err <= lim, (what, err, lim)
    for t in R.DST_TYPES:
        fin = torch.isfinite(outs[t][1])
        within(f"{t} pre", outs_r[t][0], outs[t][0])
        within(f"{t} max", outs_r[t][1][fin], outs[t][1][fin])
        within(f"{t} denominator", outs_r[t][2], outs[t][2], relative=True)
    within("gradient buffer", grad_r, grad)
    # and the float32 evaluation on the rounded rows leaves the fp32 bound its room, as on the rows themselves
    outs32, grad32 = R.attention_grads_ref(flat, plan, heads, R.ladder_douts(), dtype=torch.float32, kv=R.bf16_rows(flat))
    for t in R.DST_TYPES:
        _share(f"bf16 rows heads={heads} {t} pre", outs32[t][0], outs_r[t][0])
        _share(f"bf16 rows heads={heads} {t} dq", R.query_rows(grad32, plan, t), R.query_rows(grad_r, plan, t))
    _share(f"bf16 rows heads={heads} gradient buffer", grad32, grad_r)


@pytest.mark.parametrize("heads,cin", R.COMPOSITE_CASES)
def test_float32_composite_reference_stays_within_half_the_bound(heads, cin):
    used = [et for i, et in enumerate(R.COMPOSITE_EDGE_TYPES) if i != R.COMPOSITE_ABSENT]
    meta = R.composite_meta(R.COMPOSITE_NODE_TYPES, used, R.COMPOSITE_EDGE_TYPES, heads, cin)
    assert meta["rel_src"] == [0, 0, 0, 1] and meta["rel_r"] == [0, 2, 4, 1] and R.composite_rows(meta) == 3 * 128 + 8 * 128
    p = R.composite_params(heads, cin)
    dw, db = R.composite_cotangents(R.composite_rows(meta), cin)
    w64, b64, g64 = R.composite_grads_ref(p, meta, dw, db)
    w32, b32, g32 = R.composite_grads_ref(p, meta, dw, db, dtype=torch.float32)
    what = f"composite heads={heads} cin={cin}"
    _share(what + " big_w", w32, w64)
    _share(what + " big_b", b32, b64)
    for k in ("k_rel", "v_rel"):
        _share(f"{what} d{k}", g32[k], g64[k])
    for k in ("w", "b", "p"):
        for i, (a, b) in enumerate(zip(g32[k], g64[k])):
            _share(f"{what} d{k}[{i}]", a, b)
    # the absent edge type reaches no row: exact zero gradients in the reference too
    D, R_ = 128 // heads, len(R.COMPOSITE_EDGE_TYPES)
    for k in ("k_rel", "v_rel"):
        assert float(g64[k].view(heads, R_, D, D)[:, R.COMPOSITE_ABSENT].abs().max()) == 0.0
    assert float(g64["p"][R.COMPOSITE_ABSENT].abs().max()) == 0.0


@pytest.mark.parametrize("skip", R.GATE_SKIPS)
def test_float32_gate_reference_stays_within_half_the_bound(skip):
    for rows in R.GATE_ROWS:
        o, x, dout = R.gate_inputs(rows)
        f32, f64 = R.gate_grads_ref(o, x, skip, dout, torch.float32), R.gate_grads_ref(o, x, skip, dout)
        for nm, a, b in zip(("out", "d_o", "d_x", "d_skip"), f32, f64):
            _share(f"gate rows={rows} skip={skip:g} {nm}", a, b)


# ------------------------------------------------------------------------------------ 4. the ladder and the plans
def test_ladder_holds_the_work_items_it_was_designed_for():
    gp = _gp()
    ei, plan = R.ladder(gp)                                         # (the builder asserts the counts of both directions itself)
    C = gp.HGT_CHUNK
    assert plan["per_dst"]["b"]["col"].device.type == "cpu"         # hgt_plan works with device="cpu"
    items = (plan["per_dst"]["b"]["item_ptr"][1:] - plan["per_dst"]["b"]["item_ptr"][:-1]).tolist()
    assert items[:13] == [0, 1, 1, 1, 1, 2, 2, 16, 17, 24, 1, 1, 1] and items[13:] == [1] * 27
    assert sorted(items[:8])[-2:] == [2, 16] and items[8:10] == [17, 24]           # combine workgroups 0 and 1
    pb = plan["per_dst"]["b"]
    sizes = (pb["item_end"] - pb["item_begin"]).tolist()
    first = pb["item_ptr"].tolist()
    assert sizes[first[4]] == C and sizes[first[5]: first[6]] == [C, 1] and sizes[first[8]: first[9]] == [C] * 16 + [1]
    rev = gp.hgt_reverse_plan(pb)
    ritems = (rev["item_ptr"][1:] - rev["item_ptr"][:-1]).tolist()
    assert max(ritems) == 17 and ritems.count(2) >= 1 and int(rev["n_rows"]) == len(ritems)
    assert sum(int(v.shape[1]) for v in ei.values()) < 10000
    # the edge order inside a relation is shuffled: the plan's stable sort restores the destination order
    assert not bool((ei[R.EDGE_TYPES[0]][1][1:] >= ei[R.EDGE_TYPES[0]][1][:-1]).all())
    # the relations of one destination are concatenated in edge-type order, each in its own edge order
    want = []
    for et in R.EDGE_TYPES[:3]:
        s, d = ei[et]
        want += [R.key_row(plan, et, int(j)) for j in s[d == 9].tolist()]
    assert pb["col"][pb["rowptr"][9]: pb["rowptr"][10]].tolist() == want


def test_rows_plan_numbers_items_and_edges_across_the_types():
    _, plan = R.ladder(_gp())
    rp = R.rows_plan(plan, R.DST_TYPES, R.SIZES)
    n = sum(R.SIZES.values())
    assert rp["q_off"].numel() == n and rp["item_ptr"].numel() == n + 1 and int(rp["item_ptr"][-1]) == rp["item_dst"].numel()
    assert bool((rp["q_off"] % 4 == 0).all()) and int(rp["q_off"].max()) + 128 <= plan["total_floats"]
    assert int(rp["item_end"].max()) == rp["col"].numel() and bool((rp["item_end"] > rp["item_begin"]).all())
    assert bool((rp["item_ptr"][rp["item_dst"]] <= torch.arange(rp["item_dst"].numel())).all())
    assert bool((rp["item_ptr"][rp["item_dst"] + 1] > torch.arange(rp["item_dst"].numel())).all())
    assert int(rp["col"].max()) + 2 <= plan["total_floats"] // 128 and int(rp["col"].min()) >= 1


@pytest.mark.parametrize("world", [2, 3])
def test_destination_partitioned_plans_tile_the_unpartitioned_one(world):
    from madrigal_amd.parallel import shard_range
    gp = _gp()
    ei, plan = R.ladder(gp)
    for t in R.DST_TYPES:
        covered = 0
        for rank in range(world):
            rng = {u: shard_range(R.SIZES[u], rank, world) for u in R.SIZES}
            part = gp.hgt_plan(ei, R.EDGE_TYPES, R.SIZES, torch.device("cpu"), dst_range=rng)
            assert part["base"] == plan["base"] and part["width"] == plan["width"] and part["total_floats"] == plan["total_floats"]
            lo, hi = rng[t]
            assert lo == covered                                     # the partitions' destinations tile [0, n_t)
            covered = hi
            pp, pf = part["per_dst"][t], plan["per_dst"][t]
            assert pp["rowptr"].numel() == hi - lo + 1
            for i in range(hi - lo):
                mine = pp["col"][pp["rowptr"][i]: pp["rowptr"][i + 1]]
                assert torch.equal(mine, pf["col"][pf["rowptr"][lo + i]: pf["rowptr"][lo + i + 1]]), (t, rank, i)
            assert (pp["item_ptr"][1:] - pp["item_ptr"][:-1]).tolist() == (pf["item_ptr"][1:] - pf["item_ptr"][:-1])[lo:hi].tolist()
        assert covered == R.SIZES[t]


# ------------------------------------------------------------------------------------ 5. the CSR reference
def test_csr_ref_matches_a_plain_loop():
    wide, rowptr, col, w, x_self, _ = R.csr_case(36, 7)
    x = wide[:, 4:40].double()
    for weights in (None, w):
        for mean in (False, True):
            got = R.csr_ref(x, rowptr, col, weights, mean, x_self.double(), 1.25)
            for v in range(7):
                acc = torch.zeros(36, dtype=torch.float64)
                for e in range(int(rowptr[v]), int(rowptr[v + 1])):
                    acc += x[col[e]] * (1.0 if weights is None else float(weights[e]))
                if mean:
                    acc /= max(int(rowptr[v + 1] - rowptr[v]), 1)
                assert float((got[v] - (acc + 1.25 * x_self[v].double())).abs().max()) <= 1e-12
    assert sorted(set((rowptr[1:] - rowptr[:-1]).tolist())) == [0, 1, 3, 4, 5, 8, 9]
