"""The kernels of the knowledge-graph (HGT) encoder at op level, against the float64 references of hgt_ref.py: A the edge attention
forward (csrc/graph.hip: strided queries, several relations and source types in one softmax, the 16/17-item switch to the
cooperative merge, the one-launch row plan), B its backward (gradients written into the shared buffer's own slots, the
destination-partitioned plans, the bf16 mirror), C the composite projection weights (csrc/hgt_params.hip, every code shape of
both directions), D the gated residual and the CSR aggregation at its lane-group boundaries.
Every comparison: max|got - ref| <= 2e-5 * max(max|ref|, 1) per compared tensor unless it says otherwise.  Each check prints its
figure before it asserts."""
import pytest
import torch

import hgt_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _gp():
    from madrigal_amd import graph_plans
    return graph_plans


def _check(group, what, got, ref, tol=R.TOL):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (group, what, tuple(got.shape), tuple(ref.shape))
    err, b = float((got - ref).abs().max()), tol * max(float(ref.abs().max()), 1.0)
    print(f"[hgt-ops] {group} {what}: max err {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
    assert err <= b, (group, what, err, b)                   # a NaN in `got` fails here too


def _check_relative(group, what, got, ref, tol=R.TOL):
    got = got.detach().cpu().double()
    err = float(((got - ref).abs() / ref).max())
    print(f"[hgt-ops] {group} {what}: max err {err:.3e} (relative), bound {tol:.3e}, ratio {err / tol:.3f}")
    assert err <= tol, (group, what, err, tol)


def _ladder_gpu():
    return R.ladder(_gp(), "cuda")[1]


def _empty_rows(pd):
    return (pd["rowptr"][1:] == pd["rowptr"][:-1]).nonzero().flatten().tolist()


# ------------------------------------------------------------------------------------------------ A. forward
@pytest.mark.parametrize("q_scale", R.Q_SCALES)
@pytest.mark.parametrize("heads", R.HEADS)
def test_forward_matches_float64(ops, heads, q_scale):
    from oracle import madrigal_oracle as O
    plan = _ladder_gpu()
    outs, _ = R.ladder_reference(_gp(), heads, q_scale)
    flat = R.ladder_flat(q_scale).cuda()
    n_all, pad = sum(R.SIZES[t] for t in R.DST_TYPES), 3
    big = torch.full((n_all + 2 * pad, 128), SENTINEL, device="cuda")
    row0, pres = pad, []
    for t in R.DST_TYPES:
        pd, n = plan["per_dst"][t], R.SIZES[t]
        what = f"heads={heads} q_scale={q_scale:g} {t}"
        q = R.query_rows(flat, plan, t)
        assert q.stride(0) == 640 and not q.is_contiguous()              # ldq = 128 + 256 * R_t: a slice of the projection rows
        ref_pre, ref_m, ref_den = outs[t]
        pre, stats = ops.hgt_attention_stats(q, flat, pd, heads)
        pre2, stats2 = ops.hgt_attention_stats(q, flat, pd, heads)
        assert torch.equal(pre, pre2) and torch.equal(stats, stats2)
        _check("A", what + " pre", pre, ref_pre)
        m, den = stats[..., 0].cpu(), stats[..., 1].cpu()
        fin = torch.isfinite(ref_m)
        assert torch.equal(torch.isfinite(m), fin)
        _check("A", what + " max", m[fin], ref_m[fin])
        _check_relative("A", what + " denominator", den, ref_den)
        for i in _empty_rows(pd):                                         # no incoming edge: an exact zero row, statistics (-inf, 1e-16)
            assert float(pre[i].abs().max()) == 0.0
            assert bool((m[i] == float("-inf")).all()) and bool((den[i] == torch.tensor(1e-16, dtype=torch.float32)).all())
        # the activated launch, written into a row block of a larger buffer
        block = big[row0:row0 + n]
        others = torch.cat([big[:row0], big[row0 + n:]])                  # (a copy: the earlier types' rows and the sentinel rows)
        got = ops.hgt_attention(q, flat, pd, heads, apply_gelu=False, out=block)
        assert got.data_ptr() == block.data_ptr() and torch.equal(block, pre)             # the same launch as the stats call: bit-equal
        assert torch.equal(torch.cat([big[:row0], big[row0 + n:]]), others)
        ops.hgt_attention(q, flat, pd, heads, apply_gelu=True, out=block)
        _check("A", what + " gelu", block, O._act("gelu", ref_pre))
        first = block.clone()
        ops.hgt_attention(q, flat, pd, heads, apply_gelu=True, out=block)
        assert torch.equal(block, first) and torch.equal(torch.cat([big[:row0], big[row0 + n:]]), others)
        pres.append(pre)
        row0 += n
    assert bool((big[:pad] == SENTINEL).all()) and bool((big[row0:] == SENTINEL).all())
    # every destination type in one launch: the same arithmetic in the same order
    rp = R.rows_plan(plan, R.DST_TYPES, R.SIZES)
    what = f"heads={heads} q_scale={q_scale:g} rows"
    out_all = torch.full((n_all, 128), SENTINEL, device="cuda")
    ops.hgt_attention_rows(flat, rp, heads, out_all, apply_gelu=False)
    assert torch.equal(out_all, torch.cat(pres))
    _check("A", what + " pre", out_all, torch.cat([outs[t][0] for t in R.DST_TYPES]))
    ops.hgt_attention_rows(flat, rp, heads, out_all, apply_gelu=True)
    assert torch.equal(out_all, big[pad:pad + n_all])
    again = torch.full((n_all, 128), SENTINEL, device="cuda")
    ops.hgt_attention_rows(flat, rp, heads, again, apply_gelu=True)
    assert torch.equal(out_all, again)


# ------------------------------------------------------------------------------------------------ B. backward
def _backward_per_type(ops, plan, flat, douts, heads, kv=None, kv16=None):
    """The production arrangement of _HgtAttentionFlat.backward: one gradient buffer (pre-filled with a sentinel), each destination
    type's call writes its key | value rows and, through ``dq_out``, its own query slots.  -> (pres, stats, gradient buffer)."""
    gp = _gp()
    kv = flat if kv is None else kv
    dflat = torch.full_like(flat, SENTINEL)
    pres, stats = {}, {}
    for t in R.DST_TYPES:
        pd = plan["per_dst"][t]
        q, dq = R.query_rows(flat, plan, t), R.query_rows(dflat, plan, t)
        pres[t], stats[t] = ops.hgt_attention_stats(q, kv, pd, heads, kv16=kv16)
        got = ops.hgt_attention_bwd(q, kv, pd, gp.hgt_reverse_plan(pd), heads, douts[t], pres[t], stats[t], dflat, dq_out=dq, kv16=kv16)
        assert got.data_ptr() == dq.data_ptr()
    return pres, stats, dflat


def _check_gradient(group, what, plan_cpu, got, ref, tol=R.TOL, per_type=True):
    own = R.owned_mask(plan_cpu)
    got = got.cpu()
    assert bool((got[~own] == SENTINEL).all()), (group, what, "a float no call owns was written")
    assert float(ref[~own].abs().max()) == 0.0
    zero = torch.zeros((), dtype=got.dtype)
    _check(group, what + " gradient buffer", torch.where(own, got, zero), ref, tol)
    for t in R.DST_TYPES:
        if per_type:                                                      # (finer: each type's query gradients by their own scale)
            _check(group, f"{what} {t} dq", R.query_rows(got, plan_cpu, t), R.query_rows(ref, plan_cpu, t), tol)
        for i in _empty_rows(plan_cpu["per_dst"][t]):
            assert float(R.query_rows(got, plan_cpu, t)[i].abs().max()) == 0.0
    return torch.where(own, got, zero)


@pytest.mark.parametrize("heads,q_scale", R.BWD_CASES)
def test_backward_matches_float64_autograd(ops, heads, q_scale):
    from madrigal_amd import autograd as ag
    plan, plan_cpu = _ladder_gpu(), R.ladder(_gp())[1]
    _, ref_grad = R.ladder_reference(_gp(), heads, q_scale)
    flat = R.ladder_flat(q_scale).cuda()
    douts = {t: g.cuda() for t, g in R.ladder_douts().items()}
    what = f"heads={heads} q_scale={q_scale:g}"
    pres, _, dflat = _backward_per_type(ops, plan, flat, douts, heads)
    _, _, dflat2 = _backward_per_type(ops, plan, flat, douts, heads)
    assert torch.equal(dflat, dflat2)                                     # no atomics: bit-reproducible
    owned = _check_gradient("B", what, plan_cpu, dflat, ref_grad)
    # the autograd node: the same kernels, zeros where no call writes
    leaf = flat.clone().requires_grad_(True)
    qspec = [(plan["base"][t], R.SIZES[t], plan["width"][t]) for t in R.DST_TYPES]
    outs = ag.hgt_attention_flat(leaf, heads, [plan["per_dst"][t] for t in R.DST_TYPES], qspec)
    for t, o in zip(R.DST_TYPES, outs):
        assert torch.equal(o, pres[t])
    torch.autograd.backward(outs, [douts[t] for t in R.DST_TYPES])
    assert torch.equal(leaf.grad.cpu(), owned)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("heads", R.HEADS)
def test_destination_partition_matches_the_whole(ops, heads, world):
    from madrigal_amd import autograd as ag
    from madrigal_amd.parallel import shard_range
    gp = _gp()
    ei, plan = R.ladder(gp, "cuda")
    plan_cpu = R.ladder(gp)[1]
    _, ref_grad = R.ladder_reference(gp, heads, 1.0)
    flat = R.ladder_flat(1.0).cuda()
    douts = {t: g.cuda() for t, g in R.ladder_douts().items()}
    pres, _, dflat = _backward_per_type(ops, plan, flat, douts, heads)
    qmask = torch.zeros(flat.shape, dtype=torch.bool)
    for t in R.DST_TYPES:
        R.query_rows(qmask, plan_cpu, t)[:] = True
    total = torch.zeros(flat.shape, dtype=torch.float64)
    blocks = {t: [] for t in R.DST_TYPES}
    for rank in range(world):
        rng = {t: shard_range(R.SIZES[t], rank, world) for t in R.SIZES}
        part = gp.hgt_plan(ei, R.EDGE_TYPES, R.SIZES, torch.device("cuda"), dst_range=rng)
        dst_types = [t for t in R.DST_TYPES if rng[t][1] > rng[t][0]]
        qspec = [(plan["base"][t] + rng[t][0] * plan["width"][t], rng[t][1] - rng[t][0], plan["width"][t]) for t in dst_types]
        leaf = flat.clone().requires_grad_(True)
        outs = ag.hgt_attention_flat(leaf, heads, [part["per_dst"][t] for t in dst_types], qspec)
        torch.autograd.backward(outs, [douts[t][rng[t][0]:rng[t][1]] for t in dst_types])
        grad = leaf.grad
        mine = torch.zeros(flat.shape, dtype=torch.bool)
        for t, o in zip(dst_types, outs):
            blocks[t].append(o)
            lo, hi = rng[t]
            R.query_rows(mine, plan_cpu, t, lo, hi)[:] = True
            # this rank's query-slot gradients: the unpartitioned ones bit for bit
            assert torch.equal(R.query_rows(grad, plan, t, lo, hi), R.query_rows(dflat, plan, t, lo, hi)), (t, rank)
        g = grad.cpu()
        assert float(g[qmask & ~mine].abs().max()) == 0.0                 # the other ranks' query slots: not this rank's to write
        total += torch.where(qmask, torch.zeros((), dtype=torch.float64), g.double())
    for t in R.DST_TYPES:
        assert torch.equal(torch.cat(blocks[t]), pres[t]), t             # the forward blocks concatenate to the unpartitioned rows
    want = torch.where(qmask, torch.zeros((), dtype=torch.float64), ref_grad)
    _check("B", f"heads={heads} world={world} key | value gradients summed over the ranks", total, want)


@pytest.mark.parametrize("heads", [1, 2])
def test_bf16_mirror_equals_fp32_kernels_on_the_rounded_rows(ops, heads):
    """The mirror kernels are the fp32 kernels on the rounded rows: bit-equal to them, and within the fp32 bound of float64 autograd
    ON THOSE ROWS.  Against float64 on the unrounded rows the outputs, the statistics and the gradient buffer stay within 3e-2 (a
    distance the rounding of the inputs sets, not the kernels: test_hgt_ops_cpu.py measures it between the two float64 results)."""
    plan, plan_cpu = _ladder_gpu(), R.ladder(_gp())[1]
    outs, ref_grad = R.ladder_reference(_gp(), heads, 1.0)
    flat_cpu = R.ladder_flat(1.0)
    flat = flat_cpu.cuda()
    douts = {t: g.cuda() for t, g in R.ladder_douts().items()}
    kv16 = ops.f32_to_bf16(flat)
    assert torch.equal(kv16.cpu(), flat_cpu.to(torch.bfloat16))           # round to nearest even, as torch rounds
    pres16, stats16, d16 = _backward_per_type(ops, plan, flat, douts, heads, kv16=kv16)
    pres_r, stats_r, d_r = _backward_per_type(ops, plan, flat, douts, heads, kv=kv16.float())
    assert torch.equal(d16, d_r)
    outs_r, grad_r = R.attention_grads_ref(flat_cpu, plan_cpu, heads, R.ladder_douts(), kv=R.bf16_rows(flat_cpu))
    for t in R.DST_TYPES:
        assert torch.equal(pres16[t], pres_r[t]) and torch.equal(stats16[t], stats_r[t])
        what = f"bf16 mirror heads={heads} {t}"
        m, den = stats16[t][..., 0].cpu(), stats16[t][..., 1].cpu()
        fin = torch.isfinite(outs[t][1])
        assert torch.equal(torch.isfinite(m), fin)
        _check("B", what + " pre, rounded rows", pres16[t], outs_r[t][0])
        _check("B", what + " max, rounded rows", m[fin], outs_r[t][1][fin])
        _check_relative("B", what + " denominator, rounded rows", den, outs_r[t][2])
        _check("B", what + " pre", pres16[t], outs[t][0], tol=3e-2)
        _check("B", what + " max", m[fin], outs[t][1][fin], tol=3e-2)
        _check_relative("B", what + " denominator", den, outs[t][2], tol=3e-2)
    _check_gradient("B", f"bf16 mirror heads={heads}, rounded rows", plan_cpu, d16, grad_r)
    _check_gradient("B", f"bf16 mirror heads={heads}", plan_cpu, d16, ref_grad, tol=3e-2, per_type=False)


# ------------------------------------------------------------------------------------------------ C. composite weights
def _composite_conv(heads, cin):
    """A small HGTConv on the GPU holding hgt_ref's deterministic parameters -> (conv, projected types, plan, parameters)."""
    from madrigal_amd import models as M
    conv = M.HGTConv(cin, 128, (R.COMPOSITE_NODE_TYPES, R.COMPOSITE_EDGE_TYPES), heads).cuda()
    p = R.composite_params(heads, cin)
    with torch.no_grad():
        conv.k_rel.weight.copy_(p["k_rel"])
        conv.v_rel.weight.copy_(p["v_rel"])
        for i, t in enumerate(R.COMPOSITE_NODE_TYPES):
            conv.kqv_lin.lins[t].weight.copy_(p["w"][i])
            conv.kqv_lin.lins[t].bias.copy_(p["b"][i])
        for r, et in enumerate(R.COMPOSITE_EDGE_TYPES):
            conv.p_rel["__".join(et)].copy_(p["p"][r])
    ei = {k: v.cuda() for k, v in R.composite_edges().items()}
    plan = conv._plan(ei, R.COMPOSITE_SIZES, torch.device("cuda"), set(R.COMPOSITE_NODE_TYPES))
    assert plan["nrel"] == {"x": 3, "y": 1, "z": 0} and R.COMPOSITE_EDGE_TYPES[R.COMPOSITE_ABSENT] not in plan["used"]
    return conv, list(R.COMPOSITE_NODE_TYPES), plan, p


def _composite_grads(conv):
    g = {"k_rel": conv.k_rel.weight.grad, "v_rel": conv.v_rel.weight.grad,
         "w": [conv.kqv_lin.lins[t].weight.grad for t in R.COMPOSITE_NODE_TYPES],
         "b": [conv.kqv_lin.lins[t].bias.grad for t in R.COMPOSITE_NODE_TYPES],
         "p": [conv.p_rel["__".join(et)].grad for et in R.COMPOSITE_EDGE_TYPES]}
    out = {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in g.items()}
    conv.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("heads,cin", R.COMPOSITE_CASES)
def test_composite_weights_match_float64_autograd(heads, cin):
    conv, types, plan, p = _composite_conv(heads, cin)
    meta = R.composite_meta(types, plan["used"], R.COMPOSITE_EDGE_TYPES, heads, cin)
    rows = R.composite_rows(meta)
    dw, db = R.composite_cotangents(rows, cin)
    ref_w, ref_b, ref_g = R.composite_grads_ref(p, meta, dw, db)
    what = f"heads={heads} cin={cin}"
    runs = []
    for _ in range(2):
        big_w, big_b, offs = conv._composite_all_hip(types, plan)
        torch.autograd.backward([big_w, big_b], [dw.cuda(), db.cuda()])
        runs.append((big_w.detach().clone(), big_b.detach().clone(), _composite_grads(conv)))
    (big_w, big_b, g), (w2, b2, g2) = runs
    assert offs == [0, 128 + 3 * 256, 2 * 128 + 4 * 256, rows]
    _check("C", what + " big_w", big_w, ref_w)
    _check("C", what + " big_b", big_b, ref_b)
    assert torch.equal(big_w, w2) and torch.equal(big_b, b2)
    for k in ("k_rel", "v_rel"):
        _check("C", f"{what} d{k}", g[k], ref_g[k])
        assert torch.equal(g[k], g2[k])
    for k in ("w", "b", "p"):
        for i, (a, b, c) in enumerate(zip(g[k], ref_g[k], g2[k])):
            _check("C", f"{what} d{k}[{i}]", a, b)
            assert torch.equal(a, c)
    D, n_et = 128 // heads, len(R.COMPOSITE_EDGE_TYPES)                     # the absent edge type: exact zeros
    for k in ("k_rel", "v_rel"):
        assert float(g[k].view(heads, n_et, D, D)[:, R.COMPOSITE_ABSENT].abs().max()) == 0.0
    assert float(g["p"][R.COMPOSITE_ABSENT].abs().max()) == 0.0


def test_composite_refuses_a_head_beyond_the_register_tile(ops):
    from madrigal_amd._lib import MadrigalHipError
    heads, cin = 1, 256
    conv, types, plan, _ = _composite_conv(heads, cin)
    with pytest.raises((ValueError, MadrigalHipError)):
        conv._composite_all_hip(types, plan)
    meta = conv.__dict__["_rel_idx"][("hip", tuple(types), tuple(plan["used"]))]
    rows = meta["rows"]
    big_w, big_b = torch.full((rows, cin), SENTINEL, device="cuda"), torch.full((rows,), SENTINEL, device="cuda")
    with pytest.raises((ValueError, MadrigalHipError)):
        ops.hgt_composite(meta["ptrs"], conv.k_rel.weight, conv.v_rel.weight, meta, big_w, big_b)
    n_et = len(R.COMPOSITE_EDGE_TYPES)
    grads = torch.full((3 * (3 * 128 * cin + 3 * 128) + 2 * heads * n_et * 128 * 128 + n_et * heads,), SENTINEL, device="cuda")
    with pytest.raises((ValueError, MadrigalHipError)):
        ops.hgt_composite_bwd(meta["ptrs"], conv.k_rel.weight, conv.v_rel.weight, meta, torch.zeros((rows, cin), device="cuda"),
                              torch.zeros(rows, device="cuda"), grads)
    torch.cuda.synchronize()
    assert bool((big_w == SENTINEL).all()) and bool((big_b == SENTINEL).all()) and bool((grads == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ D. small kernels
@pytest.mark.parametrize("skip", R.GATE_SKIPS)
@pytest.mark.parametrize("rows", R.GATE_ROWS)
def test_gated_residual_matches_float64_autograd(ops, rows, skip):
    o, x, dout = R.gate_inputs(rows)
    ref = R.gate_grads_ref(o, x, skip, dout)
    s = torch.tensor([skip], device="cuda")
    out = ops.gated_residual(o.cuda(), x.cuda(), s)
    d_o, d_x, d_skip = ops.gated_residual_bwd(dout.cuda(), o.cuda(), x.cuda(), s)
    what = f"gate rows={rows} skip={skip:g}"
    for nm, got, want in zip(("out", "d_o", "d_x", "d_skip"), (out, d_o, d_x, d_skip.reshape(1)), ref):
        _check("D", f"{what} {nm}", got, want)


def _csr_strided(ops, xs, rowptr, col, w, x_self, coef, mean, F):
    """mdg_csr_aggregate on a column-slice view (ldx > F): the wrapper would copy the slice, so the entry point is called directly."""
    from madrigal_amd._lib import call
    n_dst = int(rowptr.numel()) - 1
    out = torch.full((n_dst, F), SENTINEL, device="cuda")
    assert xs.stride(0) > F and xs.stride(1) == 1
    call("mdg_csr_aggregate", xs.data_ptr(), xs.stride(0), rowptr.data_ptr(), col.data_ptr(), None if w is None else w.data_ptr(),
         x_self.data_ptr(), x_self.stride(0), None, coef, 1 if mean else 0, out.data_ptr(), F, n_dst, F, ops._stream(xs))
    return out


@pytest.mark.parametrize("n_dst", R.CSR_N_DST)
@pytest.mark.parametrize("F", R.CSR_F)
def test_csr_aggregate_at_the_lane_group_boundaries(ops, F, n_dst):
    gp = _gp()
    wide, rowptr, col, w, x_self, dout = R.csr_case(F, n_dst)
    if n_dst >= 7:
        assert sorted(set((rowptr[1:] - rowptr[:-1]).tolist())) == [0, 1, 3, 4, 5, 8, 9]
    wide_d, rp_d, col_d, w_d, self_d, dout_d = (t.cuda() for t in (wide, rowptr, col, w, x_self, dout))
    xs = wide_d[:, 4:4 + F]
    for weights in (False, True):
        for mean in (False, True):
            what = f"csr F={F} n_dst={n_dst} {'weighted' if weights else 'plain'}{' mean' if mean else ''}"
            x64 = wide[:, 4:4 + F].double().clone().requires_grad_(True)
            ref = R.csr_ref(x64, rowptr, col, w if weights else None, mean, x_self.double(), 1.25)
            got = ops.csr_aggregate(xs, rp_d, col_d, edge_weight=w_d if weights else None, x_self=self_d, self_coef_add=1.25, mean=mean)
            _check("D", what, got, ref.detach())
            assert torch.equal(_csr_strided(ops, xs, rp_d, col_d, w_d if weights else None, self_d, 1.25, mean, F), got)
            # the backward pass: the same kernel over the transposed plan
            (ref * dout.double()).sum().backward()
            tr = gp.transposed_csr(rp_d, col_d, w_d if weights else None, R.CSR_N_SRC, mean=mean)
            dx = ops.csr_aggregate(dout_d, tr["rowptr"], tr["col"], edge_weight=tr["w"])
            _check("D", what + " dx", dx, x64.grad)


def test_csr_aggregate_refuses_a_row_wider_than_256(ops):
    from madrigal_amd._lib import MadrigalHipError
    rowptr = torch.tensor([0, 2, 3], device="cuda")
    col = torch.tensor([0, 1, 2], device="cuda")
    with pytest.raises((ValueError, MadrigalHipError)):
        ops.csr_aggregate(R.rand((5, 260), 1).cuda(), rowptr, col)
