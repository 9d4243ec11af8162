"""Float64 references for the kernels of the knowledge-graph (HGT) encoder -- the edge attention of csrc/graph.hip, the composite
projection weights of csrc/hgt_params.hip, the gated residual and the CSR aggregation -- and the deterministic cases that
test_hgt_ops_cpu.py and test_hgt_ops_gpu.py share.  Pure torch: nothing here imports the package under test (the one module the
graph cases need, ``graph_plans``, is handed in by the caller).  Every formula is dtype-generic: run on a float32 copy of the
inputs it gives the "float32 evaluation of the reference" that the bound is held against."""
import contextlib
import functools
import math

import torch

from attention_ref import TOL, bound, rand  # noqa: F401  (the suite's fp32-class bound: max|got - ref| <= 2e-5 * max(max|ref|, 1))

HEADS = [1, 2, 4, 8]
Q_SCALES = [1.0, 3.0]
BWD_CASES = [(1, 1.0), (2, 1.0), (4, 1.0), (8, 1.0), (4, 3.0)]          # (heads, q_scale) of the backward tests
REF_SHARE = 0.5                # float32 reference against float64 reference: at most this share of the bound, every case

# ---------------------------------------------------------------------------------------------------- the "ladder" graph
SIZES = {"a": 300, "b": 40, "c": 64}
EDGE_TYPES = [("a", "r0", "b"), ("c", "r1", "b"), ("b", "r2", "b"), ("a", "r3", "c"), ("b", "r4", "a"), ("c", "r5", "c")]
DST_TYPES = ["a", "b", "c"]
HUB_ROW, CHUNK_ROW, CHUNK1_ROW = 5, 6, 7          # source rows of `a` with > 16C, exactly C and C + 1 edges into `b`
QUIET_FROM = 250                                   # rows of `a` from here on have no edge into `b`
C_HEAVY = 3                                        # the destination of `c` with C + 3 incoming edges


def ladder_degrees(C):
    """Incoming degree and work items of every destination of `b` (summed over its three relations)."""
    deg = [0, 1, 2, C - 1, C, C + 1, 2 * C, 16 * C, 16 * C + 1, 23 * C + 5, 7, 8, 9] + [3] * 27
    return deg, [-(-d // C) for d in deg]


def _split3(d):
    return [d // 3 + (1 if d % 3 > 0 else 0), d // 3 + (1 if d % 3 > 1 else 0), d // 3]


@functools.lru_cache(maxsize=None)
def ladder_edges(C):
    """edge_index_dict of the ladder (int64 [2, E] per edge type; the edge order inside a relation is shuffled)."""
    g = torch.Generator().manual_seed(1234)
    deg, _ = ladder_degrees(C)
    assert len(deg) == SIZES["b"]
    parts = [_split3(d) for d in deg]
    dst_of = [torch.repeat_interleave(torch.arange(SIZES["b"]), torch.tensor([p[k] for p in parts])) for k in range(3)]
    # r0 (a -> b): the skewed key rows of the reverse plan
    n0 = int(dst_of[0].numel())
    fixed = [torch.full((16 * C + 3,), HUB_ROW), torch.full((C,), CHUNK_ROW), torch.full((C + 1,), CHUNK1_ROW)]
    rest = n0 - sum(int(f.numel()) for f in fixed)
    assert rest > 0, "HGT_CHUNK leaves the a -> b relation too few edges for the skewed key rows"
    src0 = torch.cat(fixed + [torch.randint(10, QUIET_FROM, (rest,), generator=g)])
    src0 = src0[torch.randperm(n0, generator=g)]
    src1 = torch.randint(0, SIZES["c"], (int(dst_of[1].numel()),), generator=g)
    src2 = torch.randint(0, SIZES["b"], (int(dst_of[2].numel()),), generator=g)
    # c: one destination of degree C + 3 (r3 and r5), the others 0, 1 or 2 edges; a: degree 2 everywhere (r4)
    cdeg = [(C + 3) if i == C_HEAVY else i % 3 for i in range(SIZES["c"])]
    d3 = torch.repeat_interleave(torch.arange(SIZES["c"]), torch.tensor([-(-d // 2) for d in cdeg]))
    d5 = torch.repeat_interleave(torch.arange(SIZES["c"]), torch.tensor([d // 2 for d in cdeg]))
    s3 = torch.randint(0, SIZES["a"], (int(d3.numel()),), generator=g)
    s5 = torch.randint(0, SIZES["c"], (int(d5.numel()),), generator=g)
    d4 = torch.repeat_interleave(torch.arange(SIZES["a"]), 2)
    s4 = torch.randint(0, SIZES["b"], (int(d4.numel()),), generator=g)
    out = {}
    for et, s, d in zip(EDGE_TYPES, (src0, src1, src2, s3, s4, s5), (dst_of[0], dst_of[1], dst_of[2], d3, d4, d5)):
        perm = torch.randperm(int(d.numel()), generator=g)
        out[et] = torch.stack([s[perm], d[perm]]).long()
    return out


_ladders = {}


def ladder(gp, device="cpu"):
    """-> (edge_index_dict, plan) of the ladder for ``gp`` = the package's graph_plans module.  Asserts the work-item counts the
    case was designed for, in both directions, so that a change of HGT_CHUNK cannot silently empty it."""
    C = int(gp.HGT_CHUNK)
    key = (C, str(device))
    if key in _ladders:
        return _ladders[key]
    ei = {k: v.to(device) for k, v in ladder_edges(C).items()}
    plan = gp.hgt_plan(ei, EDGE_TYPES, SIZES, torch.device(device))
    assert plan["width"] == {"a": 640, "b": 640, "c": 640} and plan["total_floats"] == 404 * 640
    deg, items = ladder_degrees(C)
    pb = plan["per_dst"]["b"]
    assert (pb["rowptr"][1:] - pb["rowptr"][:-1]).tolist() == deg
    got_items = (pb["item_ptr"][1:] - pb["item_ptr"][:-1]).tolist()
    assert got_items == items, (got_items, items)
    if C > 1:
        assert items[:13] == [0, 1, 1, 1, 1, 2, 2, 16, 17, 24, 1, 1, 1]
    ic = plan["per_dst"]["c"]["item_ptr"]
    assert (ic[1:] - ic[:-1]).max().item() == 2 and int(ic[C_HEAVY + 1] - ic[C_HEAVY]) == 2
    ia = plan["per_dst"]["a"]["item_ptr"]
    assert (ia[1:] - ia[:-1]).tolist() == [1] * SIZES["a"] and SIZES["a"] % 8 != 0
    # the reverse plan of `b`: key rows of `a` under relation r0 with 17+, 1 (exactly C edges) and 2 (C + 1 edges) items, rows with none
    rev = gp.hgt_reverse_plan(pb)
    ritems = dict(zip(rev["rows"].tolist(), (rev["item_ptr"][1:] - rev["item_ptr"][:-1]).tolist()))
    per_row = torch.bincount(rev["item_row"], weights=(rev["item_end"] - rev["item_begin"]).double()).long()
    redges = dict(zip(rev["rows"].tolist(), per_row.tolist()))
    row = lambda j: key_row(plan, EDGE_TYPES[0], j)
    assert redges[row(HUB_ROW)] == 16 * C + 3 and ritems[row(HUB_ROW)] == 17
    assert redges[row(CHUNK_ROW)] == C and ritems[row(CHUNK_ROW)] == 1
    assert redges[row(CHUNK1_ROW)] == C + 1 and ritems[row(CHUNK1_ROW)] == (2 if C > 1 else C + 1)
    assert all(row(j) not in ritems for j in range(QUIET_FROM, SIZES["a"]))
    _ladders[key] = (ei, plan)
    return _ladders[key]


def key_row(plan, et, j):
    """Row, in the [*, 128] view of the flat projection buffer, of the relation-transformed key of source node j under edge type
    ``et`` (its value is the next row): restated from the layout in graph_plans.hgt_plan's docstring."""
    s = et[0]
    return (plan["base"][s] + j * plan["width"][s] + 128 + 256 * plan["slot"][et]) // 128


def ladder_flat(q_scale=1.0, seed=500):
    """The flat projection buffer the kernels read, [total / 128, 128] float32: unit normal, the query slots times ``q_scale``."""
    flat = rand((404 * 640,), seed)
    return scale_queries(flat, q_scale).view(-1, 128)


def scale_queries(flat, q_scale):
    out = flat.clone().view(404, 640)
    out[:, :128] *= q_scale
    return out.view(-1)


def ladder_douts(seed=600):
    return {t: rand((SIZES[t], 128), seed + i) for i, t in enumerate(DST_TYPES)}


def query_rows(flat, plan, t, lo=0, hi=None):
    """The [n, 128] strided view of the queries of type t's rows lo..hi, as the production code cuts it out of the flat buffer."""
    hi = SIZES[t] if hi is None else hi
    w, off = plan["width"][t], plan["base"][t] + lo * plan["width"][t]
    return flat.view(-1)[off:off + (hi - lo) * w].view(hi - lo, w)[:, 0:128]


# ---------------------------------------------------------------------------------------------------- 1. edge attention
def edge_attention_ref(flat, plan, t, heads, q_scale=1.0, rows=None):
    """-> (pre [n,128], max [n,H], denominator [n,H]) of destination type t.  Queries: the first 128 floats of t's rows times
    ``q_scale``; key / value rows ``flat.view(-1,128)[col]`` / ``[col + 1]``; alpha = exp(a - max) / (sum exp + 1e-16) per head over
    ALL incoming edges.  Differentiable in ``flat`` (index_add / scatter_reduce): keys, values and queries share one gradient.
    ``rows`` [*,128]: gather the key / value rows from this buffer instead (the bf16 mirror's rounded rows; queries stay ``flat``'s)."""
    pd = plan["per_dst"][t]
    col, rowptr = pd["col"], pd["rowptr"]
    n = int(rowptr.numel()) - 1
    D = 128 // heads
    q = query_rows(flat, plan, t, 0, n) * q_scale
    rows = flat.view(-1, 128) if rows is None else rows
    dst = torch.repeat_interleave(torch.arange(n, device=col.device), rowptr[1:] - rowptr[:-1])
    k, v = rows[col].view(-1, heads, D), rows[col + 1].view(-1, heads, D)
    a = (q[dst].view(-1, heads, D) * k).sum(-1)
    m = torch.full((n, heads), float("-inf"), dtype=flat.dtype).scatter_reduce(0, dst[:, None].expand(-1, heads), a.detach(), reduce="amax",
                                                                               include_self=True)
    e = torch.exp(a - m[dst])
    denom = torch.zeros(n, heads, dtype=flat.dtype).index_add(0, dst, e) + 1e-16
    alpha = e / denom[dst]
    pre = torch.zeros(n, heads, D, dtype=flat.dtype).index_add(0, dst, v * alpha[..., None]).reshape(n, 128)
    return pre, m, denom


def edge_attention_loop(flat, plan, edge_index, t, heads, q_scale=1.0):
    """The same quantities by a plain loop over the raw edge lists (no plan arrays: the key rows come from ``key_row``)."""
    n, D = SIZES[t], 128 // heads
    rows = flat.view(-1, 128)
    incoming = [[] for _ in range(n)]
    for et in plan["used"]:
        if et[2] != t:
            continue
        for s, d in edge_index[et].t().tolist():
            incoming[d].append(key_row(plan, et, s))
    q = query_rows(flat, plan, t) * q_scale
    pre = torch.zeros(n, 128, dtype=flat.dtype)
    m = torch.full((n, heads), float("-inf"), dtype=flat.dtype)
    denom = torch.full((n, heads), 1e-16, dtype=flat.dtype)
    for i, keys in enumerate(incoming):
        if not keys:
            continue
        qi = q[i].view(heads, D)
        a = torch.stack([(qi * rows[r].view(heads, D)).sum(1) for r in keys])          # [edges, H]
        m[i] = a.max(0).values
        w = torch.exp(a - m[i])
        denom[i] = w.sum(0) + 1e-16
        acc = torch.zeros(heads, D, dtype=flat.dtype)
        for e, r in enumerate(keys):
            acc = acc + (w[e] / denom[i]).unsqueeze(1) * rows[r + 1].view(heads, D)
        pre[i] = acc.reshape(128)
    return pre, m, denom


@contextlib.contextmanager
def fixed_order():
    """Scatter-adds in index order.  A gather's gradient adds thousands of duplicate rows (the hub key row: 16C + 3 of them); left to
    torch's threads the float32 evaluation adds them in an order that changes from run to run (in float64 the difference is 1e-16)."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def edge_attention_items(flat, plan, t, heads, q_scale=1.0):
    """The same quantities the way the kernels cut the work: one (max, sum, weighted values) partial per work item of the plan
    (item_begin .. item_end), a destination's partials merged in item order with the rescaling of an online softmax.  Ties the
    plan's item arrays to the plain formula without a GPU."""
    pd = plan["per_dst"][t]
    n, D = int(pd["rowptr"].numel()) - 1, 128 // heads
    rows, q = flat.view(-1, 128), query_rows(flat, plan, t, 0, n) * q_scale
    pre = torch.zeros(n, 128, dtype=flat.dtype)
    m = torch.full((n, heads), float("-inf"), dtype=flat.dtype)
    denom = torch.full((n, heads), 1e-16, dtype=flat.dtype)
    first, begin, end = pd["item_ptr"].tolist(), pd["item_begin"].tolist(), pd["item_end"].tolist()
    for i in range(n):
        M, L, A = m[i].clone(), torch.zeros(heads, dtype=flat.dtype), torch.zeros(heads, D, dtype=flat.dtype)
        for it in range(first[i], first[i + 1]):
            assert int(pd["item_dst"][it]) == i and begin[it] < end[it]
            cols = pd["col"][begin[it]:end[it]]
            a = (q[i].view(1, heads, D) * rows[cols].view(-1, heads, D)).sum(-1)
            mi = a.max(0).values
            w = torch.exp(a - mi)
            li, ai = w.sum(0), (w.unsqueeze(-1) * rows[cols + 1].view(-1, heads, D)).sum(0)
            mn = torch.maximum(M, mi)
            f, g = torch.exp(M - mn), torch.exp(mi - mn)                   # (exp(-inf) = 0: the first partial replaces the empty state)
            L, A, M = L * f + li * g, A * f.unsqueeze(1) + ai * g.unsqueeze(1), mn
        if first[i + 1] > first[i]:
            pre[i], m[i], denom[i] = (A / (L + 1e-16).unsqueeze(1)).reshape(128), M, L + 1e-16
    return pre, m, denom


def attention_grads_ref(flat, plan, heads, douts, dtype=torch.float64, kv=None):
    """Autograd of sum_t <pre_t, dout_t> with the buffer the kernels read (``flat``: query slots already scaled) as the leaf.
    -> ({t: (pre, max, denom)}, gradient of the whole buffer [*, 128]).  ``kv``: the buffer the key / value rows are gathered from
    when it is not ``flat`` itself (the rounded rows of the bf16 mirror); its gradient lands in the same buffer, as the kernels write it."""
    leaf = flat.to(dtype).clone().requires_grad_(True)
    rows = None if kv is None else kv.to(dtype).clone().requires_grad_(True)
    outs, loss = {}, 0.0
    with fixed_order():
        for t in DST_TYPES:
            pre, m, den = edge_attention_ref(leaf, plan, t, heads, rows=rows)
            outs[t] = (pre.detach(), m, den.detach())
            loss = loss + (pre * douts[t].to(dtype)).sum()
        loss.backward()
    grad = leaf.grad if rows is None else leaf.grad + rows.grad
    return outs, grad.view(-1, 128)


def bf16_rows(flat):
    """What the bf16 mirror holds, as float32: every float rounded to nearest even."""
    return flat.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _ladder_reference(C, heads, q_scale, gp):
    _, plan = ladder(gp)
    return attention_grads_ref(ladder_flat(q_scale), plan, heads, ladder_douts())


def ladder_reference(gp, heads, q_scale):
    """Computed once per (heads, q_scale) and shared; the tensors are not to be changed."""
    return _ladder_reference(int(gp.HGT_CHUNK), heads, float(q_scale), gp)


def owned_mask(plan):
    """bool [total / 128, 128]: the floats some destination type's backward call writes -- the key | value rows with an outgoing
    edge and the query slots of every destination type's rows."""
    own = torch.zeros(plan["total_floats"] // 128, 128, dtype=torch.bool)
    for t in DST_TYPES:
        col = plan["per_dst"][t]["col"].cpu()
        own[col] = True
        own[col + 1] = True
        query_rows(own, plan, t)[:] = True
    return own


# ---------------------------------------------------------------------------------------------------- 3. concatenated plan
def rows_plan(plan, dst_types, sizes):
    """The destination types' plans as ONE plan (the layout ops.hgt_attention_rows documents): q_off [n_dst] float offsets of the
    query rows in the flat buffer; col as is; item_dst / item_begin / item_end / item_ptr numbered across the types."""
    q_off, col, item_dst, item_begin, item_end, item_ptr = [], [], [], [], [], [0]
    n_dst = n_edges = n_items = 0
    for t in dst_types:
        pd = plan["per_dst"][t]
        q_off += [plan["base"][t] + i * plan["width"][t] for i in range(sizes[t])]
        col += pd["col"].tolist()
        item_dst += [d + n_dst for d in pd["item_dst"].tolist()]
        item_begin += [b + n_edges for b in pd["item_begin"].tolist()]
        item_end += [e + n_edges for e in pd["item_end"].tolist()]
        item_ptr += [p + n_items for p in pd["item_ptr"].tolist()[1:]]
        n_dst += sizes[t]
        n_edges += int(pd["col"].numel())
        n_items += int(pd["item_dst"].numel())
    dev = plan["per_dst"][dst_types[0]]["col"].device
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    return {"q_off": t64(q_off), "col": t64(col), "item_dst": t64(item_dst), "item_begin": t64(item_begin), "item_end": t64(item_end),
            "item_ptr": t64(item_ptr)}


# ---------------------------------------------------------------------------------------------------- 4. composite weights
COMPOSITE_NODE_TYPES = ["x", "y", "z"]
# x: three outgoing relations; y: one; z: none, wanted as a destination (query rows only); (y, absent, x) is declared, never present
COMPOSITE_EDGE_TYPES = [("x", "e0", "y"), ("y", "e1", "z"), ("x", "e2", "z"), ("y", "absent", "x"), ("x", "e3", "x")]
COMPOSITE_ABSENT = 3
COMPOSITE_SIZES = {"x": 5, "y": 3, "z": 4}
COMPOSITE_CASES = [(1, 128), (2, 128), (4, 128), (8, 128), (4, 64), (4, 36), (4, 256), (8, 256)]          # (heads, cin)


def composite_edges():
    g = torch.Generator().manual_seed(5)
    pick = lambda t: torch.randint(0, COMPOSITE_SIZES[t], (6,), generator=g)
    return {et: torch.stack([pick(et[0]), pick(et[2])]) for i, et in enumerate(COMPOSITE_EDGE_TYPES) if i != COMPOSITE_ABSENT}


def composite_meta(types, used, edge_types, heads, cin, F=128):
    """Which relation blocks follow which type's query rows: for every projected type (in order) the used edge types that leave it
    (in the order of ``used``).  Plain ints; the row offsets follow from the order."""
    rel_r, rel_src = [], []
    for i, t in enumerate(types):
        for e in used:
            if e[0] == t:
                rel_r.append(edge_types.index(e))
                rel_src.append(i)
    return {"rel_r": rel_r, "rel_src": rel_src, "n_rel": len(rel_r), "n_types": len(types), "n_edge_types": len(edge_types), "H": heads,
            "F": F, "cin": cin}


def composite_params(heads, cin, n_types=3, n_edge_types=5, seed=900, F=128):
    """Deterministic float32 parameters: {"k_rel", "v_rel" [H*R,D,D], "w" [3F,cin] per type, "b" [3F] per type, "p" [1,H] per edge type}."""
    D = F // heads
    return {"k_rel": rand((heads * n_edge_types, D, D), seed, 1.0 / math.sqrt(D)),
            "v_rel": rand((heads * n_edge_types, D, D), seed + 1, 1.0 / math.sqrt(D)),
            "w": [rand((3 * F, cin), seed + 10 + i, 1.0 / math.sqrt(cin)) for i in range(n_types)],
            "b": [rand((3 * F,), seed + 20 + i, 0.3) for i in range(n_types)],
            "p": [1.0 + rand((1, heads), seed + 30 + r, 0.3) for r in range(n_edge_types)]}


def composite_rows(meta):
    return meta["F"] * meta["n_types"] + 2 * meta["F"] * meta["n_rel"]


def composite_ref(p, meta):
    """big_w [rows, cin], big_b [rows] by the formula at the head of csrc/hgt_params.hip: per type its Q rows, then for every used
    relation r leaving it  K_r[(h,b),c] = sum_a k_rel[h,r][a,b] p_rel[r][h] / sqrt(D) Wk[(h,a),c]  and  V_r likewise without the
    scale; the bias is the extra column."""
    H, F, R, cin = meta["H"], meta["F"], meta["n_edge_types"], meta["cin"]
    D = F // H
    rel_r, rel_src = [int(v) for v in meta["rel_r"]][:meta["n_rel"]], [int(v) for v in meta["rel_src"]][:meta["n_rel"]]
    k_rel, v_rel = p["k_rel"].view(H, R, D, D), p["v_rel"].view(H, R, D, D)
    ws, bs = [], []
    for i in range(meta["n_types"]):
        W = torch.cat([p["w"][i], p["b"][i].unsqueeze(1)], 1).view(3, H, D, cin + 1)              # K | Q | V rows, the bias as column cin
        ws.append(W[1].reshape(F, cin + 1))
        for r, s in zip(rel_r, rel_src):
            if s != i:
                continue
            mk = k_rel[:, r] * (p["p"][r].view(H, 1, 1) / math.sqrt(D))
            ws.append(torch.einsum("hab,hac->hbc", mk, W[0]).reshape(F, cin + 1))
            ws.append(torch.einsum("hab,hac->hbc", v_rel[:, r], W[2]).reshape(F, cin + 1))
    big = torch.cat(ws, 0)
    return big[:, :cin], big[:, cin]


def composite_leaves(p, dtype):
    return {k: ([t.to(dtype).clone().requires_grad_(True) for t in v] if isinstance(v, list) else v.to(dtype).clone().requires_grad_(True))
            for k, v in p.items()}


def composite_grads_ref(p, meta, dbig_w, dbig_b, dtype=torch.float64):
    """-> (big_w, big_b, {name: gradient or list of gradients}) by autograd in ``dtype``; a parameter the rows do not depend on
    (the absent edge type's p_rel) gets zeros."""
    leaves = composite_leaves(p, dtype)
    big_w, big_b = composite_ref(leaves, meta)
    ((big_w * dbig_w.to(dtype)).sum() + (big_b * dbig_b.to(dtype)).sum()).backward()
    g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return big_w.detach(), big_b.detach(), {k: ([g(t) for t in v] if isinstance(v, list) else g(v)) for k, v in leaves.items()}


def composite_cotangents(rows, cin, seed=950):
    return rand((rows, cin), seed), rand((rows,), seed + 1)


# ---------------------------------------------------------------------------------------------------- 5. small references
def gated_residual_ref(o, x, skip):
    s = torch.sigmoid(skip)
    return s * o + (1 - s) * x


GATE_ROWS = [1, 5, 300]
GATE_SKIPS = [0.0, 0.7, -0.7, 12.0, -12.0]


def gate_inputs(rows, cols=128):
    return rand((rows, cols), 40 + rows), rand((rows, cols), 41 + rows), rand((rows, cols), 42 + rows)              # o, x, dout


def gate_grads_ref(o, x, skip, dout, dtype=torch.float64):
    """-> (out, d_o, d_x, d_skip [1]) by autograd in ``dtype``."""
    o, x = o.to(dtype).clone().requires_grad_(True), x.to(dtype).clone().requires_grad_(True)
    s = torch.tensor([skip], dtype=dtype, requires_grad=True)
    out = gated_residual_ref(o, x, s)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), o.grad, x.grad, s.grad


def csr_ref(x, rowptr, col, weight=None, mean=False, x_self=None, self_coef=0.0):
    """out[v] = self_coef * x_self[v] + sum_{e in row v} w[e] x[col[e]]  (mean: the sum divided by max(len(row), 1))."""
    n = int(rowptr.numel()) - 1
    cnt = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(n), cnt)
    msg = x[col] if weight is None else x[col] * weight.to(x.dtype).unsqueeze(1)
    out = torch.zeros(n, x.shape[1], dtype=x.dtype).index_add(0, dst, msg)
    if mean:
        out = out / cnt.clamp_min(1).to(x.dtype).unsqueeze(1)
    if x_self is not None:
        out = out + self_coef * x_self
    return out


CSR_F = [4, 32, 36, 64, 132, 252]
CSR_N_DST = [1, 7, 257]
CSR_DEGREES = [5, 0, 1, 3, 4, 8, 9]
CSR_N_SRC = 50


def csr_case(F, n_dst, pad=12):
    """-> (wide [n_src, F + pad] whose columns 4 .. 4 + F are x, rowptr, col, weights, x_self, dout).  Destination v has
    CSR_DEGREES[v % 7] incoming edges: every degree of the list is present from n_dst = 7 on."""
    g = torch.Generator().manual_seed(1000 + F + n_dst)
    deg = torch.tensor([CSR_DEGREES[v % len(CSR_DEGREES)] for v in range(n_dst)])
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    col = torch.randint(0, CSR_N_SRC, (E,), generator=g)
    wide = rand((CSR_N_SRC, F + pad), 1100 + F)
    return wide, rowptr, col, torch.rand(E, generator=g) + 0.5, rand((n_dst, F), 1200 + F), rand((n_dst, F), 1300 + F)
