"""The last fusion layer with queries and attention rows for the kept rows only: ops.layernorm_packed_kept,
ops.fusion_attention_kept and TransformerFusion.compact_last_queries against the kernels and the path they stand for."""
import copy

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

BOUND = {"f32": 3e-5, "bf16x3": 1e-4, "bf16": 3e-2}       # tests/test_fusion_compose_gpu.py's bounds for a path switch
CASES = [   # name, heads, head_dim, ffn, layers, norm_first, agg, bottlenecks, act: configs.SHIPPED, and a cls pooling
    ("drugbank163", 8, 64, 256, 2, True, "x-attn", 4, "gelu"),
    ("twosides105", 2, 256, 512, 2, True, "x-attn", 2, "gelu"),
    ("twosides321", 8, 256, 1024, 2, True, "x-attn", 2, "gelu"),
    ("cls", 4, 64, 256, 2, True, "cls", 2, "gelu"),
]


@pytest.fixture(scope="module")
def M():
    import madrigal_amd.models as _m
    return _m


# ---------------------------------------------------------------------------------------------- attention
def _tiles():
    """Seven tiles as (rows, kept rows, {row: blocked key bits}); every row may attend itself."""
    five_drugs = {r: (~(0b11111 << (5 * (r // 5)))) & ((1 << 25) - 1) for r in range(25)}       # 5 drugs of 5 rows: own drug only
    return [
        (32, [0, 3, 4, 17, 30, 31], {5: 0b1010, 17: 1 << 31 | 1}),                 # a full tile, kept rows at both ends
        (1, [0], {}),                                                               # a tile of one row
        (25, [5 * g + o for g in range(5) for o in (1, 2)], five_drugs),            # several drugs, two kept rows each
        (10, [4], {4: 0b10000011}),                                                 # its only kept row is blocked from keys 0, 1, 7
        (17, [0, 16], {0: 0b110, 16: 0b1}),                                         # kept rows first and last
        (9, [], {2: 0b1}),                                                          # no kept row
        (31, [1, 2, 7, 11, 13, 29], {11: 0x55555555 & ~(1 << 11)}),
    ]


def _attention_case(H, dh, seed=5):
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    starts, keep, bits = [0], [], []
    for T, kept, blocked in _tiles():
        keep += [starts[-1] + r for r in kept]
        bits += [blocked.get(r, 0) for r in range(T)]
        starts.append(starts[-1] + T)
    R, n_keep = starts[-1], len(keep)
    assert n_keep % 4 != 0
    qkv = torch.randn(R, 3 * d, generator=g).cuda()
    keep = torch.tensor(keep, dtype=torch.int64, device="cuda")
    q_slot = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    q_slot[keep] = torch.arange(n_keep, dtype=torch.int32, device="cuda")
    row_bits = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32, device="cuda")
    return qkv, keep, q_slot, row_bits, torch.tensor(starts, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("H,dh", [(1, 64), (2, 64), (8, 256)])
def test_kept_attention_equals_the_full_kernel_on_kept_rows(H, dh):
    from madrigal_amd import ops
    d = H * dh
    qkv, keep, q_slot, row_bits, row_start = _attention_case(H, dh)
    n_tiles = row_start.numel() - 1
    with torch.no_grad():
        want = ops.fusion_attention(qkv, n_tiles, 32, H, dh, row_start=row_start, row_bits=row_bits)[0].index_select(0, keep)
        assert torch.isfinite(want).all()
        q = qkv[:, :d].index_select(0, keep).contiguous()
        dead = torch.ones(qkv.shape[0], dtype=torch.bool, device="cuda")
        dead[keep] = False
        qkv[:, :d][dead] = float("nan")                      # k and v stay views of this buffer: a dead query slot read shows as NaN
        got = ops.fusion_attention_kept(q, qkv[:, d:2 * d], qkv[:, 2 * d:], n_tiles, H, dh, row_start, row_bits, q_slot)
        again = ops.fusion_attention_kept(q, qkv[:, d:2 * d], qkv[:, 2 * d:], n_tiles, H, dh, row_start, row_bits, q_slot)
    assert got.shape == (keep.numel(), d)
    assert torch.equal(got, want)
    assert torch.equal(again, got)


def test_kept_attention_writes_kept_rows_only():
    """Rows of ``out`` that no slot names stay as they were, and a slot outside ``out`` is a row that is not kept."""
    from madrigal_amd import ops
    H, dh = 2, 64
    d = H * dh
    qkv, keep, q_slot, row_bits, row_start = _attention_case(H, dh)
    n_tiles, n_keep = row_start.numel() - 1, keep.numel()
    q = qkv[:, :d].index_select(0, keep).contiguous()
    with torch.no_grad():
        full = ops.fusion_attention_kept(q, qkv[:, d:2 * d], qkv[:, 2 * d:], n_tiles, H, dh, row_start, row_bits, q_slot)
        out = torch.full((n_keep - 3, d), 7.0, device="cuda")
        ops.fusion_attention_kept(q[:n_keep - 3], qkv[:, d:2 * d], qkv[:, 2 * d:], n_tiles, H, dh, row_start, row_bits, q_slot, out=out)
        assert torch.equal(out, full[:n_keep - 3])
        none = torch.full((n_keep, d), 7.0, device="cuda")
        ops.fusion_attention_kept(q, qkv[:, d:2 * d], qkv[:, 2 * d:], n_tiles, H, dh, row_start, row_bits, torch.full_like(q_slot, -1), out=none)
        assert bool((none == 7.0).all())


# ---------------------------------------------------------------------------------------------- norm
def _slot_maps(R):
    maps = {"none": [], "all": list(range(R)), "last": [R - 1]}
    if R > 3:
        maps["every third"] = list(range(1, R, 3))
    return maps


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("R", [1, 33, 257])
@pytest.mark.parametrize("d", [64, 2048])
def test_kept_norm_images(d, R, prec):
    from madrigal_amd import ops
    g = torch.Generator().manual_seed(d + R)
    x = (torch.randn(R, d, generator=g) * 2 + 0.5).cuda()
    w, b = (1 + 0.3 * torch.randn(d, generator=g)).cuda(), (0.2 * torch.randn(d, generator=g)).cuda()
    used = lambda rows: rows * d * (4 if prec == "bf16x3" else 2)            # an image's bytes ahead of its alignment padding
    with torch.no_grad():
        y, img = ops.layernorm_packed(x, w, b, 1e-5, prec)
        for name, kept in _slot_maps(R).items():
            rows = torch.tensor(kept, dtype=torch.int64, device="cuda")
            q_slot = torch.full((R,), -1, dtype=torch.int32, device="cuda")
            q_slot[rows] = torch.arange(len(kept), dtype=torch.int32, device="cuda")
            got, got_kept = ops.layernorm_packed_kept(x, w, b, 1e-5, prec, q_slot, len(kept))
            assert torch.equal(got[:used(R)], img[:used(R)]), name
            if kept:
                want = ops.pack_operand(y.index_select(0, rows), prec)
                assert got_kept.numel() == want.numel() and torch.equal(got_kept[:used(len(kept))], want[:used(len(kept))]), name
            else:
                assert got_kept.numel() == 0


def test_kept_norm_takes_no_image_in_f32_or_at_odd_widths():
    from madrigal_amd import ops
    q_slot = torch.zeros(5, dtype=torch.int32, device="cuda")
    for d, prec in ((64, "f32"), (96, "bf16x3")):
        x, w, b = torch.randn(5, d).cuda(), torch.ones(d).cuda(), torch.zeros(d).cuda()
        assert ops.layernorm_packed_kept(x, w, b, 1e-5, prec, q_slot, 1) is None


# ---------------------------------------------------------------------------------------------- module
def _module(M, case, norm_first=None, dropout=0.3, seed=43):
    from oracle.params import fill_module
    name, H, dh, ffn, nl, nf, agg, nb, actn = case
    m = M.TransformerFusion(128, nb, nl, H, dh, ffn, dropout, actn, nf if norm_first is None else norm_first, False, agg)
    fill_module(m, seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                   # a non-trivial norm1 affine in the last layer
        L = m.transformer_encoder.layers[-1]
        L.norm1.weight.copy_(1.0 + 0.3 * torch.randn(L.norm1.weight.shape, generator=g))
        L.norm1.bias.copy_(0.2 * torch.randn(L.norm1.bias.shape, generator=g))
    return m.cuda().eval()


def _inputs(m, n=37, seed=11):
    """Token rows and a ragged padding mask: ~40 % of the tokens live, the pooled ones (bottlenecks, a leading cls) always."""
    from madrigal_amd.data import NUM_MODALITIES, NUM_NON_TX_MODALITIES
    nb, has_cls = m.num_tx_bottlenecks, 1 if m.transformer_agg == "cls" else 0
    S = has_cls + NUM_MODALITIES + nb
    g = torch.Generator().manual_seed(seed)
    seq = torch.randn(n, S, 128, generator=g) + 0.5
    kpm = torch.rand(n, S, generator=g) < 0.6
    kpm[:, :has_cls] = False
    kpm[:, has_cls + NUM_NON_TX_MODALITIES:has_cls + NUM_NON_TX_MODALITIES + nb] = False
    kpm[3, has_cls + NUM_NON_TX_MODALITIES + nb:] = True                    # one drug with hardly more than its pooled tokens
    kpm = kpm.cuda()
    plan = m.live_token_plan(kpm, None)
    tokens = seq.cuda().reshape(-1, 128).index_select(0, plan["token_index"]).contiguous()
    return tokens, plan


class _Spy:
    """Records the operands and results of the two attention wrappers while a module runs."""

    def __init__(self, monkeypatch, ops):
        self.full, self.kept = [], []
        real_full, real_kept = ops.fusion_attention, ops.fusion_attention_kept

        def full(qkv, *a, **kw):
            out = real_full(qkv, *a, **kw)
            self.full.append((qkv, out[0]))
            return out

        def kept(q, k, v, *a, **kw):
            out = real_kept(q, k, v, *a, **kw)
            self.kept.append((q, k, v, out))
            return out
        monkeypatch.setattr(ops, "fusion_attention", full)
        monkeypatch.setattr(ops, "fusion_attention_kept", kept)

    def clear(self):
        del self.full[:], self.kept[:]


def _forward(M, m, tokens, plan, prec, on):
    m.compact_last_queries = on
    with torch.no_grad(), M.precision(prec):
        return m.forward_tokens(tokens, plan)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_module_switch_on_against_off(M, monkeypatch, case, prec):
    from madrigal_amd import ops
    m = _module(M, case)
    tokens, plan = _inputs(m)
    keep, d = plan["key_rows"], m.latent_dim
    assert plan["R"] >= 4 * keep.numel() // 3              # the size rule admits the split in_proj block
    spy = _Spy(monkeypatch, ops)
    want = _forward(M, m, tokens, plan, prec, False)
    assert not spy.kept
    qkv_off, att_off = spy.full[-1]
    n_full = len(spy.full)
    spy.clear()
    got = _forward(M, m, tokens, plan, prec, True)
    assert torch.isfinite(got).all()
    err = rel_err(got.cpu(), want.cpu())
    print(f"{case[0]} {prec}: z switch on against off, max|d| / max|z| = {err:.3e}")
    assert err <= BOUND[prec]
    if prec == "f32":                                       # no operand image: the rule keeps the other path and its bits
        assert not spy.kept and torch.equal(got, want)
        return
    assert len(spy.kept) == 1 and len(spy.full) == n_full - 1          # the last layer's attention, and only it, took the new kernel
    q, k, v, att_on = spy.kept[0]
    assert torch.equal(torch.cat([k, v], 1), qkv_off[:, d:])                           # the K|V block
    same_q = torch.equal(q, qkv_off[:, :d].index_select(0, keep))
    print(f"{case[0]} {prec}: Q block bit-equal to the gathered-row block: {same_q}")
    ref = qkv_off.clone()
    ref[:, :d] = 0.0
    ref[:, :d].index_copy_(0, keep, q)                      # the full kernel on the same K|V and these queries
    with torch.no_grad():
        att_ref = ops.fusion_attention(ref, plan["n_tiles"], plan["S"], m.num_heads, m.head_dim, row_start=plan["tile_start"],
                                       row_bits=plan["row_bits"])[0].index_select(0, keep)
    assert torch.equal(att_on, att_ref)
    if same_q:
        assert torch.equal(att_on, att_off.index_select(0, keep))


def test_post_norm_and_training_keep_their_path(M, monkeypatch):
    from madrigal_amd import ops
    spy = _Spy(monkeypatch, ops)
    m = _module(M, CASES[0], norm_first=False)
    tokens, plan = _inputs(m)
    assert torch.equal(_forward(M, m, tokens, plan, "bf16x3", True), _forward(M, m, tokens, plan, "bf16x3", False))
    base = _module(M, CASES[0], dropout=0.0)
    outs = []
    for on in (False, True):                                # train()
        t = copy.deepcopy(base).train()
        t.compact_last_queries = on
        with M.precision("bf16x3"):
            outs.append(t.forward_tokens(tokens, plan).detach().clone())
    assert torch.equal(outs[0], outs[1])
    outs = []
    for on in (False, True):                                # eval(), but a gradient is wanted for the token rows
        t = copy.deepcopy(base).eval()
        for p in t.parameters():
            p.requires_grad_(False)
        t.compact_last_queries = on
        with M.precision("bf16x3"):
            o = t.forward_tokens(tokens.clone().requires_grad_(True), plan)
        assert o.requires_grad
        outs.append(o.detach().clone())
    assert torch.equal(outs[0], outs[1])
    assert not spy.kept


def test_a_last_layer_that_is_layer_0_keeps_its_path(M, monkeypatch):
    from madrigal_amd import ops
    spy = _Spy(monkeypatch, ops)
    name, H, dh, ffn, nl, nf, agg, nb, actn = CASES[0]
    m = _module(M, (name, H, dh, ffn, 1, nf, agg, nb, actn))
    tokens, plan = _inputs(m)
    assert torch.equal(_forward(M, m, tokens, plan, "bf16x3", True), _forward(M, m, tokens, plan, "bf16x3", False))
    assert not spy.kept


def test_second_call_packs_nothing_and_copies_nothing(M, monkeypatch):
    """Steady state of the new route: no operand image is packed by a launch of its own, no derived tensor is rebuilt, no row is
    scattered, and the one gather left is the residual's."""
    from madrigal_amd import _lib
    m = _module(M, CASES[2])
    tokens, plan = _inputs(m)
    first = _forward(M, m, tokens, plan, "bf16x3", True)
    L = _lib.lib()
    packs, moved = [], {"index_select": 0, "index_copy_": 0}
    real = L.mdg_pack_operand

    def counting(*a):
        packs.append(1)
        return real(*a)
    monkeypatch.setattr(L, "mdg_pack_operand", counting)
    for name in moved:
        def counted(self, *a, _real=getattr(torch.Tensor, name), _name=name, **kw):
            moved[_name] += 1
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    derived = dict(m.__dict__.get("_mdg_derived", {}))
    on = _forward(M, m, tokens, plan, "bf16x3", True)
    assert not packs and moved == {"index_select": 1, "index_copy_": 0}
    again = m.__dict__.get("_mdg_derived", {})
    assert derived.keys() == again.keys() and all(derived[k] is again[k] for k in derived)
    assert torch.equal(on, first)
    moved.update(index_select=0, index_copy_=0)
    _forward(M, m, tokens, plan, "bf16x3", False)
    assert not packs and moved == {"index_select": 3, "index_copy_": 1}            # the path it replaces: three gathers and a scatter
