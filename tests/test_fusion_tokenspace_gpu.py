"""Layer 0 of the fusion transformer in the 128-wide token space (TransformerFusion._layer0_tokenspace): the generalised attention
entry (ops.fusion_attention_qkv), the token-row kernel (ops.token_scaled_rows) and the module path against the composed-QKV path
(compose_layer0_attn = False) on the same module."""
import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

F8 = torch.float64
ATT_BOUND = 2e-5                                             # the attention kernel's fp32 bound (test_ops_gpu.test_fusion_attention)
BOUND = {"f32": 3e-5, "bf16x3": 1e-4, "bf16": 3e-2}          # of the output scale, as for the composed QKV block
SHIPPED = [   # name, heads, head_dim, ffn, layers, norm_first, agg, bottlenecks, act (configs.SHIPPED)
    ("drugbank163", 8, 64, 256, 2, True, "x-attn", 4, "gelu"),
    ("twosides105", 2, 256, 512, 2, True, "x-attn", 2, "gelu"),
    ("twosides321", 8, 256, 1024, 2, True, "x-attn", 2, "gelu"),
]


@pytest.fixture(scope="module")
def M():
    import madrigal_amd.models as _m
    return _m


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _o
    return _o


# ------------------------------------------------------------------------------------------ the generalised attention
def _attention_ref(q, k, v, tiles, H, w, hq, hk, hv, blocked, qscale):
    """fp64: per tile (first row, rows) and head, softmax over the allowed keys of q_h k_h^T * qscale, times v_h -> [R, H*w]."""
    q, k, v = q.double(), k.double(), v.double()
    out = torch.zeros(q.shape[0], H * w, dtype=F8)
    for (b, T) in tiles:
        for h in range(H):
            qh, kh, vh = q[b:b + T, h * hq:h * hq + w], k[b:b + T, h * hk:h * hk + w], v[b:b + T, h * hv:h * hv + w]
            lg = (qh @ kh.T * qscale).masked_fill(blocked[b:b + T, :T], float("-inf"))
            out[b:b + T, h * w:(h + 1) * w] = torch.softmax(lg, -1) @ vh
    return out


def _operands(R, H, w, shared, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(R, H * w, generator=g)
    kw = w if shared else H * w
    return q, torch.randn(R, kw, generator=g), torch.randn(R, kw, generator=g), (0 if shared else w)


def _run_qkv(ops, q, k, v, n, S, H, w, step, qscale, **masks):
    """Into an output whose row stride exceeds its width; the columns behind the heads must stay as they were."""
    buf = torch.full((q.shape[0], H * w + 20), 7.0, device="cuda")
    ops.fusion_attention_qkv(q.cuda(), k.cuda(), v.cuda(), n, S, H, w, w, hq=w, hk=step, hv=step, out=buf, ho=w, qscale=qscale, **masks)
    assert bool((buf[:, H * w:] == 7.0).all())
    return buf[:, :H * w].cpu()


@pytest.mark.parametrize("shared", [True, False], ids=["shared_kv", "per_head_kv"])
@pytest.mark.parametrize("w", [132, 64])
@pytest.mark.parametrize("H", [1, 8])
def test_attention_qkv_compact_tiles(ops, H, w, shared):
    """Tiles of 1, 5 and 32 live rows with per-row bit masks (width 132: a partial last 64-column piece)."""
    tiles = [(0, 1), (1, 5), (6, 32)]
    R = 38
    q, k, v, step = _operands(R, H, w, shared, 50 + H + w)
    g = torch.Generator().manual_seed(3)
    blocked = torch.rand(R, 32, generator=g) < 0.3
    blocked[torch.arange(R), torch.tensor([r - b for (b, T) in tiles for r in range(b, b + T)])] = False      # a row may attend itself
    row_bits = ops.mask_bits(blocked.cuda())
    tile_start = torch.tensor([0, 1, 6, 38], dtype=torch.int64, device="cuda")
    got = _run_qkv(ops, q, k, v, 3, 32, H, w, step, 0.37, row_start=tile_start, row_bits=row_bits)
    want = _attention_ref(q, k, v, tiles, H, w, w, step, step, blocked, np.float32(0.37).item())
    assert rel_err(got, want) <= ATT_BOUND


@pytest.mark.parametrize("S", [1, 5, 32])
@pytest.mark.parametrize("w", [132, 64])
@pytest.mark.parametrize("H", [1, 8])
def test_attention_qkv_dense_masks(ops, H, w, S):
    """Dense layout, key-padding and source masks, one key and value block shared by the heads."""
    n = 3
    q, k, v, step = _operands(n * S, H, w, True, 60 + H + w + S)
    g = torch.Generator().manual_seed(5)
    kpm = torch.rand(n, S, generator=g) < 0.3
    kpm[:, min(2, S - 1)] = False                        # one key everyone may attend (the source mask leaves it open too)
    src = torch.zeros(S, S, dtype=torch.bool)
    if S > 4:
        src[:2, -2:] = True
        src[-2:, :2] = True
    blocked = torch.zeros(n * S, 32, dtype=torch.bool)
    blocked[:, :S] = (kpm.view(n, 1, S) | src.view(1, S, S)).reshape(n * S, S)
    got = _run_qkv(ops, q, k, v, n, S, H, w, step, 1.0, kpm_bits=ops.mask_bits(kpm.cuda()), src_bits=ops.mask_bits(src.cuda()))
    want = _attention_ref(q, k, v, [(i * S, S) for i in range(n)], H, w, w, step, step, blocked, 1.0)
    assert rel_err(got, want) <= ATT_BOUND


@pytest.mark.parametrize("H,dh", [(8, 64), (2, 256), (4, 32)])
def test_old_entry_equals_the_view_call(ops, H, dh):
    """mdg_fusion_attention on a q|k|v tensor and the generalised entry on its three column views: the same bits, dense with masks
    and compact."""
    n, S, d = 5, 19, H * dh
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(n * S, 3 * d, generator=g).cuda()
    qs = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
    kb = ops.mask_bits((torch.rand(n, S, generator=g) < 0.3).cuda() & (torch.arange(S, device="cuda") != 3))
    src = torch.zeros(S, S, dtype=torch.bool)
    src[:2, -2:] = True
    sb = ops.mask_bits(src.cuda())
    views = (qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:])
    old = ops.fusion_attention(qkv, n, S, H, dh, kb, sb)[0]
    new = ops.fusion_attention_qkv(*views, n, S, H, dh, dh, hq=dh, hk=dh, hv=dh, kpm_bits=kb, src_bits=sb, qscale=qs)
    assert torch.equal(old, new)
    starts = torch.tensor([0, 7, 8, 40, 63, 95], dtype=torch.int64, device="cuda")              # tiles of 7, 1, 32, 23 and 32 rows
    bits = (torch.randint(0, 2 ** 31, (n * S,), generator=g) & ~1).to(torch.int32).cuda()       # key 0 of its tile is open to every row
    old = ops.fusion_attention(qkv, 5, S, H, dh, row_start=starts, row_bits=bits)[0]
    new = ops.fusion_attention_qkv(*views, 5, S, H, dh, dh, hq=dh, hk=dh, hv=dh, row_start=starts, row_bits=bits, qscale=qs)
    assert torch.isfinite(old).all() and torch.equal(old, new)


# ------------------------------------------------------------------------------------------ token rows -> X, r, tail
@pytest.mark.parametrize("R", [1, 333])
def test_token_scaled_rows(ops, R):
    """X = r [T, 1, 0, 0, 0], r = 1 / sqrt(|R_f [T; 1]|^2 / d + eps) and the copy of T, against fp64; the last row is all zeros (its
    factor comes from the bias column alone).  r's bound is ops.row_rstd's: 129-term fp32 dot products, then a sum of squares."""
    D, Dp, d, eps = 128, 132, 2048, 1e-5
    g = torch.Generator().manual_seed(R)
    T = torch.randn(R, D, generator=g) + 0.5
    T[-1] = 0.0
    Rf = torch.zeros(D + 1, Dp)
    Rf[:, :D + 1] = torch.randn(D + 1, D + 1, generator=g).triu()
    buf = torch.full((R, 40 + D), 7.0, device="cuda")
    X, r = ops.token_scaled_rows(T.cuda(), Rf.cuda(), d, eps, buf[:, 40:])
    t1 = torch.cat([T.double(), torch.ones(R, 1, dtype=F8)], 1)
    want_r = 1.0 / torch.sqrt((t1 @ Rf[:, :D + 1].double().T).pow(2).sum(1) / d + eps)
    assert rel_err(r.cpu(), want_r) <= 1e-5
    assert float(((r.cpu().double() - want_r).abs() / want_r).max()) <= 1e-5
    assert rel_err(X[:, :D + 1].cpu(), want_r[:, None] * t1) <= 1e-5
    assert not X[:, D + 1:].any() and torch.equal(X[-1, :D], torch.zeros(D, device="cuda"))
    assert torch.equal(buf[:, 40:].cpu(), T) and bool((buf[:, :40] == 7.0).all())


# ------------------------------------------------------------------------------------------ the module
def _module(M, case, norm_first=None, seed=41):
    from oracle.params import fill_module
    name, H, dh, ffn, nl, nf, agg, nb, actn = case
    m = M.TransformerFusion(128, nb, nl, H, dh, ffn, 0.3, actn, nf if norm_first is None else norm_first, False, agg)
    fill_module(m, seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                   # non-trivial norm1 affine: the fold must carry it
        L0 = m.transformer_encoder.layers[0]
        L0.norm1.weight.copy_(1.0 + 0.3 * torch.randn(L0.norm1.weight.shape, generator=g))
        L0.norm1.bias.copy_(0.2 * torch.randn(L0.norm1.bias.shape, generator=g))
    return m.cuda().eval()


def _inputs(m, n, seed=7):
    from madrigal_amd.data import NUM_NON_TX_MODALITIES
    S, nb = m.x_attn_key_padding_mask.shape[1], m.num_tx_bottlenecks
    g = torch.Generator().manual_seed(seed)
    seq = torch.randn(n, S, 128, generator=g) + 0.5                    # token rows with a common offset
    kpm = torch.rand(n, S, generator=g) < 0.6                          # ~40 % live tokens ...
    kpm[:, NUM_NON_TX_MODALITIES:NUM_NON_TX_MODALITIES + nb] = False  # ... and the bottleneck (key) tokens always
    return seq.cuda(), kpm.cuda()


def _run(M, m, seq, kpm, prec, live, tokenspace, grad=False):
    m.compose_layer0_attn = tokenspace
    with torch.set_grad_enabled(grad), M.precision(prec):
        if live:
            plan = m.live_token_plan(kpm, None)
            tokens = seq.reshape(-1, 128).index_select(0, plan["token_index"]).contiguous()
            return m.forward_tokens(tokens, plan).detach().cpu()
        return m(seq, kpm).detach().cpu()


def _entry(m, prec="bf16x3"):
    return m.__dict__.get("_mdg_derived", {}).get(("layer0_ts", prec))


@pytest.mark.parametrize("live", [True, False], ids=["live", "dense"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", SHIPPED, ids=[c[0] for c in SHIPPED])
def test_tokenspace_layer0_matches_composed_qkv(M, case, prec, live):
    m = _module(M, case)
    seq, kpm = _inputs(m, 37)
    want = _run(M, m, seq, kpm, prec, live, False)
    got = _run(M, m, seq, kpm, prec, live, True)
    assert torch.isfinite(got).all()
    if case[0] == "drugbank163":                            # K' = 1184 > d = 512: the predicate keeps the composed-QKV path
        assert _entry(m, prec) is None and torch.equal(got, want)
    else:
        assert _entry(m, prec) is not None                  # the token-space path ran
        err = rel_err(got, want)
        print(f"{case[0]} {prec} {'live' if live else 'dense'}: rel err {err:.2e}")
        assert err <= BOUND[prec]


@pytest.mark.parametrize("which", ["post_norm", "hooked", "training"])
def test_other_paths_keep_their_bits(M, which):
    """Post-norm layers, a forward hook on the last attention module and the autograd path do not take the token-space path."""
    m = _module(M, SHIPPED[2], norm_first=False if which == "post_norm" else None)
    seq, kpm = _inputs(m, 37)
    if which == "hooked":
        m.transformer_encoder.layers[-1].self_attn.register_forward_hook(lambda mod, i, o: None)
    grad = which == "training"
    for live in ((False,) if which == "hooked" else (True, False)):
        want = _run(M, m, seq, kpm, "bf16x3", live, False, grad)
        assert torch.equal(_run(M, m, seq, kpm, "bf16x3", live, True, grad), want)
    assert _entry(m) is None


def test_composites_follow_in_place_parameter_changes(M):
    """The composites and their images are cached on the module: a second call reuses them as they are, an in-place change of any
    source parameter rebuilds them."""
    m = _module(M, SHIPPED[2])
    seq, kpm = _inputs(m, 37)
    L0 = m.transformer_encoder.layers[0]
    sa = L0.self_attn
    g = torch.Generator().manual_seed(11)
    before = _run(M, m, seq, kpm, "bf16x3", True, True)
    first = _entry(m)
    assert torch.equal(_run(M, m, seq, kpm, "bf16x3", True, True), before)
    assert _entry(m) is first and all(a is b for a, b in zip(_entry(m)[1], first[1]))
    for p in (m.embed2latent.weight, m.embed2latent.bias, L0.norm1.weight, L0.norm1.bias, sa.in_proj_weight, sa.in_proj_bias,
              sa.out_proj.weight, sa.out_proj.bias):
        with torch.no_grad():                              # (a perturbation, not a factor: the later norms undo a scaled embed2latent)
            p.add_(0.3 * (p.abs().mean() + 0.1) * torch.randn(p.shape, generator=g).cuda())
        held = _entry(m)
        got = _run(M, m, seq, kpm, "bf16x3", True, True)
        assert _entry(m) is not held
        assert rel_err(got, before) > 1e-4
        assert rel_err(got, _run(M, m, seq, kpm, "bf16x3", True, False)) <= BOUND["bf16x3"]
        before = got
