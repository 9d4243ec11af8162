"""ops.linear_chain (mdg_linear_chain128: a chain of 128-wide dense blocks in one launch) against the chain of ops.linear
calls it stands for -- bit for bit -- and against an fp64 evaluation of the same chain."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 127, 128, 129, 333]          # partial panel, the panel edges of both panel heights, several panels
K_FIRST = [20, 68, 128]
# fp64 anchor, relative to the output scale: the project's bound for dense blocks (bf16x3 fp32-grade, bf16 single product)
TOL = {"bf16x3": 1e-4, "bf16": 3e-2}
# (MLP stages, edge stage, scale/shift on the last stage, activation, index of the stage whose bias is None)
CONFIGS = [
    (3, True, True, "relu", None),
    (3, False, True, "relu", 1),
    (3, True, False, "relu", 2),
    (2, True, False, None, None),
    (2, False, True, "relu", 0),
    (1, True, True, "relu", None),
    (1, False, False, None, None),
]


@pytest.fixture(scope="module")
def ops():
    import madrigal_amd.ops as _o
    return _o


def _case(M, K, n, edge, affine, none_bias, seed):
    g = torch.Generator().manual_seed(seed)

    def r(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).cuda()
    x = r(M, K)
    x[::5] = 0.0                                   # rows of exact zeros
    ws = [r(128, K if j == 0 else 128, s=(K if j == 0 else 128) ** -0.5) for j in range(n)]
    bs = [None if j == none_bias else r(128, s=0.5) - 0.25 for j in range(n)]       # negative pre-activations: ReLU cuts
    c = dict(x=x, ws=ws, bs=bs, e=None, we=None, scale=None, shift=None)
    if edge:
        c["e"] = r(M, 20)
        c["e"][::7] = 0.0
        c["we"] = r(K, 20, s=0.2)
    if affine:
        c["scale"] = torch.rand(128, generator=g).cuda() + 0.5
        c["shift"] = r(128, s=0.3)
    return c


def _unfused(ops, c, act, prec):
    u = c["x"]
    if c["e"] is not None:
        u = ops.linear(c["e"], c["we"], None, residual=u, precision=prec)
    n = len(c["ws"])
    for j, (w, b) in enumerate(zip(c["ws"], c["bs"])):
        last = j == n - 1
        u = ops.linear(u, w, b, scale=c["scale"] if last else None, shift=c["shift"] if last else None, act=act, precision=prec)
    return u


def _fp64(c, act):
    f = (lambda v: v.clamp_min(0)) if act == "relu" else (lambda v: v)
    u = c["x"].double()
    if c["e"] is not None:
        u = c["e"].double() @ c["we"].double().T + u
    n = len(c["ws"])
    for j, (w, b) in enumerate(zip(c["ws"], c["bs"])):
        u = u @ w.double().T
        if b is not None:
            u = u + b.double()
        if j == n - 1 and c["scale"] is not None:
            u = u * c["scale"].double() + c["shift"].double()
        u = f(u)
    return u


def _fused(ops, c, act, prec, out=None):
    return ops.linear_chain(c["x"], c["ws"], c["bs"], edge=c["e"], edge_weight=c["we"], scale=c["scale"], shift=c["shift"], act=act,
                            precision=prec, out=out)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("M", ROWS)
def test_chain_equals_unfused_and_fp64(ops, prec, M):
    seed = 0
    for K in K_FIRST:
        for n, edge, affine, act, none_bias in CONFIGS:
            seed += 1
            c = _case(M, K, n, edge, affine, none_bias, seed)
            want = _unfused(ops, c, act, prec)
            got = _fused(ops, c, act, prec)
            tag = f"M={M} K={K} stages={n} edge={edge} affine={affine} act={act} none_bias={none_bias}"
            assert torch.equal(got, want), tag
            ref = _fp64(c, act)
            err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            assert err <= TOL[prec], (tag, err)
            if act == "relu":
                assert (got == 0).any() and (got > 0).any(), tag          # the activation did cut


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("rows_switch", ["64", "128"])
def test_both_panel_heights(ops, monkeypatch, prec, rows_switch):
    from helpers import set_switch
    set_switch(monkeypatch, "MDG_CHAIN_ROWS", rows_switch)
    for M in (129, 333):
        c = _case(M, 68, 3, True, True, None, 77)
        assert torch.equal(_fused(ops, c, "relu", prec), _unfused(ops, c, "relu", prec))


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_repeatable_and_strided(ops, prec):
    M, K = 333, 68
    c = _case(M, K, 3, True, True, None, 5)
    want = _unfused(ops, c, "relu", prec)
    first = _fused(ops, c, "relu", prec)
    for _ in range(3):
        assert torch.equal(_fused(ops, c, "relu", prec), first)
    # y with ldy > 128: the columns beside it stay untouched
    wide = torch.full((M, 160), -7.0, device="cuda")
    _fused(ops, c, "relu", prec, out=wide[:, :128])
    assert torch.equal(wide[:, :128], want) and bool((wide[:, 128:] == -7.0).all())
    # the first operand and the edge operand as column slices of wider buffers (ld > K)
    xw = torch.randn(M, K + 12, device="cuda")
    xw[:, :K] = c["x"]
    ew = torch.randn(M, 32, device="cuda")
    ew[:, :20] = c["e"]
    c2 = dict(c, x=xw[:, :K], e=ew[:, :20])
    assert torch.equal(_fused(ops, c2, "relu", prec), want)


def test_bad_arguments_are_refused(ops):
    M = 16
    x = torch.randn(M, 128, device="cuda")
    b = torch.zeros(128, device="cuda")
    for width in (64, 256):                                      # stage width must be 128
        w = torch.randn(width, 128, device="cuda")
        with pytest.raises(ValueError, match="128 wide"):
            ops.linear_chain(x, [w], [None], out=torch.empty(M, width, device="cuda"))
    w = torch.randn(128, 128, device="cuda")
    with pytest.raises(ValueError, match="first-stage K"):       # K = 132
        ops.linear_chain(torch.randn(M, 132, device="cuda"), [torch.randn(128, 132, device="cuda")], [b])
    with pytest.raises(ValueError, match="16-bit"):              # the fp32 mode keeps the unfused path
        ops.linear_chain(x, [w], [b], precision="f32")
    with pytest.raises(ValueError, match="aligned"):             # misaligned first operand / result
        ops.linear_chain(torch.randn(M * 128 + 4, device="cuda")[1:M * 128 + 1].view(M, 128), [w], [b])
    with pytest.raises(ValueError, match="aligned"):
        ops.linear_chain(x, [w], [b], out=torch.empty(M * 128 + 4, device="cuda")[1:M * 128 + 1].view(M, 128))
    with pytest.raises(ValueError, match="1 to 3 stages"):
        ops.linear_chain(x, [w] * 4, [b] * 4)
