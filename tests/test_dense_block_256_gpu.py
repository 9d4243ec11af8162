"""The 256 x 256 ping-pong dense block (linear.hip: linear_pp_kernel) against float64, at its tile and k edges.

Every case first asks the library which kernel its call runs on (ops.linear_tile: the launch path's own decision) and only then
looks at numbers.  The reference is independent of the library:

  bf16     the float64 product of the bf16-ROUNDED operands (any epilogue in float64), bound 2e-6 of max|ref|: what is left is fp32
           accumulation (scripts/dense_block_emulation.py: at most 3.1e-7 for K = 4 ... 2048) and the fp32 epilogue.
  bf16x3   the float64 product of the fp32 operands, bound 2e-5 of max(max|ref|, 1): the three-product split measured at most
           1.0e-5 in the same emulation, and 1.4e-3 or more with one of the three products left out.

The forced-tile cases (MDG_LINEAR_TILE=256 at shapes the dispatcher would give to the 128-tile kernel) also require the bits of
the 128-tile kernel: both read the same operand images and add the same products in the same order per element.

Not covered: the stream-K instantiation linear_pp_kernel<*, true>.  It cannot be dispatched (launch_linear_core's sk_sw is a
constant 0), so nothing here tries to reach it.  The 16-bit images pad K to a multiple of 64, so the bf16x3 k loop (32 k per
tile) always runs an even number of tiles; an odd count exists in bf16 only (K = 4, 36, 192, 559 below).
"""
import math

import pytest
import torch

from helpers import set_switch

pytestmark = pytest.mark.gpu
BOUND = {"bf16": 2e-6, "bf16x3": 2e-5}
PRECS = ["bf16", "bf16x3"]
ACTS = ["relu", "gelu", "tanh", "sigmoid", "leakyrelu", "softplus", "selu", None]


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _f64(t, prec):
    """An operand as the mode multiplies it, in float64 (host): rounded to bf16 once in "bf16", the fp32 value itself in "bf16x3"."""
    t = t.detach().cpu()
    return (t.bfloat16() if prec == "bf16" else t).double()


def _act64(act, v):
    from oracle import madrigal_oracle as O
    return O._act(act, v)


def _err(got, ref, prec):
    scale = float(ref.abs().max())
    if prec == "bf16x3":
        scale = max(scale, 1.0)
    return float((got.detach().cpu().double() - ref).abs().max()) / scale          # NaN (an element never written) fails every bound


def _within(got, ref, prec, what):
    e = _err(got, ref, prec)
    print(f"{what} [{prec}]: {e:.3e} of the scale (bound {BOUND[prec]:.0e})")
    assert got.shape == ref.shape and e < BOUND[prec], (what, prec, e)
    return e


def _both_tiles(ops, monkeypatch, M, N, prec, fn):
    """fn() on the 256-tile kernel, then on the 128-tile kernel, the query asserted for each before anything is looked at."""
    set_switch(monkeypatch, "MDG_LINEAR_TILE", "256")
    assert ops.linear_tile(M, N, prec) == 256
    big = fn()
    set_switch(monkeypatch, "MDG_LINEAR_TILE", "128")
    assert ops.linear_tile(M, N, prec) == 128
    small = fn()
    return big, small


def _judge(big, small, ref, prec, what):
    """The 256-tile result against float64, then against the 128-tile kernel's bits (whose own distance from float64 is in the
    message if the bits differ: it says which side is off)."""
    _within(big, ref, prec, what + " (256-tile)")
    assert torch.equal(big, small), (what, prec, "256- and 128-tile results differ", _err(big, ref, prec), _err(small, ref, prec))


def _nan(M, N):
    return torch.full((M, N), float("nan"), device="cuda")


# ------------------------------------------------------------------------------------------- (a) forced 256-tile kernel, small shapes

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K", [4, 36, 68, 96, 192, 559, 2048])
@pytest.mark.parametrize("M,N", [(1, 1), (63, 65), (129, 257), (257, 129), (300, 130), (511, 513), (64, 1000)])
def test_forced_tile_plain(ops, monkeypatch, prec, M, N, K):
    """x W^T + b.  (M, N): one tile with almost every row and column clamped, raggedness on either side of the 64 / 128 / 256
    boundaries, N % 4 != 0, grids of several tiles.  K (images pad it to 64): one k tile in both modes (4), one in bf16 against two
    in bf16x3 (36), odd counts in bf16 (192 -> 3, 559 -> 9), the cv width 559 and the fusion width 2048."""
    x, w, b = _rand((M, K), 1).cuda(), _rand((N, K), 2, 1 / math.sqrt(K)).cuda(), _rand((N,), 3).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear(x, w, b, precision=prec, out=_nan(M, N), cache_weight=False))
    ref = _f64(x, prec) @ _f64(w, prec).T + b.cpu().double()
    _judge(big, small, ref, prec, f"plain {M}x{N}x{K}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", [(300, 130, 128), (513, 260, 96)])
def test_forced_tile_epilogue(ops, monkeypatch, prec, act, M, N, K):
    """alpha * act((x W^T + b) * scale + shift) + beta * residual with every activation, an [M, N] residual, alpha = 0.7, beta = 0.3."""
    x, w, b = _rand((M, K), 4).cuda(), _rand((N, K), 5, 1 / math.sqrt(K)).cuda(), _rand((N,), 6).cuda()
    scale, shift, res = (_rand((N,), 7).abs() + 0.5).cuda(), _rand((N,), 8).cuda(), _rand((M, N), 9).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear(
        x, w, b, scale=scale, shift=shift, act=act, residual=res, alpha=0.7, beta=0.3, precision=prec, out=_nan(M, N), cache_weight=False))
    pre = (_f64(x, prec) @ _f64(w, prec).T + b.cpu().double()) * scale.cpu().double() + shift.cpu().double()
    _judge(big, small, 0.7 * _act64(act, pre) + 0.3 * res.cpu().double(), prec, f"epilogue {act} {M}x{N}x{K}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(300, 130, 128), (513, 260, 96)])
def test_forced_tile_destinations_and_residual_views(ops, monkeypatch, prec, M, N, K):
    """The row-major epilogue of the 256-tile kernel where 16-byte accesses are not allowed: a [N] broadcast residual, a destination
    view starting at an odd column (the columns in front stay zero), a residual view with an odd row stride, and y aliasing the
    residual."""
    x, w, b = _rand((M, K), 31).cuda(), _rand((N, K), 32, 1 / math.sqrt(K)).cuda(), _rand((N,), 33).cuda()
    want = _f64(x, prec) @ _f64(w, prec).T + b.cpu().double()
    r_row = _rand((N,), 34).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear(x, w, b, residual=r_row, precision=prec, out=_nan(M, N), cache_weight=False))
    _judge(big, small, want + r_row.cpu().double(), prec, "broadcast residual")

    def into_view():
        wide = torch.zeros(M, N + 3, device="cuda")
        ops.linear(x, w, b, precision=prec, out=wide[:, 3:], cache_weight=False)
        return wide
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, into_view)
    assert float(big[:, :3].abs().max()) == 0.0
    _judge(big[:, 3:], small[:, 3:], want, prec, "destination at an odd column")
    assert torch.equal(big, small)
    res_wide = _rand((M, N + 1), 35).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear(x, w, b, residual=res_wide[:, 1:], precision=prec, out=_nan(M, N), cache_weight=False))
    _judge(big, small, want + res_wide[:, 1:].cpu().double(), prec, "residual with an odd row stride")
    y0 = _rand((M, N), 36)

    def in_place():
        y = y0.cuda()
        assert ops.linear(x, w, b, residual=y, precision=prec, out=y, cache_weight=False) is y
        return y
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, in_place)
    _judge(big, small, want + y0.double(), prec, "y aliasing the residual")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(300, 130, 64), (513, 1024, 192)])
def test_forced_tile_dropout_epilogue(ops, monkeypatch, prec, M, N, K):
    """dropout(x W^T + b, p, seed) + residual inside the epilogue == the three separate steps bit for bit (N % 4 != 0: the mask is hashed per
    element; N % 4 == 0: per group of four); the plain product under it is the one checked against float64."""
    p, seed = 0.3, 20240607
    x, w, b = _rand((M, K), 11).cuda(), _rand((N, K), 12, 1 / math.sqrt(K)).cuda(), _rand((N,), 13).cuda()
    r = _rand((M, N), 14).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: (
        ops.linear(x, w, b, residual=r, precision=prec, cache_weight=False, dropout_p=p, dropout_seed=seed),
        ops.linear(x, w, b, precision=prec, out=_nan(M, N), cache_weight=False)))
    ref = _f64(x, prec) @ _f64(w, prec).T + b.cpu().double()
    _judge(big[1], small[1], ref, prec, f"the product under the dropout {M}x{N}x{K}")
    assert torch.equal(big[0], ops.dropout(big[1], p, seed) + r)
    assert torch.equal(big[0], small[0])
    zero_share = float((big[0] - r == 0).float().mean())
    assert 0.2 < zero_share < 0.4, zero_share
    kept = (big[0] - r) != 0                                     # the kept entries against float64: scaled by 1 / (1 - p), residual added
    full = ref / (1.0 - p) + r.cpu().double()
    e = float((big[0].cpu().double() - full)[kept.cpu()].abs().max()) / float(full.abs().max())
    assert e < BOUND[prec], e


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(300, 130, 36), (1000, 512, 128)])
def test_forced_tile_rowscaled(ops, monkeypatch, prec, M, N, K):
    """linear_rowscaled prefers the 128-tile kernel at any size; MDG_LINEAR_TILE=256 still selects the 256-tile kernel for it
    (x then goes through the operand pre-pass): row_scale[m] * (x W^T + bias_pre) + bias on both."""
    x, w = _rand((M, K), 21).cuda(), _rand((N, K), 22, 1 / math.sqrt(K)).cuda()
    rs, bpre, b = (_rand((M,), 23).abs() + 0.25).cuda(), _rand((N,), 24).cuda(), _rand((N,), 25).cuda()
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear_rowscaled(x, w, rs, bpre, b, precision=prec, out=_nan(M, N)))
    ref = rs.cpu().double()[:, None] * (_f64(x, prec) @ _f64(w, prec).T + bpre.cpu().double()) + b.cpu().double()
    _judge(big, small, ref, prec, f"row-scaled {M}x{N}x{K}")
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: ops.linear_rowscaled(x, w, rs, precision=prec, out=_nan(M, N)))
    _judge(big, small, rs.cpu().double()[:, None] * (_f64(x, prec) @ _f64(w, prec).T), prec, f"row-scaled, no biases {M}x{N}x{K}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,K,N", [(333, 256, 192), (700, 2048, 512)])
def test_forced_tile_reads_the_image_layernorm_wrote(ops, monkeypatch, prec, M, K, N):
    """layernorm_packed -> linear_packed == layernorm -> linear bit for bit on the 256-tile kernel too, and the block is within the
    bound of float64 on the normalised rows (the rows themselves: within fp32 of a float64 LayerNorm)."""
    x = _rand((M, K), 80).cuda()
    g, beta = _rand((K,), 81).cuda(), _rand((K,), 82).cuda()
    w, bias = _rand((N, K), 83, 1 / math.sqrt(K)).cuda(), _rand((N,), 84).cuda()
    y = ops.layernorm(x, g, beta, 1e-5)
    y64 = torch.nn.functional.layer_norm(x.cpu().double(), (K,), g.cpu().double(), beta.cpu().double(), 1e-5)
    assert float((y.cpu().double() - y64).abs().max()) < 1e-5 * float(y64.abs().max())
    y_again, img = ops.layernorm_packed(x, g, beta, 1e-5, prec)
    assert torch.equal(y_again, y) and img is not None
    big, small = _both_tiles(ops, monkeypatch, M, N, prec, lambda: (
        ops.linear_packed(img, M, w, bias, act="gelu", precision=prec, out=_nan(M, N), cache_weight=False),
        ops.linear(y, w, bias, act="gelu", precision=prec, out=_nan(M, N), cache_weight=False)))
    ref = _act64("gelu", _f64(y, prec) @ _f64(w, prec).T + bias.cpu().double())
    _judge(big[0], small[0], ref, prec, f"LayerNorm's image {M}x{N}x{K}")
    assert torch.equal(big[0], big[1]) and torch.equal(small[0], small[1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,K,N", [(333, 256, 192), (700, 2048, 512)])
def test_forced_tile_reads_the_backward_images(ops, monkeypatch, prec, M, K, N):
    """dx = g W of a K -> N layer on the 256-tile kernel: from the row image linear_backward_pack wrote, against linear(g, W^T) bit
    for bit and g W in float64; the same through the PackedWeight transposed_weight_image makes of W (no fp32 W^T at all)."""
    g, w = _rand((M, N), 5).cuda(), _rand((N, K), 7, 1 / math.sqrt(N)).cuda()
    row_img, _, _ = ops.linear_backward_pack(g, prec)
    wt = ops.transpose(w)
    wt_packed, wt_img = ops.transposed_weight_image(w, prec)
    assert isinstance(wt_packed, ops.PackedWeight) and wt_packed.shape == (K, N) and wt_img is wt_packed.image
    big, small = _both_tiles(ops, monkeypatch, M, K, prec, lambda: (
        ops.linear_packed(row_img, M, wt, precision=prec, out=_nan(M, K), cache_weight=False),
        ops.linear(g, wt, precision=prec, out=_nan(M, K), cache_weight=False),
        ops.linear_packed(row_img, M, wt_packed, precision=prec, out=_nan(M, K)),
        ops.linear(g, wt_packed, precision=prec, out=_nan(M, K))))
    ref = _f64(g, prec) @ _f64(w, prec)
    _judge(big[0], small[0], ref, prec, f"dx from the packed gradient {M}x{K}<-{N}")
    for i in (1, 2, 3):
        assert torch.equal(big[i], big[0]) and torch.equal(small[i], small[0]), i


# ------------------------------------------------------------------------------------------- (b) natural dispatch

def _resident_workgroups():
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256)       # linear.hip: resident_workgroups()


def _row_split(M, N):
    """launch_linear_core's own arithmetic: (tile rows of the 256-tile head launch, tile rows left to the 128-tile kernel) when a
    product is split, else None."""
    tx, ty, P = -(-N // 256), -(-M // 256), _resident_workgroups()
    total = tx * ty
    rem = total % P
    if total > P and rem != 0:
        full_rows = (total - rem) // tx
        tail_rows = ty - full_rows
        if full_rows > 0 and tail_rows > 0 and tail_rows * tx * 2 <= P:
            return full_rows, tail_rows
    return None


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(3100, 3800, 96), (12400, 1024, 64), (4800, 6100, 160), (2700, 6144, 256)])
def test_natural_dispatch_whole_output_against_float64(ops, monkeypatch, prec, M, N, K):
    """The smallest shapes the dispatcher gives to the 256-tile kernel by itself, gelu(x W^T + b) + residual, EVERY element against
    float64.  (3100, 3800): 13 x 15 = 195 tiles, not a multiple of 8, the swizzled walk's last group has 5 tile rows, M and N ragged.
    (12400, 1024): 49 x 4 tiles, one k tile in bf16.  (4800, 6100): 456 tiles, more than one round of a 256-CU card with a remainder
    too large for the row split.  (2700, 6144): 264 tiles, the row split: 10 tile rows on the 256-tile kernel (its ty_base / tiles_y
    cut), the last on the 128-tile kernel."""
    monkeypatch.delenv("MDG_LINEAR_TILE", raising=False)
    monkeypatch.delenv("MDG_LINEAR_TAIL128", raising=False)
    from madrigal_amd._lib import lib
    lib().mdg_tuning_reload()
    tx, ty, P = -(-N // 256), -(-M // 256), _resident_workgroups()
    assert M >= 1024 and N >= 256 and tx * ty >= 192 and ops.linear_tile(M, N, prec) == 256
    split = _row_split(M, N)
    if (M, N) == (3100, 3800):
        assert (ty, tx) == (13, 15) and (tx * ty) % 8 != 0 and ty % 8 == 5 and M % 256 and N % 256 and split is None
    elif (M, N) == (12400, 1024):
        assert (ty, tx) == (49, 4) and K == 64 and split is None
    elif (M, N) == (4800, 6100):
        assert (ty, tx) == (19, 24) and (P != 256 or (tx * ty > P and (tx * ty) % P == 200 and split is None))
    else:
        assert (ty, tx) == (11, 24) and (P != 256 or split == (10, 1))
    x, w, b = _rand((M, K), 1).cuda(), _rand((N, K), 2, 1 / math.sqrt(K)).cuda(), _rand((N,), 3).cuda()
    res = _rand((M, N), 4).cuda()
    got = ops.linear(x, w, b, act="gelu", residual=res, precision=prec, out=_nan(M, N), cache_weight=False)
    ref = _act64("gelu", (_f64(x, prec) @ _f64(w, prec).T).add_(b.cpu().double())).add_(res.cpu().double())
    _within(got, ref, prec, f"natural dispatch {M}x{N}x{K}")
    del ref
    set_switch(monkeypatch, "MDG_LINEAR_TAIL128", "0")
    assert ops.linear_tile(M, N, prec) == 256
    one = ops.linear(x, w, b, act="gelu", residual=res, precision=prec, out=_nan(M, N), cache_weight=False)
    assert torch.equal(one, got)                                 # the single launch (the same launch where no split is taken)
    set_switch(monkeypatch, "MDG_LINEAR_TILE", "128")
    assert ops.linear_tile(M, N, prec) == 128
    small = ops.linear(x, w, b, act="gelu", residual=res, precision=prec, out=_nan(M, N), cache_weight=False)
    assert torch.equal(small, got)
