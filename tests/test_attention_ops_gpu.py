"""The two attention kernels of csrc/fusion.hip at op level, against float64 autograd of the plain formula (attention_ref.py):
A dense self-attention backward, B the compact ("live token") path in both directions, C dropout (mask recovered from the forward
kernel, replayed by the backward kernel, its statistics), D the one-query pooling backward, E fully masked rows in backward.
Every comparison: max|got - ref| <= 2e-5 * max(max|ref|, 1).  Each check prints its figure before it asserts."""
import functools
import math

import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _make_masks():
    from madrigal_amd import data
    return data.make_masks


def _check(group, what, got, ref):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (group, what, tuple(got.shape), tuple(ref.shape))
    err, b = float((got - ref).abs().max()), R.bound(ref)
    print(f"[attention-ops] {group} {what}: max err {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
    assert err <= b, (group, what, err, b)                   # a NaN in `got` fails here too


def _check_qkv_grads(group, what, got, ref, d):
    for i, nm in enumerate(("dq", "dk", "dv")):
        _check(group, f"{what} {nm}", got[:, i * d:(i + 1) * d], ref[:, i * d:(i + 1) * d])


def _recover(group, what, got, p_ref, allowed, p):
    """The kept / dropped mask out of dropped-out weights the forward kernel returned (``got``, any shape; ``p_ref`` the float64
    weights before dropout, ``allowed`` which entries may be non-zero at all)."""
    got = got.detach().cpu().double()
    want = p_ref / (1.0 - p)
    assert bool((got[~allowed] == 0).all()), (group, what, "a blocked weight is not an exact zero")
    g, w = got[allowed], want[allowed]
    tol = R.bound(w)
    dropped, kept = g == 0, (g - w).abs() <= tol
    worst = float((g - w).abs()[kept].max()) if bool(kept.any()) else 0.0
    print(f"[attention-ops] {group} {what} kept weights: max err {worst:.3e}, bound {tol:.3e}, ratio {worst / tol:.3f}; "
          f"{int(kept.sum())} kept, {int(dropped.sum())} dropped of {g.numel()}")
    assert bool((dropped ^ kept).all()), (group, what, "an entry is neither an exact 0 nor P / (1 - p)",
                                          float((g - w).abs()[~dropped].max()), tol)
    keep = torch.zeros_like(got)
    keep[allowed] = kept.double()
    return keep, int(kept.sum()), g.numel()


def _check_rate(group, what, kept, N, p):
    pe = R.drop_rate(p)
    dev, lim = abs(kept / N - (1.0 - pe)), 5.0 * math.sqrt(pe * (1.0 - pe) / N)
    print(f"[attention-ops] {group} {what} keep rate: {kept}/{N}, |dev| {dev:.4f}, limit {lim:.4f}")
    assert dev <= lim, (group, what, kept, N, pe)


# ------------------------------------------------------------------------------------------------ A. dense backward
@functools.lru_cache(maxsize=None)
def _dense_case(S, H, dh, masked, n=R.DENSE_N, scale=1.0):
    qkv, dout = R.dense_inputs(S, H, dh, n, scale)
    kpm, src = R.dense_masks(n, S) if masked else (None, None)
    allowed = R.dense_allowed(n, S, kpm, src)
    return (qkv, dout, kpm, src, allowed) + R.attention_rows_ref(qkv, dout, n, S, H, dh, allowed)


def _bits(ops, kpm, src):
    return (None if kpm is None else ops.mask_bits(kpm.cuda())), (None if src is None else ops.mask_bits(src.cuda()))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("S,H,dh", R.DENSE_SHAPES)
def test_dense_backward_matches_float64_autograd(ops, S, H, dh, masked):
    # (a q|k|v slice of a wider buffer, ld > 3*H*dh, is not reachable here: the wrappers make their operands contiguous first)
    n, d = R.DENSE_N, H * dh
    qkv, dout, kpm, src, _, ref_out, ref_dqkv, _ = _dense_case(S, H, dh, masked)
    kb, sb = _bits(ops, kpm, src)
    out, _ = ops.fusion_attention(qkv.cuda(), n, S, H, dh, kb, sb)
    dqkv = ops.fusion_attention_bwd(qkv.cuda(), dout.cuda(), n, S, H, dh, kb, sb)
    again = ops.fusion_attention_bwd(qkv.cuda(), dout.cuda(), n, S, H, dh, kb, sb)
    assert torch.equal(dqkv, again)
    what = f"S={S} H={H} dh={dh} {'masked' if masked else 'open'}"
    _check("A", what + " out", out, ref_out)
    _check_qkv_grads("A", what, dqkv, ref_dqkv, d)


# ------------------------------------------------------------------------------------------------ B. compact path
def _run_compact(ops, plan, qkv, dout, H, dh, p=0.0, seed=0):
    ts, rb = plan["tile_start"].cuda(), plan["row_bits"].cuda()
    out, _ = ops.fusion_attention(qkv, plan["n_tiles"], plan["S"], H, dh, row_start=ts, row_bits=rb, p_drop=p, seed=seed)
    dqkv = ops.fusion_attention_bwd(qkv, dout, plan["n_tiles"], plan["S"], H, dh, row_start=ts, row_bits=rb, p_drop=p, seed=seed)
    return out, dqkv


@pytest.mark.parametrize("H,dh", R.COMPACT_HEADS)
@pytest.mark.parametrize("name", R.MASK_CASES)
def test_compact_forward_and_backward_match_float64_autograd(ops, name, H, dh):
    plan, qkv, dout, _, ref_out, ref_dqkv, _ = R.compact_reference(name, H, dh, _make_masks())
    out, dqkv = _run_compact(ops, plan, qkv.cuda(), dout.cuda(), H, dh)
    what = f"{name} H={H} dh={dh}"
    _check("B", what + " out", out, ref_out)
    _check_qkv_grads("B", what, dqkv, ref_dqkv, H * dh)


@pytest.mark.parametrize("H,dh", R.COMPACT_HEADS)
@pytest.mark.parametrize("drug", [11, 4])                     # the 13-token drug of the 32-row tile; one of the ten that share a tile
def test_compact_drugs_sharing_a_tile_do_not_leak(ops, drug, H, dh):
    plan, qkv, dout, _, _, _, _ = R.compact_reference("mixed_tiles", H, dh, _make_masks())
    rows = plan["row_drug"] == drug
    tiles = plan["row_tile"][rows].unique()
    shared = (plan["row_tile"] == tiles[0]) & ~rows
    assert tiles.numel() == 1 and int(rows.sum()) >= 1 and int(shared.sum()) >= 1
    out0, dqkv0 = _run_compact(ops, plan, qkv.cuda(), dout.cuda(), H, dh)
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[rows] = R.rand((int(rows.sum()), qkv.shape[1]), 900 + drug, 3.0) + 1.0
    dout2[rows] = R.rand((int(rows.sum()), dout.shape[1]), 950 + drug, 3.0) - 1.0
    out1, dqkv1 = _run_compact(ops, plan, qkv2.cuda(), dout2.cuda(), H, dh)
    others = (~rows).cuda()
    assert bool(torch.isfinite(out1).all()) and bool(torch.isfinite(dqkv1).all())
    assert torch.equal(out1[others], out0[others]), "another drug's output rows moved"
    assert torch.equal(dqkv1[others], dqkv0[others]), "another drug's gradient rows moved"
    assert not torch.equal(out1[~others], out0[~others]) and not torch.equal(dqkv1[~others], dqkv0[~others])


@pytest.mark.parametrize("name", ["mixed_tiles", "full_drugs"])
def test_compact_reads_only_the_rows_handed_in(ops, name):
    H, dh, pad = 2, 64, 40
    plan, qkv, dout, _, _, _, _ = R.compact_reference(name, H, dh, _make_masks())
    Rr = plan["R"]
    out0, dqkv0 = _run_compact(ops, plan, qkv.cuda(), dout.cuda(), H, dh)
    big_qkv = torch.full((Rr + 2 * pad, qkv.shape[1]), float("nan"), device="cuda")
    big_dout = torch.full((Rr + 2 * pad, dout.shape[1]), float("nan"), device="cuda")
    big_qkv[pad:pad + Rr] = qkv.cuda()
    big_dout[pad:pad + Rr] = dout.cuda()
    out1, dqkv1 = _run_compact(ops, plan, big_qkv[pad:pad + Rr], big_dout[pad:pad + Rr], H, dh)
    assert bool(torch.isfinite(out1).all()) and bool(torch.isfinite(dqkv1).all())
    assert torch.equal(out1, out0) and torch.equal(dqkv1, dqkv0)


# ------------------------------------------------------------------------------------------------ C. dropout
@pytest.mark.parametrize("p", R.DROPOUT_P)
@pytest.mark.parametrize("S,H,dh", R.DROPOUT_DENSE_SHAPES)
def test_dense_dropout_mask_recovery_replay_and_rate(ops, S, H, dh, p):
    n, d = R.DENSE_N, H * dh
    qkv, dout, kpm, src, allowed, _, _, p_ref = _dense_case(S, H, dh, True, scale=R.DROPOUT_QK_SCALE)
    kb, sb = _bits(ops, kpm, src)
    ok = allowed.unsqueeze(1).expand(n, H, S, S)
    qkv_u = qkv.clone()
    qkv_u[:, 2 * d:] = R.unit_values([r % S for r in range(n * S)], H, dh)
    keeps = []
    for seed in R.DROPOUT_SEEDS:
        what = f"dense S={S} H={H} dh={dh} p={p} seed={seed:#x}"
        out_u, probs = ops.fusion_attention(qkv_u.cuda(), n, S, H, dh, kb, sb, want_probs=True, p_drop=p, seed=seed)
        again, _ = ops.fusion_attention(qkv_u.cuda(), n, S, H, dh, kb, sb, p_drop=p, seed=seed)
        assert torch.equal(out_u, again)                                               # the same seed: the same mask
        _check("C", what + " weights before dropout", probs, p_ref)
        pd = out_u.cpu().view(n, S, H, dh).permute(0, 2, 1, 3)                          # [n, H, query, column]: Pd, then zeros
        assert bool((pd[..., S:] == 0).all())
        keep, kept, N = _recover("C", what, pd[..., :S], p_ref, ok, p)
        _check_rate("C", what, kept, N, p)
        keeps.append(keep)
        # the backward pass replays this very mask
        ref_out, ref_dqkv, _ = R.attention_rows_ref(qkv, dout, n, S, H, dh, allowed, keep, p)
        out, _ = ops.fusion_attention(qkv.cuda(), n, S, H, dh, kb, sb, p_drop=p, seed=seed)
        dqkv = ops.fusion_attention_bwd(qkv.cuda(), dout.cuda(), n, S, H, dh, kb, sb, p_drop=p, seed=seed)
        _check("C", what + " out", out, ref_out)
        _check_qkv_grads("C", what, dqkv, ref_dqkv, d)
    differ = int((keeps[0] != keeps[1])[ok].sum())
    assert differ > N / 10, (differ, N)


@pytest.mark.parametrize("p", R.DROPOUT_P)
def test_compact_dropout_mask_recovery_replay_and_rate(ops, p):
    H, dh = 4, 32
    d = H * dh
    plan, qkv, dout, allowed, _, _, p_ref = R.compact_reference("mixed_tiles", H, dh, _make_masks(), R.DROPOUT_QK_SCALE)
    n, S, ti = plan["n"], plan["S"], plan["token_index"]
    p_loc, own = R.tile_local(plan, p_ref)
    ok = own.unsqueeze(1).expand_as(p_loc)
    qkv_u = qkv.clone()
    qkv_u[:, 2 * d:] = R.unit_values((torch.arange(plan["R"]) - plan["tile_start"][plan["row_tile"]]).tolist(), H, dh)
    ts, rb = plan["tile_start"].cuda(), plan["row_bits"].cuda()
    keeps = []
    for seed in R.DROPOUT_SEEDS:
        what = f"compact mixed_tiles H={H} dh={dh} p={p} seed={seed:#x}"
        out_u, _ = ops.fusion_attention(qkv_u.cuda(), plan["n_tiles"], S, H, dh, row_start=ts, row_bits=rb, p_drop=p, seed=seed)
        again, _ = ops.fusion_attention(qkv_u.cuda(), plan["n_tiles"], S, H, dh, row_start=ts, row_bits=rb, p_drop=p, seed=seed)
        assert torch.equal(out_u, again)
        keep_loc, kept, N = _recover("C", what, out_u.cpu().view(plan["R"], H, dh), p_loc, ok, p)    # dh = 32: the row IS Pd[x, :]
        _check_rate("C", what, kept, N, p)
        keeps.append(keep_loc)
        keep = R.tile_to_dense(plan, keep_loc, fill=1.0)
        ref_out, ref_dqkv, _ = R.attention_rows_ref(R.scatter_compact(qkv, ti, n, S), R.scatter_compact(dout, ti, n, S), n, S, H, dh,
                                                    allowed, keep, p)
        out, dqkv = _run_compact(ops, plan, qkv.cuda(), dout.cuda(), H, dh, p, seed)
        _check("C", what + " out", out, ref_out[ti])
        _check_qkv_grads("C", what, dqkv, ref_dqkv[ti], d)
    differ = int((keeps[0] != keeps[1])[ok].sum())
    assert differ > N / 10, (differ, N)


@pytest.mark.parametrize("p", R.DROPOUT_P)
@pytest.mark.parametrize("Tk,H,dh", R.POOL_SHAPES)
def test_pool_dropout_mask_recovery_replay_and_rate(ops, Tk, H, dh, p):
    n, d = R.DROPOUT_POOL_N, H * dh
    q, kv, dout = R.pool_inputs(n, Tk, H, dh, scale=R.DROPOUT_QK_SCALE)
    p_ref = R.pool_rows_ref(q, kv, dout, n, Tk, H, dh)[3]
    ok = torch.ones_like(p_ref, dtype=torch.bool)
    kv_u = kv.clone()
    kv_u[:, d:] = R.unit_values([r % Tk for r in range(n * Tk)], H, dh)
    keeps = []
    for seed in R.DROPOUT_SEEDS:
        what = f"pool Tk={Tk} H={H} dh={dh} p={p} seed={seed:#x}"
        out_u = ops.xattn_pool(q.cuda(), kv_u.cuda(), n, Tk, H, dh, p_drop=p, seed=seed)
        assert torch.equal(out_u, ops.xattn_pool(q.cuda(), kv_u.cuda(), n, Tk, H, dh, p_drop=p, seed=seed))
        pd = out_u.cpu().view(n, H, dh)
        assert bool((pd[..., Tk:] == 0).all())
        keep, kept, N = _recover("C", what, pd[..., :Tk], p_ref, ok, p)
        _check_rate("C", what, kept, N, p)
        keeps.append(keep)
        ref_out, ref_dq, ref_dkv, _ = R.pool_rows_ref(q, kv, dout, n, Tk, H, dh, keep, p)
        _check("C", what + " out", ops.xattn_pool(q.cuda(), kv.cuda(), n, Tk, H, dh, p_drop=p, seed=seed), ref_out)
        dq, dkv = ops.xattn_pool_bwd(q.cuda(), kv.cuda(), dout.cuda(), n, Tk, H, dh, p_drop=p, seed=seed)
        _check("C", what + " dq", dq, ref_dq)
        _check("C", what + " dk", dkv[:, :d], ref_dkv[:, :d])
        _check("C", what + " dv", dkv[:, d:], ref_dkv[:, d:])
    differ = int((keeps[0] != keeps[1]).sum())
    assert differ > N / 10, (differ, N)


# ------------------------------------------------------------------------------------------------ D. pooling backward
@pytest.mark.parametrize("n", R.POOL_N)
@pytest.mark.parametrize("Tk,H,dh", R.POOL_SHAPES)
def test_pool_backward_matches_float64_autograd(ops, Tk, H, dh, n):
    d = H * dh
    q, kv, dout = R.pool_inputs(n, Tk, H, dh)
    ref_out, ref_dq, ref_dkv, _ = R.pool_rows_ref(q, kv, dout, n, Tk, H, dh)
    what = f"Tk={Tk} H={H} dh={dh} n={n}"
    _check("D", what + " out", ops.xattn_pool(q.cuda(), kv.cuda(), n, Tk, H, dh), ref_out)
    dq, dkv = ops.xattn_pool_bwd(q.cuda(), kv.cuda(), dout.cuda(), n, Tk, H, dh)
    dq2, dkv2 = ops.xattn_pool_bwd(q.cuda(), kv.cuda(), dout.cuda(), n, Tk, H, dh)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    _check("D", what + " dq", dq, ref_dq)
    _check("D", what + " dk", dkv[:, :d], ref_dkv[:, :d])
    _check("D", what + " dv", dkv[:, d:], ref_dkv[:, d:])


# ------------------------------------------------------------------------------------------------ E. fully masked rows
def test_fully_masked_drug_poisons_only_its_own_gradient_rows(ops):
    n, S, H, dh = 3, 19, 2, 32
    d = H * dh
    kpm, src = R.dense_masks(n, S)
    kpm[1, :] = True
    qkv, dout = R.dense_inputs(S, H, dh, n=n)
    _, ref_dqkv, _ = R.attention_rows_ref(qkv, dout, n, S, H, dh, R.dense_allowed(n, S, kpm, src))
    kb, sb = _bits(ops, kpm, src)
    dqkv = ops.fusion_attention_bwd(qkv.cuda(), dout.cuda(), n, S, H, dh, kb, sb).cpu().view(n, S, 3 * d)
    ref_dqkv = ref_dqkv.view(n, S, 3 * d)
    # drug 1: every weight is NaN (as in the forward pass, as torch), so dv = Pd^T dO is NaN in every entry; dq and dk go through dS,
    # which the formula leaves NaN and autograd's masked_fill sets to 0: either, but no finite non-zero number
    assert bool(torch.isnan(dqkv[1, :, 2 * d:]).all())
    assert bool((torch.isnan(dqkv[1, :, :2 * d]) | (dqkv[1, :, :2 * d] == 0)).all())
    assert bool(torch.isnan(dqkv[1]).any(-1).all())
    assert bool(torch.isfinite(dqkv[[0, 2]]).all())
    _check_qkv_grads("E", "drugs 0 and 2", dqkv[[0, 2]].reshape(2 * S, 3 * d), ref_dqkv[[0, 2]].reshape(2 * S, 3 * d), d)
