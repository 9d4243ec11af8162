"""Float64 references for the two attention kernels of csrc/fusion.hip (the 32x32-tile self-attention and the one-query pooling), an
independent restatement of the compact ("live token") tile layout, and the cases that test_attention_ops_cpu.py and
test_attention_ops_gpu.py share.  Pure torch: nothing here imports the package under test (the one generator the random mask
cases need, ``data.make_masks``, is handed in by the caller)."""
import functools
import math

import torch

TOL = 2e-5                     # the suite's fp32-class bound for these kernels: max|got - ref| <= TOL * max(max|ref|, 1)
MIN_WEIGHT = 1e-3              # floor on every allowed reference weight of a dropout case (kept and dropped entries cannot be confused)

DENSE_SHAPES = [(32, 1, 32), (1, 2, 64), (19, 4, 128), (21, 2, 256), (23, 3, 96), (22, 8, 32)]          # (S, H, dh), group A
DENSE_N = 5
COMPACT_HEADS = [(4, 32), (2, 64), (1, 128)]                                                            # (H, dh), group B
MASK_CASES = ["mixed_tiles", "source_mask", "full_drugs", "random_masks"]                               # (a) .. (d)
POOL_SHAPES = [(1, 4, 32), (32, 1, 64), (4, 8, 64), (19, 4, 128), (2, 2, 256), (7, 2, 100)]             # (Tk, H, dh), group D
POOL_N = [11, 257]
DROPOUT_P = [0.3, 0.5]
DROPOUT_SEEDS = [7, 0x9E3779B97F4A7C15]
DROPOUT_DENSE_SHAPES = [(19, 4, 32), (32, 1, 64)]
DROPOUT_POOL_N = 11


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def bound(ref):
    return TOL * max(float(ref.abs().max()), 1.0)


def drop_rate(p):
    """The rate the kernels really drop at: a weight is dropped when a 16-bit field is below floor(p * 65536)."""
    return math.floor(p * 65536) / 65536


# ---------------------------------------------------------------------------------------------------- the plain formulas
def self_attention_ref(q, k, v, allowed, keep=None, p=0.0, want_probs=False):
    """q, k, v [n, S, H, dh]; allowed bool [n, S, S] (query, key); keep [n, H, S, S] (1 = kept) with dropout rate p.
    -> out [n, S, H, dh] (and the weights before dropout [n, H, S, S])."""
    dh = q.shape[-1]
    s = torch.einsum("nihd,njhd->nhij", q / math.sqrt(dh), k)
    s = s.masked_fill(~allowed.unsqueeze(1), float("-inf"))
    P = torch.softmax(s, dim=-1)
    Pd = P if keep is None else P * keep.to(P.dtype) / (1.0 - p)
    out = torch.einsum("nhij,njhd->nihd", Pd, v)
    return (out, P) if want_probs else out


def pool_ref(q, k, v, keep=None, p=0.0, want_probs=False):
    """One query shared by every drug: q [H, dh]; k, v [n, Tk, H, dh]; keep [n, H, Tk] -> out [n, H, dh] (and weights [n, H, Tk])."""
    dh = q.shape[-1]
    s = torch.einsum("hd,nthd->nht", q / math.sqrt(dh), k)
    P = torch.softmax(s, dim=-1)
    Pd = P if keep is None else P * keep.to(P.dtype) / (1.0 - p)
    out = torch.einsum("nht,nthd->nhd", Pd, v)
    return (out, P) if want_probs else out


def attention_rows_ref(qkv, dout, n, S, H, dh, allowed, keep=None, p=0.0):
    """The row layout of the ops: qkv [n*S, 3*H*dh] (q | k | v), dout [n*S, H*dh] -> float64 (out rows, dqkv rows, weights)."""
    d = H * dh
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (t.reshape(n, S, H, dh) for t in x.view(n, S, 3 * d).split(d, dim=2))
    out, P = self_attention_ref(q, k, v, allowed, keep, p, want_probs=True)
    out = out.reshape(n * S, d)
    (out * dout.double()).sum().backward()
    return out.detach(), x.grad, P.detach()


def pool_rows_ref(q, kv, dout, n, Tk, H, dh, keep=None, p=0.0):
    """q [d], kv [n*Tk, 2d] (k | v), dout [n, d] -> float64 (out [n, d], dq [d], dkv rows, weights [n, H, Tk])."""
    d = H * dh
    qq = q.double().clone().requires_grad_(True)
    x = kv.double().clone().requires_grad_(True)
    k, v = (t.reshape(n, Tk, H, dh) for t in x.split(d, dim=1))
    out, P = pool_ref(qq.view(H, dh), k, v, keep, p, want_probs=True)
    out = out.reshape(n, d)
    (out * dout.double()).sum().backward()
    return out.detach(), qq.grad, x.grad, P.detach()


# ---------------------------------------------------------------------------------------------------- compact layout
def pack_tiles(live, src_mask=None):
    """The compact layout, restated from ``TransformerFusion.live_token_plan``'s docstring with plain loops.  live bool [n, S]
    (True = the token exists), src_mask bool [S, S] (True = query position may not attend key position) or None."""
    n, S = live.shape
    lv = live.tolist()
    sm = None if src_mask is None else src_mask.tolist()
    row_drug, row_pos, row_start = [], [], [0]
    for i in range(n):                                         # live tokens are stored drug after drug
        for s in range(S):
            if lv[i][s]:
                row_drug.append(i)
                row_pos.append(s)
        row_start.append(len(row_drug))
    tile_start, fill = [0], 0                                  # consecutive whole drugs, greedily, at most 32 rows a tile
    for i in range(n):
        c = row_start[i + 1] - row_start[i]
        if fill + c > 32:
            tile_start.append(tile_start[-1] + fill)
            fill = 0
        fill += c
    tile_start.append(tile_start[-1] + fill)
    row_bits, row_tile = [], []
    for t in range(len(tile_start) - 1):
        lo, hi = tile_start[t], tile_start[t + 1]
        for r in range(lo, hi):
            bits = 0
            for j in range(32):                                # bit j set: row r may not attend row j of its tile
                rj = lo + j
                ok = rj < hi and row_drug[rj] == row_drug[r] and not (sm is not None and sm[row_pos[r]][row_pos[rj]])
                if not ok:
                    bits |= 1 << j
            row_bits.append(bits - (1 << 32) if bits >= (1 << 31) else bits)               # the same 32 bits as an int32
            row_tile.append(t)
    i64 = dict(dtype=torch.int64)
    drug, pos = torch.tensor(row_drug, **i64), torch.tensor(row_pos, **i64)
    return {"n": n, "S": S, "R": len(row_drug), "n_tiles": len(tile_start) - 1, "tile_start": torch.tensor(tile_start, **i64),
            "row_start": torch.tensor(row_start, **i64), "row_bits": torch.tensor(row_bits, dtype=torch.int32),
            "token_index": drug * S + pos, "row_drug": drug, "row_pos": pos, "row_tile": torch.tensor(row_tile, **i64)}


def scatter_compact(rows, token_index, n, S):
    """Compact rows [R, w] -> dense rows [n*S, w], zero where no token lives."""
    dense = torch.zeros((n * S, rows.shape[1]), dtype=rows.dtype)
    dense[token_index] = rows
    return dense


def gather_compact(dense, token_index):
    """Dense [n, S, ...] or [n*S, ...] -> the compact row list [R, ...]."""
    if dense.dim() >= 3:
        dense = dense.reshape((dense.shape[0] * dense.shape[1],) + tuple(dense.shape[2:]))
    return dense[token_index]


def compact_allowed(live, src_mask):
    """allowed[i, a, b]: key b of drug i is live and the source mask lets query position a see it."""
    ok = live.unsqueeze(1).expand(live.shape[0], live.shape[1], live.shape[1])
    return ok & ~src_mask.unsqueeze(0) if src_mask is not None else ok.clone()


def tile_local(plan, dense_w):
    """Per-drug weights / masks [n, H, S, S] -> the tile's own coordinates [R, H, 32]: entry (r, h, j) belongs to query row r and row
    j of r's tile; zero where that row is another drug's or past the tile.  Second result: which entries are of r's own drug."""
    H = dense_w.shape[1]
    out = torch.zeros((plan["R"], H, 32), dtype=dense_w.dtype)
    own = torch.zeros((plan["R"], 32), dtype=torch.bool)
    ts, drug, pos, tile = plan["tile_start"].tolist(), plan["row_drug"].tolist(), plan["row_pos"].tolist(), plan["row_tile"].tolist()
    for r in range(plan["R"]):
        lo, hi = ts[tile[r]], ts[tile[r] + 1]
        for rj in range(lo, hi):
            if drug[rj] == drug[r]:
                out[r, :, rj - lo] = dense_w[drug[r], :, pos[r], pos[rj]]
                own[r, rj - lo] = True
    return out, own


def tile_to_dense(plan, tile_w, fill=1.0):
    """The inverse of ``tile_local`` for a mask recovered in tile coordinates: [R, H, 32] -> [n, H, S, S], ``fill`` elsewhere."""
    H = tile_w.shape[1]
    dense = torch.full((plan["n"], H, plan["S"], plan["S"]), fill, dtype=tile_w.dtype)
    ts, drug, pos, tile = plan["tile_start"].tolist(), plan["row_drug"].tolist(), plan["row_pos"].tolist(), plan["row_tile"].tolist()
    for r in range(plan["R"]):
        lo, hi = ts[tile[r]], ts[tile[r] + 1]
        for rj in range(lo, hi):
            if drug[rj] == drug[r]:
                dense[drug[r], :, pos[r], pos[rj]] = tile_w[r, :, rj - lo]
    return dense


# ---------------------------------------------------------------------------------------------------- shared cases
def dense_masks(n, S, seed=31):
    """Key padding (p ~ 0.3, one key always open) and the source mask of test_ops_gpu.py::test_fusion_attention."""
    kpm = torch.rand(n, S, generator=torch.Generator().manual_seed(seed)) < 0.3
    kpm[:, min(3, S - 1)] = False
    src = torch.zeros(S, S, dtype=torch.bool)
    if S > 4:
        src[:2, -2:] = True
        src[-2:, :2] = True
    return kpm, src


def dense_allowed(n, S, kpm=None, src=None):
    ok = torch.ones(n, S, S, dtype=torch.bool)
    if kpm is not None:
        ok &= ~kpm.view(n, 1, S)
    if src is not None:
        ok &= ~src.view(1, S, S)
    return ok


def encoder_source_mask(nb, has_cls):
    """The encoder's [S, S] source mask: modality rows and tx rows may not attend each other (None without bottleneck tokens)."""
    if not nb:
        return None
    S0 = 19 + nb
    src = torch.zeros(S0, S0, dtype=torch.bool)
    src[:3, -16:] = True
    src[-16:, :3] = True
    if has_cls:
        full = torch.zeros(S0 + 1, S0 + 1, dtype=torch.bool)
        full[1:, 1:] = src
        src = full
    return src


def encoder_padding(absent, nb, has_cls):
    """Modality-absence masks [n, 19] -> token padding [n, S] of the sequence (cls) | 3 modalities | nb bottlenecks | 16 tx."""
    n = absent.shape[0]
    parts = ([torch.zeros(n, 1, dtype=torch.bool)] if has_cls else []) + [absent[:, :3]]
    if nb:
        parts.append(torch.zeros(n, nb, dtype=torch.bool))
    parts.append(absent[:, 3:])
    return torch.cat(parts, 1)


MIXED_SMALL = [1, 3, 2, 1, 3, 3, 2, 1, 2, 3]          # live tokens of the ten drugs that share one tile of case (a)


def mask_case(name, make_masks):
    """-> (live bool [n, S], source mask [S, S] or None).  ``make_masks``: the package's ``data.make_masks``."""
    if name == "mixed_tiles":
        # (a) ten drugs of 1..3 live tokens in one tile; 19 + 13 = a tile of exactly 32 rows; one single-token drug alone in the last
        S = 21
        counts = MIXED_SMALL + [19, 13, 1]
        g = torch.Generator().manual_seed(77)
        live = torch.zeros(len(counts), S, dtype=torch.bool)
        for i, c in enumerate(counts):
            live[i, torch.randperm(S, generator=g)[:c]] = True
        return live, None
    if name == "source_mask":
        # (b) two bottleneck tokens, S = 21, the encoder's source mask
        return ~encoder_padding(make_masks(12, 5, p_kg=0.6, p_cv=0.5, p_tx=0.2), 2, False), encoder_source_mask(2, False)
    if name == "full_drugs":
        # (c) S = 32, every token live, one drug per tile
        return torch.ones(3, 32, dtype=torch.bool), None
    if name == "random_masks":
        # (d) n = 37, cls + four bottleneck tokens, S = 24, the source mask with the cls row and column open
        return ~encoder_padding(make_masks(37, 11, p_kg=0.6, p_cv=0.5, p_tx=0.2), 4, True), encoder_source_mask(4, True)
    raise KeyError(name)


def dense_inputs(S, H, dh, n=DENSE_N, scale=1.0):
    d = H * dh
    qkv = rand((n * S, 3 * d), 30 + S)
    qkv[:, :2 * d] *= scale
    return qkv, rand((n * S, d), 60 + S)


def compact_inputs(R, H, dh, scale=1.0):
    d = H * dh
    qkv = rand((R, 3 * d), 130 + dh)
    qkv[:, :2 * d] *= scale
    return qkv, rand((R, d), 160 + dh)


def pool_inputs(n, Tk, H, dh, scale=1.0):
    d = H * dh
    kv = rand((n * Tk, 2 * d), 41)
    kv[:, :d] *= scale
    return rand((d,), 40) * scale, kv, rand((n, d), 42)


DROPOUT_QK_SCALE = 0.5       # q and k of the dropout cases: scores of a few tenths, so no allowed weight is near zero


def unit_values(rows_local, H, dh):
    """Value rows whose head-h block is the unit vector of the row's index inside its sequence / tile: then the attention output
    row of query x holds the dropped-out weights Pd[x, :] themselves."""
    R = len(rows_local)
    v = torch.zeros(R, H, dh)
    v[torch.arange(R), :, torch.as_tensor(rows_local)] = 1.0
    return v.reshape(R, H * dh)


@functools.lru_cache(maxsize=None)
def compact_reference(name, H, dh, make_masks, scale=1.0):
    """One compact case, computed once: (plan, qkv rows, dout rows, allowed, reference out rows, dqkv rows, weights [n,H,S,S])."""
    live, src = mask_case(name, make_masks)
    plan = pack_tiles(live, src)
    n, S, ti = plan["n"], plan["S"], plan["token_index"]
    qkv, dout = compact_inputs(plan["R"], H, dh, scale)
    allowed = compact_allowed(live, src)
    out, dqkv, P = attention_rows_ref(scatter_compact(qkv, ti, n, S), scatter_compact(dout, ti, n, S), n, S, H, dh, allowed)
    return plan, qkv, dout, allowed, out[ti], dqkv[ti], P
