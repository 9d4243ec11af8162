"""The x-attn pooling tail of the fusion transformer at the bench shape, folded against unfolded, piece by piece (device events,
median of 20 launches each):  python scripts/xattn_fold_bench.py [--config twosides321] [--drugs 4096] [--precision bf16x3]

Folded: kv-norm with logits (mdg_layernorm_logits) -> P = U C^T (mdg_linear_packed_x, N = H*D) -> mdg_xattn_fold_pool.
Unfolded: kv-norm (mdg_layernorm_packed) -> K|V block (N = 2d) -> mdg_xattn_pool -> out_proj + query -> latent2embed.
The product P is also timed on both tile kernels (MDG_LINEAR_TILE=128 / 256) and set against its FLOP and store bounds."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from madrigal_amd import configs, ops  # noqa: E402
from madrigal_amd._lib import lib  # noqa: E402

BF16_PEAK = 2.5e15          # dense bf16 MFMA, spec
STORE_BW = 5.9e12           # measured store ceiling of the card


def med_ms(fn, reps=20):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="twosides321", choices=sorted(configs.SHIPPED))
    ap.add_argument("--drugs", type=int, default=4096)
    ap.add_argument("--precision", default="bf16x3", choices=["f32", "bf16x3", "bf16"])
    a = ap.parse_args()
    tf = configs.SHIPPED[a.config]["tf"]
    H, dh, D, Tk, n, prec = tf["transformer_att_heads"], tf["transformer_head_dim"], 128, configs.SHIPPED[a.config]["nb"], a.drugs, a.precision
    d, R = H * dh, n * Tk
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")                   # noqa: E731
    h = r(R, d)
    gam, bet = 1.0 + 0.1 * r(d), 0.1 * r(d)
    C, G, cz = r(H * D, d) / d ** 0.5, r(H, d) / d ** 0.5, r(D)
    Wkv, bkv, qp = r(2 * d, d) / d ** 0.5, r(2 * d), r(d)
    Wo, bo, Wle, ble, q = r(d, d) / d ** 0.5, r(d), r(D, d) / d ** 0.5, r(D), r(d)
    C_img = ops.pack_operand(C, prec)
    out = {"config": a.config, "precision": prec, "rows": R, "d": d, "H": H, "N_fold": H * D}
    with torch.no_grad():
        u, img, lg = ops.layernorm_logits(h, gam, bet, 1e-5, G, prec)

        def product():
            return ops.linear_packed(img, R, C, precision=prec, weight_image=C_img) if img is not None else \
                ops.linear(u, C, precision=prec, weight_image=C_img)
        P = product()
        out["norm_plain_ms"] = med_ms(lambda: ops.layernorm_packed(h, gam, bet, 1e-5, prec, want_fp32=False))
        out["norm_logits_ms"] = med_ms(lambda: ops.layernorm_logits(h, gam, bet, 1e-5, G, prec))
        for tile in ("128", "256"):
            os.environ["MDG_LINEAR_TILE"] = tile
            lib().mdg_tuning_reload()
            out[f"product_ms_tile{tile}"] = med_ms(product)
        os.environ.pop("MDG_LINEAR_TILE")
        lib().mdg_tuning_reload()
        out["product_ms_default"] = med_ms(product)
        out["combine_ms"] = med_ms(lambda: ops.xattn_fold_pool(P, lg, cz, n, Tk))
        out["folded_tail_ms"] = med_ms(lambda: ops.xattn_fold_pool(product(), ops.layernorm_logits(h, gam, bet, 1e-5, G, prec)[2], cz, n, Tk))
        flops, store = 2.0 * R * d * H * D * (3 if prec == "bf16x3" else 1), 4.0 * R * H * D
        out["product_flop_bound_ms"] = flops / BF16_PEAK * 1e3
        out["product_store_bound_ms"] = store / STORE_BW * 1e3

        def unfolded():
            _, im = ops.layernorm_packed(h, gam, bet, 1e-5, prec, want_fp32=False)
            kv = ops.linear_packed(im, R, Wkv, bkv, precision=prec) if im is not None else \
                ops.linear(ops.layernorm(h, gam, bet, 1e-5), Wkv, bkv, precision=prec)
            pooled = ops.xattn_pool(qp, kv, n, Tk, H, dh)
            o = ops.linear(pooled, Wo, bo, residual=q, precision=prec)
            return ops.linear(o, Wle, ble, precision=prec)
        out["unfolded_tail_ms"] = med_ms(unfolded)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
