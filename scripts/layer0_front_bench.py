"""Time the front of fusion layer 0 alone -- everything from the live token rows T to h after the attention block's residual -- on
the composed-QKV path (embed2latent, row_rstd, the K = 128 QKV block, attention over 3d columns, out_proj with the residual) and
in token space (TransformerFusion._layer0_tokenspace), at the bench shape (4096 drugs, live-token layout).  Device events, median
of 20, the three arithmetic modes; the two results are compared on the way.

    python scripts/layer0_front_bench.py [drugs] [config ...]       (default: 4096, all three shipped configs)
"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from madrigal_amd import configs, data, models as M, ops

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
names = sys.argv[2:] or ["twosides321", "twosides105", "drugbank163"]
batch, bkg = data.make_batch(n, seed=0, kg_nodes=2000, kg_edges=20000)
b = data.batch_to(batch, "cuda")


def median_us(f, reps=20):
    for _ in range(3):
        f()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return sorted(times)[len(times) // 2]


for name in names:
    enc = configs.build_model(name, bkg["data"], n_outcomes=8).cuda().eval().encoder
    plan = enc._mask_plan(b["masks"], torch.device("cuda"), True)["live"]
    tf = enc.transformer
    L, H, dh, d, S, R = tf.transformer_encoder.layers[0], tf.num_heads, tf.head_dim, tf.latent_dim, plan["S"], plan["R"]
    sa = L.self_attn
    tokens = torch.randn(R, 128, device="cuda") + 0.5
    tiles = dict(row_start=plan["tile_start"], row_bits=plan["row_bits"])

    def attend(qkv, _x, out=None):
        if isinstance(qkv, tuple):
            q, k, v, w = qkv
            return ops.fusion_attention_qkv(q, k, v, plan["n_tiles"], S, H, w, w, hq=w, hk=0, hv=0, out=out, ho=w, **tiles)
        return ops.fusion_attention(qkv, plan["n_tiles"], S, H, dh, **tiles)[0]

    def old_front():
        h = M._lin(tokens, tf.embed2latent.weight, tf.embed2latent.bias)
        return M._lin(attend(tf._qkv0(L, tokens, h), None), sa.out_proj.weight, sa.out_proj.bias, residual=h)

    def new_front():
        return tf._layer0_tokenspace(L, tokens, attend)

    for prec in ("f32", "bf16x3", "bf16"):
        with torch.no_grad(), M.precision(prec):
            a, c = old_front(), new_front()
            err = float((a - c).abs().max() / a.abs().max())
            t_old, t_new = median_us(old_front), median_us(new_front)
            ok = bool(tf._tokenspace_ok())
        print(json.dumps({"config": name, "precision": prec, "rows": R, "tiles": plan["n_tiles"], "H": H, "d": d, "K_out_proj": H * 132 + 128,
                          "takes_tokenspace": ok, "old_front_us": round(t_old, 1), "new_front_us": round(t_new, 1),
                          "max_rel_diff": err}), flush=True)
