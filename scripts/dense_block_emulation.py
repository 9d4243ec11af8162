"""CPU emulation of the dense block's two 16-bit arithmetic modes: where the bounds of tests/test_dense_block_256_gpu.py come from.

    python scripts/dense_block_emulation.py

bf16:   operands rounded to bf16, exact products, fp32 accumulation (one fp32 add per 32-deep MFMA block) -- measured against the
        float64 product of the ROUNDED operands, relative to max|ref| (the test's bound: 2e-6).
bf16x3: x = hi + lo split per operand, lo.hi + hi.lo + hi.hi per 32-deep block in that order, fp32 accumulation -- measured against
        the float64 product of the fp32 operands, relative to max(max|ref|, 1) (the test's bound: 2e-5); and the same with one of
        the three products left out, which is what the bound has to catch.
Operands as the tests draw them (x ~ N(0,1), w ~ N(0,1) / sqrt(K)); K = every inner length the test file uses.  No GPU needed.
"""
import math

import torch


def rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def blocks(K):
    return [(k, min(k + 32, K)) for k in range(0, K, 32)]


def emulate_bf16(x, w):
    xr, wr = x.bfloat16().float(), w.bfloat16().float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for a, b in blocks(x.shape[1]):
        acc = acc + xr[:, a:b] @ wr[:, a:b].T
    return acc, xr.double() @ wr.double().T


def emulate_x3(x, w, skip=None):
    xh, wh = x.bfloat16().float(), w.bfloat16().float()
    xl, wl = (x - xh).bfloat16().float(), (w - wh).bfloat16().float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for a, b in blocks(x.shape[1]):
        for pr, (p, q) in enumerate(((xl, wh), (xh, wl), (xh, wh))):
            if pr != skip:
                acc = acc + p[:, a:b] @ q[:, a:b].T
    return acc, x.double() @ w.double().T


def main():
    torch.set_num_threads(8)
    M, N = 300, 260
    worst = {"bf16": 0.0, "bf16x3": 0.0}
    least_dropped = float("inf")
    print(f"{'K':>5} {'bf16':>10} {'bf16x3':>10}   bf16x3 without lo.hi / hi.lo / hi.hi")
    for K in (4, 36, 64, 68, 96, 128, 160, 192, 256, 512, 559, 2048):
        x, w = rand((M, K), 1), rand((N, K), 2, 1 / math.sqrt(K))
        got, ref = emulate_bf16(x, w)
        e1 = float((got.double() - ref).abs().max() / ref.abs().max())
        got, ref = emulate_x3(x, w)
        scale = max(float(ref.abs().max()), 1.0)
        e3 = float((got.double() - ref).abs().max()) / scale
        dropped = [float((emulate_x3(x, w, s)[0].double() - ref).abs().max()) / scale for s in range(3)]
        worst["bf16"], worst["bf16x3"] = max(worst["bf16"], e1), max(worst["bf16x3"], e3)
        least_dropped = min(least_dropped, min(dropped[:2]))
        print(f"{K:>5} {e1:>10.2e} {e3:>10.2e}   " + " / ".join(f"{d:.2e}" for d in dropped))
    print(f"worst: bf16 {worst['bf16']:.2e} (bound 2e-6), bf16x3 {worst['bf16x3']:.2e} (bound 2e-5); "
          f"smallest error of a dropped cross product {least_dropped:.2e}")


if __name__ == "__main__":
    main()
