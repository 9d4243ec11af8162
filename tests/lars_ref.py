"""The LARS input set of tests/golden/lars_reference.npz and a float64 restatement of the algorithm (madrigal/utils.py:628-662).

Shared by scripts/gen_optim_golden.py (which records the reference's own fp32 run on these inputs), tests/test_optimizers_cpu.py
and tests/test_optimizers_gpu.py.  Everything is seeded: parameter i is randn from ``manual_seed(PARAM_SEED + i)``, its gradient at
step s randn from ``manual_seed(100 * s + i)``.

The shapes cover one element, exactly one 4096-element chunk, one chunk plus a tail, 160 chunks (more than a wave), 300 chunks (more
than a block's threads) and 1-D tensors (no decay, no trust ratio).  Group B moves its parameters by about 1.5x their norm over the
run, so that a wrong trust ratio shows in ``p``; with the default coefficient it shows in ``mu`` only.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

STEPS = 6
PARAM_SEED = 5000
SHAPES = [(3, 5), (7,), (1,), (1, 1), (2, 3, 4), (1, 4096), (4097, 3), (40, 128, 128), (300, 4096), (4, 4), (5000,)]
ZERO_PARAM = 9                                              # (4,4): all zeros, zero gradient for two steps -> |p| = 0 and |u| = 0
DEFAULTS = dict(lr=.2, weight_decay=1e-6, momentum=.9)      # constructor arguments (trust_coefficient: the class default, 0.001)
TRUST_DEFAULT = 0.001
GROUPS = [(range(0, 5), dict(lr=.1, weight_decay=1e-2)),
          (range(5, 9), dict(lr=1.0, weight_decay=1e-4, momentum=.5, trust_coefficient=.3)),
          (range(9, 11), dict(lr=.3, weight_decay=0.0))]
# the two large tensors enter the fixture as every STRIDE-th element of the flattened tensor (a committed file stays below 1 MiB); the
# trust ratio is one number per tensor, so every element carries it
STRIDE = {7: 37, 8: 61}


def initial_params(dtype=torch.float32):
    ps = [torch.randn(s, generator=torch.Generator().manual_seed(PARAM_SEED + i)) for i, s in enumerate(SHAPES)]
    ps[ZERO_PARAM].zero_()
    for p in ps:
        # a one-element tensor is its own scale in the tests' measure: it starts at 4 + randn, so that it does not pass through zero
        # during the run (lr * sum of mu is about 1 for the 1-D one), where fp32 storage of p alone would cost more than the bound
        if p.numel() == 1:
            p += 4.0
    return [p.to(dtype) for p in ps]


def grad(step: int, i: int, dtype=torch.float32):
    """The gradient of parameter i at step ``step``; None = the parameter has no gradient at that step."""
    if i == 4 and step == 1:
        return None
    g = torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(100 * step + i))
    if (i == ZERO_PARAM and step < 2) or (i == 0 and step == 2):
        g.zero_()
    return g.to(dtype)


def param_groups(ps):
    return [dict(params=[ps[i] for i in idx], **kw) for idx, kw in GROUPS]


def hyper(i: int) -> dict:
    h = dict(DEFAULTS, trust_coefficient=TRUST_DEFAULT)
    for idx, kw in GROUPS:
        if i in idx:
            h.update(kw)
    return h


def lars_update(p, g, mu, lr, weight_decay, momentum, trust_coefficient):
    """One LARS update of one tensor, out of place, in the dtype of its arguments; returns (p, mu)."""
    u = g
    if p.ndim > 1:
        u = g + weight_decay * p
        pn, un = float(p.square().sum().sqrt()), float(u.square().sum().sqrt())
        if pn > 0 and un > 0:
            u = u * (trust_coefficient * pn / un)
    mu = momentum * mu + u
    return p - lr * mu, mu


@functools.lru_cache(maxsize=None)
def restatement(steps: int = STEPS):
    """(parameters, mu) after ``steps`` steps in float64; computed once per process, callers must not modify it."""
    ps = initial_params(torch.float64)
    mus = [torch.zeros_like(p) for p in ps]
    for s in range(steps):
        for i in range(len(ps)):
            g = grad(s, i, torch.float64)
            if g is not None:
                ps[i], mus[i] = lars_update(ps[i], g, mus[i], **hyper(i))
    return ps, mus


def stored(i: int, x):
    """The entries of tensor i that the fixture holds, flattened."""
    return x.reshape(-1)[::STRIDE.get(i, 1)]


def distance(a, b, floor: float = 1e-6) -> float:
    """The ``_close`` measure of tests/test_train_gpu.py: max |a - b| over max(|b|_max, floor), b the reference."""
    a, b = ((x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))).double() for x in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor)
