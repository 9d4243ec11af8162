"""numpy references for the checkpoint-ensemble spread (csrc/ensemble_spread.hip; tests/test_ensemble_spread_cpu.py, _gpu.py).

``spread64``   float64 mean(0) and std(0) (population, ddof = 0) of a [K, ...] fp32 array: the reference.
``welford32``  the kernel's recurrence restated step by step in np.float32 (spread_update / spread_finish): every operation rounded
               to fp32, no contraction, the running sum kept beside it.
``naive32``    the one-pass formula the kernel must NOT use, sum p^2 - (sum p)^2 / K in fp32: it cancels where the probabilities
               round to 1.
``cases``      the two input sets the restatement is measured on, with fixed seeds.
``E_R``        the largest absolute std error of ``welford32`` against ``spread64`` over ``cases()``, as measured.
"""
import numpy as np

E_R = 6.66e-8        # measured 6.654e-08 (uniform, K = 8); per case: test_ensemble_spread_cpu.py prints them

N_SAMPLES = 1 << 16


def spread64(p):
    p64 = np.asarray(p, dtype=np.float64)
    return p64.mean(0), p64.std(0)


def welford32(p):
    """(mean, std, M2) of the [K, ...] fp32 array ``p`` by the kernel's recurrence, every step in np.float32."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    K = p.shape[0]
    s = p[0].copy()
    mu = p[0].copy()
    m2 = np.zeros_like(p[0])
    for n in range(2, K + 1):
        x = p[n - 1]
        rn = np.float32(1.0) / np.float32(n)
        d = x - mu
        mu = mu + d * rn
        m2 = m2 + d * (x - mu)
        s = s + x
    kf = np.float32(K)
    return s / kf, np.sqrt(m2 / kf), m2


def naive32(p):
    """std by sum p^2 - (sum p)^2 / K in fp32; NaN where the difference went negative (``std_error`` counts a NaN as infinite;
    ``np.nan_to_num`` of it shows the size of the noise)."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    K = p.shape[0]
    s = p[0].copy()
    q = p[0] * p[0]
    for n in range(1, K):
        s = s + p[n]
        q = q + p[n] * p[n]
    kf = np.float32(K)
    with np.errstate(invalid="ignore"):
        return np.sqrt((q - s * s / kf) / kf)


def cases():
    """{name: [K, N_SAMPLES] fp32}: (a) uniform probabilities, (b) saturated ones, p = float32(1 - u 2^-20), u uniform in [0, 16)."""
    out = {}
    for K in (2, 5, 8):
        rng = np.random.default_rng(100 + K)
        out[f"uniform_K{K}"] = rng.random((K, N_SAMPLES), dtype=np.float64).astype(np.float32)
        u = rng.random((K, N_SAMPLES), dtype=np.float64) * 16.0
        out[f"saturated_K{K}"] = (1.0 - u * 2.0 ** -20).astype(np.float32)
    return out


def std_error(fn, p):
    """Largest absolute error of ``fn(p)``'s std against float64; a NaN counts as infinite."""
    got = fn(p)
    got = got[1] if isinstance(got, tuple) else got
    err = np.abs(got.astype(np.float64) - spread64(p)[1])
    return float(np.where(np.isnan(err), np.inf, err).max())
