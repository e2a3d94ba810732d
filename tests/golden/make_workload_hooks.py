"""Writes tests/golden/workload_hooks_kats.json: the known-answer cases of black_scholes_price, adam_update and crossentropy_terms.

Black-Scholes: the inputs and expected values of the reference's wgpu unit test (backend/wgpu/provider/ops/finance.rs:397-538), the
textbook case blsprice(100, 95, 0.1, 0.25, 0.5) = 13.6953 / 6.3497, and 500 seeded random cases.  `call` / `put` of every case are the
exact prices of the f64 inputs - mpmath at 50 digits, rounded to f64 once.  Deep learning: the two wgpu unit tests of
ops/deep_learning.rs:971-1112 as data (inputs, expected values, their tolerance of 1e-10).

    python tests/golden/make_workload_hooks.py        (needs mpmath)
"""
import json
from pathlib import Path

import mpmath as mp
import numpy as np

mp.mp.dps = 50


def exact_pair(S, K, r, T, sigma, q):
    S, K, r, T, sigma, q = [mp.mpf(float(x)) for x in (S, K, r, T, sigma, q)]
    d1 = (mp.log(S / K) + (r - q + sigma * sigma / 2) * T) / (sigma * mp.sqrt(T))
    d2 = d1 - sigma * mp.sqrt(T)
    fp, ds = S * mp.exp(-q * T), K * mp.exp(-r * T)
    return float(fp * mp.ncdf(d1) - ds * mp.ncdf(d2)), float(ds * mp.ncdf(-d2) - fp * mp.ncdf(-d1))


def cases(rows):
    out = {k: [] for k in ("price", "strike", "rate", "time", "volatility", "yield", "call", "put")}
    for S, K, r, T, sigma, q in rows:
        c, p = exact_pair(S, K, r, T, sigma, q)
        for k, v in zip(out, (S, K, r, T, sigma, q, c, p)):
            out[k].append(float(v))
    return out


def main():
    rng = np.random.default_rng(20260117)
    n = 500
    rows = np.column_stack([rng.uniform(50, 150, n), rng.uniform(50, 150, n), rng.uniform(0, 0.1, n), rng.uniform(0.05, 3, n),
                            rng.uniform(0.05, 0.8, n), rng.uniform(0, 0.05, n)])
    wgpu_rows = [(S, K, 0.05, 0.5, 0.2, 0.0) for K in (90.0, 100.0, 110.0) for S in (100.0, 110.0)]  # column-major over [2, 3]
    doc = {
        "black_scholes": {
            "wgpu_kat": {
                "price": {"shape": [2, 1], "data": [100.0, 110.0]},
                "strike": {"shape": [1, 3], "data": [90.0, 100.0, 110.0]},
                "rate": 0.05, "time": 0.5, "volatility": 0.2, "yield": 0.0,
                "output_shape": [2, 3],
                "expected_call": [13.498517482637212, 22.547751983647927, 6.888728577680624, 14.075384036381692, 2.906471321592413,
                                  7.577601435448678],
                "expected_put": [1.276409565187162, 0.32564406619787967, 4.41971978051388, 1.6063752392149624, 10.190561644708993,
                                 4.8616917585652715],
                "tolerance": 2.0e-5,
                "exact": cases(wgpu_rows),
            },
            "textbook": {"inputs": [100.0, 95.0, 0.1, 0.25, 0.5, 0.0], "call_4dp": 13.6953, "put_4dp": 6.3497,
                         "exact": cases([(100.0, 95.0, 0.1, 0.25, 0.5, 0.0)])},
            "random": cases(rows),
        },
        "adam_update": {
            "shape": [1, 3], "parameters": [1.0, 2.0, 3.0], "gradient": [0.1, -0.2, 0.3], "iteration": 1, "learn_rate": 0.01,
            "gradient_decay_factor": 0.9, "squared_gradient_decay_factor": 0.999, "epsilon": 1.0e-8,
            "expected_parameters": [0.990000001, 2.0099999995, 2.9900000003333334], "expected_average_grad": [0.01, -0.02, 0.03],
            "expected_average_sq_grad": [0.00001, 0.00004, 0.00009], "tolerance": 1.0e-10,
        },
        "crossentropy_terms": {
            "shape": [1, 2], "predictions": [0.8, 0.2], "targets": [1.0, 0.0], "weights": [2.0, 3.0], "mask": [1.0, 0.0],
            "mode": "multi-label", "expected": [float(-2 * mp.log(mp.mpf(0.8))), 0.0], "tolerance": 1.0e-10,
        },
    }
    out = Path(__file__).resolve().parent / "workload_hooks_kats.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
