"""Developer tool (GPU box): the complex gradient and the complex long FIR filter against their real siblings at equal bytes, interleaved A/B in one process.
usage: complex_calculus_bench.py [--rounds 9] [--reps 10] [--taps 16]
  gradient0 / gradient1  complex_gradient_dim of an 8192 x 4096 complex tensor along dim 0 / dim 1  against  gradient_dim of a 16384 x 4096
                         f64 tensor along the same dim: 16 B read and 16 B written per complex element, the same bytes on both sides
  fir                    complex_iir_filter_long of a 2^22 x 1 complex column signal with `taps` real coefficients  against  iir_filter_long of a
                         2^23 x 1 f64 column signal: the real one runs the LDS-tiled form, the complex one (leading = 2) the per-sample form
A round times `reps` calls of the complex op, then `reps` calls of the real op, each between device events (rmhip_timer_begin / _end);
outputs are freed inside the window on both sides (pool hits after the warm-up round, which is not counted).  The filter calls include
their coefficient read-back and the verdict's read-back: that is the call a user makes.  Reported per case: median microseconds and GB/s
of both over the rounds, each side's spread (min .. max over its rounds) and the ratio of the medians.  One JSON line per case, then the
table."""
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from runmat_amd.provider import HipProvider  # noqa: E402


def arg(name, default):
    a = sys.argv[1:]
    return int(a[a.index(name) + 1]) if name in a else default


def main():
    rounds, reps, taps = arg("--rounds", 9), arg("--reps", 10), arg("--taps", 16)
    rows_c, cols = 8192, 4096
    p = HipProvider(0)

    def complex_uniform(shape):
        re, im = p.random_uniform(shape), p.random_uniform(shape)
        z = p.complex_from_real_imag(re, im)
        p.free(re)
        p.free(im)
        return z

    z, r = complex_uniform((rows_c, cols)), p.random_uniform((2 * rows_c, cols))
    n = 1 << 22
    zs, rs = complex_uniform((n, 1)), p.random_uniform((2 * n, 1))
    b = p.upload(np.random.default_rng(5).standard_normal(taps).reshape(1, -1))
    a = p.upload(np.ones((1, 1)))

    def free_pair(pair):
        p.free(pair[0])
        p.free(pair[1])

    cases = {
        "gradient0": (32 * rows_c * cols, lambda: p.free(p.complex_gradient_dim(z, 0, 0.7)), lambda: p.free(p.gradient_dim(r, 0, 0.7))),
        "gradient1": (32 * rows_c * cols, lambda: p.free(p.complex_gradient_dim(z, 1, 0.7)), lambda: p.free(p.gradient_dim(r, 1, 0.7))),
        "fir": (32 * n, lambda: free_pair(p.complex_iir_filter_long(b, a, zs, 0)), lambda: free_pair(p.iir_filter_long(b, a, rs, 0))),
    }

    def window(fn):
        p.timer_begin()
        for _ in range(reps):
            fn()
        return p.timer_end() / reps  # ms per call

    out = []
    for name, (moved, fn, real) in cases.items():
        window(fn), window(real)  # warm-up: code objects, pool
        c_ms, r_ms = [], []
        for _ in range(rounds):
            c_ms.append(window(fn))
            r_ms.append(window(real))
        gbs = lambda ms: moved / (ms * 1e-3) / 1e9
        cm, rm = statistics.median(c_ms), statistics.median(r_ms)
        row = {"case": name, "bytes": moved, "complex_us": round(cm * 1e3, 1), "real_us": round(rm * 1e3, 1), "complex_gbs": round(gbs(cm), 1),
               "real_gbs": round(gbs(rm), 1), "real_gbs_min": round(gbs(max(r_ms)), 1), "real_gbs_max": round(gbs(min(r_ms)), 1),
               "complex_gbs_min": round(gbs(max(c_ms)), 1), "complex_gbs_max": round(gbs(min(c_ms)), 1), "ratio": round(rm / cm, 3)}
        print(json.dumps(row), flush=True)
        out.append(row)
    print(f"{'case':>10s} {'complex us':>11s} {'GB/s':>8s} {'(min .. max)':>17s} {'real us':>9s} {'GB/s':>8s} {'(min .. max)':>17s} {'ratio':>6s}")
    for r_ in out:
        print(f"{r_['case']:>10s} {r_['complex_us']:11.1f} {r_['complex_gbs']:8.1f} {r_['complex_gbs_min']:8.1f} ..{r_['complex_gbs_max']:7.1f} "
              f"{r_['real_us']:9.1f} {r_['real_gbs']:8.1f} {r_['real_gbs_min']:8.1f} ..{r_['real_gbs_max']:7.1f} {r_['ratio']:6.3f}")
    p.close()


if __name__ == "__main__":
    main()
