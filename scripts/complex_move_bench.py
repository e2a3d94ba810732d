"""Developer tool (GPU box): GB/s of the 16-byte movers (complex_transpose, complex_circshift, complex_gather_linear) against their real siblings at equal bytes moved, interleaved A/B in one process.
usage: complex_move_bench.py [--log2n 13] [--rounds 9] [--reps 10]
With N = 2^log2n (default 8192):
  transpose  complex_transpose of N x N complex        against  permute [1, 0] of a 2N x N f64 matrix (rmhip_transpose is a lazy view)
  circshift  complex_circshift by (N/2, N/2) of N x N  against  circshift by (N, N/2) of 2N x N f64
  gather     complex_gather_linear of N^2 / 4 seeded random indices out of N^2 elements  against  gather_linear of N^2 / 2 out of 2 N^2
Bytes moved: one read and one write per element (32 B per complex element, 16 B per f64 element); the gathers add their 4-byte index
reads on both sides.  A round times `reps` calls of the complex op, then `reps` calls of the real op, each between device events
(rmhip_timer_begin / _end); outputs are freed inside the window on both sides (pool hits after the warm-up round, which is not
counted).  The gathers include their index upload and the bounds verdict's read-back: that is the call a user makes.  Reported per
case: median microseconds and GB/s of both over the rounds, the real kernel's spread (min .. max over its rounds) and the ratio of the
medians.  One JSON line per case, then the table."""
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
    n = 1 << arg("--log2n", 13)
    rounds, reps = arg("--rounds", 9), arg("--reps", 10)
    p = HipProvider(0)
    re, im = p.random_uniform((n, n)), p.random_uniform((n, n))
    z = p.complex_from_real_imag(re, im)
    p.free(re)
    p.free(im)
    r = p.random_uniform((2 * n, n))
    rng = np.random.default_rng(16)
    zi = rng.integers(0, n * n, n * n // 4).astype(np.uint32)
    ri = rng.integers(0, 2 * n * n, n * n // 2).astype(np.uint32)
    cases = {
        "transpose": (32 * n * n, lambda: p.complex_transpose(z), lambda: p.permute(r, (1, 0))),
        "circshift": (32 * n * n, lambda: p.complex_circshift(z, (n // 2, n // 2)), lambda: p.circshift(r, (n, n // 2))),
        "gather": (36 * zi.size, lambda: p.complex_gather_linear(z, zi, (zi.size, 1)), lambda: p.gather_linear(r, ri, (ri.size, 1))),
    }
    real_bytes = {"transpose": 16 * 2 * n * n, "circshift": 16 * 2 * n * n, "gather": 20 * ri.size}

    def window(fn):
        p.timer_begin()
        for _ in range(reps):
            p.free(fn())
        return p.timer_end() / reps  # ms per call

    rows = []
    for name, (moved, fn, real) in cases.items():
        window(fn), window(real)  # warm-up: code objects, pool
        c_ms, r_ms = [], []
        for _ in range(rounds):
            c_ms.append(window(fn))
            r_ms.append(window(real))
        gbs = lambda ms, b: b / (ms * 1e-3) / 1e9
        cm, rm = statistics.median(c_ms), statistics.median(r_ms)
        c, rr = gbs(cm, moved), gbs(rm, real_bytes[name])
        row = {"case": name, "n": n, "complex_bytes": moved, "real_bytes": real_bytes[name], "complex_us": round(cm * 1e3, 1), "real_us": round(rm * 1e3, 1),
               "complex_gbs": round(c, 1), "real_gbs": round(rr, 1),
               "real_gbs_min": round(gbs(max(r_ms), real_bytes[name]), 1), "real_gbs_max": round(gbs(min(r_ms), real_bytes[name]), 1),
               "complex_gbs_min": round(gbs(max(c_ms), moved), 1), "complex_gbs_max": round(gbs(min(c_ms), moved), 1), "ratio": round(c / rr, 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    print(f"{'case':>10s} {'complex us':>11s} {'GB/s':>8s} {'(min .. max)':>17s} {'real us':>9s} {'GB/s':>8s} {'(min .. max)':>17s} {'ratio':>6s}")
    for r_ in rows:
        print(f"{r_['case']:>10s} {r_['complex_us']:11.1f} {r_['complex_gbs']:8.1f} {r_['complex_gbs_min']:8.1f} ..{r_['complex_gbs_max']:7.1f} "
              f"{r_['real_us']:9.1f} {r_['real_gbs']:8.1f} {r_['real_gbs_min']:8.1f} ..{r_['real_gbs_max']:7.1f} {r_['ratio']:6.3f}")
    p.close()


if __name__ == "__main__":
    main()
