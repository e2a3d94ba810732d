"""Developer tool (GPU box): GB/s of the complex elementwise kernels (C o C mul, C o R mul, abs, sin) at 2^26 complex elements against the real elem_mul at equal bytes moved, interleaved A/B in one process.
usage: complex_ew_bench.py [--log2n 26] [--rounds 9] [--reps 20]
Per case the real elem_mul runs on as many f64 elements as move the same algorithmic bytes (24 per element: two reads, one write):
  cc_mul  48 B per complex element (two 16-byte reads, one 16-byte write)      cr_mul  40 B (16 + 8 read, 16 written)
  abs     24 B (16 read, 8 written)                                            sin     32 B (16 read, 16 written; four libm calls)
A round times `reps` calls of the complex op, then `reps` calls of the real op, each between device events (rmhip_timer_begin / _end);
outputs are freed inside the window on both sides (pool hits after the warm-up round, which is not counted).  Reported per case:
median GB/s of both over the rounds, the real kernel's spread (min .. max over its rounds) and the ratio of the medians.  One JSON
line per case, then the table."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from runmat_amd.provider import HipProvider  # noqa: E402


def arg(name, default):
    a = sys.argv[1:]
    return int(a[a.index(name) + 1]) if name in a else default


def main():
    n = 1 << arg("--log2n", 26)
    rounds, reps = arg("--rounds", 9), arg("--reps", 20)
    p = HipProvider(0)
    re, im, re2, im2 = (p.random_uniform((n, 1)) for _ in range(4))
    za, zb = p.complex_from_real_imag(re, im), p.complex_from_real_imag(re2, im2)
    for h in (im, re2, im2):
        p.free(h)
    cases = {"cc_mul": (48, lambda: p.complex_binary("mul", za, zb)), "cr_mul": (40, lambda: p.complex_binary("mul", za, re)),
             "abs": (24, lambda: p.complex_unary("abs", za)), "sin": (32, lambda: p.complex_unary("sin", za))}

    def window(fn):
        p.timer_begin()
        for _ in range(reps):
            p.free(fn())
        return p.timer_end() / reps  # ms per call

    rows = []
    for name, (bytes_per, fn) in cases.items():
        moved = bytes_per * n
        m = moved // 24  # real elements that move the same bytes
        ra, rb = p.random_uniform((m, 1)), p.random_uniform((m, 1))
        real = lambda: p.elem_mul(ra, rb)
        window(fn), window(real)  # warm-up: code objects, pool
        c_ms, r_ms = [], []
        for _ in range(rounds):
            c_ms.append(window(fn))
            r_ms.append(window(real))
        gbs = lambda ms, b: b / (ms * 1e-3) / 1e9
        c, r = gbs(statistics.median(c_ms), moved), gbs(statistics.median(r_ms), 24 * m)
        row = {"case": name, "complex_elements": n, "bytes_per_element": bytes_per, "real_elements": m, "complex_gbs": round(c, 1), "real_gbs": round(r, 1),
               "real_gbs_min": round(gbs(max(r_ms), 24 * m), 1), "real_gbs_max": round(gbs(min(r_ms), 24 * m), 1),
               "complex_gbs_min": round(gbs(max(c_ms), moved), 1), "complex_gbs_max": round(gbs(min(c_ms), moved), 1), "ratio": round(c / r, 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        p.free(ra)
        p.free(rb)
    print(f"{'case':>7s} {'B/elt':>5s} {'complex GB/s':>13s} {'(min .. max)':>17s} {'real GB/s':>10s} {'(min .. max)':>17s} {'ratio':>6s}")
    for r in rows:
        print(f"{r['case']:>7s} {r['bytes_per_element']:5d} {r['complex_gbs']:13.1f} {r['complex_gbs_min']:8.1f} ..{r['complex_gbs_max']:7.1f} {r['real_gbs']:10.1f} "
              f"{r['real_gbs_min']:8.1f} ..{r['real_gbs_max']:7.1f} {r['ratio']:6.3f}")
    p.close()


if __name__ == "__main__":
    main()
