"""Developer tool (GPU box): cov(x, y) and weighted cov (rmhip_covariance_general) against the plain covariance on the same shapes, interleaved A/B in one process - us per call, spread, ratio to the plain form beside the byte ratio.
The weighted call includes its one 16-byte read-back; every timing window ends in a device synchronise (timer_end)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from runmat_amd import HipProvider

ROUNDS, CALLS = 9, 20
prov = HipProvider(0)


def window(f):
    prov.timer_begin()
    for _ in range(CALLS):
        prov.free(f())
    return prov.timer_end() / CALLS * 1e3  # us per call


for rows, cols in [(1 << 20, 8), (1 << 18, 32), (20000, 64)]:
    x = prov.fill_uniform(2, -1.0, 1.0, (rows, cols))
    xa = prov.fill_uniform(3, -1.0, 1.0, (rows, cols // 2))
    xb = prov.fill_uniform(4, -1.0, 1.0, (rows, cols // 2))
    w = prov.fill_uniform(5, 0.0, 2.0, (rows, 1))
    cases = {
        "plain": lambda: prov.covariance(x),
        "weighted": lambda: prov.covariance_general(x, weights=w),
        f"two operands {cols // 2}+{cols // 2}": lambda: prov.covariance_general(xa, second=xb),
        "two operands weighted": lambda: prov.covariance_general(xa, second=xb, weights=w),
    }
    for f in cases.values():  # warm every case: code objects, scratch, pool
        for _ in range(3):
            prov.free(f())
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):  # interleaved: one window of every case per round
        for k, f in cases.items():
            times[k].append(window(f))
    base = float(np.median(times["plain"]))
    route = "skinny" if cols <= 40 and rows >= 4096 and rows >= 64 * cols else "MFMA"
    print(f"{rows} x {cols} ({route} route), {ROUNDS} rounds of {CALLS} calls; bytes per row: plain {8 * cols}, weighted {8 * cols + 8} (ratio {(8 * cols + 8) / (8 * cols):.3f})", flush=True)
    for k, v in times.items():
        med = float(np.median(v))
        print(f"    {k:28s} {med:8.1f} us  (min {min(v):8.1f}, max {max(v):8.1f})  x{med / base:5.2f} of plain", flush=True)
    for h in (x, xa, xb, w):
        prov.free(h)
prov.close()
