"""Developer tool (GPU box): host-side cost of one fft_dim call on launch-bound shapes - an 8-point transform and a one-tile 4096-point
one - where the planning in fft_plan.h and the table lookups are what a call costs; the per-call loop of scripts/call_overhead.py.
Prints one JSON line; two builds of the library alternate through RMHIP_LIBRARY."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from runmat_amd import HipProvider
prov = HipProvider(0)
def rate(f, n=3000):
    for _ in range(50): prov.free(f())
    prov.synchronize(); t0 = time.perf_counter()
    for _ in range(n): prov.free(f())
    t1 = time.perf_counter(); prov.synchronize(); t2 = time.perf_counter()
    return {"enqueue_us": round(1e6 * (t1 - t0) / n, 3), "drained_us": round(1e6 * (t2 - t0) / n, 3)}
a = prov.upload(np.ones(8), (8,)); b = prov.upload(np.ones(4096), (4096,))
print(json.dumps({"library": os.environ.get("RMHIP_LIBRARY", "tree"), "fft 8": rate(lambda: prov.fft_dim(a, None, 0)), "fft 4096": rate(lambda: prov.fft_dim(b, None, 0))}))
