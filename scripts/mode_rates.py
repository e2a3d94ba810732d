"""Developer tool (GPU box): ms per call of mode_values for M, M + F and M + F + C against sort_dim and the sorting reduce_median_dim on the same operands.
usage: mode_rates.py [--reps N] [--small]
Shapes: 8192 x 8192 along each dimension and a vector of 1e7 elements with "all" (--small: 1024 x 1024 and 1e5, to rehearse), each on a
16-value alphabet and on all-distinct data.  The three calls share sort_lines; RMHIP_MEDIAN_SORT=1 keeps reduce_median_dim on the sort
instead of the radix selection, so its time is the sort plus one look per line, and sort_dim's is the sort plus the two emitted outputs.
Beyond the shared sort M / F reads the pair workspace once (12 bytes per padded element) and writes the candidates; C adds the run lengths
(4 bytes written, 8 read) and the compaction.  Timed with device events on the library's stream after warming every call; the tied sets'
host copy is inside the M + F + C figure.  Prints one JSON line per operand and the ratios to the two neighbours."""
import ctypes as C
import json
import os
import sys

os.environ["RMHIP_MEDIAN_SORT"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from runmat_amd import HipProvider  # noqa: E402


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    side, vec = (1024, 100_000) if "--small" in args else (8192, 10_000_000)
    p = HipProvider(0)
    lib, ctx = p._lib, p._ctx

    def timed(fn):
        fn()
        p.timer_begin()
        for _ in range(reps):
            fn()
        return p.timer_end() / reps

    def mode(h, axes, f, t):
        r = p.mode_values(h, axes, want_frequency=f, want_ties=t)
        p.free(r.values)
        if r.frequencies is not None:
            p.free(r.frequencies)

    def sort(h, dim):
        a, b = C.c_uint64(), C.c_uint64()
        p._check(lib.rmhip_sort_dim(ctx, h.buffer_id, dim, 0, 0, C.byref(a), C.byref(b)))
        p._check(lib.rmhip_free(ctx, a.value))
        p._check(lib.rmhip_free(ctx, b.value))

    rng = np.random.default_rng(5)
    for data in ("alphabet16", "distinct"):
        for shape, axes, dim in (((side, side), 0, 0), ((side, side), 1, 1), ((vec, 1), "all", 0)):
            n = shape[0] * shape[1]
            x = rng.integers(0, 16, n).astype(np.float64) if data == "alphabet16" else rng.permutation(n).astype(np.float64)
            h = p.upload(x, shape)
            out = {"data": data, "shape": list(shape), "axes": axes,
                   "mode_M_ms": timed(lambda: mode(h, axes, False, False)),
                   "mode_MF_ms": timed(lambda: mode(h, axes, True, False)),
                   "mode_MFC_ms": timed(lambda: mode(h, axes, True, True)),
                   "sort_dim_ms": timed(lambda: sort(h, dim)),
                   "median_sort_ms": timed(lambda: p.free(p.reduce_median_dim(h, dim)))}
            for k in ("mode_M_ms", "mode_MF_ms", "mode_MFC_ms"):
                out[k.replace("_ms", "_over_sort_dim")] = round(out[k] / out["sort_dim_ms"], 3)
                out[k.replace("_ms", "_over_median")] = round(out[k] / out["median_sort_ms"], 3)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
            p.free(h)
    p.close()


if __name__ == "__main__":
    main()
