"""Developer tool (GPU box): ms per call of one of
    unique     unique_rows (sorted, first occurrence), results downloaded as the entry point does
    sortrows   rmhip_sort_rows over all four columns ascending: the same four sort passes, no grouping, nothing downloaded
    download   the download of one [2^20, 1] tensor (what `ic` costs on its way to the host)
on a 2^20 x 4 matrix of integers in [0, 8).
usage: rowset_rates.py unique|sortrows|download [reps]
A host clock around calls that end in a device synchronise; three warm-up calls; prints one JSON line (median, min, max).  Each run is a
process of its own, so two builds of the library (RMHIP_LIBRARY=/path/to/librmhip.so) can be alternated from a shell loop."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from runmat_amd import HipProvider  # noqa: E402


def main():
    which, reps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 15
    p = HipProvider(0)
    x = np.random.default_rng(1).integers(0, 8, size=(1 << 20, 4)).astype(np.float64)
    h = p.upload(x.ravel(order="F"), x.shape)
    col = p.upload(np.arange(float(1 << 20)), (1 << 20, 1))
    idx, desc = (C.c_size_t * 4)(0, 1, 2, 3), (C.c_int * 4)(0, 0, 0, 0)

    def run():
        if which == "unique":
            p.unique_rows(h)
        elif which == "sortrows":  # the C entry point itself (it synchronises); the Python mirror would download both results
            sv, si = C.c_uint64(), C.c_uint64()
            p._check(p._lib.rmhip_sort_rows(p._ctx, p._id(h), idx, desc, 4, 0, C.byref(sv), C.byref(si)))
            p._check(p._lib.rmhip_free(p._ctx, sv.value))
            p._check(p._lib.rmhip_free(p._ctx, si.value))
        elif which == "download":
            p.download(col)
        else:
            raise SystemExit(__doc__)

    for _ in range(3):
        run()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    line = {"which": which, "library": os.environ.get("RMHIP_LIBRARY", "tree"), "reps": reps, "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
    if which == "unique":
        line["count"] = int(p.unique_rows(h)[0].shape[0])
    print(json.dumps(line))
    p.close()


if __name__ == "__main__":
    main()
