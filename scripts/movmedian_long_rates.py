"""Developer tool (GPU box): ms per call of moving_window_long (movmedian over long windows) against what the caller pays for those shapes without it - gather, the oracle's CPU median, upload.
usage: movmedian_long_rates.py [--reps N] [--warm N] [--small]
Shapes: 2^20 x 1 along dim 0 with windows of 101, 1001 and 4096 points, 4096 x 4096 along dim 1 with 257 points and, for scale, moving_window's own
median at 64 points on the first shape (--small: 2^14 x 1 and 256 x 256, to rehearse).  Standard normal data, shrinking endpoints.  Per case:
  long_ms      the entry point, the mean of --reps (20) calls after --warm (3), device events on the library's stream
  visits_per_s outputs x window points x 8 digit levels / long_ms: the key visits of a select that never stops early, an upper bound on the
               LDS key reads actually made (a level stops once one candidate is left), against the LDS read rate
  gather_ms / upload_ms   rmhip_download of the operand / rmhip_upload of the result, host clock around a synchronised call
  host_ms      oracle.moving_window(..., "median") on a SAMPLE of the same lines (the first `sample` points of a line along dim 0, the first
               `sample` lines along dim 1), scaled to the full size: a scaled figure, not a measurement of the whole run
One JSON line per case."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import oracle  # noqa: E402
from runmat_amd import HipProvider  # noqa: E402

LDS_KEYS_PER_S = 150e12 / 8.0  # ds_read_b64 with every CU streaming: about 150 TB/s


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
    warm = int(args[args.index("--warm") + 1]) if "--warm" in args else 3
    long_n, side = (1 << 14, 256) if "--small" in args else (1 << 20, 4096)
    p = HipProvider(0)
    sync = p.upload(np.zeros((1, 1)))

    def device_ms(fn):
        for _ in range(warm):
            fn()
        p.timer_begin()
        for _ in range(reps):
            fn()
        return p.timer_end() / reps

    def host_ms(fn):
        p.download(sync)
        t = time.perf_counter()
        out = fn()
        p.download(sync)
        return (time.perf_counter() - t) * 1e3, out

    rng = np.random.default_rng(1)
    cases = [((long_n, 1), 0, 50, 50, "long", 20000), ((long_n, 1), 0, 500, 500, "long", 20000), ((long_n, 1), 0, 2047, 2048, "long", 8192),
             ((side, side), 1, 128, 128, "long", 16), ((long_n, 1), 0, 32, 31, "moving_window", 20000)]
    for shape, dim, before, after, entry, sample in cases:
        x = rng.standard_normal(shape)
        h = p.upload(x.ravel(order="F"), list(shape))
        call = p.moving_window_long if entry == "long" else p.moving_window
        long_ms = device_ms(lambda: p.free(call(h, list(shape), dim, before, after, "median")))
        gather_ms, host = host_ms(lambda: p.download(h))
        upload_ms, hy = host_ms(lambda: p.upload(host, list(shape)))
        part = x[:min(sample, shape[0])]
        t = time.perf_counter()
        oracle.moving_window(part, dim, before, after, "median")
        cpu_ms = (time.perf_counter() - t) * 1e3 * shape[0] / part.shape[0]
        w = min(shape[dim], before + after + 1)
        visits = float(shape[0]) * shape[1] * w * 8
        print(json.dumps({"entry": entry, "shape": list(shape), "dim": dim, "window": before + after + 1, "long_ms": round(long_ms, 3),
                          "visits_per_s": float(f"{visits / (long_ms * 1e-3):.3e}"), "of_lds_rate": round(visits / (long_ms * 1e-3) / LDS_KEYS_PER_S, 4),
                          "gather_ms": round(gather_ms, 3), "upload_ms": round(upload_ms, 3), "host_ms_scaled": round(cpu_ms, 1), "sample": part.shape[0],
                          "today_over_long": round((gather_ms + cpu_ms + upload_ms) / long_ms, 1)}), flush=True)
        p.free(h)
        p.free(hy)
    p.close()


if __name__ == "__main__":
    main()
