"""Developer tool (GPU box): ms per call of iir_filter_long on one long channel against what the caller does for that shape today - gather, host loop, upload.
usage: iir_long_rates.py [--limit SECONDS]
10^6 and 10^7 samples x 1 channel, f64, orders 2, 8 and 32 (order - 1 poles of radius 0.9: conjugate pairs at evenly spaced angles, a real one when the count is odd; a random numerator).  Per case, each timed once
after one warm-up call, a device synchronise (a one-element download) inside the timed span:
  long_ms      rmhip_iir_filter_long, and the fraction of HBM bandwidth its 16 bytes per sample (one read, one write) come to
  gather_ms    rmhip_download of the signal           upload_ms   rmhip_upload of the result
  host_ms      the oracle's loop (oracle.iir_filter, interpreted Python) on the first PREFIX samples, scaled to the length - a scaled figure, not a
               measurement of the whole run, and of the Python loop, not of the reference's compiled one; skipped once --limit (default 120 s) is spent
One JSON line per case, then the table."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import oracle  # noqa: E402
from runmat_amd.provider import HipProvider  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
PREFIX = 20000


def main():
    args = sys.argv[1:]
    limit = float(args[args.index("--limit") + 1]) if "--limit" in args else 120.0
    began = time.perf_counter()
    p = HipProvider(0)
    sync = p.upload(np.zeros((1, 1)))

    def timed(fn):
        p.download(sync)
        t = time.perf_counter()
        out = fn()
        p.download(sync)
        return (time.perf_counter() - t) * 1e3, out

    rows = []
    for n in (10 ** 6, 10 ** 7):
        x = np.random.default_rng(n).standard_normal(n)
        hx = p.upload(x.reshape(n, 1))
        for order in (2, 8, 32):
            rng = np.random.default_rng(order)
            theta = np.pi * (np.arange((order - 1) // 2) + 1.0) / ((order - 1) // 2 + 1.0)
            poles = list(0.9 * np.exp(1j * theta)) + list(0.9 * np.exp(-1j * theta)) + ([0.9] if (order - 1) % 2 else [])
            b, a = rng.standard_normal(order), np.real(np.poly(poles))
            hb, ha = p.upload(b.reshape(1, -1)), p.upload(a.reshape(1, -1))
            for h in p.iir_filter_long(hb, ha, hx, 0):  # warm-up: code objects, pool
                p.free(h)
            long_ms, (y, zf) = timed(lambda: p.iir_filter_long(hb, ha, hx, 0))
            gather_ms, host = timed(lambda: p.download(hx))
            upload_ms, hy = timed(lambda: p.upload(host.reshape(n, 1)))
            host_ms = None
            if time.perf_counter() - began < limit:
                t = time.perf_counter()
                oracle.iir_filter(b, a, x[:PREFIX], 0)
                host_ms = (time.perf_counter() - t) * 1e3 * n / PREFIX
            row = {"samples": n, "order": order, "long_ms": round(long_ms, 3), "hbm_fraction": round(16.0 * n / (long_ms * 1e-3) / HBM_BYTES_PER_S, 4),
                   "gather_ms": round(gather_ms, 3), "upload_ms": round(upload_ms, 3), "host_loop_ms_scaled": None if host_ms is None else round(host_ms, 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in (y, zf, hy, hb, ha):
                p.free(h)
        p.free(hx)
    print(f"{'samples':>9s} {'order':>5s} {'long ms':>9s} {'of HBM':>7s} {'gather ms':>10s} {'upload ms':>10s} {'host loop ms (scaled)':>22s}")
    for r in rows:
        print(f"{r['samples']:9d} {r['order']:5d} {r['long_ms']:9.3f} {r['hbm_fraction']:7.4f} {r['gather_ms']:10.3f} {r['upload_ms']:10.3f} {str(r['host_loop_ms_scaled']):>22s}")
    p.close()


if __name__ == "__main__":
    main()
