"""Developer tool (GPU box): device eig (symmetric) against numpy.linalg.eigh and rmhip_cond (2-norm, the scalar Jacobi tournament) - ms per call, launches, sweeps.  Usage: eig_rates.py [--large] [--quick]
(eig and cond calls alternate inside one timed loop, after a warm-up of each; every call ends in a device synchronise; --large adds n = 4096;
cond's path, svdsolve.hip, is the one-launch-per-step tournament this change leaves as it was)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from runmat_amd import HipProvider

EIG_BLOCK, EIG_SMALL = 32, 64  # eig.hip kEigBlock / kEigSmall


def timed(prov, fn):
    prov.synchronize()
    t = time.perf_counter()
    fn()
    prov.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    sizes = [8, 64, 256, 1024] if "--quick" in sys.argv else [8, 64, 256, 512, 1024, 2048]
    if "--large" in sys.argv:
        sizes.append(4096)
    prov = HipProvider(0)
    for n in sizes:
        R = np.random.default_rng(n).uniform(-1.0, 1.0, (n, n))
        A = 0.5 * (R + R.T)
        h = prov.upload(A)

        def eig_once():
            r = prov.eig(h)
            for x in (r.eigenvalues, r.diagonal, r.right):
                prov.free(x)

        def cond_once():
            prov.free(prov.cond(h, "two"))

        reps = 7 if n <= 512 else 3 if n <= 1024 else 2 if n <= 2048 else 1
        eig_once()
        cond_once()
        l0 = prov.telemetry_snapshot()["kernel_launches"]
        eig_once()
        launches = prov.telemetry_snapshot()["kernel_launches"] - l0
        te, tc = [], []
        for _ in range(reps):  # alternate: both see the same clocks and the same neighbours on the host
            te.append(timed(prov, eig_once))
            tc.append(timed(prov, cond_once))
        t = time.perf_counter()
        w = np.linalg.eigh(A)[0]
        host_ms = (time.perf_counter() - t) * 1e3
        r = prov.eig(h)
        lam = prov.download(r.eigenvalues)
        for x in (h, r.eigenvalues, r.diagonal, r.right):
            prov.free(x)
        rec = {"n": n, "eig_ms": round(statistics.median(te), 3), "eig_ms_range": [round(min(te), 3), round(max(te), 3)],
               "cond2_ms": round(statistics.median(tc), 3), "cond2_ms_range": [round(min(tc), 3), round(max(tc), 3)],
               "numpy_eigh_ms": round(host_ms, 3), "launches": launches, "reps": reps,
               "eigenvalue_error_over_norm": float(np.max(np.abs(lam - w)) / np.max(np.abs(w)))}
        if n > EIG_SMALL:
            blocks = -(-n // EIG_BLOCK)
            per_sweep = 3 * (((blocks + 1) & ~1) - 1)  # gram, rot, apply per tournament step
            rec["launches_per_sweep"] = per_sweep
            rec["sweeps"] = (launches - 7) // per_sweep  # check, colsum, prep, dgemm, rayleigh, rank, emit around the sweeps
            rec["cond2_launches_per_sweep"] = ((n + 1) & ~1) - 1
        print(json.dumps(rec), flush=True)
    prov.close()


if __name__ == "__main__":
    main()
