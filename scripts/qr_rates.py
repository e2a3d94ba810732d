"""Developer tool (GPU box): device qr (column-pivoted, the builtin's contract) against scipy's pivoted QR and torch.linalg.qr - ms per call.  Usage: qr_rates.py [--quick] [--torch]
(--torch adds the vendor yardstick; leave it out under a kernel tracer)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from runmat_amd import HipProvider, ProviderQrOptions


def torch_yardstick(A, econ, reps, rec):
    """torch.linalg.qr (unpivoted, vendor) on the same matrix: a ceiling, not a contract peer"""
    try:
        import torch

        ta = torch.from_numpy(A).to("cuda")
        mode = "reduced" if econ else "complete"
        torch.linalg.qr(ta, mode=mode)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            torch.linalg.qr(ta, mode=mode)
        torch.cuda.synchronize()
        rec["torch_unpivoted_ms"] = round((time.perf_counter() - t) * 1e3 / reps, 3)
    except Exception as e:  # no torch / no device: the yardstick is optional
        rec["torch_error"] = str(e)[:80]


quick = "--quick" in sys.argv
shapes = [(100000, 64, True), (1000, 37, True), (2048, 2048, True), (4096, 4096, True)] if not quick else [(100000, 64, True), (2048, 2048, True)]
prov = HipProvider(0)
for m, n, econ in shapes:
    A = np.random.default_rng(m + n).standard_normal((m, n))
    h = prov.upload(A)
    opts = ProviderQrOptions(econ)

    def once():
        r = prov.qr(h, opts)
        for x in (r.q, r.r, r.perm_matrix, r.perm_vector):
            prov.free(x)

    once()
    prov.synchronize()
    reps = 3
    t0 = prov.telemetry_snapshot()["kernel_launches"]
    prov.timer_begin()
    for _ in range(reps):
        once()
    dev_ms = prov.timer_end() / reps
    launches = (prov.telemetry_snapshot()["kernel_launches"] - t0) // reps
    rec = {"shape": [m, n], "economy": econ, "rmhip_ms": round(dev_ms, 3), "launches": launches}
    try:
        import scipy.linalg

        t = time.perf_counter()
        scipy.linalg.qr(A, pivoting=True, mode="economic" if econ else "full")
        rec["scipy_pivoted_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    except ImportError:
        pass
    if "--torch" in sys.argv:
        torch_yardstick(A, econ, reps, rec)
    prov.free(h)
    print(json.dumps(rec), flush=True)
prov.close()
