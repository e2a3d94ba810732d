"""Developer tool (GPU box): qr_power_iter (CholeskyQR2) against qr economy and the composed syrk + matmul route, interleaved A/B - ms per call, fraction of HBM rate.  Usage: qr_power_iter_bench.py [--quick]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from runmat_amd import HipProvider, ProviderQrOptions

HBM_GBS = 8000.0  # HBM3E spec, as bench.py
PASSES = 5        # k_cq_gram reads P; k_cq_apply reads P and writes Q1; k_cq_apply reads Q1 and writes Q
ECON = ProviderQrOptions(True)

quick = "--quick" in sys.argv
shapes = [(1024, 8), (16384, 32), (1048576, 8), (1048576, 64)] if not quick else [(1024, 8), (16384, 32)]
rounds = 5
prov = HipProvider(0)


def free_all(res):
    for x in (res.q, res.r, res.perm_matrix, res.perm_vector):
        prov.free(x)


for m, k in shapes:
    rng = np.random.default_rng(m + k)
    P = rng.standard_normal((m, k))
    hp, hq = prov.upload(P), prov.upload(np.zeros((m, k)))

    def hook():
        res = prov.qr_power_iter(hp, None, hq, ECON)
        assert res is not None, "declined"
        free_all(res)

    def householder():
        free_all(prov.qr(hp, ECON))

    def composed():
        """Two Cholesky-QR passes from the provider's own ops: syrk, the k x k factor and inverse on the host, matmul."""
        x, r = hp, np.eye(k)
        for _ in range(2):
            hg = prov.syrk(x)  # x' * x
            ri = np.linalg.cholesky(prov.download_matrix(hg)).T
            prov.free(hg)
            hx = prov.upload(np.linalg.inv(ri))
            y = prov.matmul(x, hx)
            prov.free(hx)
            if x is not hp:
                prov.free(x)
            x, r = y, ri @ r
        prov.free(prov.upload(r))
        prov.free(x)

    arms = {"qr_power_iter": hook, "qr_economy": householder, "composed_syrk_matmul": composed}
    reps = {"qr_power_iter": 20 if m * k <= 1 << 22 else 5, "qr_economy": 3 if m * k <= 1 << 22 else 1, "composed_syrk_matmul": 10 if m * k <= 1 << 22 else 3}
    times = {a: [] for a in arms}
    launches = {}
    for a, fn in arms.items():  # warm-up: kernels loaded, pool filled
        t0 = prov.telemetry_snapshot()["kernel_launches"]
        fn()
        launches[a] = prov.telemetry_snapshot()["kernel_launches"] - t0
    prov.synchronize()
    for _ in range(rounds):
        for a, fn in arms.items():
            prov.timer_begin()
            for _ in range(reps[a]):
                fn()
            times[a].append(prov.timer_end() / reps[a])
    rec = {"shape": [m, k]}
    for a in arms:
        t = sorted(times[a])
        rec[a] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "launches": launches[a]}
    med = rec["qr_power_iter"]["median_ms"]
    rec["qr_power_iter"]["hbm_fraction"] = round(PASSES * 8.0 * m * k / (med * 1e-3) / (HBM_GBS * 1e9), 4)
    rec["speedup_over_qr_economy"] = round(rec["qr_economy"]["median_ms"] / med, 2)
    rec["speedup_over_composed"] = round(rec["composed_syrk_matmul"]["median_ms"] / med, 2)
    prov.free(hp)
    prov.free(hq)
    print(json.dumps(rec), flush=True)
prov.close()
