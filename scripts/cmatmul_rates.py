"""Developer tool (GPU box): rmhip_complex_matmul beside rmhip_matmul on the real product it embeds, interleaved in one process - ms per call (median and min over rounds), the difference, and what the two streaming passes would cost at the HBM rate.  Usage: cmatmul_rates.py [--quick]

A complex x complex product of side s runs the real product 2s x 2s x s between a split of B (reads 16 s^2 bytes, writes 16 s^2) and a
join (reads 32 s^2, writes 16 s^2); complex x real runs 2s x s x s straight into the result.  rmhip_matmul routes the real product as
it does on any commit that leaves plan_dgemm alone, so the `real` column is the yardstick the embedding is read against.  Rounds
alternate the two calls; each timed window is `reps` calls between device timers, after one warm call of each."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from runmat_amd import HipProvider

HBM = 8.0e12
MFMA = 78.6e12
ROUNDS = 7

# (kind, m, n, k): 0 complex x complex, 1 complex x real
CASES = [(0, 1024, 1024, 1024), (0, 4096, 4096, 4096), (1, 4096, 4096, 4096)]
if "--quick" in sys.argv:
    CASES = [(0, 256, 256, 256), (1, 256, 256, 256)]


def operand(prov, shape, cplx):
    hr = prov.random_uniform(shape)
    if not cplx:
        return hr
    hi = prov.random_uniform(shape)
    z = prov.complex_from_real_imag(hr, hi)
    prov.free(hr)
    prov.free(hi)
    return z


def window_ms(prov, fn, reps):
    prov.synchronize()
    prov.timer_begin()
    for _ in range(reps):
        fn()
    return prov.timer_end() / reps


prov = HipProvider(0)
for kind, m, n, k in CASES:
    M, N = 2 * m, (n if kind == 1 else 2 * n)
    za, zb = operand(prov, [m, k], True), operand(prov, [k, n], kind == 0)
    ra, rb = operand(prov, [M, k], False), operand(prov, [k, N], False)
    cplx = lambda: prov.free(prov.complex_matmul(za, zb))
    real = lambda: prov.free(prov.matmul(ra, rb))
    reps = 3 if m >= 4096 else 20
    t0 = prov.telemetry_snapshot()["kernel_launches"]
    cplx()
    launches = prov.telemetry_snapshot()["kernel_launches"] - t0
    embedded = prov.gemm_last_route()
    real()
    plain = prov.gemm_last_route()
    c_ms, r_ms = [], []
    for _ in range(ROUNDS):
        c_ms.append(window_ms(prov, cplx, reps))
        r_ms.append(window_ms(prov, real, reps))
    stream_bytes = (32.0 * k * n + 48.0 * m * n) if kind == 0 else 0.0
    flops = 2.0 * M * N * k
    cm, rm = statistics.median(c_ms), statistics.median(r_ms)
    print(json.dumps({
        "kind": kind, "m": m, "n": n, "k": k, "embedded": [M, N, k], "launches": launches,
        "embedded_kernel": embedded["kernel"], "real_kernel": plain["kernel"], "splits": embedded["splits"],
        "complex_ms": {"median": round(cm, 4), "min": round(min(c_ms), 4), "rounds": [round(x, 4) for x in c_ms]},
        "real_ms": {"median": round(rm, 4), "min": round(min(r_ms), 4), "rounds": [round(x, 4) for x in r_ms]},
        "x_real": round(cm / rm, 3), "extra_ms": round(cm - rm, 4),
        "stream_MB": round(stream_bytes / 1e6, 1), "stream_ms_at_hbm": round(stream_bytes / HBM * 1e3, 4),
        "stream_TBs_if_extra_is_streaming": round(stream_bytes / (cm - rm) / 1e9, 3) if stream_bytes and cm > rm else None,
        "real_TFLOPs": round(flops / rm / 1e9, 2), "complex_TFLOPs_of_embedded": round(flops / cm / 1e9, 2),
        "real_mfma_frac": round(flops / MFMA * 1e3 / rm, 3),
    }), flush=True)
    for h in (za, zb, ra, rb):
        prov.free(h)
prov.close()
