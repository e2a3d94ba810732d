"""Developer tool (GPU box): rmhip_complex_mldivide beside rmhip_mldivide on the embedded real system it solves, interleaved in one process - ms per call (median and min over rounds), the ratio, and what the embed / stack / join passes would cost at the HBM rate.  Usage: complex_solve_times.py [--quick]

A complex solve of order n with k right-hand sides writes E(A) = [Ar -Ai; Ai Ar] (reads 16 n^2 bytes, writes 32 n^2), stacks b, runs the
real solve of order 2n and joins the solution.  The real call solves the same E(A), built on the device beforehand with cat, against the
same stacked right-hand side: that is what the library could already do, so the `real` column is the yardstick the embedding is read
against and the table a later native complex LU is measured by (at most 2x faster, half the memory).  Parts are N(0, 1) or U(-1, 1);
`growth_fallbacks` counts the factorisations the solve path's multiplier check sent back to the grid-wide pivot rule (the real solve's
own routing, the same for both calls).  Rounds alternate the two calls; each timed window is `reps` calls between device timers, after
one warm call of each; `mrdivide_ms` is b.' / A on the same operands, after them."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from runmat_amd import HipProvider

HBM = 8.0e12
ROUNDS = 5

CASES = [(1024, 1, "normal"), (4096, 1, "normal"), (8192, 1, "normal"), (4096, 1, "uniform"), (8192, 1, "uniform")]  # (n, k, parts)
if "--quick" in sys.argv:
    CASES = [(128, 1, "normal"), (512, 1, "uniform")]


def part(prov, shape, dist):
    if dist == "normal":
        return prov.random_normal(shape)
    u = prov.random_uniform(shape)
    u2 = prov.scalar_mul(u, 2.0)
    out = prov.scalar_sub(u2, 1.0)
    prov.free(u)
    prov.free(u2)
    return out


def window_ms(prov, fn, reps):
    prov.synchronize()
    prov.timer_begin()
    for _ in range(reps):
        fn()
    return prov.timer_end() / reps


prov = HipProvider(0)
for n, k, dist in CASES:
    ar, ai = part(prov, [n, n], dist), part(prov, [n, n], dist)
    br, bi = part(prov, [n, k], dist), part(prov, [n, k], dist)
    za, zb = prov.complex_from_real_imag(ar, ai), prov.complex_from_real_imag(br, bi)
    nai = prov.scalar_mul(ai, -1.0)
    left, right = prov.cat(1, [ar, ai]), prov.cat(1, [nai, ar])
    ea, eb = prov.cat(2, [left, right]), prov.cat(1, [br, bi])
    for h in (ar, ai, br, bi, nai, left, right):
        prov.free(h)
    cplx = lambda: prov.free(prov.complex_mldivide(za, zb))
    real = lambda: prov.free(prov.mldivide(ea, eb))
    reps = 2 if n >= 4096 else 10
    t0, s0 = prov.telemetry_snapshot()["kernel_launches"], prov.lu_stats()
    cplx()
    t1, s1 = prov.telemetry_snapshot()["kernel_launches"], prov.lu_stats()
    real()
    t2, s2 = prov.telemetry_snapshot()["kernel_launches"], prov.lu_stats()
    c_ms, r_ms = [], []
    for _ in range(ROUNDS):
        c_ms.append(window_ms(prov, cplx, reps))
        r_ms.append(window_ms(prov, real, reps))
    # b.' / A: the same solve on E(A.'), whose embed pass reads A with a stride (csolve.hip) - timed beside the calls above
    zbt = prov.complex_transpose(zb)
    right_div = lambda: prov.free(prov.complex_mrdivide(zbt, za))
    right_div()
    d_ms = []
    for _ in range(ROUNDS):
        d_ms.append(window_ms(prov, right_div, reps))
    prov.free(zbt)
    stream_bytes = 48.0 * n * n + 64.0 * n * k  # embed 16 + 32 n^2; stack and join 32 n k each
    cm, rm = statistics.median(c_ms), statistics.median(r_ms)
    print(json.dumps({
        "n": n, "k": k, "parts": dist, "embedded": [2 * n, 2 * n, k], "launches": {"complex": t1 - t0, "real": t2 - t1},
        "growth_fallbacks": {"complex": s1["pivot_growth_fallbacks"] - s0["pivot_growth_fallbacks"],
                             "real": s2["pivot_growth_fallbacks"] - s1["pivot_growth_fallbacks"]},
        "last_max_multiplier": s2["last_max_multiplier"],
        "conservative_panels": s2["conservative_panels"], "one_xcd_panels": s2["one_xcd_panels"],
        "complex_ms": {"median": round(cm, 4), "min": round(min(c_ms), 4), "rounds": [round(x, 4) for x in c_ms]},
        "real_ms": {"median": round(rm, 4), "min": round(min(r_ms), 4), "rounds": [round(x, 4) for x in r_ms]},
        "mrdivide_ms": {"median": round(statistics.median(d_ms), 4), "min": round(min(d_ms), 4), "rounds": [round(x, 4) for x in d_ms]},
        "x_real": round(cm / rm, 3), "extra_ms": round(cm - rm, 4),
        "stream_MB": round(stream_bytes / 1e6, 1), "stream_ms_at_hbm": round(stream_bytes / HBM * 1e3, 4),
        "stream_TBs_if_extra_is_streaming": round(stream_bytes / (cm - rm) / 1e9, 3) if cm > rm else None,
    }), flush=True)
    for h in (za, zb, ea, eb):
        prov.free(h)
prov.close()
