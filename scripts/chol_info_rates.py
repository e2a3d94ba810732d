"""Developer tool (GPU box): ms per call of chol_info (chol's second entry point) beside chol at n = 4096 - a failed pivot late and early, and the positive definite parent.
usage: chol_info_rates.py [--n N] [--rounds N] [--warm N]      on the GPU
       chol_info_rates.py --host [--n N]                        on a CPU: the oracle's time for the failing matrix (what the caller paid)
The parent is b b' + n I (seed 1), exactly symmetric; a failed pivot at column j is the parent with a_jj = -1.  Configurations:
  chol / chol_lower            rmhip_chol on the parent (it declines the other two)
  info / info_lower            rmhip_chol_info on the parent
  info_P4000, info_P100        rmhip_chol_info on a failed pivot at column 4000 and at column 100 (scaled with --n)
Every round times each configuration once, in turn (device events on the library's stream around one call, the result freed inside the
window), after --warm (3) untimed rounds; the figures are the median and the extremes over --rounds (15).  The call holds its one
read-back, so this is the call's time on the stream, not a sum of kernel times.  One JSON line per configuration."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def matrices(n):
    b = np.random.default_rng(1).standard_normal((n, n))
    a = b @ b.T + n * np.eye(n)
    a = 0.5 * (a + a.T)
    late, early = a.copy(), a.copy()
    j_late, j_early = (n * 4000) // 4096, (n * 100) // 4096
    late[j_late, j_late] = -1.0
    early[j_early, j_early] = -1.0
    return a, late, j_late, early, j_early


def main():
    args = sys.argv[1:]
    n = int(args[args.index("--n") + 1]) if "--n" in args else 4096
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 15
    warm = int(args[args.index("--warm") + 1]) if "--warm" in args else 3
    a, late, j_late, early, j_early = matrices(n)
    if "--host" in args:
        from oracle import oracle

        for name, m, j in ((f"P{j_late}", late, j_late), (f"P{j_early}", early, j_early)):
            t = time.perf_counter()
            info = oracle.chol(m)[1]
            print(json.dumps({"config": f"oracle_{name}", "n": n, "info": info, "host_ms": round((time.perf_counter() - t) * 1e3, 1)}), flush=True)
            assert info == j + 1
        return
    from runmat_amd import HipProvider

    p = HipProvider(0)
    ha, hl, he = p.upload(a), p.upload(late), p.upload(early)
    configs = [("chol", p.chol, ha, False, 0), ("info", p.chol_info, ha, False, 0), ("chol_lower", p.chol, ha, True, 0),
               ("info_lower", p.chol_info, ha, True, 0), (f"info_P{j_late}", p.chol_info, hl, False, j_late + 1),
               (f"info_P{j_early}", p.chol_info, he, False, j_early + 1)]
    times = {name: [] for name, *_ in configs}
    for r in range(warm + rounds):
        for name, fn, h, lower, want_info in configs:
            p.timer_begin()
            res = fn(h, lower)
            p.free(res.factor)
            ms = p.timer_end()
            assert res.info == want_info, (name, res.info)
            if r >= warm:
                times[name].append(ms)
    for name, *_ in configs:
        t = np.array(times[name])
        print(json.dumps({"config": name, "n": n, "rounds": rounds, "median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3),
                          "max_ms": round(float(t.max()), 3)}), flush=True)
    p.close()


if __name__ == "__main__":
    main()
