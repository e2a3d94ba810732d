"""Developer tool (GPU box): ms per call of cond_norm (cond's second entry point: one, inf, fro) beside inv at n = 512, 2048 and 8192.
usage: cond_norm_rates.py [--sizes 512,2048,8192] [--rounds N] [--warm N]
The operand is U(-1, 1) + n I (seed n).  Every round times each configuration once, in turn (device events on the library's stream around
one call, the result freed inside the window), after --warm (2) untimed rounds; the figures are the median and the extremes over --rounds
(7).  The calls hold their read-backs, so this is the call's time on the stream, not a sum of kernel times.  One JSON line per
configuration, headed by the slab width the loaded library was built with (RMHIP_LIBRARY selects another build for a comparison)."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    args = sys.argv[1:]
    sizes = [int(s) for s in (args[args.index("--sizes") + 1] if "--sizes" in args else "512,2048,8192").split(",")]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 7
    warm = int(args[args.index("--warm") + 1]) if "--warm" in args else 2
    from runmat_amd import HipProvider

    src = open(os.path.join(ROOT, "runmat_amd", "csrc", "cond_norm.hip")).read()
    print(json.dumps({"library": os.environ.get("RMHIP_LIBRARY", "in-tree"),
                      "kCondSlabCols_in_source": int(re.search(r"kCondSlabCols = (\d+);", src).group(1))}), flush=True)
    p = HipProvider(0)
    for n in sizes:
        a = np.random.default_rng(n).uniform(-1.0, 1.0, (n, n)) + n * np.eye(n)
        h = p.upload(a)
        configs = [("cond_one", lambda: p.cond_norm(h, "one")), ("cond_inf", lambda: p.cond_norm(h, "inf")),
                   ("cond_fro", lambda: p.cond_norm(h, "fro")), ("inv", lambda: p.inv(h))]
        times = {name: [] for name, _ in configs}
        value = {}
        for r in range(warm + rounds):
            for name, fn in configs:
                p.timer_begin()
                out = fn()
                if name != "inv" and r < warm:  # the value once, outside the timed rounds
                    value[name] = float(p.download(out)[0])
                p.free(out)
                ms = p.timer_end()
                if r >= warm:
                    times[name].append(ms)
        for name, _ in configs:
            t = np.array(times[name])
            print(json.dumps({"config": name, "n": n, "rounds": rounds, "median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3),
                              "max_ms": round(float(t.max()), 3), "value": value.get(name)}), flush=True)
        p.free(h)
    p.close()


if __name__ == "__main__":
    main()
