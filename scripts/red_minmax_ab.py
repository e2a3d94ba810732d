"""Developer tool: interleaved A/B of two librmhip builds (RMHIP_LIBRARY) on reduce_min / reduce_max of an 8192 x 8192 f64 tensor -
all elements and along each dim - the HBM-bound kernels whose combine step carries the -0 < +0 order (skel_reduce.h rm_combine) and
which bench.py does not time.  Prints per case the median of each build over the rounds, and the old build's own run-to-run spread
(max - min over its rounds): the new build may be slower by no more than that.
usage: red_minmax_ab.py <old.so> <new.so> [rounds]      (scripts/build_rev.sh builds <old.so> from a revision)"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, sys
sys.path.insert(0, %r)
from runmat_amd import HipProvider
p = HipProvider(0)
N = 8192
a = p.fill_uniform(1, -3.0, 3.0, (N, N))
def timed(fn, reps=40, warm=8):
    for _ in range(warm): fn()
    p.timer_begin()
    for _ in range(reps): fn()
    return p.timer_end() / reps
f = lambda h: p.free(h)
out = {}
for op in ("min", "max"):
    for name, dim in (("all", -1), ("dim0", 0), ("dim1", 1)):
        out[op + "_" + name] = timed(lambda: f(p._reduce(op, a, dim)))
print(json.dumps(out))
p.close()
''' % ROOT
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
res = {"old": [], "new": []}
for rnd in range(rounds):
    for tag, lib in (("old", sys.argv[1]), ("new", sys.argv[2])):
        r = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, RMHIP_LIBRARY=os.path.abspath(lib)),
                           capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            sys.exit(r.stderr[-2000:])
        res[tag].append(json.loads(r.stdout.strip().splitlines()[-1]))
med = lambda xs: sorted(xs)[len(xs) // 2]
for k in res["old"][0]:
    old, new = [r[k] * 1e3 for r in res["old"]], [r[k] * 1e3 for r in res["new"]]
    print(f"{k:9s} old {med(old):7.1f} us (spread {max(old) - min(old):5.1f})   new {med(new):7.1f} us (spread {max(new) - min(new):5.1f})   "
          f"new - old {med(new) - med(old):+6.1f}")
