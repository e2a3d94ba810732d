"""Developer tool (GPU box): black_scholes_price, adam_update and crossentropy_terms at 2^26 f64 elements against the same computation composed from the elem_* / unary_* / scalar_* hooks, with the fused sin_mul_add kernel as the HBM yardstick.  Usage: workload_hooks_bench.py [--log2n K] [--reps R] [--out FILE]

Every round times, in this order, each hook, its composed baseline (what a caller had before the hooks existed: one launch and one
temporary per operation, none of the validity checks) and the yardstick, with device events around each call (a validated call also
includes its one stream synchronisation); the figure reported is the median over the rounds.  Algorithmic bytes per element (f64):
adam_update 56 (four operands in, three results out), crossentropy_terms 40 (multi-label, weights and mask), black_scholes_price 64
(six operands in, two results out), sin_mul_add 32.  The share is the hook's algorithmic bytes/s over the yardstick's."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from planner_requests import sin_mul_add_plan
from runmat_amd import HipProvider

SQRT_2 = 1.4142135623730951


class Temps:
    """Frees every intermediate of a composed expression except the handles it is told to keep."""

    def __init__(self, prov):
        self.prov, self.made = prov, []

    def __call__(self, h):
        self.made.append(h)
        return h

    def release(self, keep=()):
        for h in self.made:
            if all(h is not k for k in keep):
                self.prov.free(h)
        self.made = []


def composed_adam(prov, p0, g, m0, v0, lr, b1, b2, eps, gc, sc):
    t = Temps(prov)
    m = t(prov.elem_add(t(prov.scalar_mul(m0, b1)), t(prov.scalar_mul(g, 1.0 - b1))))
    v = t(prov.elem_add(t(prov.scalar_mul(v0, b2)), t(prov.elem_mul(t(prov.scalar_mul(g, 1.0 - b2)), g))))
    num = t(prov.scalar_mul(t(prov.scalar_div(m, gc)), lr))
    den = t(prov.scalar_add(t(prov.unary_sqrt(t(prov.scalar_div(v, sc)))), eps))
    p = t(prov.elem_sub(p0, t(prov.elem_div(num, den))))
    t.release(keep=(p, m, v))
    return p, m, v


def composed_crossentropy(prov, pred, target, weights, mask):
    t = Temps(prov)
    c = t(prov.scalar_min(t(prov.scalar_max(pred, 1.0e-12)), 1.0 - 1.0e-12))
    first = t(prov.elem_mul(t(prov.unary_neg(target)), t(prov.unary_log(c))))
    second = t(prov.elem_mul(t(prov.scalar_rsub(target, 1.0)), t(prov.unary_log(t(prov.scalar_rsub(c, 1.0))))))
    loss = t(prov.elem_mul(t(prov.elem_mul(t(prov.elem_sub(first, second)), weights)), mask))
    t.release(keep=(loss,))
    return (loss,)


def composed_black_scholes(prov, S, K, r, T, sig, q):
    t = Temps(prov)
    dp = t(prov.elem_mul(S, t(prov.unary_exp(t(prov.elem_mul(t(prov.unary_neg(q)), T))))))
    ds = t(prov.elem_mul(K, t(prov.unary_exp(t(prov.elem_mul(t(prov.unary_neg(r)), T))))))
    vs = t(prov.elem_mul(sig, t(prov.unary_sqrt(T))))
    drift = t(prov.elem_add(t(prov.elem_sub(r, q)), t(prov.elem_mul(t(prov.scalar_mul(sig, 0.5)), sig))))
    d1 = t(prov.elem_div(t(prov.elem_add(t(prov.unary_log(t(prov.elem_div(S, K)))), t(prov.elem_mul(drift, T)))), vs))
    d2 = t(prov.elem_sub(d1, vs))
    e1 = t(prov.unary_erf(t(prov.scalar_div(d1, SQRT_2))))
    e2 = t(prov.unary_erf(t(prov.scalar_div(d2, SQRT_2))))
    n1, n2 = t(prov.scalar_mul(t(prov.scalar_add(e1, 1.0)), 0.5)), t(prov.scalar_mul(t(prov.scalar_add(e2, 1.0)), 0.5))
    m1, m2 = t(prov.scalar_mul(t(prov.scalar_rsub(e1, 1.0)), 0.5)), t(prov.scalar_mul(t(prov.scalar_rsub(e2, 1.0)), 0.5))
    call = t(prov.elem_sub(t(prov.elem_mul(dp, n1)), t(prov.elem_mul(ds, n2))))
    put = t(prov.elem_sub(t(prov.elem_mul(ds, m2)), t(prov.elem_mul(dp, m1))))
    t.release(keep=(call, put))
    return call, put


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 1 << args.log2n
    prov = HipProvider(0)
    shape = (n, 1)
    u = lambda seed, lo, hi: prov.fill_uniform(seed, lo, hi, shape)  # noqa: E731
    p0, g, m0, v0 = u(1, -1, 1), u(2, -1, 1), u(3, -0.1, 0.1), u(4, 0, 1)
    pred, target, weights, mask = u(5, 0, 1), u(6, 0, 1), u(7, 0, 3), prov.fill(shape, 1.0)
    S, K, r, T, sig, q = u(8, 50, 150), u(9, 50, 150), u(10, 0, 0.1), u(11, 0.05, 3), u(12, 0.05, 0.8), u(13, 0, 0.05)
    plan, out_id = sin_mul_add_plan()
    shader = plan.generate_wgsl_for_output(out_id, "f64")
    lr, b1, b2, eps, it = 0.01, 0.9, 0.999, 1e-8, 10
    gc, sc = 1.0 - b1 ** it, 1.0 - b2 ** it

    arms = {
        "adam_update": (56, lambda: prov.adam_update(p0, g, m0, v0, iteration=it, learn_rate=lr, gradient_decay_factor=b1,
                                                     squared_gradient_decay_factor=b2, epsilon=eps)),
        "adam_update composed": (None, lambda: composed_adam(prov, p0, g, m0, v0, lr, b1, b2, eps, gc, sc)),
        "crossentropy_terms": (40, lambda: (prov.crossentropy_terms(pred, target, weights, mask, mode="multi-label"),)),
        "crossentropy_terms composed": (None, lambda: composed_crossentropy(prov, pred, target, weights, mask)),
        "black_scholes_price": (64, lambda: prov.black_scholes_price([S, K, r, T, sig, q])),
        "black_scholes_price composed": (None, lambda: composed_black_scholes(prov, S, K, r, T, sig, q)),
        "sin_mul_add fused": (32, lambda: (prov.fused_elementwise(shader, [p0, g, m0], shape, n),)),
    }

    def once(fn):
        prov.timer_begin()
        outs = fn()
        ms = prov.timer_end()
        for h in outs:
            prov.free(h)
        return ms

    for _, fn in arms.values():  # warm every arm: code objects, the pool's buckets
        once(fn)
        once(fn)
    times = {name: [] for name in arms}
    for _ in range(args.reps):
        for name, (_, fn) in arms.items():
            times[name].append(once(fn))
    rows = {}
    for name, (bpe, _) in arms.items():
        ms = statistics.median(times[name])
        rows[name] = {"ms": ms, "min_ms": min(times[name]), "max_ms": max(times[name])}
        if bpe:
            rows[name]["bytes_per_element"] = bpe
            rows[name]["algorithmic_GBps"] = bpe * n / ms / 1e6
    yard = rows["sin_mul_add fused"]["algorithmic_GBps"]
    for name in ("adam_update", "crossentropy_terms", "black_scholes_price"):
        rows[name]["share_of_yardstick"] = rows[name]["algorithmic_GBps"] / yard
        rows[name]["speedup_over_composed"] = rows[name + " composed"]["ms"] / rows[name]["ms"]
    doc = {"elements": n, "dtype": "f64", "reps": args.reps, "device": prov.device_info(), "rows": rows}
    for name, r in rows.items():
        print(f"{name:32s} {r['ms']:9.3f} ms (min {r['min_ms']:.3f}, max {r['max_ms']:.3f})"
              + (f"  {r['algorithmic_GBps']:8.0f} GB/s" if "algorithmic_GBps" in r else "")
              + (f"  {r['share_of_yardstick']:.2f} of yardstick, {r['speedup_over_composed']:.1f}x composed" if "share_of_yardstick" in r else ""),
              flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    prov.close()


if __name__ == "__main__":
    main()
