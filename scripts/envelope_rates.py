"""Developer tool (GPU box): interleaved A/B of signal_envelope's three methods against the parent commit's signal_hilbert on the same shapes - ms per call, spread, fraction of HBM.
usage: envelope_rates.py parent.so [--rounds N] [--taps L]
Shapes: 2^20 x 1, 4096 x 256 and 8192 x 128 (channel_len x channel_count), f64.  A: the PARENT commit's signal_hilbert along dimension 0
(parent.so: librmhip.so built at the parent commit, loaded through RMHIP_LIBRARY) - the transform pair the analytic method is built on.
B: this build's signal_envelope, Analytic, AnalyticFir(L) and Rms(L), L = 129 unless --taps says otherwise.
Each side runs in a fresh process per round, the rounds alternate, every process warms up before it times (HIP events on the library's stream)."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
SHAPES = [(1 << 20, 1), (4096, 256), (8192, 128)]
CHILD = r'''
import json, os, sys
sys.path.insert(0, %r)
import runmat_amd._lib as L
side, taps = sys.argv[1], int(sys.argv[2])
if side == "A":
    L.SIGNATURES.pop("rmhip_signal_envelope", None)  # absent from the parent build
from runmat_amd import HipProvider
p = HipProvider(0)
def timed(fn, reps=20, warm=5):
    for _ in range(warm): fn()
    p.timer_begin()
    for _ in range(reps): fn()
    return p.timer_end() / reps
out = {}
for n, m in %r:
    x = p.fill_uniform(1, -1.0, 1.0, (n, m))
    key = "%%dx%%d" %% (n, m)
    if side == "A":
        out[key + " hilbert_ms"] = timed(lambda: p.free(p.signal_hilbert(x, None, 0)))
    else:
        from runmat_amd import ProviderEnvelopeMethod as M, ProviderEnvelopeRequest
        def call(method):
            r = p.signal_envelope(ProviderEnvelopeRequest(x, n, m, (n, m), method))
            p.free(r.upper); p.free(r.lower)
        out[key + " analytic_ms"] = timed(lambda: call(M.Analytic()))
        out[key + " fir_ms"] = timed(lambda: call(M.AnalyticFir(taps)))
        out[key + " rms_ms"] = timed(lambda: call(M.Rms(taps)))
    p.free(x)
print(json.dumps(out))
''' % (ROOT, SHAPES)


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 4
    taps = int(args[args.index("--taps") + 1]) if "--taps" in args else 129
    parent = next((a for a in args if a.endswith(".so")), None)
    if not parent or not os.path.isfile(parent):
        sys.exit("envelope_rates.py: give the parent commit's librmhip.so - the baseline is the parent's signal_hilbert, not this build's\n" + __doc__)
    res = {"A": [], "B": []}
    for _ in range(rounds):
        for side in ("A", "B"):
            env = dict(os.environ)
            if side == "A":
                env["RMHIP_LIBRARY"] = os.path.abspath(parent)
            r = subprocess.run([sys.executable, "-c", CHILD, side, str(taps)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stderr[-2000:])
            res[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(side, r.stdout.strip().splitlines()[-1], flush=True)
    # bytes per f64 sample each call moves through HBM: hilbert = forward 24 + mask 32 + inverse 32; analytic = stats 8 +
    # centre 16 + that + bounds 32; the direct methods read the signal (stats, then the sum) and write two results
    per_sample = {"hilbert_ms": 88, "analytic_ms": 144, "fir_ms": 32, "rms_ms": 32}
    summary = {"taps": taps, "parent_library": parent}
    for side in ("A", "B"):
        for k in res[side][0]:
            shape, kind = k.split(" ")
            n, m = (int(v) for v in shape.split("x"))
            xs = sorted(r[k] for r in res[side])
            med = xs[len(xs) // 2]
            model = per_sample[kind] * n * m
            summary[k] = {"median": round(med, 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "model_bytes": model,
                          "hbm_fraction": round(model / (med * 1e-3) / HBM_BYTES_PER_S, 3)}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
