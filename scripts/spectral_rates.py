"""Developer tool (GPU box): interleaved A/B of uniform_spectral_estimate against fft_dim over an already materialised frame tensor - ms per call, spread, fraction of HBM.
usage: spectral_rates.py parent.so [--samples LOG2] [--rounds N]
Workload: 2^24 real samples, window = nfft = 1024, hop 256, one-sided.  A: the PARENT commit's fft_dim (parent.so: librmhip.so built at the parent
commit, loaded through RMHIP_LIBRARY) over a resident [1024, frames] complex tensor - the transform alone of the four-pass scheme.
B: this build's spectral call on the signal.
Each side runs in a fresh process per round, the rounds alternate, every process warms up before it times (HIP events on the library's stream)."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
CHILD = r'''
import json, os, sys
sys.path.insert(0, %r)
import numpy as np
import runmat_amd._lib as L
side, log2n = sys.argv[1], int(sys.argv[2])
if side == "A":
    L.SIGNATURES.pop("rmhip_spectral_estimate", None)  # absent from the parent build
from runmat_amd import HipProvider
p = HipProvider(0)
N, nfft, hop = 1 << log2n, 1024, 256
frames = (N - nfft) // hop + 1
def timed(fn, reps=20, warm=5):
    for _ in range(warm): fn()
    p.timer_begin()
    for _ in range(reps): fn()
    return p.timer_end() / reps
out = {"frames": frames}
if side == "A":
    re, im = p.fill_uniform(1, -1.0, 1.0, (nfft, frames)), p.fill_uniform(2, -1.0, 1.0, (nfft, frames))
    framed = p.complex_from_real_imag(re, im)
    p.free(re); p.free(im)
    out["fft_dim_ms"] = timed(lambda: p.free(p.fft_dim(framed, None, 0)))
else:
    from runmat_amd import ProviderSpectralFrameMode as M, ProviderSpectralRequest
    x = p.fill_uniform(1, -1.0, 1.0, (N, 1))
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)
    def call(rng):
        r = p.uniform_spectral_estimate(ProviderSpectralRequest(x, N, False, w, nfft, frames, M.Sliding(hop), rng, float(np.sum(w * w))))
        p.free(r.s); p.free(r.ps)
    out["onesided_ms"] = timed(lambda: call(0))
    out["twosided_ms"] = timed(lambda: call(1))
    out["centered_ms"] = timed(lambda: call(2))
    out["path"] = p.telemetry_snapshot()["kernel_launches_log"][-1]["tuning"]
print(json.dumps(out))
''' % ROOT


def main():
    args = sys.argv[1:]
    log2n = int(args[args.index("--samples") + 1]) if "--samples" in args else 24
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 4
    parent = next((a for a in args if a.endswith(".so")), None)
    if not parent or not os.path.isfile(parent):
        sys.exit("spectral_rates.py: give the parent commit's librmhip.so - the baseline is the parent's fft_dim, not this build's\n" + __doc__)
    res = {"A": [], "B": []}
    for _ in range(rounds):
        for side in ("A", "B"):
            env = dict(os.environ)
            if side == "A":
                env["RMHIP_LIBRARY"] = os.path.abspath(parent)
            r = subprocess.run([sys.executable, "-c", CHILD, side, str(log2n)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stderr[-2000:])
            res[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(side, r.stdout.strip().splitlines()[-1], flush=True)
    frames, nfft = res["A"][0]["frames"], 1024
    pts = nfft * frames
    rows = nfft // 2 + 1
    # bytes each side moves through HBM: A reads the framed tensor and writes the full spectrum; B reads the signal once, writes the full
    # spectrum (two-sided: straight into s), and the finish kernel reads the rows it keeps and writes s (unless two-sided) and ps
    sig = 8 * (1 << log2n)
    model = {"fft_dim_ms": 32 * pts, "onesided_ms": sig + 16 * pts + 40 * rows * frames, "twosided_ms": sig + 16 * pts + 24 * pts,
             "centered_ms": sig + 16 * pts + 40 * pts}
    summary = {"samples_log2": log2n, "frames": frames, "parent_library": parent, "path": res["B"][0].get("path")}
    for side in ("A", "B"):
        for k in res[side][0]:
            if not k.endswith("_ms"):
                continue
            xs = sorted(r[k] for r in res[side])
            med = xs[len(xs) // 2]
            summary[k] = {"median": round(med, 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "model_bytes": model[k],
                          "hbm_fraction": round(model[k] / (med * 1e-3) / HBM_BYTES_PER_S, 3)}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
