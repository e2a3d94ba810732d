"""GPU parity of uniform_spectral_estimate (include/rmhip.h, fft.hip) against the numpy restatement in tests/spectral_ref.py.

Tolerance, derived rather than tuned.  With S the exact spectrum of the frame the restatement forms,
    |s - S| <= delta = C * eps * max(1, log2(work)) * ||frame||_2,
C = 4 and work = nfft for a power of two, C = 8 and work = the padded convolution length otherwise (the bound tests/test_gpu_fft.py
states for the transforms).  A folded frame (mode 2) is a sum of K = ceil(window_len / nfft) products per point whose order of rounding
is the device's own: delta grows by eps * K * sum |x w| over the frame's terms.  The power follows from |s|^2 - |S|^2:
    |ps - PS| <= scale / denominator * (2 |S| delta + delta^2) + 4 * eps * PS.
numpy's FFT stands in for S (it sits at 0.05 - 0.18 of delta against a long-double DFT on these shapes).  On a precision-32 provider the
expectation is formed from the f32-rounded input and each bound grows by one f32 ulp of the value."""
import math
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import spectral_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(n) + 0.5) / n) if n > 1 else np.ones(1)


def case(name, mode, numel, window_len, nfft, frames, hop=0, input_rows=0, fpc=0, input_len=None, path=None):
    return dict(name=name, mode=mode, numel=numel, window_len=window_len, nfft=nfft, frames=frames, hop=hop, input_rows=input_rows, fpc=fpc,
                input_len=numel if input_len is None else input_len, path=path)


S, CS, FC = ref.SLIDING, ref.COLUMN_SLIDING, ref.FOLDED_COLUMNS
CASES = [
    case("sliding-64-hop16", S, 1000, 64, 64, 59, hop=16, path="fused"),            # 59 frames: no multiple of a tile's line count
    case("sliding-zero-pad", S, 500, 48, 64, 10, hop=48, path="fused"),
    case("sliding-truncate", S, 500, 80, 64, 27, hop=16, path="fused"),
    case("sliding-nfft8-500-frames", S, 507, 8, 8, 500, hop=1, path="fused"),         # many short lines per workgroup
    case("sliding-nfft2", S, 33, 2, 2, 32, hop=1, path="fused"),
    case("sliding-nfft1", S, 17, 1, 1, 17, hop=1, path="framed"),
    case("sliding-window1", S, 50, 1, 16, 17, hop=3, path="fused"),
    case("sliding-bluestein-100", S, 600, 100, 100, 14, hop=37, path="framed"),
    case("sliding-bluestein-63", S, 400, 63, 63, 34, hop=10, path="framed"),
    case("sliding-8192", S, 12288, 8192, 8192, 5, hop=1024, path="fused"),           # the single-line tile
    case("sliding-16384", S, 24576, 16384, 16384, 3, hop=4096, path="framed"),       # two passes
    case("columns-24", CS, 900, 64, 128, 24, hop=32, input_rows=300, fpc=8, path="fused"),
    case("columns-20", CS, 900, 64, 128, 20, hop=32, input_rows=300, fpc=8, path="fused"),  # no multiple of fpc
    # frame 5 (column 0, segment 5) covers 160 .. 223 and frames 6, 7 lie further out: past input_len = 200 although the last frame fits
    case("columns-past-input-len", CS, 250, 64, 64, 10, hop=32, input_rows=100, fpc=8, input_len=200, path="framed"),
    case("folded-3", FC, 600, 150, 64, 4, input_rows=150, path="framed"),
    case("folded-pad", FC, 600, 150, 256, 4, input_rows=150, path="framed"),
    # columns of 100 under a window of 150: frame 3 reads 300 .. 449, input_len = 420 < the tensor's 600 elements
    case("folded-past-input-len", FC, 600, 150, 64, 4, input_rows=100, input_len=420, path="framed"),
]
BY_NAME = {k["name"]: k for k in CASES}
_inputs = {}


def inputs(k, cplx):
    """Signal and window of a case: made once, shared, never modified."""
    key = (k["name"], cplx)
    if key not in _inputs:
        g = np.random.default_rng(zlib.crc32(repr(key).encode()))
        x = g.standard_normal(k["numel"])
        if cplx:
            x = x + 1j * g.standard_normal(k["numel"])
        w = hann(k["window_len"]) + (0.01 * g.standard_normal(k["window_len"]) if k["window_len"] > 1 else 0.0)
        x.setflags(write=False)
        w.setflags(write=False)
        _inputs[key] = (x, w)
    return _inputs[key]


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider
    p = HipProvider(0, precision="F32")
    yield p
    p.close()


def upload(p, x):
    if np.iscomplexobj(x):
        re, im = p.upload(np.ascontiguousarray(x.real), (x.size, 1)), p.upload(np.ascontiguousarray(x.imag), (x.size, 1))
        h = p.complex_from_real_imag(re, im)
        p.free(re)
        p.free(im)
        return h
    return p.upload(x, (x.size, 1))


def request(p, h, k, x, w, rng, denominator):
    from runmat_amd import ProviderSpectralFrameMode as M, ProviderSpectralRequest
    mode = {S: M.Sliding(k["hop"]), CS: M.ColumnSliding(k["hop"], k["input_rows"], k["fpc"]), FC: M.FoldedColumns(k["input_rows"])}[k["mode"]]
    return ProviderSpectralRequest(h, k["input_len"], np.iscomplexobj(x), w, k["nfft"], k["frames"], mode, rng, denominator)


def bounds(k, f, mass, s, ps, scale, denominator):
    n = k["nfft"]
    pow2 = n & (n - 1) == 0
    work = n if pow2 else 1 << math.ceil(math.log2(2 * n - 1))
    delta = (4.0 if pow2 else 8.0) * EPS * max(1.0, math.log2(work)) * np.sqrt(np.sum(np.abs(f) ** 2, axis=0))
    if k["mode"] == FC:
        delta = delta + EPS * math.ceil(k["window_len"] / n) * mass
    delta = delta[None, :] + 1e-300
    return delta, scale[:, None] / denominator * (2.0 * np.abs(s) * delta + delta ** 2) + 4.0 * EPS * ps


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def run_case(p, k, cplx, rng, f32=False):
    x, w = inputs(k, cplx)
    denominator = 2.0 * np.pi * float(np.sum(w * w))
    h = upload(p, x)
    res = p.uniform_spectral_estimate(request(p, h, k, x, w, rng, denominator))
    xe = (x.real.astype(np.float32).astype(np.float64) + (1j * x.imag.astype(np.float32).astype(np.float64) if cplx else 0.0)) if f32 else x
    s, ps, scale, f, mass = ref.estimate(xe, k["input_len"], w, k["nfft"], k["frames"], k["mode"], rng, denominator, k["hop"], k["input_rows"], k["fpc"])
    rows = s.shape[0]
    assert (res.rows, res.cols) == (rows, k["frames"]) and res.s.shape == (rows, k["frames"]) and res.ps.shape == (rows, k["frames"])
    assert p.is_complex(res.s) and not p.is_complex(res.ps)
    gs, gp = p.download_matrix(res.s), p.download_matrix(res.ps)
    assert gs.dtype == np.complex128 and gp.dtype == np.float64
    ds, dp = bounds(k, f, mass, s, ps, scale, denominator)
    if f32:
        ds, dp = ds + ulp32(np.abs(s) + ds), dp + ulp32(ps + dp)
        assert p.buffer_bits(res.ps) == 32
    es, ep = np.abs(gs - s), np.abs(gp - ps)
    print(f"{k['name']} complex={cplx} range={rng} f32={f32}: max err/bound s {float(np.max(es / ds)):.3f} ps {float(np.max(ep / dp)):.3f}")
    assert np.all(es <= ds), (k["name"], float(np.max(es / ds)))
    assert np.all(ep <= dp), (k["name"], float(np.max(ep / dp)))
    log = p.telemetry_snapshot()["kernel_launches_log"][-1]
    other = "framed" if k["path"] == "fused" else "fused"
    assert log["kernel"] == "spectral" and log["shape"] == {"rows": rows, "frames": k["frames"]} and k["path"] in log["tuning"] and other not in log["tuning"], log
    for t in (res.s, res.ps, h):
        p.free(t)


@pytest.mark.parametrize("rng", [ref.ONESIDED, ref.TWOSIDED, ref.CENTERED], ids=["onesided", "twosided", "centered"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", [k["name"] for k in CASES])
def test_against_the_restatement(prov, name, cplx, rng):
    run_case(prov, BY_NAME[name], cplx, rng)


@pytest.mark.parametrize("rng", [ref.ONESIDED, ref.TWOSIDED, ref.CENTERED], ids=["onesided", "twosided", "centered"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", ["sliding-64-hop16", "sliding-bluestein-63", "columns-20", "folded-3"])
def test_precision_32(prov32, name, cplx, rng):
    run_case(prov32, BY_NAME[name], cplx, rng, f32=True)


def test_telemetry_names_the_path(prov):
    for name, path in (("sliding-64-hop16", "fused"), ("sliding-bluestein-100", "framed")):
        k = BY_NAME[name]
        x, w = inputs(k, False)
        h = upload(prov, x)
        res = prov.uniform_spectral_estimate(request(prov, h, k, x, w, ref.ONESIDED, 1.0))
        log = prov.telemetry_snapshot()["kernel_launches_log"][-1]
        assert log["kernel"] == "spectral" and path in log["tuning"] and log["shape"] == {"rows": k["nfft"] // 2 + 1, "frames": k["frames"]}
        for t in (res.s, res.ps, h):
            prov.free(t)


@pytest.mark.parametrize("name", ["sliding-64-hop16", "sliding-bluestein-63", "columns-past-input-len", "folded-3", "sliding-16384"])
def test_two_calls_are_bit_identical(prov, name):
    k = BY_NAME[name]
    x, w = inputs(k, True)
    h = upload(prov, x)
    got = []
    for _ in range(2):
        res = prov.uniform_spectral_estimate(request(prov, h, k, x, w, ref.CENTERED, 3.0))
        got.append((prov.download(res.s).view(np.uint64).copy(), prov.download(res.ps).view(np.uint64).copy()))
        prov.free(res.s)
        prov.free(res.ps)
    prov.free(h)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_pwelch_composition_against_scipy(prov):
    """pwelch's device sequence: mode 1 -> reshape [rows, segments, columns] -> reduce_mean_nd([1]) -> reshape [rows, columns].  Both sides
    carry a transform's error, so the bound is twice the mean of the per-frame power bounds, plus the mean's own roundings."""
    signal = pytest.importorskip("scipy.signal")
    k = BY_NAME["columns-24"]
    x, w = inputs(k, False)
    fs = 2.0 * np.pi
    denominator = fs * float(np.sum(w * w))
    h = upload(prov, x)
    res = prov.uniform_spectral_estimate(request(prov, h, k, x, w, ref.ONESIDED, denominator))
    cube = prov.reshape(res.ps, (65, 8, 3))
    mean = prov.reduce_mean_nd(cube, [1])
    flat = prov.reshape(mean, (65, 3))
    got = prov.download_matrix(flat)
    _, want = signal.welch(x.reshape((300, 3), order="F"), fs=fs, window=w, nperseg=64, noverlap=32, nfft=128, detrend=False, return_onesided=True,
                           scaling="density", axis=0)
    s, ps, scale, f, mass = ref.estimate(x, k["input_len"], w, 128, 24, CS, ref.ONESIDED, denominator, 32, 300, 8)
    _, dp = bounds(k, f, mass, s, ps, scale, denominator)
    lim = 2.0 * dp.reshape((65, 8, 3), order="F").mean(axis=1) + 8 * EPS * want
    assert got.shape == want.shape and np.all(np.abs(got - want) <= lim), float(np.max(np.abs(got - want) / lim))
    for t in (res.s, res.ps, mean, h):  # (the reshapes share their source's buffer)
        prov.free(t)


def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def test_invalid_requests_are_refused_and_leave_nothing(prov):
    from dataclasses import replace
    from runmat_amd import ProviderError, ProviderSpectralFrameMode as M, ProviderSpectralRequest
    x = np.random.default_rng(5).standard_normal(600)
    w = hann(64)
    h = prov.upload(x, (600, 1))
    hc = upload(prov, x[:300] + 1j * x[300:])
    good = ProviderSpectralRequest(h, 600, False, w, 64, 10, M.Sliding(16), ref.ONESIDED, 1.0)
    col = replace(good, frame_mode=M.ColumnSliding(32, 150, 3), frame_count=12)
    fold = replace(good, frame_mode=M.FoldedColumns(150), frame_count=4)
    for ok in (good, col, fold):  # the requests the refused ones are made from are themselves served
        r = prov.uniform_spectral_estimate(ok)
        prov.free(r.s)
        prov.free(r.ps)
    bad = {
        "empty window": replace(good, window=np.zeros(0)),
        "nfft 0": replace(good, nfft=0),
        "no frames": replace(good, frame_count=0),
        "hop 0, sliding": replace(good, frame_mode=M.Sliding(0)),
        "hop 0, columns": replace(col, frame_mode=M.ColumnSliding(0, 150, 3)),
        "coverage, sliding": replace(good, frame_count=35),                      # 34 * 16 + 64 = 608 > 600
        "coverage, columns": replace(col, input_len=500),                        # frame 11: 450 + 64 + 64 = 578 > 500
        "coverage, columns, last frame": replace(col, frame_count=13),          # frame 12: column 4 starts at 600
        "no input rows, columns": replace(col, frame_mode=M.ColumnSliding(32, 0, 3)),
        "no frames per column": replace(col, frame_mode=M.ColumnSliding(32, 150, 0)),
        "coverage, folded": replace(fold, frame_count=5),                        # 5 * 150 > 600
        "no input rows, folded": replace(fold, frame_mode=M.FoldedColumns(0)),
        "denominator nan": replace(good, denominator=float("nan")),
        "denominator inf": replace(good, denominator=float("inf")),
        "denominator 0": replace(good, denominator=0.0),
        "denominator negative": replace(good, denominator=-1.0),
        "input_len beyond the tensor": replace(good, input_len=601),
        "complex flag on a real tensor": replace(good, input_complex=True),
        "real flag on a complex tensor": replace(good, input=hc, input_len=300, frame_count=5),
        "unknown mode": replace(good, frame_mode=M(3, 16, 0, 0)),
        "unknown range": replace(good, range=3),
        "negative range": replace(good, range=-1),
    }
    before = live_bytes(prov)
    for why, req in bad.items():
        with pytest.raises(ProviderError) as err:
            prov.uniform_spectral_estimate(req)
        assert err.value.code == 1, (why, err.value.code, str(err.value))
        assert live_bytes(prov) == before, why
    # a power of two beyond what fft_dim transforms along dimension 0 (2^27): UNSUPPORTED, again with nothing left behind
    with pytest.raises(ProviderError) as err:
        prov.uniform_spectral_estimate(replace(good, window=np.ones(1), nfft=1 << 28, frame_count=1))
    assert err.value.code == 2, (err.value.code, str(err.value))
    assert live_bytes(prov) == before
    r = prov.uniform_spectral_estimate(good)  # and the provider still serves
    assert r.rows == 33 and r.cols == 10
    for t in (r.s, r.ps, h, hc):
        prov.free(t)
