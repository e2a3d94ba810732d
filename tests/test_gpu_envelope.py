"""GPU parity of signal_envelope (include/rmhip.h, signal_ops.hip) against the numpy restatement in tests/envelope_ref.py.

Bounds, derived rather than tuned.  Per channel: A = mean |x|, c = x - mu the centred signal, eps = 2^-52.  The device's mean is a tree sum,
the restatement's is numpy's: both lie within n * eps * A of the true mean, so the two differ by at most
    dmu = 2 * n * eps * A.
Analytic: a shift of the mean by d shifts bin 0 of c, hence Re z, by d and mu + |z| by at most 2 d (dmu counts both sides); the transform
pair carries the bound tests/test_gpu_fft.py states for one transform, twice (forward and inverse, the mask at most doubles a bin), on
both sides of the comparison - C = 4 and work = n for a power of two, C = 8 and work = the padded convolution length otherwise:
    |delta| <= 4 * C * eps * max(1, log2 work) * ||c||_2 + dmu + 4 * eps * |value|.
FIR: q_i is a sum of at most L products added in order, c_i and every c_j carry the mean's difference:
    |delta| <= (L + 2) * eps * (|c_i| + sum |c_j k_t|) + dmu * (1 + sum |k_t|) + 4 * eps * |value|.
RMS: a sum of e - s non-negative terms, a division and a square root, so the bound is relative:
    |delta| <= (e - s + 3) * eps * upper.
tests/test_envelope_host.py checks that the f64 restatement itself sits within half of each bound against a long-double evaluation.
On a precision-32 provider the expectation is formed from the f32-rounded input and each bound grows by one f32 ulp of the value."""
import math
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import envelope_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
A, F, R = ref.ANALYTIC, ref.ANALYTIC_FIR, ref.RMS


def case(name, method, n, m, param=0, shape=None, signal="noise"):
    return dict(name=name, method=method, n=n, m=m, param=param, shape=tuple(shape) if shape else (n, m), signal=signal)


CASES = []
# analytic: 1 .. 3 are degenerate transforms, 100 and 1000 take the Bluestein path, 8192 is one tile, 16384 two passes; channels shorter than
# 4096 are summed by a wave each, 8192 by one workgroup, 16384 by two workgroups and a second launch
for _n in (1, 2, 3, 64, 100, 1000, 8192, 16384):
    CASES.append(case(f"analytic-{_n}x1", A, _n, 1))
CASES += [
    case("analytic-64-rank1", A, 64, 1, shape=(64,)),
    case("analytic-64-row", A, 64, 1, shape=(1, 64)),
    case("analytic-100-row", A, 100, 1, shape=(1, 100)),
    case("analytic-1x3", A, 1, 3),
    case("analytic-3x3", A, 3, 3),
    case("analytic-100x3", A, 100, 3),
    case("analytic-8192x3", A, 8192, 3),
    case("analytic-16384x3", A, 16384, 3),
    case("analytic-2x130", A, 2, 130),
    case("analytic-64x130", A, 64, 130),
    case("analytic-100x130", A, 100, 130),
    case("analytic-amplitudes", A, 300, 2, signal="amplitudes"),
    case("analytic-offset-1000", A, 1000, 1, signal="offset"),
    case("analytic-offset-1024x3", A, 1024, 3, signal="offset"),
]
# FIR: 50 samples lie inside one workgroup (three channels: the boundaries too), 3000 cross workgroups; L = 4001 leaves the LDS path
for _n, _long in ((50, 77), (3000, 4001)):
    for _L in (1, 2, 5, 64, 129, _long):
        CASES.append(case(f"fir-{_n}x1-L{_L}", F, _n, 1, _L))
CASES += [
    case("fir-50x3-L5", F, 50, 3, 5),
    case("fir-50x3-L64", F, 50, 3, 64),
    case("fir-50x130-L5", F, 50, 130, 5),
    case("fir-3000x3-L129", F, 3000, 3, 129),
    case("fir-50-row-L5", F, 50, 1, 5, shape=(1, 50)),
    case("fir-1x3-L5", F, 1, 3, 5),
    case("fir-amplitudes-L65", F, 300, 2, 65, signal="amplitudes"),
    case("fir-offset-1000-L33", F, 1000, 1, 33, signal="offset"),
]
# RMS: w = 6001 on 3000 samples leaves the LDS path
for _w in (1, 2, 3, 50, 77, 101):
    CASES.append(case(f"rms-50x1-w{_w}", R, 50, 1, _w))
CASES += [
    case("rms-50x3-w3", R, 50, 3, 3),
    case("rms-50x3-w50", R, 50, 3, 50),
    case("rms-50x130-w2", R, 50, 130, 2),
    case("rms-700x3-w50", R, 700, 3, 50),
    case("rms-700x1-w1000", R, 700, 1, 1000),
    case("rms-3000x1-w50", R, 3000, 1, 50),
    case("rms-3000x1-w6001", R, 3000, 1, 6001),
    case("rms-1x3-w3", R, 1, 3, 3),
    case("rms-64-rank1-w3", R, 64, 1, 3, shape=(64,)),
    case("rms-amplitudes-w51", R, 300, 2, 51, signal="amplitudes"),
]
BY_NAME = {k["name"]: k for k in CASES}
assert len(BY_NAME) == len(CASES)
F32_CASES = ["analytic-64x1", "analytic-100x3", "analytic-16384x1", "analytic-64-row", "fir-50x3-L5", "fir-3000x1-L129", "fir-3000x1-L4001", "rms-50x3-w3",
             "rms-700x1-w1000", "rms-3000x1-w6001", "rms-amplitudes-w51", "analytic-1x3"]
_inputs = {}
_expected = {}


def inputs(k):
    """The [n, m] signal of a case (channels in columns): made once, shared, never modified."""
    key = (k["signal"], k["n"], k["m"])
    if key not in _inputs:
        g = np.random.default_rng(zlib.crc32(repr(key).encode()))
        n, m = k["n"], k["m"]
        t = np.arange(n)[:, None] / float(n)
        if k["signal"] == "noise":
            x = g.standard_normal((n, m)) + 0.5 * np.arange(m)[None, :]
        elif k["signal"] == "amplitudes":  # a window or halo that leaks across the channel boundary fails by orders of magnitude
            x = g.standard_normal((n, m)) * np.array([1.0e6, 1.0])[None, :]
        else:  # a modulated tone riding on a large offset
            x = 1.0e6 + (1.0 + 0.3 * np.sin(2.0 * np.pi * 3.0 * t)) * np.sin(2.0 * np.pi * 37.0 * t + np.arange(m)[None, :])
        x = np.ascontiguousarray(x)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def expected(k, f32=False):
    """(upper, lower, aux) of the f64 restatement, computed once per case; on a precision-32 provider from the f32-rounded input"""
    key = (k["name"], f32)
    if key not in _expected:
        x = inputs(k)
        _expected[key] = ref.envelope(x.astype(np.float32).astype(np.float64) if f32 else x, k["method"], k["param"])
    return _expected[key]


def bound(k, x, upper, aux):
    """the docstring's bound on |device - restatement| for `upper` (and, RMS apart, for `lower` with |value| taken from it), [n, m]"""
    n = k["n"]
    if k["method"] == R:
        return (aux["count"][:, None] + 3.0) * EPS * np.abs(upper)
    dmu = 2.0 * n * EPS * np.mean(np.abs(x), axis=0)[None, :]
    c = aux["c"]
    if k["method"] == A:
        pow2 = n & (n - 1) == 0
        work = n if pow2 else 1 << math.ceil(math.log2(2 * n - 1))
        lead = 4.0 * (4.0 if pow2 else 8.0) * EPS * max(1.0, math.log2(work)) * np.sqrt(np.sum(c * c, axis=0))[None, :]
        return lead + dmu
    if n == 1:
        return dmu + np.zeros_like(x)
    return (k["param"] + 2.0) * EPS * (np.abs(c) + aux["mass"]) + dmu * (1.0 + aux["ksum"][:, None])


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider
    p = HipProvider(0, precision="F32")
    yield p
    p.close()


def request(h, k, method=None, param=None, **over):
    from runmat_amd import ProviderEnvelopeMethod, ProviderEnvelopeRequest
    q = dict(input=h, channel_len=k["n"], channel_count=k["m"], output_shape=k["shape"],
             method=ProviderEnvelopeMethod(k["method"] if method is None else method, k["param"] if param is None else param))
    q.update(over)
    return ProviderEnvelopeRequest(**q)


def run_case(p, k, f32=False):
    x = inputs(k)
    h = p.upload(x.reshape(-1, order="F"), k["shape"])
    res = p.signal_envelope(request(h, k))
    want_u, want_l, aux = expected(k, f32)
    assert res.upper.shape == k["shape"] and res.lower.shape == k["shape"]
    assert not p.is_complex(res.upper) and not p.is_complex(res.lower)
    if f32:
        assert p.buffer_bits(res.upper) == 32 and p.buffer_bits(res.lower) == 32
    got_u = p.download(res.upper).reshape((k["n"], k["m"]), order="F")
    got_l = p.download(res.lower).reshape((k["n"], k["m"]), order="F")
    xe = x.astype(np.float32).astype(np.float64) if f32 else x
    core = bound(k, xe, want_u, aux)
    tail = 0.0 if k["method"] == R else 4.0 * EPS
    lim_u, lim_l = core + tail * np.abs(want_u) + 1e-300, core + tail * np.abs(want_l) + 1e-300
    if f32:
        lim_u, lim_l = lim_u + ulp32(np.abs(want_u) + lim_u), lim_l + ulp32(np.abs(want_l) + lim_l)
    eu, el = np.abs(got_u - want_u), np.abs(got_l - want_l)
    print(f"{k['name']} f32={f32}: max err/bound upper {float(np.max(eu / lim_u)):.3f} lower {float(np.max(el / lim_l)):.3f}")
    assert np.all(eu <= lim_u), (k["name"], float(np.max(eu / lim_u)))
    assert np.all(el <= lim_l), (k["name"], float(np.max(el / lim_l)))
    if k["method"] == R:
        assert np.array_equal((-got_u).view(np.uint64), got_l.view(np.uint64)), "lower is not -upper bit for bit"
    else:
        # upper + lower = 2 mu_device: each of the two carries one rounding of its own magnitude, so the sum of a channel's pair sits within
        # 2 ulp (of the larger of the pair) of twice ONE number, which is read off the sample where the pair is smallest
        ulp = ulp32 if f32 else np.spacing
        size = np.maximum(np.abs(got_u), np.abs(got_l))
        s = got_u + got_l
        at = np.argmin(size, axis=0)
        cols = np.arange(k["m"])
        twice_mu, slack = s[at, cols][None, :], 2.0 * ulp(size[at, cols])[None, :]
        assert np.all(np.abs(s - twice_mu) <= 2.0 * ulp(size) + slack), k["name"]
        dmu = 2.0 * k["n"] * EPS * np.mean(np.abs(xe), axis=0)[None, :]
        assert np.all(np.abs(0.5 * twice_mu - aux["mu"][None, :]) <= dmu + slack), k["name"]
    log = p.telemetry_snapshot()["kernel_launches_log"][-1]
    assert log["kernel"] == "envelope" and log["shape"] == {"channel_len": k["n"], "channels": k["m"]} and list(log["tuning"]) == [ref.NAMES[k["method"]]], log
    for t in (res.upper, res.lower, h):
        p.free(t)


@pytest.mark.parametrize("name", [k["name"] for k in CASES])
def test_against_the_restatement(prov, name):
    run_case(prov, BY_NAME[name])


@pytest.mark.parametrize("name", F32_CASES)
def test_precision_32(prov32, name):
    run_case(prov32, BY_NAME[name], f32=True)


def test_offset_signal_keeps_its_envelope(prov):
    """1e6 + a modulated tone: the bound is taken on ||c||_2, not ||x||_2, and the envelope itself (~1) is resolved to 1e-6 of its size.
    What the case cannot do is tell centring first from clearing bin 0 afterwards: dmu = 2 n eps A is 4.4e-7 here and dominates the bound,
    while a numpy evaluation of the uncentred variant errs by 3.5e-10 (1.5e-9 on the 1024 x 3 case) - 0.001 to 0.003 of the bound.  The
    mean's own rounding allowance is of the size of the effect."""
    k = BY_NAME["analytic-offset-1000"]
    x = inputs(k)
    h = prov.upload(x.reshape(-1), k["shape"])
    res = prov.signal_envelope(request(h, k))
    got = prov.download(res.upper)
    want, _, aux = expected(k)
    lim = bound(k, x, want, aux)[:, 0] + 4.0 * EPS * np.abs(want[:, 0])
    assert float(np.max(lim)) < 1.0e-6 and np.all(np.abs(got - want[:, 0]) <= lim)
    for t in (res.upper, res.lower, h):
        prov.free(t)


@pytest.mark.parametrize("name", ["analytic-100x3", "analytic-16384x3", "fir-3000x3-L129", "rms-700x3-w50"])
def test_two_calls_are_bit_identical(prov, name):
    k = BY_NAME[name]
    h = prov.upload(inputs(k).reshape(-1, order="F"), k["shape"])
    got = []
    for _ in range(2):
        res = prov.signal_envelope(request(h, k))
        got.append((prov.download(res.upper).view(np.uint64).copy(), prov.download(res.lower).view(np.uint64).copy()))
        prov.free(res.upper)
        prov.free(res.lower)
    prov.free(h)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


GOOD = BY_NAME["analytic-100x3"]
BIG = 1 << 63


def _poisoned(value, where):
    def make(p, h):
        x = inputs(GOOD).copy()
        at = 0 if where == "first" else -1  # the first element, or the last element of the last channel
        x[at, at] = value
        return request(p.upload(x.reshape(-1, order="F"), GOOD["shape"]), GOOD), True
    return make


def _long_tail_nan(p, h):
    k = BY_NAME["analytic-16384x1"]
    x = inputs(k).copy()
    x[-1, 0] = np.nan  # the scalar tail of the last of a channel's parts
    return request(p.upload(x.reshape(-1), k["shape"]), k, method=R, param=3), True


def _complex(p, h):
    re = p.upload(inputs(GOOD).reshape(-1, order="F"), GOOD["shape"])
    hc = p.complex_from_real_imag(re, re)
    p.free(re)
    return request(hc, GOOD), True


def _fresh(n, method, param):
    def make(p, h):
        k = case("refused", method, n, 1, param)
        return request(p.upload(np.zeros(n), (n, 1)), k), True
    return make


def _reshaped(shape, n, m):
    def make(p, h):
        return request(p.upload(inputs(GOOD).reshape(-1, order="F"), shape), GOOD, channel_len=n, channel_count=m, output_shape=shape), True
    return make


# name -> (error code, maker(p, good handle) -> (request, the request's input is the maker's own and is freed afterwards))
REFUSALS = {
    "unknown method": (1, lambda p, h: (request(h, GOOD, method=3), False)),
    "negative method": (1, lambda p, h: (request(h, GOOD, method=-1), False)),
    "channel_len 0": (1, lambda p, h: (request(h, GOOD, channel_len=0), False)),
    "channel_count 0": (1, lambda p, h: (request(h, GOOD, channel_count=0), False)),
    "filter_len 0": (1, lambda p, h: (request(h, GOOD, method=F, param=0), False)),
    "window_len 0": (1, lambda p, h: (request(h, GOOD, method=R, param=0), False)),
    "n * m overflows": (1, lambda p, h: (request(h, GOOD, channel_len=BIG, channel_count=4), False)),
    "output shape overflows": (1, lambda p, h: (request(h, GOOD, output_shape=(BIG, 4)), False)),
    "output shape holds another count": (1, lambda p, h: (request(h, GOOD, output_shape=(100, 2)), False)),
    "n * m is not the tensor's count": (1, lambda p, h: (request(h, GOOD, channel_len=50, channel_count=3, output_shape=(50, 3)), False)),
    "shape [m, n]": (1, lambda p, h: (request(h, GOOD, channel_len=3, channel_count=100), False)),
    "matrix taken as one channel": (1, lambda p, h: (request(h, GOOD, channel_len=300, channel_count=1), False)),
    "rank 3": (1, _reshaped((10, 10, 3), 100, 3)),
    "rank-1 tensor as channels": (1, _reshaped((300,), 100, 3)),
    "nan first": (1, _poisoned(np.nan, "first")),
    "+inf first": (1, _poisoned(np.inf, "first")),
    "-inf first": (1, _poisoned(-np.inf, "first")),
    "nan last": (1, _poisoned(np.nan, "last")),
    "+inf last": (1, _poisoned(np.inf, "last")),
    "-inf last": (1, _poisoned(-np.inf, "last")),
    "nan at the end of a long channel": (1, _long_tail_nan),
    "complex input": (2, _complex),
    "analytic beyond the transforms": (2, _fresh((1 << 23) + 8, A, 0)),
    "fir beyond 2^36 products": (2, _fresh((1 << 18) + 1, F, (1 << 18) + 1)),
    "rms beyond 2^36 products": (2, _fresh((1 << 18) + 1, R, 1 << 40)),
}


@pytest.mark.parametrize("why", list(REFUSALS))
def test_refused_requests_leave_nothing(prov, why):
    from runmat_amd import ProviderError
    code, make = REFUSALS[why]
    h = prov.upload(inputs(GOOD).reshape(-1, order="F"), GOOD["shape"])
    ok = prov.signal_envelope(request(h, GOOD))  # (the request the refused ones are made from is itself served; it warms the pool too)
    prov.free(ok.upper)
    prov.free(ok.lower)
    req, own = make(prov, h)
    before = live_bytes(prov)
    with pytest.raises(ProviderError) as err:
        prov.signal_envelope(req)
    assert err.value.code == code, (why, err.value.code, str(err.value))
    assert live_bytes(prov) == before, why
    if own:
        prov.free(req.input)
    res = prov.signal_envelope(request(h, GOOD))  # and the provider still serves
    want, _, aux = expected(GOOD)
    got = prov.download(res.upper).reshape((100, 3), order="F")
    assert np.all(np.abs(got - want) <= bound(GOOD, inputs(GOOD), want, aux) + 4.0 * EPS * np.abs(want))
    for t in (res.upper, res.lower, h):
        prov.free(t)


def test_null_outputs_are_refused(prov):
    import ctypes as C
    h = prov.upload(inputs(GOOD).reshape(-1, order="F"), GOOD["shape"])
    dims = (C.c_size_t * 2)(100, 3)
    out = C.c_uint64()
    before = live_bytes(prov)
    for upper, lower in ((None, C.byref(out)), (C.byref(out), None), (None, None)):
        assert prov._lib.rmhip_signal_envelope(prov._ctx, h.buffer_id, 100, 3, dims, 2, 0, 0, upper, lower) == 1
        assert live_bytes(prov) == before
    prov.free(h)
