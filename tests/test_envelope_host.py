"""The numpy restatement of signal_envelope (tests/envelope_ref.py) against the CPU builtin's unit-test facts (tests/golden/envelope_kats.json),
against scipy's analytic signal, and - for every case tests/test_gpu_envelope.py runs - against its own long-double evaluation: the f64
restatement must sit within HALF of the bound the GPU test allows, which is the check that those bounds leave the expectation's own arithmetic
room."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import envelope_ref as ref  # noqa: E402
from test_gpu_envelope import BY_NAME, CASES, EPS, bound, expected, inputs  # noqa: E402

KATS = {k["name"]: k for k in json.loads((Path(__file__).resolve().parent / "golden" / "envelope_kats.json").read_text())["cases"]}
METHOD = {"analytic": ref.ANALYTIC, "analytic_fir": ref.ANALYTIC_FIR, "rms": ref.RMS}


def kat_signal(k):
    if "generate" in k:
        g = k["generate"]
        t = np.arange(g["n"]) / float(g["n"])
        amplitude = g["amplitude_offset"] + g["amplitude_depth"] * np.sin(2.0 * np.pi * t)
        return (amplitude * np.sin(2.0 * np.pi * g["carrier_cycles"] * t))[:, None], amplitude
    return np.asarray(k["x"], dtype=np.float64).reshape((k["n"], k["m"]), order="F"), None


def check_kat(k, envelope):
    """`envelope(x [n, m], method, param) -> (upper, lower)`: shared with nothing but this file's restatement; the facts are the data's"""
    x, amplitude = kat_signal(k)
    upper, lower = envelope(x, METHOD[k["method"]], k["param"])
    tol = k.get("tol", 0.0)
    for i, v in k.get("upper_at", {}).items():
        assert abs(upper[int(i), 0] - v) <= tol
    if k.get("lower_is_minus_upper"):
        assert np.array_equal(lower, -upper)
    if "upper_at_least" in k:
        assert np.all(upper >= k["upper_at_least"]) and np.all(lower <= k["lower_at_most"])
    for col, v in k.get("column_upper_equals", {}).items():
        assert np.all(np.abs(upper[:, int(col)] - v) <= tol)
    for col, v in k.get("column_upper_at_least", {}).items():
        assert np.all(upper[:, int(col)] >= v)
    if "differs_from" in k:
        other, _ = envelope(x, METHOD[k["differs_from"]["method"]], k["differs_from"]["param"])
        assert np.max(np.abs(upper - other)) > k["by_more_than"]
    if "envelope_within" in k:
        idx = slice(k["from_index"], k["to_index"] + 1)
        assert np.all(np.abs(upper[idx, 0] - amplitude[idx]) <= k["envelope_within"])


@pytest.mark.parametrize("name", list(KATS))
def test_restatement_passes_the_builtins_facts(name):
    check_kat(KATS[name], lambda x, method, param: ref.envelope(x, method, param)[:2])


def test_fir_taps_are_antisymmetric_and_vanish_on_even_offsets():
    k = ref.fir_taps(9)  # centre 4: integer offsets -4 .. 4
    assert np.array_equal(k[[0, 2, 4, 6, 8]], np.zeros(5)) and np.array_equal(k[:4], -k[:4:-1]) and k[5] > 0 > k[3]
    assert abs(k[5] - 2.0 / np.pi * ref.bessel_i0(8.0 * np.sqrt(1.0 - 0.0625)) / ref.bessel_i0(8.0)) <= 1e-16
    k = ref.fir_taps(4)  # centre 1.5: half-integer offsets, none vanishes
    assert np.all(k != 0.0) and np.allclose(k, -k[::-1], rtol=0, atol=1e-17)
    assert np.array_equal(ref.fir_taps(1), np.zeros(1))
    assert np.array_equal(ref.fir_taps(64, 10, 20), ref.fir_taps(64)[10:21])
    assert abs(ref.bessel_i0(8.0) - 427.56411572180474) <= 1e-12 * 427.56411572180474  # I0(8), Abramowitz & Stegun table 9.11


@pytest.mark.parametrize("n,m", [(2, 1), (3, 2), (64, 3), (100, 2), (1000, 1)])
def test_analytic_is_scipys_hilbert_of_the_centred_signal(n, m):
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(n).standard_normal((n, m)) + 3.0
    upper, lower, aux = ref.envelope(x, ref.ANALYTIC)
    mu = x.mean(axis=0)
    want = np.abs(signal.hilbert(x - mu[None, :], axis=0))
    # two transform pairs of the same kind: eps * log2 n * ||c||_2 each, and the means' difference
    tol = 8.0 * EPS * max(1.0, np.log2(n)) * np.sqrt(np.sum((x - mu) ** 2, axis=0))[None, :] + 4.0 * n * EPS * np.mean(np.abs(x), axis=0)[None, :]
    assert np.all(np.abs(upper - (mu[None, :] + want)) <= tol) and np.all(np.abs(lower - (mu[None, :] - want)) <= tol)


@pytest.mark.parametrize("name", [k["name"] for k in CASES])
def test_f64_restatement_sits_within_half_of_the_gpu_bound(name):
    k = BY_NAME[name]
    x = inputs(k)
    upper, lower, aux = expected(k)
    true_u, true_l, _ = ref.envelope(x, k["method"], k["param"], dtype=np.longdouble)
    core = bound(k, x, upper, aux)
    tail = 0.0 if k["method"] == ref.RMS else 4.0 * EPS
    for got, true in ((upper, true_u), (lower, true_l)):
        lim = core + tail * np.abs(got) + 1e-300
        ratio = float(np.max(np.abs(got.astype(np.longdouble) - true) / lim))
        print(f"{name}: f64 restatement at {ratio:.3f} of the bound")
        assert ratio <= 0.5, (name, ratio)
