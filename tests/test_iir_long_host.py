"""CPU checks of `rmhip_iir_filter_long`: the numpy model of its chunked scan (tests/iir_long_ref.py) meets the accuracy contract on the ten
filters the contract was chosen on and declines an unstable filter, the model of its FIR sum equals the oracle's loop, and the new entry
point is bound in every mirror without changing the served set."""
import numpy as np
import pytest

from iir_long_ref import (CHUNKS, FILTERS, UNSTABLE, chunked_filter, choose_chunk, exact_filter, fir_nested, longdouble_is_wide, noise_floor, normalise,
                          output_bound, state_bound)

N = 20001  # not a multiple of any chunk length: the tail is part of every case


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.mark.parametrize("name", list(FILTERS))
def test_model_meets_both_bounds(oracle, name):
    if not longdouble_is_wide():
        pytest.skip("np.longdouble carries fewer than 63 mantissa bits")
    b, a = FILTERS[name]
    for seed in range(3):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(N) * (1e3 if seed == 2 else 1.0)
        zi = rng.standard_normal(max(len(b), len(a)) - 1)
        got = chunked_filter(b, a, x, zi)
        assert got is not None, (name, seed)
        y, zf, L = got
        assert L in CHUNKS and N // L >= 2 and N % L, (name, L)
        y_ref, zf_ref = oracle.iir_filter(b, a, x, 0, zi)
        y_exact, zf_exact = exact_filter(b, a, x, zi)
        floor = noise_floor(b, a, x)
        out_err, st_err = np.max(np.abs(y - y_exact)), np.max(np.abs(zf - zf_exact))
        out_bound, st_bound = output_bound(y_ref, y_exact, floor), state_bound(zf_ref, zf_exact, b, a, floor)
        print(f"{name} seed {seed}: L {L}, output {out_err / (out_bound / 8):.2f} of 8, state {st_err / (st_bound / 16):.2f} of 16")
        assert out_err <= out_bound, (name, seed, out_err, out_bound)
        assert st_err <= st_bound, (name, seed, st_err, st_bound)


def test_model_chunk_rule():
    assert choose_chunk(*normalise(*UNSTABLE)) is None
    assert chunked_filter(*UNSTABLE, np.ones(N)) is None
    assert choose_chunk(*normalise(*FILTERS["integrator"])) == 256              # |T| = 1: admitted, not amplified
    assert choose_chunk(*normalise(*FILTERS["double_pole_0.995"])) > 256        # k r^k is still above 1 after 256 samples
    assert choose_chunk(*normalise(*FILTERS["double_pole_0.995"]), 600) == 0    # too short for two chunks of an admissible length
    rng = np.random.default_rng(5)
    x, b, a = rng.standard_normal(600), *FILTERS["double_pole_0.995"]
    y, zf, L = chunked_filter(b, a, x)
    from oracle import oracle as o
    wy, wz = o.iir_filter(b, a, x, 0)
    assert L == 0 and np.array_equal(y, wy) and np.array_equal(zf, wz)          # ... so the sequential recurrence answers


@pytest.mark.parametrize("taps", [2, 12, 64])
def test_fir_model_equals_the_oracle(oracle, taps):
    rng = np.random.default_rng(taps)
    b = rng.standard_normal(taps)
    for n in (700, 5):
        x = rng.standard_normal(n)
        for zi in (None, rng.standard_normal(taps - 1)):
            y, zf = fir_nested(b, [1.0], x, zi)
            wy, wz = oracle.iir_filter(b, [1.0], x, 0, zi)
            assert np.array_equal(y, wy) and np.array_equal(zf, wz), (taps, n, zi is None)
    x = rng.standard_normal(100)
    y, zf = fir_nested(2.0 * b, [2.0, 0.0, 0.0], x)                              # a(1) = 2 and explicit zero denominator taps
    wy, wz = oracle.iir_filter(2.0 * b, [2.0, 0.0, 0.0], x, 0)
    assert zf.shape == (max(taps, 3) - 1,) and np.array_equal(y, wy) and np.array_equal(zf, wz)


def test_the_entry_point_is_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    assert "rmhip_iir_filter_long" in _lib.SIGNATURES and len(_lib.SIGNATURES["rmhip_iir_filter_long"][1]) == 9
    assert _lib.SIGNATURES["rmhip_iir_filter_long"] == _lib.SIGNATURES["rmhip_iir_filter"]
    assert _lib.SERVES["rmhip_iir_filter_long"] == ("iir_filter",) and _lib.SERVES["rmhip_iir_filter"] == ("iir_filter",)
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "iir_filter_long", None))
