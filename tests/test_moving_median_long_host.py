"""CPU checks of `rmhip_moving_window_long`: the stable restatement of the moving median (tests/moving_median_ref.py) equals the oracle bit
for bit on zero-free data and gives the hand-worked results on windows of signed zeros, and the new entry point is bound in every mirror
without changing the served set."""
import re
from pathlib import Path

import numpy as np
import pytest

from moving_median_ref import moving_median

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.parametrize("n, before, after", [(130, 40, 40), (301, 100, 33), (500, 200, 200), (257, 40, 40)])
def test_helper_equals_the_oracle_on_zero_free_data(oracle, n, before, after):
    rng = np.random.default_rng(n + before)
    x = np.round(rng.uniform(1.0, 9.0, (n, 2)) * 4.0) / 4.0  # quarters: duplicates everywhere, no zero
    holes = x.copy()
    holes[rng.choice(n, 6, replace=False), 0] = np.nan
    holes[n // 3:n // 3 + before + after + 5, 1] = np.nan    # a run longer than the window: under omit some windows hold no value
    for data in (x, holes):
        for endpoints in ("shrink", "discard", -1e9, 4.25, 1e9, float("nan")):  # fills below, inside and above the data
            for nan_mode in ("include", "omit"):
                want = oracle.moving_window(data, 0, before, after, "median", endpoints, nan_mode)
                assert same_bits(moving_median(data, 0, before, after, endpoints, nan_mode), want), (endpoints, nan_mode)
    want = oracle.moving_window(holes.T, 1, before, after, "median", 4.25, "omit")
    assert same_bits(moving_median(holes.T, 1, before, after, 4.25, "omit"), want)


def test_signed_zero_kats():
    def middle(values, endpoints="shrink"):  # the one full window of the line
        k = len(values)
        return moving_median(np.array(values), 0, k // 2, k - 1 - k // 2, endpoints)[k // 2]

    assert middle([0.0, -0.0, -0.0]) == 0.0 and np.signbit(middle([0.0, -0.0, -0.0]))        # stable: 0, -0, -0 stays; the middle is -0
    assert middle([-0.0, 0.0, 0.0]) == 0.0 and not np.signbit(middle([-0.0, 0.0, 0.0]))
    assert not np.signbit(middle([0.0, -0.0]))                                                # (0.0 + -0.0) / 2 = 0.0
    assert np.signbit(middle([-0.0, -0.0]))
    # the fill rule: a rank among values equal to the fill returns the fill itself
    x = np.full(5, -0.0)
    got = moving_median(x, 0, 1, 1, 0.0)
    assert not np.signbit(got[0]) and not np.signbit(got[4])   # windows {fill, -0, -0}, {-0, -0, fill}: every rank is "equal to the fill"
    assert np.signbit(got[2])                                  # no padding in this window: its own -0
    got = moving_median(x, 0, 2, 1, 0.0)
    assert not np.signbit(got[0]) and not np.signbit(got[1])   # even totals: (fill + fill) / 2
    assert np.signbit(got[2])


def test_the_entry_point_is_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    assert _lib.SIGNATURES["rmhip_moving_window_long"] == _lib.SIGNATURES["rmhip_moving_window"]
    assert _lib.SERVES["rmhip_moving_window_long"] == ("moving_window",) and _lib.SERVES["rmhip_moving_window"] == ("moving_window",)
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "moving_window_long", None))


def test_the_mirrors_carry_the_entry_point():
    assert "moving_window_long(" in (ROOT / "include" / "rmhip_provider.hpp").read_text()
    assert "moving_window_long(" in (ROOT / "examples" / "provider_kats.cpp").read_text()
    assert "pub fn rmhip_moving_window_long(" in (ROOT / "shim" / "rmhip_sys.rs").read_text()
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index("fn moving_window<"):]
    body = body[:re.search(r"\n    fn ", body).start()]
    first, second = body.index("rmhip_moving_window(self.ctx"), body.index("rmhip_moving_window_long(self.ctx")
    assert first < second
    between = body[first:second]
    assert "RMHIP_ERR_UNSUPPORTED" in between and "Median" in between
