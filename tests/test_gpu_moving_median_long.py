"""GPU checks of `moving_window_long` (rmhip_moving_window_long, signal_ops.hip): movmedian over windows of up to 4096 points.

A median is an order statistic, so every comparison is of bits (`view(np.int64)`) where the result is not NaN and of NaN masks where it is.
The reference is the oracle's `moving_window(..., "median", ...)`; windows that hold zeros of both signs are compared with the stable
restatement in tests/moving_median_ref.py (the oracle's `qsort` is not stable), sign bits included."""
import os

import numpy as np
import pytest

from moving_median_ref import moving_median

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_SHAPE, ERR_NOT_FOUND = 1, 2, 3, 5
NAN = float("nan")


def up(prov, x):
    x = np.asarray(x, dtype=np.float64)
    return prov.upload(x.ravel(order="F"), list(x.shape))


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def median_long(prov, h, want_shape, dim, before, after, endpoints="shrink", nan_mode="include", entry=None):
    out = (entry or prov.moving_window_long)(h, list(want_shape), dim, before, after, "median", endpoints, nan_mode)
    got = prov.download(out).reshape(want_shape, order="F")
    prov.free(out)
    return got


def check(prov, oracle, x, dim, before, after, endpoints="shrink", nan_mode="include", h=None, reference=None):
    own = h is None
    h = up(prov, x) if own else h
    want = (reference or (lambda *a: oracle.moving_window(a[0], a[1], a[2], a[3], "median", a[4], a[5])))(x, dim, before, after, endpoints, nan_mode)
    got = median_long(prov, h, want.shape, dim, before, after, endpoints, nan_mode)
    if own:
        prov.free(h)
    bad = np.flatnonzero(~((got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))).ravel(order="F"))
    assert same_bits(got, want), (np.shape(x), dim, before, after, endpoints, nan_mode, bad[:8], got.ravel(order="F")[bad[:4]], want.ravel(order="F")[bad[:4]])


def raises(code, f, needle=None):
    from runmat_amd import ProviderError

    with pytest.raises(ProviderError) as e:
        f()
    assert e.value.code == code, (e.value.code, str(e.value))
    if needle is not None:
        assert needle in str(e.value), str(e.value)


def live(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def quarters(shape, seed):
    """Data rounded to quarters, away from zero: duplicates are common, no zero of either sign."""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(1.0, 9.0, shape) * 4.0) / 4.0 * rng.choice([-1.0, 1.0], shape)


@pytest.mark.parametrize("before, after", [(32, 32), (32, 33)])
def test_just_over_the_old_cap(prov, oracle, before, after):
    x = quarters((700, 1), 1)
    holes = x.copy()
    holes[[5, 333, 699], 0] = NAN
    holes[400:480, 0] = NAN  # a run longer than the window: under omit some windows hold no value
    for data in (x, holes):
        h = up(prov, data)
        for endpoints in ("shrink", "discard", -1e9, 1e9, float(x[17, 0]), NAN):
            for nan_mode in ("include", "omit"):
                check(prov, oracle, data, 0, before, after, endpoints, nan_mode, h=h)
        prov.free(h)


@pytest.mark.parametrize("before, after", [(127, 127), (127, 128), (128, 128)])
def test_tile_seams_and_parity(prov, oracle, before, after):
    x = quarters((9001, 1), 2)
    h = up(prov, x)
    for endpoints in ("shrink", 2.5):
        check(prov, oracle, x, 0, before, after, endpoints, h=h)
    prov.free(h)


def test_the_cap(prov, oracle):
    x = np.random.default_rng(3).standard_normal((5000, 1))
    h = up(prov, x)
    check(prov, oracle, x, 0, 2047, 2047, h=h)
    check(prov, oracle, x, 0, 2047, 2048, h=h)
    mark = live(prov)
    raises(ERR_UNSUPPORTED, lambda: prov.moving_window_long(h, [5000, 1], 0, 2048, 2048, "median"))  # 4097 points
    assert live(prov) == mark
    prov.free(h)


def test_window_longer_than_the_line(prov, oracle):
    x = quarters((100, 1), 4)
    for endpoints in ("shrink", 0.75):
        check(prov, oracle, x, 0, 200, 200, endpoints)


@pytest.mark.parametrize("shape, dim", [((7, 300), 1), ((3, 200, 2), 1), ((5, 4, 150), 2)], ids=str)
def test_strided_lines(prov, oracle, shape, dim):
    x = quarters(shape, 5)
    x[tuple(s // 2 for s in shape)] = NAN
    h = up(prov, x)
    for before, after in ((32, 32), (64, 64)):
        for endpoints, nan_mode in (("shrink", "include"), (1.25, "omit"), ("discard", "omit")):
            check(prov, oracle, x, dim, before, after, endpoints, nan_mode, h=h)
    prov.free(h)


def test_a_dimension_beyond_the_rank(prov, oracle):
    x = quarters((9, 11), 6)
    check(prov, oracle, x, 2, 40, 40)
    check(prov, oracle, x, 2, 40, 40, 7.0)


def test_value_classes(prov, oracle):
    rng = np.random.default_rng(7)
    n = 400
    mixed = rng.standard_normal(n)
    mixed[rng.choice(n, 120, replace=False)] = np.inf
    mixed[rng.choice(n, 120, replace=False)] = -np.inf
    near_one = (np.float64(1.0).view(np.int64) + rng.integers(0, 3, n)).view(np.float64)  # values that differ only in the last bits
    lines = {
        "constant": np.full(n, 3.5),
        "three values": rng.choice([-1.0, 0.0, 1.0], n),  # every candidate survives to the last digit
        "infinities": mixed,
        "subnormals": rng.integers(1, 50, n) * rng.choice([-1.0, 1.0], n) * 5e-324,
        "last bit": near_one,
    }
    for name, line in lines.items():
        for endpoints in ("shrink", 1.0):
            check(prov, oracle, line.reshape(n, 1), 0, 50, 50, endpoints)


@pytest.mark.parametrize("before, after", [(32, 32), (33, 33), (63, 64)])
def test_signed_zeros(prov, oracle, before, after):
    rng = np.random.default_rng(8)
    n = 500
    zeros = rng.choice([0.0, -0.0], (n, 1))
    some = zeros.copy()
    at = rng.choice(n, 40, replace=False)
    some[at, 0] = rng.choice([-1.0, 1.0], 40)
    stable = lambda x, dim, b, a, endpoints, nan_mode: moving_median(x, dim, b, a, endpoints, nan_mode)
    for data in (zeros, some):
        assert np.signbit(data).any() and not np.signbit(data).all()
        for endpoints in ("shrink", 0.0):
            check(prov, oracle, data, 0, before, after, endpoints, reference=stable)


@pytest.mark.parametrize("dim", [0, 1])
def test_both_entry_points_agree_where_both_serve(prov, dim):
    x = quarters((400, 3), 9)
    x[[3, 200, 399], 0] = NAN
    x[100:110, 1] = NAN
    x[::2, 2] = -0.0
    h = up(prov, x)
    for before, after in ((1, 1), (4, 3), (31, 31), (32, 31)):
        for endpoints in ("shrink", "discard", -2.0, 0.0, NAN):
            for nan_mode in ("include", "omit"):
                shape = list(x.shape)
                if endpoints == "discard":
                    shape[dim] = max(0, shape[dim] - before - after)
                old = median_long(prov, h, shape, dim, before, after, endpoints, nan_mode, entry=prov.moving_window)
                new = median_long(prov, h, shape, dim, before, after, endpoints, nan_mode)
                assert same_bits(new, old), (dim, before, after, endpoints, nan_mode)
    prov.free(h)


def test_precision_32_provider(built, oracle):
    from runmat_amd import HipProvider

    p32 = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    try:
        x = np.random.default_rng(10).standard_normal((600, 2))
        x32 = x.astype(np.float32).astype(np.float64)
        for before, after in ((50, 50), (50, 51)):
            want = oracle.moving_window(x32, 0, before, after, "median").astype(np.float32).astype(np.float64)
            got = median_long(p32, up(p32, x), want.shape, 0, before, after)
            assert same_bits(got, want)
    finally:
        p32.close()


def test_repeatable(prov):
    x = quarters((3000, 2), 11)
    h = up(prov, x)
    first = median_long(prov, h, x.shape, 0, 150, 150, 2.0)
    again = median_long(prov, h, x.shape, 0, 150, 150, 2.0)
    assert np.array_equal(first.view(np.int64), again.view(np.int64))
    prov.free(h)


def test_refusals_and_empties(prov):
    x = quarters((200, 1), 12)
    h = up(prov, x)
    gone = up(prov, x)
    prov.free(gone)
    mark = live(prov)
    raises(ERR_UNSUPPORTED, lambda: prov.moving_window_long(h, [200, 1], 0, 40, 40, "mean"), "rmhip_moving_window")
    assert live(prov) == mark
    raises(ERR_SHAPE, lambda: prov.moving_window_long(h, [199, 1], 0, 40, 40, "median"))
    assert live(prov) == mark
    raises(ERR_INVALID, lambda: prov.moving_window_long(h, [200, 1], 2, 40, 40, "median"))
    assert live(prov) == mark
    raises(ERR_NOT_FOUND, lambda: prov.moving_window_long(gone, [200, 1], 0, 40, 40, "median"))
    assert live(prov) == mark
    raises(ERR_UNSUPPORTED, lambda: prov.moving_window_long(prov.complex_from_real(h), [200, 1], 0, 40, 40, "median"))
    empty = prov.moving_window_long(prov.upload(np.zeros(0), [0, 3]), [0, 3], 0, 40, 40, "median")
    assert list(empty.shape) == [0, 3] and prov.download(empty).size == 0
    none = prov.moving_window_long(h, [80, 1], 0, 60, 60, "median", "discard")
    assert list(none.shape) == [80, 1]
    prov.free(none)
    none = prov.moving_window_long(h, [0, 1], 0, 100, 100, "median", "discard")  # extent <= before + after
    assert list(none.shape) == [0, 1] and prov.download(none).size == 0
    got = median_long(prov, h, (200, 1), 0, 40, 40)                                # ... and the next call is served
    assert np.all(np.isfinite(got))
    prov.free(h)
