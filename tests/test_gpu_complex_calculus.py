"""GPU checks of the calculus and filter hooks on complex-interleaved tensors (rmhip_complex_gradient_dim / _trapz_dim / _polyint /
_iir_filter / _iir_filter_long; misc_ops.hip, signal_ops.hip) against the numpy model (tests/complex_calculus_ref.py).

Gradient, polyint, the trapezoid terms and the filter's sequential forms are compared on the bits of the interleaved doubles (a computed
NaN matches a NaN: its sign and payload are the processor's); trapezoid sums meet n * eps * sum|t| per part against the strictly sequential
sum; the long filter meets its sibling's accuracy contract per part.  Every operand carries a block of special values at its head in which
the two parts of an element differ in kind - a NaN beside a zero, an infinity beside a finite value - so a part that leaked into the other
would show."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_calculus_ref as ref  # noqa: E402
from iir_long_ref import FILTERS, UNSTABLE, df2t, exact_filter, longdouble_is_wide, noise_floor, normalise, output_bound, state_bound  # noqa: E402
from test_complex_calculus_host import GRADIENT_SPACING, KATS, gradient_probe  # noqa: E402
from test_gpu_complex_move import ERR_INVALID, ERR_SHAPE, ERR_UNSUPPORTED, lib_shape, live, raises, up_c, up_r  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 1.7e308
SPECIAL_RE = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, BIG])
SPECIAL_IM = np.roll(SPECIAL_RE, 3)  # NaN, 5e-324, BIG, 0, -0, inf, -inf: every element pairs two different kinds


def data(shape, seed=0, f32=False, big=BIG, special=True, ints=False):
    """Seeded complex data of `shape`, the special block at its head (column-major).  `ints`: small integers, on which every order of
    summation is exact; `f32`: parts representable in f32 (what a precision-32 provider holds), no special block."""
    n = int(np.prod(shape, dtype=np.int64))
    rng = np.random.default_rng(2000 + seed)
    if ints:
        re, im = rng.integers(-8, 9, n).astype(np.float64), rng.integers(-8, 9, n).astype(np.float64)
    else:
        re, im = rng.standard_normal(n), rng.standard_normal(n)
    if f32:
        re, im = re.astype(np.float32).astype(np.float64), im.astype(np.float32).astype(np.float64)
    elif special and not ints:
        k = min(n, SPECIAL_RE.size)
        re[:k], im[:k] = np.where(SPECIAL_RE == BIG, big, SPECIAL_RE)[:k], np.where(SPECIAL_IM == BIG, big, SPECIAL_IM)[:k]
    return ref.join(re, im).reshape(tuple(shape), order="F")


def got(prov, h):
    return ref.from_interleaved(prov.download(h).view(np.float64), lib_shape(prov, h))


def check(prov, h, want, what, free=True):
    """`h` is complex, has the model's shape and holds its bits."""
    assert prov.is_complex(h), what
    assert tuple(lib_shape(prov, h)) == tuple(want.shape), (what, lib_shape(prov, h), want.shape)
    assert ref.same_bits(got(prov, h), want), what
    if free:
        prov.free(h)


def check_sum(prov, h, want, mag, n, what):
    """Per part: a finite model value within n * eps * sum|t|, a non-finite one reproduced in kind."""
    assert prov.is_complex(h), what
    assert tuple(lib_shape(prov, h)) == tuple(want.shape), (what, lib_shape(prov, h), want.shape)
    g, w, m = ref.interleaved(got(prov, h)), ref.interleaved(want), ref.interleaved(mag)
    fin = np.isfinite(w)
    with np.errstate(all="ignore"):
        assert np.all(np.abs(g[fin] - w[fin]) <= n * ref.EPS * m[fin]), (what, float(np.max(np.abs(g[fin] - w[fin]) / np.maximum(m[fin], 1e-300))) / (n * ref.EPS))
    assert np.array_equal(np.isnan(g[~fin]), np.isnan(w[~fin])) and np.array_equal(g[~fin][~np.isnan(g[~fin])], w[~fin][~np.isnan(w[~fin])]), what
    prov.free(h)


def kat(name):
    (c,) = [c for c in KATS if c["name"] == name]
    return c


# ---- gradient -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [0, 1, 2, 3])
def test_gradient_along_every_dimension_and_beyond_the_rank(prov, dim):
    z = data((5, 4, 3), seed=dim)
    h = up_c(prov, z)
    check(prov, prov.complex_gradient_dim(h, dim, 0.7), ref.gradient(z, dim, 0.7), ("gradient", dim))
    prov.free(h)


def test_gradient_small_extents_a_second_block_and_the_fixture(prov):
    for shape, dim, spacing in (((2, 3), 0, 3.0), ((1, 4), 0, 0.7), ((0, 3), 0, 1.0), ((0, 3), 1, 1.0), ((300, 3), 0, 3.0), ((3, 300), 1, 0.7)):
        z = data(shape, seed=10 + shape[0])
        h = up_c(prov, z)
        check(prov, prov.complex_gradient_dim(h, dim, spacing), ref.gradient(z, dim, spacing), ("gradient", shape, dim))
        prov.free(h)
    for name in ("gradient_complex_host_supported", "gradient_complex_coordinate_vector_spacing"):
        c = kat(name)
        h = up_c(prov, ref.from_interleaved(c["data"], c["shape"]))
        want = ref.from_interleaved(c["expect"], c["expect_shape"])
        if "coordinates" in c:
            hc = up_r(prov, np.array(c["coordinates"]))
            check(prov, prov.complex_gradient_dim_with_coordinates(h, c["dim"], hc), want, name)
            prov.free(hc)
        else:
            check(prov, prov.complex_gradient_dim(h, c["dim"], c["spacing"]), want, name)
        prov.free(h)


def test_gradient_multiplies_by_the_reciprocal_and_does_not_divide(prov):
    z = gradient_probe()
    h = up_c(prov, z)
    out = prov.complex_gradient_dim(h, 0, GRADIENT_SPACING)
    assert not ref.same_bits(got(prov, out), ref.gradient_quotient(z, 0, GRADIENT_SPACING))
    check(prov, out, ref.gradient(z, 0, GRADIENT_SPACING), "the seeded vector")
    prov.free(h)


def test_gradient_with_coordinates_and_refusals(prov):
    z = data((5, 4, 3), seed=20)
    coords = np.cumsum(np.random.default_rng(21).uniform(0.3, 1.7, 4))
    h, hc = up_c(prov, z), up_r(prov, coords)
    check(prov, prov.complex_gradient_dim_with_coordinates(h, 1, hc), ref.gradient(z, 1, coordinates=coords), "coordinates")
    row = up_r(prov, coords.reshape(1, 4))
    view = prov.transpose(row)  # a lazy view of a real side operand is materialised, as in the sibling
    check(prov, prov.complex_gradient_dim_with_coordinates(h, 1, view), ref.gradient(z, 1, coordinates=coords), "coordinates through a view")
    prov.free(view)
    prov.free(row)
    hcc, hr = up_c(prov, data((4, 1), seed=22)), up_r(prov, z.real)
    before = live(prov)
    raises(ERR_UNSUPPORTED, lambda: prov.complex_gradient_dim_with_coordinates(h, 1, hcc), "gradient_dim_with_coordinates: coordinates must be real")
    raises(ERR_SHAPE, lambda: prov.complex_gradient_dim_with_coordinates(h, 0, hc), "gradient: coordinate vector length must match the dimension")
    raises(ERR_UNSUPPORTED, lambda: prov.complex_gradient_dim(hr, 0, 1.0), "rmhip_gradient_dim serves it")
    raises(ERR_UNSUPPORTED, lambda: prov.gradient_dim(h, 0, 1.0), "this entry point takes real tensors")  # the sibling still refuses complex storage
    raises(ERR_INVALID, lambda: prov.complex_gradient_dim(h, -1, 1.0), "gradient_dim: dim must be >= 0")
    assert live(prov) == before
    for x in (h, hc, hcc, hr):
        prov.free(x)


# ---- trapz / cumtrapz -----------------------------------------------------------------------------------------------------------------------
def spacing_for(prov, kind, shape, dim, seed, ints=False):
    """-> (the provider's spacing argument, the model's, handles to free)"""
    rng = np.random.default_rng(3000 + seed)
    draw = (lambda n: rng.integers(1, 4, n).astype(np.float64)) if ints else (lambda n: rng.uniform(0.2, 1.8, n))
    if kind == 0:
        return None, None, []
    if kind == 1:
        return (2.0 if ints else 0.37), (2.0 if ints else 0.37), []
    if kind == 2:
        v = np.array([2.0 if ints else 0.37, 9.0])
        h = up_r(prov, v)
        return ("scalar_handle", h), v, [h]
    if kind == 3:
        v = np.cumsum(draw(shape[dim] + 2))  # longer than the dimension: the first `extent` coordinates count
        h = up_r(prov, v)
        return ("vector", h), v, [h]
    v = np.cumsum(draw(int(np.prod(shape))).reshape(shape, order="F"), axis=dim)
    h = up_r(prov, v)
    return ("tensor", h), v, [h]


@pytest.mark.parametrize("dim", [0, 1, 2])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_trapezoid_every_spacing_kind_along_every_dimension(prov, kind, dim):
    shape = (7, 5, 3)
    z = data(shape, seed=30 + kind, big=1e300)  # (1.7e308 would put the order of summation in charge of an overflow)
    zi = data(shape, seed=40 + kind, ints=True)
    for operand, ints in ((z, False), (zi, True)):
        h = up_c(prov, operand)
        arg, model, handles = spacing_for(prov, kind, shape, dim, 5 * kind + dim, ints)
        for cumulative in (False, True):
            want, mag = ref.trapz(operand, dim, kind, model, cumulative)
            out = (prov.complex_cumtrapz_dim if cumulative else prov.complex_trapz_dim)(h, dim, arg)
            if ints:
                check(prov, out, want, ("integers", kind, dim, cumulative))  # every order of summation is exact: bitwise
            else:
                check_sum(prov, out, want, mag, shape[dim], (kind, dim, cumulative))
        for x in handles + [h]:
            prov.free(x)


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_trapezoid_terms_are_exact(prov, kind):
    """An extent of two leaves one term per line: 0 + t is t, so the result shows the term's own bits - special values included."""
    for shape, dim in (((2, 5, 3), 0), ((5, 2, 3), 1), ((5, 3, 2), 2)):
        z = data(shape, seed=50 + kind)
        h = up_c(prov, z)
        arg, model, handles = spacing_for(prov, kind, shape, dim, 60 + kind)
        check(prov, prov.complex_cumtrapz_dim(h, dim, arg), ref.trapz(z, dim, kind, model, True)[0], ("cumtrapz term", kind, shape))
        check(prov, prov.complex_trapz_dim(h, dim, arg), ref.trapz(z, dim, kind, model, False)[0], ("trapz term", kind, shape))
        for x in handles + [h]:
            prov.free(x)


@pytest.mark.parametrize("shape,dim", [((3000, 2), 0), ((2, 3000), 1)], ids=str)
def test_trapezoid_lines_long_enough_to_split(prov, shape, dim):
    z, zi = data(shape, seed=70, big=1e300), data(shape, seed=71, ints=True)
    for kind in (0, 3):
        for operand, ints in ((z, False), (zi, True)):
            h = up_c(prov, operand)
            arg, model, handles = spacing_for(prov, kind, shape, dim, 72 + kind, ints)
            for cumulative in (False, True):
                want, mag = ref.trapz(operand, dim, kind, model, cumulative)
                out = (prov.complex_cumtrapz_dim if cumulative else prov.complex_trapz_dim)(h, dim, arg)
                if ints:
                    check(prov, out, want, ("integers", kind, shape, cumulative))
                else:
                    check_sum(prov, out, want, mag, shape[dim], (kind, shape, cumulative))
            for x in handles + [h]:
                prov.free(x)


def test_trapezoid_degenerate_shapes_and_the_fixture(prov):
    for shape, dim in (((1, 4), 0), ((0, 3), 0), ((3, 0), 0), ((4, 3), 3), ((4, 3), 2)):
        z = data(shape, seed=80)
        h = up_c(prov, z)
        for cumulative in (False, True):
            want, _ = ref.trapz(z, dim, 0, None, cumulative)
            assert not np.any(ref.interleaved(want)) and not np.any(np.signbit(ref.interleaved(want)))  # complex zeros (+0, +0) of the output shape
            check(prov, (prov.complex_cumtrapz_dim if cumulative else prov.complex_trapz_dim)(h, dim), want, ("degenerate", shape, dim, cumulative))
        prov.free(h)
    c = kat("trapezoid_provider_preserves_complex_storage_and_integrates_lanes")
    h = up_c(prov, ref.from_interleaved(c["data"], c["shape"]))
    check(prov, prov.complex_trapz_dim(h, c["dim"]), ref.from_interleaved(c["expect"], c["expect_shape"]), "fixture trapz")
    check(prov, prov.complex_cumtrapz_dim(h, c["dim"]), ref.from_interleaved(c["expect_cumulative"], c["expect_cumulative_shape"]), "fixture cumtrapz")
    prov.free(h)


def test_trapezoid_refusals(prov):
    z = data((7, 5), seed=90)
    h, hr = up_c(prov, z), up_r(prov, z.real)
    cs, short_v, short_t = up_c(prov, data((7, 5), seed=91)), up_r(prov, np.arange(6.0)), up_r(prov, np.arange(34.0))
    before = live(prov)
    for f in (prov.complex_trapz_dim, prov.complex_cumtrapz_dim):
        raises(ERR_UNSUPPORTED, lambda: f(h, 0, ("vector", cs)), "trapezoid: spacing vector must be real")
        raises(ERR_UNSUPPORTED, lambda: f(h, 0, ("tensor", cs)), "trapezoid: spacing tensor must be real")
        raises(ERR_UNSUPPORTED, lambda: f(h, 0, ("scalar_handle", cs)), "trapezoid: spacing tensor must be real")
        raises(ERR_SHAPE, lambda: f(h, 0, ("vector", short_v)), "trapezoid: spacing vector is shorter than integration dimension")
        raises(ERR_SHAPE, lambda: f(h, 0, ("tensor", short_t)), "trapezoid: spacing tensor is smaller than input")
        raises(ERR_UNSUPPORTED, lambda: f(hr, 0), "rmhip_trapz_dim serves it")
    raises(ERR_UNSUPPORTED, lambda: prov.trapz_dim(h, 0), "this entry point takes real tensors")
    assert live(prov) == before
    for x in (h, hr, cs, short_v, short_t):
        prov.free(x)


# ---- polyint --------------------------------------------------------------------------------------------------------------------------------
def test_polyint_orientations_lengths_and_refusals(prov):
    for shape in ((1, 5), (5, 1), (1, 1), (1, 300), (300, 1), (0, 1), (1, 0)):
        z = data(shape, seed=100 + shape[0] + shape[1])
        h = up_c(prov, z)
        check(prov, prov.complex_polyint(h, 2.5), ref.polyint(z, 2.5), ("polyint", shape))
        prov.free(h)
    empty = up_c(prov, np.zeros((0, 1), dtype=np.complex128))
    check(prov, prov.complex_polyint(empty, -0.0), ref.join([-0.0], [0.0]).reshape(1, 1), "the empty polynomial is (constant, +0)")
    m, hr = up_c(prov, data((2, 3), seed=110)), up_r(prov, np.arange(5.0).reshape(1, 5))
    before = live(prov)
    raises(ERR_INVALID, lambda: prov.complex_polyint(m, 1.0), "polyder: coefficient inputs must be vectors")
    raises(ERR_UNSUPPORTED, lambda: prov.complex_polyint(hr, 1.0), "rmhip_polyint serves it")
    raises(ERR_UNSUPPORTED, lambda: prov.polyint(m, 1.0), "this entry point takes real tensors")
    assert live(prov) == before
    for x in (empty, m, hr):
        prov.free(x)


# ---- iir_filter -----------------------------------------------------------------------------------------------------------------------------
def coef(prov, v):
    return prov.upload(np.asarray(v, dtype=np.float64).reshape(1, -1))


def real_bits_equal(prov, h, want_part, what):
    g = prov.download(h)
    w = np.asarray(want_part, dtype=np.float64).ravel(order="F")
    ng, nw = np.isnan(g), np.isnan(w)
    assert g.shape == w.shape and np.array_equal(ng, nw) and np.array_equal(g[~ng].view(np.uint64), w[~nw].view(np.uint64)), what
    prov.free(h)


def run_filter(prov, b, a, z, dim, zi, unit=False, entry=None, sibling=None, what=None):
    """The complex entry point against the per-lane model, and against the REAL entry point run on the real parts and on the imaginary
    parts, each uploaded as a real tensor: bit for bit, output and final state."""
    entry, sibling = entry or prov.complex_iir_filter, sibling or prov.iir_filter
    hb, ha, hz = coef(prov, b), coef(prov, a), up_c(prov, z)
    hzi = None if zi is None else up_c(prov, zi)
    y, zf = entry(hb, ha, hz, dim, hzi, unit)
    wy, wz = ref.iir_filter(b, [1.0] if unit else a, z, dim, zi)
    gy, gz = got(prov, y), got(prov, zf)
    check(prov, y, wy, (what, "output"))
    check(prov, zf, wz, (what, "final state"))
    for part, py, pz in (("real", gy.real, gz.real), ("imag", gy.imag, gz.imag)):
        hx = up_r(prov, getattr(z, part))
        hs = None if zi is None else up_r(prov, getattr(zi, part))
        ry, rz = sibling(hb, ha, hx, dim, hs, unit)
        real_bits_equal(prov, ry, py, (what, part, "output against the real entry point"))
        real_bits_equal(prov, rz, pz, (what, part, "state against the real entry point"))
        for x in (hx, hs):
            if x is not None:
                prov.free(x)
    for x in (hb, ha, hz, hzi):
        if x is not None:
            prov.free(x)


def filter_coefficients(order):
    rng = np.random.default_rng(400 + order)
    if order == 1:
        return np.array([2.5]), np.array([1.25])
    return rng.standard_normal(order), np.concatenate([[1.5], 0.2 * rng.standard_normal(order - 1)])


def state_for(z, dim, S, seed):
    shape = tuple(S if d == dim else s for d, s in enumerate(z.shape))
    return data(shape, seed=seed)


@pytest.mark.parametrize("order", [1, 2, 3, 9])
def test_filter_orders_dimensions_and_initial_states(prov, order):
    b, a = filter_coefficients(order)
    z = data((6, 5, 4), seed=120 + order)
    for dim in (0, 1, 2):
        for with_zi in ((False, True) if order > 1 else (False,)):
            zi = state_for(z, dim, order - 1, 130 + dim) if with_zi else None
            run_filter(prov, b, a, z, dim, zi, what=(order, dim, with_zi))


def test_filter_many_channels_unit_denominator_empty_signal_and_the_fixture(prov):
    b, a = filter_coefficients(3)
    z = data((40, 300), seed=140)
    run_filter(prov, b, a, z, 0, state_for(z, 0, 2, 141), what="300 channels")
    run_filter(prov, b, [2.0], data((6, 5), seed=142), 0, None, unit=True, what="unit denominator")
    # an empty signal hands the initial states on
    zi = data((2, 3), seed=143)
    hb, ha, hz, hzi = coef(prov, b), coef(prov, a), up_c(prov, np.zeros((0, 3), dtype=np.complex128)), up_c(prov, zi)
    y, zf = prov.complex_iir_filter(hb, ha, hz, 0, hzi)
    check(prov, y, np.zeros((0, 3), dtype=np.complex128), "empty output")
    check(prov, zf, zi, "states handed on")
    for x in (hb, ha, hz, hzi):
        prov.free(x)
    c = kat("iir_filter_provider_preserves_complex_storage_and_filters_lanes")
    hb, ha, hz = coef(prov, c["b"]), coef(prov, c["a"]), up_c(prov, ref.from_interleaved(c["data"], c["shape"]))
    y, zf = prov.complex_iir_filter(hb, ha, hz, c["dim"])
    check(prov, y, ref.from_interleaved(c["expect"], c["expect_shape"]), "fixture output")
    check(prov, zf, ref.from_interleaved(c["expect_state"], c["expect_state_shape"]), "fixture state")
    for x in (hb, ha, hz):
        prov.free(x)


def test_filter_declines_and_refusals(prov):
    b, a = filter_coefficients(3)
    hb, ha = coef(prov, b), coef(prov, a)
    long_few = up_c(prov, data((5000, 2), seed=150, special=False))
    z = data((6, 5), seed=151)
    hz, hr, hcb = up_c(prov, z), up_r(prov, z.real), up_c(prov, data((1, 3), seed=152))
    real_zi, short_zi = up_r(prov, np.zeros((2, 5))), up_c(prov, data((3, 5), seed=153))
    before = live(prov)
    for f in (prov.complex_iir_filter, prov.complex_iir_filter_long):
        raises(ERR_UNSUPPORTED, lambda: f(hcb, ha, hz, 0), "iir_filter: complex filter coefficients are not supported")
        raises(ERR_UNSUPPORTED, lambda: f(hb, hcb, hz, 0), "iir_filter: complex filter coefficients are not supported")
        raises(ERR_UNSUPPORTED, lambda: f(hb, ha, hz, 0, real_zi), "iir_filter: initial conditions storage must match the signal")
        raises(ERR_UNSUPPORTED, lambda: f(hb, ha, hr, 0), "rmhip_iir_filter serves it")
        raises(ERR_SHAPE, lambda: f(hb, ha, hz, 0, short_zi), "iir_filter: initial conditions are not compatible with the signal shape")
    # two logical channels on 10000 logical elements: declined as the sibling declines the same real shape, for the long form to take
    raises(ERR_UNSUPPORTED, lambda: prov.complex_iir_filter(hb, ha, long_few, 0), "iir_filter: 2 channels")
    raises(ERR_UNSUPPORTED, lambda: prov.iir_filter(hb, ha, hz, 0), "this entry point takes real tensors")
    assert live(prov) == before
    for x in (hb, ha, long_few, hz, hr, hcb, real_zi, short_zi):
        prov.free(x)


# ---- iir_filter_long ------------------------------------------------------------------------------------------------------------------------
LONG_SHAPES = [((ref.LONG_LEN, ref.LONG_CHANNELS), 0), ((ref.LONG_CHANNELS, ref.LONG_LEN), 1)]


def from_time_major(m, dim):
    return m if dim == 0 else np.ascontiguousarray(m.T)


@pytest.mark.parametrize("shape,dim", LONG_SHAPES, ids=str)
def test_long_fir_equals_the_model_in_value(prov, shape, dim):
    rng = np.random.default_rng(160)
    b = rng.standard_normal(4)
    z = data(shape, seed=161, special=False)
    zi = data(tuple(3 if d == dim else s for d, s in enumerate(shape)), seed=162, special=False)
    hb, ha, hz, hzi = coef(prov, b), coef(prov, [1.0]), up_c(prov, z), up_c(prov, zi)
    for state, h_state in ((None, None), (zi, hzi)):
        y, zf = prov.complex_iir_filter_long(hb, ha, hz, dim, h_state)
        wy, wz = ref.iir_filter(b, [1.0], z, dim, state)
        assert prov.is_complex(y) and prov.is_complex(zf) and tuple(lib_shape(prov, y)) == shape and tuple(lib_shape(prov, zf)) == wz.shape
        assert np.array_equal(got(prov, y), wy) and np.array_equal(got(prov, zf), wz), (shape, state is None)
        prov.free(y), prov.free(zf)
    for x in (hb, ha, hz, hzi):
        prov.free(x)


@pytest.mark.parametrize("shape,dim", LONG_SHAPES, ids=str)
@pytest.mark.parametrize("name", ref.LONG_FILTERS)
def test_long_recursive_filters_hold_the_contract_per_lane(prov, name, shape, dim):
    if not longdouble_is_wide():
        pytest.skip("np.longdouble carries fewer than 63 mantissa bits")
    b, a = FILTERS[name]
    zt, st = ref.long_signal(name)
    hb, ha, hz, hzi = coef(prov, b), coef(prov, a), up_c(prov, from_time_major(zt, dim)), up_c(prov, from_time_major(st, dim))
    y, zf = prov.complex_iir_filter_long(hb, ha, hz, dim, hzi)
    assert prov.is_complex(y) and prov.is_complex(zf) and tuple(lib_shape(prov, y)) == shape
    gy, gz = got(prov, y), got(prov, zf)
    gy, gz = (gy, gz) if dim == 0 else (gy.T, gz.T)
    bn, an = normalise(b, a)
    for part in ("real", "imag"):
        x, s0 = np.ascontiguousarray(getattr(zt, part)), np.ascontiguousarray(getattr(st, part))
        y_ref, zf_ref = df2t(bn, an, x, s0)
        y_exact, zf_exact = exact_filter(b, a, x, s0)
        floor = noise_floor(b, a, x)
        out_err, st_err = float(np.max(np.abs(getattr(gy, part) - y_exact))), float(np.max(np.abs(getattr(gz, part) - zf_exact)))
        out_bound, st_bound = output_bound(y_ref, y_exact, floor), state_bound(zf_ref, zf_exact, b, a, floor)
        print(f"{name} {shape} {part}: output {out_err / (out_bound / 8):.2f} of 8, state {st_err / (st_bound / 16):.2f} of 16")
        assert out_err <= out_bound, (name, part, out_err, out_bound)
        assert st_err <= st_bound, (name, part, st_err, st_bound)
    for x in (y, zf, hb, ha, hz, hzi):
        prov.free(x)


def test_long_short_signals_and_declines(prov):
    b, a = filter_coefficients(3)
    z = data((400, 2), seed=170)  # fewer than 512 logical samples: the bit-exact sequential form
    run_filter(prov, b, a, z, 0, state_for(z, 0, 2, 171), entry=prov.complex_iir_filter_long, sibling=prov.iir_filter_long, what="400 samples")
    rb, ra = FILTERS["double_pole_0.9"]
    hb, ha = coef(prov, rb), coef(prov, ra)
    bad = np.array(data((5000, 2), seed=172, special=False))
    bad[4321, 1] = complex(bad[4321, 1].real, np.inf)
    hbad = up_c(prov, bad)
    ub, ua = coef(prov, UNSTABLE[0]), coef(prov, UNSTABLE[1])
    ones = up_c(prov, np.ones((16500, 1), dtype=np.complex128))
    before = live(prov)
    raises(ERR_UNSUPPORTED, lambda: prov.complex_iir_filter_long(hb, ha, hbad, 0), "iir_filter: a non-finite value in the signal, the initial states or the result")
    raises(ERR_UNSUPPORTED, lambda: prov.complex_iir_filter_long(ub, ua, ones, 0), "iir_filter: filter is not contractive over a chunk")
    assert live(prov) == before
    for x in (hb, ha, hbad, ub, ua, ones):
        prov.free(x)


# ---- precision 32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def f32r(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def check32(p, h, model, what):
    """Each part is the f64 model's result rounded through f32, held in 2 x f64 storage."""
    assert p.is_complex(h), what
    raw = p.download(h)
    assert raw.dtype == np.complex128 and raw.size == model.size, what
    check(p, h, ref.round_f32(model), what)


def test_precision_32_gradient(prov32):
    z, coords = data((5, 4, 3), seed=180, f32=True), f32r(np.cumsum(np.random.default_rng(181).uniform(0.3, 1.7, 4)))
    h, hc = up_c(prov32, z), up_r(prov32, coords)
    check32(prov32, prov32.complex_gradient_dim(h, 0, 0.7), ref.gradient(z, 0, 0.7), "gradient")
    check32(prov32, prov32.complex_gradient_dim_with_coordinates(h, 1, hc), ref.gradient(z, 1, coordinates=coords), "gradient with coordinates")
    prov32.free(h), prov32.free(hc)


def test_precision_32_trapezoid(prov32):
    """One term per line (an extent of two), so the sum is the term and the one rounding through f32 is the whole difference; the terms
    themselves, 0.05 * (x0 + x1), are not representable in f32 - an intermediate rounded through f32 would show."""
    z = data((2, 5, 3), seed=182, f32=True)
    h = up_c(prov32, z)
    check32(prov32, prov32.complex_trapz_dim(h, 0, 0.1), ref.trapz(z, 0, 1, 0.1)[0], "trapz")
    check32(prov32, prov32.complex_cumtrapz_dim(h, 0, 0.1), ref.trapz(z, 0, 1, 0.1, True)[0], "cumtrapz")
    zi = data((300, 3), seed=183, ints=True)  # integers with a spacing of 0.5: exact terms and sums in any order, f32-representable
    hi = up_c(prov32, zi)
    check32(prov32, prov32.complex_cumtrapz_dim(hi, 0, 0.5), ref.trapz(zi, 0, 1, 0.5, True)[0], "cumtrapz of integers")
    prov32.free(h), prov32.free(hi)


def test_precision_32_polyint(prov32):
    z = data((1, 7), seed=184, f32=True)
    h = up_c(prov32, z)
    check32(prov32, prov32.complex_polyint(h, 0.1), ref.polyint(z, 0.1), "polyint")
    prov32.free(h)


def test_precision_32_filters(prov32):
    b, a = f32r([0.3, 0.2, 0.1]), f32r([1.0, -0.5, 0.25])
    z = data((6, 5), seed=185, f32=True)
    zi = data((2, 5), seed=186, f32=True)
    hb, ha, hz, hzi = coef(prov32, b), coef(prov32, a), up_c(prov32, z), up_c(prov32, zi)
    wy, wz = ref.iir_filter(b, a, z, 0, zi)  # the recurrence runs in f64 from end to end; only the stored results are rounded
    for f in (prov32.complex_iir_filter, prov32.complex_iir_filter_long):
        y, zf = f(hb, ha, hz, 0, hzi)
        check32(prov32, y, wy, "filter output")
        check32(prov32, zf, wz, "filter state")
    # the long form's FIR regime: equal in value to the f64 model rounded through f32
    zl = data((5000, 2), seed=187, f32=True)
    hl, one = up_c(prov32, zl), coef(prov32, [1.0])
    y, zf = prov32.complex_iir_filter_long(hb, one, hl, 0)
    wy, wz = ref.iir_filter(b, [1.0], zl, 0)
    assert prov32.is_complex(y) and np.array_equal(got(prov32, y), ref.round_f32(wy)) and np.array_equal(got(prov32, zf), ref.round_f32(wz))
    for x in (y, zf, hb, ha, hz, hzi, hl, one):
        prov32.free(x)
