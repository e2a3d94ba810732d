"""GPU checks of `iir_filter_long` (rmhip_iir_filter_long, signal_ops.hip): filter(b, a, x) on long signals with few channels.

Recursive filters run a chunked scan and are held to the accuracy contract of include/rmhip.h - with `exact` the sequential recurrence in
np.longdouble, `ref` the oracle's f64 loop and floor = order * 2^-52 * max_n sum_m |g[m]| |x[n - m]|:
    max |y - exact|  <=  8 * max(max |ref - exact|, floor),      max |zf - exact| <= 16 * max(max |ref - exact|, (sum|b| + sum|a|) * floor).
FIR filters equal the oracle in value, short and degenerate requests are bit-identical to `iir_filter` / the oracle, and every decline
raises and leaves the provider serving."""
import numpy as np
import pytest

from iir_long_ref import (FILTERS, UNSTABLE, df2t, exact_filter, exact_states_at, longdouble_is_wide, noise_floor, normalise, oracle_fir_folded, output_bound,
                          state_bound)

pytestmark = pytest.mark.gpu

RECURSIVE_SHAPES = [((20001, 1), 0), ((1, 20001), 1), ((3, 9000, 2), 1), ((9000, 5), 0)]
_REFS = {}


def bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def up(prov, v, shape=None):
    v = np.asarray(v, dtype=np.float64)
    return prov.upload(v.ravel(order="F"), list(v.shape if shape is None else shape))


def coef(prov, v):
    return prov.upload(np.asarray(v, dtype=np.float64).reshape(1, -1))


def time_major(v, dim, n):
    """shape -> (n, channels), the channels in the order of the leading then the trailing dimensions"""
    return np.moveaxis(v, dim, 0).reshape(n, -1)


def from_time_major(m, shape, dim):
    rest = [s for d, s in enumerate(shape) if d != dim]
    return np.moveaxis(m.reshape([m.shape[0]] + rest), 0, dim)


def need_longdouble():
    if not longdouble_is_wide():
        pytest.skip("np.longdouble carries fewer than 63 mantissa bits")


def references(oracle, key, b, a, n, channels, with_zi, scale=1.0):
    """Shared, never modified: signal (n x channels), zi, the oracle's and the exact results and the two bounds."""
    k = (key, n, channels, with_zi)
    if k not in _REFS:
        rng = np.random.default_rng(n * 31 + channels)
        X = rng.standard_normal((n, channels)) * scale
        S = max(len(b), len(a)) - 1
        Z = rng.standard_normal((S, channels)) if with_zi else None
        y_ref, zf_ref = oracle.iir_filter(b, a, X, 0, Z)
        y_exact, zf_exact = exact_filter(b, a, X, Z)
        floor = noise_floor(b, a, X)
        _REFS[k] = dict(X=X, Z=Z, y_exact=y_exact, zf_exact=zf_exact, out_bound=output_bound(y_ref, y_exact, floor),
                        st_bound=state_bound(zf_ref, zf_exact, b, a, floor))
        for v in _REFS[k].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REFS[k]


def run_against_contract(prov, oracle, key, b, a, shape, dim, with_zi, entry=None):
    n = shape[dim]
    channels = int(np.prod(shape)) // n
    R = references(oracle, key, b, a, n, channels, with_zi)
    x = from_time_major(R["X"], shape, dim)
    S = max(len(b), len(a)) - 1
    zshape = [S if d == dim else s for d, s in enumerate(shape)]
    hz = up(prov, from_time_major(R["Z"], zshape, dim)) if with_zi else None
    y, zf = (entry or prov.iir_filter_long)(coef(prov, b), coef(prov, a), up(prov, x), dim, hz)
    assert list(y.shape) == list(shape) and list(zf.shape) == zshape
    got_y = time_major(prov.download(y).reshape(shape, order="F"), dim, n)
    got_z = time_major(prov.download(zf).reshape(zshape, order="F"), dim, S)
    out_err, st_err = float(np.max(np.abs(got_y - R["y_exact"]))), float(np.max(np.abs(got_z - R["zf_exact"])))
    print(f"{key} {shape} dim {dim} zi {with_zi}: output {out_err / (R['out_bound'] / 8):.2f} of 8, state {st_err / (R['st_bound'] / 16):.2f} of 16")
    assert out_err <= R["out_bound"], (key, shape, with_zi, out_err, R["out_bound"])
    assert st_err <= R["st_bound"], (key, shape, with_zi, st_err, R["st_bound"])
    for h in (y, zf):
        prov.free(h)


@pytest.mark.parametrize("shape,dim", RECURSIVE_SHAPES, ids=str)
@pytest.mark.parametrize("name", list(FILTERS))
def test_recursive_filters_hold_both_bounds(prov, oracle, name, shape, dim):
    need_longdouble()
    b, a = FILTERS[name]
    for with_zi in (False, True):
        run_against_contract(prov, oracle, name, b, a, shape, dim, with_zi)


def test_denominator_is_normalised_by_a1(prov, oracle):
    need_longdouble()
    b, a = FILTERS["double_pole_0.9"]
    run_against_contract(prov, oracle, "a1=2", 2.0 * b, 2.0 * a, (20001, 1), 0, True)
    # the same request through the two scalings: the normalised coefficients are the same numbers, so are the results
    x = up(prov, references(oracle, "a1=2", 2.0 * b, 2.0 * a, 20001, 1, True)["X"])
    y1, z1 = prov.iir_filter_long(coef(prov, b), coef(prov, a), x, 0)
    y2, z2 = prov.iir_filter_long(coef(prov, 2.0 * b), coef(prov, 2.0 * a), x, 0)
    assert np.array_equal(normalise(b, a)[0], normalise(2.0 * b, 2.0 * a)[0]) and np.array_equal(normalise(b, a)[1], normalise(2.0 * b, 2.0 * a)[1])
    assert bits_equal(prov.download(y1), prov.download(y2)) and bits_equal(prov.download(z1), prov.download(z2))


def test_order_64_tables(prov, oracle):
    need_longdouble()
    b = np.random.default_rng(64).standard_normal(64)
    run_against_contract(prov, oracle, "64_over_2", b, np.array([1.0, -0.9]), (20001, 1), 0, True)  # S = 63: every lane but one holds a row of T


@pytest.mark.parametrize("shape,dim", [((100000, 1), 0), ((7, 5000), 1)], ids=str)
@pytest.mark.parametrize("taps", [2, 12, 64])
def test_fir_equals_the_oracle(prov, oracle, taps, shape, dim):
    rng = np.random.default_rng(taps + shape[0])
    b, a = rng.standard_normal(taps), np.array([1.0])
    x = rng.standard_normal(shape)
    zshape = [taps - 1 if d == dim else s for d, s in enumerate(shape)]
    zi = rng.standard_normal(zshape)
    hb, ha, hx = coef(prov, b), coef(prov, a), up(prov, x)
    for z in (None, zi):
        if shape[1] == 1:
            wy, wz = oracle_fir_folded(oracle.iir_filter, b, a, x[:, 0], None if z is None else z[:, 0])
            wy, wz = wy.reshape(shape), wz.reshape(zshape)
            head = oracle.iir_filter(b, a, x[:2000], 0, None if z is None else z)[0]
            assert np.array_equal(wy[:2000], head)  # the folded run is the oracle's loop
        else:
            wy, wz = oracle.iir_filter(b, a, x, dim, z)
        runs = [prov.iir_filter_long(hb, ha, hx, dim, None if z is None else up(prov, z))]
        if z is None:
            runs.append(prov.iir_filter_long(hb, ha, hx, dim, unit_denominator=True))
            runs.append(prov.iir_filter_long(coef(prov, 2.0 * b), coef(prov, [2.0, 0.0, 0.0]), hx, dim) if taps > 2 else runs[0])  # zero denominator taps
        for y, zf in runs:
            assert list(y.shape) == list(shape) and list(zf.shape) == zshape
            assert np.array_equal(prov.download(y).reshape(shape, order="F"), wy), (taps, shape, z is None)
            assert np.array_equal(prov.download(zf).reshape(zshape, order="F"), wz), (taps, shape, z is None)


def test_short_and_degenerate_requests_are_bit_identical(prov, oracle):
    rng = np.random.default_rng(3)
    b, a = [0.2, 0.3, 0.1], [1.0, -0.5, 0.25]
    hb, ha = coef(prov, b), coef(prov, a)
    for shape, dim in (((5,), 0), ((300, 1), 0), ((40, 7, 3), 1)):  # iir_filter serves these
        x = rng.standard_normal(shape)
        zshape = [2 if d == dim else s for d, s in enumerate(shape)]
        for z in (None, rng.standard_normal(zshape)):
            hz = None if z is None else up(prov, z)
            y0, z0 = prov.iir_filter(hb, ha, up(prov, x), dim, hz)
            y1, z1 = prov.iir_filter_long(hb, ha, up(prov, x), dim, hz)
            wy, wz = oracle.iir_filter(b, a, x, dim, z)
            assert list(y1.shape) == list(y0.shape) and list(z1.shape) == list(z0.shape)
            assert bits_equal(prov.download(y1), prov.download(y0)) and bits_equal(prov.download(z1), prov.download(z0))
            assert bits_equal(prov.download(y1).reshape(shape, order="F"), wy)
    # an empty signal hands the initial states on
    zi = rng.standard_normal((2, 3))
    y0, z0 = prov.iir_filter(hb, ha, prov.upload(np.zeros(0), [0, 3]), 0, up(prov, zi))
    y1, z1 = prov.iir_filter_long(hb, ha, prov.upload(np.zeros(0), [0, 3]), 0, up(prov, zi))
    assert list(y1.shape) == [0, 3] == list(y0.shape) and bits_equal(prov.download(z1), prov.download(z0)) and bits_equal(prov.download(z1), zi.ravel(order="F"))
    # no states: a gain, whatever the length
    x = rng.standard_normal((100000, 1))
    hg, hd = coef(prov, [3.0]), coef(prov, [1.5])
    y0, z0 = prov.iir_filter(hg, hd, up(prov, x), 0)
    y1, z1 = prov.iir_filter_long(hg, hd, up(prov, x), 0)
    assert list(z1.shape) == list(z0.shape) == [0, 1] and bits_equal(prov.download(y1), prov.download(y0))
    assert bits_equal(prov.download(y1).reshape(x.shape, order="F"), oracle.iir_filter([3.0], [1.5], x, 0)[0])
    # short, but a shape iir_filter declines (20 channels, more than 4096 elements): the sequential recurrence, bit-identical to the oracle
    x = rng.standard_normal((400, 20))
    zi = rng.standard_normal((2, 20))
    with pytest.raises(Exception):
        prov.iir_filter(hb, ha, up(prov, x), 0)
    y1, z1 = prov.iir_filter_long(hb, ha, up(prov, x), 0, up(prov, zi))
    wy, wz = oracle.iir_filter(b, a, x, 0, zi)
    assert bits_equal(prov.download(y1).reshape(x.shape, order="F"), wy) and bits_equal(prov.download(z1).reshape(wz.shape, order="F"), wz)
    # long enough for two chunks of 256, too short for two of the first admissible length: the sequential recurrence again
    b2, a2 = FILTERS["double_pole_0.995"]
    x = rng.standard_normal((600, 1))
    y1, z1 = prov.iir_filter_long(coef(prov, b2), coef(prov, a2), up(prov, x), 0)
    wy, wz = oracle.iir_filter(b2, a2, x, 0)
    assert bits_equal(prov.download(y1).reshape(x.shape, order="F"), wy) and bits_equal(prov.download(z1).reshape(wz.shape, order="F"), wz)


@pytest.mark.parametrize("name", ["double_pole_0.9", "random_12_10"])
def test_agrees_with_iir_filter_where_both_serve(prov, oracle, name):
    need_longdouble()
    b, a = FILTERS[name]
    shape = (4096, 300)
    run_against_contract(prov, oracle, name, b, a, shape, 0, True, entry=prov.iir_filter)       # the old entry is the oracle's loop: ratio <= 1
    run_against_contract(prov, oracle, name, b, a, shape, 0, True)
    R = references(oracle, name, b, a, 4096, 300, True)
    args = (coef(prov, b), coef(prov, a), up(prov, R["X"]), 0, up(prov, R["Z"]))
    old, new = prov.iir_filter(*args), prov.iir_filter_long(*args)
    for h_old, h_new, bound in ((old[0], new[0], R["out_bound"]), (old[1], new[1], R["st_bound"])):
        assert np.max(np.abs(prov.download(h_old) - prov.download(h_new))) <= 2.0 * bound  # both within `bound` of the exact result


def test_declines_raise_and_the_next_call_is_served(prov, oracle):
    from runmat_amd import _lib
    from runmat_amd.provider import ProviderError

    rng = np.random.default_rng(11)
    b, a = FILTERS["double_pole_0.9"]
    hb, ha = coef(prov, b), coef(prov, a)
    x = rng.standard_normal((20001, 1))
    hx = up(prov, x)
    good_b, good_a, good_x = [0.2, 0.3, 0.1], [1.0, -0.5, 0.25], rng.standard_normal((5,))
    want = oracle.iir_filter(good_b, good_a, good_x, 0)[0]

    def declined(code, *args, **kw):
        with pytest.raises(ProviderError) as e:
            prov.iir_filter_long(*args, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
        y, _ = prov.iir_filter_long(coef(prov, good_b), coef(prov, good_a), up(prov, good_x), 0)  # ... and the next call is served
        assert bits_equal(prov.download(y), want)
        y, zf = prov.iir_filter_long(hb, ha, hx, 0)
        assert np.all(np.isfinite(prov.download(y))) and np.all(np.isfinite(prov.download(zf)))
        prov.free(y), prov.free(zf)

    declined(_lib.ERR_UNSUPPORTED, coef(prov, UNSTABLE[0]), coef(prov, UNSTABLE[1]), up(prov, np.ones((20001, 1))), 0)  # not contractive over a chunk
    bad = x.copy()
    bad[12345, 0] = np.nan
    declined(_lib.ERR_UNSUPPORTED, hb, ha, up(prov, bad), 0)
    declined(_lib.ERR_UNSUPPORTED, coef(prov, [1.0, 0.5, 0.25]), coef(prov, [1.0]), up(prov, bad), 0)                   # FIR, NaN in x
    declined(_lib.ERR_UNSUPPORTED, hb, ha, hx, 0, up(prov, np.array([[np.inf], [0.0]])))
    declined(_lib.ERR_UNSUPPORTED, coef(prov, [1e308]), coef(prov, [1.0, -0.5]), up(prov, np.full((20001, 1), 10.0)), 0)  # the output overflows
    declined(_lib.ERR_UNSUPPORTED, coef(prov, np.ones(65)), coef(prov, [1.0]), hx, 0)                                     # order 65
    declined(_lib.ERR_UNSUPPORTED, hb, ha, prov.complex_from_real(hx), 0)
    declined(_lib.ERR_INVALID, hb, coef(prov, [0.0, 1.0]), hx, 0)                                                       # a(1) == 0
    declined(_lib.ERR_SHAPE, hb, ha, hx, 0, up(prov, np.zeros((3, 1))))                                                 # two states per channel expected


def test_iir_filter_itself_still_declines_one_long_channel(prov):
    with pytest.raises(Exception):
        prov.iir_filter(coef(prov, [0.1, 0.2]), coef(prov, [1.0, -0.3]), prov.upload(np.zeros((100000, 1))), 0)


def test_a_million_samples(prov, oracle):
    """2^20 samples, double pole at 0.995: the first and the last 4096 samples against the contract's bounds computed on those windows, the
    exact run carried through the whole signal (the oracle's loop enters the last window from the exact state, rounded)."""
    need_longdouble()
    b, a = FILTERS["double_pole_0.995"]
    n, w = 1 << 20, 4096
    x = np.random.default_rng(20).standard_normal(n)
    y, zf = prov.iir_filter_long(coef(prov, b), coef(prov, a), up(prov, x.reshape(n, 1)), 0)
    got_y, got_z = prov.download(y), prov.download(zf)
    entering = exact_states_at(b, a, x, [n - w, n])
    history = 1 << 15  # the impulse response has decayed below 1e-60 of its peak by then: the floor of the last window needs no more
    for lo, state in ((0, None), (n - w, entering[n - w])):
        win = x[lo:lo + w]
        zi = None if state is None else state.astype(np.float64)
        y_ref, zf_ref = oracle.iir_filter(b, a, win, 0, zi)
        bn, an = normalise(b, a)
        y_exact, zf_exact = exact_filter(b, a, win) if state is None else df2t(bn.astype(np.longdouble), an.astype(np.longdouble),
                                                                               win.astype(np.longdouble), state)
        floor = noise_floor(b, a, x[max(0, lo - history):lo + w], last=w)
        out_err = float(np.max(np.abs(got_y[lo:lo + w] - y_exact)))
        print(f"window at {lo}: output {out_err / (output_bound(y_ref, y_exact, floor) / 8):.2f} of 8")
        assert out_err <= output_bound(y_ref, y_exact, floor), (lo, out_err)
        if lo:
            st_err = float(np.max(np.abs(got_z - zf_exact)))
            assert np.array_equal(zf_exact, entering[n])
            print(f"final state {st_err / (state_bound(zf_ref, zf_exact, b, a, floor) / 16):.2f} of 16")
            assert st_err <= state_bound(zf_ref, zf_exact, b, a, floor), st_err
