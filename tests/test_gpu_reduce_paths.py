"""Every kernel path of the ahead-of-time reductions against exact sums, products and extrema.

`rmhip_reduce` (sum, mean, min, max, prod; both NaN modes), `rmhip_reduce_nd` and `rmhip_dot` take one of seven kernels and one of two
finalizes (reduce_plan.h route_reduction).  The shape table of tests/reduce_ref.py reaches each combination - tests/cpp/reduce_route_check.cpp
pins that on the host - and every row runs here on the f64 provider and on a precision-32 provider, with the two data classes of
reduce_ref.py: `exact` (any association order gives the same bits: bit equality) and `rounded` (bounds that hold for any order,
compared in exact arithmetic).  min / max must also agree bit for bit with rmhip_reduce_minmax_dim and the oracle, signed zeros and
infinities included.  Each rounded test prints its largest error as a fraction of the bound (`ratio ...` lines, pytest -s).

What a slice with nothing to reduce gives is the CPU builtins' answer, not the kernels': sum 0 (sum.rs:1055-1076: `saw_value` false),
prod 1 (prod.rs:963-984), mean NaN (mean.rs:1203-1206 for an empty tensor, :1252-1258 for a count of 0, :1131-1133 for all elements),
min / max NaN for a slice of NaNs in omit mode (min.rs:1065-1068, the same lines in max.rs:1261-1264).  For an EMPTY tensor the CPU's
min / max return an empty result (min.rs:996-1006), which rmhip_reduce's output shape cannot express: include/rmhip.h states NaN, and
that sentence is what test_empty_reduced_extent holds min / max to.
"""
import numpy as np
import pytest

import reduce_ref as R
from runmat_amd._lib import ERR_INVALID
from runmat_amd.provider import ProviderError

pytestmark = pytest.mark.gpu

OPS = ("sum", "mean", "min", "max", "prod")


@pytest.fixture(scope="module")
def prov32(built):
    import os
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


@pytest.fixture(params=["f64", "f32"])
def pv(request, prov):
    """(provider, is precision 32)"""
    return (prov, False) if request.param == "f64" else (request.getfixturevalue("prov32"), True)


def narrow(x, f32):
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if f32 else x


def same(got, want):
    """equal bits, NaNs matching NaNs whatever their payload"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    m = ~np.isnan(want)
    return np.array_equal(got[m].view(np.uint64), want[m].view(np.uint64))


def where_differs(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(~((got == want) & (np.signbit(got) == np.signbit(want)) | (np.isnan(got) & np.isnan(want))))
    return [(int(k), float(got[k]), float(want[k])) for k in bad[:5]], len(bad)


def reduce(p, f32, op, h, shape, dim, omit):
    out = p._reduce(op, h, dim, omit)
    assert out.shape == R.out_shape(shape, dim), (op, shape, dim, out.shape)
    if f32:
        assert p.buffer_bits(out) == 32
    got = p.download(out)
    p.free(out)
    return got


def upload(p, s2, row, shape):
    return p.upload(R.unslice(s2, *row[:3]), shape)


def ref_minmax(oracle, s2, row, shape, dim):
    """{(is_max, omit): the oracle's values in slice order}"""
    x = R.unslice(s2, *row[:3]).reshape(shape, order="F")
    return {(is_max, omit): oracle.minmax_dim(x, None if dim < 0 else dim, is_max, omit)[0].reshape(-1, order="F")
            for is_max in (False, True) for omit in (False, True)}


# ---- the exact class: every op, both modes, every NaN placement, bit equality -------------------------------------------------------
@pytest.mark.parametrize("row", R.ROUTE_TABLE, ids=R.row_id)
def test_exact_class_bits(pv, oracle, row):
    p, f32 = pv
    pre, red, post, kernel, nsplit, _ = row
    n = pre * red * post
    shape, dim = R.realise(pre, red, post)
    rng = np.random.default_rng(n + 17)
    base_s = R.slices(R.exact_sum_data(rng, n), pre, red, post)
    base_p = R.slices(R.exact_prod_data(rng, n), pre, red, post)
    for how in R.PLACEMENTS:
        s2, p2 = R.place_nans(base_s, how, nsplit, kernel), R.place_nans(base_p, how, nsplit, kernel)
        nan = np.isnan(s2)
        has_nan, counts = nan.any(axis=1), (~nan).sum(axis=1)
        tot = np.where(nan, 0.0, s2).astype(np.int64).sum(axis=1).astype(np.float64)  # |sum| < 2^43: exact
        with np.errstate(invalid="ignore", divide="ignore"):
            want = {("sum", True): tot, ("sum", False): np.where(has_nan, np.nan, tot),
                    ("mean", True): np.where(counts > 0, tot / counts, np.nan), ("mean", False): np.where(has_nan, np.nan, tot / red)}
        prods = R.exact_class_prods(p2)
        want[("prod", True)], want[("prod", False)] = prods, np.where(has_nan, np.nan, prods)
        for (is_max, omit), v in ref_minmax(oracle, s2, row, shape, dim).items():
            want[("max" if is_max else "min", omit)] = v
        hs, hp = upload(p, s2, row, shape), upload(p, p2, row, shape)
        for op in OPS:
            for omit in (False, True):
                got = reduce(p, f32, op, hp if op == "prod" else hs, shape, dim, omit)
                assert same(got, narrow(want[(op, omit)], f32)), (row, how, op, omit, where_differs(got, narrow(want[(op, omit)], f32)))
        if how == "whole":  # nothing left in omit mode: the CPU builtins' values (module docstring)
            k = 0 if pre * post == 1 else 1
            assert counts[k] == 0 and want[("sum", True)][k] == 0.0 and want[("prod", True)][k] == 1.0
            assert np.isnan(want[("mean", True)][k]) and np.isnan(want[("min", True)][k]) and np.isnan(want[("max", True)][k])
        p.free(hs)
        p.free(hp)


# ---- the rounded class: sum, mean, prod within bounds that hold for any association order -----------------------------------------
@pytest.mark.parametrize("row", R.ROUNDED_ROWS, ids=R.row_id)
def test_rounded_class_bounds(pv, row):
    p, f32 = pv
    pre, red, post, kernel, nsplit, _ = row
    n = pre * red * post
    shape, dim = R.realise(pre, red, post)
    rng = np.random.default_rng(n + 29)
    base_s = R.slices(narrow(R.rounded_sum_data(rng, n), f32), pre, red, post)
    base_p = R.slices(narrow(R.rounded_prod_data(rng, n), f32), pre, red, post)
    worst = {"sum": 0.0, "mean": 0.0, "prod": 0.0}
    for how in ("none", "boundary"):
        s2, p2 = R.place_nans(base_s, how, nsplit, kernel), R.place_nans(base_p, how, nsplit, kernel)
        has_nan = np.isnan(s2).any(axis=1)
        sums, counts = R.exact_sums(s2)
        sabs, _ = R.exact_sums(s2, absolute=True)
        prods = R.exact_prods(p2)
        hs, hp = upload(p, s2, row, shape), upload(p, p2, row, shape)
        for omit in (False, True):
            live = np.ones(len(has_nan), dtype=bool) if omit else ~has_nan  # include mode: NaN exactly where a NaN sits
            got = {op: reduce(p, f32, op, hp if op == "prod" else hs, shape, dim, omit) for op in ("sum", "mean", "prod")}
            lm = live & (counts > 0)  # omit mode with nothing left: NaN (mean.rs:1252-1258)
            for op in got:
                assert np.array_equal(np.isnan(got[op]), ~(lm if op == "mean" else live)), (row, how, op, omit)
            bs = R.sum_bound(red, sabs[live])
            ok, ratio = R.error_ratios(got["sum"][live], sums[live], R.f32_bound(bs, sums[live]) if f32 else bs)
            worst["sum"] = max(worst["sum"], ratio.max(initial=0.0))
            assert ok.all(), (row, how, "sum", omit, float(ratio.max()))
            c = counts[lm] if omit else np.full(int(lm.sum()), red)
            means = sums[lm].over(c)
            bm = R.mean_bound(red, sabs[lm], sums[lm], c)
            ok, ratio = R.error_ratios(got["mean"][lm], means, R.f32_bound(bm, means) if f32 else bm)
            worst["mean"] = max(worst["mean"], ratio.max(initial=0.0))
            assert ok.all(), (row, how, "mean", omit, float(ratio.max()))
            ok, ratio = R.prod_error_ratios(got["prod"][live], [q for q, keep in zip(prods, live) if keep], red, f32)
            worst["prod"] = max(worst["prod"], ratio.max(initial=0.0))
            assert ok.all(), (row, how, "prod", omit, float(ratio.max()))
        p.free(hs)
        p.free(hp)
    for op, w in worst.items():
        print(f"ratio {op} {'f32' if f32 else 'f64'} {R.row_id(row)} {w:.4f}")


# ---- min / max: rmhip_reduce, rmhip_reduce_minmax_dim and the oracle agree bit for bit ----------------------------------------------
def _zeros_data(rng, nslices, red, nsplit, kernel):
    """positive values with zeros of both signs as the minima: +0 and -0 at the two ends of a slice (which end has which sign alternates
    from slice to slice), at the chunk boundaries, and sprinkled at random - different lanes, waves and chunks see different zeros"""
    s2 = np.abs(rng.standard_normal((nslices, red))) + 0.5
    z = rng.random((nslices, red)) < min(0.5, 4.0 / red)
    s2[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    for k, col in enumerate([0] + R.boundary_indices(red, nsplit, kernel) + [red - 1]):
        s2[0::2, col] = 0.0 if k % 2 == 0 else -0.0
        s2[1::2, col] = -0.0 if k % 2 == 0 else 0.0
    s2[nslices // 2, :] = np.abs(s2[nslices // 2, :])  # one slice without a negative zero
    return s2


def _inf_data(rng, nslices, red):
    s2 = rng.standard_normal((nslices, red))
    at = rng.random((nslices, red)) < min(0.3, 2.0 / red)
    s2[at] = np.where(rng.random(int(at.sum())) < 0.5, np.inf, -np.inf)
    if nslices >= 3:
        s2[1, :], s2[2, :] = np.inf, -np.inf  # max of all -inf is the identity of the accumulator itself
    else:
        s2[0, :] = np.inf if red % 2 else -np.inf
    return s2


@pytest.mark.parametrize("row", R.ROUTE_TABLE, ids=R.row_id)
def test_minmax_consistency(pv, oracle, row):
    p, f32 = pv
    pre, red, post, kernel, nsplit, _ = row
    shape, dim = R.realise(pre, red, post)
    rng = np.random.default_rng(pre * red * post + 41)
    zeros = narrow(_zeros_data(rng, pre * post, red, nsplit, kernel), f32)
    infs = narrow(_inf_data(rng, pre * post, red), f32)
    with_nan = R.place_nans(infs, "first", nsplit, kernel)
    for name, s2 in (("zeros", zeros), ("-zeros", -zeros), ("inf", infs), ("-inf", -infs), ("inf+nan", with_nan)):
        h = upload(p, s2, row, shape)
        wants = ref_minmax(oracle, s2, row, shape, dim)
        for is_max in (False, True):
            for omit in (False, True):
                want = wants[(is_max, omit)]
                got = reduce(p, f32, "max" if is_max else "min", h, shape, dim, omit)
                r = p._reduce_minmax_dim("max" if is_max else "min", h, max(dim, 0), omit)  # (red, 1) along dim 0 is the all-elements view
                got_dim = p.download(r.values)
                p.free(r.values)
                p.free(r.indices)
                assert same(got, want), (row, name, is_max, omit, where_differs(got, want))
                assert same(got_dim, want), (row, name, is_max, omit, "minmax_dim", where_differs(got_dim, want))
        p.free(h)


# ---- computed non-finite values and the sign of a zero product --------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in R.ROUTE_TABLE if r[:3] in ((1, 5, 1), (1, 6000, 1), (1, 6001, 2), (7, 5000, 1), (512, 600, 1),
                                                                     (513, 600, 1), (1, 255, 1030), (255, 40, 70))], ids=R.row_id)
def test_computed_nonfinite(pv, row):
    p, f32 = pv
    pre, red, post, kernel, nsplit, _ = row
    shape, dim = R.realise(pre, red, post)
    ns = pre * post
    first, last = 0, red - 1  # different chunks wherever the row is split
    hit = ns // 2

    def run(op, s2, omit):
        h = upload(p, s2, row, shape)
        got = reduce(p, f32, op, h, shape, dim, omit)
        p.free(h)
        return got

    for omit in (False, True):
        s2 = np.ones((ns, red))
        s2[hit, first], s2[hit, last] = np.inf, -np.inf
        for op, clean in (("sum", float(red)), ("mean", 1.0)):  # inf - inf is computed, not met: NaN in both modes
            got = run(op, s2, omit)
            assert np.isnan(got[hit]) and np.all(np.delete(got, hit) == clean), (row, op, omit)
        for a, b in ((np.inf, 0.0), (0.0, np.inf), (-np.inf, -0.0)):
            s2 = np.ones((ns, red))
            s2[hit, first], s2[hit, last] = a, b
            got = run("prod", s2, omit)
            assert np.isnan(got[hit]) and np.all(np.delete(got, hit) == 1.0), (row, a, b, omit)
        for zero in (0.0, -0.0):  # the sign of a zero product is the parity of the negative factors, whatever the order
            s2 = -np.ones((ns, red))
            s2[:, first::3] = 1.0
            s2[hit, last] = zero
            s2[(hit + 1) % ns, first] = zero
            got = run("prod", s2, omit)
            want = np.where((np.signbit(s2).sum(axis=1) & 1) == 1, -1.0, 1.0) * np.where((s2 == 0).any(axis=1), 0.0, 1.0)
            assert same(got, want), (row, zero, omit, where_differs(got, want))


def test_empty_reduced_extent(pv):
    """extent 0 along the reduced dim: sum 0, prod 1, mean NaN for every output slice (module docstring), in both modes, on the
    contiguous, the generic strided and the 16-byte strided route"""
    p, f32 = pv
    for shape, dim in (((0, 4), 0), ((3, 0), 1), ((512, 0), 1), ((513, 0, 2), 1), ((0, 5), -1)):
        h = p.upload(np.zeros(shape))
        nout = int(np.prod(R.out_shape(shape, dim)))
        for omit in (False, True):
            assert same(reduce(p, f32, "sum", h, shape, dim, omit), np.zeros(nout)), (shape, dim, omit)
            assert same(reduce(p, f32, "prod", h, shape, dim, omit), np.ones(nout)), (shape, dim, omit)
            for op in ("mean", "min", "max"):  # min / max: what include/rmhip.h states for this entry point (the CPU's result is empty)
                assert np.isnan(reduce(p, f32, op, h, shape, dim, omit)).all() and nout > 0, (shape, dim, op, omit)
        p.free(h)


# ---- rmhip_dot ----------------------------------------------------------------------------------------------------------------------
DOT_ROWS = R.ROUNDED_ROWS + [(1, 17, 5000, "short", 1, True)]  # the extra row reaches the short-tile kernel over the product; [1, 6000, 1] (16-byte kernel A) is in the table


@pytest.mark.parametrize("row", DOT_ROWS, ids=R.row_id)
def test_dot_paths(pv, row):
    p, f32 = pv
    shape, _ = R.realise(*row[:3])
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + 53)
    ea, eb = R.exact_sum_data(rng, n, 12), R.exact_sum_data(rng, n, 12)  # |products| < 2^24, |sums| < 2^43
    ra, rb = narrow(R.rounded_sum_data(rng, n), f32), narrow(R.rounded_sum_data(rng, n), f32)
    h = {k: p.upload(v, shape) for k, v in (("ea", ea), ("eb", eb), ("ra", ra), ("rb", rb))}
    worst = 0.0
    for d in range(len(shape)):
        pre, red, post = int(np.prod(shape[:d])), shape[d], int(np.prod(shape[d + 1:]))
        oshape = R.out_shape(shape, d)

        def dot(x, y):
            out = p.dot(x, y, d)
            assert out.shape == oshape and (not f32 or p.buffer_bits(out) == 32), (row, d, out.shape)
            got = p.download(out)
            p.free(out)
            return got

        a2, b2 = R.slices(ea, pre, red, post), R.slices(eb, pre, red, post)
        want = (a2.astype(np.int64) * b2.astype(np.int64)).sum(axis=1).astype(np.float64)
        got = dot(h["ea"], h["eb"])
        assert same(got, narrow(want, f32)), (row, d, "exact", where_differs(got, narrow(want, f32)))
        # NaNs propagate: one in `a` at the start of the first slice, one in `b` at the end of the last; the other slices keep their bits
        n2a, n2b = a2.copy(), b2.copy()
        n2a[0, 0], n2b[-1, -1] = np.nan, np.nan
        hna, hnb = p.upload(R.unslice(n2a, pre, red, post), shape), p.upload(R.unslice(n2b, pre, red, post), shape)
        want_nan = want.copy()
        want_nan[[0, -1]] = np.nan
        got = dot(hna, hnb)
        assert same(got, narrow(want_nan, f32)), (row, d, "nan", where_differs(got, narrow(want_nan, f32)))
        p.free(hna)
        p.free(hnb)
        exact, sabs = R.exact_dots(R.slices(ra, pre, red, post), R.slices(rb, pre, red, post))
        bd = R.dot_bound(red, sabs)
        ok, ratio = R.error_ratios(dot(h["ra"], h["rb"]), exact, R.f32_bound(bd, exact) if f32 else bd)
        worst = max(worst, ratio.max(initial=0.0))
        assert ok.all(), (row, d, "rounded", float(ratio.max()))
    for v in h.values():
        p.free(v)
    print(f"ratio dot {'f32' if f32 else 'f64'} {R.row_id(row)} {worst:.4f}")


# ---- rmhip_reduce_nd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 50, 4), (514, 33, 3)])
def test_reduce_nd(pv, shape):
    p, f32 = pv
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + 67)
    # every step's result is narrowed on a precision-32 provider: integers whose sums stay below 2^24, and products of +-1 with 40
    # entries +-2^k (|k| <= 3: within 2^+-120), keep every intermediate exact in f32 too
    xs = R.exact_sum_data(rng, n, 8).reshape(shape, order="F")
    xp = rng.choice([-1.0, 1.0], size=n)
    at = rng.choice(n, size=40, replace=False)
    xp[at] *= np.ldexp(1.0, rng.integers(-3, 4, size=40))
    xp = xp.reshape(shape, order="F")
    hs, hp = p.upload(xs), p.upload(xp)
    for dims, asked in (((0, 2), [0, 2]), ((1,), [1]), ((0, 1, 2), [0, 1, 2]), ((1,), [1, 7, 1, 3]), ((0, 2), [2, 0, 2, 5])):
        oshape = tuple(1 if d in dims else e for d, e in enumerate(shape))
        xi = xs.astype(np.int64)
        want = {"sum": xi.sum(axis=dims), "min": xi.min(axis=dims), "max": xi.max(axis=dims), "prod": np.prod(xp, axis=dims)}
        for op, w in want.items():
            out = p._reduce_nd(op, hp if op == "prod" else hs, asked)
            assert out.shape == oshape and (not f32 or p.buffer_bits(out) == 32), (shape, asked, op, out.shape)
            got = p.download(out)
            p.free(out)
            w = narrow(np.asarray(w, dtype=np.float64).reshape(-1, order="F"), f32)
            assert same(got, w), (shape, asked, op, where_differs(got, w))
    p.free(hs)
    p.free(hp)
    small = p.upload(np.ones((2, 2)))
    with pytest.raises(ProviderError) as err:
        p._reduce_nd("sum", small, [5, 9])  # no valid dim is left
    assert err.value.code == ERR_INVALID
    p.free(small)


def test_reduce_nd_mean_power_of_two(pv):
    """mean over several dims is a mean of means (mean.rs:1107-1116): with power-of-two extents every division is exact"""
    p, f32 = pv
    shape = (8, 64, 4)
    x = R.exact_sum_data(np.random.default_rng(5), int(np.prod(shape)), 12).reshape(shape, order="F")
    h = p.upload(x)
    for dims in ((0, 2), (1,), (0, 1, 2)):
        cnt = int(np.prod([shape[d] for d in dims]))
        want = narrow((x.astype(np.int64).sum(axis=dims) / cnt).reshape(-1, order="F"), f32)  # |sum| < 2^23: an exact quotient
        out = p.reduce_mean_nd(h, list(dims))
        assert out.shape == tuple(1 if d in dims else e for d, e in enumerate(shape))
        got = p.download(out)
        p.free(out)
        assert same(got, want), (dims, where_differs(got, want))
    p.free(h)


# ---- a base address that is only element-aligned ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in R.ROUTE_TABLE if r[:3] in ((1, 2048, 3), (512, 40, 1))], ids=R.row_id)
def test_element_aligned_base(prov, oracle, row):
    """rmhip_wrap_external takes any device pointer: a tensor that starts 8 bytes into an allocation has even extents on a base that
    is not 16-byte aligned, which the ODD forms of the 16-byte kernels serve (reduce_plan.h).  Both data classes, f64 storage."""
    p = prov
    pre, red, post, kernel, nsplit, _ = row
    n = pre * red * post
    shape, dim = R.realise(pre, red, post)
    rng = np.random.default_rng(n + 71)

    def wrapped(flat):
        owner = p.upload(np.concatenate([[np.nan], flat]), (n + 1, 1))  # the element before the tensor must not leak in
        ptr = p.device_ptr(owner)
        assert ptr % 16 == 0
        return owner, p.wrap_external(ptr + 8, shape)

    s2 = R.place_nans(R.slices(R.exact_sum_data(rng, n), pre, red, post), "boundary", nsplit, kernel)
    p2 = R.place_nans(R.slices(R.exact_prod_data(rng, n), pre, red, post), "boundary", nsplit, kernel)
    nan = np.isnan(s2)
    tot = np.where(nan, 0.0, s2).astype(np.int64).sum(axis=1).astype(np.float64)
    (os_, hs), (op_, hp) = wrapped(R.unslice(s2, pre, red, post)), wrapped(R.unslice(p2, pre, red, post))
    assert same(reduce(p, False, "sum", hs, shape, dim, True), tot)
    assert same(reduce(p, False, "sum", hs, shape, dim, False), np.where(nan.any(axis=1), np.nan, tot))
    assert same(reduce(p, False, "mean", hs, shape, dim, True), tot / (~nan).sum(axis=1))
    assert same(reduce(p, False, "prod", hp, shape, dim, True), R.exact_class_prods(p2))
    for is_max in (False, True):
        assert same(reduce(p, False, "max" if is_max else "min", hs, shape, dim, True), ref_minmax(oracle, s2, row, shape, dim)[(is_max, True)])
    for o, h in ((os_, hs), (op_, hp)):
        p.free(h)
        p.free(o)
    r2, q2 = R.slices(R.rounded_sum_data(rng, n), pre, red, post), R.slices(R.rounded_prod_data(rng, n), pre, red, post)
    (os_, hs), (op_, hp) = wrapped(R.unslice(r2, pre, red, post)), wrapped(R.unslice(q2, pre, red, post))
    sums, counts = R.exact_sums(r2)
    sabs, _ = R.exact_sums(r2, absolute=True)
    ok, ratio = R.error_ratios(reduce(p, False, "sum", hs, shape, dim, False), sums, R.sum_bound(red, sabs))
    assert ok.all(), (row, "sum", float(ratio.max()))
    ok, ratio = R.error_ratios(reduce(p, False, "mean", hs, shape, dim, False), sums.over(counts), R.mean_bound(red, sabs, sums, counts))
    assert ok.all(), (row, "mean", float(ratio.max()))
    ok, ratio = R.prod_error_ratios(reduce(p, False, "prod", hp, shape, dim, False), R.exact_prods(q2), red)
    assert ok.all(), (row, "prod", float(ratio.max()))
    for o, h in ((os_, hs), (op_, hp)):
        p.free(h)
        p.free(o)
