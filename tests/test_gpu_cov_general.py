"""cov(x, y) and weighted cov on the device (rmhip_covariance_general) against the NumPy model of `cov_from_tensors` (tests/cov_general_ref.py).

Tolerance, the plain form's (test_gpu_parity.py::test_covariance_vs_oracle): the NaN pattern is equal and, over the finite entries,
max|got - want| <= 64 eps (1 + max|want|) sqrt(rows) - tree-ordered sums and MFMA-ordered products against the CPU's sequential loops (a
differently ordered CPU evaluation stays below 0.3 % of that bound on these shapes).  Every case also asks for an exactly symmetric result and
for the same bits from two successive calls.  The shapes are the smallest that reach each edge: the MFMA route below and just off the
tall-skinny route (41 columns), a second operand that crosses the 128-column tile boundary, both operands inside one eight-column block, an
odd tail row, the last skinny shape (40 columns), several row chunks with 90 % of the weights zero."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cov_general_ref as ref  # noqa: E402
from test_gpu_complex_move import ERR_INVALID, ERR_NOT_FOUND, ERR_SHAPE, ERR_UNSUPPORTED, live, raises, up_c  # noqa: E402
from test_gpu_f32 import close32, f32r  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def up(p, a):
    """Column-major upload (a large row-major matrix would arrive as a transpose view)."""
    a = np.asarray(a, dtype=np.float64)
    return p.upload(np.asfortranarray(a if a.ndim == 2 else a.reshape(-1, 1)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def data(rows, c1, c2, seed=0):
    rng = np.random.default_rng(rows * 3 + c1 + 7 * c2 + seed)
    m = rng.uniform(-1, 1, (rows, c1 + c2)) + np.arange(c1 + c2)
    return m[:, :c1], m[:, c1:]


def weights_of(kind, rows):
    rng = np.random.default_rng(rows + 11)
    if kind is None:
        return None
    if kind == "int":
        return np.resize(np.array([1.0, 0.0, 3.0, 2.0]), rows)
    if kind == "real":
        return rng.uniform(0, 2, rows)
    if kind == "sparse":  # 90 % of the weights zero
        return np.where(rng.uniform(0, 1, rows) < 0.9, 0.0, rng.uniform(0, 2, rows))
    raise AssertionError(kind)


def run(p, x, y=None, w=None, biased=False):
    """Two successive calls: the same bits; the downloaded matrix of the first."""
    hs = [up(p, x), up(p, y) if y is not None and y.shape[1] else None, up(p, w) if w is not None else None]
    a = p.covariance_general(hs[0], second=hs[1], weights=hs[2], biased=biased)
    b = p.covariance_general(hs[0], second=hs[1], weights=hs[2], biased=biased)
    got, again = p.download_matrix(a), p.download_matrix(b)
    for h in [a, b] + [h for h in hs if h is not None]:
        p.free(h)
    assert np.array_equal(bits(got), bits(again)), "two successive calls differ"
    return got


def check(got, want, rows):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    if fin.any():
        err, bound = np.max(np.abs(got[fin] - want[fin])), 64 * EPS * (1.0 + np.max(np.abs(want[fin]))) * np.sqrt(rows)
        print(f"max|got - want| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)
    assert np.array_equal(bits(got), bits(np.ascontiguousarray(got.T))), "not exactly symmetric"


CASES = [  # rows, c1, c2, weights
    (4, 3, 0, "int"),            # MFMA route
    (257, 100, 29, "real"),      # MFMA: the second operand crosses the 128-column boundary
    (257, 100, 29, None),
    (4096, 33, 8, "real"),       # 41 columns: just off the skinny route
    (4096, 8, 0, "real"),        # skinny
    (4097, 5, 4, None),          # skinny: both operands inside one eight-column block, odd tail row
    (4097, 5, 4, "real"),
    (4096, 33, 7, "real"),       # 40 columns: the last skinny shape
    (70001, 17, 16, "sparse"),
    (300000, 2, 1, "real"),
]


@pytest.mark.parametrize("rows,c1,c2,kind", CASES)
def test_cov_general_vs_model(prov, rows, c1, c2, kind):
    x, y = data(rows, c1, c2)
    w = weights_of(kind, rows)
    got = run(prov, x, y, w)
    check(got, ref.cov_general(x, y if c2 else None, w), rows)
    if kind is not None:  # `biased` is ignored in the weighted form
        assert np.array_equal(bits(run(prov, x, y, w, biased=True)), bits(got))


@pytest.mark.parametrize("rows,c1,c2", [(50, 3, 1), (5000, 3, 2)])  # MFMA route, skinny route
def test_cov_general_special_weight_sums(prov, rows, c1, c2):
    """Weights that are multiples of 2^-10: every sum is exact in any order, so the NaN decisions fall where the CPU's fall."""
    x, y = data(rows, c1, c2)
    w = np.zeros(rows)
    w[[1, 5, 17, 40]] = 0.25  # sum_w == 1: denom == 0
    assert np.all(np.isnan(run(prov, x, y, w)))
    w[44] = 0.25              # sum_w == 1.25
    got = run(prov, x, y, w)
    assert np.all(np.isfinite(got))
    check(got, ref.cov_general(x, y, w), rows)
    assert np.all(np.isnan(run(prov, x, y, np.zeros(rows))))
    w = np.round(np.random.default_rng(3).uniform(0, 2, rows) * 1024) / 1024
    check(run(prov, x, y, w), ref.cov_general(x, y, w), rows)


def test_cov_general_degenerate_shapes(prov):
    x, y = data(1, 2, 3)
    got = run(prov, x, y)  # rows == 1, unbiased: rows - 1 == 0
    assert got.shape == (5, 5) and np.all(np.isnan(got))
    check(run(prov, x, y, biased=True), ref.cov_general(x, y, biased=True), 1)
    check(run(prov, x, y, np.array([1.5])), ref.cov_general(x, y, np.array([1.5])), 1)  # one weighted row: sum_w - 1 > 0, all zero
    e, e2 = prov.upload(np.zeros((5, 0))), prov.upload(np.zeros((5, 0)))
    w = up(prov, np.ones(5))
    for kw in ({"second": e2}, {"weights": w}, {"second": e2, "weights": w}):
        out = prov.covariance_general(e, **kw)
        assert tuple(prov._handle(out.buffer_id).shape) == (0, 0)
        prov.free(out)
    for h in (e, e2, w):
        prov.free(h)


@pytest.mark.parametrize("rows,cols", [(60, 5), (4500, 5)])
def test_cov_general_second_may_be_the_matrix_itself(prov, rows, cols):
    x, _ = data(rows, cols, 0)
    w = weights_of("real", rows)
    h, hw = up(prov, x), up(prov, w)
    for kw, want in (({}, ref.cov_general(x, x)), ({"weights": hw}, ref.cov_general(x, x, w))):
        out = prov.covariance_general(h, second=h, **kw)
        check(prov.download_matrix(out), want, rows)
        prov.free(out)
    # a transpose view as the second operand is read as the matrix it stands for
    base = up(prov, x.T)
    view = prov.transpose(base)
    out = prov.covariance_general(h, second=view, weights=hw)
    check(prov.download_matrix(out), ref.cov_general(x, x, w), rows)
    for t in (out, view, base, h, hw):
        prov.free(t)


@pytest.mark.parametrize("rows,c1,c2", [(50, 3, 2), (5000, 6, 5)])  # MFMA route, skinny route (two column blocks)
def test_cov_general_nonfinite_values_poison_their_column(prov, rows, c1, c2):
    x, y = data(rows, c1, c2)
    w = weights_of("real", rows) + 0.5
    w[9] = 0.0
    cols = c1 + c2
    for value, row, col in ((np.inf, 7, 1), (np.nan, 9, c1 + 1), (np.inf, 9, 0)):  # row 7: positive weight; row 9: zero weight
        m = np.concatenate([x, y], axis=1)
        m[row, col] = value
        want_nan = np.zeros((cols, cols), dtype=bool)
        want_nan[col, :] = want_nan[:, col] = True
        for weights in (w, None):
            got = run(prov, m[:, :c1], m[:, c1:], weights)
            want = ref.cov_general(m[:, :c1], m[:, c1:], weights)
            assert np.array_equal(np.isnan(want), want_nan)
            check(got, want, rows)


@pytest.mark.parametrize("rows,c1,c2", [(50, 3, 2), (5000, 6, 5)])
def test_cov_general_constant_column_has_a_clean_diagonal(prov, rows, c1, c2):
    x, y = data(rows, c1, c2)
    x[:, 1] = 0.1 + 0.2
    y[:, 0] = 1.0 / 3.0
    for w in (None, weights_of("real", rows)):
        got = run(prov, x, y, w)
        check(got, ref.cov_general(x, y, w), rows)
        for d in (1, c1):
            # exactly 0 or +tiny (a mean off by at most rows eps |c|, squared), never negative and never -0
            assert 0.0 <= got[d, d] <= (rows * EPS) ** 2 and not np.signbit(got[d, d]), got[d, d]


def test_cov_general_refusals(prov):
    lib, ctx = prov._lib, prov._ctx
    import ctypes as C

    x, y = data(50, 3, 2)
    hx, hy, hw = up(prov, x), up(prov, y), up(prov, np.ones(50))
    tall = up(prov, data(4200, 3, 0)[0])
    flat = np.arange(24.0)
    three_d = prov.upload(flat, (4, 3, 2))
    w3b, w2d = prov.upload(np.ones(50), (5, 5, 2)), prov.upload(np.ones(50), (2, 25))
    z = up_c(prov, np.ones((50, 2)) + 1j)
    empty, w0 = prov.upload(np.zeros((0, 3))), prov.upload(np.zeros((0, 1)))
    before = live(prov)
    out = C.c_uint64()
    assert lib.rmhip_covariance_general(ctx, hx.buffer_id, hy.buffer_id, hw.buffer_id, 0, None) == ERR_INVALID  # null out
    for ids in ((1 << 40, hy.buffer_id, hw.buffer_id), (hx.buffer_id, 1 << 40, hw.buffer_id), (hx.buffer_id, 0, 1 << 40),
                (z.buffer_id, 1 << 40, 0)):  # an unknown id is reported before a complex operand is judged
        assert lib.rmhip_covariance_general(ctx, ids[0], ids[1], ids[2], 0, C.byref(out)) == ERR_NOT_FOUND
        assert out.value == 0
    for kw in ({"matrix": z, "second": hy}, {"matrix": hx, "second": z}, {"matrix": hx, "weights": z}):
        raises(ERR_UNSUPPORTED, lambda: prov.covariance_general(**kw), "complex")
    raises(ERR_UNSUPPORTED, lambda: prov.covariance_general(three_d, second=hy), "covariance: only 2D supported")
    raises(ERR_UNSUPPORTED, lambda: prov.covariance_general(hx, second=three_d), "covariance: only 2D supported")
    raises(ERR_UNSUPPORTED, lambda: prov.covariance_general(three_d, weights=hw), "covariance: only 2D supported")
    raises(ERR_SHAPE, lambda: prov.covariance_general(hx, second=tall), "covariance: inputs must have the same number of rows (got 50 and 4200)")
    raises(ERR_SHAPE, lambda: prov.covariance_general(tall, second=hx, weights=hw), "covariance: inputs must have the same number of rows (got 4200 and 50)")
    raises(ERR_SHAPE, lambda: prov.covariance_general(hx, weights=w2d), "covariance: weight vector must be 1-D")
    raises(ERR_SHAPE, lambda: prov.covariance_general(hx, weights=w3b), "covariance: weight vector must be 1-D")
    raises(ERR_SHAPE, lambda: prov.covariance_general(tall, weights=hw), "covariance: weight vector length mismatch (expected 4200 elements)")
    raises(ERR_SHAPE, lambda: prov.covariance_general(hx, second=hy, weights=w0), "covariance: weight vector length mismatch (expected 50 elements)")
    raises(ERR_INVALID, lambda: prov.covariance_general(empty, weights=w0), "covariance: weight vector cannot be empty")
    assert live(prov) == before
    for h, rows in ((hx, 50), (tall, 4200)):  # decided on the device, on either route
        for bad in (-0.25, np.nan, np.inf, -np.inf):
            w = np.ones(rows)
            w[rows - 3] = bad
            hb = up(prov, w)
            mark = live(prov)
            raises(ERR_INVALID, lambda: prov.covariance_general(h, weights=hb), "covariance: weights must be non-negative finite values")
            assert live(prov) == mark
            prov.free(hb)
    wr = prov.upload(np.ones(50), (1, 50))  # what is not refused: a row vector of weights
    out_h = prov.covariance_general(hx, second=hy, weights=wr)
    check(prov.download_matrix(out_h), ref.cov_general(x, y, np.ones(50)), 50)
    prov.free(out_h)
    for h in (hx, hy, hw, tall, three_d, w3b, z, empty, w0, w2d, wr):
        prov.free(h)


@pytest.mark.parametrize("rows,cols", [(257, 129), (4096, 8), (1, 4), (3, 0)])
@pytest.mark.parametrize("biased", [False, True])
def test_cov_general_of_one_operand_is_covariance(prov, rows, cols, biased):
    x, _ = data(rows, cols, 0)
    h = prov.upload(np.asfortranarray(x))
    a, b = prov.covariance_general(h, biased=biased), prov.covariance(h, biased=biased)
    assert tuple(prov._handle(a.buffer_id).shape) == (cols, cols)
    assert np.array_equal(bits(prov.download(a)), bits(prov.download(b)))
    for t in (a, b, h):
        prov.free(t)


@pytest.fixture(scope="module")
def prov32(built):
    import os
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


@pytest.mark.parametrize("rows,c1,c2", [(4096, 4, 4), (257, 20, 13)])  # skinny route (f32 read in place), MFMA route
def test_cov_general_precision_32(prov32, rows, c1, c2):
    """f32 storage read in place and widened in registers, f64 sums and products, one rounding on store: against the model on the f32-rounded
    inputs, with the tolerance tests/test_gpu_f32.py uses for the covariance of f32 storage (2 ulp of f32, 1e-7 absolute)."""
    x, y = data(rows, c1, c2)
    x, y, w = f32r(x), f32r(y), f32r(weights_of("real", rows))
    hx, hy, hw = up(prov32, x), up(prov32, y), up(prov32, w)
    a = prov32.covariance_general(hx, second=hy, weights=hw)
    b = prov32.covariance_general(hx, second=hy, weights=hw)
    assert prov32.buffer_bits(a) == 32
    got = prov32.download_matrix(a)
    assert np.array_equal(bits(got), bits(prov32.download_matrix(b)))
    assert close32(got, f32r(ref.cov_general(x, y, w)), ulps=2.0, atol=1e-7)
    assert np.array_equal(bits(got), bits(np.ascontiguousarray(got.T)))
    u = prov32.covariance_general(hx, second=hy)
    assert close32(prov32.download_matrix(u), f32r(ref.cov_general(x, y)), ulps=2.0, atol=1e-7)
    for h in (a, b, u, hx, hy, hw):
        prov32.free(h)
