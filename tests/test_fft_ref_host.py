"""fft_ref.py against the oracle's direct DFT in long double (oracle.fft_dim) - the independent ground truth of the transform tests.

Agreement: 4 eps sum|a_j| per bin (/ n for the inverse).  Both sides evaluate the same short sum in long double and round once to
double (<= eps/2 |X| <= eps/2 sum|a_j| each); the rest is headroom for the oracle's own accumulation."""
import numpy as np
import pytest

import fft_ref as R

LENGTHS = (1, 2, 3, 8, 15, 64, 100)


def shapes_for(n, dim, how):
    cur = {"exact": n, "padded": max(1, n - max(1, n // 3)), "truncated": n + 1 + n // 2}[how]
    shape = [3, 2, 2]
    shape[dim] = cur
    return tuple(shape), (None if how == "exact" else n)


@pytest.mark.parametrize("how", ["exact", "padded", "truncated"])
@pytest.mark.parametrize("dim", [0, 1, 2])
@pytest.mark.parametrize("n", LENGTHS)
def test_sparse_transform_matches_the_oracle(oracle, n, dim, how):
    shape, length = shapes_for(n, dim, how)
    for real in (True, False):
        case = R.impulse_case(shape, dim, length, seed=1000 * n + 10 * dim + len(how), real=real)
        x = case.dense()
        assert x.shape == shape and np.isrealobj(x) == real and case.n == n and case.lines == 4 * 3 // (3 if dim == 0 else 2)
        lines = np.arange(case.lines)
        bins = R.bins_to_check(n)
        assert np.array_equal(bins, np.arange(n))
        sum_a = np.sum(np.abs(case.amps(lines)), axis=1)[:, None]
        for inverse in (False, True):
            want = oracle.fft_dim(x, length, dim, inverse)
            assert want.shape == case.oshape
            got = R.sparse_dft(case, lines, bins, inverse)
            ref = want.reshape(-1, order="F")[case.out_index(lines, bins)]
            assert np.all(np.abs(got - ref) <= 4 * R.EPS * sum_a / (n if inverse else 1)), (shape, dim, length, real, inverse)
            # the norms the tolerance is built from are those of the dense input
            dense_lim = np.moveaxis(R.bound(x, n, dim, inverse), dim, -1).reshape(-1, order="F")
            assert np.allclose(R.line_bound(case.norms(lines), n, inverse), dense_lim, rtol=4 * R.EPS, atol=0)   # (the order of the sum)


def test_case_layout():
    case = R.impulse_case((3, 40, 2), 1, 16, seed=5, real=False)       # truncated: markers at n and at cur - 1 of every line
    x = case.dense()
    assert case.inner == 3 and case.outer == 2 and case.lines == 6 and list(case.markers) == [16, 39]
    assert np.all(x[:, 16, :] == R.MARKER * (1 + 1j)) and np.all(x[:, 39, :] == R.MARKER * (1 + 1j))
    assert list(case.pos[:3]) == [0, 1, 15] and 9 in case.pos and case.pos[-1] % 2 == 1 and np.all(case.pos < 16)
    assert np.count_nonzero(x) == case.lines * (len(case.pos) + 2)
    for l in range(case.lines):                                        # line l = i + inner * o, scaled by 1 + l / 64: all distinct
        i, o = l % 3, l // 3
        for p, a in case.terms(l):
            assert x[i, p, o] == a and a == case.base[list(case.pos).index(p)] * (1 + l / 64)
    assert np.all(case.base.real != case.base.imag) and len({a for _, a in case.terms(0)} | {a for _, a in case.terms(1)}) == 2 * len(case.pos)
    short = R.impulse_case((2, 5), 0, 3, seed=1, real=True)            # cur = 2, n = 3: the positions clip onto 0 and 1
    assert list(short.pos) == [0, 1] and short.markers.size == 0 and np.isrealobj(short.dense()) and np.all(short.base.imag == 0)
    one = R.impulse_case((1,), 0, None, seed=1, real=True)
    assert list(one.pos) == [0]
    padded = R.impulse_case((10,), 0, 16, seed=2, real=False)          # padded: nothing beyond the input, last term at cur - 1
    assert padded.markers.size == 0 and padded.pos[2] == 9 and np.all(padded.pos <= 9)


def test_bins_to_check():
    for n in (1, 7, 1 << 18):
        assert np.array_equal(R.bins_to_check(n), np.arange(n))
    for n, bnd in ((1 << 21, (1 << 10,)), (1 << 26, (1 << 8, 1 << 17)), (5_000_000, (1 << 8, 1 << 16))):
        b = R.bins_to_check(n, bnd, seed=3)
        assert b.dtype == np.int64 and np.all(np.diff(b) > 0) and b[0] == 0 and b[-1] == n - 1 and 70000 < b.size <= 1 << 18
        have = set(b.tolist())
        for lo, hi in [(0, 4096), (n - 4096, n), (n // 2 - 2048, n // 2 + 2048)] + [(m - 2048, m + 2048) for m in bnd]:
            assert all(f in have for f in range(max(0, lo), hi))
        assert np.array_equal(b, R.bins_to_check(n, bnd, seed=3))


def test_long_lines_against_numpy():
    """Beyond the oracle's reach (O(n^2)): numpy's transform of the dense line stays far inside the kernels' tolerance of the
    closed form, at a chirp length and at a power of two."""
    for n in (300007, 1 << 20):
        case = R.impulse_case((n,), 0, None, seed=n, real=False)
        bins = R.bins_to_check(n, (1 << 10,), seed=1)
        x = case.dense()
        table = R.phase_table(case.pos, n, bins)
        for inverse in (False, True):
            got = (np.fft.ifft if inverse else np.fft.fft)(x)[bins]
            want = R.sparse_dft(case, [0], bins, inverse, table)[0]
            assert np.max(np.abs(got - want)) <= 0.25 * R.line_bound(case.norms([0])[0], n, inverse)
