"""CPU twin of tests/test_gpu_reduce_paths.py: the exact references of tests/reduce_ref.py on hand-computed cases, and a plain
sequential f64 loop (the oracle's sum and mean, numpy's cumulative product and sum) held against every bound on every table entry
of the rounded class - a correct implementation can satisfy them - and against bit equality on the exact class."""
import math
from fractions import Fraction

import numpy as np
import pytest

import reduce_ref as R

F = Fraction


def test_hand_cases():
    s2 = np.array([[1.0, 2.0 ** -60, -1.0], [0.1, 0.2, np.nan], [np.nan, np.nan, np.nan]])
    sums, counts = R.exact_sums(s2)  # the first row spans 60 binades: the Fraction path
    assert sums.fractions() == [F(1, 2 ** 60), F(0.1) + F(0.2), F(0)] and counts.tolist() == [3, 2, 0]
    assert R.exact_sums(s2, absolute=True)[0].fractions()[0] == 2 + F(1, 2 ** 60)
    t2 = np.array([[1.5, -0.75, 3.0], [2.0 ** -8, 1.0, np.nan]])  # 10 binades: the int64 path
    assert R.exact_sums(t2)[0].fractions() == [F(15, 4), F(257, 256)]
    assert R.exact_prods(np.array([[1.5, -0.75, 3.0, np.nan], [0.0, 5.0, -2.0, 1.0], [-0.0, -5.0, 1.0, 1.0]])) == [(True, 27, 27, -3), (False, 0, 0, 0),
                                                                                                                 (False, 0, 0, 0)]
    neg, lo, hi, e = R.exact_prods(np.array([[1.0 + 2.0 ** -52] * 3]))[0]
    assert not neg and lo == hi and F(lo) * F(2) ** e == (1 + F(1, 2 ** 52)) ** 3
    x = np.full((1, 300), -(1.0 + 2.0 ** -52))  # 300 * 53 bits: enclosed, not exact
    (neg, lo, hi, e), p = R.exact_prods(x)[0], (1 + F(1, 2 ** 52)) ** 300
    assert not neg and lo < hi and F(lo) * F(2) ** e <= p <= F(hi) * F(2) ** e and F(hi - lo, lo) <= F(1, 2 ** 380)
    neg, lo, hi = R.prod_enclosure(R.exact_prods(np.array([[1.5, -0.75, 3.0]])))
    assert neg.tolist() == [True] and lo.fractions() == hi.fractions() == [F(27, 8)]
    d, da = R.exact_dots(np.array([[0.1, -0.2, 3.0]]), np.array([[0.3, 0.7, -2.0 ** -7]]))
    assert d.fractions() == [F(0.1) * F(0.3) - F(0.2) * F(0.7) - F(3, 128)] and da.fractions() == [F(0.1) * F(0.3) + F(0.2) * F(0.7) + F(3, 128)]
    assert R.gamma(0) == 0 and R.gamma(3) == F(3, 2 ** 53 - 3)
    q = R.Q.floats([0.1, -3.0, 0.0, 2.0 ** -1070])
    assert q.fractions() == [F(0.1), F(-3), F(0), F(2.0 ** -1070)] and np.array_equal(q.to_f64(), [0.1, -3.0, 0.0, 2.0 ** -1070])
    assert (q * F(1, 3) + 1).fractions()[1] == 0 and abs(q - 1).fractions()[1] == 4 and q.over([1, 2, 3, 4]).fractions()[1] == F(-3, 2)
    assert q.le(F(0)).tolist() == [False, True, True, False] and q.maximum(F(1, 20)).fractions()[:3] == [F(0.1), F(1, 20), F(1, 20)]
    assert R.sum_bound(1, R.Q.floats([5.0])).fractions() == [0]
    assert R.sum_bound(4, R.Q.floats([5.0])).fractions() == [5 * R.gamma(3)]
    assert R.mean_bound(4, R.Q.floats([5.0]), R.Q.floats([-3.0]), [2]).fractions() == [R.gamma(3) * 5 / 2 * (1 + R.U) + R.U * F(3, 2)]
    assert R.f32_bound(R.Q.of(0), R.Q.floats([3.0])).fractions() == [F(3, 2 ** 24)]
    ok, ratio = R.error_ratios([1.0, 1.0 + 2.0 ** -52, 2.0, 3.0], R.Q.floats([1.0, 1.0, 2.0, 3.5]), R.Q.of(F(1, 2 ** 52)) * R.Q.floats([1.0, 1.0, 0.0, 0.0]))
    assert ok.tolist() == [True, True, True, False] and ratio.tolist() == [0.0, 1.0, 0.0, math.inf]
    ok, ratio = R.prod_error_ratios([-3.375, 3.375, 0.0, -0.0, 1.0], [(True, 27, 27, -3)] * 2 + [(False, 0, 0, 0)] * 3, 4)
    assert ok.tolist() == [True, False, True, True, False] and ratio[0] == 0.0
    assert R.boundary_indices(6000, 3, "strided") == [1999, 2000, 3999, 4000] and R.chunk_starts(6000, 3, "contig_v2") == [2000, 2048, 4000, 4096]
    assert R.chunk_starts(600, 2, "contig") == [300, 512] and R.chunk_starts(600, 2, "strided_v2") == [300]
    # 40000 f64 are 64 KiB and more (blocks of 1024), 40000 f32 are not (blocks of 256): both cuts
    assert R.chunk_starts(10000, 4, "contig") == [2500, 2560, 3072, 5000, 5120, 6144, 7500, 7680, 9216]
    assert R.chunk_starts(70000, 9, "contig") == sorted({7778 * k for k in range(1, 9)} | {8192 * k for k in range(1, 9)})
    assert R.boundary_indices(6000, 3) == [1999, 2000, 3999, 4000] and R.boundary_indices(5, 1) == [1, 2] and R.boundary_indices(1, 1) == [0]
    x = np.arange(24.0)
    assert np.array_equal(R.slices(x, 2, 3, 4)[1 + 2 * 3], [19.0, 21.0, 23.0])  # slice (i=1, j=3): elements 1 + 2 * (r + 3 * 3)
    assert np.array_equal(R.unslice(R.slices(x, 2, 3, 4), 2, 3, 4), x)
    assert R.realise(1, 9, 1) == ((9, 1), -1) and R.realise(1, 9, 4) == ((9, 4), 0) and R.realise(5, 9, 1) == ((5, 9), 1)


def test_placements():
    s2 = np.arange(7 * 10, dtype=np.float64).reshape(7, 10)
    for how, cols in (("first", [0]), ("last", [9]), ("boundary", [4, 5])):
        nan = np.isnan(R.place_nans(s2, how, 2))
        assert nan[0::3][:, cols].all() and nan.sum() == 3 * len(cols), how
    nan = np.isnan(R.place_nans(s2, "whole", 2))
    assert nan[[1, 4]].all() and nan.sum() == 20 and np.isnan(R.place_nans(s2[:1], "whole", 1)).all()
    assert not np.isnan(R.place_nans(s2, "none", 2)).any()


@pytest.mark.parametrize("row", R.ROUNDED_ROWS, ids=R.row_id)
def test_sequential_f64_meets_every_bound(row, oracle):
    pre, red, post = row[:3]
    n = pre * red * post
    rng = np.random.default_rng(1000 + n)
    shape, dim = R.realise(pre, red, post)
    dims = "all" if dim < 0 else [dim]
    for f32 in (False, True):
        x = R.rounded_sum_data(rng, n)
        x = R.to_f32(x) if f32 else x
        for how in ("none", "boundary"):
            s2 = R.place_nans(R.slices(x, pre, red, post), how, row[4], row[3])
            flat = R.unslice(s2, pre, red, post).reshape(shape, order="F")
            sums, counts = R.exact_sums(s2)
            sabs, _ = R.exact_sums(s2, absolute=True)
            if how == "none":  # math.fsum is the rounding of the exact sum
                assert np.array_equal(sums[:64].to_f64(), [math.fsum(r) for r in s2[:64]])
            narrow = (lambda g: g.astype(np.float32).astype(np.float64)) if f32 else (lambda g: g)
            got_s = narrow(oracle.reduce_sum(flat, dims, omitnan=True).reshape(-1, order="F"))
            got_m = narrow(oracle.reduce_sum(flat, dims, omitnan=True, mean=True).reshape(-1, order="F"))
            bs = R.sum_bound(red, sabs)
            assert R.error_ratios(got_s, sums, R.f32_bound(bs, sums) if f32 else bs)[0].all(), (row, how)
            some = counts > 0
            means = sums[some].over(counts[some])
            bm = R.mean_bound(red, sabs[some], sums[some], counts[some])
            assert R.error_ratios(got_m[some], means, R.f32_bound(bm, means) if f32 else bm)[0].all(), (row, how)
            assert np.isnan(got_m[~some]).all()
        p2 = R.slices(R.to_f32(R.rounded_prod_data(rng, n)) if f32 else R.rounded_prod_data(rng, n), pre, red, post)
        seq = np.cumprod(p2, axis=1)[:, -1]
        assert R.prod_error_ratios(narrow(seq), R.exact_prods(p2), red, f32)[0].all(), row
        a2, b2 = R.slices(R.rounded_sum_data(rng, n), pre, red, post), R.slices(R.rounded_sum_data(rng, n), pre, red, post)
        if f32:
            a2, b2 = R.to_f32(a2), R.to_f32(b2)
        d, da = R.exact_dots(a2, b2)
        bd = R.dot_bound(red, da)
        assert R.error_ratios(narrow(np.cumsum(a2 * b2, axis=1)[:, -1]), d, R.f32_bound(bd, d) if f32 else bd)[0].all(), row


@pytest.mark.parametrize("row", R.ROUNDED_ROWS, ids=R.row_id)
def test_exact_class_is_order_independent(row):
    """a sequential loop, its reverse and numpy's pairwise order give the reference's bits; the integer references agree with the
    big-integer ones"""
    pre, red, post = row[:3]
    n = pre * red * post
    rng = np.random.default_rng(2000 + n)
    s2 = R.slices(R.exact_sum_data(rng, n), pre, red, post)
    want = R.exact_sums(s2)[0].to_f64()
    assert np.array_equal(want, s2.astype(np.int64).sum(axis=1).astype(np.float64))
    assert np.array_equal(np.cumsum(s2, axis=1)[:, -1], want) and np.array_equal(np.cumsum(s2[:, ::-1], axis=1)[:, -1], want)
    p2 = R.place_nans(R.slices(R.exact_prod_data(rng, n), pre, red, post), "boundary", row[4], row[3])
    wantp = R.exact_class_prods(p2)
    big = R.exact_prods(p2)
    assert all(q[1] == q[2] for q in big)
    assert np.array_equal(wantp, [(-1.0 if q[0] else 1.0) * float(F(q[1]) * F(2) ** q[3]) for q in big])
    q2 = np.where(np.isnan(p2), 1.0, p2)
    assert np.array_equal(np.cumprod(q2, axis=1)[:, -1], wantp) and np.array_equal(np.cumprod(q2[:, ::-1], axis=1)[:, -1], wantp)
    a2, b2 = R.slices(R.exact_sum_data(rng, n, 12), pre, red, post), R.slices(R.exact_sum_data(rng, n, 12), pre, red, post)
    wantd = (a2.astype(np.int64) * b2.astype(np.int64)).sum(axis=1)
    lo2, hi2 = np.abs(a2) + 4096.0, np.abs(b2) + 4096.0  # one binade each: within the span exact_dots takes
    assert [F(int(w)) for w in (lo2.astype(np.int64) * hi2.astype(np.int64)).sum(axis=1)] == R.exact_dots(lo2, hi2)[0].fractions()
    assert np.array_equal(np.cumsum(a2 * b2, axis=1)[:, -1], wantd.astype(np.float64))


def test_route_table_is_the_host_checks_table(tmp_path):
    """tests/cpp/reduce_route_check.cpp prints the table it pins against reduce_plan.h: the GPU tests' ROUTE_TABLE must be that list"""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "reduce_route_check"
    c = subprocess.run(["g++", "-std=c++17", "-O1", f"-I{root / 'runmat_amd' / 'csrc'}", str(root / "tests" / "cpp" / "reduce_route_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("row ")]
    assert [(int(a), int(b), int(c), k, int(n), f == "flat") for a, b, c, k, n, f in rows] == R.ROUTE_TABLE
    for tag, table in (("acc", R.ACC_ROUTE_TABLE), ("gen", R.GEN_ROUTE_TABLE)):  # the accumulator and generated families' tables
        rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(tag + " ")]
        assert [(int(a), int(b), int(c), k, int(n), f == "flat", int(gx), int(bl)) for a, b, c, k, n, f, gx, bl in rows] == table, tag
