"""GPU checks of `chol_info` (rmhip_chol_info, runmat_amd/csrc/chol.hip): the failure forms of `[R, p] = chol(A)` on the device.

Expectations come from tests/chol_info_ref.py - a piece of the positive definite parent's factor as oracle.chol computes it, exact zeros
elsewhere - which tests/test_chol_info_host.py pins to the oracle case by case on the CPU.  `info` and the zero pattern are exact; kept
entries are within 20 cond(parent) eps max|want| of the oracle, the bound test_chol_matches_the_oracle uses for the same two summation
orders; the lower form is exactly the transpose.  Sizes: n = 200 recurses 128 + (64 + 8), leaves ending at 63, 127 and 191; n = 2049
gives depth; n = 4224 reaches the panelled update (a trailing block of more than 2048 columns)."""
import numpy as np
import pytest

import chol_info_ref as ref

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 2
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def truth(oracle):
    """n -> (the oracle's factor of the parent, cond(parent)); computed once per size."""
    cache = {}

    def get(n):
        if n not in cache:
            r0, info = oracle.chol(ref.parent(n))
            assert info == 0
            r0.setflags(write=False)
            cache[n] = (r0, float(np.linalg.cond(ref.parent(n))))
        return cache[n]
    return get


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, precision="F32")
    yield p
    p.close()


def live(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def factor(prov, h, lower=False, entry=None):
    res = (entry or prov.chol_info)(h, lower)
    got = prov.download_matrix(res.factor)
    prov.free(res.factor)
    return got, res.info


def check(prov, case, r0, cond):
    n = r0.shape[0]
    want_info, want = ref.expected(r0, case.kind, case.col)
    h = prov.upload(case.a)
    got, info = factor(prov, h)
    low, low_info = factor(prov, h, True)
    prov.free(h)
    err, bound = float(np.max(np.abs(got - want))), 20 * cond * EPS * float(np.max(np.abs(want), initial=0.0))
    print(f"chol_info n={n} {case.name}: info {info} (want {want_info}), max error {err:.3e}, bound {bound:.3e}")
    assert info == want_info and low_info == want_info, case.name
    assert not np.isnan(got).any(), case.name
    assert np.array_equal(got != 0.0, want != 0.0), case.name
    assert np.array_equal(got != 0.0, ref.keep_mask(n, case.kind, case.col)), case.name
    assert err <= bound, case.name
    assert np.array_equal(low.view(np.uint64), got.T.view(np.uint64)), case.name
    return got


@pytest.mark.parametrize("n, j", [(n, j) for n in (200, 2049) for j in ref.P_COLUMNS[n]])
def test_a_failed_pivot_keeps_the_columns_before_it_and_the_column_above_it(prov, truth, n, j):
    r0, cond = truth(n)
    check(prov, ref.Case(f"P{j}", ref.lowered(ref.parent(n), r0, j), "P", j), r0, cond)


def test_asymmetry_reports_its_column_and_leaves_it_zero(prov, truth):
    r0, cond = truth(200)
    for case in ref.asymmetry_cases(r0):
        got = check(prov, case, r0, cond)
        if case.kind == "A":
            assert not got[:, case.col].any(), case.name


def test_non_finite_entries_never_reach_the_factor(prov, truth):
    r0, cond = truth(200)
    for case in ref.nonfinite_cases():
        check(prov, case, r0, cond)  # asserts a NaN-free result


@pytest.mark.parametrize("n", [1, 3, 64, 65, 200])
def test_success_is_chol_bit_for_bit(prov, n):
    a = ref.parent(200)[:n, :n] if n < 200 else ref.parent(200)  # a leading block of a positive definite matrix is one
    h = prov.upload(np.ascontiguousarray(a))
    for lower in (False, True):
        got, info = factor(prov, h, lower)
        want, want_info = factor(prov, h, lower, entry=prov.chol)
        assert info == 0 and want_info == 0
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, lower)
    prov.free(h)


def test_the_empty_matrix(prov):
    res = prov.chol_info(prov.upload(np.zeros((0, 0))))
    assert tuple(res.factor.shape) == (0, 0) and res.info == 0


def test_a_tiny_pivot_is_declined_unless_it_is_the_last(prov, oracle):
    from runmat_amd import ProviderError

    for name, a, t, declined in ref.tiny_cases():
        h = prov.upload(a)
        if declined:
            assert oracle.chol(a)[1] == t + 1, name  # the host's answer for what is declined here
            for lower in (False, True):
                mark = live(prov)
                with pytest.raises(ProviderError) as e:
                    prov.chol_info(h, lower)
                assert e.value.code == ERR_UNSUPPORTED, (name, str(e.value))
                assert live(prov) == mark, name  # nothing left behind
        else:
            want, want_info = oracle.chol(a)
            got, info = factor(prov, h)
            assert info == 0 and want_info == 0 and got[t, t] == 1e-13
            assert np.max(np.abs(got - want)) <= 20 * np.linalg.cond(a[:t, :t]) * EPS * np.max(np.abs(want))
            assert np.array_equal(factor(prov, h, True)[0], got.T)
        prov.free(h)


def test_the_references_failure_kat(prov):
    """chol_gpu_failure_flag, chol.rs:1008-1021."""
    h = prov.upload(np.array([[1.0, 2.0], [2.0, 1.0]]))
    got, info = factor(prov, h)
    assert info == 2 and np.array_equal(got, [[1.0, 2.0], [0.0, 0.0]])
    got, info = factor(prov, h, True)
    assert info == 2 and np.array_equal(got, [[1.0, 0.0], [2.0, 0.0]])


def test_a_first_pivot_that_fails_leaves_nothing(prov):
    a = ref.parent(200).copy()
    a[0, 0] = -1.0
    h = prov.upload(a)
    for lower in (False, True):
        got, info = factor(prov, h, lower)
        assert info == 1 and not got.any() and not np.signbit(got).any()
    prov.free(h)


def test_precision_32_provider(prov32, oracle, truth):
    a = ref.parent(200)
    h = prov32.upload(a)
    for lower in (False, True):
        got, info = factor(prov32, h, lower)
        want, want_info = factor(prov32, h, lower, entry=prov32.chol)
        assert info == 0 and want_info == 0 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), lower
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))  # f32 storage
    prov32.free(h)
    # a failed pivot: the device factors the widened f32 data, and so does the oracle here
    j = 129
    widened = ref.lowered(a, truth(200)[0], j).astype(np.float32).astype(np.float64)
    want, want_info = oracle.chol(widened)
    assert want_info == j + 1
    h = prov32.upload(widened)
    got, info = factor(prov32, h)
    low, low_info = factor(prov32, h, True)
    prov32.free(h)
    assert info == want_info and low_info == want_info
    assert np.array_equal(got != 0.0, want != 0.0) and np.array_equal(low, got.T)
    # kept entries: the f64 factor of the widened data rounded once to f32 - half an f32 ulp on top of the f64 bound, which is far below it
    assert np.max(np.abs(got - want)) <= 2.0 ** -23 * np.max(np.abs(want))


def test_the_panelled_update_before_a_failed_pivot(prov):
    """n = 4224 splits 2112 + 2112: the trailing update runs panel by panel.  The oracle's n^3 loop is too slow here, so the kept block is
    checked by R[:j, :j]' R[:j, :j] = A[:j, :j] (50 j eps max|A|, the residual bound of test_chol_matches_the_oracle) and the zero pattern."""
    n, j = 4224, 4000
    b = np.random.default_rng(n).standard_normal((n, 64))
    a = b @ b.T + n * np.eye(n)
    a = 0.5 * (a + a.T)
    a[j, j] = -1.0
    h = prov.upload(a)
    got, info = factor(prov, h)
    low, low_info = factor(prov, h, True)
    prov.free(h)
    assert info == j + 1 and low_info == j + 1
    assert not np.isnan(got).any()
    assert np.array_equal(got != 0.0, ref.keep_mask(n, "P", j))
    r = got[:j, :j]
    resid = float(np.max(np.abs(r.T @ r - a[:j, :j])))
    print(f"chol_info n={n} P{j}: max |R'R - A| = {resid:.3e}, bound {50 * j * EPS * np.max(np.abs(a)):.3e}")
    assert resid <= 50 * j * EPS * np.max(np.abs(a))
    # column j above the pivot: R[:j, :j]' R[:j, j] = A[:j, j]
    assert np.max(np.abs(r.T @ got[:j, j] - a[:j, j])) <= 50 * j * EPS * np.max(np.abs(a))
    assert np.array_equal(low, got.T)
