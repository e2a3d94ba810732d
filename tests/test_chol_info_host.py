"""CPU checks of `rmhip_chol_info`: the expectations the GPU tests use (tests/chol_info_ref.py: a piece of the parent's factor, exact
zeros elsewhere) are what oracle.chol returns for every case, at n = 200 and n = 2049; and the entry point is bound in every mirror
without changing the served set."""
import re
from pathlib import Path

import numpy as np
import pytest

import chol_info_ref as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def factors(oracle):
    out = {}
    for n in (200, 2049):
        r0, info = oracle.chol(ref.parent(n))
        assert info == 0
        out[n] = r0
    return out


def check_case(oracle, case, r0):
    n = r0.shape[0]
    got, info = oracle.chol(case.a)
    want_info, want = ref.expected(r0, case.kind, case.col)
    assert info == want_info, (case.name, info)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), case.name  # kept entries bit-equal to the parent's, zeros exact
    assert np.array_equal(got != 0.0, ref.keep_mask(n, case.kind, case.col)), case.name


@pytest.mark.parametrize("n", [200, 2049])
def test_a_failed_pivot_keeps_the_parents_columns_and_the_column_above_it(oracle, factors, n):
    assert min(factors[n][j, j] ** 2 for j in range(n)) > 100.0  # every pivot of the parent is far from the tests' thresholds
    for case in ref.pivot_cases(n, factors[n]):
        check_case(oracle, case, factors[n])


def test_asymmetry_reports_its_column_and_leaves_it_unformed(oracle, factors):
    cases = ref.asymmetry_cases(factors[200])
    assert len(cases) == 2 * len(ref.A_PAIRS) + 3
    for case in cases:
        check_case(oracle, case, factors[200])
        if case.kind == "A":
            assert not oracle.chol(case.a)[0][:, case.col].any()


def test_non_finite_entries(oracle, factors):
    for case in ref.nonfinite_cases():
        check_case(oracle, case, factors[200])
        assert not np.isnan(oracle.chol(case.a)[0]).any()


def test_tiny_pivots(oracle):
    for name, a, t, declined in ref.tiny_cases():
        r, info = oracle.chol(a)
        assert info == (t + 1 if declined else 0), name  # the denominator test of column t + 1 reports row t
        if not declined:
            assert r[t, t] == 1e-13
    r, info = oracle.chol(np.diag([1.0, 1.0, 1e-26, 1.0, 1.0]))
    assert info == 3 and not r[2:, :].any() and np.array_equal(r[:2, :2], np.eye(2))
    r, info = oracle.chol(np.diag([1.0, 1.0, 1.0, 1.0, 1e-26]))
    assert info == 0 and r[4, 4] == 1e-13


def test_reference_kat_and_first_pivot(oracle):
    r, info = oracle.chol(np.array([[1.0, 2.0], [2.0, 1.0]]))  # chol_gpu_failure_flag, chol.rs:1008-1021
    assert info == 2 and np.array_equal(r, [[1.0, 2.0], [0.0, 0.0]])
    a = ref.parent(200).copy()
    a[0, 0] = -1.0
    r, info = oracle.chol(a)
    assert info == 1 and not r.any()


def test_the_entry_point_is_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    assert _lib.SERVES["rmhip_chol_info"] == ("chol",) == _lib.SERVES["rmhip_chol"]
    assert _lib.SIGNATURES["rmhip_chol_info"] == _lib.SIGNATURES["rmhip_chol"]
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "chol_info", None))


def test_the_mirrors_carry_the_entry_point():
    assert "chol_info(" in (ROOT / "include" / "rmhip_provider.hpp").read_text()
    assert "chol_info(" in (ROOT / "examples" / "provider_kats.cpp").read_text()
    assert "pub fn rmhip_chol_info(" in (ROOT / "shim" / "rmhip_sys.rs").read_text()
    assert "def chol_info(" in (ROOT / "runmat_amd" / "provider.py").read_text()
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index("fn chol<"):]
    body = body[:re.search(r"\n    fn ", body).start()]
    assert "rmhip_chol_info(self.ctx" in body and "rmhip_chol(self.ctx" not in body  # the second entry point alone: no double factorisation
