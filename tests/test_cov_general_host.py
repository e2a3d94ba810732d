"""Host checks of the general covariance form (cov(x, y), weighted cov): the NumPy model of `cov_from_tensors` (tests/cov_general_ref.py) against
the oracle's plain form and numpy.cov, its NaN and diagonal rules, and the bindings - the C ABI entry point as a second entry point of
`covariance`, the Python and C++ mirrors, the shim's dispatch."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import cov_general_ref as ref  # noqa: E402


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("rows,cols", [(1, 3), (2, 2), (4, 3), (257, 9), (1000, 7), (5000, 1)])
@pytest.mark.parametrize("biased", [False, True])
def test_model_is_the_oracle_on_the_plain_form(oracle, rows, cols, biased):
    x = np.random.default_rng(rows * 3 + cols).uniform(-1, 1, (rows, cols)) + np.arange(cols)
    x[:, 0] = 2.5  # a constant column: zero products of either sign
    assert np.array_equal(bits(ref.cov_general(x, biased=biased)), bits(oracle.covariance(x, biased)))
    if rows > 3:
        x[3, cols - 1] = np.inf
        got, want = ref.cov_general(x, biased=biased), oracle.covariance(x, biased)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got[~np.isnan(want)]), bits(want[~np.isnan(want)]))


def test_model_splits_columns_like_one_matrix():
    x = np.random.default_rng(5).standard_normal((300, 7))
    assert np.array_equal(bits(ref.cov_general(x[:, :4], x[:, 4:])), bits(ref.cov_general(x)))
    assert np.array_equal(bits(ref.cov_general(x[:, 0], x[:, 1])), bits(ref.cov_general(x[:, :2])))  # vectors are columns
    with pytest.raises(ValueError, match="same number of rows"):
        ref.cov_general(x, x[:-1])
    with pytest.raises(ValueError, match="expected 300 elements"):
        ref.cov_general(x, weights=np.ones(299))


@pytest.mark.parametrize("rows,c1,c2", [(4, 3, 0), (257, 5, 4), (1000, 2, 1)])
def test_model_matches_numpy_for_integer_weights(rows, c1, c2):
    rng = np.random.default_rng(rows + c1)
    x, y = rng.uniform(-1, 1, (rows, c1)) + np.arange(c1), rng.uniform(-1, 1, (rows, c2))
    w = rng.integers(0, 4, rows)
    w[0] = 3  # the sum of the weights exceeds 1
    got = ref.cov_general(x, y if c2 else None, weights=w.astype(np.float64), biased=True)  # `biased` is ignored with weights
    want = np.cov(np.concatenate([x, y], axis=1), rowvar=False, fweights=w).reshape(c1 + c2, c1 + c2)
    assert np.max(np.abs(got - want)) <= 1e-12
    assert np.array_equal(got, got.T)


def test_model_nan_and_diagonal_rules():
    x = np.random.default_rng(8).uniform(-1, 1, (40, 4))
    w = np.ones(40)
    assert np.all(np.isnan(ref.cov_general(x[:1], x[:1])))                                   # rows - 1 == 0
    assert not np.any(np.isnan(ref.cov_general(x[:1], x[:1], biased=True)))                  # rows == 1, biased: all zero
    assert ref.cov_general(np.zeros((5, 0))).shape == (0, 0)
    assert np.all(np.isnan(ref.cov_general(x, weights=np.zeros(40))))                         # sum_w <= 0
    one = np.zeros(40)
    one[3] = 1.0
    assert np.all(np.isnan(ref.cov_general(x, weights=one)))                                  # sum_w - 1 <= 0
    one[4] = 0.25
    assert np.all(np.isfinite(ref.cov_general(x, weights=one)))                               # sum_w == 1.25
    for bad, wt in ((np.inf, 1.0), (np.nan, 0.0)):  # a zero weight does not shield a non-finite value: the column's mean refuses it
        xn, wn = x.copy(), w.copy()
        xn[7, 2], wn[7] = bad, wt
        c = ref.cov_general(xn, weights=wn)
        want_nan = np.zeros((4, 4), dtype=bool)
        want_nan[2, :] = want_nan[:, 2] = True
        assert np.array_equal(np.isnan(c), want_nan)
        assert np.array_equal(np.isnan(ref.cov_general(xn[:, :2], xn[:, 2:])), want_nan)
    assert ref.sanitize(True, -1e-13) == 0.0 and ref.sanitize(False, -1e-13) == -1e-13
    assert ref.sanitize(True, -1e-12) == -1e-12 and ref.sanitize(True, 3.0) == 3.0 and np.isnan(ref.sanitize(True, np.nan))
    const = x.copy()
    const[:, 1] = 0.1 + 0.2  # a constant column: variance exactly 0 or +tiny, never negative
    assert ref.cov_general(const, weights=w)[1, 1] >= 0.0


def test_entry_point_is_a_second_entry_point_of_covariance():
    from runmat_amd import HipProvider, _lib

    assert "rmhip_covariance_general" in _lib.SIGNATURES
    assert _lib.SERVES["rmhip_covariance_general"] == ("covariance",) == _lib.SERVES["rmhip_covariance"]
    from runmat_amd._abi import ARG_NAMES

    assert ARG_NAMES["rmhip_covariance_general"] ==("ctx", "matrix", "second_or_0", "weights_or_0", "biased", "out")
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "covariance_general", None))


def test_the_cpp_mirror_and_the_shim_call_the_entry_point():
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    assert re.search(r"\bcovariance_general\(", hpp) and "rmhip_covariance_general(ctx_" in hpp
    assert "covariance_general(" in (ROOT / "examples" / "provider_kats.cpp").read_text()
    assert "pub fn rmhip_covariance_general(" in (ROOT / "shim" / "rmhip_sys.rs").read_text()
    src = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = src[src.index("fn covariance<'a>"):src.index("fn covariance_to_correlation")]
    assert "rmhip_covariance_general(self.ctx" in body and "rmhip_covariance(self.ctx" in body
    refusal = body.index("options.rows != CovRows::All")  # the other rows modes are refused before either call
    assert "return Err(" in body[refusal:body.index("rmhip_covariance_general(self.ctx")]
    assert refusal < body.index("rmhip_covariance(self.ctx")
    assert re.search(r"has_weight_vector && weights\.is_none\(\)\s*\{\s*return Err\(", body)
