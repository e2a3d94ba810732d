"""CPU checks of `qr_power_iter`: the numpy model of the CholeskyQR2 algorithm (tests/qr_power_ref.py) accepts the accept grid within the
accuracy conditions the GPU test sets, and declines every case of the decline list; the two new entry points are bound in every mirror."""
import numpy as np
import pytest

from qr_power_ref import (ACCEPT_CONDS, ACCEPT_SCALE, ACCEPT_SHAPES, EPS, cholqr2, decline_cases, make_case, numpy_qr_positive, orth_error,
                          residual)


@pytest.mark.parametrize("m,k", ACCEPT_SHAPES)
def test_model_accepts_the_grid_within_the_conditions(m, k):
    for cond in ACCEPT_CONDS:
        rng = np.random.default_rng(1000 * m + 10 * k + int(np.log10(cond)))
        P = make_case(m, k, cond, rng, ACCEPT_SCALE)
        Q, R, why = cholqr2(P)
        assert Q is not None, (cond, why)
        Qn, Rn = numpy_qr_positive(P)
        cond2 = np.linalg.cond(P)
        assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0)
        assert orth_error(Q) <= 4.0 * max(orth_error(Qn), 4.0 * EPS), cond
        assert residual(Q, R, P) <= 4.0 * max(residual(Qn, Rn, P), 4.0 * EPS), cond
        assert np.abs(Q - Qn).max() <= 16.0 * cond2 * EPS, cond
        assert np.abs(R - Rn).max() <= 16.0 * cond2 * EPS * np.abs(Rn).max(), cond


@pytest.mark.parametrize("seed", range(4))
def test_model_declines_the_decline_list(seed):
    rng = np.random.default_rng(seed)
    for name, P in decline_cases(rng).items():
        Q, R, why = cholqr2(P)
        assert Q is None, (name, why)
    for cond in (1e12, 1e14):
        assert cholqr2(make_case(257, 8, cond, rng))[0] is None, cond
    P = rng.standard_normal((257, 8))
    P[:, 7] = P[:, 0] + P[:, 1]  # a column equal to the sum of two others
    assert cholqr2(P)[0] is None
    assert cholqr2(rng.standard_normal((8, 17)))[2] == "shape" and cholqr2(rng.standard_normal((100, 65)))[2] == "shape"


def test_both_entry_points_are_bound():
    from runmat_amd import HipProvider, _lib

    assert "rmhip_qr_power_iter" in _lib.SIGNATURES and "rmhip_take_matmul_sources" in _lib.SIGNATURES
    assert _lib.SERVES["rmhip_qr_power_iter"] == ("qr_power_iter",)
    assert _lib.SERVES["rmhip_take_matmul_sources"] == ("take_matmul_sources",)
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "qr_power_iter", None)) and callable(getattr(HipProvider, "take_matmul_sources", None))
    assert len(_lib.SIGNATURES["rmhip_qr_power_iter"][1]) == 8 and len(_lib.SIGNATURES["rmhip_take_matmul_sources"][1]) == 5
