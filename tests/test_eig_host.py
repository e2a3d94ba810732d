"""CPU checks around `eig` (rmhip_eig): the surface exists in the Python mirror, LAPACK itself meets the bounds of tests/eig_cases.py on
every case the GPU tests use (so a GPU failure cannot be blamed on the inputs), and the reason the blocked path shifts the matrix."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import eig_cases  # noqa: E402


def test_surface():
    import runmat_amd
    from runmat_amd import HipProvider, _lib

    assert callable(getattr(HipProvider, "eig", None))
    assert "eig" in {m for methods in _lib.SERVES.values() for m in methods}
    assert "ProviderEigResult" in runmat_amd.__all__
    fields = list(runmat_amd.ProviderEigResult.__dataclass_fields__)
    assert fields == ["eigenvalues", "diagonal", "right", "left"]
    assert _lib.SIGNATURES["rmhip_eig"][1][2:] == _lib.SIGNATURES["rmhip_qr"][1][3:]  # (ctx, a, compute_left, out4)


@pytest.mark.parametrize("family,n", eig_cases.all_cases())
def test_lapack_meets_the_bounds(family, n):
    a, w_ref = eig_cases.case(family, n)
    w, v = np.linalg.eigh(a)
    eig_cases.check_f64(a, w_ref, w, v)


def test_cases_are_symmetric_and_cover_both_signs():
    for family, n in eig_cases.all_cases():
        a, w = eig_cases.case(family, n)
        assert a.shape == (n, n) and np.array_equal(a, a.T) and np.all(np.isfinite(a))
    assert eig_cases.case("plus_minus_one", 64)[1][0] < -0.99 and eig_cases.case("neg_ones", 65)[1][0] == pytest.approx(-65.0)


def _one_sided_jacobi(a, sweeps=30):
    """The naive iteration: rotate column pairs of W = A until they are orthogonal, V accumulates the rotations."""
    w = a.astype(np.float64).copy()
    n = a.shape[0]
    v = np.eye(n)
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                alpha, beta, gamma = w[:, p] @ w[:, p], w[:, q] @ w[:, q], w[:, p] @ w[:, q]
                if gamma == 0.0 or abs(gamma) < 1e-15 * np.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                for m in (w, v):
                    x, y = m[:, p].copy(), m[:, q].copy()
                    m[:, p], m[:, q] = c * x - s * y, s * x + c * y
        if not rotated:
            break
    return w, v


def test_one_sided_jacobi_needs_the_shift():
    """[0 1; 1 0] has orthogonal columns already: the one-sided iteration stops at once with V = I, which holds no eigenvector of the
    matrix (+1 and -1 share a singular value).  On A + s I with s above ||A||_inf the same iteration finds them."""
    a = np.array([[0.0, 1.0], [1.0, 0.0]])
    _, v = _one_sided_jacobi(a)
    assert np.array_equal(v, np.eye(2))
    assert np.linalg.norm(a @ v - v * np.diag(v.T @ a @ v)) > 0.5
    _, v = _one_sided_jacobi(a + 1.5 * np.eye(2))
    lam = np.diag(v.T @ a @ v)
    assert np.linalg.norm(a @ v - v * lam) <= 1e-15
    assert sorted(np.round(lam, 12).tolist()) == [-1.0, 1.0]
