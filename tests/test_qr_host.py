"""CPU checks of the numpy restatement of the reference's `qr` builtin (tests/qr_host.py), the yardstick of tests/test_gpu_qr.py."""
import numpy as np
import pytest

from qr_host import EPS_CLEAN, householder, qr_host

scipy_linalg = pytest.importorskip("scipy.linalg")


def fmat(values, rows, cols):
    return np.array(values, dtype=np.float64).reshape((rows, cols), order="F")


def check_structure(A, res, tol=1e-10):
    Q, R, E = res.q, res.r, res.perm_matrix
    assert np.allclose(Q.T @ Q, np.eye(Q.shape[1]), atol=tol)
    assert np.allclose(Q @ R, A @ E, atol=tol)


def test_reference_unit_test_properties():
    # qr_single_output_returns_upper_triangular
    A = fmat([1, 4, 2, 5], 2, 2)
    res = qr_host(A)
    assert np.array_equal(res.r, np.triu(res.r))
    # qr_three_outputs_reconstructs_input
    A = fmat([1, 1, 1, 0, 1, 1], 3, 2)
    res = qr_host(A)
    assert res.q.shape == (3, 3) and res.r.shape == (3, 2) and res.perm_matrix.shape == (2, 2)
    check_structure(A, res)
    # qr_vector_option_returns_pivot_vector
    res = qr_host(fmat([1, 1, 0, 1, 1, 0], 3, 2))
    assert res.perm_vector.shape == (2, 1) and set(res.perm_vector[:, 0]) == {1.0, 2.0}
    # qr_economy_shapes_for_tall_matrix
    econ = qr_host(fmat(range(1, 13), 4, 3), economy=True)
    assert econ.q.shape == (4, 3) and econ.r.shape == (3, 3)
    # qr_economy_wide_matrix_matches_full
    A = fmat(range(1, 13), 3, 4)
    full, econ = qr_host(A), qr_host(A, economy=True)
    assert np.allclose(full.q, econ.q, atol=1e-10) and np.allclose(full.r, econ.r, atol=1e-10)
    # the wgpu parity matrix with a zero row
    A = fmat([3, 0, 4, 4, 0, 5], 3, 2)
    check_structure(A, qr_host(A))


def test_eye3_ties_resolve_to_the_last_index():
    res = qr_host(np.eye(3))
    assert res.perm_vector[:, 0].tolist() == [3.0, 1.0, 2.0]
    assert res.perm_vector.shape == (3, 1)
    E = res.perm_matrix
    assert all(E[int(res.perm_vector[c, 0]) - 1, c] == 1.0 for c in range(3))
    check_structure(np.eye(3), res)


def test_householder_quirks():
    col = np.array([-2.0, 1e-7])  # tail^2 <= 1e-12 with a negative alpha still reflects
    tau = householder(col)
    assert abs(tau - 2.0) <= 1e-12 and col[0] > 0.0 and col[1] != 0.0
    col = np.array([-3.0])  # no tail at all (the last row of a square or wide matrix): a negative alpha reflects to |alpha|
    assert householder(col) == 2.0 and col[0] == 3.0
    col = np.array([2.0, 1e-7])  # ... a non-negative alpha drops the tail
    assert householder(col) == 0.0 and col.tolist() == [2.0, 0.0]
    col = np.array([1e-13, 1e-7])  # tiny alpha and tail: the column is zeroed
    assert householder(col) == 0.0 and col.tolist() == [0.0, 0.0]
    col = np.array([0.0, 3.0, 4.0])  # sign +1 for alpha = 0: beta = -5
    assert householder(col) == 1.0 and col[0] == -5.0


def test_empty_shapes():
    for (m, n) in [(0, 0), (3, 0), (0, 3)]:
        full, econ = qr_host(np.zeros((m, n))), qr_host(np.zeros((m, n)), economy=True)
        assert full.q.shape == (m, m) and np.array_equal(full.q, np.eye(m))
        assert full.r.shape == (m, n)
        assert full.perm_matrix.shape == (n, n) and full.perm_vector.shape == (n, 1)
        assert econ.q.shape == ((m, n) if m >= n else (m, m)) and econ.r.shape == ((n, n) if m >= n else (m, n))


@pytest.mark.parametrize("shape", [(6, 4), (40, 17), (17, 40), (64, 64), (200, 31)])
def test_matches_lapack_pivoted_qr_where_pivots_are_separated(shape):
    rng = np.random.default_rng(sum(shape))
    tried = 0
    for _ in range(20):
        A = rng.standard_normal(shape) * np.logspace(0, -3, shape[1])  # graded columns separate the pivots
        res = qr_host(A)
        if min(res.gaps) <= 1e-6:
            continue
        tried += 1
        Q, R, P = scipy_linalg.qr(A, pivoting=True)
        m, n = shape
        if m <= n and R[m - 1, m - 1] < 0.0:  # dlarfg leaves a one-element column alone; the builtin reflects it (tau = 2)
            R[m - 1, :] = -R[m - 1, :]
            Q[:, m - 1] = -Q[:, m - 1]
        assert np.array_equal(res.perm, P)
        nrm = np.linalg.norm(A)
        assert np.max(np.abs(res.r - R)) <= 1e-12 * nrm
        assert np.max(np.abs(res.q - Q)) <= 1e-12 * max(1.0, np.sqrt(shape[0]))
        if tried >= 3:
            break
    assert tried > 0


def test_clean_zeroes_tiny_entries():
    A = np.array([[1.0, 1e-13], [0.0, 1.0]])
    res = qr_host(A)
    assert np.all((res.r == 0.0) | (np.abs(res.r) > EPS_CLEAN))
    assert np.all((res.q == 0.0) | (np.abs(res.q) > EPS_CLEAN))
