"""GPU checks of `eig` (rmhip_eig, runmat_amd/csrc/eig.hip) for real symmetric matrices against LAPACK (numpy.linalg.eigh / eigvalsh)
under the bounds of tests/eig_cases.py: (E) eigenvalues, (R) residual, (O) orthogonality."""
import numpy as np
import pytest

import eig_cases
from eig_cases import EPS
from runmat_amd import HipProvider, ProviderError, _lib

pytestmark = pytest.mark.gpu


def run(prov, A, left=False, shape=None):
    """(eigenvalues [n], diagonal, right, left or None) downloaded; every handle freed."""
    h = prov.upload(A, shape)
    try:
        res = prov.eig(h, left)
    finally:
        prov.free(h)
    n = A.shape[0]
    assert res.eigenvalues.shape == ((n, 1) if n else (0, 0)) and res.diagonal.shape == (n, n) and res.right.shape == (n, n)
    assert (res.left is not None) == left
    out = [prov.download_matrix(x) for x in (res.eigenvalues, res.diagonal, res.right)]
    out.append(prov.download_matrix(res.left) if left else None)
    for x in (res.eigenvalues, res.diagonal, res.right) + ((res.left,) if left else ()):
        prov.free(x)
    return out[0].reshape(-1), out[1], out[2], out[3]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def live_bytes(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
def test_two_by_two(prov):
    lam, D, V, _ = run(prov, np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(lam, [1.0, 3.0], rtol=0, atol=4 * EPS)
    r = 1.0 / np.sqrt(2.0)
    assert np.allclose(np.abs(V), r, rtol=0, atol=4 * EPS)
    assert V[0, 0] * V[1, 0] < 0 and V[0, 1] * V[1, 1] > 0  # [1, -1] / sqrt 2 for 1, [1, 1] / sqrt 2 for 3
    assert np.array_equal(D, np.diag(lam))


def test_exchange_two(prov):
    lam, _, V, _ = run(prov, np.array([[0.0, 1.0], [1.0, 0.0]]))
    assert np.allclose(lam, [-1.0, 1.0], rtol=0, atol=4 * EPS)
    assert V[0, 0] * V[1, 0] < 0 and V[0, 1] * V[1, 1] > 0


def test_scalar_zero_identity(prov):
    lam, D, V, _ = run(prov, np.array([[5.0]]))
    assert lam.tolist() == [5.0] and D.tolist() == [[5.0]] and V.tolist() == [[1.0]]
    lam, D, V, _ = run(prov, np.zeros((3, 3)))
    assert np.array_equal(lam, np.zeros(3)) and np.array_equal(D, np.zeros((3, 3))) and np.array_equal(V, np.eye(3))
    lam, D, V, _ = run(prov, np.eye(5))
    assert np.array_equal(lam, np.ones(5)) and np.array_equal(D, np.eye(5)) and np.array_equal(V, np.eye(5))


def _assert_exact_diagonal(d, lam, V):
    n = d.size
    assert np.array_equal(lam, np.sort(d))
    assert np.all((V == 0.0) | (V == 1.0)) and np.array_equal(V.sum(axis=0), np.ones(n)) and np.array_equal(V.sum(axis=1), np.ones(n))
    assert np.array_equal(d[np.argmax(V, axis=0)], lam)


def test_diagonal_exact(prov):
    d = np.array([3.0, -1.0, 2.0, -1.0])
    lam, _, V, _ = run(prov, np.diag(d))
    assert lam.tolist() == [-1.0, -1.0, 2.0, 3.0]
    _assert_exact_diagonal(d, lam, V)
    assert np.argmax(V, axis=0).tolist() == [1, 3, 2, 0]  # the sort is stable


@pytest.mark.parametrize("n", [64, 65])
def test_unsorted_diagonal_exact_both_paths(prov, n):
    A, _ = eig_cases.case("diagonal", n)
    lam, D, V, _ = run(prov, A)
    _assert_exact_diagonal(np.diag(A).copy(), lam, V)
    assert np.array_equal(D, np.diag(lam))


# ---- shape sweep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n", eig_cases.all_cases())
def test_shape_sweep(prov, family, n):
    A, w_ref = eig_cases.case(family, n)
    h = prov.upload(A)
    res = prov.eig(h)
    assert res.eigenvalues.shape == (n, 1) and res.diagonal.shape == (n, n) and res.right.shape == (n, n) and res.left is None
    lam = prov.download_matrix(res.eigenvalues).reshape(-1)
    D, V, back = prov.download_matrix(res.diagonal), prov.download_matrix(res.right), prov.download_matrix(h)
    for x in (h, res.eigenvalues, res.diagonal, res.right):
        prov.free(x)
    print("eig figures", family, n, eig_cases.figures(A, w_ref, lam, V), "bound", 20 * n * EPS)
    assert np.array_equal(bits(back), bits(A))  # the input buffer is untouched
    assert np.array_equal(bits(D), bits(np.diag(lam)))
    eig_cases.check_f64(A, w_ref, lam, V)


# ---- +lambda / -lambda pairs share a singular value: both paths must keep their vectors apart -----------------------------------------------
@pytest.mark.parametrize("n", [64, 65])
def test_exchange_matrix(prov, n):
    A, w_ref = eig_cases.case("exchange", n)
    lam, _, V, _ = run(prov, A)
    assert np.allclose(np.abs(lam), 1.0, rtol=0, atol=20 * n * EPS) and np.sum(lam < 0) == n // 2
    eig_cases.check_f64(A, w_ref, lam, V)


def test_kron_plus_minus(prov):
    M, _ = eig_cases.case("uniform", 40)
    A = np.kron(np.array([[0.0, 1.0], [1.0, 0.0]]), M)
    w_ref = np.linalg.eigvalsh(A)
    lam, _, V, _ = run(prov, A)
    eig_cases.check_f64(A, w_ref, lam, V)
    assert np.max(np.abs(lam + lam[::-1])) <= 2 * max(1e-12, 20 * 80 * EPS) * np.max(np.abs(w_ref))  # symmetric about zero: (E) twice


# ---- left vectors, scaling, determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 130])
def test_left_vectors(prov, n):
    A, _ = eig_cases.case("uniform", n)
    h = prov.upload(A)
    res = prov.eig(h, True)
    none = prov.eig(h, False)
    assert res.left is not None and res.left.buffer_id != res.right.buffer_id and res.left.shape == (n, n)
    assert none.left is None
    assert np.array_equal(bits(prov.download(res.left)), bits(prov.download(res.right)))
    for x in (h, res.eigenvalues, res.diagonal, res.right, res.left, none.eigenvalues, none.diagonal, none.right):
        prov.free(x)


@pytest.mark.parametrize("n", [33, 130])
def test_scale_equivariance(prov, n):
    A, _ = eig_cases.case("uniform", n)
    lam, _, V, _ = run(prov, A)
    for k in (-400, 300):
        s = 2.0 ** k
        lam_s, D_s, V_s, _ = run(prov, A * s)
        assert np.array_equal(bits(V_s), bits(V)), k
        assert np.array_equal(bits(lam_s), bits(lam * s)), k
        assert np.array_equal(bits(D_s), bits(np.diag(lam * s))), k


def test_deterministic(prov):
    A, _ = eig_cases.case("uniform", 130)
    a, b = run(prov, A, True), run(prov, A, True)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


# ---- launch budget of the one-launch path ---------------------------------------------------------------------------------------------------
def test_small_path_launch_budget(prov):
    deltas = []
    for n in (2, 64):
        A, _ = eig_cases.case("uniform", n)
        h = prov.upload(A)
        t0 = prov.telemetry_snapshot()
        res = prov.eig(h, True)
        t1 = prov.telemetry_snapshot()
        assert t1["download_bytes"] == t0["download_bytes"]
        deltas.append(t1["kernel_launches"] - t0["kernel_launches"])
        for x in (h, res.eigenvalues, res.diagonal, res.right, res.left):
            prov.free(x)
    assert deltas[0] == deltas[1] and 1 <= deltas[0] <= 8, deltas


# ---- the chain the surface leads to: covariance -> eig without leaving the device ---------------------------------------------------------------
def test_pca_chain_on_device(prov):
    n = 48
    X = prov.random_normal((2000, n))
    C0 = prov.covariance(X)
    Ct = prov.transpose(C0)
    S = prov.elem_add(C0, Ct)
    C = prov.scalar_mul(S, 0.5)
    assert prov.issymmetric(C)
    res = prov.eig(C)
    Ch = prov.download_matrix(C)
    lam, V = prov.download_matrix(res.eigenvalues).reshape(-1), prov.download_matrix(res.right)
    for x in (X, C0, Ct, S, C, res.eigenvalues, res.diagonal, res.right):
        prov.free(x)
    w_ref = np.linalg.eigvalsh(Ch)
    eig_cases.check_f64(Ch, w_ref, lam, V)
    assert abs(np.sum(lam) - np.trace(Ch)) <= 20 * n * EPS * np.max(np.abs(w_ref))


# ---- precision 32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 96])
def test_precision32(n):
    A = eig_cases.case("uniform", n)[0].astype(np.float32).astype(np.float64)
    w_ref = np.linalg.eigvalsh(A)
    p32 = HipProvider(0, "F32")
    try:
        h = p32.upload(A)
        res = p32.eig(h, True)
        assert all(p32.buffer_bits(x) == 32 for x in (res.eigenvalues, res.diagonal, res.right, res.left))
        lam, V, L = p32.download_matrix(res.eigenvalues).reshape(-1), p32.download_matrix(res.right), p32.download_matrix(res.left)
    finally:
        p32.close()
    assert np.array_equal(bits(V), bits(L))
    eig_cases.check_f32(A, w_ref, lam, V)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _good_call(prov):
    lam, _, _, _ = run(prov, np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(lam, [1.0, 3.0], rtol=0, atol=4 * EPS)


def _refused(prov, h, code):
    before = live_bytes(prov)
    with pytest.raises(ProviderError) as err:
        prov.eig(h, True)
    assert err.value.code == code, (err.value.code, str(err.value))
    assert live_bytes(prov) == before
    _good_call(prov)
    assert live_bytes(prov) == before
    prov.free(h)


@pytest.mark.parametrize("n", [2, 70])
def test_refuses_nonsymmetric(prov, n):
    A = np.array(eig_cases.case("uniform", n)[0])
    if n == 2:
        A = np.array([[4.0, 1.0], [2.0, 3.0]])  # the reference's own provider test matrix
    else:
        A[3, 60] = np.nextafter(A[3, 60], 2.0)  # one ulp off
    _refused(prov, prov.upload(A), _lib.ERR_UNSUPPORTED)


@pytest.mark.parametrize("n", [3, 70])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_refuses_nonfinite(prov, n, bad):
    A = np.array(eig_cases.case("uniform", n)[0])
    A[1, 1] = bad
    _refused(prov, prov.upload(A), _lib.ERR_UNSUPPORTED)


def test_refuses_above_the_cap(prov):
    _refused(prov, prov.fill((4097, 4097), 0.0), _lib.ERR_UNSUPPORTED)


def test_refuses_complex(prov):
    r = prov.upload(np.eye(2))
    z = prov.complex_from_real(r)
    prov.free(r)
    _refused(prov, z, _lib.ERR_UNSUPPORTED)


def test_invalid_shapes(prov):
    _refused(prov, prov.upload(np.ones((3, 4))), _lib.ERR_INVALID)
    _refused(prov, prov.upload(np.ones(8), (2, 2, 2)), _lib.ERR_INVALID)


def test_trailing_unit_dimensions_are_a_matrix(prov):
    A, w_ref = eig_cases.case("uniform", 7)
    lam, _, V, _ = run(prov, A, shape=None)
    h = prov.upload(A.reshape(-1, order="F"), (7, 7, 1, 1))
    res = prov.eig(h)
    assert np.array_equal(bits(prov.download(res.eigenvalues)), bits(lam))
    for x in (h, res.eigenvalues, res.diagonal, res.right):
        prov.free(x)


def test_empty(prov):
    h = prov.upload(np.zeros(0), (0, 0))
    res = prov.eig(h, True)
    for x in (res.eigenvalues, res.diagonal, res.right, res.left):
        assert x.shape == (0, 0)
        prov.free(x)
    prov.free(h)
