"""GPU checks of `qr` (rmhip_qr, runmat_amd/csrc/qr.hip) against the numpy restatement of the reference's CPU builtin (tests/qr_host.py)."""
import math

import numpy as np
import pytest

from qr_host import qr_host
from runmat_amd import HipProvider, ProviderError, ProviderQrOptions, ProviderQrPivot

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NB = 32  # reflectors per panel of Q (qr.hip kQrNb)


def fmat(values, rows, cols):
    return np.array(values, dtype=np.float64).reshape((rows, cols), order="F")


def run(prov, A, economy=False, vector=False, shape=None):
    h = prov.upload(A, shape)
    res = prov.qr(h, ProviderQrOptions(economy, ProviderQrPivot.Vector() if vector else ProviderQrPivot.Matrix()))
    out = tuple(prov.download_matrix(x) for x in (res.q, res.r, res.perm_matrix, res.perm_vector))
    for x in (h, res.q, res.r, res.perm_matrix, res.perm_vector):
        prov.free(x)
    return out


def assert_matches(got, want, tol, A):
    Q, R, E, pv = got
    scale = max(1.0, float(np.linalg.norm(A)))
    assert Q.shape == want.q.shape and R.shape == want.r.shape
    assert E.shape == want.perm_matrix.shape and pv.shape == want.perm_vector.shape
    assert np.array_equal(pv, want.perm_vector), (pv.ravel(), want.perm_vector.ravel())
    assert np.array_equal(E, want.perm_matrix)
    assert np.max(np.abs(Q - want.q), initial=0.0) <= tol
    assert np.max(np.abs(R - want.r), initial=0.0) <= tol * scale


def check_structure(A, got, economy):
    Q, R, E, pv = got
    m, n = A.shape
    p = min(m, n)
    econ = economy and m >= n
    assert Q.shape == ((m, n) if econ else (m, m)) and R.shape == ((n, n) if econ else (m, n))
    assert E.shape == (n, n) and pv.shape == (n, 1)
    perm = pv[:, 0].astype(np.int64) - 1
    assert sorted(perm.tolist()) == list(range(n))
    assert np.array_equal(E, np.eye(n)[:, perm])
    assert np.all(np.tril(R, -1) == 0.0)
    d = np.abs(np.diag(R))[:p]
    assert np.all(d[1:] <= d[:-1] * (1 + 1e-12) + 1e-300)
    na = np.linalg.norm(A)
    assert np.linalg.norm(A @ E - Q @ R) <= 20 * max(m, n) * EPS * max(na, 1e-300)
    assert np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1])), initial=0.0) <= 20 * m * EPS


KATS = [
    fmat([1, 4, 2, 5], 2, 2),
    fmat([1, 1, 1, 0, 1, 1], 3, 2),
    fmat([1, 1, 0, 1, 1, 0], 3, 2),
    fmat(range(1, 13), 4, 3),
    fmat(range(1, 13), 3, 4),
    fmat([3, 0, 4, 4, 0, 5], 3, 2),  # a zero row
    np.eye(1), np.eye(3), np.eye(5), np.eye(4)[:, :3], np.eye(4)[:3, :],
    np.zeros((3, 4)), np.zeros((4, 3)), np.zeros((1, 1)),
    fmat([1, 2, 3, 4, 0, 1, -1, 2, 1, 2, 3, 4], 4, 3),  # columns 0 and 2 identical: the tie goes to column 2
    fmat([2, -1, 3, 2, -1, 3, 2, -1, 3], 3, 3),  # three identical columns
]


def test_eye3_perm_vector(prov):
    Q, R, E, pv = run(prov, np.eye(3))
    assert pv.ravel().tolist() == [3.0, 1.0, 2.0]


@pytest.mark.parametrize("economy", [False, True])
def test_reference_kats(prov, economy):
    for A in KATS:
        got = run(prov, A, economy)
        assert_matches(got, qr_host(A, economy), 1e-12, A)


def test_quirks(prov):
    cases = [
        np.array([[-2.0, 0.5], [1e-7, 0.1]]),  # tail^2 <= 1e-12, alpha < 0: reflects, R(0,0) > 0
        np.array([[2.0, 0.5], [1e-7, 0.1]]),  # tail^2 <= 1e-12, alpha >= 0: tail dropped, tau 0
        np.array([[1e-13, 0.0], [1e-7, 0.0]]),  # tiny alpha and tail: the column is zeroed
        np.array([[3.0, 1.0, -4.0], [0.0, 2.0, 1e-8]]),  # last row of a wide matrix: one-element reflector
        1e-7 * np.random.default_rng(3).standard_normal((6, 4)),  # every norm below 1e-12
    ]
    for A in cases:
        for economy in (False, True):
            got = run(prov, A, economy)
            want = qr_host(A, economy)
            assert_matches(got, want, 1e-12, A)
            assert np.array_equal(got[1] == 0.0, want.r == 0.0), A
            assert np.array_equal(got[0] == 0.0, want.q == 0.0), A


SHAPES = [(1, 1), (1, 7), (7, 1), (3, 2), (2, 3), (64, 64), (65, 63), (257, 129), (129, 257), (512, 512), (1000, 37), (37, 1000)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("economy", [False, True])
def test_shape_sweep(prov, shape, economy):
    rng = np.random.default_rng(shape[0] * 1009 + shape[1])
    A = rng.standard_normal(shape)
    got = run(prov, A, economy)
    check_structure(A, got, economy)
    want = qr_host(A, economy)
    if all(g > 1e-10 for g in want.gaps):
        assert_matches(got, want, 1e-10 * max(1.0, np.linalg.norm(A)), A)


def test_graded_columns_match_exactly_in_perm(prov):
    rng = np.random.default_rng(11)
    A = rng.standard_normal((300, 90)) * np.logspace(0, -4, 90)[rng.permutation(90)]
    want = qr_host(A, True)
    assert min(want.gaps) > 1e-6
    assert_matches(run(prov, A, True), want, 1e-10, A)


def _device_structure(prov, A, economy):
    m, n = A.shape
    ha = prov.upload(A)
    res = prov.qr(ha, ProviderQrOptions(economy, ProviderQrPivot.Matrix()))
    ae = prov.matmul(ha, res.perm_matrix)
    qr = prov.matmul(res.q, res.r)
    qt = prov.transpose(res.q)
    qtq = prov.matmul(qt, res.q)
    r = prov.download_matrix(res.r)
    pv = prov.download_matrix(res.perm_vector)
    diff = np.linalg.norm(prov.download_matrix(ae) - prov.download_matrix(qr))
    orth = np.max(np.abs(prov.download_matrix(qtq) - np.eye(qtq.shape[0])))
    for h in (ha, res.q, res.r, res.perm_matrix, res.perm_vector, ae, qr, qt, qtq):
        prov.free(h)
    p = min(m, n)
    assert sorted((pv[:, 0] - 1).astype(int).tolist()) == list(range(n))
    assert np.all(np.tril(r, -1) == 0.0)
    d = np.abs(np.diag(r))[:p]
    assert np.all(d[1:] <= d[:-1] * (1 + 1e-12))
    assert diff <= 20 * max(m, n) * EPS * np.linalg.norm(A), diff
    assert orth <= 20 * m * EPS, orth


@pytest.mark.parametrize("m,n,economy", [(4096, 4096, True), (2048, 2048, False), (100000, 64, True)])
def test_large(prov, m, n, economy):
    A = np.random.default_rng(m + n).standard_normal((m, n))
    _device_structure(prov, A, economy)


def test_no_host_round_trip_and_launch_budget(prov):
    A = np.random.default_rng(5).standard_normal((300, 200))
    h = prov.upload(A)
    t0 = prov.telemetry_snapshot()
    res = prov.qr(h, ProviderQrOptions(True))
    t1 = prov.telemetry_snapshot()
    p = 200
    assert t1["download_bytes"] == t0["download_bytes"]
    assert t1["kernel_launches"] - t0["kernel_launches"] <= 4 * p + 64 * math.ceil(p / NB) + 64
    for x in (h, res.q, res.r, res.perm_matrix, res.perm_vector):
        prov.free(x)


def test_deterministic(prov):
    A = np.random.default_rng(8).standard_normal((700, 300))
    a, b = run(prov, A, True), run(prov, A, True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_power_iteration_loop(prov):
    n, k = 2048, 16
    rng = np.random.default_rng(21)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = 2.0 ** -np.arange(n, dtype=np.float64)
    G = (U * lam) @ U.T
    G = 0.5 * (G + G.T)
    Q0, _ = np.linalg.qr(U[:, :k] + 1e-3 * rng.standard_normal((n, k)))
    hg, hq = prov.upload(G), prov.upload(Q0)
    want = Q0
    for _ in range(5):
        prod = prov.matmul(hg, hq)
        res = prov.qr(prod, ProviderQrOptions(True))
        prov.free(prod)
        for x in (hq, res.r, res.perm_matrix, res.perm_vector):
            prov.free(x)
        hq = res.q
        ref = qr_host(G @ want, economy=True)
        assert min(ref.gaps) > 1e-3
        want = ref.q
    got = prov.download_matrix(hq)
    prov.free(hg)
    prov.free(hq)
    assert np.max(np.abs(got - want)) <= 1e-10


def test_precision32():
    A = np.random.default_rng(2).standard_normal((90, 40)) * np.logspace(0, -2, 40)
    want = qr_host(A.astype(np.float32).astype(np.float64), True)
    assert min(want.gaps) > 1e-3
    p32 = HipProvider(0, "F32")
    try:
        h = p32.upload(A)
        res = p32.qr(h, ProviderQrOptions(True, ProviderQrPivot.Vector()))
        assert p32.buffer_bits(res.q) == 32 and p32.buffer_bits(res.r) == 32
        Q, R, pv = (p32.download_matrix(x) for x in (res.q, res.r, res.perm_vector))
    finally:
        p32.close()
    assert np.array_equal(pv, want.perm_vector)
    assert np.array_equal(Q, want.q.astype(np.float32).astype(np.float64)) or np.max(np.abs(Q - want.q)) <= 1e-5
    assert np.max(np.abs(R - want.r)) <= 1e-5 * np.linalg.norm(A)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e200])
def test_refusals(prov, bad):
    A = np.ones((4, 3))
    A[2, 1] = bad
    h = prov.upload(A)
    with pytest.raises(ProviderError):
        prov.qr(h)
    prov.free(h)


def test_refuses_three_dimensions(prov):
    h = prov.upload(np.ones(8), (2, 2, 2))
    with pytest.raises(ProviderError):
        prov.qr(h)
    prov.free(h)


@pytest.mark.parametrize("m,n", [(0, 0), (3, 0), (0, 3)])
@pytest.mark.parametrize("economy", [False, True])
def test_empty_shapes(prov, m, n, economy):
    want = qr_host(np.zeros((m, n)), economy)
    h = prov.upload(np.zeros(m * n), (m, n))
    res = prov.qr(h, ProviderQrOptions(economy))
    assert res.q.shape == want.q.shape and res.r.shape == want.r.shape
    assert res.perm_matrix.shape == want.perm_matrix.shape and res.perm_vector.shape == want.perm_vector.shape
    if want.q.size:
        assert np.array_equal(prov.download_matrix(res.q), want.q)
    if want.perm_matrix.size:
        assert np.array_equal(prov.download_matrix(res.perm_matrix), want.perm_matrix)
        assert np.array_equal(prov.download_matrix(res.perm_vector), want.perm_vector)
    for x in (h, res.q, res.r, res.perm_matrix, res.perm_vector):
        prov.free(x)
