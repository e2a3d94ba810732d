"""Seeded symmetric test matrices and the acceptance bounds of `eig` (rmhip_eig, runmat_amd/csrc/eig.hip), shared by
test_eig_host.py (LAPACK against the same bounds) and test_gpu_eig.py.  Every builder returns a bitwise symmetric float64 matrix."""
import numpy as np

EPS = 2.0 ** -52
SIZES = (2, 3, 7, 33, 63, 64, 65, 96, 130, 200)  # odd padding player, the LDS boundary, first blocked size, ragged last block, odd block count
LARGE = (("uniform", 520), ("clusters", 520))


def _sym(a):
    return 0.5 * (a + a.T)


def _orth(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


def uniform(n, rng):
    return _sym(rng.uniform(-1.0, 1.0, (n, n)))


def covariance(n, rng):
    return _sym(np.atleast_2d(np.cov(rng.standard_normal((3 * n + 5, n)), rowvar=False)))


def plus_minus_one(n, rng):
    q = _orth(rng, n)
    return _sym((q * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)) @ q.T)


def graded(n, rng):
    q = _orth(rng, n)
    return _sym((q * np.logspace(0.0, -12.0, n)) @ q.T)


def clusters(n, rng):
    q = _orth(rng, n)
    return _sym((q * (1.0 + (np.arange(n) // 4))) @ q.T)


def exchange(n, rng):
    return np.fliplr(np.eye(n)).copy()


def ones(n, rng):
    return np.ones((n, n))


def neg_ones(n, rng):
    return -np.ones((n, n))  # eigenvalue -n sits at -||A||_inf: a shift by the norm alone would make the shifted matrix singular


def laplacian(n, rng):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def diagonal(n, rng):
    return np.diag(rng.permutation(np.arange(n) - n // 3).astype(np.float64))


FAMILIES = {f.__name__: f for f in (uniform, covariance, plus_minus_one, graded, clusters, exchange, ones, neg_ones, laplacian, diagonal)}
_cache = {}


def case(family, n):
    """The matrix of (family, n) and LAPACK's ascending eigenvalues for it, computed once; both are read-only."""
    key = (family, n)
    if key not in _cache:
        a = FAMILIES[family](n, np.random.default_rng(1000 * sorted(FAMILIES).index(family) + n))
        assert np.array_equal(a, a.T)
        w = np.linalg.eigvalsh(a)
        a.setflags(write=False)
        w.setflags(write=False)
        _cache[key] = (a, w)
    return _cache[key]


def all_cases():
    return [(f, n) for f in FAMILIES for n in SIZES] + list(LARGE)


def figures(a, w_ref, lam, v):
    """(E, R, O) as ratios to their bounds' scales: |lam - lam_ref| / ||A||_2, ||A V - V diag(lam)||_F / ||A||_F, max |V'V - I|."""
    n = a.shape[0]
    n2 = max(float(np.max(np.abs(w_ref), initial=0.0)), 1e-300)
    nf = max(float(np.linalg.norm(a)), 1e-300)
    e = float(np.max(np.abs(lam - w_ref), initial=0.0)) / n2
    r = float(np.linalg.norm(a @ v - v * lam)) / nf
    o = float(np.max(np.abs(v.T @ v - np.eye(n)), initial=0.0))
    return e, r, o


def check_f64(a, w_ref, lam, v):
    """(E) max |lam - lam_ref| <= max(1e-12, 20 n eps) ||A||_2, (R) ||A V - V diag(lam)||_F <= 20 n eps ||A||_F,
    (O) max |V'V - I| <= 20 n eps; eigenvalues ascending."""
    n = a.shape[0]
    e, r, o = figures(a, w_ref, lam, v)
    assert np.all(lam[1:] >= lam[:-1]), "eigenvalues are not ascending"
    assert e <= max(1e-12, 20 * n * EPS), ("E", e, 20 * n * EPS)
    assert r <= 20 * n * EPS, ("R", r, 20 * n * EPS)
    assert o <= 20 * n * EPS, ("O", o, 20 * n * EPS)


def check_f32(a, w_ref, lam, v):
    """The reference's F32 tolerance for all three: 1e-5 max(1, ||A||_2)."""
    n = a.shape[0]
    tol = 1e-5 * max(1.0, float(np.max(np.abs(w_ref), initial=0.0)))
    assert np.all(lam[1:] >= lam[:-1])
    assert np.max(np.abs(lam - w_ref), initial=0.0) <= tol
    assert np.linalg.norm(a @ v - v * lam) <= tol
    assert np.max(np.abs(v.T @ v - np.eye(n)), initial=0.0) <= tol
