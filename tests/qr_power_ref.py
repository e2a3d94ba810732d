"""Host model of `qr_power_iter` (runmat_amd/csrc/cholqr.hip) in numpy f64, and the generator of its test matrices.

CholeskyQR2 with the library's two verdicts:
    G1 = P'P,  R1 = chol(G1)  (verdict A: every pivot g_jj - sum r_pj^2 finite and > 0),  X1 = inv(R1) by back-substitution,  Q1 = P X1
    G2 = Q1'Q1,  verdict B: ||G2 - I||_F <= 1/2,  R2 = chol(G2) (verdict A again),  X2 = inv(R2),  Q = Q1 X2,  R = R2 R1
A failed verdict is a decline (`None`): the caller then runs the pivoted Householder `qr`.  The device sums the Gram matrices over row
slices in a fixed order of its own, so the model agrees with it to rounding, not bit for bit; the tests measure both against
numpy.linalg.qr.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
MAX_COLS = 64


def chol_upper(G):
    """Upper factor R of G = R'R, row by row with in-order dot products; None when a pivot is not finite and positive (verdict A)."""
    k = G.shape[0]
    R = np.zeros_like(G)
    with np.errstate(all="ignore"):
        for i in range(k):
            d = G[i, i] - np.dot(R[:i, i], R[:i, i])
            if not (np.isfinite(d) and d > 0.0):
                return None
            R[i, i] = np.sqrt(d)
            for j in range(i + 1, k):
                R[i, j] = (G[i, j] - np.dot(R[:i, i], R[:i, j])) / R[i, i]
    return R


def inv_upper(R):
    """inv(R) of an upper triangular R, column by column by back-substitution."""
    k = R.shape[0]
    X = np.zeros_like(R)
    for j in range(k):
        X[j, j] = 1.0 / R[j, j]
        for i in range(j - 1, -1, -1):
            X[i, j] = -np.dot(R[i, i + 1:j + 1], X[i + 1:j + 1, j]) / R[i, i]
    return X


def cholqr2(P):
    """(Q, R, why) with Q, R None on a decline; `why` names the verdict."""
    P = np.asarray(P, dtype=np.float64)
    m, k = P.shape
    if not (1 <= k <= MAX_COLS and m >= k):
        return None, None, "shape"
    with np.errstate(all="ignore"):
        R1 = chol_upper(P.T @ P)
        if R1 is None:
            return None, None, "verdict A, pass 1"
        Q1 = P @ inv_upper(R1)
        G2 = Q1.T @ Q1
        dev2 = np.sum((G2 - np.eye(k)) ** 2)
        if not dev2 <= 0.25:
            return None, None, "verdict B"
        R2 = chol_upper(G2)
        if R2 is None:
            return None, None, "verdict A, pass 2"
        Q = Q1 @ inv_upper(R2)
        R = np.triu(R2 @ R1)
    return Q, R, "ok"


def make_case(m, k, cond, rng, scale=1.0):
    """m x k matrix with singular values logspace(0, -log10(cond), k) times `scale` and random singular vectors."""
    U, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    s = np.logspace(0.0, -np.log10(cond), k) if k > 1 else np.ones(1)
    return ((U * s) @ V.T) * scale


def numpy_qr_positive(P):
    """numpy's Householder QR with the signs moved so that diag(R) > 0 (the factorisation CholeskyQR2 converges to)."""
    Q, R = np.linalg.qr(P)
    sg = np.where(np.diag(R) < 0.0, -1.0, 1.0)
    return Q * sg, (R.T * sg).T


def orth_error(Q):
    return float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max())


def residual(Q, R, P):
    return float(np.linalg.norm(Q @ R - P) / np.linalg.norm(P))


ACCEPT_SHAPES = [(1, 1), (64, 1), (65, 3), (257, 8), (1000, 17), (4097, 33), (64, 64), (20000, 64)]
ACCEPT_CONDS = [1.0, 1e3, 1e6]
ACCEPT_SCALE = 3.7


def decline_cases(rng):
    """name -> matrix for the value-driven declines (the argument-driven ones are built where the entry point is called)."""
    out = {}
    out["cond1e10_65x3"] = make_case(65, 3, 1e10, rng)
    out["cond1e10_1000x17"] = make_case(1000, 17, 1e10, rng)
    P = rng.standard_normal((257, 8))
    P[:, 7] = P[:, 0]
    out["duplicated_column"] = P
    P = rng.standard_normal((257, 8))
    P[:, 4] = 0.0
    out["zero_column"] = P
    out["all_zero"] = np.zeros((257, 8))
    out["scale_1e155"] = rng.standard_normal((257, 8)) * 1e155
    out["scale_1e-170"] = rng.standard_normal((257, 8)) * 1e-170
    P = rng.standard_normal((257, 8))
    P[100, 3] = np.nan
    out["nan_entry"] = P
    P = rng.standard_normal((257, 8))
    P[100, 3] = np.inf
    out["inf_entry"] = P
    return out
