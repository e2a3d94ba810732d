"""What `rmhip_complex_mldivide` / `_mrdivide` / `_inv` must compute, for the host and the GPU tests.

    embed(Ar, Ai)                     E(A) = [Ar -Ai; Ai Ar] in the block layout k_csolve_embed writes (csolve.hip)
    stack(kind, Br, Bi)               the real right-hand side: [Br; Bi], [Br; 0] or, for a real A, [Br | Bi]
    join(kind, T, n, k)               the complex solution from the real one
    solve_ref(A, B, tol_dim=None)     the reference's host path (mldivide_complex, mldivide.rs:343-395) in complex128: the minimum-norm
                                      least-squares solution from an SVD with tol = eps * max(rows, cols) * max(s_max, 1); `tol_dim`
                                      replaces max(rows, cols) (the test of the tolerance asks what the embedded dimension would give)
    tolerance_case()                  the matrix of the tolerance test
    expected_plan(entry, kind, m, n, nrhs)   the fields plan_csolve (runmat_amd/csrc/csolve_plan.h) must return

The embedding.  A x = b  <=>  E(A) [xr; xi] = [br; bi].  A -> E(A) is a ring homomorphism that maps A' to E(A)', so it preserves
products, inverses, pseudo-inverses and with them least-squares and minimum-norm solutions; with A = U S V', E(A) = E(U) E(S) E(V)' is
an SVD of E(A): its singular values are A's, each twice.  Operand kinds are complex_matmul's: 0 both complex, 1 A complex and b real,
2 A real and b complex (no embedding: A \\ [Br | Bi]).
"""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float64).eps)
KINDS = (0, 1, 2)
MLDIVIDE, MRDIVIDE, INV = 0, 1, 2  # csolve_plan.h CSOLVE_*

# (n, k) of the square GPU cases: 2n = 64 is the small solver's last order, 33 the first on the blocked path, 2n = 260 is ragged against
# the 128-row padding of the blocked LU
SQUARE_SHAPES = [(2, 1), (2, 3), (3, 1), (3, 3), (16, 1), (16, 3), (32, 1), (33, 3), (130, 1), (300, 1)]
# (m, n, k): tall, then wide
RECT_SHAPES = [(5, 2, 1), (40, 7, 3), (300, 30, 2), (2, 5, 1), (30, 300, 2)]
INV_ORDERS = [2, 3, 33, 130]
MRDIVIDE_SHAPES = [(3, 2), (33, 1)]  # (n, k): B is k x n, A n x n


def embed(Ar, Ai):
    Ar, Ai = np.asarray(Ar, dtype=np.float64), np.asarray(Ai, dtype=np.float64)
    return np.asfortranarray(np.block([[Ar, -Ai], [Ai, Ar]]))


def kind_of(Ai, Bi):
    assert Ai is not None or Bi is not None
    return 0 if Ai is not None and Bi is not None else (1 if Ai is not None else 2)


def operands(rng, kind, m, n, k):
    """Gaussian parts; None for the imaginary part of the real operand."""
    Ar, Br = rng.standard_normal((m, n)), rng.standard_normal((m, k))
    Ai = rng.standard_normal((m, n)) if kind != 2 else None
    Bi = rng.standard_normal((m, k)) if kind != 1 else None
    return Ar, Ai, Br, Bi


def stack(kind, Br, Bi):
    if kind == 2:
        return np.asfortranarray(np.concatenate([Br, Bi], axis=1))
    return np.asfortranarray(np.concatenate([Br, Bi if kind == 0 else np.zeros_like(Br)], axis=0))


def join(kind, T, n, k):
    T = np.asarray(T)
    assert T.shape == ((n, 2 * k) if kind == 2 else (2 * n, k))
    return T[:, :k] + 1j * T[:, k:] if kind == 2 else T[:n, :] + 1j * T[n:, :]


def as_complex(re, im):
    return np.asarray(re, dtype=np.float64) + 1j * (np.asarray(im, dtype=np.float64) if im is not None else 0.0)


def solve_ref(A, B, tol_dim=None):
    A, B = np.asarray(A, dtype=np.complex128), np.asarray(B, dtype=np.complex128)
    m, n = A.shape
    U, s, Vh = np.linalg.svd(A, full_matrices=False)
    tol = EPS * (tol_dim if tol_dim else max(m, n)) * max(float(s.max(initial=0.0)), 1.0)
    keep = s > tol
    coef = (U[:, keep].conj().T @ B) / s[keep, None]
    return Vh[keep, :].conj().T @ coef


def tolerance_case(n=8, seed=7):
    """A = Q diag(1, ..., 1, 1.5 n eps) with Q a random unitary: its smallest singular value lies between the tolerance counted with n
    and the one counted with 2n."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    d = np.ones(n)
    d[-1] = 1.5 * n * EPS
    return Q * d[None, :]


def expected_plan(entry, kind, m, n, nrhs):
    emb = kind != 2
    aw = 4 * m * n if emb else (m * n if entry == MRDIVIDE else 0)
    return dict(M=2 * m if emb else m, N=2 * n if emb else n, NRHS=nrhs if emb else 2 * nrhs, embed_a=int(emb),
                transpose_a=int(entry == MRDIVIDE), tol_dim=max(m, n), a_workspace=aw, workspace=aw + 2 * m * nrhs, result=2 * n * nrhs)
