"""Exact dyadic LU systems: matrices whose partial-pivoting factors, and whose solutions, are ONE bit pattern in fp64 whatever
the order in which a correct kernel groups its additions (host only, numpy).

The construction
    k = min(rows, cols)
    L  rows x k, unit lower, entries below the diagonal from {0, +1/2, -1/2}, about half of them nonzero
    d  k pivots from {2, 4, -2, -4}
    N  k x cols, unit upper, the same entry set above the diagonal;  U = diag(d) N  (entries in {0, +-1, +-2}, diagonal +-2, +-4)
    perm  permutes rows inside aligned groups of 64 only;  A[perm[i], :] = (L U)[i, :]

Why partial pivoting must give back L, U and perm
    At step j the candidates are L[i, j] d[j]: the true pivot has magnitude |d_j|, every other at most |d_j| / 2.  The maximum is unique by
    a factor of two, so the grid-wide first-maximum rule and a rule that compares a truncated key pick the same row.  The pivot row sits
    in the same group of 64 as column j, so a search restricted to the 256 rows from a panel's first column finds it, and every
    multiplier is at most 1/2.

Why every step is exact
    Every quantity an elimination forms is a partial sum of products l u with l in (1/2) Z and u in Z: a multiple of 1/2 bounded by the
    matching entry of |L| |U| (a trailing entry is A_ij minus a SUBSET of its own terms, i.e. the sum of the others).  Pivots are powers
    of two, so a / d, a * (1 / d) and a Newton-refined reciprocal are exact.  With an integer X and B = A X the substitutions form partial
    sums of l u x: multiples of 1/2 bounded by |L| |U| |X|.  A kernel that multiplies with the explicit inverse of an aligned 16 x 16
    diagonal block meets entries of inv(L_bb) = sum_{m<16} (I - L_bb)^m, multiples of 2^-15, and of inv(U_bb) = inv(N_bb) inv(D_b),
    multiples of 2^-17; its operand is exactly L_bb (or U_bb) times the block of the result.  `bit_budget` turns this into a number of
    bits; the cases of the tests keep it at or below 50 of fp64's 53.

The sign of an exact zero is the one thing the construction does not fix.  IEEE 754 gives 0 / d and 0 * (1 / d) the sign of d (-0.0 under
a negative pivot), while the same zero formed as a sum of products with an inverted block, or by cancellation, is +0.0: both are
correct roundings of the same exact value, and which one a factorisation stores depends on how it groups the work
(tests/test_lu_exact_host.py shows the two on the host).  So `mismatches` compares bit patterns (uint64 views: a one-ulp error, a NaN
payload or a denormal all count) and lets a zero whose value the arithmetic computed carry either sign; the zeros a kernel writes as
constants (above L's diagonal, below U's, in P) must be +0.0.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

GROUP = 64   # rows are permuted inside aligned groups of this size
BLOCK = 16   # order of the diagonal blocks a kernel may invert
BIT_CAP = 50


@dataclass(frozen=True)
class Case:
    A: np.ndarray
    L: np.ndarray      # rows x k
    U: np.ndarray      # k x cols
    perm: np.ndarray   # perm[i] = row of A that ends at position i (0-based)

    @property
    def rows(self):
        return self.A.shape[0]

    @property
    def cols(self):
        return self.A.shape[1]

    @property
    def k(self):
        return min(self.A.shape)


def group_perm(rows: int, kind: str, rng) -> np.ndarray:
    """A permutation of 0..rows-1 that moves rows only inside aligned groups of 64 (the last group may be short)."""
    perm = np.arange(rows)
    for g0 in range(0, rows, GROUP):
        g1 = min(rows, g0 + GROUP)
        if kind == "random":
            perm[g0:g1] = g0 + rng.permutation(g1 - g0)
        elif kind == "reverse":
            perm[g0:g1] = perm[g0:g1][::-1]
        elif kind != "identity":
            raise ValueError(kind)
    return perm


def case(rows: int, cols: int, seed: int, perm_kind: str = "random", density: float = 0.5) -> Case:
    rng = np.random.default_rng([seed, rows, cols])
    k = min(rows, cols)
    half = density / 2

    def entries(shape):
        return rng.choice(np.array([0.0, 0.5, -0.5]), size=shape, p=[1.0 - density, half, half])

    L = np.tril(entries((rows, k)), -1) + np.eye(rows, k)
    d = rng.choice(np.array([2.0, 4.0, -2.0, -4.0]), size=k)
    N = np.triu(entries((k, cols)), 1) + np.eye(k, cols)
    U = d[:, None] * N + 0.0   # (+ 0.0: a -0.0 from d * 0 becomes +0.0)
    perm = group_perm(rows, perm_kind, rng)
    A = np.empty((rows, cols))
    A[perm] = (L @ U) + 0.0    # exact: see the module docstring
    return Case(A, L, U, perm)


def rhs(c: Case, nrhs: int, seed: int, xmax: int = 3):
    """Integer X (cols x nrhs, entries in [-xmax, xmax]) and B = A X (exact)."""
    rng = np.random.default_rng([seed, c.rows, c.cols, nrhs])
    X = rng.integers(-xmax, xmax + 1, size=(c.cols, nrhs)).astype(np.float64)
    return X, (c.A @ X) + 0.0


# ---- bitwise comparison ---------------------------------------------------------------------------------------------------------------
def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def mismatches(got, want, computed=None) -> int:
    """Entries of `got` whose bit pattern is not `want`'s.  Where `computed` is true (default: everywhere) and `want` is zero, a zero of
    either sign matches - see the module docstring; everywhere else the sign bit of a zero counts like any other bit."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return max(got.size, want.size, 1)
    g, w = _bits(got), _bits(want)
    free = want == 0.0
    if computed is not None:
        free &= np.asarray(computed, dtype=bool)
    sign = np.uint64(1) << np.uint64(63)
    bad = np.where(free, (g | sign) != (w | sign), g != w)
    return int(np.count_nonzero(bad))


def lu_outputs_expected(c: Case, perm_got: np.ndarray):
    """`combined`, `lower` (rows x rows), `upper` (rows x cols), `perm_matrix`, `perm_vector` (1-based, rows x 1) as the provider's `lu`
    returns them, for the final row order `perm_got`.  Rows that never become pivots (rows > cols) end wherever the interchanges leave
    them, so L's rows follow the order that was actually produced: L_got == L_orig[perm_got] with L_orig[perm[i]] = L[i]."""
    rows, cols, k = c.rows, c.cols, c.k
    L_orig = np.empty_like(c.L)
    L_orig[c.perm] = c.L
    Lp = L_orig[perm_got]                       # rows x k
    lower = np.eye(rows)
    lower[:, :k] = Lp
    upper = np.zeros((rows, cols))
    upper[:k] = c.U
    combined = upper.copy()
    strict = np.tril(np.ones((rows, k), dtype=bool), -1)
    combined[:, :k][strict] = Lp[strict]
    pm = np.zeros((rows, rows))
    pm[np.arange(rows), perm_got] = 1.0
    pv = (perm_got + 1.0).reshape(rows, 1)
    return combined, lower, upper, pm, pv


def compare_lu(c: Case, combined, lower, upper, perm_matrix, perm_vector) -> dict:
    """Mismatch counts of the five outputs of `lu` against the construction (all zero for a correct factorisation)."""
    rows, cols, k = c.rows, c.cols, c.k
    out = {}
    pv = np.asarray(perm_vector, dtype=np.float64).reshape(-1)
    perm_got = pv.astype(np.int64) - 1
    ok_perm = pv.shape == (rows,) and np.array_equal(np.sort(perm_got), np.arange(rows)) and np.array_equal(perm_got + 1.0, pv)
    out["perm_valid"] = 0 if ok_perm else 1
    if not ok_perm:
        return out
    out["perm_pivots"] = int(np.count_nonzero(perm_got[:k] != c.perm[:k]))
    e_comb, e_low, e_up, e_pm, e_pv = lu_outputs_expected(c, perm_got)
    i, j = np.indices((rows, cols))
    out["upper"] = mismatches(upper, e_up, computed=i <= j)
    i2, j2 = np.indices((rows, rows))
    out["lower"] = mismatches(lower, e_low, computed=(i2 > j2) & (j2 < k))
    out["combined"] = mismatches(combined, e_comb)
    out["perm_matrix"] = mismatches(perm_matrix, e_pm, computed=np.zeros((rows, rows), dtype=bool))
    out["perm_vector"] = mismatches(np.asarray(perm_vector).reshape(rows, 1), e_pv)
    return out


def failed(report: dict) -> dict:
    return {k: v for k, v in report.items() if v}


# ---- the bits a partial sum can need ------------------------------------------------------------------------------------------------------
def _bits_for(bound: float, granularity_log2: int) -> int:
    """Bits of an integer multiple of 2^granularity_log2 with magnitude <= bound."""
    if bound <= 0:
        return 0
    return int(np.floor(np.log2(bound))) + 1 - granularity_log2


def _diag_blocks(T: np.ndarray):
    k = min(T.shape)
    for b0 in range(0, k, BLOCK):
        b1 = min(k, b0 + BLOCK)
        yield b0, b1, T[b0:b1, b0:b1]


def tri_inv(T: np.ndarray) -> np.ndarray:
    """Inverse of a small triangular matrix with a power-of-two diagonal by substitution (exact on this module's data)."""
    if T.shape[0] > 1 and np.any(np.triu(T, 1)):
        return tri_inv(T.T).T
    n = T.shape[0]
    X = np.eye(n)
    for i in range(n):
        X[i] = (X[i] - T[i, :i] @ X[:i]) / T[i, i]
    return X


def bit_budget(c: Case, X: np.ndarray | None = None) -> dict:
    """Upper bounds on the bits any partial sum can need, by the form of the arithmetic.
      form1  plain elimination (and, with X, substitution): multiples of 2^-1 bounded by |L| |U| (|L| |U| |X|)
      form2  the factorisation through explicit inverses of aligned 16 x 16 diagonal blocks:
               rows below   X_b = A_b inv(U_bb),  A_b = L_{.,b} U_bb exactly:  sums of <= 16 products (2^-17 Z)(2^-1 Z)
               block row    X_b = inv(L_bb) A_b,  A_b = L_bb U_{b,.} exactly:   sums of <= 16 products (2^-15 Z)(2^-1 Z)
             and the inverses themselves (substitution on a block: multiples of 2^-15 / 2^-17 bounded by |inv|'s row sums)
      form3  the solves through the same inverses: forward t = L_bb Y_b with Y = U X (2^-15 Z)(2^-1 Z), backward t = U_bb X_b
             (2^-17 Z)(Z); the t are themselves form-1 partial sums."""
    aL, aU = np.abs(c.L), np.abs(c.U)
    S = float((aL @ aU).max())
    out = {"form1": _bits_for(S, -1)}
    Y = aX = None
    if X is not None:
        aX = np.abs(X)
        Y = aU @ aX
        out["form1"] = max(out["form1"], _bits_for(float((aL @ Y).max()), -1))
    f2 = f3 = 0
    Lsq = c.L[: c.k]
    for b0, b1, Lbb in _diag_blocks(Lsq):
        inv = np.abs(tri_inv(Lbb))
        op = float((np.abs(Lbb) @ aU[b0:b1]).max())
        f2 = max(f2, _bits_for(float(inv.sum(axis=1).max()) * op, -16), _bits_for(float(inv.sum(axis=1).max()), -15))
        if Y is not None:
            f3 = max(f3, _bits_for(float(inv.sum(axis=1).max()) * float((np.abs(Lbb) @ Y[b0:b1]).max()), -16))
    for b0, b1, Ubb in _diag_blocks(c.U[:, : c.k]):
        inv = np.abs(tri_inv(Ubb))
        op = float((aL[:, b0:b1] @ np.abs(Ubb)).max())
        f2 = max(f2, _bits_for(float(inv.sum(axis=0).max()) * op, -18), _bits_for(float(inv.sum(axis=0).max()), -17))
        if aX is not None:
            f3 = max(f3, _bits_for(float(inv.sum(axis=1).max()) * float((np.abs(Ubb) @ aX[b0:b1]).max()), -17))
    out["form2"] = f2
    if X is not None:
        out["form3"] = f3
    return out


def bit_budget_worst_case(n: int, nrhs: int, xmax: int, lmax: float = 0.5, umax: float = 2.0, dmax: float = 4.0) -> dict:
    """The same three bounds from the construction's parameters alone (every entry at its largest magnitude), for operands that are
    built on the device and never seen by the host.  |inv(L_bb)| <= inv(I - |L_bb - I|), whose largest row sum for a 16 x 16 block
    with lmax below the diagonal is (1 + lmax)^15; |inv(U_bb)| <= that over the smallest pivot (dmax / 2)."""
    rowL = lmax * (n - 1) + 1.0              # largest row sum of |L|
    rowU = umax * (n - 1) + dmax             # largest row sum of |U|
    S = lmax * umax * (n - 1) + dmax         # largest entry of |L| |U|
    Y = rowU * xmax * nrhs                   # largest entry of |U| |X| summed over the right-hand sides
    inv_row = (1.0 + lmax) ** (BLOCK - 1)
    blkL = lmax * (BLOCK - 1) + 1.0
    blkU = umax * (BLOCK - 1) + dmax
    form1 = max(_bits_for(S, -1), _bits_for(rowL * Y, -1))
    form2 = max(_bits_for(inv_row * blkL * dmax, -16), _bits_for(inv_row / (dmax / 2) * lmax * blkU, -18), _bits_for(inv_row, -17))
    form3 = max(_bits_for(inv_row * blkL * Y, -16), _bits_for(inv_row / (dmax / 2) * blkU * xmax * nrhs, -17))
    return {"form1": form1, "form2": form2, "form3": form3}


# ---- host models used by the host test (never by the product) ---------------------------------------------------------------------------
def numpy_lu(A: np.ndarray, nb: int = 1):
    """Right-looking partial-pivoting LU (first maximum), panels of `nb` columns (nb = 1: the textbook rank-1 form).
    Returns combined factors, perm, and the largest runner-up / pivot ratio met."""
    A = np.array(A, dtype=np.float64)
    rows, cols = A.shape
    k = min(rows, cols)
    perm = np.arange(rows)
    worst = 0.0
    for j0 in range(0, k, nb):
        j1 = min(k, j0 + nb)
        for j in range(j0, j1):
            col = np.abs(A[j:, j])
            p = int(np.argmax(col))
            piv = col[p]
            if col.size > 1:
                worst = max(worst, float(np.partition(col, -2)[-2] / piv))
            if p:
                A[[j, j + p]] = A[[j + p, j]]
                perm[[j, j + p]] = perm[[j + p, j]]
            A[j + 1:, j] /= A[j, j]
            if j + 1 < j1:
                A[j + 1:, j + 1:j1] -= np.outer(A[j + 1:, j], A[j, j + 1:j1])
        if j1 < cols:
            for i in range(j0 + 1, j1):  # U12 = inv(L11) A12 by rows
                A[i, j1:] -= A[i, j0:i] @ A[j0:i, j1:]
            if j1 < rows:
                A[j1:, j1:] -= A[j1:, j0:j1] @ A[j0:j1, j1:]
    return A, perm, worst


def substitute(L: np.ndarray, U: np.ndarray, PB: np.ndarray):
    """Forward and back substitution by rows: (Y, X)."""
    n = L.shape[0]
    Y = np.array(PB, dtype=np.float64)
    for i in range(1, n):
        Y[i] -= L[i, :i] @ Y[:i]
    X = Y.copy()
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            X[i] -= U[i, i + 1:] @ X[i + 1:]
        X[i] /= U[i, i]
    return Y, X


def forward_inverse_model(L: np.ndarray, PB: np.ndarray, reverse: bool):
    """Forward solve with explicitly inverted 16 x 16 diagonal blocks, the off-diagonal contributions summed first to last or last to
    first: the association of a blocked kernel, in two orders."""
    n = L.shape[0]
    Y = np.zeros_like(PB, dtype=np.float64)
    starts = list(range(0, n, BLOCK))
    for b0 in starts:
        b1 = min(n, b0 + BLOCK)
        t = np.array(PB[b0:b1], dtype=np.float64)
        prev = [s for s in starts if s < b0]
        for c0 in (prev[::-1] if reverse else prev):
            t = t - L[b0:b1, c0:c0 + BLOCK] @ Y[c0:c0 + BLOCK]
        Y[b0:b1] = tri_inv(L[b0:b1, b0:b1]) @ t
    return Y
