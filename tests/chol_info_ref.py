"""Cases and expectations for `rmhip_chol_info` (runmat_amd/csrc/chol.hip): the failure forms of `[R, p] = chol(A)` as the reference's
Cholesky-Crout reports them (chol.rs:374-433, restated in oracle.chol).

Columns are taken left to right; column j (0-based) raises, in this order,
    A(j)  a pair (i, j), i < j, fails |a_ij - a_ji| <= 1e-12 max(|a_ij|, |a_ji|, 1): info = j + 1, column j is not formed;
    T(j)  the root of pivot j - 1 is <= 1e-12 (the denominator test): info = j; the entry point declines these;
    P(j)  the pivot is not finite or <= 0: info = j + 1, rows < j of column j have been formed and are kept.
Only the upper triangle enters the sums, so every case below is a change to a positive definite PARENT that leaves the columns before
the event alone: what the reference keeps is a piece of the parent's factor, bit for bit (`expected`).  tests/test_chol_info_host.py pins
that to oracle.chol on the CPU; the GPU tests then need one factorisation of each parent by the oracle."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

EPS = np.finfo(float).eps
P_COLUMNS = {200: (0, 17, 63, 64, 65, 127, 128, 129, 191, 192, 199),  # 200 recurses 128 + (64 + 8): leaves end at 63, 127, 191
             2049: (1023, 1024, 2048)}
A_PAIRS = ((0, 1), (3, 64), (63, 64), (5, 170), (198, 199))
SEEDS = {200: 3, 2049: 2049}  # 200: the matrix of test_chol_reference_vector_and_refusals, made exactly symmetric


@lru_cache(maxsize=None)
def parent(n):
    """b b' + n I, exactly symmetric; read-only (shared between tests)."""
    b = np.random.default_rng(SEEDS[n]).standard_normal((n, n))
    a = b @ b.T + n * np.eye(n)
    a = 0.5 * (a + a.T)
    a.setflags(write=False)
    return a


@dataclass
class Case:
    name: str
    a: np.ndarray
    kind: str  # "ok", "A" or "P"
    col: int   # the event's column (0-based); unused for "ok"


def expected(r0, kind, col):
    """(info, upper factor) the reference returns for an event of `kind` in column `col` of a matrix whose parent has the factor r0."""
    n = r0.shape[0]
    if kind == "ok":
        return 0, r0.copy()
    want = np.zeros((n, n))
    want[:col, :col] = r0[:col, :col]
    if kind == "P":
        want[:col, col] = r0[:col, col]
    return col + 1, want


def keep_mask(n, kind, col):
    """The entries the reference keeps: everything else is exact zero."""
    rows, cols = np.indices((n, n))
    if kind == "ok":
        return rows <= cols
    keep = (rows <= cols) & (cols < col)
    if kind == "P":
        keep |= (cols == col) & (rows < col)
    return keep


def lowered(a, r0, j):
    """The parent with a_jj lowered so that pivot j becomes about -1."""
    m = a.copy()
    m[j, j] -= r0[j, j] ** 2 + 1.0
    return m


def pivot_cases(n, r0):
    a = parent(n)
    return [Case(f"P{j}", lowered(a, r0, j), "P", j) for j in P_COLUMNS[n]]


def asymmetry_cases(r0):
    """n = 200.  A perturbation of 1e-6 of the upper or of the lower entry of a pair; then the orderings of A and P."""
    a = parent(200)
    out = []
    for i, j in A_PAIRS:
        for where, (r, c) in (("upper", (i, j)), ("lower", (j, i))):
            m = a.copy()
            m[r, c] += 1e-6
            out.append(Case(f"A({i},{j}){where}", m, "A", j))
    m = lowered(a, r0, 150)          # A before P: pair (9, 70) comes first
    m[9, 70] += 1e-6
    out.append(Case("A70 before P150", m, "A", 70))
    m = lowered(a, r0, 40)           # P before A
    m[9, 70] += 1e-6
    out.append(Case("P40 before A70", m, "P", 40))
    m = lowered(a, r0, 70)           # both in one column: the symmetry check comes first
    m[70, 9] += 1e-6
    out.append(Case("A70 and P70", m, "A", 70))
    return out


def nonfinite_cases():
    """n = 200.  NaN, +Inf, -Inf and 0 on the diagonal give P; a NaN pair and an Inf pair (Inf - Inf) off the diagonal give A."""
    a = parent(200)
    out = []
    for j, v in ((100, np.nan), (64, np.inf), (127, -np.inf), (3, 0.0)):
        m = a.copy()
        m[j, j] = v
        out.append(Case(f"diag{j}={v}", m, "P", j))
    for (i, j), v in (((7, 100), np.nan), ((64, 129), np.inf)):
        m = a.copy()
        m[i, j] = m[j, i] = v
        out.append(Case(f"pair({i},{j})={v}", m, "A", j))
    return out


def small_spd(k, seed):
    b = np.random.default_rng(seed).standard_normal((k, k))
    a = b @ b.T + k * np.eye(k)
    return 0.5 * (a + a.T)


def block_diag(*blocks):
    blocks = [np.atleast_2d(np.asarray(b, dtype=np.float64)) for b in blocks]
    n = sum(b.shape[0] for b in blocks)
    out = np.zeros((n, n))
    at = 0
    for b in blocks:
        out[at:at + b.shape[0], at:at + b.shape[0]] = b
        at += b.shape[0]
    return out


def tiny_cases():
    """(name, matrix, column of the pivot whose root is 1e-13, declined?): a tiny pivot before the last column is the reference's T event
    in the next column (info = that pivot's 1-based column) and is declined; a tiny LAST pivot is a success."""
    return [("mid41", block_diag(small_spd(40, 1), 1e-26, small_spd(40, 2)), 40, True),
            ("leaf-end63", block_diag(small_spd(63, 3), 1e-26, small_spd(66, 4)), 63, True),
            ("last", block_diag(small_spd(40, 1), 1e-26), 40, False)]
