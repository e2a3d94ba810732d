"""numpy restatement of the reference's CPU `qr` builtin for real input (builtins/math/linalg/factor/qr.rs:576-870).

    qr_host(A, economy=False) -> QrHost(q, r, perm_matrix, perm_vector, gaps)

* pivoting is always on: before step k the squared norms of rows k..m-1 of columns k..n-1 are recomputed from the current matrix and the
  pivot is their arg-max, ties to the LAST index (`Iterator::max_by`); whole columns, norms and permutation entries are swapped;
* `householder` with its quirks: a column with tail^2 <= 1e-12 and |alpha| <= 1e-12 is zeroed (tau 0); a tail^2 <= 1e-12 with alpha >= 0 is
  dropped (tau 0, R(k,k) = alpha); otherwise beta = -sign(alpha) sqrt(alpha^2 + t) (sign +1 when |alpha| <= 1e-12), the tail divided by
  alpha - beta (zeroed when |alpha - beta| <= 1e-12), tau = (beta - alpha) / beta (0 when |beta| <= 1e-12).  num-complex divides real values
  as x d / d^2: so does this file;
* `apply_householder`: dot = sum v_i a_ij, dot *= tau, a_ij -= v_i dot, skipped when tau == 0;
* Q = H_0 ... H_{p-1} I (`build_q`), R the upper trapezoid, both cleaned at |x| <= 1e-12; economy with m >= n keeps Q(:, :n), R(:n, :);
  perm_matrix E(perm[c], c) = 1, perm_vector n x 1, 1-based.

`gaps[k]` is the relative gap (best - second) / best between the two leading candidate norms at step k (inf with one candidate, 0 when the
best norm is 0): where it is small, a different summation order may pick a different, equally valid pivot.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np

EPS_CLEAN = 1.0e-12


@dataclass
class QrHost:
    q: np.ndarray
    r: np.ndarray
    perm_matrix: np.ndarray
    perm_vector: np.ndarray
    gaps: List[float] = field(default_factory=list)
    taus: List[float] = field(default_factory=list)

    @property
    def perm(self) -> np.ndarray:
        return (self.perm_vector[:, 0] - 1).astype(np.int64)


def _div(x, d):
    """num-complex division of real values: x * d / d^2"""
    return (x * d) / (d * d)


def householder(col: np.ndarray) -> float:
    """In place on col = A(k:m, k); returns tau (qr.rs:742-792)."""
    if col.size == 0:
        return 0.0
    alpha = float(col[0])
    t = float(np.sum(col[1:] * col[1:])) if col.size > 1 else 0.0
    aa = abs(alpha)
    if t <= EPS_CLEAN and aa <= EPS_CLEAN:
        col[:] = 0.0
        return 0.0
    if t <= EPS_CLEAN and alpha >= 0.0:
        col[1:] = 0.0
        return 0.0
    total = np.sqrt(aa * aa + t)
    sign = 1.0 if aa <= EPS_CLEAN else _div(alpha, aa)
    beta = -sign * total
    tau = 0.0 if abs(beta) <= EPS_CLEAN else _div(beta - alpha, beta)
    d = alpha - beta
    if abs(d) <= EPS_CLEAN:
        col[1:] = 0.0
    else:
        col[1:] = _div(col[1:], d)
    col[0] = beta
    return float(tau)


def _clean(x: np.ndarray) -> np.ndarray:
    x = x.copy()
    x[np.abs(x) <= EPS_CLEAN] = 0.0
    return x


def qr_host(A, economy: bool = False) -> QrHost:
    A = np.array(A, dtype=np.float64, copy=True)
    if A.ndim > 2:
        raise ValueError("qr: input must be 2-D")
    if A.ndim < 2:
        A = A.reshape(-1, 1) if A.ndim == 1 else A.reshape(1, 1)
    m, n = A.shape
    p = min(m, n)
    W = np.asfortranarray(A)
    perm = np.arange(n)
    taus, gaps = [], []
    norms = np.sum(W * W, axis=0)
    for k in range(p):
        cand = norms[k:]
        best = float(np.max(cand))
        piv = k + int(np.flatnonzero(cand == best)[-1])  # ties: the last index
        if cand.size > 1:
            second = float(np.max(np.delete(cand, piv - k)))
            gaps.append(0.0 if best == 0.0 else (best - second) / best)
        else:
            gaps.append(float("inf"))
        if piv != k:
            W[:, [k, piv]] = W[:, [piv, k]]
            norms[[k, piv]] = norms[[piv, k]]
            perm[[k, piv]] = perm[[piv, k]]
        tau = householder(W[k:, k])
        taus.append(tau)
        if tau != 0.0:
            v = np.concatenate(([1.0], W[k + 1:, k]))
            dot = (v @ W[k:, k + 1:]) * tau
            W[k:, k + 1:] -= np.outer(v, dot)
        norms[k + 1:] = np.sum(W[k + 1:, k + 1:] * W[k + 1:, k + 1:], axis=0)
    Q = np.eye(m)
    for k in range(p - 1, -1, -1):
        tau = taus[k]
        if tau == 0.0:
            continue
        v = np.concatenate(([1.0], W[k + 1:, k]))
        dot = (v @ Q[k:, :]) * tau
        Q[k:, :] -= np.outer(v, dot)
    R = np.triu(W)
    R[np.abs(R) <= EPS_CLEAN] = 0.0
    Q, R = _clean(Q), _clean(R)
    if economy and m >= n:
        Q, R = Q[:, :n].copy(), R[:n, :].copy()
    E = np.zeros((n, n))
    E[perm, np.arange(n)] = 1.0
    pv = (perm + 1).astype(np.float64).reshape(n, 1)
    return QrHost(Q, R, E, pv, gaps, taus)


def power_iteration(G: np.ndarray, Q0: np.ndarray, iters: int) -> np.ndarray:
    """Subspace iteration Q = qr(G * Q, 0) with the restatement."""
    Q = Q0
    for _ in range(iters):
        Q = qr_host(G @ Q, economy=True).q
    return Q
