"""NumPy restatement of `cov_from_tensors(left, right, CovRows::All, weight)`: `combine_tensors` + `covariance_dense` (cov.rs:362-385, 901-1003),
`covariance_unweighted_pair` / `covariance_weighted_pair` (:1080-1126) and `sanitize_covariance` (:1218-1236).

Sums are sequential (`np.cumsum(...)[-1]` adds in index order, as the CPU's loops do); the weighted pair skips rows of weight 0 and multiplies
`(w * (x - mx)) * (y - my)` in the CPU's order; a column with a non-finite value has a NaN mean and poisons its pairs; the upper triangle
(i <= j) is computed and mirrored.  The model of the device's general covariance entry point (`oracle.covariance` covers only the plain form)."""
import numpy as np


def _seq_sum(a, axis=0):
    """Sequential sum along `axis` starting from +0.0, as `let mut sum = 0.0; sum += v` does (np.sum is pairwise)."""
    a = np.asarray(a, dtype=np.float64)
    zero = np.zeros(a.shape[:axis] + (1,) + a.shape[axis + 1:])
    return np.take(np.cumsum(np.concatenate([zero, a], axis=axis), axis=axis), -1, axis=axis)


def combine(left, right=None):
    """combine_tensors: [left | right] column-wise; vectors are columns."""
    m = np.asarray(left, dtype=np.float64)
    m = m.reshape(-1, 1) if m.ndim < 2 else m
    if right is not None:
        r = np.asarray(right, dtype=np.float64)
        r = r.reshape(-1, 1) if r.ndim < 2 else r
        if r.shape[0] != m.shape[0]:
            raise ValueError(f"cov: inputs must have the same number of rows (got {m.shape[0]} and {r.shape[0]})")
        m = np.concatenate([m, r], axis=1)
    return m


def sanitize(diagonal, value):
    """sanitize_covariance: a finite diagonal entry in (-1e-12, 0) is rounding noise."""
    if diagonal and np.isfinite(value) and -1.0e-12 < value < 0.0:
        return 0.0
    return value


def cov_general(left, right=None, weights=None, biased=False):
    m = combine(left, right)
    rows, cols = m.shape
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != rows:
            raise ValueError(f"cov: weight vector length mismatch (expected {rows} elements)")
    if cols == 0:
        return np.zeros((0, 0))
    out = np.full((cols, cols), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        if w is None:
            denom = float(rows) if biased else float(rows) - 1.0
            if denom <= 0.0:
                return out
            divisor, wk, mk = float(rows), None, m
        else:
            sum_w = float(_seq_sum(w))  # `biased` plays no part in the weighted form
            if sum_w <= 0.0:
                return out
            denom = sum_w - 1.0
            if denom <= 0.0:
                return out
            divisor = sum_w
            keep = w != 0.0  # covariance_weighted_pair: `if weight == 0.0 { continue; }`
            wk, mk = w[keep], m[keep]
        finite_col = np.all(np.isfinite(m), axis=0)
        sums = _seq_sum(m if w is None else w[:, None] * m)
        means = np.where(finite_col, sums / divisor, np.nan)
        for i in range(cols):
            di = mk[:, i] - means[i]
            lhs = di if wk is None else wk * di
            acc = _seq_sum(lhs[:, None] * (mk[:, i:] - means[i:]))
            for j in range(i, cols):
                if not np.isfinite(means[i]) or not np.isfinite(means[j]):
                    value = np.nan
                elif not np.all(np.isfinite(mk[:, i])) or not np.all(np.isfinite(mk[:, j])):
                    value = np.nan
                else:
                    value = acc[j - i] / denom
                value = sanitize(i == j, value)
                out[i, j] = value
                out[j, i] = value
    return out
