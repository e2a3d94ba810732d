"""Stable restatement of the moving median (moving.rs:1282-1323) for the tests of `rmhip_moving_window_long`: the oracle sorts with `qsort`,
which is not stable, so windows that hold zeros of both signs are checked against this instead.  "Sorted" is numpy's stable argsort of the
window's non-NaN values: -0.0 and 0.0 compare equal and keep window order, and the element comes back with its own bits."""
import numpy as np


def _kth_fill(sorted_vals, fill, fc, k):
    less = int(np.sum(sorted_vals < fill))
    equal = int(np.sum(sorted_vals == fill))
    if k < less:
        return sorted_vals[k]
    if k < less + equal + fc:
        return fill
    return sorted_vals[k - fc]


def _line_median(line, before, after, ep, fill, omit):
    n = len(line)
    centers = range(before, n - after) if ep == 1 else range(n)
    out = np.empty(len(centers))
    for j, c in enumerate(centers):
        start, end = c - before, c + after
        w = line[min(max(start, 0), n):min(max(end + 1, 0), n)]
        fc = (max(-start, 0) + max(end - n + 1, 0)) if ep == 2 else 0
        nan = np.isnan(w)
        saw_nan = bool(nan.any()) and not omit
        if fc and (saw_nan or (np.isnan(fill) and not omit)):
            out[j] = np.nan
            continue
        if fc and np.isnan(fill):
            fc = 0
        vals = w[~nan]
        if saw_nan or (len(vals) == 0 and fc == 0):
            out[j] = np.nan
            continue
        s = vals[np.argsort(vals, kind="stable")]
        total = len(s) + fc
        mid = total // 2
        kth = (lambda k: s[k]) if fc == 0 else (lambda k: _kth_fill(s, fill, fc, k))
        with np.errstate(over="ignore"):
            out[j] = kth(mid) if total % 2 else (kth(mid - 1) + kth(mid)) / 2.0
    return out


def moving_median(x, dim, before, after, endpoints="shrink", nan_mode="include"):
    """The median of `oracle.moving_window(x, dim, before, after, "median", endpoints, nan_mode)`, with a stable sort."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(list(x.shape) + [1] * max(0, dim + 1 - x.ndim))
    ep, fill = (0, 0.0) if endpoints == "shrink" else (1, 0.0) if endpoints == "discard" else (2, np.float64(endpoints))
    return np.apply_along_axis(_line_median, dim, x, before, after, ep, fill, nan_mode == "omit")
