"""Plain-numpy restatement of signal_envelope, written from the contract in include/rmhip.h (not from any implementation).

`envelope(x, method, param, dtype)` takes the channels as the columns of a float64 array [n, m] and works in `dtype`: numpy's float64 (the
expectation of the GPU tests) or numpy's longdouble (the truth the host test measures that expectation against).  In long double the transform
is a radix-2 recursion for powers of two and a direct DFT otherwise, with the angles reduced as integers before they are scaled; the RMS
window sums are `math.fsum` over the exactly split squares.  Besides the two envelopes it returns what the tests' bounds are made of."""
import math

import numpy as np

ANALYTIC, ANALYTIC_FIR, RMS = 0, 1, 2
NAMES = {ANALYTIC: "analytic", ANALYTIC_FIR: "analytic_fir", RMS: "rms"}


def bessel_i0(x: float) -> float:
    """sum (x^2/4)^j / (j!)^2, stopped after 32 terms or when a term is <= 1e-15 of the sum"""
    y = x * x / 4.0
    term, total = 1.0, 1.0
    for k in range(1, 33):
        term *= y / float(k * k)
        total += term
        if abs(term) <= abs(total) * 1.0e-15:
            break
    return total


def fir_taps(length: int, first: int = 0, last: int = None) -> np.ndarray:
    """k[t] = ideal(t - (L-1)/2) * kaiser(t) for t = first .. last, in f64 and in the header's operation order"""
    last = length - 1 if last is None else last
    center = (float(length) - 1.0) / 2.0
    denominator = bessel_i0(8.0)
    out = np.zeros(last - first + 1)
    for t in range(first, last + 1):
        k = float(t) - center
        if k == 0.0 or (k == math.floor(k) and int(k) % 2 == 0):
            ideal = 0.0
        else:
            ideal = 2.0 / (math.pi * k)
        if length <= 1:
            kaiser = 1.0
        else:
            r = 2.0 * float(t) / float(length - 1) - 1.0
            kaiser = bessel_i0(8.0 * math.sqrt(max(0.0, 1.0 - r * r))) / denominator
        out[t - first] = ideal * kaiser
    return out


def _pi(dtype):
    return np.pi if dtype == np.float64 else dtype(4) * np.arctan(dtype(1))


def _twiddle(num, den, sign, dtype):
    """exp(sign * 2 pi i * num / den) for integer arrays num (already reduced mod den)"""
    ang = dtype(2) * _pi(dtype) * num.astype(dtype) / dtype(den)
    return np.cos(ang) + sign * 1j * np.sin(ang)


def _fft_pow2(a, sign, dtype):
    n = a.shape[0]
    if n == 1:
        return a
    even, odd = _fft_pow2(a[0::2], sign, dtype), _fft_pow2(a[1::2], sign, dtype)
    w = _twiddle(np.arange(n // 2), n, sign, dtype)[:, None] * odd
    return np.concatenate([even + w, even - w], axis=0)


def dft(a: np.ndarray, dtype, inverse: bool = False) -> np.ndarray:
    """the DFT of every column (unscaled forward, 1/n inverse)"""
    n = a.shape[0]
    if dtype == np.float64:
        return np.fft.ifft(a, axis=0) if inverse else np.fft.fft(a, axis=0)
    sign = 1.0 if inverse else -1.0
    if n & (n - 1) == 0:
        out = _fft_pow2(a, sign, dtype)
    else:
        jk = np.outer(np.arange(n), np.arange(n)) % n
        out = _twiddle(jk, n, sign, dtype) @ a
    return out / dtype(n) if inverse else out


def hilbert_mask(n: int) -> np.ndarray:
    """1, 2 ... 2, [1], 0 ... 0"""
    h = np.zeros(n)
    h[0] = 1.0
    if n % 2 == 0:
        h[n // 2] = 1.0
        h[1:n // 2] = 2.0
    else:
        h[1:(n + 1) // 2] = 2.0
    return h


def _fsum_squares(x: np.ndarray, s: int, e: int) -> float:
    """sum of x[s:e]^2 to long-double accuracy: each square split into a float64 head and the remainder of the long-double product"""
    seg = x[s:e]
    hi = seg * seg
    lo = (seg.astype(np.longdouble) * seg.astype(np.longdouble) - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]))


def envelope(x: np.ndarray, method: int, param: int = 0, dtype=np.float64):
    """x: float64 [n, m], channels in columns.  Returns (upper, lower, aux) in `dtype`; aux holds `mu` [m], `c` [n, m] (the centred signal,
    methods 0 and 1), `mass` and `ksum` [n, m] (method 1: sum |c_j k_t| and sum |k_t| over the taps each output reaches) and `count` [n]
    (method 2: e - s)."""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    xd = x.astype(dtype)
    aux = {}
    if method == RMS:
        w = int(param)
        hb, ha = (w - 1) // 2, w // 2
        idx = np.arange(n)
        s = np.maximum(0, idx - hb)
        e = np.minimum(n, idx + ha + 1)
        count = e - s
        aux["count"] = count
        upper = np.zeros((n, m), dtype=dtype)
        if dtype == np.float64:
            sq = xd * xd
            acc = np.zeros((n, m))
            for k in range(int(count.max())):  # ascending j = s + k
                live = k < count
                acc[live] = acc[live] + sq[s[live] + k]
            upper = np.sqrt(acc / count[:, None])
        else:
            for col in range(m):
                for i in range(n):
                    upper[i, col] = np.sqrt(dtype(_fsum_squares(x[:, col], int(s[i]), int(e[i]))) / dtype(int(count[i])))
        return upper, -upper, aux
    mu = np.sum(xd, axis=0) / dtype(n)
    c = xd - mu[None, :]
    aux["mu"], aux["c"] = mu, c
    if n == 1:
        return xd.copy(), xd.copy(), aux
    if method == ANALYTIC:
        spec = dft(c.astype(np.complex128 if dtype == np.float64 else np.clongdouble), dtype)
        z = dft(spec * hilbert_mask(n).astype(dtype)[:, None], dtype, inverse=True)
        mag = np.hypot(z.real, z.imag)
    else:
        length = int(param)
        half = length // 2
        first, last = max(0, half - (n - 1)), min(length - 1, half + n - 1)
        taps = fir_taps(length, first, last).astype(dtype)
        q = np.zeros((n, m), dtype=dtype)
        mass = np.zeros((n, m), dtype=dtype)
        ksum = np.zeros(n, dtype=dtype)
        for t in range(first, last + 1):  # ascending t
            d = t - half
            i0, i1 = max(0, -d), min(n, n - d)
            if i1 <= i0:
                continue
            p = c[i0 + d:i1 + d] * taps[t - first]
            q[i0:i1] = q[i0:i1] + p
            mass[i0:i1] += np.abs(p)
            ksum[i0:i1] += abs(taps[t - first])
        aux["mass"], aux["ksum"] = mass, ksum
        mag = np.hypot(c, q)
    return mu[None, :] + mag, mu[None, :] - mag, aux
