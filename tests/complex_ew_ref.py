"""Reference for the complex elementwise entry points (rmhip_complex_unary / _binary / _scalar): the CPU builtins' rules restated on
separate real and imaginary f64 arrays with numpy REAL arithmetic only, so every step rounds once - never numpy's complex multiply or
divide, which are free to use other formulas.  The rules and their sources are the table in include/rmhip.h.

`binary`, `scalar`, `unary` give the f64 results (bit-exact targets for add / sub / mul / div, the scalar forms, real, imag, conj, sign);
`unary_wide` evaluates the transcendental formulas in np.longdouble for the ops that are compared by tolerance."""
import math
from fractions import Fraction

import numpy as np

PI = math.pi
BINARY = ("add", "sub", "mul", "div")
SCALAR = ("add", "sub", "mul", "div", "rsub", "rdiv")
UNARY_REAL = ("abs", "angle", "real", "imag")
UNARY_COMPLEX = ("conj", "sign", "sin", "cos", "tan", "sinh", "cosh", "sinc")
BIT_EXACT_UNARY = ("real", "imag", "conj", "sign")
TOLERANCE_UNARY = ("abs", "angle", "sin", "cos", "tan", "sinh", "cosh", "sinc")


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once: math.fma where Python has it, otherwise exact rational arithmetic rounded by float()."""
    if hasattr(math, "fma"):
        try:
            return math.fma(a, b, c)
        except (OverflowError, ValueError):  # (math.fma raises where C returns inf / NaN)
            pass
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.copysign(math.inf, a * b + c)


def _f(x):
    return np.asarray(x, dtype=np.float64)


def div(ar, ai, br, bi):
    """num-complex Div: every term kept."""
    with np.errstate(all="ignore"):
        d = br * br + bi * bi
        return (ar * br + ai * bi) / d, (ai * br - ar * bi) / d


def binary(op, kind, ar, ai, br, bi):
    """kind "cc": (ar, ai) o (br, bi); "cr": (ar, ai) o br with `bi` ignored; "rc": ar o (br, bi) with `ai` ignored.  Arrays of one shape."""
    ar, br = _f(ar), _f(br)
    ai = np.zeros_like(ar) if kind == "rc" else _f(ai)
    bi = np.zeros_like(br) if kind == "cr" else _f(bi)
    with np.errstate(all="ignore"):
        if op == "div":
            return div(ar, ai, br, bi)
        if kind == "cc":
            if op == "add":
                return ar + br, ai + bi
            if op == "sub":
                return ar - br, ai - bi
            if op == "mul":
                return ar * br - ai * bi, ar * bi + ai * br
        elif kind == "cr":
            if op == "add":
                return ar + br, ai.copy()
            if op == "sub":
                return ar - br, ai.copy()
            if op == "mul":
                return ar * br, ai * br
        else:
            if op == "add":
                return ar + br, bi.copy()
            if op == "sub":
                return ar - br, -bi  # a negation: +0 -> -0
            if op == "mul":
                return ar * br, ar * bi
    raise ValueError((op, kind))


def scalar(op, zr, zi, s):
    """z op s; rsub / rdiv are s - z and s ./ z."""
    zr, zi = _f(zr), _f(zi)
    sv = np.full_like(zr, s)
    if op in ("rsub", "rdiv"):
        return binary(op[1:], "rc", sv, None, zr, zi)
    return binary(op, "cr", zr, zi, sv, None)


def _sign(re, im):
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(re), np.abs(im))
        nr, ni = re / scale, im / scale
        mag = np.sqrt(nr * nr + ni * ni)
        out_r, out_i = nr / mag, ni / mag
        zero = (scale == 0.0) | (mag == 0.0)
        out_r, out_i = np.where(zero, 0.0, out_r), np.where(zero, 0.0, out_i)
        re_inf, im_inf = np.isinf(re), np.isinf(im)
        real = np.where(re_inf, np.copysign(1.0, re), 0.0)
        imag = np.where(im_inf, np.copysign(1.0, im), 0.0)
        norm = np.sqrt(real * real + imag * imag)
        any_inf = re_inf | im_inf
        out_r, out_i = np.where(any_inf, real / norm, out_r), np.where(any_inf, imag / norm, out_i)
        nan = np.isnan(re) | np.isnan(im)
        out_r, out_i = np.where(nan, np.nan, out_r), np.where(nan, np.nan, out_i)
        origin = (re == 0.0) & (im == 0.0)
        return np.where(origin, 0.0, out_r), np.where(origin, 0.0, out_i)


def _sinc_real(x):
    with np.errstate(all="ignore"):
        scaled = _f(PI * x)
        finite_int = np.isfinite(x) & (x == np.trunc(x))
        general = np.sin(scaled) / scaled
    return np.where(x == 0.0, 1.0, np.where(finite_int, 0.0, general))


def sinc_scaled(re, im):
    """The two f64 products pi * re, pi * im the complex sinc starts from (exact f64 operations on both sides)."""
    return _f(PI * _f(re)), _f(PI * _f(im))


def _sinc(re, im):
    sr, si = sinc_scaled(re, im)
    with np.errstate(all="ignore"):
        nr, ni = np.sin(sr) * np.cosh(si), np.cos(sr) * np.sinh(si)
        sisi = si * si
        d = np.array([fma(float(a), float(a), float(b)) for a, b in zip(sr.ravel(), sisi.ravel())], dtype=np.float64).reshape(sr.shape)
        out_r, out_i = (nr * sr + ni * si) / d, (ni * sr - nr * si) / d
    axis = im == 0.0
    return np.where(axis, _sinc_real(re), out_r), np.where(axis, 0.0, out_i)


def unary(op, re, im):
    """f64 result: one array for abs / angle / real / imag, a (re, im) pair otherwise.  The transcendental parts come from numpy's libm
    here; tests compare those ops by tolerance against `unary_wide`."""
    re, im = _f(re), _f(im)
    with np.errstate(all="ignore"):
        if op == "abs":
            return np.hypot(re, im)
        if op == "angle":
            return np.arctan2(im, re)
        if op == "real":
            return re.copy()
        if op == "imag":
            return im.copy()
        if op == "conj":
            return re.copy(), -im
        if op == "sign":
            return _sign(re, im)
        if op == "sin":
            return np.sin(re) * np.cosh(im), np.cos(re) * np.sinh(im)
        if op == "cos":
            return np.cos(re) * np.cosh(im), (-np.sin(re)) * np.sinh(im)
        if op == "sinh":
            return np.sinh(re) * np.cos(im), np.cosh(re) * np.sin(im)
        if op == "cosh":
            return np.cosh(re) * np.cos(im), np.sinh(re) * np.sin(im)
        if op == "tan":
            two_re, two_im = 2.0 * re, 2.0 * im
            ic = 1.0 / np.cosh(two_im)
            d = 1.0 + np.cos(two_re) * ic
            return (np.sin(two_re) * ic) / d, np.tanh(two_im) / d
        if op == "sinc":
            return _sinc(re, im)
    raise ValueError(op)


def longdouble_is_wide() -> bool:
    return np.finfo(np.longdouble).nmant >= 63


def unary_wide(op, re, im):
    """The same formulas in np.longdouble (near-exact parts for the tolerance family); sinc starts from the f64 products pi * re, pi * im
    and is the quotient rule only (im != 0)."""
    L = np.longdouble
    x, y = _f(re).astype(L), _f(im).astype(L)
    with np.errstate(all="ignore"):
        if op == "abs":
            return np.hypot(x, y)
        if op == "angle":
            return np.arctan2(y, x)
        if op == "sin":
            return np.sin(x) * np.cosh(y), np.cos(x) * np.sinh(y)
        if op == "cos":
            return np.cos(x) * np.cosh(y), -np.sin(x) * np.sinh(y)
        if op == "sinh":
            return np.sinh(x) * np.cos(y), np.cosh(x) * np.sin(y)
        if op == "cosh":
            return np.cosh(x) * np.cos(y), np.sinh(x) * np.sin(y)
        if op == "tan":
            ic = 1 / np.cosh(2 * y)
            d = 1 + np.cos(2 * x) * ic
            return np.sin(2 * x) * ic / d, np.tanh(2 * y) / d
        if op == "sinc":
            sr, si = (v.astype(L) for v in sinc_scaled(re, im))
            nr, ni = np.sin(sr) * np.cosh(si), np.cos(sr) * np.sinh(si)
            d = sr * sr + si * si
            return (nr * sr + ni * si) / d, (ni * sr - nr * si) / d
    raise ValueError(op)


def tan_denominator(re, im):
    """d of the tan rule: 1 + cos(2 re) / cosh(2 im).  The tolerance tests keep |d| >= 0.25."""
    return 1.0 + np.cos(2.0 * _f(re)) / np.cosh(2.0 * _f(im))


def tolerance_inputs(op, n=4096, seed=31):
    """(re, im) of the tolerance family: real parts from the range tests/test_gpu_parity.py uses for the real function (+-20 for sinh /
    cosh, +-10 otherwise), imaginary parts in [-5, 5].  sinh / cosh of a complex argument take the REAL part hyperbolically, so for them
    the +-20 range is the real part's; sin / cos / tan / sinc keep +-10.  tan: two groups built so that |d| >= 0.25 everywhere - away from
    the real axis (|im| in [0.5, 5]: |cos(2 re) / cosh(2 im)| <= 1 / cosh(1) = 0.648) and, near it (|im| < 0.5), real parts in
    [-0.5, 0.5] where cos(2 re) >= cos(1) > 0.  sinc: |im| >= 2^-20 so that every element takes the quotient rule."""
    rng = np.random.default_rng(seed)
    span = 20.0 if op in ("sinh", "cosh") else 10.0
    re = rng.uniform(-span, span, n)
    im = rng.uniform(-5.0, 5.0, n)
    if op == "tan":
        half = n // 2
        im[:half] = np.copysign(rng.uniform(0.5, 5.0, half), im[:half])
        re[half:] = rng.uniform(-0.5, 0.5, n - half)
        im[half:] = rng.uniform(-0.5, 0.5, n - half)
    if op == "sinc":
        im = np.where(np.abs(im) < 2.0 ** -20, 2.0 ** -20, im)
    return re, im


def same_bits(a, b) -> bool:
    """Equal values with equal signs of zero; NaN matches NaN whatever its payload."""
    a, b = _f(a).ravel(), _f(b).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def interleave(re, im):
    out = np.empty(2 * np.asarray(re).size, dtype=np.float64)
    out[0::2], out[1::2] = _f(re).ravel(), _f(im).ravel()
    return out
