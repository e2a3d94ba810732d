"""Exact references, data classes and error bounds for the ahead-of-time reductions (rmhip_reduce, rmhip_reduce_nd, rmhip_dot).

Everything works slice-wise on the column-major [pre, red, post] view of a tensor: `slices(flat, pre, red, post)` is the 2-D array
[nslices, red] whose row `i + pre * j` is output slice (i, j) - the order of the kernels' outputs.  Standard library and numpy only.

References (all exact; a NaN entry is left out and counted):
  sum / mean   `exact_sums`: every f64 is mantissa * 2^exponent; the mantissas of a slice are summed as integers on a common exponent
               (vectorised in int64 halves while the exponents of a tensor span <= 16 binades, `Fraction` otherwise).  `math.fsum`
               of a slice is the rounding of this value, which the host test checks.  Results are `Q`s: arrays of exact rationals.
  prod         `exact_prods`: the product of the integer mantissas in a pairwise tree, with the exponent sum; exact up to 400 bits,
               beyond that an enclosure 2^-380 wide, which the comparison takes the unfavourable end of.
  dot          `exact_dots`: the integer mantissas cut in 21-bit limbs, the limb products summed in int64 and put together as integers.
  min / max    the oracle's `minmax_dim` (the CPU builtin's rules); not restated here.

Data classes, seeded:
  exact    every association order gives the same bits (integer-valued sums and dots with |partial sums| < 2^53; products of +-1,
           at most 300 entries +-2^k with |k| <= 3 and at most 8 small odd integers), so a result is compared for bit equality.
  rounded  full mantissas; the result is compared against a bound that holds for ANY association order, with u = 2^-53 and
           gamma_k = k u / (1 - k u)  (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2 and lemma 3.1):
             sum   |got - S|   <= gamma_(red-1) * sum|x|
             mean  |got - S/c| <= gamma_(red-1) * sum|x| / c * (1 + u) + u * |S/c|        (c counted values, one more division)
             prod  |got - P|   <= gamma_(red-1) * |P|
             dot   |got - D|   <= gamma_red * sum|a b|
           and on a precision-32 provider (f32-representable inputs, f64 accumulation, ONE final rounding to f32) the bound B above
           becomes B + 2^-24 * (|exact| + B).  The comparisons are evaluated in exact integer arithmetic (`error_ratios`), not in f64.
"""
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
U32 = Fraction(1, 2 ** 24)
ROUNDED_LIMIT = 300_000  # the rounded class is used where pre * red * post stays below this (cost of the exact references)

# (pre, red, post, kernel, nsplit, flat finalize) on 256 CUs / 8 XCDs at either storage width: the list tests/cpp/reduce_route_check.cpp
# pins against reduce_plan.h route_reduction.
ROUTE_TABLE = [
    (1, 3, 1025, "short", 1, True), (1, 255, 1030, "short", 1, True), (1, 1, 1024, "short", 1, True),
    (1, 255, 1023, "contig", 1, False), (1, 256, 1024, "contig", 1, True),
    (1, 300, 40, "contig", 1, False), (1, 2047, 3, "contig", 1, False), (1, 5, 1, "contig", 1, False),
    (1, 2048, 3, "contig_v2", 1, False), (1, 6000, 1, "contig_v2", 3, False), (1, 70000, 1, "contig_v2", 9, False),
    (1, 4096, 1030, "contig_v2", 2, True),
    (1, 2049, 3, "contig_v2_odd", 2, False), (1, 6001, 2, "contig_v2_odd", 3, False), (1, 70001, 1, "contig_v2_odd", 9, False),
    (1, 2049, 1030, "contig_v2_odd", 2, True),
    (2, 9, 1, "strided", 1, False), (6, 50, 4, "strided", 1, False),
    (7, 5000, 1, "strided", 10, False), (300, 257, 1, "strided", 17, False), (3, 70000, 1, "strided", 69, False),
    (511, 600, 1, "strided", 38, False),
    (255, 40, 70, "strided", 3, True), (16, 20, 1100, "strided", 1, True),
    (512, 40, 1, "strided_v2", 3, False), (512, 600, 1, "strided_v2", 38, False),
    (514, 33, 3, "strided_v2", 3, True), (1100, 20, 1, "strided_v2", 2, True), (600, 16, 30, "strided_v2", 1, True),
    (513, 37, 1, "strided_v2_odd", 3, False), (1001, 9, 1, "strided_v2_odd", 1, False), (513, 600, 1, "strided_v2_odd", 38, False),
    (515, 33, 3, "strided_v2_odd", 3, True), (1025, 20, 1, "strided_v2_odd", 2, True), (601, 16, 30, "strided_v2_odd", 1, True),
]
ROUNDED_ROWS = [r for r in ROUTE_TABLE if r[0] * r[1] * r[2] <= ROUNDED_LIMIT]

# The same for the two families whose launchers have kernels of their own: (pre, red, post, kernel, nsplit, flat finalize, grid.x,
# block).  ACC: the accumulator reductions of reduce2.hip (min / max with indices, std, nnz / any / all, moments); GEN: the generated
# fused reductions (rmhip_fused_reduction), which reduce axis 0 ([1, red, slices]) or axis 1 ([slices, red, 1]).
ACC_ROUTE_TABLE = [
    (1, 3, 1025, "short", 1, True, 5, 256), (1, 255, 1030, "short", 1, True, 65, 256), (1, 255, 1023, "contig", 1, False, 1, 256),
    (1, 256, 1024, "contig", 1, True, 1, 256), (1, 300, 40, "contig", 1, False, 1, 256), (1, 1023, 3, "contig", 1, False, 1, 256),
    (1, 1024, 3, "contig_v2", 1, False, 1, 256), (1, 2048, 3, "contig_v2", 1, False, 1, 256),
    (1, 6000, 1, "contig_v2", 3, False, 3, 256), (1, 70000, 1, "contig_v2", 9, False, 9, 256),
    (1, 4096, 1030, "contig_v2", 2, True, 2, 256), (1, 1025, 3, "contig_v2_odd", 1, False, 1, 256),
    (1, 2047, 3, "contig_v2_odd", 1, False, 1, 256), (1, 2049, 3, "contig_v2_odd", 2, False, 2, 256),
    (1, 6001, 2, "contig_v2_odd", 3, False, 3, 256), (1, 70001, 1, "contig_v2_odd", 9, False, 9, 256),
    (1, 1025, 1030, "contig_v2_odd", 1, True, 1, 256), (2, 9, 1, "strided", 1, False, 1, 256),
    (7, 5000, 1, "strided", 313, False, 1, 256), (100, 600, 1, "strided", 38, False, 1, 256),
    (128, 257, 3, "strided", 17, False, 1, 256), (300, 257, 1, "strided", 17, False, 2, 256),
    (3, 70000, 1, "strided", 2048, False, 1, 256), (511, 600, 1, "strided", 38, False, 2, 256),
    (255, 40, 70, "strided", 3, True, 1, 256), (16, 20, 1100, "strided", 2, True, 1, 256),
    (512, 40, 1, "strided_v2", 3, False, 1, 256), (512, 600, 1, "strided_v2", 38, False, 1, 256),
    (514, 33, 3, "strided_v2", 3, True, 2, 192), (600, 16, 30, "strided_v2", 1, True, 2, 192),
    (513, 37, 1, "strided_v2_odd", 3, False, 2, 192), (513, 600, 1, "strided_v2_odd", 38, False, 2, 192),
    (515, 33, 3, "strided_v2_odd", 3, True, 2, 192), (601, 16, 30, "strided_v2_odd", 1, True, 2, 192),
]
GEN_ROUTE_TABLE = [
    (1, 5, 1, "contig", 1, False, 1, 256), (1, 300, 40, "contig", 1, False, 1, 256), (1, 2049, 3, "contig", 2, False, 2, 256),
    (1, 6001, 2, "contig", 3, False, 3, 256), (1, 17, 5000, "contig", 1, True, 1, 256), (1, 2048, 3, "contig_v2", 1, False, 1, 256),
    (1, 6000, 1, "contig_v2", 3, False, 3, 256), (1, 70000, 1, "contig_v2", 9, False, 9, 1024),
    (1, 4096, 1030, "contig_v2", 2, True, 2, 256), (7, 5000, 1, "strided", 10, False, 1, 256),
    (300, 257, 1, "strided", 17, False, 2, 256), (511, 600, 1, "strided", 38, False, 2, 256),
    (513, 600, 1, "strided", 38, False, 3, 256), (1001, 9, 1, "strided", 1, False, 4, 256),
    (1025, 20, 1, "strided", 2, True, 5, 256), (512, 40, 1, "strided_v2", 3, False, 1, 256),
    (512, 600, 1, "strided_v2", 38, False, 1, 256), (1100, 20, 1, "strided_v2", 2, True, 8, 128),
    (8192, 100, 1, "strided_v2", 7, True, 16, 256),
]


def row_id(row) -> str:
    return f"{row[0]}x{row[1]}x{row[2]}-{row[3]}"


def realise(pre: int, red: int, post: int):
    """(tensor shape, dim) whose [pre, red, post] view is the row: dim -1 (all elements) for [1, n, 1]"""
    if pre == 1 and post == 1:
        return (red, 1), -1
    if pre == 1:
        return (red, post), 0
    if post == 1:
        return (pre, red), 1
    return (pre, red, post), 1


def out_shape(shape, dim):
    return (1, 1) if dim < 0 else tuple(1 if d == dim else e for d, e in enumerate(shape))


def slices(flat, pre: int, red: int, post: int) -> np.ndarray:
    v = np.asarray(flat, dtype=np.float64).reshape((pre, red, post), order="F")
    return np.ascontiguousarray(v.transpose(2, 0, 1).reshape(pre * post, red))


def unslice(s2: np.ndarray, pre: int, red: int, post: int) -> np.ndarray:
    """the column-major flat data of a [nslices, red] array"""
    return np.ascontiguousarray(s2.reshape(post, pre, red).transpose(1, 2, 0)).reshape(-1, order="F")


def gamma(k: int) -> Fraction:
    return Fraction(k, 2 ** 53 - k) if k > 0 else Fraction(0)


class Q:
    """an array of exact rationals: numerators and positive denominators as numpy object arrays of Python integers (never reduced -
    the numbers here stay within a few hundred bits), so that whole output tensors are compared exactly without a Python loop"""

    def __init__(self, n, d=1):
        self.n, self.d = np.broadcast_arrays(np.asarray(n, dtype=object), np.asarray(d, dtype=object))

    @staticmethod
    def of(x):
        if isinstance(x, Q):
            return x
        f = Fraction(x)
        return Q(f.numerator, f.denominator)

    @staticmethod
    def dyadic(m, e):
        """m * 2^e for an integer array m and an integer (array) e"""
        m, e = np.asarray(m).astype(object), np.asarray(e).astype(object)
        one = np.ones(np.broadcast(m, e).shape, dtype=object)
        return Q(m << np.maximum(e, 0), one << np.maximum(-e, 0))

    @staticmethod
    def floats(x):
        """the exact values of finite f64s"""
        x = np.asarray(x, dtype=np.float64)
        assert np.isfinite(x).all()
        mi, e = _mant_exp(x)
        return Q.dyadic(mi, np.where(mi != 0, e, 0))

    def __add__(self, o):
        o = Q.of(o)
        return Q(self.n * o.d + o.n * self.d, self.d * o.d)

    def __sub__(self, o):
        o = Q.of(o)
        return Q(self.n * o.d - o.n * self.d, self.d * o.d)

    def __mul__(self, o):
        o = Q.of(o)
        return Q(self.n * o.n, self.d * o.d)

    def over(self, c):
        """divided by positive integers"""
        return Q(self.n, self.d * np.asarray(c).astype(object))

    def __abs__(self):
        return Q(np.abs(self.n), self.d)

    def le(self, o) -> np.ndarray:
        o = Q.of(o)
        return (self.n * o.d <= o.n * self.d).astype(bool)

    def maximum(self, o):
        o = Q.of(o)
        w = self.le(o)
        return Q(np.where(w, o.n, self.n), np.where(w, o.d, self.d))

    def __getitem__(self, k):
        return Q(self.n[k], self.d[k])

    def fractions(self):
        return [Fraction(int(a), int(b)) for a, b in zip(self.n.ravel(), self.d.ravel())]

    def to_f64(self) -> np.ndarray:
        """correctly rounded (Python's integer true division is)"""
        return np.array([int(a) / int(b) for a, b in zip(self.n.ravel(), self.d.ravel())], dtype=np.float64).reshape(self.n.shape)


def error_ratios(got, exact, bound):
    """(ok, ratio): ok[k] is the EXACT truth of |got[k] - exact[k]| <= bound[k]; ratio[k] is error / bound rounded to f64 for reports
    (0 where both are zero, inf where only the bound is)"""
    err = abs(Q.floats(got) - exact)
    bound = Q.of(bound)
    ok = err.le(bound)
    num, den = err.n * bound.d, bound.n * err.d
    ratio = np.array([0.0 if a == 0 else math.inf if b == 0 else a / b for a, b in zip(num.ravel(), den.ravel())]).reshape(num.shape)
    return ok, ratio


def _mant_exp(x: np.ndarray):
    m, e = np.frexp(x)
    return np.ldexp(m, 53).astype(np.int64), e.astype(np.int64) - 53


# ---- sums -------------------------------------------------------------------------------------------------------------------------
def exact_sums(s2: np.ndarray, absolute: bool = False):
    """(exact slice sums over the non-NaN entries as a Q, array of their counts)"""
    nan = np.isnan(s2)
    w = np.where(nan, 0.0, np.abs(s2) if absolute else s2)
    assert np.isfinite(w).all(), "exact_sums: finite values and NaNs only"
    counts = (~nan).sum(axis=1)
    mi, e = _mant_exp(w)
    nz = mi != 0
    if not nz.any():
        return Q(np.zeros(s2.shape[0], dtype=object)), counts
    emin = int(e[nz].min())
    if int(e[nz].max()) - emin <= 16 and s2.shape[1] <= 1 << 17:  # halves of 27 bits, shifted by <= 16, summed over <= 2^17: < 2^61
        sh = np.where(nz, e - emin, 0)
        hi = mi >> 27
        lo = mi - (hi << 27)
        H, L = (hi << sh).sum(axis=1).astype(object), (lo << sh).sum(axis=1).astype(object)
        return Q.dyadic((H << 27) + L, emin), counts
    fr = [sum((Fraction(float(x)) for x in row), Fraction(0)) for row in w]
    return Q([f.numerator for f in fr], [f.denominator for f in fr]), counts


def sum_bound(red: int, sum_abs: Q) -> Q:
    return sum_abs * gamma(red - 1)


def mean_bound(red: int, sum_abs: Q, s: Q, c) -> Q:
    return (sum_abs * (gamma(red - 1) * (1 + U)) + abs(s) * U).over(c)


def f32_bound(b: Q, exact: Q) -> Q:
    return b + (abs(Q.of(exact)) + b) * U32


# ---- products ---------------------------------------------------------------------------------------------------------------------
PROD_BITS = 400  # an enclosed product keeps this many bits; 70001 truncations widen it by less than 2^-380 relatively


def _tree(items):
    """pairwise product of (lo, hi, shift) enclosures of positive integers: lo * 2^shift <= value <= hi * 2^shift, with lo == hi as
    long as the product fits PROD_BITS bits"""
    while len(items) > 1:
        nxt = []
        for i in range(0, len(items) - 1, 2):
            (al, ah, ash), (bl, bh, bsh) = items[i], items[i + 1]
            lo, hi, sh = al * bl, ah * bh, ash + bsh
            extra = hi.bit_length() - PROD_BITS
            if extra > 0:
                lo, hi, sh = lo >> extra, -((-hi) >> extra), sh + extra
            nxt.append((lo, hi, sh))
        if len(items) & 1:
            nxt.append(items[-1])
        items = nxt
    return items[0] if items else (1, 1, 0)


def exact_prods(s2: np.ndarray):
    """per slice (negative, lo, hi, E): the product P of the non-NaN entries has lo * 2^E <= |P| <= hi * 2^E (Python integers), with
    lo == hi - the exact product - whenever its odd part has at most PROD_BITS bits; the mantissas are multiplied in a pairwise tree
    and the exponents summed"""
    w = np.where(np.isnan(s2), 1.0, s2)
    assert np.isfinite(w).all(), "exact_prods: finite values and NaNs only"
    mi, e = _mant_exp(np.abs(w))
    tz = np.zeros_like(mi)  # drop the trailing zero bits of the mantissas (1 and 2^k become 1)
    low = mi & -mi
    nz = mi != 0
    tz[nz] = np.log2(low[nz].astype(np.float64)).astype(np.int64)
    mi = mi >> tz
    e = np.where(nz, e + tz, 0)
    neg = (np.signbit(w).sum(axis=1) & 1) == 1
    out = []
    for row, es, ng in zip(mi.tolist(), e.sum(axis=1), neg):
        lo, hi, sh = _tree([(m, m, 0) for m in row])
        out.append((bool(ng) and lo != 0, lo, hi, int(es) + sh if lo else 0))
    return out


def prod_enclosure(prods):
    """(negative, lo, hi) of exact_prods' slices as a bool array and two Qs"""
    neg = np.array([q[0] for q in prods], dtype=bool)
    ex = np.array([q[3] for q in prods], dtype=object)
    return neg, Q.dyadic(np.array([q[1] for q in prods], dtype=object), ex), Q.dyadic(np.array([q[2] for q in prods], dtype=object), ex)


def prod_error_ratios(got, prods, red: int, f32: bool = False):
    """(ok, ratio) of |got - P| <= gamma_(red-1) |P| (with the precision-32 term if `f32`), rigorous although P is only enclosed: the
    error is taken against the far end of the enclosure and the bound from its near end; the sign must be P's (a zero P asks for 0)"""
    got = np.asarray(got, dtype=np.float64)
    neg, lo, hi = prod_enclosure(prods)
    g = abs(Q.floats(got))
    err = abs(g - lo).maximum(abs(g - hi))
    b = lo * gamma(red - 1)
    if f32:
        b = f32_bound(b, lo)
    ok = err.le(b)
    num, den = err.n * b.d, b.n * err.d
    ratio = np.array([0.0 if x == 0 else math.inf if y == 0 else x / y for x, y in zip(num, den)])
    zero = np.array([int(x) == 0 for x in lo.n], dtype=bool)
    sign_ok = np.where(zero | (got == 0), True, (got < 0) == neg)
    return ok & sign_ok, np.where(sign_ok, ratio, math.inf)


# ---- dot --------------------------------------------------------------------------------------------------------------------------
def exact_dots(a2: np.ndarray, b2: np.ndarray):
    """(exact sum of a*b per slice, exact sum of |a*b| per slice) as Qs; finite data spanning <= 9 binades per operand"""
    assert np.isfinite(a2).all() and np.isfinite(b2).all() and a2.shape == b2.shape and a2.shape[1] <= 1 << 17
    limbs, emins = [], []
    for x in (a2, b2):
        mi, e = _mant_exp(np.abs(x))
        nz = mi != 0
        emin = int(e[nz].min()) if nz.any() else 0
        assert not nz.any() or int(e[nz].max()) - emin <= 9, "exact_dots: operand spans more than 9 binades"
        big = mi << np.where(nz, e - emin, 0)  # < 2^62
        limbs.append([(big >> (21 * k)) & ((1 << 21) - 1) for k in range(3)])
        emins.append(emin)
    sgn = (np.sign(a2) * np.sign(b2)).astype(np.int64)
    tot = np.zeros(a2.shape[0], dtype=object)
    tot_abs = np.zeros(a2.shape[0], dtype=object)
    for i in range(3):
        for j in range(3):
            p = limbs[0][i] * limbs[1][j]  # < 2^42, summed over <= 2^17
            tot = tot + ((sgn * p).sum(axis=1).astype(object) << (21 * (i + j)))
            tot_abs = tot_abs + (p.sum(axis=1).astype(object) << (21 * (i + j)))
    ex = emins[0] + emins[1]
    return Q.dyadic(tot, ex), Q.dyadic(tot_abs, ex)


def dot_bound(red: int, sum_abs: Q) -> Q:
    return sum_abs * gamma(red)


# ---- data -------------------------------------------------------------------------------------------------------------------------
def exact_sum_data(rng, n: int, bits: int = 20) -> np.ndarray:
    """integers in (-2^bits, 2^bits): f32-representable for bits <= 24; sums of up to 2^(53-bits) of them are exact in any order"""
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=n).astype(np.float64)


def exact_prod_data(rng, n: int) -> np.ndarray:
    """+-1 everywhere; at most 300 entries +-2^k, |k| <= 3 (sum |k| <= 900 < 1022: no subset over- or underflows) and at most 8 odd
    integers from {3, ..., 15} (their product < 15^8 < 2^32: every partial product is exact), at random positions"""
    x = rng.choice([-1.0, 1.0], size=n)
    npow = min(300, n // 2)
    if npow:
        at = rng.choice(n, size=npow, replace=False)
        x[at] = rng.choice([-1.0, 1.0], size=npow) * np.ldexp(1.0, rng.integers(-3, 4, size=npow))
    nodd = min(8, n // 3)
    if nodd:
        at = rng.choice(n, size=nodd, replace=False)
        x[at] = rng.choice([-1.0, 1.0], size=nodd) * rng.choice([3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0], size=nodd)
    return x


def exact_class_prods(s2: np.ndarray) -> np.ndarray:
    """the exact products of exact_prod_data slices (NaNs left out) as f64, built from integer pieces: the parity of the negative
    entries, the sum of the binary exponents and the product of the <= 8 mantissas that are not 1"""
    w = np.where(np.isnan(s2), 1.0, s2)
    m, e = np.frexp(np.abs(w))          # |w| = (2 m) * 2^(e - 1), 2 m in [1, 2): 1 for a power of two, odd / 2^j otherwise
    odd = np.prod(2.0 * m, axis=1)      # <= 8 factors != 1 per tensor, product of small dyadics: exact
    neg = (w < 0).sum(axis=1) & 1
    return np.where(neg == 1, -1.0, 1.0) * np.ldexp(odd, (e.astype(np.int64) - 1).sum(axis=1).astype(np.int32))


def rounded_sum_data(rng, n: int) -> np.ndarray:
    """full mantissas over 9 binades with random signs (cancellation): +-uniform[1, 2) * 2^k, k in -8 .. 0"""
    return rng.choice([-1.0, 1.0], size=n) * np.ldexp(rng.uniform(1.0, 2.0, size=n), rng.integers(-8, 1, size=n))


def rounded_prod_data(rng, n: int) -> np.ndarray:
    """+-(1 + d), |d| <= 2^-12: a sub-product of up to 70001 of them stays within 2^+-26"""
    return rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.uniform(-2.0 ** -12, 2.0 ** -12, size=n))


def to_f32(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float32).astype(np.float64)


# ---- NaN placement ----------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("none", "first", "last", "boundary", "whole")


def chunk_starts(red: int, nsplit: int, kernel: str = ""):
    """the first element of every chunk but the first, as the kernels cut a slice (skel_reduce.h): ceil(red / nsplit) elements for the
    strided kernels; for the contiguous ones that length rounded up to the block size - in elements, or in pairs for the 16-byte
    forms - where the block is 1024 threads for slices of 64 KiB and more and 256 below (reduce_plan.h), at either storage width"""
    c = -(-red // nsplit)
    starts = {c * s for s in range(1, nsplit)}
    if kernel.startswith("contig"):
        unit = 2 if "v2" in kernel else 1  # elements per thread and step
        for elem_bytes in (8, 4):
            bs = 1024 if red * elem_bytes >= 65536 else 256
            chunk = -(-(-(-(red // unit) // nsplit)) // bs) * bs * unit
            starts |= {chunk * s for s in range(1, nsplit)}
    return sorted(b for b in starts if 0 < b < red)


def boundary_indices(red: int, nsplit: int, kernel: str = ""):
    """the last element of every chunk and the first of the next (chunk_starts); the middle pair of an unsplit slice"""
    if nsplit <= 1:
        return sorted({max(red // 2 - 1, 0), min(red // 2, red - 1)})
    return sorted({i for b in chunk_starts(red, nsplit, kernel) for i in (b - 1, b)})


def place_nans(s2: np.ndarray, how: str, nsplit: int, kernel: str = "") -> np.ndarray:
    """a copy with NaNs in every third slice (ids 0, 3, ...), the others stay clean; 'whole' fills ids 1, 4, ... (a lone slice: itself)"""
    out = s2.copy()
    n, red = out.shape
    if how == "none":
        return out
    if how == "whole":
        out[0 if n == 1 else slice(1, None, 3), :] = np.nan
        return out
    cols = {"first": [0], "last": [red - 1], "boundary": boundary_indices(red, nsplit, kernel)}[how]
    out[0::3, cols] = np.nan
    return out
