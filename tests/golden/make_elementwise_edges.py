"""Writes tests/golden/elementwise_edges_{trig,exp_log,hyperbolic,binary}.json: exact values of the elementwise functions at the
edges of their domains.

Per function: the arguments as 64-bit patterns in hex (NaN and -0 survive), `want` = the correctly rounded double of the exact
result (bits again), `resid` = (exact - want) / ulp(want) to three decimals - a test adds it back to measure an error against the real
value instead of against its rounding - and `exact`: the indices whose result IEEE 754 / C Annex F fix to the bit (f(+-0), f(+-inf),
the special-case table of pow; and every sqrt, which is `want` itself whatever its resid).  ulp(want) is the spacing of doubles at |want|, 2^-1074 below the smallest normal.

Everything is computed twice with mpmath, at PREC and at 2 * PREC bits (PREC = 1400 covers the 1024-bit argument reduction of
sin / cos / tan at the largest double with room to spare), rounded by integer arithmetic on the mantissa (subnormal results keep
fewer than 53 bits, overflow gives +-inf, underflow +-0, ties go to even); the files are written only if both runs give the same
bits.  Special values (NaN, +-inf, +-0 arguments and results) never reach mpmath: they follow the tables of C Annex F below.

Arguments per unary function: the special values of both signs; the doubles just outside the domain; eight consecutive doubles on
each side of every domain boundary and of every overflow / underflow / saturation threshold (found by bisection on the rounded
exact result); the branch points libm implementations share, with their neighbours; a seeded ladder of 64 random mantissas whose
exponents cover the whole finite domain; a short ladder of values exact in binary32 for the precision-32 provider; for sin / cos /
tan the doubles (and the binary32 values) nearest k pi/2, +-pi/4, the neighbourhood of 2^20 and a few famous hard cases.

    python tests/golden/make_elementwise_edges.py        (needs mpmath; about a minute)
"""
import json
import math
import random
import struct
from pathlib import Path

import mpmath as mp

PREC = 1400
MAX = 1.7976931348623157e308
FLT_MAX = 3.4028234663852886e38
MIN_NORMAL = 2.0 ** -1022
MAX_SUB = 2.0 ** -1022 - 2.0 ** -1074
TINY = 2.0 ** -1074
INF, NAN = math.inf, math.nan
MAX_BYTES = 103892  # the largest fixture before these (accel_provider_methods.json)


# ---- bits ------------------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def hexbits(x):
    return format(bits(x), "016x")


def key(x):
    """Doubles in order as integers: key(next double above x) == key(x) + 1 (-0 and +0 share 0)."""
    b = bits(x)
    return b if b < 1 << 63 else -(b - (1 << 63))


def unkey(k):
    return from_bits(k) if k >= 0 else from_bits((1 << 63) - k)


def step(x, n):
    return unkey(key(x) + n)


def f32r(x):
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(INF, x)


def is_odd_int(y):
    return math.isfinite(y) and y == math.floor(y) and abs(y) < 2.0 ** 53 and int(y) % 2 == 1


def is_int(y):
    return math.isfinite(y) and y == math.floor(y)


# ---- rounding an mpf to the nearest double ------------------------------------------------------------
def round_double(v):
    """Nearest double of the mpf v, ties to even, by integer arithmetic on its mantissa."""
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return 0.0
    e = exp + bc - 1  # floor(log2 |v|)
    if e > 1023:
        return -INF if sign else INF
    q = max(e, -1022) - 52  # exponent of one unit in the last place
    shift = exp - q
    if shift >= 0:
        n = man << shift
    else:
        n = man >> -shift
        rest = man & ((1 << -shift) - 1)
        half = 1 << (-shift - 1)
        if rest > half or (rest == half and (n & 1)):
            n += 1
    if n == 0:
        return -0.0 if sign else 0.0
    if n.bit_length() + q > 1024:
        return -INF if sign else INF
    r = math.ldexp(n, q)
    return -r if sign else r


def ulp(w):
    a = abs(w)
    if a < MIN_NORMAL:
        return mp.mpf(2) ** -1074
    return mp.mpf(2) ** (math.frexp(a)[1] - 53)


def finish(v):
    """(want, resid, is_exact) of an exact result: a float for the values Annex F names, an mpf for everything else."""
    if isinstance(v, float):
        return v, 0.0, True
    w = round_double(v)
    if math.isinf(w):
        return w, 0.0, False
    r = (v - mp.mpf(w)) / ulp(w)
    resid = round(float(r), 3) + 0.0  # + 0.0: no "-0.0" in the file
    return w, resid, bool(v == mp.mpf(w))


# ---- exact unary functions -----------------------------------------------------------------------------
def _pi(k):
    return mp.pi * k


# stand-ins where the true value is out of mpmath's comfortable reach and its rounding is not in doubt: anything beyond 2^1100 in
# magnitude (rounds to +-inf, its reciprocal to +-0) and a value within 2^-3000 of +-1 (rounds to +-1, resid 0.000)
HUGE = mp.mpf(2) ** 3000
ALMOST_ONE = mp.mpf(1)  # tanh / erf beyond |x| = 1100 differ from 1 by less than 2^-3000


def exact_unary(name, x):
    """A float for the results fixed to the bit (NaN, +-inf, +-0, 1, -1 at special arguments), an mpf otherwise."""
    if math.isnan(x):
        return NAN
    zero, inf, neg = x == 0.0, math.isinf(x), math.copysign(1.0, x) < 0
    X = None if inf else mp.mpf(x)
    if name in ("sin", "tan"):
        return x if zero else NAN if inf else getattr(mp, name)(X)
    if name == "cos":
        return 1.0 if zero else NAN if inf else mp.cos(X)
    if name == "asin":
        return x if zero else NAN if abs(x) > 1 else mp.asin(X)
    if name == "acos":
        return NAN if abs(x) > 1 else 0.0 if x == 1.0 else mp.acos(X)
    if name == "atan":
        return x if zero else (-_pi(0.5) if neg else _pi(0.5)) if inf else mp.atan(X)
    if name == "sinh":
        return x if zero or inf else HUGE * math.copysign(1.0, x) if abs(x) > 1100 else mp.sinh(X)
    if name == "cosh":
        return 1.0 if zero else INF if inf else HUGE if abs(x) > 1100 else mp.cosh(X)
    if name == "tanh":
        return x if zero else math.copysign(1.0, x) if inf else ALMOST_ONE * math.copysign(1.0, x) if abs(x) > 1100 else mp.tanh(X)
    if name == "asinh":
        return x if zero or inf else mp.asinh(X)
    if name == "acosh":
        return NAN if x < 1 else INF if inf else 0.0 if x == 1.0 else mp.acosh(X)
    if name == "atanh":
        return x if zero else NAN if abs(x) > 1 else math.copysign(INF, x) if abs(x) == 1 else mp.atanh(X)
    if name in ("exp", "exp2"):
        if zero:
            return 1.0
        if inf:
            return 0.0 if neg else INF
        if abs(x) > 1100:
            return 1 / HUGE if neg else HUGE
        return mp.exp(X) if name == "exp" else mp.mpf(2) ** X
    if name == "expm1":
        return x if zero else (-1.0 if neg else INF) if inf else HUGE if x > 1100 else mp.expm1(X)
    if name in ("log", "log2", "log10"):
        if zero:
            return -INF
        if neg:
            return NAN
        if inf:
            return INF
        if x == 1.0:
            return 0.0
        return mp.log(X) if name == "log" else mp.log(X) / mp.log(2 if name == "log2" else 10)
    if name == "log1p":
        return x if zero else NAN if x < -1 else -INF if x == -1 else INF if inf else mp.log1p(X)
    if name == "sqrt":
        return x if zero else NAN if neg else INF if inf else mp.sqrt(X)
    if name == "erf":
        return x if zero else math.copysign(1.0, x) if inf else ALMOST_ONE * math.copysign(1.0, x) if abs(x) > 1100 else mp.erf(X)
    raise KeyError(name)


def fixed_unary(name, x):
    """Is f(x) fixed to the bit?  Every sqrt (IEEE 754), and f at +-0 and +-inf (Annex F)."""
    return name == "sqrt" or x == 0.0 or math.isinf(x)


# ---- exact binary functions ----------------------------------------------------------------------------
def exact_pow(x, y):  # C Annex F.10.4.4
    if y == 0.0 or x == 1.0:
        return 1.0
    if math.isnan(x) or math.isnan(y):
        return NAN
    if x == 0.0:
        if is_odd_int(y):
            return math.copysign(INF, x) if y < 0 else x
        return INF if y < 0 else 0.0
    if math.isinf(y):
        if x == -1.0:
            return 1.0
        return (INF if y < 0 else 0.0) if abs(x) < 1 else (0.0 if y < 0 else INF)
    if math.isinf(x):
        if x < 0 and is_odd_int(y):
            return -0.0 if y < 0 else -INF
        return 0.0 if y < 0 else INF
    if x < 0 and not is_int(y):
        return NAN
    if abs(mp.mpf(y) * mp.log(mp.mpf(abs(x)))) > 2000:  # far beyond either end of the range
        v = HUGE if (y > 0) == (abs(x) > 1) else 1 / HUGE
    else:
        v = mp.power(mp.mpf(abs(x)), mp.mpf(y))
    return -v if x < 0 and is_odd_int(y) else v


def exact_hypot(a, b):
    if math.isinf(a) or math.isinf(b):
        return INF
    if math.isnan(a) or math.isnan(b):
        return NAN
    if a == 0.0 and b == 0.0:
        return 0.0
    return mp.sqrt(mp.mpf(a) ** 2 + mp.mpf(b) ** 2)


def exact_atan2(y, x):  # C Annex F.10.1.4
    if math.isnan(x) or math.isnan(y):
        return NAN
    s = math.copysign(1.0, y)
    xneg = math.copysign(1.0, x) < 0
    if y == 0.0:
        return s * _pi(1) if xneg else y
    if x == 0.0:
        return s * _pi(0.5)
    if math.isinf(y):
        return s * _pi(0.75 if xneg else 0.25) if math.isinf(x) else s * _pi(0.5)
    if math.isinf(x):
        return s * _pi(1) if xneg else math.copysign(0.0, y)
    v = mp.atan2(mp.mpf(y), mp.mpf(x))
    return v


EXACT_BINARY = {"pow": exact_pow, "hypot": exact_hypot, "atan2": exact_atan2}
SPECIAL_OPERANDS = (0.0, -0.0, 1.0, -1.0, INF, -INF)


def fixed_binary(name, a, b):
    """pow: the rows of its Annex F table (x among +-0, 1, +-inf or y among +-0, +-inf); hypot / atan2: zero or infinite operands,
    and the 3-4-5 triple among the subnormals."""
    if name == "pow":
        return a in (0.0, 1.0, INF, -INF) or b in (0.0, INF, -INF)
    return any(v == 0.0 or math.isinf(v) for v in (a, b)) or (a, b) == (3 * 2.0 ** -1070, 4 * 2.0 ** -1070)


# ---- argument sets -------------------------------------------------------------------------------------
def both(vals):
    return [s * v for v in vals for s in (1.0, -1.0)]


SPECIALS = both([0.0, TINY, MAX_SUB, MIN_NORMAL, 1.0, MAX, INF]) + [NAN]
LN2 = 0.6931471805599453
BRANCH = [2.0 ** -54, 2.0 ** -28, 2.0 ** -27, 2.0 ** -26, 2.0 ** -10, 0.5 * LN2, 1.5 * LN2, 0.5, math.sqrt(0.5), math.sqrt(2.0), 22.0,
          2.0 ** 28, 2.0 ** 52, 2.0 ** 53]


def around(t, n=8):
    """n doubles up to and including t, and the n above it."""
    return [step(t, k) for k in range(-n + 1, n + 1)]


def boundary(t, n=8):
    """t with n doubles on each side."""
    return [step(t, k) for k in range(-n, n + 1)]


def branch_points():
    out = []
    for b in BRANCH:
        out += [step(b, -1), b, step(b, 1), -b]
    return out


def ladder(rng, lo_exp, hi, signed, count=64, mant_bits=52):
    """`count` magnitudes 2^e * (1 + random mantissa), e evenly spread over [lo_exp, log2 hi], never above hi; with 23 mantissa bits
    they are rounded to binary32 (only its subnormals change)."""
    hi_exp = math.frexp(hi)[1] - 1
    out = []
    for i in range(count):
        e = lo_exp + round(i * (hi_exp - lo_exp) / (count - 1))
        m = 1.0 + (rng.getrandbits(mant_bits) + 0.0) / (1 << mant_bits)
        v = min(math.ldexp(m, e), hi)
        if mant_bits == 23:
            v = f32r(v)
        out.append(-v if signed and rng.getrandbits(1) else v)
    return out


def last_false(pred, lo, hi):
    """The largest double in [lo, hi) at which pred is false; pred(lo) is false, pred(hi) true, pred monotone."""
    a, b = key(lo), key(hi)
    assert not pred(lo) and pred(hi)
    while b - a > 1:
        m = (a + b) // 2
        if pred(unkey(m)):
            b = m
        else:
            a = m
    return unkey(a)


def rounded(name, x):
    return finish(exact_unary(name, x))[0]


def nearest_pi_multiples():
    ks = list(range(1, 65)) + [2 ** j for j in range(7, 31)]
    return [round_double(mp.pi * k / 2) for k in ks]


# name -> (family, largest magnitude of the finite domain, signed ladder?, lowest ladder exponent)
UNARY = {
    "sin": ("trig", MAX, True, -1074), "cos": ("trig", MAX, True, -1074), "tan": ("trig", MAX, True, -1074),
    "asin": ("trig", 1.0, True, -1074), "acos": ("trig", 1.0, True, -1074), "atan": ("trig", MAX, True, -1074),
    "sinh": ("hyperbolic", 711.0, True, -1074), "cosh": ("hyperbolic", 711.0, True, -1074), "tanh": ("hyperbolic", MAX, True, -1074),
    "asinh": ("hyperbolic", MAX, True, -1074), "acosh": ("hyperbolic", MAX, False, 0), "atanh": ("hyperbolic", 1.0, True, -1074),
    "exp": ("exp_log", 746.0, True, -1074), "exp2": ("exp_log", 1076.0, True, -1074), "expm1": ("exp_log", 710.0, True, -1074),
    "log": ("exp_log", MAX, False, -1074), "log2": ("exp_log", MAX, False, -1074), "log10": ("exp_log", MAX, False, -1074),
    "log1p": ("exp_log", MAX, False, -1074), "sqrt": ("exp_log", MAX, False, -1074), "erf": ("exp_log", MAX, True, -1074),
}


def in_domain(name, x):
    if name in ("asin", "acos", "atanh"):
        return abs(x) <= 1
    if name == "acosh":
        return x >= 1
    if name in ("log", "log2", "log10", "sqrt"):
        return x >= 0
    if name == "log1p":
        return x >= -1
    return True


def unary_arguments(name):
    rng = random.Random("elementwise edges " + name)
    _, hi, signed, lo_exp = UNARY[name]
    xs = list(SPECIALS)
    # just outside the domain, and every boundary with eight doubles on each side
    if name in ("asin", "acos", "atanh"):
        xs += boundary(1.0) + boundary(-1.0)
    if name == "acosh":
        xs += boundary(1.0) + [-1.0, -2.0]
    if name in ("log", "log2", "log10"):
        xs += boundary(1.0) + [step(0.0, k) for k in range(-8, 9)] + [-1.0]
    if name == "sqrt":
        xs += [step(0.0, k) for k in range(-8, 9)] + boundary(1.0) + boundary(4.0)
    if name == "log1p":
        xs += boundary(-1.0) + [step(0.0, k) for k in range(-8, 9)] + [-2.0]
    # overflow / underflow / saturation thresholds of the rounded exact result
    if name in ("exp", "exp2", "expm1"):
        xs += around(last_false(lambda x: math.isinf(rounded(name, x)), 700.0, 1100.0))
    if name in ("exp", "exp2"):
        xs += around(last_false(lambda x: rounded(name, x) >= MIN_NORMAL, -1100.0, -700.0))
        xs += around(last_false(lambda x: rounded(name, x) > 0.0, -1100.0, -700.0))
        xs += [88.72283935546875, 88.72284698486328, 89.0, -103.0, -104.0, 128.0, -150.0]  # around the ends of binary32
    if name == "expm1":
        xs += around(last_false(lambda x: rounded(name, x) > -1.0, -50.0, -30.0))
    if name in ("expm1", "log1p"):
        xs += [1e-17, -1e-17]  # f(x) = x to the last bit; exp(x) - 1 and log(x + 1) give 0
    if name in ("sinh", "cosh"):
        t = last_false(lambda x: math.isinf(rounded(name, x)), 700.0, 720.0)  # 710.4758600739439
        xs += around(t) + [-v for v in around(t)] + [90.0, -90.0]
    if name == "tanh":
        t = last_false(lambda x: rounded(name, x) == 1.0, 15.0, 25.0)  # near 19.06
        xs += around(t) + [-v for v in around(t)]
    if name == "erf":
        xs += around(last_false(lambda x: rounded(name, x) == 1.0, 4.0, 8.0))
    if name in ("sin", "cos", "tan"):
        near = nearest_pi_multiples()
        xs += near + [f32r(v) for v in near]
        xs += both([round_double(mp.pi / 4)]) + both([step(1048576.0, -1), 1048576.0, step(1048576.0, 1)])
        xs += both([1048575.9375, 1048576.125]) + [1e22, float.fromhex("0x1.6ac5b262ca1ffp+849"), 3e6, -7e9, f32r(1e22), FLT_MAX, -FLT_MAX]
    xs += [v for v in branch_points() if in_domain(name, v)]
    lad = ladder(rng, lo_exp, hi, signed)
    if name == "log1p":
        lad += [-v for v in ladder(rng, -1074, 1.0, False, count=16)]
    xs += lad
    # values exact in binary32, over its whole exponent range (for a precision-32 provider)
    xs += ladder(rng, max(lo_exp, -149), min(hi, FLT_MAX), signed, count=16, mant_bits=23)
    if name in ("asin", "acos", "atanh", "acosh"):
        xs = [v for v in xs if in_domain(name, v) or abs(v) < 4 or math.isinf(v) or v != v]  # only the near outside is of interest
    seen, out = set(), []
    for v in xs:
        if bits(v) not in seen:
            seen.add(bits(v))
            out.append(v)
    return out


def binary_arguments(name):
    rng = random.Random("elementwise edges " + name)
    special = list(SPECIAL_OPERANDS) + [NAN]
    pairs = []
    if name == "pow":
        generic_y = [-3.0, -2.0, -0.5, 0.5, 2.0, 3.0, 2.5, 2.0 ** 60, -(2.0 ** 60), TINY, MAX, -MAX]
        generic_x = [-2.0, -0.5, 0.5, 2.0, TINY, -TINY, MAX, -MAX]
        pairs += [(x, y) for x in special for y in special + generic_y]
        pairs += [(x, y) for x in generic_x for y in special]
        # negative finite bases: odd, even, non-integer and huge even exponents
        pairs += [(x, y) for x in (-2.0, -0.75, -8.0, -1e10, -TINY) for y in (3.0, -3.0, 4.0, -4.0, 2.5, 1.0 / 3.0, 2.0 ** 53, 2.0 ** 60,
                                                                             1e300, 2.0 ** 53 - 1.0, 101.0)]
        # the ends of the range
        pairs += [(2.0, 1023.0), (2.0, 1024.0), (2.0, -1074.0), (2.0, -1075.0), (2.0, -1076.0), (10.0, 308.0), (10.0, 309.0), (10.0, -323.0),
                  (10.0, -324.0), (1e-5, 64.6), (10.0, 39.0), (10.0, 38.0), (10.0, -45.0), (0.5, 1074.0), (0.5, 1075.0)]
        # a logarithm carried beyond double precision
        pairs += [(1.0 + 2.0 ** -52, 2.0 ** 53), (1.0 - 2.0 ** -52, 2.0 ** 53), (1.0 - 2.0 ** -53, 2.0 ** 54), (1.0 + 2.0 ** -52, -(2.0 ** 53)),
                  (1.0 + 2.0 ** -52, 2.0 ** 62), (1.0 - 2.0 ** -53, 2.0 ** 63)]
        # y == 2 (the exact product) and its two neighbours (the library), over the ladder
        xs = ladder(rng, -1074, MAX, True) + ladder(rng, -149, FLT_MAX, True, count=16, mant_bits=23)
        xs += [1.3407807929942597e154, -1.3407807929942597e154, step(1.3407807929942597e154, -1), TINY, -TINY, MAX_SUB, -0.0, 0.0, 3.0,
               1.4916681462400413e-154, 2.0 ** -537, 2.0 ** -538]
        pairs += [(x, y) for y in (2.0, step(2.0, 1), step(2.0, -1)) for x in xs]
        # general exponents over the ladder of bases
        ys = [rng.choice([-1.0, 1.0]) * math.ldexp(1.0 + rng.random(), rng.randrange(-8, 9)) for _ in range(64)]
        pairs += list(zip(ladder(rng, -1074, MAX, False), ys))
    elif name == "hypot":
        pairs += [(x, y) for x in special + [2.5, -MAX] for y in special + [2.5]]
        pairs += [(1e308, 1e308), (MAX, MAX), (3 * 2.0 ** -1070, 4 * 2.0 ** -1070), (INF, NAN), (NAN, -INF), (TINY, TINY), (TINY, -TINY),
                  (MAX_SUB, MIN_NORMAL), (1.0, 2.0 ** 60), (2.0 ** 60, 1.0), (1.0, 2.0 ** 27), (1.0, 2.0 ** 26), (2.0 ** -1074, 2.0 ** -1014),
                  (3.0, 4.0), (5.0, 12.0), (3e38, 3e38), (1e-45, 1e-45)]
        xs, ys = ladder(rng, -1074, MAX, True), ladder(rng, -1074, MAX, True)
        pairs += [(x, 0.0) for x in xs[::4]] + [(-0.0, y) for y in ys[1::8]]
        pairs += list(zip(xs, ys))  # the same exponent in both operands
        pairs += list(zip(xs, ys[8:] + ys[:8])) + list(zip(xs, ys[-1:] + ys[:-1]))  # exponents 8 rungs and one rung apart
        f = ladder(rng, -149, FLT_MAX, True, count=16, mant_bits=23)
        pairs += list(zip(f, f[1:] + f[:1]))
    else:  # atan2(y, x)
        pairs += [(y, x) for y in both([0.0, INF]) for x in both([0.0, INF])]
        pairs += [(y, x) for y in special + [2.5, -2.5] for x in special + [2.5, -2.5]]
        pairs += [(2.0 ** -1070, 2.0 ** 1000), (-(2.0 ** -1070), 2.0 ** 1000), (2.0 ** -1070, -(2.0 ** 1000)), (1.0, TINY), (1.0, -TINY),
                  (TINY, 1.0), (-TINY, -1.0), (TINY, TINY), (MAX, MAX), (MAX, -MAX), (TINY, MAX), (MAX, TINY), (MIN_NORMAL, 1.0),
                  (2.0 ** -1022, 2.0), (1.0, 2.0 ** 60), (2.0 ** 60, 1.0), (1.0, -(2.0 ** 60))]
        ys, xs = ladder(rng, -1074, MAX, True), ladder(rng, -1074, MAX, True)
        pairs += list(zip(ys, xs)) + list(zip(ys, xs[4:] + xs[:4])) + list(zip(ys, xs[-1:] + xs[:-1]))
        f = ladder(rng, -149, FLT_MAX, True, count=16, mant_bits=23)
        pairs += list(zip(f, f[1:] + f[:1]))
    seen, out = set(), []
    for a, b in pairs:
        k = (bits(a), bits(b))
        if k not in seen:
            seen.add(k)
            out.append((a, b))
    return out


# ---- the documents -------------------------------------------------------------------------------------
def entry_unary(name, xs):
    want, resid, exact = [], [], []
    for i, x in enumerate(xs):
        w, r, is_exact = finish(exact_unary(name, x))
        want.append(hexbits(w))
        resid.append(r)
        if (is_exact or name == "sqrt") and fixed_unary(name, x) and not math.isnan(w):
            exact.append(i)
    return {"x": [hexbits(x) for x in xs], "want": want, "resid": resid, "exact": exact}


def entry_binary(name, pairs):
    want, resid, exact = [], [], []
    for i, (a, b) in enumerate(pairs):
        w, r, is_exact = finish(EXACT_BINARY[name](a, b))
        want.append(hexbits(w))
        resid.append(r)
        if is_exact and fixed_binary(name, a, b) and not math.isnan(w):
            exact.append(i)
    return {"a": [hexbits(a) for a, _ in pairs], "b": [hexbits(b) for _, b in pairs], "want": want, "resid": resid, "exact": exact}


def documents(prec, arguments):
    mp.mp.prec = prec
    docs = {}
    for name, (family, *_rest) in UNARY.items():
        docs.setdefault(family, {})[name] = entry_unary(name, arguments[name])
    for name in EXACT_BINARY:
        docs.setdefault("binary", {})[name] = entry_binary(name, arguments[name])
    return docs


def render(family, functions):
    head = {"about": "exact values at the domain edges; written by make_elementwise_edges.py (see its docstring for the fields)",
            "family": family, "precision_bits": [PREC, 2 * PREC]}
    lines = [json.dumps(k) + ": " + json.dumps(v) for k, v in head.items()]
    body = []
    for name, e in functions.items():
        rows = [json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in e.items()]
        body.append(json.dumps(name) + ": {\n   " + ",\n   ".join(rows) + "\n  }")
    return "{\n " + ",\n ".join(lines) + ',\n "functions": {\n  ' + ",\n  ".join(body) + "\n }\n}\n"


def main():
    mp.mp.prec = PREC  # the thresholds are located at the lower precision; both runs then share the arguments
    arguments = {name: unary_arguments(name) for name in UNARY}
    arguments.update({name: binary_arguments(name) for name in EXACT_BINARY})
    low, high = documents(PREC, arguments), documents(2 * PREC, arguments)
    for family in low:
        for name in low[family]:
            if low[family][name] != high[family][name]:
                bad = [i for i, (p, q) in enumerate(zip(low[family][name]["want"], high[family][name]["want"])) if p != q]
                raise SystemExit(f"{name}: {PREC} and {2 * PREC} bits disagree (want differs at {bad}); nothing written")
    here = Path(__file__).resolve().parent
    for family, functions in low.items():
        text = render(family, functions)
        assert json.loads(text)["functions"] == functions
        out = here / f"elementwise_edges_{family}.json"
        if len(text) > MAX_BYTES:
            raise SystemExit(f"{out.name}: {len(text)} bytes, more than {MAX_BYTES}; nothing written for it")
        out.write_text(text)
        print(f"wrote {out} ({len(text)} bytes, " + ", ".join(f"{n} {len(e['want'])}" for n, e in functions.items()) + ")")


if __name__ == "__main__":
    main()
