"""Elementwise math at the edges of its domains (-m gpu) against exact values: tests/golden/elementwise_edges_*.json holds, per
function, the special values, the doubles around every domain boundary and overflow / underflow threshold, the usual libm branch
points, arguments next to multiples of pi/2, the Annex F tables of pow / hypot / atan2 and a ladder of magnitudes over the whole
finite domain, each with the correctly rounded exact result (tests/golden/make_elementwise_edges.py, mpmath; glibc alone passes:
test_elementwise_edges_host.py).  Every path that serves a function is held to the project's own bound against the exact value:

  * the per-op kernel (`unary_*` / `elem_*`), the fused f64 kernel, and for log1p / expm1 / log10 the planner's lossy spelling, which
    the front end must turn back into the library function;
  * the same on a precision-32 provider for the arguments exact in binary32: equal to the f64 provider's result rounded once, and
    within one binary32 ulp of the exact value rounded once (generated sin / cos run rm_sincos_r32: only the second).

NaN exactly where the exact result is NaN; +-inf, +-0 and every result IEEE 754 / Annex F fix (and pow(x, 2), the exact product)
equal to the bit; everything else |(got - want) / ulp(want) - resid| <= bound."""
import numpy as np
import pytest

import elementwise_edges as ee
from test_gpu_f32 import f32r, same_values
from test_gpu_parity import LIBM_ULP, SINC_ABS, _run_fused, bits_equal

pytestmark = pytest.mark.gpu

UNARY = sorted(LIBM_ULP) + ["sqrt", "erf"]
FUSED_UNARY = [n for n in UNARY if n != "erf"]  # the planner's vocabulary (fusion.rs:2971-3000) has no erf
REWRITTEN = {"log1p": "log(input0.data[i0] + f64(1.0))", "expm1": "(exp(input0.data[i0]) - f64(1.0))",
             "log10": "(log(input0.data[i0]) * f64(0.4342944819032518))"}

# Edge bounds: where ocml's own function, called exactly as the library calls it (`cos(v)`, `tan(v)`), exceeds the project's bound at
# an edge, that argument gets a named bound here - the measured error rounded up to a whole ulp; LIBM_ULP holds everywhere else.
#   0x1.6ac5b262ca1ffp+849, the double nearest a multiple of pi/2 (6381956970095103 * 2^797 = (2k + 1) pi/2 - 4.69e-19; 61 bits
#   cancel in the reduction): ocml's cos is 404.955 ulp from the exact -4.687165924254627611e-19 and its tan 693.361 ulp from
#   -2.1334853...e18, per-op and fused alike (MI355X, ROCm 7 ocml, first run of this file; glibc is 7.955 / 14.361 ulp off at the same
#   argument).  sin there is 1 to the last bit.
HARDEST_REDUCTION = float.fromhex("0x1.6ac5b262ca1ffp+849")
COS_HARDEST_REDUCTION_ULP = 405
TAN_HARDEST_REDUCTION_ULP = 694
EDGE_ULP = {"cos": (HARDEST_REDUCTION, COS_HARDEST_REDUCTION_ULP), "tan": (HARDEST_REDUCTION, TAN_HARDEST_REDUCTION_ULP)}


def edge_bounds(name, entry):
    """The bound per point: the project's own, and the named edge bound at its one argument."""
    limits = np.full(entry["want"].shape, float(ee.bound(name)))
    if name in EDGE_ULP:
        x, ulps = EDGE_ULP[name]
        at = ee.same_bits(entry["args"][0], np.full(limits.shape, x))
        assert np.count_nonzero(at) == 1
        limits[at] = ulps
    return limits


@pytest.fixture(scope="module")
def prov32(built):
    import os
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def _column(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 1)


def _per_op(p, name, args):
    hs = [p.upload(_column(a)) for a in args]
    out = getattr(p, ("elem_" if name in ee.BINARY else "unary_") + name)(*hs)
    got = p.download(out)
    for h in hs + [out]:
        p.free(h)
    return got


def _plan(name):
    from planner_requests import FusionGroupPlan

    p = FusionGroupPlan()
    ins = [p.input() for _ in range(2 if name in ee.BINARY else 1)]
    return p, (p.primitive("ElemPow", *ins) if name == "pow" else p.builtin(name, *ins))


def _fused(p, name, args, scalar_ty="f64"):
    plan, out = _plan(name)
    hs = [p.upload(_column(a)) for a in args]
    n = int(np.size(args[0]))
    res = p.fused_elementwise(plan.generate_wgsl_for_output(out, scalar_ty), hs, (n, 1), n)
    got = p.download(res)
    for h in hs + [res]:
        p.free(h)
    return got


def _judge(name, got, entry, path):
    # pow(x, 2) is the product rounded once (rm_pow, skel_common.h): correctly rounded, so `want` itself
    square = ee.same_bits(entry["args"][1], np.full(entry["want"].shape, 2.0)) if name == "pow" else None
    limits = edge_bounds(name, entry)
    fails, worst = ee.judge(name, got, entry, limits, also_bitwise=square)
    held = limits == ee.bound(name)
    rest = ee.judge(name, np.where(held, got, entry["want"]), entry, limits, also_bitwise=square)[1] if not held.all() else worst
    print(f"edge-accuracy {path} {name}: max {rest:.3f} ulp against exact over {entry['want'].size} points (bound {ee.bound(name)})"
          + (f"; {worst:.3f} ulp at the edge bound {limits.max():.0f}" if not held.all() else ""))
    assert not fails, f"{len(fails)} of {entry['want'].size} points:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("name", UNARY + list(ee.BINARY))
def test_per_op_kernels_at_the_edges(prov, name):
    e = ee.load()[name]
    _judge(name, _per_op(prov, name, e["args"]), e, "per-op")


@pytest.mark.parametrize("name", FUSED_UNARY + list(ee.BINARY))
def test_fused_kernels_at_the_edges(prov, name):
    e = ee.load()[name]
    _judge(name, _fused(prov, name, e["args"]), e, "fused")


@pytest.mark.parametrize("name", sorted(REWRITTEN))
def test_rewritten_spellings_are_the_library_functions(prov, name):
    """The planner spells log1p(x) as log(x + 1), expm1(x) as (exp(x) - 1) and log10(x) as (log(x) * 0.434...) (builtin_expr,
    fusion.rs:3005-3019); the CPU builtins call libm's functions, so the front end rewrites exactly these spellings.  The fused kernel
    of the lossy text must return what the per-op kernel's library call returns, bit for bit, over every edge - log1p(2^-54) is 2^-54,
    not log(1) = 0 - while the same arithmetic arriving as two steps (a user's own log(x + 1)) stays as written and differs."""
    from planner_requests import FusionGroupPlan, builtin_expr

    assert builtin_expr(name, ["input0.data[i0]"], "f64") == REWRITTEN[name]
    plan, out = _plan(name)
    assert REWRITTEN[name] in plan.generate_wgsl_for_output(out, "f64")
    e = ee.load()[name]
    (x,) = e["args"]
    fused, per_op = _fused(prov, name, e["args"]), _per_op(prov, name, e["args"])
    _judge(name, fused, e, "rewritten")
    assert bits_equal(fused, per_op)
    # |x| <= 2^-54: f(x) = x - x^2/2 + ... rounds to x; the bound above keeps the library within 2 ulp of it (nonzero for a normal
    # x), and at 1e-17 it must be x itself, where the lossy form gives log(1) = exp(x) - 1 = 0
    tiny = (np.abs(x) <= 2.0 ** -54) & (np.abs(x) >= 2.0 ** -1022)
    if name != "log10":
        at = np.abs(x) == 1e-17
        assert np.count_nonzero(tiny) >= 8 and np.all(fused[tiny] != 0.0) and np.count_nonzero(at) == 2 and bits_equal(fused[at], x[at])
    # the unrewritten form: the constant arrives as an input, so the text is two steps and no rewrite applies
    q = FusionGroupPlan()
    a, c = q.input(), q.input()
    if name == "log1p":
        r, cval = q.builtin("log", q.primitive("Add", a, c)), 1.0
    elif name == "expm1":
        r, cval = q.primitive("Sub", q.builtin("exp", a), c), 1.0
    else:
        r, cval = q.primitive("ElemMul", q.builtin("log", a), c), 0.4342944819032518
    plain = _run_fused(prov, q, r, [_column(x), np.array([[cval]])], (x.size, 1)).reshape(-1)
    if name != "log10":
        assert np.all(plain[tiny] == 0.0)
    assert not bits_equal(plain, fused)


def _within_one_f32_ulp(got, want32):
    got, want32 = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want32, dtype=np.float64).reshape(-1)
    if got.shape != want32.shape or not np.array_equal(np.isnan(got), np.isnan(want32)):
        return False
    m = ~np.isnan(want32)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = np.spacing(np.abs(want32[m]).astype(np.float32)).astype(np.float64)  # NaN at inf: only equality passes there
        return bool(np.all((got[m] == want32[m]) | (np.abs(got[m] - want32[m]) <= sp)))


@pytest.mark.parametrize("name", UNARY + list(ee.BINARY))
def test_precision32_provider_at_the_edges(prov32, prov, name):
    """The arguments exact in binary32 (with exp(88.72...) and exp(89), cosh(90), pow(10, 39): the f64 result overflows binary32 and inf
    is stored; exp(-103), exp(-104): a binary32 subnormal and 0).  Arithmetic is f64 in registers, rounded once on store."""
    e = ee.load()[name]
    m = ee.f32_exact(e)
    args = [a[m] for a in e["args"]]
    assert np.count_nonzero(m) >= 25, np.count_nonzero(m)
    want32 = f32r(e["want"][m])
    got = _per_op(prov32, name, args)
    assert same_values(got, f32r(_per_op(prov, name, args))), name
    assert _within_one_f32_ulp(got, want32), name
    if name == "erf":
        return
    got = _fused(prov32, name, args, "f32")
    if name in ("sin", "cos"):  # rm_sincos_r32: the short form below 2^20, the library above
        zero = args[0] == 0.0
        assert name == "cos" or np.array_equal(np.signbit(got[zero]), np.signbit(args[0][zero]))  # sin(-0) = -0
    else:
        assert same_values(got, f32r(_fused(prov, name, args))), name
    assert _within_one_f32_ulp(got, want32), name


# ---- the bitwise ops on a wider grid ---------------------------------------------------------------------
from elementwise_edges import EXACT_BINARY, EXACT_UNARY, T52, T53, T60, WIDE  # noqa: E402


def test_per_op_exact_ops_bitwise_on_the_wide_grid(prov, oracle):
    X, Y = np.meshgrid(WIDE, WIDE, indexing="ij")
    hx, hy = prov.upload(X), prov.upload(Y)
    for op in EXACT_UNARY:
        h = getattr(prov, "unary_" + op)(hx)
        assert bits_equal(prov.download_matrix(h), oracle.unary(op, X)), op
        prov.free(h)
    for op in EXACT_BINARY:
        h = prov._binary(op, hx, hy)
        got, want = prov.download_matrix(h), oracle.binary(op, X, Y)
        assert bits_equal(got, want), (op, [(float(a).hex(), float(b).hex()) for a, b in zip(X[got != want][:5], Y[got != want][:5])])
        prov.free(h)
    prov.free(hx)
    prov.free(hy)


def test_fused_exact_ops_bitwise_on_the_wide_grid(prov, oracle):
    from planner_requests import FusionGroupPlan

    X, Y = np.meshgrid(WIDE, WIDE, indexing="ij")
    for op in EXACT_UNARY:
        p = FusionGroupPlan()
        assert bits_equal(_run_fused(prov, p, p.builtin(op, p.input()), [X], X.shape), oracle.unary(op, X)), op
    for op in EXACT_BINARY:
        p = FusionGroupPlan()
        a, b = p.input(), p.input()
        got, want = _run_fused(prov, p, p.builtin(op, a, b), [X, Y], X.shape), oracle.binary(op, X, Y)
        assert bits_equal(got, want), (op, [(float(a).hex(), float(b).hex()) for a, b in zip(X[got != want][:5], Y[got != want][:5])])


def test_scalar_ops_with_special_scalars_bitwise(prov, oracle):
    x = WIDE.reshape(-1, 1)
    hx = prov.upload(x)
    for s in (0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, T60, 5e-324):
        S = np.full(x.shape, s)
        for op, want in (("add", oracle.binary("add", x, S)), ("sub", oracle.binary("sub", x, S)), ("mul", oracle.binary("mul", x, S)),
                         ("div", oracle.binary("div", x, S)), ("rsub", oracle.binary("sub", S, x)), ("rdiv", oracle.binary("div", S, x)),
                         ("max", oracle.binary("max", x, S)), ("min", oracle.binary("min", x, S))):
            h = getattr(prov, "scalar_" + op)(hx, s)
            assert bits_equal(prov.download_matrix(h), want), (op, s)
            prov.free(h)
    prov.free(hx)


def test_sinc_at_integers_and_half_integers(prov, oracle):
    k = np.array([1.0, 2.0, 3.0, 7.0, 100.0, 2.0 ** 20, 2.0 ** 40, 2.0 ** 51])
    half = np.array([0.5, 1.5, 2.5, 1000.5, 2.0 ** 30 + 0.5, 2.0 ** 51 + 0.5])
    parts = [k, np.nextafter(k, np.inf), np.nextafter(k, 0.0), half, [T52, T52 + 1.0, T53, 1e300, 5e-324, 1e-310, 2.0 ** -30]]
    x = np.concatenate([np.concatenate(parts), -np.concatenate(parts), [0.0, -0.0, np.inf, -np.inf, np.nan]]).reshape(-1, 1)
    got = _per_op(prov, "sinc", (x,)).reshape(-1, 1)
    with np.errstate(invalid="ignore"):
        want = oracle.unary("sinc", x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.max(np.abs(got[fin] - want[fin])) <= SINC_ABS
    whole = fin & (x == np.trunc(x)) & (x != 0.0)
    assert np.all(got[whole] == 0.0) and np.all(got[x == 0.0] == 1.0)  # sinc(integer) = 0, sinc(+-0) = 1
