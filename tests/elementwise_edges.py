"""TEST INFRASTRUCTURE: reads tests/golden/elementwise_edges_*.json (exact values at the domain edges, written by
tests/golden/make_elementwise_edges.py with mpmath) and judges a result against them.  Shared by the CPU check of the fixture itself
(test_elementwise_edges_host.py: glibc must pass) and the device tests (test_gpu_elementwise_edges.py).  Needs numpy only."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
FAMILIES = ("trig", "exp_log", "hyperbolic", "binary")
BINARY = ("pow", "hypot", "atan2")
MAX_FIXTURE_BYTES = 103892  # the largest fixture before these files (accel_provider_methods.json)
_cache = {}


def fixture_paths():
    return [GOLDEN / f"elementwise_edges_{f}.json" for f in FAMILIES]


def _f64(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64).view(np.float64)


def load():
    """name -> {"args": (x,) or (a, b), "want", "resid", "exact" (bool mask)}; read once, never modified."""
    if not _cache:
        for path in fixture_paths():
            for name, e in json.loads(path.read_text())["functions"].items():
                args = (_f64(e["a"]), _f64(e["b"])) if name in BINARY else (_f64(e["x"]),)
                exact = np.zeros(len(e["want"]), dtype=bool)
                exact[e["exact"]] = True
                entry = {"args": args, "want": _f64(e["want"]), "resid": np.array(e["resid"], dtype=np.float64), "exact": exact}
                for v in entry.values():
                    for a in (v if isinstance(v, tuple) else (v,)):
                        a.setflags(write=False)
                _cache[name] = entry
    return _cache


def bound(name):
    """The project's own bounds: LIBM_ULP, 2 for pow / hypot / atan2 (test_fused_pow_hypot_atan2), erf as test_unary_erf_sinc_single
    states it, sqrt correctly rounded.  They were set against glibc, itself up to an ulp off; against exact values they carry that
    ulp as slack."""
    from test_gpu_parity import BINARY_LIBM_ULP, ERF_ULP, LIBM_ULP

    if name == "sqrt":
        return 0
    if name == "erf":
        return ERF_ULP
    return BINARY_LIBM_ULP if name in BINARY else LIBM_ULP[name]


def ulp_of(want):
    """Spacing of the doubles at |want|, 2^-1074 for a subnormal want."""
    with np.errstate(invalid="ignore"):
        return np.spacing(np.maximum(np.abs(want), 2.2250738585072014e-308))


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


def errors(got, want, resid):
    """|(got - want) / ulp(want) - resid| = the error against the exact value in ulps of want; inf where one side is finite and
    the other is not (a failure, not a large error), 0 where both are NaN or the same infinity."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        e = np.abs((got - want) / ulp_of(want) - resid)
    nonfinite = ~np.isfinite(got) | ~np.isfinite(want)
    agree = (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))
    return np.where(nonfinite, np.where(agree, 0.0, np.inf), e)


def judge(name, got, entry, limit, also_bitwise=None):
    """(list of failure descriptions, largest error in ulps over the points held to `limit`, a number or one per point).  NaN exactly
    where the fixture has NaN; +-inf, +-0 and every result the fixture marks exact (and `also_bitwise`, a mask) bit-equal; everything
    else within `limit`."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    want, resid = entry["want"], entry["resid"]
    limit = np.broadcast_to(np.asarray(limit, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bitwise = np.isinf(want) | (want == 0.0) | entry["exact"]
    if also_bitwise is not None:
        bitwise = bitwise | also_bitwise
    nan = np.isnan(want)
    err = errors(got, want, resid)
    bad = np.where(nan, ~np.isnan(got), np.where(bitwise, ~same_bits(got, want), ~(err <= limit)))
    fails = []
    for i in np.flatnonzero(bad):
        args = ", ".join(float(a[i]).hex() for a in entry["args"])
        kind = "NaN" if nan[i] else "bitwise" if bitwise[i] else f"{err[i]:.3f} ulp > {limit[i]:g}"
        fails.append(f"{name}({args}) = {float(got[i]).hex()}, want {float(want[i]).hex()} [{kind}]")
    measured = err[~nan & ~bitwise]
    return fails, float(measured.max()) if measured.size else 0.0


def f32_exact(entry):
    """Mask of the points whose arguments are all exactly representable in binary32."""
    m = np.ones(entry["want"].shape, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in entry["args"]:
            r = a.astype(np.float32).astype(np.float64)
            m &= same_bits(a, r) | (np.isnan(a) & np.isnan(r))
    return m


# ---- a wider grid for the ops that are exact to the bit (mod, rem, max, min, round, floor, ceil, fix, sign, scalar_*) -------------
T52, T53, T60 = 2.0 ** 52, 2.0 ** 53, 2.0 ** 60
WIDE = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.0, 5.0, -7.25, np.inf, -np.inf, np.nan,
                 T52 - 0.5, -(T52 - 0.5), T52, -T52, T52 + 1.0, -(T52 + 1.0), T52 / 2 + 0.5, -(T52 / 2 + 0.5), T53, -T53,
                 0.5 - 2.0 ** -54, -(0.5 - 2.0 ** -54), 0.5 + 2.0 ** -53, T60, -T60, 3.0 * T60, T60 + 256.0,
                 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e-300, 1.7976931348623157e308])
EXACT_UNARY = ("round", "floor", "ceil", "fix", "sign")
EXACT_BINARY = ("mod", "rem", "max", "min")
