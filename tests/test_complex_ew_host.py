"""CPU checks of the complex elementwise entry points: the numpy restatement of the CPU builtins' rules (tests/complex_ew_ref.py)
reproduces the builtins' own known answers, the three entry points are bound in every mirror without changing the served set, and
complex_ew.hip compiles for gfx950 within the register budget its 1024-thread blocks need."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_ew_ref as ref  # noqa: E402
from test_kernel_resources import _pick, _resources  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps


def _num(v):
    return float(v)  # numbers, or the strings inf / -inf / nan


def test_reference_reproduces_the_builtins_known_answers():
    cases = json.loads((ROOT / "tests" / "golden" / "complex_ew_kats.json").read_text())["cases"]
    assert len(cases) >= 20
    for case in cases:
        re, im = (np.array([_num(v)]) for v in case["z"])
        got = ref.unary(case["op"], re, im)
        got = [got] if case["op"] in ref.UNARY_REAL else list(got)
        want = [_num(v) for v in case["expect"]]
        assert len(got) == len(want), case
        for g, w in zip(got, want):
            if case["tol"] == 0:
                assert ref.same_bits(g, [w]), (case, g)
            else:
                assert abs(float(g[0]) - w) <= case["tol"], (case, g)


def test_fma_rounds_once():
    a = 1.0 + 2.0 ** -30
    assert ref.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60  # the product's low bits survive; a * a - 1.0 loses them
    assert a * a - 1.0 != ref.fma(a, a, -1.0)
    assert ref.fma(3.0, 4.0, 5.0) == 17.0 and math.isinf(ref.fma(1e308, 10.0, 0.0))


def test_mul_and_div_agree_with_numpy_complex_to_a_few_ulp():
    # a sanity check of the restatement only: numpy's complex product / quotient use other formulas, so parts agree to a few ulp of |z|
    rng = np.random.default_rng(7)
    ar, ai, br, bi = rng.standard_normal((4, 4096))
    a, b = ar + 1j * ai, br + 1j * bi
    for op, want in (("mul", a * b), ("div", a / b)):
        gr, gi = ref.binary(op, "cc", ar, ai, br, bi)
        err = np.abs((gr + 1j * gi) - want) / np.abs(want)
        assert err.max() <= 4 * EPS, (op, err.max() / EPS)
    gr, gi = ref.binary("div", "cr", ar, ai, br, None)
    assert np.max(np.abs((gr + 1j * gi) - a / br) / np.abs(a / br)) <= 4 * EPS
    gr, gi = ref.binary("div", "rc", ar, None, br, bi)
    assert np.max(np.abs((gr + 1j * gi) - ar / b) / np.abs(ar / b)) <= 4 * EPS


def test_signed_zero_rules_of_the_mixed_forms():
    z = np.array([0.0])
    assert ref.same_bits(ref.scalar("rsub", [1.0], z, 1.0)[1], [-0.0])      # s - z negates the imaginary part: +0 -> -0
    assert ref.same_bits(ref.scalar("sub", [1.0], z, 1.0)[1], [0.0])        # z - s keeps it
    assert ref.same_bits(ref.scalar("add", [1.0], [-0.0], 1.0)[1], [-0.0])  # z + s keeps it: no + 0.0
    r, i = ref.scalar("div", [1.0], [2.0], 0.0)                             # z / 0: (1*0 + 2*0) / 0 = NaN in both parts
    assert np.isnan(r[0]) and np.isnan(i[0])
    r, i = ref.scalar("rdiv", [1.0], [2.0], 0.0)                            # 0 / z: (0*1 + 0*2) / 5, (0*1 - 0*2) / 5
    assert ref.same_bits(r, [0.0]) and ref.same_bits(i, [0.0])


def test_tolerance_inputs_keep_the_tan_denominator_away_from_zero():
    re, im = ref.tolerance_inputs("tan")
    assert np.min(np.abs(ref.tan_denominator(re, im))) >= 0.25
    re, im = ref.tolerance_inputs("sinc")
    assert np.all(im != 0.0)


def test_entry_points_are_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    arity = {"rmhip_complex_unary": 4, "rmhip_complex_binary": 5, "rmhip_complex_scalar": 5}
    for name, n in arity.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
    assert _lib.SIGNATURES["rmhip_complex_unary"] == _lib.SIGNATURES["rmhip_unary"]
    assert _lib.SIGNATURES["rmhip_complex_binary"] == _lib.SIGNATURES["rmhip_binary"]
    assert _lib.SIGNATURES["rmhip_complex_scalar"] == _lib.SIGNATURES["rmhip_scalar"]
    assert _lib.SERVES["rmhip_complex_unary"] == ("unary_abs", "unary_angle", "unary_real", "unary_imag", "unary_conj", "unary_sign", "unary_sin",
                                                  "unary_cos", "unary_tan", "unary_sinh", "unary_cosh", "unary_sinc")
    assert _lib.SERVES["rmhip_complex_binary"] == ("elem_add", "elem_sub", "elem_mul", "elem_div")
    assert _lib.SERVES["rmhip_complex_scalar"] == ("scalar_add", "scalar_sub", "scalar_mul", "scalar_div", "scalar_rsub", "scalar_rdiv")
    ops = _lib.ENUMS["rmhip_complex_unary_op"]
    assert [k for k, _ in sorted(ops.items(), key=lambda kv: kv[1])] == [
        "RMHIP_CABS", "RMHIP_CANGLE", "RMHIP_CREAL", "RMHIP_CIMAG", "RMHIP_CCONJ", "RMHIP_CSIGN", "RMHIP_CSIN", "RMHIP_CCOS", "RMHIP_CTAN",
        "RMHIP_CSINH", "RMHIP_CCOSH", "RMHIP_CSINC", "RMHIP_COMPLEX_UNARY_OP_COUNT"]
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    for method in ("complex_unary", "complex_binary", "complex_scalar"):
        assert callable(getattr(HipProvider, method, None)), method


def test_complex_kernels_fit_the_register_budget():
    """1024-thread blocks are four waves per SIMD: at most 128 VGPRs, and a streaming kernel must not touch scratch (the libm bodies of
    sin / cos / tan / sinh / cosh / sinc are the large ones)."""
    res = _resources("complex_ew.hip")
    for needle in ("k_cx_binary_tile", "k_cx_binary_pair", "k_cx_bcast", "k_cx_unaryI", "k_cx_unary_real"):
        for name, r in _pick(res, needle).items():
            assert r["vgpr"] + r["agpr"] <= 128 and r["scratch"] == 0 and r["occupancy"] >= 4, (name, r)
    assert len(_pick(res, "k_cx_unaryI")) == 8 and len(_pick(res, "k_cx_unary_real")) == 8  # every op, real results in f64 and f32 storage
