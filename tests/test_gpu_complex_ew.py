"""GPU checks of the complex elementwise entry points (rmhip_complex_unary / _binary / _scalar, complex_ew.hip) against the numpy
restatement of the CPU builtins' rules (tests/complex_ew_ref.py).

Bit-exact family (add, sub, mul, div over complex o complex / complex o real / real o complex, the six scalar forms, conj, real, imag,
sign): equal bits, NaN positions and signs of zero included.  Tolerance family (abs, angle, sin, cos, tan, sinh, cosh, sinc): each part
within a first-order bound computed here from the formula - every libm call contributes the ulp figure tests/test_gpu_parity.py holds for
it, every arithmetic step half an ulp, with the condition factors (1 / |d| of tan and sinc) the formula carries - of the same formula
evaluated in np.longdouble."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_ew_ref as ref  # noqa: E402
from test_gpu_parity import BINARY_LIBM_ULP, LIBM_ULP  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
U = EPS / 2  # one correctly rounded operation
ERR_UNSUPPORTED, ERR_SHAPE, ERR_NOT_FOUND = 2, 3, 5
SIZES = (1, 2, 3, 255, 256, 257, 4097, 2 ** 20 + 3)  # the last exceeds one grid-stride pass; odd sizes take the pair layout's tail
SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1.7e308])
KINDS = ("cc", "cr", "rc")


def up(prov, x, shape=None):
    x = np.asarray(x, dtype=np.float64)
    return prov.upload(x.ravel(order="F"), shape if shape is not None else (x.shape if x.ndim >= 2 else (x.size, 1)))


def up_c(prov, re, im, shape=None):
    hr, hi = up(prov, re, shape), up(prov, im, shape)
    z = prov.complex_from_real_imag(hr, hi)
    prov.free(hr)
    prov.free(hi)
    return z


def parts(prov, h):
    z = prov.download(h)
    return z.real.copy(), z.imag.copy()


def live(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def free_all(prov, *hs):
    for h in hs:
        prov.free(h)


def check_bits(prov, h, want, what):
    assert prov.is_complex(h), what
    gr, gi = parts(prov, h)
    assert ref.same_bits(gr, want[0]) and ref.same_bits(gi, want[1]), what
    prov.free(h)


def run_bit_exact(prov, ar, ai, br, bi, scalars, what):
    """Every bit-exact op on one set of same-shape operands: binary over the three kinds, the scalar forms, conj / real / imag / sign."""
    za, zb, ra, rb = up_c(prov, ar, ai), up_c(prov, br, bi), up(prov, ar), up(prov, br)
    for op in ref.BINARY:
        check_bits(prov, prov.complex_binary(op, za, zb), ref.binary(op, "cc", ar, ai, br, bi), (what, op, "cc"))
        check_bits(prov, prov.complex_binary(op, za, rb), ref.binary(op, "cr", ar, ai, br, None), (what, op, "cr"))
        check_bits(prov, prov.complex_binary(op, ra, zb), ref.binary(op, "rc", ar, None, br, bi), (what, op, "rc"))
    for op in ref.SCALAR:
        for s in scalars:
            check_bits(prov, prov.complex_scalar(op, za, s), ref.scalar(op, ar, ai, s), (what, op, s))
    for op in ("conj", "sign"):
        check_bits(prov, prov.complex_unary(op, za), ref.unary(op, ar, ai), (what, op))
    for op in ("real", "imag"):
        h = prov.complex_unary(op, za)
        assert not prov.is_complex(h) and prov.buffer_bits(h) == 64 and h.shape == za.shape
        assert ref.same_bits(prov.download(h), ref.unary(op, ar, ai)), (what, op)
        prov.free(h)
    free_all(prov, za, zb, ra, rb)


@pytest.mark.parametrize("n", SIZES)
def test_bit_exact_family_on_random_data(prov, n):
    ar, ai, br, bi = np.random.default_rng(n).standard_normal((4, n))
    run_bit_exact(prov, ar, ai, br, bi, (0.75,), n)


def test_bit_exact_family_on_special_values(prov):
    ar, ai, br, bi = (g.ravel() for g in np.meshgrid(SPECIAL, SPECIAL, SPECIAL, SPECIAL, indexing="ij"))  # 9^4 rows
    run_bit_exact(prov, ar, ai, br, bi, (), "special")
    zr, zi = (g.ravel() for g in np.meshgrid(SPECIAL, SPECIAL, indexing="ij"))
    z = up_c(prov, zr, zi)
    for op in ref.SCALAR:
        for s in SPECIAL:
            check_bits(prov, prov.complex_scalar(op, z, float(s)), ref.scalar(op, zr, zi, float(s)), ("special", op, s))
    prov.free(z)


def test_named_special_rows(prov):
    z = up_c(prov, [1.0, 1.0, 0.0, np.inf, np.nan, -np.inf], [0.0, 2.0, 0.0, np.nan, np.inf, 3.0])
    gr, gi = parts(prov, prov.complex_scalar("rsub", z, 1.0))      # s - z with bi = +0: the imaginary part is -0
    assert ref.same_bits(gr[:1], [0.0]) and ref.same_bits(gi[:1], [-0.0])
    gr, gi = parts(prov, prov.complex_scalar("div", z, 0.0))       # z / 0: 0 / 0 in both parts
    assert np.isnan(gr[1]) and np.isnan(gi[1])
    gr, gi = parts(prov, prov.complex_scalar("rdiv", z, 0.0))      # 0 / z: (0 + 0) / 5, (0 - 0) / 5
    assert ref.same_bits(gr[1:2], [0.0]) and ref.same_bits(gi[1:2], [0.0])
    assert np.isnan(gr[2]) and np.isnan(gi[2])                     # 0 / 0
    gr, gi = parts(prov, prov.complex_unary("sign", z))
    keep = [0, 2, 3, 4, 5]                                         # (row 1 is a general value: the random and table tests hold its bits)
    assert ref.same_bits(gr[keep], [1.0, 0.0, np.nan, np.nan, -1.0])   # inf beside NaN: NaN + NaN i; -inf + 3i: -1 + 0i
    assert ref.same_bits(gi[keep], [0.0, 0.0, np.nan, np.nan, 0.0])


# ---- broadcasting ------------------------------------------------------------------------------------------------------------------------
def _operand(prov, rng, shape, cplx):
    re, im = rng.standard_normal(shape), rng.standard_normal(shape)
    flat = lambda v: v.ravel(order="F")
    if cplx:
        return up_c(prov, flat(re), flat(im), shape), re, im
    return up(prov, flat(re), shape), re, None


BCAST = [((5, 1), True, (1, 7), True), ((5, 1), True, (1, 7), False), ((5, 1), False, (1, 7), True),
         ((1, 1), True, (4, 3), False), ((4, 3), False, (1, 1), True), ((1, 1), True, (4, 3), True), ((4, 3), True, (1, 1), False),
         ((3, 1, 4), True, (1, 5, 1), True), ((3, 1, 4), False, (1, 5, 1), True), ((3, 1, 4), True, (1, 5, 1), False),
         ((300, 1), True, (1, 3), True), ((1, 1), True, (1, 1), False), ((700, 2), True, (700, 1), False)]


@pytest.mark.parametrize("sa,ca,sb,cb", BCAST)
def test_broadcast_shapes_and_bits(prov, sa, ca, sb, cb):
    rng = np.random.default_rng(len(sa) * 100 + sa[0] + 7 * cb + ca)
    ha, ar, ai = _operand(prov, rng, sa, ca)
    hb, br, bi = _operand(prov, rng, sb, cb)
    kind = "cc" if ca and cb else ("cr" if ca else "rc")
    oshape = np.broadcast_shapes(sa, sb)
    bc = lambda v: None if v is None else np.broadcast_to(v, oshape).ravel(order="F")  # the index plan: numpy front-pads like broadcast.rs
    for op in ref.BINARY:
        h = prov.complex_binary(op, ha, hb)
        assert tuple(h.shape) == tuple(oshape), (op, h.shape)
        check_bits(prov, h, ref.binary(op, kind, bc(ar), bc(ai), bc(br), bc(bi)), (sa, sb, kind, op))
    free_all(prov, ha, hb)


def test_broadcast_refusals_and_empty_results(prov):
    from runmat_amd import ProviderError

    rng = np.random.default_rng(2)
    z23, _, _ = _operand(prov, rng, (2, 3), True)
    v3 = prov.upload(np.ones(3))                       # a length-3 vector as the mirror holds it: the column [3, 1]
    before = live(prov)
    with pytest.raises(ProviderError) as e:
        prov.complex_binary("add", z23, v3)
    assert e.value.code == ERR_SHAPE and str(e.value) == "size mismatch between inputs (dimension 1 has lengths 2 and 3)" and live(prov) == before
    with pytest.raises(ProviderError) as e2:           # the message rmhip_binary gives
        prov.elem_add(prov.complex_unary("real", z23), v3)
    assert str(e2.value) == str(e.value)
    # (an explicit rank-1 shape [3] is front-padded to [1, 3] - broadcast.rs aligns trailing dimensions - and conforms, as in rmhip_binary)
    row3 = up(prov, np.ones(3), (3,))
    h, hr = prov.complex_binary("add", z23, row3), prov.elem_add(prov.complex_unary("real", z23), row3)
    assert tuple(h.shape) == tuple(hr.shape) == (2, 3)
    # nine dimensions, broadcast in alternation: nothing collapses
    sa, sb = (2, 1) * 4 + (2,), (1, 2) * 4 + (1,)
    z9, _, _ = _operand(prov, rng, sa, True)
    r9, _, _ = _operand(prov, rng, sb, False)
    before = live(prov)
    with pytest.raises(ProviderError) as e:
        prov.complex_binary("mul", z9, r9)
    assert e.value.code == ERR_UNSUPPORTED and live(prov) == before
    # [0, 3] o [1, 3]: an empty complex tensor
    z0 = up_c(prov, np.zeros(0), np.zeros(0), (0, 3))
    r13 = up(prov, np.ones(3), (1, 3))
    for a, b in ((z0, r13), (r13, z0)):
        h = prov.complex_binary("div", a, b)
        assert tuple(h.shape) == (0, 3) and prov.is_complex(h) and prov.download(h).size == 0
        prov.free(h)
    for op in ("abs", "sin"):
        h = prov.complex_unary(op, z0)
        assert tuple(h.shape) == (0, 3) and prov.is_complex(h) == (op == "sin")
        prov.free(h)
    h = prov.complex_scalar("rdiv", z0, 2.0)
    assert tuple(h.shape) == (0, 3) and prov.is_complex(h)


# ---- tolerance family --------------------------------------------------------------------------------------------------------------------
def _L(name):
    return LIBM_ULP[name] * EPS


def bounds(op, re, im):
    """First-order absolute error bound of each part: a libm call is within its ulp figure (relative L), a rounded operation within U."""
    W = np.longdouble
    x, y = re.astype(W), im.astype(W)
    a = np.abs
    if op in ("abs", "angle"):
        return (BINARY_LIBM_ULP * EPS * a(ref.unary_wide(op, re, im)),)
    if op == "sin":
        return a(np.sin(x) * np.cosh(y)) * (_L("sin") + _L("cosh") + U), a(np.cos(x) * np.sinh(y)) * (_L("cos") + _L("sinh") + U)
    if op == "cos":
        return a(np.cos(x) * np.cosh(y)) * (_L("cos") + _L("cosh") + U), a(np.sin(x) * np.sinh(y)) * (_L("sin") + _L("sinh") + U)
    if op == "sinh":
        return a(np.sinh(x) * np.cos(y)) * (_L("sinh") + _L("cos") + U), a(np.cosh(x) * np.sin(y)) * (_L("cosh") + _L("sin") + U)
    if op == "cosh":
        return a(np.cosh(x) * np.cos(y)) * (_L("cosh") + _L("cos") + U), a(np.sinh(x) * np.sin(y)) * (_L("sinh") + _L("sin") + U)
    if op == "tan":
        ic = 1 / np.cosh(2 * y)
        e_ic = _L("cosh") + U                                    # 1 / cosh(2 im): the call and the division (2 * im is exact)
        p = np.cos(2 * x) * ic
        d = 1 + p
        rel_d = (a(p) * (_L("cos") + e_ic + U) + U * a(d)) / a(d)  # the product's error and the sum's rounding, over |d|
        wr, wi = np.sin(2 * x) * ic / d, np.tanh(2 * y) / d
        return a(wr) * (_L("sin") + e_ic + U + rel_d + U), a(wi) * (_L("tanh") + rel_d + U)
    if op == "sinc":
        sr, si = (v.astype(W) for v in ref.sinc_scaled(re, im))
        nr, ni = np.sin(sr) * np.cosh(si), np.cos(sr) * np.sinh(si)
        e_nr, e_ni = _L("sin") + _L("cosh") + U, _L("cos") + _L("sinh") + U
        d = sr * sr + si * si
        rel_d = 2 * U                                            # si * si rounded, then one fused rounding of a sum of positive terms
        A, B = nr * sr + ni * si, ni * sr - nr * si
        err_a = a(nr * sr) * (e_nr + U) + a(ni * si) * (e_ni + U) + U * a(A)
        err_b = a(ni * sr) * (e_ni + U) + a(nr * si) * (e_nr + U) + U * a(B)
        return err_a / d + a(A / d) * (rel_d + U), err_b / d + a(B / d) * (rel_d + U)
    raise ValueError(op)


@pytest.mark.parametrize("op", ref.TOLERANCE_UNARY)
def test_tolerance_family(prov, op):
    assert ref.longdouble_is_wide()
    re, im = ref.tolerance_inputs(op)
    if op == "tan":
        assert np.min(np.abs(ref.tan_denominator(re, im))) >= 0.25  # by construction (complex_ew_ref.tolerance_inputs): nothing is filtered
    z = up_c(prov, re, im)
    h = prov.complex_unary(op, z)
    wide = ref.unary_wide(op, re, im)
    if op in ref.UNARY_REAL:
        assert not prov.is_complex(h)
        got, wide = (prov.download(h),), (wide,)
    else:
        assert prov.is_complex(h)
        got = parts(prov, h)
    worst = 0.0
    for g, w, b in zip(got, wide, bounds(op, re, im)):
        assert np.all(np.isfinite(g))
        ratio = np.abs(g.astype(np.longdouble) - w) / (b + np.longdouble(1e-320))
        worst = max(worst, float(np.max(ratio)))
    print(f"complex {op}: largest error / bound = {worst:.3f}")
    assert worst <= 1.0, (op, worst)
    free_all(prov, z, h)


def test_tolerance_family_edge_rows(prov):
    z = up_c(prov, [np.inf, np.nan, 0.0, -0.0, 0.0, -0.0], [np.nan, -np.inf, 0.0, 0.0, -0.0, -0.0])
    assert ref.same_bits(prov.download(prov.complex_unary("abs", z))[:2], [np.inf, np.inf])          # an infinite part beside a NaN part
    assert ref.same_bits(prov.download(prov.complex_unary("angle", z))[2:], [0.0, math.pi, -0.0, -math.pi])  # atan2(+-0, +-0)
    k = up_c(prov, [0.0, 1.0, -3.0, 2.0 ** 40, 0.5], [0.0, 0.0, -0.0, 0.0, 0.0])
    gr, gi = parts(prov, prov.complex_unary("sinc", k))
    assert ref.same_bits(gr[:4], [1.0, 0.0, 0.0, 0.0]) and ref.same_bits(gi, np.zeros(5))            # sinc(0) = 1, sinc(k) = 0, real axis: im = +0
    assert abs(gr[4] - 2.0 / math.pi) <= 4 * EPS


# ---- storage kinds, refusals, precision 32 -------------------------------------------------------------------------------------------------
def test_storage_kind_of_every_result(prov):
    z = up_c(prov, [1.0, -2.0, 0.5], [0.25, 3.0, -1.0])
    r = up(prov, [2.0, 4.0, 8.0])
    for op in ref.UNARY_REAL:
        h = prov.complex_unary(op, z)
        assert not prov.is_complex(h) and prov.buffer_bits(h) == 64 and prov.logical_isreal(h) is True and tuple(h.shape) == (3, 1), op
    for op in ref.UNARY_COMPLEX:
        h = prov.complex_unary(op, z)
        assert prov.is_complex(h) and prov.logical_isreal(h) is False and tuple(h.shape) == (3, 1), op
    for op in ref.BINARY:
        for a, b in ((z, z), (z, r), (r, z)):
            assert prov.is_complex(prov.complex_binary(op, a, b)), op
    for op in ref.SCALAR:
        assert prov.is_complex(prov.complex_scalar(op, z, 2.0)), op


def test_refusals_leave_nothing_behind(prov):
    from runmat_amd import ProviderError, _lib

    z = up_c(prov, [1.0, 2.0], [3.0, 4.0])
    r = up(prov, [1.0, 2.0])
    gone = up_c(prov, [1.0], [1.0])
    prov.free(gone)
    before = live(prov)

    def refused(code, f):
        with pytest.raises(ProviderError) as e:
            f()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert live(prov) == before

    refused(ERR_UNSUPPORTED, lambda: prov.complex_binary("add", r, r))       # only real operands: rmhip_binary serves those
    refused(ERR_UNSUPPORTED, lambda: prov.complex_unary("abs", r))
    refused(ERR_UNSUPPORTED, lambda: prov.complex_scalar("add", r, 1.0))
    binary_codes = _lib.ENUMS["rmhip_binary_op"]
    for name, code in binary_codes.items():
        if name not in ("RMHIP_ADD", "RMHIP_SUB", "RMHIP_MUL", "RMHIP_DIV"):  # pow, max, min, hypot, atan2, mod, rem, comparisons, logicals, the count
            refused(ERR_UNSUPPORTED, lambda code=code: prov.complex_binary(code, z, z))
    for code in (-1, _lib.ENUMS["rmhip_scalar_op"]["RMHIP_SMAX"], _lib.ENUMS["rmhip_scalar_op"]["RMHIP_SMIN"], _lib.ENUMS["rmhip_scalar_op"]["RMHIP_SCALAR_OP_COUNT"]):
        refused(ERR_UNSUPPORTED, lambda code=code: prov.complex_scalar(code, z, 1.0))
    for code in (-1, _lib.ENUMS["rmhip_complex_unary_op"]["RMHIP_COMPLEX_UNARY_OP_COUNT"]):
        refused(ERR_UNSUPPORTED, lambda code=code: prov.complex_unary(code, z))
    refused(ERR_UNSUPPORTED, lambda: prov.complex_binary(-1, z, z))
    refused(ERR_NOT_FOUND, lambda: prov.complex_unary("abs", gone))
    refused(ERR_NOT_FOUND, lambda: prov.complex_binary("add", z, gone))
    refused(ERR_NOT_FOUND, lambda: prov.complex_binary("add", gone, r))
    refused(ERR_NOT_FOUND, lambda: prov.complex_scalar("mul", gone, 2.0))


def test_old_entry_points_still_refuse_complex_storage(prov):
    """The dispatch rule lives in the caller (the Rust shim chooses by handle_storage): rmhip_unary / rmhip_binary / rmhip_scalar keep
    refusing complex operands, so changing that is a deliberate change of this test."""
    from runmat_amd import ProviderError

    z = up_c(prov, [1.0, 2.0], [3.0, 4.0])
    r = up(prov, [1.0, 2.0])
    for f in (lambda: prov.unary_sin(z), lambda: prov.unary_abs(z), lambda: prov.elem_add(z, r), lambda: prov.elem_add(r, z), lambda: prov.elem_mul(z, z),
              lambda: prov.scalar_add(z, 1.0), lambda: prov.scalar_rdiv(z, 1.0), lambda: prov.unary_real(z)):
        with pytest.raises(ProviderError) as e:
            f()
        assert e.value.code == ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, "F32")
    yield p
    p.close()


def f32r(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def test_precision_32_rounds_each_result_once(prov32, prov):
    rng = np.random.default_rng(32)
    ar, ai, br, bi = f32r(rng.standard_normal((4, 1001)))  # f32-representable inputs: both providers hold the same values
    res = {}
    for p in (prov, prov32):
        za, zb, rb = up_c(p, ar, ai), up_c(p, br, bi), up(p, br)
        mul, div, mixed, ab = p.complex_binary("mul", za, zb), p.complex_binary("div", za, zb), p.complex_binary("div", za, rb), p.complex_unary("abs", za)
        assert p.is_complex(mul) and p.is_complex(div) and p.is_complex(mixed) and not p.is_complex(ab)
        assert p.buffer_bits(ab) == (32 if p is prov32 else 64)
        res[p] = (*parts(p, mul), *parts(p, div), *parts(p, mixed), p.download(ab))
    for g32, g64 in zip(res[prov32], res[prov]):
        assert ref.same_bits(g32, f32r(g64))
    assert not ref.same_bits(res[prov][0], f32r(res[prov][0]))  # (the f64 products are not f32 values: the rounding is observable)


# ---- a pipeline that stays on the device -----------------------------------------------------------------------------------------------------
def test_circular_convolution_stays_resident(prov):
    n = 64
    rng = np.random.default_rng(64)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    ha, hb = up(prov, a), up(prov, b)
    downloaded = prov.telemetry_snapshot()["download_bytes"]
    fa, fb = prov.fft_dim(ha, None, 0), prov.fft_dim(hb, None, 0)
    prod = prov.complex_binary("mul", fa, fb)
    back = prov.ifft_dim(prod, None, 0)
    out = prov.fft_extract_real(back)
    assert prov.is_complex(prod) and prov.is_complex(back) and not prov.is_complex(out)
    assert prov.telemetry_snapshot()["download_bytes"] == downloaded      # nothing came back between the uploads and the final read
    got = prov.download(out)
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    want = np.array([sum(al[j] * bl[(k - j) % n] for j in range(n)) for k in range(n)], dtype=np.longdouble)
    # the transform tolerance of tests/test_gpu_fft.py (4 eps log2(n) ||line||_2 per point, before the inverse's 1 / n), carried through the
    # product: |dP_k| <= |A_k| lim_b + |B_k| lim_a + lim_a lim_b + 4 eps |P_k|, the inverse averages it and adds its own share for P
    FA, FB = np.fft.fft(a), np.fft.fft(b)
    lim_a, lim_b = (4 * EPS * math.log2(n) * np.linalg.norm(v) for v in (a, b))
    dP = np.abs(FA) * lim_b + np.abs(FB) * lim_a + lim_a * lim_b + 4 * EPS * np.abs(FA * FB)
    lim = np.mean(dP) + 4 * EPS * math.log2(n) * np.linalg.norm(FA * FB) / n
    err = float(np.max(np.abs(got.astype(np.longdouble) - want)))
    print(f"circular convolution: error / bound = {err / lim:.3f}")
    assert err <= lim
