"""GPU checks of `pagefun(@mtimes)` with a complex operand (rmhip_complex_pagefun; runmat_amd/csrc/complex_pagefun.hip) against the numpy
restatement of the host builtin's three loops (tests/complex_pagefun_ref.py): small pages bit-exact, the matrix-core tier within the
derived gate (2k eps sum|a||b| per part, k eps for the mixed kinds) and bit-exact on Gaussian integers, the tier and the operand kind
read from the launch log on both sides of the boundary."""
import numpy as np
import pytest

import complex_pagefun_ref as ref
from pagefun_host import build_request
from runmat_amd import HipProvider, PagefunOp, PagefunRequest, ProviderError
from runmat_amd import _lib

pytestmark = pytest.mark.gpu

KIND_IDS = {0: "cc", 1: "cr", 2: "rc"}
kinds = pytest.mark.parametrize("kind", ref.KINDS, ids=lambda k: KIND_IDS[k])


def request(handles, lhs_shape, rhs_shape):
    r = build_request(lhs_shape, rhs_shape)
    return PagefunRequest(PagefunOp.Mtimes, list(handles), r.output_shape, r.page_dims, r.input_page_dims)


def last_launch(prov):
    log = [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "complex_pagefun"]
    return log[-1]


def up(prov, re, im=None):
    """A real tensor, or the complex-interleaved one of the two parts."""
    hr = prov.upload(re.ravel(order="F"), re.shape)
    if im is None:
        return hr
    hi = prov.upload(im.ravel(order="F"), im.shape)
    z = prov.complex_from_real_imag(hr, hi)
    prov.free(hr)
    prov.free(hi)
    return z


def parts(prov, h):
    z = prov.download(h).reshape(h.shape, order="F")
    return np.asfortranarray(z.real), np.asfortranarray(z.imag)


def run(prov, Ar, Ai, Br, Bi):
    """-> (Cr, Ci, tier or None for an empty result); the launch's operand kind and the result's storage are checked on the way."""
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    hc = prov.complex_pagefun(request([ha, hb], Ar.shape, Br.shape))
    assert list(hc.shape) == build_request(Ar.shape, Br.shape).output_shape and prov.is_complex(hc)
    tier = None
    if np.prod(hc.shape):
        e = last_launch(prov)
        tier = e["tuning"]["tier"]
        assert e["tuning"]["kind"] == ref.kind_of(Ai, Bi)
    Cr, Ci = parts(prov, hc)
    for h in (ha, hb, hc):
        prov.free(h)
    return Cr, Ci, tier


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_bitwise(got, want):
    """Bit for bit; a NaN matches any NaN (the host's and the device's default NaNs may differ in sign and payload)."""
    for g, w in zip(got, want):
        assert g.shape == w.shape
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn)
        assert np.array_equal(bits(g)[~gn], bits(w)[~wn])


def assert_gate(got, args, want, extra=0.0):
    """`extra`: a further relative allowance on the same sums of |a||b| (the one f32 rounding of a precision-32 result)."""
    g, s = ref.gate(*args), ref.magnitude(*args)
    for part, (x, w) in enumerate(zip(got, want)):
        assert x.shape == w.shape
        excess = np.abs(x - w) - (g[part] + extra * s[part])
        assert np.all(excess <= 0), (part, np.max(excess))


# ---- small tier: bit-exact -----------------------------------------------------------------------------------------------------------
@kinds
def test_small_sweep_bitwise(prov, kind):
    rng = np.random.default_rng(100 + kind)
    sides = (1, 2, 5, 16, 31, 32)
    for m in sides:
        for n in sides:
            for k in sides:
                args = ref.operands(rng, kind, (m, k, 3), (k, n, 3))
                Cr, Ci, tier = run(prov, *args)
                assert tier == 2, (m, n, k)
                assert_bitwise((Cr, Ci), ref.cpagefun_host(*args))


def special_pages(rng, kind):
    """Six 5x4 by 4x3 pages: all -0.0 products, zeros against -1, a NaN, an Inf, a -Inf on the right, Inf * 0."""
    Ar, Ai, Br, Bi = ref.operands(rng, kind, (5, 4, 6), (4, 3, 6))
    a_parts = [x for x in (Ar, Ai) if x is not None]
    b_parts = [x for x in (Br, Bi) if x is not None]
    for x in a_parts:
        x[:, :, 0], x[:, :, 1] = -0.0, 0.0
    for x in b_parts:
        x[:, :, 0], x[:, :, 1] = 1.0, -1.0
    if Bi is not None:
        Bi[:, :, 0] = 0.0  # every product of page 0 is then a zero and every k-term -0.0 or +0.0
    a_parts[-1][1, 2, 2] = np.nan
    a_parts[0][0, 0, 3] = np.inf
    b_parts[-1][3, 1, 4] = -np.inf
    a_parts[-1][2, 1, 5], b_parts[0][1, 2, 5] = np.inf, 0.0
    return Ar, Ai, Br, Bi


@kinds
def test_small_special_values_bitwise(prov, kind):
    args = special_pages(np.random.default_rng(2), kind)
    Cr, Ci, tier = run(prov, *args)
    assert tier == 2
    want = ref.cpagefun_host(*args)
    assert not np.any(np.signbit(Cr[:, :, 0])) and not np.any(np.signbit(Ci[:, :, 0]))
    assert np.any(np.isnan(want[0]) | np.isnan(want[1])) and np.any(np.isinf(want[0])) and np.any(np.isinf(want[1]))
    assert_bitwise((Cr, Ci), want)


@pytest.mark.parametrize("m,n,k,tier", [(5, 3, 4, 2), (40, 36, 20, 3)])
def test_mixed_kinds_keep_an_inf_on_both_tiers(prov, m, n, k, tier):
    """complex x real (and its mirror) never multiplies by an implied zero: Inf stays Inf where the complex x complex form with a zero
    imaginary part gives NaN.  The real operand is positive, so no Inf meets a zero or an Inf of the other sign."""
    rng = np.random.default_rng(3)
    Zr, Zi = rng.standard_normal((m, k, 2)), rng.standard_normal((m, k, 2))
    Zr[1, 2, 0], Zi[m - 1, k - 1, 1] = np.inf, np.inf
    R = rng.uniform(0.5, 2.0, (k, n, 2))
    Cr, Ci, t = run(prov, Zr, Zi, R, None)
    assert t == tier
    assert np.all(Cr[1, :, 0] == np.inf) and np.all(Ci[m - 1, :, 1] == np.inf) and not np.any(np.isnan(Cr)) and not np.any(np.isnan(Ci))
    assert np.array_equal(np.isinf(Cr), np.isinf(ref.cpagefun_host(Zr, Zi, R, None)[0]))
    Cr0, Ci0, _ = run(prov, Zr, Zi, R, np.zeros_like(R))
    assert np.all(np.isnan(Ci0[1, :, 0])) and np.all(np.isnan(Cr0[m - 1, :, 1]))
    # the mirror image: real x complex, the operands transposed page by page
    Rt, Zrt, Zit = (np.ascontiguousarray(np.swapaxes(x, 0, 1)) for x in (R, Zr, Zi))
    Dr, Di, t = run(prov, Rt, None, Zrt, Zit)
    assert t == tier
    assert np.all(Dr[:, 1, 0] == np.inf) and np.all(Di[:, m - 1, 1] == np.inf) and not np.any(np.isnan(Dr)) and not np.any(np.isnan(Di))


# ---- boundaries and the matrix-core tier ---------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k,tier", [(32, 32, 32, 2), (33, 32, 32, 3), (32, 33, 32, 3), (32, 32, 33, 3)])
def test_tier_boundaries(prov, kind, m, n, k, tier):
    rng = np.random.default_rng(5)
    args = ref.operands(rng, kind, (m, k, 2), (k, n, 2), ints=True)
    Cr, Ci, t = run(prov, *args)
    assert t == tier
    assert_bitwise((Cr, Ci), ref.cpagefun_host(*args))


@kinds
@pytest.mark.parametrize("m,n,k,p", [(33, 33, 33, 5), (64, 64, 64, 3), (100, 40, 70, 3), (65, 130, 17, 2)])
def test_mfma_tier_gate_and_exact_integers(prov, kind, m, n, k, p):
    rng = np.random.default_rng(m * 7 + n)
    args = ref.operands(rng, kind, (m, k, p), (k, n, p))
    Cr, Ci, t = run(prov, *args)
    assert t == 3
    assert_gate((Cr, Ci), args, ref.cpagefun_host(*args))
    args = ref.operands(rng, kind, (m, k, p), (k, n, p), ints=True)
    Cr, Ci, t = run(prov, *args)
    assert t == 3
    assert_bitwise((Cr, Ci), ref.cpagefun_host(*args))


# ---- broadcasting and lazy real operands ---------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("lhs_pages,rhs_pages", [((5,), (5,)), ((1,), (5,)), ((5,), (1,)), ((3, 1), (1, 4)), ((2, 1, 3, 2), (1, 2, 3, 1))])
@pytest.mark.parametrize("m,n,k", [(4, 3, 5), (40, 36, 20)])
def test_broadcast_patterns(prov, kind, lhs_pages, rhs_pages, m, n, k):
    rng = np.random.default_rng(7)
    args = ref.operands(rng, kind, (m, k) + lhs_pages, (k, n) + rhs_pages)
    Cr, Ci, tier = run(prov, *args)
    want = ref.cpagefun_host(*args)
    if max(m, n, k) <= 32:
        assert tier == 2
        assert_bitwise((Cr, Ci), want)
    else:
        assert tier == 3
        assert_gate((Cr, Ci), args, want)


def test_repmat_transpose_and_lazy_normal_real_operands(prov):
    rng = np.random.default_rng(12)
    # real x complex, the real operand a repmat view: [3 x 4] tiled to [3, 4, 5]
    R = rng.standard_normal((3, 4))
    hr = prov.upload(R.ravel(order="F"), R.shape)
    hrv = prov.repmat(hr, [1, 1, 5])
    Qr, Qi = rng.standard_normal((4, 2, 5)), rng.standard_normal((4, 2, 5))
    hq = up(prov, Qr, Qi)
    he = prov.complex_pagefun(request([hrv, hq], [3, 4, 5], Qr.shape))
    assert last_launch(prov)["tuning"]["kind"] == 2 and last_launch(prov)["tuning"]["tier"] == 2
    assert_bitwise(parts(prov, he), ref.cpagefun_host(np.repeat(R[:, :, None], 5, axis=2), None, Qr, Qi))
    # complex x real, the real operand a transpose view shared by every page, on the matrix-core tier
    Bt = rng.standard_normal((36, 20))  # B = Bt' is 20 x 36
    hbt = prov.upload(Bt.ravel(order="F"), Bt.shape)
    hbv = prov.transpose(hbt)
    Pr, Pi = rng.standard_normal((40, 20, 3)), rng.standard_normal((40, 20, 3))
    hp = up(prov, Pr, Pi)
    hd = prov.complex_pagefun(request([hp, hbv], Pr.shape, [20, 36]))
    assert last_launch(prov)["tuning"]["kind"] == 1 and last_launch(prov)["tuning"]["tier"] == 3
    args = (Pr, Pi, Bt.T.copy(), None)
    assert_gate(parts(prov, hd), args, ref.cpagefun_host(*args))
    # a lazy random_normal real operand is settled first; its handle then holds the values the product used
    hn = prov.random_normal([4, 3, 100])
    Mr, Mi = rng.standard_normal((3, 5, 100)), rng.standard_normal((3, 5, 100))
    hm = up(prov, Mr, Mi)
    hf = prov.complex_pagefun(request([hn, hm], [4, 3, 100], Mr.shape))
    N = prov.download(hn).reshape((4, 3, 100), order="F")
    assert_bitwise(parts(prov, hf), ref.cpagefun_host(N, None, Mr, Mi))
    for h in (hr, hrv, hq, he, hbt, hbv, hp, hd, hn, hm, hf):
        prov.free(h)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
@kinds
def test_more_than_65535_small_pages(prov, kind):
    rng = np.random.default_rng(8)
    args = ref.operands(rng, kind, (2, 2, 70000), (2, 2, 70000))
    Cr, Ci, tier = run(prov, *args)
    assert tier == 2
    assert_bitwise((Cr, Ci), ref.cpagefun_host(*args))


def test_more_than_65535_mfma_pages(prov):
    rng = np.random.default_rng(9)
    args = ref.operands(rng, 0, (33, 2, 70000), (2, 33, 70000), ints=True)
    Cr, Ci, tier = run(prov, *args)
    assert tier == 3
    want = ref.cpagefun_host(*args)
    assert_bitwise((Cr, Ci), want)


@kinds
def test_empties_and_k_zero(prov, kind):
    for lhs, rhs in [((2, 2, 0), (2, 2, 0)), ((0, 3, 4), (3, 2, 4)), ((3, 2, 4), (2, 0, 4)), ((2, 2, 0), (2, 2, 5)), ((2, 2, 3, 0), (2, 2))]:
        Ar, Br = np.zeros(lhs), np.zeros(rhs)
        Cr, Ci, _ = run(prov, Ar, Ar.copy() if kind != 2 else None, Br, Br.copy() if kind != 1 else None)
        assert list(Cr.shape) == build_request(lhs, rhs).output_shape and Cr.size == 0 and Ci.size == 0
    rng = np.random.default_rng(10)
    for lhs, rhs in [((3, 0, 4), (0, 5, 4)), ((40, 0, 2), (0, 300, 2)), ((3, 0), (0, 5, 6))]:
        args = ref.operands(rng, kind, lhs, rhs)
        Cr, Ci, _ = run(prov, *args)
        assert list(Cr.shape) == build_request(lhs, rhs).output_shape and Cr.size
        for x in (Cr, Ci):
            assert np.all(x == 0.0) and not np.any(np.signbit(x))


# ---- refusals and the result's kind --------------------------------------------------------------------------------------------------
def test_refusals(prov):
    rng = np.random.default_rng(11)
    A, B = rng.standard_normal((3, 4, 2)), rng.standard_normal((4, 5, 2))
    ha, hb = up(prov, A, A), up(prov, B)  # complex x real
    hra = up(prov, A)
    hb3 = up(prov, rng.standard_normal((4, 5, 3)))
    la, lb = (2, 1) * 4 + (2,), (1, 2) * 4 + (1,)  # nine page dimensions that do not collapse: the operands alternate in broadcasting
    h9a, h9b = up(prov, np.ones((1, 1) + la), np.ones((1, 1) + la)), up(prov, np.ones((1, 1) + lb))
    live = prov.telemetry_snapshot()["bytes_allocated"]

    def code(req, call=None):
        with pytest.raises(ProviderError) as e:
            (call or prov.complex_pagefun)(req)
        return e.value.code

    ok = request([ha, hb], A.shape, B.shape)
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha], [3, 4, 2], [2], [[2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb, hb], ok.output_shape, [2], [[2], [2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], ok.output_shape, [2], [[2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [hb, ha], [4, 4, 2], [2], [[2], [2]])) == _lib.ERR_SHAPE  # 4x5 * 3x4
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb3], [3, 5, 3], [3], [[2], [3]])) == _lib.ERR_SHAPE
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 3], [2], [[2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5], [2], [[2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 3], [3], [[3], [3]])) == _lib.ERR_INVALID  # 24 logical elements, not 36
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 2], [1], [[2], [2]])) == _lib.ERR_INVALID  # page_dims disagree
    assert code(PagefunRequest("mrdivide", [ha, hb], ok.output_shape, ok.page_dims, ok.input_page_dims)) == _lib.ERR_UNSUPPORTED
    # an op the library does not know, past the Python mirror's own check
    import ctypes as C
    ids = (C.c_uint64 * 2)(ha.buffer_id, hb.buffer_id)
    pd, ipd, osh, out = (C.c_size_t * 1)(2), (C.c_size_t * 2)(2, 2), (C.c_size_t * 3)(3, 5, 2), C.c_uint64(7)
    assert prov._lib.rmhip_complex_pagefun(prov._ctx, 99, ids, 2, pd, 1, ipd, osh, 3, C.byref(out)) == _lib.ERR_UNSUPPORTED and out.value == 0
    assert code(request([h9a, h9b], (1, 1) + la, (1, 1) + lb)) == _lib.ERR_UNSUPPORTED
    # two real operands are the real entry point's, a complex one is not
    with pytest.raises(ProviderError) as e:
        prov.complex_pagefun(request([hra, hb], A.shape, B.shape))
    assert e.value.code == _lib.ERR_UNSUPPORTED and "rmhip_pagefun" in str(e.value)
    assert code(ok, prov.pagefun) == _lib.ERR_UNSUPPORTED
    assert prov.telemetry_snapshot()["bytes_allocated"] == live  # a refused call allocates nothing: no result is left behind
    for h in (ha, hb, hra, hb3, h9a, h9b):
        prov.free(h)


def test_result_is_complex_interleaved(prov):
    rng = np.random.default_rng(15)
    args = ref.operands(rng, 1, (3, 4, 2), (4, 5, 2))
    ha, hb = up(prov, args[0], args[1]), up(prov, args[2])
    hc = prov.complex_pagefun(request([ha, hb], (3, 4, 2), (4, 5, 2)))
    assert prov.is_complex(hc) and list(hc.shape) == [3, 5, 2]
    flat = prov.download(hc)
    assert flat.dtype == np.complex128 and flat.view(np.float64).size == 2 * 3 * 5 * 2
    want = ref.cpagefun_host(*args)
    assert np.array_equal(bits(flat.view(np.float64)), bits(ref.interleave(*want)))
    for h in (ha, hb, hc):
        prov.free(h)


# ---- precision 32 --------------------------------------------------------------------------------------------------------------------
def test_f32_provider_rounds_each_part_once():
    p32 = HipProvider(0, precision="F32")
    try:
        rng = np.random.default_rng(13)
        f32 = lambda x: None if x is None else x.astype(np.float32).astype(np.float64)
        for kind in ref.KINDS:
            for (m, n, k, p), exact in [((5, 4, 3, 50), True), ((40, 33, 20, 3), False)]:
                args = tuple(f32(x) for x in ref.operands(rng, kind, (m, k, p), (k, n, p)))
                got = run(p32, *args)
                want = ref.cpagefun_host(*args)
                assert got[2] == (2 if exact else 3)
                for x in got[:2]:
                    assert np.array_equal(x, f32(x))  # every part is an f32 value
                if exact:
                    assert_bitwise(got[:2], tuple(f32(w) for w in want))
                else:
                    assert_gate(got[:2], args, want, extra=2.0 ** -24)
    finally:
        p32.close()


# ---- determinism, inputs, host traffic and launches ----------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k,pages", [(4, 4, 4, 1000), (40, 40, 40, 50)])
def test_two_calls_bitwise_identical_and_inputs_unchanged(prov, kind, m, n, k, pages):
    rng = np.random.default_rng(14)
    Ar, Ai, Br, Bi = ref.operands(rng, kind, (m, k, pages), (k, n, pages))
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    req = request([ha, hb], Ar.shape, Br.shape)
    h1, h2 = prov.complex_pagefun(req), prov.complex_pagefun(req)
    assert np.array_equal(bits(prov.download(h1).view(np.float64)), bits(prov.download(h2).view(np.float64)))
    for h, re_, im_ in ((ha, Ar, Ai), (hb, Br, Bi)):
        flat = prov.download(h)
        want = ref.interleave(re_, im_) if im_ is not None else re_.ravel(order="F")
        assert np.array_equal(bits(flat.view(np.float64)), bits(want))
    for h in (ha, hb, h1, h2):
        prov.free(h)


@kinds
@pytest.mark.parametrize("m,k,n", [(4, 4, 4), (16, 16, 16), (40, 40, 40)])
def test_no_host_read_and_at_most_two_launches(prov, kind, m, k, n):
    P = 20000 if max(m, n, k) <= 16 else 500

    def operand(shape, cplx):
        hr = prov.random_uniform(shape)
        if not cplx:
            return hr
        hi = prov.random_uniform(shape)
        z = prov.complex_from_real_imag(hr, hi)
        prov.free(hr)
        prov.free(hi)
        return z

    ha, hb = operand([m, k, P], kind != 2), operand([k, n, P], kind != 1)
    req = request([ha, hb], ha.shape, hb.shape)
    prov.free(prov.complex_pagefun(req))  # warm
    t0 = prov.telemetry_snapshot()
    hc = prov.complex_pagefun(req)
    t1 = prov.telemetry_snapshot()
    assert t1["download_bytes"] == t0["download_bytes"]
    assert 1 <= t1["kernel_launches"] - t0["kernel_launches"] <= 2
    for h in (ha, hb, hc):
        prov.free(h)
