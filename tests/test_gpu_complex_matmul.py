"""GPU checks of `A * B` with a complex-interleaved operand (rmhip_complex_matmul; runmat_amd/csrc/cgemm.hip around one real product of
dgemm.hip, routed by gemm_plan.h plan_cgemm) against the host loops (tests/complex_matmul_ref.py over complex_pagefun_ref.py): the small
route bit-exact, the embedded product within the derived gate (2k eps sum|a||b| per part, k eps for the mixed kinds) and bit-exact on
Gaussian integers, route and operand kind read from the launch log on both sides of the boundary, the class of non-finite values, the
shape and refusal rules, views, precision 32 and a chain behind fft_dim."""
import ctypes as C

import numpy as np
import pytest

import complex_matmul_ref as ref
from runmat_amd import HipProvider, ProviderError
from runmat_amd import _lib

pytestmark = pytest.mark.gpu

KIND_IDS = {0: "cc", 1: "cr", 2: "rc"}
kinds = pytest.mark.parametrize("kind", ref.KINDS, ids=lambda k: KIND_IDS[k])
shape_id = lambda v: "x".join(str(d) for d in v) if isinstance(v, tuple) else str(v)


def last_launch(prov):
    log = [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "complex_matmul"]
    return log[-1]


def live_bytes(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]  # what the buffers alive hold: a pooled block belongs to no buffer


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
    """-> (Cr, Ci, route or None for an empty result or k == 0); the logged operand kind and the result's storage are checked on the way."""
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    hc = prov.complex_matmul(ha, hb)
    assert list(hc.shape) == [Ar.shape[0], Br.shape[1]] and prov.is_complex(hc)
    route = None
    if Ar.shape[0] and Br.shape[1]:
        e = last_launch(prov)
        assert e["tuning"]["kind"] == ref.kind_of(Ai, Bi)
        assert e["shape"] == {"m": Ar.shape[0], "n": Br.shape[1], "k": Ar.shape[1]}
        route = e["tuning"]["route"] or None
    Cr, Ci = parts(prov, hc)
    for h in (ha, hb, hc):
        prov.free(h)
    return Cr, Ci, route


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_bitwise(got, want):
    """Bit for bit; a NaN matches any NaN (the host's and the device's default NaNs may differ in sign and payload)."""
    for g, w in zip(got, want):
        assert g.shape == w.shape
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn)
        assert np.array_equal(bits(g)[~gn], bits(w)[~wn])


def assert_gate(got, args, want, ulp32=False, label=""):
    """`ulp32`: one f32 ulp of the reference part on top of the gate (the one f32 rounding of a precision-32 result).  The worst ratio is
    printed before it is held to 1."""
    g = ref.gate(*args)
    for part, (x, w) in enumerate(zip(got, want)):
        assert x.shape == w.shape
        bound = g[part] + (np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) if ulp32 else 0.0)
        d = np.abs(x - w)
        print(f"{label} part {part}: worst |device - host| / bound = {np.max(d / np.maximum(bound, 1e-300)):.4f}")
        assert np.all(d <= bound), (part, float(np.max(d - bound)))


# ---- small route: bit-exact ------------------------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k", ref.SMALL_SHAPES)
def test_small_route_bitwise(prov, kind, m, n, k):
    args = ref.operands(np.random.default_rng(100 + kind), kind, (m, k), (k, n))
    Cr, Ci, route = run(prov, *args)
    assert route == 2
    assert_bitwise((Cr, Ci), ref.cmatmul_host(*args))


# ---- boundaries and the embedded product -----------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k", ref.BOUNDARY_SHAPES)
def test_one_past_the_small_route_embeds(prov, kind, m, n, k):
    args = ref.operands(np.random.default_rng(5), kind, (m, k), (k, n), ints=True)
    Cr, Ci, route = run(prov, *args)
    assert route == 4
    assert_bitwise((Cr, Ci), ref.cmatmul_host(*args))


@kinds
@pytest.mark.parametrize("m,n,k", ref.EMBED_SHAPES)
def test_embed_route_gate_and_exact_integers(prov, kind, m, n, k):
    rng = np.random.default_rng(m * 7 + n)
    args = ref.operands(rng, kind, (m, k), (k, n))
    Cr, Ci, route = run(prov, *args)
    real = prov.gemm_last_route()  # the embedded real product, as launch_dgemm ran it
    print(f"kind {kind} {m}x{n}x{k}: embedded product on {real['kernel']!r} guard={real['guard']} splits={real['splits']}")
    assert route == 4 and real["kernel"]
    if (m, n, k) == ref.EMBED_SHAPES[-1]:
        assert real["splits"] > 1
    assert_gate((Cr, Ci), args, ref.cmatmul_host(*args), label=f"kind {kind} {m}x{n}x{k}")
    args = ref.operands(rng, kind, (m, k), (k, n), ints=True)
    Cr, Ci, route = run(prov, *args)
    assert route == 4
    assert_bitwise((Cr, Ci), ref.cmatmul_host(*args))


# ---- non-finite values -----------------------------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k,route", [(5, 4, 3, 2), (40, 36, 21, 4)])
def test_one_planted_non_finite_keeps_its_class(prov, kind, m, n, k, route):
    """One +Inf, -Inf or NaN in either part of either operand, the other entries Gaussian integers in -4..4 (so every finite part is exact
    and its sign is decided): isnan, isinf and the sign of every part are the host loop's.  The planted spot walks over the corners, the
    last k index included, where the guarded tiles zero their k tail."""
    rng = np.random.default_rng(50 + kind)
    spots_a = [(0, 0), (m - 1, k - 1), (1, k - 1)]
    spots_b = [(0, 0), (k - 1, n - 1), (k - 1, 1)]
    case = 0
    for value in (np.inf, -np.inf, np.nan):
        for operand, part in ((0, 0), (0, 1), (1, 0), (1, 1)):
            args = list(ref.operands(rng, kind, (m, k), (k, n), ints=True))
            target = args[2 * operand + part]
            if target is None:
                continue  # the real operand of a mixed kind has no imaginary part
            target[(spots_a if operand == 0 else spots_b)[case % 3]] = value
            case += 1
            Cr, Ci, r = run(prov, *args)
            assert r == route
            for g, w in zip((Cr, Ci), ref.cmatmul_host(*args)):
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (value, operand, part)
                ok = ~np.isnan(w)
                assert np.array_equal(np.signbit(g)[ok], np.signbit(w)[ok]), (value, operand, part)
                assert np.array_equal(bits(g)[ok], bits(w)[ok])


@pytest.mark.parametrize("m,n,k,route", [(5, 3, 4, 2), (40, 36, 20, 4)])
def test_mixed_kinds_keep_an_inf_on_both_routes(prov, m, n, k, route):
    """complex x real (and its mirror) never multiplies by an implied zero: Inf stays Inf where the complex x complex form with a zero
    imaginary part gives NaN.  The real operand is positive, so no Inf meets a zero or an Inf of the other sign."""
    rng = np.random.default_rng(3)
    Zr, Zi = rng.standard_normal((m, k)), rng.standard_normal((m, k))
    Zr[1, 2], Zi[m - 1, k - 1] = np.inf, np.inf
    R = rng.uniform(0.5, 2.0, (k, n))
    Cr, Ci, r = run(prov, Zr, Zi, R, None)
    assert r == route
    assert np.all(Cr[1, :] == np.inf) and np.all(Ci[m - 1, :] == np.inf) and not np.any(np.isnan(Cr)) and not np.any(np.isnan(Ci))
    want = ref.cmatmul_host(Zr, Zi, R, None)
    assert np.array_equal(np.isinf(Cr), np.isinf(want[0])) and np.array_equal(np.isinf(Ci), np.isinf(want[1]))
    Cr0, Ci0, _ = run(prov, Zr, Zi, R, np.zeros_like(R))
    assert np.all(np.isnan(Ci0[1, :])) and np.all(np.isnan(Cr0[m - 1, :]))
    Dr, Di, r = run(prov, R.T.copy(), None, Zr.T.copy(), Zi.T.copy())  # the mirror image: real x complex
    assert r == route
    assert np.all(Dr[:, 1] == np.inf) and np.all(Di[:, m - 1] == np.inf) and not np.any(np.isnan(Dr)) and not np.any(np.isnan(Di))


# ---- shape rules and refusals ------------------------------------------------------------------------------------------------------------
@kinds
def test_empties_and_k_zero(prov, kind):
    for lhs, rhs in [((0, 3), (3, 4)), ((3, 2), (2, 0)), ((0, 0), (0, 0)), ((0, 40), (40, 50))]:
        Ar, Br = np.zeros(lhs), np.zeros(rhs)
        Cr, Ci, _ = run(prov, Ar, Ar.copy() if kind != 2 else None, Br, Br.copy() if kind != 1 else None)
        assert Cr.shape == (lhs[0], rhs[1]) and Cr.size == 0 and Ci.size == 0
    for lhs, rhs in [((3, 0), (0, 5)), ((40, 0), (0, 300))]:
        Ar, Br = np.zeros(lhs), np.zeros(rhs)
        Cr, Ci, route = run(prov, Ar, Ar.copy() if kind != 2 else None, Br, Br.copy() if kind != 1 else None)
        assert route is None and Cr.shape == (lhs[0], rhs[1]) and Cr.size
        for x in (Cr, Ci):
            assert np.all(x == 0.0) and not np.any(np.signbit(x))


def test_refusals_leave_nothing_behind(prov):
    rng = np.random.default_rng(11)
    A, B = rng.standard_normal((3, 4)), rng.standard_normal((4, 5))
    ha, hb, hra = up(prov, A, A), up(prov, B), up(prov, A)
    hbig, hrbig = up(prov, rng.standard_normal((40, 50)), rng.standard_normal((40, 50))), up(prov, rng.standard_normal((40, 50)))
    T3 = rng.standard_normal((4, 5, 2))
    h3 = up(prov, T3, T3)
    live = live_bytes(prov)

    def refused(a, b, call=None):
        with pytest.raises(ProviderError) as e:
            (call or prov.complex_matmul)(a, b)
        assert live_bytes(prov) == live  # no result and no workspace is left behind
        return e.value

    e = refused(hra, hb)  # both real
    assert e.code == _lib.ERR_UNSUPPORTED and "rmhip_matmul" in str(e)
    e = refused(ha, h3)  # a 3-D operand
    assert e.code == _lib.ERR_UNSUPPORTED and "only 2D" in str(e)
    assert refused(h3, hb).code == _lib.ERR_UNSUPPORTED
    e = refused(hb, ha)  # 4x5 * 3x4
    assert e.code == _lib.ERR_SHAPE and "inner dims must agree" in str(e)
    assert refused(hbig, ha).code == _lib.ERR_SHAPE and refused(hrbig, hbig).code == _lib.ERR_SHAPE  # past the small route as well
    # rmhip_matmul keeps refusing complex storage, either side
    assert refused(ha, hb, prov.matmul).code == _lib.ERR_UNSUPPORTED and refused(hra, hbig, prov.matmul).code == _lib.ERR_UNSUPPORTED
    # past the Python mirror: a null out, unknown ids (out is cleared), and their order
    fn, ctx = prov._lib.rmhip_complex_matmul, prov._ctx
    out = C.c_uint64(7)
    assert fn(ctx, ha.buffer_id, hb.buffer_id, None) == _lib.ERR_INVALID
    assert fn(ctx, 1 << 60, hb.buffer_id, None) == _lib.ERR_INVALID
    assert fn(ctx, 1 << 60, hb.buffer_id, C.byref(out)) == _lib.ERR_NOT_FOUND and out.value == 0
    out = C.c_uint64(7)
    assert fn(ctx, ha.buffer_id, 1 << 60, C.byref(out)) == _lib.ERR_NOT_FOUND and out.value == 0
    out = C.c_uint64(7)
    assert fn(ctx, hra.buffer_id, h3.buffer_id, C.byref(out)) == _lib.ERR_UNSUPPORTED and out.value == 0
    # and the call that is served still is
    hc = prov.complex_matmul(ha, hb)
    assert_bitwise(parts(prov, hc), ref.cmatmul_host(A, A, B, None))
    for h in (ha, hb, hra, hbig, hrbig, h3, hc):
        prov.free(h)


# ---- views, lazy operands and precision 32 -----------------------------------------------------------------------------------------------
def test_transpose_view_and_lazy_normal_real_operands(prov):
    rng = np.random.default_rng(12)
    # complex x real, the real operand a transpose view, on the embedded route
    Bt = rng.standard_normal((36, 20))  # B = Bt' is 20 x 36
    hbt = prov.upload(Bt.ravel(order="F"), Bt.shape)
    hbv = prov.transpose(hbt)
    Pr, Pi = rng.standard_normal((40, 20)), rng.standard_normal((40, 20))
    hp = up(prov, Pr, Pi)
    hd = prov.complex_matmul(hp, hbv)
    assert last_launch(prov)["tuning"] == {"kind": 1, "route": 4}
    args = (Pr, Pi, Bt.T.copy(), None)
    assert_gate(parts(prov, hd), args, ref.cmatmul_host(*args), label="transpose view")
    # real x complex, the real operand a transpose view, on the small route; the view's base keeps its values
    At = rng.standard_normal((4, 3))  # A = At' is 3 x 4
    hat = prov.upload(At.ravel(order="F"), At.shape)
    hav = prov.transpose(hat)
    Qr, Qi = rng.standard_normal((4, 2)), rng.standard_normal((4, 2))
    hq = up(prov, Qr, Qi)
    he = prov.complex_matmul(hav, hq)
    assert last_launch(prov)["tuning"] == {"kind": 2, "route": 2}
    assert_bitwise(parts(prov, he), ref.cmatmul_host(At.T.copy(), None, Qr, Qi))
    assert np.array_equal(bits(prov.download(hat)), bits(At.ravel(order="F")))
    # a lazy random_normal real operand is settled first; its handle then holds the values the product used
    hn = prov.random_normal([4, 3])
    Mr, Mi = rng.standard_normal((3, 5)), rng.standard_normal((3, 5))
    hm = up(prov, Mr, Mi)
    hf = prov.complex_matmul(hn, hm)
    N = prov.download(hn).reshape((4, 3), order="F")
    assert_bitwise(parts(prov, hf), ref.cmatmul_host(N, None, Mr, Mi))
    for h in (hbt, hbv, hp, hd, hat, hav, hq, he, hn, hm, hf):
        prov.free(h)


def test_f32_provider_rounds_each_part_once():
    """Operands as a precision-32 provider holds them (the real one of a mixed kind in f32 storage), the reference on the values they
    hold: the small route gives the f32 rounding of the bit-exact value, the embedded one an f32 value within the gate plus one f32 ulp
    of the reference part - kind 1 included, whose join runs only here."""
    p32 = HipProvider(0, precision="F32")
    try:
        rng = np.random.default_rng(13)
        for kind in ref.KINDS:
            for (m, n, k), route in [((5, 4, 3), 2), ((40, 33, 20), 4), ((129, 40, 16), 4)]:
                Ar, Ai, Br, Bi = ref.operands(rng, kind, (m, k), (k, n))
                ha, hb = up(p32, Ar, Ai), up(p32, Br, Bi)
                held = []
                for h, im in ((ha, Ai), (hb, Bi)):
                    flat = p32.download(h).reshape(h.shape, order="F")
                    held += [np.asfortranarray(flat.real), np.asfortranarray(flat.imag)] if im is not None else [np.asfortranarray(flat), None]
                for x in held:
                    assert x is None or np.array_equal(x, ref.f32_round(x))
                hc = p32.complex_matmul(ha, hb)
                assert p32.is_complex(hc) and last_launch(p32)["tuning"] == {"kind": kind, "route": route}
                got, want = parts(p32, hc), ref.cmatmul_host(*held)
                for x in got:
                    assert np.array_equal(x, ref.f32_round(x))  # every part is an f32 value
                if route == 2:
                    assert_bitwise(got, tuple(ref.f32_round(w) for w in want))
                else:
                    assert_gate(got, held, want, ulp32=True, label=f"f32 kind {kind} {m}x{n}x{k}")
                for h in (ha, hb, hc):
                    p32.free(h)
    finally:
        p32.close()


# ---- determinism, inputs, host traffic and launches --------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k,launches", [(5, 4, 3, (1, 1, 1)), (33, 40, 17, (3, 1, 3)), (64, 64, 2048, (4, 2, 4))], ids=shape_id)
def test_two_calls_bitwise_identical_inputs_unchanged_no_host_read(prov, kind, m, n, k, launches):
    """`launches`, per kind: one for the small route; split, product and join around an embedded product (the product alone for
    complex x real), one more where the product splits along k and sums its slices."""
    Ar, Ai, Br, Bi = ref.operands(np.random.default_rng(14), kind, (m, k), (k, n))
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    h1 = prov.complex_matmul(ha, hb)
    t0 = prov.telemetry_snapshot()
    h2 = prov.complex_matmul(ha, hb)
    t1 = prov.telemetry_snapshot()
    assert t1["download_bytes"] == t0["download_bytes"]
    assert t1["kernel_launches"] - t0["kernel_launches"] == launches[kind]
    assert np.array_equal(bits(prov.download(h1).view(np.float64)), bits(prov.download(h2).view(np.float64)))
    for h, re_, im_ in ((ha, Ar, Ai), (hb, Br, Bi)):
        flat = prov.download(h)
        want = ref.interleave(re_, im_) if im_ is not None else re_.ravel(order="F")
        assert np.array_equal(bits(flat.view(np.float64)), bits(want))
    for h in (ha, hb, h1, h2):
        prov.free(h)


def test_a_transform_result_times_a_real_matrix_stays_on_the_device(prov):
    """H * fft(x): x is 64 x 3, H real 40 x 64 - real x complex on the embedded route, against the host loop on the downloaded F."""
    rng = np.random.default_rng(16)
    X, H = rng.standard_normal((64, 3)), rng.standard_normal((40, 64))
    hx, hh = up(prov, X), up(prov, H)
    t0 = prov.telemetry_snapshot()
    hF = prov.fft_dim(hx, None, 0)
    hc = prov.complex_matmul(hh, hF)
    t1 = prov.telemetry_snapshot()
    assert t1["download_bytes"] == t0["download_bytes"] and t1["upload_bytes"] == t0["upload_bytes"]
    assert prov.is_complex(hc) and list(hc.shape) == [40, 3] and last_launch(prov)["tuning"] == {"kind": 2, "route": 4}
    Fr, Fi = parts(prov, hF)
    args = (H, None, Fr, Fi)
    assert_gate(parts(prov, hc), args, ref.cmatmul_host(*args), label="H * fft(x)")
    for h in (hx, hh, hF, hc):
        prov.free(h)
