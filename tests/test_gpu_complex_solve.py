"""GPU checks of `A \\ b`, `b / A` and `inv(A)` with a complex-interleaved operand (rmhip_complex_mldivide / _mrdivide / _inv, solve.cpp;
the passes of csolve.hip around ONE real solve, planned by csolve_plan.h): bit equality with `mldivide` on the embedded real system the
tests build themselves (tests/complex_solve_ref.py embed / stack / join), parity with the reference's host path (solve_ref) at the gates
the real solve is already held to, the rank tolerance counted in complex dimensions, singular and rank-deficient systems, the refusals,
views, precision 32, a chain behind fft_dim and the launch log.

The parity gate is the one tests/test_gpu_solvepath.py (lines 327, 349: LU and small-solver answers against the oracle) and
tests/test_gpu_svdpath.py (line 35, tol=1e-9: SVD answers) hold rmhip_mldivide to: max |x - want| <= 1e-9 * max(1, max |want|)."""
import ctypes as C

import numpy as np
import pytest

import complex_solve_ref as ref
from runmat_amd import HipProvider, ProviderError
from runmat_amd import _lib

pytestmark = pytest.mark.gpu

GATE = 1e-9  # test_gpu_solvepath.py:327,349 and test_gpu_svdpath.py:35
KIND_IDS = {0: "cc", 1: "cr", 2: "rc"}
kinds = pytest.mark.parametrize("kind", ref.KINDS, ids=lambda k: KIND_IDS[k])
shape_id = lambda v: "x".join(str(d) for d in v) if isinstance(v, tuple) else str(v)
ALL_SHAPES = [(n, n, k) for n, k in ref.SQUARE_SHAPES] + ref.RECT_SHAPES


def up(prov, re, im=None):
    """A real tensor, or the complex-interleaved one of the two parts."""
    re = np.asarray(re, dtype=np.float64)
    hr = prov.upload(re.ravel(order="F"), re.shape)
    if im is None:
        return hr
    hi = prov.upload(np.asarray(im, dtype=np.float64).ravel(order="F"), re.shape)
    z = prov.complex_from_real_imag(hr, hi)
    prov.free(hr)
    prov.free(hi)
    return z


def upz(prov, Z):
    return up(prov, np.ascontiguousarray(Z.real), np.ascontiguousarray(Z.imag))


def take(prov, h, free=True):
    x = prov.download(h).reshape(h.shape, order="F")
    if free:
        prov.free(h)
    return x


def bits(z):
    return np.ascontiguousarray(z).view(np.float64).view(np.uint64)


def live_bytes(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]  # what the buffers alive hold: a pooled block belongs to no buffer


def last_launch(prov):
    return [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "complex_solve"][-1]


def fallbacks(prov, name):
    return dict(prov.telemetry_snapshot()["solve_fallbacks"]).get(name, 0)


def device_solve(prov, Ar, Ai, Br, Bi):
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    hx = prov.complex_mldivide(ha, hb)
    assert prov.is_complex(hx) and list(hx.shape) == [Ar.shape[1], Br.shape[1]]
    x = take(prov, hx)
    prov.free(ha)
    prov.free(hb)
    return x


def embedded_real_solve(prov, kind, Ar, Ai, Br, Bi):
    """rmhip_mldivide on the real system the tests embed and stack on the host, re-joined."""
    ha = up(prov, ref.embed(Ar, Ai) if kind != 2 else Ar)
    hb = up(prov, ref.stack(kind, Br, Bi))
    T = take(prov, prov.mldivide(ha, hb))
    prov.free(ha)
    prov.free(hb)
    return ref.join(kind, T, Ar.shape[1], Br.shape[1])


def assert_parity(x, want, label):
    worst = float(np.max(np.abs(x - want))) / (GATE * max(1.0, float(np.max(np.abs(want)))))
    print(f"{label}: worst |device - host| / gate = {worst:.3e}")
    assert x.shape == want.shape and worst <= 1.0


# ---- 1. bit equality with the real solve ---------------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k", ALL_SHAPES, ids=shape_id)
def test_bitwise_the_real_solve_of_the_embedded_system(prov, kind, m, n, k):
    args = ref.operands(np.random.default_rng(1000 * kind + 7 * m + n + k), kind, m, n, k)
    x = device_solve(prov, *args)
    e = last_launch(prov)
    assert e["shape"] == {"m": m, "n": n, "nrhs": k} and e["tuning"] == {"kind": kind, "entry": ref.MLDIVIDE}
    want = embedded_real_solve(prov, kind, *args)
    assert x.shape == want.shape == (n, k) and np.array_equal(bits(x), bits(want))


@pytest.mark.parametrize("n", ref.INV_ORDERS)
def test_inv_bitwise_the_embedded_solve_against_the_identity(prov, n):
    rng = np.random.default_rng(20 + n)
    Ar, Ai = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    ha = up(prov, Ar, Ai)
    hx = prov.complex_inv(ha)
    assert prov.is_complex(hx) and list(hx.shape) == [n, n]
    assert last_launch(prov)["tuning"] == {"kind": 0, "entry": ref.INV} and last_launch(prov)["shape"] == {"m": n, "n": n, "nrhs": n}
    x = take(prov, hx)
    prov.free(ha)
    want = embedded_real_solve(prov, 0, Ar, Ai, np.eye(n), np.zeros((n, n)))
    assert np.array_equal(bits(x), bits(want))
    assert_parity(x, ref.solve_ref(Ar + 1j * Ai, np.eye(n)), f"inv {n}")


@kinds
@pytest.mark.parametrize("n,k", ref.MRDIVIDE_SHAPES, ids=shape_id)
def test_mrdivide_bitwise_the_transposed_mldivide(prov, kind, n, k):
    """B / A against (A.' \\ B.').' with the transposes taken on the host: plain ones, not conjugate ones."""
    rng = np.random.default_rng(30 + n + kind)
    Ar, Br = rng.standard_normal((n, n)), rng.standard_normal((k, n))
    Ai = rng.standard_normal((n, n)) if kind != 2 else None
    Bi = rng.standard_normal((k, n)) if kind != 1 else None
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    hx = prov.complex_mrdivide(hb, ha)
    assert prov.is_complex(hx) and list(hx.shape) == [k, n]
    e = last_launch(prov)
    assert e["shape"] == {"m": n, "n": n, "nrhs": k} and e["tuning"] == {"kind": kind, "entry": ref.MRDIVIDE}
    x = take(prov, hx)
    prov.free(ha)
    prov.free(hb)
    t = lambda M: None if M is None else np.ascontiguousarray(M.T)
    want = device_solve(prov, t(Ar), t(Ai), t(Br), t(Bi)).T
    assert np.array_equal(bits(x), bits(want))
    A, B = ref.as_complex(Ar, Ai), ref.as_complex(Br, Bi)
    assert_parity(x, ref.solve_ref(A.T, B.T).T, f"mrdivide kind {kind} {n}x{k}")


# ---- 2. parity with the host contract ------------------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("m,n,k", ALL_SHAPES, ids=shape_id)
def test_parity_with_the_reference_solve(prov, kind, m, n, k):
    Ar, Ai, Br, Bi = ref.operands(np.random.default_rng(2000 * kind + 7 * m + n + k), kind, m, n, k)
    x = device_solve(prov, Ar, Ai, Br, Bi)
    assert_parity(x, ref.solve_ref(ref.as_complex(Ar, Ai), ref.as_complex(Br, Bi)), f"kind {kind} {m}x{n}x{k}")


# ---- 3. the tolerance counts with the complex dimensions -----------------------------------------------------------------------------------
def test_the_rank_tolerance_counts_the_complex_dimensions(prov):
    """n = 8, A = Q diag(1, ..., 1, 1.5 n eps): the smallest singular value (1.498 n eps; 1.489 and 1.493 n eps in E(A), measured in
    tests/test_complex_solve_host.py) lies between the tolerance of the reference, n eps, which keeps it, and the one the embedded
    dimensions would give, 2n eps, which drops it.  A class check: norm(x) within a factor 2 of the keeping answer, which is more than
    1e6 times the dropping one."""
    A = ref.tolerance_case()
    n = A.shape[0]
    b = np.ones((n, 1), dtype=np.complex128)
    keep, drop = np.linalg.norm(ref.solve_ref(A, b)), np.linalg.norm(ref.solve_ref(A, b, tol_dim=2 * n))
    assert keep > 1e6 * drop
    ha, hb = upz(prov, A), upz(prov, b)
    s0 = prov.lu_stats()["svd_solves"]
    x = take(prov, prov.complex_mldivide(ha, hb))
    assert prov.lu_stats()["svd_solves"] == s0 + 1
    got = np.linalg.norm(x)
    print(f"norm(x): device {got:.4e}, tolerance from n {keep:.4e}, from 2n {drop:.4e}")
    assert keep / 2 <= got <= 2 * keep
    prov.free(ha)
    prov.free(hb)


# ---- 4. singular and rank-deficient systems ------------------------------------------------------------------------------------------------
def rank_deficient(rng, m, n, rank):
    return (rng.standard_normal((m, rank)) + 1j * rng.standard_normal((m, rank))) @ (rng.standard_normal((rank, n)) + 1j * rng.standard_normal((rank, n)))


def test_singular_square_system_minimum_norm_and_inv_refuses(prov):
    rng = np.random.default_rng(41)
    A = rank_deficient(rng, 3, 3, 2)
    b = A @ (rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2)))  # consistent
    ha, hb = upz(prov, A), upz(prov, b)
    s0 = prov.lu_stats()["svd_solves"]
    x = take(prov, prov.complex_mldivide(ha, hb))
    assert prov.lu_stats()["svd_solves"] == s0 + 1
    assert_parity(x, ref.solve_ref(A, b), "rank 2 of 3")
    live, f0 = live_bytes(prov), fallbacks(prov, "inv:singular")
    with pytest.raises(ProviderError) as e:
        prov.complex_inv(ha)
    assert e.value.code == _lib.ERR_SINGULAR
    assert fallbacks(prov, "inv:singular") == f0 + 1 and live_bytes(prov) == live
    assert prov.lu_stats()["svd_solves"] == s0 + 1  # inv never takes the minimum-norm answer
    prov.free(ha)
    prov.free(hb)


def test_tall_rank_deficient_system(prov):
    rng = np.random.default_rng(42)
    A = rank_deficient(rng, 6, 3, 2)
    b = rng.standard_normal((6, 2)) + 1j * rng.standard_normal((6, 2))
    ha, hb = upz(prov, A), upz(prov, b)
    s0 = prov.lu_stats()["svd_solves"]
    x = take(prov, prov.complex_mldivide(ha, hb))
    assert prov.lu_stats()["svd_solves"] == s0 + 1
    assert_parity(x, ref.solve_ref(A, b), "6x3 rank 2")
    prov.free(ha)
    prov.free(hb)


# ---- 5. refusals and shapes ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(prov):
    rng = np.random.default_rng(51)
    A, B = rng.standard_normal((3, 3)), rng.standard_normal((3, 2))
    ha, hb, hra, hrb = up(prov, A, A[::-1].copy()), up(prov, B, B), up(prov, A), up(prov, B)
    h4 = up(prov, rng.standard_normal((4, 2)), rng.standard_normal((4, 2)))
    T3 = rng.standard_normal((3, 2, 2))
    h3 = up(prov, T3, T3)
    hs = up(prov, np.array([[2.0]]), np.array([[1.0]]))
    hrect = up(prov, rng.standard_normal((3, 4)), rng.standard_normal((3, 4)))
    hwide = up(prov, np.zeros((3, 65536)), np.zeros((3, 65536)))
    hhalf = up(prov, np.zeros((3, 32768)), np.zeros((3, 32768)))
    he = prov.zeros_with_storage([0, 3], "complex")
    he1 = prov.zeros_with_storage([0, 1], "complex")
    live = live_bytes(prov)

    def refused(call, *args):
        with pytest.raises(ProviderError) as e:
            call(*args)
        assert live_bytes(prov) == live  # no result and no workspace is left behind
        return e.value

    for call, sibling in ((prov.complex_mldivide, "rmhip_mldivide"), (prov.complex_mrdivide, "rmhip_mrdivide")):
        e = refused(call, hra, hrb)  # both real
        assert e.code == _lib.ERR_UNSUPPORTED and f"both operands are real ({sibling} serves them)" in str(e)
    e = refused(prov.complex_inv, hra)
    assert e.code == _lib.ERR_UNSUPPORTED and "rmhip_inv serves it" in str(e)
    e = refused(prov.complex_mldivide, ha, h3)  # more than two dimensions
    assert e.code == _lib.ERR_UNSUPPORTED and "mldivide: only 2D supported" in str(e)
    e = refused(prov.complex_mrdivide, h3, ha)
    assert e.code == _lib.ERR_UNSUPPORTED and "mrdivide: only 2D supported" in str(e)
    for call, args in ((prov.complex_mldivide, (hs, hb)), (prov.complex_mrdivide, (hb, hs)), (prov.complex_inv, (hs,))):  # a 1 x 1 divisor
        e = refused(call, *args)
        assert e.code == _lib.ERR_UNSUPPORTED and "scalar operands use the CPU path" in str(e)
    e = refused(prov.complex_mldivide, ha, h4)
    assert e.code == _lib.ERR_SHAPE and "mldivide: row mismatch (3 vs 4)" in str(e)
    e = refused(prov.complex_mrdivide, h4, ha)  # 4 x 2 / 3 x 3
    assert e.code == _lib.ERR_SHAPE and "mrdivide: column mismatch (2 vs 3)" in str(e)
    e = refused(prov.complex_mldivide, ha, hwide)  # 65536 embedded right-hand sides
    assert e.code == _lib.ERR_UNSUPPORTED and "more than 65535 right-hand sides" in str(e)
    e = refused(prov.complex_mldivide, hra, hhalf)  # a real A doubles the columns
    assert e.code == _lib.ERR_UNSUPPORTED and "more than 65535 right-hand sides" in str(e)
    e = refused(prov.complex_mldivide, he, he1)  # an empty system, as the sibling
    assert e.code == _lib.ERR_UNSUPPORTED and "mldivide: empty system" in str(e)
    e = refused(prov.complex_inv, hrect)
    assert e.code == _lib.ERR_INVALID and "inv: input must be a square matrix." in str(e)
    e = refused(prov.complex_inv, h3)
    assert e.code == _lib.ERR_INVALID and "inv: inputs must be 2-D matrices." in str(e)
    # the real siblings keep refusing complex storage with their old message
    for call, args in ((prov.mldivide, (ha, hrb)), (prov.mldivide, (hra, hb)), (prov.mrdivide, (hb, hra)), (prov.inv, (ha,))):
        e = refused(call, *args)
        assert e.code == _lib.ERR_UNSUPPORTED and "this entry point takes real tensors" in str(e)
    # past the Python mirror: a null out, unknown ids (out is cleared), and their order
    for fn in (prov._lib.rmhip_complex_mldivide, prov._lib.rmhip_complex_mrdivide):
        out = C.c_uint64(7)
        assert fn(prov._ctx, ha.buffer_id, hb.buffer_id, None) == _lib.ERR_INVALID
        assert fn(prov._ctx, 1 << 60, hb.buffer_id, None) == _lib.ERR_INVALID
        assert fn(prov._ctx, 1 << 60, hb.buffer_id, C.byref(out)) == _lib.ERR_NOT_FOUND and out.value == 0
        out = C.c_uint64(7)
        assert fn(prov._ctx, hra.buffer_id, 1 << 60, C.byref(out)) == _lib.ERR_NOT_FOUND and out.value == 0
    out = C.c_uint64(7)
    assert prov._lib.rmhip_complex_inv(prov._ctx, ha.buffer_id, None) == _lib.ERR_INVALID
    assert prov._lib.rmhip_complex_inv(prov._ctx, 1 << 60, C.byref(out)) == _lib.ERR_NOT_FOUND and out.value == 0
    assert live_bytes(prov) == live
    # and the calls that are served still are
    x = take(prov, prov.complex_mldivide(ha, hb))
    assert_parity(x, ref.solve_ref(A + 1j * A[::-1], B + 1j * B), "after the refusals")
    for h in (ha, hb, hra, hrb, h4, h3, hs, hrect, hwide, hhalf, he, he1):
        prov.free(h)


def test_inv_keeps_a_trailing_singleton_and_the_empty_matrix(prov):
    rng = np.random.default_rng(52)
    Ar, Ai = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    ha = up(prov, Ar, Ai)
    h3 = up(prov, Ar.reshape(3, 3, 1), Ai.reshape(3, 3, 1))  # (a reshape would rename the shape of `ha` itself)
    hx, hy = prov.complex_inv(ha), prov.complex_inv(h3)
    assert list(hx.shape) == [3, 3] and list(hy.shape) == [3, 3, 1] and prov.is_complex(hy)
    assert np.array_equal(bits(prov.download(hx)), bits(prov.download(hy)))
    he = prov.zeros_with_storage([0, 0], "complex")
    hz = prov.complex_inv(he)
    assert list(hz.shape) == [0, 0] and prov.is_complex(hz) and prov.download(hz).size == 0
    for h in (ha, h3, hx, hy, he, hz):
        prov.free(h)


def test_a_real_operand_given_as_a_transpose_view(prov):
    rng = np.random.default_rng(53)
    Ar, Ai = rng.standard_normal((33, 33)), rng.standard_normal((33, 33))
    Bt = rng.standard_normal((2, 33))  # b = Bt.' is 33 x 2
    hbt = up(prov, Bt)
    hbv = prov.transpose(hbt)
    ha = up(prov, Ar, Ai)
    x = take(prov, prov.complex_mldivide(ha, hbv))
    assert last_launch(prov)["tuning"] == {"kind": 1, "entry": ref.MLDIVIDE}
    assert np.array_equal(bits(x), bits(device_solve(prov, Ar, Ai, np.ascontiguousarray(Bt.T), None)))
    # real \ complex with the real matrix a view; the view's base keeps its values
    hat = up(prov, np.ascontiguousarray(Ar.T))
    hav = prov.transpose(hat)
    hc = up(prov, Ai[:, :3].copy(), Ar[:, :3].copy())
    y = take(prov, prov.complex_mldivide(hav, hc))
    assert last_launch(prov)["tuning"] == {"kind": 2, "entry": ref.MLDIVIDE}
    assert np.array_equal(bits(y), bits(device_solve(prov, Ar, None, Ai[:, :3].copy(), Ar[:, :3].copy())))
    assert np.array_equal(prov.download(hat).view(np.uint64), np.ascontiguousarray(Ar.T).ravel(order="F").view(np.uint64))
    for h in (hbt, hbv, ha, hat, hav, hc):
        prov.free(h)


# ---- 6. precision 32 -----------------------------------------------------------------------------------------------------------------------
def f32_round(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


@kinds
@pytest.mark.parametrize("m,n,k", [(3, 3, 2), (33, 33, 1)], ids=shape_id)
def test_f32_provider_rounds_each_part_once(prov, kind, m, n, k):
    """Operands that f32 holds exactly (the real one of a mixed kind lives in f32 storage there): the precision-32 result is the f32
    rounding of the precision-64 result of the same call, part by part - the solve runs in f64 and rounds once, in the join."""
    args = [None if a is None else f32_round(a) for a in ref.operands(np.random.default_rng(60 + kind + n), kind, m, n, k)]
    want = device_solve(prov, *args)
    p32 = HipProvider(0, precision="F32")
    try:
        got = device_solve(p32, *args)
        assert last_launch(p32)["tuning"] == {"kind": kind, "entry": ref.MLDIVIDE}
    finally:
        p32.close()
    assert np.array_equal(bits(got.real.copy()), bits(f32_round(want.real))) and np.array_equal(bits(got.imag.copy()), bits(f32_round(want.imag)))


# ---- 7. a chain ----------------------------------------------------------------------------------------------------------------------------
def test_equalising_a_transform_stays_on_the_device(prov):
    """x = fft(s), y = H * x, H \\ y = x: every intermediate is resident (no upload or download between the first and the last call)."""
    rng = np.random.default_rng(71)
    S, Hr, Hi = rng.standard_normal((64, 3)), rng.standard_normal((64, 64)), rng.standard_normal((64, 64))
    hs, hr, hi = up(prov, S), up(prov, Hr), up(prov, Hi)
    t0 = prov.telemetry_snapshot()
    hx = prov.fft_dim(hs, None, 0)
    hh = prov.complex_from_real_imag(hr, hi)
    hy = prov.complex_matmul(hh, hx)
    hz = prov.complex_mldivide(hh, hy)
    t1 = prov.telemetry_snapshot()
    assert t1["download_bytes"] == t0["download_bytes"] and t1["upload_bytes"] == t0["upload_bytes"]
    assert prov.is_complex(hz) and list(hz.shape) == [64, 3] and last_launch(prov)["tuning"] == {"kind": 0, "entry": ref.MLDIVIDE}
    assert_parity(take(prov, hz), take(prov, hx), "H \\ (H * fft(s))")
    for h in (hs, hr, hi, hh, hy):
        prov.free(h)


# ---- 8. launch log: kind and entry are asserted in the tests above for every kind and entry point ------------------------------------------
def test_two_calls_bitwise_identical_and_inputs_unchanged(prov):
    Ar, Ai, Br, Bi = ref.operands(np.random.default_rng(81), 0, 40, 40, 2)
    ha, hb = up(prov, Ar, Ai), up(prov, Br, Bi)
    x1 = take(prov, prov.complex_mldivide(ha, hb))
    t0 = prov.telemetry_snapshot()
    x2 = take(prov, prov.complex_mldivide(ha, hb))
    assert np.array_equal(bits(x1), bits(x2))
    assert np.array_equal(bits(prov.download(ha)), bits((Ar + 1j * Ai).ravel(order="F")))
    assert np.array_equal(bits(prov.download(hb)), bits((Br + 1j * Bi).ravel(order="F")))
    assert prov.telemetry_snapshot()["mldivide_count"] == t0["mldivide_count"] + 1  # the sibling's timer
    for h in (ha, hb):
        prov.free(h)
