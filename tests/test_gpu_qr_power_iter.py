"""GPU checks of `qr_power_iter` and `take_matmul_sources` (rmhip_qr_power_iter, runmat_amd/csrc/cholqr.hip; rmhip_take_matmul_sources).

The yardstick of every accepted result is numpy's Householder QR of the same matrix (tests/qr_power_ref.py numpy_qr_positive), never the
code under test: orthogonality and residual within 4 x max(numpy's own figure, 4 eps) - the factor 4 covers the different order of the
slice partials - and Q, R within the first-order perturbation bound 16 cond_2(P) eps of numpy's factors.  Every decline is an ordinary
finite-arithmetic outcome (a Cholesky pivot that is not positive and finite, or ||Q1'Q1 - I||_F > 1/2).
"""
import functools

import numpy as np
import pytest

from qr_power_ref import (ACCEPT_CONDS, ACCEPT_SCALE, ACCEPT_SHAPES, EPS, decline_cases, make_case, numpy_qr_positive, orth_error,
                          residual)
from runmat_amd import HipProvider, ProviderError, ProviderQrOptions, ProviderQrPivot
from runmat_amd import _lib

pytestmark = pytest.mark.gpu

ECON = ProviderQrOptions(True, ProviderQrPivot.Matrix())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


@functools.lru_cache(maxsize=None)
def accept_case(m, k, cond):
    """(P, numpy's Q, numpy's R, cond_2(P), numpy's orthogonality error, numpy's residual), computed once and shared (read only)."""
    rng = np.random.default_rng(1000 * m + 10 * k + int(np.log10(cond)))
    P = make_case(m, k, cond, rng, ACCEPT_SCALE)
    Qn, Rn = numpy_qr_positive(P)
    out = (P, Qn, Rn, float(np.linalg.cond(P)), orth_error(Qn), residual(Qn, Rn, P))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def hook(prov, hp, hq, lhs=None, options=ECON):
    """Run the hook; (Q, R, E, pv) as host arrays with the four outputs freed again, or None for a decline."""
    res = prov.qr_power_iter(hp, lhs, hq, options)
    if res is None:
        return None
    hs = (res.q, res.r, res.perm_matrix, res.perm_vector)
    out = tuple(prov.download_matrix(h) for h in hs)
    for h in hs:
        prov.free(h)
    return out


def check_accepted(P, got, ref, label):
    """The issue's conditions on an accepted result; returns the measured figures (printed by the caller before it asserts)."""
    Q, R, E, pv = got
    m, k = P.shape
    _, Qn, Rn, cond2, orth_np, res_np = ref
    assert Q.shape == (m, k) and R.shape == (k, k) and E.shape == (k, k) and pv.shape == (k, 1), label
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0), label
    assert np.array_equal(bits(E), bits(np.eye(k))), label
    assert np.array_equal(bits(pv), bits(np.arange(1, k + 1, dtype=np.float64).reshape(k, 1))), label
    fig = {"orth": orth_error(Q), "orth_np": orth_np, "resid": residual(Q, R, P), "resid_np": res_np,
           "dq": float(np.abs(Q - Qn).max()), "dr": float(np.abs(R - Rn).max() / np.abs(Rn).max()), "cond": cond2}
    print(f"{label}: orth {fig['orth'] / EPS:.2f} eps (numpy {orth_np / EPS:.2f}), resid {fig['resid'] / EPS:.2f} eps (numpy "
          f"{res_np / EPS:.2f}), dQ {fig['dq'] / (cond2 * EPS):.2f} cond eps, dR {fig['dr'] / (cond2 * EPS):.2f} cond eps")
    assert fig["orth"] <= 4.0 * max(orth_np, 4.0 * EPS), (label, fig)
    assert fig["resid"] <= 4.0 * max(res_np, 4.0 * EPS), (label, fig)
    assert fig["dq"] <= 16.0 * cond2 * EPS, (label, fig)
    assert fig["dr"] <= 16.0 * cond2 * EPS, (label, fig)
    return fig


@pytest.mark.parametrize("cond", ACCEPT_CONDS)
@pytest.mark.parametrize("m,k", ACCEPT_SHAPES)
def test_accept_grid(prov, m, k, cond):
    ref = accept_case(m, k, cond)
    P = ref[0]
    q0 = np.full((m, k), 0.25)
    hp, hq = prov.upload(P), prov.upload(q0)
    first = hook(prov, hp, hq)
    assert first is not None, "declined"
    check_accepted(P, first, ref, f"{m}x{k} cond {cond:g}")
    second = hook(prov, hp, hq)
    assert second is not None
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[1]), bits(second[1]))  # same input, same bits
    # no input is freed or written
    assert np.array_equal(bits(prov.download_matrix(hp)), bits(P))
    assert np.array_equal(bits(prov.download_matrix(hq)), bits(q0))
    prov.free(hp)
    prov.free(hq)


def test_pivot_option_only_selects_the_shown_output(prov):
    ref = accept_case(257, 8, 1e3)
    hp, hq = prov.upload(ref[0]), prov.upload(np.zeros((257, 8)))
    a = hook(prov, hp, hq)
    b = hook(prov, hp, hq, options=ProviderQrOptions(True, ProviderQrPivot.Vector()))
    assert a is not None and b is not None
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    prov.free(hp)
    prov.free(hq)


def test_driven_the_way_the_builtin_drives_it(prov):
    """A real matmul product 1024 x 8, then take_matmul_sources, then qr_power_iter with the sources it returned."""
    rng = np.random.default_rng(77)
    A = rng.standard_normal((1024, 1024)) / 32.0
    B, _ = np.linalg.qr(rng.standard_normal((1024, 8)))
    ha, hb = prov.upload(A), prov.upload(B)
    hp = prov.matmul(ha, hb)
    src = prov.take_matmul_sources(hp)
    assert src is not None and src[0].buffer_id == ha.buffer_id and src[1].buffer_id == hb.buffer_id
    assert src[0].shape == (1024, 1024) and src[1].shape == (1024, 8)
    P = prov.download_matrix(hp)
    Qn, Rn = numpy_qr_positive(P)
    ref = (P, Qn, Rn, float(np.linalg.cond(P)), orth_error(Qn), residual(Qn, Rn, P))
    got = hook(prov, hp, src[1], lhs=src[0])
    assert got is not None
    check_accepted(P, got, ref, "matmul 1024x8")
    assert np.array_equal(bits(prov.download_matrix(hp)), bits(P))
    assert np.array_equal(bits(prov.download_matrix(hb)), bits(B)) and np.array_equal(bits(prov.download_matrix(ha)), bits(A))
    for h in (ha, hb, hp):
        prov.free(h)


def fall_through(prov, hp, non_finite_or_huge):
    """What the caller does after a decline: `qr` on the same product.  rmhip_qr's own contract hands a non-finite matrix or one with
    max |a| >= 1e150 on to the host path (UNSUPPORTED); everything else it factors."""
    try:
        res = prov.qr(hp, ECON)
    except ProviderError as e:
        assert non_finite_or_huge and e.code == _lib.ERR_UNSUPPORTED, e
        return
    assert not non_finite_or_huge
    for h in (res.q, res.r, res.perm_matrix, res.perm_vector):
        prov.free(h)


VALUE_DECLINES = ["cond1e10_65x3", "cond1e10_1000x17", "duplicated_column", "zero_column", "all_zero", "scale_1e155", "scale_1e-170",
                  "nan_entry", "inf_entry"]


@pytest.mark.parametrize("name", VALUE_DECLINES)
def test_value_driven_declines(prov, name):
    P = decline_cases(np.random.default_rng(5))[name]
    hp, hq = prov.upload(P), prov.upload(np.zeros(P.shape))
    before = live_bytes(prov)
    assert prov.qr_power_iter(hp, None, hq, ECON) is None
    assert live_bytes(prov) == before  # a decline leaves no buffer behind
    assert np.array_equal(bits(prov.download_matrix(hp)), bits(P))
    fall_through(prov, hp, name in ("scale_1e155", "nan_entry", "inf_entry"))
    prov.free(hp)
    prov.free(hq)


def test_argument_driven_declines(prov):
    rng = np.random.default_rng(6)
    cases = {
        "economy=0": (rng.standard_normal((257, 8)), (257, 8), ProviderQrOptions(False, ProviderQrPivot.Matrix())),
        "m<k": (rng.standard_normal((8, 17)), (8, 17), ECON),
        "k>64": (rng.standard_normal((1000, 65)), (1000, 65), ECON),
        "q_handle of another shape": (rng.standard_normal((257, 8)), (256, 8), ECON),
    }
    for why, (P, qshape, opts) in cases.items():
        hp, hq = prov.upload(P), prov.upload(np.zeros(qshape))
        before = live_bytes(prov)
        assert prov.qr_power_iter(hp, None, hq, opts) is None, why
        assert live_bytes(prov) == before, why
        fall_through(prov, hp, False)
        prov.free(hp)
        prov.free(hq)


def test_errors(prov):
    P = accept_case(65, 3, 1.0)[0]
    hp, hq = prov.upload(P), prov.upload(np.zeros((65, 3)))
    gone = prov.upload(np.zeros((65, 3)))
    prov.free(gone)
    for args in ((gone, None, hq), (hp, gone, hq), (hp, None, gone)):
        with pytest.raises(ProviderError) as e:
            prov.qr_power_iter(*args, ECON)
        assert e.value.code == _lib.ERR_NOT_FOUND
    import ctypes as C

    outs, served = (C.c_uint64 * 4)(), C.c_int()
    assert prov._lib.rmhip_qr_power_iter(prov._ctx, hp.buffer_id, 0, hq.buffer_id, 1, 0, None, C.byref(served)) == _lib.ERR_INVALID
    assert prov._lib.rmhip_qr_power_iter(prov._ctx, hp.buffer_id, 0, hq.buffer_id, 1, 0, outs, None) == _lib.ERR_INVALID
    found = C.c_int()
    assert prov._lib.rmhip_take_matmul_sources(prov._ctx, hp.buffer_id, None, None, C.byref(found)) == _lib.ERR_INVALID
    prov.free(hp)
    prov.free(hq)


def test_take_matmul_sources(prov):
    rng = np.random.default_rng(8)
    A, B = rng.standard_normal((40, 24)), rng.standard_normal((24, 8))
    ha, hb = prov.upload(A), prov.upload(B)
    hp = prov.matmul(ha, hb)
    launches = prov.telemetry_snapshot()["kernel_launches"]
    got = prov.take_matmul_sources(hp)
    again = prov.take_matmul_sources(hp)
    assert prov.telemetry_snapshot()["kernel_launches"] == launches  # no kernel runs
    assert got is not None and (got[0].buffer_id, got[1].buffer_id) == (ha.buffer_id, hb.buffer_id)
    assert again is None  # a take
    prov.free(hp)
    # an operand freed before the take
    ha2 = prov.upload(A)
    hp = prov.matmul(ha2, hb)
    prov.free(ha2)
    assert prov.take_matmul_sources(hp) is None
    prov.free(hp)
    # the product freed before the take
    hp = prov.matmul(ha, hb)
    prov.free(hp)
    assert prov.take_matmul_sources(hp) is None
    # buffers that no matmul made
    assert prov.take_matmul_sources(ha) is None
    he = prov.matmul_epilogue(ha, hb, alpha=2.0)
    assert prov.take_matmul_sources(he) is None
    for h in (he, ha, hb):
        prov.free(h)


def test_power_iteration_end_to_end(prov):
    """40 rounds of P = G Q; [Q, R] = qr(P, 'econ') through the two hooks: diag(R) converges to the four largest eigenvalues."""
    rng = np.random.default_rng(9)
    n, k = 256, 4
    lam = np.concatenate([[1.0, 0.5, 0.25, 0.125], 0.0625 * rng.uniform(0.0, 1.0, n - 4)])  # top-4 gap ratio 0.5
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    G = (V * lam) @ V.T
    G = 0.5 * (G + G.T)
    top = np.sort(np.linalg.eigvalsh(G))[::-1][:k]
    Q0, _ = np.linalg.qr(rng.standard_normal((n, k)))
    hg, hq = prov.upload(G), prov.upload(Q0)
    R = None
    for _ in range(40):
        hp = prov.matmul(hg, hq)
        src = prov.take_matmul_sources(hp)
        assert src is not None and src[1].buffer_id == hq.buffer_id
        res = prov.qr_power_iter(hp, src[0], src[1], ECON)
        assert res is not None, "a round declined"
        prov.free(hp)  # the caller frees the product itself
        prov.free(hq)
        hq = res.q
        R = prov.download_matrix(res.r)
        for h in (res.r, res.perm_matrix, res.perm_vector):
            prov.free(h)
    rel = np.abs(np.diag(R) - top) / top
    print("power iteration: relative error of diag(R)", rel)
    assert np.all(rel <= 1e-10), rel
    prov.free(hq)
    prov.free(hg)


def test_f32_provider():
    """Precision 32: the f64 kernels on a widened copy, outputs rounded to f32 storage.  Rounding unit-norm columns to f32 perturbs each
    inner product by at most 2 * 2^-24; the bound doubles that."""
    rng = np.random.default_rng(10)
    p32 = HipProvider(0, "F32")
    try:
        P = make_case(257, 8, 1e3, rng).astype(np.float32).astype(np.float64)
        hp, hq = p32.upload(P), p32.upload(np.zeros((257, 8)))
        got = hook(p32, hp, hq)
        assert got is not None
        Q, R, E, pv = got
        assert np.array_equal(E, np.eye(8)) and np.array_equal(pv.ravel(), np.arange(1.0, 9.0))
        assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0)
        o, r = orth_error(Q), residual(Q, R, P)
        print(f"f32 provider: orth {o / 2.0 ** -22:.3f} x 2^-22, resid {r / 2.0 ** -22:.3f} x 2^-22")
        assert o <= 2.0 ** -22 and r <= 2.0 ** -22
        assert np.array_equal(bits(p32.download_matrix(hp)), bits(P))
        p32.free(hp)
        p32.free(hq)
    finally:
        p32.close()
