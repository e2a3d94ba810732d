"""GPU checks of `pagefun(@mtimes)` (rmhip_pagefun; runmat_amd/csrc/pagefun.hip, dgemm.hip k_pgemm_w8) against the numpy restatement of
the host builtin (tests/pagefun_host.py): tiny pages bit-exact, matrix-core tiers within k eps sum|a||b|, the tier read from the launch
log on both sides of every boundary."""
import json
from pathlib import Path

import numpy as np
import pytest

from pagefun_host import build_request, pagefun_host
from runmat_amd import HipProvider, PagefunOp, PagefunRequest, ProviderError
from runmat_amd import _lib

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KATS = json.loads((Path(__file__).resolve().parent / "golden" / "pagefun_kats.json").read_text())
SIDES = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33)


def request(prov_handles, lhs_shape, rhs_shape):
    r = build_request(lhs_shape, rhs_shape)
    return PagefunRequest(PagefunOp.Mtimes, list(prov_handles), r.output_shape, r.page_dims, r.input_page_dims)


def last_tier(prov):
    log = [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "pagefun"]
    return log[-1]["tuning"]["tier"]


def run(prov, A, B, keep=False):
    ha, hb = prov.upload(A.ravel(order="F"), A.shape), prov.upload(B.ravel(order="F"), B.shape)
    hc = prov.pagefun(request([ha, hb], A.shape, B.shape))
    tier = last_tier(prov) if np.prod(hc.shape) else None
    C = prov.download(hc).reshape(hc.shape, order="F")
    assert list(hc.shape) == build_request(A.shape, B.shape).output_shape
    for h in (ha, hb, hc):
        prov.free(h)
    return C, tier


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_bitwise(got, want):
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want))


def assert_bound(got, A, B, want):
    r = build_request(A.shape, B.shape)
    bound = pagefun_host(np.abs(A), np.abs(B)) * max(r.k, 1) * EPS
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= bound), np.max(np.abs(got - want) - bound)


def rand(rng, shape, ints=False):
    if ints:
        return rng.integers(-4, 5, size=shape).astype(np.float64)
    return rng.standard_normal(shape)


# ---- the reference's unit tests -----------------------------------------------------------------------------------------------------
def arr(spec):
    return np.array(spec["data"], dtype=np.float64).reshape(spec["shape"], order="F")


@pytest.mark.parametrize("kat", KATS["products"], ids=lambda k: k["name"])
def test_reference_products(prov, kat):
    C, _ = run(prov, arr(kat["lhs"]), arr(kat["rhs"]))
    assert list(C.shape) == kat["out"]["shape"]
    assert C.ravel(order="F").tolist() == kat["out"]["data"]


@pytest.mark.parametrize("kat", KATS["errors"], ids=lambda k: k["name"])
def test_reference_errors(prov, kat):
    A, B = arr(kat["lhs"]), arr(kat["rhs"])
    ha, hb = prov.upload(A.ravel(order="F"), A.shape), prov.upload(B.ravel(order="F"), B.shape)
    # the request as a caller that skipped the builtin's checks would pass it: the provider refuses with SHAPE
    pd = [max(a, b) for a, b in zip(list(A.shape[2:]) + [1], list(B.shape[2:]) + [1])][:max(A.ndim, B.ndim) - 2]
    ipd = [list(A.shape[2:]) + [1] * (len(pd) - (A.ndim - 2)), list(B.shape[2:]) + [1] * (len(pd) - (B.ndim - 2))]
    with pytest.raises(ProviderError) as e:
        prov.pagefun(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [A.shape[0], B.shape[1]] + pd, pd, ipd))
    assert e.value.code == _lib.ERR_SHAPE
    prov.free(ha)
    prov.free(hb)


# ---- tiny tier: bit-exact ------------------------------------------------------------------------------------------------------------
def test_tiny_sweep_bitwise(prov):
    rng = np.random.default_rng(1)
    for m in SIDES:
        for n in SIDES:
            for k in SIDES:
                A, B = rand(rng, (m, k, 3)), rand(rng, (k, n, 3))
                C, tier = run(prov, A, B)
                want = pagefun_host(A, B)
                if max(m, n, k) <= 32:
                    assert tier == 2, (m, n, k)
                    assert_bitwise(C, want)
                else:
                    assert tier == 3, (m, n, k)
                    assert_bound(C, A, B, want)


def test_tiny_special_values_bitwise(prov):
    rng = np.random.default_rng(2)
    A, B = rand(rng, (5, 4, 6)), rand(rng, (4, 3, 6))
    A[:, :, 0], B[:, :, 0] = -0.0, 1.0  # every product -0.0: +0.0
    A[:, :, 1], B[:, :, 1] = 0.0, -1.0
    A[1, 2, 2] = np.nan
    A[0, 0, 3] = np.inf
    B[3, 1, 4] = -np.inf
    A[2, 1, 5], B[1, 2, 5] = np.inf, 0.0  # inf * 0
    C, tier = run(prov, A, B)
    assert tier == 2
    want = pagefun_host(A, B)
    assert not np.any(np.signbit(C[:, :, 0]))
    assert_bitwise(C, want)


# ---- matrix-core tiers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,p,tier", [(33, 33, 33, 5, 3), (64, 64, 64, 7, 3), (100, 40, 70, 3, 3), (255, 300, 64, 2, 3),
                                          (256, 256, 256, 2, 4), (300, 257, 129, 3, 4), (513, 260, 37, 2, 4)])
def test_mfma_tiers_bound_and_exact_integers(prov, m, n, k, p, tier):
    rng = np.random.default_rng(m * 7 + n)
    A, B = rand(rng, (m, k, p)), rand(rng, (k, n, p))
    C, t = run(prov, A, B)
    assert t == tier
    assert_bound(C, A, B, pagefun_host(A, B))
    A, B = rand(rng, (m, k, p), ints=True), rand(rng, (k, n, p), ints=True)
    C, t = run(prov, A, B)
    assert t == tier
    assert_bitwise(C, pagefun_host(A, B))


@pytest.mark.parametrize("m,n,k,tier", [(32, 32, 32, 2), (33, 32, 32, 3), (32, 33, 32, 3), (32, 32, 33, 3), (255, 256, 8, 3),
                                        (256, 255, 8, 3), (256, 256, 8, 4), (256, 256, 1, 4)])
def test_tier_boundaries(prov, m, n, k, tier):
    rng = np.random.default_rng(5)
    A, B = rand(rng, (m, k, 2), ints=True), rand(rng, (k, n, 2), ints=True)
    C, t = run(prov, A, B)
    assert t == tier
    assert_bitwise(C, pagefun_host(A, B))


@pytest.mark.parametrize("m,n,k", [(4, 4, 4), (40, 40, 40), (300, 300, 20)])
def test_shared_lhs_tier_is_the_reshaped_matmul(prov, m, n, k):
    rng = np.random.default_rng(6)
    P = 9
    A, B = rand(rng, (m, k)), rand(rng, (k, n, P))
    ha, hb = prov.upload(A.ravel(order="F"), A.shape), prov.upload(B.ravel(order="F"), B.shape)
    hc = prov.pagefun(request([ha, hb], A.shape, B.shape))
    assert last_tier(prov) == 1
    hb2 = prov.upload(B.ravel(order="F"), (k, n * P))
    hm = prov.matmul(ha, hb2)
    assert_bitwise(prov.download(hc), prov.download(hm))
    assert_bound(prov.download(hc).reshape((m, n, P), order="F"), A, B, pagefun_host(A, B))
    for h in (ha, hb, hc, hb2, hm):
        prov.free(h)


# ---- broadcasting --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lhs_pages,rhs_pages", [((5,), (5,)), ((1,), (5,)), ((5,), (1,)), ((3, 1), (1, 4)), ((2, 3, 4), (2, 1, 4)),
                                                 ((2, 1, 3, 2), (1, 2, 3, 1)), ((2, 1, 3, 1, 2, 2), (1, 2, 3, 2, 1, 2))])
@pytest.mark.parametrize("m,n,k", [(4, 3, 5), (40, 36, 20)])
def test_broadcast_patterns(prov, lhs_pages, rhs_pages, m, n, k):
    rng = np.random.default_rng(7)
    A, B = rand(rng, (m, k) + lhs_pages), rand(rng, (k, n) + rhs_pages)
    C, tier = run(prov, A, B)
    want = pagefun_host(A, B)
    if max(m, n, k) <= 32 and tier == 2:
        assert_bitwise(C, want)
    else:
        assert_bound(C, A, B, want)
    if np.prod(lhs_pages) == 1:
        assert tier == 1
    else:
        assert tier == (2 if max(m, n, k) <= 32 else 3)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def test_more_than_65535_pages(prov):
    rng = np.random.default_rng(8)
    A, B = rand(rng, (3, 3, 100000)), rand(rng, (3, 3, 100000))
    C, tier = run(prov, A, B)
    assert tier == 2
    assert_bitwise(C, pagefun_host(A, B))
    A, B = rand(rng, (33, 2, 70000), ints=True), rand(rng, (2, 33, 70000), ints=True)
    C, tier = run(prov, A, B)
    assert tier == 3
    assert_bitwise(C, pagefun_host(A, B))


def test_operand_larger_than_4gib(prov):
    P = (1 << 25) + (1 << 20)  # 16 P doubles: 4.4 GB in A and in C
    ha = prov.random_uniform([4, 4, P])
    rng = np.random.default_rng(9)
    B = rand(rng, (4, 4))
    hb = prov.upload(B.ravel(order="F"), B.shape)
    hc = prov.pagefun(request([ha, hb], [4, 4, P], [4, 4]))
    assert last_tier(prov) == 2
    sample = np.array([0, 1, 12345, (1 << 25) - 1, 1 << 25, (1 << 25) + 7, P - 2, P - 1], dtype=np.int64)
    idx = (sample[:, None] * 16 + np.arange(16)[None, :]).ravel()
    hga = prov.gather_linear(ha, idx, [4, 4, len(sample)])
    hgc = prov.gather_linear(hc, idx, [4, 4, len(sample)])
    A_s = prov.download(hga).reshape((4, 4, len(sample)), order="F")
    C_s = prov.download(hgc).reshape((4, 4, len(sample)), order="F")
    assert_bitwise(C_s, pagefun_host(A_s, B))
    for h in (ha, hb, hc, hga, hgc):
        prov.free(h)


def test_empties_and_k_zero(prov):
    for lhs, rhs in [((2, 2, 0), (2, 2, 0)), ((0, 3, 4), (3, 2, 4)), ((3, 2, 4), (2, 0, 4)), ((2, 2, 0), (2, 2, 5)), ((2, 2, 3, 0), (2, 2))]:
        A, B = np.zeros(lhs), np.zeros(rhs)
        C, _ = run(prov, A, B)
        assert list(C.shape) == build_request(lhs, rhs).output_shape and C.size == 0
    rng = np.random.default_rng(10)
    for lhs, rhs in [((3, 0, 4), (0, 5, 4)), ((40, 0, 2), (0, 300, 2)), ((3, 0), (0, 5, 6))]:
        A, B = rand(rng, lhs), rand(rng, rhs)
        C, _ = run(prov, A, B)
        assert_bitwise(C, pagefun_host(A, B))
        assert C.size and np.all(C == 0.0) and not np.any(np.signbit(C))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(prov):
    rng = np.random.default_rng(11)
    A, B = rand(rng, (3, 4, 2)), rand(rng, (4, 5, 2))
    ha, hb = prov.upload(A.ravel(order="F"), A.shape), prov.upload(B.ravel(order="F"), B.shape)

    def code(req):
        with pytest.raises(ProviderError) as e:
            prov.pagefun(req)
        return e.value.code

    ok = request([ha, hb], A.shape, B.shape)
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha], [3, 4, 2], [2], [[2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb, hb], ok.output_shape, [2], [[2], [2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], ok.output_shape, [2], [[2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [hb, ha], [4, 4, 2], [2], [[2], [2]])) == _lib.ERR_SHAPE  # 4x5 * 3x4
    hb3 = prov.upload(rand(rng, (4, 5, 3)), (4, 5, 3))
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb3], [3, 5, 3], [3], [[2], [3]])) == _lib.ERR_SHAPE
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 3], [2], [[2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5], [2], [[2], [2]])) == _lib.ERR_INVALID
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 3], [3], [[3], [3]])) == _lib.ERR_INVALID  # 24 elements, not 36
    assert code(PagefunRequest(PagefunOp.Mtimes, [ha, hb], [3, 5, 2], [1], [[2], [2]])) == _lib.ERR_INVALID  # page_dims disagree
    hz = prov.complex_from_real(ha)
    assert code(PagefunRequest(PagefunOp.Mtimes, [hz, hb], ok.output_shape, ok.page_dims, ok.input_page_dims)) == _lib.ERR_UNSUPPORTED
    assert code(PagefunRequest("mrdivide", [ha, hb], ok.output_shape, ok.page_dims, ok.input_page_dims)) == _lib.ERR_UNSUPPORTED
    for h in (ha, hb, hb3, hz):
        prov.free(h)


# ---- lazy operands -------------------------------------------------------------------------------------------------------------------
def test_transpose_repmat_and_lazy_normal_operands(prov):
    rng = np.random.default_rng(12)
    At = rand(rng, (6, 5))  # A = At' is 5 x 6
    B = rand(rng, (6, 4, 7))
    hat, hb = prov.upload(At.ravel(order="F"), At.shape), prov.upload(B.ravel(order="F"), B.shape)
    ha = prov.transpose(hat)
    hc = prov.pagefun(request([ha, hb], [5, 6], B.shape))
    assert_bound(prov.download(hc).reshape((5, 4, 7), order="F"), At.T.copy(), B, pagefun_host(At.T.copy(), B))
    # a transposed right operand on the tiny tier: bit-exact
    P = rand(rng, (5, 6, 3))
    hp = prov.upload(P.ravel(order="F"), P.shape)
    Bt = rand(rng, (3, 6))
    hbt = prov.upload(Bt.ravel(order="F"), Bt.shape)
    hbv = prov.transpose(hbt)
    hd = prov.pagefun(request([hp, hbv], P.shape, [6, 3]))
    assert last_tier(prov) == 2
    assert_bitwise(prov.download(hd).reshape((5, 3, 3), order="F"), pagefun_host(P, Bt.T.copy()))
    # repmat view: [3 x 4] tiled to [3, 4, 5]
    R = rand(rng, (3, 4))
    hr = prov.upload(R.ravel(order="F"), R.shape)
    hrv = prov.repmat(hr, [1, 1, 5])
    Q = rand(rng, (4, 2, 5))
    hq = prov.upload(Q.ravel(order="F"), Q.shape)
    he = prov.pagefun(request([hrv, hq], [3, 4, 5], Q.shape))
    assert_bitwise(prov.download(he).reshape((3, 2, 5), order="F"), pagefun_host(np.repeat(R[:, :, None], 5, axis=2), Q))
    # lazy random_normal operands (settled first; the handle then holds the values the product used)
    hn = prov.random_normal([4, 3, 1000])
    hm = prov.random_normal([3, 5, 1000])
    hf = prov.pagefun(request([hn, hm], [4, 3, 1000], [3, 5, 1000]))
    N, M = prov.download(hn).reshape((4, 3, 1000), order="F"), prov.download(hm).reshape((3, 5, 1000), order="F")
    assert_bitwise(prov.download(hf).reshape((4, 5, 1000), order="F"), pagefun_host(N, M))
    for h in (hat, hb, ha, hc, hp, hbt, hbv, hd, hr, hrv, hq, he, hn, hm, hf):
        prov.free(h)


# ---- precision 32 --------------------------------------------------------------------------------------------------------------------
def test_f32_provider_rounds_once():
    p32 = HipProvider(0, precision="F32")
    try:
        rng = np.random.default_rng(13)
        for (m, n, k, p), exact in [((5, 4, 3, 50), True), ((40, 33, 20, 3), False)]:
            A = rand(rng, (m, k, p)).astype(np.float32).astype(np.float64)
            B = rand(rng, (k, n, p)).astype(np.float32).astype(np.float64)
            ha, hb = p32.upload(A.ravel(order="F"), A.shape), p32.upload(B.ravel(order="F"), B.shape)
            hc = p32.pagefun(request([ha, hb], A.shape, B.shape))
            C = p32.download(hc).reshape((m, n, p), order="F")
            want = pagefun_host(A, B)
            if exact:
                assert_bitwise(C, want.astype(np.float32).astype(np.float64))
            else:
                assert np.all(np.abs(C - want) <= pagefun_host(np.abs(A), np.abs(B)) * (k * EPS + 2.0 ** -24))
            for h in (ha, hb, hc):
                p32.free(h)
    finally:
        p32.close()


# ---- determinism, inputs, host traffic and launches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,lhs_pages", [(4, 4, 4, 1000), (40, 40, 40, 50), (260, 270, 100, 2), (20, 20, 20, 1)])
def test_two_calls_bitwise_identical_and_inputs_unchanged(prov, m, n, k, lhs_pages):
    rng = np.random.default_rng(14)
    A, B = rand(rng, (m, k, lhs_pages)), rand(rng, (k, n, 1000 if lhs_pages in (1, 1000) else lhs_pages))
    ha, hb = prov.upload(A.ravel(order="F"), A.shape), prov.upload(B.ravel(order="F"), B.shape)
    req = request([ha, hb], A.shape, B.shape)
    h1, h2 = prov.pagefun(req), prov.pagefun(req)
    assert_bitwise(prov.download(h1), prov.download(h2))
    assert_bitwise(prov.download(ha).reshape(A.shape, order="F"), A)
    assert_bitwise(prov.download(hb).reshape(B.shape, order="F"), B)
    for h in (ha, hb, h1, h2):
        prov.free(h)


@pytest.mark.parametrize("m,k,n,shared", [(4, 4, 4, False), (16, 16, 16, False), (40, 40, 40, False), (4, 4, 4, True)])
def test_no_host_read_and_at_most_two_launches(prov, m, k, n, shared):
    P = 100000 if max(m, n, k) <= 16 else 2000
    ha = prov.random_uniform([m, k] + ([] if shared else [P]))
    hb = prov.random_uniform([k, n, P])
    req = request([ha, hb], ha.shape, hb.shape)
    prov.free(prov.pagefun(req))  # warm
    t0 = prov.telemetry_snapshot()
    hc = prov.pagefun(req)
    t1 = prov.telemetry_snapshot()
    assert t1["download_bytes"] == t0["download_bytes"]
    assert 1 <= t1["kernel_launches"] - t0["kernel_launches"] <= 2
    for h in (ha, hb, hc):
        prov.free(h)
