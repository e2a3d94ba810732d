"""tests/gemm_ref.py on the host (CPU only): the integer reference is exact for the stated operand ranges in f64 and f32, in any
association order; the frames are what they claim; and every row of the route tables has the divisibility and alignment properties
its route name claims under the launchers' rules (dgemm.hip launch_dgemm_impl, sgemm.hip launch_sgemm_trans) at 256 compute units."""
import numpy as np
import pytest

import gemm_ref as G

TILE, SMALL_TILE, KT = 128, 64, 16


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dtype,top", [(64, np.float64, 8), (32, np.float32, 4)])
def test_integer_reference_is_exact_in_every_accumulation_order(bits, dtype, top):
    rng = np.random.default_rng(11)
    k = G.K_MAX
    A, B = G.operand(rng, 24, k, bits), G.operand(rng, k, 20, bits)
    assert np.all(A != 0) and np.all(B != 0) and np.abs(A).max() == top and np.abs(B).max() == top
    assert set(np.unique(np.abs(A))) == set(range(1, top + 1))
    P = G.exact_product(A, B)
    assert P.dtype == np.int64
    # the worst case stays inside the format's integer range
    assert top * top * k < (2 ** 53 if bits == 64 else 2 ** 24)
    a, b = A.astype(dtype), B.astype(dtype)
    assert np.array_equal(a.astype(np.float64), A)
    terms = a[:, :, None] * b[None, :, :]  # [i, k, j], every product exact in `dtype`
    assert terms.dtype == dtype and np.array_equal(terms.astype(np.int64).sum(axis=1), P)
    orders = {
        "forward": lambda t: np.add.accumulate(t, axis=1, dtype=dtype)[:, -1, :],
        "backward": lambda t: np.add.accumulate(t[:, ::-1, :], axis=1, dtype=dtype)[:, -1, :],
        "pairwise": lambda t: t.sum(axis=1, dtype=dtype),
        "slices of 128": lambda t: sum((t[:, s:s + 128, :].sum(axis=1, dtype=dtype) for s in range(0, k, 128)), np.zeros((24, 20), dtype)),
        "four interleaved chains": lambda t: sum((np.add.accumulate(t[:, s::4, :], axis=1, dtype=dtype)[:, -1, :] for s in range(4)),
                                                 np.zeros((24, 20), dtype)),
        "permuted": lambda t: np.add.accumulate(t[:, np.random.default_rng(5).permutation(k), :], axis=1, dtype=dtype)[:, -1, :],
    }
    for name, f in orders.items():
        got = f(terms)
        assert got.dtype == dtype and np.array_equal(got.astype(np.int64), P), name
    assert np.array_equal((a @ b).astype(np.int64), P)  # BLAS, whatever its order
    # the all-maximal operand reaches the bound and is still exact
    worst = np.full((1, k), float(top), dtype) @ np.full((k, 1), float(top), dtype)
    assert worst.dtype == dtype and int(worst[0, 0]) == top * top * k


def test_scalars_and_the_clamped_epilogue_stay_exact():
    rng = np.random.default_rng(3)
    A, B = G.operand(rng, 40, G.K_MAX), G.operand(rng, G.K_MAX, 30)
    P = G.exact_product(A, B)
    from fractions import Fraction

    C0 = G.operand(rng, 40, 30)
    for alpha in G.ALPHAS:
        for beta in G.ALPHAS:
            got = alpha * P.astype(np.float64) + beta * C0
            i, j = 7, 11
            assert Fraction(float(got[i, j])) == Fraction(alpha) * int(P[i, j]) + Fraction(beta) * Fraction(float(C0[i, j]))
            assert np.all(got == np.round(got * 2) / 2)  # halves at the finest
    c = G.case("epilogue", 40, 30, G.K_MAX, "w8g guard epi1")
    rs, cs = G.epilogue_scales(c)
    v = G.epilogue_exact(P, rs, cs)
    want = [[min(max((Fraction(int(P[i, j])) * Fraction(1, 2) - 2) * Fraction(float(rs[i, 0])) / Fraction(float(cs[0, j])),
                     Fraction(-32)), Fraction(48)) for j in range(30)] for i in range(40)]
    assert all(Fraction(float(v[i, j])) == want[i][j] for i in range(40) for j in range(30))
    assert (v == -32).any() and (v == 48).any() and ((v > -32) & (v < 48)).any()  # both clamps and the middle are exercised


def test_frames_hold_what_they_claim():
    c = G.case("blk", 65, 63, 17, "small guard", alpha=2.0, beta=-1.0, fa=G.ODD_BASE)
    A, B, P = G.operands(c)
    pa, va, pb, vb, pc, vc, want = G.framed(c, A, B, P)
    assert pa.shape == (3 + 65 + 1, 1 + 17 + 1) and va == (3, 1, 65, 17) and vb == (2, 1, 17, 63) and vc == (2, 1, 65, 63)
    inside = np.zeros(pa.shape, bool)
    inside[3:68, 1:18] = True
    assert np.isnan(pa[~inside]).all() and np.array_equal(pa[inside].reshape(65, 17), A)
    assert not np.isnan(pc).any() and not np.isnan(want).any()
    out = np.ones(pc.shape, bool)
    out[2:67, 1:64] = False
    assert G.same_bits(pc[out], want[out]) and len(np.unique(pc[out])) == out.sum() and np.all(pc[out] <= -1e6)
    assert np.array_equal(want[2:67, 1:64], 2.0 * P - pc[2:67, 1:64])
    c0 = G.case("blk", 64, 64, 16, "small", alpha=1.0, beta=0.0)
    _, _, _, _, pc0, _, want0 = G.framed(c0, *G.operands(c0))
    assert np.isnan(pc0[2:66, 1:65]).all() and not np.isnan(want0).any()  # beta == 0: the old C must not be read
    assert not G.same_bits(np.array([0.0]), np.array([-0.0])) and G.same_bits(np.array([1.5, np.nan]), np.array([1.5, np.nan]))


# ---- the tables against the launchers' rules --------------------------------------------------------------------------------------------
def layout(c):
    """(lda, ldb, A base even, B base even) in elements, as the entry point hands them to the launcher."""
    m, n, k, e = c["m"], c["n"], c["k"], c["entry"]
    if e == "blk":
        fa, fb = c.get("fa", G.EVEN), c.get("fb", G.EVEN)
        lda, ldb = fa[0] + m + fa[2], fb[0] + k + fb[2]
        return lda, ldb, (fa[0] + fa[1] * lda) % 2 == 0, (fb[0] + fb[1] * ldb) % 2 == 0
    ta, tb = e in ("matmul_ta", "syrk"), e == "matmul_tb"
    return (k if ta else m), (n if tb else k), True, True  # whole buffers: allocations are at least 16-byte aligned


def model(c, knobs=None, bits=64):
    """The route the launchers' conditions give for a case at G.NUM_CUS compute units, outside the look-ahead LU.  This is a MIRROR of
    launch_dgemm_impl / launch_sgemm_trans, kept in step with them by hand - a threshold that moves there moves here too - and not an
    independent specification: it says why a row has its route (which divisibility, alignment or block-count rule), while what
    actually runs is decided by tests/test_gpu_gemm_paths.py against the launcher's own record."""
    knobs = knobs or {}
    m, n, k, e = c["m"], c["n"], c["k"], c["entry"]
    ta, tb, ep = e in ("matmul_ta", "syrk"), e == "matmul_tb", e == "epilogue"
    epi = (2 if "pow" in c else 1) if ep else 0
    if e == "pagefun":
        assert m >= 256 and n >= 256 and max(m, n, k) > 32 and c["pages"] > 1  # rmhip_pagefun's tier 4
        return G.route("pgemm guard", 1, k)
    lda, ldb, a_even, b_even = layout(c)
    vec_ok = lda % 2 == 0 and ldb % 2 == 0 and a_even and b_even  # f32: 8-byte alignment of 4-byte elements, the same parity rule
    fast = m % TILE == 0 and n % TILE == 0 and k % KT == 0 and k > 0 and vec_ok
    blocks = -(-m // TILE) * -(-n // TILE)
    splits, chunk = 1, k
    if not ep and blocks * 4 <= G.NUM_CUS and k >= 1024:
        want = -(-2 * G.NUM_CUS // blocks)
        gran = 1024 if k >= 8192 else 256 if k >= 2048 else 128
        ch = -(--(-k // want) // gran) * gran
        if -(-k // ch) > 1:
            splits, chunk = -(-k // ch), ch
    fast_k = fast and (splits == 1 or k % chunk == 0)
    guard_on = knobs.get("RMHIP_GEMM_GUARD", "1") != "0"
    if bits == 32:
        w8 = knobs.get("RMHIP_SGEMM_W8", "1") != "0"
        if not fast and guard_on and w8 and not tb and splits == 1 and k >= 1:
            return G.route("s_w8g guard" + (" ta" if ta else ""), 1, k)
        if fast_k and splits == 1 and w8 and not tb:
            return G.route("s_w8" + (" ta" if ta else ""), 1, k)
        return G.route("s_w4" + ("" if fast_k else " edge") + (" ta" if ta else "") + (" tb" if tb else ""), splits, chunk)
    alpha, beta = c.get("alpha", 1.0), c.get("beta", 0.0)
    preload = knobs.get("RMHIP_GEMM_PRELOAD", "1") != "0" and not (ep or ta or tb) and splits == 1 and alpha == -1.0 and beta == 1.0 and k > 0
    w8_on = knobs.get("RMHIP_GEMM_W8", "1") != "0"
    guard_ok = guard_on and not tb and k >= 1
    skinny = (m <= SMALL_TILE or n <= SMALL_TILE) and k < 1024
    small_shape = not (ep or ta or tb) and splits == 1 and k > 0 and ((k <= 1024 and blocks * 2 <= G.NUM_CUS) or skinny)
    small_whole = m % SMALL_TILE == 0 and n % SMALL_TILE == 0 and k % KT == 0 and vec_ok
    pre = " pre" if preload else ""
    if knobs.get("RMHIP_GEMM_SMALL", "1") != "0" and small_shape and (small_whole or guard_ok):
        return G.route("small" + ("" if small_whole else " guard") + pre, 1, k)
    w8_fast = fast and chunk % KT == 0
    if w8_fast and ep and w8_on:
        return G.route(f"w8 epi{epi}", 1, k)
    if w8_fast and ta and w8_on:
        return G.route("w8 ta", splits, chunk)
    if w8_fast and splits > 1 and not tb and w8_on:
        return G.route("w8", splits, chunk)
    if fast_k and splits == 1 and not (ep or ta or tb) and w8_on:
        return G.route("w8" + pre, 1, k)
    if not fast and guard_ok and w8_on and (splits == 1 or chunk % KT == 0):
        return G.route("w8g guard" + (f" epi{epi}" if ep else " ta" if ta else pre), splits, chunk)
    if ep:
        return G.route(f"w4 edge epi{epi}", splits, chunk)
    if ta or tb:
        return G.route("w4" + ("" if fast_k else " edge") + (" ta" if ta else " tb"), splits, chunk)
    return G.route("w4" + (pre if fast_k and preload else "" if fast_k else " edge"), splits, chunk)


def test_case_ids_are_unique_and_k_stays_exact():
    for table in [G.F64_CASES, G.F32_CASES, *G.KNOB_CASES.values(), *G.F32_KNOB_CASES.values()]:
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
        for c in table:
            assert 1 <= c["k"] <= G.K_MAX and c["m"] * c["n"] <= 2049 * 1153, c["id"]  # exact sums; a download of at most 2049 x 1153
            assert 2.0 * c["m"] * c["n"] * c["k"] * c.get("pages", 1) <= 4e9, c["id"]  # a few GFLOP at most


@pytest.mark.parametrize("c", G.F64_CASES, ids=lambda c: c["id"])
def test_f64_rows_have_the_properties_their_routes_claim(c):
    assert model(c) == c["route"], (model(c), c["route"])


@pytest.mark.parametrize("knob", sorted(G.KNOB_CASES))
def test_knob_rows_have_the_properties_their_routes_claim(knob):
    for c in G.KNOB_CASES[knob]:
        assert model(c, {knob: "0"}) == c["route"], (c["id"], model(c, {knob: "0"}))
    # and the setting is what selects them: all but the anchor rows of a table route elsewhere by default
    assert sum(model(c) != c["route"] for c in G.KNOB_CASES[knob]) >= len(G.KNOB_CASES[knob]) - 2


@pytest.mark.parametrize("c", G.F32_CASES, ids=lambda c: c["id"])
def test_f32_rows_have_the_properties_their_routes_claim(c):
    assert model(c, bits=32) == c["route"], (model(c, bits=32), c["route"])


def test_f32_knob_rows_have_the_properties_their_routes_claim():
    for c in G.F32_KNOB_CASES["RMHIP_SGEMM_W8"]:
        assert model(c, {"RMHIP_SGEMM_W8": "0"}, bits=32) == c["route"], c["id"]


def test_the_tables_cover_every_instantiation_reachable_from_the_abi():
    """Kernel and template flags of every launch site in launch_dgemm_impl, launch_pgemm_w8 and launch_sgemm_trans, with and without
    split-K; the three that only the look-ahead LU selects (k_dgemm_w8p, the YIELD form, the upd_small rule) are not reachable here."""
    def keys(tables):
        return {(c["route"]["kernel"], c["route"]["guard"], c["route"]["pre"], c["route"]["ta"], c["route"]["tb"], c["route"]["epi"],
                 c["route"]["splits"] > 1) for t in tables for c in t}

    f64 = keys([G.F64_CASES, *G.KNOB_CASES.values()])
    want = {("small", g, p, 0, 0, 0, False) for g in (0, 1) for p in (0, 1)}
    want |= {("w8", 0, p, 0, 0, 0, False) for p in (0, 1)} | {("w8", 0, 0, 0, 0, 0, True)}
    want |= {("w8", 0, 0, 1, 0, 0, s) for s in (False, True)} | {("w8", 0, 0, 0, 0, e, False) for e in (1, 2)}
    want |= {("w8g", 1, p, 0, 0, 0, False) for p in (0, 1)} | {("w8g", 1, 0, 0, 0, 0, True)}
    want |= {("w8g", 1, 0, 1, 0, 0, s) for s in (False, True)} | {("w8g", 1, 0, 0, 0, e, False) for e in (1, 2)}
    want |= {("w4", g, 0, ta, 1 - ta, 0, s) for g in (0, 1) for ta in (0, 1) for s in (False, True)}  # A' or B', whole / edge, +- split
    want |= {("w4", g, 0, 0, 0, 0, s) for g in (0, 1) for s in (False, True)} | {("w4", 0, 1, 0, 0, 0, False)}
    want |= {("w4", 1, 0, 0, 0, e, False) for e in (1, 2)} | {("pgemm", 1, 0, 0, 0, 0, False)}
    assert want <= f64, sorted(want - f64)
    f32 = keys([G.F32_CASES, *G.F32_KNOB_CASES.values()])
    want32 = {("s_w8", 0, 0, ta, 0, 0, False) for ta in (0, 1)} | {("s_w8g", 1, 0, ta, 0, 0, False) for ta in (0, 1)}
    want32 |= {("s_w4", g, 0, ta, tb, 0, s) for g in (0, 1) for ta, tb in ((0, 0), (1, 0), (0, 1)) for s in (False, True)}
    assert want32 <= f32, sorted(want32 - f32)
