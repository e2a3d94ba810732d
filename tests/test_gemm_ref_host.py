"""tests/gemm_ref.py on the host (CPU only): the integer reference is exact for the stated operand ranges in f64 and f32, in any
association order; the frames are what they claim; and every row of the route tables has the divisibility and alignment properties
its route name claims under the launchers' own rule - gemm_plan.h plan_dgemm / plan_sgemm, run through tests/cpp/gemm_route_check.cpp -
at 256 compute units; and the routes that only the look-ahead LU's sites select."""
import numpy as np
import pytest

import gemm_ref as G

TILE, SMALL_TILE = 128, 64


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


ABI = dict(num_cus=G.NUM_CUS, in_lookahead=0, lds_pad=0, chain_prio=0, counter=0, yield_word=0, small_upd=1024)
KNOB_ORDER = ("RMHIP_GEMM_SMALL", "RMHIP_GEMM_W8", "RMHIP_GEMM_PRELOAD", "RMHIP_GEMM_GUARD", "RMHIP_SGEMM_W8")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """The launchers' own rule: tests/cpp/gemm_route_check.cpp --table runs plan_dgemm / plan_sgemm (runmat_amd/csrc/gemm_plan.h), the
    function launch_dgemm_impl and launch_sgemm_trans execute.  plan(rows) takes (case, knobs, bits, site) tuples and returns, per row,
    the route as rmhip_gemm_last_route would report it plus tiles_m, tiles_n and prio, or {"unsupported": message}."""
    import subprocess

    from test_host_plan import compile_check

    exe = compile_check(tmp_path_factory.mktemp("gemm_route_check"), "gemm_route_check")

    def run(rows):
        lines = []
        for c, knobs, bits, site in rows:
            e = c["entry"]
            ta, tb = c.get("ta", e in ("matmul_ta", "syrk")), c.get("tb", e == "matmul_tb")
            epi = c.get("epi", ((2 if "pow" in c else 1) if e == "epilogue" else 0))
            lda, ldb, a_even, b_even = layout(c)  # f32: 8-byte alignment of 4-byte elements, the same parity rule
            s = dict(ABI, **(site or {}))
            on = [int((knobs or {}).get(k, "1") != "0") for k in KNOB_ORDER]
            lines.append(" ".join(str(x) for x in [bits, c["m"], c["n"], c["k"], lda, ldb, int(a_even), int(b_even), int(ta), int(tb), epi,
                                                   c.get("alpha", 1.0), c.get("beta", 0.0), *s.values(), *on]))
        r = subprocess.run([str(exe), "--table"], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = []
        for ln in r.stdout.splitlines():
            if ln.startswith("unsupported: "):
                out.append({"unsupported": ln[len("unsupported: "):]})
                continue
            w = ln.split()
            keys = ("guard", "pre", "ta", "tb", "epi", "yield", "splits", "k_chunk", "tiles_m", "tiles_n", "prio")
            out.append({"kernel": w[0], **{k: int(v) for k, v in zip(keys, w[1:])}})
        assert len(out) == len(rows), r.stdout
        return out

    return run


def reported(r):
    """The fields rmhip_gemm_last_route reports (G.route's keys)."""
    return {k: r[k] for k in ("kernel", "guard", "pre", "ta", "tb", "epi", "yield", "splits", "k_chunk")}


def planned(plan, table, knobs=None, bits=64):
    """Each case's planned route at G.NUM_CUS compute units, outside the look-ahead LU.  rmhip_pagefun's large-page tier has its own
    launcher with the one route 'pgemm guard' and does not pass through the plan: those rows are checked for the tier's conditions."""
    out = iter(plan([(c, knobs, bits, None) for c in table if c["entry"] != "pagefun"]))
    routes = []
    for c in table:
        if c["entry"] == "pagefun":
            assert c["m"] >= 256 and c["n"] >= 256 and max(c["m"], c["n"], c["k"]) > 32 and c["pages"] > 1  # rmhip_pagefun's tier 4
            routes.append(G.route("pgemm guard", 1, c["k"]))
        else:
            routes.append(reported(next(out)))
    return routes


def test_case_ids_are_unique_and_k_stays_exact():
    for table in [G.F64_CASES, G.F32_CASES, *G.KNOB_CASES.values(), *G.F32_KNOB_CASES.values()]:
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
        for c in table:
            assert 1 <= c["k"] <= G.K_MAX and c["m"] * c["n"] <= 2049 * 1153, c["id"]  # exact sums; a download of at most 2049 x 1153
            assert 2.0 * c["m"] * c["n"] * c["k"] * c.get("pages", 1) <= 4e9, c["id"]  # a few GFLOP at most


@pytest.fixture(scope="module")
def default_routes(plan):
    """id -> planned route of every row of every table, at the default knobs (planned once for the module)."""
    out = {}
    for bits, tables in ((64, [G.F64_CASES, *G.KNOB_CASES.values()]), (32, [G.F32_CASES, *G.F32_KNOB_CASES.values()])):
        rows = [c for t in tables for c in t]
        out.update({(bits, c["id"]): r for c, r in zip(rows, planned(plan, rows, bits=bits))})
    return out


@pytest.mark.parametrize("c", G.F64_CASES, ids=lambda c: c["id"])
def test_f64_rows_have_the_properties_their_routes_claim(default_routes, c):
    assert default_routes[64, c["id"]] == c["route"], (default_routes[64, c["id"]], c["route"])


@pytest.mark.parametrize("knob", sorted(G.KNOB_CASES))
def test_knob_rows_have_the_properties_their_routes_claim(plan, default_routes, knob):
    for c, got in zip(G.KNOB_CASES[knob], planned(plan, G.KNOB_CASES[knob], {knob: "0"})):
        assert got == c["route"], (c["id"], got)
    # and the setting is what selects them: all but the anchor rows of a table route elsewhere by default
    assert sum(default_routes[64, c["id"]] != c["route"] for c in G.KNOB_CASES[knob]) >= len(G.KNOB_CASES[knob]) - 2


@pytest.mark.parametrize("c", G.F32_CASES, ids=lambda c: c["id"])
def test_f32_rows_have_the_properties_their_routes_claim(default_routes, c):
    assert default_routes[32, c["id"]] == c["route"], (default_routes[32, c["id"]], c["route"])


def test_f32_knob_rows_have_the_properties_their_routes_claim(plan, default_routes):
    table = G.F32_KNOB_CASES["RMHIP_SGEMM_W8"]
    for c, got in zip(table, planned(plan, table, {"RMHIP_SGEMM_W8": "0"}, bits=32)):
        assert got == c["route"], (c["id"], got)
    assert sum(default_routes[32, c["id"]] != c["route"] for c in table) >= len(table) - 2


# ---- the rules only the look-ahead LU reaches (host-only rows: no entry point selects a site, so the GPU suite cannot iterate them) ----
MAIN = dict(in_lookahead=1)                # the LU's main stream: four-wave blocks that fit beside the update streams'
UPD = dict(in_lookahead=1, lds_pad=1)      # an update stream: one padded block per CU
_big = dict(m=2048, n=1152)                # 144 tiles of 128 x 128: past the 128 tiles of the small-update rule


def _lu(text, site, m, n, k, update=True, yield_=0, splits=1, k_chunk=None, **opts):
    c = G.case("blk", m, n, k, text, splits, k_chunk, **(dict(alpha=-1.0, beta=1.0) if update else dict(alpha=1.0, beta=0.0)), **opts)
    c["route"]["yield"] = yield_
    return c, site


LU_ROWS = [
    # update stream with a tile counter left: the persistent kernel; without one, or for a ragged shape, the eight-wave tiles
    _lu("w8p", dict(UPD, counter=1), k=128, **_big), _lu("w8p", dict(UPD, counter=1), k=128, update=False, **_big),
    _lu("w8 pre", UPD, k=128, **_big), _lu("w8g guard pre", dict(UPD, counter=1), m=2049, n=1153, k=128),
    # update stream with a yield word: the update C - A B watches it, any other product does not
    _lu("w8 pre", dict(UPD, yield_word=1), k=128, yield_=1, **_big), _lu("w8", dict(UPD, yield_word=1), k=128, update=False, **_big),
    _lu("w8p", dict(UPD, yield_word=1, counter=1), k=128, **_big),
    # update stream, k <= small_upd and at most 128 tiles: the 64 x 64 tiles, before the persistent kernel; the boundaries
    _lu("small pre", UPD, m=2048, n=1024, k=1024), _lu("small pre", dict(UPD, counter=1), m=2048, n=1024, k=1024),
    _lu("small guard pre", UPD, m=2047, n=1024, k=1024),
    _lu("w8 pre", UPD, m=128, n=16512, k=1024),                          # 129 tiles
    _lu("w8g guard pre", UPD, m=2048, n=1024, k=1025),                   # k = small_upd + 1 (ragged, so the guarded tile)
    _lu("w8 pre", UPD, m=2048, n=1024, k=1040),
    _lu("w8 pre", dict(UPD, small_upd=0), m=2048, n=1024, k=1024), _lu("small pre", dict(UPD, small_upd=128), m=2048, n=1024, k=128),
    _lu("w8 pre", dict(UPD, small_upd=128), m=2048, n=1024, k=144),
    # main stream inside the look-ahead: four-wave tiles, whole and ragged; split-K only from k = 8192
    _lu("w4", MAIN, k=128, update=False, **_big), _lu("w4 pre", MAIN, k=128, **_big), _lu("w4 edge", MAIN, m=2049, n=1153, k=128),
    _lu("w4 pre", dict(MAIN, chain_prio=1), k=128, **_big),
    _lu("w4", MAIN, m=128, n=128, k=2048, update=False), _lu("w4", MAIN, m=128, n=128, k=8192, update=False, splits=8, k_chunk=1024),
]


def test_the_rules_only_the_lookahead_lu_reaches(plan):
    got = plan([(c, None, 64, site) for c, site in LU_ROWS])
    for (c, site), r in zip(LU_ROWS, got):
        assert reported(r) == c["route"], (c["id"], site, r)
        assert r["prio"] == site.get("chain_prio", 0) and (r["tiles_m"], r["tiles_n"]) == tuple(
            -(-x // (SMALL_TILE if r["kernel"] == "small" else TILE)) for x in (c["m"], c["n"])), (c["id"], r)
    # every instantiation and rule the tables of gemm_ref.py cannot reach is in these rows
    keys = {(c["route"]["kernel"], c["route"]["pre"], c["route"]["yield"]) for c, _ in LU_ROWS}
    assert {("w8p", 0, 0), ("w8", 1, 1), ("small", 1, 0), ("w4", 0, 0), ("w4", 1, 0)} <= keys


def test_requests_no_kernel_serves_are_refused_by_the_plan(plan):
    base = dict(entry="blk", m=128, n=128, k=16)
    got = plan([(dict(base, ta=True, tb=True), None, 64, None), (dict(base, ta=True, epi=1), None, 64, None),
                (dict(base, tb=True, epi=2), None, 64, None), (dict(base, ta=True, tb=True), None, 32, None)])
    assert got == [{"unsupported": "dgemm: A' * B' is not instantiated"},
                   {"unsupported": "dgemm: epilogue with transposed operands is not instantiated"},
                   {"unsupported": "dgemm: epilogue with transposed operands is not instantiated"},
                   {"unsupported": "sgemm: A' * B' is not instantiated"}]


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
