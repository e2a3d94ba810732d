"""Host checks of the exact dyadic LU construction (tests/lu_exact_ref.py) for every host-built case of tests/test_gpu_lu_exact.py:
the bit budget is a CONDITION (<= 50 bits; thin out L, N or X before touching the cap), a plain numpy partial-pivoting LU and the
oracle's C restatement of host_lu.rs give back L, U and perm to the bit with every runner-up at most half the pivot, substitution
gives back X, and the comparison functions reject a one-ulp error, a dropped l*u term and two swapped rows.

The numpy LU runs its textbook rank-1 form (nb = 1) up to order 700 and at 1153; the other orders run it in 64-column panels (same
arithmetic, grouped; the rank-1 form at 2176 alone takes longer than this whole file should).  The oracle factors every order up to
1153 and skips 1280, 2100 and 2176 (cubic scalar C: ~3 s together).

The path every table row is meant to reach is a CLAIM, checked here against the dispatch itself: tests/cpp/lu_route_check.cpp --table walks
the plans of runmat_amd/csrc/lu_plan.h the way the drivers do and names the driver, the panel kernels, the triangular-solve kernels, the
substitution form and the padding of a row (shape, mode, the row's environment as knob values, 256 compute units)."""
import numpy as np
import pytest

import lu_exact_ref as ref
import test_gpu_lu_exact as table


def _nb(n):
    return 1 if n <= 700 or n == 1153 else 64


@pytest.mark.parametrize("rows,cols,kind", table.HOST_LU_CASES)
def test_lu_cases_are_exact_and_reproduced_on_the_host(oracle, rows, cols, kind):
    c = table.lu_case(rows, cols, kind)
    budget = ref.bit_budget(c)
    assert max(budget.values()) <= ref.BIT_CAP, budget
    assert np.array_equal(np.sort(c.perm), np.arange(rows)) and np.all(c.perm // ref.GROUP == np.arange(rows) // ref.GROUP)
    if kind == "identity":
        assert np.array_equal(c.perm, np.arange(rows))
    if kind == "reverse" and rows % ref.GROUP == 0:
        assert np.array_equal(c.perm.reshape(-1, ref.GROUP), np.arange(rows).reshape(-1, ref.GROUP)[:, ::-1])
    F, perm, worst = ref.numpy_lu(c.A, _nb(max(rows, cols)))
    assert worst <= 0.5  # every runner-up at most half the pivot: the pivot choice cannot depend on the rule's tie-breaking
    comb, low, up, pm, pv = ref.lu_outputs_expected(c, perm)
    assert np.array_equal(perm[: c.k], c.perm[: c.k]) and ref.mismatches(F, comb) == 0
    assert not ref.failed(ref.compare_lu(c, comb, low, up, pm, pv))
    if max(rows, cols) <= 1153:
        assert not ref.failed(ref.compare_lu(c, *oracle.lu(c.A)))


@pytest.mark.parametrize("n", sorted({n for n, _ in table.HOST_SOLVE_CASES}))
def test_solve_cases_are_exact_and_reproduced_on_the_host(oracle, n):
    c = table.lu_case(n, n)
    F, perm, worst = ref.numpy_lu(c.A, _nb(n))
    assert worst <= 0.5 and np.array_equal(perm, c.perm)
    Lf, Uf = np.tril(F, -1) + np.eye(n), np.triu(F)
    assert ref.mismatches(Lf, c.L) == 0 and ref.mismatches(Uf, c.U) == 0
    if n <= 1153:
        assert not ref.failed(ref.compare_lu(c, *oracle.lu(c.A)))
    if n > 256:  # what test_gpu_lu_exact.expected_multiplier relies on: a nonzero of L under the first top block, in its first panel
        assert np.any(c.L[256:, :16] != 0.0) and np.abs(np.tril(c.L, -1)).max() == 0.5
    for nrhs in sorted({r for m, r in table.HOST_SOLVE_CASES if m == n}):
        _, X, B = table.solve_case(n, nrhs)
        budget = ref.bit_budget(c, X)
        assert max(budget.values()) <= ref.BIT_CAP, (nrhs, budget)
        Y, Xg = ref.substitute(Lf, Uf, B[perm])
        assert ref.mismatches(Y, c.U @ X) == 0 and ref.mismatches(Xg, X) == 0
    for kind in ("identity", "reverse"):
        if n in (300, 1280):
            ck = table.lu_case(n, n, kind)
            assert max(ref.bit_budget(ck, ref.rhs(ck, 5, 13)[0]).values()) <= ref.BIT_CAP


@pytest.mark.parametrize("n", table.TRI_ORDERS)
def test_triangular_hint_cases_are_exact(n):
    c = table.lu_case(n, n)
    for nrhs in table.TRI_NRHS:
        X, _ = ref.rhs(c, nrhs, 17)
        for T in (c.L, c.U, c.L.T, c.U.T):
            # partial sums of a triangular solve are partial sums of T X: multiples of 1/2 bounded by |T| |X|
            assert ref._bits_for(float((np.abs(T) @ np.abs(X)).max()), -1) <= ref.BIT_CAP
        Y, Xg = ref.substitute(c.L, c.U, (c.L @ (c.U @ X)))
        assert ref.mismatches(Xg, X) == 0


def test_two_level_case_meets_the_budget_for_every_draw():
    budget = ref.bit_budget_worst_case(table.SUPER_N, table.SUPER_NRHS, table.SUPER_XMAX)
    assert budget == {"form1": 30, "form2": 30, "form3": 45} and max(budget.values()) <= ref.BIT_CAP
    # the worst case dominates what a drawn case needs
    c = table.lu_case(300, 300)
    X, _ = ref.rhs(c, 2, 1)
    drawn, worst = ref.bit_budget(c, X), ref.bit_budget_worst_case(300, 2, 3)
    assert all(drawn[k] <= worst[k] for k in drawn)


@pytest.mark.parametrize("n", [64, 300, 1153])
def test_inverse_form_gives_the_same_y_in_two_summation_orders(n):
    c, X, B = table.solve_case(n, 5) if (n, 5) in table.HOST_SOLVE_CASES else (table.lu_case(n, n),) + ref.rhs(table.lu_case(n, n), 5, 11)
    PB = B[c.perm]
    y1 = ref.forward_inverse_model(c.L, PB, reverse=False)
    y2 = ref.forward_inverse_model(c.L, PB, reverse=True)
    assert ref.mismatches(y1, y2) == 0 and ref.mismatches(y1, c.U @ X) == 0
    # the inverted blocks are multiples of 2^-15 (L) and 2^-17 (U), as the budget assumes
    for b0 in range(0, n - n % ref.BLOCK, ref.BLOCK):
        il = ref.tri_inv(c.L[b0:b0 + 16, b0:b0 + 16]) * 2.0 ** 15
        iu = ref.tri_inv(c.U[b0:b0 + 16, b0:b0 + 16]) * 2.0 ** 17
        assert np.array_equal(il, np.rint(il)) and np.array_equal(iu, np.rint(iu))
        assert ref.mismatches(il @ c.L[b0:b0 + 16, b0:b0 + 16], np.eye(16) * 2.0 ** 15) == 0


def test_the_sign_of_a_computed_zero_depends_on_the_association():
    """Why `mismatches` leaves the sign of a COMPUTED zero free: the textbook step 0 / d gives -0.0 under a negative pivot, the product
    of the same row with the inverted block gives +0.0 - two correct roundings of one exact value."""
    c = table.lu_case(300, 300)
    F, perm, _ = ref.numpy_lu(c.A, 1)
    comb = ref.lu_outputs_expected(c, perm)[0]
    strict = ref._bits(F) != ref._bits(comb)
    assert strict.any() and np.all(F[strict] == 0.0) and np.all(np.signbit(F[strict])) and ref.mismatches(F, comb) == 0
    i, j = np.nonzero(strict)
    assert np.all(i > j) and np.all(np.diag(c.U)[j] < 0)  # multipliers under negative pivots, nowhere else
    a_rows = (c.L[16:32, :16] @ c.U[:16, :16])           # rows below a 16 x 16 block, as a rows-below kernel meets them
    via_inverse = a_rows @ ref.tri_inv(c.U[:16, :16])
    assert ref.mismatches(via_inverse, c.L[16:32, :16]) == 0 and not np.signbit(via_inverse[via_inverse == 0.0]).any()


def test_the_comparison_rejects_one_ulp_a_dropped_term_and_swapped_rows():
    c = table.lu_case(300, 300)
    perm = c.perm.copy()
    comb, low, up, pm, pv = ref.lu_outputs_expected(c, perm)
    assert not ref.failed(ref.compare_lu(c, comb, low, up, pm, pv))
    # one ulp in one entry of the combined factor
    bad = comb.copy()
    bad[200, 100] = np.nextafter(bad[200, 100] if bad[200, 100] else 0.5, np.inf)
    assert ref.failed(ref.compare_lu(c, bad, low, up, pm, pv)) == {"combined": 1}
    assert ref.mismatches(np.nextafter(up, np.inf), up) == up.size
    # one l*u term dropped in one trailing element: U[i, j] keeps a term that the elimination should have removed
    i, j = 250, 280
    kk = int(np.nonzero((c.L[i, :i] != 0) & (c.U[:i, j] != 0))[0][0])
    bad_up = up.copy()
    bad_up[i, j] += c.L[i, kk] * c.U[kk, j]
    bad_comb = comb.copy()
    bad_comb[i, j] = bad_up[i, j]
    assert ref.failed(ref.compare_lu(c, bad_comb, low, bad_up, pm, pv)) == {"upper": 1, "combined": 1}
    # two rows of perm swapped inside a group (with every output kept consistent with the wrong order)
    p2 = perm.copy()
    p2[[70, 75]] = p2[[75, 70]]
    comb2, low2, up2, pm2, pv2 = ref.lu_outputs_expected(c, p2)
    rep = ref.failed(ref.compare_lu(c, comb2, low2, up2, pm2, pv2))
    assert rep.get("perm_pivots") == 2, rep
    # and an inconsistent perm_matrix, a non-permutation and a -0.0 among the constant zeros
    assert "perm_matrix" in ref.failed(ref.compare_lu(c, comb, low, up, pm2, pv))
    pv_bad = pv.copy()
    pv_bad[3] = pv_bad[4]
    assert ref.failed(ref.compare_lu(c, comb, low, up, pm, pv_bad)) == {"perm_valid": 1}
    low_bad = low.copy()
    low_bad[0, 299] = -0.0
    assert ref.failed(ref.compare_lu(c, comb, low_bad, up, pm, pv)) == {"lower": 1}
    # solutions: a stale column, one ulp, a NaN
    X, _ = ref.rhs(c, 5, 11)
    stale = X.copy()
    stale[:, 4] = X[:, 3]
    assert ref.mismatches(stale, X) > 0 and ref.mismatches(X + 0.0, X) == 0
    nan = X.copy()
    nan[0, 0] = np.nan
    assert ref.mismatches(nan, X) == 1 and ref.mismatches(X[:, :4], X) > 0


# ---- the tables' path claims against the dispatch itself (runmat_amd/csrc/lu_plan.h through tests/cpp/lu_route_check.cpp --table) -------------
NUM_CUS = 256  # an MI355X


def _knob_fields(environment):
    """The row's environment as lu_knobs() / lu_process_knobs() read it, in the field order of `lu_route_check --table`."""
    e = dict(environment)
    flag = lambda name, default, on: int(on(e[name])) if name in e else default
    fields = [flag("RMHIP_LU_FAST", 1, lambda v: v[0] != "0"), flag("RMHIP_LU_LOOKAHEAD", -1, lambda v: v[0] == "1"), int(e.get("RMHIP_LU_NB", -1)),
              flag("RMHIP_LU_PANEL", 0, lambda v: v[0] == "c"), flag("RMHIP_LU_PANEL_DEBUG", 0, lambda v: v[0] == "1"),
              flag("RMHIP_LU_SUBST", 0, lambda v: v[0] == "p"), flag("RMHIP_LU_PAD", 1, lambda v: v[0] != "0"),
              flag("RMHIP_LU_SUPER", 1, lambda v: int(v) != 0), flag("RMHIP_LU_RB_MFMA", 1, lambda v: int(v) != 0),
              flag("RMHIP_LU_TRSM_MFMA", 1, lambda v: int(v) != 0), int(e.get("RMHIP_LU_SUPER_ROWS", -1)), int(e.get("RMHIP_LU_IPREP", -1)),
              e.get("RMHIP_LU_SUPER_SEQ", "-"), e.get("RMHIP_LU_SUPER_LATE", "-")]
    return " ".join(str(f) for f in fields)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """planned(lines) -> one dict per case line: the key=value fields of the tool's answer, and `seen`, the set of its bare words."""
    from test_host_plan import compile_check

    exe = compile_check(tmp_path_factory.mktemp("lu_route_check"), "lu_route_check")

    def run(lines):
        import subprocess

        r = subprocess.run([str(exe), "--table"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = []
        for ln in r.stdout.splitlines():
            words = ln.split()
            d = dict(w.split("=", 1) for w in words if "=" in w)
            d["seen"] = {w for w in words if "=" not in w}
            out.append(d)
        assert len(out) == len(lines)
        return out

    return run


def _lu_line(rows, cols, mode, environment):
    return f"lu {rows} {cols} {mode} {NUM_CUS} {_knob_fields(environment)}"


def _solve_line(n, nrhs, environment):
    return f"solve {n} {nrhs} {NUM_CUS} {_knob_fields(environment)}"


_KERNEL_WORD = {"k_rp_below": "below:valu", "k_rp_below_mfma": "below:mfma", "k_trsm_lower_mfma<4>": "trsm:mfma4",
                "k_trsm_lower_mfma<8>": "trsm:mfma8", "k_trsm_lower_2p": "trsm:two_pass", "k_trsm_fused": "trsm:fused"}


def test_lu_table_rows_take_the_path_they_name(planned):
    """The sixth field of every LU_TABLE row, word by word: the driver, the panel kernel family, the wide tail, the two-pass solve
    (claimed by a row if and only if the plan launches it)."""
    got = planned([_lu_line(rows, cols, 0, knobs) for _, rows, cols, knobs, _, _ in table.LU_TABLE])
    for (rid, rows, cols, knobs, _, path), g in zip(table.LU_TABLE, got):
        claims = [w.strip() for w in path.split("+")]
        assert set(claims) <= {"getrf_rec", "getrf_blocked", "k_lu_panel2", "k_lu_col", "k_build_plist", "wide tail", "k_trsm_lower_2p"}, (rid, path)
        assert g["fast"] == "0", rid
        if "getrf_rec" in claims or "getrf_blocked" in claims:
            assert g["driver"] == ("blocked" if "getrf_blocked" in claims else "rec"), (rid, g)
        if "k_lu_panel2" in claims:
            assert "panel:persistent" in g["seen"] and "panel:columns" not in g["seen"], (rid, g)
        if "k_lu_col" in claims:
            assert "k_build_plist" in claims and "panel:columns" in g["seen"] and "panel:persistent" not in g["seen"], (rid, g)
        assert ("wide tail" in claims) == ("wide_tail" in g["seen"]), (rid, g)
        assert ("k_trsm_lower_2p" in claims) == ("trsm:two_pass" in g["seen"]), (rid, g)
        assert "panel:top" not in g["seen"] and "unsupported:" not in g["seen"], (rid, g)


def test_solve_table_rows_take_the_path_the_table_names(planned):
    """SOLVE_TABLE's comment and SOLVE_REACH: the driver by order, the padding of 2100, the substitution form and its column groups by
    (order, nrhs), and for each kernel of SOLVE_REACH exactly the listed orders.  The one-launch solver's orders are asked as
    RMHIP_NO_SMALL_SOLVE sends them: through the blocked kernels."""
    got = planned([_solve_line(n, nrhs, {}) for n, nrhs in table.SOLVE_TABLE])
    for (n, nrhs), g in zip(table.SOLVE_TABLE, got):
        order = 2176 if n == 2100 else n
        assert int(g["order"]) == order and g["padded"] == str(int(n == 2100)), (n, g)
        assert g["driver"] == ("rec" if order < 1152 else "blocked") and g["fast"] == "1" and "panel:top" in g["seen"], (n, g)
        want = "rec" if nrhs > 8 else ("chain" if order >= 385 else "pair")
        assert g["subst"] == want and int(g["groups"]) == ((nrhs + 3) // 4 if want == "chain" else 0), (n, nrhs, g)
    by_order = {n: g for (n, _), g in zip(table.SOLVE_TABLE, got)}
    for kernel, orders in table.SOLVE_REACH.items():
        reached = tuple(n for n in table.SOLVE_ORDERS if n > 64 and _KERNEL_WORD[kernel] in by_order[n]["seen"])
        assert reached == orders, (kernel, reached)


def test_knob_rows_change_what_their_comment_says(planned):
    for knobs, cases in table.KNOB_TABLE:
        got = planned([_solve_line(n, nrhs, knobs) for n, nrhs in cases])
        base = planned([_solve_line(n, nrhs, {}) for n, nrhs in cases])
        grid = planned([_lu_line(int(g["order"]), int(g["order"]), 0, knobs) for g in got])  # the refactorisation a growth failure asks for
        for (n, nrhs), g, b, m0 in zip(cases, got, base, grid):
            if "RMHIP_LU_FAST" in knobs:  # the grid-wide rule behind a solve: k_lu_panel2 panels, no solve-path kernel
                assert g["fast"] == "0" and "panel:persistent" in g["seen"] and "panel:top" not in g["seen"], (n, g)
                assert g["driver"] == ("blocked" if int(g["order"]) >= 5120 else "rec"), (n, g)
            elif "RMHIP_LU_SUBST" in knobs:  # k_trsm_fused + k_rhs_update where the default is k_subst_chain
                assert g["subst"] == "pair" and b["subst"] == "chain", (n, g)
            elif knobs.get("RMHIP_LU_LOOKAHEAD") == "0":
                assert g["driver"] == "rec" and b["driver"] == "blocked", (n, g)
            elif knobs.get("RMHIP_LU_LOOKAHEAD") == "1":
                assert g["driver"] == "blocked" and b["driver"] == "rec", (n, g)
            elif "RMHIP_LU_PAD" in knobs:
                assert (g["padded"], int(g["order"])) == ("0", n) and (b["padded"], int(b["order"])) == ("1", 2176), (n, g)
            elif "RMHIP_LU_TEST_GROWTH" in knobs:  # the solve path runs as usual, then mode 0 at the same order
                assert {k: v for k, v in g.items()} == {k: v for k, v in b.items()} and m0["fast"] == "0" and "panel:persistent" in m0["seen"], (n, g)
            else:  # RMHIP_NO_SMALL_SOLVE: a switch of solve.cpp - these orders then take the solve path's recursive driver
                assert "RMHIP_NO_SMALL_SOLVE" in knobs and n <= 64 and g["driver"] == "rec" and "panel:top" in g["seen"], (n, g)


def test_process_switch_rows_change_what_their_comment_says(planned):
    for switches in table.PROCESS_SWITCHES:
        got = planned([_solve_line(n, nrhs, switches) for n, nrhs in table.PROCESS_ORDERS])
        base = planned([_solve_line(n, nrhs, {}) for n, nrhs in table.PROCESS_ORDERS])
        for (n, nrhs), g, b in zip(table.PROCESS_ORDERS, got, base):
            seen = g["seen"]
            assert g["driver"] == b["driver"] and g["order"] == b["order"] and g["subst"] == b["subst"], (switches, n, g)
            if switches.get("RMHIP_LU_TRSM_MFMA") == "0":  # no matrix-core solve; the two-pass kernel inside the look-ahead driver
                assert not seen & {"trsm:mfma4", "trsm:mfma8"} and "trsm:fused" in seen, (switches, n, g)
                assert ("trsm:two_pass" in seen) == (g["driver"] == "blocked"), (switches, n, g)
            if switches.get("RMHIP_LU_RB_MFMA") == "0":  # k_rp_below under every panel with rows below a top block
                assert "below:mfma" not in seen and "below:valu" in seen, (switches, n, g)
            if "RMHIP_LU_TRSM_MFMA" not in switches:  # the default, and RMHIP_LU_SMALL_UPD (a switch of the GEMM plan): the default's kernels
                assert seen == b["seen"], (switches, n, g)


def test_super_plans_run_the_driver_their_row_names(planned):
    got = planned([_solve_line(table.SUPER_N, table.SUPER_NRHS, plan) for plan in table.SUPER_PLANS])
    default, one_level, alternative = got
    assert default["driver"] == "super" and default["widths"] == "128,512,", default           # 512-column panels, then 128 from 6144 rows
    assert one_level["driver"] == "blocked" and one_level["widths"] == "128,", one_level      # RMHIP_LU_SUPER=0
    assert alternative["driver"] == "super" and alternative["widths"] == "128,256,", alternative
    for g in got:
        assert g["fast"] == "1" and {"below:mfma", "trsm:mfma4", "trsm:mfma8"} <= g["seen"] and g["subst"] == "chain", g
    # kSuperMin: no smaller order reaches getrf_super (a solve of order 8065 .. 8191 is padded to 8192 and does)
    below = planned([_lu_line(8191, 8191, 1, {}), _solve_line(8064, 2, {}), _solve_line(8191, 2, {})])
    assert [g["driver"] for g in below] == ["blocked", "blocked", "super"]


def test_shapes_the_dispatch_sends_elsewhere_than_one_might_expect(planned):
    la = lambda nb: {"RMHIP_LU_LOOKAHEAD": "1", "RMHIP_LU_NB": str(nb)}
    # RMHIP_LU_NB=256 below 8192 + 128 remaining columns runs 128-wide panels (plan_blocked: nb_late = min(nb, kNbLate)); what it changes
    # at these orders is only plan_lu_factor's `kmin > nb` test
    wide, narrow, at_nb = planned([_lu_line(700, 700, 0, la(256)), _lu_line(700, 700, 0, la(128)), _lu_line(256, 256, 0, la(256))])
    assert wide["driver"] == "blocked" and wide["widths"] == narrow["widths"] == "60,128," and at_nb["driver"] == "rec"
    # kmin = 64 = the smallest nb: a forced look-ahead still takes getrf_rec, and the wide one its laswp + trsm_lower_rec tail
    w, t = planned([_lu_line(64, 700, 0, la(64)), _lu_line(700, 64, 0, la(64))])
    assert w["driver"] == t["driver"] == "rec" and "wide_tail" in w["seen"] and "wide_tail" not in t["seen"]
    # 200 x 330 and 330 x 200 do reach getrf_blocked with RMHIP_LU_NB=64, and end in an 8-column panel
    for g in planned([_lu_line(200, 330, 0, la(64)), _lu_line(330, 200, 0, la(64))]):
        assert g["driver"] == "blocked" and g["widths"] == "8,64," and "wide_tail" not in g["seen"], g
    # RMHIP_LU_FAST=0 behind a solve runs the grid-wide rule (not counted as a solve-path factorisation), at n <= 64 too
    for g in planned([_solve_line(n, 1, {"RMHIP_LU_FAST": "0"}) for n in (17, 64, 300)]):
        assert g["fast"] == "0" and g["driver"] == "rec" and "panel:persistent" in g["seen"], g
