"""Every LU and triangular-solve path of lu.hip / small_solve.hip against EXACT dyadic factors (tests/lu_exact_ref.py): matrices whose
partial-pivoting L, U, perm and whose solutions are one bit pattern in fp64 under every grouping of the additions, so a dropped k-slice,
a skipped update, a wrong entry of an inverted block, two mis-ordered rows or a stale right-hand-side column is a bit mismatch instead of
a residual below a tolerance.  No U(-1,1) data, no tolerances, no residuals here; the comparisons are `lu_exact_ref.mismatches`
(uint64 views; only the sign of a computed zero is free, see that module).

THE TABLE.  One row per case: what it runs and the path it is meant to reach, named by the rule of runmat_amd/csrc/lu_plan.h that sends it
there.  `lu_stats` cannot tell which kernel ran; the rules are the evidence, and tests/test_lu_exact_host.py checks every claim of the
tables below against them (tests/cpp/lu_route_check.cpp --table plans each row as the drivers do).  Kernels named as reached:
  k_lu_panel2        rows rec-*, lookahead-*, rect-*, perm-* of LU_TABLE (plan_base_panel: PanelKind::persistent, the default of `lu`)
  k_lu_col           rows columns-* and perm-*-columns (plan_lu_factor: RMHIP_LU_PANEL=columns -> !persistent -> PanelKind::columns)
  k_build_plist      the same rows
  k_rp_top           every blocked solve: the rows of SOLVE_TABLE with n > 64 or nrhs > 16 (plan_lu_factor: fast for mode 1 ->
                     PanelKind::top)
  k_rp_below         solves with rows below a top block under a base panel that is not 64 wide - 300, 1151 - and every panel with rows
                     below under RMHIP_LU_RB_MFMA=0 (plan_base_panel: inverses = rb_mfma && w == 64, PanelBelow::valu); SOLVE_REACH
  k_rp_below_mfma    solves of order 257, 513, 1151, 1152, 1153, 1280, 2100 (padded to 2176), 2176, 8192: 64-wide base panels with rows
                     below (PanelBelow::mfma); SOLVE_REACH
  k_laswp_lists      every `lu` and blocked solve; empty lists under the identity permutation, full ones under the reversal
  k_trsm_fused       MODE 0: `lu` of order > 64, and ragged blocks (plan_trsm: TrsmKernel::fused); MODE 1 / 2: linsolve's triangular
                     hints and the substitution in pairs (plan_substitute: SubstForm::pair - n < 385, RMHIP_LU_SUBST=pair)
  k_trsm_lower_2p    the look-ahead driver without inverses, 65..128-wide blocks: rows lookahead-* with RMHIP_LU_NB >= 128, and
                     RMHIP_LU_TRSM_MFMA=0 behind a solve of order >= 1152 (plan_trsm: TrsmKernel::two_pass)
  k_trsm_lower_mfma  solves from order 129: <4> inside a 128-wide panel's recursion, <8> on 128-wide diagonal blocks (plan_trsm:
                     mfma4 / mfma8 once the inverses of the block are queued); SOLVE_REACH
  k_gather_rows      every blocked solve
  k_rhs_update       substitution in pairs
  k_subst_chain<0/2> n >= 385 with nrhs <= 8 (plan_substitute: four or more 128-row blocks, in groups of four columns - nrhs 5 is
                     4 + 1, nrhs 8 is 4 + 4); nrhs > 8 takes trsm_lower_rec / trsm_upper_rec with a dgemm in between (SubstForm::rec)
  k_lu_pad_identity  order 2100 (lu_pad_rows: n >= 2048 and not a multiple of 128 factors at 2176; RMHIP_LU_PAD=0 does not)
  k_lu_extract       every `lu` (solve.cpp)
  small_solve.hip    2 <= n <= 64 with nrhs <= 16 (small_solve_applies)
  getrf_super        order 8192 on the solve path (plan_lu_factor: kSuperMin), one child process per plan
Not reachable from these entry points: k_permute_rows, k_permute_rows_dev and k_compose_swaps serve rmhip_blk_swap_rows only, a building
block of the row-partitioned driver, which is out of scope here.

Shapes the dispatch sends elsewhere than one might expect (the first three and the last are asserted against the plan by
tests/test_lu_exact_host.py):
  * RMHIP_LU_NB=256 below 8192 + 128 remaining columns runs 128-wide panels (plan_blocked: nb_late = min(nb, kNbLate)); what NB=256
    changes at these orders is only the `kmin > nb` test of plan_lu_factor.
  * 64 x 700 and 700 x 64 have kmin = 64 = the smallest nb, so a forced look-ahead still takes getrf_rec (plan_lu_factor) and the wide
    one its laswp + trsm_lower_rec tail (lu_factor_device).
  * 200 x 330 and 330 x 200 do reach getrf_blocked with RMHIP_LU_NB=64.
  * linsolve refuses 1 x 1 operands (solve.cpp: the CPU path), so the triangular hints start at n = 2 and n = 1 is asserted to raise.
  * mrdivide(B', A') transposes both operands back (solve.cpp): it factors A itself, so the transposed system U' L' P never
    has to be exact; linsolve with `transposed` is fed A' for the same reason.
  * RMHIP_LU_FAST=0 behind a solve runs the grid-wide rule, which the statistics do not count as a solve-path factorisation
    (lu_copy_and_factor); n <= 64 then takes the blocked kernels too (solve.cpp).

Order 8192 (operands built on the device, three plans, one child each).  Bit budget from the construction's parameters alone
(lu_exact_ref.bit_budget_worst_case(8192, 2, 3): every entry at its largest magnitude): form 1 30 bits, form 2 30 bits, form 3 45 bits.
Measured on an MI355X: each child 0.19 - 0.23 s from provider creation to the downloaded solution (the solve itself 0.045 s), 0.44 - 0.48 s
per test with the interpreter's start (WALL_8192 below).
"""
import contextlib
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import lu_exact_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

# measured on an MI355X (seconds per test, child interpreter included): default plan / RMHIP_LU_SUPER=0 / the alternative plan
WALL_8192 = (0.45, 0.48, 0.44)

LA = "RMHIP_LU_LOOKAHEAD"
NB = "RMHIP_LU_NB"

# ---- 3a: `lu` (grid-wide rule).  (id, rows, cols, per-call environment, permutation, path) ------------------------------------------------
LU_TABLE = []
for _n in (1, 2, 17, 63, 64, 65, 130, 255, 256, 257, 513, 700, 1153):
    # getrf_rec (plan_lu_factor: `lu` is mode 0, look-ahead only from kBlockedMin) -> k_lu_panel2; 1..64 one base panel, 65 / 130 ragged
    # halves (rec_split: h = w/2 rounded up to 16), 255..257 one / two 256-row panel blocks (plan_base_panel), 1153 recursion depth 5
    LU_TABLE.append((f"rec-{_n}", _n, _n, {}, "random", "getrf_rec + k_lu_panel2"))
for _n in (17, 65, 257, 700):
    LU_TABLE.append((f"columns-{_n}", _n, _n, {"RMHIP_LU_PANEL": "columns"}, "random", "getrf_rec + k_lu_col + k_build_plist"))
for _n, _nb in ((200, 64), (300, 64), (300, 128), (700, 128), (700, 256), (1153, 64), (1153, 256)):
    # getrf_blocked forced (plan_lu_factor: lookahead); 200 with 64-wide panels ends in an 8-column panel; nb >= 128: k_trsm_lower_2p
    # (plan_trsm)
    LU_TABLE.append((f"lookahead-{_n}-nb{_nb}", _n, _n, {LA: "1", NB: str(_nb)}, "random",
                     "getrf_blocked" + (" + k_trsm_lower_2p" if _nb >= 128 else "")))
for _r, _c in ((200, 330), (330, 200), (64, 700), (700, 64)):
    LU_TABLE.append((f"rect-{_r}x{_c}-rec", _r, _c, {}, "random", "getrf_rec" + (" + wide tail" if _c > _r else "")))
    LU_TABLE.append((f"rect-{_r}x{_c}-la", _r, _c, {LA: "1", NB: "64"}, "random",
                     "getrf_blocked" if min(_r, _c) > 64 else "getrf_rec" + (" + wide tail" if _c > _r else "")))  # 64: kmin = nb
for _kind in ("identity", "reverse"):
    # empty row-move lists / full 64-entry lists in k_laswp_lists (and k_build_plist under columns)
    LU_TABLE.append((f"perm-{_kind}-300", 300, 300, {}, _kind, "getrf_rec"))
    LU_TABLE.append((f"perm-{_kind}-300-columns", 300, 300, {"RMHIP_LU_PANEL": "columns"}, _kind, "k_lu_col + k_build_plist"))
    LU_TABLE.append((f"perm-{_kind}-700-la", 700, 700, {LA: "1", NB: "128"}, _kind, "getrf_blocked + k_trsm_lower_2p"))

# ---- 3b: the solves.  (n, nrhs) ----------------------------------------------------------------------------------------------------------------
# 2..64: small_solve.hip; 65..1151: getrf_rec on the solve path (plan_lu_factor: kBlockedMinFast); 1152..: getrf_blocked; 2100: padded to
# 2176; nrhs 1, 3: one chain / pair group, 5: 4 + 1, 8: 4 + 4, 16 / 17: trsm_*_rec (plan_substitute) and, at n <= 64, 16 the small
# solver's last width and 17 the first that leaves it (small_solve_applies)
SOLVE_ORDERS = (2, 17, 33, 64, 65, 129, 255, 257, 300, 513, 1151, 1152, 1153, 1280, 2100, 2176)
SOLVE_TABLE = [(n, 1) for n in SOLVE_ORDERS] + [(17, 3), (33, 16), (33, 17), (64, 5), (64, 16), (64, 17), (65, 5), (300, 3), (300, 5),
                                                (300, 8), (300, 17), (513, 5), (513, 8), (513, 16), (1153, 3), (1153, 5), (1153, 17),
                                                (1280, 5), (1280, 8), (2100, 5), (2176, 17)]
# which orders of SOLVE_ORDERS above 64 reach which kernel under the default knobs - these and no others
SOLVE_REACH = {
    "k_rp_below": (300, 1151),
    "k_rp_below_mfma": (257, 513, 1151, 1152, 1153, 1280, 2100, 2176),
    "k_trsm_lower_mfma<4>": (129, 255, 257, 513, 1151, 1152, 1153, 1280, 2100, 2176),
    "k_trsm_lower_mfma<8>": (255, 257, 513, 1152, 1153, 1280, 2100, 2176),
    "k_trsm_lower_2p": (),
}
# per-call knobs (lu_knobs(), solve_knobs(): read at every call).  (knob, [(n, nrhs)])
KNOB_TABLE = [
    ({"RMHIP_LU_FAST": "0"}, [(17, 1), (64, 3), (300, 5), (1153, 1), (2100, 5)]),         # grid-wide rule behind a solve (plan_lu_factor: fast)
    ({"RMHIP_NO_SMALL_SOLVE": "1"}, [(2, 1), (17, 3), (33, 16), (64, 1), (64, 5)]),       # blocked kernels at n <= 64 (solve.cpp)
    ({"RMHIP_LU_SUBST": "pair"}, [(513, 1), (513, 5), (1153, 3), (1280, 8), (2100, 5)]),   # k_trsm_fused + k_rhs_update (plan_substitute: pair)
    ({"RMHIP_LU_LOOKAHEAD": "0"}, [(1152, 1), (1153, 5), (1280, 3), (2100, 1)]),         # getrf_rec where the default is getrf_blocked
    ({"RMHIP_LU_LOOKAHEAD": "1"}, [(129, 1), (300, 5), (513, 3), (700, 1)]),             # getrf_blocked where the default is getrf_rec
    ({"RMHIP_LU_PAD": "0"}, [(2100, 1), (2100, 5)]),                                     # ragged order unpadded (lu_pad_rows)
    ({"RMHIP_LU_TEST_GROWTH": "1"}, [(65, 1), (300, 5), (1153, 3), (2100, 1)]),          # forced refactorisation (lu_factor_device)
]
TRI_ORDERS = (2, 17, 64, 65, 300, 1153)
TRI_NRHS = (1, 3, 17)
# ---- 3c: per-process switches (lu_process_knobs(): read once), one child each ---------------------------------------------------------------
PROCESS_SWITCHES = [
    {},
    {"RMHIP_LU_RB_MFMA": "0", "RMHIP_LU_TRSM_MFMA": "0"},   # k_rp_below and k_trsm_fused / k_trsm_lower_2p everywhere
    {"RMHIP_LU_TRSM_MFMA": "0"},
    {"RMHIP_LU_SMALL_UPD": "0"},                            # 128 x 128 tiles only on the update streams
]
PROCESS_ORDERS = [(n, nrhs) for n in (300, 1153, 1280, 2100) for nrhs in (1, 5)]
# ---- 3d: the two-level driver --------------------------------------------------------------------------------------------------------------------
SUPER_PLANS = [
    {},
    {"RMHIP_LU_SUPER": "0"},
    {"RMHIP_LU_SUPER_SEQ": "512:256/1024:256", "RMHIP_LU_SUPER_ROWS": "2048", "RMHIP_LU_SUPER_LATE": "512:128"},
]
SUPER_N, SUPER_NRHS, SUPER_XMAX = 8192, 2, 3

HOST_LU_CASES = sorted({(r, c, kind) for _, r, c, _, kind, _ in LU_TABLE})
HOST_SOLVE_CASES = sorted(set(SOLVE_TABLE) | {p for _, ps in KNOB_TABLE for p in ps} | set(PROCESS_ORDERS))


@functools.lru_cache(maxsize=None)
def lu_case(rows, cols, kind="random"):
    return ref.case(rows, cols, 7, kind)


@functools.lru_cache(maxsize=None)
def solve_case(n, nrhs):
    c = lu_case(n, n)
    return (c,) + ref.rhs(c, nrhs, 11)


def expected_multiplier(c, small):
    """`last_max_multiplier`: the largest multiplier BELOW a panel's 256-row top block; 0 when nothing lies below one (n <= 256) and on
    the one-launch solver, exactly 1/2 once L has a nonzero under the first top block (the host test pins that for every such case)."""
    return 0.0 if small or c.rows <= 256 else 0.5


@contextlib.contextmanager
def env(kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update(kv)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _take(prov, h):
    out = prov.download_matrix(h)
    prov.free(h)
    return out


# ---- 3a ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", LU_TABLE, ids=[r[0] for r in LU_TABLE])
def test_lu_factors_are_the_constructed_bits(prov, row):
    _, rows, cols, knobs, kind, _ = row
    c = lu_case(rows, cols, kind)
    ha = prov.upload(c.A)
    with env(knobs):
        r = prov.lu(ha)
    got = [_take(prov, h) for h in (r.combined, r.lower, r.upper, r.perm_matrix, r.perm_vector)]
    prov.free(ha)
    report = ref.compare_lu(c, *got)
    print(row[0], report)
    assert not ref.failed(report), (row[0], report)


# ---- 3b ---------------------------------------------------------------------------------------------------------------------------------------------
def _solve_and_check(prov, c, X, B, small, counted=True, fallbacks=0, check_multiplier=True):
    ha, hb = prov.upload(c.A), prov.upload(B)
    s0 = prov.lu_stats()
    x = _take(prov, prov.mldivide(ha, hb))
    s1 = prov.lu_stats()
    prov.free(ha)
    prov.free(hb)
    bad = ref.mismatches(x, X)
    print(f"n={c.rows} nrhs={X.shape[1]} mismatches={bad} multiplier={s1['last_max_multiplier']}")
    assert bad == 0, (c.rows, X.shape[1], bad)
    assert s1["solve_path_factorizations"] == s0["solve_path_factorizations"] + (1 if counted else 0)
    assert s1["pivot_growth_fallbacks"] == s0["pivot_growth_fallbacks"] + fallbacks
    if check_multiplier:
        assert s1["last_max_multiplier"] == expected_multiplier(c, small), s1


@pytest.mark.parametrize("n,nrhs", SOLVE_TABLE)
def test_mldivide_linsolve_mrdivide_return_the_integer_solution(prov, n, nrhs):
    c, X, B = solve_case(n, nrhs)
    small = 2 <= n <= 64 and nrhs <= 16
    _solve_and_check(prov, c, X, B, small)
    ha, hb = prov.upload(c.A), prov.upload(B)
    xl = _take(prov, prov.linsolve(ha, hb).solution)
    assert ref.mismatches(xl, X) == 0
    from runmat_amd import ProviderLinsolveOptions

    hat, hbt = prov.upload(np.ascontiguousarray(c.A.T)), prov.upload(np.ascontiguousarray(B.T))
    xt = _take(prov, prov.linsolve(hat, hb, ProviderLinsolveOptions(transposed=True)).solution)  # (A')' \ B
    assert ref.mismatches(xt, X) == 0
    s0 = prov.lu_stats()
    xr = _take(prov, prov.mrdivide(hbt, hat))  # B' / A' = (A \ B)'
    s1 = prov.lu_stats()
    assert xr.shape == (nrhs, n) and ref.mismatches(xr.T, X) == 0
    assert s1["solve_path_factorizations"] == s0["solve_path_factorizations"] + 1
    assert s1["pivot_growth_fallbacks"] == s0["pivot_growth_fallbacks"]
    for h in (ha, hb, hat, hbt):
        prov.free(h)


@pytest.mark.parametrize("kind", ["identity", "reverse"])
def test_solves_with_empty_and_full_row_move_lists(prov, kind):
    for n, nrhs in ((300, 1), (1280, 5)):
        c = lu_case(n, n, kind)
        X, B = ref.rhs(c, nrhs, 13)
        _solve_and_check(prov, c, X, B, False)


@pytest.mark.parametrize("knobs,cases", KNOB_TABLE, ids=["+".join(f"{k}={v}" for k, v in kt[0].items()) for kt in KNOB_TABLE])
def test_per_call_knobs_return_the_same_bits(prov, knobs, cases):
    grid_wide = knobs.get("RMHIP_LU_FAST") == "0"
    forced = "RMHIP_LU_TEST_GROWTH" in knobs
    blocked_small = grid_wide or "RMHIP_NO_SMALL_SOLVE" in knobs
    for n, nrhs in cases:
        c, X, B = solve_case(n, nrhs)
        small = 2 <= n <= 64 and nrhs <= 16 and not blocked_small
        with env(knobs):
            # the grid-wide rule is not counted and leaves the multiplier statistic alone; the forced refactorisation counts one fallback,
            # no accepted solve-path factorisation, and has measured the multipliers before it "failed"
            _solve_and_check(prov, c, X, B, small, counted=not (grid_wide or forced), fallbacks=1 if forced else 0,
                             check_multiplier=not grid_wide)


@pytest.mark.parametrize("n", TRI_ORDERS)
def test_linsolve_triangular_hints_return_the_integer_solution(prov, n):
    """`lower` on the constructed unit-lower L, `upper` on U, and both `transposed` forms (solve.cpp swaps the hint): one
    k_trsm_fused launch up to 128, the recursive halving with dgemm above (trsm_split, trsm_lower_rec / trsm_upper_rec)."""
    from runmat_amd import ProviderLinsolveOptions as Opt

    c = lu_case(n, n)
    hl, hu = prov.upload(c.L), prov.upload(c.U)
    for nrhs in TRI_NRHS:
        X, _ = ref.rhs(c, nrhs, 17)
        for h, T, opt in ((hl, c.L, Opt(lower=True)), (hu, c.U, Opt(upper=True)),
                          (hl, c.L.T, Opt(lower=True, transposed=True)), (hu, c.U.T, Opt(upper=True, transposed=True))):
            hb = prov.upload((T @ X) + 0.0)
            got = _take(prov, prov.linsolve(h, hb, opt).solution)
            prov.free(hb)
            assert ref.mismatches(got, X) == 0, (n, nrhs, opt)
    prov.free(hl)
    prov.free(hu)


def test_linsolve_leaves_scalars_to_the_cpu_path(prov):
    from runmat_amd import ProviderError, ProviderLinsolveOptions as Opt

    with pytest.raises(ProviderError):
        prov.linsolve(prov.upload(np.array([[2.0]])), prov.upload(np.array([[6.0]])), Opt(lower=True))


# ---- 3c, 3d: fresh processes -------------------------------------------------------------------------------------------------------------------------
_CHILD_HEAD = f"""
import json, sys, time
import numpy as np
sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})
import lu_exact_ref as ref
from runmat_amd import HipProvider
t0 = time.time()
prov = HipProvider(0)
out = {{"mismatches": {{}}, "stats": {{}}}}
"""
_CHILD_TAIL = """
out["seconds"] = time.time() - t0
print(json.dumps(out))
prov.close()
"""
_CHILD_ORDERS = """
for n, nrhs in ORDERS:
    c = ref.case(n, n, 7)
    X, B = ref.rhs(c, nrhs, 11)
    s0 = prov.lu_stats()
    x = prov.download_matrix(prov.mldivide(prov.upload(c.A), prov.upload(B)))
    s1 = prov.lu_stats()
    key = f"{n}x{nrhs}"
    out["mismatches"][key] = ref.mismatches(x, X)
    out["stats"][key] = [s1["solve_path_factorizations"] - s0["solve_path_factorizations"],
                         s1["pivot_growth_fallbacks"] - s0["pivot_growth_fallbacks"], s1["last_max_multiplier"]]
"""
_CHILD_SUPER = """
n, nrhs = N, NRHS
def tri(upper):
    r = prov.random_integer_range(-1, 1, (n, n))
    h = prov.scalar_mul(r, 0.5); prov.free(r)
    t = prov.triu(h, 1) if upper else prov.tril(h, -1); prov.free(h)
    e = prov.eye((n, n))
    s = prov.elem_add(t, e); prov.free(t); prov.free(e)
    return s
rng = np.random.default_rng(8192)
L = tri(False)
Nn = tri(True)
d = prov.upload(rng.choice(np.array([2.0, 4.0, -2.0, -4.0]), size=(n, 1)))
U = prov.elem_mul(Nn, d); prov.free(Nn); prov.free(d)          # rows scaled: U = diag(d) N
A0 = prov.matmul(L, U); prov.free(L); prov.free(U)              # exact (tests/test_gpu_gemm_paths.py)
F = prov.flip(prov.reshape(A0, (64, n * n // 64)), [0]); prov.free(A0)   # column-major: rows reversed inside every aligned group of 64
A = prov.reshape(F, (n, n))
X = rng.integers(-XMAX, XMAX + 1, size=(n, nrhs)).astype(np.float64)
hx = prov.upload(X)
B = prov.matmul(A, hx); prov.free(hx)
prov.synchronize()
t1 = time.time()
s0 = prov.lu_stats()
x = prov.download_matrix(prov.mldivide(A, B))
s1 = prov.lu_stats()
out["solve_seconds"] = time.time() - t1
out["mismatches"]["8192"] = ref.mismatches(x, X)
out["stats"]["8192"] = [s1["solve_path_factorizations"] - s0["solve_path_factorizations"],
                        s1["pivot_growth_fallbacks"] - s0["pivot_growth_fallbacks"], s1["last_max_multiplier"]]
"""


def _child(body, switches, timeout):
    r = subprocess.run([sys.executable, "-c", _CHILD_HEAD + body + _CHILD_TAIL], env=dict(os.environ, **switches), capture_output=True,
                       text=True, timeout=timeout)
    # 134 / 139 / 124 / 137 (abort, segmentation fault, time limits) included: any failure of the child fails the test here, before
    # anything else is started on the device
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(switches, out)
    return out


@pytest.mark.parametrize("switches", PROCESS_SWITCHES, ids=["default", "rb+trsm-valu", "trsm-valu", "small-upd-0"])
def test_per_process_switches_return_the_same_bits(built, switches):
    out = _child(f"ORDERS = {PROCESS_ORDERS!r}\n" + _CHILD_ORDERS, switches, 300)
    assert set(out["mismatches"]) == {f"{n}x{nrhs}" for n, nrhs in PROCESS_ORDERS}
    assert not any(out["mismatches"].values()), out
    for key, (fast, fallbacks, multiplier) in out["stats"].items():
        assert (fast, fallbacks, multiplier) == (1, 0, 0.5), (key, out)


@pytest.mark.parametrize("plan", SUPER_PLANS, ids=["default", "super-0", "alternative-plan"])
def test_two_level_driver_returns_the_integer_solution(built, plan):
    """n = 8192 (kSuperMin is a constexpr of lu_plan.h: no smaller order reaches getrf_super), operands built on the device; only the
    n x 2 solution crosses the bus.  The bit budget holds for every matrix the construction can produce (45 of 53 bits)."""
    budget = ref.bit_budget_worst_case(SUPER_N, SUPER_NRHS, SUPER_XMAX)
    assert max(budget.values()) <= ref.BIT_CAP, budget
    out = _child(f"N, NRHS, XMAX = {SUPER_N}, {SUPER_NRHS}, {SUPER_XMAX}\n" + _CHILD_SUPER, plan, 300)
    assert out["mismatches"] == {"8192": 0}, out
    assert out["stats"]["8192"] == [1, 0, 0.5], out
