"""Host checks of the exact dyadic LU construction (tests/lu_exact_ref.py) for every host-built case of tests/test_gpu_lu_exact.py:
the bit budget is a CONDITION (<= 50 bits; thin out L, N or X before touching the cap), a plain numpy partial-pivoting LU and the
oracle's C restatement of host_lu.rs give back L, U and perm to the bit with every runner-up at most half the pivot, substitution
gives back X, and the comparison functions reject a one-ulp error, a dropped l*u term and two swapped rows.

The numpy LU runs its textbook rank-1 form (nb = 1) up to order 700 and at 1153; the other orders run it in 64-column panels (same
arithmetic, grouped; the rank-1 form at 2176 alone takes longer than this whole file should).  The oracle factors every order up to
1153 and skips 1280, 2100 and 2176 (cubic scalar C: ~3 s together)."""
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
