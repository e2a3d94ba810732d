"""CPU twin of tests/test_gpu_scan_paths.py: the route tables of tests/scan_ref.py are the ones tests/cpp/scan_route_check.cpp pins
against reduce_plan.h; the sequential references are the oracle's `cumulative`; a numpy model of the chunked scan reproduces them - bit
for bit on the exact classes, within the derived bounds on the rounded ones - and each classical defect switched on in that model is
caught by the data classes and placements on some table row: the evidence that the GPU tests can fail."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import scan_ref as S

ROOT = Path(__file__).resolve().parent.parent
CHUNKED_ROWS = [r for r in S.SCAN_ROUTE_TABLE if r[5] > 1]
MODEL_ROWS = [r for r in CHUNKED_ROWS if S.numel(r) <= 2_500_000]


def test_route_tables_are_the_host_checks_tables(tmp_path):
    exe = tmp_path / "scan_route_check"
    c = subprocess.run(["g++", "-std=c++17", "-O1", f"-I{ROOT / 'runmat_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "scan_route_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def rows(tag):
        return [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(tag + " ")]

    gpu = rows("row")
    assert [(int(a), int(b), int(c), k, int(lpb), int(n), int(la)) for a, b, c, k, lpb, n, la, _ in gpu] == S.SCAN_ROUTE_TABLE
    assert [int(g[7]) for g in gpu] == [S.chunk_steps(row) for row in S.SCAN_ROUTE_TABLE]
    assert [(int(a), int(b), int(c), k, int(lpb), int(n), int(la)) for a, b, c, k, lpb, n, la in rows("host")] == S.SCAN_HOST_ROWS
    assert [(int(a), int(b), int(c), f, int(n), int(cl)) for a, b, c, f, n, cl in rows("ext")] == S.CUMEXT_ROUTE_TABLE
    assert S.Z_SPILL_ROW in S.SCAN_ROUTE_TABLE and "scan route ok" in r.stdout


def test_placements_follow_the_route():
    row = (40, 9001, 1, "staged", 32, 8, 3)
    assert S.chunk_steps(row) == 1152
    assert S.positions(row) == [1151, 1152, 2303, 8064, 9000, 0, 1, 63, 64, 8999]
    assert S.special_lines(row) == [0, 39, 31, 32] and S.inf_pairs(row) == [(1151, 8064)]
    big = (1, 4300000, 1, "chunks", 0, 263, 3)
    assert S.positions(big)[:10] == [16383, 16384, 32767, 262 * 16384, 4299999, 256 * 16384 - 1, 256 * 16384, 256 * 16384 + 1, 2047, 2048]
    assert S.inf_pairs(big) == [(16383, 262 * 16384), (256 * 16384 - 1, 256 * 16384)] and S.special_lines(big) == [0]
    assert S.positions((1, 1, 5, "short", 0, 1, 1)) == [0] and S.inf_pairs((1, 1, 5, "short", 0, 1, 1)) == []
    assert S.positions((1, 256, 3, "chunks", 0, 1, 1)) == [0, 1, 63, 64, 254, 255]
    assert S.special_lines(S.Z_SPILL_ROW) == [0, 65536, 65534, 65535] and S.special_lines((33, 4095, 2, "staged", 32, 1, 1)) == [0, 65, 31, 32]
    for row in S.SCAN_ROUTE_TABLE:
        for prod in (False, True):
            vs = S.variants(row, prod)
            singles = [sp for name, _, sp in vs if name.startswith("one_nan")]
            assert sorted(p for sp in singles for _, p, _ in sp) == sorted(S.positions(row)), row  # every position, once
            for sp in singles:
                assert len({ln for ln, _, _ in sp}) == len(sp), row  # one NaN per line
            assert all(p is None or p in S.hold_columns(row) for _, _, sp in vs for _, p, _ in sp), row
    ext = (2, 70001, 1, "thread", 273, 257)
    assert {256, 257, 513, 514, 2 * 257 - 1, 70000 - 257} <= set(S.cumext_columns(ext)) and S.cumext_columns((1, 1, 1, "wave", 1, 256)) == [0]


def test_data_classes():
    rng = np.random.default_rng(7)
    hold = [0, 5, 17, 299_999]
    x = S.exact_prod_lines(rng, 2, 300_000, hold)
    mag = np.abs(x)
    odd = np.isin(mag, [3.0, 5.0, 7.0])
    assert (odd.sum(axis=1) <= 8).all() and odd.any() and (np.log2(mag[~odd]) % 1 == 0).all() and (mag[:, hold] == 1.0).all()
    for lines in (x, x[:, ::-1]):  # forward prefixes are +-2^t times the odd entries met so far; backward ones stay bounded as well
        p = np.cumprod(lines, axis=1)
        assert np.abs(p).max() <= 2.0 ** 41 * 7.0 ** 8 and np.abs(p).min() >= 2.0 ** -41
    p = np.cumprod(x, axis=1)
    assert np.abs(p).max() <= 2.0 ** 20 * 7.0 ** 8 and np.abs(p).min() >= 2.0 ** -20
    assert (p[:, 1:] != p[:, :-1]).mean() > 0.95  # neighbouring prefixes differ (a sign, an exponent or an odd factor)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)  # f32 holds every prefix
    # any grouping: chunk products times prefix of chunk products
    c = x[:, :299_520].reshape(2, 260, 1152)
    tot = np.multiply.reduce(c, axis=2)
    assert np.array_equal(np.multiply.accumulate(tot, axis=1)[:, -1], p[:, 299_519])
    # leaving held entries out (omit mode) moves no exponent
    y = x.copy()
    y[:, hold] = 1.0
    q = np.cumprod(y, axis=1)
    assert np.array_equal(np.abs(q), np.abs(p))
    s = S.exact_sum_lines(rng, 3, 1000)
    assert np.signbit(s[0, 0]) and s[0, 0] == 0 and (np.signbit(s) & (s == 0)).sum() > 20 and np.abs(s).max() == 5 and np.array_equal(s, np.round(s))
    r = S.rounded_prod_lines(rng, 2, 100_000)
    assert np.abs(np.log2(np.abs(np.cumprod(r, axis=1)))).max() < 8.01 and np.abs(S.rounded_sum_lines(rng, 2, 1000)).max() < 1.0


def test_seq_scan_hand_cases():
    nan, inf = np.nan, np.inf
    x = np.array([[-0.0, -0.0, 2.0, nan, 3.0], [nan, nan, nan, nan, nan], [1.0, inf, 2.0, -inf, 1.0]])
    assert S.same_bits(S.seq_scan(x, False, False), [[0.0, 0.0, 2.0, nan, nan], [nan] * 5, [1.0, inf, inf, nan, nan]])
    assert S.same_bits(S.seq_scan(x, False, True), [[0.0, 0.0, 2.0, 2.0, 5.0], [0.0] * 5, [1.0, inf, inf, nan, nan]])
    assert S.same_bits(S.seq_scan(x, True, True), [[-0.0, 0.0, 0.0, 0.0, 0.0], [1.0] * 5, [1.0, inf, inf, -inf, -inf]])
    z = np.array([[2.0, 0.0, -3.0, inf, 1.0]])
    assert S.same_bits(S.seq_scan(z, True, False), [[2.0, 0.0, -0.0, nan, nan]]) and S.same_bits(S.seq_scan(z, True, True), [[2.0, 0.0, -0.0, nan, nan]])
    assert not S.same_bits([0.0], [-0.0]) and S.same_bits([np.float64("nan")], [-np.float64("nan")]) and not S.same_bits([1.0], [nan])
    # gamma_3 * (1 + 2 + 3) is 2.25 * 2^-50, and 2^-50 is the spacing of doubles at 6
    ok, ratio = S.scan_error_ratios(np.array([[1.0, 3.0, 6.0 + 3 * 2.0 ** -50]]), np.array([[1.0, 2.0, 3.0]]), False)
    assert not ok and 1.3 < ratio < 1.34
    ok, ratio = S.scan_error_ratios(np.array([[1.0, 3.0, 6.0 + 2.0 ** -50]]), np.array([[1.0, 2.0, 3.0]]), False)
    assert ok and 0.44 < ratio < 0.45


@pytest.mark.parametrize("row", [r for r in S.SCAN_ROUTE_TABLE if r[:3] in ((7, 5000, 1), (17, 9001, 3), (1, 70001, 3))], ids=S.row_id)
def test_references_are_the_oracles(row, oracle):
    """`seq_scan` of scan-ordered lines, put back in memory order, is the oracle's `cumulative`: both classes, both ops, directions and
    NaN modes, with every placement"""
    pre, n, post = row[:3]
    shape, dim = S.realise(pre, n, post)
    rng = np.random.default_rng(S.numel(row) + 3)
    for prod in (False, True):
        bases = [S.exact_lines(rng, row, prod), (S.rounded_prod_lines if prod else S.rounded_sum_lines)(rng, pre * post, n)]
        for base in bases:
            for name, modes, specials in S.variants(row, prod):
                lines = S.apply_specials(base, specials)
                for reverse in (False, True):
                    x = S.unslice(S.to_memory(lines, reverse), pre, n, post).reshape(shape, order="F")
                    for mode in modes:
                        omit = mode == "omit"
                        want = S.slices(oracle.cumulative(x, max(dim, 0), prod=prod, reverse=reverse, omitnan=omit), pre, n, post)
                        got = S.to_memory(S.seq_scan(lines, prod, omit), reverse)
                        assert S.same_bits(got, want), (row, prod, name, reverse, mode, S.where_differs(got, want))
                        if name == "whole_nan" and omit:
                            ln = S.special_lines(row)[-1]
                            assert S.same_bits(got[ln], np.full(n, 1.0 if prod else 0.0))


@pytest.mark.parametrize("row", MODEL_ROWS, ids=S.row_id)
def test_model_reproduces_the_references(row):
    pre, n, post = row[:3]
    chunk = S.chunk_steps(row)
    rng = np.random.default_rng(S.numel(row) + 5)
    for prod in (False, True):
        base = S.exact_lines(rng, row, prod)
        for name, modes, specials in S.variants(row, prod):
            lines = S.apply_specials(base, specials)
            for reverse in (False, True):
                for mode in modes:
                    omit = mode == "omit"
                    want = S.to_memory(S.seq_scan(lines, prod, omit), reverse)
                    got = S.chunked_model(S.to_memory(lines, reverse), prod, reverse, omit, chunk)
                    assert S.same_bits(got, want), (row, prod, name, reverse, mode, S.where_differs(got, want))
        lines = (S.rounded_prod_lines if prod else S.rounded_sum_lines)(rng, pre * post, n)
        for reverse in (False, True):
            got = S.to_memory(S.chunked_model(S.to_memory(lines, reverse), prod, reverse, False, chunk), reverse)
            ok, ratio = S.scan_error_ratios(got, lines, prod)
            assert ok and ratio > 0, (row, prod, reverse, ratio)  # within the bound, and not the sequential bits (the grouping differs)


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_every_seeded_defect_is_caught(defect):
    """with the defect switched on, the model misses the exact class's reference on some row, variant, direction and mode - for sums
    AND for products, except the sign of zero, which only a sum can get wrong"""
    caught = {}
    for prod in (False, True):
        for row in MODEL_ROWS:
            rng = np.random.default_rng(S.numel(row) + 5)
            base = S.exact_lines(rng, row, prod)
            for name, modes, specials in S.variants(row, prod):
                lines = S.apply_specials(base, specials)
                for reverse in (False, True):
                    for mode in modes:
                        omit = mode == "omit"
                        want = S.to_memory(S.seq_scan(lines, prod, omit), reverse)
                        got = S.chunked_model(S.to_memory(lines, reverse), prod, reverse, omit, S.chunk_steps(row), defect)
                        if not S.same_bits(got, want) and prod not in caught:
                            caught[prod] = (S.row_id(row), name, reverse, mode)
                if prod in caught:
                    break
            if prod in caught:
                break
    print(f"defect {defect}: caught by {caught}")
    assert False in caught, defect
    assert True in caught or defect == "negative_zero_kept", defect
    if defect == "second_trip_restarts":
        assert all(S.SCAN_ROUTE_TABLE[[S.row_id(r) for r in S.SCAN_ROUTE_TABLE].index(c[0])][5] > S.CARRY_TRIP for c in caught.values())
    if defect == "nan_total_not_carried":
        assert all(c[1].startswith("one_nan") or c[1] in ("many_nan", "whole_nan") for c in caught.values()) and all(c[3] == "include" for c in caught.values())


def test_cumext_cases_have_what_they_promise():
    rng = np.random.default_rng(11)
    row = (7, 5000, 1, "thread", 19, 264)
    cases = dict(S.cumext_cases(rng, row))
    cols = S.cumext_columns(row)
    assert {263, 264, 527, 528, 4999 - 264, 4999 - 263, 0, 4999} <= set(cols)
    assert (cases["ties"][0::2][:, cols] == 9).all() and (cases["ties"][1::2][:, cols] == -9).all() and np.abs(np.delete(cases["ties"], cols, axis=1)).max() == 3
    z = cases["zeros"]
    assert (z[:, cols] == 0).all() and np.signbit(z[0, cols[0]]) != np.signbit(z[0, cols[1]]) and np.signbit(z[0, cols[0]]) != np.signbit(z[2, cols[0]])
    assert (z[0::2] >= 0).all() and (z[1::2] <= 0).all()
    n = cases["nans"]
    assert np.isnan(n[4]).all() and np.isnan(n[3, :70]).all() and not np.isnan(n[3, 70:]).any() and np.isnan(n[0, cols[1]]) and not np.isnan(n[1]).any()
    assert np.isinf(cases["infs"]).sum() > 2 * len(cols)
