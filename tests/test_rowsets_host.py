"""The 'rows' forms of unique / union / setdiff / ismember without a GPU: the Python restatement of the CPU builtins (tests/rowset_ref.py)
reproduces the reference's own unit tests (tests/golden/rowset_kats.json), agrees with numpy's `unique(axis=0)` and with the element oracle
on one-column inputs, and keeps the edge rules (zeros, NaN payloads, kept bits, rows without columns, ranks); the shared comparison header
(runmat_amd/csrc/row_keys.h) passes its C++ sweep, plain and under the address / undefined-behaviour sanitizers; and the four entry points
exist in the ABI table and in the three mirrors."""
import json
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import rowset_ref as ref

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "rowset_kats.json").read_text())


def arr(values, shape):
    return np.array([np.nan if v == "nan" else v for v in values], dtype=np.float64).reshape(shape, order="F")


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def from_bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


# ---- the reference's known answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KATS["unique"], ids=lambda k: k["name"])
def test_unique_kats(k):
    values, ia, ic = ref.unique_rows(arr(k["a"], k["shape"]), k["order"], k["occ"])
    assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"]
    assert ia.shape == (len(k["ia"]), 1) and ia.ravel().tolist() == k["ia"] and ic.shape == (k["shape"][0], 1) and ic.ravel().tolist() == k["ic"]


@pytest.mark.parametrize("k", KATS["union"], ids=lambda k: k["name"])
def test_union_kats(k):
    values, ia, ib = ref.union_rows(arr(k["a"], k["a_shape"]), arr(k["b"], k["b_shape"]), k["order"])
    assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"]
    assert ia.ravel().tolist() == k["ia"] and ib.ravel().tolist() == k["ib"] and ia.shape == (len(k["ia"]), 1) and ib.shape == (len(k["ib"]), 1)


@pytest.mark.parametrize("k", KATS["setdiff"], ids=lambda k: k["name"])
def test_setdiff_kats(k):
    values, ia = ref.setdiff_rows(arr(k["a"], k["a_shape"]), arr(k["b"], k["b_shape"]), k["order"])
    assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"] and ia.ravel().tolist() == k["ia"]


@pytest.mark.parametrize("k", KATS["ismember"], ids=lambda k: k["name"])
def test_ismember_kats(k):
    mask, loc = ref.ismember_rows(arr(k["a"], k["a_shape"]), arr(k["b"], k["b_shape"]))
    assert mask.dtype == np.uint8 and mask.ravel().tolist() == k["mask"] and loc.ravel().tolist() == k["loc"] and loc.shape == tuple(k["loc_shape"])


@pytest.mark.parametrize("k", KATS["errors"], ids=lambda k: k["name"])
def test_error_kats(k):
    a = np.zeros(k["a_shape"])
    fn = {"unique": lambda: ref.unique_rows(a), "union": lambda: ref.union_rows(a, np.zeros(k.get("b_shape", [1, 1]))),
          "setdiff": lambda: ref.setdiff_rows(a, np.zeros(k.get("b_shape", [1, 1]))), "ismember": lambda: ref.ismember_rows(a, np.zeros(k.get("b_shape", [1, 1])))}[k["op"]]
    with pytest.raises(ref.RowsError) as e:
        fn()
    assert str(e.value) == k["message"]


# ---- against independent implementations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_agrees_with_numpy_on_integer_matrices(seed):
    rng = np.random.default_rng(zlib.crc32(f"rowsets-numpy-{seed}".encode()))
    for _ in range(25):
        rows, cols = int(rng.integers(1, 40)), int(rng.integers(1, 5))
        x = rng.integers(-2, 3, size=(rows, cols)).astype(np.float64)
        values, ia, ic = ref.unique_rows(x, "sorted", "first")
        want_v, want_i, want_c = np.unique(x, axis=0, return_index=True, return_inverse=True)
        assert np.array_equal(values, want_v) and np.array_equal(ia.ravel(), want_i + 1.0) and np.array_equal(ic.ravel(), np.ravel(want_c) + 1.0)
        stable = ref.unique_rows(x, "stable", "last")
        assert np.array_equal(stable[0], x[np.sort(want_i)])  # the same rows in order of first appearance
        assert np.array_equal(x[stable[1].ravel().astype(int) - 1], stable[0]) and np.array_equal(stable[0][stable[2].ravel().astype(int) - 1], x)
        assert all(int(stable[1][g, 0]) - 1 == max(np.flatnonzero((x == stable[0][g]).all(axis=1))) for g in range(stable[0].shape[0]))


POOL = np.array([0.0, -0.0, 1.0, -1.0, 2.5, np.inf, -np.inf, np.nan, from_bits(0xFFF8000000000001), 5e-324])


@pytest.mark.parametrize("seed", range(6))
def test_agrees_with_the_element_oracle_on_one_column(seed):
    from oracle import oracle as orc

    rng = np.random.default_rng(zlib.crc32(f"rowsets-elements-{seed}".encode()))
    for _ in range(20):
        na, nb = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        a, b = (rng.choice(POOL[: int(rng.integers(2, POOL.size + 1))], size=(n, 1)) for n in (na, nb))
        for order in ("sorted", "stable"):
            if na:
                for occ in ("first", "last"):
                    assert all(same_bits(g, w) for g, w in zip(ref.unique_rows(a, order, occ), orc.unique(a, order, occ)))
            assert all(same_bits(g, w) for g, w in zip(ref.union_rows(a, b, order), orc.union(a, b, order)))
            assert all(same_bits(g, w) for g, w in zip(ref.setdiff_rows(a, b, order), orc.setdiff(a, b, order)))
        mask, loc = ref.ismember_rows(a, b)
        want = orc.ismember(a, b)
        assert np.array_equal(mask, want[0]) and np.array_equal(loc, want[1])


def test_the_sort_key_orders_as_the_comparison():
    rng = np.random.default_rng(zlib.crc32(b"rowsets-order-key"))
    for _ in range(60):
        rows = rng.choice(POOL[: int(rng.integers(2, POOL.size + 1))], size=(int(rng.integers(0, 30)), int(rng.integers(0, 4)))).tolist()
        assert sorted(range(len(rows)), key=lambda r: ref.order_key(rows[r])) == ref.sorted_by_compare(rows)
        for a in rows[:6]:
            for b in rows[:6]:
                c = ref.compare_numeric_rows(a, b)
                assert (ref.order_key(a) < ref.order_key(b)) == (c < 0) and (ref.order_key(a) == ref.order_key(b)) == (c == 0)


# ---- the edge rules ---------------------------------------------------------------------------------------------------------------------
def test_zeros_and_nan_payloads_are_one_key_and_the_first_bits_stay():
    nan_a, nan_b = from_bits(0x7FF8000000000000), from_bits(0xFFF8000000000ABC)
    x = np.array([[-0.0, nan_b], [0.0, nan_a], [1.0, 2.0], [0.0, nan_b]])
    for order in ("sorted", "stable"):
        for occ, ia in (("first", [1.0, 3.0]), ("last", [4.0, 3.0])):
            values, got_ia, ic = ref.unique_rows(x, order, occ)
            assert same_bits(values, np.array([[-0.0, nan_b], [1.0, 2.0]])) and got_ia.ravel().tolist() == ia and ic.ravel().tolist() == [1.0, 1.0, 2.0, 1.0]
    assert ref.canonicalize_f64(nan_b) == ref.NAN_KEY and ref.canonicalize_f64(-0.0) == 0 and ref.row_key([-0.0, nan_b]) == ref.row_key([0.0, nan_a])
    assert [k for _, k in ref._rows_of(x, 4, 2)] == [ref.row_key(r) for r in x]  # the keys taken for a whole tensor at once are the scalar ones
    # NaN sorts after every number, inf included; the zeros tie in column 0, so column 1 decides between them
    y = np.array([[np.nan, 0.0], [np.inf, 0.0], [0.0, 5.0], [-0.0, 4.0], [-np.inf, 1.0]])
    assert same_bits(ref.unique_rows(y)[0], y[[4, 3, 2, 1, 0]])
    # union keeps a's bits for a row both hold, setdiff drops it, ismember reports b's lowest row
    b = np.array([[3.0, 3.0], [0.0, nan_a], [-0.0, nan_a]])
    values, ia, ib = ref.union_rows(x, b, "stable")
    assert same_bits(values, np.array([[-0.0, nan_b], [1.0, 2.0], [3.0, 3.0]])) and ia.ravel().tolist() == [1.0, 3.0] and ib.ravel().tolist() == [1.0]
    values, ia = ref.setdiff_rows(x, b)
    assert same_bits(values, np.array([[1.0, 2.0]])) and ia.tolist() == [[3.0]]
    mask, loc = ref.ismember_rows(x, b)
    assert mask.ravel().tolist() == [1, 1, 0, 1] and loc.ravel().tolist() == [2.0, 2.0, 0.0, 2.0]


def test_rows_without_columns_and_empty_operands():
    e = ref.unique_rows(np.zeros((0, 4)))
    assert e[0].shape == (0, 4) and e[1].shape == (0, 1) and e[2].shape == (0, 1)
    assert [t.shape for t in ref.unique_rows(np.zeros((0, 0)))] == [(0, 0), (0, 1), (0, 1)]
    with pytest.raises(ref.RowsError, match=r"unique: Tensor data length 0 doesn't match shape \[5, 1\] \(5 elements\)"):
        ref.unique_rows(np.zeros((5, 0)))
    # the two-operand forms: every zero-column row is the same row
    z5, z0 = np.zeros((5, 0)), np.zeros((0, 0))
    for order in ("sorted", "stable"):
        v, ia, ib = ref.union_rows(z5, np.zeros((3, 0)), order)
        assert v.shape == (1, 0) and ia.tolist() == [[1.0]] and ib.shape == (0, 1)
        v, ia, ib = ref.union_rows(z0, z5, order)
        assert v.shape == (1, 0) and ia.shape == (0, 1) and ib.tolist() == [[1.0]]
        assert [t.shape for t in ref.union_rows(z0, z0, order)] == [(0, 0), (0, 1), (0, 1)]
        v, ia = ref.setdiff_rows(z5, z0, order)
        assert v.shape == (1, 0) and ia.tolist() == [[1.0]]
        assert [t.shape for t in ref.setdiff_rows(z5, np.zeros((2, 0)), order)] == [(0, 0), (0, 1)]
    mask, loc = ref.ismember_rows(z5, np.zeros((2, 0)))
    assert mask.ravel().tolist() == [1] * 5 and loc.ravel().tolist() == [1.0] * 5
    assert ref.ismember_rows(z5, z0)[0].ravel().tolist() == [0] * 5
    # empty operands with columns
    a = np.array([[1.0, 2.0], [1.0, 2.0], [0.0, 1.0]])
    v, ia, ib = ref.union_rows(a, np.zeros((0, 2)))
    assert np.array_equal(v, [[0.0, 1.0], [1.0, 2.0]]) and ia.ravel().tolist() == [3.0, 1.0] and ib.shape == (0, 1)
    v, ia, ib = ref.union_rows(np.zeros((0, 2)), a, "stable")
    assert np.array_equal(v, [[1.0, 2.0], [0.0, 1.0]]) and ia.shape == (0, 1) and ib.ravel().tolist() == [1.0, 3.0]
    assert ref.setdiff_rows(np.zeros((0, 2)), a)[0].shape == (0, 2) and np.array_equal(ref.setdiff_rows(a, np.zeros((0, 2)), "stable")[1].ravel(), [1.0, 3.0])
    assert ref.ismember_rows(np.zeros((0, 2)), a)[0].shape == (0, 1)


def test_ranks():
    for bad in (np.zeros(4), np.zeros((2, 2, 1)), np.float64(3.0)):
        with pytest.raises(ref.RowsError):
            ref.unique_rows(bad)
        with pytest.raises(ref.RowsError):
            ref.union_rows(bad, np.zeros((2, 2)))
        with pytest.raises(ref.RowsError):
            ref.setdiff_rows(np.zeros((2, 2)), bad)
    # ismember: rank 0 / 1 / 2 as (1, 1) / (n, 1) / (r, c)
    mask, loc = ref.ismember_rows(np.array([2.0, 5.0, 2.0]), np.array([[7.0], [2.0], [2.0]]))
    assert mask.shape == (3, 1) and mask.ravel().tolist() == [1, 0, 1] and loc.ravel().tolist() == [2.0, 0.0, 2.0]
    mask, loc = ref.ismember_rows(np.float64(7.0), np.array([1.0, 7.0]))
    assert mask.tolist() == [[1]] and loc.tolist() == [[2.0]]
    with pytest.raises(ref.RowsError):
        ref.ismember_rows(np.zeros((2, 2, 1)), np.zeros((2, 2)))
    with pytest.raises(ref.RowsError, match="same number of columns"):
        ref.ismember_rows(np.zeros((3, 2)), np.zeros(3))


# ---- the shared comparison header ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]], ids=["plain", "sanitized"])
def test_row_keys_header(tmp_path, flags):
    exe = tmp_path / "row_keys_check"
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, f"-I{ROOT / 'runmat_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "row_keys_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "row keys ok" in r.stdout, r.stdout + r.stderr


def test_header_key_matches_sort_key():
    """row_keys.h's key is order_ops.hip's sort_key(x, 0, 0) line by line: NaN -> ~0, zeros merged, negative -> ~bits, else bits | sign bit."""
    src = (ROOT / "runmat_amd" / "csrc" / "order_ops.hip").read_text()
    hdr = (ROOT / "runmat_amd" / "csrc" / "row_keys.h").read_text()
    assert '#include "row_keys.h"' in src
    for piece in ("if (x != x) return", "if (x == 0.0) x = 0.0;", "(u >> 63) ? ~u : (u | 0x8000000000000000ull)"):
        assert piece in src and piece in hdr, piece


# ---- the entry points and their mirrors ---------------------------------------------------------------------------------------------------
def test_entry_points_and_mirrors_exist():
    from runmat_amd import HipProvider, _lib

    for name, method in (("rmhip_unique_rows", "unique"), ("rmhip_union_rows", "union"), ("rmhip_setdiff_rows", "setdiff"), ("rmhip_ismember_rows", "ismember")):
        assert name in _lib.SIGNATURES and tuple(_lib.SERVES[name]) == (method,), name
    for method in ("unique_rows", "union_rows", "setdiff_rows", "ismember_rows"):
        assert callable(getattr(HipProvider, method, None)), method
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    for method in ("unique_rows", "set_union_rows", "setdiff_rows", "ismember_rows"):
        assert re.search(rf"\b{method}\s*\(const GpuTensorHandle&", hpp), method
    assert "rows: not served" not in hpp
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    for name in ("rmhip_unique_rows", "rmhip_union_rows", "rmhip_setdiff_rows", "rmhip_ismember_rows"):
        assert f"{name}(self.ctx" in shim, name
    assert "'rows' form is not served" not in shim
