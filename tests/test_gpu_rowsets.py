"""GPU parity of the 'rows' forms of unique / union / setdiff / ismember (include/rmhip.h, order_ops.hip: one stable sort pass per column,
head flags over whole rows, row gather, lexicographic search) - bit-exact against the restatement of the CPU builtins (tests/rowset_ref.py).

Matrices are drawn from integer ranges of 2 to 4 values so that rows repeat, with NaN, -0.0, inf and NaNs of other payloads sprinkled in.
The shapes sit at the code's own boundaries: SORT_C = 2048 rows (LDS-local sort versus global steps), SCAN_CHUNK = 1024 ranks per head-flag
workgroup, and 65 536."""
import json
import zlib
from pathlib import Path

import numpy as np
import pytest

import rowset_ref as ref

pytestmark = pytest.mark.gpu

KATS = json.loads((Path(__file__).parent / "golden" / "rowset_kats.json").read_text())
ERR_SHAPE = 3
ORDERS = ("sorted", "stable")
OCCURRENCES = ("first", "last")


def arr(values, shape):
    return np.array([np.nan if v == "nan" else v for v in values], dtype=np.float64).reshape(shape, order="F")


def from_bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def up(p, x):
    x = np.asarray(x, dtype=np.float64)
    return p.upload(x.reshape(-1, order="F"), x.shape)


def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def draw(rng, rows, cols, span=None, lo=0):
    """integers of `span` values with the special values sprinkled in (a matrix of more than six elements)"""
    span = int(rng.integers(2, 5)) if span is None else span
    x = rng.integers(lo, lo + span, size=(rows, cols)).astype(np.float64)
    flat = x.reshape(-1)
    if flat.size > 6:
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 11))] = np.nan
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 13))] = -0.0
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 17))] = np.inf
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 19))] = from_bits(0xFFF8000000000ABC)
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 23))] = from_bits(0x7FF0000000000001)
    return x


def check_unique(p, x, rounded=None):
    """x as uploaded; `rounded`: what the provider stores (a precision-32 provider rounds on upload)"""
    h = up(p, x)
    for order in ORDERS:
        for occ in OCCURRENCES:
            got, want = p.unique_rows(h, order=order, occurrence=occ), ref.unique_rows(x if rounded is None else rounded, order, occ)
            for name, g, w in zip(("values", "ia", "ic"), got, want):
                assert same_bits(g, w), (order, occ, name, g.shape, w.shape)
    p.free(h)


def check_pair(p, a, b):
    ha, hb = up(p, a), up(p, b)
    for order in ORDERS:
        for name, got, want in (("union", p.union_rows(ha, hb, order=order), ref.union_rows(a, b, order)),
                                ("setdiff", p.setdiff_rows(ha, hb, order=order), ref.setdiff_rows(a, b, order))):
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert same_bits(g, w), (name, order, g.shape, w.shape)
    mask, loc = p.ismember_rows(ha, hb)
    want = ref.ismember_rows(a, b)
    assert mask.dtype == np.uint8 and mask.shape == want[0].shape and np.array_equal(mask, want[0]) and same_bits(loc, want[1])
    p.free(ha), p.free(hb)


# ---- the reference's known answers through the provider -------------------------------------------------------------------------------------
def test_reference_kats(prov):
    for k in KATS["unique"]:
        values, ia, ic = prov.unique_rows(up(prov, arr(k["a"], k["shape"])), order=k["order"], occurrence=k["occ"])
        assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"], k["name"]
        assert ia.ravel().tolist() == k["ia"] and ic.ravel().tolist() == k["ic"] and ia.shape == (len(k["ia"]), 1) and ic.shape == (k["shape"][0], 1), k["name"]
    for k in KATS["union"]:
        values, ia, ib = prov.union_rows(up(prov, arr(k["a"], k["a_shape"])), up(prov, arr(k["b"], k["b_shape"])), order=k["order"])
        assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"], k["name"]
        assert ia.ravel().tolist() == k["ia"] and ib.ravel().tolist() == k["ib"], k["name"]
    for k in KATS["setdiff"]:
        values, ia = prov.setdiff_rows(up(prov, arr(k["a"], k["a_shape"])), up(prov, arr(k["b"], k["b_shape"])), order=k["order"])
        assert values.shape == tuple(k["values_shape"]) and values.ravel(order="F").tolist() == k["values"] and ia.ravel().tolist() == k["ia"], k["name"]
    for k in KATS["ismember"]:
        mask, loc = prov.ismember_rows(up(prov, arr(k["a"], k["a_shape"])), up(prov, arr(k["b"], k["b_shape"])))
        assert mask.ravel().tolist() == k["mask"] and loc.ravel().tolist() == k["loc"] and loc.shape == tuple(k["loc_shape"]), k["name"]


@pytest.mark.parametrize("k", KATS["errors"], ids=lambda k: k["name"])
def test_reference_error_kats(prov, k):
    from runmat_amd import ProviderError

    a, b = up(prov, np.zeros(k["a_shape"])), up(prov, np.zeros(k.get("b_shape", [1, 1])))
    before = live_bytes(prov)
    call = {"unique": lambda: prov.unique_rows(a), "union": lambda: prov.union_rows(a, b), "setdiff": lambda: prov.setdiff_rows(a, b),
            "ismember": lambda: prov.ismember_rows(a, b)}[k["op"]]
    with pytest.raises(ProviderError) as e:
        call()
    assert e.value.code == ERR_SHAPE and str(e.value) == k["message"]
    assert live_bytes(prov) == before  # a refused call leaves no buffer behind
    prov.free(a), prov.free(b)


# ---- unique_rows ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 5), (2, 2), (4, 2), (1023, 3), (1025, 3), (2047, 2), (2048, 2), (2049, 7), (4097, 33), (70000, 2), (300, 1), (0, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_unique_rows(prov, shape):
    rng = np.random.default_rng(zlib.crc32(f"unique-rows-{shape}".encode()))
    check_unique(prov, draw(rng, *shape))


def test_unique_rows_of_a_transpose_view(prov):
    rng = np.random.default_rng(77)
    base = draw(rng, 3, 1500, span=2)  # the view's logical shape is [1500, 3]
    hb = up(prov, base)
    h = prov.transpose(hb)
    for got, want in zip(prov.unique_rows(h, order="stable", occurrence="last"), ref.unique_rows(base.T, "stable", "last")):
        assert same_bits(got, want)
    prov.free(h), prov.free(hb)


def test_rows_differing_in_the_last_column_only(prov):
    rng = np.random.default_rng(5)
    x = np.tile(np.array([[2.0, np.nan, -0.0, 7.0, 0.0]]), (1500, 1))
    x[:, -1] = rng.integers(0, 4, size=1500)
    check_unique(prov, x)


def test_zeros_and_nan_payloads_form_one_group_with_the_first_bits(prov):
    payloads = [from_bits(0x7FF8000000000000 + k) for k in range(1, 1301)]
    x = np.empty((1300, 3))
    x[:, 0] = np.where(np.arange(1300) % 2 == 0, -0.0, 0.0)
    x[:, 1] = payloads
    x[:, 2] = 4.0
    h = up(prov, x)
    for order in ORDERS:
        values, ia, ic = prov.unique_rows(h, order=order, occurrence="last")
        assert same_bits(values, x[:1]) and ia.tolist() == [[1300.0]] and np.all(ic == 1.0) and ic.shape == (1300, 1)
    prov.free(h)
    x[::3, 2] = 5.0  # two groups, interleaved: the first bits are those of rows 1 and 0
    check_unique(prov, x)


def test_all_rows_equal(prov):
    x = np.tile(np.array([[3.0, np.nan, -0.0]]), (1500, 1))
    h = up(prov, x)
    for order in ORDERS:
        for occ, ia in (("first", 1.0), ("last", 1500.0)):
            values, got_ia, ic = prov.unique_rows(h, order=order, occurrence=occ)
            assert same_bits(values, x[:1]) and got_ia.tolist() == [[ia]] and np.all(ic == 1.0)
    prov.free(h)
    check_unique(prov, x)


def test_all_rows_distinct(prov):
    rng = np.random.default_rng(11)
    x = draw(rng, 3000, 3, span=2)
    x[:, 1] = rng.permutation(3000)  # the middle column alone tells the rows apart
    check_unique(prov, x)
    assert ref.unique_rows(x)[0].shape == (3000, 3)


def test_a_group_straddling_a_chunk_of_ranks(prov):
    """ranks 0..999 and 1050..2049 are rows of their own, ranks 1000..1049 one group across the boundary at rank 1024"""
    rng = np.random.default_rng(13)
    lo = np.column_stack([np.zeros(1000), np.arange(1000.0)])
    mid = np.tile(np.array([[1.0, np.nan]]), (50, 1))
    hi = np.column_stack([np.full(1000, 2.0), np.arange(1000.0)])
    x = np.vstack([lo, mid, hi])[rng.permutation(2050)]
    want = ref.unique_rows(x)
    assert want[0].shape == (2001, 2) and np.array_equal(want[0][1000], [1.0, np.nan], equal_nan=True)
    check_unique(prov, x)


# ---- union_rows / setdiff_rows / ismember_rows -----------------------------------------------------------------------------------------------
def overlapping(rng, a, rows_b, cols, span):
    """rows_b rows: about half taken from a (when it has any), the rest drawn one value higher - b overlaps a partly"""
    fresh = draw(rng, rows_b, cols, span=span, lo=1)
    if a.shape[0] and rows_b:
        take = rng.random(rows_b) < 0.5
        fresh[take] = a[rng.integers(0, a.shape[0], size=int(take.sum()))]
    return fresh


@pytest.mark.parametrize("cols", [1, 3, 8])
@pytest.mark.parametrize("ra,rb", [(1, 1), (40, 25), (3000, 5000), (70000, 1000), (5, 0), (0, 5), (0, 0)], ids=str)
def test_two_operand_forms(prov, ra, rb, cols):
    rng = np.random.default_rng(zlib.crc32(f"pair-rows-{ra}-{rb}-{cols}".encode()))
    span = int(rng.integers(2, 5))
    a = draw(rng, ra, cols, span=span)
    check_pair(prov, a, overlapping(rng, a, rb, cols, span))


def test_rows_without_columns(prov):
    for ra, rb in ((5, 3), (0, 5), (5, 0), (0, 0)):
        check_pair(prov, np.zeros((ra, 0)), np.zeros((rb, 0)))


def test_ismember_rows_reports_the_lowest_row_of_b(prov):
    rng = np.random.default_rng(17)
    b = draw(rng, 2500, 2, span=3)  # at most some dozens of distinct rows: every one many times over
    a = draw(rng, 700, 2, span=4)
    mask, loc = prov.ismember_rows(up(prov, a), up(prov, b))
    want = ref.ismember_rows(a, b)
    assert np.array_equal(mask, want[0]) and same_bits(loc, want[1]) and 0 < mask.sum() < 700
    hit = int(np.flatnonzero(mask.ravel())[0])
    keys = [ref.row_key(r) for r in b]
    assert keys.index(ref.row_key(a[hit])) + 1 == loc[hit, 0] and keys.count(ref.row_key(a[hit])) > 1


def test_ismember_rows_of_rank_one_operands(prov):
    a, b = np.array([2.0, np.nan, 5.0, -0.0, 2.0]), np.array([7.0, 0.0, 2.0, 2.0, from_bits(0xFFF8000000000001)])
    ha, hb = prov.upload(a, (5,)), prov.upload(b, (5,))
    mask, loc = prov.ismember_rows(ha, hb)
    want = ref.ismember_rows(a, b)
    assert mask.shape == (5, 1) and np.array_equal(mask, want[0]) and same_bits(loc, want[1]) and loc.ravel().tolist() == [3.0, 5.0, 0.0, 2.0, 3.0]
    h2 = up(prov, b.reshape(5, 1))  # rank 1 against rank 2: the same rows
    assert same_bits(prov.ismember_rows(ha, h2)[1], want[1])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_nothing_behind(prov):
    from runmat_amd import ProviderError

    a, b, cube, flat0 = up(prov, np.zeros((6, 3))), up(prov, np.zeros((4, 2))), up(prov, np.zeros((2, 3, 2))), up(prov, np.zeros((5, 0)))
    before = live_bytes(prov)
    refused = [lambda: prov.union_rows(a, b), lambda: prov.setdiff_rows(a, b), lambda: prov.ismember_rows(a, b), lambda: prov.unique_rows(cube),
               lambda: prov.union_rows(cube, a), lambda: prov.setdiff_rows(a, cube), lambda: prov.ismember_rows(cube, a), lambda: prov.unique_rows(flat0)]
    for call in refused:
        with pytest.raises(ProviderError) as e:
            call()
        assert e.value.code == ERR_SHAPE
        assert live_bytes(prov) == before
    with pytest.raises(ProviderError, match=r"unique: Tensor data length 0 doesn't match shape \[5, 1\] \(5 elements\)"):
        prov.unique_rows(flat0)
    # and a served call releases its work arrays
    prov.unique_rows(a), prov.union_rows(a, a, order="stable"), prov.setdiff_rows(a, a), prov.ismember_rows(a, a)
    assert live_bytes(prov) == before


# ---- precision-32 provider ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, precision="F32")
    yield p
    p.close()


def test_precision_32(prov32):
    rng = np.random.default_rng(23)
    x = rng.integers(0, 4, size=(2100, 3)) * 0.1  # tenths: rounded on upload, still distinct in f32
    x.reshape(-1)[::7] = np.nan
    x.reshape(-1)[1::11] = -0.0
    rounded = x.astype(np.float32).astype(np.float64)
    assert not np.array_equal(x[~np.isnan(x)], rounded[~np.isnan(x)])
    check_unique(prov32, x, rounded)
    b = rng.integers(1, 5, size=(400, 3)) * 0.1
    hb, ha = up(prov32, b), up(prov32, x)
    rb = b.astype(np.float32).astype(np.float64)
    for g, w in zip(prov32.union_rows(ha, hb), ref.union_rows(rounded, rb)):
        assert same_bits(g, w)
    for g, w in zip(prov32.setdiff_rows(ha, hb, order="stable"), ref.setdiff_rows(rounded, rb, "stable")):
        assert same_bits(g, w)
    mask, loc = prov32.ismember_rows(ha, hb)
    assert np.array_equal(mask, ref.ismember_rows(rounded, rb)[0]) and same_bits(loc, ref.ismember_rows(rounded, rb)[1])


# ---- the shared row order still serves sort_rows --------------------------------------------------------------------------------------------
def test_sort_rows_is_unchanged(prov, oracle):
    rng = np.random.default_rng(29)
    m = draw(rng, 2049, 3, span=4)
    columns = [(c, "ascend") for c in range(3)]
    h = up(prov, m)
    before = prov.telemetry_snapshot()["kernel_launches"]
    r = prov.sort_rows(h, columns)
    launches = prov.telemetry_snapshot()["kernel_launches"] - before
    want_v, want_i = oracle.sort_rows(m, columns, "auto")
    assert same_bits(r.values, want_v) and np.array_equal(r.indices, want_i)
    # per key: the keys, the LDS sort, one global step and one LDS merge for the 4096-pair workspace, the composition - then the emit
    assert launches == 3 * 5 + 1
