"""GPU parity of modulate_constellation and modulate_bits_constellation (include/rmhip.h "modulation", runmat_amd/csrc/comms_ops.hip)
against the Python restatement of the CPU loops in tests/comms_ref.py.  Results are copies of table entries, so everything is compared
by its bits; every table carries a few -0.0 and denormal entries to prove it.  A refused call must name the CPU's message for the FIRST
failing element in traversal order, leave no buffer behind, and be followed by a valid call that succeeds.  Sizes sit where the code
changes path - a 16-byte load, a wave, one workgroup's span, a ballot word, a tile, the LDS table budget - all read from the sources."""
import re
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import comms_ref as ref  # noqa: E402
from runmat_amd import HipProvider, ProviderError, _lib  # noqa: E402

pytestmark = pytest.mark.gpu
CSRC = Path(__file__).resolve().parent.parent / "runmat_amd" / "csrc"


def _constant(name):
    for f in ("modulate_check.h", "comms_ops.hip"):
        m = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*(\d+)\s*;", (CSRC / f).read_text())
        if m:
            return int(m.group(1))
    raise AssertionError(f"{name} not found in the sources")


BLOCK = _constant("MOD_BLOCK")
LOAD_BYTES = _constant("MOD_LOAD_BYTES")
TILE = _constant("MOD_BIT_TILE")
BPS_MAX = _constant("MOD_BPS_MAX")
LDS_LAST = _constant("MOD_TABLE_LDS_BYTES") // 16  # the last order whose table is staged in LDS
UNROLL = _constant("MOD_SYM_UNROLL")
SPAN64 = BLOCK * UNROLL * LOAD_BYTES // 8          # elements one workgroup takes per trip: f64 storage
SPAN32 = BLOCK * UNROLL * LOAD_BYTES // 4          # f32 storage
WAVE64, WAVE32 = 64 * LOAD_BYTES // 8, 64 * LOAD_BYTES // 4  # elements of one wave's load: the span the lanes exchange symbols over


@pytest.fixture(scope="module")
def prov32(built):
    import os

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@pytest.fixture(scope="module")
def tables():
    """order -> 2 * order doubles; entries 0, 1 and the last hold -0.0 and denormals.  Built once, never changed."""
    cache = {}

    def table(order):
        if order not in cache:
            t = rng_of(f"table-{order}").standard_normal(2 * order)
            t[0], t[1] = -0.0, 5e-324
            t[-1], t[-2] = -0.0, -2.5e-310
            t.setflags(write=False)
            cache[order] = t
        return cache[order]

    return table


def f32(x):
    with np.errstate(over="ignore"):  # 1e300 stored as f32 is +Inf
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def flat(x):
    return np.asarray(x, dtype=np.float64).reshape(-1, order="F")


def run_symbols(p, h, data, shape, table, round32=False):
    """the call on handle `h` against the restatement on `data` (what the handle holds, linear order)"""
    want, second = ref.modulate_constellation(data, shape, f32(table) if round32 else table)
    if isinstance(want, str):
        before = live_bytes(p)
        with pytest.raises(ProviderError) as e:
            p.modulate_constellation(h, table)
        assert e.value.code == _lib.ERR_INVALID and str(e.value) == want, (str(e.value), want, second)
        assert live_bytes(p) == before
        return
    out = p.modulate_constellation(h, table)
    try:
        assert tuple(out.shape) == tuple(second) and p.is_complex(out)
        got = p.download(out).view(np.float64)
        assert np.array_equal(ref.bits(got), ref.bits(want)), (shape, len(table) // 2)
    finally:
        p.free(out)


def check_symbols(p, x, shape, table, round32=False):
    x = flat(x)
    h = p.upload(x, shape)
    try:
        run_symbols(p, h, f32(x) if round32 else x, shape, table, round32)
    finally:
        p.free(h)


def check_bits(p, x, shape, rows, bps, table, round32=False):
    x = flat(x)
    h = p.upload(x, shape)
    try:
        want, second = ref.modulate_bits_constellation(f32(x) if round32 else x, shape, rows, bps, f32(table) if round32 else table)
        if isinstance(want, str):
            before = live_bytes(p)
            with pytest.raises(ProviderError) as e:
                p.modulate_bits_constellation(h, rows, bps, table)
            assert e.value.code == _lib.ERR_INVALID and str(e.value) == want, (str(e.value), want, second)
            assert live_bytes(p) == before
            return
        out = p.modulate_bits_constellation(h, rows, bps, table)
        try:
            assert tuple(out.shape) == tuple(second) and p.is_complex(out)
            got = p.download(out).view(np.float64)
            assert np.array_equal(ref.bits(got), ref.bits(want)), (shape, bps, len(table) // 2)
        finally:
            p.free(out)
    finally:
        p.free(h)


def bits_of(symbols, bps):
    """MSB first, group after group"""
    s = np.asarray(symbols, dtype=np.uint64)
    return ((s[:, None] >> np.arange(bps - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64).reshape(-1)


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------
LENGTHS64 = [0, 1, 2, 3, 63, 64, 65, WAVE64 - 1, WAVE64 + 1, BLOCK * LOAD_BYTES // 8 + 1, SPAN64 - 1, SPAN64, SPAN64 + 1, 3 * SPAN64 + 1]
ORDERS = [2, 4, 64, LDS_LAST, LDS_LAST + 1]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", LENGTHS64)
def test_symbols_lengths_and_orders(prov, tables, n, order):
    x = rng_of(f"sym-{n}-{order}").integers(0, order, n).astype(np.float64)
    if n:
        x[-1] = order - 1  # the table's last pair is read
    check_symbols(prov, x, (n, 1), tables(order))


@pytest.mark.parametrize("order", [4, LDS_LAST + 1])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 65, WAVE32 - 1, WAVE32 + 1, BLOCK * LOAD_BYTES // 4 + 3, SPAN32 - 1, SPAN32, SPAN32 + 1, 3 * SPAN32 + 1])
def test_symbols_f32_storage(prov32, tables, n, order):
    x = rng_of(f"sym32-{n}-{order}").integers(0, order, n).astype(np.float64)
    if n:
        x[0] = 1e-10  # stored as f32 it is still within 1e-9 of 0
    check_symbols(prov32, x, (n, 1), tables(order), round32=True)


@pytest.mark.parametrize("shape", [(77, 1), (1, 77), (3, 5, 7), (0, 3)])
def test_symbols_shapes(prov, tables, shape):
    x = rng_of(f"shape-{shape}").integers(0, 64, int(np.prod(shape))).astype(np.float64)
    check_symbols(prov, x, shape, tables(64))


def test_symbols_from_lazy_views(prov, tables):
    base = rng_of("views").integers(0, 64, (5, 9)).astype(np.float64)
    h = prov.upload(flat(base), base.shape)
    try:
        t = prov.transpose(h)
        try:
            run_symbols(prov, t, flat(base.T), (9, 5), tables(64))
        finally:
            prov.free(t)
        r = prov.repmat(h, [2, 3])
        try:
            run_symbols(prov, r, flat(np.tile(base, (2, 3))), (10, 27), tables(64))
        finally:
            prov.free(r)
    finally:
        prov.free(h)


def test_symbols_from_a_lazy_random_normal(prov, tables):
    """a lazy random_normal handle is materialised on use; normals are no integers, so the call is refused at the restatement's element"""
    h = prov.random_normal([2048, 1])
    try:
        with pytest.raises(ProviderError) as e:
            prov.modulate_constellation(h, tables(4))
        want, index = ref.modulate_constellation(prov.download(h), (2048, 1), tables(4))
        assert index is not None and e.value.code == _lib.ERR_INVALID and str(e.value) == want
    finally:
        prov.free(h)


@pytest.mark.parametrize("order", [8, 64, LDS_LAST + 1])
def test_symbol_edge_values(prov, tables, order):
    """every edge value alone among valid symbols, in a lane of the vector loop and in the scalar tail"""
    n = WAVE64 + 71
    base = rng_of(f"edges-{order}").integers(0, order, n).astype(np.float64)
    for v in ref.symbol_edges(order):
        for pos in (36, 37, WAVE64 + 3, n - 1):  # both slots of a load, a second wave load, the scalar tail
            x = base.copy()
            x[pos] = v
            check_symbols(prov, x, (n, 1), tables(order))


def test_symbol_edge_values_f32_storage(prov32, tables):
    base = rng_of("edges32").integers(0, 8, 71).astype(np.float64)
    for v in ref.symbol_edges(8) + [1e-10]:
        x = base.copy()
        x[37] = v
        check_symbols(prov32, x, (71, 1), tables(8), round32=True)


def test_symbols_first_failing_element_wins_across_workgroups(prov, tables):
    n = 4 * SPAN64 + 3
    base = rng_of("first").integers(0, 4, n).astype(np.float64)
    lo, hi = 100, 100 + 2 * SPAN64  # two workgroups apart
    classes = {"finite": np.nan, "integer": 0.5, "range": 4.0}
    for a, b in [("finite", "integer"), ("integer", "finite"), ("range", "finite"), ("finite", "range"), ("range", "integer"), ("integer", "range")]:
        x = base.copy()
        x[lo], x[hi] = classes[a], classes[b]
        want, index = ref.modulate_constellation(x, (n, 1), tables(4))
        assert index == lo and want == ref.SYMBOL_MESSAGES[["finite", "integer", "range"].index(a)]
        check_symbols(prov, x, (n, 1), tables(4))
        check_symbols(prov, base, (n, 1), tables(4))  # a following valid call on the same context succeeds
    x = base.copy()
    x[n - 1], x[0] = np.inf, 7.0  # the scalar tail against the first vector lane
    check_symbols(prov, x, (n, 1), tables(4))


# ---- bits ------------------------------------------------------------------------------------------------------------------------------
BIT_CASES = [(1, 2), (2, 4), (3, 8), (3, 5), (4, 16), (5, 32), (7, 128), (8, 256), (12, 4096), (12, 1000), (32, LDS_LAST + 1), (32, 3)]


def group_counts(bps):
    """the last group just before, across and just after a ballot word's end, a tile's end and the second tile's end, then three tiles and a bit"""
    counts = {1}
    for boundary in (64, TILE, 2 * TILE):
        counts.update({boundary // bps, boundary // bps + 1, boundary // bps + 2})
    counts.add(3 * TILE // bps + 5)
    return sorted(c for c in counts if c > 0)


@pytest.mark.parametrize("bps,order", BIT_CASES)
def test_bits_group_counts(prov, tables, bps, order):
    rng = rng_of(f"bits-{bps}-{order}")
    for groups in group_counts(bps):
        symbols = rng.integers(0, order, groups)
        symbols[-1] = order - 1
        check_bits(prov, bits_of(symbols, bps), (groups * bps, 1), groups * bps, bps, tables(order))


@pytest.mark.parametrize("bps,order", [(3, 8), (32, 3), (12, 4096)])
def test_bits_f32_storage(prov32, tables, bps, order):
    rng = rng_of(f"bits32-{bps}-{order}")
    for groups in (1, TILE // bps + 1, 2 * TILE // bps + 2):
        x = bits_of(rng.integers(0, order, groups), bps)
        x[int(np.argmin(x))] = 1e-10  # a zero bit (if any): stored as f32 it is still within 1e-9 of 0
        check_bits(prov32, x, (groups * bps, 1), groups * bps, bps, tables(order), round32=True)


@pytest.mark.parametrize("tail", [(1,), (3,), (2, 2)])
def test_bits_shapes(prov, tables, tail):
    bps, rows = 3, 3 * 231  # 693 rows: channels start inside ballot words, groups straddle them
    channels = int(np.prod(tail))
    x = bits_of(rng_of(f"bitshape-{tail}").integers(0, 8, channels * rows // bps), bps)
    check_bits(prov, x, (rows,) + tail, rows, bps, tables(8))


def test_bits_empty(prov, tables):
    check_bits(prov, np.empty(0), (4, 0), 4, 2, tables(4))


def test_bit_edge_values(prov, tables):
    """every edge value as the first, a middle and the last bit of a group (the other bits 0 and 1), one bit per symbol too"""
    base = bits_of(rng_of("bitedges").integers(0, 8, 50), 3)
    for v in ref.bit_edges():
        for pos in (66, 67, 68):  # group 22: elements 66 .. 68, behind the first ballot word
            x = base.copy()
            x[pos] = v
            check_bits(prov, x, (150, 1), 150, 3, tables(8))
        x = base.copy()
        x[100] = v
        check_bits(prov, x, (150, 1), 150, 1, tables(2))


def test_bits_first_failing_element_wins(prov, tables):
    bps, groups = 3, 3 * TILE // 3 + 40
    n = groups * bps
    table = tables(5)  # symbols 5, 6, 7 are out of range
    base = bits_of(rng_of("bitfirst").integers(0, 5, groups), bps)
    k = 30
    far = (2 * TILE + 100) // bps  # a group two tiles on: another workgroup

    def with_range_error(x, g):
        x[g * bps:(g + 1) * bps] = [1, 1, 0]

    for other in (k + 1, far):
        # a range error in group k, a non-bit in a later group: the range error, at group k's last bit
        x = base.copy()
        with_range_error(x, k)
        x[other * bps] = 2.0
        assert ref.modulate_bits_constellation(x, (n, 1), n, bps, table) == (ref.BIT_MESSAGES[2], k * bps + bps - 1)
        check_bits(prov, x, (n, 1), n, bps, table)
        # the reverse: a non-bit in group k, a range error later
        x = base.copy()
        x[k * bps + 2] = np.nan
        with_range_error(x, other)
        assert ref.modulate_bits_constellation(x, (n, 1), n, bps, table) == (ref.BIT_MESSAGES[0], k * bps + 2)
        check_bits(prov, x, (n, 1), n, bps, table)
        check_bits(prov, base, (n, 1), n, bps, table)  # a following valid call on the same context succeeds
    # inside one group: a non-bit last bit of a group whose other bits already exceed the order
    x = base.copy()
    x[k * bps:(k + 1) * bps] = [1, 1, 0.5]
    assert ref.modulate_bits_constellation(x, (n, 1), n, bps, table) == (ref.BIT_MESSAGES[1], k * bps + 2)
    check_bits(prov, x, (n, 1), n, bps, table)
    # two classes of bit errors, two tiles apart, both orders
    for a, b in ((np.inf, 2.0), (2.0, np.inf)):
        x = base.copy()
        x[50], x[50 + 2 * TILE] = a, b
        check_bits(prov, x, (n, 1), n, bps, table)


# ---- refusals on the host --------------------------------------------------------------------------------------------------------------
def refused(p, call, code, text):
    before = live_bytes(p)
    with pytest.raises(ProviderError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert live_bytes(p) == before


def test_host_side_refusals(prov, tables):
    t4 = tables(4)
    h = prov.upload(np.zeros(8), (4, 2))
    c = prov.complex_from_real(h)
    try:
        for bad in (t4[:7], t4[:0]):
            refused(prov, lambda: prov.modulate_constellation(h, bad), _lib.ERR_INVALID, "modulate_constellation " + ref.TABLE_MESSAGE)
            refused(prov, lambda: prov.modulate_bits_constellation(h, 4, 2, bad), _lib.ERR_INVALID, "modulate_bits_constellation " + ref.TABLE_MESSAGE)
        refused(prov, lambda: prov.modulate_bits_constellation(h, 4, 0, t4), _lib.ERR_INVALID, ref.GROUPING_MESSAGE)
        refused(prov, lambda: prov.modulate_bits_constellation(h, 0, 2, t4), _lib.ERR_INVALID, ref.GROUPING_MESSAGE)
        refused(prov, lambda: prov.modulate_bits_constellation(h, 4, 3, t4), _lib.ERR_INVALID, ref.MULTIPLE_MESSAGE)
        refused(prov, lambda: prov.modulate_bits_constellation(h, 8, 2, t4), _lib.ERR_INVALID, ref.ROWS_MESSAGE)
        refused(prov, lambda: prov.modulate_constellation(c, t4), _lib.ERR_UNSUPPORTED, "modulate_constellation requires a real-valued symbol input")
        refused(prov, lambda: prov.modulate_bits_constellation(c, 4, 2, t4), _lib.ERR_UNSUPPORTED, "modulate_bits_constellation requires a real-valued bit input")
        # the CPU's order: a complex input before a bad table, a bad table before the grouping
        refused(prov, lambda: prov.modulate_bits_constellation(c, 4, 0, t4[:7]), _lib.ERR_UNSUPPORTED, "real-valued bit input")
        refused(prov, lambda: prov.modulate_bits_constellation(h, 4, 0, t4[:7]), _lib.ERR_INVALID, ref.TABLE_MESSAGE)
        check_symbols(prov, np.zeros(8), (4, 2), t4)  # the context still serves
    finally:
        prov.free(c)
        prov.free(h)
    wide = prov.upload(np.zeros(BPS_MAX + 1), (BPS_MAX + 1, 1))
    try:
        refused(prov, lambda: prov.modulate_bits_constellation(wide, BPS_MAX + 1, BPS_MAX + 1, t4), _lib.ERR_UNSUPPORTED, "bits per symbol")
    finally:
        prov.free(wide)
    gone = prov.upload(np.zeros(4), (4, 1))
    prov.free(gone)
    refused(prov, lambda: prov.modulate_constellation(gone, t4), _lib.ERR_NOT_FOUND, "buffer not found")
    refused(prov, lambda: prov.modulate_bits_constellation(gone, 4, 2, t4), _lib.ERR_NOT_FOUND, "buffer not found")


def test_reference_kats_on_the_device(prov):
    import json

    kats = json.loads((Path(__file__).resolve().parent / "golden" / "modulation_kats.json").read_text())["cases"]
    for kat in kats:
        table = np.array(kat["constellation"], dtype=np.float64)
        if kat["hook"] == "modulate_constellation":
            check_symbols(prov, kat["data"], tuple(kat["shape"]), table)
        elif kat.get("index", 0) is None:  # refused before the data is read
            h = prov.upload(np.array(kat["data"], dtype=np.float64), tuple(kat["shape"]))
            try:
                refused(prov, lambda: prov.modulate_bits_constellation(h, kat["input_rows"], kat["bits_per_symbol"], table), _lib.ERR_INVALID, kat["error"])
            finally:
                prov.free(h)
        else:
            check_bits(prov, kat["data"], tuple(kat["shape"]), kat["input_rows"], kat["bits_per_symbol"], table)
