"""GPU parity of mode_values (include/rmhip.h, the "mode" section of order_ops.hip) against the Python restatement of mode.rs in
tests/mode_ref.py.  Every result is a copy of an input element or an integer count, so everything is compared by its bits: M, F, the
tied values, their offsets and counts.  Each case runs with every combination of want_frequency / want_ties (F switches a store, ties add
the run-length array and the compaction).  Inputs are small and seeded from the case's name; sizes sit around the places where the code
changes path: one row of a wave (64), the wave-per-line bound, the sort's tile SORT_C, the scan's MODE_CHUNK - both read from the source."""
import ctypes as C
import re
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mode_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
CSRC = Path(__file__).resolve().parent.parent / "runmat_amd" / "csrc"


def _constant(name):
    for f in ("mode_runs.h", "order_ops.hip"):
        m = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*(\d+)\s*;", (CSRC / f).read_text())
        if m:
            return int(m.group(1))
    raise AssertionError(f"{name} not found in the sources")


MODE_CHUNK = _constant("MODE_CHUNK")
SORT_C = _constant("SORT_C")
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def check(p, x, axes, rounded=None):
    """x as uploaded; `rounded`: what the provider stores (a precision-32 provider rounds on upload)"""
    x = np.asarray(x, dtype=np.float64)
    M, F, ties = ref.mode(x if rounded is None else rounded, axes)
    tv, to, tc = ref.ragged(ties)
    h = p.upload(x.reshape(-1, order="F"), x.shape if x.ndim else (1, 1))
    try:
        for want_f, want_t in FLAGS:
            r = p.mode_values(h, axes, want_frequency=want_f, want_ties=want_t)
            try:
                why = (axes, want_f, want_t, x.shape)
                assert tuple(r.values.shape) == M.shape, why
                assert np.array_equal(ref.bits(p.download(r.values)), ref.bits(M.reshape(-1, order="F"))), why
                assert (r.frequencies is not None) == want_f and (r.ties is not None) == want_t, why
                if want_f:
                    assert tuple(r.frequencies.shape) == F.shape, why
                    assert np.array_equal(ref.bits(p.download(r.frequencies)), ref.bits(F.reshape(-1, order="F"))), why
                if want_t:
                    assert r.ties.values.shape == tv.shape and np.array_equal(ref.bits(r.ties.values), ref.bits(tv)), why
                    assert r.ties.offsets == to and r.ties.counts == tc, why
            finally:
                p.free(r.values)
                if r.frequencies is not None:
                    p.free(r.frequencies)
    finally:
        p.free(h)


# ---- column lengths x alphabets ------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 63, 64, 65, SORT_C - 1, SORT_C, SORT_C + 1, 5000]
ALPHABETS = [2, 7, 1000, 0]  # 0: all-distinct doubles (F = 1, the whole sorted line tied)


@pytest.mark.parametrize("alphabet", ALPHABETS)
@pytest.mark.parametrize("n", LENGTHS)
def test_columns(prov, n, alphabet):
    rng = rng_of(f"columns-{n}-{alphabet}")
    cols = 3
    x = rng.permuted(rng.standard_normal((n, cols)) * 100.0, axis=0) if alphabet == 0 else (rng.integers(0, alphabet, (n, cols)) - alphabet // 2).astype(np.float64)
    if alphabet == 0:
        assert all(np.unique(x[:, j]).size == n for j in range(cols))
    check(prov, x, 0)


# ---- lines split over several chunks -------------------------------------------------------------------------------------------------
N_SPLIT = 3 * MODE_CHUNK + 17


def _split_majority(rng):  # one value is 60 % of the line: sorted, its run crosses two chunk boundaries
    k = int(0.6 * N_SPLIT)
    return np.concatenate([np.full(k, 5.0), rng.integers(-2000, 2000, N_SPLIT - k).astype(np.float64) * 3.0 + 1.0])


def _split_boundary(rng):  # the longest run ends exactly on a chunk boundary: MODE_CHUNK - 10 distinct smaller values, then a run of 10
    return np.concatenate([-1.0 - np.arange(MODE_CHUNK - 10), np.full(10, 0.5), 1.0 + np.arange(N_SPLIT - MODE_CHUNK)])


def _split_two_maximal(rng):  # two runs of 40 in different chunks (sorted positions ~100 and ~2.5 chunks): both tied, the smaller wins
    rest = N_SPLIT - 80
    lo = -10.0 - np.arange(100)
    mid = 10.0 + np.arange(int(2.5 * MODE_CHUNK) - 140)
    hi = 1e6 + np.arange(rest - lo.size - mid.size)
    return np.concatenate([lo, np.full(40, 0.0), mid, np.full(40, 9e5), hi])


SPLITS = {"majority": _split_majority, "boundary": _split_boundary, "two-maximal": _split_two_maximal}


@pytest.mark.parametrize("kind", list(SPLITS))
def test_split_lines(prov, kind):
    rng = rng_of(f"split-{kind}")
    line = SPLITS[kind](rng)
    assert line.size == N_SPLIT
    check(prov, rng.permutation(line).reshape(N_SPLIT, 1), 0)
    check(prov, rng.permutation(line).reshape(1, N_SPLIT), "all")


def test_three_split_lines_side_by_side(prov):
    rng = rng_of("split-three")
    x = np.stack([rng.permutation(SPLITS[k](rng)) for k in SPLITS], axis=1)
    check(prov, x, 0)
    check(prov, np.ascontiguousarray(x.T), 1)


# ---- strided lines, ranks, axes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 130), (100, 130)])
@pytest.mark.parametrize("dim", [0, 1])
def test_strided_lines(prov, shape, dim):
    rng = rng_of(f"strided-{shape}-{dim}")
    check(prov, rng.integers(0, 5, shape).astype(np.float64), dim)


@pytest.mark.parametrize("axes", [0, 1, 2, 3, 5, "all", "default"])
def test_rank_three(prov, axes):
    rng = rng_of(f"rank3-{axes}")
    x = rng.integers(0, 3, (3, 5, 4)).astype(np.float64)
    x[1, 2, 3] = np.nan
    check(prov, x, axes)


@pytest.mark.parametrize("shape", [(1, 1, 7), (1, 1), (4, 1)])
def test_default_axis(prov, shape):
    rng = rng_of(f"default-{shape}")
    check(prov, rng.integers(0, 3, shape).astype(np.float64), "default")


# ---- special values ----------------------------------------------------------------------------------------------------------------------
PAYLOAD_NAN = np.array([0x7FF800000000BEEF, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)


def test_all_nan_line_between_ordinary_ones(prov):
    x = np.array([[1.0, np.nan, 3.0], [1.0, PAYLOAD_NAN[0], 3.0], [2.0, PAYLOAD_NAN[1], 4.0], [2.0, np.nan, 4.0], [2.0, np.nan, 3.0]])
    check(prov, x, 0)
    check(prov, np.ascontiguousarray(x.T), 1)


def test_nan_as_the_most_frequent_entry_is_ignored(prov):
    x = np.array([np.nan, 4.0, np.nan, 2.0, np.nan, 4.0, PAYLOAD_NAN[0], 2.0, 7.0]).reshape(-1, 1)
    check(prov, x, 0)
    check(prov, x, "all")


def test_payload_nan_in_single_element_slices(prov):
    x = np.array([[1.0, PAYLOAD_NAN[0], -0.0, PAYLOAD_NAN[1]]])
    check(prov, x, 0)  # extent 1
    check(prov, x, 2)  # beyond the rank
    check(prov, x.reshape(4, 1), 1)


@pytest.mark.parametrize("first", [-0.0, 0.0])
def test_zero_keeps_the_sign_of_its_first_occurrence(prov, first):
    x = np.array([3.0, first, -first, 3.0, first, -first, 1.0]).reshape(-1, 1)
    check(prov, x, 0)
    wide = np.concatenate([np.arange(1.0, 301.0), [first, -first, -first], np.arange(-300.0, 0.0)]).reshape(-1, 1)  # zeros beyond one row of a wave
    check(prov, wide, 0)


def test_infinities_as_the_mode(prov):
    x = np.array([[np.inf, -np.inf, np.inf], [1.0, -np.inf, np.inf], [np.inf, 2.0, -np.inf], [2.0, -np.inf, -np.inf]])
    check(prov, x, 0)
    check(prov, x, 1)
    check(prov, x, "all")


# ---- empty operands ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axes", [((0, 3), 0), ((0, 3), 1), ((3, 0), "default"), ((3, 0), 0), ((3, 0), 1), ((0, 3), "all"), ((0, 3), 4), ((0, 1), "default")])
def test_empty_operands(prov, shape, axes):
    check(prov, np.empty(shape), axes)


# ---- precision-32 provider -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, precision="F32")
    yield p
    p.close()


@pytest.mark.parametrize("shape,axes", [((300, 4), 0), ((4, 300), 1), ((N_SPLIT, 1), "all"), ((5, 6), 3)])
def test_precision_32(prov32, shape, axes):
    rng = rng_of(f"f32-{shape}-{axes}")
    x = rng.integers(0, 9, shape) * 0.1  # tenths: distinct in f64, still distinct - and rounded - in f32
    x.reshape(-1)[::7] = np.nan
    x.reshape(-1)[1::11] = -0.0
    check(prov32, x, axes, rounded=x.astype(np.float32).astype(np.float64))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def live_bytes(p):
    t = p.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def test_refusals_leave_nothing(prov):
    from runmat_amd import ProviderError

    h = prov.upload(np.arange(12.0), (3, 4))
    ok = prov.mode_values(h, 0, want_frequency=True, want_ties=True)  # warms the pool
    prov.free(ok.values)
    prov.free(ok.frequencies)
    v, f, n = C.c_uint64(), C.c_uint64(), C.c_size_t()
    before = live_bytes(prov)
    lib, ctx = prov._lib, prov._ctx
    assert lib.rmhip_mode_values(ctx, h.buffer_id, 0, 1, 0, None, C.byref(f), C.byref(n), None, None, None, None) == 1
    assert lib.rmhip_mode_values(ctx, h.buffer_id, -3, 1, 0, C.byref(v), C.byref(f), C.byref(n), None, None, None, None) == 1
    assert lib.rmhip_mode_values(ctx, h.buffer_id, 0, 1, 1, C.byref(v), C.byref(f), C.byref(n), None, None, None, None) == 1
    assert live_bytes(prov) == before
    with pytest.raises(ProviderError):
        prov.mode_values(h, -1)
    assert live_bytes(prov) == before
    check(prov, np.arange(12.0).reshape(3, 4) % 3, 0)  # and the provider still serves
    prov.free(h)


def test_results_repeat_bit_for_bit(prov):
    rng = rng_of("repeat")
    x = rng.integers(0, 50, (N_SPLIT, 2)).astype(np.float64)
    h = prov.upload(x)
    got = []
    for _ in range(2):
        r = prov.mode_values(h, 0, want_frequency=True, want_ties=True)
        got.append((prov.download(r.values), prov.download(r.frequencies), r.ties.values, r.ties.offsets, r.ties.counts))
        prov.free(r.values)
        prov.free(r.frequencies)
    prov.free(h)
    assert all(np.array_equal(ref.bits(a), ref.bits(b)) for a, b in zip(got[0][:3], got[1][:3])) and got[0][3:] == got[1][3:]
