"""GPU checks of the shape and indexing hooks on complex-interleaved tensors (rmhip_complex_reshape / _transpose / _permute / _repmat /
_gather_linear / _scatter_linear / _circshift / _flip / _cat; tensor_ops.hip, move_kernels.h) against the numpy model
(tests/complex_move_ref.py).  Everything is data movement: every comparison is on the bits of the interleaved doubles, and every operand
carries a block of special values (signed zeros, infinities, a NaN with a payload, the smallest subnormal, a value near the largest)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_move_ref as ref  # noqa: E402
from test_gpu_parity import BINARY_LIBM_ULP  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ERR_INVALID, ERR_UNSUPPORTED, ERR_SHAPE, ERR_NOT_FOUND = 1, 2, 3, 5
NAN_PAYLOAD = np.array([0x7ff8000000abc123], dtype=np.uint64).view(np.float64)[0]
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, NAN_PAYLOAD, 5e-324, 1.7e308])


def data(shape, seed=0, f32=False):
    """Seeded complex data of `shape`; the leading elements are the special values (real parts ascending through SPECIAL, imaginary parts
    descending, so the two parts of an element differ)."""
    n = int(np.prod(shape, dtype=np.int64))
    rng = np.random.default_rng(1000 + seed)
    re, im = rng.standard_normal(n), rng.standard_normal(n)
    if f32:
        re, im = re.astype(np.float32).astype(np.float64), im.astype(np.float32).astype(np.float64)
    else:
        k = min(n, SPECIAL.size)
        re[:k], im[:k] = SPECIAL[:k], SPECIAL[::-1][:k]
    z = np.empty(n, dtype=np.complex128)
    z.real, z.imag = re, im
    return z.reshape(tuple(shape), order="F")


def up_c(prov, z):
    z = np.asarray(z, dtype=np.complex128)
    f = ref.flat(z)
    shape = z.shape if z.ndim >= 2 else (z.size, 1)
    hr, hi = prov.upload(f.real.copy(), shape), prov.upload(f.imag.copy(), shape)
    h = prov.complex_from_real_imag(hr, hi)
    prov.free(hr)
    prov.free(hi)
    return h


def up_r(prov, x, shape=None):
    x = np.asarray(x, dtype=np.float64)
    return prov.upload(x.ravel(order="F"), shape if shape is not None else (x.shape if x.ndim >= 2 else (x.size, 1)))


def live(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def lib_shape(prov, h):
    """The shape the library holds for the id (a handle's own `shape` may come from the call's arguments)."""
    return prov._handle(h.buffer_id).shape


def check(prov, h, want, what, free=True):
    """`h` is complex, has the model's shape and holds its bits."""
    assert prov.is_complex(h), what
    assert tuple(lib_shape(prov, h)) == tuple(want.shape), (what, lib_shape(prov, h), want.shape)
    assert np.array_equal(prov.download(h).view(np.float64).view(np.uint64), ref.bits(want)), what
    if free:
        prov.free(h)


def raises(code, f, needle=None):
    from runmat_amd import ProviderError

    with pytest.raises(ProviderError) as e:
        f()
    assert e.value.code == code, (e.value.code, str(e.value))
    if needle is not None:
        assert needle in str(e.value), str(e.value)


def test_upload_helper_keeps_the_special_bits(prov):
    z = data((3, 5))
    h = up_c(prov, z)
    check(prov, h, z, "upload")


# ---- transpose / permute: every path of the dispatcher --------------------------------------------------------------------------------------
# tiled with tile edges on both sides | merge to a plain copy | index copy (output dim 0 of 300 / 600, the other extent below 8: the steps of
# the 8-byte per-lane ladder; 200: one element per lane) | the flat kernel (dim 0 below 128, 64 or more outer coordinates)
@pytest.mark.parametrize("shape", [(8, 8), (63, 65), (64, 64), (65, 63), (129, 257), (1, 9), (9, 1), (7, 300), (2, 600), (3, 200), (1030, 5)])
def test_transpose(prov, shape):
    z = data(shape, seed=shape[0])
    h = up_c(prov, z)
    check(prov, prov.complex_transpose(h), ref.transpose(z), ("transpose", shape))
    check(prov, prov.complex_permute(h, (1, 0)), ref.permute(z, (1, 0)), ("permute", shape))
    prov.free(h)


@pytest.mark.parametrize("order", [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)])
def test_permute_three_dimensions_under_every_order(prov, order):
    z = data((5, 66, 9), seed=3)
    h = up_c(prov, z)
    check(prov, prov.complex_permute(h, order), ref.permute(z, order), order)
    prov.free(h)


def test_permute_other_ranks_and_refusals(prov):
    z = data((3, 4, 5, 6), seed=4)
    h = up_c(prov, z)
    check(prov, prov.complex_permute(h, (3, 1, 0, 2)), ref.permute(z, (3, 1, 0, 2)), "rank 4")
    prov.free(h)
    m = data((4, 5), seed=5)
    hm = up_c(prov, m)
    check(prov, prov.complex_permute(hm, (2, 0, 1)), ref.permute(m, (2, 0, 1)), "order longer than the rank")
    e = np.zeros((0, 3), dtype=np.complex128)
    he = up_c(prov, e)
    check(prov, prov.complex_permute(he, (1, 0)), ref.permute(e, (1, 0)), "empty permute")
    check(prov, prov.complex_transpose(he), ref.transpose(e), "empty transpose")
    before = live(prov)
    raises(ERR_INVALID, lambda: prov.complex_permute(hm, (0, 2)), "permute: invalid dimension index 3")
    raises(ERR_INVALID, lambda: prov.complex_permute(hm, (1, 1)), "permute: duplicate dimension index 2 encountered")
    raises(ERR_INVALID, lambda: prov.complex_permute(hm, (0,)), "permute: order length must be at least the number of dimensions")
    h3 = up_c(prov, data((2, 2, 2)))
    before3 = live(prov)
    raises(ERR_UNSUPPORTED, lambda: prov.complex_transpose(h3), "transpose: only 2D supported")
    assert live(prov) == before3
    prov.free(h3)
    assert live(prov) == before
    prov.free(hm)
    prov.free(he)


# ---- reshape ------------------------------------------------------------------------------------------------------------------------------------
def test_reshape_returns_the_same_id_and_keeps_the_storage_kind(prov):
    z = data((6, 4), seed=6)
    h = up_c(prov, z)
    r = prov.complex_reshape(h, (3, 8))
    assert r.buffer_id == h.buffer_id and prov.is_complex(r)
    check(prov, r, z.reshape((3, 8), order="F"), "reshape", free=False)
    raises(ERR_SHAPE, lambda: prov.complex_reshape(r, (5, 5)), "reshape: element count mismatch (25 vs 24)")
    check(prov, r, z.reshape((3, 8), order="F"), "reshape after a refusal")


# ---- repmat -------------------------------------------------------------------------------------------------------------------------------------
def test_repmat(prov):
    z = data((3, 2), seed=7)
    h = up_c(prov, z)
    for reps in ((2,), (2, 3), (1, 1, 4)):
        check(prov, prov.complex_repmat(h, reps), ref.repmat(z, reps), reps)
    empty = prov.complex_repmat(h, (0, 2))  # a zero factor: an empty complex tensor of the tiled shape
    check(prov, empty, ref.repmat(z, (0, 2)), "zero factor")
    prov.free(h)
    s = data((1, 1), seed=8)
    hs = up_c(prov, s)
    check(prov, prov.complex_repmat(hs, (257, 3)), ref.repmat(s, (257, 3)), "scalar")
    raises(ERR_INVALID, lambda: prov.complex_repmat(hs, ()), "repmat: replication factors must be specified")  # the sibling's rule and message
    prov.free(hs)


# ---- circshift ------------------------------------------------------------------------------------------------------------------------------------
def test_circshift(prov):
    z = data((257, 3), seed=9)
    h = up_c(prov, z)
    for shifts in ((1,), (-1, 2), (1000, -7), (3, 1, 5, -2)):  # the last: more shifts than dimensions
        check(prov, prov.complex_circshift(h, shifts), ref.circshift(z, shifts), shifts)
    prov.free(h)


def test_circshift_of_a_long_line_is_fftshift(prov):
    n = 2 ** 20 + 3
    z = data((n, 1), seed=10)
    h = up_c(prov, z)
    out = prov.complex_circshift(h, (n // 2,))
    got = prov.download(out)
    assert np.array_equal(got.view(np.uint64), np.fft.fftshift(prov.download(h)).view(np.uint64))
    check(prov, out, ref.circshift(z, (n // 2,)), "half shift")
    prov.free(h)


# ---- flip -----------------------------------------------------------------------------------------------------------------------------------------
def test_flip(prov):
    z = data((37, 6), seed=11)
    h = up_c(prov, z)
    for axes in ((0,), (1,), (0, 1), (0, 0), (4,)):  # named twice: flipped back; beyond the rank: an extent-1 dimension
        check(prov, prov.complex_flip(h, axes), ref.flip(z, axes), axes)
    prov.free(h)
    r = data((1, 300), seed=12)
    hr = up_c(prov, r)
    for axes in ((0,), (1,)):
        check(prov, prov.complex_flip(hr, axes), ref.flip(r, axes), ("row", axes))
    prov.free(hr)


# ---- cat ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_cat(prov, dim):
    shapes = {1: [(3, 5), (4, 5), (1, 5)], 2: [(3, 5), (3, 2), (3, 9)], 3: [(3, 5), (3, 5), (3, 5, 2)]}[dim]
    zs = [data(s, seed=20 + k) for k, s in enumerate(shapes)]
    hs = [up_c(prov, z) for z in zs]
    check(prov, prov.complex_cat(dim, hs[:2]), ref.cat(dim, zs[:2]), ("two", dim))
    check(prov, prov.complex_cat(dim, hs), ref.cat(dim, zs), ("three", dim))
    for h in hs:
        prov.free(h)


def test_cat_refusals(prov):
    a, b = up_c(prov, data((3, 5))), up_c(prov, data((4, 6)))
    r = up_r(prov, np.ones((3, 5)))
    before = live(prov)
    raises(ERR_SHAPE, lambda: prov.complex_cat(1, [a, b]), "cat: dimension 2 mismatch between input 1 (size 5) and input 2 (size 6)")
    raises(ERR_INVALID, lambda: prov.complex_cat(1, [a]), "cat: at least two input arrays are required")
    raises(ERR_INVALID, lambda: prov.complex_cat(0, [a, a]), "cat: dimension must be >= 1")
    raises(ERR_UNSUPPORTED, lambda: prov.complex_cat(1, [a, r]))  # a real input among complex ones: the caller gathers
    raises(ERR_UNSUPPORTED, lambda: prov.complex_cat(1, [r, a]))
    assert live(prov) == before
    for h in (a, b, r):
        prov.free(h)


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------------
# fewer than 4096 indices: the bounds check is a host loop; from 4096 on it rides in the kernel
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097])
def test_gather(prov, n):
    z = data((50, 41), seed=30)
    h = up_c(prov, z)
    idx = np.random.default_rng(n).integers(0, z.size, n).astype(np.uint32)
    if n > 2:
        idx[1] = idx[0]          # repeats
        idx[-1] = z.size - 1     # the last element
    shape = (n, 1) if n % 2 else (n // 2, 2)
    check(prov, prov.complex_gather_linear(h, idx, shape), ref.gather(z, idx, shape), n)
    prov.free(h)


@pytest.mark.parametrize("n", [100, 5000])
def test_gather_out_of_bounds_names_the_first_position_and_leaves_nothing(prov, n):
    z = data((50, 41), seed=31)
    h = up_c(prov, z)
    before = live(prov)
    for pos in (0, n - 1):
        idx = np.zeros(n, dtype=np.uint32)
        idx[pos] = z.size
        raises(ERR_INVALID, lambda: prov.complex_gather_linear(h, idx, (n, 1)), f"gather_linear: index {z.size} (position {pos}) out of bounds")
        assert live(prov) == before
    idx = np.full(n, z.size + 7, dtype=np.uint32)  # every position offends: the first one is named
    raises(ERR_INVALID, lambda: prov.complex_gather_linear(h, idx, (n, 1)), f"gather_linear: index {z.size + 7} (position 0) out of bounds")
    raises(ERR_SHAPE, lambda: prov.complex_gather_linear(h, np.zeros(n, dtype=np.uint32), (n + 1, 1)), "gather_linear: output shape holds")
    assert live(prov) == before
    prov.free(h)


# ---- scatter --------------------------------------------------------------------------------------------------------------------------------------
# 4095 indices: host-resolved duplicates; 4096 into 5000 elements (5000 <= 64 * 4096): owners resolved on the device; 4096 into 2^20 elements
# (more than 64 per index): the host path again
@pytest.mark.parametrize("n,target", [(4095, 5000), (4096, 5000), (4096, 2 ** 20)])
def test_scatter_last_duplicate_wins(prov, n, target):
    z, v = data((target, 1), seed=40), data((n, 1), seed=41)
    rng = np.random.default_rng(n + target)
    idx = rng.integers(0, target, n).astype(np.uint32)
    idx[: n // 2] = rng.integers(0, 37, n // 2)  # many duplicates among few targets
    idx[-1] = idx[0]
    ht, hv = up_c(prov, z), up_c(prov, v)
    prov.complex_scatter_linear(ht, idx, hv)
    check(prov, ht, ref.scatter(z, idx, v), (n, target))
    check(prov, hv, v, "values untouched")


@pytest.mark.parametrize("n", [100, 4096])
def test_scatter_refusals_leave_the_target_untouched(prov, n):
    z, v = data((5000, 1), seed=42), data((n, 1), seed=43)
    ht, hv = up_c(prov, z), up_c(prov, v)
    rt, rv = up_r(prov, np.zeros((5000, 1))), up_r(prov, np.ones((n, 1)))
    before = live(prov)
    for pos in (0, n - 1):
        idx = np.arange(n, dtype=np.uint32)
        idx[pos] = 5000
        raises(ERR_INVALID, lambda: prov.complex_scatter_linear(ht, idx, hv), f"scatter_linear: index 5000 (position {pos}) out of bounds")
        check(prov, ht, z, "target after an out-of-bounds index", free=False)
    idx = np.arange(n, dtype=np.uint32)
    raises(ERR_UNSUPPORTED, lambda: prov.complex_scatter_linear(ht, idx, rv), "scatter_linear: storage mismatch target=ComplexInterleaved values=Real")
    raises(ERR_UNSUPPORTED, lambda: prov.complex_scatter_linear(rt, idx, hv), "scatter_linear: storage mismatch target=Real values=ComplexInterleaved")
    raises(ERR_SHAPE, lambda: prov.complex_scatter_linear(ht, idx[:-1], hv),
           f"scatter_linear: values raw length {2 * n} does not match index count {n - 1} for lane factor 2")
    assert live(prov) == before
    check(prov, ht, z, "target after the refusals")
    assert np.array_equal(prov.download(rt), np.zeros(5000))
    for h in (hv, rt, rv):
        prov.free(h)


# ---- every entry point: real operands, unknown ids ----------------------------------------------------------------------------------------------------
def test_real_operands_and_unknown_ids_are_refused_with_nothing_left(prov):
    z = up_c(prov, data((4, 3)))
    r = up_r(prov, np.ones((4, 3)))
    gone = up_c(prov, data((4, 3)))
    prov.free(gone)
    idx = np.arange(3, dtype=np.uint32)
    before = live(prov)
    calls = {
        "reshape": lambda h: prov.complex_reshape(h, (3, 4)),
        "transpose": lambda h: prov.complex_transpose(h),
        "permute": lambda h: prov.complex_permute(h, (1, 0)),
        "repmat": lambda h: prov.complex_repmat(h, (2, 2)),
        "gather_linear": lambda h: prov.complex_gather_linear(h, idx, (3, 1)),
        "circshift": lambda h: prov.complex_circshift(h, (1,)),
        "flip": lambda h: prov.complex_flip(h, (0,)),
    }
    for name, f in calls.items():
        raises(ERR_UNSUPPORTED, lambda: f(r), f"rmhip_{name} serves it")
        raises(ERR_NOT_FOUND, lambda: f(gone))
        assert live(prov) == before, name
    raises(ERR_UNSUPPORTED, lambda: prov.complex_cat(1, [r, r]), "rmhip_cat serves")
    raises(ERR_NOT_FOUND, lambda: prov.complex_cat(1, [z, gone]))
    raises(ERR_UNSUPPORTED, lambda: prov.complex_scatter_linear(r, idx, r), "rmhip_scatter_linear serves")
    raises(ERR_NOT_FOUND, lambda: prov.complex_scatter_linear(gone, idx, z))
    raises(ERR_NOT_FOUND, lambda: prov.complex_scatter_linear(z, idx, gone))
    assert live(prov) == before
    assert tuple(lib_shape(prov, r)) == (4, 3)  # the refused reshape changed nothing
    prov.free(z)
    prov.free(r)


def test_real_entry_points_still_refuse_complex_storage(prov):
    """The dispatch rule lives in the caller (the Rust shim chooses by handle_storage): changing that is a deliberate change of this test."""
    z = up_c(prov, data((4, 3)))
    raises(ERR_UNSUPPORTED, lambda: prov.permute(z, (1, 0)))
    raises(ERR_UNSUPPORTED, lambda: prov.circshift(z, (1,)))
    raises(ERR_UNSUPPORTED, lambda: prov.gather_linear(z, np.arange(2, dtype=np.uint32), (2, 1)))
    prov.free(z)


# ---- a chain that stays on the device ---------------------------------------------------------------------------------------------------------------
def test_shifted_half_spectrum_magnitudes_stay_resident(prov):
    rows, cols = 1024, 6
    x = np.random.default_rng(77).standard_normal((rows, cols))
    hx = up_r(prov, x)
    z = prov.fft_dim(hx, None, 0)
    zh = prov.download(z).reshape((rows, cols), order="F")  # the reference input of every later step
    downloaded = prov.telemetry_snapshot()["download_bytes"]
    uploaded = prov.telemetry_snapshot()["upload_bytes"]
    shifted = prov.complex_circshift(z, (512,))
    idx = (np.arange(513)[:, None] + rows * np.arange(cols)[None, :]).ravel(order="F").astype(np.uint32)  # the first 513 rows of every column
    half = prov.complex_gather_linear(shifted, idx, (513, cols))
    t = prov.complex_transpose(half)
    mag = prov.complex_unary("abs", t)
    snap = prov.telemetry_snapshot()
    assert snap["download_bytes"] == downloaded and snap["upload_bytes"] == uploaded  # (the index slice is not a tensor upload)
    want = ref.transpose(ref.gather(ref.circshift(zh, (512,)), idx, (513, cols)))
    check(prov, t, want, "moves", free=False)
    assert not prov.is_complex(mag) and tuple(lib_shape(prov, mag)) == (cols, 513)
    w = ref.flat(want)
    exact = np.hypot(w.real.astype(np.longdouble), w.imag.astype(np.longdouble))
    err = np.abs(prov.download(mag).astype(np.longdouble) - exact)
    assert np.all(err <= BINARY_LIBM_ULP * EPS * exact)
    for h in (hx, z, shifted, half, t, mag):
        prov.free(h)


# ---- a precision-32 provider: the same bits ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, "F32")
    yield p
    p.close()


def test_precision_32_moves_the_same_bits(prov32, prov):
    z = data((65, 63), seed=50, f32=True)  # f32-representable parts: both providers hold the same values
    idx = np.random.default_rng(51).integers(0, z.size, 4097).astype(np.uint32)
    for n in (4097, 100):
        got = {}
        for p in (prov, prov32):
            h = up_c(p, z)
            t, g = p.complex_transpose(h), p.complex_gather_linear(h, idx[:n], (n, 1))
            assert p.is_complex(t) and p.is_complex(g)
            got[p] = (p.download(t).view(np.uint64), p.download(g).view(np.uint64))
            for x in (h, t, g):
                p.free(x)
        assert np.array_equal(got[prov][0], ref.bits(ref.transpose(z))) and np.array_equal(got[prov][1], ref.bits(ref.gather(z, idx[:n], (n, 1))))
        assert np.array_equal(got[prov32][0], got[prov][0]) and np.array_equal(got[prov32][1], got[prov][1])
