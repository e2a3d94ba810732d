"""Every path of fft_pow2 / fft_bluestein (fft.hip) against the closed-form transform of impulse lines (fft_ref.py).

One case table, CASES, names every path the launchers can take; each case states the number of kernel launches its path makes
and the test asserts it from the telemetry, so a case that stops exercising its path (a moved threshold, say) fails.  With
lg = log2(n), `inner` = the product of the dimensions before the transformed one, M = the chirp convolution's length:

  path     selected by (fft_plan.h)                                launches   what runs
  tile0    pow2_passes = 1 -> one_pass: inner == 1, lg <= 13       1          one tile, points contiguous (mode 0); plan_tile: 256 / 512 / 1024 threads
  tile1    pow2_passes = 1 -> one_pass: inner > 1, lg <= 8         1          one tile, lines contiguous (mode 1)
  two0     pow2_passes = 2 -> two_pass: inner == 1, lg 14..22      2          m1 = 2^(lg // 2) strided, step twiddle, then mode 2
  two1     pow2_passes = 2 -> two_pass: inner > 1, lg 9..24        2          both passes mode 1
  three    pow2_passes = 3 -> three_pass: inner == 1, lg 23..27    3          splits lg 23: 7, 8, 8; 24: 8, 8, 8; 26: 8, 9, 9
  chirp    plan_entry: n not a power of two -> plan_chirp          2 p + 2    p = pow2_passes of the length-M transform at that inner
  chirp3   plan_chirp with M = 2^24 (n > 2^22)                     8          M = 2^24 in three passes: mul_in and valid through pass A
  slabs    plan_chirp: nslabs > 1 (inner M outer > 2^26)           per slab   the outer dimension in pieces (chirp_slab: o0 > 0 offsets)
and test_table_cache_eviction re-checks results after fft_tables has been cleared (more than 64 entries).  These are the counts the
drivers make when they walk the plan; tests/test_fft_paths_host.py asserts every case's family and count against fft_plan.h on the
CPU, and none differed.

Tolerance: the project's own (fft_ref.bound, shared with test_gpu_fft.py): per bin C eps log2(work length) ||line||_2, C = 4 for
powers of two and 8 for the chirp path, / n for the inverse.  On an impulse line that is a bound relative to |a|.  Every line of
every case is checked; lines of more than 2^18 points at a structured sample of at most 2^18 bins (fft_ref.bins_to_check) - only
the slabs case samples lines (every line of the outer indices around the slab boundary, every 97th elsewhere: ~170 000 lines).

Input is built on the device (zeros, scatter_linear), results of more than 2^22 points are read through complex_unary('real' /
'imag') and gather_linear, so nothing large crosses the bus.

Padding: a transform longer than its input must read zeros past the input's end.  What the ABI lets a test plant there is the next
line - in a padded case of several lines the first point past line l is line l + 1's position-0 impulse - and that is checked by
the two-line padded cases.  Past the LAST line lies memory the ABI gives no handle on; `poison` first fills and frees a block of the
size of the result with 1e6, which the pool may or may not hand back as the input's neighbourhood: best effort, not a guarantee.

Measured on an MI355X, max err / lim per family over all its cases (forward and inverse, real and complex; every case prints its
own figure, `pytest -rP`):
  tile0 0.21 (lg 2; 0.06-0.09 from lg 7 on)   tile1 0.21   two0 0.075   two1 0.084   three 0.051
  chirp 0.14 (n = 3 x 3 lines; 0.05-0.11 elsewhere)   chirp3 (n = 5 000 000) 0.049   slabs 0.11   dense lines 0.035-0.12
The error falls relative to the bound as passes are added (the bound grows with log2 n, the impulse's error with the passes it
crosses): no family is near 1, and no bin stands out.
"""
import numpy as np
import pytest

import fft_ref as R

pytestmark = pytest.mark.gpu

DOWNLOAD_UP_TO = 1 << 22
VARIANTS_ALL = (("real", False), ("real", True), ("complex", False), ("complex", True))
VARIANTS_REAL = (("real", False), ("real", True))


def case(cid, path, launches, shape, dim=0, length=None, variants=VARIANTS_ALL, boundaries=()):
    return pytest.param(dict(path=path, launches=launches, shape=shape, dim=dim, length=length, variants=variants, boundaries=boundaries), id=f"{path}-{cid}")


def tile0_lines(lg):
    """B + 1, B = the lines per tile plan_tile (fft_plan.h) gives a mode-0 tile of 2^lg points: one full tile and a tile of one line."""
    m = 1 << lg
    cap = 2048 if m <= 2048 else 4096
    return max(1, min(256, cap // m)) + 1


CASES = []
# one tile, points contiguous: every lg with 1 line and with B + 1 lines; the three thread counts (m <= 2048, 4096, 8192) with 3 lines
for lg in range(1, 14):
    CASES.append(case(f"lg{lg}", "tile0", 1, (1 << lg,)))
    CASES.append(case(f"lg{lg}x{tile0_lines(lg)}", "tile0", 1, (1 << lg, tile0_lines(lg))))
for lg in (11, 12, 13):
    CASES.append(case(f"lg{lg}x3", "tile0", 1, (1 << lg, 3)))
# one tile, lines contiguous: inner = 257 is full tiles of MAXB (or fewer) lines and a partial one
for lg in (1, 2, 3, 5, 7, 8):
    for inner in (2, 5, 257):
        CASES.append(case(f"{inner}xlg{lg}", "tile1", 1, (inner, 1 << lg), 1))
CASES.append(case("5xlg5x3", "tile1", 1, (5, 1 << 5, 3), 1))
CASES.append(case("5xlg8x3", "tile1", 1, (5, 1 << 8, 3), 1))
# two passes, inner == 1: the output index is j1 + m1 j2, m1 = 2^(lg // 2)
for lg in (14, 15, 16, 17, 18, 21, 22):
    CASES.append(case(f"lg{lg}", "two0", 2, (1 << lg,), boundaries=(1 << (lg // 2),)))
CASES.append(case("lg14x3", "two0", 2, (1 << 14, 3)))
CASES.append(case("lg15x3", "two0", 2, (1 << 15, 3)))
CASES.append(case("padded", "two0", 2, ((1 << 14) + 5,), 0, 1 << 15))
CASES.append(case("paddedx2", "two0", 2, ((1 << 14) + 5, 2), 0, 1 << 15))      # line 0's first absent point is line 1's impulse
CASES.append(case("truncated", "two0", 2, ((1 << 15) + 7,), 0, 1 << 14))
# two passes, inner > 1
CASES.append(case("3xlg9", "two1", 2, (3, 1 << 9), 1))
CASES.append(case("2xlg12x2", "two1", 2, (2, 1 << 12, 2), 1))
CASES.append(case("3xlg15", "two1", 2, (3, 1 << 15), 1))
CASES.append(case("2xlg20", "two1", 2, (2, 1 << 20), 1, boundaries=(1 << 10,)))
CASES.append(case("5x1000to1024", "two1", 2, (5, 1000), 1, 1024))              # padding across the pass boundary (m2 = 32)
CASES.append(case("5x1100to1024", "two1", 2, (5, 1100), 1, 1024))
# three passes: j = j1 + m1 j2 + m1 m2 j3
CASES.append(case("lg23", "three", 3, (1 << 23,), variants=VARIANTS_REAL, boundaries=(1 << 7, 1 << 15)))
CASES.append(case("lg24", "three", 3, (1 << 24,), variants=VARIANTS_REAL, boundaries=(1 << 8, 1 << 16)))
CASES.append(case("lg26", "three", 3, (1 << 26,), variants=VARIANTS_REAL, boundaries=(1 << 8, 1 << 17)))
CASES.append(case("lg23x2", "three", 3, (1 << 23, 2), variants=VARIANTS_REAL, boundaries=(1 << 7, 1 << 15)))
# chirp convolution: launches = 2 p + 2; M = 2^13 is the longest single tile at inner == 1, M = 2^8 at inner > 1
for n in (3, 5, 6, 7, 9, 15, 17, 31, 33, 127, 129, 257, 1000, 4095, 4097, 65537):
    p = 1 if 2 * n - 1 <= 1 << 13 else 2
    CASES.append(case(f"n{n}", "chirp", 2 * p + 2, (n,)))
    CASES.append(case(f"n{n}x3", "chirp", 2 * p + 2, (n, 3)))
CASES.append(case("6xn100", "chirp", 4, (6, 100), 1))                           # M = 2^8, one tile
CASES.append(case("3xn4097", "chirp", 6, (3, 4097), 1))                         # M = 2^14, two passes
CASES.append(case("257xn7", "chirp", 4, (257, 7), 1))
CASES.append(case("n5000000", "chirp3", 8, (5_000_000,), boundaries=(1 << 8, 1 << 16)))   # M = 2^24: mul_in and valid through pass A
CASES.append(case("1000to1500", "chirp", 4, (1000,), 0, 1500))
CASES.append(case("1000to1500x2", "chirp", 4, (1000, 2), 0, 1500))
CASES.append(case("1000to999", "chirp", 4, (1000,), 0, 999))


def launches_of(prov):
    return prov.telemetry_snapshot()["kernel_launches"]


def to_device(prov, c):
    idx, v = c.entries()

    def plane(vals):
        h = prov.zeros(c.shape)
        hv = prov.upload(np.ascontiguousarray(vals), (vals.size, 1))
        prov.scatter_linear(h, idx, hv)
        prov.free(hv)
        return h

    re = plane(v.real)
    if c.real:
        return re
    im = plane(v.imag)
    z = prov.complex_from_real_imag(re, im)
    prov.free(re)
    prov.free(im)
    return z


def poison(prov, c):
    h = prov.fill((2 * int(np.prod(c.oshape)), 1), R.MARKER)
    prov.free(h)


def fetch(prov, out, idx):
    """The complex result's elements at the linear indices `idx` (any shape)."""
    total = int(np.prod(out.shape, dtype=np.int64))
    if total <= DOWNLOAD_UP_TO:
        return prov.download(out)[idx]
    parts = []
    for op in ("real", "imag"):
        plane = prov.complex_unary(op, out)
        g = prov.gather_linear(plane, idx.ravel(), (idx.size, 1))
        parts.append(prov.download(g).reshape(idx.shape))
        prov.free(g)
        prov.free(plane)
    return parts[0] + 1j * parts[1]


def transform(prov, h, c, inverse, launches):
    """The transform, run twice; the smaller launch count of the two is the path's (the first call may build tables, and a table
    cache eviction can cost one rebuild).  Returns the second result."""
    f = prov.ifft_dim if inverse else prov.fft_dim
    t0 = launches_of(prov)
    first = f(h, c.length, c.dim)
    t1 = launches_of(prov)
    out = f(h, c.length, c.dim)
    t2 = launches_of(prov)
    prov.free(first)
    assert prov.is_complex(out) and tuple(out.shape) == c.oshape
    assert min(t1 - t0, t2 - t1) == launches, (t1 - t0, t2 - t1, launches)
    return out


def note(path, ratio):
    print(f"RATIO {path} {ratio:.4f}")


def c_seed(spec):
    return int(np.prod(spec["shape"])) % 9973 + (spec["length"] or 0)


@pytest.mark.parametrize("spec", CASES)
def test_path(prov, spec):
    worst = 0.0
    tables = {}
    for kind, inverse in spec["variants"]:
        c = R.impulse_case(spec["shape"], spec["dim"], spec["length"], seed=c_seed(spec), real=kind == "real")
        lines = np.arange(c.lines)
        bins = R.bins_to_check(c.n, spec["boundaries"], seed=11)
        key = tuple(c.pos)
        if key not in tables:
            tables[key] = R.phase_table(c.pos, c.n, bins)
        want = R.sparse_dft(c, lines, bins, inverse, tables[key])
        lim = R.line_bound(c.norms(lines), c.n, inverse)[:, None]
        if c.n > c.cur:
            poison(prov, c)
        h = to_device(prov, c)
        out = transform(prov, h, c, inverse, spec["launches"])
        got = fetch(prov, out, c.out_index(lines, bins))
        prov.free(out)
        prov.free(h)
        ratio = np.abs(got - want) / lim
        worst = max(worst, float(np.max(ratio)))
        assert np.all(ratio <= 1.0), (kind, inverse, float(np.max(ratio)), np.argwhere(ratio > 1.0)[:8].tolist())
    note(spec["path"], worst)


def test_chirp_in_outer_slabs(prov):
    """inner M outer > 2^26: M = 8, slab = inner M = 2^16, 1024 outer indices per piece, so the last 6 of 1030 run in a second piece
    with o0 = 1024 offsets on the input and the result.  Forward, real input; every line of outer indices 1020..1029 and every
    97th line elsewhere, all three bins of each."""
    c = R.impulse_case((8192, 2, 1030), 1, 3, seed=4, real=True)
    assert c.inner * 8 * c.outer > 1 << 26 and list(c.pos) == [0, 1]
    lines = np.unique(np.concatenate([np.arange(0, 1020 * 8192, 97), np.arange(1020 * 8192, 1030 * 8192)]))
    assert lines.size >= 10000
    bins = R.bins_to_check(3)
    want = R.sparse_dft(c, lines, bins, False)
    lim = R.line_bound(c.norms(lines), 3, False)[:, None]
    poison(prov, c)
    h = to_device(prov, c)
    out = transform(prov, h, c, False, 2 * (2 * 1 + 2))
    got = fetch(prov, out, c.out_index(lines, bins))
    prov.free(out)
    prov.free(h)
    ratio = np.abs(got - want) / lim
    note("slabs", float(np.max(ratio)))
    assert np.all(ratio <= 1.0), (float(np.max(ratio)), lines[np.argwhere(ratio > 1.0)[:8, 0]].tolist())


HERMITIAN = [p for p in CASES if (p.values[0]["length"] or p.values[0]["shape"][p.values[0]["dim"]]) <= 1 << 18]


@pytest.mark.parametrize("spec", HERMITIAN)
def test_real_input_is_hermitian(prov, spec):
    """X[(n - f) mod n] = conj(X[f]) for a real line, forward and inverse, within 2 lim: what a packed real-input kernel breaks first."""
    c = R.impulse_case(spec["shape"], spec["dim"], spec["length"], seed=c_seed(spec), real=True)
    lines = np.arange(c.lines)
    f = np.arange(c.n)
    h = to_device(prov, c)
    for inverse in (False, True):
        out = (prov.ifft_dim if inverse else prov.fft_dim)(h, c.length, c.dim)
        got = prov.download(out)
        prov.free(out)
        a, b = got[c.out_index(lines, f)], got[c.out_index(lines, (c.n - f) % c.n)]
        lim = R.line_bound(c.norms(lines), c.n, inverse)[:, None]
        assert np.all(np.abs(b - np.conj(a)) <= 2 * lim), (inverse, float(np.max(np.abs(b - np.conj(a)) / lim)))
    prov.free(h)


@pytest.mark.parametrize("inverse", [False, True], ids=["fft", "ifft"])
@pytest.mark.parametrize("shape,dim,own_error", [((1 << 15,), 0, 1), ((1 << 17,), 0, 1), ((3, 1 << 15), 1, 1), ((1 << 23,), 0, 2), ((1 << 24,), 0, 2),
                                                 ((5_000_000,), 0, 2)], ids=str)
def test_dense_lines_on_the_new_paths(prov, shape, dim, own_error, inverse):
    """Random normal lines against pocketfft on the paths no dense test ran: the forward transform of real lines, the inverse of
    complex ones.  Long lines carry test_gpu_fft.py's factor 2 for pocketfft's own error."""
    rng = np.random.default_rng(shape[dim] + dim)
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if inverse else rng.standard_normal(shape)
    up = lambda v: prov.upload(np.ascontiguousarray(v).ravel(order="F"), shape)
    if inverse:
        re, im = up(x.real), up(x.imag)
        h = prov.complex_from_real_imag(re, im)
        prov.free(re)
        prov.free(im)
    else:
        h = up(x)
    out = (prov.ifft_dim if inverse else prov.fft_dim)(h, None, dim)
    got = prov.download(out).reshape(shape, order="F")
    prov.free(out)
    prov.free(h)
    want = (np.fft.ifft if inverse else np.fft.fft)(x, axis=dim)
    lim = own_error * R.bound(x, shape[dim], dim, inverse)
    ratio = float(np.max(np.abs(got - want) / lim))
    print(f"RATIO dense-{shape} {ratio:.4f}")
    assert ratio <= 1.0, ratio


def test_table_cache_eviction(prov):
    """fft_tables is cleared when it passes 64 entries.  A length-1000 transform, then 70 other lengths (more than 64 new tables),
    then length 1000 again: the same bits; and a 2^14 line still meets its bound."""
    def run(n, seed):
        c = R.impulse_case((n,), 0, None, seed=seed, real=False)
        h = to_device(prov, c)
        out = prov.fft_dim(h, None, 0)
        got = prov.download(out)
        prov.free(out)
        prov.free(h)
        return c, got

    c1000, first = run(1000, 1)
    others = [1 << lg for lg in range(14, 23)] + [1001 + 2 * k for k in range(61)]
    assert len(set(others)) == 70 and 1000 not in others
    for n in others:
        run(n, n)
    _, again = run(1000, 1)
    assert np.array_equal(first.view(np.float64).view(np.uint64), again.view(np.float64).view(np.uint64))
    c, got = run(1 << 14, 2)
    bins = R.bins_to_check(c.n)
    err = np.abs(got - R.sparse_dft(c, [0], bins, False)[0])
    assert np.all(err <= R.line_bound(c.norms([0])[0], c.n, False))
    assert np.all(np.abs(again - R.sparse_dft(c1000, [0], R.bins_to_check(1000), False)[0]) <= R.line_bound(c1000.norms([0])[0], 1000, False))
