"""A closed-form reference for the transforms of fft.hip: lines made of a handful of impulses, whose transform is a short sum.

A line holds amplitudes a_j at positions p_j and zeros elsewhere.  Bin f of its length-n transform is

    X[f] = sum_j a_j * exp(-/+ 2 pi i * ((p_j * f) mod n) / n)          (times 1 / n for the inverse)

with (p_j * f) mod n taken in int64 (p * f < 2^54 for every length the kernels accept) and the phase in long double - 80-bit on
x86, asserted below -, so every term is exact to ~1e-19 |a_j| and a bin costs O(terms): no FFT library and no O(n^2) sum stands
between the kernel and the definition.  Per bin the kernels' tolerance (`bound`, shared with test_gpu_fft.py) is then a bound
RELATIVE to |a|: a wrong twiddle, a misplaced line or a point read from past the input shows in full.

  impulse_case(shape, dim, length, seed, real)   the lines of one case (an ImpulseCase): positions, amplitudes, markers
  sparse_dft(case, lines, bins, inverse)         the exact transform of some lines at some bins, rounded to complex128
  bins_to_check(n, boundaries, seed)             every bin up to 2^18 points, a structured sample of at most 2^18 above
  bound / line_bound                             the project's tolerance, from a dense array or from the lines' norms
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble
# the phase is computed in extended precision; without an 80-bit long double this module would have to reduce the phase to an octant
# in integers and add 2 eps sum|a_j| to every bound - no such platform runs this suite, so it is refused instead
assert np.finfo(LD).eps < 1e-18, "fft_ref needs an extended-precision long double"
TWO_PI = 8 * np.arctan(LD(1))
MARKER = 1e6            # planted where the transform must not look
ALL_BINS_UP_TO = 1 << 18

# five terms per line; unequal real and imaginary parts, so a dropped conjugation or swapped components shows
BASE = np.array([1.0 + 0.5j, -0.75 + 1.25j, 0.625 - 1.5j, 1.375 + 0.25j, -0.5 - 0.875j])


def line_bound(norm, n, inverse):
    """C * eps * log2(work length) * ||line||_2 (+ 1e-300): C = 4 for power-of-two lengths, 8 for the chirp path, / n for the inverse."""
    pow2 = n & (n - 1) == 0
    work = n if pow2 else 1 << math.ceil(math.log2(2 * n - 1))
    c = 4.0 if pow2 else 8.0
    return c * EPS * max(1.0, math.log2(work)) * norm / (n if inverse else 1) + 1e-300


def bound(x, n, dim, inverse):
    """Per-line error bound, broadcastable against the result."""
    xs = x.reshape(x.shape + (1,) * max(0, dim + 1 - x.ndim))
    norm = np.sqrt(np.sum(np.abs(np.take(xs, range(min(n, xs.shape[dim])), axis=dim)) ** 2, axis=dim, keepdims=True))
    return line_bound(norm, n, inverse)


class ImpulseCase:
    """The lines of one case.  Line l = i + inner * o (i over the dimensions before `dim`, o over those after it) holds amplitude
    amps(l)[t] at position pos[t] < min(cur, n), and - in a truncated case - MARKER at the positions `markers` >= n."""

    def __init__(self, shape, dim, length, seed, real):
        shape = list(shape)
        while len(shape) <= dim:
            shape.append(1)
        self.shape, self.dim, self.real, self.length = tuple(shape), dim, bool(real), length
        self.cur = shape[dim]
        self.n = self.cur if length is None else int(length)
        self.inner = int(np.prod(shape[:dim], dtype=np.int64))
        self.outer = int(np.prod(shape[dim + 1:], dtype=np.int64))
        self.lines = self.inner * self.outer
        self.oshape = tuple(shape[:dim] + [self.n] + shape[dim + 1:])
        rng = np.random.default_rng(seed)
        last = min(self.cur, self.n) - 1
        odd = min(last, 2 * int(rng.integers(0, max(1, (last + 1) // 2))) + 1)
        want = [0, 1, last, self.n // 2 + 1, odd]
        pos = []
        for p in want:
            p = min(max(p, 0), last)
            if p not in pos:        # positions that clip onto each other keep the first term only
                pos.append(p)
        self.pos = np.array(pos, dtype=np.int64)
        base = BASE[:len(pos)] * (1.0 + 0.25 * rng.random(len(pos)))
        self.base = base.real + 0j if real else base
        self.markers = np.array(sorted({self.n, self.cur - 1}) if self.n < self.cur else [], dtype=np.int64)
        self.marker_value = MARKER + 0j if real else MARKER * (1 + 1j)

    def amps(self, lines):
        """[len(lines), terms] complex128: the amplitudes as stored - every line scaled by 1 + l / 64, so no two lines agree."""
        l = np.asarray(lines, dtype=np.int64)
        return self.base[None, :] * (1.0 + l[:, None] / 64.0)

    def norms(self, lines):
        """||line||_2 over the points the transform reads (the markers lie outside them)."""
        return np.sqrt(np.sum(np.abs(self.amps(lines)) ** 2, axis=1))

    def entries(self):
        """(zero-based column-major linear indices, complex values) of every nonzero input element."""
        l = np.arange(self.lines, dtype=np.int64)
        i, o = l % self.inner, l // self.inner
        p = np.concatenate([self.pos, self.markers])
        v = np.concatenate([self.amps(l), np.full((self.lines, len(self.markers)), self.marker_value)], axis=1)
        idx = i[:, None] + self.inner * (p[None, :] + self.cur * o[:, None])
        return idx.ravel(), v.ravel()

    def dense(self):
        """The input tensor (float64 for a real case)."""
        idx, v = self.entries()
        flat = np.zeros(int(np.prod(self.shape, dtype=np.int64)), dtype=np.complex128)
        flat[idx] = v
        x = flat.reshape(self.shape, order="F")
        return np.ascontiguousarray(x.real) if self.real else x

    def terms(self, line):
        """[(position, amplitude)] of one line."""
        a = self.amps([line])[0]
        return [(int(p), complex(v)) for p, v in zip(self.pos, a)]

    def out_index(self, lines, bins):
        """[len(lines), len(bins)] linear indices of those bins in the column-major result."""
        l = np.asarray(lines, dtype=np.int64)
        return (l % self.inner)[:, None] + self.inner * (np.asarray(bins, dtype=np.int64)[None, :] + self.n * (l // self.inner)[:, None])


def impulse_case(shape, dim=0, length=None, seed=0, real=False):
    return ImpulseCase(shape, dim, length, seed, real)


def phase_table(pos, n, bins):
    """(cos, sin) of 2 pi ((p f) mod n) / n in long double, [terms, len(bins)]."""
    f = np.asarray(bins, dtype=np.int64)
    assert n < 1 << 27 and (f.size == 0 or (0 <= f.min() and f.max() < n))
    k = (np.asarray(pos, dtype=np.int64)[:, None] * f[None, :]) % n
    ph = TWO_PI * k.astype(LD) / LD(n)
    return np.cos(ph), np.sin(ph)


def sparse_dft(case, lines, bins, inverse, table=None):
    """[len(lines), len(bins)] complex128: the exact transform, rounded once.  `table` = phase_table(case.pos, case.n, bins), to share
    it between the forward and the inverse transform of the same lines."""
    co, si = table if table is not None else phase_table(case.pos, case.n, bins)
    if inverse:
        si = -si
    a = case.amps(lines)
    ar, ai = a.real.astype(LD), a.imag.astype(LD)
    re = ar @ co + ai @ si          # a (cos - i sin) forward, a (cos + i sin) inverse
    im = ai @ co - ar @ si
    if inverse:
        re, im = re / LD(case.n), im / LD(case.n)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def bins_to_check(n, boundaries=(), seed=0):
    """Sorted bins: all of them up to 2^18 points; above, the first and last 4096, 4096 around n / 2 and around every pass boundary
    (the multiples m1, m1 m2 at which the output index crosses from one pass's digit to the next) and 2^16 seeded ones."""
    if n <= ALL_BINS_UP_TO:
        return np.arange(n, dtype=np.int64)
    parts = [np.arange(4096), np.arange(n - 4096, n), np.arange(n // 2 - 2048, n // 2 + 2048)]
    for b in boundaries:
        parts.append(np.arange(max(0, b - 2048), min(n, b + 2048)))
    parts.append(np.random.default_rng(seed).integers(0, n, 1 << 16))
    out = np.unique(np.concatenate(parts).astype(np.int64))
    assert out.size <= ALL_BINS_UP_TO
    return out
