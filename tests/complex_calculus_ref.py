"""Reference for the calculus and filter hooks on complex-interleaved tensors (rmhip_complex_gradient_dim / _trapz_dim / _polyint /
_iir_filter / _iir_filter_long): numpy on complex128 arrays of the LOGICAL shape, column-major.

The two parts of an element are independent lanes in every one of these hooks, so the model never multiplies or divides a complex array
by anything (numpy would widen a real factor to s + 0i and let an Inf in one part turn the other into NaN): it takes the parts out, works
on two float64 arrays with the operations in the order the header states, and puts them together again.

  gradient   (x[k+1] - x[k-1]) * (1.0 / den): the reciprocal rounded once, then multiplied into both parts;
  trapezoid  t = (0.5 * w) * (x[k] + x[k+1]), summed strictly in sequence per lane (the total, or every prefix);
  polyint    both parts of coefficient idx over logical_len - idx, (constant, +0) appended;
  filter     tests/iir_long_ref.py's sequential recurrence on the real parts and on the imaginary parts."""
import numpy as np

from iir_long_ref import df2t, normalise

EPS = 2.0 ** -52


def flat(z):
    """Column-major flat complex128 copy."""
    return np.ascontiguousarray(np.asarray(z, dtype=np.complex128).ravel(order="F"))


def interleaved(z):
    return flat(z).view(np.float64)


def from_interleaved(data, shape):
    """Interleaved doubles (re, im, ...) in column-major order -> complex128 array of `shape`."""
    return np.asarray(data, dtype=np.float64).view(np.complex128).reshape(tuple(shape), order="F")


def join(re, im):
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def same_bits(a, b) -> bool:
    """Equal shapes and, per part, equal bits - signs of zero included; a NaN matches a NaN whatever its payload (a computed NaN's sign
    and payload are the processor's choice)."""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    if a.shape != b.shape:
        return False
    x, y = interleaved(a), interleaved(b)
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))


def matrix_shape(shape):
    shape = tuple(int(s) for s in shape)
    return (1, 1) if len(shape) == 0 else (shape[0], 1) if len(shape) == 1 else shape


def _time_major(z, dim):
    """(the array with `dim` first, the padded shape): shapes are padded with 1s up to `dim`."""
    shape = tuple(z.shape) + (1,) * max(0, dim + 1 - z.ndim)
    return np.moveaxis(z.reshape(shape, order="F"), dim, 0), shape


# ---- gradient -------------------------------------------------------------------------------------------------------------------------------

def _denominators(n, spacing, coordinates):
    k = np.arange(n)
    if coordinates is None:
        den = np.full(n, 2.0 * spacing)
        den[0] = den[-1] = spacing
        return den
    c = np.asarray(coordinates, dtype=np.float64).ravel()
    assert c.size == n
    den = np.empty(n)
    den[0], den[-1] = c[1] - c[0], c[n - 1] - c[n - 2]
    den[1:-1] = c[k[1:-1] + 1] - c[k[1:-1] - 1]
    return den


def _gradient(z, dim, spacing, coordinates, quotient):
    z = np.asarray(z, dtype=np.complex128)
    z = z.reshape(matrix_shape(z.shape), order="F")
    out = np.zeros(z.shape, dtype=np.complex128)
    if z.size == 0 or dim >= z.ndim or z.shape[dim] <= 1:
        return out
    x = np.moveaxis(z, dim, 0)
    n = x.shape[0]
    den = _denominators(n, float(spacing), coordinates).reshape((n,) + (1,) * (x.ndim - 1))
    parts = []
    with np.errstate(all="ignore"):
        for lane in (x.real, x.imag):
            num = np.empty_like(lane)
            num[0], num[-1] = lane[1] - lane[0], lane[-1] - lane[-2]
            num[1:-1] = lane[2:] - lane[:-2]
            parts.append(num / den if quotient else num * (1.0 / den))
    np.moveaxis(out, dim, 0)[...] = join(*parts)
    return out


def gradient(z, dim, spacing=1.0, coordinates=None):
    """The complex rule: difference * (1.0 / den) per part.  The result has the matrix shape of `z` (a vector [n] is [n, 1])."""
    return _gradient(z, dim, spacing, coordinates, False)


def gradient_quotient(z, dim, spacing=1.0, coordinates=None):
    """The REAL kernel's rule, difference / den, applied to both parts: what the complex hook must NOT compute."""
    return _gradient(z, dim, spacing, coordinates, True)


# ---- trapezoid ------------------------------------------------------------------------------------------------------------------------------

def trapz_terms(z, dim, kind=0, spacing=None):
    """-> (terms, shape): terms[k] = (0.5 * w_k) * (x[k] + x[k+1]) for the n - 1 intervals along `dim`, time-major, per part; `shape` is
    the operand's matrix shape padded up to `dim`.  kind 0 Unit, 1 Scalar, 2 ScalarHandle (first element of `spacing`), 3 Vector
    (coordinates of the dimension), 4 Tensor (coordinates in the operand's layout)."""
    z = np.asarray(z, dtype=np.complex128)
    z = z.reshape(matrix_shape(z.shape), order="F")
    x, shape = _time_major(z, dim)
    n = x.shape[0]
    if z.size == 0 or n <= 1:
        return np.zeros((0,) + x.shape[1:], dtype=np.complex128), shape
    tail = (1,) * (x.ndim - 1)
    if kind == 0:
        w = np.ones((n - 1,) + tail)
    elif kind == 1:
        w = np.full((n - 1,) + tail, float(spacing))
    elif kind == 2:
        w = np.full((n - 1,) + tail, float(np.asarray(spacing, dtype=np.float64).ravel(order="F")[0]))
    elif kind == 3:
        sp = np.asarray(spacing, dtype=np.float64).ravel(order="F")
        w = (sp[1:n] - sp[:n - 1]).reshape((n - 1,) + tail)
    else:
        sp = np.asarray(spacing, dtype=np.float64).ravel(order="F")[:z.size].reshape(shape, order="F")
        sp = np.moveaxis(sp, dim, 0)
        w = sp[1:] - sp[:-1]
    with np.errstate(all="ignore"):
        hw = 0.5 * w
        return join(hw * (x.real[:-1] + x.real[1:]), hw * (x.imag[:-1] + x.imag[1:])), shape


def trapz(z, dim, kind=0, spacing=None, cumulative=False):
    """-> (result, magnitude): the strictly sequential per-lane sum of the terms (cumulative: every prefix, 0 at k = 0) and, in the same
    layout, the sum of |t| it ran over - n * EPS * magnitude is the accuracy bound per part, n the extent along `dim`."""
    terms, shape = trapz_terms(z, dim, kind, spacing)
    n = shape[dim]
    rest = terms.shape[1:]
    acc_r, acc_i, mag_r, mag_i = (np.zeros(rest) for _ in range(4))
    steps = n if cumulative else 1
    res = np.zeros((steps,) + rest, dtype=np.complex128)
    mag = np.zeros((steps,) + rest, dtype=np.complex128)
    with np.errstate(all="ignore"):
        for k in range(terms.shape[0]):
            acc_r, acc_i = acc_r + terms[k].real, acc_i + terms[k].imag
            mag_r, mag_i = mag_r + np.abs(terms[k].real), mag_i + np.abs(terms[k].imag)
            if cumulative:
                res[k + 1], mag[k + 1] = join(acc_r, acc_i), join(mag_r, mag_i)
        if not cumulative and int(np.prod(rest, dtype=np.int64)):
            res[0], mag[0] = join(acc_r, acc_i), join(mag_r, mag_i)
    oshape = tuple(shape) if cumulative else tuple(1 if d == dim else s for d, s in enumerate(shape))
    if int(np.prod(shape, dtype=np.int64)) == 0 and cumulative:
        return np.zeros(oshape, dtype=np.complex128), np.zeros(oshape, dtype=np.complex128)
    to_shape = lambda v: np.ascontiguousarray(np.moveaxis(v, 0, dim)).reshape(oshape)
    return to_shape(res), to_shape(mag)


# ---- polyint --------------------------------------------------------------------------------------------------------------------------------

def polyint(p, constant=0.0):
    """Row -> [1, n + 1], column -> [n + 1, 1], scalar -> [1, 2], no elements -> [1, 1]."""
    p = np.asarray(p, dtype=np.complex128)
    big = [d for d, s in enumerate(p.shape) if s > 1]
    assert len(big) <= 1, "polynomial coefficients must form a vector"
    c = flat(p)
    n = c.size
    power = (n - np.arange(n)).astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.concatenate([join(c.real / power, c.imag / power), join(np.array([float(constant)]), np.array([0.0]))])
    column = bool(big) and big[0] == 0
    return out.reshape((n + 1, 1) if column and n + 1 > 1 else (1, n + 1))


# ---- filter ---------------------------------------------------------------------------------------------------------------------------------

def iir_filter(b, a, z, dim, zi=None):
    """-> (y, zf): the sequential recurrence per lane along `dim`; y has z's shape, zf the state shape (extent order - 1 at `dim`)."""
    bn, an = normalise(b, a)
    S = bn.size - 1
    z = np.asarray(z, dtype=np.complex128)
    x, shape = _time_major(z, dim)
    zshape = tuple(S if d == dim else s for d, s in enumerate(shape))
    st = np.zeros((S,) + x.shape[1:], dtype=np.complex128)
    if zi is not None:
        st = np.moveaxis(np.asarray(zi, dtype=np.complex128).reshape(zshape, order="F"), dim, 0)
    ys, zs = [], []
    with np.errstate(all="ignore"):
        for lane, s0 in ((x.real, st.real), (x.imag, st.imag)):
            if S == 0:  # a gain: no state is added, the sign of a zero survives
                ys.append(bn[0] * lane)
                zs.append(np.zeros((0,) + lane.shape[1:]))
            else:
                y, zf = df2t(bn, an, np.ascontiguousarray(lane), np.ascontiguousarray(s0))
                ys.append(y)
                zs.append(zf)
    y = np.ascontiguousarray(np.moveaxis(join(*ys), 0, dim)).reshape(z.shape)
    zf = np.ascontiguousarray(np.moveaxis(join(*zs), 0, dim))
    return y, zf


# The long form's recursive cases: two stable filters of tests/iir_long_ref.py's FILTERS on 5000 logical samples x 2 logical channels
# (a tail that is no multiple of any chunk length), with initial states.  Shared by the GPU test and by the host check that the numpy model
# of the chunked scan stays inside the accuracy contract on exactly these inputs.
LONG_FILTERS = ("double_pole_0.9", "order4_conj_0.9")
LONG_LEN, LONG_CHANNELS = 5000, 2
_LONG = {}


def long_signal(name):
    """-> (z, zi): time-major complex arrays (LONG_LEN x LONG_CHANNELS, states x LONG_CHANNELS); never modified."""
    if name not in _LONG:
        from iir_long_ref import FILTERS

        b, a = FILTERS[name]
        S = max(len(b), len(a)) - 1
        rng = np.random.default_rng(7000 + LONG_FILTERS.index(name))
        z = join(rng.standard_normal((LONG_LEN, LONG_CHANNELS)), rng.standard_normal((LONG_LEN, LONG_CHANNELS)))
        zi = join(rng.standard_normal((S, LONG_CHANNELS)), rng.standard_normal((S, LONG_CHANNELS)))
        z.setflags(write=False)
        zi.setflags(write=False)
        _LONG[name] = (z, zi)
    return _LONG[name]


def round_f32(z):
    """Each part rounded through f32: what a precision-32 context stores for a complex result."""
    z = np.asarray(z, dtype=np.complex128)
    with np.errstate(all="ignore"):
        return join(z.real.astype(np.float32).astype(np.float64), z.imag.astype(np.float32).astype(np.float64))
