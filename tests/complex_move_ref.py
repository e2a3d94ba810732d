"""Reference for the shape and indexing hooks on complex-interleaved tensors (rmhip_complex_reshape / _transpose / _permute / _repmat /
_gather_linear / _scatter_linear / _circshift / _flip / _cat): numpy on complex128 arrays of the LOGICAL shape.  Memory order is
column-major, so flat views are taken with order="F"; a linear index counts logical (re, im) elements.  Everything here moves elements
and computes nothing, so results are compared on the bits of the interleaved doubles."""
import numpy as np


def flat(z):
    """Column-major flat complex128 copy."""
    return np.ascontiguousarray(np.asarray(z, dtype=np.complex128).ravel(order="F"))


def bits(z):
    return flat(z).view(np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def from_interleaved(data, shape):
    """Interleaved doubles (re, im, ...) in column-major order -> complex128 array of `shape`."""
    return np.asarray(data, dtype=np.float64).view(np.complex128).reshape(tuple(shape), order="F")


def _padded(z, rank):
    return z.reshape(tuple(z.shape) + (1,) * (rank - z.ndim), order="F")


def permute(z, order):
    """out dimension d is source dimension order[d]; the shape is padded with 1s to len(order)."""
    return np.transpose(_padded(z, len(order)), order)


def transpose(z):
    return permute(z if z.ndim >= 2 else _padded(z, 2), (1, 0))


def repmat_shape(shape, reps):
    """The provider's rank rules: one factor tiles every dimension of a shape of at least two dimensions."""
    orig = max(len(shape), 1)
    rank = max(orig, 2) if len(reps) == 1 else max(orig, len(reps))
    base = tuple(shape) + (1,) * (rank - len(shape))
    factors = (reps[0],) * rank if len(reps) == 1 else tuple(reps) + (1,) * (rank - len(reps))
    return base, factors


def repmat(z, reps):
    base, factors = repmat_shape(z.shape, reps)
    return np.tile(z.reshape(base, order="F"), factors)


def circshift(z, shifts):
    """out(c) = in((c - shift) mod extent); shifts beyond the rank meet extent-1 dimensions; the result keeps the operand's shape."""
    w = _padded(z, max(z.ndim, len(shifts)))
    for d, s in enumerate(shifts):
        n = w.shape[d]
        if n > 1:
            w = np.roll(w, int(s) % n, axis=d)
    return w.reshape(z.shape, order="F")


def flip(z, axes):
    """An axis named twice flips back; an axis beyond the rank is an extent-1 dimension."""
    w = z
    for ax in axes:
        if ax < w.ndim:
            w = np.flip(w, axis=ax)
    return w


def cat(dim_one_based, zs):
    dz = dim_one_based - 1
    rank = max([dz + 1] + [z.ndim for z in zs])
    out = np.concatenate([_padded(z, rank) for z in zs], axis=dz)
    shape = list(out.shape)  # normalize_concat_shape: trailing 1s dropped down to max(dim, 2) dimensions
    min_len = min(max(dz + 1, 2), len(shape))
    while len(shape) > min_len and shape[-1] == 1:
        shape.pop()
    if len(shape) == 1:
        shape.append(1)
    return out.reshape(tuple(shape), order="F")


def gather(z, indices, out_shape):
    return flat(z)[np.asarray(indices, dtype=np.int64)].reshape(tuple(out_shape), order="F")


def scatter(z, indices, values):
    """The sequential loop: a later duplicate overwrites an earlier one."""
    out, v = flat(z), flat(values)
    for k, i in enumerate(indices):
        out[int(i):int(i) + 1] = v[k:k + 1]  # (array to array: the bytes, NaN payloads included)
    return out.reshape(z.shape, order="F")
