"""A Python restatement of the reference's `mode` (builtins/stats/summary/mode.rs:436-576, 806-853), the yardstick of the mode_values tests.

Per slice: NaNs are skipped; values are counted under a key that is the bit pattern with both zeros on one key (`canonical_bits`,
:848-853), an entry keeping the value of its FIRST occurrence; M is the smallest value with the highest count, F that count, the tied set
every value with that count in ascending order.  A slice without a number gives NaN, 0 and an empty set.  Everything is a copy of an
input element or an integer, so results are compared by their bits.

`mode(x, axes)` takes a numpy array (any rank; a scalar is [1, 1], a vector [n, 1] - the provider's `matrix_shape`) and axes "default",
"all" or a zero-based dimension, and returns (M, F, ties): M and F as column-major arrays of the output shape, ties as a list of float64
arrays, one per output slice in column-major order.
"""
import numpy as np

NAN_BITS = 0x7FF8000000000000
CANONICAL_NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def canonical_bits(v: float) -> int:
    return 0 if v == 0.0 else int(np.float64(v).view(np.uint64))  # mode.rs:848-853


def scalar_mode(values):
    """mode.rs:806-846 -> (value, frequency, ties)"""
    counts = {}
    for v in values:
        if v != v:
            continue
        key = canonical_bits(v)
        if key in counts:
            counts[key][1] += 1
        else:
            counts[key] = [v, 1]
    if not counts:
        return CANONICAL_NAN, 0.0, np.empty(0)
    top = max(c for _, c in counts.values())
    tied = sorted((v for v, c in counts.values() if c == top))  # distinct keys: no two compare equal, the order is total
    return tied[0], float(top), np.array(tied, dtype=np.float64)


def matrix_shape(shape):
    shape = tuple(int(s) for s in shape)
    return (1, 1) if len(shape) == 0 else (shape[0], 1) if len(shape) == 1 else shape


def default_dim(shape):
    return next((k for k, e in enumerate(shape) if e != 1), 0)  # mode.rs:436-445, zero-based


def mode(x, axes="default"):
    x = np.asarray(x, dtype=np.float64)
    shape = matrix_shape(x.shape)
    flat = x.reshape(-1, order="F")
    if axes == "all":  # mode.rs:447-455
        oshape, slices = (1, 1), [flat]
    else:
        dim = default_dim(shape) if axes == "default" else int(axes)
        if dim >= len(shape):  # mode.rs:486-515: every slice one element
            oshape, slices = shape, [flat[k:k + 1] for k in range(flat.size)]
        else:  # mode.rs:517-560
            oshape = shape[:dim] + (1,) + shape[dim + 1:]
            before = int(np.prod(shape[:dim], dtype=np.int64))
            after = int(np.prod(shape[dim + 1:], dtype=np.int64))
            n = shape[dim]
            slices = [flat[b + a * before * n: b + a * before * n + n * before: before] if n else flat[:0] for a in range(after) for b in range(before)]
    res = [scalar_mode(s) for s in slices]
    M = np.array([r[0] for r in res], dtype=np.float64).reshape(oshape, order="F")
    F = np.array([r[1] for r in res], dtype=np.float64).reshape(oshape, order="F")
    return M, F, [r[2] for r in res]


def ragged(ties):
    """The trait's ragged form (`ProviderModeTiedSets`): values [total, 1], offsets, counts."""
    counts = [int(t.size) for t in ties]
    offsets = [int(o) for o in np.concatenate(([0], np.cumsum(counts)[:-1]))] if counts else []
    values = np.concatenate(ties).reshape(-1, 1) if ties else np.empty((0, 1))
    return values, offsets, counts
