"""A Python restatement of the reference's numeric 'rows' forms of unique / union / setdiff / ismember
(builtins/array/sorting_sets: unique.rs:558-662, union.rs:546-622 + 1281-1330, setdiff.rs:498-552 + 891-930, ismember.rs:440-480 + 755-765),
the yardstick of the rows-form tests.

A row's key is the tuple of its columns' `canonicalize_f64` keys (unique.rs:1347-1355: every NaN one key, both zeros one key, anything else
its bit pattern); the CPU's hash maps become dicts over those tuples, walked in the CPU's order, so an entry keeps the bits of its FIRST
occurrence.  The sorted order is `compare_numeric_rows` (:1357-1379): column 0 first, NaN after every number, the zeros equal - a stable
sort, as `sort_by` is.  Everything is a copy of an input element or an integer, so results are compared by their bits.

Inputs are numpy arrays whose `.shape` is the tensor's shape (rank matters: unique / union / setdiff want exactly 2, ismember takes
0 / 1 / 2); outputs are float64 arrays shaped as the CPU's tensors ([count, cols], [k, 1]), the mask a uint8 [rows_a, 1].  The CPU's errors
are `RowsError`s carrying its message.
"""
from functools import cmp_to_key

import numpy as np

NAN_KEY = 0x7FF8000000000000


class RowsError(ValueError):
    """an `Err(...)` of the CPU builtin"""


def canonicalize_f64(v: float) -> int:  # unique.rs:1347-1355
    if v != v:
        return NAN_KEY
    if v == 0.0:
        return 0
    return int(np.float64(v).view(np.uint64))


def compare_f64(a: float, b: float) -> int:  # unique.rs:1357-1369
    if a != a:
        return 0 if b != b else 1
    if b != b:
        return -1
    return -1 if a < b else 1 if a > b else 0


def compare_numeric_rows(a, b) -> int:  # unique.rs:1371-1379
    for lhs, rhs in zip(a, b):
        o = compare_f64(lhs, rhs)
        if o:
            return o
    return 0


def row_key(row) -> tuple:
    return tuple(canonicalize_f64(v) for v in row)


def _rows_of(x, rows, cols):
    """the rows of a column-major tensor, each as (row_data, key): row_data a float64 array (bits intact), key the tuple of the canonical
    keys - `canonicalize_f64` applied to the whole tensor at once"""
    flat = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, order="F"))
    keys = np.where(flat != flat, np.uint64(NAN_KEY), np.where(flat == 0.0, np.uint64(0), flat.view(np.uint64)))
    m, k = flat.reshape((rows, cols), order="F"), keys.reshape((rows, cols), order="F").tolist()
    return [(m[r], tuple(k[r])) for r in range(rows)]


def _tensor(data, shape, what):
    """`Tensor::new` (runmat-builtins lib.rs:626-635): the data length must match the shape"""
    expected = int(np.prod(shape, dtype=np.int64))
    if len(data) != expected:
        raise RowsError(f"{what}: Tensor data length {len(data)} doesn't match shape {list(shape)} ({expected} elements)")
    return np.array(data, dtype=np.float64).reshape(shape, order="F")


def _matrix(entries, order, cols):
    """values[row_pos + col * count] = entry.row_data[col]"""
    values = np.zeros((len(order), cols), dtype=np.float64, order="F")
    for pos, e in enumerate(order):
        values[pos, :] = entries[e][0]
    return values


def order_key(row) -> tuple:
    """a sort key under which tuples compare as `compare_numeric_rows` does: per column (is NaN, the number or 0) - Python's -0.0 == 0.0"""
    return tuple((True, 0.0) if v != v else (False, v) for v in row)


def sorted_by_compare(rows):
    """`order.sort_by(compare_numeric_rows)` as written: a stable sort of the indices under the comparison itself"""
    return sorted(range(len(rows)), key=cmp_to_key(lambda a, b: compare_numeric_rows(rows[a], rows[b])))


def _sorted(entries):
    keys = [order_key(e[0].tolist()) for e in entries]  # the same order as sorted_by_compare (tests/test_rowsets_host.py), without a call per comparison
    return sorted(range(len(entries)), key=keys.__getitem__)


def unique_rows(x, order="sorted", occurrence="first"):
    """unique.rs:558-662 -> (values [count, cols], ia [count, 1], ic [rows, 1])"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise RowsError("unique: 'rows' option requires a 2-D matrix input")
    rows, cols = x.shape
    if rows == 0 or cols == 0:
        return _tensor([], (0, cols), "unique"), _tensor([], (0, 1), "unique"), _tensor([], (rows, 1), "unique")
    entries, index, row_entry = [], {}, []  # entry: [row_data, first, last]
    for r, (row, k) in enumerate(_rows_of(x, rows, cols)):
        if k in index:
            entries[index[k]][2] = r
        else:
            index[k] = len(entries)
            entries.append([row, r, r])
        row_entry.append(index[k])
    ordr = _sorted(entries) if order == "sorted" else list(range(len(entries)))
    position = {e: pos for pos, e in enumerate(ordr)}
    ia = [float(entries[e][2 if occurrence == "last" else 1] + 1) for e in ordr]
    ic = [float(position[e] + 1) for e in row_entry]
    return _matrix(entries, ordr, cols), _tensor(ia, (len(ordr), 1), "unique"), _tensor(ic, (rows, 1), "unique")


def _two_matrices(a, b, name):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2:
        raise RowsError(f"{name}: 'rows' option requires 2-D numeric matrices")
    if a.shape[1] != b.shape[1]:
        raise RowsError(f"{name}: inputs must have the same number of columns when using 'rows'")
    return a, b


def union_rows(a, b, order="sorted"):
    """union.rs:546-622, 1281-1330 -> (values [count, cols], ia [na, 1], ib [nb, 1])"""
    a, b = _two_matrices(a, b, "union")
    cols = a.shape[1]
    entries, index = [], {}  # entry: [row_data, a_row or None, b_row or None]; the list order is `order_rank`
    for r, (row, k) in enumerate(_rows_of(a, a.shape[0], cols)):
        if k not in index:
            index[k] = len(entries)
            entries.append([row, r, None])
    for r, (row, k) in enumerate(_rows_of(b, b.shape[0], cols)):
        if k in index:
            e = entries[index[k]]
            if e[1] is None and e[2] is None:
                e[2] = r
        else:
            index[k] = len(entries)
            entries.append([row, None, r])
    ordr = _sorted(entries) if order == "sorted" else list(range(len(entries)))
    ia, ib = [], []
    for e in ordr:
        if entries[e][1] is not None:
            ia.append(float(entries[e][1] + 1))
        elif entries[e][2] is not None:
            ib.append(float(entries[e][2] + 1))
    return _matrix(entries, ordr, cols), _tensor(ia, (len(ia), 1), "union"), _tensor(ib, (len(ib), 1), "union")


def setdiff_rows(a, b, order="sorted"):
    """setdiff.rs:498-552, 891-930 -> (values [count, cols], ia [count, 1])"""
    a, b = _two_matrices(a, b, "setdiff")
    cols = a.shape[1]
    b_keys = {k for _, k in _rows_of(b, b.shape[0], cols)}
    seen, entries = set(), []  # entry: [row_data, row_index]
    for r, (row, k) in enumerate(_rows_of(a, a.shape[0], cols)):
        if k in b_keys or k in seen:
            continue
        seen.add(k)
        entries.append([row, r])
    ordr = _sorted(entries) if order == "sorted" else list(range(len(entries)))
    ia = [float(entries[e][1] + 1) for e in ordr]
    return _matrix(entries, ordr, cols), _tensor(ia, (len(ordr), 1), "setdiff")


def tensor_rows_cols(t, name):  # ismember.rs:755-765
    if t.ndim == 0:
        return 1, 1
    if t.ndim == 1:
        return t.shape[0], 1
    if t.ndim == 2:
        return t.shape[0], t.shape[1]
    raise RowsError(f"{name}: 'rows' option requires 2-D numeric matrices")


def ismember_rows(a, b):
    """ismember.rs:440-480 -> (mask uint8 [rows_a, 1], loc [rows_a, 1])"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    rows_a, cols_a = tensor_rows_cols(a, "ismember")
    rows_b, cols_b = tensor_rows_cols(b, "ismember")
    if cols_a != cols_b:
        raise RowsError("ismember: inputs must have the same number of columns when using 'rows'")
    lowest = {}
    for r, (_, k) in enumerate(_rows_of(b, rows_b, cols_b)):
        lowest.setdefault(k, r + 1)
    mask, loc = np.zeros((rows_a, 1), dtype=np.uint8), np.zeros((rows_a, 1), dtype=np.float64)
    for r, (_, k) in enumerate(_rows_of(a, rows_a, cols_a)):
        pos = lowest.get(k)
        if pos is not None:
            mask[r, 0], loc[r, 0] = 1, float(pos)
    return mask, loc
