"""A numpy restatement of the in-process provider's two modulation loops (crates/runmat-accelerate/src/simple_provider.rs:4143-4310), the
contract of `modulate_constellation` and `modulate_bits_constellation`.  Each function returns `(interleaved, shape)` - the result's
(re, im) doubles in linear order and its shape - or `(message, failing index)`: the CPU stops at the first failing element in traversal
order, at its first failing check, and the index is that element's linear position in the input (for a group's range error, its last bit).
The loops are written element by element on purpose; nothing here is vectorised, so nothing can reorder the checks."""
import math

import numpy as np

SYMBOL_MESSAGES = ("modulate_constellation: symbols must be finite integers",
                   "modulate_constellation: symbols must be nonnegative integers",
                   "modulate_constellation: symbols must be in range")
BIT_MESSAGES = ("modulate_bits_constellation: bits must be finite",
                "modulate_bits_constellation: bits must be 0 or 1",
                "modulate_bits_constellation: symbols must be in range")
TABLE_MESSAGE = "requires interleaved real/imag constellation pairs"
GROUPING_MESSAGE = "modulate_bits_constellation: invalid bit grouping"
MULTIPLE_MESSAGE = "modulate_bits_constellation: bit rows must be a multiple of bits_per_symbol"
ROWS_MESSAGE = "modulate_bits_constellation: input_rows must match the input leading dimension"


def rust_round(v: float) -> float:
    """f64::round: halves away from zero (Python's round() goes to even)"""
    return math.copysign(math.floor(abs(v) + 0.5), v) if abs(v) < 2.0 ** 52 else v


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def modulate_constellation(data, shape, constellation):
    """simple_provider.rs:4153-4206; `data` in linear (column-major) order"""
    table = [float(v) for v in constellation]
    if not table or len(table) % 2:
        return "modulate_constellation " + TABLE_MESSAGE, None
    order = len(table) // 2
    out = []
    for i, value in enumerate(float(v) for v in data):
        if not math.isfinite(value):
            return SYMBOL_MESSAGES[0], i
        rounded = rust_round(value)
        if not (abs(value - rounded) <= 1e-9 and rounded >= 0.0):
            return SYMBOL_MESSAGES[1], i
        if not rounded < order:  # the CPU's `as usize` saturates, so a huge value compares as out of range
            return SYMBOL_MESSAGES[2], i
        symbol = int(rounded)
        out += [table[2 * symbol], table[2 * symbol + 1]]
    return np.array(out, dtype=np.float64), tuple(shape)


def modulate_bits_constellation(data, shape, input_rows, bits_per_symbol, constellation):
    """simple_provider.rs:4220-4308; `data` in linear (column-major) order"""
    table = [float(v) for v in constellation]
    if not table or len(table) % 2:
        return "modulate_bits_constellation " + TABLE_MESSAGE, None
    if input_rows == 0 or bits_per_symbol == 0:
        return GROUPING_MESSAGE, None
    if input_rows % bits_per_symbol:
        return MULTIPLE_MESSAGE, None
    order = len(table) // 2
    data = [float(v) for v in data]
    if len(shape) == 0 or shape[0] != input_rows:
        return ROWS_MESSAGE, None
    output_rows = input_rows // bits_per_symbol
    channels = len(data) // input_rows
    out = []
    for channel in range(channels):
        for group in range(output_rows):
            symbol = 0
            for bit_idx in range(bits_per_symbol):
                i = channel * input_rows + group * bits_per_symbol + bit_idx
                value = data[i]
                if not math.isfinite(value):
                    return BIT_MESSAGES[0], i
                rounded = rust_round(value)
                if not (abs(value - rounded) <= 1e-9 and (rounded == 0.0 or rounded == 1.0)):
                    return BIT_MESSAGES[1], i
                symbol = (symbol << 1) | int(rounded)
            if not symbol < order:
                return BIT_MESSAGES[2], i
            out += [table[2 * symbol], table[2 * symbol + 1]]
    return np.array(out, dtype=np.float64), (output_rows,) + tuple(shape[1:])


# ---- the edge values both hooks must judge exactly as the loops above do -----------------------------------------------------------------
def _around(v: float):
    """v and the two neighbouring doubles on each side"""
    lo1 = np.nextafter(v, -np.inf)
    hi1 = np.nextafter(v, np.inf)
    return [float(np.nextafter(lo1, -np.inf)), float(lo1), float(v), float(hi1), float(np.nextafter(hi1, np.inf))]


def symbol_edges(order: int):
    """-0.0 and -1e-10 (symbol 0); k +- 1e-9 with their neighbours for k in {0, 1, 7}: the tolerance's edge as the f64 subtraction sees it;
    a half; the last symbol plus 1e-10; the order itself; 1e300 and 2^53 (finite integers far out of range); NaN and the infinities"""
    values = [-0.0, -1e-10, 2.0000000004]
    for k in (0.0, 1.0, 7.0):
        values += _around(k - 1e-9) + _around(k + 1e-9)
    values += [0.5, -1.0, order - 1 + 1e-10, float(order), 1e300, 2.0 ** 53, float("nan"), float("inf"), float("-inf")]
    return values


def bit_edges():
    values = [-0.0, -1e-10, 1e-10, 1.0 + 1e-10, 2.0, 0.5, -1.0, 1e300, 2.0 ** 53, float("nan"), float("inf"), float("-inf")]
    for k in (0.0, 1.0):
        values += _around(k - 1e-9) + _around(k + 1e-9)
    return values
