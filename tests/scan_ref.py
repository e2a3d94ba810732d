"""Route tables, data classes, references, NaN / Inf placements and a model of the chunked scan for the cumulative scans
(rmhip_cumulative: cumsum_scan / cumprod_scan, reduce2.hip launch_cumulative; rmhip_cumextreme: cummin_scan / cummax_scan, order_ops.hip
launch_cumextreme).  Standard library and numpy only; tests/test_scan_ref_host.py checks this module on the CPU, tests/test_gpu_scan_paths.py
drives the kernels with it.

Everything works on SCAN-ORDERED lines: a 2-D array [nlines, len] whose row `i + pre * j` is line (i, j) of the column-major
[pre, len, post] view (reduce_ref.slices) and whose column k is the k-th element the scan meets.  A forward scan reads a line as it lies
in memory, a reverse scan reads it back to front, so one set of lines and ONE reference serve both directions: `to_memory` flips the
columns for a reverse scan, and the expected output is the reference flipped the same way.

Data classes, seeded:
  exact sums      integers in [-5, 5] with some entries -0.0: every association order gives the same bits.  The CPU's running value
                  starts at +0, so no output is ever -0.0 - line 0 starts with -0.0 to hold the kernels to that.
  exact products  telescoping exponents: targets t_i in [-20, 20], x_i = +-2^(t_i - t_(i-1)) with t_(-1) = 0, so the prefix of a line is
                  +-2^(t_i) and the product of ANY contiguous segment is +-2^(t_j - t_i), within 2^+-40.  At most eight entries per line
                  are +-3, +-5 or +-7 (their product < 7^8 < 2^23) and sit, like every entry a placement overwrites, where the target does
                  not move (t_i = t_(i-1)), so that leaving one out in omit mode shifts nothing.  Every grouping the kernels use is exact,
                  f32 holds every prefix, and neighbouring prefixes differ - a carry taken from the wrong chunk shows.
  rounded sums    full mantissas in (-1, 1).
  rounded products  x_i = +-fl(2^(s_i - s_(i-1))) with real s_i in [-8, 8]: prefixes stay within 2^+-8 up to rounding.

References: the exact classes take numpy's sequential cumsum / cumprod of the scan-ordered line started from the identity
(`seq_scan`; the host test holds it to the oracle's `cumulative`); the rounded classes the same scan in np.longdouble with the bound
  |got - S_k| <= (gamma_k + k 2^-63) sum_(i<=k) |x_i|,   |got - P_k| <= (gamma_k + k 2^-63) |P_k|,   gamma_k = k u / (1 - k u), u = 2^-53:
output k is the sum (product) of the first k values in SOME association order started from the identity - k operations, each within u
(Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1) - and the 80-bit reference's own k roundings are within 2^-64 each.
"""
import numpy as np

from reduce_ref import realise, slices, unslice  # noqa: F401  (re-exported for the tests)

NUM_CUS = 256  # the CU count the tables were pinned for (tests/cpp/scan_route_check.cpp)
CONTIG_CHUNK = 16384  # reduce_plan.h SCAN_CHUNK
CONTIG_TILE = 2048    # a block's tile inside a chunk: 256 threads x 8 elements
CARRY_TRIP = 256      # chunk totals the carry kernel scans per trip

# (pre, len, post, kernel, lines per block, chunks per line, launches) on 256 CUs: the list tests/cpp/scan_route_check.cpp pins against
# reduce_plan.h route_scan.  Every row runs on the GPU.
SCAN_ROUTE_TABLE = [
    (2, 9, 1, "lines_64x32", 0, 1, 1), (7, 5000, 1, "lines_64x32", 0, 1, 1), (40, 255, 3, "lines_64x32", 0, 1, 1),
    (262144, 3, 1, "lines_256x8", 0, 1, 1), (512, 2, 512, "lines_256x8", 0, 1, 1),
    (8, 256, 1, "staged", 32, 1, 1), (40, 300, 1, "staged", 32, 1, 1), (33, 4095, 2, "staged", 32, 1, 1),
    (64, 256, 256, "staged", 64, 1, 1), (16384, 256, 1, "staged", 64, 1, 1),
    (9, 4096, 1, "staged", 32, 4, 3), (40, 9001, 1, "staged", 32, 8, 3), (17, 9001, 3, "staged", 32, 8, 3),
    (32, 8192, 2, "staged", 32, 8, 3), (8, 300000, 1, "staged", 32, 276, 3),
    (1, 1, 5, "short", 0, 1, 1), (1, 3, 1025, "short", 0, 1, 1), (1, 16, 300, "short", 0, 1, 1), (1, 255, 17, "short", 0, 1, 1),
    (1, 256, 3, "chunks", 0, 1, 1), (1, 16384, 2, "chunks", 0, 1, 1), (1, 16385, 2, "chunks", 0, 2, 3),
    (1, 70001, 3, "chunks", 0, 5, 3), (1, 4300000, 1, "chunks", 0, 263, 3), (1, 256, 65537, "chunks", 0, 1, 1),
]
# the two sides of the thresholds the GPU rows do not straddle: pinned by the host check, not run on the GPU
SCAN_HOST_ROWS = [
    (2048, 4096, 1, "staged", 32, 4, 3), (2049, 4096, 1, "staged", 32, 1, 1),
    (65535, 256, 1, "staged", 64, 1, 1), (65536, 256, 1, "lines_64x32", 0, 1, 1),
    (100, 255, 1, "lines_64x32", 0, 1, 1), (100, 256, 1, "staged", 32, 1, 1), (7, 256, 1, "lines_64x32", 0, 1, 1),
    (262143, 3, 1, "lines_64x32", 0, 1, 1), (16320, 256, 1, "staged", 32, 1, 1), (8, 4096, 65536, "lines_256x8", 0, 1, 1),
    (1, 255, 3, "short", 0, 1, 1),
]
# (pre, len, post, form, chunks per line, chunk length): reduce_plan.h route_cumextreme on 256 CUs
CUMEXT_ROUTE_TABLE = [
    (1, 511, 3, "wave", 1, 512), (1, 512, 3, "wave", 2, 256), (1, 300000, 1, "wave", 586, 512),
    (1, 600, 2048, "wave", 1, 768), (1, 600, 2047, "wave", 2, 512),
    (300, 511, 1, "thread", 1, 511), (300, 512, 1, "thread", 2, 256), (7, 5000, 1, "thread", 19, 264), (2, 70001, 1, "thread", 273, 257),
]

Z_SPILL_ROW = (1, 256, 65537, "chunks", 0, 1, 1)  # 16.8 M elements: sums of the exact class only
F32_LIMIT = 1_000_000      # rows below this many elements also run on a precision-32 provider
ROUNDED_LIMIT = 5_000_000  # the rounded class runs on rows up to this many elements
BIT_IDENTICAL = ("lines_64x32", "lines_256x8", "short")  # the CPU's own sequence of operations; so is "staged" with one chunk


def row_id(row) -> str:
    return f"{row[0]}x{row[1]}x{row[2]}-{row[3]}"


def numel(row) -> int:
    return row[0] * row[1] * row[2]


def chunk_steps(row) -> int:
    """elements per chunk as the kernel cuts a line: whole tiles of 64 steps for the staged form, SCAN_CHUNK for the contiguous one
    (whatever the chunk count); 0 for the forms without chunks"""
    _, n, _, kernel, _, nchunks, _ = row
    if kernel == "staged":
        return -(-(-(-n // nchunks)) // 64) * 64
    return CONTIG_CHUNK if kernel == "chunks" else 0


def is_cpu_sequence(row) -> bool:
    return row[3] in BIT_IDENTICAL or (row[3] == "staged" and row[5] == 1)


def to_memory(lines: np.ndarray, reverse: bool) -> np.ndarray:
    """scan-ordered lines <-> lines as they lie in memory (its own inverse)"""
    return lines[:, ::-1] if reverse else lines


# ---- placements ---------------------------------------------------------------------------------------------------------------------
def positions(row):
    """scan positions where a special value must sit, the route's own boundaries first: the ends of the first chunks, both ends of the
    (ragged) last chunk, either side of the carry kernel's second trip; for the contiguous form also a tile boundary; then the ends of
    the line and of a wave's first row"""
    n, kernel, nchunks = row[1], row[3], row[5]
    c = chunk_steps(row)
    p = []
    if c:
        p += [c - 1, c, 2 * c - 1]
        if nchunks > 1:
            p += [(nchunks - 1) * c, n - 1]
        if nchunks > CARRY_TRIP:
            p += [CARRY_TRIP * c - 1, CARRY_TRIP * c, CARRY_TRIP * c + 1]
    if kernel == "chunks":
        p += [CONTIG_TILE - 1, CONTIG_TILE]
    p += [0, 1, 63, 64, n - 2, n - 1]
    out = []
    for q in p:
        if 0 <= q < n and q not in out:
            out.append(q)
    return out


def special_lines(row):
    """the first and the last line; for the staged form lines 31 and 32 (the last lane of a 32-line block and the first of the next:
    with pre = 33 the second block has 31 idle lanes); for more contiguous lines than grid y holds, either side of the spill into z"""
    nl = row[0] * row[2]
    want = [0, nl - 1]
    if row[3] == "staged":
        want += [31, 32]
    if row[3] == "chunks" and nl > 65535:
        want += [65534, 65535]
    out = []
    for q in want:
        if 0 <= q < nl and q not in out:
            out.append(q)
    return out


def inf_pairs(row):
    """[(a, b)]: scan positions in one chunk and in a LATER one (the second and the last but one element of a line without chunks);
    with more than 256 chunks also the last chunk of the carry kernel's first trip and the first of its second"""
    n, nchunks = row[1], row[5]
    c = chunk_steps(row)
    if n < 2:
        return []
    if nchunks > 1:
        pairs = [(c - 1, (nchunks - 1) * c)]
        if nchunks > CARRY_TRIP:
            pairs.append((CARRY_TRIP * c - 1, CARRY_TRIP * c))
        return pairs
    return [(1, n - 2)] if n >= 4 else [(0, n - 1)]


def hold_columns(row):
    """every column a placement may overwrite: the exact products keep their target exponent there"""
    cols = set(positions(row))
    for a, b in inf_pairs(row):
        cols |= {a, b}
    return sorted(cols)


def variants(row, prod: bool, single_nans: bool = True):
    """[(name, modes, [(line, position, value)])]: what to write into a copy of the clean lines, and in which NaN modes
    ('include', 'omit') to run it.
      clean      nothing
      one_nan*   ONE NaN per line, every position of `positions` on some line (the special lines first; as many variants as the
                 row's line count needs).  Include mode: everything before it is compared as numbers, everything from it on is NaN
      many_nan   every position on every special line
      whole_nan  a line of NaNs: omit mode gives +0 (sums) or 1.0 (products) throughout
      inf_pair*  +Inf in one chunk, -Inf in a later one: the sum is NaN from the second on in BOTH modes (Inf - Inf is computed, not met);
                 the product is -Inf
      zero_inf*  products: 0 in one chunk, Inf in a later one - zero up to the Inf, NaN from it on"""
    nl = row[0] * row[2]
    pos, sl = positions(row), special_lines(row)
    both = ("include", "omit")
    out = [("clean", both, [])]
    if single_nans:
        targets = sl + [int(q) for q in np.linspace(0, nl - 1, num=min(nl, len(pos))).astype(np.int64) if int(q) not in sl]
        per = len(targets)
        for v in range(-(-len(pos) // per)):
            out.append((f"one_nan{v}", ("include",), [(targets[k], p, np.nan) for k, p in enumerate(pos[v * per:(v + 1) * per])]))
    out.append(("many_nan", both, [(ln, p, np.nan) for ln in sl for p in pos]))
    out.append(("whole_nan", both, [(sl[-1], None, np.nan)]))
    for k, (a, b) in enumerate(inf_pairs(row)):
        out.append((f"inf_pair{k}", both, [(ln, q, v) for ln in sl for q, v in ((a, np.inf), (b, -np.inf))]))
        if prod:
            out.append((f"zero_inf{k}", both, [(ln, q, v) for ln in sl for q, v in ((a, 0.0), (b, np.inf))]))
    return out


def apply_specials(lines: np.ndarray, specials) -> np.ndarray:
    out = lines.copy()
    for ln, p, v in specials:
        if p is None:
            out[ln, :] = v
        else:
            out[ln, p] = v
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def exact_sum_lines(rng, nl: int, n: int) -> np.ndarray:
    x = rng.integers(-5, 6, size=(nl, n)).astype(np.float64)
    x[rng.random((nl, n)) < 1.0 / 16] = -0.0
    x[0, 0] = -0.0
    return x


def exact_prod_lines(rng, nl: int, n: int, hold=()) -> np.ndarray:
    """see the module docstring; `hold`: columns where the target exponent stays (the placements' columns)"""
    t = np.zeros((nl, n + 1), dtype=np.int64)  # column 0 is t_(-1) = 0
    t[:, 1:] = rng.integers(-20, 21, size=(nl, n))
    held = np.zeros((nl, n + 1), dtype=bool)
    held[:, [h + 1 for h in hold]] = True
    nodd = min(8, n // 3)
    odd_at = rng.integers(0, n, size=(nl, nodd))  # (a repeated column: fewer than eight)
    rows = np.arange(nl)[:, None]
    held[rows, odd_at + 1] = True
    src = np.where(held, 0, np.arange(n + 1)[None, :])
    np.maximum.accumulate(src, axis=1, out=src)  # the last column before that is not held
    t = np.take_along_axis(t, src, axis=1)
    x = np.ldexp(rng.choice([-1.0, 1.0], size=(nl, n)), (t[:, 1:] - t[:, :-1]).astype(np.int32))
    x[rows, odd_at] = rng.choice([-1.0, 1.0], size=(nl, nodd)) * rng.choice([3.0, 5.0, 7.0], size=(nl, nodd))
    return x


def rounded_sum_lines(rng, nl: int, n: int) -> np.ndarray:
    return rng.uniform(-1.0, 1.0, size=(nl, n))


def rounded_prod_lines(rng, nl: int, n: int) -> np.ndarray:
    s = np.zeros((nl, n + 1))
    s[:, 1:] = rng.uniform(-8.0, 8.0, size=(nl, n))
    return rng.choice([-1.0, 1.0], size=(nl, n)) * np.exp2(s[:, 1:] - s[:, :-1])


def exact_lines(rng, row, prod: bool) -> np.ndarray:
    nl, n = row[0] * row[2], row[1]
    return exact_prod_lines(rng, nl, n, hold_columns(row)) if prod else exact_sum_lines(rng, nl, n)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def seq_scan(lines: np.ndarray, prod: bool, omit: bool, dtype=np.float64) -> np.ndarray:
    """the CPU's scan of scan-ordered lines: left to right from the identity (+0 or 1.0).  Include mode: the running value does what
    NaN does by itself; omit mode: a NaN leaves it alone.  numpy's accumulate is the plain sequential loop but starts from the first
    element, so the identity is combined into that one by hand (0 + -0.0 is +0)."""
    ident = 1.0 if prod else 0.0
    v = np.where(np.isnan(lines), ident, lines) if omit else lines
    v = v.astype(dtype)  # a copy
    v[:, 0] = (ident * v[:, 0]) if prod else (ident + v[:, 0])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumprod(v, axis=1) if prod else np.cumsum(v, axis=1)


def same_bits(got, want) -> bool:
    """equal bits, signed zeros included; a NaN matches a NaN of any payload"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return np.array_equal(np.where(wn, 0.0, got).view(np.uint64), np.where(wn, 0.0, want).view(np.uint64))


def where_differs(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    bad = np.flatnonzero(~(((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))))
    return [(int(k), float(got[k]), float(want[k])) for k in bad[:5]], len(bad)


def scan_bounds(lines: np.ndarray, prod: bool):
    """(the scan of finite scan-ordered lines in np.longdouble, the module docstring's bound on every output)"""
    n = lines.shape[1]
    ld = np.longdouble
    k = np.arange(1, n + 1).astype(ld)
    u = ld(2.0) ** -53
    factor = k * u / (1 - k * u) + k * ld(2.0) ** -63
    ref = seq_scan(lines, prod, False, dtype=ld)
    scale = np.abs(ref) if prod else np.cumsum(np.abs(lines).astype(ld), axis=1)
    return ref, factor[None, :] * scale


def scan_error_ratios(got: np.ndarray, lines: np.ndarray, prod: bool, bounds=None):
    """(ok, largest error / bound) of scan-ordered outputs; `bounds`: scan_bounds(lines, prod) where several outputs share them"""
    ref, bound = scan_bounds(lines, prod) if bounds is None else bounds
    err = np.abs(got.astype(np.longdouble) - ref)
    ok = bool((err <= bound).all())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return ok, float(ratio.max())


# ---- a model of the chunked scan ------------------------------------------------------------------------------------------------------
DEFECTS = ("carry_is_previous_total", "ragged_carry_dropped", "second_trip_restarts", "nan_total_not_carried", "reverse_walks_chunks_forward",
           "negative_zero_kept")


def chunked_model(mem_lines: np.ndarray, prod: bool, reverse: bool, omit: bool, chunk: int, defect=None) -> np.ndarray:
    """The three passes of the chunked forms on lines AS THEY LIE IN MEMORY: every chunk's total (in numpy's own grouping - any will do),
    the carry into every chunk - an exclusive scan of the line's totals, 256 per trip with the running carry handed from trip to trip -
    and every chunk scanned from its carry; NaN policies and canonical NaNs as the kernels have them.  `defect` switches one of the
    classical mistakes on (DEFECTS): the host test shows that the data classes and placements of this module catch each of them."""
    assert defect is None or defect in DEFECTS
    ident = 1.0 if prod else 0.0
    op = np.multiply if prod else np.add
    s = to_memory(mem_lines, reverse)
    nl, n = s.shape
    nch = -(-n // chunk)
    with np.errstate(invalid="ignore", over="ignore"):
        padded = np.full((nl, nch * chunk), ident)
        padded[:, :n] = np.where(np.isnan(s), ident, s) if omit else s
        c3 = padded.reshape(nl, nch, chunk)
        tot = op.reduce(c3, axis=2)
        if defect == "nan_total_not_carried":
            tot = np.where(np.isnan(tot), ident, tot)
        if defect == "reverse_walks_chunks_forward" and reverse:
            tot = tot[:, ::-1]
        carries = np.empty_like(tot)
        carry = np.full(nl, ident)
        for c0 in range(0, nch, CARRY_TRIP):
            incl = op.accumulate(tot[:, c0:c0 + CARRY_TRIP], axis=1)
            carries[:, c0] = carry
            carries[:, c0 + 1:c0 + CARRY_TRIP] = op(carry[:, None], incl[:, :-1])
            carry = np.full(nl, ident) if defect == "second_trip_restarts" else op(carry, incl[:, -1])
        if defect == "carry_is_previous_total":
            carries[:, 1:] = tot[:, :-1]
        if defect == "reverse_walks_chunks_forward" and reverse:
            carries = carries[:, ::-1]
        if defect == "ragged_carry_dropped" and n % chunk:
            carries[:, -1] = ident
        c3 = c3.copy()
        c3[:, :, 0] = op(carries, c3[:, :, 0])
        out = op.accumulate(c3, axis=2).reshape(nl, nch * chunk)[:, :n]
    out = np.where(np.isnan(out), np.nan, out)
    if defect == "negative_zero_kept":
        first = padded[:, 0]
        out[:, 0] = np.where(first == 0, first, out[:, 0])
    return to_memory(out, reverse)


# ---- cummin / cummax ------------------------------------------------------------------------------------------------------------------
def cumext_columns(row):
    """memory columns on either side of everything a cummin / cummax route cuts, for both scan directions: the chunks, the run of
    chunks one thread of the carry kernel owns when a line has more than 256 of them, a wave's rows of 64 and trips of 256, the ends"""
    n, nchunks, c = row[1], row[4], row[5]
    p = [0, 1, 63, 64, 255, 256, n - 2, n - 1]
    if nchunks > 1:
        p += [c - 1, c, 2 * c - 1, 2 * c, (nchunks - 1) * c - 1, (nchunks - 1) * c]
        if nchunks > 256:
            per = -(-nchunks // 256)
            p += [per * c - 1, per * c, 2 * per * c - 1, 2 * per * c]
    cols = set()
    for q in p:
        if 0 <= q < n:
            cols |= {q, n - 1 - q}
    return sorted(cols)


def cumext_cases(rng, row):
    """[(name, lines as they lie in memory)]
      ties    small integers (ties everywhere); the cut columns hold the line's extreme - the largest value on even lines, the smallest
              on odd ones - so the first occurrence must win across every cut, in both directions
      zeros   positive (even lines) or negative (odd lines) values with zeros as the extreme: +0 and -0 alternate along the cut columns
              (the other way round on every other pair of lines), more zeros at random: the FIRST zero's sign is the answer
      nans    `ties` with NaNs on the cut columns of the first, the last and every seventh line, a leading run of NaNs and a line of NaNs
      infs    normal deviates with infinities of both signs"""
    nl, n = row[0] * row[2], row[1]
    cols = cumext_columns(row)
    even = (np.arange(nl) % 2 == 0)[:, None]
    ties = rng.integers(-3, 4, size=(nl, n)).astype(np.float64)
    ties[:, cols] = np.where(even, 9.0, -9.0)
    zeros = (np.abs(rng.standard_normal((nl, n))) + 0.5) * np.where(even, 1.0, -1.0)
    z = rng.random((nl, n)) < min(0.5, 4.0 / n)
    zeros[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    flip = ((np.arange(nl) // 2) % 2 == 0)[:, None]
    for k, col in enumerate(cols):
        zeros[:, col:col + 1] = np.where(flip == (k % 2 == 0), 0.0, -0.0)
    nans = ties.copy()
    pick = sorted(set(range(0, nl, 7)) | {nl - 1})
    nans[np.ix_(pick, cols[1::2])] = np.nan
    nans[nl // 2, :min(n, 70)] = np.nan
    if nl > 2:
        nans[nl // 2 + 1, :] = np.nan
    infs = rng.standard_normal((nl, n))
    at = rng.random((nl, n)) < min(0.3, 2.0 / n)
    infs[at] = np.where(rng.random(int(at.sum())) < 0.5, np.inf, -np.inf)
    infs[0, cols] = np.inf
    infs[nl - 1, cols] = -np.inf
    return [("ties", ties), ("zeros", zeros), ("nans", nans), ("infs", infs)]
