"""Exact references, framed operands and the route table for the GEMM kernels (dgemm.hip, sgemm.hip).

Operands are integer valued and NONZERO, so every term of every inner product matters (a zero would hide a dropped or duplicated
element): f64 entries from {+-1 .. +-8}, f32 entries from {+-1 .. +-4}.  With k <= K_MAX = 2100 every product and every partial sum,
in any association order, is an exact integer - below 64 * 2100 < 2^53, respectively 16 * 2100 < 2^24 - so the reference is
`A.astype(int64) @ B.astype(int64)` and a kernel's result is compared for equality, not against a bound.  Scalars and scales are
powers of two or +-1 (alpha, beta from {1, -1, 2, 0.5, 0}), so alpha * A B + beta * C and the clamped epilogue stay exact too.  Only
the EP_POW epilogue rounds; `pow_tolerance` is the bound tests/test_gpu_parity.py test_matmul_epilogue_vs_oracle uses.

Frames (`blk_gemm`, the one entry point that takes views): each operand is a view inside a larger buffer; outside the views A and B
hold NaN and C holds a sentinel pattern, and where beta == 0 the C view itself holds NaN.  `framed` returns the expected FULL C
buffer: after the product it must match bit for bit (view exact, frame untouched), and no NaN may appear - a clamped load that is
multiplied by zero instead of selected away would show as one.  Every other entry point (matmul, transpose views, syrk,
matmul_epilogue, pagefun, and all of precision 32) takes and returns whole buffers, so those routes - w8g ta, w8g epi, w4 edge tb,
pgemm, every f32 kernel - are checked for exact values only: nothing can be poisoned beside their operands, and a guarded read or
write past them would not be seen here.

The case tables give, for each case, the entry point, the shape and the route the launcher must report (rmhip_gemm_last_route):
kernel, flags, splits, k_chunk.  The expectations are written down for NUM_CUS = 256 compute units (the thresholds are
blocks * 4 <= num_cus for split-K and blocks * 2 <= num_cus for the 64 x 64 tiles); tests/test_gemm_ref_host.py checks them against
the divisibility and alignment rules of the launchers, tests/test_gpu_gemm_paths.py against what ran.  `run_case` is shared by the
GPU tests and the child processes they start for the process-static RMHIP_GEMM_* knobs.  numpy and the standard library only.
"""
import hashlib
import zlib

import numpy as np

NUM_CUS = 256
K_MAX = 2100
ALPHAS = (1.0, -1.0, 2.0, 0.5, 0.0)

# frames of a view inside its parent: (row offset, column offset, rows behind, columns behind)
EVEN = (2, 1, 2, 1)      # even offset, and an even leading dimension when the view's row count is even: 16-byte loads stay legal
ODD_BASE = (3, 1, 1, 1)  # odd row offset: the base is 8 bytes past a 16-byte boundary
ODD_LD = (2, 1, 3, 1)    # odd parent row count when the view's is even


def route(text, splits=1, k_chunk=None):
    """'w8g ta' -> the dict rmhip_gemm_last_route reports; `edge` (w4, s_w4) and `guard` name the same field."""
    words = text.split()
    flags = set(words[1:])
    assert flags <= {"guard", "edge", "pre", "ta", "tb", "epi1", "epi2"}, text
    return {"kernel": words[0], "guard": int("guard" in flags or "edge" in flags), "pre": int("pre" in flags), "ta": int("ta" in flags),
            "tb": int("tb" in flags), "epi": 1 if "epi1" in flags else 2 if "epi2" in flags else 0, "yield": 0, "splits": splits,
            "k_chunk": k_chunk}


def case(entry, m, n, k, text, splits=1, k_chunk=None, **opts):
    """entry: matmul | matmul_ta | matmul_tb | syrk | epilogue | blk | pagefun.  opts: alpha, beta (blk), fa / fb / fc (blk frames),
    pow (epilogue with an exponent), pages."""
    r = route(text, splits, k if k_chunk is None else k_chunk)
    name = f"{entry}-{m}x{n}x{k}-{text.replace(' ', '_')}" + "".join(f"-{key}{val}" for key, val in sorted(opts.items()))
    return {"id": name.replace(" ", ""), "entry": entry, "m": m, "n": n, "k": k, "route": r, **opts}


def _updates(m, n, k, text, **kw):
    """C <- C - A B through blk_gemm: the preloaded-C forms."""
    return case("blk", m, n, k, text, alpha=-1.0, beta=1.0, **kw)


# ---- f64, default knobs -------------------------------------------------------------------------------------------------------------
F64_CASES = [
    # 64 x 64 tiles: at most 128 tiles of 128 x 128 and k <= 1024, or a skinny output
    case("matmul", 64, 64, 16, "small"), case("matmul", 192, 128, 1008, "small"),
    case("matmul", 2048, 1024, 16, "small"),   # 128 tiles: the last that stays small
    case("matmul", 64, 16512, 16, "small"),    # 129 tiles, skinny
    case("blk", 64, 64, 16, "small", alpha=1.0, beta=0.0), case("blk", 64, 64, 16, "small", alpha=0.5, beta=2.0),
    case("blk", 128, 192, 32, "small", alpha=0.0, beta=-1.0),
    _updates(64, 64, 16, "small pre"), _updates(128, 192, 32, "small pre"),
    case("matmul", 1, 1, 1, "small guard"), case("matmul", 65, 63, 17, "small guard"), case("matmul", 63, 130, 33, "small guard"),
    case("matmul", 1, 300, 5, "small guard"),
    case("blk", 65, 63, 17, "small guard", alpha=1.0, beta=0.0), case("blk", 63, 130, 33, "small guard", alpha=2.0, beta=-1.0),
    case("blk", 64, 64, 16, "small guard", alpha=1.0, beta=0.0, fa=ODD_BASE),
    case("blk", 64, 64, 16, "small guard", alpha=1.0, beta=0.0, fa=ODD_LD),
    case("blk", 64, 64, 16, "small guard", alpha=1.0, beta=0.0, fb=ODD_BASE),
    _updates(1, 1, 1, "small guard pre"), _updates(65, 63, 17, "small guard pre"), _updates(63, 130, 33, "small guard pre"),
    _updates(64, 64, 16, "small guard pre", fa=ODD_BASE), _updates(64, 64, 16, "small guard pre", fa=ODD_LD),
    # eight-wave 128 x 128 tile
    case("matmul", 2048, 1152, 16, "w8"),      # 144 tiles: the first past the small boundary
    case("matmul", 1664, 640, 1040, "w8"),     # 65 tiles, k > 1024: neither small nor split
    case("blk", 2048, 1152, 16, "w8", alpha=1.0, beta=0.0), case("blk", 2048, 1152, 16, "w8", alpha=0.5, beta=-1.0),
    _updates(2048, 1152, 16, "w8 pre"),
    case("matmul", 128, 128, 1024, "w8", 8, 128), case("matmul", 128, 128, 1040, "w8", 9, 128),  # the last slice 16 long
    case("matmul", 256, 128, 2048, "w8", 8, 256),
    case("blk", 128, 128, 1024, "w8", 8, 128, alpha=2.0, beta=-1.0), case("blk", 128, 128, 1040, "w8", 9, 128, alpha=2.0, beta=-1.0),
    case("blk", 256, 128, 2048, "w8", 8, 256, alpha=2.0, beta=-1.0),
    case("blk", 128, 128, 1024, "w8", 8, 128, alpha=-1.0, beta=1.0),  # an update that splits is not preloaded
    case("matmul_ta", 128, 128, 16, "w8 ta"), case("matmul_ta", 256, 128, 48, "w8 ta"),
    case("matmul_ta", 128, 128, 2048, "w8 ta", 8, 256), case("syrk", 128, 128, 2048, "w8 ta", 8, 256),
    case("epilogue", 128, 128, 16, "w8 epi1"), case("epilogue", 256, 128, 48, "w8 epi1"),
    case("epilogue", 128, 128, 16, "w8 epi2", pow=1.5), case("epilogue", 256, 128, 48, "w8 epi2", pow=1.5),
    # guarded eight-wave tile
    case("matmul", 2049, 1153, 17, "w8g guard"),
    case("blk", 2049, 1153, 17, "w8g guard", alpha=0.5, beta=-1.0),
    case("blk", 2048, 1152, 16, "w8g guard", alpha=1.0, beta=0.0, fa=ODD_BASE),
    case("blk", 2048, 1152, 16, "w8g guard", alpha=1.0, beta=0.0, fb=ODD_LD),
    _updates(2049, 1153, 17, "w8g guard pre"), _updates(2048, 1152, 16, "w8g guard pre", fa=ODD_BASE),
    case("matmul", 100, 100, 1100, "w8g guard", 9, 128),   # the last slice 76 long
    case("matmul", 129, 127, 2050, "w8g guard", 9, 256),   # the last slice 2 long
    case("blk", 100, 100, 1100, "w8g guard", 9, 128, alpha=2.0, beta=-1.0),
    case("blk", 129, 127, 2050, "w8g guard", 9, 256, alpha=2.0, beta=-1.0),
    case("matmul_ta", 65, 63, 17, "w8g guard ta"), case("matmul_ta", 2, 300, 5, "w8g guard ta"),
    case("matmul_ta", 100, 100, 1100, "w8g guard ta", 9, 128), case("syrk", 100, 100, 1100, "w8g guard ta", 9, 128),
    case("epilogue", 65, 63, 17, "w8g guard epi1"), case("epilogue", 130, 129, 31, "w8g guard epi1"),
    case("epilogue", 65, 63, 17, "w8g guard epi2", pow=1.5), case("epilogue", 130, 129, 31, "w8g guard epi2", pow=1.5),
    # A * B': the four-wave tile, whole and element-checked
    case("matmul_tb", 128, 128, 16, "w4 tb"), case("matmul_tb", 256, 128, 48, "w4 tb"), case("matmul_tb", 65, 63, 17, "w4 edge tb"),
    case("matmul_tb", 128, 128, 2048, "w4 tb", 8, 256), case("matmul_tb", 128, 128, 1040, "w4 edge tb", 9, 128),
    case("matmul_tb", 100, 100, 1100, "w4 edge tb", 9, 128),
    # pagefun's large-page tier (pages of at least 256 x 256 that share no operand)
    case("pagefun", 258, 257, 17, "pgemm guard", pages=3),
]

# ---- f64, one child process per process-static knob ---------------------------------------------------------------------------------
KNOB_CASES = {
    "RMHIP_GEMM_W8": [  # = 0: the four-wave tile for whole tiles
        case("blk", 2048, 1152, 16, "w4", alpha=1.0, beta=0.0), case("matmul", 1664, 640, 1040, "w4"),
        _updates(2048, 1152, 16, "w4 pre"),
        case("matmul_ta", 128, 128, 16, "w4 ta"), case("matmul_ta", 128, 128, 2048, "w4 ta", 8, 256),
        case("matmul", 128, 128, 1024, "w4", 8, 128), case("matmul", 128, 128, 1040, "w4 edge", 9, 128),
        case("blk", 256, 128, 2048, "w4", 8, 256, alpha=2.0, beta=-1.0),
        case("epilogue", 128, 128, 16, "w4 edge epi1"), case("epilogue", 256, 128, 48, "w4 edge epi2", pow=1.5),
        case("matmul", 2049, 1153, 17, "w4 edge"), case("matmul", 64, 64, 16, "small"),
    ],
    "RMHIP_GEMM_GUARD": [  # = 0: the element-checking four-wave tile for everything ragged
        case("matmul", 2049, 1153, 17, "w4 edge"), case("matmul", 65, 63, 17, "w4 edge"), case("matmul", 1, 1, 1, "w4 edge"),
        case("blk", 63, 130, 33, "w4 edge", alpha=2.0, beta=-1.0), _updates(65, 63, 17, "w4 edge"),
        case("blk", 64, 64, 16, "w4 edge", alpha=1.0, beta=0.0, fa=ODD_BASE), case("blk", 64, 64, 16, "w4 edge", alpha=1.0, beta=0.0, fb=ODD_LD),
        case("matmul", 100, 100, 1100, "w4 edge", 9, 128), case("blk", 129, 127, 2050, "w4 edge", 9, 256, alpha=2.0, beta=-1.0),
        case("matmul_ta", 65, 63, 17, "w4 edge ta"), case("matmul_ta", 2, 300, 5, "w4 edge ta"),
        case("matmul_ta", 100, 100, 1100, "w4 edge ta", 9, 128),
        case("epilogue", 65, 63, 17, "w4 edge epi1"), case("epilogue", 130, 129, 31, "w4 edge epi2", pow=1.5),
        case("matmul", 64, 64, 16, "small"), case("matmul", 2048, 1152, 16, "w8"),
    ],
    "RMHIP_GEMM_SMALL": [  # = 0: the 128 x 128 tiles on the small shapes
        case("matmul", 128, 128, 16, "w8"), case("matmul", 256, 128, 1008, "w8"), case("matmul", 128, 16512, 16, "w8"),
        case("matmul", 64, 64, 16, "w8g guard"), case("matmul", 64, 16512, 16, "w8g guard"),
        _updates(128, 256, 32, "w8 pre"), _updates(64, 64, 16, "w8g guard pre"),
        case("matmul", 1, 1, 1, "w8g guard"), case("matmul", 65, 63, 17, "w8g guard"), case("matmul", 63, 130, 33, "w8g guard"),
        _updates(65, 63, 17, "w8g guard pre"), _updates(128, 128, 16, "w8g guard pre", fa=ODD_BASE),
    ],
    "RMHIP_GEMM_PRELOAD": [  # = 0: the updates on the kernels that read C at the end
        _updates(64, 64, 16, "small"), _updates(65, 63, 17, "small guard"), _updates(2048, 1152, 16, "w8"),
        _updates(2049, 1153, 17, "w8g guard"), _updates(64, 64, 16, "small guard", fa=ODD_LD),
    ],
}

# ---- f32 matrix-core kernels (a precision-32 provider; sgemm.hip has the same 128 x 128 x 16 tile) --------------------------------------
F32_CASES = [
    case("matmul", 128, 128, 16, "s_w8"), case("matmul", 256, 128, 48, "s_w8"), case("matmul", 128, 384, 1008, "s_w8"),
    case("matmul_ta", 128, 128, 16, "s_w8 ta"), case("matmul_ta", 256, 128, 48, "s_w8 ta"), case("syrk", 128, 128, 48, "s_w8 ta"),
    case("matmul", 1, 1, 1, "s_w8g guard"), case("matmul", 65, 63, 17, "s_w8g guard"), case("matmul", 130, 129, 31, "s_w8g guard"),
    case("matmul", 128, 128, 17, "s_w8g guard"),
    case("matmul_ta", 65, 63, 17, "s_w8g guard ta"), case("matmul_ta", 2, 300, 5, "s_w8g guard ta"),
    case("matmul_ta", 130, 129, 31, "s_w8g guard ta"), case("syrk", 63, 63, 130, "s_w8g guard ta"),
    case("matmul_tb", 128, 128, 16, "s_w4 tb"), case("matmul_tb", 256, 128, 48, "s_w4 tb"),
    case("matmul_tb", 65, 63, 17, "s_w4 edge tb"), case("matmul_tb", 130, 129, 31, "s_w4 edge tb"),
    # split-K: whole slices, a ragged last slice of a whole-tile shape, a ragged shape (the default-on home of k_sgemm<true, ...>)
    case("matmul", 128, 128, 1024, "s_w4", 8, 128), case("matmul", 256, 128, 2048, "s_w4", 8, 256),
    case("matmul", 128, 128, 1040, "s_w4 edge", 9, 128), case("matmul", 100, 100, 1100, "s_w4 edge", 9, 128),
    case("matmul", 129, 127, 2050, "s_w4 edge", 9, 256),
    case("matmul_ta", 128, 128, 2048, "s_w4 ta", 8, 256), case("syrk", 128, 128, 1024, "s_w4 ta", 8, 128),
    case("matmul_ta", 128, 128, 1040, "s_w4 edge ta", 9, 128), case("matmul_ta", 100, 100, 1100, "s_w4 edge ta", 9, 128),
    case("matmul_tb", 128, 128, 2048, "s_w4 tb", 8, 256), case("matmul_tb", 128, 128, 1040, "s_w4 edge tb", 9, 128),
    case("matmul_tb", 100, 100, 1100, "s_w4 edge tb", 9, 128),
]
F32_KNOB_CASES = {
    "RMHIP_SGEMM_W8": [  # = 0: the four-wave kernel for everything
        case("matmul", 128, 128, 16, "s_w4"), case("matmul", 256, 128, 48, "s_w4"), case("matmul_ta", 128, 128, 16, "s_w4 ta"),
        case("matmul", 65, 63, 17, "s_w4 edge"), case("matmul_ta", 65, 63, 17, "s_w4 edge ta"), case("matmul_ta", 2, 300, 5, "s_w4 edge ta"),
        case("matmul_tb", 128, 128, 16, "s_w4 tb"),
    ],
}


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def operand(rng, rows, cols, bits=64):
    """Nonzero integers: +-1 .. +-8 (f64) or +-1 .. +-4 (f32), as float64."""
    top = 8 if bits == 64 else 4
    return (rng.integers(1, top + 1, (rows, cols)) * rng.choice((-1, 1), (rows, cols))).astype(np.float64)


def exact_product(A, B):
    """The reference: the product in int64 (the entries are integers by construction)."""
    Ai, Bi = A.astype(np.int64), B.astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B) and A.shape[1] <= K_MAX
    return Ai @ Bi


def operands(c, bits=64):
    """(A, B, P) of a case: A is m x k, B is k x n, P = A B exactly (int64); seeded by the case's id."""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    if c["entry"] == "syrk":  # A' A of a k x m matrix
        assert c["m"] == c["n"]
        B = operand(rng, c["k"], c["n"], bits)
        A = B.T.copy()
    else:
        A, B = operand(rng, c["m"], c["k"], bits), operand(rng, c["k"], c["n"], bits)
    return A, B, exact_product(A, B)


def sentinel(rows, cols):
    """The frame of C: distinct, finite, not integers of the operands' range."""
    return -(1.0e6 + np.arange(rows * cols, dtype=np.float64).reshape(rows, cols, order="F") * 0.5)


def frame(X, f, fill=np.nan):
    """X as a view inside a parent: (parent, view tuple without the handle)."""
    r0, c0, r1, c1 = f
    parent = np.full((r0 + X.shape[0] + r1, c0 + X.shape[1] + c1), fill, dtype=np.float64)
    parent[r0:r0 + X.shape[0], c0:c0 + X.shape[1]] = X
    return parent, (r0, c0, X.shape[0], X.shape[1])


def framed(c, A, B, P):
    """The blk_gemm form of a case: parents of A, B (NaN outside the views) and C (sentinels outside; nonzero integers inside, or NaN
    where beta == 0), the three views and the expected full C buffer."""
    alpha, beta = c["alpha"], c["beta"]
    assert alpha in ALPHAS and beta in ALPHAS
    assert not (beta == 0.0 and alpha < 0.0)  # the sign of an exactly cancelling sum would depend on where alpha is applied
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()) ^ 0x5A5A)
    m, n = P.shape
    C0 = operand(rng, m, n) if beta != 0.0 else np.full((m, n), np.nan)
    pa, va = frame(A, c.get("fa", EVEN))
    pb, vb = frame(B, c.get("fb", EVEN))
    f = c.get("fc", EVEN)
    pc = sentinel(f[0] + m + f[2], f[1] + n + f[3])
    want = pc.copy()
    pc[f[0]:f[0] + m, f[1]:f[1] + n] = C0
    Pf = P.astype(np.float64)
    want[f[0]:f[0] + m, f[1]:f[1] + n] = alpha * Pf + beta * C0 if beta != 0.0 else alpha * Pf + 0.0
    return pa, va, pb, vb, pc, (f[0], f[1], m, n), want


EPILOGUE = dict(alpha=0.5, beta=-2.0, clamp_min=-32.0, clamp_max=48.0)  # with power-of-two row and column scales: exact
EPILOGUE_POW = dict(alpha=2.0 ** -6, clamp_min=0.0)                       # then pow: the one rounded case
EPS = 2.0 ** -52


def epilogue_scales(c):
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()) ^ 0xA5A5)
    pw = np.array([0.5, 1.0, 2.0, -1.0, -2.0])
    return rng.choice(pw, (c["m"], 1)), rng.choice(pw, (1, c["n"]))


def epilogue_exact(P, rs, cs):
    """EPILOGUE on the exact product, in the reference's order (scale, shift, row, column, clamps); every step is exact."""
    v = P.astype(np.float64) * EPILOGUE["alpha"] + EPILOGUE["beta"]
    v = v * rs
    v = v / cs
    return np.minimum(np.maximum(v, EPILOGUE["clamp_min"]), EPILOGUE["clamp_max"])


def pow_tolerance(A, B, alpha):
    """test_matmul_epilogue_vs_oracle's bound: (|alpha| * 4 + 1) * (k + 4) * eps * (|A| |B|) + 1e-13."""
    return (abs(alpha) * 4.0 + 1.0) * (A.shape[1] + 4) * EPS * (np.abs(A) @ np.abs(B)) + 1e-13


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- one case on a provider -----------------------------------------------------------------------------------------------------------
def run_case(prov, c, bits=64, swapped=False, oracle=None):
    """Runs case `c` once and returns {"route", "equal", "nan", "detail"}.  `swapped`: the product of the transposes, B' A' = (A B)',
    with the operands materialised the other way round (rows and columns of the output exchange; the route is the same because the
    tiles are square); it exists for matmul, blk and epilogue cases."""
    A, B, P = operands(c, bits)
    entry = c["entry"]
    if swapped:
        assert entry in ("matmul", "blk", "epilogue")
        A, B, P = B.T.copy(), A.T.copy(), P.T.copy()
    hs, detail, out_bits = [], "", bits  # (blk_gemm writes into the caller's f64 buffer: no new buffer whose width could differ)

    def up(x):  # column-major data with its shape: a plain buffer (a large row-major array would come back as a transpose view)
        x = np.asarray(x, dtype=np.float64)
        hs.append(prov.upload(x.ravel(order="F"), x.shape))
        return hs[-1]

    def up2(flat, shape):
        hs.append(prov.upload(flat, shape))
        return hs[-1]

    try:
        if entry == "blk":
            if swapped:
                c = dict(c, fa=c.get("fb", EVEN), fb=c.get("fa", EVEN))
            pa, va, pb, vb, pc, vc, want = framed(c, A, B, P)
            ha, hb, hc = up(pa), up(pb), up(pc)
            prov.blk_gemm(c["alpha"], (ha, *va), (hb, *vb), c["beta"], (hc, *vc))
            r = prov.gemm_last_route()
            got = prov.download_matrix(hc)
        elif entry == "pagefun":
            from runmat_amd import PagefunOp, PagefunRequest

            pages = c["pages"]
            rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
            As = [operand(rng, c["m"], c["k"]) for _ in range(pages)]
            Bs = [operand(rng, c["k"], c["n"]) for _ in range(pages)]
            want = np.stack([exact_product(a, b) for a, b in zip(As, Bs)], axis=2).astype(np.float64)
            A3, B3 = np.stack(As, axis=2), np.stack(Bs, axis=2)
            ha, hb = up2(A3.ravel(order="F"), A3.shape), up2(B3.ravel(order="F"), B3.shape)
            req = PagefunRequest(PagefunOp.Mtimes, [ha, hb], [c["m"], c["n"], pages], [pages], [[pages], [pages]])
            hs.append(prov.pagefun(req))
            r = prov.gemm_last_route()
            out_bits = prov.buffer_bits(hs[-1])
            got = prov.download(hs[-1]).reshape(want.shape, order="F")
        else:
            want = P.astype(np.float64)
            if entry == "matmul":
                hs.append(prov.matmul(up(A), up(B)))
            elif entry == "matmul_ta":  # A is stored k x m and consumed through a transpose view
                t = prov.transpose(up(A.T.copy()))
                hs.append(t)
                hs.append(prov.matmul(t, up(B)))
            elif entry == "matmul_tb":
                t = prov.transpose(up(B.T.copy()))
                hs.append(t)
                hs.append(prov.matmul(up(A), t))
            elif entry == "syrk":
                hs.append(prov.syrk(up(B)))
            elif entry == "epilogue":
                rs, cs = epilogue_scales(c)
                if swapped:
                    rs, cs = cs.T.copy(), rs.T.copy()
                if "pow" in c:
                    kw = dict(EPILOGUE_POW, pow_exponent=c["pow"])
                    hs.append(prov.matmul_epilogue(up(A), up(B), **kw))
                else:
                    want = epilogue_exact(P, rs, cs)
                    hs.append(prov.matmul_epilogue(up(A), up(B), row_scale=up(rs), col_scale=up(cs), col_op="divide", **EPILOGUE))
            else:
                raise ValueError(entry)
            r = prov.gemm_last_route()
            out = hs[-1]
            out_bits = prov.buffer_bits(out)
            got = prov.download_matrix(out)
        nan = bool(np.isnan(got).any())
        if entry == "epilogue" and "pow" in c:
            assert oracle is not None, "the EP_POW cases compare with oracle.matmul_epilogue"
            ref, _ = oracle.matmul_epilogue(A, B, **dict(EPILOGUE_POW, pow_exponent=c["pow"]))  # A B itself is exact in the oracle's f64 as well
            err = np.abs(got - ref)
            tol = pow_tolerance(A, B, EPILOGUE_POW["alpha"])
            equal = bool(np.all(err <= tol))
            if not equal:
                detail += f" max err / tol {float(np.max(err / tol)):.3g};"
        else:
            equal = same_bits(got, want)
            if not equal and got.shape == want.shape:
                bad = np.argwhere(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
                detail += f" {len(bad)} elements differ, first at {tuple(int(x) for x in bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r};"
                if entry == "blk":
                    r0, c0, rows, cols = vc
                    outside = [(int(a), int(b)) for a, b in bad if not (r0 <= a < r0 + rows and c0 <= b < c0 + cols)]
                    detail += f" {len(outside)} of them in the frame;"
        return {"id": c["id"] + ("-swapped" if swapped else ""), "route": r, "want_route": c["route"], "equal": equal, "nan": nan, "bits": out_bits,
                "want_bits": bits,
                "detail": detail.strip(), "digest": hashlib.sha1(np.ascontiguousarray(got).tobytes()).hexdigest()}
    finally:
        for h in hs:
            prov.free(h)


def check(res):
    """The assertions every case makes, in one place: the attested route, then the bits."""
    assert res["route"] == res["want_route"], f"{res['id']}: ran {res['route']}, the table says {res['want_route']}"
    assert res["bits"] == res["want_bits"], f"{res['id']}: the result is stored in {res['bits']} bits, not {res['want_bits']}"
    assert not res["nan"], f"{res['id']}: NaN in the result ({res['detail']})"
    assert res["equal"], f"{res['id']}: {res['detail']}"


def has_swap(c):
    return c["entry"] in ("matmul", "blk", "epilogue")


def child_main(table, knob, bits):
    """Body of the child process of one knob setting (the knobs are read once per process): every case of the knob's table, and its
    swapped form, on a fresh provider; one JSON line back.  Stops at the first error of the library."""
    import json
    import os

    from oracle import oracle
    from runmat_amd import HipProvider, ProviderError

    oracle.lib()
    prov = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32" if bits == 32 else "F64")
    out = {"compute_units": int(prov.device_info_struct()["compute_units"]), "results": [], "error": None}
    try:
        for c in {"f64": KNOB_CASES, "f32": F32_KNOB_CASES}[table][knob]:
            for swapped in ((False, True) if has_swap(c) else (False,)):
                out["results"].append(run_case(prov, c, bits, swapped, oracle))
    except ProviderError as e:
        out["error"] = str(e)
    print(json.dumps(out))
    prov.close()
