"""TEST INFRASTRUCTURE: coded operands, exact expectations and the case table for every form of the generated elementwise kernels.

`rmhip_fused_elementwise` launches one of four kernels of the module codegen.cpp generates - `rm_ew_fast` (16-byte vectors),
`rm_ew_fast1` (element-sized accesses, for memory that is not 16-byte aligned), `rm_ew_bcast` (dim 0 along the threads, a block per
chunk of dim 0 and outer index) and `rm_ew_bcast_flat` (threads over the flat output) - and the `RMHIP_EW_*` knobs reshape each of
them.  What can go wrong there is the mapping of elements to threads: a stride, a loop bound, a tail, a chunk edge.  So the operands
here are exact integers that encode each element's own position, the two programs keep every operand recoverable from a result, and
an expectation is numpy integer arithmetic - bit equality, no tolerance.

Plain numpy; nothing here touches the GPU.  tests/test_ew_forms_host.py pins this module, tests/test_gpu_ew_forms.py runs the table.
"""
from __future__ import annotations

import numpy as np

from planner_requests import FusionGroupPlan

PERIOD = 60491  # prime: no multiple of a block, grid, chunk or vector stride, so a shifted read of operand 0 never finds its own value
SCALAR_START = 4242  # position a 1-element operand's value is coded from (so that no scalar is 0)
CUS = 256  # compute units of an MI355X: what the host test resolves the symbolic lengths with; the GPU test asks the device

KNOB_NAMES = ("UNROLL", "BLOCK", "BLOCKS_PER_CU", "NT", "NT_LOAD", "NT_STORE", "CHUNKED", "BCAST_BLOCK", "BCAST_ELEMS")
KNOBS = {
    "K0": {},
    "K1": {"UNROLL": 4, "BLOCK": 64, "BLOCKS_PER_CU": 1},
    "K2": {"CHUNKED": 1, "UNROLL": 2, "BLOCK": 128, "BLOCKS_PER_CU": 1},
    "K3": {"CHUNKED": 1},
    "K4": {"NT": 0},
    "K5": {"UNROLL": 8},
    "K6": {"BCAST_BLOCK": 64, "BCAST_ELEMS": 1},
    "K7": {"BCAST_BLOCK": 1024, "BCAST_ELEMS": 8},
}
STREAMING_KNOBS = ("K0", "K1", "K2", "K3", "K4", "K5")  # the sets that leave the broadcast form alone


def set_knobs(monkeypatch, name):
    """Exactly the knob set `name` in the environment (EwTuning::from_env reads it at every kernel fetch)."""
    for k in KNOB_NAMES:
        monkeypatch.delenv("RMHIP_EW_" + k, raising=False)
    for k, v in KNOBS[name].items():
        monkeypatch.setenv("RMHIP_EW_" + k, str(v))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def coded(shape, k, start=0):
    """Operand k of the given shape as int64: element j of its column-major storage holds a code of `start + j`.  Operand 0 is
    `j mod PERIOD`; operand k >= 1 is `((5 + 2k) j + k) mod 256` - `(7 j + 1) mod 256` for the second, `(9 j + 2) mod 256` for the
    third, so that two byte-sized operands of one program never move together."""
    n = int(np.prod(shape, dtype=np.int64))
    j = np.arange(start, start + n, dtype=np.int64)
    v = j % PERIOD if k == 0 else ((5 + 2 * k) * j + k) % 256
    return v.reshape(shape, order="F")


def scalar_value(k):
    return int(coded((1, 1), k, SCALAR_START)[0, 0])


# ---- programs ---------------------------------------------------------------------------------------------------------------------
def _times256(p, v):
    for _ in range(8):  # the planner's requests carry constants as inputs; eight doublings keep the three / two inputs the programs are about
        v = p.primitive("Add", v, v)
    return v


def shader(prog, scalar_ty):
    """P1: three inputs, one output `a*256 + b - c`.  P3: two inputs, three outputs `a*256 + b`, `b*256 + a`, `a - b`.
    With a < PERIOD and b, c < 256 every intermediate and result is an integer of magnitude at most 60490 * 256 + 255 < 2^24: exact
    in f64 arithmetic and in f32 storage."""
    p = FusionGroupPlan()
    if prog == "P1":
        a, b, c = p.input(), p.input(), p.input()
        out = p.primitive("Sub", p.primitive("Add", _times256(p, a), b), c)
        return p.generate_wgsl_for_output(out, scalar_ty)
    assert prog == "P3"
    a, b = p.input(), p.input()
    outs = [p.primitive("Add", _times256(p, a), b), p.primitive("Add", _times256(p, b), a), p.primitive("Sub", a, b)]
    return p.generate_wgsl_for_outputs(outs, scalar_ty)


N_IN = {"P1": 3, "P3": 2}
N_OUT = {"P1": 1, "P3": 3}


def expected(prog, operands, out_shape):
    """The program over int64 operands (numpy broadcasting, which front-pads shapes as padded_strides does) -> one flat column-major
    f64 array per output."""
    ops = [np.asarray(x, dtype=np.int64) for x in operands]
    if prog == "P1":
        a, b, c = ops
        res = [a * 256 + b - c]
    else:
        a, b = ops
        res = [a * 256 + b, b * 256 + a, a - b]
    rank = len(out_shape)
    out = []
    for r in res:
        assert np.max(np.abs(r)) <= 1 << 24
        r = np.broadcast_to(r.reshape((1,) * (rank - r.ndim) + r.shape), out_shape)
        out.append(np.ascontiguousarray(r.reshape(-1, order="F")).astype(np.float64))
    return out


# ---- the launcher's decisions, restated (rmhip_ops.cpp rmhip_fused_elementwise, host_shape.h) ------------------------------------------
def collapsed_shape(op_shapes, out_shape):
    """Output shape after padded_strides + collapse for plain operands (a repmat view that replicates an extent-1 dim has the strides
    of its base, so it is described by the base's shape): extent-1 dims dropped, dim d + 1 merged into d where every operand is
    contiguous across the boundary or broadcast on both sides."""
    rank = len(out_shape)
    strides = []
    for sh in op_shapes:
        sh = list(sh)
        while len(sh) > rank and sh[-1] == 1:
            sh.pop()
        while len(sh) > rank and sh[0] == 1:
            sh.pop(0)
        sh = [1] * (rank - len(sh)) + sh
        st, s = [], 1
        for d in range(rank):
            assert sh[d] in (1, out_shape[d]), (sh, out_shape)
            st.append(0 if sh[d] == 1 else s)
            s *= sh[d]
        strides.append(st)
    ns, nst = [], [[] for _ in strides]
    for d in range(rank):
        if out_shape[d] == 1:
            continue
        if ns and all((st[-1] == 0 and s[d] == 0) or (st[-1] != 0 and s[d] == st[-1] * ns[-1]) for st, s in zip(nst, strides)):
            ns[-1] *= out_shape[d]
            continue
        ns.append(out_shape[d])
        for st, s in zip(nst, strides):
            st.append(s[d])
    return tuple(ns) if ns else (1,)


def expected_form(length, collapsed, aligned, knobs=None):
    """0 rm_ew_fast, 1 rm_ew_fast1, 2 rm_ew_bcast, 3 rm_ew_bcast_flat.  `aligned`: every streamed (non-scalar) operand starts on a
    16-byte boundary.  No knob moves a request between forms (the argument is there so that a change which makes one do so has to
    say how)."""
    del knobs
    if len(collapsed) == 1:
        return 0 if aligned else 1
    outer = int(np.prod(collapsed[1:], dtype=np.int64))
    return 3 if collapsed[0] < 128 and outer >= 64 and length < 1 << 31 else 2


def tuning(knob_set, prec, cus=CUS):
    """The effective numbers of a knob set: vec, block, unroll, grid cap G, elements per full trip of one block P."""
    k = KNOBS[knob_set]
    vec = 4 if prec == "f32" else 2
    block = (k.get("BLOCK", 1024) // 64) * 64
    unroll = k.get("UNROLL", 0) or 1
    return dict(vec=vec, block=block, unroll=unroll, G=cus * k.get("BLOCKS_PER_CU", 16), P=block * unroll * vec)


def trips(length, vec, block, unroll, grid):
    """Trips of the busiest thread through the (unrolled) streaming loop: `grid` blocks of `block` threads take `unroll` vectors
    of `vec` elements each per trip.  (vec = 1 for rm_ew_fast1.)  The chunked walk gives the same count: a block's chunk is the
    grid's share rounded up to whole trips."""
    nvec = length // vec
    per_pass = grid * block * unroll
    return -(-nvec // per_pass)


def resolve_len(spec, knob_set, prec, cus=CUS):
    """A length of the table: an int, or (g, h, v, k) = g * G * P + h * (P / 2) + v * vec * block + k in the knob set's numbers."""
    if spec is None or isinstance(spec, int):
        return spec
    t = tuning(knob_set, prec, cus)
    g, h, v, k = spec
    return g * t["G"] * t["P"] + h * (t["P"] // 2) + v * t["vec"] * t["block"] + k


BIG = (1, 0, 1, 1)  # G*P + vec*block + 1: the one multi-trip length of a set with the default block and grid cap
# 1, 2, 3, 4, 5, vec*block - 1, vec*block, vec*block + 1, P - 1, P + 1, G*P - 1, G*P, G*P + 1, BIG, 2*G*P + P/2 + 3: the main loop, the
# remainder loop, a ragged last trip and the odd (n & 3) tail
ALL_LENS = [1, 2, 3, 4, 5, (0, 0, 1, -1), (0, 0, 1, 0), (0, 0, 1, 1), (0, 2, 0, -1), (0, 2, 0, 1), (1, 0, 0, -1), (1, 0, 0, 0), (1, 0, 0, 1),
            BIG, (2, 1, 0, 3)]
MULTI_LENS = [BIG, (2, 1, 0, 3)]  # those that need a second trip (G*P + 1 still fills the first one exactly and adds a tail element)
SMALL_LENS = [1, 2, 3, 4, 5, (0, 0, 1, -1), (0, 0, 1, 0), (0, 0, 1, 1), (0, 2, 0, -1), (0, 2, 0, 1), 70001]
SOME_LENS = [2, 5, (0, 2, 0, 1), (1, 0, 0, 1), BIG, (2, 1, 0, 3)]


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# One list for both test files.  A row: id, prog, prec ("f64" | "f32": the provider), knobs (a key of KNOBS), ops (one spec per input),
# form (what the launch record must say) and either
#   lens: symbolic lengths n - the output is n x 1, a "full" operand n x 1 - with multi = those lengths that must record >= 2 trips, or
#   out:  the output shape, for operands given by their own shapes.
# Operand specs: ("full",) | ("scalar",) a [1,1] tensor | ("mis",) a full operand 8 bytes into an allocation one element longer |
# ("mis_scalar",) the same pointer as a [1,1] tensor | ("shape", s) a plain tensor of shape s | ("repmat", base, reps) a stride-0 view |
# ("transpose", s) the transpose view of a tensor of shape s.
FULL, SCALAR, MIS, MIS_SCALAR = ("full",), ("scalar",), ("mis",), ("mis_scalar",)
TABLE = []


def _stream(id_, prog, prec, knobs, ops, lens, form=0, multi=()):
    TABLE.append(dict(id=id_, prog=prog, prec=prec, knobs=knobs, ops=list(ops), lens=list(lens), out=None, form=form, multi=list(multi)))


def _shaped(id_, prog, prec, knobs, ops, out, form=None):
    ops = [o if isinstance(o[0], str) else ("shape", tuple(o)) for o in ops]
    if form is None:
        form = expected_form(int(np.prod(out, dtype=np.int64)), collapsed_shape([effective_shape(o) for o in ops], out), True, KNOBS[knobs])
    TABLE.append(dict(id=id_, prog=prog, prec=prec, knobs=knobs, ops=ops, lens=None, out=tuple(out), form=form, multi=[]))


def effective_shape(spec):
    """Shape whose padded strides are the operand's at launch: a stride-0 view reads its base, a transpose view is materialised."""
    if spec[0] == "shape":
        return spec[1]
    if spec[0] == "repmat":
        assert all(r == 1 or b == 1 for b, r in zip(spec[1], spec[2])), "only views that replicate extent-1 dims"
        return spec[1]
    assert spec[0] == "transpose"
    return spec[1][::-1]


def operand_values(spec, k, n=None):
    """int64 values of operand k in its LOGICAL shape (what the program sees), for a streaming row of length n or a shaped row."""
    kind = spec[0]
    if kind == "full":
        return coded((n, 1), k)
    if kind == "scalar":
        return coded((1, 1), k, SCALAR_START)
    if kind == "mis":
        return coded((n + 1, 1), k)[1:]
    if kind == "mis_scalar":
        return coded((2, 1), k, SCALAR_START)[1:]
    if kind == "shape":
        return coded(spec[1], k)
    if kind == "repmat":
        return np.tile(coded(spec[1], k), spec[2])
    assert kind == "transpose"
    return np.ascontiguousarray(coded(spec[1], k).T)


# -- streaming: every length under the two knob sets whose grid cap is small, both programs, both precisions
for _prec in ("f64", "f32"):
    for _k in ("K1", "K2"):
        _stream(f"stream-P1-{_k}-{_prec}", "P1", _prec, _k, [FULL, FULL, FULL], ALL_LENS, multi=MULTI_LENS)
        _stream(f"stream-P3-{_k}-{_prec}", "P3", _prec, _k, [FULL, FULL], ALL_LENS, multi=MULTI_LENS)
    _stream(f"stream-P1-K0-{_prec}", "P1", _prec, "K0", [FULL, FULL, FULL], SMALL_LENS)
# the default kernel and plain loads / stores at the small lengths; eight vectors per thread around its own P; the chunk walk alone
_stream("stream-P3-K4-f64", "P3", "f64", "K4", [FULL, FULL], SMALL_LENS)
_stream("stream-P3-K0-f64", "P3", "f64", "K0", [FULL, FULL], SMALL_LENS)
_stream("stream-P1-K4-f64", "P1", "f64", "K4", [FULL, FULL, FULL], SMALL_LENS)
_stream("stream-P3-K5-f64", "P3", "f64", "K5", [FULL, FULL], [3, (0, 2, 0, -1), (0, 2, 0, 1), (0, 4, 0, 3), (0, 7, 0, 5)])
_stream("stream-P3-K3-f64", "P3", "f64", "K3", [FULL, FULL], [1, 3, 2049, 70001])
# one multi-trip case under each set that keeps the default grid cap: one full-size input, two [1,1] scalars.  Under K3 the chunk is
# the grid's share rounded up to whole trips - two trips of 1024 vectors for a share of 1025 - so the upper half of the blocks begin
# beyond the end.
for _k in ("K0", "K3", "K4", "K5"):
    _stream(f"big-P1-{_k}-f64", "P1", "f64", _k, [FULL, SCALAR, SCALAR], [BIG], multi=[BIG])
# -- [1,1] scalars in each input slot: the scalar-mask kernels still report form 0
for _slot in range(3):
    _stream(f"scalar{_slot}-P1-K1-f64", "P1", "f64", "K1", [SCALAR if s == _slot else FULL for s in range(3)], SOME_LENS, multi=MULTI_LENS)
for _slot in range(2):
    _stream(f"scalar{_slot}-P3-K1-f64", "P3", "f64", "K1", [SCALAR if s == _slot else FULL for s in range(2)], SOME_LENS, multi=MULTI_LENS)
_stream("scalar1-P1-K2-f32", "P1", "f32", "K2", [FULL, SCALAR, FULL], SOME_LENS, multi=MULTI_LENS)
# -- misalignment (f64 provider; wrap_external adopts f64 memory only, so form 1 on f32 storage is unreachable): the operand 8 bytes into
# its allocation in each slot -> rm_ew_fast1; the same pointer as a 1-element operand is read as a scalar -> rm_ew_fast
for _slot in range(3):
    _stream(f"mis{_slot}-P1-K1-f64", "P1", "f64", "K1", [MIS if s == _slot else FULL for s in range(3)], ALL_LENS[1:], form=1, multi=MULTI_LENS)
    _stream(f"mis-scalar{_slot}-P1-K1-f64", "P1", "f64", "K1", [MIS_SCALAR if s == _slot else FULL for s in range(3)], SOME_LENS, multi=MULTI_LENS)
for _slot in range(2):
    _stream(f"mis{_slot}-P3-K2-f64", "P3", "f64", "K2", [MIS if s == _slot else FULL for s in range(2)], ALL_LENS[1:], form=1, multi=MULTI_LENS)
_stream("mis0-P3-K0-f64", "P3", "f64", "K0", [MIS, FULL], SMALL_LENS[1:], form=1)
# -- shapes that collapse to rank 1
for _prec in ("f64", "f32"):
    _shaped(f"rank1-vs-row-{_prec}", "P1", _prec, "K1", [(1, 3001), (3001,), (1, 3001)], (1, 3001))
    _shaped(f"cube-{_prec}", "P3", _prec, "K1", [(3, 5, 7), (3, 5, 7)], (3, 5, 7))
    _shaped(f"trailing-ones-{_prec}", "P3", _prec, "K2", [(2049, 1, 1), (2049, 1, 1)], (2049, 1, 1))
    _shaped(f"transpose-full-{_prec}", "P3", _prec, "K1", [("transpose", (9, 33)), (33, 9)], (33, 9))
# -- broadcast: the edges of the switch between rm_ew_bcast and rm_ew_bcast_flat (d0 < 128 and outer >= 64)
for _prec in ("f64", "f32"):
    for _d0 in (127, 128):
        for _outer in (63, 64):
            _shaped(f"switch-P1-{_d0}x{_outer}-{_prec}", "P1", _prec, "K0", [(_d0, _outer), (_d0, 1), (1, _outer)], (_d0, _outer))
            _shaped(f"switch-P3-{_d0}x{_outer}-{_prec}", "P3", _prec, "K0", [(_d0, 1), (1, _outer)], (_d0, _outer))
# -- broadcast: the edges of a block's chunk of dim 0 (bcast_block * bcast_elems; f32 storage defaults to 8 elements per thread)
for _prec, _k, _per in (("f64", "K0", 1024), ("f32", "K0", 2048), ("f64", "K6", 64), ("f32", "K6", 64), ("f64", "K7", 8192), ("f32", "K7", 8192)):
    for _d0 in (_per - 1, _per, _per + 1, 2 * _per + 1):
        _shaped(f"chunk-P1-{_k}-{_d0}-{_prec}", "P1", _prec, _k, [(_d0, 3), (1, 3), (_d0, 1)], (_d0, 3))
        _shaped(f"chunk-P3-{_k}-{_d0}-{_prec}", "P3", _prec, _k, [(1, 3), (_d0, 1)], (_d0, 3))
# -- broadcast: rank 4 and rank 8 after collapsing, on both forms; views as operands; the flat form's grid-stride loop
for _prec in ("f64", "f32"):
    _shaped(f"rank4-flat-{_prec}", "P3", _prec, "K0", [(5, 1, 11, 1), (1, 7, 1, 13)], (5, 7, 11, 13))
    _shaped(f"rank4-block-{_prec}", "P3", _prec, "K0", [(130, 1, 3, 1), (1, 2, 1, 3)], (130, 2, 3, 3))
    _shaped(f"rank8-flat-{_prec}", "P1", _prec, "K0", [(2, 1, 3, 1, 2, 1, 3, 1), (1, 3, 1, 2, 1, 3, 1, 2), (1, 1)], (2, 3, 3, 2, 2, 3, 3, 2))
    _shaped(f"rank8-block-{_prec}", "P3", _prec, "K0", [(129, 1, 3, 1, 2, 1, 3, 1), (1, 3, 1, 2, 1, 3, 1, 2)], (129, 3, 3, 2, 2, 3, 3, 2))
    _shaped(f"repmat-view-{_prec}", "P1", _prec, "K0", [("repmat", (1030, 1), (1, 5)), (1030, 5), ("repmat", (1, 5), (1030, 1))], (1030, 5))
    _shaped(f"repmat-view-flat-{_prec}", "P3", _prec, "K0", [("repmat", (37, 1), (1, 70)), (1, 70)], (37, 70))
    _shaped(f"transpose-view-{_prec}", "P3", _prec, "K0", [("transpose", (5, 1030)), (1, 5)], (1030, 5))
    _shaped(f"flat-stride-{_prec}", "P3", _prec, "K0", [(127, 1), (1, 16600)], (127, 16600))
FLAT_STRIDE_ROWS = ("flat-stride-f64", "flat-stride-f32")  # 127 * 16600 elements > 256 threads * 16 blocks per CU * 256 CUs: two trips

ROW = {r["id"]: r for r in TABLE}
assert len(ROW) == len(TABLE)

# the 2-D grid of rm_ew_bcast and of the per-op k_bcast2: 128 x 1048577 gives one chunk per column, 1048577 blocks > 1048576 = gx, so
# gy = 2 and all but one block of the second row are padding that must leave (rem != 0).  A 1 GiB result; not a row of TABLE because
# its expectation is compared in slabs.
GRID2D = dict(a=(128, 1), b=(1, 1048577), out=(128, 1048577), form=2, grid=2 * 1048576)


def compile_key(row, n=None):
    """What makes a distinct kernel module: program, scalar mask, knob set, precision.  (A length-1 request reads every operand as a scalar.)"""
    if row["lens"] is None:
        mask = 0
        if len(collapsed_shape([effective_shape(o) for o in row["ops"]], row["out"])) == 1:
            mask = sum(1 << k for k, o in enumerate(row["ops"]) if int(np.prod(effective_shape(o))) == 1)
    else:
        mask = sum(1 << k for k, o in enumerate(row["ops"]) if n == 1 or o[0] in ("scalar", "mis_scalar"))
    return (row["prog"], mask, row["knobs"], row["prec"])
