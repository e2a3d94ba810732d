"""Every form of the generated elementwise kernels, and of the per-op streaming and broadcast kernels, on coded operands.

The rows of tests/ew_forms_ref.py run here on the f64 provider and on a precision-32 provider, under the RMHIP_EW_* knob sets the table
names.  Operands are exact integers that encode each element's own position and the programs keep them recoverable, so every
assertion on values is bit equality against numpy integer arithmetic.  After each fused call the launch record must name the form the
table expects (0 rm_ew_fast, 1 rm_ew_fast1, 2 rm_ew_bcast, 3 rm_ew_bcast_flat), the grid the launcher's rule gives, and - where the row
says so - a grid that leaves every thread at least two trips through its loop.  The per-op hooks record no form: values only.
"""
import contextlib

import numpy as np
import pytest

import ew_forms_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prov32(built):
    import os
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


@pytest.fixture(scope="module")
def cus(prov):
    return int(prov.device_info_struct()["compute_units"])


@pytest.fixture
def pick(prov, request):
    """precision name -> provider"""
    return lambda prec: prov if prec == "f64" else request.getfixturevalue("prov32")


SHADERS = {(prog, ty): R.shader(prog, ty) for prog in ("P1", "P3") for ty in ("f64", "f32")}


def last_record(p):
    log = [e for e in p.telemetry_snapshot()["kernel_launches_log"] if e["kernel"].startswith("fused_elementwise")]
    return log[-1]


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def first_differences(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return [(int(k), float(got[k]), float(want[k])) for k in bad[:5]], len(bad)


def up(p, values, shape):
    return p.upload(np.asarray(values, dtype=np.float64).reshape(-1, order="F"), shape)


@contextlib.contextmanager
def operands(p, row, n=None):
    """The row's inputs on the device: (handles, values as the program sees them, [(handle that owns storage, its values)]).  Everything
    is freed on the way out, views before what they view."""
    handles, values, owners, frees = [], [], [], []
    try:
        for k, spec in enumerate(row["ops"]):
            kind = spec[0]
            v = R.operand_values(spec, k, n)
            if kind in ("mis", "mis_scalar"):  # 8 bytes into an allocation one element longer: never on a 16-byte boundary
                whole = R.coded((n + 1, 1), k) if kind == "mis" else R.coded((2, 1), k, R.SCALAR_START)
                owner = up(p, whole, whole.shape)
                frees.append(owner)
                p.synchronize()
                ptr = p.device_ptr(owner)
                assert ptr % 16 == 0
                h = p.wrap_external(ptr + 8, v.shape)
                owners.append((owner, whole))
            elif kind == "repmat":
                base = up(p, R.coded(spec[1], k), spec[1])
                frees.append(base)
                h = p.repmat(base, list(spec[2]))
                owners.append((base, R.coded(spec[1], k)))
            elif kind == "transpose":
                base = up(p, R.coded(spec[1], k), spec[1])
                frees.append(base)
                h = p.transpose(base)
            else:
                h = up(p, v, v.shape if kind != "shape" else spec[1])
                owners.append((h, v))
            frees.append(h)
            assert tuple(h.shape) == tuple(v.shape) or kind == "shape"
            handles.append(h)
            values.append(v)
        yield handles, values, owners
    finally:
        for h in reversed(frees):
            p.free(h)


def launch(p, row, handles, out_shape):
    """One fused call of the row's program -> (flat results, the launch record)."""
    n = int(np.prod(out_shape, dtype=np.int64))
    outs = p.fused_elementwise_multi(SHADERS[(row["prog"], p.scalar_ty())], handles, out_shape, n, R.N_OUT[row["prog"]])
    rec = last_record(p)
    try:
        assert rec["kernel"] == ("fused_elementwise" if len(outs) == 1 else "fused_elementwise_multi") and rec["shape"]["len"] == n
        assert all(p.buffer_bits(h) == (32 if p.scalar_ty() == "f32" else 64) for h in outs)
        return [p.download(h) for h in outs], rec
    finally:
        for h in outs:
            p.free(h)


def check_values(row, got, values, out_shape, what):
    want = R.expected(row["prog"], values, out_shape)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), (row["id"], what, f"output {k}", first_differences(g, w))


def stream_grid(n, form, t):
    """The launcher's grid for a streaming request of n elements (rmhip_ops.cpp)."""
    work = n if form == 1 else n // t["vec"]
    return min(max(-(-work // (t["block"] * t["unroll"])), 1), t["G"])


def bcast_grid(row, n, prec, cus):
    col = R.collapsed_shape([R.effective_shape(o) for o in row["ops"]], row["out"])
    if row["form"] == 3:
        return min(-(-n // 256), cus * 16)
    k = R.KNOBS[row["knobs"]]
    per = (k.get("BCAST_BLOCK", 256) // 64) * 64 * k.get("BCAST_ELEMS", 8 if prec == "f32" else 4)
    return -(-col[0] // per) * int(np.prod(col[1:], dtype=np.int64))


# ---- the streaming forms: every length of the row, the form, the grid, the trips ----------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in R.TABLE if r["lens"]], ids=lambda r: r["id"])
def test_streaming_rows(pick, cus, monkeypatch, row):
    p = pick(row["prec"])
    R.set_knobs(monkeypatch, row["knobs"])
    t = R.tuning(row["knobs"], row["prec"], cus)
    multi = [R.resolve_len(s, row["knobs"], row["prec"], cus) for s in row["multi"]]
    for spec in row["lens"]:
        n = R.resolve_len(spec, row["knobs"], row["prec"], cus)
        with operands(p, row, n) as (handles, values, _):
            got, rec = launch(p, row, handles, (n, 1))
        check_values(row, got, values, (n, 1), f"n = {n}")
        form = row["form"] if n > 1 else 0  # (a 1-element request reads every operand as a scalar)
        tun = rec["tuning"]
        assert tun["form"] == form and tun["wg"] == t["block"] and tun["unroll"] == t["unroll"], (row["id"], n, tun)
        assert tun["grid"] == stream_grid(n, form, t), (row["id"], n, tun)
        if n in multi:
            assert R.trips(n, 1 if form == 1 else t["vec"], t["block"], t["unroll"], tun["grid"]) >= 2, (row["id"], n, tun)


# ---- shapes that collapse to rank 1, and the broadcast forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in R.TABLE if r["lens"] is None], ids=lambda r: r["id"])
def test_shaped_rows(pick, cus, monkeypatch, row):
    p = pick(row["prec"])
    R.set_knobs(monkeypatch, row["knobs"])
    out = row["out"]
    n = int(np.prod(out, dtype=np.int64))
    with operands(p, row) as (handles, values, _):
        got, rec = launch(p, row, handles, out)
    check_values(row, got, values, out, "")
    tun = rec["tuning"]
    assert tun["form"] == row["form"], (row["id"], tun)
    if row["form"] >= 2:
        assert tun["grid"] == bcast_grid(row, n, row["prec"], cus), (row["id"], tun)
    else:
        assert tun["grid"] == stream_grid(n, 0, R.tuning(row["knobs"], row["prec"], cus)), (row["id"], tun)
    if row["id"] in R.FLAT_STRIDE_ROWS:
        assert tun["grid"] * 256 * 2 <= n  # every thread of rm_ew_bcast_flat walks its grid-stride loop at least twice


def test_blocks_per_cu_is_read_for_a_program_already_cached(prov, cus, monkeypatch):
    """The grid cap does not change the generated source; a kernel cached under one value must not serve a launch under another."""
    row = dict(R.ROW["stream-P3-K0-f64"])
    n = 3 * cus * 2048 + 6
    with operands(prov, row, n) as (handles, values, _):
        R.set_knobs(monkeypatch, "K0")
        got, rec = launch(prov, row, handles, (n, 1))
        assert rec["tuning"]["grid"] == 3 * cus + 1
        check_values(row, got, values, (n, 1), "default cap")
        monkeypatch.setenv("RMHIP_EW_BLOCKS_PER_CU", "1")
        got, rec = launch(prov, row, handles, (n, 1))
        assert rec["tuning"]["grid"] == cus and rec["tuning"]["form"] == 0
        check_values(row, got, values, (n, 1), "one block per CU")
        monkeypatch.setenv("RMHIP_EW_BLOCKS_PER_CU", "2")
        got, rec = launch(prov, row, handles, (n, 1))
        assert rec["tuning"]["grid"] == 2 * cus
        check_values(row, got, values, (n, 1), "two blocks per CU")


# ---- determinism: one multi-trip (multi-block) row per form ------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id,spec", [("stream-P1-K1-f64", (2, 1, 0, 3)), ("mis1-P1-K1-f64", (2, 1, 0, 3)), ("chunk-P1-K0-2049-f64", None),
                                         ("flat-stride-f64", None)], ids=["fast", "fast1", "bcast", "bcast_flat"])
def test_two_calls_give_the_same_bits_and_leave_the_inputs_alone(prov, cus, monkeypatch, row_id, spec):
    row = R.ROW[row_id]
    R.set_knobs(monkeypatch, row["knobs"])
    n = R.resolve_len(spec, row["knobs"], row["prec"], cus)
    out = row["out"] or (n, 1)
    with operands(prov, row, n) as (handles, values, owners):
        first, rec1 = launch(prov, row, handles, out)
        second, rec2 = launch(prov, row, handles, out)
        assert rec1["tuning"] == rec2["tuning"] and rec1["tuning"]["form"] == row["form"]
        for a, b in zip(first, second):
            assert same_bits(a, b)
        check_values(row, first, values, out, "first call")
        for h, v in owners:
            assert same_bits(prov.download(h), v.reshape(-1, order="F")), row_id


# ---- the per-op hooks on memory that is not 16-byte aligned: k_plain1 / k_plain2 ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 1025, 70001])
def test_per_op_hooks_on_a_misaligned_operand(prov, n):
    row = dict(ops=[R.MIS, R.FULL])
    with operands(prov, row, n) as ((hm, hf), (vm, vf), owners):
        vm, vf = vm.reshape(-1), vf.reshape(-1)
        cases = [(prov.unary_abs(hm), vm), (prov.unary_floor(hm), vm), (prov.scalar_mul(hm, 256.0), vm * 256),
                 (prov.scalar_rsub(hm, 7.0), 7 - vm), (prov.elem_add(hm, hf), vm + vf), (prov.elem_add(hf, hm), vf + vm),
                 (prov.elem_sub(hf, hm), vf - vm), (prov.elem_sub(hm, hm), vm - vm)]
        for k, (h, want) in enumerate(cases):
            got = prov.download(h)
            prov.free(h)
            assert same_bits(got, want + 0.0), (n, k, first_differences(got, want))
        for h, v in owners:
            assert same_bits(prov.download(h), v.reshape(-1, order="F"))


# ---- the per-op hooks' 16-byte kernels on f32 storage: the tail of one to three elements ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 4096, 4097, 4098, 4099, 70001, 70002, 70003])
def test_per_op_hooks_f32_tails(prov32, n):
    row = dict(ops=[R.FULL, R.FULL])
    with operands(prov32, row, n) as ((ha, hb), (va, vb), _):
        va, vb = va.reshape(-1), vb.reshape(-1)
        cases = [(prov32.unary_abs(ha), va), (prov32.scalar_mul(ha, 256.0), va * 256), (prov32.scalar_rsub(hb, 7.0), 7 - vb),
                 (prov32.elem_add(ha, hb), va + vb), (prov32.elem_sub(hb, ha), vb - va)]
        for k, (h, want) in enumerate(cases):
            assert prov32.buffer_bits(h) == 32
            got = prov32.download(h)
            prov32.free(h)
            assert same_bits(got, want + 0.0), (n, k, first_differences(got, want))


# ---- the per-op broadcast kernels at the same edges: k_bcast2 / k_bcast2_flat ------------------------------------------------------------------
def bcast_pairs(prec):
    per = 2048 if prec == "f32" else 1024  # kBlock * BcastE<T> (ew_kernels.hip)
    pairs = [((d0, 1), (1, outer)) for d0 in (127, 128) for outer in (63, 64)]
    pairs += [((d0, outer), (1, outer)) for d0 in (127, 128) for outer in (63, 64)]
    pairs += [((1, 3), (d0, 1)) for d0 in (per - 1, per, per + 1, 2 * per + 1)]
    pairs += [((5, 1, 11, 1), (1, 7, 1, 13)), ((130, 1, 3, 1), (1, 2, 1, 3)), ((127, 1), (1, 16600))]
    return pairs


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_per_op_broadcast_edges(pick, prec):
    p = pick(prec)
    for sa, sb in bcast_pairs(prec):
        va, vb = R.coded(sa, 0), R.coded(sb, 1)
        ha, hb = up(p, va, sa), up(p, vb, sb)
        h = p.elem_sub(ha, hb)
        want = va - vb
        assert tuple(h.shape) == want.shape
        got = p.download(h)
        for x in (h, ha, hb):
            p.free(x)
        assert same_bits(got, want.reshape(-1, order="F") + 0.0), (prec, sa, sb, first_differences(got, want.reshape(-1, order="F")))


# ---- the 2-D grid: more than 1048576 blocks, the second row of the grid nearly all padding ---------------------------------------------------
def check_grid2d(got, f, va, vb):
    """got: the flat 128 x 1048577 result; f(a column, b values of a slab of columns) -> the slab's expectation, compared slab by slab."""
    rows, cols = R.GRID2D["out"]
    got = got.reshape(cols, rows)  # column-major: one row of this view per column of the result
    a = va.reshape(1, rows)
    for c0 in range(0, cols, 1 << 16):
        b = vb.reshape(-1)[c0:c0 + (1 << 16)].reshape(-1, 1)
        want = f(a, b).astype(np.float64)
        g = got[c0:c0 + (1 << 16)]
        assert np.array_equal(g.view(np.uint64), want.view(np.uint64)), (c0, first_differences(g.reshape(-1), want.reshape(-1)))


def test_broadcast_2d_grid_fused(prov, monkeypatch):
    R.set_knobs(monkeypatch, "K0")
    g = R.GRID2D
    row = dict(id="grid2d", prog="P1", ops=[("shape", g["a"]), ("shape", g["b"]), R.SCALAR])
    with operands(prov, row) as (handles, values, _):
        got, rec = launch(prov, row, handles, g["out"])
    assert rec["tuning"]["form"] == g["form"] and rec["tuning"]["grid"] == g["grid"], rec
    c = int(values[2][0, 0])
    check_grid2d(got[0], lambda a, b: a * 256 + b - c, values[0], values[1])


def test_broadcast_2d_grid_per_op(prov):
    g = R.GRID2D
    va, vb = R.coded(g["a"], 0), R.coded(g["b"], 1)
    ha, hb = up(prov, va, g["a"]), up(prov, vb, g["b"])
    h = prov.elem_add(ha, hb)
    assert tuple(h.shape) == g["out"]
    got = prov.download(h)
    for x in (h, ha, hb):
        prov.free(x)
    check_grid2d(got, lambda a, b: a + b, va, vb)
