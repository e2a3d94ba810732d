"""Host half of the elementwise-forms suite: pins tests/ew_forms_ref.py and what each RMHIP_EW_* knob does to the generated source.

Nothing here needs a GPU: the front-end translates and hipRTC cross-compiles for gfx950 on any machine.  The GPU half
(tests/test_gpu_ew_forms.py) runs the same table and compares bits.
"""
import numpy as np
import pytest

import ew_forms_ref as R

SHIFTS = (1, 2, 4, 64, 256, 1024, 2048)


def grid_shifts():
    """grid x block of every streaming knob set, in vectors and in elements of either precision, and a whole unrolled trip of the grid"""
    out = set()
    for k in R.STREAMING_KNOBS:
        for prec in ("f64", "f32"):
            t = R.tuning(k, prec)
            out |= {t["G"] * t["block"], t["G"] * t["block"] * t["vec"], t["G"] * t["P"]}
        out |= {256 * 16 * R.CUS}  # rm_ew_bcast_flat's stride
    return sorted(out)


def test_coded_operands_are_distinct_under_every_shift():
    """A kernel that reads or writes `shift` elements away from where it should must change the result.  Operand 0 differs from itself
    under every shift that is no multiple of its prime period; the byte-sized operands repeat every 256 elements, which is why each
    program keeps operand 0 recoverable from its results: the RESULTS differ under every shift, at every position."""
    shifts = list(SHIFTS) + grid_shifts()
    assert all(s % R.PERIOD for s in shifts)  # operand 0 at j and j + s: (s mod PERIOD) or that minus PERIOD apart, never 0
    lens = sorted({R.resolve_len(n, r["knobs"], r["prec"]) for r in R.TABLE if r["lens"] for n in r["lens"]})
    assert lens[0] == 1 and lens[-1] > 64 * 1024 * 1024
    window = 40000  # results repeat with period 256 * PERIOD; a window per shift, the arithmetic above covers the rest
    here = [R.coded((window, 1), k) for k in range(3)]
    for s in shifts:
        there = [R.coded((window, 1), k, start=s) for k in range(3)]  # the operands `s` elements on
        assert not np.any(here[0] == there[0]), s
        for prog, n_in in R.N_IN.items():
            for x, y in list(zip(R.expected(prog, here[:n_in], (window, 1)), R.expected(prog, there[:n_in], (window, 1))))[:2]:
                assert not np.any(x == y), (prog, s)  # a*256 + b - c; a*256 + b and b*256 + a
    for s in (1, 2, 4, 64):  # the byte-sized operands on their own: every shift below their period
        for k in (1, 2):
            v = R.coded((4096, 1), k)
            assert not np.any(v[:-s] == v[s:]), (k, s)
    # both operands of P3 are recoverable from its first output
    a, b = R.coded((R.PERIOD * 2, 1), 0), R.coded((R.PERIOD * 2, 1), 1)
    o = R.expected("P3", [a, b], a.shape)
    assert np.array_equal(o[0] // 256, a.reshape(-1)) and np.array_equal(o[0] % 256, b.reshape(-1))
    assert R.scalar_value(0) and R.scalar_value(1) and R.scalar_value(2)


@pytest.mark.parametrize("shapes,out", [
    ([(5, 1), (1, 7), (5, 7)], (5, 7)),
    ([(3, 5, 7), (3, 5, 7), (3, 5, 7)], (3, 5, 7)),
    ([(4, 1, 3), (1, 6, 1), (1, 1)], (4, 6, 3)),
], ids=["outer", "cube", "rank3"])
def test_expected_outputs_agree_with_oracle_chains(oracle, shapes, out):
    ops = [R.coded(s, k).astype(np.float64) for k, s in enumerate(shapes)]

    def times256(x):
        for _ in range(8):
            x = oracle.binary("add", x, x)
        return x

    a, b, c = ops
    want = {"P1": [oracle.binary("sub", oracle.binary("add", times256(a), b), c)],
            "P3": [oracle.binary("add", times256(a), b), oracle.binary("add", times256(b), a), oracle.binary("sub", a, b)]}
    for prog, n_in in R.N_IN.items():
        got = R.expected(prog, [R.coded(s, k) for k, s in enumerate(shapes[:n_in])], out)
        assert len(got) == R.N_OUT[prog]
        for g, w in zip(got, want[prog]):
            w = np.broadcast_to(w, out).reshape(-1, order="F")
            assert np.array_equal(g.view(np.uint64), np.ascontiguousarray(w).view(np.uint64)), (prog, shapes)
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g)  # exact in f32 storage too


def test_helpers_restate_the_launcher():
    assert R.collapsed_shape([(7, 9), (7, 9)], (7, 9)) == (63,)
    assert R.collapsed_shape([(7, 9), (1, 1)], (7, 9)) == (63,)
    assert R.collapsed_shape([(7, 1), (1, 9)], (7, 9)) == (7, 9)
    assert R.collapsed_shape([(3001,), (1, 3001)], (1, 3001)) == (3001,)
    assert R.collapsed_shape([(2049, 1, 1)], (2049, 1, 1)) == (2049,)
    assert R.collapsed_shape([(2, 3, 4), (2, 3, 1)], (2, 3, 4)) == (6, 4)
    assert R.collapsed_shape([(1, 1)], (1, 1)) == (1,)
    assert R.collapsed_shape([(5, 1, 11, 1), (1, 7, 1, 13)], (5, 7, 11, 13)) == (5, 7, 11, 13)
    assert [R.expected_form(10, (10,), al) for al in (True, False)] == [0, 1]
    assert [R.expected_form(d0 * o, (d0, o), True) for d0 in (127, 128) for o in (63, 64)] == [2, 3, 2, 2]
    assert R.expected_form(1 << 31, (2, 1 << 30), True) == 2
    assert R.tuning("K1", "f64") == dict(vec=2, block=64, unroll=4, G=256, P=512)
    assert R.tuning("K0", "f32") == dict(vec=4, block=1024, unroll=1, G=4096, P=4096)
    assert R.trips(512 * 256, 2, 64, 4, 256) == 1 and R.trips(512 * 256 + 2, 2, 64, 4, 256) == 2 and R.trips(1, 2, 64, 4, 1) == 0
    assert R.resolve_len((2, 1, 0, 3), "K1", "f64") == 2 * 256 * 512 + 256 + 3 and R.resolve_len(R.BIG, "K0", "f64") == 4096 * 2048 + 2048 + 1


def test_table_reaches_every_form_knob_set_and_precision():
    ids = [r["id"] for r in R.TABLE]
    assert len(set(ids)) == len(ids)
    have = {(r["form"], r["prec"]) for r in R.TABLE}
    # rm_ew_fast1 on f32 storage would need an f32 buffer off a 16-byte boundary: every f32 buffer is the library's own allocation
    # (rmhip_wrap_external adopts f64 memory only), so (1, "f32") cannot occur
    assert have == {(0, "f64"), (1, "f64"), (2, "f64"), (3, "f64"), (0, "f32"), (2, "f32"), (3, "f32")}
    assert {r["knobs"] for r in R.TABLE} == set(R.KNOBS)
    for k in R.STREAMING_KNOBS:  # a second trip under every streaming knob set; under the two small ones for both fast forms
        multi = [r for r in R.TABLE if r["knobs"] == k and r["multi"]]
        assert multi and all(set(r["multi"]) <= set(r["lens"]) for r in multi), k
        for r in multi:
            t = R.tuning(k, r["prec"])
            for n in r["multi"]:
                n = R.resolve_len(n, k, r["prec"])
                assert R.trips(n, 1 if r["form"] == 1 else t["vec"], t["block"], t["unroll"], t["G"]) >= 2, (r["id"], n)
    assert {r["form"] for r in R.TABLE if r["knobs"] in ("K1", "K2") and r["multi"]} == {0, 1}
    for r in R.TABLE:
        assert len(r["ops"]) == R.N_IN[r["prog"]]
        if r["lens"] is None:  # the form of a shaped row is what the restated decision gives
            n = int(np.prod(r["out"], dtype=np.int64))
            col = R.collapsed_shape([R.effective_shape(o) for o in r["ops"]], r["out"])
            assert r["form"] == R.expected_form(n, col, True, R.KNOBS[r["knobs"]]), r["id"]
            assert n <= 1 << 22
        else:
            mis = any(o[0] == "mis" for o in r["ops"])
            assert r["form"] == (1 if mis else 0) and not (mis and 1 in r["lens"]), r["id"]
    # the switch and the chunk edges are both sides of their thresholds
    assert {ROW["form"] for i, ROW in R.ROW.items() if i.startswith("switch-")} == {2, 3}
    keys = {R.compile_key(r, R.resolve_len(n, r["knobs"], r["prec"])) for r in R.TABLE for n in (r["lens"] or [None])}
    assert len(keys) <= 48, len(keys)  # distinct kernel modules the GPU file compiles (about a third of a second each)


def kernel_text(src, name):
    i = src.index(" " + name + "(")
    j = src.find('extern "C"', i)
    return src[i:j if j >= 0 else len(src)]


@pytest.mark.parametrize("knobs", list(R.KNOBS))
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_knob_sets_translate_compile_and_change_the_source(built, monkeypatch, knobs, ty):
    from runmat_amd import wgsl_compile_check, wgsl_translate

    k = R.KNOBS[knobs]
    for prog in ("P1", "P3"):
        sh = R.shader(prog, ty)
        R.set_knobs(monkeypatch, "K0")
        base = wgsl_translate(sh)
        R.set_knobs(monkeypatch, knobs)
        src = wgsl_translate(sh)
        wgsl_compile_check(sh)  # hipRTC, --offload-arch=gfx950
        assert (src == base) == (knobs == "K0")
        fast, fast1, bcast = (kernel_text(src, n) for n in ("rm_ew_fast", "rm_ew_fast1", "rm_ew_bcast"))
        t = R.tuning(knobs, ty)
        for body in (fast, fast1):
            assert f"__launch_bounds__({t['block']}) rm_ew_fast(" in src and f"__launch_bounds__({t['block']}) rm_ew_fast1(" in src
            u = t["unroll"]
            header = f"for (; i + {u - 1} * stride < nvec; i += {u} * stride) {{"
            assert (header in body) == (u > 1)  # the unrolled main loop ...
            assert body.count("for (; i < nvec; i += stride) {") == 1  # ... is always followed by the remainder loop
            assert body.count("rm_body(") == (t["vec"] if body is fast else 1) * (u + 1 if u > 1 else 1) + (1 if body is fast else 0)
            chunked = bool(k.get("CHUNKED"))
            assert ("rm_u64 chunk = (nvec_all + gridDim.x - 1) / gridDim.x;" in body) == chunked
            assert (f"const rm_u64 per_iter = {t['block'] * u}ull;" in body) == chunked
            assert ("const rm_u64 begin = (rm_u64)blockIdx.x * chunk;" in body) == chunked
            assert (f"const rm_u64 stride = (rm_u64)gridDim.x * {t['block']};" in body) == (not chunked)
            assert ("__builtin_nontemporal" in body) == (k.get("NT", 1) == 1)
        bb, be = (k.get("BCAST_BLOCK", 256) // 64) * 64, k.get("BCAST_ELEMS", 4)
        assert f"__launch_bounds__({bb}) rm_ew_bcast(" in src and f"const rm_u64 i0 = chunk * {bb * be}ull + threadIdx.x;" in bcast
        assert bcast.count("if (i < d0) {") == be and f"const rm_u64 i = i0 + {(be - 1) * bb}ull;" in bcast
        assert "if (rem != 0) return;" in bcast
    # the grid cap is a launch parameter: it leaves the source alone
    R.set_knobs(monkeypatch, "K0")
    monkeypatch.setenv("RMHIP_EW_BLOCKS_PER_CU", "1")
    assert wgsl_translate(sh) == base
