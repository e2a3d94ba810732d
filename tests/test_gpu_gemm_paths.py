"""Every GEMM kernel variant reachable from the C ABI against exact integer products, with the route attested.

Each case of tests/gemm_ref.py runs once: the launcher's record (`gemm_last_route()`: kernel, template flags, splits, k_chunk) must be
the table's row, and the result must equal the int64 product of the nonzero-integer operands BIT FOR BIT - for `blk_gemm` the whole C
buffer, whose frame around the view must come back untouched while NaN surrounds the A and B views (and fills the C view where
beta == 0).  blk_gemm is the only entry that takes views: the routes reached through whole buffers (A' / B' views, syrk, epilogue,
pagefun, all of f32) are checked for exact values and storage width, not for reads or writes beside their buffers.  Only the EP_POW epilogue rounds; it is compared with oracle.matmul_epilogue at test_matmul_epilogue_vs_oracle's bound.
Cases of the matmul, blk_gemm and epilogue entries run a second time as the product of the transposes (rows and columns exchanged,
same route): an m / n mix-up cannot hide behind a square shape.

The table is written for 256 compute units; on another device every test here FAILS with a message (the thresholds are
blocks * 4 <= num_cus for split-K, blocks * 2 <= num_cus for the 64 x 64 tiles).

route                     selected by                                                                  shapes (m, n, k)
small                     matmul / blk_gemm; <= 128 tiles of 128 x 128 and k <= 1024, or skinny          (64,64,16) (192,128,1008) (2048,1024,16) (64,16512,16)
small pre                 blk_gemm(-1, A, B, 1, C)                                                      (64,64,16) (128,192,32)
small guard (+- pre)      the same, ragged, or an A / B view on an odd offset / odd leading dimension   (1,1,1) (65,63,17) (63,130,33) (64,64,16)
w8                        matmul / blk_gemm on whole tiles past the small boundary                      (2048,1152,16) (1664,640,1040)
w8 pre                    blk_gemm(-1, .., 1, ..)                                                       (2048,1152,16)
w8 split                  <= 64 tiles and k >= 1024; blk_gemm(2, .., -1, ..) reduces with beta          (128,128,1024) 8 x 128, (128,128,1040) 9 x 128, (256,128,2048) 8 x 256
w8 ta (+- split)          matmul of a transpose view of A; syrk                                         (128,128,16) (256,128,48) (128,128,2048); syrk of 2048 x 128
w8 epi1 / epi2            matmul_epilogue without / with pow_exponent                                   (128,128,16) (256,128,48)
w8g (+- pre)              ragged past the small boundary, or a misaligned view of whole tiles           (2049,1153,17) (2048,1152,16)
w8g split                 ragged, <= 64 tiles, k >= 1024                                                (100,100,1100) 9 x 128, (129,127,2050) 9 x 256
w8g ta (+- split)         ragged A' view; syrk                                                          (65,63,17) (2,300,5) (100,100,1100)
w8g epi1 / epi2           ragged matmul_epilogue                                                        (65,63,17) (130,129,31)
w4 tb, w4 edge tb         matmul of a transpose view of B (+- split)                                    (128,128,16) (256,128,48) (65,63,17) (128,128,2048) (128,128,1040) (100,100,1100)
pgemm                     pagefun(@mtimes), pages of at least 256 x 256 and no shared operand (tier 4)  3 pages of (258,257,17)
w4, w4 pre, w4 ta         RMHIP_GEMM_W8=0 (child process), whole tiles, +- split                        (2048,1152,16) (1664,640,1040) (128,128,16) (128,128,2048) ...
w4 edge (plain, ta, epi)  RMHIP_GEMM_GUARD=0 (child process), ragged shapes and misaligned views         (2049,1153,17) (65,63,17) (2,300,5) (100,100,1100) ...
w8 / w8g on small shapes  RMHIP_GEMM_SMALL=0 (child process)                                            (128,128,16) (64,64,16) (65,63,17) ...
non-pre on the updates    RMHIP_GEMM_PRELOAD=0 (child process): same bits as the preloaded forms        (64,64,16) (65,63,17) (2048,1152,16) (2049,1153,17)
s_w8, s_w8g (+- ta)       precision-32 provider: matmul, A' view, syrk; whole / ragged tiles            (128,128,16) (256,128,48) (65,63,17) (130,129,31) ...
s_w4 tb (whole / edge)    precision-32 provider: B' view                                                (128,128,16) (65,63,17) ...
s_w4 split                precision-32 provider, <= 64 tiles and k >= 1024: plain, ta, tb; ragged         (128,128,1024) (128,128,1040) (100,100,1100) (129,127,2050) ...
                          slices or shapes are the default-on home of k_sgemm<true, ...>
s_w4 (+- ta, edge)        RMHIP_SGEMM_W8=0 (child process)                                              (128,128,16) (65,63,17)

(Two shapes that look natural for a row are not in it, because the code routes them elsewhere: pages of 130 x 65 are served by
pagefun's 64 x 64 matrix-core tier - k_pgemm_w8 takes pages from 256 x 256 - and the transpose of a vector is the same memory, not a
view, so (1,300,5) cannot arrive as A'; (2,300,5) is the smallest that does, and (1,300,5) runs as a plain skinny product.)

Out of reach from the ABI, selected only inside the look-ahead LU and covered by the LU suites (test_gpu_lookahead.py,
test_gpu_lu_r05.py, test_gpu_lu_stress.py): k_dgemm_w8p, the YIELD instantiation of k_dgemm_w8, and the upd_small rule that sends the
update streams' few-tile products to the 64 x 64 tiles.  There is no back door for them here.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def require_256(cus):
    assert cus == G.NUM_CUS, (f"the route table of tests/gemm_ref.py is written for {G.NUM_CUS} compute units; this device has {cus}: "
                              "the split-K and small-tile thresholds move with the count, so the expected routes do not apply")


def run_both(prov, c, bits, oracle):
    require_256(int(prov.device_info_struct()["compute_units"]))
    first = G.run_case(prov, c, bits, False, oracle)
    G.check(first)
    if G.has_swap(c):
        G.check(G.run_case(prov, c, bits, True, oracle))
    return first


def test_route_is_empty_before_the_first_product(built):
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")))
    try:
        r = p.gemm_last_route()
        assert r["kernel"] == "" and r["splits"] == 0 and r["k_chunk"] == 0
        G.check(G.run_case(p, G.F64_CASES[0]))
        assert p.gemm_last_route()["kernel"] == "small"
    finally:
        p.close()


@pytest.mark.parametrize("c", G.F64_CASES, ids=lambda c: c["id"])
def test_f64_route_and_exact_product(prov, oracle, c):
    run_both(prov, c, 64, oracle)


@pytest.mark.parametrize("c", G.F32_CASES, ids=lambda c: c["id"])
def test_f32_route_and_exact_product(prov32, oracle, c):
    run_both(prov32, c, 32, oracle)


def child(table, knob, bits):
    """One fresh process with `knob`=0 (the knobs are process-static): gemm_ref.child_main runs the knob's table."""
    code = (f"import sys; sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'tests')!r}]; import gemm_ref; "
            f"gemm_ref.child_main({table!r}, {knob!r}, {bits})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{knob: "0"}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    require_256(out["compute_units"])
    assert out["error"] is None, (out["error"], [x["id"] for x in out["results"]])
    cases = {"f64": G.KNOB_CASES, "f32": G.F32_KNOB_CASES}[table][knob]
    assert len(out["results"]) == sum(2 if G.has_swap(c) else 1 for c in cases)
    for res in out["results"]:
        G.check(res)
    return {res["id"]: res for res in out["results"]}


@pytest.mark.parametrize("knob", ["RMHIP_GEMM_W8", "RMHIP_GEMM_GUARD", "RMHIP_GEMM_SMALL"])
def test_f64_knob_selected_variants(built, knob):
    child("f64", knob, 64)


def test_updates_without_preload_give_the_same_bits(prov, oracle):
    res = child("f64", "RMHIP_GEMM_PRELOAD", 64)
    for c in G.KNOB_CASES["RMHIP_GEMM_PRELOAD"]:
        assert res[c["id"]]["route"]["pre"] == 0
        here = G.run_case(prov, c, 64, False, oracle)  # this process: the preloaded form of the same update
        assert here["route"]["pre"] == 1 and here["route"]["kernel"] == res[c["id"]]["route"]["kernel"], here
        assert here["equal"] and here["digest"] == res[c["id"]]["digest"], c["id"]


def test_f32_knob_selected_variants(built):
    child("f32", "RMHIP_SGEMM_W8", 32)
