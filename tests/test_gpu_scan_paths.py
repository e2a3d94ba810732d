"""Every launch form of the cumulative scans against exact prefix sums and products, and of cummin / cummax against the oracle.

`rmhip_cumulative` (cumsum_scan, cumprod_scan) takes one of five kernels, the staged one with 32 or 64 lines per block, the staged and
the contiguous one with one chunk per line (one launch) or several (three launches: chunk totals, carries, the scan from the carries) -
reduce_plan.h route_scan.  The shape table of tests/scan_ref.py reaches each of them, with up to 256 chunks per line and with more (the
carry kernel's second trip), with a ragged last chunk, with idle lanes in a 32-line block and with contiguous lines spilling into grid
z; tests/cpp/scan_route_check.cpp pins that on the host for 256 CUs, and every test here counts the launches.  The data classes,
placements and bounds are scan_ref.py's: `exact` (any association order gives the same bits: compared for bit equality, signed zeros
included, a NaN matching any NaN) and `rounded` (bounds that hold for any order).  Each rounded test prints its largest error as a
fraction of the bound (`ratio ...` lines, pytest -s).  `rmhip_cumextreme` (route_cumextreme) must give the oracle's values and indices
bit for bit.

The ratios an MI355X printed when this module was written, sum / prod per row (the bounds are derived, not fitted to these):
  lines_64x32  2x9x1 0.0000 / 0.2659   7x5000x1 0.1359 / 0.4177   40x255x3 0.3294 / 0.5670
  lines_256x8  262144x3x1 0.3330 / 0.6315   512x2x512 0.0000 / 0.4971
  staged, one chunk   8x256x1 0.2417 / 0.4746   40x300x1 0.3145 / 0.4919   33x4095x2 0.2642 / 0.4918
                      64x256x256 0.4893 / 0.6025   16384x256x1 0.4893 / 0.6025   (64 lines per block)
  staged, chunked     9x4096x1 0.0836 / 0.4130   40x9001x1 0.3190 / 0.5062   17x9001x3 0.2169 / 0.5211   32x8192x2 0.1569 / 0.4776
                      8x300000x1 0.1733 / 0.3816
  short        1x1x5 0.0000 / 0.0000   1x3x1025 0.3284 / 0.5617   1x16x300 0.3294 / 0.5313   1x255x17 0.3271 / 0.4539
  chunks       1x256x3 0.0690 / 0.3496   1x16384x2 0.0262 / 0.3355   1x16385x2 0.0352 / 0.1771   1x70001x3 0.0348 / 0.3011
               1x4300000x1 0.0074 / 0.2125
"""
import numpy as np
import pytest

import scan_ref as S

pytestmark = pytest.mark.gpu

GPU_ROWS = [r for r in S.SCAN_ROUTE_TABLE if r != S.Z_SPILL_ROW]
F32_ROWS = [r for r in GPU_ROWS if S.numel(r) < S.F32_LIMIT]
ROUNDED_ROWS = [r for r in GPU_ROWS if S.numel(r) <= S.ROUNDED_LIMIT]


@pytest.fixture(scope="module")
def prov32(built):
    import os
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


@pytest.fixture(scope="module", autouse=True)
def pinned_cu_count(prov):
    """the tables hold on the CU count they were pinned for; on another device the routes differ and nothing here applies"""
    cus = int(prov.device_info_struct()["compute_units"])
    if cus != S.NUM_CUS:
        pytest.skip(f"the scan route tables are pinned for {S.NUM_CUS} CUs, this device reports {cus}")


def narrow(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def launches(p) -> int:
    return int(p.telemetry_snapshot()["kernel_launches"])


def scan(p, h, row, prod, reverse, omit, count=True):
    """the scan's output as lines in memory order; on the f64 provider the launch count must be the route's"""
    pre, n, post = row[:3]
    dim = max(S.realise(pre, n, post)[1], 0)
    before = launches(p) if count else 0
    out = (p.cumprod_scan if prod else p.cumsum_scan)(h, dim, reverse, omit)
    if count:
        assert launches(p) - before == row[6], (row, prod, reverse, omit, "launches", launches(p) - before)
    got = p.download(out)
    p.free(out)
    return S.slices(got, pre, n, post)


def upload(p, mem_lines, row):
    pre, n, post = row[:3]
    return p.upload(S.unslice(mem_lines, pre, n, post), S.realise(pre, n, post)[0])


def run_exact(p, row, prod, reverse, f32, single_nans=True, only=None):
    rng = np.random.default_rng(S.numel(row) + (31 if prod else 17))
    base = S.exact_lines(rng, row, prod)
    for name, modes, specials in S.variants(row, prod, single_nans):
        if only is not None and name not in only:
            continue
        lines = S.apply_specials(base, specials)
        h = upload(p, S.to_memory(lines, reverse), row)
        has_nan = any(v != v for _, _, v in specials)
        want = None
        for mode in modes:
            omit = mode == "omit"
            if want is None or has_nan:  # without a NaN in the input both modes have one reference
                want = S.to_memory(S.seq_scan(lines, prod, omit), reverse)
                want = narrow(want) if f32 else want
            got = scan(p, h, row, prod, reverse, omit, count=not f32)
            assert S.same_bits(got, want), (row, "prod" if prod else "sum", name, "reverse" if reverse else "forward", mode, S.where_differs(got, want))
        p.free(h)


# ---- the exact class: sums and products, both directions, both NaN modes, every placement; bit equality and launch counts -----------
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("prod", [False, True], ids=["sum", "prod"])
@pytest.mark.parametrize("row", GPU_ROWS, ids=S.row_id)
def test_exact_class_bits(prov, row, prod, reverse):
    run_exact(prov, row, prod, reverse, False)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("prod", [False, True], ids=["sum", "prod"])
@pytest.mark.parametrize("row", F32_ROWS, ids=S.row_id)
def test_exact_class_precision32(prov32, row, prod, reverse):
    """f32 storage: the inputs and every prefix of the exact classes are f32 numbers, so the result is the f64 scan narrowed once"""
    run_exact(prov32, row, prod, reverse, True)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_lines_spilling_into_grid_z(prov, reverse):
    """65537 contiguous lines of 256: line 65535 is the first of grid z = 1.  16.8 M elements, so sums only: clean, one NaN per line
    at every placement (the lines either side of the spill among them) and all of them together"""
    run_exact(prov, S.Z_SPILL_ROW, False, reverse, False, only=("clean", "one_nan0", "many_nan"))


# ---- the rounded class: within bounds that hold for any association order; the CPU's own bits where the form is its sequence --------
@pytest.mark.parametrize("prod", [False, True], ids=["sum", "prod"])
@pytest.mark.parametrize("row", ROUNDED_ROWS, ids=S.row_id)
def test_rounded_class_bounds(prov, oracle, row, prod):
    pre, n, post = row[:3]
    shape, dim = S.realise(pre, n, post)
    rng = np.random.default_rng(S.numel(row) + (43 if prod else 29))
    lines = (S.rounded_prod_lines if prod else S.rounded_sum_lines)(rng, pre * post, n)
    bounds = S.scan_bounds(lines, prod)
    worst = 0.0
    for reverse in (False, True):
        mem = S.to_memory(lines, reverse)
        h = upload(prov, mem, row)
        for omit in (False, True):  # no NaN here: both modes compute the same
            got = scan(prov, h, row, prod, reverse, omit)
            ok, ratio = S.scan_error_ratios(S.to_memory(got, reverse), lines, prod, bounds)
            worst = max(worst, ratio)
            assert ok, (row, "prod" if prod else "sum", reverse, omit, ratio)
            if S.is_cpu_sequence(row):
                x = S.unslice(mem, pre, n, post).reshape(shape, order="F")
                want = S.slices(oracle.cumulative(x, max(dim, 0), prod=prod, reverse=reverse, omitnan=omit), pre, n, post)
                assert S.same_bits(got, want), (row, "prod" if prod else "sum", reverse, omit, "not the CPU's bits", S.where_differs(got, want))
        prov.free(h)
    print(f"ratio {'prod' if prod else 'sum'} {S.row_id(row)} {worst:.4f}")


# ---- cummin / cummax: values and indices are the oracle's, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("row", S.CUMEXT_ROUTE_TABLE, ids=S.row_id)
def test_cumextreme_paths(prov, oracle, row):
    pre, n, post, _, nchunks, _ = row
    shape, dim = S.realise(pre, n, post)
    dim = max(dim, 0)
    rng = np.random.default_rng(S.numel(row) + 59)
    for name, mem in S.cumext_cases(rng, row):
        x = S.unslice(mem, pre, n, post).reshape(shape, order="F")
        h = upload(prov, mem, row)
        for is_max in (False, True):
            for reverse in (False, True):
                for omit in (False, True):
                    before = launches(prov)
                    r = (prov.cummax_scan if is_max else prov.cummin_scan)(h, dim, reverse, omit)
                    assert launches(prov) - before == (3 if nchunks > 1 else 1), (row, name, "launches")
                    gv, gi = prov.download(r.values), prov.download(r.indices)
                    prov.free(r.values)
                    prov.free(r.indices)
                    wv, wi = oracle.cumextreme(x, dim, is_max, reverse, omit)
                    what = (row, name, "max" if is_max else "min", "reverse" if reverse else "forward", "omit" if omit else "include")
                    assert S.same_bits(gv, wv.reshape(-1, order="F")), (what, "values", S.where_differs(gv, wv.reshape(-1, order="F")))
                    assert S.same_bits(gi, wi.reshape(-1, order="F")), (what, "indices", S.where_differs(gi, wi.reshape(-1, order="F")))
        prov.free(h)
