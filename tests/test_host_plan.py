"""Host logic that needs no GPU, checked by small C++ programs over sweeps of shapes: the reduction launch geometry and the
routing of a shape to its kernel and finalize (reduce_plan.h), the broadcast stride preparation / dimension collapsing of the elementwise entry points
(host_shape.h), including the in-place addressing of lazy repmat views, the GEMM dispatch (gemm_plan.h), the LU dispatch (lu_plan.h) and the
transforms' dispatch and pass addressing (fft_plan.h)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def compile_check(out_dir, name):
    """tests/cpp/<name>.cpp against the library's headers, with a plain host compiler and every warning an error."""
    exe = Path(out_dir) / name
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'runmat_amd' / 'csrc'}",
                        str(ROOT / "tests" / "cpp" / f"{name}.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    return exe


@pytest.mark.parametrize("name,needle", [("reduce_plan_check", "reduce plan ok"), ("reduce_route_check", "reduce route ok"),
                                         ("broadcast_prep_check", "broadcast prep ok"),
                                         ("repmat_view_check", "repmat view ok")])
def test_host_logic(tmp_path, name, needle):
    exe = compile_check(tmp_path, name)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and needle in r.stdout, r.stdout + r.stderr


def test_gemm_plan_routes_the_sweep_as_the_launchers_ladders_did(tmp_path):
    """plan_dgemm / plan_sgemm over the fixed sweep of gemm_route_check.cpp (shapes, layouts, operations, every site of the look-ahead
    LU, three device sizes, each knob off): per group, the case count and the digest of the routes equal what the launchers' former
    if-ladders gave (tests/golden/gemm_routes.txt, recorded from them).  `gemm_route_check --dump` prints the routes themselves."""
    exe = compile_check(tmp_path, "gemm_route_check")
    r = subprocess.run([str(exe), "--sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [ln for ln in (ROOT / "tests" / "golden" / "gemm_routes.txt").read_text().splitlines() if ln and not ln.startswith("#")]
    got = r.stdout.splitlines()
    assert len(want) == 108 and len({ln.rsplit(" ", 2)[0] for ln in want}) == 108  # 2 precisions x (13 sites + 5 knobs) x 3 device sizes
    assert all(int(ln.split()[-2]) == 11 * 11 * 13 * 9 * (7 if ln.startswith("f64") else 3) for ln in want)
    differing = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not differing, differing[:5]


def test_lu_plan_routes_the_sweep_as_the_drivers_conditions_did(tmp_path):
    """lu_plan.h over the fixed sweep of lu_route_check.cpp (factor routes around every threshold under each knob, base panels, triangular
    solves, the step lists of the one-level and the two-level driver, substitution, padding; three device sizes): per group, the case
    count and the digest of the routes equal what the drivers' former conditions gave (tests/golden/lu_routes.txt, recorded from them).
    `lu_route_check --dump` prints the routes themselves."""
    exe = compile_check(tmp_path, "lu_route_check")
    r = subprocess.run([str(exe), "--sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [ln for ln in (ROOT / "tests" / "golden" / "lu_routes.txt").read_text().splitlines() if ln and not ln.startswith("#")]
    got = r.stdout.splitlines()
    # 16 settings x 3 device sizes; 3 panel families x one-XCD on / off x 3; 3; fast on / off x one-XCD on / off x 3; 6 plans; 3; padding
    groups = {"factor": 48, "panel": 18, "trsm": 3, "blocked": 12, "super": 6, "subst": 3, "pad": 1}
    assert len(want) == sum(groups.values()) == 91 and len({ln.rsplit(" ", 2)[0] for ln in want}) == 91
    assert {k: sum(ln.split()[0] == k for ln in want) for k in groups} == groups
    assert all(int(ln.split()[-2]) > 0 for ln in want)
    differing = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not differing, differing[:5]


@pytest.fixture(scope="module")
def fft_route_check(tmp_path_factory):
    return compile_check(tmp_path_factory.mktemp("fft_route_check"), "fft_route_check")


def test_fft_plan_routes_the_sweep_as_the_drivers_conditions_did(fft_route_check):
    """fft_plan.h over the fixed sweep of fft_route_check.cpp (every power-of-two length lg 0..28 at five inners, two outers, four input
    lengths; tiles at every line-count boundary; the entry's routes; Bluestein's sizes around every boundary of M, both refusals, the
    slab and work-tensor limits; the length predicate; the spectral decision): per group, the case count and the digest of the routes
    equal what the drivers' former conditions gave (tests/golden/fft_routes.txt, recorded from them).  `fft_route_check --dump` prints
    the routes themselves."""
    r = subprocess.run([str(fft_route_check), "--sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [ln for ln in (ROOT / "tests" / "golden" / "fft_routes.txt").read_text().splitlines() if ln and not ln.startswith("#")]
    got = r.stdout.splitlines()
    # 5 inners x 2 outers; 3 modes; 1; 4 outers; 1; 3 frame modes x 3 ranges
    groups = {"pow2": 10, "tile": 3, "entry": 1, "chirp": 4, "served": 1, "spectral": 9}
    assert len(want) == sum(groups.values()) == 28 and len({ln.rsplit(" ", 2)[0] for ln in want}) == 28
    assert {k: sum(ln.split()[0] == k for ln in want) for k in groups} == groups
    assert all(int(ln.split()[-2]) > 0 for ln in want)
    differing = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not differing, differing[:5]


def test_fft_tiles_fit_the_kernel(fft_route_check):
    """Every tile of that sweep: at most 8 points per thread, at most 160 KiB of LDS, enough workgroups for the lines, radices that
    multiply to the line length with the twiddle-free one first."""
    r = subprocess.run([str(fft_route_check), "--invariants"], capture_output=True, text=True)
    assert r.returncode == 0 and "fft tile invariants ok" in r.stdout, r.stdout + r.stderr


def test_fft_pass_addressing_is_the_transform(fft_route_check):
    """The exact model: every pass of the one-, two- and three-pass routes, the one-point pass and the fused spectral frames, run on
    the host on impulses held as exponents of w_n, gives the transform's definition exponent for exponent, writes every element once,
    reads only what the pass before wrote and stays inside its buffers (fft_route_check.cpp states the cases)."""
    r = subprocess.run([str(fft_route_check), "--model"], capture_output=True, text=True)
    assert r.returncode == 0 and "fft model ok" in r.stdout, r.stdout + r.stderr
