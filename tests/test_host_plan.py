"""Host logic that needs no GPU, checked by small C++ programs over sweeps of shapes: the reduction launch geometry and the
routing of a shape to its kernel and finalize (reduce_plan.h), the broadcast stride preparation / dimension collapsing of the elementwise entry points
(host_shape.h), including the in-place addressing of lazy repmat views, the GEMM dispatch (gemm_plan.h) and the LU dispatch (lu_plan.h)."""
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
