"""The path claims of tests/test_gpu_fft_paths.py against fft_plan.h, on the CPU: every case of its table names a path family and
states the launches that path makes; `fft_route_check --table` plans the case's shape, dim and length and must name the same family
and count.  So a case that stops exercising its path (a moved threshold, say) fails here, before a GPU runs it."""
import subprocess

import pytest

import test_gpu_fft_paths as paths
from test_host_plan import compile_check


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """case id -> (family, launches, the rest of the line), all cases planned in one run."""
    exe = compile_check(tmp_path_factory.mktemp("fft_route_check"), "fft_route_check")
    specs = [p.values[0] for p in paths.CASES] + [SLABS]
    text = "".join(f"{s['dim']} {-1 if s['length'] is None else s['length']} {len(s['shape'])} {' '.join(map(str, s['shape']))}\n" for s in specs)
    r = subprocess.run([str(exe), "--table"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(specs)
    return {i: (ln[0], int(ln[1]), ln[2:]) for i, ln in zip([p.id for p in paths.CASES] + ["slabs"], lines)}


# test_chirp_in_outer_slabs: its shape, and the launches it asserts
SLABS = dict(path="slabs", launches=2 * (2 * 1 + 2), shape=(8192, 2, 1030), dim=1, length=3)


@pytest.mark.parametrize("cid,spec", [(p.id, p.values[0]) for p in paths.CASES], ids=[p.id for p in paths.CASES])
def test_case_takes_the_path_it_names(planned, cid, spec):
    family, launches, _ = planned[cid]
    assert (family, launches) == (spec["path"], spec["launches"])


def test_the_slabs_case_runs_in_two_pieces(planned):
    family, launches, rest = planned["slabs"]
    assert family == "chirp" and launches == SLABS["launches"] and "slabs=2" in rest and "M=8" in rest


def test_every_family_of_the_table_is_exercised():
    assert {p.values[0]["path"] for p in paths.CASES} == {"tile0", "tile1", "two0", "two1", "three", "chirp", "chirp3"}
