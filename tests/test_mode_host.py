"""mode_values without a GPU: the Python restatement of mode.rs (tests/mode_ref.py) reproduces the reference's own unit tests
(tests/golden/mode_kats.json) and agrees with an independent brute force, and the host-side pieces of the run scan
(runmat_amd/csrc/mode_runs.h: geometry, candidate order, the closing search) pass their C++ sweep."""
import json
import subprocess
import zlib
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import mode_ref

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "mode_kats.json").read_text())["cases"]


def _arr(values):
    return np.array([np.nan if v is None else v for v in values], dtype=np.float64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(mode_ref.bits(a), mode_ref.bits(b))


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_restatement_reproduces_the_reference_kats(kat):
    x = _arr(kat["data"]).reshape(kat["shape"], order="F")
    M, F, ties = mode_ref.mode(x, kat["axes"])
    want = _arr(kat["M"]).reshape(kat["M_shape"], order="F")
    assert M.shape == tuple(kat["M_shape"]) and F.shape == M.shape
    assert np.array_equal(np.isnan(M), np.isnan(want)) and np.array_equal(M[~np.isnan(M)], want[~np.isnan(want)])
    assert np.array_equal(mode_ref.bits(M)[np.isnan(M)], np.full(int(np.isnan(M).sum()), mode_ref.NAN_BITS, dtype=np.uint64))
    if "F" in kat:
        assert np.array_equal(F.reshape(-1, order="F"), _arr(kat["F"]))
    if "C" in kat:
        assert len(ties) == len(kat["C"]) and all(np.array_equal(t, _arr(c)) for t, c in zip(ties, kat["C"]))


def brute(values):
    """Independent of mode_ref.scalar_mode: a Counter over (is zero, bits) keys and a linear look for first occurrences."""
    nums = [v for v in values if not np.isnan(v)]
    if not nums:
        return None, 0, []
    tally = Counter("zero" if v == 0 else float(v).hex() for v in nums)
    top = max(tally.values())
    first = {}
    for v in nums:
        first.setdefault("zero" if v == 0 else float(v).hex(), v)
    tied = sorted((first[k] for k, c in tally.items() if c == top), key=lambda v: (v,))
    return tied[0], top, tied


POOL = np.array([0.0, -0.0, 1.0, -1.0, 2.5, np.inf, -np.inf, np.nan, 3.0, 5e-324, -5e-324])


@pytest.mark.parametrize("seed", range(8))
def test_restatement_agrees_with_a_brute_force(seed):
    rng = np.random.default_rng(zlib.crc32(f"mode-host-{seed}".encode()))
    for _ in range(40):  # 8 x 40 cases
        rows, cols = int(rng.integers(0, 7)), int(rng.integers(0, 5))
        x = rng.choice(POOL[: int(rng.integers(2, POOL.size + 1))], size=(rows, cols))
        for axes in ("default", "all", 0, 1, 2):
            M, F, ties = mode_ref.mode(x, axes)
            shape = mode_ref.matrix_shape(x.shape)
            dim = mode_ref.default_dim(shape) if axes == "default" else axes
            if axes == "all":
                slices, oshape = [x.reshape(-1, order="F")], (1, 1)
            elif dim >= 2:
                slices, oshape = [np.array([v]) for v in x.reshape(-1, order="F")], shape
            elif dim == 0:
                slices, oshape = [x[:, j] for j in range(cols)], (1, cols)
            else:
                slices, oshape = [x[i, :] for i in range(rows)], (rows, 1)
            assert M.shape == oshape and F.shape == oshape and len(ties) == len(slices)
            for k, s in enumerate(slices):
                m, f, tied = brute(list(s))
                got_m, got_f = M.reshape(-1, order="F")[k], F.reshape(-1, order="F")[k]
                assert got_f == f
                if m is None:
                    assert mode_ref.bits(got_m) == mode_ref.NAN_BITS and ties[k].size == 0
                else:
                    assert _same(np.float64(got_m), np.float64(m)) and _same(ties[k], np.array(tied, dtype=np.float64))


def test_ragged_form():
    values, offsets, counts = mode_ref.ragged([np.array([1.0, 2.0]), np.empty(0), np.array([5.0])])
    assert values.shape == (3, 1) and offsets == [0, 2, 2] and counts == [2, 0, 1]
    assert mode_ref.ragged([])[0].shape == (0, 1)


def test_run_scan_host_pieces(tmp_path):
    exe = tmp_path / "mode_runs_check"
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'runmat_amd' / 'csrc'}",
                        str(ROOT / "tests" / "cpp" / "mode_runs_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "mode runs ok" in r.stdout, r.stdout + r.stderr


def test_provider_exposes_mode_values():
    import runmat_amd

    assert callable(getattr(runmat_amd.HipProvider, "mode_values", None))
    assert runmat_amd.ModeResult and runmat_amd.ModeTiedSets
    from runmat_amd import _lib
    assert "rmhip_mode_values" in _lib.SIGNATURES
