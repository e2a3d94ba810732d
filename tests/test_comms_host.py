"""The modulation hooks without a GPU: the Python restatement of the CPU loops (tests/comms_ref.py) reproduces the reference's own unit
tests (tests/golden/modulation_kats.json) and stops at the first failing element with the CPU's message; the host-side pieces of the
kernels (runmat_amd/csrc/modulate_check.h: the per-element verdicts, the error key, the cut of a symbol out of ballot words) pass their
C++ sweep - plain and under AddressSanitizer + UBSan, as a program of their own - and judge every edge value as the restatement does."""
import functools
import json
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import comms_ref as ref

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "modulation_kats.json").read_text())
KATS = GOLDEN["cases"]


def run_kat(kat):
    if kat["hook"] == "modulate_constellation":
        return ref.modulate_constellation(kat["data"], kat["shape"], kat["constellation"])
    return ref.modulate_bits_constellation(kat["data"], kat["shape"], kat["input_rows"], kat["bits_per_symbol"], kat["constellation"])


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_restatement_reproduces_the_reference_kats(kat):
    got, second = run_kat(kat)
    if "error" in kat:
        assert got == kat["error"] and second == kat["index"]
        return
    assert tuple(second) == tuple(kat["expected_shape"]) and got.size == 2 * int(np.prod(kat["expected_shape"]))
    assert np.all(np.abs(got - np.array(kat["expected"], dtype=np.float64)) < GOLDEN["tolerance"])
    # every output pair is a copy of a table pair
    pairs = {(a, b) for a, b in ref.bits(kat["constellation"]).reshape(-1, 2).tolist()}
    assert all((a, b) in pairs for a, b in ref.bits(got).reshape(-1, 2).tolist())


def test_restatement_stops_at_the_first_failing_element():
    table = [float(v) for v in range(8)]  # order 4
    assert ref.modulate_constellation([0, 0.5, float("nan")], [3, 1], table) == (ref.SYMBOL_MESSAGES[1], 1)
    assert ref.modulate_constellation([0, float("nan"), 0.5], [3, 1], table) == (ref.SYMBOL_MESSAGES[0], 1)
    assert ref.modulate_constellation([4, float("nan")], [2, 1], table) == (ref.SYMBOL_MESSAGES[2], 0)
    assert ref.modulate_constellation([1e300], [1, 1], table) == (ref.SYMBOL_MESSAGES[2], 0)
    out, shape = ref.modulate_constellation([-0.0, -1e-10, 2.0000000004], [1, 3], table)
    assert shape == (1, 3) and out.tolist() == [0, 1, 0, 1, 4, 5]
    out, shape = ref.modulate_constellation([], [0, 3], table)
    assert shape == (0, 3) and out.size == 0
    # bits, order 3 under two bits per symbol: group 1 = (1, 1) is out of range at its last bit, before the non-bit of group 2
    short = table[:6]
    assert ref.modulate_bits_constellation([0, 1, 1, 1, 2, 0], [6, 1], 6, 2, short) == (ref.BIT_MESSAGES[2], 3)
    assert ref.modulate_bits_constellation([0, 1, 2, 0, 1, 1], [6, 1], 6, 2, short) == (ref.BIT_MESSAGES[1], 2)
    assert ref.modulate_bits_constellation([0, 1, 1, float("inf")], [4, 1], 4, 2, short) == (ref.BIT_MESSAGES[0], 3)
    out, shape = ref.modulate_bits_constellation([0, 1, 1, 0, -1e-10, 0], [6, 1], 6, 2, short)
    assert shape == (3, 1) and out.tolist() == [2, 3, 4, 5, 0, 1]
    # the host-side refusals in the CPU's order
    assert ref.modulate_bits_constellation([0], [1, 1], 0, 0, [1.0])[0].endswith(ref.TABLE_MESSAGE)
    assert ref.modulate_bits_constellation([0], [1, 1], 0, 2, short)[0] == ref.GROUPING_MESSAGE
    assert ref.modulate_bits_constellation([0] * 3, [3, 1], 3, 2, short)[0] == ref.MULTIPLE_MESSAGE
    assert ref.modulate_bits_constellation([0] * 4, [2, 2], 4, 2, short)[0] == ref.ROWS_MESSAGE
    out, shape = ref.modulate_bits_constellation([], [4, 0], 4, 2, short)
    assert shape == (2, 0) and out.size == 0


CXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'runmat_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "modulate_check_test.cpp")]


@functools.lru_cache(maxsize=None)
def _program(tmp, sanitized):
    exe = Path(tmp) / ("modulate_check_san" if sanitized else "modulate_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    c = subprocess.run(CXX + flags + ["-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    return str(exe)


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("modulate_check"))


def _hex(v):
    return struct.pack(">d", v).hex()


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_host_pieces_self_check(build_dir, sanitized):
    r = subprocess.run([_program(build_dir, sanitized)], capture_output=True, text=True)
    assert r.returncode == 0 and "modulate check ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("order", [2, 8, 64])
def test_symbol_verdicts_match_the_restatement(build_dir, sanitized, order):
    values = ref.symbol_edges(order)
    r = subprocess.run([_program(build_dir, sanitized), "symbols", str(order)] + [_hex(v) for v in values], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(values)
    table = [float(k) for k in range(2 * order)]  # pair s is (2 s, 2 s + 1): the result names the symbol
    for v, line in zip(values, lines):
        got, second = ref.modulate_constellation([v], [1, 1], table)
        want = f"0 {int(got[0]) // 2}" if second == (1, 1) else f"{ref.SYMBOL_MESSAGES.index(got) + 1} -"
        assert line == want, (v, _hex(v), line, want)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_bit_verdicts_match_the_restatement(build_dir, sanitized):
    values = ref.bit_edges()
    r = subprocess.run([_program(build_dir, sanitized), "bits"] + [_hex(v) for v in values], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(values)
    table = [0.0, 1.0, 2.0, 3.0]  # one bit per symbol
    for v, line in zip(values, lines):
        got, second = ref.modulate_bits_constellation([v], [1, 1], 1, 1, table)
        want = f"0 {int(got[0]) // 2}" if second == (1, 1) else f"{ref.BIT_MESSAGES.index(got) + 1} -"
        assert line == want, (v, _hex(v), line, want)


def test_edge_lists_hold_what_they_promise():
    e = ref.symbol_edges(8)
    got = [ref.modulate_constellation([v], [1, 1], [float(k) for k in range(16)]) for v in e]
    verdict = {_hex(v): (g if s != (1, 1) else int(g[0]) // 2) for v, (g, s) in zip(e, got)}
    assert verdict[_hex(-0.0)] == 0 and verdict[_hex(-1e-10)] == 0 and verdict[_hex(2.0000000004)] == 2
    assert verdict[_hex(0.5)] == ref.SYMBOL_MESSAGES[1] and verdict[_hex(-1.0)] == ref.SYMBOL_MESSAGES[1]
    assert verdict[_hex(1e300)] == ref.SYMBOL_MESSAGES[2] and verdict[_hex(2.0 ** 53)] == ref.SYMBOL_MESSAGES[2] and verdict[_hex(8.0)] == ref.SYMBOL_MESSAGES[2]
    assert verdict[_hex(7 + 1e-10)] == 7 and verdict[_hex(float("inf"))] == ref.SYMBOL_MESSAGES[0]
    # the tolerance's edge is really straddled: around each k +- 1e-9 some neighbours pass and some fail
    for k in (1.0, 7.0):
        for centre in (k - 1e-9, k + 1e-9):
            kinds = {isinstance(verdict[_hex(v)], int) for v in ref._around(centre)}
            assert kinds == {True, False}, (k, centre)


def test_provider_exposes_the_modulation_hooks():
    import runmat_amd
    from runmat_amd import _lib

    assert callable(getattr(runmat_amd.HipProvider, "modulate_constellation", None))
    assert callable(getattr(runmat_amd.HipProvider, "modulate_bits_constellation", None))
    assert _lib.SERVES["rmhip_modulate_constellation"] == ("modulate_constellation",)
    assert _lib.SERVES["rmhip_modulate_bits_constellation"] == ("modulate_bits_constellation",)
