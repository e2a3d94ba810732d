"""Bit-identity of the transforms across a refactor of fft.hip's host side: the SHA-256 digests of the downloaded results of a fixed
case list (fft_bits_cases.py: the smallest shape per route, hash-made inputs) equal those recorded on an MI355X from the revision that
tests/golden/fft_bits.json names (scripts/record_fft_bits.py).  No path of the transforms uses atomics, so unchanged kernels with
unchanged launch parameters give unchanged bits; a digest that differs is a finding about the change, not a reason to re-record."""
import json
import os
from pathlib import Path

import pytest

import fft_bits_cases

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "fft_bits.json").read_text())


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider
    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def test_golden_covers_the_case_list():
    assert sorted(GOLDEN["digests"]) == sorted(cid for cid, _, _ in fft_bits_cases.CASES) and GOLDEN["recorded_from"] and GOLDEN["date"]


@pytest.mark.parametrize("cid,precision,run", fft_bits_cases.CASES, ids=[c[0] for c in fft_bits_cases.CASES])
def test_bits(prov, prov32, cid, precision, run):
    assert run(prov32 if precision == "F32" else prov) == GOLDEN["digests"][cid]
