"""The kernels of rmhip_iir_filter_long (runmat_amd/csrc/signal_ops.hip) compile for gfx950 without scratch for filters of order <= 8 (the
instantiations that keep states, coefficients and a row of T in registers), and none of them holds more than 64 KiB of LDS per block -
all of it static, so the compiler's resource remarks are the whole account."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402

KERNELS = ("k_fir_long", "k_fir_long_state", "k_iir_chunks", "k_iir_states", "k_iir_correct")
SMALL_ORDER = ("k_iir_chunksILi8E", "k_iir_statesILi7E", "k_iir_correctILi7E")  # order <= 8: MAXO = 8, S <= 7


@functools.lru_cache(maxsize=None)
def _remarks() -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "signal_ops.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _field(label: str) -> dict:
    pat = re.compile(r"Function Name: (\S+).*?" + re.escape(label) + r": (\d+)", re.S)
    return {m.group(1): int(m.group(2)) for m in pat.finditer(_remarks())}


def test_every_kernel_of_the_long_form_is_compiled():
    names = _field("ScratchSize [bytes/lane]")
    for needle in KERNELS + SMALL_ORDER + ("k_iir_chunksILi64E", "k_iir_statesILi63E", "k_iir_correctILi63E"):
        assert _pick(names, needle)


def test_no_scratch_up_to_order_8():
    scratch = _field("ScratchSize [bytes/lane]")
    for needle in SMALL_ORDER + ("k_fir_long",):
        hits = _pick(scratch, needle)
        assert all(v == 0 for v in hits.values()), hits


def test_lds_stays_within_64_kib_per_block():
    lds = _field("LDS Size [bytes/block]")
    for needle in KERNELS:
        hits = _pick(lds, needle)
        assert all(v <= 64 * 1024 for v in hits.values()), hits
    assert all(v > 0 for v in _pick(lds, "k_iir_correct").values())  # the H tile is staged
    assert all(v > 0 for v in _pick(lds, "10k_fir_longE").values())   # and so is the FIR window
