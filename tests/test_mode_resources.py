"""The kernels of mode_values (the "mode" section of runmat_amd/csrc/order_ops.hip) compile for gfx950 without scratch, and their static
LDS - a few words of hand-over between the four waves of a chunk - stays at or under 64 KiB per block."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402

KERNELS = ("k_mode_runs", "k_mode_pick", "k_mode_tie_count", "k_mode_tie_emit", "k_mode_single")


@functools.lru_cache(maxsize=None)
def _remarks() -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "order_ops.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _field(label: str) -> dict:
    pat = re.compile(rf"Function Name: (\S+).*?{re.escape(label)}: (\d+)", re.S)
    return {m.group(1): int(m.group(2)) for m in pat.finditer(_remarks())}


def test_mode_kernels_use_no_scratch():
    hits = _pick(_field("ScratchSize [bytes/lane]"), "k_mode_")
    for needle in KERNELS:
        assert _pick(hits, needle), needle
    assert len(_pick(hits, "k_mode_runs")) == 2  # a wave per line, a workgroup per chunk
    assert all(v == 0 for v in hits.values()), hits


def test_mode_kernels_stay_within_64_kib_of_lds():
    hits = _pick(_field("LDS Size [bytes/block]"), "k_mode_")
    assert hits and all(v <= 64 * 1024 for v in hits.values()), hits
