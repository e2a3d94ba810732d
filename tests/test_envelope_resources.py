"""The kernels of signal_envelope (runmat_amd/csrc/signal_ops.hip) compile for gfx950 without scratch; the streaming ones hold no more LDS
than a block reduction needs, and the two tiled ones stay at or under 64 KiB per block - their static share from the compiler's remarks
plus the dynamic share the host code caps (ENV_LDS_BYTES)."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402

BLOCK = 256
REDUCTION_LDS = (BLOCK // 64) * (8 + 4)  # one double and one flag per wave


@functools.lru_cache(maxsize=None)
def _remarks() -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "signal_ops.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _lds() -> dict:
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", _remarks(), re.S)}


def test_envelope_kernels_use_no_scratch():
    pat = re.compile(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", re.S)
    scratch = {m.group(1): int(m.group(2)) for m in pat.finditer(_remarks())}
    hits = _pick(scratch, "k_env_")
    for needle in ("k_env_stats", "k_env_center", "k_env_bounds", "k_env_fir", "k_env_rms"):
        assert _pick(hits, needle)
    assert all(v == 0 for v in hits.values()), hits


def test_streaming_kernels_hold_a_block_reductions_lds_at_most():
    for needle in ("k_env_stats", "k_env_center", "k_env_bounds"):
        hits = _pick(_lds(), needle)
        assert all(v <= REDUCTION_LDS for v in hits.values()), hits


def test_tiled_kernels_stay_within_64_kib():
    cap = re.search(r"constexpr size_t ENV_LDS_BYTES = (\d+)u \* 1024;", (SRC / "signal_ops.hip").read_text())
    assert cap, "ENV_LDS_BYTES not found"
    dynamic = int(cap.group(1)) * 1024
    for needle in ("k_env_fir", "k_env_rms"):
        hits = _pick(_lds(), needle)
        assert all(v + dynamic <= 64 * 1024 for v in hits.values()), (hits, dynamic)
