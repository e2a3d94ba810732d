"""The kernels of uniform_spectral_estimate (runmat_amd/csrc/fft.hip) compile for gfx950 without scratch: the frame and finish kernels
hold no LDS, and the tile kernel's window-loading instantiation stays in the register class of the transforms' own."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402


@functools.lru_cache(maxsize=None)
def _remarks() -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "fft.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def test_spectral_kernels_use_no_scratch():
    pat = re.compile(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", re.S)
    res = {m.group(1): {"regs": int(m.group(2)) + int(m.group(3)), "scratch": int(m.group(4)), "occupancy": int(m.group(5))} for m in pat.finditer(_remarks())}
    for needle in ("k_spectral_frame", "k_spectral_finish", "k_fft_tile"):
        for name, r in _pick(res, needle).items():
            assert r["scratch"] == 0, (name, r)
    plain, win = _pick(res, "k_fft_tile", "ELb0E"), _pick(res, "k_fft_tile", "ELb1E")
    assert len(plain) == 3 and len(win) == 3
    # __launch_bounds__(NT, 4): the window load may not cost the tile kernel an occupancy step against the transforms' instantiation
    for name, r in win.items():
        twin = plain[name.replace("ELb1E", "ELb0E")]
        assert r["occupancy"] >= twin["occupancy"] and r["regs"] <= max(128, twin["regs"]), (name, r, twin)


def test_frame_and_finish_kernels_hold_no_lds():
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", _remarks(), re.S)}
    for needle in ("k_spectral_frame", "k_spectral_finish"):
        hits = {k: v for k, v in lds.items() if needle in k}
        assert hits, needle
        assert all(v == 0 for v in hits.values()), hits
