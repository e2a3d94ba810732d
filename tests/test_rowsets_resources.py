"""The kernels of the 'rows' set forms (runmat_amd/csrc/order_ops.hip) compile for gfx950 without scratch - the row comparison loops over
the columns in registers, whatever their count - and the row head-flag kernel holds no more LDS than the element one it is shaped after."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402

ROW_KERNELS = ("k_row_heads", "k_rows_gather", "k_rows_stack", "k_rows_member")


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
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"Function Name: (\S+).*?{re.escape(label)}: (\d+)", _remarks(), re.S)}


def test_row_kernels_use_no_scratch():
    scratch = _field("ScratchSize [bytes/lane]")
    for needle in ROW_KERNELS:
        hits = _pick(scratch, needle)
        assert all(v == 0 for v in hits.values()), hits


def test_row_heads_holds_no_more_lds_than_group_heads():
    lds = _field("LDS Size [bytes/block]")
    element = max(_pick(lds, "k_group_heads").values())
    assert all(v <= element for v in _pick(lds, "k_row_heads").values()), (lds, element)


def test_the_reused_scan_kernels_are_still_there():
    names = _field("ScratchSize [bytes/lane]")
    for needle in ("k_chunk_offsets", "k_group_ids", "k_unique_inverse", "k_rows_keys", "k_rows_compose"):
        assert _pick(names, needle)
