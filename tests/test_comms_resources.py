"""The kernels of the modulation hooks (runmat_amd/csrc/comms_ops.hip) compile for gfx950 without scratch, within the vector-register budget of
eight waves per SIMD (64), and with exactly the LDS they declare: the table's budget MOD_TABLE_LDS_BYTES in the LDS-table variants,
none in the global-table ones, plus - in the bit kernel - one ballot word per 64 elements of MOD_BIT_TILE and one more for the group
that straddles the tile's end.  Eight workgroups of MOD_BLOCK threads (the CU's 32 waves) then fit the CU's 160 KiB."""
import functools
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick  # noqa: E402


def _constant(name):
    m = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*(\d+)\s*;", (SRC / "modulate_check.h").read_text())
    assert m, name
    return int(m.group(1))


TABLE = _constant("MOD_TABLE_LDS_BYTES")
WORDS = (_constant("MOD_BIT_TILE") // 64 + 1) * 8
BLOCK = _constant("MOD_BLOCK")


@functools.lru_cache(maxsize=None)
def _remarks() -> str:
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "comms_ops.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _field(label: str) -> dict:
    pat = re.compile(rf"Function Name: (\S+).*?{re.escape(label)}: (\d+)", re.S)
    return {m.group(1): int(m.group(2)) for m in pat.finditer(_remarks())}


def _variants(res: dict, kernel: str, lds_table: bool) -> dict:
    """the f64- and the f32-storage instantiation of `kernel` with the given table switch (mangled template arguments: Lb1E / Lb0E)"""
    hits = _pick(res, kernel, "Lb1E" if lds_table else "Lb0E")
    assert len(hits) == 2, hits
    return hits


def test_modulation_kernels_use_no_scratch_and_at_most_64_vgprs():
    scratch = _pick(_field("ScratchSize [bytes/lane]"), "k_modulate_")
    assert len(scratch) == 8 and all(v == 0 for v in scratch.values()), scratch  # 2 kernels x 2 storage types x 2 table paths
    vgprs = _pick(_field("VGPRs"), "k_modulate_")
    assert len(vgprs) == 8 and all(v <= 64 for v in vgprs.values()), vgprs  # 512 / 64: eight waves per SIMD


def test_modulation_kernels_declare_the_lds_they_use():
    lds = _field("LDS Size [bytes/block]")
    assert all(v == TABLE for v in _variants(lds, "k_modulate_symbols", True).values()), lds
    assert all(v == 0 for v in _variants(lds, "k_modulate_symbols", False).values()), lds
    assert all(v == WORDS for v in _variants(lds, "k_modulate_bits", False).values()), lds
    for v in _variants(lds, "k_modulate_bits", True).values():
        assert TABLE + WORDS <= v <= TABLE + WORDS + 16, lds  # the table is 16-byte aligned behind the words
    # the budget's reason: eight workgroups - 32 waves of 64 lanes - resident in the CU's 160 KiB
    assert BLOCK == 256 and 8 * max(lds[k] for k in _pick(lds, "k_modulate_")) <= 160 * 1024
