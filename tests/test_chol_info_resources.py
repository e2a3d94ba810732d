"""The kernels rmhip_chol_info adds (runmat_amd/csrc/chol.hip) compile for gfx950 without scratch: the lower form of the extraction keeps
its 16 loads of a tile in registers, which only works while the loop over them is unrolled.  The leaf kernel is the one rmhip_chol
launches - a single instantiation, no scratch either (a row of 64 doubles per lane, every index a compile-time constant)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_chol_extraction_kernels_use_no_scratch():
    res = _resources("chol.hip")
    for name in ("k_chol_extract_upper", "k_chol_extract_lower", "k_chol_tiny_root"):
        for kernel, r in _pick(res, name).items():
            assert r["scratch"] == 0, (kernel, r)
    leaves = _pick(res, "k_potf2")
    assert len(leaves) == 1 and all(r["scratch"] == 0 for r in leaves.values()), leaves
