"""The streaming kernels around the embedded solve of `rmhip_complex_mldivide` / `_mrdivide` / `_inv` (runmat_amd/csrc/csolve.hip) compile
for gfx950 without scratch and at full occupancy: the embed, the four forms of the stack and the two forms of the join."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_csolve_kernels_use_no_scratch_and_few_registers():
    res = _resources("csolve.hip")
    embed, stack, join = _pick(res, "k_csolve_embed"), _pick(res, "k_csolve_stack"), _pick(res, "k_csolve_join")
    assert len(embed) == 1 and len(stack) == 4 and len(join) == 2, (sorted(embed), sorted(stack), sorted(join))
    for name, r in {**embed, **stack, **join}.items():
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 64 and r["occupancy"] == 8, (name, r)  # 64 registers: eight waves per SIMD
    assert len(res) == 7  # nothing else lives in the file: the solve runs in the kernels of lu.hip, small_solve.hip and svdsolve.hip
