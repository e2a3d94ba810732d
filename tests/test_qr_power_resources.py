"""The CholeskyQR2 kernels (runmat_amd/csrc/cholqr.hip) compile for gfx950 without scratch: k_cq_apply keeps a whole row of up to 64
columns in registers, which only works while every index into it is a compile-time constant."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_cholqr_kernels_use_no_scratch():
    res = _resources("cholqr.hip")
    cq = _pick(res, "k_cq_")
    for name in ("k_cq_gram", "k_cq_sum", "k_cq_factor", "k_cq_apply"):
        assert any(name in k for k in cq), name
    # every column padding of the two templated kernels, and k_cq_apply with and without the Gram part
    for kp in (8, 16, 32, 64):
        assert _pick(cq, f"k_cq_gramILi{kp}E")
        assert _pick(cq, f"k_cq_applyILi{kp}ELb0E") and _pick(cq, f"k_cq_applyILi{kp}ELb1E")
    spilled = {k: v["scratch"] for k, v in cq.items() if v["scratch"] != 0}
    assert not spilled, spilled
