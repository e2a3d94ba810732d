"""The qr kernels (runmat_amd/csrc/qr.hip) compile for gfx950 without scratch: the slice kernels keep v for their rows in registers."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_qr_kernels_use_no_scratch():
    res = _resources("qr.hip")
    qr = _pick(res, "k_qr_")
    for name in ("k_qr_pivot", "k_qr_swap", "k_qr_reflect", "k_qr_update", "k_qr_init", "k_qr_larft"):
        assert any(name in k for k in qr), name
    spilled = {k: v["scratch"] for k, v in qr.items() if v["scratch"] != 0}
    assert not spilled, spilled
