"""The complex pagefun kernels (runmat_amd/csrc/complex_pagefun.hip) compile for gfx950 without scratch in all three operand kinds, and
the matrix-core kernel, which keeps two accumulator sets (re and im of a 32 x 32 wave tile), stays within 256 VGPR + AGPR."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_complex_pagefun_kernels_use_no_scratch_and_fit_their_registers():
    res = _resources("complex_pagefun.hip")
    small, mfma = _pick(res, "k_cpage_small"), _pick(res, "k_cpage_mfma")
    assert len(small) == 3 and len(mfma) == 3, (sorted(small), sorted(mfma))  # one instantiation per operand kind
    for name, r in {**small, **mfma}.items():
        assert r["scratch"] == 0, (name, r)
    for name, r in mfma.items():
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
    assert not [k for k in res if "k_pagefun_" in k]  # the real sibling's resource test selects its kernels by that prefix
