"""The pagefun kernels (runmat_amd/csrc/pagefun.hip, and the paged GEMM tile k_pgemm_w8 in dgemm.hip) compile for gfx950 without
scratch: page offsets are computed from the kernel argument with constant indices, and the paged tile keeps its accumulators in
registers at two waves per SIMD."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_pagefun_kernels_use_no_scratch():
    res = _resources("pagefun.hip")
    pf = _pick(res, "k_pagefun_")
    for name in ("k_pagefun_tiny", "k_pagefun_mfma"):
        assert any(name in k for k in pf), name
    spilled = {k: v["scratch"] for k, v in pf.items() if v["scratch"] != 0}
    assert not spilled, spilled


def test_paged_gemm_tile_uses_no_scratch():
    res = _resources("dgemm.hip")
    for name, r in _pick(res, "k_pgemm_w8").items():
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 256, (name, r)
