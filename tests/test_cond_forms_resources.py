"""Every kernel of runmat_amd/csrc/cond_norm.hip compiles for gfx950 without scratch: the accumulate kernel keeps its batch of loads in
registers, which only works while the loops over the batch stay unrolled."""
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import SRC, _resources  # noqa: E402


def test_cond_norm_kernels_use_no_scratch():
    res = _resources("cond_norm.hip")
    declared = set(re.findall(r"__global__ void (?:__launch_bounds__\([^)]*\) )?(k_\w+)\(", (SRC / "cond_norm.hip").read_text()))
    assert declared >= {"k_cond_fill", "k_cond_accumulate", "k_cond_fold", "k_cond_verdict", "k_cond_finish", "k_cond_scalar"}, declared
    for name in declared:
        hits = {k: r for k, r in res.items() if name in k}
        assert hits, f"{name} was not compiled"
        for kernel, r in hits.items():
            assert r["scratch"] == 0, (kernel, r)
    assert len({k for k in res if "k_cond_accumulate" in k}) == 2  # with and without the finiteness check
