"""The streaming kernels around the embedded product of `rmhip_complex_matmul` (runmat_amd/csrc/cgemm.hip) compile for gfx950 without
scratch: the split of B into its planes and the join in all three operand kinds."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_cgemm_kernels_use_no_scratch():
    res = _resources("cgemm.hip")
    split, join = _pick(res, "k_cgemm_split_b"), _pick(res, "k_cgemm_join")
    assert len(split) == 1 and len(join) == 3, (sorted(split), sorted(join))  # one join instantiation per operand kind
    for name, r in {**split, **join}.items():
        assert r["scratch"] == 0, (name, r)
    assert not [k for k in res if "k_dgemm" in k or "k_cpage_" in k]  # the siblings' resource tests select their kernels by those prefixes
