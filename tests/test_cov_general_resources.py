"""Register / scratch budget of the weighted tall-skinny Gram kernel (special.hip k_gram_skinny_w), checked at compile time as
tests/test_kernel_resources.py checks k_gram_skinny: an 8 x 8 block of products and two rows of both operand sides per thread, no spills,
two workgroups per CU.  The weighted column-sums pass and the centring pass stream and must not touch scratch either."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402


def test_weighted_gram_kernels_keep_their_register_budgets():
    res = _resources("special.hip")
    hits = _pick(res, "15k_gram_skinny_wI")
    assert len(hits) == 2, sorted(hits)  # f64 and f32 storage
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 256 and r["occupancy"] >= 2, (name, r)
    for key in ("k_cov_wsums", "k_cov_centre", "k_cov_finish"):
        for name, r in _pick(res, key).items():
            assert r["scratch"] == 0, (name, r)
