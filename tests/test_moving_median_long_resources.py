"""The kernel of rmhip_moving_window_long (runmat_amd/csrc/signal_ops.hip) compiles for gfx950 without scratch - the selection keeps no
per-thread array - and with no static LDS: its keys and counters are dynamic, sized per launch by the entry point (at most 44 KiB)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_iir_long_resources import _field  # noqa: E402  (one compilation of signal_ops.hip serves both files)
from test_kernel_resources import _pick  # noqa: E402


def test_the_select_kernel_has_no_scratch_and_fits_eight_waves():
    scratch = _pick(_field("ScratchSize [bytes/lane]"), "k_movmed_long")
    assert scratch and all(v == 0 for v in scratch.values()), scratch
    spills = _pick(_field("VGPRs Spill"), "k_movmed_long")
    assert spills and all(v == 0 for v in spills.values()), spills
    vgprs = _pick(_field("VGPRs"), "k_movmed_long")
    assert all(v <= 64 for v in vgprs.values()), vgprs  # eight waves per SIMD: LDS, not registers, sets the occupancy
    lds = _pick(_field("LDS Size [bytes/block]"), "k_movmed_long")
    assert all(v == 0 for v in lds.values()), lds
