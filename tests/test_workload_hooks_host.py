"""CPU checks of the three workload hooks (black_scholes_price, adam_update, crossentropy_terms; runmat_amd/csrc/workload_ops.hip):
the ABI tags and the host mirrors, the Python mirror's request layout against provider_broadcast_index, the numpy restatement the GPU
tests compare with against exact values, and the compiled kernels' resources."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import _pick, _resources  # noqa: E402
from workload_hooks_ref import (EPS, adam_ref, black_scholes_bound, black_scholes_ref, broadcast_index,  # noqa: E402
                                crossentropy_ref)

KATS = json.loads((ROOT / "tests" / "golden" / "workload_hooks_kats.json").read_text())
HOOKS = ("black_scholes_price", "adam_update", "crossentropy_terms")
INPUT_KEYS = ("price", "strike", "rate", "time", "volatility", "yield")


# ---- the ABI and its mirrors ----------------------------------------------------------------------------------------------------
def test_entry_points_are_tagged_and_bound():
    from runmat_amd import _lib

    for name in HOOKS:
        assert _lib.SERVES.get(f"rmhip_{name}") == (name,), name
        assert f"rmhip_{name}" in _lib.SIGNATURES


def test_every_mirror_has_the_three_methods():
    from runmat_amd import HipProvider

    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index("impl AccelProvider for HipProvider"):]
    for name in HOOKS:
        assert callable(getattr(HipProvider, name, None)), name
        assert re.search(rf"\b{name}\s*\(", hpp) and f"rmhip_{name}(ctx_" in hpp, name
        assert re.search(rf"\bfn {name}\b", body) and f"rmhip_{name}(self.ctx" in body, name


def test_library_exports_the_entry_points(built):
    from runmat_amd import _lib

    lib = _lib.load()
    for name in HOOKS:
        assert getattr(lib, f"rmhip_{name}") is not None


# ---- request layout -------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [
    [(), (), (), (), (), ()],
    [(7, 9)] * 6,
    [(4, 1), (1, 5), (), (1, 1), (1,), ()],
    [(3, 1, 4), (1, 5, 1), (), (), (), ()],
    [(5,), (1, 5), (5, 1), (), (), ()],
    [(2, 1, 3, 1, 2, 1, 2, 1), (1, 2, 1, 1, 1, 2, 1, 2), (), (), (), ()],
    [(0, 3), (1, 3), (), (), (), ()],
    [(4, 5), (5,), (), (), (), ()],  # refused: a rank-1 shape is a column, [5, 1] against [4, 5]
]


@pytest.mark.parametrize("shapes", LAYOUT_CASES[:-1], ids=lambda s: "x".join(str(len(t)) for t in s) + "_" + str(s[0]))
def test_request_layout_reproduces_provider_broadcast_index(shapes):
    """The Python mirror aligns shapes and computes strides as blsprice does; provider_broadcast_index over that layout must read what
    numpy's broadcasting (trailing dimensions aligned, the same rule) reads."""
    from runmat_amd import HipProvider

    out_shape, aligned, strides = HipProvider.black_scholes_request_layout(shapes)
    canon = [(1, 1) if len(s) == 0 else (s[0], 1) if len(s) == 1 else tuple(s) for s in shapes]
    assert out_shape == tuple(np.broadcast_shapes(*canon)) or 0 in out_shape
    n = int(np.prod(out_shape))
    for s, a, st in zip(canon, aligned, strides):
        assert len(a) == len(st) == len(out_shape) and tuple(e for e in a[len(a) - len(s):]) == s and all(e == 1 for e in a[:len(a) - len(s)])
        step = 1
        for e, x in zip(a, st):  # compute_strides (broadcast.rs:49-57)
            assert x == step
            step *= max(e, 1)
        if n == 0:
            continue
        data = np.arange(int(np.prod(s)), dtype=np.float64) + 0.5
        want = np.broadcast_to(data.reshape(s, order="F"), out_shape).ravel(order="F")
        got = np.array([data[broadcast_index(i, out_shape, a, st)] for i in range(n)])
        assert np.array_equal(got, want)


def test_request_layout_refuses_shapes_that_do_not_broadcast():
    from runmat_amd import HipProvider, ProviderError

    with pytest.raises(ProviderError, match="size mismatch between inputs"):
        HipProvider.black_scholes_request_layout(LAYOUT_CASES[-1])


# ---- the restatement against exact values ---------------------------------------------------------------------------------------
def _exact_sets():
    bs = KATS["black_scholes"]
    return {"random": bs["random"], "wgpu_kat": bs["wgpu_kat"]["exact"], "textbook": bs["textbook"]["exact"]}


@pytest.mark.parametrize("name", ["random", "wgpu_kat", "textbook"])
def test_black_scholes_restatement_is_within_the_bound_of_exact_values(name):
    case = _exact_sets()[name]
    a = [np.array(case[k]) for k in INPUT_KEYS]
    call, put = black_scholes_ref(*a)
    bound = black_scholes_bound(a[0], a[1], a[2], a[3], a[5])
    for got, want in ((call, np.array(case["call"])), (put, np.array(case["put"]))):
        err = np.abs(got - want)
        print(name, "max error in units of eps (S' + K'):", float(np.max(err / (bound / 8.0))))
        assert np.all(err <= bound)


def test_fixture_agrees_with_the_reference_and_the_textbook():
    bs = KATS["black_scholes"]
    assert len(bs["random"]["price"]) == 500
    w = bs["wgpu_kat"]
    assert np.max(np.abs(np.array(w["exact"]["call"]) - np.array(w["expected_call"]))) < w["tolerance"]
    assert np.max(np.abs(np.array(w["exact"]["put"]) - np.array(w["expected_put"]))) < w["tolerance"]
    t = bs["textbook"]
    assert round(t["exact"]["call"][0], 4) == t["call_4dp"] and round(t["exact"]["put"][0], 4) == t["put_4dp"]


def test_deep_learning_restatements_meet_the_reference_kats():
    k = KATS["adam_update"]
    p, m, v = adam_ref(k["parameters"], k["gradient"], None, None, k["iteration"], k["learn_rate"], k["gradient_decay_factor"],
                       k["squared_gradient_decay_factor"], k["epsilon"])
    assert np.max(np.abs(p - k["expected_parameters"])) < k["tolerance"]
    assert np.max(np.abs(m - k["expected_average_grad"])) < k["tolerance"]
    assert np.max(np.abs(v - k["expected_average_sq_grad"])) < k["tolerance"]
    k = KATS["crossentropy_terms"]
    loss = crossentropy_ref(k["predictions"], k["targets"], k["weights"], k["mask"], multi_label=k["mode"] == "multi-label")
    assert np.max(np.abs(loss - k["expected"])) < k["tolerance"]
    assert EPS == 2.0 ** -52


# ---- compiled resources ---------------------------------------------------------------------------------------------------------
def test_workload_kernels_use_no_scratch():
    """Every kernel of workload_ops.hip: the strided pricing kernel reads its dimension table from the kernel argument with constant
    indices, and none of the closed forms (log, exp, erf, divisions, square root) may spill."""
    res = _resources("workload_ops.hip")
    for needle, count in (("k_adam_update", 8), ("k_crossentropy_terms", 16), ("k_black_scholes_flat", 2), ("k_black_scholes_strided", 4)):
        assert len(_pick(res, needle)) == count, (needle, sorted(_pick(res, needle)))
    spilled = {k: v["scratch"] for k, v in res.items() if v["scratch"] != 0}
    assert not spilled, spilled
