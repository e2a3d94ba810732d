"""GPU checks of black_scholes_price, adam_update and crossentropy_terms (runmat_amd/csrc/workload_ops.hip) against the numpy restatements
of the CPU provider (tests/workload_hooks_ref.py) and the exact values of tests/golden/workload_hooks_kats.json.

Bounds.  Adam has no transcendental: bit for bit.  Cross-entropy: the device logarithm is within 2 ulp (tests/test_gpu_parity.py), plus
one rounding per product and per subtraction: |got - want| <= 4 eps (|t ln c| + |(1 - t) ln(1 - c)|) w m, the second term in the
multi-label mode only.  Black-Scholes against exact prices: |err| <= 8 eps (S e^{-qT} + K e^{-rT}).  A common shift of d1 and d2
cancels to first order (S' phi(d1) = K' phi(d2)), so the rounding errors d1 and d2 share do not matter; what remains is 2 ulp for each
exp and erf, the 0.5 (1 + erf) rounding and the d1 - sigma sqrt(T) subtraction: about 6 of these units.  The f64 CPU restatement
itself measures 1.0 on the fixture's range (tests/test_workload_hooks_host.py prints it)."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from runmat_amd import HipProvider, ProviderError
from runmat_amd import _lib
from workload_hooks_ref import (EPS, adam_ref, black_scholes_bound, black_scholes_ref, crossentropy_bound, crossentropy_ref)

pytestmark = pytest.mark.gpu

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "workload_hooks_kats.json").read_text())
INPUT_KEYS = ("price", "strike", "rate", "time", "volatility", "yield")


@pytest.fixture(scope="module")
def prov32(built):
    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def up(p, a, shape=None):
    a = np.asarray(a, dtype=np.float64)
    shape = tuple(shape) if shape is not None else (a.shape if a.ndim >= 2 else (a.size, 1) if a.ndim == 1 else (1, 1))
    return p.upload(a.ravel(order="F"), shape)


def down(p, handles):
    out = [p.download(h).reshape(h.shape, order="F") for h in handles]
    for h in handles:
        p.free(h)
    return out


# ---- adam_update ----------------------------------------------------------------------------------------------------------------
ADAM_SCALARS = dict(learn_rate=0.01, gradient_decay_factor=0.9, squared_gradient_decay_factor=0.999, epsilon=1.0e-8)
ADAM_SHAPES = [(1,), (2,), (3,), (255,), (256,), (257,), (2049, 3)]
_adam_data = {}


def adam_inputs(shape):
    """Seeded operands per shape, generated once and left unchanged."""
    if shape not in _adam_data:
        rng = np.random.default_rng(int(np.prod(shape)))
        _adam_data[shape] = (rng.standard_normal(shape), rng.standard_normal(shape), 0.1 * rng.standard_normal(shape), rng.uniform(0.0, 1.0, shape))
    return _adam_data[shape]


def run_adam(p, p0, g, m0, v0, iteration, **scalars):
    hs = [up(p, p0), up(p, g), None if m0 is None else up(p, m0), None if v0 is None else up(p, v0)]
    try:
        outs = p.adam_update(hs[0], hs[1], hs[2], hs[3], iteration=iteration, **scalars)
    finally:
        for h in hs:
            if h is not None:
                p.free(h)
    assert all(tuple(o.shape) == tuple(hs[0].shape) for o in outs)
    return down(p, outs)


def adam_case(p, shape, moments, iteration, to_bits=bits, rnd=lambda a: a):
    p0, g, m0, v0 = [rnd(a) for a in adam_inputs(shape)]
    m0 = m0 if moments in ("both", "first") else None
    v0 = v0 if moments in ("both", "second") else None
    b1, b2 = ADAM_SCALARS["gradient_decay_factor"], ADAM_SCALARS["squared_gradient_decay_factor"]
    want = adam_ref(p0, g, m0, v0, iteration, ADAM_SCALARS["learn_rate"], b1, b2, ADAM_SCALARS["epsilon"])
    got = run_adam(p, p0, g, m0, v0, iteration, **ADAM_SCALARS)
    for name, a, b in zip(("parameters", "average_grad", "average_sq_grad"), got, want):
        assert np.array_equal(to_bits(a).ravel(), to_bits(b.reshape(a.shape)).ravel()), (name, shape, moments, iteration)


@pytest.mark.parametrize("iteration", [1, 1000])
@pytest.mark.parametrize("moments", ["both", "none", "first", "second"])
@pytest.mark.parametrize("shape", ADAM_SHAPES, ids=str)
def test_adam_update_is_bit_exact(prov, shape, moments, iteration):
    adam_case(prov, shape, moments, iteration)


@pytest.mark.parametrize("moments,iteration", [("both", 1000), ("none", 1)])
def test_adam_update_is_bit_exact_at_four_million_elements(prov, moments, iteration):
    adam_case(prov, (1 << 22,), moments, iteration)


@pytest.mark.parametrize("moments,iteration", [("both", 1000), ("none", 1), ("first", 1), ("second", 1000)])
@pytest.mark.parametrize("shape", [(1,), (3,), (255,), (257,), (2049, 3)], ids=str)
def test_adam_update_f32_storage_rounds_once(prov32, shape, moments, iteration):
    adam_case(prov32, shape, moments, iteration, to_bits=bits32, rnd=f32)


def test_adam_update_reference_kat(prov):
    k = KATS["adam_update"]
    got = run_adam(prov, np.array(k["parameters"]).reshape(k["shape"]), np.array(k["gradient"]).reshape(k["shape"]), None, None, k["iteration"],
                   learn_rate=k["learn_rate"], gradient_decay_factor=k["gradient_decay_factor"],
                   squared_gradient_decay_factor=k["squared_gradient_decay_factor"], epsilon=k["epsilon"])
    for a, key in zip(got, ("expected_parameters", "expected_average_grad", "expected_average_sq_grad")):
        assert a.shape == tuple(k["shape"]) and np.max(np.abs(a.ravel() - k[key])) < k["tolerance"], key


def test_adam_update_errors_carry_the_reference_text_and_leave_the_provider_usable(prov):
    p0, g = np.ones(300), np.full(300, 0.5)
    bad_g = g.copy()
    bad_g[257] = np.nan
    with pytest.raises(ProviderError, match="adam_update: inputs must contain finite values") as e:
        run_adam(prov, p0, bad_g, None, None, 1, **ADAM_SCALARS)
    assert e.value.code == _lib.ERR_INVALID
    big = p0.copy()
    big[3] = 1.7e308
    neg = g.copy()
    neg[3] = -1.0
    with pytest.raises(ProviderError, match="adam_update: update produced a non-finite value") as e:
        run_adam(prov, big, neg, None, None, 1, **{**ADAM_SCALARS, "learn_rate": 1e308})
    assert e.value.code == _lib.ERR_INVALID
    neg[200] = np.inf  # an input failure wins over an output failure
    with pytest.raises(ProviderError, match="adam_update: inputs must contain finite values"):
        run_adam(prov, big, neg, None, None, 1, **{**ADAM_SCALARS, "learn_rate": 1e308})
    with pytest.raises(ProviderError, match="adam_update: iteration must be positive"):
        run_adam(prov, p0, g, None, None, 0, **ADAM_SCALARS)
    with pytest.raises(ProviderError, match="adam_update: optimizer tensors must match parameter shape"):
        run_adam(prov, p0, g[:299], None, None, 1, **ADAM_SCALARS)
    with pytest.raises(ProviderError, match=r"adam_update: gradient decay factor must be in \[0, 1\)"):
        run_adam(prov, p0, g, None, None, 1, **{**ADAM_SCALARS, "gradient_decay_factor": 1.0})
    test_adam_update_reference_kat(prov)


# ---- crossentropy_terms ---------------------------------------------------------------------------------------------------------
def ce_inputs(n):
    rng = np.random.default_rng(100 + n)
    special_p = np.array([0.0, 1.0, 1e-300, 1.0 - 2.0 ** -53, -0.5, 1.5, 0.0, 1.0, 0.5, 1e-13, 1.0 - 1e-13])
    special_t = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.25, 0.75])
    pred, target = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    k = min(n, special_p.size)
    pred[:k], target[:k] = special_p[:k], special_t[:k]
    target[rng.integers(0, n, n // 4)] = 0.0
    target[rng.integers(0, n, n // 4)] = 1.0
    weights = rng.uniform(0.0, 3.0, n)
    weights[rng.integers(0, n, n // 8)] = 0.0
    mask = rng.integers(0, 2, n).astype(np.float64)
    return pred, target, weights, mask


def run_ce(p, pred, target, weights, mask, multi):
    hs = [up(p, pred), up(p, target), None if weights is None else up(p, weights), None if mask is None else up(p, mask)]
    try:
        out = p.crossentropy_terms(hs[0], hs[1], hs[2], hs[3], mode="multi-label" if multi else "single-label")
    finally:
        for h in hs:
            if h is not None:
                p.free(h)
    assert tuple(out.shape) == tuple(hs[0].shape)
    return down(p, [out])[0]


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("operands", ["plain", "weights", "mask", "both"])
@pytest.mark.parametrize("n", [1, 3, 11, 257, 6147])
def test_crossentropy_terms_within_the_logarithm_bound(prov, n, operands, multi):
    pred, target, weights, mask = ce_inputs(n)
    weights = weights if operands in ("weights", "both") else None
    mask = mask if operands in ("mask", "both") else None
    want = crossentropy_ref(pred, target, weights, mask, multi).reshape(n, 1)
    bound = crossentropy_bound(pred, target, weights, mask, multi).reshape(n, 1)
    got = run_ce(prov, pred, target, weights, mask, multi)
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        print("crossentropy", n, operands, multi, "max err / bound:", float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert np.all(err <= bound), float(np.max(err - bound))
    zero = want == 0.0
    assert np.array_equal(bits(got[zero]), bits(want[zero]))  # the same zero, sign included


def test_crossentropy_terms_reference_kat(prov):
    k = KATS["crossentropy_terms"]
    a = [np.array(k[key]).reshape(k["shape"]) for key in ("predictions", "targets", "weights", "mask")]
    got = run_ce(prov, a[0], a[1], a[2], a[3], k["mode"] == "multi-label")
    assert got.shape == tuple(k["shape"]) and np.max(np.abs(got.ravel() - k["expected"])) < k["tolerance"]


def test_crossentropy_terms_f32_storage(prov32):
    pred, target, weights, mask = [f32(a) for a in ce_inputs(257)]
    for multi in (False, True):
        want = crossentropy_ref(pred, target, weights, mask, multi)
        got = run_ce(prov32, pred, target, weights, mask, multi).ravel()
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


CE_ERRORS = [
    ("pred_nan", "crossentropy_terms: inputs must contain finite values"),
    ("weight_negative", "crossentropy_terms: weights must contain finite nonnegative values"),
    ("mask_half", "crossentropy_terms: mask must contain binary 0 or 1 values"),
    ("target_above_one", r"crossentropy_terms: targets must be probabilities in the range \[0, 1\]"),
    ("loss_overflow", "crossentropy_terms: loss produced a non-finite value"),
]


@pytest.mark.parametrize("kind,message", CE_ERRORS, ids=[k for k, _ in CE_ERRORS])
def test_crossentropy_terms_error_classes_and_their_priority(prov, kind, message):
    """Each request holds its own failure and every failure of lower priority, at other elements: the highest one is reported."""
    n = 300
    pred, target, weights, mask = np.full(n, 0.5), np.full(n, 0.5), np.ones(n), np.ones(n)
    order = [k for k, _ in CE_ERRORS]
    for k in order[order.index(kind):]:
        if k == "pred_nan":
            pred[290] = np.nan
        elif k == "weight_negative":
            weights[5] = -1.0
        elif k == "mask_half":
            mask[100] = 0.5
        elif k == "target_above_one":
            target[257] = 1.5
        else:
            pred[7], target[7], weights[7] = 0.0, 1.0, 1e308
    with pytest.raises(ProviderError, match=message) as e:
        run_ce(prov, pred, target, weights, mask, True)
    assert e.value.code == _lib.ERR_INVALID
    test_crossentropy_terms_reference_kat(prov)  # the provider still serves the next call


def test_crossentropy_terms_refuses_empty_and_mismatched_operands(prov):
    with pytest.raises(ProviderError, match="crossentropy_terms: predictions must not be empty"):
        run_ce(prov, np.zeros((0, 3)), np.zeros((0, 3)), None, None, False)
    with pytest.raises(ProviderError, match="crossentropy_terms: targets must match prediction shape"):
        run_ce(prov, np.full((2, 3), 0.5), np.full((3, 2), 0.5), None, None, False)
    with pytest.raises(ProviderError, match="crossentropy_terms: weights and mask must match prediction shape"):
        run_ce(prov, np.full((2, 3), 0.5), np.full((2, 3), 0.5), np.ones((6, 1)), None, False)


# ---- black_scholes_price --------------------------------------------------------------------------------------------------------
def run_bs(p, arrays, shapes=None):
    shapes = shapes or [None] * 6
    hs = [up(p, a, s) for a, s in zip(arrays, shapes)]
    try:
        call, put = p.black_scholes_price(hs)
    finally:
        for h in hs:
            p.free(h)
    assert tuple(call.shape) == tuple(put.shape)
    return down(p, [call, put])


def exact_sets():
    bs = KATS["black_scholes"]
    return {"random": bs["random"], "wgpu_kat": bs["wgpu_kat"]["exact"], "textbook": bs["textbook"]["exact"]}


@pytest.mark.parametrize("name", ["random", "wgpu_kat", "textbook"])
def test_black_scholes_fixture_cases_against_exact_values(prov, name):
    case = exact_sets()[name]
    a = [np.array(case[k]) for k in INPUT_KEYS]
    bound = black_scholes_bound(a[0], a[1], a[2], a[3], a[5]).reshape(-1, 1)
    call, put = run_bs(prov, a)
    for label, got, want in (("call", call, case["call"]), ("put", put, case["put"])):
        err = np.abs(got - np.array(want).reshape(-1, 1))
        print("black_scholes", name, label, "max error in units of eps (S' + K'):", float(np.max(err / (bound / 8.0))))
        assert np.all(err <= bound), float(np.max(err / (bound / 8.0)))


def test_black_scholes_reference_kat_broadcasts_resident_inputs(prov):
    w = KATS["black_scholes"]["wgpu_kat"]
    arrays = [np.array(w["price"]["data"]), np.array(w["strike"]["data"]), w["rate"], w["time"], w["volatility"], w["yield"]]
    call, put = run_bs(prov, arrays, [w["price"]["shape"], w["strike"]["shape"], None, None, None, None])
    assert call.shape == tuple(w["output_shape"])
    assert np.max(np.abs(call.ravel(order="F") - w["expected_call"])) < w["tolerance"]
    assert np.max(np.abs(put.ravel(order="F") - w["expected_put"])) < w["tolerance"]
    t = KATS["black_scholes"]["textbook"]
    call, put = run_bs(prov, t["inputs"])
    assert round(float(call[0, 0]), 4) == t["call_4dp"] and round(float(put[0, 0]), 4) == t["put_4dp"]


def test_black_scholes_edge_elements(prov):
    """T = 0 and sigma = 0 price to the intrinsic pair, invalid elements to (NaN, NaN).  Bit for bit where the restatement involves no
    transcendental of a non-zero argument (exp(+-0) = 1 on both sides); the sigma = 0 elements with a real discount factor carry the
    device exponential and are held to the pricing bound instead."""
    #                 T = 0      T = 0      T = 0     sigma = 0, no discounting   price < 0  strike = 0  rate = Inf  vol < 0  NaN time  -0 time
    price = np.array([100.0,     90.0,      100.0,    120.0,    80.0,    100.0,   -1.0,      100.0,      100.0,      100.0,   100.0,    100.0])
    strike = np.array([95.0,     95.0,      100.0,    100.0,    100.0,   100.0,   100.0,     0.0,        100.0,      100.0,   100.0,    90.0])
    rate = np.array([0.05,       0.05,      0.03,     0.0,      0.0,     -0.0,    0.05,      0.05,       np.inf,     0.05,    0.05,     0.05])
    time = np.array([0.0,        0.0,       0.0,      2.0,      2.0,     1.0,     1.0,       1.0,        1.0,        1.0,     np.nan,   -0.0])
    vol = np.array([0.2,         0.2,       0.0,      0.0,      0.0,     0.0,     0.2,       0.2,        0.2,        -0.1,    0.2,      0.2])
    yld = np.array([0.01,        0.01,      0.02,     0.0,      -0.0,    0.0,     0.0,       0.0,        0.0,        0.0,     0.0,      0.01])
    arrays = [price, strike, rate, time, vol, yld]
    want = black_scholes_ref(*arrays)
    got = run_bs(prov, arrays)
    for g, w in zip(got, want):
        g = g.ravel()
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.isnan(w).sum() == 5
        ok = ~np.isnan(w)
        assert np.array_equal(bits(g[ok]), bits(w[ok]))
    assert got[0][0, 0] == 5.0 and got[1][1, 0] == 5.0 and got[0][3, 0] == 20.0 and got[1][4, 0] == 20.0
    # sigma = 0 with discounting: max(S e^{-qT} - K e^{-rT}, 0) through the device exponential
    arrays = [np.array([120.0, 80.0]), np.array([100.0, 100.0]), np.array([0.05, 0.02]), np.array([2.0, 0.5]), np.zeros(2), np.array([0.01, 0.03])]
    want = black_scholes_ref(*arrays)
    got = run_bs(prov, arrays)
    bound = black_scholes_bound(arrays[0], arrays[1], arrays[2], arrays[3], arrays[5])
    for g, w in zip(got, want):
        assert np.all(np.abs(g.ravel() - w) <= bound)


def bs_operands(shapes, seed):
    """Random operands in the fixture's ranges, one per shape (() = a scalar)."""
    rng = np.random.default_rng(seed)
    ranges = [(50, 150), (50, 150), (0, 0.1), (0.05, 3), (0.05, 0.8), (0, 0.05)]
    return [rng.uniform(lo, hi, s) for (lo, hi), s in zip(ranges, shapes)]


BS_SHAPES = {
    "all_scalar": [()] * 6,
    "all_7x9": [(7, 9)] * 6,
    "column_against_row": [(4, 1), (1, 5), (), (), (), ()],
    "three_dims": [(3, 1, 4), (1, 5, 1), (), (), (), ()],
    "eight_dims_that_merge": [(2, 3, 4, 1, 1, 1, 1, 5), (1, 1, 1, 1, 1, 1, 1, 5), (), (), (), ()],
    "eight_dims_alternating": [(2, 1, 3, 1, 2, 1, 2, 1), (1, 2, 1, 1, 1, 2, 1, 2), (), (), (), ()],
    "tail_257": [(257, 1), (257, 1), (), (), (257, 1), ()],
    "flat_2049x3": [(2049, 3)] * 3 + [(), (2049, 3), ()],
    "strided_2049x3": [(2049, 3), (2049, 1), (), (1, 3), (), ()],
}


@pytest.mark.parametrize("name", list(BS_SHAPES), ids=list(BS_SHAPES))
def test_black_scholes_broadcasting_against_the_flat_restatement(prov, name):
    shapes = BS_SHAPES[name]
    arrays = bs_operands(shapes, 7 + len(name))
    want = black_scholes_ref(*arrays)
    full = np.broadcast_arrays(*arrays)
    out_shape = full[0].shape if full[0].ndim >= 2 else (1, 1)
    bound = black_scholes_bound(full[0], full[1], full[2], full[3], full[5]).reshape(out_shape)
    got = run_bs(prov, arrays)
    # the same request with every operand expanded on the host: the flat kernel, the same arithmetic - bit for bit
    expanded = run_bs(prov, [np.ascontiguousarray(a).reshape(out_shape) for a in full])
    for g, w, x in zip(got, want, expanded):
        assert g.shape == out_shape
        assert np.all(np.abs(g - w.reshape(out_shape)) <= bound)
        assert np.array_equal(bits(g), bits(x))


def test_black_scholes_zero_extent_and_refusals(prov):
    call, put = run_bs(prov, [np.zeros((0, 3)), np.full((1, 3), 100.0), 0.05, 0.5, 0.2, 0.0])
    assert call.shape == put.shape == (0, 3)
    ten = [(2, 1) * 5, (1, 2) * 5, (), (), (), ()]
    with pytest.raises(ProviderError, match="after collapsing") as e:
        run_bs(prov, bs_operands(ten, 3))
    assert e.value.code == _lib.ERR_INVALID
    # the C entry point's own checks: a length that is not the shape's, an input whose buffer is not its shape's size
    import ctypes as C
    hs = [up(prov, np.full((2, 1), 100.0))] + [up(prov, 0.5) for _ in range(5)]
    ids = (C.c_uint64 * 6)(*[h.buffer_id for h in hs])
    osh = (C.c_size_t * 2)(2, 1)
    std = (C.c_size_t * 12)(*([1, 2] * 6))
    call, put = C.c_uint64(), C.c_uint64()
    good = (C.c_size_t * 12)(*([2, 1] + [1, 1] * 5))
    lib = _lib.load()
    assert lib.rmhip_black_scholes_price(prov._ctx, ids, good, std, osh, 2, 3, C.byref(call), C.byref(put)) == _lib.ERR_INVALID
    wrong = (C.c_size_t * 12)(*([2, 1] + [2, 1] + [1, 1] * 4))
    assert lib.rmhip_black_scholes_price(prov._ctx, ids, wrong, std, osh, 2, 2, C.byref(call), C.byref(put)) == _lib.ERR_INVALID
    assert "shape does not match buffer length" in _lib.last_error()
    assert lib.rmhip_black_scholes_price(prov._ctx, ids, good, std, osh, 2, 2, C.byref(call), C.byref(put)) == _lib.OK
    for h in hs:
        prov.free(h)
    lib.rmhip_free(prov._ctx, call.value)
    lib.rmhip_free(prov._ctx, put.value)


def test_black_scholes_f32_storage_within_one_f32_ulp(prov32):
    case = KATS["black_scholes"]["random"]
    a = [f32(case[k]) for k in INPUT_KEYS]
    single = a[:2] + [a[2][:1], a[3], a[4], a[5][:1]]  # rate and yield as single elements
    for arrays in (a, single):
        want = black_scholes_ref(*[x.reshape(-1, 1) for x in arrays])
        got = run_bs(prov32, arrays)
        for g, w in zip(got, want):
            w32 = w.ravel().astype(np.float32)
            assert np.all(np.abs(g.ravel() - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64))
