"""Host-side checks of the calculus and filter hooks on complex-interleaved tensors: the numpy model (tests/complex_calculus_ref.py)
against the reference providers' known answers (tests/golden/complex_calculus_kats.json), the bindings of the five rmhip_complex_* entry
points, the shim's dispatch, and the compile-time resources of the new kernels."""
import json
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_calculus_ref as ref  # noqa: E402
from iir_long_ref import FILTERS, chunked_filter, exact_filter, longdouble_is_wide, noise_floor, output_bound, state_bound  # noqa: E402
from test_kernel_resources import _pick, _resources  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "complex_calculus_kats.json").read_text())["cases"]

# entry point -> (real sibling, the trait methods both serve, the provider mirrors)
ENTRY_POINTS = {
    "rmhip_complex_gradient_dim": ("rmhip_gradient_dim", ("gradient_dim", "gradient_dim_with_coordinates"),
                                   ("complex_gradient_dim", "complex_gradient_dim_with_coordinates")),
    "rmhip_complex_trapz_dim": ("rmhip_trapz_dim", ("trapz_dim", "cumtrapz_dim"), ("complex_trapz_dim", "complex_cumtrapz_dim")),
    "rmhip_complex_polyint": ("rmhip_polyint", ("polyint",), ("complex_polyint",)),
    "rmhip_complex_iir_filter": ("rmhip_iir_filter", ("iir_filter",), ("complex_iir_filter",)),
    "rmhip_complex_iir_filter_long": ("rmhip_iir_filter_long", ("iir_filter",), ("complex_iir_filter_long",)),
}
# the seeded vector on which the two gradient rules part (chosen here, on the CPU; the GPU test uses the same one)
GRADIENT_SEED, GRADIENT_LEN, GRADIENT_SPACING = 5, 64, 0.7  # (a spacing of 0.3 never tells them apart, 0.7 does in a quarter of the parts)


def gradient_probe():
    rng = np.random.default_rng(GRADIENT_SEED)
    return ref.join(rng.standard_normal(GRADIENT_LEN), rng.standard_normal(GRADIENT_LEN)).reshape(GRADIENT_LEN, 1)


def test_the_fixture_holds_the_four_reference_cases():
    assert [c["name"] for c in KATS] == [
        "gradient_complex_host_supported",
        "gradient_complex_coordinate_vector_spacing",
        "iir_filter_provider_preserves_complex_storage_and_filters_lanes",
        "trapezoid_provider_preserves_complex_storage_and_integrates_lanes"]


def test_model_reproduces_every_known_answer_bitwise():
    for c in KATS:
        z = ref.from_interleaved(c["data"], c["shape"])
        want = ref.from_interleaved(c["expect"], c["expect_shape"])
        if c["op"] == "gradient":
            got = ref.gradient(z, c["dim"], c.get("spacing", 1.0), c.get("coordinates"))
            assert ref.same_bits(got, want), (c["name"], got)
        elif c["op"] == "iir_filter":
            y, zf = ref.iir_filter(c["b"], c["a"], z, c["dim"])
            assert ref.same_bits(y, want), (c["name"], y)
            assert ref.same_bits(zf, ref.from_interleaved(c["expect_state"], c["expect_state_shape"])), (c["name"], zf)
        else:
            assert c["op"] == "trapezoid", c["op"]
            total, _ = ref.trapz(z, c["dim"], c["spacing_kind"])
            assert ref.same_bits(total, want), (c["name"], total)
            running, _ = ref.trapz(z, c["dim"], c["spacing_kind"], cumulative=True)
            assert ref.same_bits(running, ref.from_interleaved(c["expect_cumulative"], c["expect_cumulative_shape"])), (c["name"], running)


def test_model_rules_the_kats_do_not_reach():
    inf, nan = np.inf, np.nan
    # lanes never meet: an Inf or a NaN in one part leaves the other finite
    z = ref.join([1.0, inf, 2.0, 4.0], [nan, 1.0, 3.0, 5.0]).reshape(4, 1)
    g = ref.gradient(z, 0, 2.0)
    assert np.all(np.isfinite(g.imag[2:])) and np.all(np.isfinite(g.real[[1, 3]])) and np.all(np.isnan(g.imag[:2])) and np.all(np.isinf(g.real[[0, 2]]))
    t, _ = ref.trapz(z, 0, 1, 0.5)
    assert np.isinf(t.real[0, 0]) and np.isnan(t.imag[0, 0]) and t.shape == (1, 1)
    p = ref.polyint(z.T, 7.0)
    assert p.shape == (1, 5) and p[0, 4] == 7.0 and np.isinf(p.real[0, 1]) and p.imag[0, 1] == 1.0 / 3.0
    y, zf = ref.iir_filter([1.0, 0.5], [1.0, -0.5], z, 0)
    assert np.all(np.isfinite(y.real[:1])) and np.all(np.isnan(y.imag)) and zf.shape == (1, 1)
    # shapes
    assert ref.gradient(np.zeros(3, dtype=complex), 0).shape == (3, 1) and ref.gradient(np.zeros((0, 3), dtype=complex), 0).shape == (0, 3)
    assert ref.same_bits(ref.gradient(z, 3), np.zeros((4, 1)))
    assert ref.trapz(np.ones((2, 3), dtype=complex), 3)[0].shape == (2, 3, 1, 1) and ref.trapz(np.ones((2, 3), dtype=complex), 1, cumulative=True)[0].shape == (2, 3)
    assert ref.trapz(np.ones((0, 3), dtype=complex), 0)[0].shape == (1, 3)
    assert ref.polyint(np.zeros((3, 1), dtype=complex)).shape == (4, 1) and ref.polyint(np.zeros((1, 1), dtype=complex)).shape == (1, 2)
    assert ref.polyint(np.zeros((0, 1), dtype=complex), 2.0).shape == (1, 1) and ref.polyint(np.zeros((0, 1), dtype=complex), 2.0)[0, 0] == 2.0
    # a gain keeps the sign of a zero; the spacing kinds index the width by the logical element
    assert ref.same_bits(ref.iir_filter([2.0], [1.0], ref.join([-0.0], [0.0]).reshape(1, 1), 0)[0], ref.join([-0.0], [0.0]).reshape(1, 1))
    x = ref.join([1.0, 2.0, 4.0], [0.0, 1.0, 0.0]).reshape(3, 1)
    assert ref.same_bits(ref.trapz(x, 0, 3, [0.0, 1.0, 3.0])[0], ref.join([7.5], [1.5]).reshape(1, 1))
    assert ref.same_bits(ref.trapz(x, 0, 4, [0.0, 1.0, 3.0])[0], ref.trapz(x, 0, 3, [0.0, 1.0, 3.0])[0])
    assert ref.same_bits(ref.trapz(x, 0, 2, [2.0, 9.0])[0], ref.trapz(x, 0, 1, 2.0)[0])


def test_the_two_gradient_rules_part_on_the_seeded_vector():
    """(x[k+1] - x[k-1]) * (1.0 / den) and (x[k+1] - x[k-1]) / den differ in the last bit of some elements: data that cannot tell them apart
    would let the real kernel's quotient pass for the complex rule."""
    z = gradient_probe()
    rule, quotient = ref.interleaved(ref.gradient(z, 0, GRADIENT_SPACING)), ref.interleaved(ref.gradient_quotient(z, 0, GRADIENT_SPACING))
    differing = int(np.count_nonzero(rule.view(np.uint64) != quotient.view(np.uint64)))
    assert differing >= 1, differing
    assert np.max(np.abs(rule - quotient) / np.abs(quotient)) <= 2.0 ** -52  # ... and by no more than that bit


def test_entry_points_are_bound_as_second_entry_points_of_served_hooks():
    from runmat_amd import HipProvider, _lib

    for name, (sibling, methods, mirrors) in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sibling], name
        assert _lib.SERVES[name] == _lib.SERVES[sibling] == methods, (name, _lib.SERVES[name])
        for mirror in mirrors:
            assert callable(getattr(HipProvider, mirror, None)), mirror
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)


def test_the_shim_and_the_cpp_mirror_dispatch_every_hook():
    src = (ROOT / "shim" / "hip_provider.rs").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    bodies = {"gradient_dim": "gradient_dim", "gradient_dim_with_coordinates": "gradient_dim_with_coordinates", "trapz_dim": "trapezoid",
              "polyint": "polyint", "iir_filter": "iir_filter"}
    for name, (sibling, methods, mirrors) in ENTRY_POINTS.items():
        assert f"pub fn {name}(" in sys_rs, name
        for mirror in mirrors:
            assert re.search(r"\b%s\(" % mirror, hpp), mirror
        for method in methods:
            if method not in bodies:
                continue
            body = re.search(r"fn %s\b.*?\n    }\n" % bodies[method], src, re.S)
            assert body, method
            assert f"{name}(self.ctx" in body.group(0) and "is_complex" in body.group(0) and "complex_handle" in body.group(0), (name, method)
    body = re.search(r"fn iir_filter\b.*?\n    }\n", src, re.S).group(0)  # the two-step sequence, once per storage kind
    assert body.count("RMHIP_ERR_UNSUPPORTED") == 2 and "rmhip_iir_filter_long(self.ctx" in body


def test_new_kernels_stay_in_registers():
    """One 16-byte element per thread, a handful of values live: none of the new kernels may touch scratch.  (The filter kernels gained no
    instantiation: the complex entry points launch the real ones on the [2, S...] view.)"""
    misc, signal = _resources("misc_ops.hip"), _resources("signal_ops.hip")
    picked = {**_pick(misc, "k_gradient_cx"), **_pick(misc, "k_trapz_terms_cx"), **_pick(misc, "k_round_f32"), **_pick(signal, "k_polyint_cx")}
    assert len(_pick(misc, "k_trapz_terms_cx")) == 4, sorted(_pick(misc, "k_trapz_terms_cx"))
    for name, r in picked.items():
        assert r["scratch"] == 0, (name, r)
    for name, r in {**_pick(signal, "k_iirILi8E"), **_pick(signal, "k_iir_chunksILi8E")}.items():
        assert r["scratch"] == 0, (name, r)


def test_chunked_scan_model_stays_inside_the_contract_for_the_gpu_inputs():
    """The GPU test holds the long form to the sibling's accuracy contract per lane on these inputs; the numpy model of the chunked scan
    must itself be inside it, with room, or the yardsticks would be the wrong ones."""
    if not longdouble_is_wide():
        import pytest

        pytest.skip("np.longdouble carries fewer than 63 mantissa bits")
    for name in ref.LONG_FILTERS:
        b, a = FILTERS[name]
        z, zi = ref.long_signal(name)
        LONG_LEN = ref.LONG_LEN
        for lane, s0 in ((z.real, zi.real), (z.imag, zi.imag)):
            for ch in range(lane.shape[1]):
                x, st = lane[:, ch], s0[:, ch]
                got = chunked_filter(b, a, x, st)
                assert got is not None and got[2] > 0 and LONG_LEN % got[2] != 0, (name, got and got[2])
                y_ref, zf_ref = ref.df2t(*ref.normalise(b, a), x.copy(), st.copy())
                y_exact, zf_exact = exact_filter(b, a, x, st)
                floor = noise_floor(b, a, x)
                assert np.max(np.abs(got[0] - y_exact)) <= 0.5 * output_bound(y_ref, y_exact, floor), name
                assert np.max(np.abs(got[1] - zf_exact)) <= 0.5 * state_bound(zf_ref, zf_exact, b, a, floor), name
