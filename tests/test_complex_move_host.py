"""Host-side checks of the shape and indexing hooks on complex-interleaved tensors: the numpy model (tests/complex_move_ref.py) against
the reference providers' known answers (tests/golden/complex_move_kats.json), the bindings of the nine rmhip_complex_* entry points, and
the compile-time resources of the 16-byte kernels."""
import json
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import complex_move_ref as ref  # noqa: E402
from test_kernel_resources import _pick, _resources  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "complex_move_kats.json").read_text())["cases"]

# entry point -> (real sibling, the one trait method both serve)
ENTRY_POINTS = {
    "rmhip_complex_reshape": ("rmhip_reshape", "reshape"),
    "rmhip_complex_transpose": ("rmhip_transpose", "transpose"),
    "rmhip_complex_permute": ("rmhip_permute", "permute"),
    "rmhip_complex_repmat": ("rmhip_repmat", "repmat"),
    "rmhip_complex_gather_linear": ("rmhip_gather_linear", "gather_linear"),
    "rmhip_complex_scatter_linear": ("rmhip_scatter_linear", "scatter_linear"),
    "rmhip_complex_circshift": ("rmhip_circshift", "circshift"),
    "rmhip_complex_flip": ("rmhip_flip", "flip"),
    "rmhip_complex_cat": ("rmhip_cat", "cat"),
}


def test_the_fixture_holds_the_five_reference_cases():
    assert [c["name"] for c in KATS] == [
        "transpose_complex_interleaved_downloads_by_logical_element",
        "transpose_complex_interleaved_feeds_downstream_abs_in_transposed_order",
        "permute_complex_interleaved_three_dimensional_stays_resident",
        "wgpu_linear_gather_and_scatter_copy_complex_logical_elements",
        "linear_gather_and_scatter_copy_complex_logical_elements"]


def test_model_reproduces_every_known_answer():
    for c in KATS:
        z = ref.from_interleaved(c["data"], c["shape"])
        if c["op"] == "transpose":
            got = ref.transpose(z)
            assert got.shape == tuple(c["expect_shape"]) and ref.same_bits(got, ref.from_interleaved(c["expect"], c["expect_shape"])), c["name"]
        elif c["op"] == "transpose_abs":
            got = ref.transpose(z)
            mags = np.abs(ref.flat(got))
            assert got.shape == tuple(c["expect_shape"]) and np.all(np.abs(mags - np.sqrt(c["expect_squares"])) <= c["tolerance"]), c["name"]
        elif c["op"] == "permute":
            got = ref.permute(z, c["order"])
            assert got.shape == tuple(c["expect_shape"]) and ref.same_bits(got, ref.from_interleaved(c["expect"], c["expect_shape"])), c["name"]
        else:
            assert c["op"] == "gather_scatter", c["op"]
            g = ref.gather(z, c["gather_indices"], c["gather_shape"])
            assert ref.same_bits(g, ref.from_interleaved(c["expect_gathered"], c["gather_shape"])), c["name"]
            t = ref.scatter(np.zeros(c["target_shape"], dtype=np.complex128), c["scatter_indices"], g)
            assert ref.same_bits(t, ref.from_interleaved(c["expect_target"], c["target_shape"])), c["name"]


def test_model_rules_the_kats_do_not_reach():
    z = (np.arange(6) + 1j * np.arange(6, 12)).reshape((3, 2), order="F")
    assert ref.repmat(z, (2,)).shape == (6, 4) and ref.repmat(z, (2, 3)).shape == (6, 6) and ref.repmat(z, (1, 1, 4)).shape == (3, 2, 4)
    assert ref.repmat(z, (0, 2)).shape == (0, 4)
    assert ref.same_bits(ref.circshift(z, (1,)), np.roll(z, 1, axis=0)) and ref.same_bits(ref.circshift(z, (-2, 3, 7)), np.roll(z, (1, 1), axis=(0, 1)))
    assert ref.same_bits(ref.flip(z, (0, 0)), z) and ref.same_bits(ref.flip(z, (5,)), z) and ref.same_bits(ref.flip(z, (0, 1)), z[::-1, ::-1])
    assert ref.cat(3, [z, z]).shape == (3, 2, 2) and ref.cat(1, [z, z]).shape == (6, 2)
    assert ref.cat(1, [z.reshape((3, 2, 1), order="F"), z]).shape == (6, 2)  # trailing 1s dropped down to max(dim, 2) dimensions
    assert ref.permute(z, (2, 0, 1)).shape == (1, 3, 2)
    s = ref.scatter(np.zeros((4, 1), dtype=np.complex128), [1, 1, 3, 1], np.array([1 + 1j, 2 + 2j, 3 + 3j, 4 + 4j]))
    assert ref.same_bits(s, np.array([0, 4 + 4j, 0, 3 + 3j]).reshape(4, 1))  # the last duplicate wins
    nan = np.array([0x7ff8000000000123, 0x8000000000000000], dtype=np.uint64).view(np.complex128)  # a NaN payload, a negative zero
    assert np.array_equal(ref.bits(ref.scatter(np.zeros((2, 1), dtype=np.complex128), [1], nan))[2:], nan.view(np.uint64))


def test_entry_points_are_bound_as_second_entry_points_of_served_hooks():
    from runmat_amd import HipProvider, _lib

    for name, (sibling, method) in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sibling], name
        assert _lib.SERVES[name] == (method,) and method in _lib.SERVES[sibling], name
        assert callable(getattr(HipProvider, name[len("rmhip_"):], None)), name
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)


def test_the_shim_dispatches_every_hook_on_storage():
    src = (ROOT / "shim" / "hip_provider.rs").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    for name, (sibling, method) in ENTRY_POINTS.items():
        assert f"pub fn {name}(" in sys_rs, name
        body = re.search(r"fn %s\b.*?\n    }\n" % method, src, re.S)
        assert body, method
        assert f"{name}(self.ctx" in body.group(0) and f"{sibling}(self.ctx" in body.group(0) and "is_complex" in body.group(0), method


def test_sixteen_byte_kernels_stay_in_registers_and_keep_their_occupancy():
    """One 16-byte element per load: no kernel may spill, and the tiled permutation must keep the occupancy its LDS tile implies - a
    32 x 65 tile of 16-byte elements is 33 280 bytes, four blocks of four waves per CU (160 KiB of LDS): four waves per SIMD."""
    res = _resources("tensor_ops.hip")
    v2d = "Dv2_d"  # the mangled ext_vector_type(2) of double
    moved = {}
    for needle in ("k_index_copyI", "k_index_copy_flatI", "k_gatherI", "k_gather_checkedI", "k_scatterI", "k_scatter_ownedI"):
        hits = {k: v for k, v in _pick(res, needle).items() if v2d in k}
        assert hits, needle
        moved.update(hits)
    tiled = _pick(res, "k_permute_tiled16")
    assert len(tiled) == 1, sorted(tiled)
    for name, r in {**moved, **tiled}.items():
        assert r["scratch"] == 0, (name, r)
    (name, r), = tiled.items()
    ti, tj = (int(v) for v in re.search(r"k_permute_tiled16ILi(\d+)ELi(\d+)E", name).groups())
    lds = ti * (tj + 1) * 16
    assert r["occupancy"] >= (4 if lds <= 40 * 1024 else 2), (name, r, lds)
