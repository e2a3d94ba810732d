"""CPU checks of `rmhip_complex_pagefun`: the reference the GPU tests use (tests/complex_pagefun_ref.py) is bit-equal to the three host
loops written as plain scalar loops, reproduces hand-computed Gaussian-integer products, stays inside the GPU tests' gate against
numpy's complex matmul and keeps the loops' quirks; and the entry point is bound in every mirror, dispatched by the shim on the
inputs' storage, without changing the served set."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import complex_pagefun_ref as ref
from pagefun_host import build_request

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "complex_pagefun_kats.json").read_text())


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def part(spec, key):
    return None if spec[key] is None else np.array(spec[key], dtype=np.float64).reshape(spec["shape"], order="F")


@pytest.mark.parametrize("kat", KATS["products"], ids=lambda k: k["name"])
def test_hand_computed_products(kat):
    args = (part(kat["lhs"], "re"), part(kat["lhs"], "im"), part(kat["rhs"], "re"), part(kat["rhs"], "im"))
    for f in (ref.cpagefun_host, ref.cpagefun_scalar):
        re_, im_ = f(*args)
        assert list(re_.shape) == kat["out"]["shape"]
        assert re_.ravel(order="F").tolist() == kat["out"]["re"] and im_.ravel(order="F").tolist() == kat["out"]["im"]


@pytest.mark.parametrize("kind", ref.KINDS)
def test_restatement_is_bit_equal_to_the_scalar_loops(kind):
    rng = np.random.default_rng(20 + kind)
    sides = (1, 2, 3, 5)
    for m in sides:
        for n in sides:
            for k in sides:
                for lhs_pages, rhs_pages in (((3,), (3,)), ((1,), (2,)), ((2, 1), (1, 3))):
                    args = ref.operands(rng, kind, (m, k) + lhs_pages, (k, n) + rhs_pages)
                    got, want = ref.cpagefun_host(*args), ref.cpagefun_scalar(*args)
                    for g, w in zip(got, want):
                        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (m, n, k, lhs_pages, rhs_pages)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("lhs,rhs", [((3, 4, 5), (4, 2, 5)), ((3, 4, 1), (4, 2, 5)), ((33, 70, 3), (70, 40)), ((2, 3, 2, 1), (3, 4, 1, 3)),
                                     ((7, 9, 2, 1, 3, 2), (9, 5, 1, 2, 3, 1))])
def test_against_numpy_complex_matmul_within_the_gate(kind, lhs, rhs):
    """The worst ratio is printed; two correct evaluations are expected well inside the gate the GPU tests use."""
    rng = np.random.default_rng(31)
    Ar, Ai, Br, Bi = ref.operands(rng, kind, lhs, rhs)
    got_re, got_im = ref.cpagefun_host(Ar, Ai, Br, Bi)
    r = build_request(lhs, rhs)
    A = Ar + 1j * (Ai if Ai is not None else 0.0)
    B = Br + 1j * (Bi if Bi is not None else 0.0)
    pa = np.moveaxis(A.reshape(A.shape[:2] + tuple(r.input_page_dims[0]), order="F"), (0, 1), (-2, -1))
    pb = np.moveaxis(B.reshape(B.shape[:2] + tuple(r.input_page_dims[1]), order="F"), (0, 1), (-2, -1))
    want = np.moveaxis(np.matmul(pa, pb), (-2, -1), (0, 1))
    g_re, g_im = ref.gate(Ar, Ai, Br, Bi)
    assert got_re.shape == want.shape == g_re.shape
    d_re, d_im = np.abs(got_re - want.real), np.abs(got_im - want.imag)
    print(f"worst |restatement - numpy| / gate: re {np.max(d_re / g_re):.3f} im {np.max(d_im / g_im):.3f}")
    assert np.all(d_re <= g_re) and np.all(d_im <= g_im)


def test_sum_rounding_quirks():
    # an all -0.0 page sums to +0.0 in both parts, in every kind: 0.0 + (-0.0) = +0.0
    nz, one = np.full((2, 2), -0.0), np.ones((2, 2))
    for args in ((nz, nz, one, -nz), (nz, nz, one, None), (nz, None, one, -nz)):
        re_, im_ = ref.cpagefun_host(*args)
        assert np.all(re_ == 0.0) and np.all(im_ == 0.0) and not np.any(np.signbit(re_)) and not np.any(np.signbit(im_))
    # complex x real with Inf in the complex operand is Inf; complex x complex with a zero imaginary part filled in multiplies Inf by 0
    Ar, Ai = np.array([[np.inf, 1.0]]), np.array([[2.0, np.inf]])
    Br = np.array([[3.0], [5.0]])
    re_, im_ = ref.cpagefun_host(Ar, Ai, Br, None)
    assert re_[0, 0] == np.inf and im_[0, 0] == np.inf
    re0, im0 = ref.cpagefun_host(Ar, Ai, Br, np.zeros_like(Br))
    assert np.isnan(re0[0, 0]) and np.isnan(im0[0, 0])
    # and the mirror image: real x complex
    re_, im_ = ref.cpagefun_host(Br.T.copy(), None, Ar.T.copy(), Ai.T.copy())
    assert re_[0, 0] == np.inf and im_[0, 0] == np.inf
    re0, im0 = ref.cpagefun_host(Br.T.copy(), np.zeros((1, 2)), Ar.T.copy(), Ai.T.copy())
    assert np.isnan(re0[0, 0]) and np.isnan(im0[0, 0])
    # k == 0: (+0, +0); an empty side: an empty result of the right shape
    re_, im_ = ref.cpagefun_host(np.zeros((3, 0, 2)), np.zeros((3, 0, 2)), np.zeros((0, 4, 2)), None)
    assert re_.shape == (3, 4, 2) and not np.any(np.signbit(re_)) and not np.any(np.signbit(im_)) and np.all(re_ == 0) and np.all(im_ == 0)
    assert ref.cpagefun_host(np.zeros((0, 3, 2)), np.zeros((0, 3, 2)), np.zeros((3, 4, 2)), None)[0].shape == (0, 4, 2)


def test_the_entry_point_is_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    assert _lib.SERVES["rmhip_complex_pagefun"] == ("pagefun",)
    assert _lib.SIGNATURES["rmhip_complex_pagefun"] == _lib.SIGNATURES["rmhip_pagefun"]
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "complex_pagefun", None))


def test_the_mirrors_carry_the_entry_point():
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    kats = (ROOT / "examples" / "provider_kats.cpp").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    py = (ROOT / "runmat_amd" / "provider.py").read_text()
    header = (ROOT / "include" / "rmhip.h").read_text()
    assert " complex_pagefun(" in hpp and "p.complex_pagefun(" in kats and "pub fn rmhip_complex_pagefun(" in sys_rs and "def complex_pagefun(" in py
    assert re.search(r"/\* @serves pagefun \*/\nRMHIP_API int rmhip_complex_pagefun\(", header)
    section = header[header.index("complex-interleaved storage (fft.hip)"):header.index("RMHIP_API int rmhip_storage(")]
    assert "rmhip_complex_pagefun" in section  # the list of complex-capable entry points
    assert "complex_pagefun.hip" in (ROOT / "runmat_amd" / "csrc" / "Makefile").read_text().split("SRCS_HIP :=")[1].splitlines()[0]
    src = (ROOT / "runmat_amd" / "csrc" / "complex_pagefun.hip").read_text()
    assert "k_pagefun_" not in re.sub(r"//[^\n]*", "", src)  # the sibling's resource test selects its kernels by that prefix
    assert "atomic" not in src


def test_the_shim_dispatches_on_the_storage_of_either_input():
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index("fn pagefun(&self"):]
    body = body[:re.search(r"\n    fn ", body).start()]
    real, cplx = body.index("rmhip_pagefun(self.ctx"), body.index("rmhip_complex_pagefun(self.ctx")
    rule = body.index("if !request.inputs.iter().any(Self::is_complex)")
    assert rule < real < body.index("} else {") < cplx < body.index("self.complex_handle(out)")
    assert real < body.index("self.handle(out)") < body.index("} else {")
