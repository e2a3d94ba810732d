"""CPU checks of `rmhip_complex_matmul`: the entry point is bound in every mirror without changing the served set, the shim chooses it
by the storage of either operand, the embedding the library runs (tests/complex_matmul_ref.py embed_model) stays inside the GPU tests'
gate against the host loops and is bit-equal on Gaussian integers, and plan_cgemm (gemm_plan.h), run through
tests/cpp/cgemm_route_check.cpp, returns the fields of that file's table and hands plan_dgemm a product it has a kernel for."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import complex_matmul_ref as ref

ROOT = Path(__file__).resolve().parent.parent
GPU_SHAPES = ref.SMALL_SHAPES + ref.BOUNDARY_SHAPES + ref.EMBED_SHAPES


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_the_entry_point_is_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    restype, argtypes = _lib.SIGNATURES["rmhip_complex_matmul"]
    assert len(argtypes) == 4 and (restype, argtypes) == _lib.SIGNATURES["rmhip_matmul"]
    assert _lib.SERVES["rmhip_complex_matmul"] == ("matmul",)
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "complex_matmul", None))


def test_the_mirrors_carry_the_entry_point():
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    header = (ROOT / "include" / "rmhip.h").read_text()
    assert "rmhip_complex_matmul(ctx_" in hpp and "rmhip_complex_matmul(self.ctx" in shim and "pub fn rmhip_complex_matmul(" in sys_rs
    assert re.search(r"/\* @serves matmul \*/\nRMHIP_API int rmhip_complex_matmul\(", header)
    section = header[header.index("complex-interleaved storage (fft.hip)"):header.index("RMHIP_API int rmhip_storage(")]
    assert "rmhip_complex_matmul" in section  # the list of complex-capable entry points
    assert "cgemm.hip" in (ROOT / "runmat_amd" / "csrc" / "Makefile").read_text().split("SRCS_HIP :=")[1].splitlines()[0].split()
    src = re.sub(r"//[^\n]*", "", (ROOT / "runmat_amd" / "csrc" / "cgemm.hip").read_text())
    assert "k_cgemm_split_b" in src and "k_cgemm_join" in src and "atomic" not in src and "__shared__" not in src


def test_the_shim_dispatches_on_the_storage_of_either_operand():
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index("fn matmul<'a>(&'a self"):]
    body = body[:re.search(r"\n    fn ", body).start()]
    rule = body.index("if !Self::is_complex(a) && !Self::is_complex(b)")
    real, cplx = body.index("rmhip_matmul(self.ctx"), body.index("rmhip_complex_matmul(self.ctx")
    assert rule < real < body.index("self.handle(out)") < body.index("} else {") < cplx < body.index("self.complex_handle(out)")


def test_the_reference_on_2d_shapes_is_the_scalar_loops():
    rng = np.random.default_rng(40)
    for kind in ref.KINDS:
        for m, n, k in [(1, 1, 1), (5, 4, 3), (3, 7, 6)]:
            args = ref.operands(rng, kind, (m, k), (k, n))
            for g, w in zip(ref.cmatmul_host(*args), ref.cmatmul_scalar(*args)):
                assert g.shape == w.shape == (m, n) and np.array_equal(bits(g), bits(w))


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("m,n,k", GPU_SHAPES, ids=lambda v: str(v))
def test_embed_model_within_the_gate_and_exact_on_gaussian_integers(kind, m, n, k):
    """The worst ratio is printed: the embedding in an order of its own is expected well inside the gate the GPU tests hold the device
    to."""
    rng = np.random.default_rng(1000 * kind + m + n + k)
    args = ref.operands(rng, kind, (m, k), (k, n))
    want, got, g = ref.cmatmul_host(*args), ref.embed_model(*args), ref.gate(*args)
    worst = []
    for x, w, b in zip(got, want, g):
        assert x.shape == w.shape == b.shape == (m, n)
        assert np.all(np.abs(x - w) <= b)
        worst.append(float(np.max(np.abs(x - w) / b)))
    print(f"kind {kind} {m}x{n}x{k}: worst |embed - host| / gate: re {worst[0]:.3f} im {worst[1]:.3f}")
    args = ref.operands(rng, kind, (m, k), (k, n), ints=True)  # parts in -4..4: partial sums below 2^53 at every k used
    for x, w in zip(ref.embed_model(*args), ref.cmatmul_host(*args)):
        assert np.array_equal(bits(x), bits(w))
    # precision 32: the model's value is an f32 value within the gate plus one f32 ulp of the reference part
    for x, w, b in zip(ref.embed_model(*args, r32=True), ref.cmatmul_host(*args), g):
        assert np.array_equal(x, ref.f32_round(x)) and np.array_equal(x, ref.f32_round(w))


def test_mixed_kinds_keep_an_inf_in_the_model():
    Ar, Ai = np.array([[np.inf, 1.0]]), np.array([[2.0, np.inf]])
    Br = np.array([[3.0], [5.0]])
    for f in (ref.cmatmul_host, ref.embed_model):
        re_, im_ = f(Ar, Ai, Br, None)
        assert re_[0, 0] == np.inf and im_[0, 0] == np.inf
        re_, im_ = f(Br.T.copy(), None, Ar.T.copy(), Ai.T.copy())
        assert re_[0, 0] == np.inf and im_[0, 0] == np.inf


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from test_host_plan import compile_check

    exe = compile_check(tmp_path_factory.mktemp("cgemm_route_check"), "cgemm_route_check")

    def run(cases):
        text = "".join(f"{kind} {m} {n} {k} {int(r32)}\n" for kind, m, n, k, r32 in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases), r.stdout
        return lines

    return run


def test_plan_cgemm_returns_the_table_and_a_real_product_with_a_kernel(plan):
    extra = [(31, 31, 31), (1, 33, 1), (4096, 4096, 4096), (1, 1, 100000), (70000, 3, 2)]
    cases = [(kind, m, n, k, r32) for kind in ref.KINDS for (m, n, k) in GPU_SHAPES + extra for r32 in (False, True)]
    for case, line in zip(cases, plan(cases)):
        left, right = line.split(" | ")
        w = left.split()
        got = dict(route=w[0], **{key: int(v) for key, v in zip(("M", "N", "K", "lda", "ldb", "split_b", "join", "workspace"), w[1:])})
        want = ref.expected_plan(*case)
        assert got == want, (case, got, want)
        kernel, splits = right.split()
        kind, m, n, k, _ = case
        if want["route"] == "small":
            assert (kernel, splits) == ("-", "0")
        else:
            assert kernel in ("small", "w8", "w8g", "w4") and int(splits) >= 1, (case, line)
            assert want["workspace"] <= 2 * k * n + 4 * m * n  # the stated memory cost beyond the result
    # split-K serves the long-k shape of the GPU tests in every kind
    for line in plan([(kind, 64, 64, 2048, False) for kind in ref.KINDS]):
        assert int(line.split()[-1]) > 1, line


def test_plan_cgemm_refuses_an_embedded_extent_of_2_32(plan):
    big = 1 << 31
    lines = plan([(0, big, 40, 40, False), (1, big, 40, 40, False), (2, big, 40, 40, False), (2, 40, big, 40, False), (1, 40, big, 40, False),
                  (1, 40, 40, 1 << 32, False), (0, big - 1, 40, 40, False)])
    refused = [ln.startswith("unsupported: ") for ln in lines]
    assert refused == [True, True, False, True, False, True, False], lines
