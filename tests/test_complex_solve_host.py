"""CPU checks of `rmhip_complex_mldivide` / `_mrdivide` / `_inv`: the entry points are bound in every mirror without changing the served
set, the shim chooses them by the storage of either operand, the embedding the library runs (tests/complex_solve_ref.py) gives the
reference's solution and doubles its singular values, and plan_csolve (csolve_plan.h), run through tests/cpp/csolve_plan_check.cpp,
returns the fields of that file's table, counts the tolerance in complex dimensions and refuses what the real solve cannot take."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import complex_solve_ref as ref

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"rmhip_complex_mldivide": "mldivide", "rmhip_complex_mrdivide": "mrdivide", "rmhip_complex_inv": "inv"}


def test_the_entry_points_are_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    for name, hook in ENTRIES.items():
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["rmhip_" + hook]  # the sibling's signature
        assert _lib.SERVES[name] == (hook,)
        assert callable(getattr(HipProvider, name[len("rmhip_"):], None))
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)


def test_the_mirrors_carry_the_entry_points():
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    header = (ROOT / "include" / "rmhip.h").read_text()
    section = header[header.index("complex-interleaved storage (fft.hip)"):header.index("RMHIP_API int rmhip_storage(")]
    for name, hook in ENTRIES.items():
        assert f"{name}(ctx_" in hpp and f"{name}(self.ctx" in shim and f"pub fn {name}(" in sys_rs, name
        assert re.search(r"/\* @serves %s \*/\nRMHIP_API int %s\(" % (hook, name), header), name
        assert name in section, name  # the list of complex-capable entry points
    assert "csolve.hip" in (ROOT / "runmat_amd" / "csrc" / "Makefile").read_text().split("SRCS_HIP :=")[1].splitlines()[0].split()
    src = re.sub(r"//[^\n]*", "", (ROOT / "runmat_amd" / "csrc" / "csolve.hip").read_text())
    for kernel in ("k_csolve_embed", "k_csolve_stack", "k_csolve_join"):
        assert kernel in src
    assert "atomic" not in src and "__shared__" not in src


@pytest.mark.parametrize("hook,args", [("mldivide", ("lhs", "rhs")), ("mrdivide", ("lhs", "rhs")), ("inv", ("matrix",))])
def test_the_shim_dispatches_on_the_storage_of_either_operand(hook, args):
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    body = shim[shim.index(f"fn {hook}<'a>(&'a self"):]
    body = body[:re.search(r"\n    fn ", body).start()]
    rule = body.index("if " + " && ".join(f"!Self::is_complex({a})" for a in args))
    real, cplx = body.index(f"rmhip_{hook}(self.ctx"), body.index(f"rmhip_complex_{hook}(self.ctx")
    assert rule < real < body.index("self.handle(out)") < body.index("} else {") < cplx < body.index("self.complex_handle(out)")


@pytest.mark.parametrize("m,n,k", [(2, 2, 1), (3, 3, 2), (5, 2, 3), (2, 5, 1)], ids=str)
def test_the_embedded_real_solve_is_the_complex_solve(m, n, k):
    """lstsq on E(A) and [br; bi], re-joined, against solve_ref on the complex system: least squares (tall) and minimum norm (wide)
    included.  Both are backward stable on Gaussian operands (cond below ~1e2 at these sizes): 1e-12 relative leaves three digits."""
    rng = np.random.default_rng(10 * m + n + k)
    for kind in ref.KINDS:
        Ar, Ai, Br, Bi = ref.operands(rng, kind, m, n, k)
        want = ref.solve_ref(ref.as_complex(Ar, Ai), ref.as_complex(Br, Bi))
        Areal = ref.embed(Ar, Ai) if kind != 2 else Ar
        T = np.linalg.lstsq(Areal, ref.stack(kind, Br, Bi), rcond=None)[0]
        got = ref.join(kind, T, n, k)
        assert got.shape == want.shape == (n, k)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want)))), kind
    # the singular values of E(A) are A's, each twice
    Ar, Ai, _, _ = ref.operands(rng, 0, m, n, k)
    s = np.linalg.svd(Ar + 1j * Ai, compute_uv=False)
    se = np.linalg.svd(ref.embed(Ar, Ai), compute_uv=False)
    assert se.shape == (2 * min(m, n),) and np.allclose(se, np.repeat(s, 2), rtol=1e-13, atol=0)


def test_the_embedding_layout_and_the_join():
    Ar, Ai = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), np.array([[0.5, 0.0], [-1.0, 7.0], [0.0, 8.0]])
    E = ref.embed(Ar, Ai)
    assert E.shape == (6, 4) and np.array_equal(E[:3, :2], Ar) and np.array_equal(E[3:, :2], Ai)
    assert np.array_equal(E[:3, 2:], -Ai) and np.array_equal(E[3:, 2:], Ar)
    assert np.signbit(E[0, 3]) and not np.signbit(E[3, 1])  # -Ai keeps the sign of a zero: the kernel negates, it does not subtract
    x = np.array([[1.0 + 2.0j], [3.0 - 1.0j]])
    b = (Ar + 1j * Ai) @ x
    assert np.allclose(E @ np.concatenate([x.real, x.imag]), np.concatenate([b.real, b.imag]), rtol=1e-15)
    assert np.array_equal(ref.join(0, np.concatenate([x.real, x.imag]), 2, 1), x)
    assert np.array_equal(ref.join(2, np.concatenate([x.real, x.imag], axis=1), 2, 1), x)


def test_the_tolerance_window_of_the_gpu_test():
    """n = 8, A = Q diag(1, ..., 1, 1.5 n eps): the smallest singular value of A and the two smallest of E(A) lie inside
    (n eps, 2n eps), so the reference (tolerance from n) keeps the value and a tolerance from 2n would drop it."""
    A = ref.tolerance_case()
    n = A.shape[0]
    s = np.linalg.svd(A, compute_uv=False)
    se = np.linalg.svd(ref.embed(A.real, A.imag), compute_uv=False)
    print("smallest singular values in units of n eps:", s[-1] / (n * ref.EPS), se[-2:] / (n * ref.EPS))
    for v in (s[-1], se[-1], se[-2]):
        assert 1.2 * n * ref.EPS < v < 1.8 * n * ref.EPS
    assert max(s[0], se[0]) <= 1.0 + 1e-12
    b = np.ones((n, 1), dtype=np.complex128)
    keep, drop = ref.solve_ref(A, b), ref.solve_ref(A, b, tol_dim=2 * n)
    assert np.linalg.norm(keep) > 1e6 * np.linalg.norm(drop)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from test_host_plan import compile_check

    exe = compile_check(tmp_path_factory.mktemp("csolve_plan_check"), "csolve_plan_check")

    def run(cases):
        text = "".join(" ".join(str(v) for v in case) + "\n" for case in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases), r.stdout
        return lines

    return run


def test_plan_csolve_returns_the_table(plan):
    shapes = [(n, n, k) for n, k in ref.SQUARE_SHAPES] + ref.RECT_SHAPES + [(n, n, n) for n in ref.INV_ORDERS] + [(8192, 8192, 1)]
    cases = [(entry, kind, m, n, k) for entry in (ref.MLDIVIDE, ref.MRDIVIDE) for kind in ref.KINDS for (m, n, k) in shapes]
    cases += [(ref.INV, 0, n, n, n) for n in ref.INV_ORDERS]
    keys = ("M", "N", "NRHS", "embed_a", "transpose_a", "tol_dim", "a_workspace", "workspace", "result")
    for case, line in zip(cases, plan(cases)):
        got = dict(zip(keys, (int(v) for v in line.split())))
        assert got == ref.expected_plan(*case), (case, got)
        entry, kind, m, n, k = case
        assert got["tol_dim"] == max(m, n)  # the complex dimensions, not the embedded ones
        stated = (4 * m * n + 2 * m * k) if kind != 2 else 2 * m * k + (m * n if entry == ref.MRDIVIDE else 0)  # include/rmhip.h
        assert got["workspace"] <= stated and got["result"] == 2 * n * k


def test_plan_csolve_refuses_what_the_real_solve_cannot_take(plan):
    big = 1 << 30  # 2 * big = 2^31: one past the LU's largest dimension
    lines = plan([(0, 0, big, 4, 1), (0, 1, 4, big, 1), (0, 2, 2 * big - 1, 4, 1), (0, 2, 2 * big, 4, 1), (0, 0, big - 1, 4, 1),
                  (0, 0, 4, 4, 65536), (0, 0, 4, 4, 65535), (0, 2, 4, 4, 32768), (0, 2, 4, 4, 32767), (1, 0, 4, big, 2), (2, 0, big, big, big)])
    refused = [ln.startswith("unsupported: ") for ln in lines]
    assert refused == [True, True, False, True, False, True, False, True, False, True, True], lines
    assert "2^31" in lines[0] and "65535 right-hand sides" in lines[5]
