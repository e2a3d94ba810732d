"""CPU checks of `rmhip_cond_norm` and `rmhip_linsolve_rcond`: the reference the GPU tests use (tests/cond_forms_ref.py) reproduces the
reference's own KATs and agrees with a second CPU evaluation far inside the GPU tests' gate; and both entry points are bound in every
mirror, dispatched by the shim as INTEGRATION.md says, without changing the served set."""
import re
from pathlib import Path

import numpy as np
import pytest

import cond_forms_ref as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def test_the_reference_reproduces_the_kats(oracle):
    for name, a, norm, want in ref.EXACT:
        assert abs(ref.cond_ref(oracle, a, norm) - want) <= 1e-12, name
    for name, a in ref.SINGULAR:
        for norm in ref.NORMS:
            assert ref.cond_ref(oracle, a, norm) == np.inf, (name, norm)
    assert ref.cond_ref(oracle, np.zeros((0, 3)), "one") == 0.0
    for v, want in ref.SCALARS:
        assert ref.cond_ref(oracle, np.array([[v]]), "fro") == want
    with pytest.raises(ValueError, match="must be square"):
        ref.cond_ref(oracle, ref.NON_SQUARE, "inf")
    assert oracle.inv(ref.TINY_PIVOT) is not None  # the host's LU answers with rounding noise: not a singular verdict
    assert ref.rcond_ref(np.zeros((3, 3))) == 0.0 and ref.rcond_ref(np.diag([2.0, 2.0])) == 1.0
    assert ref.rcond_ref(ref.rank_deficient()) <= 20 * ref.EPS


def test_the_recorded_values_are_the_oracles(oracle):
    """tests/golden/cond_forms_ref.json against the oracle, bit for bit, at every order up to LIVE_MAX (the larger ones take the oracle's
    single-threaded inverse half a minute each); ref.recorded() itself ties every entry to today's matrices and slab width."""
    rec = ref.recorded()
    assert len(rec) == len(ref.orders()) * len(ref.KINDS)
    for case in ref.generated():
        if case.a.shape[0] <= ref.LIVE_MAX:
            assert ref.cond_ref_all(oracle, case.a) == rec[case.name], case.name


def test_two_cpu_evaluations_agree_within_the_gate():
    """Every generated case, all three norms: the oracle's composition against LAPACK's inverse.  The worst ratio is printed; the GPU tests'
    gate is n eps kappa ref, and two correct evaluations are expected well inside it."""
    worst, rec = 0.0, ref.recorded()
    for case in ref.generated():
        n = case.a.shape[0]
        for norm in ref.NORMS:
            want, other = rec[case.name][norm], ref.cond_numpy(case.a, norm)
            assert np.isfinite(want) and want >= 1.0, (case.name, norm, want)
            ratio = abs(other - want) / ref.gate(n, want)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case.name, norm, want, other, ratio)
    print(f"worst |numpy - oracle| / (n eps kappa ref) = {worst:.3f}")


def test_the_entry_points_are_bound_and_the_served_set_unchanged():
    from runmat_amd import HipProvider, _lib

    assert _lib.SERVES["rmhip_cond_norm"] == ("cond",)
    assert _lib.SERVES["rmhip_linsolve_rcond"] == ("linsolve",)
    assert _lib.SIGNATURES["rmhip_cond_norm"] == _lib.SIGNATURES["rmhip_cond"]
    assert _lib.SIGNATURES["rmhip_linsolve_rcond"] == _lib.SIGNATURES["rmhip_linsolve"]
    served = set()
    for methods in _lib.SERVES.values():
        served.update(methods)
    assert len(served) == 230, len(served)
    assert callable(getattr(HipProvider, "cond_norm", None)) and callable(getattr(HipProvider, "linsolve_rcond", None))


def _shim_body(shim: str, name: str) -> str:
    body = shim[shim.index(f"fn {name}<"):]
    return body[:re.search(r"\n    fn ", body).start()]


def test_the_mirrors_carry_the_entry_points():
    hpp = (ROOT / "include" / "rmhip_provider.hpp").read_text()
    kats = (ROOT / "examples" / "provider_kats.cpp").read_text()
    sys_rs = (ROOT / "shim" / "rmhip_sys.rs").read_text()
    py = (ROOT / "runmat_amd" / "provider.py").read_text()
    for name in ("cond_norm", "linsolve_rcond"):
        assert f" {name}(" in hpp and f"p.{name}(" in kats and f"pub fn rmhip_{name}(" in sys_rs and f"def {name}(" in py, name
    assert "kCondSlabCols" in (ROOT / "runmat_amd" / "csrc" / "cond_norm.hip").read_text() and 1 <= ref.slab_cols() <= 1024
    assert "cond_norm.hip" in (ROOT / "runmat_amd" / "csrc" / "Makefile").read_text()


def test_the_shim_dispatches_on_the_norm_and_on_rcond():
    shim = (ROOT / "shim" / "hip_provider.rs").read_text()
    cond = _shim_body(shim, "cond")
    assert "rmhip_cond(self.ctx" in cond and "rmhip_cond_norm(self.ctx" in cond
    two = cond.index("ProviderCondNorm::Two)")  # the condition of the dispatch, after the code table
    assert two < cond.index("rmhip_cond(self.ctx") < cond.index("} else {") < cond.index("rmhip_cond_norm(self.ctx")
    lin = _shim_body(shim, "linsolve")
    assert "rmhip_linsolve(self.ctx" in lin and "rmhip_linsolve_rcond(self.ctx" in lin
    assert "let triangular = o.lower || o.upper;" in lin
    rule = lin.index("if !triangular && (o.need_rcond || o.rcond.is_some())")
    assert rule < lin.index("rmhip_linsolve_rcond(self.ctx") < lin.index("} else {") < lin.index("rmhip_linsolve(self.ctx")
