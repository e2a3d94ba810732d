"""GPU checks of `cond_norm` (rmhip_cond_norm, runmat_amd/csrc/cond_norm.hip) and `linsolve_rcond` (rmhip_linsolve_rcond, solve.cpp).

cond: every generated case of tests/cond_forms_ref.py in the three norms against the oracle's composition, within
|got - ref| <= n eps kappa_p ref with kappa_p = ref - the first-order forward bound of an LU inverse with constant 1, not a fitted number
(two CPU evaluations differ by a small fraction of it, tests/test_cond_forms_host.py).  The orders straddle the slab width read from the
source: one slab, exactly one, one and a column, two and three columns.  rcond: 1e-10 relative against numpy's SVD, the tolerance
test_rank_cond_pinv applies to the same decomposition, and the solution bit for bit the plain call's."""
import numpy as np
import pytest

import cond_forms_ref as ref

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_SINGULAR = 1, 2, 7


@pytest.fixture(scope="module")
def truth(oracle):
    """case -> {norm: the oracle's value}: recomputed here up to order LIVE_MAX, read from the recorded file above it (the oracle's
    inverse is a single-threaded loop; tests/test_cond_forms_host.py pins the file to the oracle)."""
    rec = ref.recorded()

    def get(case):
        return ref.cond_ref_all(oracle, case.a) if case.a.shape[0] <= ref.LIVE_MAX else rec[case.name]
    return get


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(0, precision="F32")
    yield p
    p.close()


def live(prov):
    t = prov.telemetry_snapshot()
    return t["bytes_allocated"] - t["bytes_pooled"]


def cond_of(prov, h, norm):
    out = prov.cond_norm(h, norm)
    assert tuple(out.shape) == (1, 1)
    v = float(prov.download(out)[0])
    prov.free(out)
    return v


def declined(prov, call, code=ERR_UNSUPPORTED, text=None):
    from runmat_amd import ProviderError

    mark = live(prov)
    with pytest.raises(ProviderError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    if text is not None:
        assert text in str(e.value), str(e.value)
    assert live(prov) == mark  # nothing left behind
    return str(e.value)


@pytest.mark.parametrize("n, kind", ref.case_keys())
def test_cond_values_within_the_forward_bound(prov, truth, n, kind):
    case = ref.case(n, kind)
    h = prov.upload(case.a)
    want = truth(case)
    for norm in ref.NORMS:
        got = cond_of(prov, h, norm)
        ratio = abs(got - want[norm]) / ref.gate(n, want[norm])
        print(f"cond_norm {case.name} {norm}: got {got:.17g} ref {want[norm]:.17g} ratio {ratio:.4f}")
        assert ratio <= 1.0, (case.name, norm, got, want[norm], ratio)
    prov.free(h)


def test_cond_exact_cases(prov):
    for name, a, norm, want in ref.EXACT:
        assert abs(cond_of(prov, prov.upload(a), norm) - want) <= 1e-12, name
    for name, a in ref.SINGULAR:
        for norm in ref.NORMS:
            assert cond_of(prov, prov.upload(a), norm) == np.inf, (name, norm)
    for norm in ref.NORMS:
        assert cond_of(prov, prov.upload(np.zeros((0, 3))), norm) == 0.0
        for v, want in ref.SCALARS:
            assert cond_of(prov, prov.upload(np.array([[v]])), norm) == want, (v, norm)


def test_cond_declines_and_leaves_nothing_behind(prov, oracle):
    tiny, bad, rect = prov.upload(ref.TINY_PIVOT), prov.upload(ref.with_inf()), prov.upload(ref.NON_SQUARE)
    assert oracle.inv(ref.TINY_PIVOT) is not None  # the host's answer for what is declined here is a number, not Inf
    for norm in ref.NORMS:
        declined(prov, lambda: prov.cond_norm(tiny, norm), text="pivot 3")
        declined(prov, lambda: prov.cond_norm(bad, norm), text="non-finite")
        declined(prov, lambda: prov.cond_norm(rect, norm), ERR_INVALID, ref.SQUARE_TEXT)
    declined(prov, lambda: prov.cond_norm(tiny, "two"), text="rmhip_cond")
    cube, z = prov.upload(np.zeros((2, 2, 2))), prov.complex_from_real(prov.upload(np.eye(2)))
    declined(prov, lambda: prov.cond_norm(cube, "one"), ERR_INVALID, "2-D matrices or vectors")
    declined(prov, lambda: prov.cond_norm(z, "one"), text="real tensors")


def test_cond_is_deterministic_and_cleans_up(prov):
    n = ref.slab_cols() + 1
    a = ref.matrix(n, "plain")
    h = prov.upload(a)
    before = live(prov)
    first = prov.cond_norm(h, "one")
    one_output = live(prov) - before  # what a [1, 1] result holds (the pool's smallest block)
    prov.free(first)
    assert one_output > 0 and live(prov) == before
    mark = live(prov)
    for norm in ref.NORMS:
        o1, o2 = prov.cond_norm(h, norm), prov.cond_norm(h, norm)
        assert live(prov) == mark + 2 * one_output  # the earlier count plus the outputs, nothing else
        assert prov.download(o1).view(np.uint64)[0] == prov.download(o2).view(np.uint64)[0], norm
        prov.free(o1)
        prov.free(o2)
        assert live(prov) == mark
    assert np.array_equal(prov.download_matrix(h).view(np.uint64), a.view(np.uint64))  # the operand is unchanged
    prov.free(h)


def test_cond_on_a_precision_32_provider(prov32, oracle):
    n = 65
    a32 = ref.matrix(n, "dominant").astype(np.float32).astype(np.float64)
    h = prov32.upload(a32)
    for norm in ref.NORMS:
        want = ref.cond_ref(oracle, a32, norm)
        got = cond_of(prov32, h, norm)
        assert got == float(np.float32(got))  # stored as f32
        err, bound = abs(got - want), ref.gate(n, want) + 2.0 ** -24 * want
        print(f"cond_norm f32 {norm}: got {got:.9g} ref {want:.17g} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (norm, got, want)
    prov32.free(h)


def solve(prov, entry, a, b, **opts):
    from runmat_amd import ProviderLinsolveOptions

    ha, hb = prov.upload(a), prov.upload(b)
    res = entry(ha, hb, ProviderLinsolveOptions(**opts))
    x = prov.download_matrix(res.solution)
    for h in (res.solution, ha, hb):
        prov.free(h)
    return x, res.reciprocal_condition


def test_linsolve_rcond_values(prov):
    x, r = solve(prov, prov.linsolve_rcond, 2.0 * np.eye(2), np.ones((2, 1)), need_rcond=True)
    assert r == 1.0 and np.array_equal(x, [[0.5], [0.5]])
    rng = np.random.default_rng(405030)
    for m, n in ((40, 40), (50, 30), (30, 50)):
        a = rng.standard_normal((m, n))
        for transposed in (False, True):
            b = rng.standard_normal((n if transposed else m, 3))
            want = ref.rcond_ref(a.T if transposed else a)
            x, r = solve(prov, prov.linsolve_rcond, a, b, need_rcond=True, transposed=transposed)
            plain, nan = solve(prov, prov.linsolve, a, b, transposed=transposed)
            print(f"linsolve_rcond {m}x{n} transposed={transposed}: rcond {r:.17g} ref {want:.17g}")
            assert abs(r - want) <= 1e-10 * want, (m, n, transposed, r, want)
            assert np.isnan(nan) and np.array_equal(x.view(np.uint64), plain.view(np.uint64)), (m, n, transposed)
    a, b = ref.rank_deficient(20, 10), rng.standard_normal((20, 2))
    x, r = solve(prov, prov.linsolve_rcond, a, b, need_rcond=True)
    plain, _ = solve(prov, prov.linsolve, a, b)
    assert 0.0 <= r <= 20 * ref.EPS and np.array_equal(x.view(np.uint64), plain.view(np.uint64))


def test_linsolve_rcond_thresholds_and_refusals(prov):
    from runmat_amd import ProviderLinsolveOptions

    a, b = prov.upload(np.diag([1.0, 1e-9])), prov.upload(np.ones((2, 1)))
    declined(prov, lambda: prov.linsolve_rcond(a, b, ProviderLinsolveOptions(rcond=1e-6)), ERR_SINGULAR, ref.SINGULAR_TEXT)
    res = prov.linsolve_rcond(a, b, ProviderLinsolveOptions(rcond=1e-12))
    assert abs(res.reciprocal_condition - 1e-9) <= 1e-10 * 1e-9
    assert np.allclose(prov.download_matrix(res.solution), [[1.0], [1e9]], rtol=1e-12, atol=0.0)
    prov.free(res.solution)
    declined(prov, lambda: prov.linsolve_rcond(a, b, ProviderLinsolveOptions(lower=True, need_rcond=True)), text="rmhip_linsolve")
    declined(prov, lambda: prov.linsolve_rcond(a, b, ProviderLinsolveOptions()), text="rmhip_linsolve")


def test_the_siblings_decline_as_before(prov):
    from runmat_amd import ProviderLinsolveOptions

    eye = prov.upload(np.eye(3))
    declined(prov, lambda: prov.cond(eye, "fro"))
    a, b = prov.upload(np.array([[2.0, 1.0], [1.0, 3.0]])), prov.upload(np.ones((2, 1)))
    declined(prov, lambda: prov.linsolve(a, b, ProviderLinsolveOptions(need_rcond=True)))
