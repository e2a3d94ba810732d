"""The executors' call SEQUENCES for the special fusion patterns on the device: `execute_centered_gram`,
`execute_power_step_normalize`, `execute_explained_variance`, `execute_image_normalize` and `execute_matmul_epilogue` of
planner_exec.py (crates/runmat-accelerate/src/fusion_exec.rs:630-1206) driving librmhip.so.  The per-hook tests of
test_gpu_parity.py call every hook with fresh, plain, resident operands; here the hooks run in the order RunMat issues them, on
owned and borrowed operands, on views, on a lazy `random_normal`, and on one handle id that is reshaped twice in between.

Every sequence is checked two ways:
  * bit equality with the same hooks called one by one on fresh, plain, resident uploads of the same values - a sequence must not
    change arithmetic.  It holds wherever the operand is plain by the time the kernel reads it; where `matmul` consumes a
    transpose view in place (another kernel variant, another summation order) only the bound applies, and the case says so;
  * a bound against a high-precision reference of the whole composition: the per-hook tests' own bounds
    (test_gpu_parity.py: covariance, matmul_power_step, image_normalize, matmul_epilogue), and for the chained products of
    ExplainedVariance the first-order inner-product bound applied twice, 2 (n + 4) eps (|Qr| |G| |Q|).
test_exec_sequences_host.py is the CPU twin (call order, descriptors, accounting) on the oracle-backed double."""
import os

import numpy as np
import pytest

from planner_exec import (CallRecorder, derive_matmul_epilogue, execute_centered_gram, execute_explained_variance,
                          execute_image_normalize, execute_matmul_epilogue, execute_power_step_normalize)
from planner_requests import FusionGroupPlan, matmul_epilogue_plans
from test_exec_sequences_host import epilogue_values, explained_variance_bound, explained_variance_reference

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
U32 = 2.0 ** -24  # unit roundoff of f32 storage
NOT_FOUND = 5


def f32r(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def prov32(built):
    from runmat_amd import HipProvider

    p = HipProvider(int(os.environ.get("RMHIP_TEST_DEVICE", "0")), precision="F32")
    yield p
    p.close()


@pytest.fixture()
def lazy(prov):
    """Lazy `random_normal` handles from 2 elements on for the test, the library's default restored afterwards."""
    prov.set_lazy_random(True, 2)
    yield prov
    prov.set_lazy_random(True, 1024)


def table_shape(prov, h):
    """The shape the LIBRARY keeps for this id (a Python handle carries its own copy)."""
    return prov._handle(h.buffer_id).shape


def assert_intact(prov, h, values):
    """The id still answers, the library's record of its shape is the values' shape, and the bytes are the same."""
    assert table_shape(prov, h) == values.shape, "stale shape after the sequence"
    assert same_bits(prov.download(prov._handle(h.buffer_id)).reshape(values.shape, order="F"), values)


def assert_gone(prov, handles):
    from runmat_amd import ProviderError
    for h in handles:
        with pytest.raises(ProviderError) as e:
            prov.download(h)
        assert e.value.code == NOT_FOUND


def assert_accounted(prov, rec, result):
    """Everything the sequence uploaded or created, except its result, was freed exactly once and is gone."""
    made = [h.buffer_id for h in rec.created]
    assert len(set(made)) == len(made)
    assert sorted(rec.freed) == sorted(set(made) - ({result.buffer_id} if result is not None else set()))
    assert_gone(prov, [h for h in rec.created if result is None or h.buffer_id != result.buffer_id])


def free_all(prov, handles):
    for h in handles:
        prov.free(h)


class Operand:
    """One operand of a sequence: `value` is what the executor receives (a handle or a host array), `array` its values, `watch`
    the (handle, values) pairs that must read back unchanged afterwards (the operand itself when resident, a view's base, a
    second live view of the same base), `keep` everything the test frees at the end."""

    def __init__(self, value, array, watch=(), keep=()):
        self.value, self.array, self.watch, self.keep = value, array, list(watch), list(keep)


def make_operand(prov, kind, X):
    if kind == "host":
        return Operand(X, X)
    if kind == "resident":
        h = prov.upload(X)
        return Operand(h, X, [(h, X)], [h])
    if kind == "tview":  # transpose(base) as a live view; the caller keeps the base and a second view of it
        base = prov.upload(np.ascontiguousarray(X.T))
        view, other = prov.transpose(base), prov.transpose(base)
        return Operand(view, X, [(view, X), (base, np.ascontiguousarray(X.T)), (other, X)], [view, other, base])
    if kind == "repmat11":  # repmat(X, [1, 1]): the same bytes under a second id
        base = prov.upload(X)
        view = prov.repmat(base, (1, 1))
        return Operand(view, X, [(view, X), (base, X)], [view, base])
    raise ValueError(kind)


# =====================================================================================================================
# ExplainedVariance
# =====================================================================================================================
EV_SIZES = [1, 2, 3, 17, 64, 65, 129, 257]  # one element; the 64 x 64 tile at and past a tile; the 128-wide tile at and past one
EV_VARIANTS = ["resident", "host", "tview_q", "tview_g", "tview_both", "repmat11", "repmat_columns_q", "repmat_scalar_g",
               "lazy_q", "same_handle"]


def ev_operands(prov, variant, n):
    rng = np.random.default_rng(1000 + n)
    Q, G = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))  # asymmetric with probability one
    if variant == "same_handle":
        q = make_operand(prov, "resident", Q)
        return q, Operand(q.value, Q)
    if variant == "repmat_columns_q":  # a real lazy repmat view: an n x 1 column tiled to n x n (every column the same, Q != Q')
        col = rng.uniform(-1, 1, (n, 1))
        base = prov.upload(col)
        view = prov.repmat(base, (1, n))
        Qv = np.tile(col, (1, n))
        return Operand(view, Qv, [(view, Qv), (base, col)], [view, base]), make_operand(prov, "resident", G)
    if variant == "repmat_scalar_g":  # a 1 x 1 tensor tiled up to n x n
        base = prov.upload(np.array([[0.625]]))
        view = prov.repmat(base, (n, n))
        Gv = np.full((n, n), 0.625)
        return make_operand(prov, "resident", Q), Operand(view, Gv, [(view, Gv), (base, np.array([[0.625]]))], [view, base])
    if variant == "lazy_q":  # Q from random_normal on a lazy-enabled provider: no storage until the first matmul reads it
        state = 0x51ED270B ^ (n * 7919)
        prov.set_lazy_random(False, 2)
        prov.set_rng_state(state)
        eager = prov.random_normal((n, n))
        Qv = prov.download_matrix(eager)
        prov.free(eager)
        prov.set_lazy_random(True, 2)
        prov.set_rng_state(state)
        before = prov.lazy_random_stats()["created"]
        h = prov.random_normal((n, n))
        assert prov.lazy_random_stats()["created"] - before == (1 if n * n >= 2 else 0)
        return Operand(h, Qv, [(h, Qv)], [h]), make_operand(prov, "resident", G)
    kinds = {"resident": ("resident", "resident"), "host": ("host", "host"), "tview_q": ("tview", "resident"),
             "tview_g": ("resident", "tview"), "tview_both": ("tview", "tview"), "repmat11": ("repmat11", "repmat11")}[variant]
    return make_operand(prov, kinds[0], Q), make_operand(prov, kinds[1], G)


def ev_one_by_one(prov, Q, G):
    """The same hooks on fresh, plain, resident uploads: (Q as [c, r]) * G, * Q, diag."""
    hq, hg = prov.upload(Q), prov.upload(G)
    hqr = prov.upload(Q.reshape(-1, order="F"), (Q.shape[1], Q.shape[0]))
    tmp = prov.matmul(hqr, hg)
    product = prov.matmul(tmp, hq)
    diag = prov.diag_extract(product, 0)
    out = prov.download(diag)
    free_all(prov, [hq, hg, hqr, tmp, product, diag])
    return out


@pytest.mark.parametrize("variant", EV_VARIANTS)
@pytest.mark.parametrize("n", EV_SIZES)
def test_explained_variance_sequence(lazy, n, variant):
    from runmat_amd import ProviderError

    prov = lazy
    q, g = ev_operands(prov, variant, n)
    q_id = q.value.buffer_id if not isinstance(q.value, np.ndarray) else None
    rec = CallRecorder(prov)
    if n == 1:
        # a 1 x 1 product is vector-like: diag_extract refuses it as the reference's does (simple_provider.rs:3281-3287), after
        # all three products; the sequence must still leave nothing behind and the operands as they were
        with pytest.raises(ProviderError) as e:
            execute_explained_variance(rec, q.value, g.value)
        assert e.value.code == 3 and "diag: matrix input required" in str(e.value)
        out = None
    else:
        out = execute_explained_variance(rec, q.value, g.value)
        assert out.shape == (n, 1) and table_shape(prov, out) == (n, 1)
        got = prov.download(out)
        want, bound = explained_variance_reference(q.array, g.array), explained_variance_bound(q.array, g.array)
        err = np.abs(got - want)
        print(f"explained variance n={n} {variant}: max err/bound = {np.max(err / bound):.3g}")
        assert np.all(err <= bound)
        if variant in ("tview_g", "tview_both"):
            # G is still a transpose view when the products read it: matmul consumes it in place through the
            # transposed-operand kernel, whose summation order is not the plain kernel's.  Only the bound applies.
            pass
        else:
            assert same_bits(got, ev_one_by_one(prov, q.array, g.array))
        if n >= 3:  # a real transpose instead of the reshape would be noticed: diag(Q' G Q) is far outside the bound
            wrong = np.diag(q.array.T.astype(np.longdouble) @ g.array.astype(np.longdouble) @ q.array.astype(np.longdouble))
            assert np.all(np.abs(wrong - want) > bound)
    assert_accounted(prov, rec, out)
    if q_id is not None:
        assert q.value.buffer_id == q_id
    for h, values in q.watch + g.watch:  # Q back to n x n with its bytes; bases and other live views untouched
        assert_intact(prov, h, values)
    free_all(prov, q.keep + g.keep + ([out] if out is not None else []))


def test_explained_variance_nonsquare_q_is_the_shape_error(prov):
    """fusion_gpu.rs's 4 x 2 case: the first matmul (4x2 * 4x4) is the provider's shape error; nothing the caller owns is touched."""
    from runmat_amd import ProviderError

    rng = np.random.default_rng(42)
    Q, G = rng.uniform(-1, 1, (4, 2)), rng.uniform(-1, 1, (4, 4))
    hq, hg = prov.upload(Q), prov.upload(G)
    for qv, gv in ((hq, hg), (Q, G), (hq, G)):
        rec = CallRecorder(prov)
        with pytest.raises(ProviderError) as e:
            execute_explained_variance(rec, qv, gv)
        assert e.value.code == 3 and "inner dims must agree" in str(e.value)
        assert rec.calls.count("matmul") == 1 and "reshape" not in rec.calls
        assert_accounted(prov, rec, None)
        assert_intact(prov, hq, Q)
        assert_intact(prov, hg, G)
    follow = prov.matmul(hg, hq)  # both usable in a following call
    assert same_bits(prov.download_matrix(follow), prov.download_matrix(prov.matmul(prov.upload(G), prov.upload(Q))))
    free_all(prov, [follow, hq, hg])


def test_a_stale_shape_would_be_detected(prov):
    """`assert_intact` reads the library's record: a handle left with the swapped shape fails it."""
    Q = np.random.default_rng(43).uniform(-1, 1, (5, 3))
    h = prov.upload(Q)
    assert_intact(prov, h, Q)
    prov.reshape(h, (3, 5))  # what the sequence does to Q in between
    with pytest.raises(AssertionError, match="stale shape"):
        assert_intact(prov, h, Q)
    prov.reshape(h, (5, 3))
    assert_intact(prov, h, Q)
    prov.free(h)


@pytest.mark.parametrize("n", [3, 65, 129])
def test_explained_variance_sequence_f32(prov32, prov, n, monkeypatch):
    """Precision 32 with the widen -> dgemm -> round-once products (RMHIP_F32_MATMUL=f64, as
    test_f32_matmul_solve_and_friends_use_f64_kernels_on_widened_operands runs them) against the f64 sequence on the same
    f32-rounded operands.  Two intermediates are STORED in f32, T = Qr*G and P = T*Q (the diagonal is a copy of P's):
        T32 = T (1 + d1),  P32 = (T32 * Q) (1 + d2),  |d1|, |d2| <= u = 2^-24
    so entry i of the diagonal differs from the f64 sequence's by at most
        u (|T| |Q|)_ii + u |P32_ii|
    plus what the f64 arithmetic itself contributes: the second product runs on other inputs, so its rounding errors no longer
    cancel, and T is known here only through a numpy product - both within (n + 4) eps (|Qr| |G| |Q|)_ii each, and the second-order
    u^2 |P_ii| = 16 eps |P_ii| is below (n + 4) eps (|Qr| |G| |Q|)_ii as well; 4 (n + 4) eps (|Qr| |G| |Q|)_ii covers the three."""
    monkeypatch.setenv("RMHIP_F32_MATMUL", "f64")
    rng = np.random.default_rng(2000 + n)
    Q, G = f32r(rng.uniform(-1, 1, (n, n))), f32r(rng.uniform(-1, 1, (n, n)))
    h32q, h32g, h64q, h64g = prov32.upload(Q), prov32.upload(G), prov.upload(Q), prov.upload(G)
    rec = CallRecorder(prov32)
    out32 = execute_explained_variance(rec, h32q, h32g)
    out64 = execute_explained_variance(prov, h64q, h64g)
    assert out32.shape == (n, 1) and prov32.buffer_bits(out32) == 32
    got32, got64 = prov32.download(out32), prov.download(out64)
    bound = U32 * (np.diag(np.abs(Q @ G) @ np.abs(Q)) + np.abs(got32)) + 2 * explained_variance_bound(Q, G)
    print(f"explained variance f32 n={n}: max err/bound = {np.max(np.abs(got32 - got64) / bound):.3g}")
    assert np.all(np.abs(got32 - got64) <= bound)
    assert same_bits(got32, f32r(got32))
    assert_accounted(prov32, rec, out32)
    assert_intact(prov32, h32q, Q)
    assert_intact(prov32, h32g, G)
    assert prov32.buffer_bits(h32q) == 32
    host = execute_explained_variance(prov32, Q, G)  # owned uploads: the same values
    assert same_bits(prov32.download(host), got32)
    free_all(prov32, [h32q, h32g, out32, host])
    free_all(prov, [h64q, h64g, out64])


# =====================================================================================================================
# CenteredGram
# =====================================================================================================================
def covariance_checks(prov, oracle, got, x, biased):
    """The assertions of test_gpu_parity.py::test_covariance_vs_oracle, unchanged (the symmetry also over a NaN pattern)."""
    rows, cols = x.shape
    want = oracle.covariance(x, biased)
    assert got.shape == (cols, cols) and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    if fin.any():  # tolerance: tree-ordered column means and MFMA-ordered products vs the sequential CPU loops
        assert np.max(np.abs(got[fin] - want[fin])) <= 64 * EPS * (1.0 + np.max(np.abs(want[fin]))) * np.sqrt(rows)
        assert np.array_equal(got, got.T, equal_nan=True)


def covariance_one_by_one(prov, x, biased):
    h = prov.upload(x)
    c = prov.covariance(h, biased=biased)
    out = prov.download_matrix(c)
    free_all(prov, [h, c])
    return out


@pytest.mark.parametrize("kind", ["resident", "host", "tview"])
@pytest.mark.parametrize("normalization", ["unbiased", "biased"])
@pytest.mark.parametrize("rows,cols", [(4, 3), (1, 5), (257, 129), (4096, 8)])  # the last: the tall-skinny VALU Gram kernel
def test_centered_gram_sequence(prov, oracle, rows, cols, normalization, kind):
    x = np.random.default_rng(rows * 3 + cols).uniform(-1, 1, (rows, cols))
    op = make_operand(prov, kind, x)
    rec = CallRecorder(prov)
    out = execute_centered_gram(rec, op.value, normalization)
    got = prov.download_matrix(out)
    covariance_checks(prov, oracle, got, x, normalization == "biased")
    # (a transpose view is materialised under its own id by the first step of the hook: plain by the time the kernels read it)
    assert same_bits(got, covariance_one_by_one(prov, x, normalization == "biased"))
    assert rec.calls == (["upload"] if kind == "host" else []) + ["covariance"] + (["free"] if kind == "host" else [])
    assert_accounted(prov, rec, out)
    for h, values in op.watch:
        assert_intact(prov, h, values)
    free_all(prov, op.keep + [out])


@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("rows,cols", [(257, 9), (4096, 8)])
def test_centered_gram_sequence_nonfinite(prov, oracle, rows, cols, poison):
    x = np.random.default_rng(rows + cols).uniform(-1, 1, (rows, cols))
    x[rows // 3, 2] = poison
    for value in (x, prov.upload(x)):
        rec = CallRecorder(prov)
        out = execute_centered_gram(rec, value, "unbiased")
        got = prov.download_matrix(out)
        covariance_checks(prov, oracle, got, x, False)
        assert np.isnan(got[2, :]).all() and np.isnan(got[:, 2]).all() and np.isfinite(np.delete(np.delete(got, 2, 0), 2, 1)).all()
        assert same_bits(got, covariance_one_by_one(prov, x, False))
        assert_accounted(prov, rec, out)
        prov.free(out)


# =====================================================================================================================
# PowerStepNormalize
# =====================================================================================================================
@pytest.mark.parametrize("kind", ["resident", "host", "tview_lhs_host_rhs"])
@pytest.mark.parametrize("m,k,n", [(2, 2, 2), (64, 32, 8), (257, 129, 33)])
def test_power_step_normalize_sequence(prov, oracle, m, k, n, kind):
    rng = np.random.default_rng(m + k + n)
    A, B = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (k, n))
    lhs = make_operand(prov, {"resident": "resident", "host": "host", "tview_lhs_host_rhs": "tview"}[kind], A)
    rhs = make_operand(prov, "resident" if kind == "resident" else "host", B)
    rec = CallRecorder(prov)
    out = execute_power_step_normalize(rec, lhs.value, rhs.value, 1e-12)
    got = prov.download_matrix(out)
    want = oracle.matmul_power_step(A, B, 1e-12)
    assert np.max(np.abs(got - want)) <= 64 * (k + m) * EPS  # test_gpu_parity.py::test_matmul_power_step_vs_oracle
    assert np.max(np.abs((got * got).sum(axis=0) - 1.0)) < 1e-9
    if kind != "tview_lhs_host_rhs":
        # (with lhs a transpose view the hook's own matmul consumes it in place through the transposed-operand kernel: another
        # summation order, so only the bound above applies there)
        ha, hb = prov.upload(A), prov.upload(B)
        one = prov.matmul_power_step(ha, hb, 1e-12)
        assert same_bits(got, prov.download_matrix(one))
        free_all(prov, [ha, hb, one])
    assert_accounted(prov, rec, out)
    for h, values in lhs.watch + rhs.watch:
        assert_intact(prov, h, values)
    free_all(prov, lhs.keep + rhs.keep + [out])


def test_power_step_normalize_zero_column_without_epsilon(prov, oracle):
    """A zero column of rhs gives a zero column of the product and 0 / sqrt(0 + 0): whatever the oracle yields there."""
    rng = np.random.default_rng(77)
    A, B = rng.uniform(-1, 1, (64, 32)), rng.uniform(-1, 1, (32, 8))
    B[:, 3] = 0.0
    lhs = make_operand(prov, "tview", A)
    rec = CallRecorder(prov)
    out = execute_power_step_normalize(rec, lhs.value, B, 0.0)
    got, want = prov.download_matrix(out), oracle.matmul_power_step(A, B, 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.max(np.abs(got[fin] - want[fin])) <= 64 * (32 + 64) * EPS
    assert_accounted(prov, rec, out)
    for h, values in lhs.watch:
        assert_intact(prov, h, values)
    free_all(prov, lhs.keep + [out])


# =====================================================================================================================
# ImageNormalize
# =====================================================================================================================
IMAGE_DESCRIPTORS = {"epsilon": dict(), "all": dict(gain=1.05, bias=-0.02, gamma=1.8, clamp_zero=True), "noclamp": dict(clamp_zero=False)}


@pytest.mark.parametrize("kind", ["resident", "host", "reshaped"])
@pytest.mark.parametrize("desc", sorted(IMAGE_DESCRIPTORS))
@pytest.mark.parametrize("shape", [(3, 16, 20), (1, 7, 9), (300, 4, 4)])  # the last: a batch above IN_MAX_BATCH
def test_image_normalize_sequence(prov, oracle, shape, desc, kind):
    opts = IMAGE_DESCRIPTORS[desc]
    x = np.random.default_rng(sum(shape)).uniform(-1, 1, shape)
    if kind == "reshaped":  # uploaded as a matrix, made rank 3 in place under the same id
        flat = prov.upload(x.reshape(-1, order="F"), (shape[0] * shape[1], shape[2]))
        value = prov.reshape(flat, shape)
        assert value.buffer_id == flat.buffer_id
        op = Operand(value, x, [(value, x)], [value])
    else:
        op = make_operand(prov, kind, x)
    rec = CallRecorder(prov)
    out = execute_image_normalize(rec, op.value, 1e-6, **opts)
    assert out.shape == shape
    got = prov.download(out).reshape(shape, order="F")
    want = oracle.image_normalize(x, 1e-6, **opts)
    # tolerance of test_gpu_parity.py::test_image_normalize_vs_oracle: tree-ordered plane sums here, sequential on the CPU
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    hx = prov.upload(x)
    one = prov.image_normalize(hx, *shape, 1e-6, **opts)
    assert same_bits(got.reshape(-1, order="F"), prov.download(one))
    assert rec.log[-1 if kind != "host" else 1][1][1:4] == shape
    assert_accounted(prov, rec, out)
    for h, values in op.watch:
        assert_intact(prov, h, values)
    free_all(prov, op.keep + [hx, one, out])


def test_image_normalize_refuses_other_ranks_before_any_call(prov):
    from runmat_amd import ProviderError

    for shape in ((4, 4), (2, 3, 4, 5)):
        h = prov.upload(np.ones(shape))
        rec = CallRecorder(prov)
        with pytest.raises(ProviderError) as e:
            execute_image_normalize(rec, h, 1e-6)
        assert str(e.value) == f"image normalize: expected 3-D input tensor, got shape {list(shape)}"
        assert rec.calls == []
        assert_intact(prov, h, np.ones(shape))
        prov.free(h)


# =====================================================================================================================
# MatmulEpilogue
# =====================================================================================================================
EPILOGUE_SHAPES = [(200, 96, 136), (256, 64, 128), (5, 7, 3)]  # edge tiles; the eight-wave tile; smaller than any tile
_EPILOGUE_INPUTS = {}


def epilogue_inputs(m, k, n):
    """One set of operands per shape, shared by every plan and left unchanged."""
    if (m, k, n) not in _EPILOGUE_INPUTS:
        vals = epilogue_values(np.random.default_rng(23 + m), m, k, n)
        vals["base"] = (k + 4) * EPS * (np.abs(vals["A"]) @ np.abs(vals["B"]))
        for v in vals.values():
            v.setflags(write=False)
        _EPILOGUE_INPUTS[(m, k, n)] = vals
    return _EPILOGUE_INPUTS[(m, k, n)]


def oracle_descriptor(want, vals):
    kw = {f: want[f] for f in ("alpha", "beta", "row_op", "col_op", "clamp_min", "clamp_max", "pow_exponent")}
    kw["row_scale"] = vals[want["row_scale"]] if want["row_scale"] else None
    kw["col_scale"] = vals[want["col_scale"]] if want["col_scale"] else None
    return kw


def within_epilogue_bound(got, want, alpha, base):
    """test_gpu_parity.py::test_matmul_epilogue_vs_oracle: (4 |alpha| + 1) (k + 4) eps |A||B| + 1e-13 (scales <= 2 each way); a
    power of a negative value is NaN on both sides."""
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = ~np.isnan(want)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= ((abs(alpha) * 4.0 + 1.0) * base + 1e-13)[fin]))


def evaluate_plan(oracle, plan, values):
    """The plan op by op on the CPU oracle: mtimes, then every elementwise op on full matrices."""
    env = dict(values)
    env.update({vid: np.array([[c]]) for vid, c in plan.const_values.items()})
    names = {"Add": "add", "Sub": "sub", "Mul": "mul", "ElemMul": "mul", "ElemDiv": "div", "ElemPow": "pow", "Pow": "pow",
             "max": "max", "min": "min"}
    for op in plan.operations:
        if op.name == "mtimes":
            env[op.output] = oracle.matmul(env[op.inputs[0]], env[op.inputs[1]])
        else:
            env[op.output] = oracle.binary(names[op.name], env[op.inputs[0]], env[op.inputs[1]])
    return env[plan.operations[-1].output]


@pytest.mark.parametrize("name", sorted(n for n, p in matmul_epilogue_plans().items() if not p[3]["diag"]))
@pytest.mark.parametrize("m,k,n", EPILOGUE_SHAPES)
def test_matmul_epilogue_sequence_from_plan(prov, oracle, m, k, n, name):
    plan, roles, output, want = matmul_epilogue_plans()[name]
    vals = epilogue_inputs(m, k, n)
    okw = oracle_descriptor(want, vals)
    expect, _ = oracle.matmul_epilogue(vals["A"], vals["B"], **okw)
    results = []
    for resident in (True, False):
        callers = [prov.upload(vals[r]) for r in roles] if resident else []
        rec = CallRecorder(prov)
        out = execute_matmul_epilogue(rec, plan, callers if resident else [vals[r] for r in roles], plan.const_values, output)
        assert out.shape == (m, n) and table_shape(prov, out) == (m, n)
        got = prov.download_matrix(out)
        assert within_epilogue_bound(got, expect, want["alpha"], vals["base"])
        assert_accounted(prov, rec, out)
        for h, r in zip(callers, roles):
            assert_intact(prov, h, vals[r])
        results.append(got)
        free_all(prov, callers + [out])
    assert same_bits(results[0], results[1])
    # the hook itself with the ready-made descriptor on fresh uploads
    hs = {r: prov.upload(vals[r]) for r in roles}
    gk = dict(okw, row_scale=hs.get(want["row_scale"]), col_scale=hs.get(want["col_scale"]))
    one = prov.matmul_epilogue(hs["A"], hs["B"], **gk)
    assert same_bits(results[0], prov.download_matrix(one))
    free_all(prov, list(hs.values()) + [one])
    if want["faithful"]:  # scale, bias, row, column, clamps, power in the epilogue's own order: the plan op by op agrees
        by_ops = evaluate_plan(oracle, plan, {vid: vals[r] for vid, r in zip(plan.inputs, roles)})
        assert within_epilogue_bound(results[0], by_ops, want["alpha"], vals["base"])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("m,k,n", EPILOGUE_SHAPES)
def test_matmul_epilogue_diag_output_outlives_the_matrix(prov, prov32, oracle, m, k, n, precision):
    """`diag(.)` as the plan's output: the kernel writes the diagonal in place into `zeros([min(m, n), 1])`, the executor frees
    the matrix and returns the diagonal.  At precision 32 the diagonal is narrowed into the f32 storage after the launch."""
    p = prov if precision == "f64" else prov32
    vals = epilogue_inputs(m, k, n)
    A, B = (vals["A"], vals["B"]) if precision == "f64" else (f32r(vals["A"]), f32r(vals["B"]))
    plan_d, _, out_d, want = matmul_epilogue_plans()["diag_is_output"]
    plan_m, _, out_m, _ = matmul_epilogue_plans()["diag_not_output"]
    ha, hb = p.upload(A), p.upload(B)
    # the same call without the free: the matrix comes back and its diag_output stays resident
    rec_m = CallRecorder(p)
    matrix = execute_matmul_epilogue(rec_m, plan_m, [ha, hb], plan_m.const_values, out_m)
    assert rec_m.calls == ["zeros", "matmul_epilogue"] and matrix.shape == (m, n)
    kept_diag = rec_m.created[0]
    full = p.download_matrix(matrix)
    assert same_bits(p.download(kept_diag), np.diag(full)[: min(m, n)].copy())
    rec = CallRecorder(p)
    diag = execute_matmul_epilogue(rec, plan_d, [ha, B], plan_d.const_values, out_d)
    assert rec.calls == ["upload", "zeros", "matmul_epilogue", "free", "free"]
    assert diag.shape == (min(m, n), 1) and table_shape(p, diag) == (min(m, n), 1) and diag == rec.created[1]
    freed_matrix = rec.created[2]
    assert freed_matrix.shape == (m, n) and rec.freed == [rec.created[0].buffer_id, freed_matrix.buffer_id]
    assert_gone(p, [rec.created[0], freed_matrix])
    got = p.download(diag)  # still readable after the matrix has been freed
    assert same_bits(got, np.diag(full)[: min(m, n)].copy())
    expect, dg = oracle.matmul_epilogue(A, B, alpha=3.0, diag=True)
    if precision == "f64":
        assert np.all(np.abs(got - dg) <= (13.0 * np.diag(vals["base"]))[: min(m, n)] + 1e-13)
    else:
        assert p.buffer_bits(diag) == 32 and same_bits(got, f32r(got))
        assert np.all(np.abs(got - dg) <= U32 * np.abs(dg) + (13.0 * np.diag(vals["base"]))[: min(m, n)] + 1e-13)
    # the storage freed with the matrix is reused by the next allocations; the diagonal must not move with it
    scratch = [p.zeros((m, n)) for _ in range(3)]
    assert same_bits(p.download(diag), got)
    assert_intact(p, ha, A)
    free_all(p, scratch + [ha, hb, matrix, kept_diag, diag])


def test_matmul_epilogue_row_scale_as_a_transposed_vector(prov, oracle):
    m, k, n = 200, 96, 136
    vals = epilogue_inputs(m, k, n)
    plan, roles, output, want = matmul_epilogue_plans()["row_divide"]
    base = prov.upload(np.ascontiguousarray(vals["r"].T))  # 1 x m
    view = prov.transpose(base)                             # m x 1
    assert view.shape == (m, 1)
    ha, hb = prov.upload(vals["A"]), prov.upload(vals["B"])
    rec = CallRecorder(prov)
    out = execute_matmul_epilogue(rec, plan, [ha, hb, view], plan.const_values, output)
    assert rec.log[0][2]["row_scale"] == view and rec.log[0][2]["row_op"] == "divide"
    expect, _ = oracle.matmul_epilogue(vals["A"], vals["B"], row_scale=vals["r"], row_op="divide")
    got = prov.download_matrix(out)
    assert within_epilogue_bound(got, expect, 1.0, vals["base"])
    hr = prov.upload(vals["r"])
    one = prov.matmul_epilogue(ha, hb, row_scale=hr, row_op="divide")
    assert same_bits(got, prov.download_matrix(one))
    assert_intact(prov, base, np.ascontiguousarray(vals["r"].T))
    assert_intact(prov, view, vals["r"])
    free_all(prov, [base, view, ha, hb, hr, one, out])


def test_matmul_epilogue_scalar_operand_is_the_soft_shape_error(prov):
    """A [1, 1] operand has one column, so the rules make it a row scale - of length 1 < m.  The provider refuses softly."""
    from runmat_amd import ProviderError

    m, k, n = 5, 7, 3
    vals = epilogue_inputs(m, k, n)
    p = FusionGroupPlan()
    a, b, s = p.input(), p.input(), p.input()
    p.builtin("diag", p.primitive("ElemMul", p.builtin("mtimes", a, b), s))
    ha, hs = prov.upload(vals["A"]), prov.upload(np.array([[2.0]]))
    _, _, desc, _, _ = derive_matmul_epilogue(p, {a: ha, s: hs}, p.const_values)
    assert desc["row_scale"] == hs and desc["col_scale"] is None
    rec = CallRecorder(prov)
    with pytest.raises(ProviderError) as e:
        execute_matmul_epilogue(rec, p, [ha, vals["B"], hs], p.const_values)
    assert e.value.code == 3 and "row scale length 1 < 5 rows" in str(e.value)
    assert rec.calls == ["upload", "zeros", "matmul_epilogue", "free", "free"]
    assert_accounted(prov, rec, None)  # nothing leaked: the upload and the diag buffer are gone
    assert_intact(prov, ha, vals["A"])
    assert_intact(prov, hs, np.array([[2.0]]))
    hr = prov.upload(vals["r"])  # and the provider is still usable, with the same plan
    out = execute_matmul_epilogue(prov, p, [ha, vals["B"], hr], p.const_values)
    assert out.shape == (min(m, n), 1)
    full = (vals["A"] @ vals["B"]) * vals["r"]
    assert np.allclose(prov.download(out), np.diag(full), rtol=0, atol=5 * (k + 4) * EPS * 2 * k)
    free_all(prov, [ha, hs, hr, out])
