"""CPU checks of the numpy restatement of the host `pagefun(@mtimes)` (tests/pagefun_host.py): the reference's unit tests
(tests/golden/pagefun_kats.json) and np.matmul with broadcasting within the fma bound."""
import json
from pathlib import Path

import numpy as np
import pytest

from pagefun_host import PagefunError, build_request, pagefun_host

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "pagefun_kats.json").read_text())
EPS = np.finfo(np.float64).eps


def arr(spec):
    return np.array(spec["data"], dtype=np.float64).reshape(spec["shape"], order="F")


@pytest.mark.parametrize("kat", KATS["products"], ids=lambda k: k["name"])
def test_reference_products(kat):
    out = pagefun_host(arr(kat["lhs"]), arr(kat["rhs"]))
    assert list(out.shape) == kat["out"]["shape"]
    assert out.ravel(order="F").tolist() == kat["out"]["data"]


@pytest.mark.parametrize("kat", KATS["errors"], ids=lambda k: k["name"])
def test_reference_errors(kat):
    with pytest.raises(PagefunError) as e:
        pagefun_host(arr(kat["lhs"]), arr(kat["rhs"]))
    assert e.value.kind == kat["kind"]


def test_build_request_fields():
    r = build_request([3, 4, 2, 1, 5], [4, 6, 1, 7])
    assert r.page_dims == [2, 7, 5] and r.output_shape == [3, 6, 2, 7, 5]
    assert r.input_page_dims == [[2, 1, 5], [1, 7, 1]]
    assert build_request([], [1, 1]).output_shape == [1, 1]
    assert build_request([5], [5, 2]).output_shape == [1, 2]  # a vector is one row
    assert build_request([2, 2, 0], [2, 2, 5]).page_dims == [0]  # a zero extent wins without a mismatch


@pytest.mark.parametrize("lhs,rhs", [((3, 4, 5), (4, 2, 5)), ((3, 4, 1), (4, 2, 5)), ((3, 4, 5), (4, 2)), ((2, 3, 2, 1), (3, 4, 1, 3)),
                                     ((2, 3, 2, 3, 4), (3, 4, 2, 1, 4)), ((7, 9, 2, 1, 3, 1, 2, 2), (9, 5, 1, 2, 3, 2, 1, 2))])
def test_against_matmul_within_fma_bound(lhs, rhs):
    rng = np.random.default_rng(11)
    A, B = rng.standard_normal(lhs), rng.standard_normal(rhs)
    got = pagefun_host(A, B)
    r = build_request(A.shape, B.shape)
    # numpy's matmul broadcasts leading batch dimensions: move the pages in front
    pa = np.moveaxis(A.reshape(A.shape[:2] + tuple(r.input_page_dims[0]), order="F"), (0, 1), (-2, -1))
    pb = np.moveaxis(B.reshape(B.shape[:2] + tuple(r.input_page_dims[1]), order="F"), (0, 1), (-2, -1))
    want = np.moveaxis(np.matmul(pa, pb), (-2, -1), (0, 1))
    bound = np.moveaxis(np.matmul(np.abs(pa), np.abs(pb)), (-2, -1), (0, 1)) * r.k * EPS
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= bound)


def test_sum_rounding_quirks():
    # an all -0.0 product page sums to +0.0; NaN and Inf propagate as in the loop
    A = np.array([[-0.0, 1.0], [np.inf, 2.0]])
    B = np.array([[1.0, np.nan], [-0.0, 1.0]])
    out = pagefun_host(A, B)
    assert np.signbit(out[0, 0]) == False and out[0, 0] == 0.0  # noqa: E712
    assert np.isinf(out[1, 0]) and np.isnan(out[1, 1]) and np.isnan(out[0, 1])
