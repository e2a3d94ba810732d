"""numpy restatement of the reference's host `pagefun(@mtimes, A, B)` (builtins/acceleration/gpu/pagefun.rs).

    build_request(lhs_shape, rhs_shape) -> PagefunShapes(output_shape, page_dims, input_page_dims, m, k, n)
    pagefun_host(A, B) -> the product pages, shaped output_shape

* `build_request` restates `build_pagefun_request` (:450-530) over `canonical_matrix_shape` (:899-911): a 0-D shape is 1 x 1, a 1-D shape
  [s] is 1 x s, dimensions 3.. are pages.  Per page dimension the target extent starts at 1; a 0 extent makes it 0 (and ends the check),
  an extent other than 1 sets it or must equal it (else the page-dimension error).  Inner dimensions that differ are the
  inner-dimension error.  `input_page_dims` are the operands' page extents padded with 1s to the common rank;
* `pagefun_host` restates the per-page loop (:330-384): output page p, column-major over page_dims, multiplies the operands' pages
  at p's multi-index, index 0 where an operand's extent is 1, with matmul_real (common/linalg.rs:6-32): sum = 0.0, sum += a*b in k
  order.  Written as S = 0.0; S = S + A[:, k] * B[k, :] over all pages at once: every product and sum is rounded separately in the
  same order, so it is bit-exact to the Rust loop.
Arrays are column-major in meaning: an array's numpy shape is its MATLAB shape and its data is read in Fortran order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np


class PagefunError(ValueError):
    """`kind` is "inner" (PAGEFUN_ERROR_MATRIX_DIM_MISMATCH) or "page" (PAGEFUN_ERROR_PAGE_DIM_MISMATCH)."""

    def __init__(self, kind: str, message: str):
        super().__init__(message)
        self.kind = kind


@dataclass
class PagefunShapes:
    output_shape: List[int]
    page_dims: List[int]
    input_page_dims: List[List[int]]
    m: int
    k: int
    n: int


def canonical_matrix_shape(shape: Sequence[int]) -> List[int]:
    if len(shape) == 0:
        return [1, 1]
    if len(shape) == 1:
        return [1, int(shape[0])]
    return [int(s) for s in shape]


def build_request(lhs_shape: Sequence[int], rhs_shape: Sequence[int]) -> PagefunShapes:
    lhs, rhs = canonical_matrix_shape(lhs_shape), canonical_matrix_shape(rhs_shape)
    (m, k), lhs_pages = lhs[:2], lhs[2:]
    (kb, n), rhs_pages = rhs[:2], rhs[2:]
    if k != kb:
        raise PagefunError("inner", f"inner matrix dimensions must agree ({m}x{k} * {kb}x{n})")
    rank = max(len(lhs_pages), len(rhs_pages))
    page_dims = []
    for d in range(rank):
        target = 1
        for size in (lhs_pages[d] if d < len(lhs_pages) else 1, rhs_pages[d] if d < len(rhs_pages) else 1):
            if size == 0:
                target = 0
                break
            if size != 1:
                if target == 1:
                    target = size
                elif target != size:
                    raise PagefunError("page", f"page dimension {d + 3} mismatch ({target} vs {size})")
        page_dims.append(target)
    ipd = [list(lhs_pages) + [1] * (rank - len(lhs_pages)), list(rhs_pages) + [1] * (rank - len(rhs_pages))]
    return PagefunShapes([m, n] + page_dims, page_dims, ipd, m, k, n)


def page_indices(page_dims: Sequence[int], operand_dims: Sequence[int]) -> np.ndarray:
    """The operand page each output page reads (0-based, column-major over the operand's own page extents)."""
    pages = int(np.prod(page_dims, dtype=np.int64)) if page_dims else 1
    if not page_dims:
        return np.zeros(pages, dtype=np.int64)
    idx = np.unravel_index(np.arange(pages, dtype=np.int64), tuple(page_dims), order="F")
    sub = [np.zeros_like(i) if e == 1 else i for i, e in zip(idx, operand_dims)]
    return np.ravel_multi_index(sub, tuple(operand_dims), order="F").astype(np.int64)


def pagefun_host(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    req = build_request(A.shape, B.shape)
    m, k, n = req.m, req.k, req.n
    pages = int(np.prod(req.page_dims, dtype=np.int64)) if req.page_dims else 1
    if m == 0 or n == 0 or pages == 0:
        return np.zeros(req.output_shape, dtype=np.float64, order="F")
    va = int(np.prod(req.input_page_dims[0], dtype=np.int64))
    vb = int(np.prod(req.input_page_dims[1], dtype=np.int64))
    A3 = A.reshape((m, k, va), order="F")[:, :, page_indices(req.page_dims, req.input_page_dims[0])]
    B3 = B.reshape((k, n, vb), order="F")[:, :, page_indices(req.page_dims, req.input_page_dims[1])]
    S = np.zeros((m, n, pages), dtype=np.float64)
    for kk in range(k):
        S = S + A3[:, kk:kk + 1, :] * B3[kk:kk + 1, :, :]
    return S.reshape(req.output_shape, order="F")
