"""numpy restatement of the reference's host `pagefun(@mtimes, A, B)` when at least one operand is complex
(builtins/acceleration/gpu/pagefun.rs:330-384; pages reach `mtimes` as Tensor or ComplexTensor values, :786-823, so exactly one of three
loops of builtins/common/linalg.rs runs per page pair, mtimes.rs:348-359).

    cpagefun_host(Ar, Ai, Br, Bi) -> (Cr, Ci), shaped build_request(...).output_shape; Ai or Bi is None for a real operand (not both)

On separate float64 re / im arrays, over all pages at once, every product, difference and sum its own operation in the loops' order:
  kind 0  complex x complex (matmul_complex :57-85):        re = 0.0; im = 0.0; per k  re += ar*br - ai*bi;  im += ar*bi + ai*br
  kind 1  complex x real    (matmul_complex_real :88-116):  re += ar*br;  im += ai*br
  kind 2  real x complex    (matmul_real_complex :119-147): re += ar*br;  im += ar*bi
The k-term is formed first (two rounded products, one rounded difference or sum) and then added to the accumulator.  The mixed kinds are
not kind 0 with a zero part filled in: no product with an implied zero is formed.  numpy's complex multiply is never used.
Arrays are column-major in meaning, as in pagefun_host.py, whose `build_request` and `page_indices` give the shapes and the page map.

    gate(Ar, Ai, Br, Bi) -> (bound_re, bound_im): what two evaluations in different orders may differ by.  Each part is a sum of 2k
    rounded products (kind 0) or k (mixed); the first-order bound of one evaluation is (terms) eps/2 sum|a||b|, two evaluations differ
    by at most twice that.  With EPS = 2^-52 and S = pagefun_host on absolute values:
        |d re| <= 2k EPS (S(|Ar|,|Br|) + S(|Ai|,|Bi|)),  |d im| <= 2k EPS (S(|Ar|,|Bi|) + S(|Ai|,|Br|))
    and k EPS times the single surviving term for the mixed kinds.
"""
from __future__ import annotations

import numpy as np

from pagefun_host import build_request, page_indices, pagefun_host

EPS = 2.0 ** -52
KINDS = (0, 1, 2)  # complex x complex, complex x real, real x complex


def kind_of(Ai, Bi) -> int:
    assert Ai is not None or Bi is not None, "two real operands are pagefun_host's"
    return 0 if Ai is not None and Bi is not None else (1 if Ai is not None else 2)


def _paged(X, rows, cols, page_dims, operand_dims):
    vol = int(np.prod(operand_dims, dtype=np.int64))
    return np.asarray(X, dtype=np.float64).reshape((rows, cols, vol), order="F")[:, :, page_indices(page_dims, operand_dims)]


def cpagefun_host(Ar, Ai, Br, Bi):
    kind = kind_of(Ai, Bi)
    req = build_request(np.shape(Ar), np.shape(Br))
    m, k, n = req.m, req.k, req.n
    pages = int(np.prod(req.page_dims, dtype=np.int64)) if req.page_dims else 1
    if m == 0 or n == 0 or pages == 0:
        z = np.zeros(req.output_shape, dtype=np.float64, order="F")
        return z, z.copy()
    ar = _paged(Ar, m, k, req.page_dims, req.input_page_dims[0])
    br = _paged(Br, k, n, req.page_dims, req.input_page_dims[1])
    ai = _paged(Ai, m, k, req.page_dims, req.input_page_dims[0]) if Ai is not None else None
    bi = _paged(Bi, k, n, req.page_dims, req.input_page_dims[1]) if Bi is not None else None
    re = np.zeros((m, n, pages), dtype=np.float64)
    im = np.zeros((m, n, pages), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for kk in range(k):
            a_r, b_r = ar[:, kk:kk + 1, :], br[kk:kk + 1, :, :]
            if kind == 0:
                a_i, b_i = ai[:, kk:kk + 1, :], bi[kk:kk + 1, :, :]
                p_rr = a_r * b_r
                p_ii = a_i * b_i
                p_ri = a_r * b_i
                p_ir = a_i * b_r
                t_re = p_rr - p_ii
                t_im = p_ri + p_ir
                re = re + t_re
                im = im + t_im
            elif kind == 1:
                a_i = ai[:, kk:kk + 1, :]
                re = re + a_r * b_r
                im = im + a_i * b_r
            else:
                b_i = bi[kk:kk + 1, :, :]
                re = re + a_r * b_r
                im = im + a_r * b_i
    return re.reshape(req.output_shape, order="F"), im.reshape(req.output_shape, order="F")


def cpagefun_scalar(Ar, Ai, Br, Bi):
    """The three loops as plain Python scalar loops, page by page (small shapes only): what the restatement must equal bit for bit."""
    kind = kind_of(Ai, Bi)
    req = build_request(np.shape(Ar), np.shape(Br))
    m, k, n = req.m, req.k, req.n
    pages = int(np.prod(req.page_dims, dtype=np.int64)) if req.page_dims else 1
    ia, ib = page_indices(req.page_dims, req.input_page_dims[0]), page_indices(req.page_dims, req.input_page_dims[1])
    flat = lambda X: None if X is None else np.asarray(X, dtype=np.float64).ravel(order="F").tolist()
    ar, ai, br, bi = flat(Ar), flat(Ai), flat(Br), flat(Bi)
    re, im = [0.0] * (m * n * pages), [0.0] * (m * n * pages)
    for p in range(pages):
        oa, ob, oc = int(ia[p]) * m * k, int(ib[p]) * k * n, p * m * n
        for j in range(n):
            for i in range(m):
                sr, si = 0.0, 0.0
                for kk in range(k):
                    xa, xb = oa + i + kk * m, ob + kk + j * k
                    if kind == 0:
                        sr += ar[xa] * br[xb] - ai[xa] * bi[xb]
                        si += ar[xa] * bi[xb] + ai[xa] * br[xb]
                    elif kind == 1:
                        sr += ar[xa] * br[xb]
                        si += ai[xa] * br[xb]
                    else:
                        sr += ar[xa] * br[xb]
                        si += ar[xa] * bi[xb]
                re[oc + i + j * m], im[oc + i + j * m] = sr, si
    shape = req.output_shape
    return np.array(re).reshape(shape, order="F"), np.array(im).reshape(shape, order="F")


def magnitude(Ar, Ai, Br, Bi):
    """(S_re, S_im): the sums of |a||b| over the products each part is made of (S = pagefun_host on absolute values)."""
    kind = kind_of(Ai, Bi)
    S = lambda X, Y: pagefun_host(np.abs(X), np.abs(Y))
    if kind == 0:
        return S(Ar, Br) + S(Ai, Bi), S(Ar, Bi) + S(Ai, Br)
    if kind == 1:
        return S(Ar, Br), S(Ai, Br)
    return S(Ar, Br), S(Ar, Bi)


def gate(Ar, Ai, Br, Bi):
    k = max(build_request(np.shape(Ar), np.shape(Br)).k, 1)
    factor = (2 * k if kind_of(Ai, Bi) == 0 else k) * EPS
    s_re, s_im = magnitude(Ar, Ai, Br, Bi)
    return factor * s_re, factor * s_im


def operands(rng, kind, lhs_shape, rhs_shape, ints=False):
    """(Ar, Ai, Br, Bi) for `kind`: standard normal parts, or Gaussian integers with parts in -4..4 (exact in any order)."""
    def part(shape):
        if ints:
            return rng.integers(-4, 5, size=shape).astype(np.float64)
        return rng.standard_normal(shape)

    Ar, Br = part(lhs_shape), part(rhs_shape)
    Ai = part(lhs_shape) if kind != 2 else None
    Bi = part(rhs_shape) if kind != 1 else None
    return Ar, Ai, Br, Bi


def interleave(re, im) -> np.ndarray:
    """2 * numel doubles (re, im, re, im, ...) in column-major element order: what upload / download carry for a complex tensor."""
    out = np.empty(2 * np.size(re), dtype=np.float64)
    out[0::2] = np.asarray(re, dtype=np.float64).ravel(order="F")
    out[1::2] = np.asarray(im, dtype=np.float64).ravel(order="F")
    return out
