"""What `rmhip_complex_matmul` must compute, for the host and the GPU tests: a thin layer over tests/complex_pagefun_ref.py on 2-D shapes
(the builtin's fallback runs the same three loops of builtins/common/linalg.rs on the gathered operands, mtimes.rs:173-218).

    cmatmul_host(Ar, Ai, Br, Bi) -> (Cr, Ci)   the host loop (cpagefun_host on one page); Ai or Bi is None for a real operand
    gate(Ar, Ai, Br, Bi)                       that file's gate: 2k eps (S + S') per part for kind 0, k eps S for the mixed kinds
    embed_model(Ar, Ai, Br, Bi, r32=False)     the numpy statement of the embedding the library runs above 32 on a side
    expected_plan(kind, m, n, k, r32)          the fields plan_cgemm (runmat_amd/csrc/gemm_plan.h) must return

The embedding.  A complex-interleaved column-major A (m x k) is, read as doubles, the real matrix A~ (2m x k) whose even rows are A_re
and odd rows A_im.  With P = [B_re | B_im] (k x 2n):

    kind 1  complex x real     A~ (2m x k) * B (k x n)         is the interleaved result itself
    kind 2  real x complex     T (m x 2n)  = A * P             C(i, j) = (T[i, j], T[i, n + j])
    kind 0  complex x complex  T (2m x 2n) = A~ * P            re = T[2i, j] - T[2i+1, n+j],  im = T[2i, n+j] + T[2i+1, j]

`embed_model` forms the real product with numpy's matmul (an order of its own, like the matrix cores'), then the one rounded difference
and sum.  Why the gate holds for it and for the device: each block of T is a k-term sum of rounded or fused products, within
k eps/2 S of the exact sum to first order; the difference or sum of two blocks adds one rounding, at most eps/2 (S + S'); the host
loop's own error is of the same size; for k >= 1 the total is at most (k + 1) eps (S + S') <= 2k eps (S + S').  The mixed kinds have one
block per part: k eps S.  Split-K only shortens the chains.
"""
from __future__ import annotations

import numpy as np

import complex_pagefun_ref as pref
from complex_pagefun_ref import EPS, KINDS, interleave, kind_of, magnitude, operands  # noqa: F401  (re-exported for the tests)

SMALL = 32  # gemm_plan::kPageSmall: at most this on every side -> the bit-exact small route

# (m, n, k) of the GPU tests: every shape the smallest that reaches its path
SMALL_SHAPES = [(1, 1, 1), (5, 4, 3), (32, 32, 32)]
BOUNDARY_SHAPES = [(33, 32, 32), (32, 33, 32), (32, 32, 33)]
EMBED_SHAPES = [
    (33, 40, 17),     # odd k: odd leading dimension of the planes
    (130, 5, 70),     # skinny
    (1, 1, 129),      # one output
    (129, 129, 16),   # ragged edge of 2m = 258
    (128, 128, 64),   # whole tiles
    (64, 64, 2048),   # split-K
]


def _check_2d(Ar, Br):
    assert np.ndim(Ar) == 2 and np.ndim(Br) == 2 and np.shape(Ar)[1] == np.shape(Br)[0]


def cmatmul_host(Ar, Ai, Br, Bi):
    _check_2d(Ar, Br)
    return pref.cpagefun_host(Ar, Ai, Br, Bi)


def cmatmul_scalar(Ar, Ai, Br, Bi):
    _check_2d(Ar, Br)
    return pref.cpagefun_scalar(Ar, Ai, Br, Bi)


def gate(Ar, Ai, Br, Bi):
    _check_2d(Ar, Br)
    return pref.gate(Ar, Ai, Br, Bi)


def f32_round(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def embed_model(Ar, Ai, Br, Bi, r32=False):
    """The table above in numpy; r32: each part rounded through f32 once, at the end."""
    _check_2d(Ar, Br)
    kind = kind_of(Ai, Bi)
    m, k = Ar.shape
    n = Br.shape[1]
    if kind == 2:
        At = np.asarray(Ar, dtype=np.float64)
    else:
        At = np.empty((2 * m, k), dtype=np.float64)
        At[0::2, :], At[1::2, :] = Ar, Ai
    P = np.asarray(Br, dtype=np.float64) if kind == 1 else np.concatenate([Br, Bi], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        T = At @ P if k else np.zeros((At.shape[0], P.shape[1]))
        if kind == 1:
            re, im = T[0::2, :], T[1::2, :]
        elif kind == 2:
            re, im = T[:, :n], T[:, n:]
        else:
            re = T[0::2, :n] - T[1::2, n:]
            im = T[0::2, n:] + T[1::2, :n]
    if r32:
        re, im = f32_round(re), f32_round(im)
    return np.asfortranarray(re), np.asfortranarray(im)


def expected_plan(kind, m, n, k, r32):
    """plan_cgemm's fields (m, n, k >= 1: the empty cases never reach the plan)."""
    if m <= SMALL and n <= SMALL and k <= SMALL:
        return dict(route="small", M=0, N=0, K=0, lda=0, ldb=0, split_b=0, join=0, workspace=0)
    M = m if kind == 2 else 2 * m
    N = n if kind == 1 else 2 * n
    split = kind != 1
    join = kind != 1 or bool(r32)
    return dict(route="embed", M=M, N=N, K=k, lda=M, ldb=k, split_b=int(split), join=int(join),
                workspace=(2 * k * n if split else 0) + (M * N if join else 0))
