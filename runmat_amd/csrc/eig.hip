// eig.hip -- `eig(a, compute_left)` (crates/runmat-accelerate-api/src/lib.rs:2491-2497 -> ProviderEigResult { eigenvalues, diagonal, right,
// left } :786-791) for REAL, BITWISE SYMMETRIC matrices of order n <= kEigMaxN.  Everything else is refused with the soft error and the
// builtin's host path answers (builtins/math/linalg/factor/eig.rs:436-461: any Err becomes Ok(None)).  Eigenvalues come back ascending
// (MATLAB's order for symmetric input; the reference's Schur order is unpinned, eig.rs:1196-1207), `right` has orthonormal columns, and
// `left` - inv(V)' normalised to left_k . right_k = 1 (eig.rs:890-940), which is V itself for an orthonormal V - is a copy of `right`.
//
// Scaling.  max |a| is brought into [0.5, 1) by a power of two (exact), the eigenvalues are multiplied back at the end: no squared entry
// overflows or underflows, and eig(2^k A) returns bitwise the vectors of eig(A).  A zero matrix gives lambda = 0, V = I.
//
// n <= 64: ONE launch, one workgroup.  Two-sided cyclic Jacobi on A in LDS with V beside it (jacobi_lds): the round-robin tournament of
// jac_pair (common.h, shared with svdsolve.hip) orders the pairs, so the rotations of a step are disjoint; the column phase (A <- A J, V <- V J) and the row phase
// (A <- J' A) each run over all pairs at once.  The 2 x 2 pivot block is written from the closed forms (a_pq = a_qp = 0 exactly), a pair
// with |a_pq| <= 2^-58 (of the scaled matrix; exact zeros included) is skipped, and the iteration ends after a sweep without a rotation.
// The same launch checks symmetry and finiteness, sorts (stable, ascending) and writes every output; the host reads one status word.
//
// 64 < n <= 4096: blocked one-sided Jacobi with the same LDS solver inside.  One-sided Jacobi on an indefinite A would diagonalise A^2 -
// +lambda and -lambda share a singular subspace, [0 1; 1 0] already has orthogonal columns - so it runs on B = A + s I with
// s = 1.5 ||A||_inf of the scaled matrix: B has A's eigenvectors and a spectrum inside [0.5, 2.5] ||A||_inf, so no column of W = B V
// ever gets small and the relative test below is meaningful for every pair.  Columns are grouped in blocks of 32; a tournament step
// over block pairs is three launches:
//   (a) k_eig_gram, pairs x row slices of 256: the slice's part of the 64 x 64 Gram matrix G of the pair's columns (row chunks staged in
//       LDS, fixed-order sums);
//   (b) k_eig_rot, one workgroup per pair: G = the parts summed in slice order.  The pair is left alone when every
//       |g_pq| / sqrt(g_pp g_qq) is below tol = max(1e-15, sqrt(n) eps) - the threshold of svdsolve.hip, raised to the rounding level of
//       a dot product of length n as LAPACK's dgesvj does: G is recomputed from W every time, and below that level a degenerate cluster
//       (ones(n): n - 1 equal eigenvalues) keeps rotating noise by large angles and never settles; a zero column counts as orthogonal.
//       Otherwise ONE sweep of jacobi_lds over G (pairs below tol / 10 skipped) gives an orthogonal Q - a sweep over G is a sweep of
//       one-sided rotations over the pair's columns, so the whole remains a cyclic one-sided Jacobi - which one Newton-Schulz step
//       re-orthogonalises (polish_q);
//   (c) k_eig_apply, pairs x row slices: the slice's rows of the pair's columns of W and of V times Q.
// A sweep is 3 (ceil(n / 32) - 1) launches (3 more for an odd block count) against the n - 1 of the scalar tournament, and the host reads
// one 8-byte word per sweep; 60 sweeps without convergence are refused.  Then lambda_k = v_k' A v_k against the UNSHIFTED scaled matrix
// (one dgemm, fixed-order dots), a stable rank sort, and one pass that permutes V and writes the outputs.
// Small eigenvalues therefore have ABSOLUTE accuracy of about n eps ||A||, as from LAPACK's syev - not the relative accuracy a one-sided
// Jacobi SVD gives singular values.
//
// Reproducible run to run: every sum has a fixed order, no float atomics; the only atomics are integer / ordered-bits maxima on control
// words.  No grid-wide barrier: every tournament step is an ordinary launch on the context's stream.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
constexpr int kEigMaxN = 4096;      // the SVD path's cap (kSvdMaxColsDefault)
constexpr int kEigSmall = 64;       // up to here the whole problem lives in the LDS of one workgroup
constexpr int kEigBlock = 32;       // columns per block of the blocked form (a pair is kEigSmall columns)
constexpr int kLd = kEigSmall + 1;  // leading dimension of the LDS matrices: row walks of the row phase stay off one bank
constexpr int kEigThreads = 256;
constexpr int kPairsPerWave = kEigSmall / 2 / (kEigThreads / 64);  // pairs of a tournament step each wave carries through jacobi_lds
constexpr int kEigSweeps = 60;      // as jacobi_svd
constexpr int kSliceRows = 256;     // rows per workgroup of the Gram and update launches of a step
constexpr int kInnerSweeps = 1;     // sweeps over a block pair's Gram matrix per visit
constexpr double kSkip = 0x1p-58;   // rotations below this (relative to the largest entry) are skipped
constexpr double kOrth = 1.0e-15;   // svdsolve.hip: pairs orthogonal to 1e-15 are left alone (the floor of the blocked form's tolerance)
constexpr u64 kNanBits = 0x7ff8000000000000ull;

enum : u64 { EIG_OK = 0, EIG_ASYM = 1, EIG_NONFINITE = 2, EIG_NOCONV = 3 };

struct EigLds {
    double S[kEigSmall * kLd];  // the symmetric matrix being diagonalised / a staged row chunk
    double U[kEigSmall * kLd];  // the accumulated rotations
    int rank[kEigSmall];        // sorted position of every eigenvalue (k_eig_small)
    u64 word;
    int flag;
};

// Two-sided cyclic Jacobi on the symmetric m x m matrix L.S (m <= kEigSmall), rotations accumulated into L.U (the caller sets it to the
// identity).  A pair is rotated when |a_pq| > thr and |a_pq| > rel sqrt(|a_pp a_qq|), otherwise a_pq is dropped.  Every thread of the
// workgroup calls it.  Returns the sweeps taken, or -1 when max_sweeps ended with a rotation.
__device__ __forceinline__ int jacobi_lds(EigLds& L, int m, double thr, double rel, int max_sweeps) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int M = (m + 1) & ~1, npairs = M / 2;
    if (m < 2) return 0;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        int rotated = 0;
        for (int t = 0; t < M - 1; ++t) {
            // wave w owns the pairs w, w + 4, ... of the step through both phases; its lane `it` works out the rotation of pair w + 4 it
            // and writes the 2 x 2 pivot block, which no other thread touches during the step
            double c = 1.0, s = 0.0;
            int p = 0, q = 0;
            if (lane < kPairsPerWave && w + 4 * lane < npairs) {
                jac_pair(M, t, w + 4 * lane, &p, &q);
                if (p > q) {
                    const int tmp = p;
                    p = q;
                    q = tmp;
                }
                if (q < m) {  // q == m: the padding player of an odd order
                    const double apq = L.S[p + q * kLd], app = L.S[p + p * kLd], aqq = L.S[q + q * kLd];
                    if (fabs(apq) > thr && fabs(apq) > rel * sqrt(fabs(app * aqq))) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = c * tt;
                        L.S[p + p * kLd] = app - tt * apq;
                        L.S[q + q * kLd] = aqq + tt * apq;
                        rotated = 1;
                    }
                    L.S[p + q * kLd] = 0.0;  // below the threshold: dropped
                    L.S[q + p * kLd] = 0.0;
                }
            }
            double cc[kPairsPerWave], ss[kPairsPerWave];
            int pp[kPairsPerWave], qq[kPairsPerWave];
#pragma unroll
            for (int it = 0; it < kPairsPerWave; ++it) {
                cc[it] = __shfl(c, it, 64);
                ss[it] = lane < m ? __shfl(s, it, 64) : 0.0;  // s == 0: nothing to do for this pair
                pp[it] = __shfl(p, it, 64);
                qq[it] = __shfl(q, it, 64);
            }
            // column phase, row `lane`: A <- A J (outside the pivot block), V <- V J.  The pairs are disjoint, so the loads of four pairs
            // go out together before their stores
            double xs[4], ys[4], xu[4], yu[4];
#pragma unroll
            for (int h = 0; h < kPairsPerWave; h += 4) {
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    if (ss[h + it] != 0.0) {
                        xs[it] = L.S[lane + pp[h + it] * kLd];
                        ys[it] = L.S[lane + qq[h + it] * kLd];
                        xu[it] = L.U[lane + pp[h + it] * kLd];
                        yu[it] = L.U[lane + qq[h + it] * kLd];
                    }
                }
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const double ci = cc[h + it], si = ss[h + it];
                    if (si != 0.0) {
                        if (lane != pp[h + it] && lane != qq[h + it]) {
                            L.S[lane + pp[h + it] * kLd] = ci * xs[it] - si * ys[it];
                            L.S[lane + qq[h + it] * kLd] = si * xs[it] + ci * ys[it];
                        }
                        L.U[lane + pp[h + it] * kLd] = ci * xu[it] - si * yu[it];
                        L.U[lane + qq[h + it] * kLd] = si * xu[it] + ci * yu[it];
                    }
                }
            }
            __syncthreads();
            // row phase, column `lane`: A <- J' A
#pragma unroll
            for (int h = 0; h < kPairsPerWave; h += 4) {
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    if (ss[h + it] != 0.0) {
                        xs[it] = L.S[pp[h + it] + lane * kLd];
                        ys[it] = L.S[qq[h + it] + lane * kLd];
                    }
                }
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const double ci = cc[h + it], si = ss[h + it];
                    if (si != 0.0 && lane != pp[h + it] && lane != qq[h + it]) {
                        L.S[pp[h + it] + lane * kLd] = ci * xs[it] - si * ys[it];
                        L.S[qq[h + it] + lane * kLd] = si * xs[it] + ci * ys[it];
                    }
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) return sweep;
    }
    return -1;
}

__device__ __forceinline__ void lds_identity(double* U) {
    for (int e = threadIdx.x; e < kEigSmall * kEigSmall; e += kEigThreads) U[(e & 63) + (e >> 6) * kLd] = (e & 63) == (e >> 6) ? 1.0 : 0.0;
}

__device__ __forceinline__ u64 abs_bits(double x) { return (u64)__double_as_longlong(fabs(x)); }  // NaN payloads order above +Inf

// the power of two that brings amax into [0.5, 1): amax = f 2^e
__device__ __forceinline__ int scale_exponent(double amax) {
    int e = 0;
    if (amax > 0.0) (void)frexp(amax, &e);
    return e;
}

// ---- n <= kEigSmall: everything in one launch -----------------------------------------------------------------------------------------
// status[0] = EIG_*.  Outputs (written only when the status is EIG_OK): vals n, diag n x n, right n x n.
__global__ void __launch_bounds__(kEigThreads) k_eig_small(const double* __restrict__ A, int n, double* __restrict__ vals, double* __restrict__ diag,
                                                           double* __restrict__ right, u64* __restrict__ status) {
    __shared__ EigLds L;
    const int tid = threadIdx.x;
    if (tid == 0) {
        L.word = 0;
        L.flag = 0;
    }
    __syncthreads();
    u64 mx = 0;
    for (int e = tid; e < n * n; e += kEigThreads) {
        const double x = A[e];
        L.S[(e % n) + (e / n) * kLd] = x;
        const u64 b = abs_bits(x);
        mx = b > mx ? b : mx;
    }
    if (mx) atomicMax(&L.word, mx);
    __syncthreads();
    int asym = 0;
    for (int e = tid; e < n * n; e += kEigThreads) {
        const int i = e % n, j = e / n;
        if (!(L.S[i + j * kLd] == L.S[j + i * kLd])) asym = 1;
    }
    if (asym) L.flag = 1;
    __syncthreads();
    const double amax = __longlong_as_double((long long)L.word);
    const u64 bad = !(amax < __builtin_inf()) ? EIG_NONFINITE : (L.flag ? EIG_ASYM : EIG_OK);
    if (bad != EIG_OK) {  // uniform
        if (tid == 0) status[0] = bad;
        return;
    }
    const int ex = scale_exponent(amax);
    for (int e = tid; e < n * n; e += kEigThreads) {
        const int idx = (e % n) + (e / n) * kLd;
        L.S[idx] = ldexp(L.S[idx], -ex);
    }
    lds_identity(L.U);
    __syncthreads();
    const int sweeps = jacobi_lds(L, n, kSkip, 0.0, kEigSweeps);
    if (sweeps < 0) {
        if (tid == 0) status[0] = EIG_NOCONV;
        return;
    }
    // stable ascending rank of every eigenvalue, then column k of V goes to column rank[k]
    if (tid < n) {
        const double d = L.S[tid + tid * kLd];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double o = L.S[j + j * kLd];
            r += (o < d || (o == d && j < tid)) ? 1 : 0;
        }
        L.rank[tid] = r;
        vals[r] = ldexp(d, ex);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += kEigThreads) {
        const int i = e % n, k = e / n, r = L.rank[k];
        right[i + r * n] = L.U[i + k * kLd];
        diag[i + r * n] = i == r ? ldexp(L.S[k + k * kLd], ex) : 0.0;
    }
    if (tid == 0) status[0] = EIG_OK;
}

// ---- blocked form ---------------------------------------------------------------------------------------------------------------------
// ctl[0] = max |a| as bits (NaN above +Inf), ctl[1] = 1 when a(i,j) != a(j,i) somewhere, ctl[2] = ||A_scaled||_inf as bits,
// ctl[3] = the sweep's word: largest relative off-diagonal of an active pair as bits (NaN bits: non-finite data)
__global__ void __launch_bounds__(kEigThreads) k_eig_check(const double* __restrict__ A, u64 n, u64* __restrict__ ctl) {
    u64 mx = 0;
    int asym = 0;
    const u64 total = n * n;
    for (u64 e = (u64)blockIdx.x * kEigThreads + threadIdx.x; e < total; e += (u64)gridDim.x * kEigThreads) {
        const u64 i = e % n, j = e / n;
        const double x = A[e];
        if (i < j && !(x == A[j + i * n])) asym = 1;
        const u64 b = abs_bits(x);
        mx = b > mx ? b : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctl[0], mx);
    if (asym) atomicMax(&ctl[1], (u64)1);
}

__device__ __forceinline__ double eig_block_sum(double s, double* sh4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // sh4 may still be read from the previous call
    if ((threadIdx.x & 63) == 0) sh4[w] = s;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// one workgroup per column: its absolute sum in the scaled matrix (= the row sum, by symmetry), maximum into ctl[2]
__global__ void __launch_bounds__(kEigThreads) k_eig_colsum(const double* __restrict__ A, u64 n, u64* __restrict__ ctl) {
    __shared__ double sh4[4];
    const int ex = scale_exponent(__longlong_as_double((long long)ctl[0]));
    const double* a = A + (u64)blockIdx.x * n;
    double s = 0.0;
    for (u64 i = threadIdx.x; i < n; i += kEigThreads) s += fabs(ldexp(a[i], -ex));
    s = eig_block_sum(s, sh4);
    if (threadIdx.x == 0) atomicMax(&ctl[2], (u64)__double_as_longlong(s));
}

// As = the scaled matrix, W = As + 1.5 ||As||_inf I, V = I
__global__ void __launch_bounds__(kEigThreads) k_eig_prep(const double* __restrict__ A, u64 n, const u64* __restrict__ ctl, double* __restrict__ As,
                                                          double* __restrict__ W, double* __restrict__ V) {
    const int ex = scale_exponent(__longlong_as_double((long long)ctl[0]));
    const double shift = 1.5 * __longlong_as_double((long long)ctl[2]);
    const u64 total = n * n;
    for (u64 e = (u64)blockIdx.x * kEigThreads + threadIdx.x; e < total; e += (u64)gridDim.x * kEigThreads) {
        const bool d = e % n == e / n;
        const double x = ldexp(A[e], -ex);
        As[e] = x;
        W[e] = d ? x + shift : x;
        V[e] = d ? 1.0 : 0.0;
    }
}

// rows r0 .. r0 + 63 of the pair's 64 columns into L.S (zeros beyond the matrix)
__device__ __forceinline__ void stage_chunk(double* S, const double* __restrict__ M, u64 n, u64 r0, u64 c0, u64 c1) {
    for (int e = threadIdx.x; e < kEigSmall * kEigSmall; e += kEigThreads) {
        const int r = e & 63, cc = e >> 6;
        const u64 col = cc < kEigBlock ? c0 + (u64)cc : c1 + (u64)(cc - kEigBlock), row = r0 + (u64)r;
        S[r + cc * kLd] = (row < n && col < n) ? M[row + col * n] : 0.0;
    }
}

// M(rows, pair) <- M(rows, pair) Q for rows [row_lo, row_hi) with Q = L.U, chunk by chunk through L.S; sums over k in index order
__device__ __forceinline__ void apply_q(EigLds& L, double* __restrict__ M, u64 n, u64 row_lo, u64 row_hi, u64 c0, u64 c1) {
    const int tr = threadIdx.x & 15, tc = threadIdx.x >> 4;
    for (u64 r0 = row_lo; r0 < row_hi; r0 += kEigSmall) {
        __syncthreads();
        stage_chunk(L.S, M, n, r0, c0, c1);
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
        for (int k = 0; k < kEigSmall; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = L.S[(tr + 16 * u) + k * kLd];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = L.U[k + (4 * tc + v) * kLd];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int cc = 4 * tc + v;
            const u64 col = cc < kEigBlock ? c0 + (u64)cc : c1 + (u64)(cc - kEigBlock);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u64 row = r0 + (u64)(tr + 16 * u);
                if (row < n && col < n) M[row + col * n] = acc[u][v];
            }
        }
    }
}

// Q <- Q (1.5 I - 0.5 Q'Q), one Newton-Schulz step towards the orthogonal polar factor, through L.S.  Q is a product of some hundred
// rotations per column and ||Q'Q - I|| ~ sqrt(rotations) eps reaches 1e-14; V takes one such factor per step, and whatever V loses in
// orthogonality the eigenvalues and the residual lose with it.  The step squares that error down to the rounding of two 64-term sums.
__device__ __forceinline__ void polish_q(EigLds& L) {
    const int ta = threadIdx.x & 15, tb = threadIdx.x >> 4;
    double t[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) t[u][v] = 0.0;
    for (int k = 0; k < kEigSmall; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = L.U[k + (4 * ta + u) * kLd];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = L.U[k + (4 * tb + v) * kLd];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) t[u][v] += a[u] * b[v];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) L.S[(4 * ta + u) + (4 * tb + v) * kLd] = (4 * ta + u == 4 * tb + v ? 1.5 : 0.0) - 0.5 * t[u][v];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) t[u][v] = 0.0;
    for (int k = 0; k < kEigSmall; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = L.U[(ta + 16 * u) + k * kLd];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = L.S[k + (4 * tb + v) * kLd];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) t[u][v] += a[u] * b[v];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) L.U[(ta + 16 * u) + (4 * tb + v) * kLd] = t[u][v];
}

// the block pair (I < J) that workgroup b of tournament step `step` over P (even) players takes; false for the padding player's pair
__device__ __forceinline__ bool block_pair(int P, int step, int b, int nblocks, u64* c0, u64* c1) {
    int bi, bj;
    jac_pair(P, step, b, &bi, &bj);
    if (bi > bj) {
        const int tmp = bi;
        bi = bj;
        bj = tmp;
    }
    *c0 = (u64)bi * kEigBlock;
    *c1 = (u64)bj * kEigBlock;
    return bj < nblocks;
}

// Step launch 1, grid (pairs, row slices of kSliceRows): the slice's part of G = [W_I W_J]' [W_I W_J] into Gp[pair][slice].  Thread
// (ta, tb) owns the 4 x 4 block at (4 ta, 4 tb); rows summed in index order.
__global__ void __launch_bounds__(kEigThreads) k_eig_gram(const double* __restrict__ W, u64 n, int nblocks, int P, int step, double* __restrict__ Gp) {
    __shared__ double S[kEigSmall * kLd];
    u64 c0, c1;
    if (!block_pair(P, step, blockIdx.x, nblocks, &c0, &c1)) return;
    const int ta = threadIdx.x & 15, tb = threadIdx.x >> 4;
    double g[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) g[u][v] = 0.0;
    const u64 row_lo = (u64)blockIdx.y * kSliceRows, row_hi = row_lo + kSliceRows < n ? row_lo + kSliceRows : n;
    for (u64 r0 = row_lo; r0 < row_hi; r0 += kEigSmall) {
        __syncthreads();
        stage_chunk(S, W, n, r0, c0, c1);
        __syncthreads();
        for (int r = 0; r < kEigSmall; ++r) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = S[r + (4 * ta + u) * kLd];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = S[r + (4 * tb + v) * kLd];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) g[u][v] += a[u] * b[v];
        }
    }
    double* out = Gp + ((u64)blockIdx.x * gridDim.y + blockIdx.y) * (kEigSmall * kEigSmall);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(4 * ta + u) + (4 * tb + v) * kEigSmall] = g[u][v];
}

// Step launch 2, one workgroup per pair: G = the slices' parts summed in slice order; the pair is left alone (active[pair] = 0) when all
// its columns are orthogonal to tol, otherwise Q[pair] = the rotations of kInnerSweeps sweeps over G, polished
__global__ void __launch_bounds__(kEigThreads) k_eig_rot(const double* __restrict__ Gp, int nslices, int nblocks, int P, int step, double tol,
                                                         double* __restrict__ Q, int* __restrict__ active, u64* __restrict__ ctl) {
    __shared__ EigLds L;
    const int tid = threadIdx.x;
    u64 c0, c1;
    if (!block_pair(P, step, blockIdx.x, nblocks, &c0, &c1)) return;
    if (tid == 0) L.word = 0;
    const double* gp = Gp + (u64)blockIdx.x * nslices * (kEigSmall * kEigSmall);
    for (int e = tid; e < kEigSmall * kEigSmall; e += kEigThreads) {
        double g = 0.0;
        for (int sl = 0; sl < nslices; ++sl) g += gp[(u64)sl * (kEigSmall * kEigSmall) + e];
        L.S[(e & 63) + (e >> 6) * kLd] = g;
    }
    __syncthreads();
    u64 worst = 0;
    for (int e = tid; e < kEigSmall * kEigSmall; e += kEigThreads) {
        const int p = e & 63, q = e >> 6;
        const double g = L.S[p + q * kLd];
        if (p < q && g != 0.0) {
            const double den = sqrt(L.S[p + p * kLd] * L.S[q + q * kLd]);
            if (den > 0.0) {  // a zero-norm column counts as orthogonal
                const double lim = fabs(g) / den;
                const u64 b = lim == lim ? (u64)__double_as_longlong(lim) : kNanBits;
                worst = b > worst ? b : worst;
            }
        }
    }
    if (worst) atomicMax(&L.word, worst);
    __syncthreads();
    const double lim = __longlong_as_double((long long)L.word);
    if (lim < tol) {  // uniform
        if (tid == 0) active[blockIdx.x] = 0;
        return;
    }
    double gmax = 0.0;
    for (int k = 0; k < kEigSmall; ++k) gmax = fmax(gmax, L.S[k + k * kLd]);
    lds_identity(L.U);
    __syncthreads();
    // kInnerSweeps sweeps, converged or not: a sweep over G is a sweep of one-sided rotations over the pair's 64 columns, so the whole is
    // a cyclic one-sided Jacobi in another order, and the next visit of the pair goes on where this one stopped
    (void)jacobi_lds(L, kEigSmall, kSkip * gmax, 0.1 * tol, kInnerSweeps);
    if (tid == 0) {
        atomicMax(&ctl[3], lim == lim ? L.word : kNanBits);
        active[blockIdx.x] = 1;
    }
    polish_q(L);
    __syncthreads();
    double* q = Q + (u64)blockIdx.x * (kEigSmall * kEigSmall);
    for (int e = tid; e < kEigSmall * kEigSmall; e += kEigThreads) q[e] = L.U[(e & 63) + (e >> 6) * kLd];
}

// Step launch 3, grid (pairs, row slices): the slice's rows of the pair's columns of W and of V times Q[pair]
__global__ void __launch_bounds__(kEigThreads) k_eig_apply(double* __restrict__ W, double* __restrict__ V, u64 n, int nblocks, int P, int step,
                                                           const double* __restrict__ Q, const int* __restrict__ active) {
    __shared__ EigLds L;
    u64 c0, c1;
    if (!block_pair(P, step, blockIdx.x, nblocks, &c0, &c1) || !active[blockIdx.x]) return;
    const double* q = Q + (u64)blockIdx.x * (kEigSmall * kEigSmall);
    for (int e = threadIdx.x; e < kEigSmall * kEigSmall; e += kEigThreads) L.U[(e & 63) + (e >> 6) * kLd] = q[e];
    const u64 row_lo = (u64)blockIdx.y * kSliceRows, row_hi = row_lo + kSliceRows < n ? row_lo + kSliceRows : n;
    apply_q(L, W, n, row_lo, row_hi, c0, c1);
    apply_q(L, V, n, row_lo, row_hi, c0, c1);
}

// lam[k] = V(:, k)' T(:, k) with T = As V, one workgroup per column
__global__ void __launch_bounds__(kEigThreads) k_eig_rayleigh(const double* __restrict__ V, const double* __restrict__ T, u64 n, double* __restrict__ lam) {
    __shared__ double sh4[4];
    const double *v = V + (u64)blockIdx.x * n, *t = T + (u64)blockIdx.x * n;
    double s = 0.0;
    for (u64 i = threadIdx.x; i < n; i += kEigThreads) s += v[i] * t[i];
    s = eig_block_sum(s, sh4);
    if (threadIdx.x == 0) lam[blockIdx.x] = s;
}

// stable ascending rank of lam[k]
__global__ void __launch_bounds__(kEigThreads) k_eig_rank(const double* __restrict__ lam, int n, int* __restrict__ rank) {
    const int k = blockIdx.x * kEigThreads + threadIdx.x;
    if (k >= n) return;
    const double d = lam[k];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const double o = lam[j];
        r += (o < d || (o == d && j < k)) ? 1 : 0;
    }
    rank[k] = r;
}

// right(:, rank[k]) = V(:, k), diag = diag(unscaled lam) in that order, vals alike
__global__ void __launch_bounds__(kEigThreads) k_eig_emit(const double* __restrict__ V, const double* __restrict__ lam, const int* __restrict__ rank, u64 n,
                                                          const u64* __restrict__ ctl, double* __restrict__ vals, double* __restrict__ diag,
                                                          double* __restrict__ right) {
    const int ex = scale_exponent(__longlong_as_double((long long)ctl[0]));
    const u64 total = n * n;
    for (u64 e = (u64)blockIdx.x * kEigThreads + threadIdx.x; e < total; e += (u64)gridDim.x * kEigThreads) {
        const u64 i = e % n, k = e / n, r = (u64)rank[k];
        const double d = ldexp(lam[k], ex);
        right[i + r * n] = V[e];
        diag[i + r * n] = i == r ? d : 0.0;
        if (i == 0) vals[r] = d;
    }
}

unsigned eig_grid(u64 total) { return (unsigned)std::max<u64>(1, std::min<u64>((total + kEigThreads - 1) / kEigThreads, 4096)); }

int eig_small(Context* c, const double* A, int n, double* vals, double* diag, double* right) {
    std::shared_ptr<Allocation> st;
    RMHIP_TRY(c->alloc_device(1, &st));
    u64* status = reinterpret_cast<u64*>(st->ptr);
    hipLaunchKernelGGL(k_eig_small, dim3(1), dim3(kEigThreads), 0, c->stream, A, n, vals, diag, right, status);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    u64 got = ~0ull;
    RMHIP_HIP_CHECK(hipMemcpyAsync(&got, status, sizeof got, hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    switch (got) {
        case EIG_OK: return RMHIP_OK;
        case EIG_ASYM: return fail(RMHIP_ERR_UNSUPPORTED, "eig: the matrix is not bitwise symmetric; the host path answers");
        case EIG_NONFINITE: return fail(RMHIP_ERR_UNSUPPORTED, "eig: non-finite input; the host path answers");
        default: return fail(RMHIP_ERR_UNSUPPORTED, "eig: no convergence in %d sweeps; the host path answers", kEigSweeps);
    }
}

int eig_blocked(Context* c, const double* A, u64 n, double* vals, double* diag, double* right) {
    std::shared_ptr<Allocation> ctl_mem, as_mem, w_mem, v_mem, lam_mem, rank_mem;
    RMHIP_TRY(c->alloc_device(4, &ctl_mem));
    u64* ctl = reinterpret_cast<u64*>(ctl_mem->ptr);
    RMHIP_HIP_CHECK(hipMemsetAsync(ctl, 0, 4 * sizeof(u64), c->stream));
    hipLaunchKernelGGL(k_eig_check, dim3(eig_grid(n * n)), dim3(kEigThreads), 0, c->stream, A, n, ctl);
    c->tel.kernel_launches++;
    u64 head[2] = {0, 0};
    RMHIP_HIP_CHECK(hipMemcpyAsync(head, ctl, sizeof head, hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    double amax;
    std::memcpy(&amax, &head[0], sizeof amax);
    if (!std::isfinite(amax)) return fail(RMHIP_ERR_UNSUPPORTED, "eig: non-finite input; the host path answers");
    if (head[1]) return fail(RMHIP_ERR_UNSUPPORTED, "eig: the matrix is not bitwise symmetric; the host path answers");
    RMHIP_TRY(c->alloc_device(n * n, &v_mem));
    RMHIP_TRY(c->alloc_device(n, &lam_mem));
    RMHIP_TRY(c->alloc_device(n / 2 + 1, &rank_mem));
    double *V = v_mem->ptr, *lam = lam_mem->ptr;
    int* rank = reinterpret_cast<int*>(rank_mem->ptr);
    // (a zero matrix needs no special case: every Gram matrix is zero, no pair is active, lambda = 0 and V = I)
    RMHIP_TRY(c->alloc_device(n * n, &as_mem));
    RMHIP_TRY(c->alloc_device(n * n, &w_mem));
    double *As = as_mem->ptr, *W = w_mem->ptr;
    hipLaunchKernelGGL(k_eig_colsum, dim3((unsigned)n), dim3(kEigThreads), 0, c->stream, A, n, ctl);
    hipLaunchKernelGGL(k_eig_prep, dim3(eig_grid(n * n)), dim3(kEigThreads), 0, c->stream, A, n, (const u64*)ctl, As, W, V);
    c->tel.kernel_launches += 2;
    const int nblocks = (int)((n + kEigBlock - 1) / kEigBlock), P = (nblocks + 1) & ~1;
    // columns count as orthogonal at |cos| < max(1e-15, sqrt(n) eps): the rounding level of a computed dot product of length n, the
    // tolerance of LAPACK's one-sided Jacobi (dgesvj, CTOL = sqrt(m)); 1e-15 is the threshold of svdsolve.hip
    const double tol = std::max(kOrth, std::sqrt((double)n) * 0x1p-52);
    bool converged = false;
    const unsigned pairs = (unsigned)(P / 2), nslices = (unsigned)((n + kSliceRows - 1) / kSliceRows);
    std::shared_ptr<Allocation> gp_mem, q_mem, act_mem;
    RMHIP_TRY(c->alloc_device((size_t)pairs * nslices * kEigSmall * kEigSmall, &gp_mem));
    RMHIP_TRY(c->alloc_device((size_t)pairs * kEigSmall * kEigSmall, &q_mem));
    RMHIP_TRY(c->alloc_device(pairs / 2 + 1, &act_mem));
    int* active = reinterpret_cast<int*>(act_mem->ptr);
    for (int sweep = 0; sweep < kEigSweeps && !converged; ++sweep) {
        RMHIP_HIP_CHECK(hipMemsetAsync(ctl + 3, 0, sizeof(u64), c->stream));
        for (int step = 0; step < P - 1; ++step) {
            hipLaunchKernelGGL(k_eig_gram, dim3(pairs, nslices), dim3(kEigThreads), 0, c->stream, (const double*)W, n, nblocks, P, step, gp_mem->ptr);
            hipLaunchKernelGGL(k_eig_rot, dim3(pairs), dim3(kEigThreads), 0, c->stream, (const double*)gp_mem->ptr, (int)nslices, nblocks, P, step, tol,
                               q_mem->ptr, active, ctl);
            hipLaunchKernelGGL(k_eig_apply, dim3(pairs, nslices), dim3(kEigThreads), 0, c->stream, W, V, n, nblocks, P, step, (const double*)q_mem->ptr,
                               (const int*)active);
        }
        c->tel.kernel_launches += 3 * (uint64_t)(P - 1);
        RMHIP_HIP_CHECK(hipGetLastError());
        u64 bits = 0;
        RMHIP_HIP_CHECK(hipMemcpyAsync(&bits, ctl + 3, sizeof bits, hipMemcpyDeviceToHost, c->stream));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
        double off;
        std::memcpy(&off, &bits, sizeof off);
        if (!(off == off)) return fail(RMHIP_ERR_UNSUPPORTED, "eig: non-finite data in a block pair; the host path answers");
        RMHIP_TRACEF("eig: n %llu sweep %d largest |cos| of an active pair %.3g (tol %.3g)", n, sweep, off, tol);
        converged = off < tol;  // no pair was active
    }
    if (!converged) return fail(RMHIP_ERR_UNSUPPORTED, "eig: no convergence in %d sweeps; the host path answers", kEigSweeps);
    RMHIP_TRY(launch_dgemm(c, n, n, n, 1.0, As, n, V, n, 0.0, W, n));  // W is free now: T = As V
    hipLaunchKernelGGL(k_eig_rayleigh, dim3((unsigned)n), dim3(kEigThreads), 0, c->stream, (const double*)V, (const double*)W, n, lam);
    c->tel.kernel_launches++;
    hipLaunchKernelGGL(k_eig_rank, dim3((unsigned)((n + kEigThreads - 1) / kEigThreads)), dim3(kEigThreads), 0, c->stream, (const double*)lam, (int)n, rank);
    hipLaunchKernelGGL(k_eig_emit, dim3(eig_grid(n * n)), dim3(kEigThreads), 0, c->stream, (const double*)V, (const double*)lam, (const int*)rank, n,
                       (const u64*)ctl, vals, diag, right);
    c->tel.kernel_launches += 2;
    RMHIP_HIP_CHECK(hipGetLastError());
    // the workspaces go back to the pool while the launches above may still be queued: same stream, so the next user orders after them
    return RMHIP_OK;
}

}  // namespace
}  // namespace rmhip

int rmhip_eig(rmhip_ctx* ctx, rmhip_buf a, int compute_left, rmhip_buf out4[4]) {
    CTX_OR_FAIL(ctx);
    if (!out4) return fail(RMHIP_ERR_INVALID, "eig: null output");
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    Buffer ab;
    RMHIP_TRY(c->lookup(a, &ab));
    if (ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "eig: complex input; the host path answers");
    const std::vector<size_t>& s = ab.shape;
    for (size_t d = 2; d < s.size(); ++d)
        if (s[d] != 1) return fail(RMHIP_ERR_INVALID, "eig: input must be 2-D");
    const size_t rows = s.empty() ? 1 : s[0], cols = s.size() < 2 ? 1 : s[1];
    if (rows != cols) return fail(RMHIP_ERR_INVALID, "eig: input must be a square matrix (%zu x %zu)", rows, cols);  // eig.rs:507-512
    const size_t n = rows;
    if (n > (size_t)kEigMaxN) return fail(RMHIP_ERR_UNSUPPORTED, "eig: order %zu is above %d; the host path answers", n, kEigMaxN);
    RMHIP_TRY(c->get(a, &ab));
    const size_t shv[2] = {n, n ? (size_t)1 : (size_t)0}, shm[2] = {n, n};
    Buffer vb, db, rb, lb;
    int rc = c->new_buffer(shv, 2, &out4[0], &vb);
    if (!rc) rc = c->new_buffer(shm, 2, &out4[1], &db);
    if (!rc) rc = c->new_buffer(shm, 2, &out4[2], &rb);
    if (!rc && compute_left) rc = c->new_buffer(shm, 2, &out4[3], &lb);
    if (!rc && n > 0) {
        rc = n <= (size_t)kEigSmall ? eig_small(c, ab.data(), (int)n, vb.data(), db.data(), rb.data())
                                    : eig_blocked(c, ab.data(), (u64)n, vb.data(), db.data(), rb.data());
        if (!rc && compute_left && hipMemcpyAsync(lb.data(), rb.data(), n * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = fail(RMHIP_ERR_HIP, "eig: copy failed");
    }
    if (rc) {
        for (int i = 0; i < 4; ++i) {
            if (out4[i]) rmhip_free(ctx, out4[i]);
            out4[i] = 0;
        }
    }
    return rc;
}
