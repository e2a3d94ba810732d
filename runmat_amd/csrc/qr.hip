// qr.hip -- `qr(a, options)` (crates/runmat-accelerate-api/src/lib.rs:2509-2515 -> ProviderQrResult { q, r, perm_matrix, perm_vector }
// :665-670).  The contract is the reference's CPU builtin (builtins/math/linalg/factor/qr.rs:576-870): column-pivoted Householder QR whose
// pivot is the arg-max (ties: the LAST index) of the squared norms of rows k..m-1 RECOMPUTED from the current matrix before every step,
// reflectors with the builtin's quirks (householder, :742-792), Q = H_0 ... H_{p-1} I, R = the cleaned upper trapezoid, both cleaned at
// |x| <= 1e-12.
//
// Factorisation: right-looking Householder with the rank-1 trailing update, four launches per column, all of them spread over the rows:
//     k_qr_pivot    column blocks: squared norms from the previous step's per-slice partial sums (fixed order), block arg-max
//     k_qr_swap     row blocks:    global arg-max from the block results, whole-column swap, permutation swap, partial sums of the tail
//     k_qr_reflect  rows x cols:   reflector scalars from the tail sums (every block alike), v for the block's rows, partial A(k:m, j)' v
//     k_qr_update   rows x cols:   dot_j = tau * sum of the partials, A(k:m, j) -= v dot_j, partial sums of squares of rows k+1..m-1
// The norms the next pivot reads are therefore RECOMPUTED from the updated matrix, as the reference does, in one fused pass with the
// update (no downdating, no cancellation restarts); the only difference from the host loop is summation order.  No float atomics: every
// reduction is a per-slice partial plus a fixed-order sum.
//
// Q: reflectors accumulated backwards onto the identity in panels of kQrNb, compact WY (T from V'V as dlarft forms it), three dgemms per
// panel (V' Q, T W, Q -= V W2).  A tau == 0 reflector has a zero row and column in T and drops out.
//
// Refused (RMHIP_ERR_UNSUPPORTED, the builtin's host path answers): more than two dimensions, a non-finite entry, max |a| >= 1e150 (the
// reference's x d / d^2 forms overflow beyond that), a full Q that does not fit in device memory.  Detecting the first two costs the one
// device -> host read of a call, taken from the first norm pass.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
constexpr double kEpsClean = 1.0e-12;  // EPS_CLEAN, qr.rs:1025
constexpr int kQrNb = 32;              // reflectors per compact-WY panel of Q
constexpr int kCb = 16;                // trailing columns per block of the two-dimensional kernels (4 per wave)
constexpr int kSwapRows = 1024;        // rows per block of k_qr_swap (4 per thread)

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;  // lane 0
}

// 256 threads: fixed-order block sum (lane sums, wave tree, waves in order); the result is valid in thread 0
__device__ __forceinline__ double block_sum(double s, double* sh4) {
    s = wave_sum(s);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh4[w] = s;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// First pass: W = A, per-slice partial sums of squares of every column, max |a| as bits (NaN payloads order above +Inf) into *flag.
template <int RPL>
__global__ void __launch_bounds__(256) k_qr_init(const double* __restrict__ A, double* __restrict__ W, u64 m, u64 n,
                                                 double* __restrict__ Pn, unsigned long long* __restrict__ flag) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 rs = blockIdx.x, r0 = rs * (u64)(64 * RPL);
    unsigned long long mx = 0;
#pragma unroll
    for (int t = 0; t < kCb / 4; ++t) {
        const u64 col = (u64)blockIdx.y * kCb + (u64)w + 4u * (u64)t;
        if (col >= n) break;
        double ss = 0.0;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const u64 i = r0 + (u64)lane + 64u * (u64)q;
            if (i < m) {
                const double x = A[i + col * m];
                W[i + col * m] = x;
                ss += x * x;
                const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(x));
                mx = b > mx ? b : mx;
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) Pn[rs * n + col] = ss;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && mx) atomicMax(flag, mx);
}

// Step k, launch 1: norms of columns k..n-1 (rows k..m-1) = sum over slices rs_lo..gr-1 of the partials, block arg-max (ties: last index)
__global__ void __launch_bounds__(256) k_qr_pivot(const double* __restrict__ Pn, u64 n, u64 k, u64 rs_lo, u64 gr, double* __restrict__ best) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const u64 col = k + (u64)blockIdx.x * 256 + threadIdx.x;
    double v = -1.0;
    long long idx = -1;
    if (col < n) {
        double s = 0.0;
        for (u64 r = rs_lo; r < gr; ++r) s += Pn[r * n + col];
        v = s;
        idx = (long long)col;
    }
    sv[threadIdx.x] = v;
    si[threadIdx.x] = idx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double ov = sv[threadIdx.x + h];
            const long long oi = si[threadIdx.x + h];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi > si[threadIdx.x])) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best[2 * blockIdx.x] = sv[0];
        best[2 * blockIdx.x + 1] = (double)si[0];
    }
}

// Step k, launch 2: pivot = arg-max over the pivot blocks; swap whole columns k and pivot; partial sums of squares of the new column's tail
__global__ void __launch_bounds__(256) k_qr_swap(double* __restrict__ W, u64 m, u64 k, const double* __restrict__ best, int nbest,
                                                 int* __restrict__ perm, double* __restrict__ S) {
    __shared__ u64 piv_s;
    __shared__ double sh4[4];
    if (threadIdx.x == 0) {
        double bv = -2.0, bi = -1.0;
        for (int b = 0; b < nbest; ++b) {
            const double v = best[2 * b], i = best[2 * b + 1];
            if (v > bv || (v == bv && i > bi)) {
                bv = v;
                bi = i;
            }
        }
        piv_s = bi < 0.0 ? k : (u64)bi;
    }
    __syncthreads();
    const u64 piv = piv_s;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kSwapRows / 256; ++q) {
        const u64 i = (u64)blockIdx.x * kSwapRows + threadIdx.x + 256u * (u64)q;
        if (i < m) {
            const double a = W[i + piv * m];
            if (piv != k) {
                W[i + piv * m] = W[i + k * m];
                W[i + k * m] = a;
            }
            if (i > k) s += a * a;
        }
    }
    s = block_sum(s, sh4);
    if (threadIdx.x == 0) {
        S[blockIdx.x] = s;
        if (blockIdx.x == 0 && piv != k) {
            const int t = perm[k];
            perm[k] = perm[piv];
            perm[piv] = t;
        }
    }
}

// householder (qr.rs:742-792) for a real column: mode 0 = column zeroed, 1 = tail zeroed (tau 0, R(k,k) = alpha), 2 = reflect.
// num-complex division of real values is x d / d^2: tau and the tail scaling use that form.
struct Reflector {
    int mode;
    double tau, diag, d, dd;
    bool zero_tail;
};
__device__ __forceinline__ Reflector make_reflector(double alpha, double t) {
    Reflector r{2, 0.0, 0.0, 0.0, 1.0, false};
    const double aa = fabs(alpha);
    if (t <= kEpsClean && aa <= kEpsClean) {
        r.mode = 0;
        r.zero_tail = true;
        return r;
    }
    if (t <= kEpsClean && alpha >= 0.0) {
        r.mode = 1;
        r.zero_tail = true;
        r.diag = alpha;
        return r;
    }
    const double total = sqrt(aa * aa + t);
    const double sign = aa <= kEpsClean ? 1.0 : (alpha * aa) / (aa * aa);
    const double beta = -sign * total;
    r.tau = fabs(beta) <= kEpsClean ? 0.0 : ((beta - alpha) * beta) / (beta * beta);
    r.d = alpha - beta;
    r.dd = r.d * r.d;
    r.zero_tail = fabs(r.d) <= kEpsClean;
    r.diag = beta;
    return r;
}

// Step k, launch 3: reflector scalars (every block alike from the same partial sums), v of the block's rows (row k: 1), partial dots
// P[rs, j] = sum_{i in slice, i >= k} A(i, j) v_i for the block's trailing columns j > k.
template <int RPL>
__global__ void __launch_bounds__(256) k_qr_reflect(const double* __restrict__ W, u64 m, u64 n, u64 k, u64 rs0, const double* __restrict__ S,
                                                    int ns, double* __restrict__ vbuf, double* __restrict__ P, double* __restrict__ scal,
                                                    double* __restrict__ taus) {
    __shared__ double sh[3];
    __shared__ int sscale;
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int b = 0; b < ns; ++b) t += S[b];
        const Reflector r = make_reflector(W[k + k * m], t);
        sh[0] = r.tau;
        sh[1] = r.d;
        sh[2] = r.dd;
        sscale = r.zero_tail ? 0 : 1;
        if (blockIdx.x == 0 && blockIdx.y == 0) {
            scal[0] = r.tau;
            scal[1] = r.diag;
            taus[k] = r.tau;
        }
    }
    __syncthreads();
    const double tau = sh[0], d = sh[1], dd = sh[2];
    const bool scale_tail = sscale != 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 rs = rs0 + blockIdx.x, r0 = rs * (u64)(64 * RPL);
    double v[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const u64 i = r0 + (u64)lane + 64u * (u64)q;
        double x = 0.0;
        if (i == k) x = 1.0;
        else if (i > k && i < m) x = scale_tail ? (W[i + k * m] * d) / dd : 0.0;
        v[q] = x;
        if (blockIdx.y == 0 && i > k && i < m) vbuf[i] = x;
    }
    if (tau == 0.0) return;  // apply_householder is skipped (qr.rs:710)
#pragma unroll
    for (int t = 0; t < kCb / 4; ++t) {
        const u64 col = k + 1 + (u64)blockIdx.y * kCb + (u64)w + 4u * (u64)t;
        if (col >= n) break;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const u64 i = r0 + (u64)lane + 64u * (u64)q;
            if (i >= k && i < m) s += v[q] * W[i + col * m];
        }
        s = wave_sum(s);
        if (lane == 0) P[rs * n + col] = s;
    }
}

// Step k, launch 4: dot_j = tau * sum_rs P[rs, j]; A(k:m, j) -= v dot_j; partial sums of squares of rows k+1..m-1 for the next pivot.
// Blocks of column block 0 also store the reflector into column k (v below the diagonal, R(k,k) on it).
template <int RPL>
__global__ void __launch_bounds__(256) k_qr_update(double* __restrict__ W, u64 m, u64 n, u64 k, u64 rs0, u64 gr, const double* __restrict__ vbuf,
                                                   const double* __restrict__ P, double* __restrict__ Pn, const double* __restrict__ scal) {
    const double tau = scal[0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 rs = rs0 + blockIdx.x, r0 = rs * (u64)(64 * RPL);
    double v[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const u64 i = r0 + (u64)lane + 64u * (u64)q;
        v[q] = i == k ? 1.0 : ((i > k && i < m) ? vbuf[i] : 0.0);
        if (blockIdx.y == 0 && w == 0) {
            if (i == k) W[k + k * m] = scal[1];
            else if (i > k && i < m) W[i + k * m] = v[q];
        }
    }
#pragma unroll
    for (int t = 0; t < kCb / 4; ++t) {
        const u64 col = k + 1 + (u64)blockIdx.y * kCb + (u64)w + 4u * (u64)t;
        if (col >= n) break;
        double dot = 0.0;
        if (tau != 0.0) {
            double s = 0.0;
            for (u64 r = rs0 + (u64)lane; r < gr; r += 64) s += P[r * n + col];
            s = wave_sum(s);
            dot = __shfl(s, 0, 64) * tau;
        }
        double ss = 0.0;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const u64 i = r0 + (u64)lane + 64u * (u64)q;
            if (i >= k && i < m) {
                double x = W[i + col * m];
                if (tau != 0.0) {
                    x = x - v[q] * dot;
                    W[i + col * m] = x;
                }
                if (i > k) ss += x * x;
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) Pn[rs * n + col] = ss;
    }
}

// unit-lower copy of the panel's reflectors: V[r, l] = 1 (r == l), 0 (r < l), W(k0 + r, k0 + l) below
__global__ void __launch_bounds__(256) k_qr_vcopy(const double* __restrict__ W, u64 m, u64 k0, int kb, double* __restrict__ V) {
    const u64 rows = m - k0, total = rows * (u64)kb;
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) {
        const u64 r = e % rows, l = e / rows;
        V[e] = r == l ? 1.0 : (r < l ? 0.0 : W[(k0 + r) + (k0 + l) * m]);
    }
}

// dlarft (forward, columnwise) from G = V'V: T(i,i) = tau_i, T(0:i, i) = T(0:i, 0:i) * (-tau_i G(0:i, i)).  One block, kb <= 64.
__global__ void __launch_bounds__(64) k_qr_larft(const double* __restrict__ G, const double* __restrict__ taus, int kb, double* __restrict__ Tout) {
    __shared__ double T[kQrNb][kQrNb + 1];
    __shared__ double wv[kQrNb];
    const int r = threadIdx.x;
    for (int i = 0; i < kb; ++i) {
        const double ti = taus[i];
        if (r < i) wv[r] = -ti * G[r + (u64)i * kb];
        __syncthreads();
        if (r < i) {
            double s = 0.0;
            for (int q = r; q < i; ++q) s += T[r][q] * wv[q];
            T[r][i] = s;
        }
        if (r == i) T[i][i] = ti;
        if (r > i && r < kb) T[r][i] = 0.0;
        __syncthreads();
    }
    for (int col = 0; col < kb; ++col)
        if (r < kb) Tout[r + (u64)col * kb] = T[r][col];
}

__global__ void __launch_bounds__(256) k_qr_eye(double* __restrict__ Q, u64 m, u64 ncq) {
    const u64 total = m * ncq;
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) Q[e] = (e % m) == (e / m) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(256) k_qr_clean(double* __restrict__ Q, u64 total) {
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) {
        const double x = Q[e];
        Q[e] = fabs(x) <= kEpsClean ? 0.0 : x;
    }
}

// R = the cleaned upper trapezoid of the factored matrix, rr rows (m, or n in economy mode with m >= n)
__global__ void __launch_bounds__(256) k_qr_r(const double* __restrict__ W, u64 m, u64 n, u64 rr, double* __restrict__ R) {
    const u64 total = rr * n;
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) {
        const u64 i = e % rr, j = e / rr;
        double x = 0.0;
        if (i <= j) {
            x = W[i + j * m];
            if (fabs(x) <= kEpsClean) x = 0.0;
        }
        R[e] = x;
    }
}

// perm_matrix E(perm[c], c) = 1 (n x n) and perm_vector perm[c] + 1 (n x 1)
__global__ void __launch_bounds__(256) k_qr_perm(const int* __restrict__ perm, u64 n, double* __restrict__ E, double* __restrict__ pv) {
    const u64 total = n * n;
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) {
        const u64 i = e % n, j = e / n;
        E[e] = (u64)perm[j] == i ? 1.0 : 0.0;
        if (i == 0) pv[j] = (double)(perm[j] + 1);
    }
}

__global__ void __launch_bounds__(256) k_qr_iota(int* __restrict__ perm, u64 n) {
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < n; e += (u64)gridDim.x * 256) perm[e] = (int)e;
}

unsigned grid_for(u64 total) {
    const u64 b = (total + 255) / 256;
    return (unsigned)std::max<u64>(1, std::min<u64>(b, 4096));
}

int rows_per_lane(u64 m) {  // slices of 64 * RPL rows, at most ~64 slices: the per-slice partials stay cheap to sum
    const u64 want = (m + 64 * 64 - 1) / (64 * 64);
    return want <= 4 ? 4 : want <= 8 ? 8 : want <= 16 ? 16 : 32;
}

template <int RPL>
int factor_steps(Context* c, double* A, double* W, u64 m, u64 n, double* Pn, double* P, double* best, double* S, double* vbuf, double* scal,
                 double* taus, int* perm, unsigned long long* flag) {
    const u64 rsz = 64 * RPL, gr = (m + rsz - 1) / rsz, p = std::min(m, n);
    const unsigned ncb0 = (unsigned)((n + kCb - 1) / kCb);
    RMHIP_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_qr_init<RPL>, dim3((unsigned)gr, ncb0), dim3(256), 0, c->stream, A, W, m, n, Pn, flag);
    hipLaunchKernelGGL(k_qr_iota, dim3(grid_for(n)), dim3(256), 0, c->stream, perm, n);
    c->tel.kernel_launches += 2;
    unsigned long long got = 0;
    RMHIP_HIP_CHECK(hipMemcpyAsync(&got, flag, sizeof got, hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    double amax;
    std::memcpy(&amax, &got, sizeof amax);
    if (!(amax < 1.0e150)) {  // NaN (payload bits above +Inf), Inf, or large enough for the reference's d^2 forms to overflow
        return fail(RMHIP_ERR_UNSUPPORTED, "qr: %s input; the host path answers", std::isfinite(amax) ? "max |a| >= 1e150" : "non-finite");
    }
    const unsigned g2 = (unsigned)((m + kSwapRows - 1) / kSwapRows);
    for (u64 k = 0; k < p; ++k) {
        const u64 rs0 = k / rsz, rs_lo = k == 0 ? 0 : (k - 1) / rsz;
        const unsigned nb1 = (unsigned)((n - k + 255) / 256);
        hipLaunchKernelGGL(k_qr_pivot, dim3(nb1), dim3(256), 0, c->stream, (const double*)Pn, n, k, rs_lo, gr, best);
        hipLaunchKernelGGL(k_qr_swap, dim3(g2), dim3(256), 0, c->stream, W, m, k, (const double*)best, (int)nb1, perm, S);
        const unsigned ncb = (unsigned)std::max<u64>(1, (n - k - 1 + kCb - 1) / kCb);
        const dim3 g2d((unsigned)(gr - rs0), ncb);
        hipLaunchKernelGGL(k_qr_reflect<RPL>, g2d, dim3(256), 0, c->stream, (const double*)W, m, n, k, rs0, (const double*)S, (int)g2, vbuf, P,
                           scal, taus);
        hipLaunchKernelGGL(k_qr_update<RPL>, g2d, dim3(256), 0, c->stream, W, m, n, k, rs0, gr, (const double*)vbuf, (const double*)P, Pn,
                           (const double*)scal);
        c->tel.kernel_launches += 4;
    }
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

// Q(:, 0:ncq) = H_0 ... H_{p-1} I, panels of kQrNb applied backwards to the columns they touch
int build_q(Context* c, const double* W, u64 m, u64 p, const double* taus, double* Q, u64 ncq) {
    hipLaunchKernelGGL(k_qr_eye, dim3(grid_for(m * ncq)), dim3(256), 0, c->stream, Q, m, ncq);
    c->tel.kernel_launches++;
    if (p > 0) {
        std::shared_ptr<Allocation> v, g, t, w1, w2;
        RMHIP_TRY(c->alloc_device(m * kQrNb, &v));
        RMHIP_TRY(c->alloc_device(kQrNb * kQrNb, &g));
        RMHIP_TRY(c->alloc_device(kQrNb * kQrNb, &t));
        RMHIP_TRY(c->alloc_device(kQrNb * ncq, &w1));
        RMHIP_TRY(c->alloc_device(kQrNb * ncq, &w2));
        for (u64 k0 = ((p - 1) / kQrNb) * kQrNb;; k0 -= kQrNb) {
            const int kb = (int)std::min<u64>(kQrNb, p - k0);
            const u64 rows = m - k0, cols = ncq - k0;
            hipLaunchKernelGGL(k_qr_vcopy, dim3(grid_for(rows * kb)), dim3(256), 0, c->stream, W, m, k0, kb, v->ptr);
            c->tel.kernel_launches++;
            RMHIP_TRY(launch_dgemm_trans(c, true, false, kb, kb, rows, 1.0, v->ptr, rows, v->ptr, rows, 0.0, g->ptr, kb));
            hipLaunchKernelGGL(k_qr_larft, dim3(1), dim3(64), 0, c->stream, (const double*)g->ptr, taus + k0, kb, t->ptr);
            c->tel.kernel_launches++;
            double* Qs = Q + k0 + k0 * m;
            RMHIP_TRY(launch_dgemm_trans(c, true, false, kb, cols, rows, 1.0, v->ptr, rows, Qs, m, 0.0, w1->ptr, kb));
            RMHIP_TRY(launch_dgemm(c, kb, cols, kb, 1.0, t->ptr, kb, w1->ptr, kb, 0.0, w2->ptr, kb));
            RMHIP_TRY(launch_dgemm(c, rows, cols, kb, -1.0, v->ptr, rows, w2->ptr, kb, 1.0, Qs, m));
            if (k0 == 0) break;
        }
        // the panel scratch goes back to the pool while the dgemms above may still be queued: same stream, so the next user orders after them
    }
    hipLaunchKernelGGL(k_qr_clean, dim3(grid_for(m * ncq)), dim3(256), 0, c->stream, Q, m * ncq);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace
}  // namespace rmhip

int rmhip_qr(rmhip_ctx* ctx, rmhip_buf a, int economy, int pivot_vector, rmhip_buf out4[4]) {
    CTX_OR_FAIL(ctx);
    (void)pivot_vector;  // ProviderQrOptions.pivot only selects which output the builtin shows: both are always returned
    if (!out4) return fail(RMHIP_ERR_INVALID, "qr: null output");
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    Buffer ab;
    RMHIP_TRY(c->lookup(a, &ab));
    if (ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "qr: complex input; the host path answers");
    if (ab.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "qr: input must be 2-D");  // from_tensor, qr.rs:899
    RMHIP_TRY(c->get(a, &ab));
    const std::vector<size_t>& s = ab.shape;
    const u64 m = s.empty() ? 1 : s[0], n = s.size() < 2 ? 1 : s[1], p = std::min(m, n);
    const bool econ = economy && m >= n;
    const u64 ncq = econ ? n : m, rr = econ ? n : m;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const double need = 8.0 * ((double)m * ncq + 2.0 * (double)m * n + (double)rr * n + 2.0 * (double)n * n + 2.0 * kQrNb * (double)(m + ncq));
        if (need > 0.9 * (double)(free_b + c->pooled_bytes))
            return fail(RMHIP_ERR_UNSUPPORTED, "qr: %s needs %.3g bytes of device memory; the host path answers", econ ? "economy" : "full", need);
    }
    const size_t shq[2] = {(size_t)m, (size_t)ncq}, shr[2] = {(size_t)rr, (size_t)n}, she[2] = {(size_t)n, (size_t)n}, shv[2] = {(size_t)n, 1};
    Buffer qb, rb, eb, vb;
    int rc = c->new_buffer(shq, 2, &out4[0], &qb);
    if (!rc) rc = c->new_buffer(shr, 2, &out4[1], &rb);
    if (!rc) rc = c->new_buffer(she, 2, &out4[2], &eb);
    if (!rc) rc = c->new_buffer(shv, 2, &out4[3], &vb);
    std::shared_ptr<Allocation> wk, pn, pp, best, sbuf, vbuf, scal, taus, perm, flag;
    const int rpl = rows_per_lane(std::max<u64>(m, 1));
    const u64 gr = (m + 64 * rpl - 1) / (64 * rpl);
    if (!rc) rc = c->alloc_device(std::max<u64>(1, m * n), &wk);
    if (!rc) rc = c->alloc_device(std::max<u64>(1, gr * n), &pn);
    if (!rc) rc = c->alloc_device(std::max<u64>(1, gr * n), &pp);
    if (!rc) rc = c->alloc_device(2 * ((n + 255) / 256) + 2, &best);
    if (!rc) rc = c->alloc_device((m + kSwapRows - 1) / kSwapRows + 1, &sbuf);
    if (!rc) rc = c->alloc_device(std::max<u64>(1, m), &vbuf);
    if (!rc) rc = c->alloc_device(4, &scal);
    if (!rc) rc = c->alloc_device(std::max<u64>(1, p), &taus);
    if (!rc) rc = c->alloc_device(n / 2 + 1, &perm);
    if (!rc) rc = c->alloc_device(1, &flag);
    int* permp = perm ? reinterpret_cast<int*>(perm->ptr) : nullptr;
    if (!rc && m * n == 0) {  // p = 0: identity permutation, Q = eye, R = zeros
        hipLaunchKernelGGL(k_qr_iota, dim3(grid_for(n)), dim3(256), 0, c->stream, permp, n);
        c->tel.kernel_launches++;
    } else if (!rc) {
        unsigned long long* fl = reinterpret_cast<unsigned long long*>(flag->ptr);
        switch (rpl) {
            case 4: rc = factor_steps<4>(c, ab.data(), wk->ptr, m, n, pn->ptr, pp->ptr, best->ptr, sbuf->ptr, vbuf->ptr, scal->ptr, taus->ptr, permp, fl); break;
            case 8: rc = factor_steps<8>(c, ab.data(), wk->ptr, m, n, pn->ptr, pp->ptr, best->ptr, sbuf->ptr, vbuf->ptr, scal->ptr, taus->ptr, permp, fl); break;
            case 16: rc = factor_steps<16>(c, ab.data(), wk->ptr, m, n, pn->ptr, pp->ptr, best->ptr, sbuf->ptr, vbuf->ptr, scal->ptr, taus->ptr, permp, fl); break;
            default: rc = factor_steps<32>(c, ab.data(), wk->ptr, m, n, pn->ptr, pp->ptr, best->ptr, sbuf->ptr, vbuf->ptr, scal->ptr, taus->ptr, permp, fl); break;
        }
    }
    if (!rc && m * ncq > 0) rc = build_q(c, wk->ptr, m, m * n == 0 ? 0 : p, taus->ptr, qb.data(), ncq);
    if (!rc && rr * n > 0) {
        hipLaunchKernelGGL(k_qr_r, dim3(grid_for(rr * n)), dim3(256), 0, c->stream, (const double*)wk->ptr, m, n, rr, rb.data());
        c->tel.kernel_launches++;
    }
    if (!rc && n > 0) {
        hipLaunchKernelGGL(k_qr_perm, dim3(grid_for(n * n)), dim3(256), 0, c->stream, (const int*)permp, n, eb.data(), vb.data());
        c->tel.kernel_launches++;
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(RMHIP_ERR_HIP, "qr: launch failed");
    if (rc) {
        for (int i = 0; i < 4; ++i) {
            if (out4[i]) rmhip_free(ctx, out4[i]);
            out4[i] = 0;
        }
    }
    return rc;
}
