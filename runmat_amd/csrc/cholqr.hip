// cholqr.hip -- `qr_power_iter(product, product_lhs, q_handle, options)` (crates/runmat-accelerate-api/src/lib.rs:2522-2531 ->
// Option<ProviderQrPowerIterResult { q, r, perm_matrix, perm_vector }> :673-678): the economy QR of a tall matmul product inside the
// power-iteration loop `[Q, R] = qr(G*Q, 'econ')` (builtins/math/linalg/factor/qr.rs:436-458).  The product has at most 64 columns and is
// far from rank deficient there, so no pivoting is needed and the factorisation is CholeskyQR2 in f64:
//     G1 = P'P,   R1 = chol(G1),  X1 = inv(R1),  Q1 = P X1
//     G2 = Q1'Q1, R2 = chol(G2),  X2 = inv(R2),  Q  = Q1 X2,  R = R2 R1,  identity permutation
// Two verdicts decide whether the result is returned at all (otherwise the call DECLINES - the trait's Ok(None) - and the caller runs qr):
//     A  every Cholesky pivot g_jj - sum_p r_pj^2 is finite and > 0.  A NaN or Inf anywhere in column j, squares that overflow, an all-zero
//        or underflowed Gram matrix all make a pivot fail, so no separate pass looks for them.
//     B  ||G2 - I||_F <= 1/2: then cond(Q1) <= sqrt(3) and the second pass restores orthogonality to rounding level.
// Kernels (every pass streams the m x k data once, 8 m k bytes; no launch chain per column):
//     k_cq_gram    row slices: the slice's partial upper triangle of P'P, 4 x 4 register tiles, rows staged through LDS
//     k_cq_sum     the partials added in a fixed order (16 segments of consecutive slices, then the segments in order)
//     k_cq_factor  one block: Cholesky row by row with in-order dot products, the inverse by back-substitution, both in LDS; the second
//                  call checks verdict B first and writes R = R2 R1 (exact zeros below the diagonal) and the two permutation outputs
//     k_cq_apply   row slices, one row per thread in registers: Y = X inv(R) over the triangle's terms only, inv(R) in LDS; the first
//                  call also forms the slice's partial Gram matrix of Q1
// All sums run in a fixed order and there are no float atomics: the same input gives the same bits.  One device -> host read per call (the
// verdict word, after the second factor kernel).  After a failed verdict A the launches already queued compute on NaNs: they branch on
// nothing data-dependent and index nothing by data, so they are harmless.
//
// Departures from the reference's wgpu backend (ops/linalg/decomposition.rs:243-421), on purpose: no input is freed or written (the wgpu
// code frees `product` and may overwrite q_handle's storage; its caller frees the product itself); no EPS clamps (they return a
// non-orthogonal Q for a rank-deficient product - here such a product declines); `product_lhs` is validated and otherwise unused (the
// reference recomputes a zero product from it - here a zero product declines); f64, two passes.
#include <algorithm>
#include <cmath>

#include "common.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
constexpr int kCqMaxCols = 64;
constexpr int kCqChunk = 64;       // rows staged per step of the Gram tiles
constexpr int kCqMaxParts = 512;   // row slices (partials) per pass at most
constexpr int kCqSeg = 16;         // segments of k_cq_sum
constexpr int kCqLds = 64 * 66;    // doubles: the staged chunk [64][KP + 2], reused for the tile groups' results (4096)
constexpr unsigned kFailA1 = 1, kFailB = 2, kFailA2 = 3;

// 256 threads as T = (KP/4)^2 tiles of 4 x 4 times G = 256 / T row groups: group g takes rows g, g + G, ... of a chunk
template <int KP>
struct CqGeom {
    static constexpr int NT = KP / 4, T = NT * NT, G = 256 / T, LD = KP + 2;
};

template <int KP>
__device__ __forceinline__ void cq_gram_chunk(const double* __restrict__ L, double (&acc)[4][4]) {
    typedef CqGeom<KP> Ge;
    const int tt = threadIdx.x % Ge::T, g = threadIdx.x / Ge::T, ti = tt / Ge::NT, tj = tt % Ge::NT;
    if (ti > tj) return;  // upper triangle of tiles
    for (int r = g; r < kCqChunk; r += Ge::G) {
        const double* row = L + r * Ge::LD;
        double a[4], b[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            a[x] = row[4 * ti + x];
            b[x] = row[4 * tj + x];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
    }
}

// the row groups' tiles added in group order; entry (i, j) of the k x k partial for every tile of the upper triangle.
// Every thread calls this after the block's last cq_gram_chunk; L is overwritten.
template <int KP>
__device__ __forceinline__ void cq_gram_store(double* __restrict__ L, const double (&acc)[4][4], int k, double* __restrict__ part) {
    typedef CqGeom<KP> Ge;
    __syncthreads();
    const int tt = threadIdx.x % Ge::T, g = threadIdx.x / Ge::T;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) L[(g * Ge::T + tt) * 16 + x * 4 + y] = acc[x][y];
    __syncthreads();
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        const int et = e >> 4, x = (e >> 2) & 3, y = e & 3, ti = et / Ge::NT, tj = et % Ge::NT;
        const int i = 4 * ti + x, j = 4 * tj + y;
        if (ti > tj || i >= k || j >= k) continue;
        double s = L[e];
        for (int q = 1; q < Ge::G; ++q) s += L[q * KP * KP + e];
        part[i + j * k] = s;
    }
}

template <int KP>
__global__ void __launch_bounds__(256) k_cq_gram(const double* __restrict__ P, u64 m, int k, u64 rpb, double* __restrict__ parts) {
    typedef CqGeom<KP> Ge;
    __shared__ __attribute__((aligned(16))) double L[kCqLds];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[4][4] = {};
    const u64 row0 = (u64)blockIdx.x * rpb, rend = std::min<u64>(m, row0 + rpb);
    for (u64 c0 = row0; c0 < rend; c0 += kCqChunk) {
        const u64 i = c0 + (u64)lane;
#pragma unroll
        for (int q = 0; q < KP / 4; ++q) {
            const int j = w + 4 * q;
            L[lane * Ge::LD + j] = (j < k && i < m) ? P[i + (u64)j * m] : 0.0;
        }
        __syncthreads();
        cq_gram_chunk<KP>(L, acc);
        __syncthreads();
    }
    cq_gram_store<KP>(L, acc, k, parts + (u64)blockIdx.x * (u64)(k * k));
}

// G(i, j), i <= j = the nb partials in a fixed order: segment s adds partials s per .. (s + 1) per - 1 in order, then the segments in order
__global__ void __launch_bounds__(256) k_cq_sum(const double* __restrict__ parts, int nb, int k, double* __restrict__ G) {
    __shared__ double sh[kCqSeg][16];
    const int kk = k * k, le = threadIdx.x & 15, seg = threadIdx.x >> 4, e = blockIdx.x * 16 + le;
    const bool live = e < kk && (e % k) <= (e / k);
    const int per = (nb + kCqSeg - 1) / kCqSeg, p0 = seg * per, p1 = std::min(nb, p0 + per);
    double s = 0.0;
    if (live) {
#pragma unroll 4
        for (int p = p0; p < p1; ++p) s += parts[(u64)p * kk + e];
    }
    sh[seg][le] = s;
    __syncthreads();
    if (seg == 0 && live) {
        double t = sh[0][le];
#pragma unroll
        for (int q = 1; q < kCqSeg; ++q) t += sh[q][le];
        G[e] = t;
    }
}

__device__ __forceinline__ double cq_wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;  // lane 0
}

// One block.  M[64][65] holds both triangles: R(i, j) (i <= j) at M[i][j + 1], inv(R)(i, j) (i <= j) at M[j][i].
#define CQ_R(i, j) M[(i) * 65 + (j) + 1]
#define CQ_X(i, j) M[(j) * 65 + (i)]
__global__ void __launch_bounds__(256) k_cq_factor(const double* __restrict__ G, int k, int second, double* __restrict__ r1,
                                                   double* __restrict__ rinv, double* __restrict__ R, double* __restrict__ E,
                                                   double* __restrict__ pv, unsigned* __restrict__ verdict) {
    __shared__ double M[64 * 65];
    __shared__ double sh4[4];
    __shared__ unsigned s_fail;
    const int t = threadIdx.x, kk = k * k;
    if (t == 0) s_fail = second ? *verdict : 0u;
    __syncthreads();
    if (s_fail) return;  // pass 1 failed verdict A: nothing below is needed (uniform)
    double dev = 0.0;
    for (int e = t; e < kk; e += 256) {
        const int i = e % k, j = e / k;
        if (i > j) continue;
        const double g = G[e];
        CQ_R(i, j) = g;
        const double d = i == j ? g - 1.0 : g;
        dev += i == j ? d * d : 2.0 * (d * d);
    }
    if (second) {  // verdict B: ||G2 - I||_F^2 <= 1/4, lane sums then a fixed tree; NaN fails
        dev = cq_wave_sum(dev);
        if ((t & 63) == 0) sh4[t >> 6] = dev;
        __syncthreads();
        if (t == 0 && !(((sh4[0] + sh4[1]) + sh4[2]) + sh4[3] <= 0.25)) s_fail = kFailB;
    }
    __syncthreads();
    if (s_fail) {
        if (t == 0) *verdict = s_fail;
        return;
    }
    // Cholesky, row i: the pivot (verdict A), then R(i, j) for j > i, one thread per column, dot products in order p = 0 .. i-1
    for (int i = 0; i < k; ++i) {
        if (t == i) {
            double s = 0.0;
            for (int p = 0; p < i; ++p) s += CQ_R(p, i) * CQ_R(p, i);
            const double d = CQ_R(i, i) - s;
            if (!(d > 0.0 && d <= 1.7976931348623157e308)) s_fail = second ? kFailA2 : kFailA1;
            CQ_R(i, i) = sqrt(d);
        }
        __syncthreads();
        if (t > i && t < k) {
            double s = 0.0;
            for (int p = 0; p < i; ++p) s += CQ_R(p, i) * CQ_R(p, t);
            CQ_R(i, t) = (CQ_R(i, t) - s) / CQ_R(i, i);
        }
        __syncthreads();
    }
    // inv(R), column j by back-substitution
    if (t < k) {
        const int j = t;
        CQ_X(j, j) = 1.0 / CQ_R(j, j);
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int p = i + 1; p <= j; ++p) s += CQ_R(i, p) * CQ_X(p, j);
            CQ_X(i, j) = -s / CQ_R(i, i);
        }
    }
    __syncthreads();
    for (int e = t; e < kk; e += 256) {
        const int i = e % k, j = e / k;
        rinv[e] = i <= j ? CQ_X(i, j) : 0.0;
        if (!second) {
            r1[e] = i <= j ? CQ_R(i, j) : 0.0;
        } else {
            double s = 0.0;
            if (i <= j) {
                for (int p = i; p <= j; ++p) s += CQ_R(i, p) * r1[p + j * k];
            }
            R[e] = s;
            E[e] = i == j ? 1.0 : 0.0;
            if (i == 0) pv[j] = (double)(j + 1);
        }
    }
    if (t == 0 && s_fail) *verdict = s_fail;
}
#undef CQ_R
#undef CQ_X

// Y(i, :) = X(i, :) inv(R): thread = row, the row in registers, column j = sum over p = 0 .. j in order (descending j, in place).
// GRAM: the slice's partial Gram matrix of Y as well, 64 rows at a time through LDS.
template <int KP, bool GRAM>
__global__ void __launch_bounds__(256) k_cq_apply(const double* __restrict__ X, u64 m, int k, const double* __restrict__ rinv,
                                                  double* __restrict__ Y, u64 rpb, double* __restrict__ parts) {
    typedef CqGeom<KP> Ge;
    __shared__ double Ri[KP * (KP + 1) / 2];  // packed upper triangle: (p, j) at j (j + 1) / 2 + p
    __shared__ __attribute__((aligned(16))) double L[GRAM ? kCqLds : 1];
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        const int p = e % KP, j = e / KP;
        if (p <= j) Ri[j * (j + 1) / 2 + p] = j < k ? rinv[p + j * k] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[4][4] = {};
    const u64 row0 = (u64)blockIdx.x * rpb, rend = std::min<u64>(m, row0 + rpb);
    for (u64 g0 = row0; g0 < rend; g0 += 256) {
        const u64 i = g0 + threadIdx.x;
        asm volatile("" ::: "memory");  // keeps the reads of Ri inside the iteration: hoisted out of the loop they would occupy the whole register file
        double x[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) x[p] = (p < k && i < m) ? X[i + (u64)p * m] : 0.0;
#pragma unroll
        for (int j = KP - 1; j >= 0; --j) {
            if (j < k) {
                double s = 0.0;
#pragma unroll
                for (int p = 0; p <= j; ++p) s = fma(x[p], Ri[j * (j + 1) / 2 + p], s);
                x[j] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < k && i < m) Y[i + (u64)j * m] = x[j];
        if (GRAM) {
#pragma unroll 1
            for (int turn = 0; turn < 4; ++turn) {
                if (w == turn) {
#pragma unroll
                    for (int j = 0; j < KP; ++j) L[lane * Ge::LD + j] = x[j];
                }
                __syncthreads();
                cq_gram_chunk<KP>(L, acc);
                __syncthreads();
            }
        }
    }
    if (GRAM) cq_gram_store<KP>(L, acc, k, parts + (u64)blockIdx.x * (u64)(k * k));
}

template <int KP>
int cq_run(Context* c, const double* P, u64 m, int k, double* q1, double* Q, double* parts, double* gsum, double* r1, double* rinv, double* R,
           double* E, double* pv, unsigned* verdict, u64 rpb, unsigned nb, unsigned* verdict_host) {
    const unsigned sum_grid = (unsigned)((k * k + 15) / 16);
    RMHIP_HIP_CHECK(hipMemsetAsync(verdict, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_cq_gram<KP>, dim3(nb), dim3(256), 0, c->stream, P, m, k, rpb, parts);
    hipLaunchKernelGGL(k_cq_sum, dim3(sum_grid), dim3(256), 0, c->stream, (const double*)parts, (int)nb, k, gsum);
    hipLaunchKernelGGL(k_cq_factor, dim3(1), dim3(256), 0, c->stream, (const double*)gsum, k, 0, r1, rinv, R, E, pv, verdict);
    hipLaunchKernelGGL((k_cq_apply<KP, true>), dim3(nb), dim3(256), 0, c->stream, P, m, k, (const double*)rinv, q1, rpb, parts);
    hipLaunchKernelGGL(k_cq_sum, dim3(sum_grid), dim3(256), 0, c->stream, (const double*)parts, (int)nb, k, gsum);
    hipLaunchKernelGGL(k_cq_factor, dim3(1), dim3(256), 0, c->stream, (const double*)gsum, k, 1, r1, rinv, R, E, pv, verdict);
    c->tel.kernel_launches += 6;
    RMHIP_HIP_CHECK(hipGetLastError());
    RMHIP_HIP_CHECK(hipMemcpyAsync(verdict_host, verdict, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (*verdict_host) return RMHIP_OK;
    hipLaunchKernelGGL((k_cq_apply<KP, false>), dim3(nb), dim3(256), 0, c->stream, (const double*)q1, m, k, (const double*)rinv, Q, rpb,
                       (double*)nullptr);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace
}  // namespace rmhip

int rmhip_qr_power_iter(rmhip_ctx* ctx, rmhip_buf product, rmhip_buf product_lhs, rmhip_buf q_handle, int economy, int pivot_vector,
                        rmhip_buf out4[4], int* served) {
    CTX_OR_FAIL(ctx);
    (void)pivot_vector;  // ProviderQrOptions.pivot only selects which output the builtin shows: both are always returned
    if (!out4 || !served) return fail(RMHIP_ERR_INVALID, "qr_power_iter: null output");
    *served = 0;
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    Buffer pb, lb, qh;
    RMHIP_TRY(c->lookup(product, &pb));
    if (product_lhs) RMHIP_TRY(c->lookup(product_lhs, &lb));
    RMHIP_TRY(c->lookup(q_handle, &qh));
    // declines: the caller runs qr
    (void)lb;
    if (!economy || pb.cplx || pb.shape.size() > 2 || qh.shape != pb.shape) return RMHIP_OK;
    const u64 m = pb.shape.empty() ? 1 : pb.shape[0], kc = pb.shape.size() < 2 ? 1 : pb.shape[1];
    if (kc < 1 || kc > (u64)kCqMaxCols || m < kc) return RMHIP_OK;
    const int k = (int)kc;
    RMHIP_TRY(c->get(product, &pb));  // f64 data in the plain layout (a widened copy on a precision-32 provider)
    // row slices: at most kCqMaxParts of them, a multiple of 256 rows each
    const u64 rpb = std::max<u64>(256, (((m + kCqMaxParts - 1) / kCqMaxParts) + 255) / 256 * 256);
    const unsigned nb = (unsigned)((m + rpb - 1) / rpb);
    const size_t shq[2] = {(size_t)m, (size_t)k}, shr[2] = {(size_t)k, (size_t)k}, shv[2] = {(size_t)k, 1};
    Buffer qb, rb, eb, vb;
    int rc = c->new_buffer(shq, 2, &out4[0], &qb);
    if (!rc) rc = c->new_buffer(shr, 2, &out4[1], &rb);
    if (!rc) rc = c->new_buffer(shr, 2, &out4[2], &eb);
    if (!rc) rc = c->new_buffer(shv, 2, &out4[3], &vb);
    std::shared_ptr<Allocation> q1, parts, small;
    if (!rc) rc = c->alloc_device(m * k, &q1);
    if (!rc) rc = c->alloc_device((size_t)nb * k * k, &parts);
    if (!rc) rc = c->alloc_device(3 * (size_t)k * k + 1, &small);  // the summed Gram matrix, R1, inv(R), the verdict word
    unsigned verdict = 0;
    if (!rc) {
        double* gsum = small->ptr;
        double* r1 = gsum + k * k;
        double* rinv = r1 + k * k;
        unsigned* vw = reinterpret_cast<unsigned*>(rinv + k * k);
#define CQ_RUN(KP) cq_run<KP>(c, pb.data(), m, k, q1->ptr, qb.data(), parts->ptr, gsum, r1, rinv, rb.data(), eb.data(), vb.data(), vw, rpb, nb, &verdict)
        rc = k <= 8 ? CQ_RUN(8) : k <= 16 ? CQ_RUN(16) : k <= 32 ? CQ_RUN(32) : CQ_RUN(64);
#undef CQ_RUN
    }
    if (rc || verdict) {
        for (int i = 0; i < 4; ++i) {
            if (out4[i]) rmhip_free(ctx, out4[i]);
            out4[i] = 0;
        }
        return rc;
    }
    c->record_launch("qr_power_iter", {{"m", m}, {"k", (uint64_t)k}}, {{"slices", nb}, {"passes", 5}});
    *served = 1;
    return RMHIP_OK;
}
