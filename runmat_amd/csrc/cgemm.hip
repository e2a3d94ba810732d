// cgemm.hip -- the two streaming passes around the one real product that serves `A * B` with a complex-interleaved operand
// (rmhip_complex_matmul, rmhip_ops.cpp; the embedding and its table: gemm_plan.h plan_cgemm).  The product itself runs in
// launch_dgemm (dgemm.hip); nothing here multiplies.
//   k_cgemm_split_b     B (k x n interleaved) -> the planes [B_re | B_im] (k x 2n real, ld k): the product's right operand, kinds 0 and 2
//   k_cgemm_join<KIND>  T, the real product, -> the interleaved result C (m x n):
//     kind 0  T is 2m x 2n (ld 2m): re = T[2i, j] - T[2i+1, n+j], im = T[2i, n+j] + T[2i+1, j] - one rounded difference, one rounded sum
//     kind 1  T is 2m x n (ld 2m), the interleaved result already: the pass only rounds (a precision-32 context; otherwise it is not run)
//     kind 2  T is m x 2n (ld m): C(i, j) = (T[i, j], T[i, n+j])
// Every extent is whole columns, so each pass is flat over the m n (k n) logical elements: element e of C reads pair e of the left half
// of T and pair (or double) e of the right half, mn further on.  `r32`: each part is rounded through f32 once, on the store (storage
// stays 2 x f64).  Grid-stride loops under a block cap; no LDS, no scratch.
#include "common.h"

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr u64 kGridCap = 1ull << 20;  // blocks per launch; elements beyond it are taken by the grid-stride loops

__device__ __forceinline__ double round_part(double v, int r32) { return r32 ? (double)(float)v : v; }

// one 16-byte load per complex element, two coalesced 8-byte stores
__global__ void __launch_bounds__(kThreads) k_cgemm_split_b(const v2d* __restrict__ B, double* __restrict__ P, u64 kn) {
    for (u64 e = (u64)blockIdx.x * kThreads + threadIdx.x; e < kn; e += (u64)gridDim.x * kThreads) {
        const v2d z = B[e];
        P[e] = z.x;
        P[kn + e] = z.y;
    }
}

// T's base is 16-byte aligned and, for kinds 0 and 1, its leading dimension 2m is even: the row pair (2i, 2i+1) of a column is one
// 16-byte load.  The Makefile's -ffp-contract=off has nothing to contract here; the difference and the sum are each rounded once.
template <int KIND>
__global__ void __launch_bounds__(kThreads) k_cgemm_join(const double* __restrict__ T, v2d* __restrict__ C, u64 mn, int r32) {
    for (u64 e = (u64)blockIdx.x * kThreads + threadIdx.x; e < mn; e += (u64)gridDim.x * kThreads) {
        double re, im;
        if (KIND == 0) {
            const v2d x = ((const v2d*)T)[e], y = ((const v2d*)T)[mn + e];  // (Ar Br, Ai Br), (Ar Bi, Ai Bi)
            re = x.x - y.y;
            im = y.x + x.y;
        } else if (KIND == 1) {
            const v2d x = ((const v2d*)T)[e];
            re = x.x;
            im = x.y;
        } else {
            re = T[e];
            im = T[mn + e];
        }
        C[e] = v2d{round_part(re, r32), round_part(im, r32)};
    }
}

unsigned capped_grid(u64 work) {
    const u64 blocks = (work + kThreads - 1) / kThreads;
    return (unsigned)(blocks < kGridCap ? blocks : kGridCap);
}

}  // namespace

int launch_cgemm_split_b(Context* c, const double* B, double* planes, size_t kn) {
    if (kn == 0) return RMHIP_OK;
    hipLaunchKernelGGL(k_cgemm_split_b, dim3(capped_grid(kn)), dim3(kThreads), 0, c->stream, (const v2d*)B, planes, (u64)kn);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int launch_cgemm_join(Context* c, int kind, const double* T, double* C, size_t mn) {
    if (kind < 0 || kind > 2) return fail(RMHIP_ERR_INVALID, "complex_matmul: operand kind %d", kind);
    if (mn == 0) return RMHIP_OK;
    const dim3 grid(capped_grid(mn)), block(kThreads);
    const int r32 = c->precision == 32 ? 1 : 0;
    if (kind == 0) hipLaunchKernelGGL(k_cgemm_join<0>, grid, block, 0, c->stream, T, (v2d*)C, (u64)mn, r32);
    else if (kind == 1) hipLaunchKernelGGL(k_cgemm_join<1>, grid, block, 0, c->stream, T, (v2d*)C, (u64)mn, r32);
    else hipLaunchKernelGGL(k_cgemm_join<2>, grid, block, 0, c->stream, T, (v2d*)C, (u64)mn, r32);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace rmhip
