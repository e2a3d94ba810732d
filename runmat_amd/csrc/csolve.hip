// csolve.hip -- the streaming passes around the one real solve that serves `A \ b`, `b / A` and `inv(A)` with a complex-interleaved
// operand (rmhip_complex_mldivide / _mrdivide / _inv, solve.cpp; the embedding and its table: csolve_plan.h plan_csolve).
// The solve itself runs in the cores of solve.cpp on the kernels of lu.hip, small_solve.hip, special.hip and svdsolve.hip; nothing here
// does arithmetic beyond one negation and the f32 rounding of a precision-32 result.
//   k_csolve_embed        A (m x n interleaved, ld m) -> E(A) = [Ar -Ai; Ai Ar], 2m x 2n real, column-major, ld 2m, in BLOCK layout:
//                         E[i, j] = re, E[m+i, j] = im, E[i, n+j] = -im, E[m+i, n+j] = re.  `transposed`: E(A.') (2n x 2m, ld 2n) - the
//                         same stores, the element read from the swapped index.
//   k_csolve_stack<KIND>  the right-hand side B of a system of m rows and k columns -> the real right-hand side:
//     kind 0  B complex: [Br; Bi]   2m x k, ld 2m
//     kind 1  B real:    [Br; 0]    2m x k, ld 2m
//     kind 2  B complex: [Br | Bi]  m x 2k, ld m   (A is real and is not embedded)
//     kind 3  no B:      [I; 0]     2m x k, ld 2m  (inv: k == m)
//                         `transposed`: B is stored k x m (ld k) and B.' is stacked (mrdivide).
//   k_csolve_join<KIND>   T, the real solution, -> the interleaved X (n x k):
//     kinds 0, 1  T is 2n x k (ld 2n): X[i, c] = (T[i, c], T[n+i, c])
//     kind 2      T is n x 2k (ld n):  X[i, c] = (T[i, c], T[i, k+c])
//                         `transposed`: X.' is written (k x n, ld k).  `r32`: each part is rounded through f32 once, here (storage stays
//                         2 x f64).
// One thread per element: threadIdx / blockIdx.x run down a column of the OUTPUT of embed and stack (of T for the join), so every store
// stream of embed and stack, and every load stream of the join, is contiguous; blockIdx.y strides over the columns.  One 16-byte load
// (store) per complex element.  No LDS, no scratch, no read-modify-write.  The loads of the `transposed` forms of embed and stack are
// STRIDED (adjacent threads read elements one stored column apart: 16 m bytes for the embed), so those passes stream only on their
// store side; the same holds for the stores of the transposed join.  mrdivide alone takes them (within the spread of
// mldivide's time at orders 1024 to 8192).
#include "common.h"

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr u64 kGridY = 65535;  // columns beyond it are taken by the loop over blockIdx.y

__device__ __forceinline__ double round_part(double v, int r32) { return r32 ? (double)(float)v : v; }

// rows / cols: the extents of one block of the output (m x n, or n x m when transposed); the output is 2 rows x 2 cols, ld 2 rows
__global__ void __launch_bounds__(kThreads) k_csolve_embed(const v2d* __restrict__ A, double* __restrict__ E, u64 m, u64 rows, u64 cols,
                                                           int transposed) {
    const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (t >= rows) return;
    const u64 ld = 2 * rows;
    for (u64 s = blockIdx.y; s < cols; s += gridDim.y) {
        const v2d z = transposed ? A[s + t * m] : A[t + s * m];
        double* const left = E + t + s * ld;
        double* const right = left + cols * ld;
        left[0] = z.x;
        left[rows] = z.y;
        right[0] = -z.y;
        right[rows] = z.x;
    }
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) k_csolve_stack(const double* __restrict__ B, double* __restrict__ T, u64 m, u64 k, int transposed) {
    const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    for (u64 c = blockIdx.y; c < k; c += gridDim.y) {
        const u64 src = transposed ? c + t * k : t + c * m;
        if (KIND == 0) {
            const v2d z = ((const v2d*)B)[src];
            T[t + c * 2 * m] = z.x;
            T[m + t + c * 2 * m] = z.y;
        } else if (KIND == 1) {
            T[t + c * 2 * m] = B[src];
            T[m + t + c * 2 * m] = 0.0;
        } else if (KIND == 2) {
            const v2d z = ((const v2d*)B)[src];
            T[t + c * m] = z.x;
            T[t + (k + c) * m] = z.y;
        } else {
            T[t + c * 2 * m] = t == c ? 1.0 : 0.0;
            T[m + t + c * 2 * m] = 0.0;
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) k_csolve_join(const double* __restrict__ T, v2d* __restrict__ X, u64 n, u64 k, int transposed,
                                                          int r32) {
    const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    for (u64 c = blockIdx.y; c < k; c += gridDim.y) {
        double re, im;
        if (KIND == 2) {
            re = T[t + c * n];
            im = T[t + (k + c) * n];
        } else {
            re = T[t + c * 2 * n];
            im = T[n + t + c * 2 * n];
        }
        X[transposed ? c + t * k : t + c * n] = v2d{round_part(re, r32), round_part(im, r32)};
    }
}

dim3 column_grid(size_t rows, size_t cols) {
    return dim3((unsigned)((rows + kThreads - 1) / kThreads), (unsigned)(cols < kGridY ? cols : kGridY));
}

}  // namespace

int launch_csolve_embed(Context* c, const double* A, size_t m, size_t n, bool transposed, double* E) {
    if (m == 0 || n == 0) return RMHIP_OK;
    const size_t rows = transposed ? n : m, cols = transposed ? m : n;
    hipLaunchKernelGGL(k_csolve_embed, column_grid(rows, cols), dim3(kThreads), 0, c->stream, (const v2d*)A, E, (u64)m, (u64)rows, (u64)cols,
                       transposed ? 1 : 0);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int launch_csolve_stack(Context* c, int kind, const double* B, size_t m, size_t k, bool transposed, double* T) {
    if (kind < 0 || kind > 3) return fail(RMHIP_ERR_INVALID, "complex solve: operand kind %d", kind);
    if (m == 0 || k == 0) return RMHIP_OK;
    const dim3 grid = column_grid(m, k), block(kThreads);
    const int tr = transposed ? 1 : 0;
    if (kind == 0) hipLaunchKernelGGL(k_csolve_stack<0>, grid, block, 0, c->stream, B, T, (u64)m, (u64)k, tr);
    else if (kind == 1) hipLaunchKernelGGL(k_csolve_stack<1>, grid, block, 0, c->stream, B, T, (u64)m, (u64)k, tr);
    else if (kind == 2) hipLaunchKernelGGL(k_csolve_stack<2>, grid, block, 0, c->stream, B, T, (u64)m, (u64)k, tr);
    else hipLaunchKernelGGL(k_csolve_stack<3>, grid, block, 0, c->stream, B, T, (u64)m, (u64)k, tr);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int launch_csolve_join(Context* c, int kind, const double* T, size_t n, size_t k, bool transposed, double* X) {
    if (kind < 0 || kind > 2) return fail(RMHIP_ERR_INVALID, "complex solve: operand kind %d", kind);
    if (n == 0 || k == 0) return RMHIP_OK;
    const dim3 grid = column_grid(n, k), block(kThreads);
    const int tr = transposed ? 1 : 0, r32 = c->precision == 32 ? 1 : 0;
    if (kind == 2) hipLaunchKernelGGL(k_csolve_join<2>, grid, block, 0, c->stream, T, (v2d*)X, (u64)n, (u64)k, tr, r32);
    else hipLaunchKernelGGL(k_csolve_join<0>, grid, block, 0, c->stream, T, (v2d*)X, (u64)n, (u64)k, tr, r32);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace rmhip
