// pagefun.hip -- `pagefun(@mtimes, A, B)` (crates/runmat-accelerate-api/src/lib.rs:2386, PagefunRequest :603-614): every output page
// p is A(:, :, a(p)) * B(:, :, b(p)), where a(p) / b(p) take index 0 along each page dimension the operand broadcasts (extent 1).
// The contract is the host builtin's per-page loop (builtins/acceleration/gpu/pagefun.rs:330-384) over matmul_real
// (builtins/common/linalg.rs:6-32): sum = 0.0, then sum += a*b in k order, product and sum rounded separately.
//
// Tiers (chosen on the host, rmhip_ops.cpp rmhip_pagefun):
//   1  shared left operand: one launch_dgemm over C(m, n P) = A(m, k) B(k, n P)              (no kernel here)
//   2  tiny pages (m, n, k <= 32): k_pagefun_tiny, VALU in the CPU's order - bit-exact to the host builtin
//   3  medium pages: k_pagefun_mfma, a 64 x 64 tile of one page per work item on v_mfma_f64_16x16x4_f64
//   4  large pages (m, n >= 256): k_pgemm_w8 in dgemm.hip, the guarded eight-wave GEMM tile per (page, tile)
// Every kernel walks its work items with a grid-stride loop (any page count, grids far below 2^32 work-items), computes page offsets in
// 64 bits from the per-operand strides of PageMap, and sums each output element in one fixed order: results are bit-reproducible.
#include "common.h"

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kTinyThreads = 256;
constexpr unsigned kTinyLdsDoubles = 3072;  // A, B and C pages one block stages: 24 KiB, so that six blocks fit a CU's LDS
constexpr unsigned kGridCap = 1u << 20;     // blocks per launch; work items beyond it are taken by the grid-stride loops

// n consecutive doubles from src to dst with 16-byte accesses when both ends are 16-byte aligned (one end global, the other LDS)
__device__ __forceinline__ void copy_run(const double* __restrict__ src, double* __restrict__ dst, unsigned n) {
    const unsigned t = threadIdx.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const unsigned h = n >> 1;
        for (unsigned i = t; i < h; i += kTinyThreads) ((v2d*)dst)[i] = ((const v2d*)src)[i];
        if ((n & 1) && t == 0) dst[n - 1] = src[n - 1];
    } else {
        for (unsigned i = t; i < n; i += kTinyThreads) dst[i] = src[i];
    }
}

// Tier 2.  A block stages G consecutive output pages: an operand that is not broadcast holds them as one contiguous run (16-byte loads),
// a broadcast one is gathered page by page from offsets computed once per page.  C goes back as one contiguous run.  The product is the
// CPU's loop: s = 0.0; s = s + a*b (the Makefile's -ffp-contract=off keeps the multiply and the add separately rounded).
__global__ void __launch_bounds__(kTinyThreads) k_pagefun_tiny(const double* __restrict__ A, const double* __restrict__ B,
                                                               double* __restrict__ C, unsigned m, unsigned n, unsigned k, u64 pages,
                                                               unsigned G, const PageMap pm, int a_dense, int b_dense) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned mk = m * k, kn = k * n, mn = m * n;
    double* const As = lds;
    double* const Bs = As + G * mk;
    double* const Cs = Bs + G * kn;
    u64* const offs = (u64*)(Cs + G * mn);  // [2 G]: element offsets of the A and B page of each staged output page
    const unsigned t = threadIdx.x;
    const u64 groups = (pages + G - 1) / G;
    for (u64 grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const u64 p0 = grp * G;
        const unsigned gn = (pages - p0) < G ? (unsigned)(pages - p0) : G;
        if (!(a_dense && b_dense)) {
            for (unsigned g = t; g < gn; g += kTinyThreads) {
                u64 oa, ob;
                pm.offsets(p0 + g, oa, ob);
                offs[2 * g] = oa;
                offs[2 * g + 1] = ob;
            }
            __syncthreads();
        }
        if (a_dense) copy_run(A + p0 * mk, As, gn * mk);
        else
            for (unsigned i = t; i < gn * mk; i += kTinyThreads) {
                const unsigned g = i / mk;
                As[i] = A[offs[2 * g] + (i - g * mk)];
            }
        if (b_dense) copy_run(B + p0 * kn, Bs, gn * kn);
        else
            for (unsigned i = t; i < gn * kn; i += kTinyThreads) {
                const unsigned g = i / kn;
                Bs[i] = B[offs[2 * g + 1] + (i - g * kn)];
            }
        __syncthreads();
        for (unsigned i = t; i < gn * mn; i += kTinyThreads) {
            const unsigned g = i / mn, r = i - g * mn, j = r / m, row = r - j * m;
            const double* a = As + g * mk + row;
            const double* b = Bs + g * kn + j * k;
            double s = 0.0;
            for (unsigned kk = 0; kk < k; ++kk) s = s + a[kk * m] * b[kk];
            Cs[i] = s;
        }
        __syncthreads();
        copy_run(Cs, C + p0 * mn, gn * mn);
        __syncthreads();  // the next group overwrites the staging
    }
}

// Tier 3.  Work item = (page, 64 x 64 tile of it); four waves of 32 x 32 (2 x 2 MFMA tiles).  Operand roles as in dgemm.hip: the MFMA
// A operand is the B^T tile and the B operand the A^T tile, so the lane-contiguous MFMA column is the memory-contiguous row of C.
// LDS: A tile [k][m] (row stride 80: 80 % 32 == 16 puts the two k rows a half-wave reads in disjoint bank halves), B tile [n][k]
// (row stride 18: 16 n rows x 2 k cover the 64 banks once).  Rows, columns and k beyond the page are staged as zeros.
constexpr int kMt = 64, kKc = 16, kSa = kMt + 16, kSb = kKc + 2;

__global__ void __launch_bounds__(256) k_pagefun_mfma(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                      unsigned m, unsigned n, unsigned k, u64 pages, unsigned tiles_m, unsigned tiles_n,
                                                      const PageMap pm) {
    __shared__ __attribute__((aligned(16))) double As[kKc * kSa];
    __shared__ __attribute__((aligned(16))) double Bs[kMt * kSb];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int l15 = lane & 15, lq = lane >> 4;
    const u64 tpp = (u64)tiles_m * tiles_n, work = pages * tpp, mn = (u64)m * n;
    for (u64 w = blockIdx.x; w < work; w += gridDim.x) {
        const u64 p = w / tpp;
        const unsigned tt = (unsigned)(w - p * tpp);
        const unsigned m0 = (tt % tiles_m) * kMt, n0 = (tt / tiles_m) * kMt;
        u64 oa, ob;
        pm.offsets(p, oa, ob);
        const double* const Ap = A + oa;
        const double* const Bp = B + ob;
        double* const Cp = C + p * mn;
        v4d acc[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = v4d{0.0, 0.0, 0.0, 0.0};
        for (unsigned k0 = 0; k0 < k; k0 += kKc) {
#pragma unroll
            for (int e = t; e < kMt * kKc; e += 256) {
                const unsigned am = e & 63, ak = e >> 6;  // A: 64 contiguous rows per k
                As[ak * kSa + am] = (m0 + am < m && k0 + ak < k) ? Ap[(m0 + am) + (u64)(k0 + ak) * m] : 0.0;
                const unsigned bk = e & 15, bn = e >> 4;  // B: 16 contiguous k per column
                Bs[bn * kSb + bk] = (k0 + bk < k && n0 + bn < n) ? Bp[(k0 + bk) + (u64)(n0 + bn) * k] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kKc / 4; ++kk) {
                double af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = As[(kk * 4 + lq) * kSa + wm * 32 + i * 16 + l15];
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = Bs[(wn * 32 + j * 16 + l15) * kSb + kk * 4 + lq];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j], af[i], acc[j][i], 0, 0, 0);
            }
            __syncthreads();
        }
        // f64 MFMA result layout: column lane & 15 (= row mm of C), row (lane >> 4) + 4 r (= column nn of C)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned mm = m0 + wm * 32 + i * 16 + l15, nn = n0 + wn * 32 + j * 16 + 4 * r + lq;
                    if (mm < m && nn < n) Cp[mm + (u64)nn * m] = acc[j][i][r];
                }
    }
}

unsigned capped_grid(u64 work) { return (unsigned)(work < kGridCap ? work : kGridCap); }

}  // namespace

int launch_pagefun_tiny(Context* c, const double* A, const double* B, double* C, unsigned m, unsigned n, unsigned k, u64 pages,
                        const PageMap& pm, bool a_dense, bool b_dense, unsigned* pages_per_block) {
    if (m > 32 || n > 32 || k > 32) return fail(RMHIP_ERR_INVALID, "pagefun: tiny tier called with a %ux%ux%u page", m, n, k);
    const unsigned per_page = m * k + k * n + m * n;
    unsigned G = kTinyLdsDoubles / per_page;
    if (G > 1) G &= ~1u;  // an even count keeps every staged run 16-byte aligned when a page has an odd element count
    const u64 groups = (pages + G - 1) / G;
    const size_t lds_bytes = sizeof(double) * ((size_t)G * per_page + 2 * (size_t)G);
    hipLaunchKernelGGL(k_pagefun_tiny, dim3(capped_grid(groups)), dim3(kTinyThreads), lds_bytes, c->stream, A, B, C, m, n, k, pages, G, pm,
                       (int)a_dense, (int)b_dense);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    if (pages_per_block) *pages_per_block = G;
    return RMHIP_OK;
}

int launch_pagefun_mfma(Context* c, const double* A, const double* B, double* C, unsigned m, unsigned n, unsigned k, u64 pages,
                        const PageMap& pm) {
    const unsigned tiles_m = (m + kMt - 1) / kMt, tiles_n = (n + kMt - 1) / kMt;
    hipLaunchKernelGGL(k_pagefun_mfma, dim3(capped_grid(pages * tiles_m * tiles_n)), dim3(256), 0, c->stream, A, B, C, m, n, k, pages,
                       tiles_m, tiles_n, pm);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace rmhip
