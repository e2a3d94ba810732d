// complex_pagefun.hip -- `pagefun(@mtimes, A, B)` with at least one complex-interleaved operand (rmhip_complex_pagefun, rmhip_ops.cpp;
// the real sibling is pagefun.hip).  The contract is the host builtin's per-page loop (builtins/acceleration/gpu/pagefun.rs:330-384),
// which hands each page pair to exactly one of three loops of builtins/common/linalg.rs:
//   kind 0  complex x complex (matmul_complex :57-85):       re += ar*br - ai*bi;  im += ar*bi + ai*br   (the k-term formed first)
//   kind 1  complex x real    (matmul_complex_real :88-116): re += ar*br;          im += ai*br
//   kind 2  real x complex    (matmul_real_complex :119-147): re += ar*br;         im += ar*bi
// The mixed kinds never form a product with an implied zero part: an Inf in the complex operand stays Inf.  Both kernels keep that.
//
// Tiers (chosen on the host; numbered like the sibling's):
//   2  small pages (m, n, k <= 32): k_cpage_small<KIND>, VALU in the CPU's order - bit-exact to the host builtin
//   3  everything larger: k_cpage_mfma<KIND>, a 64 x 64 tile of one page per work item on v_mfma_f64_16x16x4_f64, the interleaved
//      operands split into re / im planes while staging
// Page offsets come from PageMap in elements and are doubled for an interleaved operand.  Both kernels walk their work with grid-stride
// loops and sum every output element in one fixed order: results are bit-reproducible.  `r32`: a precision-32 context rounds each part
// of the result through f32 once, on the final store (storage stays 2 x f64).
#include "common.h"

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kSmallThreads = 256;
constexpr unsigned kSmallLdsDoubles = 3072;  // the pages one block stages: 24 KiB, six blocks to a CU; a larger page triple goes alone
constexpr unsigned kGridCap = 1u << 20;      // blocks per launch; work items beyond it are taken by the grid-stride loops

__device__ __forceinline__ double round_part(double v, int r32) { return r32 ? (double)(float)v : v; }

// n consecutive doubles from src to dst with 16-byte accesses when both ends are 16-byte aligned (one end global, the other LDS)
__device__ __forceinline__ void copy_run(const double* __restrict__ src, double* __restrict__ dst, unsigned n) {
    const unsigned t = threadIdx.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const unsigned h = n >> 1;
        for (unsigned i = t; i < h; i += kSmallThreads) ((v2d*)dst)[i] = ((const v2d*)src)[i];
        if ((n & 1) && t == 0) dst[n - 1] = src[n - 1];
    } else {
        for (unsigned i = t; i < n; i += kSmallThreads) dst[i] = src[i];
    }
}

// Tier 2.  A block stages G consecutive output pages as k_pagefun_tiny does: an operand that is not broadcast holds them as one
// contiguous run, a broadcast one is gathered page by page.  EA / EB: doubles per element of A / B (2 interleaved, 1 real).  C is
// staged interleaved and goes back as one contiguous run.  The Makefile's -ffp-contract=off keeps every product, difference and sum
// separately rounded.
template <int KIND>
__global__ void __launch_bounds__(kSmallThreads) k_cpage_small(const double* __restrict__ A, const double* __restrict__ B,
                                                               double* __restrict__ C, unsigned m, unsigned n, unsigned k, u64 pages,
                                                               unsigned G, const PageMap pm, int a_dense, int b_dense, int r32) {
    constexpr unsigned EA = KIND == 2 ? 1 : 2, EB = KIND == 1 ? 1 : 2;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned mk = m * k * EA, kn = k * n * EB, mn = m * n;  // doubles per A page, per B page; elements per C page
    double* const Cs = lds;
    double* const As = Cs + G * 2 * mn;
    double* const Bs = As + G * mk;
    u64* const offs = (u64*)(Bs + G * kn);  // [2 G]: offsets in doubles of the A and B page of each staged output page
    const unsigned t = threadIdx.x;
    const u64 groups = (pages + G - 1) / G;
    for (u64 grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const u64 p0 = grp * G;
        const unsigned gn = (pages - p0) < G ? (unsigned)(pages - p0) : G;
        if (!(a_dense && b_dense)) {
            for (unsigned g = t; g < gn; g += kSmallThreads) {
                u64 oa, ob;
                pm.offsets(p0 + g, oa, ob);
                offs[2 * g] = oa * EA;
                offs[2 * g + 1] = ob * EB;
            }
            __syncthreads();
        }
        if (a_dense) copy_run(A + p0 * mk, As, gn * mk);
        else
            for (unsigned i = t; i < gn * mk; i += kSmallThreads) {
                const unsigned g = i / mk;
                As[i] = A[offs[2 * g] + (i - g * mk)];
            }
        if (b_dense) copy_run(B + p0 * kn, Bs, gn * kn);
        else
            for (unsigned i = t; i < gn * kn; i += kSmallThreads) {
                const unsigned g = i / kn;
                Bs[i] = B[offs[2 * g + 1] + (i - g * kn)];
            }
        __syncthreads();
        for (unsigned i = t; i < gn * mn; i += kSmallThreads) {
            const unsigned g = i / mn, r = i - g * mn, j = r / m, row = r - j * m;
            const double* a = As + g * mk + row * EA;
            const double* b = Bs + g * kn + j * k * EB;
            double re = 0.0, im = 0.0;
            for (unsigned kk = 0; kk < k; ++kk) {
                if (KIND == 0) {
                    const double ar = a[kk * m * 2], ai = a[kk * m * 2 + 1], br = b[kk * 2], bi = b[kk * 2 + 1];
                    const double tr = ar * br - ai * bi, ti = ar * bi + ai * br;
                    re = re + tr;
                    im = im + ti;
                } else if (KIND == 1) {
                    const double ar = a[kk * m * 2], ai = a[kk * m * 2 + 1], br = b[kk];
                    re = re + ar * br;
                    im = im + ai * br;
                } else {
                    const double ar = a[kk * m], br = b[kk * 2], bi = b[kk * 2 + 1];
                    re = re + ar * br;
                    im = im + ar * bi;
                }
            }
            ((v2d*)Cs)[i] = v2d{round_part(re, r32), round_part(im, r32)};
        }
        __syncthreads();
        copy_run(Cs, C + p0 * 2 * mn, gn * 2 * mn);
        __syncthreads();  // the next group overwrites the staging
    }
}

// Tier 3.  Work item = (page, 64 x 64 tile of it); four waves of 32 x 32 (2 x 2 MFMA tiles), operand roles and LDS strides as in
// k_pagefun_mfma: the MFMA A operand is the B^T tile and the B operand the A^T tile, A planes [k][m] with row stride 80, B planes
// [n][k] with row stride 18.  An interleaved operand is read as 16-byte (re, im) pairs and split into its two planes while staging;
// rows, columns and k beyond the page are staged as zeros.  Kind 0 takes four accumulations per k-step into two accumulator sets,
// Cr += Ar Br, Cr += (-Ai) Bi (the sign flipped on the fragment: exact), Ci += Ar Bi, Ci += Ai Br; the mixed kinds take two.
constexpr int kMt = 64, kKc = 16, kSa = kMt + 16, kSb = kKc + 2;

template <int KIND>
__global__ void __launch_bounds__(256) k_cpage_mfma(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                    unsigned m, unsigned n, unsigned k, u64 pages, unsigned tiles_m, unsigned tiles_n,
                                                    const PageMap pm, int r32) {
    constexpr bool AC = KIND != 2, BC = KIND != 1;  // which operand is interleaved
    __shared__ __attribute__((aligned(16))) double Ar[kKc * kSa];
    __shared__ __attribute__((aligned(16))) double Ai[AC ? kKc * kSa : 2];
    __shared__ __attribute__((aligned(16))) double Br[kMt * kSb];
    __shared__ __attribute__((aligned(16))) double Bi[BC ? kMt * kSb : 2];
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
        const double* const Ap = A + oa * (AC ? 2 : 1);
        const double* const Bp = B + ob * (BC ? 2 : 1);
        v2d* const Cp = (v2d*)C + p * mn;
        v4d accr[2][2], acci[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                accr[j][i] = v4d{0.0, 0.0, 0.0, 0.0};
                acci[j][i] = v4d{0.0, 0.0, 0.0, 0.0};
            }
        for (unsigned k0 = 0; k0 < k; k0 += kKc) {
#pragma unroll
            for (int e = t; e < kMt * kKc; e += 256) {
                const unsigned am = e & 63, ak = e >> 6;  // A: 64 contiguous rows per k
                const bool a_in = m0 + am < m && k0 + ak < k;
                const u64 ia = (m0 + am) + (u64)(k0 + ak) * m;
                if (AC) {
                    const v2d z = a_in ? ((const v2d*)Ap)[ia] : v2d{0.0, 0.0};
                    Ar[ak * kSa + am] = z.x;
                    Ai[ak * kSa + am] = z.y;
                } else {
                    Ar[ak * kSa + am] = a_in ? Ap[ia] : 0.0;
                }
                const unsigned bk = e & 15, bn = e >> 4;  // B: 16 contiguous k per column
                const bool b_in = k0 + bk < k && n0 + bn < n;
                const u64 ib = (k0 + bk) + (u64)(n0 + bn) * k;
                if (BC) {
                    const v2d z = b_in ? ((const v2d*)Bp)[ib] : v2d{0.0, 0.0};
                    Br[bn * kSb + bk] = z.x;
                    Bi[bn * kSb + bk] = z.y;
                } else {
                    Br[bn * kSb + bk] = b_in ? Bp[ib] : 0.0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kKc / 4; ++kk) {
                double afr[2], afi[2], bfr[2], bfi[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int ia = (kk * 4 + lq) * kSa + wm * 32 + i * 16 + l15;
                    afr[i] = Ar[ia];
                    afi[i] = AC ? Ai[ia] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ib = (wn * 32 + j * 16 + l15) * kSb + kk * 4 + lq;
                    bfr[j] = Br[ib];
                    bfi[j] = BC ? Bi[ib] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        accr[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[j], afr[i], accr[j][i], 0, 0, 0);
                        if (KIND == 0) {
                            accr[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfi[j], -afi[i], accr[j][i], 0, 0, 0);
                            acci[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfi[j], afr[i], acci[j][i], 0, 0, 0);
                            acci[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[j], afi[i], acci[j][i], 0, 0, 0);
                        } else if (KIND == 1) {
                            acci[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[j], afi[i], acci[j][i], 0, 0, 0);
                        } else {
                            acci[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfi[j], afr[i], acci[j][i], 0, 0, 0);
                        }
                    }
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
                    if (mm < m && nn < n) Cp[mm + (u64)nn * m] = v2d{round_part(accr[j][i][r], r32), round_part(acci[j][i][r], r32)};
                }
    }
}

unsigned capped_grid(u64 work) { return (unsigned)(work < kGridCap ? work : kGridCap); }

}  // namespace

int launch_cpage_small(Context* c, int kind, const double* A, const double* B, double* C, unsigned m, unsigned n, unsigned k, u64 pages,
                       const PageMap& pm, bool a_dense, bool b_dense, unsigned* pages_per_block) {
    if (m > 32 || n > 32 || k > 32) return fail(RMHIP_ERR_INVALID, "complex_pagefun: small tier called with a %ux%ux%u page", m, n, k);
    if (kind < 0 || kind > 2) return fail(RMHIP_ERR_INVALID, "complex_pagefun: operand kind %d", kind);
    const unsigned ea = kind == 2 ? 1 : 2, eb = kind == 1 ? 1 : 2;
    const unsigned per_page = ea * m * k + eb * k * n + 2 * m * n;  // at most 6144 doubles: 48 KiB
    unsigned G = kSmallLdsDoubles / per_page;
    if (G == 0) G = 1;
    if (G > 1) G &= ~1u;  // an even count keeps every staged run 16-byte aligned when a real page has an odd element count
    const u64 groups = (pages + G - 1) / G;
    const size_t lds_bytes = sizeof(double) * ((size_t)G * per_page + 2 * (size_t)G);
    const dim3 grid(capped_grid(groups)), block(kSmallThreads);
    const int r32 = c->precision == 32 ? 1 : 0;
    if (kind == 0)
        hipLaunchKernelGGL(k_cpage_small<0>, grid, block, lds_bytes, c->stream, A, B, C, m, n, k, pages, G, pm, (int)a_dense, (int)b_dense, r32);
    else if (kind == 1)
        hipLaunchKernelGGL(k_cpage_small<1>, grid, block, lds_bytes, c->stream, A, B, C, m, n, k, pages, G, pm, (int)a_dense, (int)b_dense, r32);
    else
        hipLaunchKernelGGL(k_cpage_small<2>, grid, block, lds_bytes, c->stream, A, B, C, m, n, k, pages, G, pm, (int)a_dense, (int)b_dense, r32);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    if (pages_per_block) *pages_per_block = G;
    return RMHIP_OK;
}

int launch_cpage_mfma(Context* c, int kind, const double* A, const double* B, double* C, unsigned m, unsigned n, unsigned k, u64 pages,
                      const PageMap& pm) {
    if (kind < 0 || kind > 2) return fail(RMHIP_ERR_INVALID, "complex_pagefun: operand kind %d", kind);
    const unsigned tiles_m = (m + kMt - 1) / kMt, tiles_n = (n + kMt - 1) / kMt;
    const dim3 grid(capped_grid(pages * tiles_m * tiles_n)), block(256);
    const int r32 = c->precision == 32 ? 1 : 0;
    if (kind == 0) hipLaunchKernelGGL(k_cpage_mfma<0>, grid, block, 0, c->stream, A, B, C, m, n, k, pages, tiles_m, tiles_n, pm, r32);
    else if (kind == 1) hipLaunchKernelGGL(k_cpage_mfma<1>, grid, block, 0, c->stream, A, B, C, m, n, k, pages, tiles_m, tiles_n, pm, r32);
    else hipLaunchKernelGGL(k_cpage_mfma<2>, grid, block, 0, c->stream, A, B, C, m, n, k, pages, tiles_m, tiles_n, pm, r32);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace rmhip
