// cond_norm.hip -- `cond(A, p)` for p = 1, inf and 'fro' (rmhip_cond_norm, the second entry point of the hook `cond`).
//
// Reference behaviour restated here (crates/runmat-runtime/src/builtins/math/linalg/solve/cond.rs):
//   * :276-300  empty -> 0, one element -> (a == 0 ? Inf : 1), the 1 / inf / fro forms need a square matrix;
//   * :343-357  the inverse is nalgebra's `try_inverse` (LU with partial pivoting); None -> Inf;
//   * :384-414  norm(A) * norm(inv(A)), a product that is not finite -> Inf; One: largest column sum of |a|, Inf: largest row sum of
//               |a| (columns added in ascending order), Fro: sqrt(sum a^2) without scaling.
//
// The path.  One factor copy of A (the LU's padded workspace, mode 0 of lu_factor_device: the reference's pivot rule) and the inverse
// in column slabs of kCondSlabCols columns: k_cond_fill writes P E(:, j0 : j0 + w) - the row-permuted identity slab, which is what
// lu_solve_device's gather would make of E - lu_substitute_device turns it into A^-1(:, j0 : j0 + w) in place, and k_cond_accumulate
// folds the slab into the three norms.  The n x n inverse never exists: beyond the operand the call holds n^2 + n W + O(n) doubles.
// A itself goes through the same accumulate kernel in the same slabs.
//
// Sums.  One lane per row walks the slab's columns in ascending order and adds |x| into that row's running sum (rowsum[n] lives in
// memory between slabs): the CPU's loop order, bit for bit.  The same lane adds x^2 into the row's sum of squares.  The column sums
// cross lanes: a __shfl_down tree per 64-row wave, one partial per (wave, column), folded over the waves in ascending order by
// k_cond_fold, which keeps the running maximum.  No floating-point atomics and no order that depends on timing: two calls on one
// operand give the same bits.
//
// Verdict (the only read-back this file adds; the factorisation reads its pivots back itself): a non-finite entry of A, and the FIRST pivot
// at the LU's cut-off (|u_kk| <= 1e-12).  lu_factor_device carries on past such a pivot - it zeroes the sub-column, skips the
// update and counts the pivot in *info_host - so the diagonal of the finished factor holds every pivot it met, but the pivots after
// the first skipped one are not the reference's (nalgebra does not skip a tiny nonzero pivot).  Hence the first one decides, not a
// count of zeros on the diagonal: exactly zero -> the whole remaining column was zero, nalgebra's try_inverse returns None -> Inf;
// nonzero -> RMHIP_ERR_UNSUPPORTED (the host's LU divides by its own rounding noise there).
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"

using namespace rmhip;

namespace rmhip {
namespace {

// Columns of the inverse formed per solve; the workspace is n x kCondSlabCols doubles.  Every slab's substitutions read both triangles
// again, so wider is faster: ms per call on an MI355X (scripts/cond_norm_rates.py, docs/EXPERIMENTS.md) at n = 2048 / 8192 with 256
// columns 17.7 / 204, with 512 13.5 / 137, with 1024 11.3 / 96.4 (n = 512 is one slab from 512 on: 2.5 / 2.3 / 2.3).  1024 is the
// widest the interface allows (64 MiB at n = 8192).
constexpr int kCondSlabCols = 1024;
constexpr int kCondWave = 64;    // rows per workgroup of k_cond_accumulate: one wave, so the column sums need no LDS stage
// Independent loads in flight per lane.  One wave per 64 rows is all the parallelism the row order leaves (128 waves at n = 8192), so the
// kernel runs at the latency of a batch: 8 loads per batch gave 0.31 ms per 64 MiB slab in a kernel trace.
constexpr int kCondUnroll = 32;
constexpr int kCondFoldThreads = 1024;  // one column per thread for a full slab
constexpr double kCondPivotCut = 1.0e-12;  // LU_EPS of lu.hip (host_lu.rs:3)

typedef unsigned long long u64;

// X (n x w, ld n) = rows perm[0 .. n) of E(:, j0 : j0 + w): X(i, jj) = (perm[i] == j0 + jj)
__global__ void __launch_bounds__(256) k_cond_fill(double* __restrict__ X, u64 n, int w, u64 j0, const int* __restrict__ perm) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 p = (u64)perm[i];
    for (int jj = blockIdx.y; jj < w; jj += gridDim.y) X[i + (u64)jj * n] = (p == j0 + (u64)jj) ? 1.0 : 0.0;
}

__device__ __forceinline__ double cond_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum, fixed order
}

// One slab S (n x w, leading dimension ld), read once.  Lane = row: rowsum[i] += |s_ij| and rowsq[i] += s_ij^2 for j ascending;
// colpart[block * w + j] = the sum of |s_ij| over the block's 64 rows.  CHECK: *nonfinite = 1 when an entry is NaN or Inf.
template <bool CHECK>
__global__ void __launch_bounds__(kCondWave) k_cond_accumulate(const double* __restrict__ S, u64 ld, u64 n, int w, double* __restrict__ rowsum,
                                                               double* __restrict__ rowsq, double* __restrict__ colpart,
                                                               int* __restrict__ nonfinite) {
    const int lane = threadIdx.x;
    const u64 i = (u64)blockIdx.x * kCondWave + lane;
    const bool in = i < n;
    const double* s = S + (in ? i : 0);
    double* cp = colpart + (u64)blockIdx.x * (u64)w;
    double rs = in ? rowsum[i] : 0.0, rq = in ? rowsq[i] : 0.0;
    bool bad = false;
    for (int j = 0; j < w; j += kCondUnroll) {
        double v[kCondUnroll];
#pragma unroll
        for (int u = 0; u < kCondUnroll; ++u) v[u] = (in && j + u < w) ? s[(u64)(j + u) * ld] : 0.0;
#pragma unroll
        for (int u = 0; u < kCondUnroll; ++u) {
            if (j + u < w) {  // wave-uniform
                const double a = fabs(v[u]);
                rs += a;
                rq += v[u] * v[u];
                if (CHECK) bad = bad || !(a < __builtin_inf());  // NaN or Inf
                const double cs = cond_wave_sum(a);
                if (lane == 0) cp[j + u] = cs;
            }
        }
    }
    if (in) {
        rowsum[i] = rs;
        rowsq[i] = rq;
    }
    if (CHECK && bad) *nonfinite = 1;  // every writer stores the same word
}

// The slab's column sums from the per-wave partials (waves ascending), and the running maximum over all slabs so far.  One block.
__global__ void __launch_bounds__(kCondFoldThreads) k_cond_fold(const double* __restrict__ colpart, int nblk, int w, double* __restrict__ colmax) {
    __shared__ double s_max[kCondFoldThreads];
    double m = 0.0;
    for (int j = threadIdx.x; j < w; j += kCondFoldThreads) {
        double sum = 0.0;
#pragma unroll 8
        for (int b = 0; b < nblk; ++b) sum += colpart[(u64)b * (u64)w + j];
        m = sum > m || sum != sum ? sum : m;  // a NaN sum stays (the finish kernel maps what is not finite to Inf)
    }
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (int off = kCondFoldThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double a = s_max[threadIdx.x], b = s_max[threadIdx.x + off];
            s_max[threadIdx.x] = (b > a || b != b) ? b : a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = *colmax, b = s_max[0];
        *colmax = (b > a || b != b) ? b : a;
    }
}

// verdict[0] = an entry of A was not finite (set by k_cond_accumulate); verdict[1] = index of the first pivot with !(|u_kk| > 1e-12),
// -1 for none; verdict[2] = that pivot is exactly zero.  One block.
__global__ void __launch_bounds__(256) k_cond_verdict(const double* __restrict__ LU, u64 ld, u64 n, int* __restrict__ verdict) {
    __shared__ unsigned s_first[256];
    unsigned first = 0xffffffffu;
    for (u64 k = threadIdx.x; k < n; k += 256)
        if (!(fabs(LU[k + k * ld]) > kCondPivotCut)) {
            first = (unsigned)k;
            break;  // ascending per thread: its first hit is its smallest
        }
    s_first[threadIdx.x] = first;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const unsigned a = s_first[threadIdx.x], b = s_first[threadIdx.x + off];
            s_first[threadIdx.x] = b < a ? b : a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned k = s_first[0];
        verdict[1] = k == 0xffffffffu ? -1 : (int)k;
        verdict[2] = k != 0xffffffffu && LU[(u64)k + (u64)k * ld] == 0.0;
    }
}

// block-wide fixed-order reductions of the finish kernel (256 threads)
template <bool MAX>
__device__ __forceinline__ double cond_block_reduce(double v, double* lds) {
    __syncthreads();  // lds may still be read from the previous call
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double a = lds[threadIdx.x], b = lds[threadIdx.x + off];
            lds[threadIdx.x] = MAX ? ((b > a || b != b) ? b : a) : a + b;
        }
        __syncthreads();
    }
    return lds[0];
}

// norm 1 One, 2 Inf, 3 Fro of one matrix from its sums
__device__ double cond_norm_of(int norm, const double* __restrict__ rowsum, const double* __restrict__ rowsq, const double* __restrict__ colmax, u64 n,
                               double* lds) {
    if (norm == 1) return *colmax;
    double acc = 0.0;
    if (norm == 2) {
        for (u64 i = threadIdx.x; i < n; i += 256) {
            const double r = rowsum[i];
            acc = (r > acc || r != r) ? r : acc;
        }
        return cond_block_reduce<true>(acc, lds);
    }
    for (u64 i = threadIdx.x; i < n; i += 256) acc += rowsq[i];
    return sqrt(cond_block_reduce<false>(acc, lds));
}

// sums: [rowsum A | rowsq A | rowsum inv | rowsq inv | colmax A, colmax inv]
__global__ void __launch_bounds__(256) k_cond_finish(const double* __restrict__ sums, u64 n, int norm, double* __restrict__ out) {
    __shared__ double lds[256];
    const double na = cond_norm_of(norm, sums, sums + n, sums + 4 * n, n, lds);
    const double ni = cond_norm_of(norm, sums + 2 * n, sums + 3 * n, sums + 4 * n + 1, n, lds);
    if (threadIdx.x == 0) {
        const double p = na * ni;
        out[0] = (p - p == 0.0) ? p : __builtin_inf();  // cond.rs:384-388: a product that is not finite is Inf
    }
}

// cond.rs:284-290: one element
__global__ void k_cond_scalar(const double* __restrict__ a, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = a[0] == 0.0 ? __builtin_inf() : 1.0;  // NaN: 1, as on the CPU
}

int cond_launched(Context* c, const char* what) {
    c->tel.kernel_launches++;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RMHIP_OK : fail(RMHIP_ERR_HIP, "cond: %s: %s", what, hipGetErrorString(e));
}

// the three sums of an n x n matrix M (leading dimension ld), slab by slab, into rowsum / rowsq / *colmax
template <bool CHECK>
int cond_accumulate_slab(Context* c, const double* S, size_t ld, size_t n, size_t w, double* rowsum, double* rowsq, double* colpart, double* colmax,
                         int* nonfinite) {
    const unsigned nblk = (unsigned)((n + kCondWave - 1) / kCondWave);
    hipLaunchKernelGGL(k_cond_accumulate<CHECK>, dim3(nblk), dim3(kCondWave), 0, c->stream, S, (u64)ld, (u64)n, (int)w, rowsum, rowsq, colpart, nonfinite);
    RMHIP_TRY(cond_launched(c, "accumulate"));
    hipLaunchKernelGGL(k_cond_fold, dim3(1), dim3(kCondFoldThreads), 0, c->stream, (const double*)colpart, (int)nblk, (int)w, colmax);
    return cond_launched(c, "fold");
}

int scalar_out(Context* c, double v, rmhip_buf* out) {
    const size_t one[2] = {1, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(one, 2, out, &ob));
    return launch_fill(c, ob.data(), 1, v);
}

}  // namespace
}  // namespace rmhip

extern "C" {

int rmhip_cond_norm(rmhip_ctx* ctx, rmhip_buf matrix, int norm, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (norm < 0 || norm > 3) return fail(RMHIP_ERR_INVALID, "cond: unknown norm code %d", norm);
    if (norm == 0) return fail(RMHIP_ERR_UNSUPPORTED, "cond_norm: the 2-norm is served by rmhip_cond");
    Buffer mb;
    RMHIP_TRY(c->get(matrix, &mb));  // a complex tensor is refused here; f32 storage arrives as a widened copy
    for (size_t d = 2; d < mb.shape.size(); ++d)
        if (mb.shape[d] != 1) return fail(RMHIP_ERR_INVALID, "cond: inputs must be 2-D matrices or vectors");
    const size_t rows = mb.shape.empty() ? 1 : mb.shape[0], cols = mb.shape.size() < 2 ? 1 : mb.shape[1];
    if (rows == 0 || cols == 0) return scalar_out(c, 0.0, out);  // cond.rs:278-280
    const size_t one[2] = {1, 1};
    if (rows == 1 && cols == 1) {
        Buffer ob;
        RMHIP_TRY(c->new_buffer(one, 2, out, &ob));
        hipLaunchKernelGGL(k_cond_scalar, dim3(1), dim3(64), 0, c->stream, (const double*)mb.data(), ob.data());
        const int rc = cond_launched(c, "scalar");
        if (rc) {
            rmhip_free(ctx, *out);
            *out = 0;
        }
        return rc;
    }
    if (rows != cols) return fail(RMHIP_ERR_INVALID, "cond: matrix must be square for the requested norm.");
    const size_t n = rows;
    if (n > 0x7fffffffULL) return fail(RMHIP_ERR_UNSUPPORTED, "cond: dimension exceeds 2^31");
    const size_t W = n < (size_t)kCondSlabCols ? n : (size_t)kCondSlabCols;
    const size_t nblk = (n + kCondWave - 1) / kCondWave, ldw = lu_padded_ld(n);
    std::shared_ptr<Allocation> sums_mem, part_mem, flag_mem, work, perm_mem, slab;
    RMHIP_TRY(c->alloc_device(4 * n + 2, &sums_mem));  // rowsum, rowsq of A and of the inverse; the two column maxima
    RMHIP_TRY(c->alloc_device(nblk * W, &part_mem));
    RMHIP_TRY(c->alloc_device(2, &flag_mem));
    double* sums = sums_mem->ptr;
    int* verdict = (int*)flag_mem->ptr;
    RMHIP_HIP_CHECK(hipMemsetAsync(sums, 0, (4 * n + 2) * sizeof(double), c->stream));
    RMHIP_HIP_CHECK(hipMemsetAsync(verdict, 0, 2 * sizeof(double), c->stream));
    for (size_t j0 = 0; j0 < n; j0 += W) {  // A, through the code path of the inverse
        const size_t w = n - j0 < W ? n - j0 : W;
        RMHIP_TRY(cond_accumulate_slab<true>(c, mb.data() + j0 * n, n, n, w, sums, sums + n, part_mem->ptr, sums + 4 * n, verdict));
    }
    RMHIP_TRY(c->alloc_device(ldw * n, &work));
    RMHIP_TRY(c->alloc_device((n + 2) / 2 + 1, &perm_mem));
    int* perm = (int*)perm_mem->ptr;
    int info = 0;
    RMHIP_TRY(lu_copy_and_factor(c, mb.data(), n, n, work->ptr, ldw, perm, &info));
    hipLaunchKernelGGL(k_cond_verdict, dim3(1), dim3(256), 0, c->stream, (const double*)work->ptr, (u64)ldw, (u64)n, verdict);
    RMHIP_TRY(cond_launched(c, "verdict"));
    int h[3] = {0, -1, 0};
    RMHIP_HIP_CHECK(hipMemcpyAsync(h, verdict, sizeof h, hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (h[0]) return fail(RMHIP_ERR_UNSUPPORTED, "cond: non-finite data (CPU path)");
    if (h[1] >= 0 && h[2]) return scalar_out(c, INFINITY, out);  // try_inverse is None, cond.rs:354-356
    if (h[1] >= 0 || info > 0)
        return fail(RMHIP_ERR_UNSUPPORTED, "cond: pivot %d is at most 1e-12 and not zero; the host's LU answers (CPU path)", h[1] + 1);
    RMHIP_TRY(c->alloc_device(n * W, &slab));
    for (size_t j0 = 0; j0 < n; j0 += W) {
        const size_t w = n - j0 < W ? n - j0 : W;
        int rc = RMHIP_SUBST_RETRY;
        for (int round = 0; round < 2 && rc == RMHIP_SUBST_RETRY; ++round) {  // a second round only after the chain kernel timed out
            hipLaunchKernelGGL(k_cond_fill, dim3((unsigned)((n + 255) / 256), (unsigned)(w < 64 ? w : 64)), dim3(256), 0, c->stream, slab->ptr, (u64)n, (int)w,
                               (u64)j0, (const int*)perm);
            RMHIP_TRY(cond_launched(c, "fill"));
            rc = lu_substitute_device(c, work->ptr, n, ldw, slab->ptr, w, n);
        }
        RMHIP_TRY(rc);
        RMHIP_TRY(cond_accumulate_slab<false>(c, slab->ptr, n, n, w, sums + 2 * n, sums + 3 * n, part_mem->ptr, sums + 4 * n + 1, nullptr));
    }
    Buffer ob;
    RMHIP_TRY(c->new_buffer(one, 2, out, &ob));
    hipLaunchKernelGGL(k_cond_finish, dim3(1), dim3(256), 0, c->stream, (const double*)sums, (u64)n, norm, ob.data());
    const int rc = cond_launched(c, "finish");  // (the workspaces go back to the pool in stream order)
    if (rc) {
        rmhip_free(ctx, *out);
        *out = 0;
    }
    return rc;
}

}  // extern "C"
