// solve.cpp -- the dense-solve half of the C ABI (include/rmhip.h): which solver answers a system.
//   lu                                     the blocked factorisation (lu.hip) in a padded workspace
//   mldivide / mrdivide / inv / linsolve   one square general solve (small solver -> padded blocked LU -> SVD where the entry point's
//                                          policy allows it), one rectangular solve (Gram least squares -> SVD), triangular solves
//   rmhip_blk_*                            the view building blocks of the row-partitioned solve (sharded.cpp)
// The kernels live in lu.hip, small_solve.hip, svdsolve.hip, special.hip and dgemm.hip; the switches of the dispatch are solve_knobs().
#include <cmath>
#include <limits>
#include <memory>
#include <vector>

#include "common.h"
#include "csolve_plan.h"
#include "host_shape.h"

using namespace rmhip;

// The switches of the solve dispatch (docs/KNOBS.md), read here and nowhere else; each is on when the variable is set at all.
namespace rmhip {
SolveKnobs solve_knobs() {
    SolveKnobs k;
    k.svd_path = std::getenv("RMHIP_NO_SVD_PATH") == nullptr;
    k.small_solve = std::getenv("RMHIP_NO_SMALL_SOLVE") == nullptr;
    k.gram_skinny = std::getenv("RMHIP_NO_GRAM_SKINNY") == nullptr;
    return k;
}
}  // namespace rmhip

// Copy `src` (rows x cols, dense) into the padded workspace and factor it; when the persistent panel kernels
// report that their workgroups were not co-resident the copy is refreshed and factored conservatively.
// pad_n > rows (square systems on the solve path): factor [A 0; 0 I] of order pad_n instead - see lu_pad_rows
int rmhip::lu_copy_and_factor(Context* c, const double* src, size_t rows, size_t cols, double* work, size_t ldw, int* perm, int* info,
                              bool solve_path, size_t pad_n) {
    // solve_path: the caller only needs SOME stable factorisation (mldivide / linsolve / mrdivide: the pivots never leave the provider),
    // so the first attempt restricts pivoting to each panel's top block and checks the multipliers (lu.hip, k_rp_below); when that
    // check fails the copy is refreshed and factored with the reference's grid-wide rule.
    int mode = solve_path ? 1 : 0;
    for (int attempt = 0; attempt < 4; ++attempt) {  // [solve path ->] one-XCD panels -> spread panels -> one launch per column
        // (Tried: only the first 1024 columns here and the rest on the factorisation's update stream, under the first panel - the 0.8 ms
        // of a 2 GiB copy off the critical path on paper; n = 16384 98.9 vs 98.6-99.0 ms, n = 8192 34.6 vs 34.6: nothing.)
        if (rows && cols) {
            hipError_t e = hipMemcpy2DAsync(work, ldw * sizeof(double), src, rows * sizeof(double), rows * sizeof(double), cols,
                                            hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return fail(RMHIP_ERR_HIP, "lu copy: %s", hipGetErrorString(e));
        }
        const bool padded = pad_n > rows && rows == cols;
        if (padded) RMHIP_TRY(lu_pad_identity_device(c, work, ldw, rows, pad_n));
        const int rc = lu_factor_device(c, work, padded ? pad_n : rows, padded ? pad_n : cols, ldw, perm, info, nullptr, mode);
        if (rc == RMHIP_LU_GROWTH) {
            mode = 0;
            c->lu_growth_fallbacks++;
            // telemetry.solve_fallbacks names it when a multiplier actually exceeded the bound; a pivot at the singular cut-off inside a
            // top block also lands here (the grid-wide rule has to confirm it), and is then reported as what it turns out to be
            if (!(c->lu_last_growth <= c->lu_tau) || lu_knobs().test_growth) c->record_solve_fallback("lu:pivot_growth");
            continue;
        }
        if (rc == RMHIP_OK && mode == 1 && c->lu_last_fast) c->lu_fast_count++;  // RMHIP_LU_FAST=0 / conservative panels: the grid-wide rule ran
        if (rc != RMHIP_LU_RETRY) return rc;
    }
    return fail(RMHIP_ERR_HIP, "lu: factorisation failed on every panel path");
}

size_t rmhip::lu_padded_ld(size_t rows) { return rows >= 256 ? ((rows + 1) & ~(size_t)1) + 32 : ((rows + 1) & ~(size_t)1); }

// X (n x nrhs, ld n) = A^-1 B from factors of order np >= n (np > n: the padded system)
static int lu_solve_padded(Context* c, const double* LU, size_t n, size_t np, size_t ldw, const int* perm, const double* B, size_t nrhs, double* X) {
    if (nrhs == 0) return RMHIP_OK;  // (a zero-height hipMemcpy2DAsync is hipErrorInvalidValue)
    if (np == n) return lu_solve_device(c, LU, n, ldw, perm, B, nrhs, n, X, n);
    std::shared_ptr<Allocation> bp, xp;
    RMHIP_TRY(c->alloc_device(np * nrhs, &bp));
    RMHIP_TRY(c->alloc_device(np * nrhs, &xp));
    RMHIP_HIP_CHECK(hipMemsetAsync(bp->ptr, 0, sizeof(double) * np * nrhs, c->stream));
    RMHIP_HIP_CHECK(hipMemcpy2DAsync(bp->ptr, np * sizeof(double), B, n * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDeviceToDevice, c->stream));
    RMHIP_TRY(lu_solve_device(c, LU, np, ldw, perm, bp->ptr, nrhs, np, xp->ptr, np));
    RMHIP_HIP_CHECK(hipMemcpy2DAsync(X, n * sizeof(double), xp->ptr, np * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDeviceToDevice, c->stream));
    return RMHIP_OK;
}

// solve_fallbacks (telemetry.rs:95-99): a soft failure of a solve is what sends the caller to its CPU path
static int count_fallback(Context* c, int rc, const char* unsupported, const char* singular) {
    if (rc == RMHIP_ERR_UNSUPPORTED) c->record_solve_fallback(unsupported);
    else if (rc == RMHIP_ERR_SINGULAR) c->record_solve_fallback(singular);
    return rc;
}

// The corrected semi-normal equations of lstsq_full_rank on a factored Gram matrix (`lu`, order min(m, n)): X = the refined solution.
// `skinny_gram`: the (n + nrhs)^2 Gram buffer of [A | b] when the VALU Gram kernel serves the tall system (A'b and A'r come out of it).
static int lstsq_refined_solve(Context* c, const double* A, size_t m, size_t n, const double* B, size_t nrhs, const double* lu, size_t ldw,
                               const int* perm, double* skinny_gram, double* X) {
    const size_t g = m > n ? n : m, gl = n + nrhs;
    std::shared_ptr<Allocation> t1, t2, t3;
    RMHIP_TRY(c->alloc_device(g * nrhs, &t1));  // right-hand side of the Gram system
    RMHIP_TRY(c->alloc_device(g * nrhs, &t2));  // its solution
    RMHIP_TRY(c->alloc_device(m * nrhs, &t3));  // residual b - A x
    if (m > n) {
        if (skinny_gram)  // A'b = the last nrhs columns of the Gram matrix of [A | b]
            RMHIP_HIP_CHECK(hipMemcpy2DAsync(t1->ptr, n * sizeof(double), skinny_gram + n * gl, gl * sizeof(double), n * sizeof(double), nrhs,
                                             hipMemcpyDeviceToDevice, c->stream));
        else RMHIP_TRY(launch_dgemm_trans(c, true, false, n, nrhs, m, 1.0, A, m, B, m, 0.0, t1->ptr, n));         // A'b
        RMHIP_TRY(lu_solve_device(c, lu, n, ldw, perm, t1->ptr, nrhs, n, X, n));                                  // x0
        RMHIP_HIP_CHECK(hipMemcpyAsync(t3->ptr, B, m * nrhs * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        RMHIP_TRY(launch_dgemm(c, m, nrhs, n, -1.0, A, m, X, n, 1.0, t3->ptr, m));                                // r = b - A x0
        if (skinny_gram) {  // A'r the same way
            RMHIP_TRY(gram_skinny_device(c, A, m, n, nullptr, 1.0, false, skinny_gram, t3->ptr, nrhs));
            RMHIP_HIP_CHECK(hipMemcpy2DAsync(t1->ptr, n * sizeof(double), skinny_gram + n * gl, gl * sizeof(double), n * sizeof(double), nrhs,
                                             hipMemcpyDeviceToDevice, c->stream));
        } else RMHIP_TRY(launch_dgemm_trans(c, true, false, n, nrhs, m, 1.0, A, m, t3->ptr, m, 0.0, t1->ptr, n));  // A'r
        RMHIP_TRY(lu_solve_device(c, lu, n, ldw, perm, t1->ptr, nrhs, n, t2->ptr, n));                            // dx
        return launch_binary_same(c, RMHIP_ADD, X, t2->ptr, X, n * nrhs);
    }
    RMHIP_TRY(lu_solve_device(c, lu, m, ldw, perm, B, nrhs, m, t2->ptr, m));                           // y0
    RMHIP_TRY(launch_dgemm_trans(c, true, false, n, nrhs, m, 1.0, A, m, t2->ptr, m, 0.0, X, n));       // x0 = A'y0
    RMHIP_HIP_CHECK(hipMemcpyAsync(t3->ptr, B, m * nrhs * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    RMHIP_TRY(launch_dgemm(c, m, nrhs, n, -1.0, A, m, X, n, 1.0, t3->ptr, m));                         // r = b - A x0
    RMHIP_TRY(lu_solve_device(c, lu, m, ldw, perm, t3->ptr, nrhs, m, t2->ptr, m));                     // dy
    return launch_dgemm_trans(c, true, false, n, nrhs, m, 1.0, A, m, t2->ptr, m, 1.0, X, n);           // x += A'dy
}

// Rectangular A\b for FULL-RANK, reasonably conditioned A.  The reference answers every shape with the SVD's minimum-norm
// least-squares solution (mldivide.rs:380-404); for full column rank (rows > cols) that is the unique least-squares
// solution, for full row rank (rows < cols) the minimum-norm solution A' (A A')^-1 b.  Both come from the kernels already
// here: the Gram matrix on the MFMA path (A'A or AA'), its LU with partial pivoting, and ONE step of refinement on the
// residual (corrected semi-normal equations): x0 = G^-1 A'b, r = b - A x0, x = x0 + G^-1 A'r - error ~ eps * cond(A) once
// cond(A)^2 * eps < 1.  Anything else stays with the caller's CPU SVD path: a pivot of G below the LU's cut-off, or a
// pivot ratio min|u_ii| / max|u_ii| below 1e-11 (cond(A) beyond ~3e5, or rank deficient) -> RMHIP_ERR_UNSUPPORTED.
static int lstsq_full_rank(rmhip_ctx* ctx, Context* c, const double* A, size_t m, size_t n, const double* B, size_t nrhs,
                           rmhip_buf* out) {
    if (m == 0 || n == 0 || nrhs == 0) return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: empty system");
    const bool tall = m > n;
    const size_t g = tall ? n : m;  // order of the Gram matrix
    std::shared_ptr<Allocation> gram, work, perm_mem;
    // Regression shapes - many observations of a few variables: the Gram matrix of [A | b] on the VALU kernel (special.hip) holds A'A
    // and A'b from ONE pass over both; the MFMA route ran 256-wide split-k tiles for 8-32 useful columns (2^20 x 8 \ b: 2.0 ms).
    const bool skinny = tall && gram_skinny_applies(m, n + nrhs) && solve_knobs().gram_skinny;
    const size_t gl = skinny ? n + nrhs : g;  // leading dimension of the Gram buffer
    RMHIP_TRY(c->alloc_device(gl * gl, &gram));
    // G = A'A (tall) or A A' (wide); the transposed operand is read in place
    if (skinny) RMHIP_TRY(gram_skinny_device(c, A, m, n, nullptr, 1.0, false, gram->ptr, B, nrhs));
    else if (tall) RMHIP_TRY(launch_dgemm_trans(c, true, false, n, n, m, 1.0, A, m, A, m, 0.0, gram->ptr, n));
    else RMHIP_TRY(launch_dgemm_trans(c, false, true, m, m, n, 1.0, A, m, A, m, 0.0, gram->ptr, m));
    const size_t ldw = lu_padded_ld(g);
    RMHIP_TRY(c->alloc_device(ldw * g, &work));
    RMHIP_TRY(c->alloc_device((g + 2) / 2 + 1, &perm_mem));
    int* perm = (int*)perm_mem->ptr;
    int info = 0;
    if (skinny) {  // the leading n x n block of the (n + nrhs)^2 Gram matrix
        std::shared_ptr<Allocation> sq;
        RMHIP_TRY(c->alloc_device(g * g, &sq));
        RMHIP_HIP_CHECK(hipMemcpy2DAsync(sq->ptr, g * sizeof(double), gram->ptr, gl * sizeof(double), g * sizeof(double), g, hipMemcpyDeviceToDevice, c->stream));
        RMHIP_TRY(lu_copy_and_factor(c, sq->ptr, g, g, work->ptr, ldw, perm, &info, true));
    } else {
        RMHIP_TRY(lu_copy_and_factor(c, gram->ptr, g, g, work->ptr, ldw, perm, &info, true));
    }
    if (info > 0)
        return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: rank-deficient rectangular system (%d pivot(s) of the Gram matrix <= 1e-12): CPU SVD path", info);
    {
        // (a strided device-to-host copy of the diagonal - one 8-byte row per pivot - took 15 of the 20 ms of a 1000 x 10000 solve)
        double lo = INFINITY, hi = 0.0;
        size_t zeros = 0;
        RMHIP_TRY(diag_stats_device(c, work->ptr, ldw, g, &lo, &hi, &zeros));
        if (!(lo > 1e-11 * hi))
            return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: ill-conditioned rectangular system (Gram pivot ratio %.2e): CPU SVD path", hi > 0 ? lo / hi : 0.0);
    }
    Buffer ob;
    rmhip_buf oid = 0;
    const size_t oshape[2] = {n, nrhs};
    RMHIP_TRY(c->new_buffer(oshape, 2, &oid, &ob));
    const int rc = lstsq_refined_solve(c, A, m, n, B, nrhs, work->ptr, ldw, perm, skinny ? gram->ptr : nullptr, ob.data());
    if (rc) {
        rmhip_free(ctx, oid);
        return rc;
    }
    *out = oid;
    return RMHIP_OK;
}

// What the LU / Gram paths refuse - singular, rank-deficient or ill-conditioned systems - answered the way the reference answers every
// system: minimum-norm least squares from an SVD with its tolerance rule (svdsolve.hip), as long as min(rows, cols) <= svd_max_cols().
// `refused` is the status of the path that gave up, returned unchanged when the entry point does not allow an SVD answer (`allowed`),
// the system is too large for the SVD path or RMHIP_NO_SVD_PATH is set.  `tol_dim` is handed through to svd_solve_device (0: max(m, n)).
static int svd_fallback(rmhip_ctx* ctx, Context* c, bool allowed, int refused, const double* A, size_t m, size_t n, const double* B, size_t nrhs,
                        rmhip_buf* out, size_t tol_dim = 0) {
    if (!allowed || (m < n ? m : n) > (size_t)svd_max_cols() || !solve_knobs().svd_path) return refused;
    Buffer ob;
    rmhip_buf oid = 0;
    const size_t oshape[2] = {n, nrhs};
    RMHIP_TRY(c->new_buffer(oshape, 2, &oid, &ob));
    int rank = 0;
    const int rc = svd_solve_device(c, A, m, n, B, nrhs, ob.data(), &rank, tol_dim);
    if (rc) {
        rmhip_free(ctx, oid);
        return rc;
    }
    c->svd_solves++;
    *out = oid;
    return RMHIP_OK;
}

// A rectangular system: the Gram route, then the SVD for what it refuses (an empty system is refused by both)
static int solve_rectangular(rmhip_ctx* ctx, Context* c, bool allow_svd, const double* A, size_t m, size_t n, const double* B, size_t nrhs,
                             rmhip_buf* out, size_t tol_dim = 0) {
    const int rc = lstsq_full_rank(ctx, c, A, m, n, B, nrhs, out);
    if (rc != RMHIP_ERR_UNSUPPORTED || !m || !n || !nrhs) return rc;
    return svd_fallback(ctx, c, allow_svd, rc, A, m, n, B, nrhs, out, tol_dim);
}

// How an entry point wants its general square system answered
struct SolvePolicy {
    const char* who;            // the entry point the messages name
    const char* singular_hint;  // how its pivot-at-the-cut-off message ends
    bool ratio_proxy;           // a tiny pivot RATIO (no pivot at the cut-off) is refused too and left to the SVD: mldivide yes, linsolve no
    bool allow_svd;             // a refused system may be answered by the SVD (inv: no - the minimum-norm solution is no inverse)
};

// X = A \ B for a general square A of order n >= 1: the one-launch small solver where it applies, otherwise the blocked LU in the padded
// workspace; a pivot at the cut-off (or, under `ratio_proxy`, a tiny pivot ratio) sets the SINGULAR message and the SVD answers if it may.
// `tol_dim` only reaches the SVD's rank tolerance (0: n); the ratio proxy below is a routing heuristic and counts with the order it is given.
static int solve_square_general(rmhip_ctx* ctx, Context* c, SolvePolicy p, const double* A, size_t n, const double* B, size_t nrhs,
                                rmhip_buf* out, size_t tol_dim = 0) {
    const SolveKnobs knobs = solve_knobs();
    auto at_cutoff = [&](size_t pivots) {
        const int refused = fail(RMHIP_ERR_SINGULAR, "%s: %zu pivot(s) <= 1e-12; %s", p.who, pivots, p.singular_hint);
        return nrhs ? svd_fallback(ctx, c, p.allow_svd, refused, A, n, n, B, nrhs, out, tol_dim) : refused;  // no right-hand side: nothing for the SVD to answer
    };
    // A nearly singular matrix need not produce a pivot below the cut-off, yet the reference would DROP its small singular values
    // (s_i <= eps * n * max(s_max, 1), mldivide.rs:396-404) where an LU divides by them.  Pivot ratio as the (cheap, rough) proxy of
    // the condition number: below 1e3 * n * eps the SVD decides.
    const bool proxy = p.ratio_proxy && knobs.svd_path;
    const double ratio_floor = 1.0e3 * (double)n * 2.220446049250313e-16;
    auto tiny_ratio = [&](double mn, double mx) {
        const int refused = fail(RMHIP_ERR_SINGULAR, "%s: pivot ratio %.2e: numerically singular", p.who, mx > 0 ? mn / mx : 0.0);
        return svd_fallback(ctx, c, p.allow_svd, refused, A, n, n, B, nrhs, out, tol_dim);
    };
    Buffer ob;
    rmhip_buf oid = 0;
    const size_t oshape[2] = {n, nrhs};
    // Small systems: elimination, substitution and the pivot statistics in ONE launch of one workgroup (small_solve.hip) - the blocked
    // path below is a dozen launches and two read-backs whatever the order.  Same decisions on the pivots.  RMHIP_LU_FAST=0 (the
    // grid-wide rule everywhere) and RMHIP_NO_SMALL_SOLVE=1 keep the blocked path.
    if (small_solve_applies(n, nrhs) && lu_knobs().fast && knobs.small_solve) {
        RMHIP_TRY(c->new_buffer(oshape, 2, &oid, &ob));
        double mn = 0.0, mx = 0.0;
        size_t bad = 0;
        const int rc = small_solve_device(c, A, B, n, nrhs, ob.data(), &mn, &mx, &bad);
        const bool ratio_refused = !rc && !bad && proxy && !(mn > ratio_floor * mx);
        if (rc || bad || ratio_refused) {
            rmhip_free(ctx, oid);
            return rc ? rc : bad ? at_cutoff(bad) : tiny_ratio(mn, mx);
        }
        c->lu_fast_count++;
        c->lu_last_growth = 0.0;  // partial pivoting over the whole column: every multiplier is <= 1
        *out = oid;
        return RMHIP_OK;
    }
    // Factorisation workspace with a PADDED leading dimension: with lda a large power of two every
    // element of a row maps to the same HBM channel / L2 slice, and the panel kernels (one lane per
    // row, walking across columns) serialise on it; +32 doubles rotates the channel per column.
    const size_t np = lu_pad_rows(n, lu_knobs().pad);  // order of the factorisation (the next multiple of 128 for a large ragged n)
    const size_t ldw = lu_padded_ld(np);
    std::shared_ptr<Allocation> work, perm_mem;  // pooled, released in stream order
    RMHIP_TRY(c->alloc_device(ldw * np, &work));
    RMHIP_TRY(c->alloc_device((np + 2) / 2 + 1, &perm_mem));
    int* perm = (int*)perm_mem->ptr;
    int info = 0;
    RMHIP_TRY(lu_copy_and_factor(c, A, n, n, work->ptr, ldw, perm, &info, true, np));
    if (info > 0) return at_cutoff((size_t)info);  // up to svd_max_cols(): the SVD answer on the device
    // the proxy only where the SVD path is cheap (n <= kSvdProxyMaxCols, < 0.5 s); larger systems keep the LU answer unless a pivot
    // fell below the cut-off
    if (proxy && n <= (size_t)kSvdProxyMaxCols && n <= (size_t)svd_max_cols() && n > 1 && nrhs) {
        double mn = 0.0, mx = 0.0;
        size_t zeros = 0;
        if (diag_stats_device(c, work->ptr, ldw, n, &mn, &mx, &zeros) == RMHIP_OK && !(mn > ratio_floor * mx)) return tiny_ratio(mn, mx);
    }
    RMHIP_TRY(c->new_buffer(oshape, 2, &oid, &ob));
    const int rc = lu_solve_padded(c, work->ptr, n, np, ldw, perm, B, nrhs, ob.data());
    if (rc) {
        rmhip_free(ctx, oid);
        return rc;
    }
    *out = oid;
    return RMHIP_OK;
}

// X = other * (1 / divisor) for a 1 x 1 divisor (mldivide.rs:321-325, mrdivide.rs:321-325); both operands as Context::get hands them over
static int scale_by_reciprocal(rmhip_ctx* ctx, Context* c, const Buffer& divisor, const Buffer& other, const std::vector<size_t>& oshape,
                               rmhip_buf* out) {
    double d = 0.0;
    RMHIP_HIP_CHECK(hipMemcpyAsync(&d, divisor.data(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    Buffer ob;
    RMHIP_TRY(c->new_buffer(oshape.data(), 2, out, &ob));
    int rc = launch_scalar(c, RMHIP_SMUL, other.data(), 1.0 / d, ob.data(), other.numel);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

// A \ B behind mldivide, mrdivide (on the transposes) and inv (B = I, allow_svd = false); the messages name mldivide for all three
static int mldivide_impl(rmhip_ctx* ctx, Context* c, rmhip_buf a, rmhip_buf b, bool allow_svd, rmhip_buf* out) {
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab, bb;
    RMHIP_TRY(c->get(a, &ab));
    RMHIP_TRY(c->get(b, &bb));
    if (ab.shape.size() > 2 || bb.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: only 2D supported");
    const std::vector<size_t> as = normalize_matrix_shape(ab.shape), bs = normalize_matrix_shape(bb.shape);
    if (ab.numel == 1) return scale_by_reciprocal(ctx, c, ab, bb, bs, out);  // scalar lhs: rhs * (1/lhs)
    if (as[0] != bs[0]) return fail(RMHIP_ERR_SHAPE, "mldivide: row mismatch (%zu vs %zu)", as[0], bs[0]);
    if (as[0] != as[1]) return solve_rectangular(ctx, c, allow_svd, ab.data(), as[0], as[1], bb.data(), bs[1], out);
    if (as[0] == 0) return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: empty system");
    const SolvePolicy policy{"mldivide", "matrix is numerically singular, use the CPU SVD path", true, allow_svd};
    return solve_square_general(ctx, c, policy, ab.data(), as[0], bb.data(), bs[1], out);
}

// ---- the dense solves on complex-interleaved operands (csolve_plan.h, csolve.hip) ------------------------------------------------------
// One real solve of the embedded system through the cores above, between an embed / stack pass and a join.  The system is m x n with nrhs
// right-hand sides in COMPLEX extents; `transposed` (mrdivide): A is stored n x m and B nrhs x m, the system is A.' X.' = B.' with PLAIN
// transposes, and the join writes X (nrhs x n).  `kind` is complex_matmul's (0 both complex, 1 A complex and B real, 2 A real and B
// complex); inv passes kind 0 with B == nullptr, its right-hand side is [I; 0].  Both operands as Context::get_any hands them over.
// The result is a complex buffer of shape `oshape`; the real solution the cores register is freed before returning.  `pl` is the
// caller's plan_csolve(entry, kind, m, n, nrhs), already found servable; m and n are not zero.  The messages of the cores name mldivide
// for all three entry points, as mldivide_impl's do for the real ones.
static int complex_solve(rmhip_ctx* ctx, Context* c, const CsolvePlan& pl, int entry, int kind, const double* A, const double* B, size_t m,
                         size_t n, size_t nrhs, bool allow_svd, const size_t* oshape, size_t orank, rmhip_buf* out) {
    const bool transposed = pl.transpose_a;
    std::shared_ptr<Allocation> ws;  // [E(A) or the transposed real A][stacked right-hand side]; back in the pool on return, in stream order
    RMHIP_TRY(c->alloc_device(pl.workspace ? pl.workspace : 1, &ws));
    double* const T = ws->ptr + pl.a_workspace;
    const double* Areal = A;
    if (pl.embed_a) {
        RMHIP_TRY(launch_csolve_embed(c, A, transposed ? n : m, transposed ? m : n, transposed, ws->ptr));
        Areal = ws->ptr;
    } else if (transposed) {
        RMHIP_TRY(transpose_device(c, A, n, n, m, ws->ptr, m));
        Areal = ws->ptr;
    }
    RMHIP_TRY(launch_csolve_stack(c, B ? kind : 3, B, m, nrhs, transposed, T));
    rmhip_buf xid = 0;
    if (pl.M != pl.N) {
        RMHIP_TRY(solve_rectangular(ctx, c, allow_svd, Areal, pl.M, pl.N, T, pl.NRHS, &xid, pl.tol_dim));
    } else {
        const SolvePolicy policy{"mldivide", "matrix is numerically singular, use the CPU SVD path", true, allow_svd};
        RMHIP_TRY(solve_square_general(ctx, c, policy, Areal, pl.M, T, pl.NRHS, &xid, pl.tol_dim));
    }
    Buffer xb, ob;
    int rc = c->lookup(xid, &xb);
    if (!rc) rc = c->new_buffer_complex(oshape, orank, out, &ob);
    if (!rc) {
        rc = launch_csolve_join(c, kind, xb.data(), n, nrhs, transposed, ob.data());
        if (rc) {
            rmhip_free(ctx, *out);
            *out = 0;
        }
    }
    rmhip_free(ctx, xid);
    if (rc) return rc;
    c->record_launch("complex_solve", {{"m", m}, {"n", n}, {"nrhs", nrhs}}, {{"kind", (uint64_t)kind}, {"entry", (uint64_t)entry}});
    return RMHIP_OK;
}

// A \ B or (divide_right) B / A with at least one complex-interleaved operand; `who` is "mldivide" or "mrdivide"
static int complex_divide_impl(rmhip_ctx* ctx, Context* c, bool divide_right, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    const char* who = divide_right ? "mrdivide" : "mldivide";
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    *out = 0;
    Buffer ra, rb;
    RMHIP_TRY(c->lookup(a, &ra));
    RMHIP_TRY(c->lookup(b, &rb));
    if (!ra.cplx && !rb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_%s: both operands are real (rmhip_%s serves them)", who, who);
    if (ra.shape.size() > 2 || rb.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "%s: only 2D supported", who);
    const std::vector<size_t> as = normalize_matrix_shape(ra.shape), bs = normalize_matrix_shape(rb.shape);
    // the reference's scalar form is an elementwise complex reciprocal and product: it stays with the host
    if (ra.numel == 1) return fail(RMHIP_ERR_UNSUPPORTED, "complex_%s: scalar operands use the CPU path", who);
    if (!divide_right && as[0] != bs[0]) return fail(RMHIP_ERR_SHAPE, "mldivide: row mismatch (%zu vs %zu)", as[0], bs[0]);
    if (divide_right && bs[1] != as[1]) return fail(RMHIP_ERR_SHAPE, "mrdivide: column mismatch (%zu vs %zu)", bs[1], as[1]);
    const int kind = ra.cplx && rb.cplx ? 0 : (ra.cplx ? 1 : 2);
    // the system the solve sees: A (m x n) X = B, or A.' (m x n) X.' = B.'
    const size_t m = divide_right ? as[1] : as[0], n = divide_right ? as[0] : as[1], nrhs = divide_right ? bs[0] : bs[1];
    const CsolvePlan pl = plan_csolve(divide_right ? CSOLVE_MRDIVIDE : CSOLVE_MLDIVIDE, kind, m, n, nrhs);
    if (pl.unsupported) return fail(RMHIP_ERR_UNSUPPORTED, "%s", pl.unsupported);
    if (m == 0 || n == 0) return fail(RMHIP_ERR_UNSUPPORTED, "mldivide: empty system");
    Buffer ab, bb;
    RMHIP_TRY(c->get_any(a, &ab));
    RMHIP_TRY(c->get_any(b, &bb));
    const size_t oshape[2] = {divide_right ? nrhs : n, divide_right ? n : nrhs};
    return complex_solve(ctx, c, pl, divide_right ? CSOLVE_MRDIVIDE : CSOLVE_MLDIVIDE, kind, ab.data(), bb.data(), m, n, nrhs, true, oshape, 2,
                         out);
}

extern "C" {

int rmhip_complex_mldivide(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.mldivide_count, &c->tel.mldivide_ns);
    return count_fallback(c, complex_divide_impl(ctx, c, false, a, b, out), "mldivide:unsupported", "mldivide:singular");
}

int rmhip_complex_mrdivide(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.mrdivide_count, &c->tel.mrdivide_ns);
    return count_fallback(c, complex_divide_impl(ctx, c, true, a, b, out), "mrdivide:unsupported", "mrdivide:singular");
}

int rmhip_complex_inv(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    *out = 0;
    Buffer ab;
    RMHIP_TRY(c->lookup(a, &ab));
    if (!ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_inv: the operand is real (rmhip_inv serves it)");
    // rmhip_inv's shape rules and wording (matrix_dimensions, inv.rs:209-230)
    const std::vector<size_t>& s = ab.shape;
    size_t rows = 1, cols = 1;
    if (s.size() == 1) {
        if (s[0] != 1) return fail(RMHIP_ERR_INVALID, "inv: input must be a square matrix.");
    } else if (s.size() >= 2) {
        for (size_t d = 2; d < s.size(); ++d)
            if (s[d] != 1) return fail(RMHIP_ERR_INVALID, "inv: inputs must be 2-D matrices.");
        rows = s[0];
        cols = s[1];
    }
    if (rows != cols) return fail(RMHIP_ERR_INVALID, "inv: input must be a square matrix.");
    if (rows == 1) return fail(RMHIP_ERR_UNSUPPORTED, "complex_inv: scalar operands use the CPU path");
    if (rows == 0) return c->new_buffer_complex(s.data(), s.size(), out);
    // (an order the real solve cannot take is refused in mldivide's words, as rmhip_inv refuses it through mldivide_impl)
    const CsolvePlan pl = plan_csolve(CSOLVE_INV, 0, rows, rows, rows);
    if (pl.unsupported) return count_fallback(c, fail(RMHIP_ERR_UNSUPPORTED, "%s", pl.unsupported), "inv:unsupported", "inv:singular");
    // ONE embedded solve E(A) \ [I; 0], not inv(E(A)); a singular matrix is RMHIP_ERR_SINGULAR as in rmhip_inv - the minimum-norm
    // solution mldivide would return is no inverse
    return count_fallback(c, complex_solve(ctx, c, pl, CSOLVE_INV, 0, ab.data(), nullptr, rows, rows, rows, false, s.data(), s.size(), out),
                          "inv:unsupported", "inv:singular");
}

int rmhip_lu(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf out5[5]) {
    CTX_OR_FAIL(ctx);
    if (!out5) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab;
    RMHIP_TRY(c->get(a, &ab));
    if (ab.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "lu: only 2D supported");
    const std::vector<size_t> shape = normalize_matrix_shape(ab.shape);
    const size_t rows = shape[0], cols = shape[1];
    Buffer comb, L, U, P, piv;
    rmhip_buf ids[5] = {0, 0, 0, 0, 0};
    const size_t s_comb[2] = {rows, cols}, s_l[2] = {rows, rows}, s_piv[2] = {rows, 1};
    int rc = c->new_buffer(s_comb, 2, &ids[0], &comb);
    if (!rc) rc = c->new_buffer(s_l, 2, &ids[1], &L);
    if (!rc) rc = c->new_buffer(s_comb, 2, &ids[2], &U);
    if (!rc) rc = c->new_buffer(s_l, 2, &ids[3], &P);
    if (!rc) rc = c->new_buffer(s_piv, 2, &ids[4], &piv);
    int* perm = nullptr;
    std::shared_ptr<Allocation> perm_mem;  // pooled (a hipMalloc / hipFree pair costs two device synchronisations per call)
    if (!rc) rc = c->alloc_device((rows + 2) / 2 + 1, &perm_mem);
    if (!rc) perm = (int*)perm_mem->ptr;
    const size_t ldw = lu_padded_ld(rows);
    std::shared_ptr<Allocation> work;
    if (!rc) rc = c->alloc_device(ldw * (cols ? cols : 1), &work);
    int info = 0;
    if (!rc) rc = lu_copy_and_factor(c, ab.data(), rows, cols, work->ptr, ldw, perm, &info);
    if (!rc && ab.numel) {
        hipError_t e = hipMemcpy2DAsync(comb.data(), rows * sizeof(double), work->ptr, ldw * sizeof(double), rows * sizeof(double),
                                        cols, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = fail(RMHIP_ERR_HIP, "lu copy back: %s", hipGetErrorString(e));
    }
    if (!rc) rc = lu_extract_device(c, comb.data(), rows, cols, perm, L.data(), U.data(), P.data(), piv.data());
    if (rc) {
        for (auto id : ids)
            if (id) rmhip_free(ctx, id);
        return rc;
    }
    for (int i = 0; i < 5; ++i) out5[i] = ids[i];
    return RMHIP_OK;
}

int rmhip_mldivide(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.mldivide_count, &c->tel.mldivide_ns);
    return count_fallback(c, mldivide_impl(ctx, c, a, b, true, out), "mldivide:unsupported", "mldivide:singular");
}

int rmhip_inv(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab;
    RMHIP_TRY(c->get_raw(a, &ab));
    // matrix_dimensions + inv_real_tensor_impl (inv.rs:209-230, 258-280)
    const std::vector<size_t>& s = ab.shape;
    size_t rows = 1, cols = 1;
    if (s.size() == 1) {
        if (s[0] != 1) return fail(RMHIP_ERR_INVALID, "inv: input must be a square matrix.");
    } else if (s.size() >= 2) {
        for (size_t d = 2; d < s.size(); ++d)
            if (s[d] != 1) return fail(RMHIP_ERR_INVALID, "inv: inputs must be 2-D matrices.");
        rows = s[0];
        cols = s[1];
    }
    if (rows != cols) return fail(RMHIP_ERR_INVALID, "inv: input must be a square matrix.");
    if (rows == 0) {
        Buffer ob;
        return c->new_buffer(s.data(), s.size(), out, &ob);
    }
    // X = A \ I on the LU path (the CPU's nalgebra `try_inverse` is the same factorisation followed by the same substitutions); a pivot
    // below the solver's cut-off is RMHIP_ERR_SINGULAR and the caller's CPU path words the "singular to working precision" error
    rmhip_buf eye = 0, x = 0, same = 0;
    const size_t sq[2] = {rows, rows};
    const std::vector<size_t> given = s;  // (rmhip_reshape renames the shape of the SAME buffer: the operand gets its own back below)
    int rc = rmhip_eye(ctx, sq, 2, &eye);
    const bool reshaped = !rc && given.size() != 2;
    if (reshaped) rc = rmhip_reshape(ctx, a, sq, 2, &same);
    // mldivide answers a singular square system with the minimum-norm solution; inv must not
    if (!rc) rc = count_fallback(c, mldivide_impl(ctx, c, a, eye, false, &x), "inv:unsupported", "inv:singular");
    if (reshaped) rmhip_reshape(ctx, a, given.data(), given.size(), &same);
    if (eye) rmhip_free(ctx, eye);
    if (rc) return rc;
    if (given.size() > 2) {  // inv.rs:402-412: a trailing singleton dimension is kept
        rc = rmhip_reshape(ctx, x, given.data(), given.size(), &same);
        if (rc) {
            rmhip_free(ctx, x);
            return rc;
        }
    }
    *out = x;
    return RMHIP_OK;
}

int rmhip_mrdivide(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.mrdivide_count, &c->tel.mrdivide_ns);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab, bb;
    RMHIP_TRY(c->get_raw(a, &ab));
    RMHIP_TRY(c->get_raw(b, &bb));
    if (ab.shape.size() > 2 || bb.shape.size() > 2)
        return count_fallback(c, fail(RMHIP_ERR_UNSUPPORTED, "mrdivide: only 2D supported"), "mrdivide:unsupported", "mrdivide:singular");
    const std::vector<size_t> as = normalize_matrix_shape(ab.shape), bs = normalize_matrix_shape(bb.shape);
    if (ab.numel == 1) {  // scalar divisor: lhs * (1/rhs)
        RMHIP_TRY(c->get(a, &ab));
        RMHIP_TRY(c->get(b, &bb));
        return scale_by_reciprocal(ctx, c, ab, bb, bs, out);
    }
    if (bs[1] != as[1]) return fail(RMHIP_ERR_SHAPE, "mrdivide: column mismatch (%zu vs %zu)", bs[1], as[1]);  // mrdivide.rs:327
    // X = B / A  <=>  A' X' = B'  (mrdivide.rs:379-388): transpose views feed the LU path (a view is materialised on first use)
    rmhip_buf at = 0, bt = 0, xt = 0, x = 0;
    int rc = rmhip_transpose(ctx, a, &at);
    if (!rc) rc = rmhip_transpose(ctx, b, &bt);
    if (!rc) rc = mldivide_impl(ctx, c, at, bt, true, &xt);
    if (!rc) rc = rmhip_transpose(ctx, xt, &x);
    if (!rc) rc = c->settle_view(x);  // the result is a plain buffer, not a view of the temporary
    if (at) rmhip_free(ctx, at);
    if (bt) rmhip_free(ctx, bt);
    if (xt) rmhip_free(ctx, xt);
    if (rc) {
        if (x) rmhip_free(ctx, x);
        return count_fallback(c, rc, "mrdivide:unsupported", "mrdivide:singular");
    }
    *out = x;
    return RMHIP_OK;
}

// serve_rcond: the call came through rmhip_linsolve_rcond - a general matrix with need_rcond / has_rcond, which rmhip_linsolve declines;
// the solution is the one the sibling computes with both fields cleared, rcond comes from the Jacobi singular values
static int linsolve_impl(rmhip_ctx* ctx, Context* c, rmhip_buf a, rmhip_buf b, const rmhip_linsolve_options_t* opts, rmhip_buf* out,
                         double* reciprocal_condition, bool serve_rcond) {
    if (!out || !opts) return fail(RMHIP_ERR_INVALID, "linsolve: null argument");
    Buffer ab, bb;
    RMHIP_TRY(c->get(a, &ab));
    RMHIP_TRY(c->get(b, &bb));
    if (ab.shape.size() > 2 || bb.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "linsolve: only 2D supported");
    std::vector<size_t> as = normalize_matrix_shape(ab.shape);
    if (ab.numel == 1 || bb.numel == 1)  // linsolve.rs:408-412: scalar operands stay on the host path
        return fail(RMHIP_ERR_UNSUPPORTED, "linsolve: scalar operands use the CPU path");
    bool lower = opts->lower != 0, upper = opts->upper != 0;
    const double* A = ab.data();
    std::shared_ptr<Allocation> at;
    if (opts->transposed) {  // linsolve.rs:698-705: materialise A' and swap the triangle hints
        RMHIP_TRY(c->alloc_device(ab.numel ? ab.numel : 1, &at));
        RMHIP_TRY(transpose_device(c, ab.data(), as[0], as[0], as[1], at->ptr, as[1]));
        std::swap(as[0], as[1]);
        A = at->ptr;
        if (lower || upper) std::swap(lower, upper);
    }
    // normalize_rhs_tensor (linsolve.rs:972-984): a rank-1 rhs of the right length is a column
    std::vector<size_t> bs = normalize_matrix_shape(bb.shape);
    if (bs[0] != as[0]) {
        if (bb.shape.size() == 1 && bb.shape[0] == as[0]) bs = {as[0], 1};
        else return fail(RMHIP_ERR_SHAPE, "linsolve: Matrix dimensions must agree.");
    }
    const size_t n = as[0], nrhs = bs[1];
    const bool triangular = lower || upper;
    if (triangular && as[0] != as[1]) return fail(RMHIP_ERR_SHAPE, "linsolve: triangular solves need a square matrix");
    if (serve_rcond && triangular)
        return fail(RMHIP_ERR_UNSUPPORTED, "linsolve_rcond: the lower / upper hints are served by rmhip_linsolve");
    if (serve_rcond && !opts->need_rcond && !opts->has_rcond)
        return fail(RMHIP_ERR_UNSUPPORTED, "linsolve_rcond: no rcond asked for; rmhip_linsolve serves the plain solve");
    if (!serve_rcond && !triangular && (opts->need_rcond || opts->has_rcond))
        return fail(RMHIP_ERR_UNSUPPORTED, "linsolve: rcond of a general matrix needs its singular values (CPU path)");
    double rcond = std::numeric_limits<double>::quiet_NaN();  // stays NaN for a general matrix unless serve_rcond, whichever solver answered
    if (serve_rcond) {
        if (as[0] == 0 || as[1] == 0 || nrhs == 0) return fail(RMHIP_ERR_UNSUPPORTED, "linsolve: empty system");
        // linsolve.rs:933-944, 1000-1009: sigma_min / sigma_max of the (transposed) matrix, and the caller's threshold before any solve.
        // Non-finite data and min(rows, cols) > svd_max_cols() are refused by the decomposition (RMHIP_ERR_UNSUPPORTED).
        std::vector<double> sv;
        RMHIP_TRY(svd_values_host(c, "linsolve", A, as[0], as[1], &sv));
        rcond = svd_rcond(sv);
        if (opts->has_rcond && rcond < opts->rcond) return fail(RMHIP_ERR_SINGULAR, "linsolve: matrix is singular to working precision.");
    }
    rmhip_buf oid = 0;
    int rc = RMHIP_OK;
    if (as[0] != as[1]) {  // rectangular: least squares / minimum norm as rmhip_mldivide (linsolve.rs:933-970 is the SVD solve)
        rc = solve_rectangular(ctx, c, true, A, as[0], as[1], bb.data(), nrhs, &oid);
    } else if (n == 0) {
        return fail(RMHIP_ERR_UNSUPPORTED, "linsolve: empty system");
    } else if (triangular) {
        double mn = 0.0, mx = 0.0;
        size_t zeros = 0;
        RMHIP_TRY(diag_stats_device(c, A, n, n, &mn, &mx, &zeros));
        if (zeros) return fail(RMHIP_ERR_SINGULAR, "linsolve: matrix is singular to working precision.");
        rcond = mx == 0.0 ? 0.0 : mn / mx;
        if (opts->has_rcond && rcond < opts->rcond)
            return fail(RMHIP_ERR_SINGULAR, "linsolve: matrix is singular to working precision.");
        Buffer ob;
        const size_t oshape[2] = {n, nrhs};
        RMHIP_TRY(c->new_buffer(oshape, 2, &oid, &ob));
        hipError_t e = hipMemcpyAsync(ob.data(), bb.data(), sizeof(double) * n * nrhs, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = fail(RMHIP_ERR_HIP, "linsolve: %s", hipGetErrorString(e));
        if (!rc)
            rc = lower ? trsm_lower_nonunit_device(c, A, n, n, ob.data(), n, nrhs) : trsm_upper_device(c, A, n, n, ob.data(), n, nrhs);
    } else {  // the same solvers and therefore the same bits as mldivide's; no pivot-ratio proxy
        const SolvePolicy policy{"linsolve", "use the CPU SVD path", false, true};
        rc = solve_square_general(ctx, c, policy, A, n, bb.data(), nrhs, &oid);
    }
    if (at) (void)hipStreamSynchronize(c->stream);  // the transposed copy is released on return
    if (rc) {
        if (oid) rmhip_free(ctx, oid);
        return rc;
    }
    *out = oid;
    if (reciprocal_condition) *reciprocal_condition = rcond;
    return RMHIP_OK;
}

int rmhip_linsolve(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, const rmhip_linsolve_options_t* opts, rmhip_buf* out,
                   double* reciprocal_condition) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.linsolve_count, &c->tel.linsolve_ns);
    return count_fallback(c, linsolve_impl(ctx, c, a, b, opts, out, reciprocal_condition, false), "linsolve:unsupported", "linsolve:singular");
}

int rmhip_linsolve_rcond(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, const rmhip_linsolve_options_t* opts, rmhip_buf* out,
                         double* reciprocal_condition) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.linsolve_count, &c->tel.linsolve_ns);
    return count_fallback(c, linsolve_impl(ctx, c, a, b, opts, out, reciprocal_condition, true), "linsolve:unsupported", "linsolve:singular");
}

// ---- block-level building blocks (views) ----------------------------------------------------------
namespace {
struct ViewPtr {
    Buffer buf;
    double* ptr = nullptr;
    size_t ld = 0, rows = 0, cols = 0;
};
// write: the block is updated in place - lazy views of the same storage held under other handles are materialised first
int resolve_view(Context* c, const rmhip_view_t* v, ViewPtr* out, bool write = false) {
    if (!v) return fail(RMHIP_ERR_INVALID, "null view");
    RMHIP_TRY(c->get_raw(v->buf, &out->buf));
    if (write) RMHIP_TRY(c->detach_views_of(v->buf));
    if (out->buf.dtype != DT_F64)  // in-place block updates cannot go through a widened temporary
        return fail(RMHIP_ERR_UNSUPPORTED, "block views address f64 storage; this buffer is f32 (precision-32 provider)");
    RMHIP_TRY(c->get(v->buf, &out->buf));
    const std::vector<size_t> s = normalize_matrix_shape(out->buf.shape);
    if (s.size() != 2) return fail(RMHIP_ERR_UNSUPPORTED, "view: only 2D buffers");
    if (v->row_off + v->rows > s[0] || v->col_off + v->cols > s[1])
        return fail(RMHIP_ERR_SHAPE, "view [%zu+%zu, %zu+%zu] exceeds buffer %zux%zu", v->row_off, v->rows, v->col_off, v->cols, s[0], s[1]);
    out->ld = s[0];
    out->rows = v->rows;
    out->cols = v->cols;
    out->ptr = out->buf.data() + v->row_off + v->col_off * s[0];
    return RMHIP_OK;
}
}  // namespace

int rmhip_blk_copy(rmhip_ctx* ctx, const rmhip_view_t* src, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    ViewPtr v;
    RMHIP_TRY(resolve_view(c, src, &v));
    Buffer ob;
    const size_t oshape[2] = {v.rows, v.cols};
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    if (v.rows && v.cols)
        RMHIP_HIP_CHECK(hipMemcpy2DAsync(ob.data(), v.rows * sizeof(double), v.ptr, v.ld * sizeof(double), v.rows * sizeof(double),
                                         v.cols, hipMemcpyDeviceToDevice, c->stream));
    return RMHIP_OK;
}

int rmhip_blk_assign(rmhip_ctx* ctx, const rmhip_view_t* dst, rmhip_buf src) {
    CTX_OR_FAIL(ctx);
    ViewPtr v;
    RMHIP_TRY(resolve_view(c, dst, &v, true));
    Buffer sb;
    RMHIP_TRY(c->get(src, &sb));
    if (sb.numel != v.rows * v.cols) return fail(RMHIP_ERR_SHAPE, "blk_assign: source has %zu elements, view %zux%zu", sb.numel, v.rows, v.cols);
    if (v.rows && v.cols)
        RMHIP_HIP_CHECK(hipMemcpy2DAsync(v.ptr, v.ld * sizeof(double), sb.data(), v.rows * sizeof(double), v.rows * sizeof(double),
                                         v.cols, hipMemcpyDeviceToDevice, c->stream));
    return RMHIP_OK;
}

int rmhip_blk_gemm(rmhip_ctx* ctx, double alpha, const rmhip_view_t* a, const rmhip_view_t* b, double beta,
                   const rmhip_view_t* cv) {
    CTX_OR_FAIL(ctx);
    ViewPtr va, vb, vc;
    RMHIP_TRY(resolve_view(c, a, &va));
    RMHIP_TRY(resolve_view(c, b, &vb));
    RMHIP_TRY(resolve_view(c, cv, &vc, true));
    if (va.cols != vb.rows || vc.rows != va.rows || vc.cols != vb.cols)
        return fail(RMHIP_ERR_SHAPE, "blk_gemm: %zux%zu * %zux%zu -> %zux%zu", va.rows, va.cols, vb.rows, vb.cols, vc.rows, vc.cols);
    if (va.cols == 0) return RMHIP_OK;
    return launch_dgemm(c, va.rows, vb.cols, va.cols, alpha, va.ptr, va.ld, vb.ptr, vb.ld, beta, vc.ptr, vc.ld);
}

int rmhip_blk_trsm(rmhip_ctx* ctx, int upper, const rmhip_view_t* t, const rmhip_view_t* b) {
    CTX_OR_FAIL(ctx);
    ViewPtr vt, vb;
    RMHIP_TRY(resolve_view(c, t, &vt));
    RMHIP_TRY(resolve_view(c, b, &vb, true));
    if (upper == 2) {
        // B <- B U^-1 (the multipliers of a row block against a factored diagonal tile: L21 = A21 U11^-1).  X U = B is U' X' = B': both
        // operands are transposed into temporaries (k_transpose, 64 x 64 LDS tiles), U' is lower with a stored diagonal - the
        // kernels of `linsolve`'s LT hint - and the solution is transposed back in place.  O(rows w) extra traffic around O(rows w^2) work.
        if (vt.rows != vt.cols || vb.cols != vt.rows)
            return fail(RMHIP_ERR_SHAPE, "blk_trsm (right): triangle %zux%zu vs block %zux%zu", vt.rows, vt.cols, vb.rows, vb.cols);
        const size_t w = vt.rows, m = vb.rows;
        if (w == 0 || m == 0) return RMHIP_OK;
        std::shared_ptr<Allocation> tt, bt;
        RMHIP_TRY(c->alloc_device(w * w, &tt));
        RMHIP_TRY(c->alloc_device(w * m, &bt));
        RMHIP_TRY(transpose_device(c, vt.ptr, vt.ld, w, w, tt->ptr, w));
        RMHIP_TRY(transpose_device(c, vb.ptr, vb.ld, m, w, bt->ptr, w));
        RMHIP_TRY(trsm_lower_nonunit_device(c, tt->ptr, w, w, bt->ptr, w, m));
        RMHIP_TRY(transpose_device(c, bt->ptr, w, w, m, vb.ptr, vb.ld));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the temporaries go back to the pool on return
        return RMHIP_OK;
    }
    if (vt.rows != vt.cols || vb.rows != vt.rows) return fail(RMHIP_ERR_SHAPE, "blk_trsm: triangle %zux%zu vs rhs %zux%zu", vt.rows, vt.cols, vb.rows, vb.cols);
    return upper ? trsm_upper_device(c, vt.ptr, vt.ld, vt.rows, vb.ptr, vb.ld, vb.cols)
                 : trsm_lower_unit_device(c, vt.ptr, vt.ld, vt.rows, vb.ptr, vb.ld, vb.cols);
}

int rmhip_blk_lu(rmhip_ctx* ctx, const rmhip_view_t* a, rmhip_buf* ipiv_out, int* info) {
    CTX_OR_FAIL(ctx);
    if (!ipiv_out) return fail(RMHIP_ERR_INVALID, "null ipiv_out");
    ViewPtr va;
    RMHIP_TRY(resolve_view(c, a, &va, true));
    // the interchange vector is written on the device by the factorisation itself (round 6: it used to travel device -> host -> device
    // with a stream drain at each end, and rmhip_blk_swap_rows fetched it back again)
    const size_t kmin = va.rows < va.cols ? va.rows : va.cols;
    const size_t oshape[2] = {kmin, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(oshape, 2, ipiv_out, &ob));
    int inf = 0;
    int frc = RMHIP_LU_GROWTH;
    if (c->blk_lu_solve_path && va.rows > 0 && va.cols > 0) {
        // the solve path's kernels (k_rp_top / k_rp_below_mfma / matrix-core solves): the block is saved first - a multiplier beyond
        // the bound clobbers it - and restored for the grid-wide rule
        std::shared_ptr<Allocation> keep;
        frc = c->alloc_device(va.rows * va.cols, &keep);
        if (frc == RMHIP_OK) {
            hipError_t e = hipMemcpy2DAsync(keep->ptr, va.rows * sizeof(double), va.ptr, va.ld * sizeof(double), va.rows * sizeof(double), va.cols,
                                            hipMemcpyDeviceToDevice, c->stream);
            frc = e == hipSuccess ? lu_factor_device(c, va.ptr, va.rows, va.cols, va.ld, nullptr, &inf, nullptr, 1, ob.data())
                                  : fail(RMHIP_ERR_HIP, "blk_lu: saving the block: %s", hipGetErrorString(e));
            if (frc == RMHIP_LU_GROWTH || frc == RMHIP_LU_RETRY) {
                e = hipMemcpy2DAsync(va.ptr, va.ld * sizeof(double), keep->ptr, va.rows * sizeof(double), va.rows * sizeof(double), va.cols,
                                     hipMemcpyDeviceToDevice, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                frc = e == hipSuccess ? RMHIP_LU_GROWTH : fail(RMHIP_ERR_HIP, "blk_lu: restoring the block: %s", hipGetErrorString(e));
            }
        }
    }
    if (frc == RMHIP_LU_GROWTH) frc = lu_factor_device(c, va.ptr, va.rows, va.cols, va.ld, nullptr, &inf, nullptr, 0, ob.data());
    if (frc == RMHIP_LU_RETRY)  // in place: the block is clobbered and there is no copy to restart from
        frc = fail(RMHIP_ERR_HIP, "blk_lu: panel workgroups were not co-resident (device shared?); the block is invalid");
    if (frc != RMHIP_OK) {
        rmhip_free(ctx, *ipiv_out);  // do not leak the interchange vector on the error paths
        *ipiv_out = 0;
        return frc;
    }
    if (info) *info = inf;
    return RMHIP_OK;
}

int rmhip_blk_lu_deferred(rmhip_ctx* ctx, const rmhip_view_t* a, rmhip_buf guard, rmhip_buf* ipiv_out) {
    CTX_OR_FAIL(ctx);
    if (!ipiv_out) return fail(RMHIP_ERR_INVALID, "null ipiv_out");
    ViewPtr va;
    RMHIP_TRY(resolve_view(c, a, &va, true));
    Buffer gb;
    RMHIP_TRY(c->get(guard, &gb));
    if (gb.numel != 1 || gb.dtype != DT_F64) return fail(RMHIP_ERR_INVALID, "blk_lu_deferred: the guard is a 1 x 1 f64 tensor");
    const size_t kmin = va.rows < va.cols ? va.rows : va.cols;
    if (kmin == 0) return fail(RMHIP_ERR_INVALID, "blk_lu_deferred: empty view");
    const size_t oshape[2] = {kmin, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(oshape, 2, ipiv_out, &ob));
    int inf = 0;
    // solve-path panel kernels, no saved copy, no host read: the status lands in *guard (lu.hip, deferred form)
    int frc = lu_factor_device(c, va.ptr, va.rows, va.cols, va.ld, nullptr, &inf, nullptr, 1, ob.data(), gb.data());
    if (frc == RMHIP_LU_GROWTH || frc == RMHIP_LU_RETRY)  // (only when the deferred form was not taken: the ordinary checks ran and refused)
        frc = fail(RMHIP_ERR_GROWTH, "blk_lu_deferred: the panel was refused (multiplier bound or panel placement); the block is invalid");
    if (frc != RMHIP_OK) {
        rmhip_free(ctx, *ipiv_out);
        *ipiv_out = 0;
    }
    return frc;
}

int rmhip_blk_swap_rows(rmhip_ctx* ctx, const rmhip_view_t* a, rmhip_buf ipiv) {
    CTX_OR_FAIL(ctx);
    ViewPtr va;
    RMHIP_TRY(resolve_view(c, a, &va, true));
    Buffer pb;
    RMHIP_TRY(c->get(ipiv, &pb));
    // composed and applied on the device (no stream drain, no hipMalloc / hipFree); RMHIP_BLK_SWAP_DEVICE=0 or a view too tall for
    // the LDS map: the host composition, which also REPORTS an out-of-range target (the device form skips it)
    static const bool dev_path = !(std::getenv("RMHIP_BLK_SWAP_DEVICE") && std::getenv("RMHIP_BLK_SWAP_DEVICE")[0] == '0');
    if (dev_path) {
        const int rc = lu_swap_rows_from_device(c, va.ptr, va.ld, va.rows, va.cols, pb.data(), pb.numel);
        if (rc != RMHIP_ERR_UNSUPPORTED) return rc;
    }
    std::vector<double> host(pb.numel);
    if (pb.numel) {
        RMHIP_HIP_CHECK(hipMemcpyAsync(host.data(), pb.data(), pb.numel * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    std::vector<int> piv(host.size());
    for (size_t k = 0; k < host.size(); ++k) {
        if (!(host[k] >= 0.0) || host[k] >= (double)va.rows) return fail(RMHIP_ERR_INVALID, "swap_rows: pivot %zu out of range", k);
        piv[k] = (int)host[k];
    }
    return lu_swap_rows_device(c, va.ptr, va.ld, va.cols, piv);
}

}  // extern "C"
