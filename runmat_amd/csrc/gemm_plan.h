// gemm_plan.h -- which kernel a dense product runs, as a pure host function.  launch_dgemm_impl (dgemm.hip) and launch_sgemm_trans
// (sgemm.hip) fill a GemmProblem and a GemmSite, call plan_dgemm / plan_sgemm and execute the GemmRoute they get: the route is the
// decision, the launch follows it, and rmhip_gemm_last_route reports it.  No HIP header and no Context: tests/cpp/gemm_route_check.cpp
// compiles this file with a plain host compiler and checks the rules (the tables of tests/gemm_ref.py and a sweep whose expected
// digests, tests/golden/gemm_routes.txt, were taken from the launchers' former if-ladders).  A plan consumes nothing: the tile counter
// of the persistent kernel is taken by the launcher, and only when the route says w8p.  plan_cgemm (at the end) says how a product with
// a complex-interleaved operand is embedded in one real product; tests/cpp/cgemm_route_check.cpp checks it the same way.
#pragma once
#include <cstddef>

namespace rmhip {

// What a GEMM launcher call ran.  `kernel` is a literal.  rmhip_gemm_last_route reports the fields up to k_chunk.
struct GemmRoute {
    const char* kernel = "";  // small, w8, w8g, w8p, w4, pgemm, s_w8, s_w8g, s_w4
    int guard = 0;            // GUARD (small, w8g, pgemm, s_w8g) / EDGE (w4, s_w4): the form that checks its bounds
    int pre = 0, ta = 0, tb = 0, epi = 0, yield = 0;
    unsigned splits = 0, k_chunk = 0;  // splits == 0: no product yet
    // what the launcher needs beside them
    unsigned tiles_m = 0, tiles_n = 0;  // the kernel's tile grid (64 x 64 tiles for `small`, 128 x 128 otherwise)
    int prio = 0;                       // GemmArgs::prio
    const char* unsupported = nullptr;  // set: no kernel serves the request, and this is the message
};

// The process-wide switches (gemm_knobs() in dgemm.hip reads them; docs/KNOBS.md "GEMM dispatch").  All on by default, "0" turns one off.
struct GemmKnobs {
    bool small = true;     // RMHIP_GEMM_SMALL: the 64 x 64 tiles
    bool w8 = true;        // RMHIP_GEMM_W8: the eight-wave f64 kernels (plain, guarded, persistent)
    bool preload = true;   // RMHIP_GEMM_PRELOAD: C <- C - A B with C loaded into the accumulators first
    bool guard = true;     // RMHIP_GEMM_GUARD: ragged shapes on the guarded tiles instead of the element-checking four-wave kernel
    bool sgemm_w8 = true;  // RMHIP_SGEMM_W8: the eight-wave f32 kernels
    int rowmap = 0;        // RMHIP_MFMA_ROWMAP: bring-up selector of the accumulator row formula (GemmArgs::rowmap)
};

// Where the call is made: the context's state that bears on the choice.
struct GemmSite {
    int num_cus = 256;
    bool in_lookahead = false;  // inside the LU's look-ahead driver
    bool lds_pad = false;       // the stream's blocks carry an LDS pad (one per CU): an update stream
    bool chain_prio = false;    // the two-level LU's main-stream launches raise their wave priority
    bool counter = false;       // a tile counter is left for the persistent kernel
    bool yield_word = false;    // the two-level LU named a word its update blocks watch
    long small_upd = 0;         // LuProcessKnobs::small_upd
};

struct GemmProblem {
    size_t m = 0, n = 0, k = 0, lda = 0, ldb = 0;
    bool a_aligned = true, b_aligned = true;  // the base allows the kernel's vector loads (16 bytes in f64, 8 in f32)
    bool ta = false, tb = false;
    int epi = 0;  // 0 none, 1 epilogue, 2 epilogue with EP_POW (f64 only)
    double alpha = 1.0, beta = 0.0;  // f64 only
};

namespace gemm_plan {
constexpr size_t kTile = 128, kSmallTile = 64, kTileK = 16;
constexpr unsigned kSmallUpdBlocks = 128;  // upd_small: at most this many 128 x 128 tiles
inline unsigned tiles(size_t x, size_t t) { return (unsigned)((x + t - 1) / t); }
}  // namespace gemm_plan

// Split-K: few output tiles but a long k (A'*A of a tall matrix, dot-product-like shapes) would leave most CUs idle; give every CU
// about two blocks.  A block walks its k range at about 1 us per 16 columns - one memory latency per tile with nothing else resident -
// so few blocks with a long k are latency bound whatever the tile: 4096 x 100 with k = 4096 (32 tiles) 547 -> 97 us, 32 x 512 with
// k = 8192 on one slice 1100 us.  Chunks are multiples of 128, so every slice but the last is a whole number of k tiles.
struct SplitK {
    unsigned splits;
    size_t k_chunk;
};
inline SplitK plan_split_k(size_t k, unsigned blocks, int num_cus, size_t min_k) {
    if (blocks * 4 > (unsigned)num_cus || k < min_k) return {1, k};
    const size_t want = (2 * (size_t)num_cus + blocks - 1) / blocks;
    const size_t gran = k >= 8192 ? 1024 : (k >= 2048 ? 256 : 128);
    const size_t chunk = ((k + want - 1) / want + gran - 1) / gran * gran;
    const unsigned splits = (unsigned)((k + chunk - 1) / chunk);
    return splits > 1 ? SplitK{splits, chunk} : SplitK{1, k};
}

// f64: C = alpha * op(A) * op(B) + beta * C, or the epilogue form.
inline GemmRoute plan_dgemm(const GemmProblem& p, const GemmSite& s, const GemmKnobs& kn) {
    using namespace gemm_plan;
    GemmRoute r;
    const bool ep = p.epi != 0, ta = p.ta, tb = p.tb, plain = !ep && !ta && !tb;
    if (ta && tb) return r.unsupported = "dgemm: A' * B' is not instantiated", r;
    if (ep && (ta || tb)) return r.unsupported = "dgemm: epilogue with transposed operands is not instantiated", r;
    const size_t m = p.m, n = p.n, k = p.k;
    r.tiles_m = tiles(m, kTile);
    r.tiles_n = tiles(n, kTile);
    const unsigned blocks = r.tiles_m * r.tiles_n;
    r.ta = ta, r.tb = tb, r.epi = p.epi;
    // the streams of the look-ahead LU: the main stream's blocks must fit beside the update streams' (no eight-wave blocks, and a
    // raised wave priority in the two-level driver); an update stream's blocks must stay too big to share a CU with a panel block
    const bool main_stream = s.in_lookahead && !s.lds_pad, abi = !s.in_lookahead && !s.lds_pad;
    r.prio = main_stream && s.chain_prio;
    const bool vec_ok = p.lda % 2 == 0 && p.ldb % 2 == 0 && p.a_aligned && p.b_aligned;
    const bool fast = m % kTile == 0 && n % kTile == 0 && k % kTileK == 0 && k > 0 && vec_ok;
    const SplitK sk = ep ? SplitK{1, k} : plan_split_k(k, blocks, s.num_cus, s.in_lookahead ? 8192 : 1024);
    r.splits = sk.splits;
    r.k_chunk = (unsigned)sk.k_chunk;
    const bool unsplit = sk.splits == 1;
    const bool fast_k = fast && (unsplit || k % sk.k_chunk == 0);  // the unguarded four-wave kernel: the last slice whole as well
    // C <- C - A*B (the LU's updates): C preloaded into the accumulators
    const bool preload = kn.preload && plain && unsplit && p.alpha == -1.0 && p.beta == 1.0 && k > 0;
    // shapes that are not whole tiles - any m, n, k, leading dimensions, 8-byte aligned bases - run the same kernels with clamped
    // operand loads, a zeroed k tail and checked stores (GUARD); A * B' and a disabled guard go to the element-checking k_dgemm
    const bool guard_ok = kn.guard && !tb && k >= 1;

    // 64 x 64 tiles: the big tiles would cover at most half of the CUs and k is short; skinny products - at most 64 rows or columns
    // of output - waste half of every 128 x 128 tile or more (100000 x 50 x 50 52 -> 30 us, 200000 x 16 x 16 34 -> 20 us; a longer
    // k splits instead).  The look-ahead LU's update streams run their few-tile products - the dgemm steps of the W-wide triangular
    // solves, 14-112 tiles of 128 x 128 for 0.1-0.2 ms each - on them as well: four times the blocks, 16384 69.1 -> 67.6 ms,
    // 8192 20.6 -> 20.2 (RMHIP_LU_SMALL_UPD = largest k, 0 = off).
    const bool skinny = (m <= kSmallTile || n <= kSmallTile) && k < 1024 && !s.in_lookahead;
    const bool upd_small = s.small_upd > 0 && s.lds_pad && s.in_lookahead && (long)k <= s.small_upd && blocks <= kSmallUpdBlocks;
    const bool small_shape = plain && unsplit && k > 0 && (!s.lds_pad || upd_small) &&
                             ((k <= 1024 && (size_t)blocks * 2 <= (size_t)s.num_cus) || skinny || upd_small);
    const bool small_whole = m % kSmallTile == 0 && n % kSmallTile == 0 && k % kTileK == 0 && vec_ok;
    if (kn.small && small_shape && (small_whole || guard_ok)) {
        r.kernel = "small";
        r.guard = !small_whole;
        r.pre = preload;
        r.tiles_m = tiles(m, kSmallTile);
        r.tiles_n = tiles(n, kSmallTile);
        return r;
    }
    // update stream of the look-ahead LU while the panels sit on one XCD: the persistent eight-wave kernel that stays off it
    if (kn.w8 && fast && plain && unsplit && s.lds_pad && s.counter) return r.kernel = "w8p", r;
    // eight-wave tile (scripts/gemm_w8_ab.py, TFLOP/s four-wave -> eight-wave, both with the pipelined k loop: 4096^3 68.6 -> 71.9,
    // 8192^3 69.5 -> 72.3, 4096^2 x 16384 68.8 -> 72.5, 8192^2 x 1024 68.4 -> 70.7, 12288 x 4096 x 2048 68.5 -> 71.4; equal at
    // 2048^3 and at 16384^2 x 128 / 256: four pipelined waves per SIMD leave the matrix pipe fewer gaps than two) - but not on the
    // main stream inside the look-ahead LU.  A plain unsplit product runs it on the update streams too; the epilogue, A' * B
    // (70.7 -> 72.5 at 8192^3; A * B' measured 69.8 against 70.2 and stays on k_dgemm) and split-K only outside the LU.
    const bool w8_ok = kn.w8 && !tb && !main_stream;
    if (w8_ok && fast && ((plain && unsplit) || abi)) {
        r.kernel = "w8";
        r.pre = preload;
        r.yield = preload && s.lds_pad && s.yield_word;  // the two-level LU's update streams: the variant that checks the yield word
        return r;
    }
    if (w8_ok && !fast && guard_ok) {  // its guarded form: plain or transposed A; plain, preloaded-C or epilogue store; split-K
        r.kernel = "w8g";
        r.guard = 1;
        r.pre = preload;
        return r;
    }
    r.kernel = "w4";
    r.guard = ep || !fast_k;
    r.pre = fast_k && preload;
    return r;
}

// f32: C = op(A) * op(B).  The site matters through its compute-unit count only.
inline GemmRoute plan_sgemm(const GemmProblem& p, const GemmSite& s, const GemmKnobs& kn) {
    using namespace gemm_plan;
    GemmRoute r;
    if (p.ta && p.tb) return r.unsupported = "sgemm: A' * B' is not instantiated", r;
    const size_t m = p.m, n = p.n, k = p.k;
    r.tiles_m = tiles(m, kTile);
    r.tiles_n = tiles(n, kTile);
    r.ta = p.ta, r.tb = p.tb;
    const bool vec_ok = p.lda % 2 == 0 && p.ldb % 2 == 0 && p.a_aligned && p.b_aligned;
    const bool fast = m % kTile == 0 && n % kTile == 0 && k % kTileK == 0 && k > 0 && vec_ok;
    const SplitK sk = plan_split_k(k, r.tiles_m * r.tiles_n, s.num_cus, 1024);
    r.splits = sk.splits;
    r.k_chunk = (unsigned)sk.k_chunk;
    const bool fast_k = fast && (sk.splits == 1 || k % sk.k_chunk == 0);
    // eight-wave tiles for unsplit A * B and A' * B (syrk, covariance, transpose views), guarded when the shape is not whole tiles
    if (kn.sgemm_w8 && !p.tb && sk.splits == 1 && (fast || (kn.guard && k >= 1))) {
        r.kernel = fast ? "s_w8" : "s_w8g";
        r.guard = !fast;
        return r;
    }
    r.kernel = "s_w4";
    r.guard = !fast_k;
    return r;
}

// A product with a complex-interleaved operand (rmhip_complex_matmul, rmhip_ops.cpp; kernels cgemm.hip): kind 0 complex x complex,
// 1 complex x real, 2 real x complex, as in complex_pagefun.hip.  An interleaved column-major A (m x k) is, read as doubles, the real
// matrix A~ (2m x k, ld 2m) whose even rows are A_re and odd rows A_im, so every kind is ONE real product through launch_dgemm, which
// plan_dgemm routes like any other:
//   kind 1  A~ (2m x k) * B (k x n)                      is the interleaved result itself
//   kind 2  T (m x 2n)  = A * [B_re | B_im]              join: C(i, j) = (T[i, j], T[i, n + j])
//   kind 0  T (2m x 2n) = A~ * [B_re | B_im]             join: re = T[2i, j] - T[2i+1, n+j], im = T[2i, n+j] + T[2i+1, j]
// `split_b`: B is first split into the planes [B_re | B_im] (k x 2n, ld k).  `join`: the product goes to T and a streaming pass forms
// the result - kinds 0 and 2 always, kind 1 only in a precision-32 context, whose rounding is that pass.  `workspace` counts doubles:
// 2kn for the planes (laid first) plus MN for T, so beyond the 2mn doubles of the result a call holds at most 2kn + 4mn doubles.
// Products of at most kPageSmall on every side take the bit-exact small tier of complex pagefun as one page (`small`, nothing embedded).
// The caller answers m == 0, n == 0 and k == 0 before it plans.
namespace gemm_plan {
constexpr size_t kPageSmall = 32;
}
struct CgemmPlan {
    const char* route = "";  // small, embed
    size_t M = 0, N = 0, K = 0, lda = 0, ldb = 0;  // the embedded real product (ldc = M)
    bool split_b = false, join = false;
    size_t workspace = 0;
    const char* unsupported = nullptr;  // set: an embedded extent does not fit the launcher's 32-bit sides
};
inline CgemmPlan plan_cgemm(int kind, size_t m, size_t n, size_t k, bool r32) {
    CgemmPlan p;
    if (m <= gemm_plan::kPageSmall && n <= gemm_plan::kPageSmall && k <= gemm_plan::kPageSmall) return p.route = "small", p;
    p.route = "embed";
    p.M = kind == 2 ? m : 2 * m;
    p.N = kind == 1 ? n : 2 * n;
    p.K = k;
    p.lda = p.M;
    p.ldb = k;
    p.split_b = kind != 1;
    p.join = kind != 1 || r32;
    p.workspace = (p.split_b ? 2 * k * n : 0) + (p.join ? p.M * p.N : 0);
    if (p.M > 0xffffffffULL || p.N > 0xffffffffULL || p.K > 0xffffffffULL) p.unsupported = "complex_matmul: an embedded extent exceeds 2^32";
    return p;
}

}  // namespace rmhip
