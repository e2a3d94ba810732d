// csolve_plan.h -- how a dense solve with a complex-interleaved operand is served by ONE real solve (host-only, no HIP; the entry
// points rmhip_complex_mldivide / _mrdivide / _inv in solve.cpp execute what plan_csolve decides, tests/cpp/csolve_plan_check.cpp prints
// it).  A complex system is a real system of twice the order,
//     A x = b   <=>   [Ar -Ai; Ai Ar] [xr; xi] = [br; bi],
// and A -> E(A) preserves products, adjoints, inverses, pseudo-inverses, least-squares and minimum-norm solutions; the singular values of
// E(A) are A's, each twice.  So every decision of the real dispatch (pivot cut-off, growth guard, ratio proxy, Gram guard, SVD fallback)
// answers the complex system.  (m, n, nrhs) are the COMPLEX extents of the system the solve sees: for mrdivide those of A.' X.' = B.', for
// inv nrhs == n and the right-hand side is [I; 0].
//     kind 0  A complex, b complex   E(A) \ [Br; Bi]    2m x 2n, 2m x nrhs
//     kind 1  A complex, b real      E(A) \ [Br; 0]     the same
//     kind 2  A real,    b complex   A \ [Br | Bi]      m x n, m x 2 nrhs: no embedding, half the memory and a quarter of the
//                                                       factorisation flops of kind 0
#pragma once
#include <cstddef>

namespace rmhip {

enum : int { CSOLVE_MLDIVIDE = 0, CSOLVE_MRDIVIDE = 1, CSOLVE_INV = 2 };

struct CsolvePlan {
    size_t M = 0, N = 0, NRHS = 0;  // the real system handed to the cores of solve.cpp
    bool embed_a = false;           // A goes through k_csolve_embed (kinds 0 and 1); kind 2 solves on A as it is
    bool transpose_a = false;       // mrdivide: E(A.') is written by the embed kernel; a real A (kind 2) is transposed into a temporary
    size_t tol_dim = 0;             // the SVD path's rank tolerance counts with the complex max(m, n), not the embedded one
    size_t a_workspace = 0;         // doubles of E(A) (4mn), or of mrdivide's transposed real A (mn), at the start of the workspace
    size_t workspace = 0;           // doubles beyond what the real solve of (M, N, NRHS) takes itself: a_workspace and the stacked right-hand side
                                    // (2m nrhs) - the bound include/rmhip.h states: 4mn + 2m nrhs (kinds 0, 1), 2m nrhs (kind 2; + mn for mrdivide)
    size_t result = 0;              // the real solution before the join: 2n nrhs doubles
    const char* unsupported = nullptr;  // set: the real solve cannot take the embedded system, and this is the message
};

inline CsolvePlan plan_csolve(int entry, int kind, size_t m, size_t n, size_t nrhs) {
    CsolvePlan p;
    p.embed_a = kind != 2;
    p.transpose_a = entry == CSOLVE_MRDIVIDE;
    p.M = p.embed_a ? 2 * m : m;
    p.N = p.embed_a ? 2 * n : n;
    p.NRHS = p.embed_a ? nrhs : 2 * nrhs;
    p.tol_dim = m > n ? m : n;
    // the limits of the real solve: lu_plan.h refuses a dimension beyond 2^31 - 1, lu_solve_device more than 65535 right-hand sides
    if (m > 0x7fffffffULL || n > 0x7fffffffULL || p.M > 0x7fffffffULL || p.N > 0x7fffffffULL) return p.unsupported = "lu: dimension exceeds 2^31", p;
    if (nrhs > 65535 || p.NRHS > 65535) return p.unsupported = "mldivide: more than 65535 right-hand sides", p;
    p.a_workspace = p.embed_a ? 4 * m * n : (p.transpose_a ? m * n : 0);
    p.workspace = p.a_workspace + 2 * m * nrhs;
    p.result = 2 * n * nrhs;
    return p;
}

}  // namespace rmhip
