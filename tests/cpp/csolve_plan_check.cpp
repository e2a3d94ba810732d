// Host-logic check of how a dense solve with a complex-interleaved operand is embedded in one real solve (runmat_amd/csrc/csolve_plan.h
// plan_csolve), the function rmhip_complex_mldivide / _mrdivide / _inv execute.  Reads one case per line from stdin,
//     entry kind m n nrhs          (entry 0 mldivide, 1 mrdivide, 2 inv; the extents are the complex ones of the system solved)
// and prints per case
//     M N NRHS embed_a transpose_a tol_dim a_workspace workspace result
// or "unsupported: <message>".  tests/test_complex_solve_host.py compares with tests/complex_solve_ref.py expected_plan.  No GPU needed.
#include <cstdio>

#include "csolve_plan.h"

using namespace rmhip;

int main() {
    char text[256];
    while (std::fgets(text, sizeof text, stdin)) {
        int entry, kind;
        unsigned long long m, n, nrhs;
        if (std::sscanf(text, "%d %d %llu %llu %llu", &entry, &kind, &m, &n, &nrhs) != 5 || entry < 0 || entry > 2 || kind < 0 || kind > 2) {
            std::fprintf(stderr, "bad case line: %s", text);
            return 2;
        }
        const CsolvePlan p = plan_csolve(entry, kind, m, n, nrhs);
        if (p.unsupported) {
            std::printf("unsupported: %s\n", p.unsupported);
            continue;
        }
        std::printf("%zu %zu %zu %d %d %zu %zu %zu %zu\n", p.M, p.N, p.NRHS, (int)p.embed_a, (int)p.transpose_a, p.tol_dim, p.a_workspace, p.workspace,
                    p.result);
    }
    return 0;
}
