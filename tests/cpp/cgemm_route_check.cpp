// Host-logic check of how a product with a complex-interleaved operand is embedded in one real product (runmat_amd/csrc/gemm_plan.h
// plan_cgemm), the function rmhip_complex_matmul executes.  Reads one case per line from stdin,
//     kind m n k r32
// and prints per case the plan and, for an embedded product, the route plan_dgemm gives the real product the launcher is handed
// (alpha 1, beta 0, aligned bases, the entry point's own site, every knob on):
//     route M N K lda ldb split_b join workspace | kernel splits        (kernel "-" and splits 0 for the small route)
// or "unsupported: <message>".  tests/test_complex_matmul_host.py compares with tests/complex_matmul_ref.py expected_plan.  No GPU needed.
#include <cstdio>

#include "gemm_plan.h"

using namespace rmhip;

int main() {
    char text[256];
    while (std::fgets(text, sizeof text, stdin)) {
        int kind, r32;
        unsigned long long m, n, k;
        if (std::sscanf(text, "%d %llu %llu %llu %d", &kind, &m, &n, &k, &r32) != 5 || kind < 0 || kind > 2) {
            std::fprintf(stderr, "bad case line: %s", text);
            return 2;
        }
        const CgemmPlan p = plan_cgemm(kind, m, n, k, r32 != 0);
        if (p.unsupported) {
            std::printf("unsupported: %s\n", p.unsupported);
            continue;
        }
        const char* kernel = "-";
        unsigned splits = 0;
        if (p.M) {
            GemmProblem g;
            g.m = p.M, g.n = p.N, g.k = p.K, g.lda = p.lda, g.ldb = p.ldb;
            const GemmRoute r = plan_dgemm(g, GemmSite{}, GemmKnobs{});
            kernel = r.unsupported ? "unsupported" : r.kernel;
            splits = r.splits;
        }
        std::printf("%s %zu %zu %zu %zu %zu %d %d %zu | %s %u\n", p.route, p.M, p.N, p.K, p.lda, p.ldb, (int)p.split_b, (int)p.join, p.workspace,
                    kernel, splits);
    }
    return 0;
}
