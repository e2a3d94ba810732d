// Host-logic check of the GEMM dispatch (runmat_amd/csrc/gemm_plan.h plan_dgemm / plan_sgemm), the function the launchers execute.
//   --table   reads one case per line from stdin and prints the planned route, one per line (tests/test_gemm_ref_host.py feeds it the
//             tables of tests/gemm_ref.py and its own rows for the routes only the LU selects):
//               bits m n k lda ldb a_aligned b_aligned ta tb epi alpha beta
//               num_cus in_lookahead lds_pad chain_prio counter yield_word small_upd  small w8 preload guard sgemm_w8
//   --sweep   plans a fixed sweep of shapes, layouts, operations, sites, device sizes and knob settings and prints per group the number
//             of cases and the 64-bit FNV-1a digest of the routes' lines; tests/test_host_plan.py compares with
//             tests/golden/gemm_routes.txt, which was taken from the launchers' if-ladders before the plan was extracted from them.
//   --dump    the sweep with every route printed under its group's line.
// A route's line: kernel guard pre ta tb epi yield splits k_chunk tiles_m tiles_n prio, or "unsupported: <message>".  No GPU needed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "gemm_plan.h"

using namespace rmhip;

static std::string line_of(const GemmRoute& r) {
    if (r.unsupported) return std::string("unsupported: ") + r.unsupported + "\n";
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s %d %d %d %d %d %d %u %u %u %u %d\n", r.kernel, r.guard, r.pre, r.ta, r.tb, r.epi, r.yield, r.splits,
                  r.k_chunk, r.tiles_m, r.tiles_n, r.prio);
    return buf;
}

static int table_mode() {
    char text[512];
    while (std::fgets(text, sizeof text, stdin)) {
        int bits, aa, ba, ta, tb, la, pad, prio, counter, yield, small, w8, preload, guard, sgemm_w8;
        unsigned long long m, n, k, lda, ldb;
        GemmProblem p;
        GemmSite s;
        GemmKnobs kn;
        const int got = std::sscanf(text, "%d %llu %llu %llu %llu %llu %d %d %d %d %d %lf %lf %d %d %d %d %d %d %ld %d %d %d %d %d", &bits, &m, &n, &k,
                                    &lda, &ldb, &aa, &ba, &ta, &tb, &p.epi, &p.alpha, &p.beta, &s.num_cus, &la, &pad, &prio, &counter, &yield,
                                    &s.small_upd, &small, &w8, &preload, &guard, &sgemm_w8);
        if (got != 25 || (bits != 64 && bits != 32)) {
            std::fprintf(stderr, "bad case line (%d fields): %s", got, text);
            return 2;
        }
        p.m = m, p.n = n, p.k = k, p.lda = lda, p.ldb = ldb;
        p.a_aligned = aa, p.b_aligned = ba, p.ta = ta, p.tb = tb;
        s.in_lookahead = la, s.lds_pad = pad, s.chain_prio = prio, s.counter = counter, s.yield_word = yield;
        kn.small = small, kn.w8 = w8, kn.preload = preload, kn.guard = guard, kn.sgemm_w8 = sgemm_w8;
        std::fputs(line_of(bits == 64 ? plan_dgemm(p, s, kn) : plan_sgemm(p, s, kn)).c_str(), stdout);
    }
    return 0;
}

struct NamedSite {
    const char* name;
    GemmSite site;
};
struct NamedKnobs {
    const char* name;
    GemmKnobs knobs;
};

static GemmSite site(bool la, bool pad, bool prio, bool counter, bool yield, long small_upd) {
    GemmSite s;
    s.in_lookahead = la, s.lds_pad = pad, s.chain_prio = prio, s.counter = counter, s.yield_word = yield, s.small_upd = small_upd;
    return s;
}

static void sweep_group(int bits, const NamedSite& ns, const NamedKnobs& nk, int num_cus, bool dump) {
    static const size_t MN[] = {1, 63, 64, 65, 128, 129, 192, 1024, 2049, 4096, 16512};
    static const size_t KS[] = {0, 1, 15, 16, 17, 128, 1008, 1024, 1040, 2048, 2050, 8192, 16384};
    // operations: plain, A' * B, A * B', epilogue, epilogue with pow, the update C - A B, 2 A B - C (f32 has the first three)
    struct Op {
        bool ta, tb;
        int epi;
        double alpha, beta;
    };
    static const Op OPS[] = {{false, false, 0, 1.0, 0.0}, {true, false, 0, 1.0, 0.0},  {false, true, 0, 1.0, 0.0}, {false, false, 1, 1.0, 0.0},
                             {false, false, 2, 1.0, 0.0}, {false, false, 0, -1.0, 1.0}, {false, false, 0, 2.0, -1.0}};
    GemmSite s = ns.site;
    s.num_cus = num_cus;
    uint64_t h = 1469598103934665603ull;
    unsigned long count = 0;
    std::string all;
    for (size_t m : MN)
        for (size_t n : MN)
            for (size_t k : KS)
                for (int la = 0; la < 3; ++la)      // layout of A: aligned, odd base, odd leading dimension
                    for (int lb = 0; lb < 3; ++lb)  // and of B
                        for (int o = 0; o < (bits == 64 ? 7 : 3); ++o) {
                            const Op& op = OPS[o];
                            GemmProblem p;
                            p.m = m, p.n = n, p.k = k;
                            p.ta = op.ta, p.tb = op.tb, p.epi = op.epi, p.alpha = op.alpha, p.beta = op.beta;
                            const size_t rows_a = op.ta ? k : m, rows_b = op.tb ? n : k;  // the smallest leading dimension of that parity
                            p.lda = rows_a + ((rows_a % 2 == 0) == (la == 2) ? 1 : 0);
                            p.ldb = rows_b + ((rows_b % 2 == 0) == (lb == 2) ? 1 : 0);
                            p.a_aligned = la != 1;
                            p.b_aligned = lb != 1;
                            const std::string line = line_of(bits == 64 ? plan_dgemm(p, s, nk.knobs) : plan_sgemm(p, s, nk.knobs));
                            for (unsigned char ch : line) h = (h ^ ch) * 1099511628211ull;
                            ++count;
                            if (dump) {
                                char head[160];
                                std::snprintf(head, sizeof head, "  %zu %zu %zu A%d B%d op%d: ", m, n, k, la, lb, o);
                                all += head + line;
                            }
                        }
    std::printf("f%d %s %s cus=%d %lu %016llx\n", bits, ns.name, nk.name, num_cus, count, (unsigned long long)h);
    std::fputs(all.c_str(), stdout);
}

static int sweep_mode(bool dump) {
    // ABI; the look-ahead LU's main stream; its update streams; a padded stream outside the look-ahead (the row-partitioned solve's)
    const NamedSite sites[] = {
        {"abi", site(false, false, false, false, false, 1024)},
        {"main", site(true, false, false, false, false, 1024)},
        {"main+prio", site(true, false, true, false, false, 1024)},
        {"upd-su0", site(true, true, false, false, false, 0)},
        {"upd+ctr-su0", site(true, true, false, true, false, 0)},
        {"upd+yield-su0", site(true, true, false, false, true, 0)},
        {"upd+ctr+yield-su0", site(true, true, false, true, true, 0)},
        {"upd-su1024", site(true, true, false, false, false, 1024)},
        {"upd+ctr-su1024", site(true, true, false, true, false, 1024)},
        {"upd+yield-su1024", site(true, true, false, false, true, 1024)},
        {"upd+ctr+yield-su1024", site(true, true, false, true, true, 1024)},
        {"pad", site(false, true, false, false, false, 1024)},
        {"pad+yield", site(false, true, false, false, true, 1024)},
    };
    NamedKnobs knobs[] = {{"default", {}},          {"RMHIP_GEMM_SMALL=0", {}}, {"RMHIP_GEMM_W8=0", {}}, {"RMHIP_GEMM_PRELOAD=0", {}},
                          {"RMHIP_GEMM_GUARD=0", {}}, {"RMHIP_SGEMM_W8=0", {}}};
    knobs[1].knobs.small = false;
    knobs[2].knobs.w8 = false;
    knobs[3].knobs.preload = false;
    knobs[4].knobs.guard = false;
    knobs[5].knobs.sgemm_w8 = false;
    const int cus[] = {256, 64, 304};
    for (int bits : {64, 32}) {
        for (const NamedSite& ns : sites)
            for (int c : cus) sweep_group(bits, ns, knobs[0], c, dump);
        for (int i = 1; i < 6; ++i)
            for (int c : cus) sweep_group(bits, sites[0], knobs[i], c, dump);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--table")) return table_mode();
    if (argc == 2 && !std::strcmp(argv[1], "--sweep")) return sweep_mode(false);
    if (argc == 2 && !std::strcmp(argv[1], "--dump")) return sweep_mode(true);
    std::fprintf(stderr, "usage: gemm_route_check --table < cases | --sweep | --dump\n");
    return 2;
}
