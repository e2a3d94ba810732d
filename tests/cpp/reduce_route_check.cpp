// Host-logic check of the reduction routing (runmat_amd/csrc/reduce_plan.h route_reduction): the shape table that
// tests/test_gpu_reduce_paths.py drives on the device (tests/reduce_ref.py ROUTE_TABLE is the same list) must take the stated
// kernel, partial count and finalize on 256 CUs / 8 XCDs at both storage widths, and must reach every kernel with both finalizes.
// No GPU needed.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "reduce_plan.h"

using namespace rmhip;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::fprintf(stderr, "FAIL %s: ", #cond);      \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fputc('\n', stderr);                      \
            ++failures;                                    \
        }                                                  \
    } while (0)

struct Row {
    uint64_t pre, red, post;
    ReduceKernel kernel;
    uint64_t nsplit;
    bool flat;
};
using K = ReduceKernel;
static const Row TABLE[] = {
    {1, 3, 1025, K::SHORT, 1, true},
    {1, 255, 1030, K::SHORT, 1, true},
    {1, 1, 1024, K::SHORT, 1, true},
    {1, 255, 1023, K::CONTIG, 1, false},  // one slice below the short threshold
    {1, 256, 1024, K::CONTIG, 1, true},
    {1, 300, 40, K::CONTIG, 1, false},
    {1, 2047, 3, K::CONTIG, 1, false},
    {1, 5, 1, K::CONTIG, 1, false},
    {1, 2048, 3, K::CONTIG_V2, 1, false},
    {1, 6000, 1, K::CONTIG_V2, 3, false},
    {1, 70000, 1, K::CONTIG_V2, 9, false},
    {1, 4096, 1030, K::CONTIG_V2, 2, true},
    {1, 2049, 3, K::CONTIG_V2_ODD, 2, false},
    {1, 6001, 2, K::CONTIG_V2_ODD, 3, false},
    {1, 70001, 1, K::CONTIG_V2_ODD, 9, false},
    {1, 2049, 1030, K::CONTIG_V2_ODD, 2, true},
    {2, 9, 1, K::STRIDED, 1, false},
    {6, 50, 4, K::STRIDED, 1, false},
    {7, 5000, 1, K::STRIDED, 10, false},
    {300, 257, 1, K::STRIDED, 17, false},
    {3, 70000, 1, K::STRIDED, 69, false},
    {511, 600, 1, K::STRIDED, 38, false},
    {255, 40, 70, K::STRIDED, 3, true},
    {16, 20, 1100, K::STRIDED, 1, true},
    {512, 40, 1, K::STRIDED_V2, 3, false},
    {512, 600, 1, K::STRIDED_V2, 38, false},
    {514, 33, 3, K::STRIDED_V2, 3, true},
    {1100, 20, 1, K::STRIDED_V2, 2, true},
    {600, 16, 30, K::STRIDED_V2, 1, true},
    {513, 37, 1, K::STRIDED_V2_ODD, 3, false},
    {1001, 9, 1, K::STRIDED_V2_ODD, 1, false},
    {513, 600, 1, K::STRIDED_V2_ODD, 38, false},
    {515, 33, 3, K::STRIDED_V2_ODD, 3, true},
    {1025, 20, 1, K::STRIDED_V2_ODD, 2, true},
    {601, 16, 30, K::STRIDED_V2_ODD, 1, true},
};

int main() {
    bool reached[7][2] = {};
    for (const Row& t : TABLE)  // the table itself, for tests/test_reduce_ref_host.py to hold the GPU tests' copy against
        std::printf("row %llu %llu %llu %s %llu %s\n", (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post,
                    reduce_kernel_name(t.kernel), (unsigned long long)t.nsplit, t.flat ? "flat" : "wave");
    for (unsigned eb : {8u, 4u})
        for (const Row& t : TABLE) {
            CHECK(t.pre * t.red * t.post <= 4300000ull, "[%llu,%llu,%llu] is larger than the GPU tests allow", (unsigned long long)t.pre,
                  (unsigned long long)t.red, (unsigned long long)t.post);
            const ReduceRoute r = route_reduction(t.pre, t.red, t.post, 256, 8, eb, true);
            CHECK(r.valid && r.kernel == t.kernel && r.nsplit == t.nsplit && r.flat_final == t.flat,
                  "[%llu,%llu,%llu] at %u bytes: %s nsplit %llu %s, table says %s nsplit %llu %s", (unsigned long long)t.pre,
                  (unsigned long long)t.red, (unsigned long long)t.post, eb, reduce_kernel_name(r.kernel), (unsigned long long)r.nsplit,
                  r.flat_final ? "flat" : "wave", reduce_kernel_name(t.kernel), (unsigned long long)t.nsplit, t.flat ? "flat" : "wave");
            if (r.valid) reached[(int)r.kernel][r.flat_final ? 1 : 0] = true;
            // what the kernels need of the route: chunks that cover the reduced extent, one partial per slice for SHORT, the wide
            // geometry covering every pair of lines
            if (!r.valid) continue;
            if (r.kernel == K::SHORT) CHECK(r.nsplit == 1 && t.red < 256 && 4096 / t.red >= 1, "short tile");
            if (r.kernel == K::STRIDED_V2 || r.kernel == K::STRIDED_V2_ODD) {
                CHECK((uint64_t)r.wide.bx * r.wide.win >= (t.pre + 1) / 2 && r.wide.win <= r.wide.threads && r.wide.threads <= 256, "wide windows");
                CHECK((r.kernel == K::STRIDED_V2_ODD) == ((t.pre & 1) != 0), "odd form for odd pre");
            }
            if (r.kernel == K::CONTIG_V2 || r.kernel == K::CONTIG_V2_ODD) CHECK((r.kernel == K::CONTIG_V2_ODD) == ((t.red & 1) != 0), "odd form for odd red");
            CHECK(ceil_div_u64(t.red, r.nsplit) * r.nsplit >= t.red, "chunks cover red");
        }
    for (int k = 0; k < 7; ++k)
        for (int f = 0; f < 2; ++f) {
            if (k == (int)K::SHORT && f == 0) continue;  // SHORT needs >= 1024 slices and has one partial: always the flat finalize
            CHECK(reached[k][f], "%s with the %s finalize is not in the table", reduce_kernel_name((K)k), f ? "flat" : "wave");
            if (reached[k][f]) std::printf("reached %s + %s\n", reduce_kernel_name((K)k), f ? "flat" : "wave");
        }
    CHECK(reached[(int)K::SHORT][1] && !reached[(int)K::SHORT][0], "short always finalizes flat");

    // an element-aligned base turns the even forms into the ODD ones and nothing else
    for (const Row& t : TABLE) {
        const ReduceRoute a = route_reduction(t.pre, t.red, t.post, 256, 8, 8, true), u = route_reduction(t.pre, t.red, t.post, 256, 8, 8, false);
        const K want = a.kernel == K::CONTIG_V2 ? K::CONTIG_V2_ODD : a.kernel == K::STRIDED_V2 ? K::STRIDED_V2_ODD : a.kernel;
        CHECK(u.kernel == want && u.nsplit == a.nsplit && u.flat_final == a.flat_final, "unaligned base [%llu,%llu,%llu]", (unsigned long long)t.pre,
              (unsigned long long)t.red, (unsigned long long)t.post);
    }
    // the two-operand skeletons: no unaligned-pair form of kernel A, no 16-byte form of kernel B, the first flat clause only
    {
        const ReduceRoute s = route_reduction(1, 17, 5000, 256, 8, 8, true, true), v = route_reduction(1, 6000, 1, 256, 8, 8, true, true),
                          o = route_reduction(1, 6001, 2, 256, 8, 8, true, true), w = route_reduction(512, 600, 1, 256, 8, 8, true, true),
                          m = route_reduction(255, 40, 70, 256, 8, 8, true, true);
        CHECK(s.kernel == K::SHORT && s.nsplit == 1 && s.flat_final, "dot short");
        CHECK(v.kernel == K::CONTIG_V2 && v.nsplit == 3 && !v.flat_final, "dot contig_v2");
        CHECK(o.kernel == K::CONTIG && o.nsplit == 3, "dot odd slice: %s", reduce_kernel_name(o.kernel));
        CHECK(w.kernel == K::STRIDED && w.nsplit == w.plan.nsplit && w.nsplit > 1, "dot strided: %s", reduce_kernel_name(w.kernel));
        CHECK(m.kernel == K::STRIDED && m.nsplit == 3 && m.flat_final, "dot strided, split, post > 1, flat");
        CHECK(reduce_flat_final(32, 16384) && !reduce_flat_final(32, 16384, true) && !reduce_flat_final(9, 1024) && reduce_flat_final(8, 1024, true),
              "flat finalize clauses");
    }
    // an empty reduced extent still gets one (empty) chunk per slice on every route
    for (uint64_t pre : {1ull, 3ull, 512ull, 513ull}) {
        const ReduceRoute e = route_reduction(pre, 0, 1, 256, 8, 8, true);
        CHECK(e.valid && e.nsplit == 1, "red == 0 at pre %llu: nsplit %llu", (unsigned long long)pre, (unsigned long long)e.nsplit);
    }
    const ReduceRoute none = route_reduction(0, 5, 1, 256, 8, 8, true);
    CHECK(!none.valid, "no output slices");
    if (failures) return 1;
    std::puts("reduce route ok");
    return 0;
}
