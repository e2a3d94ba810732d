// Host-logic check of the reduction routing (runmat_amd/csrc/reduce_plan.h route_reduction): the shape table that
// tests/test_gpu_reduce_paths.py drives on the device (tests/reduce_ref.py ROUTE_TABLE is the same list) must take the stated
// kernel, partial count and finalize on 256 CUs / 8 XCDs at both storage widths, and must reach every kernel with both finalizes.
// The accumulator family (reduce2.hip) and the generated one (rmhip_fused_reduction) have a table each, with the launch's grid.x and
// block as well (ACC_TABLE / GEN_TABLE; tests/reduce_ref.py ACC_ROUTE_TABLE / GEN_ROUTE_TABLE are the same lists).
// No GPU needed.
#include <cstddef>
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

// the families whose launchers used to decide for themselves: also the launch (grid.x, block).  The values were taken from those
// launchers before they moved into the route.
struct FamRow {
    uint64_t pre, red, post;
    ReduceKernel kernel;
    uint64_t nsplit;
    bool flat;
    unsigned gx, block;
};
static const FamRow ACC_TABLE[] = {
    {1, 3, 1025, K::SHORT, 1, true, 5, 256},
    {1, 255, 1030, K::SHORT, 1, true, 65, 256},
    {1, 255, 1023, K::CONTIG, 1, false, 1, 256},
    {1, 256, 1024, K::CONTIG, 1, true, 1, 256},
    {1, 300, 40, K::CONTIG, 1, false, 1, 256},
    {1, 1023, 3, K::CONTIG, 1, false, 1, 256},  // the 16-byte kernel A starts at 1024 here, not at 2048
    {1, 1024, 3, K::CONTIG_V2, 1, false, 1, 256},
    {1, 2048, 3, K::CONTIG_V2, 1, false, 1, 256},
    {1, 6000, 1, K::CONTIG_V2, 3, false, 3, 256},
    {1, 70000, 1, K::CONTIG_V2, 9, false, 9, 256},  // 256-thread blocks, the partial count of the plan's 1024
    {1, 4096, 1030, K::CONTIG_V2, 2, true, 2, 256},
    {1, 1025, 3, K::CONTIG_V2_ODD, 1, false, 1, 256},
    {1, 2047, 3, K::CONTIG_V2_ODD, 1, false, 1, 256},
    {1, 2049, 3, K::CONTIG_V2_ODD, 2, false, 2, 256},
    {1, 6001, 2, K::CONTIG_V2_ODD, 3, false, 3, 256},
    {1, 70001, 1, K::CONTIG_V2_ODD, 9, false, 9, 256},
    {1, 1025, 1030, K::CONTIG_V2_ODD, 1, true, 1, 256},
    {2, 9, 1, K::STRIDED, 1, false, 1, 256},
    {7, 5000, 1, K::STRIDED, 313, false, 1, 256},  // 256 lanes along `pre`, no rows along `red`: not the plan's 10
    {100, 600, 1, K::STRIDED, 38, false, 1, 256},  // (the plan: tx 128, ty 2, 19 partials)
    {128, 257, 3, K::STRIDED, 17, false, 1, 256},
    {300, 257, 1, K::STRIDED, 17, false, 2, 256},
    {3, 70000, 1, K::STRIDED, 2048, false, 1, 256},
    {511, 600, 1, K::STRIDED, 38, false, 2, 256},
    {255, 40, 70, K::STRIDED, 3, true, 1, 256},
    {16, 20, 1100, K::STRIDED, 2, true, 1, 256},
    {512, 40, 1, K::STRIDED_V2, 3, false, 1, 256},
    {512, 600, 1, K::STRIDED_V2, 38, false, 1, 256},
    {514, 33, 3, K::STRIDED_V2, 3, true, 2, 192},
    {600, 16, 30, K::STRIDED_V2, 1, true, 2, 192},
    {513, 37, 1, K::STRIDED_V2_ODD, 3, false, 2, 192},
    {513, 600, 1, K::STRIDED_V2_ODD, 38, false, 2, 192},
    {515, 33, 3, K::STRIDED_V2_ODD, 3, true, 2, 192},
    {601, 16, 30, K::STRIDED_V2_ODD, 1, true, 2, 192},
};
// generated kernels reduce axis 0 ([1, red, slices]) or axis 1 ([slices, red, 1]); no SHORT and no ODD forms: such shapes take the
// 8-byte kernels
static const FamRow GEN_TABLE[] = {
    {1, 5, 1, K::CONTIG, 1, false, 1, 256},
    {1, 300, 40, K::CONTIG, 1, false, 1, 256},
    {1, 2049, 3, K::CONTIG, 2, false, 2, 256},
    {1, 6001, 2, K::CONTIG, 3, false, 3, 256},
    {1, 17, 5000, K::CONTIG, 1, true, 1, 256},
    {1, 2048, 3, K::CONTIG_V2, 1, false, 1, 256},
    {1, 6000, 1, K::CONTIG_V2, 3, false, 3, 256},
    {1, 70000, 1, K::CONTIG_V2, 9, false, 9, 1024},
    {1, 4096, 1030, K::CONTIG_V2, 2, true, 2, 256},
    {7, 5000, 1, K::STRIDED, 10, false, 1, 256},
    {300, 257, 1, K::STRIDED, 17, false, 2, 256},
    {511, 600, 1, K::STRIDED, 38, false, 2, 256},
    {513, 600, 1, K::STRIDED, 38, false, 3, 256},
    {1001, 9, 1, K::STRIDED, 1, false, 4, 256},
    {1025, 20, 1, K::STRIDED, 2, true, 5, 256},
    {512, 40, 1, K::STRIDED_V2, 3, false, 1, 256},
    {512, 600, 1, K::STRIDED_V2, 38, false, 1, 256},
    {1100, 20, 1, K::STRIDED_V2, 2, true, 8, 128},
    {8192, 100, 1, K::STRIDED_V2, 7, true, 16, 256},
};

// a family's table: every row as stated at both storage widths, every kernel the family has reached with both finalizes
template <size_t N>
static void check_family(const char* name, const FamRow (&table)[N], const ReduceFamily& fam, std::initializer_list<ReduceKernel> kernels) {
    bool reached[7][2] = {};
    for (const FamRow& t : table)
        std::printf("%s %llu %llu %llu %s %llu %s %u %u\n", name, (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post,
                    reduce_kernel_name(t.kernel), (unsigned long long)t.nsplit, t.flat ? "flat" : "wave", t.gx, t.block);
    for (unsigned eb : {8u, 4u})
        for (const FamRow& t : table) {
            CHECK(t.pre * t.red * t.post <= 4300000ull, "%s [%llu,%llu,%llu] is larger than the GPU tests allow", name, (unsigned long long)t.pre,
                  (unsigned long long)t.red, (unsigned long long)t.post);
            const ReduceRoute r = route_reduction(t.pre, t.red, t.post, 256, 8, eb, true, fam);
            CHECK(r.valid && r.kernel == t.kernel && r.nsplit == t.nsplit && r.flat_final == t.flat && r.gx == t.gx && r.block == t.block,
                  "%s [%llu,%llu,%llu] at %u bytes: %s nsplit %llu %s grid.x %u block %u, table says %s nsplit %llu %s grid.x %u block %u", name,
                  (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post, eb, reduce_kernel_name(r.kernel),
                  (unsigned long long)r.nsplit, r.flat_final ? "flat" : "wave", r.gx, r.block, reduce_kernel_name(t.kernel), (unsigned long long)t.nsplit,
                  t.flat ? "flat" : "wave", t.gx, t.block);
            if (!r.valid) continue;
            reached[(int)r.kernel][r.flat_final ? 1 : 0] = true;
            CHECK(r.nslices == t.pre * t.post && ceil_div_u64(t.red, r.nsplit) * r.nsplit >= t.red, "%s: slices and chunks", name);
            const bool contig = t.pre == 1, wide = r.kernel == K::STRIDED_V2 || r.kernel == K::STRIDED_V2_ODD;
            if (r.kernel == K::SHORT) CHECK(r.nsplit == 1 && (uint64_t)r.gx * r.span >= r.nslices && r.span * t.red <= REDUCE_SHORT_TILE && r.span <= r.block, "%s: short tile", name);
            else if (contig) CHECK(r.gx == r.nsplit && (uint64_t)r.gy * r.gz >= t.post, "%s: kernel A's grid", name);
            else CHECK(r.gy == r.nsplit && r.gz == t.post && (uint64_t)r.gx * r.span * (wide ? 2 : 1) >= t.pre && r.span <= r.block, "%s: kernel B's grid", name);
        }
    for (ReduceKernel k : kernels)
        for (int f = 0; f < 2; ++f) {
            if (k == K::SHORT && f == 0) continue;  // always the flat finalize
            CHECK(reached[(int)k][f], "%s: %s with the %s finalize is not in the table", name, reduce_kernel_name(k), f ? "flat" : "wave");
        }
    for (int k = 0; k < 7; ++k) {
        bool has = false;
        for (ReduceKernel q : kernels) has = has || (int)q == k;
        CHECK(has || (!reached[k][0] && !reached[k][1]), "%s reaches %s, which it does not have", name, reduce_kernel_name((K)k));
    }
}

int main() {
    bool reached[7][2] = {};
    for (const Row& t : TABLE)  // the table itself, for tests/test_reduce_ref_host.py to hold the GPU tests' copy against
        std::printf("row %llu %llu %llu %s %llu %s\n", (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post,
                    reduce_kernel_name(t.kernel), (unsigned long long)t.nsplit, t.flat ? "flat" : "wave");
    for (unsigned eb : {8u, 4u})
        for (const Row& t : TABLE) {
            CHECK(t.pre * t.red * t.post <= 4300000ull, "[%llu,%llu,%llu] is larger than the GPU tests allow", (unsigned long long)t.pre,
                  (unsigned long long)t.red, (unsigned long long)t.post);
            const ReduceRoute r = route_reduction(t.pre, t.red, t.post, 256, 8, eb, true, REDUCE_PLAIN);
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
                CHECK((uint64_t)r.gx * r.span >= (t.pre + 1) / 2 && r.span <= r.block && r.block <= 256, "wide windows");
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
        const ReduceRoute a = route_reduction(t.pre, t.red, t.post, 256, 8, 8, true, REDUCE_PLAIN), u = route_reduction(t.pre, t.red, t.post, 256, 8, 8, false, REDUCE_PLAIN);
        const K want = a.kernel == K::CONTIG_V2 ? K::CONTIG_V2_ODD : a.kernel == K::STRIDED_V2 ? K::STRIDED_V2_ODD : a.kernel;
        CHECK(u.kernel == want && u.nsplit == a.nsplit && u.flat_final == a.flat_final, "unaligned base [%llu,%llu,%llu]", (unsigned long long)t.pre,
              (unsigned long long)t.red, (unsigned long long)t.post);
    }
    // the two-operand skeletons: no unaligned-pair form of kernel A, no 16-byte form of kernel B, the first flat clause only
    {
        const ReduceFamily& D = REDUCE_DOT;
        const ReduceRoute s = route_reduction(1, 17, 5000, 256, 8, 8, true, D), v = route_reduction(1, 6000, 1, 256, 8, 8, true, D),
                          o = route_reduction(1, 6001, 2, 256, 8, 8, true, D), w = route_reduction(512, 600, 1, 256, 8, 8, true, D),
                          m = route_reduction(255, 40, 70, 256, 8, 8, true, D), e = route_reduction(1, 6000, 1, 256, 8, 8, false, D);
        CHECK(s.kernel == K::SHORT && s.nsplit == 1 && s.flat_final, "dot short");
        CHECK(v.kernel == K::CONTIG_V2 && v.nsplit == 3 && !v.flat_final, "dot contig_v2");
        CHECK(o.kernel == K::CONTIG && o.nsplit == 3, "dot odd slice: %s", reduce_kernel_name(o.kernel));
        CHECK(e.kernel == K::CONTIG && e.nsplit == 3, "dot element-aligned base: %s", reduce_kernel_name(e.kernel));
        CHECK(w.kernel == K::STRIDED && w.nsplit == plan_reduction(512, 600, 1, 256, 8).nsplit && w.nsplit > 1, "dot strided: %s", reduce_kernel_name(w.kernel));
        CHECK(m.kernel == K::STRIDED && m.nsplit == 3 && m.flat_final, "dot strided, split, post > 1, flat");
        CHECK(reduce_flat_final(32, 16384, REDUCE_PLAIN) && !reduce_flat_final(32, 16384, D) && !reduce_flat_final(9, 1024, REDUCE_PLAIN) && reduce_flat_final(8, 1024, D),
              "flat finalize clauses");
        CHECK(reduce_flat_final(32, 16384, REDUCE_ACCUMULATOR) && !reduce_flat_final(32, 16384, REDUCE_GENERATED) && reduce_flat_final(8, 1024, REDUCE_GENERATED),
              "flat finalize clauses of the accumulator and generated families");
    }
    check_family("acc", ACC_TABLE, REDUCE_ACCUMULATOR,
                 {K::SHORT, K::CONTIG, K::CONTIG_V2, K::CONTIG_V2_ODD, K::STRIDED, K::STRIDED_V2, K::STRIDED_V2_ODD});
    check_family("gen", GEN_TABLE, REDUCE_GENERATED, {K::CONTIG, K::CONTIG_V2, K::STRIDED, K::STRIDED_V2});
    // an element-aligned base: the accumulator family takes the ODD forms, the generated one the 8-byte kernels
    for (const FamRow& t : ACC_TABLE) {
        const ReduceRoute a = route_reduction(t.pre, t.red, t.post, 256, 8, 8, true, REDUCE_ACCUMULATOR), u = route_reduction(t.pre, t.red, t.post, 256, 8, 8, false, REDUCE_ACCUMULATOR);
        const K want = a.kernel == K::CONTIG_V2 ? K::CONTIG_V2_ODD : a.kernel == K::STRIDED_V2 ? K::STRIDED_V2_ODD : a.kernel;
        CHECK(u.kernel == want && u.nsplit == a.nsplit && u.flat_final == a.flat_final && u.gx == a.gx && u.block == a.block, "acc unaligned base [%llu,%llu,%llu]",
              (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post);
    }
    for (const FamRow& t : GEN_TABLE) {
        const ReduceRoute u = route_reduction(t.pre, t.red, t.post, 256, 8, 8, false, REDUCE_GENERATED);
        CHECK(u.kernel == (t.pre == 1 ? K::CONTIG : K::STRIDED) && u.nsplit == plan_reduction(t.pre, t.red, t.post, 256, 8).nsplit, "gen unaligned base [%llu,%llu,%llu]",
              (unsigned long long)t.pre, (unsigned long long)t.red, (unsigned long long)t.post);
    }
    // an empty reduced extent still gets one (empty) chunk per slice on every route
    for (uint64_t pre : {1ull, 3ull, 512ull, 513ull}) {
        const ReduceRoute e = route_reduction(pre, 0, 1, 256, 8, 8, true, REDUCE_PLAIN);
        CHECK(e.valid && e.nsplit == 1, "red == 0 at pre %llu: nsplit %llu", (unsigned long long)pre, (unsigned long long)e.nsplit);
    }
    const ReduceRoute none = route_reduction(0, 5, 1, 256, 8, 8, true, REDUCE_PLAIN);
    CHECK(!none.valid, "no output slices");
    if (failures) return 1;
    std::puts("reduce route ok");
    return 0;
}
