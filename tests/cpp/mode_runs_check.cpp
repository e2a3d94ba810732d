// Host check of mode_runs.h (the GPU-free pieces of mode_values): the geometry tiles every line exactly once, the closing search ends
// a chunk's open run where a linear walk does (runs that end on the chunk's last element, on the next chunk's first, at the line's end),
// the candidate order is total and is "longer, then earlier head", and a scalar model of the run scan built from these pieces finds
// the same winner as a brute force over the whole line.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mode_runs.h"

using namespace rmhip;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

static const uint64_t PAD = ~0ull;

static uint64_t lp_of(uint64_t len) {
    uint64_t lp = 2;
    while (lp < len) lp <<= 1;
    return lp;
}

static void check_geometry(uint64_t nlines, uint64_t len) {
    const uint64_t lp = lp_of(len);
    const ModeGeom g = mode_geometry(lp);
    CHECK(g.chunk * g.per_line == lp && g.chunk >= 1, "lp %llu: chunk %llu x %llu", (unsigned long long)lp, (unsigned long long)g.chunk, (unsigned long long)g.per_line);
    CHECK((g.wave != 0) == (lp <= MODE_WAVE_LP), "lp %llu: granularity", (unsigned long long)lp);
    CHECK(g.wave ? g.per_line == 1 : (g.chunk <= MODE_CHUNK && g.chunk % (64 * MODE_WAVES) == 0), "lp %llu: unit size", (unsigned long long)lp);
    std::vector<unsigned char> seen(nlines * lp, 0);
    const uint64_t units = nlines * g.per_line;
    for (uint64_t u = 0; u < units; ++u) {
        const uint64_t line = u / g.per_line, c0 = (u % g.per_line) * g.chunk;
        for (uint64_t i = c0; i < c0 + g.chunk; ++i) seen[line * lp + i]++;
    }
    for (unsigned char s : seen) CHECK(s == 1, "lp %llu lines %llu: an element covered %d times", (unsigned long long)lp, (unsigned long long)nlines, (int)s);
    const uint64_t grid = mode_grid(g, nlines);
    CHECK(g.wave ? grid * MODE_WAVES >= units && (grid - 1) * MODE_WAVES < units : grid == units, "grid %llu for %llu units", (unsigned long long)grid,
          (unsigned long long)units);
}

static void check_candidates() {
    const uint32_t lens[] = {1, 2, 3, 64, 65, 0x7fffffffu, 0xffffffffu}, heads[] = {0, 1, 63, 64, 2047, 2048, 0x7ffffffeu};
    std::vector<uint64_t> all{0};
    for (uint32_t l : lens)
        for (uint32_t h : heads) {
            const uint64_t c = mode_cand(l, h);
            CHECK(mode_cand_len(c) == l && mode_cand_head(c) == h, "pack (%u, %u)", l, h);
            CHECK(mode_cand_better(c, 0) && !mode_cand_better(0, c), "(%u, %u) against no run", l, h);
            all.push_back(c);
        }
    for (uint64_t a : all)
        for (uint64_t b : all) {
            const bool rule = mode_cand_len(a) > mode_cand_len(b) || (mode_cand_len(a) == mode_cand_len(b) && a != 0 && b != 0 && mode_cand_head(a) < mode_cand_head(b)) ||
                              (a != 0 && b == 0);
            CHECK(mode_cand_better(a, b) == rule, "order of %llx and %llx", (unsigned long long)a, (unsigned long long)b);
            CHECK(a == b || mode_cand_better(a, b) != mode_cand_better(b, a), "total order of %llx and %llx", (unsigned long long)a, (unsigned long long)b);
            CHECK(mode_cand_best(a, b) == std::max(a, b), "best of %llx and %llx", (unsigned long long)a, (unsigned long long)b);
        }
}

// the run scan in scalar form, unit by unit and stretch by stretch as the kernel cuts the line: a stretch owns the runs that start in it
static uint64_t scan_line(const std::vector<uint64_t>& k, std::vector<uint32_t>* runlen) {
    const uint64_t lp = k.size();
    const ModeGeom g = mode_geometry(lp);
    const int wpu = g.wave ? 1 : MODE_WAVES;
    uint64_t best = 0;
    runlen->assign(lp, 0);
    for (uint64_t u = 0; u < g.per_line; ++u) {
        const uint64_t c0 = u * g.chunk, c1 = c0 + g.chunk, q = g.chunk / wpu;
        uint64_t end_of_chunk = c1;  // the one search of the chunk
        if (c1 < lp && k[c1 - 1] != PAD) end_of_chunk = mode_upper_bound(k.data(), c1, lp, k[c1 - 1]);
        if (c1 == lp) end_of_chunk = lp;
        std::vector<uint32_t> first(wpu, MODE_NONE);
        for (int w = 0; w < wpu; ++w)
            for (uint64_t i = c0 + w * q; i < c0 + (w + 1) * q; ++i)
                if (i == 0 || k[i] != k[i - 1]) {
                    first[w] = (uint32_t)i;
                    break;
                }
        for (int w = 0; w < wpu; ++w) {
            const uint64_t s0 = c0 + w * q, s1 = s0 + q;
            uint64_t stretch_end = end_of_chunk;
            for (int v = wpu - 1; v > w; --v)
                if (first[v] != MODE_NONE) stretch_end = first[v];
            for (uint64_t i = s0; i < s1; ++i) {
                if (!(i == 0 || k[i] != k[i - 1]) || k[i] == PAD) continue;
                uint64_t nb = i + 1;
                while (nb < s1 && k[nb] == k[nb - 1]) ++nb;
                if (nb == s1) nb = stretch_end;  // open at the stretch's end: the kernel does not look past it
                (*runlen)[i] = (uint32_t)(nb - i);
                best = mode_cand_best(best, mode_cand((uint32_t)(nb - i), (uint32_t)i));
            }
        }
    }
    return best;
}

static void check_scan(const std::vector<uint64_t>& k, const char* what) {
    const uint64_t lp = k.size();
    uint64_t want = 0;
    std::vector<uint32_t> want_len(lp, 0), got_len;
    for (uint64_t i = 0; i < lp;) {
        uint64_t j = i + 1;
        while (j < lp && k[j] == k[i]) ++j;
        if (k[i] != PAD) {
            want_len[i] = (uint32_t)(j - i);
            if (j - i > mode_cand_len(want)) want = mode_cand((uint32_t)(j - i), (uint32_t)i);  // the first of the longest
        }
        CHECK(mode_upper_bound(k.data(), i + 1, lp, k[i]) == j, "%s: upper bound from %llu", what, (unsigned long long)i);
        i = j;
    }
    const uint64_t got = scan_line(k, &got_len);
    CHECK(got == want, "%s (lp %llu): winner (%u, %u), expected (%u, %u)", what, (unsigned long long)lp, mode_cand_len(got), mode_cand_head(got), mode_cand_len(want),
          mode_cand_head(want));
    CHECK(got_len == want_len, "%s (lp %llu): run lengths", what, (unsigned long long)lp);
}

// a sorted line of `len` keys in runs of the given lengths (cycled), padded to its power of two
static std::vector<uint64_t> line_of(uint64_t len, const std::vector<uint64_t>& runs, uint64_t nans) {
    std::vector<uint64_t> k(lp_of(len), PAD);
    uint64_t i = 0, key = 100, r = 0;
    while (i + nans < len) {
        uint64_t n = std::min<uint64_t>(runs[r++ % runs.size()], len - nans - i);
        while (n--) k[i++] = key;
        key += 7;
    }
    return k;
}

int main() {
    const uint64_t C = MODE_CHUNK, lens[] = {1, 2, 3, 63, 64, 65, MODE_WAVE_LP - 1, MODE_WAVE_LP, MODE_WAVE_LP + 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 17, 4 * C, 8 * C};
    for (uint64_t len : lens)
        for (uint64_t nlines : {1ull, 2ull, 3ull, 4ull, 5ull, 64ull, 65ull}) check_geometry(nlines, len);
    check_candidates();
    const uint64_t Q = C / MODE_WAVES;
    for (uint64_t len : lens) {
        check_scan(line_of(len, {1}, 0), "all distinct");
        check_scan(line_of(len, {len}, 0), "one value");
        check_scan(line_of(len, {1}, len), "all NaN");
        check_scan(line_of(len, {3, 1, 3, 2}, len / 3), "short runs and NaNs");
        check_scan(line_of(len, {C}, 0), "runs that end on a chunk's last element");
        check_scan(line_of(len, {C + 1, C - 1}, 0), "runs that end on a chunk's first element");
        check_scan(line_of(len, {C - 1, 2 * C + 2}, 1), "runs across two chunk boundaries");
        check_scan(line_of(len, {Q, Q - 1, Q + 1, 64, 63, 65}, 0), "runs around the quarters and the rows");
        check_scan(line_of(len, {5, C, 5, C}, 2), "two longest runs in different chunks: the first wins");
    }
    std::srand(12345);
    for (int t = 0; t < 200; ++t) {
        std::vector<uint64_t> runs;
        for (int r = 0; r < 8; ++r) runs.push_back(1 + std::rand() % (t % 2 ? 40 : (int)(2 * C)));
        const uint64_t len = 1 + std::rand() % (5 * C);
        check_scan(line_of(len, runs, std::rand() % 3 ? 0 : std::rand() % len), "random runs");
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("mode runs ok\n");
    return 0;
}
