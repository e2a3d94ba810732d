// Host-logic check of the scan routing (runmat_amd/csrc/reduce_plan.h route_scan and route_cumextreme): the shape tables that
// tests/test_gpu_scan_paths.py drives on the device (tests/scan_ref.py SCAN_ROUTE_TABLE / SCAN_HOST_ROWS / CUMEXT_ROUTE_TABLE are the
// same lists) must take the stated kernel, lines per block, chunk count and launch count on 256 CUs; the GPU rows must reach every
// kernel form, both lines-per-block values and one, up to 256 and more than 256 chunks per line (the carry kernel's second trip); no
// shape may reach 64 lines per block with more than one chunk (launch_cumulative has no such instantiation); and the routes must
// decide what the launchers' own chains decided before the routes existed (restated below).  No GPU needed.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reduce_plan.h"

using namespace rmhip;
typedef unsigned long long ull;

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
    uint64_t pre, len, post;
    ScanKernel kernel;
    unsigned lines_per_block;  // 0 unless STAGED
    uint64_t nchunks;
    unsigned launches;
};
using K = ScanKernel;
static const Row GPU_TABLE[] = {
    {2, 9, 1, K::LINES_64x32, 0, 1, 1},
    {7, 5000, 1, K::LINES_64x32, 0, 1, 1},
    {40, 255, 3, K::LINES_64x32, 0, 1, 1},  // len below the staged threshold
    {262144, 3, 1, K::LINES_256x8, 0, 1, 1},
    {512, 2, 512, K::LINES_256x8, 0, 1, 1},
    {8, 256, 1, K::STAGED, 32, 1, 1},
    {40, 300, 1, K::STAGED, 32, 1, 1},
    {33, 4095, 2, K::STAGED, 32, 1, 1},  // len just under the chunking threshold; 31 idle lanes in the second block
    {64, 256, 256, K::STAGED, 64, 1, 1},
    {16384, 256, 1, K::STAGED, 64, 1, 1},
    {9, 4096, 1, K::STAGED, 32, 4, 3},
    {40, 9001, 1, K::STAGED, 32, 8, 3},  // chunks of 1152: a ragged last chunk
    {17, 9001, 3, K::STAGED, 32, 8, 3},
    {32, 8192, 2, K::STAGED, 32, 8, 3},
    {8, 300000, 1, K::STAGED, 32, 276, 3},  // chunks of 1088: the carry kernel's second trip
    {1, 1, 5, K::SHORT, 0, 1, 1},
    {1, 3, 1025, K::SHORT, 0, 1, 1},
    {1, 16, 300, K::SHORT, 0, 1, 1},
    {1, 255, 17, K::SHORT, 0, 1, 1},  // 16 lines per block
    {1, 256, 3, K::CHUNKS, 0, 1, 1},
    {1, 16384, 2, K::CHUNKS, 0, 1, 1},
    {1, 16385, 2, K::CHUNKS, 0, 2, 3},  // one element in the last chunk
    {1, 70001, 3, K::CHUNKS, 0, 5, 3},
    {1, 4300000, 1, K::CHUNKS, 0, 263, 3},  // the carry kernel's second trip
    {1, 256, 65537, K::CHUNKS, 0, 1, 1},    // lines spill into grid z
};
// pinned here only: the two sides of every threshold the GPU rows do not already straddle
static const Row HOST_TABLE[] = {
    {2048, 4096, 1, K::STAGED, 32, 4, 3},  // 64 line blocks: the last count that is chunked on 256 CUs
    {2049, 4096, 1, K::STAGED, 32, 1, 1},
    {65535, 256, 1, K::STAGED, 64, 1, 1},  // one line below num_cus * 256
    {65536, 256, 1, K::LINES_64x32, 0, 1, 1},
    {100, 255, 1, K::LINES_64x32, 0, 1, 1},
    {100, 256, 1, K::STAGED, 32, 1, 1},
    {7, 256, 1, K::LINES_64x32, 0, 1, 1},  // pre below 8
    {262143, 3, 1, K::LINES_64x32, 0, 1, 1},  // one line below num_cus * 1024
    {16320, 256, 1, K::STAGED, 32, 1, 1},     // 255 blocks of 64 lines would leave a CU idle: 32 lines per block
    {8, 4096, 65536, K::LINES_256x8, 0, 1, 1},  // post beyond grid y: not staged
    {1, 255, 3, K::SHORT, 0, 1, 1},
};

struct ExtRow {
    uint64_t pre, len, post;
    bool wave;
    uint64_t nchunks, chunk_len;
};
static const ExtRow CUMEXT_TABLE[] = {
    {1, 511, 3, true, 1, 512},
    {1, 512, 3, true, 2, 256},
    {1, 300000, 1, true, 586, 512},
    {1, 600, 2048, true, 1, 768},  // enough lines: not chunked
    {1, 600, 2047, true, 2, 512},
    {300, 511, 1, false, 1, 511},
    {300, 512, 1, false, 2, 256},
    {7, 5000, 1, false, 19, 264},
    {2, 70001, 1, false, 273, 257},  // a thread of the carry kernel owns two chunks
};

// ---- the launchers' own chains as they stood before route_scan / route_cumextreme (reduce2.hip, order_ops.hip) ----
struct Legacy {
    int kernel;  // ScanKernel
    unsigned lpb;
    uint64_t nchunks, chunk_steps;
    unsigned per_block, gx, gy, gz, block, launches;
    bool valid;
};
static Legacy legacy_scan(uint64_t pre, uint64_t len, uint64_t post, uint64_t cus) {
    Legacy o{};
    o.valid = true;
    o.nchunks = 1;
    o.gx = o.gy = o.gz = 1;
    o.launches = 1;
    const uint64_t lines = pre * post;
    if (pre > 1) {
        if (pre >= 8 && len >= 256 && lines < cus * 256 && post <= 65535) {
            const bool half = pre < 64 || ceil_div_u64(pre, 64) * post < cus;
            const uint64_t line_blocks = ceil_div_u64(pre, half ? 32 : 64) * post;
            uint64_t nchunks = 1, chunk_steps = ceil_div_u64(len, 64) * 64;
            if (line_blocks * 4 <= cus && len >= 4096) {
                uint64_t want = ceil_div_u64(cus * 4, line_blocks), most = len / 1024;
                if (want > most) want = most;
                if (want > 65535) want = 65535;
                if (want > 1) {
                    chunk_steps = ceil_div_u64(ceil_div_u64(len, want), 64) * 64;
                    nchunks = ceil_div_u64(len, chunk_steps);
                }
            }
            o.kernel = (int)K::STAGED;
            o.lpb = half ? 32 : 64;
            o.nchunks = nchunks;
            o.chunk_steps = chunk_steps;
            o.gx = (unsigned)ceil_div_u64(pre, half ? 32 : 64);
            o.gy = (unsigned)post;
            o.gz = (unsigned)nchunks;
            o.block = 512;
            o.launches = nchunks > 1 ? 3 : 1;
        } else if (lines >= cus * 1024) {
            o.kernel = (int)K::LINES_256x8;
            o.gx = (unsigned)ceil_div_u64(lines, 256);
            o.block = 256;
        } else {
            o.kernel = (int)K::LINES_64x32;
            o.gx = (unsigned)ceil_div_u64(lines, 64);
            o.block = 64;
        }
        return o;
    }
    if (len < 256) {
        unsigned per_block = (unsigned)(4096 / len);
        if (per_block > 256) per_block = 256;
        o.kernel = (int)K::SHORT;
        o.per_block = per_block;
        o.gx = (unsigned)ceil_div_u64(lines, per_block);
        o.block = 256;
        return o;
    }
    const uint64_t gy = lines < 65535 ? lines : 65535, gz = ceil_div_u64(lines, gy);
    o.kernel = (int)K::CHUNKS;
    if (gz > 65535) {
        o.valid = false;
        return o;
    }
    o.nchunks = ceil_div_u64(len, 16384);
    o.chunk_steps = 16384;
    o.gx = (unsigned)o.nchunks;
    o.gy = (unsigned)gy;
    o.gz = (unsigned)gz;
    o.block = 256;
    o.launches = o.nchunks > 1 ? 3 : 1;
    return o;
}
struct LegacyExt {
    bool wave;
    uint64_t nchunks, chunk_len;
    unsigned grid, launches;
};
static LegacyExt legacy_cumext(uint64_t pre, uint64_t len, uint64_t post, uint64_t cus) {
    const uint64_t nlines = pre * post;
    const bool wave = pre == 1;
    const uint64_t want = wave ? cus * 8 : cus * 512;
    uint64_t nchunks = 1;
    if (nlines < want && len >= 512) {
        nchunks = std::min<uint64_t>((want + nlines - 1) / nlines, len / 256);
        nchunks = std::min<uint64_t>(nchunks, 8192);
    }
    uint64_t chunk_len = (len + nchunks - 1) / nchunks;
    if (wave) chunk_len = (chunk_len + 64 * 4 - 1) / (64 * 4) * (64 * 4);
    nchunks = (len + chunk_len - 1) / chunk_len;
    const uint64_t pieces = nlines * nchunks;
    return {wave, nchunks, chunk_len, (unsigned)(wave ? (pieces + 3) / 4 : (pieces + 255) / 256), nchunks > 1 ? 3u : 1u};
}

static void check_row(const Row& t, const char* tag) {
    const ScanRoute r = route_scan(t.pre, t.len, t.post, 256);
    CHECK(r.valid && r.kernel == t.kernel && r.lines_per_block == t.lines_per_block && r.nchunks == t.nchunks && r.launches == t.launches,
          "%s [%llu,%llu,%llu]: %s lines/block %u nchunks %llu launches %u, table says %s %u %llu %u", tag, (ull)t.pre, (ull)t.len, (ull)t.post,
          scan_kernel_name(r.kernel), r.lines_per_block, (ull)r.nchunks, r.launches, scan_kernel_name(t.kernel), t.lines_per_block, (ull)t.nchunks,
          t.launches);
}

// what the kernels need of a route: the grid covers every line and chunk, the chunks cover the line in whole tiles
static void check_geometry(uint64_t pre, uint64_t len, uint64_t post, const ScanRoute& r) {
    CHECK(r.nlines == pre * post && r.launches == (r.nchunks > 1 ? 3u : 1u), "[%llu,%llu,%llu]: lines and launches", (ull)pre, (ull)len, (ull)post);
    switch (r.kernel) {
        case K::LINES_64x32:
        case K::LINES_256x8:
            CHECK(r.block == (r.kernel == K::LINES_64x32 ? 64u : 256u) && (uint64_t)r.gx * r.block >= r.nlines && r.gy == 1 && r.gz == 1 && r.nchunks == 1,
                  "[%llu,%llu,%llu]: lines grid", (ull)pre, (ull)len, (ull)post);
            break;
        case K::STAGED:
            CHECK((r.lines_per_block == 32 || r.lines_per_block == 64) && (uint64_t)r.gx * r.lines_per_block >= pre && r.gy == post && r.gz == r.nchunks &&
                      r.gz <= 65535 && r.block == SCAN_STAGED_THREADS && r.chunk_steps % SCAN_STAGED_STEPS == 0 && r.chunk_steps * r.nchunks >= len &&
                      r.chunk_steps * (r.nchunks - 1) < len,
                  "[%llu,%llu,%llu]: staged grid and chunks", (ull)pre, (ull)len, (ull)post);
            CHECK(r.nchunks == 1 || r.lines_per_block == 32, "[%llu,%llu,%llu]: 64 lines per block with %llu chunks", (ull)pre, (ull)len, (ull)post, (ull)r.nchunks);
            break;
        case K::SHORT:
            CHECK(r.per_block >= 1 && r.per_block <= r.block && r.per_block * len <= SCAN_SHORT_TILE && (uint64_t)r.gx * r.per_block >= r.nlines && r.block == SCAN_BLOCK,
                  "[%llu,%llu,%llu]: short tile", (ull)pre, (ull)len, (ull)post);
            break;
        case K::CHUNKS:
            CHECK(r.gx == r.nchunks && (uint64_t)r.gy * r.gz >= r.nlines && r.gy <= 65535 && r.gz <= 65535 && r.chunk_steps == SCAN_CHUNK && r.nchunks * SCAN_CHUNK >= len &&
                      (r.nchunks - 1) * SCAN_CHUNK < len && r.block == SCAN_BLOCK,
                  "[%llu,%llu,%llu]: chunks grid", (ull)pre, (ull)len, (ull)post);
            break;
    }
}

int main() {
    // the tables themselves, for tests/test_scan_ref_host.py to hold tests/scan_ref.py against; a GPU row also with the route's chunk
    // length, which the placements of tests/scan_ref.py derive from the row
    for (const Row& t : GPU_TABLE)
        std::printf("row %llu %llu %llu %s %u %llu %u %llu\n", (ull)t.pre, (ull)t.len, (ull)t.post, scan_kernel_name(t.kernel), t.lines_per_block, (ull)t.nchunks, t.launches,
                    (ull)route_scan(t.pre, t.len, t.post, 256).chunk_steps);
    for (const Row& t : HOST_TABLE)
        std::printf("host %llu %llu %llu %s %u %llu %u\n", (ull)t.pre, (ull)t.len, (ull)t.post, scan_kernel_name(t.kernel), t.lines_per_block, (ull)t.nchunks, t.launches);
    for (const ExtRow& t : CUMEXT_TABLE)
        std::printf("ext %llu %llu %llu %s %llu %llu\n", (ull)t.pre, (ull)t.len, (ull)t.post, t.wave ? "wave" : "thread", (ull)t.nchunks, (ull)t.chunk_len);

    bool kernel_reached[5] = {}, lpb32 = false, lpb64 = false;
    bool chunks_reached[5][3] = {};  // [kernel][1 chunk, 2 .. 256, more than 256]
    bool z_spill = false, idle_lanes = false, ragged_staged = false, ragged_chunks = false;
    for (const Row& t : GPU_TABLE) {
        check_row(t, "gpu row");
        CHECK(t.pre * t.len * t.post <= 17000000ull, "[%llu,%llu,%llu] is larger than the GPU tests allow", (ull)t.pre, (ull)t.len, (ull)t.post);
        const ScanRoute r = route_scan(t.pre, t.len, t.post, 256);
        if (!r.valid) continue;
        check_geometry(t.pre, t.len, t.post, r);
        kernel_reached[(int)r.kernel] = true;
        chunks_reached[(int)r.kernel][r.nchunks == 1 ? 0 : r.nchunks <= 256 ? 1 : 2] = true;
        if (r.kernel == K::STAGED) {
            (r.lines_per_block == 32 ? lpb32 : lpb64) = true;
            idle_lanes = idle_lanes || (t.pre % 32 != 0 && t.pre > 32);
            ragged_staged = ragged_staged || (r.nchunks > 1 && t.len % r.chunk_steps != 0);
        }
        if (r.kernel == K::CHUNKS) {
            z_spill = z_spill || r.gz > 1;
            ragged_chunks = ragged_chunks || (r.nchunks > 1 && t.len % SCAN_CHUNK != 0);
        }
    }
    for (int k = 0; k < 5; ++k) CHECK(kernel_reached[k], "%s is reached by no GPU row", scan_kernel_name((K)k));
    CHECK(lpb32 && lpb64, "both lines-per-block values of the staged form");
    for (K k : {K::STAGED, K::CHUNKS})
        for (int n = 0; n < 3; ++n) CHECK(chunks_reached[(int)k][n], "%s with %s is reached by no GPU row", scan_kernel_name(k), n == 0 ? "one chunk" : n == 1 ? "2 .. 256 chunks" : "more than 256 chunks");
    CHECK(z_spill && idle_lanes && ragged_staged && ragged_chunks, "grid z spill %d, idle lanes %d, ragged last chunk staged %d / contiguous %d", z_spill, idle_lanes, ragged_staged, ragged_chunks);
    for (const Row& t : HOST_TABLE) check_row(t, "host row");

    // a sweep: the route is the launcher's former chain, its geometry holds, and 64 lines per block never come with chunks
    std::vector<uint64_t> extents;
    for (int b = 0; b <= 18; ++b)
        for (long long d = -1; d <= 1; ++d) {
            const long long v = (1ll << b) + d;
            if (v >= 1 && std::find(extents.begin(), extents.end(), (uint64_t)v) == extents.end()) extents.push_back((uint64_t)v);
        }
    unsigned long long swept = 0;
    for (int cus : {256, 128, 64})
        for (uint64_t pre : extents)
            for (uint64_t post : extents)
                for (uint64_t len : {255ull, 256ull, 4095ull, 4096ull, 70001ull}) {
                    const ScanRoute r = route_scan(pre, len, post, cus);
                    const Legacy o = legacy_scan(pre, len, post, (uint64_t)cus);
                    ++swept;
                    CHECK(r.valid == o.valid, "[%llu,%llu,%llu] on %d CUs: valid", (ull)pre, (ull)len, (ull)post, cus);
                    if (!r.valid || !o.valid) continue;
                    CHECK((int)r.kernel == o.kernel && r.nchunks == o.nchunks && r.gx == o.gx && r.gy == o.gy && r.gz == o.gz && r.block == o.block && r.launches == o.launches &&
                              (r.kernel != K::STAGED || (r.lines_per_block == o.lpb && r.chunk_steps == o.chunk_steps)) && (r.kernel != K::SHORT || r.per_block == o.per_block),
                          "[%llu,%llu,%llu] on %d CUs: the route differs from the launcher's former chain", (ull)pre, (ull)len, (ull)post, cus);
                    check_geometry(pre, len, post, r);
                    if (failures > 20) return 1;
                }
    std::printf("swept %llu shapes\n", swept);
    {
        const ScanRoute none = route_scan(0, 5, 1, 256), many = route_scan(1, 256, 65535ull * 65535ull + 1, 256), most = route_scan(1, 256, 65535ull * 65535ull, 256);
        CHECK(!none.valid && !many.valid && most.valid && most.gz == 65535, "no lines, and more contiguous lines than grid (y, z) holds");
    }

    // cummin / cummax
    bool ext_reached[2][3] = {};
    for (const ExtRow& t : CUMEXT_TABLE) {
        const CumextRoute r = route_cumextreme(t.pre, t.len, t.post, 256);
        CHECK(r.valid && r.wave == t.wave && r.nchunks == t.nchunks && r.chunk_len == t.chunk_len, "cumext [%llu,%llu,%llu]: %s nchunks %llu chunk %llu, table says %s %llu %llu",
              (ull)t.pre, (ull)t.len, (ull)t.post, r.wave ? "wave" : "thread", (ull)r.nchunks, (ull)r.chunk_len, t.wave ? "wave" : "thread", (ull)t.nchunks, (ull)t.chunk_len);
        ext_reached[r.wave ? 0 : 1][r.nchunks == 1 ? 0 : r.nchunks <= 256 ? 1 : 2] = true;
    }
    for (int w = 0; w < 2; ++w)
        for (int n = 0; n < 3; ++n) CHECK(ext_reached[w][n], "cumext %s form with %s is in no row", w == 0 ? "wave" : "thread", n == 0 ? "one chunk" : n == 1 ? "2 .. 256 chunks" : "more than 256 chunks");
    for (int cus : {256, 128, 64})
        for (uint64_t pre : extents)
            for (uint64_t post : extents)
                for (uint64_t len : {1ull, 255ull, 511ull, 512ull, 600ull, 5000ull, 70001ull, 300000ull}) {
                    const CumextRoute r = route_cumextreme(pre, len, post, cus);
                    const LegacyExt o = legacy_cumext(pre, len, post, (uint64_t)cus);
                    CHECK(r.valid && r.wave == o.wave && r.nchunks == o.nchunks && r.chunk_len == o.chunk_len && r.grid == o.grid && r.launches == o.launches && r.block == 256,
                          "cumext [%llu,%llu,%llu] on %d CUs: the route differs from the launcher's former chain", (ull)pre, (ull)len, (ull)post, cus);
                    CHECK(r.chunk_len * r.nchunks >= len && r.chunk_len * (r.nchunks - 1) < len && (!r.wave || r.chunk_len % CUMEXT_WAVE_TRIP == 0) &&
                              (uint64_t)r.grid * (r.wave ? 4 : 256) >= r.nlines * r.nchunks,
                          "cumext [%llu,%llu,%llu] on %d CUs: chunks and grid", (ull)pre, (ull)len, (ull)post, cus);
                    if (failures > 20) return 1;
                }
    CHECK(!route_cumextreme(1, 0xffffffffull, 1, 256).valid && route_cumextreme(1, 0xfffffffeull, 1, 256).valid && !route_cumextreme(0, 5, 1, 256).valid, "cumext limits");
    if (failures) return 1;
    std::puts("scan route ok");
    return 0;
}
