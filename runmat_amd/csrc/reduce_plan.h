// reduce_plan.h -- launch geometry for the [pre, red, post] reduction skeletons (skel_reduce.h).
// Shared by the ahead-of-time reductions and the hipRTC fused reductions.  The cumulative scans along a dimension choose here as
// well: route_scan (cumsum / cumprod, reduce2.hip) and route_cumextreme (cummin / cummax, order_ops.hip) at the end of this file.
//
// Contrast with the reference: its generated reduction runs ONE workgroup per slice
// (crates/runmat-accelerate/src/fusion.rs:1983-2030), i.e. a single CU for `sum(x,'all')`.
// Here every shape is split until the grid covers the 256 CUs several times over, with a
// deterministic second stage.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rmhip {

struct ReducePlan {
    bool contiguous;  // kernel A (pre == 1) or kernel B
    uint64_t nslices; // pre * post
    uint64_t nsplit;  // partials per slice
    int tx;           // kernel B: threads along `pre` per block (power of two)
    unsigned gx, gy, gz;
    bool valid;       // false: geometry exceeds grid limits (caller reports UNSUPPORTED)
};

inline uint64_t ceil_div_u64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Kernel B walks `red` in nsplit chunks of ceil(red / nsplit) columns and the blocks of all chunks run in lockstep.  When a
// chunk spans a multiple of 256 KiB (power-of-two shapes: 8192 x 8192 f64 in 64 chunks = 8 MiB each) every block is at the
// same offset of its chunk at the same time; 65 chunks of 127 columns instead measured 112 -> 105 us for sum(x,2) at 8192^2
// and 115 -> 102 us at 16384 x 4096 (docs/EXPERIMENTS.md section 3.3).  The block COUNT matters
// more (plan_strided_wide); this only moves the generic kernel off its worst point.
inline uint64_t dealias_nsplit(uint64_t red, uint64_t nsplit, uint64_t column_stride_bytes, uint64_t max_split) {
    if (nsplit <= 1 || column_stride_bytes == 0) return nsplit;
    for (int tries = 0; tries < 8 && nsplit < max_split; ++tries) {
        const uint64_t chunk = ceil_div_u64(red, nsplit);
        if (chunk <= 8 || (chunk * column_stride_bytes) % (256u * 1024u) != 0) break;
        ++nsplit;
    }
    return nsplit;
}

// Requires pre >= 1 and post >= 1 (callers return early when there are no output slices).
// `elem_bytes`: storage width of the reduced tensor (8, or 4 on a precision-32 provider).
inline ReducePlan plan_reduction(uint64_t pre, uint64_t red, uint64_t post, int num_cus, unsigned elem_bytes = 8) {
    ReducePlan p{};
    if (pre == 0 || post == 0) {
        p.valid = false;
        return p;
    }
    const uint64_t target_blocks = (uint64_t)num_cus * 8;  // ~2048 blocks of 256 threads
    p.nslices = pre * post;
    if (pre == 1) {
        p.contiguous = true;
        // slices of 64 KiB and more stream with RM_ABLOCK threads, shorter ones keep RM_RBLOCK (more resident blocks hide
        // the fixed per-block reduction latency)
        const uint64_t bs = red * elem_bytes >= 65536 ? 1024 : 256;
        uint64_t max_split = ceil_div_u64(red, bs * 8);  // >= 8 elements per thread per block
        if (max_split < 1) max_split = 1;
        uint64_t want = ceil_div_u64(target_blocks, post ? post : 1);
        if (want < 1) want = 1;
        p.nsplit = want < max_split ? want : max_split;
        if (p.nsplit > 4096) p.nsplit = 4096;
        p.tx = (int)bs;  // block size of kernel A
        p.gx = (unsigned)p.nsplit;
        // slices spread over (y, z)
        uint64_t gy = post < 65535 ? post : 65535;
        if (gy < 1) gy = 1;
        p.gy = (unsigned)gy;
        p.gz = (unsigned)ceil_div_u64(post ? post : 1, gy);
    } else {
        p.contiguous = false;
        int tx = 256;
        while (tx > 1 && (uint64_t)tx / 2 >= pre) tx /= 2;  // smallest power of two >= pre, capped at 256
        p.tx = tx;
        const uint64_t bx = ceil_div_u64(pre, (uint64_t)tx);
        const uint64_t ty = 256 / tx;
        uint64_t max_split = ceil_div_u64(red, 16 * ty);  // >= 16 elements per thread
        if (max_split < 1) max_split = 1;
        uint64_t want = ceil_div_u64(target_blocks, bx * (post ? post : 1));
        if (want < 1) want = 1;
        p.nsplit = want < max_split ? want : max_split;
        p.nsplit = dealias_nsplit(red, p.nsplit, pre * elem_bytes, max_split);
        if (p.nsplit > 65535) p.nsplit = 65535;
        p.gx = (unsigned)bx;
        p.gy = (unsigned)p.nsplit;
        p.gz = (unsigned)(post ? post : 1);
    }
    p.valid = p.gz <= 65535u && p.gy <= 65535u && p.gx >= 1;
    if (!p.contiguous && post > 65535) p.valid = false;
    return p;
}

// Geometry of kernel B over 16-byte vectors (a thread owns two adjacent lines; skel_reduce.h rm_reduce_strided_v2, reduce2.hip
// k_r2_strided_v2): `bx` windows of `win` <= 256 pairs along `pre`, a block of as many waves as its window needs, THREE blocks per
// CU over (bx, nsplit, post).  Every block is a strided column walk and the blocks run in lockstep, so the block COUNT decides the
// rate, and not monotonically: sum(x,2) at 8192^2 took 104 / 100 / 86 / 101 / 93 / 96 us at 1 ... 6 blocks per CU, 113 at 8 (the
// generic kernel B's count), 130 at 16.  The number of windows is a multiple of the XCD count: workgroups go to the XCDs round robin
// in launch order (x fastest), so with bx % xcds == 0 a window - the same 4 KiB of every column - is always walked by the same XCD
// whatever the chunk, otherwise the windows rotate over the XCDs from chunk to chunk (8200 x 8192, 17 -> 24 windows: 109 -> 90 us).
// The windows are balanced in 128-byte granules, so a row count just above a multiple of 512 leaves no column of nearly empty
// blocks (8256 rows: 109 -> 86 us).  Tables: docs/EXPERIMENTS.md section 3.3.
struct StridedWidePlan {
    unsigned bx, win, threads;
    uint64_t nsplit;
};
inline StridedWidePlan plan_strided_wide(uint64_t pre, uint64_t red, uint64_t post, int num_cus, int xcds_probed, unsigned elem_bytes) {
    StridedWidePlan w{};
    const unsigned xcds = xcds_probed > 0 ? (unsigned)xcds_probed : 8u;
    const uint64_t npairs = (pre + 1) / 2;
    const bool pin = pre / 2 >= (uint64_t)xcds * 64;
    w.bx = (unsigned)ceil_div_u64(npairs, 256);
    if (pin) w.bx = (w.bx + xcds - 1) / xcds * xcds;
    w.win = (unsigned)((ceil_div_u64(npairs, w.bx) + 7) / 8 * 8);
    if (w.win > 256) w.win = 256;
    w.bx = (unsigned)ceil_div_u64(npairs, w.win);
    if (pin) w.bx = (w.bx + xcds - 1) / xcds * xcds;  // (trailing windows may be empty)
    w.threads = (w.win + 63) / 64 * 64;
    uint64_t want = ceil_div_u64((uint64_t)num_cus * 3, (uint64_t)w.bx * (post ? post : 1));
    const uint64_t max_split = ceil_div_u64(red, 16);
    w.nsplit = want < 1 ? 1 : want;
    if (w.nsplit > max_split) w.nsplit = max_split;
    if (w.nsplit < 1) w.nsplit = 1;  // red == 0: one (empty) chunk per slice, the finalize writes the empty reduction's value
    w.nsplit = dealias_nsplit(red, w.nsplit, pre * elem_bytes, max_split);
    if (w.nsplit > 65535) w.nsplit = 65535;
    return w;
}

// ---- which kernel serves a [pre, red, post] reduction, with how many partials per slice, on which grid, and which finalize ----
// The one place where a reduction launcher chooses: run_reduce (reduce_kernels.hip), run_r2 (reduce2.hip) and rmhip_fused_reduction
// (rmhip_ops.cpp) switch over the route's kernel and launch what it says.  A pure function of the shape, the device's CU / XCD
// counts, the storage width, the operands' alignment and the caller's kernel family, so tests/cpp/reduce_route_check.cpp pins every
// family's choice without a GPU.
enum class ReduceKernel { SHORT, CONTIG, CONTIG_V2, CONTIG_V2_ODD, STRIDED, STRIDED_V2, STRIDED_V2_ODD };
inline const char* reduce_kernel_name(ReduceKernel k) {
    switch (k) {
        case ReduceKernel::SHORT: return "short";
        case ReduceKernel::CONTIG: return "contig";
        case ReduceKernel::CONTIG_V2: return "contig_v2";
        case ReduceKernel::CONTIG_V2_ODD: return "contig_v2_odd";
        case ReduceKernel::STRIDED: return "strided";
        case ReduceKernel::STRIDED_V2: return "strided_v2";
        case ReduceKernel::STRIDED_V2_ODD: return "strided_v2_odd";
    }
    return "?";
}
// What a caller's kernel family can do.  The families differ where their kernels were measured apart; the route keeps each as it is.
struct ReduceFamily {
    bool short_tile;        // has the SHORT kernel (a tile of short contiguous slices per block)
    uint64_t wide_a_from;   // kernel A runs over 16-byte vectors from this slice length on
    bool odd_pairs;         // has the unaligned-pair (ODD) forms; without them such shapes take CONTIG / STRIDED
    bool wide_b;            // has kernel B over 16-byte vectors
    bool lanes_256;         // kernel A in 256-thread blocks whatever the slice length (its nsplit still the plan's), and the narrow
                            // kernel B with 256 lanes along `pre` and no rows along `red`
    bool flat_many_slices;  // the finalize's second flat clause (<= 32 partials from 16384 slices)
};
constexpr ReduceFamily REDUCE_PLAIN{true, 2048, true, true, false, true};         // run_reduce over one tensor
constexpr ReduceFamily REDUCE_DOT{true, 2048, false, false, false, false};        // run_reduce over the product of two
constexpr ReduceFamily REDUCE_ACCUMULATOR{true, 1024, true, true, true, true};    // reduce2.hip run_r2
constexpr ReduceFamily REDUCE_GENERATED{false, 2048, false, true, false, false};  // rmhip_fused_reduction (hipRTC kernels)

static constexpr unsigned REDUCE_SHORT_TILE = 4096;  // elements of a SHORT block's LDS tile
// Many slices with a handful of partials each: one thread per slice (the flat finalize) instead of one wave.
inline bool reduce_flat_final(uint64_t nsplit, uint64_t nslices, const ReduceFamily& fam) {
    return (nsplit <= 8 && nslices >= 1024) || (fam.flat_many_slices && nsplit <= 32 && nslices >= 16384);
}
struct ReduceRoute {
    bool valid;  // false: the geometry exceeds the grid limits (the caller reports UNSUPPORTED)
    ReduceKernel kernel;
    uint64_t nslices;  // pre * post
    uint64_t nsplit;   // partials per slice as the kernel and the finalize see them
    bool flat_final;
    unsigned gx, gy, gz, block;  // stage 1's launch
    unsigned span;  // the kernel's geometry argument - SHORT: slices per block; STRIDED: lanes along `pre`; STRIDED_V2*: pairs per window
};
// `aligned`: every operand's base address is a multiple of what the family's pair loads need (the caller's test).
inline ReduceRoute route_reduction(uint64_t pre, uint64_t red, uint64_t post, int num_cus, int xcds, unsigned elem_bytes, bool aligned,
                                   const ReduceFamily& fam) {
    ReduceRoute r{};
    const ReducePlan p = plan_reduction(pre, red, post, num_cus, elem_bytes);
    r.valid = p.valid;
    if (!r.valid) return r;
    r.nslices = p.nslices;
    r.nsplit = p.nsplit;
    r.gx = p.gx;
    r.gy = p.gy;
    r.gz = p.gz;
    const bool pairs = aligned && ((p.contiguous ? red : pre) & 1) == 0;  // else the ODD form: unaligned pairs, one element left over
    if (p.contiguous) {
        r.block = fam.lanes_256 ? 256u : (unsigned)p.tx;
        if (fam.short_tile && red >= 1 && red < 256 && p.nslices >= 1024) {
            r.kernel = ReduceKernel::SHORT;
            r.nsplit = 1;
            r.span = REDUCE_SHORT_TILE / (unsigned)red < 256 ? REDUCE_SHORT_TILE / (unsigned)red : 256;
            r.gx = (unsigned)ceil_div_u64(p.nslices, r.span);
            r.gy = r.gz = 1;
            r.block = 256;
        } else if (red >= fam.wide_a_from && (pairs || fam.odd_pairs))
            r.kernel = pairs ? ReduceKernel::CONTIG_V2 : ReduceKernel::CONTIG_V2_ODD;
        else
            r.kernel = ReduceKernel::CONTIG;
    } else if (fam.wide_b && pre >= 512 && post <= 65535 && (pairs || fam.odd_pairs)) {
        const StridedWidePlan w = plan_strided_wide(pre, red, post, num_cus, xcds, elem_bytes);
        r.kernel = pairs ? ReduceKernel::STRIDED_V2 : ReduceKernel::STRIDED_V2_ODD;
        r.nsplit = w.nsplit;
        r.gx = w.bx;
        r.gy = (unsigned)w.nsplit;
        r.gz = (unsigned)post;
        r.block = w.threads;
        r.span = w.win;
    } else {
        r.kernel = ReduceKernel::STRIDED;
        r.block = 256;
        r.span = (unsigned)p.tx;
        if (fam.lanes_256) {
            r.span = 256;
            r.gx = (unsigned)ceil_div_u64(pre, 256);
            const uint64_t want = ceil_div_u64((uint64_t)num_cus * 8, (uint64_t)r.gx * post), max_split = ceil_div_u64(red, 16);
            r.nsplit = want > max_split ? max_split : want;
            if (r.nsplit < 1) r.nsplit = 1;
            r.nsplit = dealias_nsplit(red, r.nsplit, pre * elem_bytes, max_split);
            if (r.nsplit > 65535) r.nsplit = 65535;
            r.gy = (unsigned)r.nsplit;
        }
    }
    r.flat_final = reduce_flat_final(r.nsplit, r.nslices, fam);
    return r;
}

// ---- which kernel serves a cumulative sum / product over [pre, len, post], in how many chunks, on which grid, in how many launches ----
// launch_cumulative (reduce2.hip) switches over this and launches what it says; tests/cpp/scan_route_check.cpp pins it without a GPU.
//   LINES_64x32 / LINES_256x8  one thread per strided line (blocks of 64 threads with 32 loads in flight, or 256 with 8)
//   STAGED   few long strided lines: a block walks `lines_per_block` adjacent lines in LDS tiles of SCAN_STAGED_STEPS steps; lines of
//            4096 steps and more on a quarter of the CUs or fewer are cut into `nchunks` chunks of `chunk_steps` (grid z) and take
//            three launches: chunk totals, k_scan_carries, the scan from the carries
//   SHORT    contiguous lines below 256 elements: `per_block` lines per block in an LDS tile
//   CHUNKS   contiguous lines from 256 elements on: chunks of SCAN_CHUNK elements (grid x), lines over grid (y, z); three launches
//            when a line has more than one chunk
// A chunked STAGED scan always has 32 lines per block: 64 lines per block need ceil(pre / 64) * post >= num_cus line blocks, chunks
// need four times the line blocks to be at most num_cus.
enum class ScanKernel { LINES_64x32, LINES_256x8, STAGED, SHORT, CHUNKS };
inline const char* scan_kernel_name(ScanKernel k) {
    switch (k) {
        case ScanKernel::LINES_64x32: return "lines_64x32";
        case ScanKernel::LINES_256x8: return "lines_256x8";
        case ScanKernel::STAGED: return "staged";
        case ScanKernel::SHORT: return "short";
        case ScanKernel::CHUNKS: return "chunks";
    }
    return "?";
}
static constexpr unsigned SCAN_STAGED_STEPS = 64, SCAN_STAGED_THREADS = 512;  // a STAGED tile's steps, its block
static constexpr unsigned SCAN_SHORT_TILE = 4096;                             // elements of a SHORT block's LDS tile
static constexpr unsigned SCAN_BLOCK = 256;                                   // SHORT, CHUNKS and the carry kernel
static constexpr uint64_t SCAN_CHUNK = 8 * SCAN_BLOCK * 8;                    // 16384: eight tiles of 256 threads x 8 elements
struct ScanRoute {
    bool valid;  // false: no lines, or the contiguous lines exceed the grid limits (the caller reports UNSUPPORTED)
    ScanKernel kernel;
    unsigned lines_per_block;  // STAGED: 32 or 64
    uint64_t nlines;           // pre * post (the carry kernel's grid)
    uint64_t nchunks;          // STAGED, CHUNKS: chunks per line (1 elsewhere)
    uint64_t chunk_steps;      // STAGED: steps per chunk, a multiple of SCAN_STAGED_STEPS; CHUNKS: SCAN_CHUNK
    unsigned per_block;        // SHORT: lines per block
    unsigned gx, gy, gz, block;
    unsigned launches;         // 1, or 3 with more than one chunk per line
};
inline ScanRoute route_scan(uint64_t pre, uint64_t len, uint64_t post, int num_cus) {
    ScanRoute r{};
    if (pre == 0 || len == 0 || post == 0) return r;
    const uint64_t cus = (uint64_t)num_cus;
    r.valid = true;
    r.nlines = pre * post;
    r.nchunks = 1;
    r.launches = 1;
    r.gx = r.gy = r.gz = 1;
    if (pre > 1) {
        if (pre >= 8 && len >= 256 && r.nlines < cus * 256 && post <= 65535) {  // few long lines: staged tiles
            const bool half = pre < 64 || ceil_div_u64(pre, 64) * post < cus;   // 64 lines per block would leave CUs (or lanes) idle
            r.kernel = ScanKernel::STAGED;
            r.lines_per_block = half ? 32 : 64;
            const uint64_t line_blocks = ceil_div_u64(pre, r.lines_per_block) * post;
            r.chunk_steps = ceil_div_u64(len, SCAN_STAGED_STEPS) * SCAN_STAGED_STEPS;
            // a quarter of the CUs or fewer would run chains of len steps: chunks along the line (never with 64 lines per block)
            if (half && line_blocks * 4 <= cus && len >= 4096) {
                uint64_t want = ceil_div_u64(cus * 4, line_blocks), most = len / 1024;  // chunks of >= 1024 steps
                if (want > most) want = most;
                if (want > 65535) want = 65535;
                if (want > 1) {
                    r.chunk_steps = ceil_div_u64(ceil_div_u64(len, want), SCAN_STAGED_STEPS) * SCAN_STAGED_STEPS;
                    r.nchunks = ceil_div_u64(len, r.chunk_steps);
                }
            }
            r.gx = (unsigned)ceil_div_u64(pre, r.lines_per_block);
            r.gy = (unsigned)post;
            r.gz = (unsigned)r.nchunks;
            r.block = SCAN_STAGED_THREADS;
        } else if (r.nlines >= cus * 1024) {  // plenty of lines: four waves per block, eight loads deep
            r.kernel = ScanKernel::LINES_256x8;
            r.gx = (unsigned)ceil_div_u64(r.nlines, 256);
            r.block = 256;
        } else {
            r.kernel = ScanKernel::LINES_64x32;
            r.gx = (unsigned)ceil_div_u64(r.nlines, 64);
            r.block = 64;
        }
    } else if (len < 256) {  // short contiguous lines: a tile of lines per block, a thread per line
        r.kernel = ScanKernel::SHORT;
        r.per_block = (unsigned)(SCAN_SHORT_TILE / len);
        if (r.per_block > SCAN_BLOCK) r.per_block = SCAN_BLOCK;
        r.gx = (unsigned)ceil_div_u64(r.nlines, r.per_block);
        r.block = SCAN_BLOCK;
    } else {  // long contiguous lines: blocked scans over chunks (a line of one chunk: the last pass only)
        r.kernel = ScanKernel::CHUNKS;
        const uint64_t gy = r.nlines < 65535 ? r.nlines : 65535, gz = ceil_div_u64(r.nlines, gy);
        if (gz > 65535) {
            r.valid = false;
            return r;
        }
        r.chunk_steps = SCAN_CHUNK;
        r.nchunks = ceil_div_u64(len, SCAN_CHUNK);
        r.gx = (unsigned)r.nchunks;
        r.gy = (unsigned)gy;
        r.gz = (unsigned)gz;
        r.block = SCAN_BLOCK;
    }
    if (r.nchunks > 1) r.launches = 3;
    return r;
}

// ---- cummin / cummax (order_ops.hip launch_cumextreme): one wave (pre == 1) or one thread per (line, chunk) ----
// Enough independent pieces for the device - eight waves per CU of wave pieces, two waves per SIMD of thread pieces - in chunks of
// 256 elements and more; a wave's chunk is a multiple of its trip of CUMEXT_WAVE_TRIP elements.  More than one chunk per line: three
// launches (chunk summaries, k_cumext_carries, the scan from the carries).
static constexpr unsigned CUMEXT_WAVE_TRIP = 64 * 4;
struct CumextRoute {
    bool valid;  // false: no lines, or a dimension whose positions do not fit 32 bits (the caller reports UNSUPPORTED)
    bool wave;
    uint64_t nlines, nchunks, chunk_len;
    unsigned grid, block;
    unsigned launches;
};
inline CumextRoute route_cumextreme(uint64_t pre, uint64_t len, uint64_t post, int num_cus) {
    CumextRoute r{};
    r.nlines = pre * post;
    if (r.nlines == 0 || len == 0 || len >= 0xffffffffull) return r;
    r.valid = true;
    r.wave = pre == 1;
    const uint64_t want = r.wave ? (uint64_t)num_cus * 8 : (uint64_t)num_cus * 512;
    r.nchunks = 1;
    if (r.nlines < want && len >= 512) {
        r.nchunks = ceil_div_u64(want, r.nlines);
        if (r.nchunks > len / 256) r.nchunks = len / 256;
        if (r.nchunks > 8192) r.nchunks = 8192;
    }
    r.chunk_len = ceil_div_u64(len, r.nchunks);
    if (r.wave) r.chunk_len = ceil_div_u64(r.chunk_len, CUMEXT_WAVE_TRIP) * CUMEXT_WAVE_TRIP;
    r.nchunks = ceil_div_u64(len, r.chunk_len);
    const uint64_t pieces = r.nlines * r.nchunks;
    r.grid = (unsigned)(r.wave ? ceil_div_u64(pieces, 4) : ceil_div_u64(pieces, 256));
    r.block = 256;
    r.launches = r.nchunks > 1 ? 3 : 1;
    return r;
}

}  // namespace rmhip
