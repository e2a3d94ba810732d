// mode_runs.h -- the pieces of mode_values (order_ops.hip, section "mode") that need no GPU: which granularity a sorted line of `lp`
// pairs is scanned at, the order of two run candidates, and the search that closes the run left open at the end of a chunk.
// Host and device code alike; tests/cpp/mode_runs_check.cpp exercises them on the CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MODE_HD __host__ __device__
#else
#define MODE_HD
#endif

namespace rmhip {

constexpr uint64_t MODE_WAVE_LP = 256;  // up to here one wave scans a whole line (at most four rows of 64 pairs)
constexpr uint64_t MODE_CHUNK = 2048;   // beyond: one workgroup of four waves per chunk of this many pairs, a quarter each
constexpr int MODE_WAVES = 4;           // waves per workgroup of the run scan

// How the sorted lines (each padded to lp, a power of two >= 2) are cut into units of work.  A unit is one wave (wave != 0: a whole
// line) or one workgroup (a chunk); the units of a line are consecutive, so unit u covers [u % per_line * chunk, + chunk) of line
// u / per_line.
struct ModeGeom {
    int wave;           // 1: a wave per line, MODE_WAVES lines per workgroup; 0: a workgroup per chunk
    uint64_t chunk;     // pairs per unit
    uint64_t per_line;  // units per line: lp / chunk
};

MODE_HD inline ModeGeom mode_geometry(uint64_t lp) {
    ModeGeom g;
    g.wave = lp <= MODE_WAVE_LP ? 1 : 0;
    g.chunk = g.wave || lp < MODE_CHUNK ? lp : MODE_CHUNK;
    g.per_line = lp / g.chunk;
    return g;
}

// workgroups of the run scan over `nlines` lines
MODE_HD inline uint64_t mode_grid(const ModeGeom& g, uint64_t nlines) {
    return g.wave ? (nlines + MODE_WAVES - 1) / MODE_WAVES : nlines * g.per_line;
}

// A run candidate: its length and the index of its head in the sorted line, as ONE ordered word - the longer run is the better one, of
// two equally long runs the one whose head comes first (the smaller value).  0 is "no run"; a run has length >= 1.
constexpr uint32_t MODE_NONE = 0xffffffffu;
MODE_HD inline uint64_t mode_cand(uint32_t len, uint32_t head) { return ((uint64_t)len << 32) | (uint32_t)~head; }
MODE_HD inline uint32_t mode_cand_len(uint64_t c) { return (uint32_t)(c >> 32); }
MODE_HD inline uint32_t mode_cand_head(uint64_t c) { return ~(uint32_t)c; }
MODE_HD inline bool mode_cand_better(uint64_t a, uint64_t b) { return a > b; }
MODE_HD inline uint64_t mode_cand_best(uint64_t a, uint64_t b) { return mode_cand_better(b, a) ? b : a; }

// keys[lo .. hi) ascending and nothing before `lo` exceeds `key`: the first index in [lo, hi) whose key is greater than `key`, or hi.
// Doubling steps from lo, then bisection: a run that ends soon after lo costs a few probes, the longest log2(hi - lo) twice over.
template <class K>  // a 64-bit unsigned key (`unsigned long` and `unsigned long long` are distinct types)
MODE_HD inline uint64_t mode_upper_bound(const K* keys, uint64_t lo, uint64_t hi, K key) {
    uint64_t step = 1;
    while (lo < hi) {
        const uint64_t p = lo + (step - 1);
        if (p >= hi) break;
        if (keys[p] > key) {
            hi = p;
            break;
        }
        lo = p + 1;
        step <<= 1;
    }
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] > key) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace rmhip
