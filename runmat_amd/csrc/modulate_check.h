// modulate_check.h -- the pieces of modulate_constellation / modulate_bits_constellation (comms_ops.hip) that need no GPU: the verdict on
// one symbol and on one bit (simple_provider.rs:4182-4196, 4276-4290), the ordered error key, and the cut of one symbol out of the
// ballot words of a tile.  Host and device code alike; tests/cpp/modulate_check_test.cpp exercises them on the CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MOD_HD __host__ __device__
#else
#define MOD_HD
#endif

namespace rmhip {

constexpr int MOD_BLOCK = 256;              // threads per workgroup of both kernels (four waves)
constexpr int MOD_LOAD_BYTES = 16;          // symbol kernel: one load per thread and trip, 2 symbols of f64 storage, 4 of f32
constexpr int MOD_SYM_UNROLL = 4;          // symbol kernel: loads in flight per thread; a workgroup's trip is MOD_BLOCK * MOD_SYM_UNROLL loads
constexpr int MOD_BIT_TILE = 2048;          // bit kernel: input elements per workgroup and trip, a multiple of 64 (one ballot word per wave load)
constexpr int MOD_BPS_MAX = 32;             // bits per symbol served; a group reaches at most MOD_BPS_MAX - 1 elements into the next tile
constexpr int MOD_TABLE_LDS_BYTES = 16384;  // the table is staged in LDS up to this size (order <= 1024), read from global memory above

// verdict codes, in the order the CPU runs its checks
constexpr unsigned MOD_OK = 0, MOD_NOT_FINITE = 1, MOD_NOT_INTEGER = 2, MOD_OUT_OF_RANGE = 3;

// One ordered word per failing element: the CPU stops at the first failing element in traversal order and, within an element, at the
// first failing check - the minimum over all keys of a launch names both.  A group's range error carries the index of its LAST bit.
constexpr uint64_t MOD_KEY_NONE = ~0ull;
MOD_HD inline uint64_t mod_key(uint64_t index, unsigned code) { return (index << 2) | code; }
MOD_HD inline uint64_t mod_key_index(uint64_t key) { return key >> 2; }
MOD_HD inline unsigned mod_key_code(uint64_t key) { return (unsigned)(key & 3); }

// Nearest integer.  The CPU rounds halves away from zero, this rounds them to even: only values within 1e-9 of an integer pass the
// check that follows, and for those (and for every |v| >= 2^52) the two agree.
MOD_HD inline double mod_round(double v) { return __builtin_rint(v); }

// simple_provider.rs:4183-4196.  `order` is the table's point count as a double (exact below 2^53); the comparison happens in floating
// point and the integer is formed only after it passed, so 1e300 is "in range", never a wrapped index.  *symbol is written on MOD_OK only.
MOD_HD inline unsigned mod_symbol_check(double v, double order, uint64_t* symbol) {
    if (!__builtin_isfinite(v)) return MOD_NOT_FINITE;
    const double r = mod_round(v);
    if (!(__builtin_fabs(v - r) <= 1e-9 && r >= 0.0)) return MOD_NOT_INTEGER;
    if (!(r < order)) return MOD_OUT_OF_RANGE;
    *symbol = (uint64_t)r;  // -0.0 is symbol 0
    return MOD_OK;
}

// simple_provider.rs:4276-4284.  *bit is written on MOD_OK only.
MOD_HD inline unsigned mod_bit_check(double v, unsigned* bit) {
    if (!__builtin_isfinite(v)) return MOD_NOT_FINITE;
    const double r = mod_round(v);
    if (!(__builtin_fabs(v - r) <= 1e-9 && (r == 0.0 || r == 1.0))) return MOD_NOT_INTEGER;
    *bit = r == 1.0 ? 1u : 0u;
    return MOD_OK;
}

MOD_HD inline uint32_t mod_reverse32(uint32_t x) {
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// words[w] bit l is the bit value of tile element 64 * w + l (a wave's ballot: lane l is bit l).  The symbol of the group whose first
// bit is tile element `offset` (< MOD_BIT_TILE), most significant bit first, 1 <= bps <= MOD_BPS_MAX.  Reads words[offset / 64] and,
// when the group straddles, words[offset / 64 + 1]: the caller keeps one word beyond the tile's own.
MOD_HD inline uint32_t mod_cut_symbol(const uint64_t* words, unsigned offset, unsigned bps) {
    const unsigned w = offset >> 6, sh = offset & 63;
    uint64_t field = words[w] >> sh;
    if (sh + bps > 64) field |= words[w + 1] << (64 - sh);
    return mod_reverse32((uint32_t)field) >> (32 - bps);  // element offset + j lands at bit bps - 1 - j; later elements fall off
}

// the groups whose FIRST bit lies in tile t, [first, last): the tile that owns them
MOD_HD inline uint64_t mod_tile_first_group(uint64_t tile, unsigned bps) { return (tile * MOD_BIT_TILE + bps - 1) / bps; }

}  // namespace rmhip
