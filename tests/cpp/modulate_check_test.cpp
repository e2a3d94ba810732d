// Host-side check of runmat_amd/csrc/modulate_check.h, the pieces of the modulation kernels that need no GPU.
//   modulate_check_test                         self-checks: key order, bit reversal, the cut of a symbol out of ballot words for every
//                                               bits-per-symbol and every offset (straddling words and the tile's end included) against
//                                               a bit-by-bit reading, tile ownership of groups; prints "modulate check ok"
//   modulate_check_test symbols ORDER HEX...    one line "code symbol" per value (a double given as the 16 hex digits of its bits)
//   modulate_check_test bits HEX...             one line "code bit" per value
// tests/test_comms_host.py compares the two listing modes with the Python restatement of the CPU loops on the edge values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "modulate_check.h"

using namespace rmhip;

static double from_hex(const char* s) {
    const uint64_t u = std::strtoull(s, nullptr, 16);
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

static int fails = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++fails;                                                     \
        }                                                                \
    } while (0)

static uint64_t next_random(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s ^ (s >> 29);
}

static void self_check() {
    // keys: index before code, and a group's range error (code 3 at its last bit) after that bit's own checks and before the next element
    EXPECT(mod_key(5, MOD_NOT_FINITE) < mod_key(5, MOD_NOT_INTEGER) && mod_key(5, MOD_NOT_INTEGER) < mod_key(5, MOD_OUT_OF_RANGE));
    EXPECT(mod_key(5, MOD_OUT_OF_RANGE) < mod_key(6, MOD_NOT_FINITE) && mod_key(0, MOD_NOT_FINITE) < MOD_KEY_NONE);
    EXPECT(mod_key_index(mod_key(1ull << 40, 2)) == 1ull << 40 && mod_key_code(mod_key(1ull << 40, 2)) == 2);
    EXPECT(mod_key((1ull << 61) + 7, 3) < MOD_KEY_NONE);
    EXPECT(mod_reverse32(1u) == 0x80000000u && mod_reverse32(0x80000000u) == 1u && mod_reverse32(0x0000ffffu) == 0xffff0000u &&
           mod_reverse32(0x12345678u) == 0x1e6a2c48u);
    EXPECT(MOD_BIT_TILE % 64 == 0 && MOD_BPS_MAX == 32 && MOD_TABLE_LDS_BYTES % 16 == 0);

    // the cut against a bit-by-bit reading: random words, every bps, every offset at which a group of the tile can start
    const int nwords = MOD_BIT_TILE / 64 + 1;
    std::vector<uint64_t> words(nwords);
    uint64_t seed = 0x243f6a8885a308d3ull;
    for (int round = 0; round < 3; ++round) {
        for (auto& w : words) w = round == 0 ? next_random(seed) : (round == 1 ? ~0ull : next_random(seed) & next_random(seed));
        for (unsigned bps = 1; bps <= (unsigned)MOD_BPS_MAX; ++bps)
            for (unsigned offset = 0; offset < (unsigned)MOD_BIT_TILE; ++offset) {
                uint64_t want = 0;
                for (unsigned j = 0; j < bps; ++j) {
                    const unsigned e = offset + j;  // < MOD_BIT_TILE + 31: inside the extra word
                    want = (want << 1) | ((words[e >> 6] >> (e & 63)) & 1);
                }
                if (mod_cut_symbol(words.data(), offset, bps) != want) {
                    std::printf("FAILED cut: bps %u offset %u\n", bps, offset);
                    ++fails;
                    offset = MOD_BIT_TILE;
                }
            }
    }
    // ownership: over consecutive tiles every group is owned exactly once, by the tile that holds its first bit
    for (unsigned bps = 1; bps <= (unsigned)MOD_BPS_MAX; ++bps) {
        EXPECT(mod_tile_first_group(0, bps) == 0);
        for (uint64_t t = 0; t < 70; ++t) {
            const uint64_t g0 = mod_tile_first_group(t, bps), g1 = mod_tile_first_group(t + 1, bps);
            EXPECT(g0 <= g1 && g0 * bps >= t * MOD_BIT_TILE && (g0 == 0 || (g0 - 1) * bps < t * MOD_BIT_TILE));
            EXPECT(g1 == g0 || ((g1 - 1) * bps < (t + 1) * MOD_BIT_TILE && (g1 - 1) * bps + bps - 1 < (t + 1) * MOD_BIT_TILE + MOD_BPS_MAX - 1));
        }
    }
    // a tile far out: no 32-bit wrap in the group arithmetic
    EXPECT(mod_tile_first_group(1ull << 40, 3) == ((1ull << 40) * MOD_BIT_TILE + 2) / 3);
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "symbols")) {
        const double order = (double)std::strtoull(argv[2], nullptr, 10);
        for (int k = 3; k < argc; ++k) {
            uint64_t symbol = ~0ull;
            const unsigned code = mod_symbol_check(from_hex(argv[k]), order, &symbol);
            if (code == MOD_OK) std::printf("0 %llu\n", (unsigned long long)symbol);
            else std::printf("%u -\n", code);
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "bits")) {
        for (int k = 2; k < argc; ++k) {
            unsigned bit = 9;
            const unsigned code = mod_bit_check(from_hex(argv[k]), &bit);
            if (code == MOD_OK) std::printf("0 %u\n", bit);
            else std::printf("%u -\n", code);
        }
        return 0;
    }
    self_check();
    if (fails) return 1;
    std::printf("modulate check ok\n");
    return 0;
}
