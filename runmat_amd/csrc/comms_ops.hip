// comms_ops.hip -- the two modulation hooks behind qammod / pskmod on a resident tensor: symbols or bits in, constellation points out.
//   modulate_constellation        crates/runmat-accelerate-api/src/lib.rs:1961-1968   (simple_provider.rs:4143-4208)
//   modulate_bits_constellation   lib.rs:1970-1977                                    (simple_provider.rs:4210-4310)
// The CPU provider is the contract.  Results are copies of table entries: bit-exact.  The table (order points, re / im interleaved) is
// staged once per workgroup into LDS while it fits MOD_TABLE_LDS_BYTES and read from global memory above that: one kernel body, a
// template switch.  16 KiB lets eight workgroups of 256 threads - the CU's 32 waves - stay resident in its 160 KiB.
// Validation happens on the device, in the same pass (modulate_check.h): every failing element forms the key (index << 2) | code, the
// launch keeps the minimum - per thread, per wave by shuffles, then one 64-bit atomicMin per failing wave on a word the host set to
// all ones - and the host reads that word once.  The minimum does not depend on scheduling: it IS the element the CPU's loop stops
// at, with the check it stops on.  A value that fails never indexes the table; its output is zeros (the host frees the output).
// Byte model: symbols 8 B in + 16 B out per sample (4 + 16 on f32 storage); bits 8 * bps B in + 16 B out per symbol.
#include "common.h"
#include "modulate_check.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

static_assert(MOD_BIT_TILE % 64 == 0 && MOD_BLOCK % 64 == 0, "a wave load is one ballot word");
static_assert(MOD_BPS_MAX <= 32, "a symbol is cut out of 32 bits");
constexpr int MOD_WORDS = MOD_BIT_TILE / 64 + 1;  // the tile's ballot words and one more for the group that straddles its end
constexpr u64 MOD_TABLE_LDS_POINTS = MOD_TABLE_LDS_BYTES / sizeof(v2d);

template <class T>
struct LoadOf;
template <>
struct LoadOf<double> {
    typedef v2d type;
};
template <>
struct LoadOf<float> {
    typedef v4f type;
};

// Every thread calls this once, at the end of its kernel: the smallest key of the wave, then one atomic per failing wave.
__device__ __forceinline__ void report_key(u64 key, u64* __restrict__ verdict) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key != MOD_KEY_NONE) atomicMin(verdict, key);
}

// the table this workgroup reads: its LDS copy (LDS_TABLE: order <= MOD_TABLE_LDS_POINTS, the host's choice) or the global one
template <bool LDS_TABLE>
__device__ __forceinline__ const v2d* stage_table(const v2d* __restrict__ table, u64 order) {
    if constexpr (LDS_TABLE) {
        __shared__ v2d staged[MOD_TABLE_LDS_POINTS];
        for (u64 i = threadIdx.x; i < order; i += MOD_BLOCK) staged[i] = table[i];
        __syncthreads();
        return staged;
    } else {
        return table;
    }
}

__device__ __forceinline__ v2d symbol_point(double v, double order, const v2d* tab, u64 index, u64& key) {
    uint64_t symbol = 0;
    const unsigned code = mod_symbol_check(v, order, &symbol);
    v2d p = {0.0, 0.0};
    if (code == MOD_OK) p = tab[symbol];
    else {
        const u64 k = mod_key(index, code);
        key = k < key ? k : key;
    }
    return p;
}

// ---- symbols: MOD_SYM_UNROLL 16-byte loads per thread and trip (2 symbols each of f64 storage, 4 of f32), one 16-byte store per symbol ----
// The loads of a trip are issued together; a wave's load covers 64 * N consecutive symbols, lane t holding symbols N t .. N t + N - 1.
// Stored that way each store instruction would write every other 16 bytes of its span, so the lanes first exchange their validated
// 32-bit symbol numbers (N * N shuffles): store j of the wave then writes symbols 64 j .. 64 j + 63 of the chunk, one contiguous KiB.
// `vec` == 0 (an input base that is not 16-byte aligned): every element goes through the scalar loop, which otherwise takes the tail
// and is coalesced as it is (one element per lane).
constexpr uint32_t MOD_NO_SYMBOL = 0xffffffffu;  // a failed element: its output is zeros (the host refuses orders beyond 2^32 - 1)

template <class T, bool LDS_TABLE>
__global__ void __launch_bounds__(MOD_BLOCK) k_modulate_symbols(const T* __restrict__ in, const v2d* __restrict__ table, u64 order, u64 n, int vec,
                                                                v2d* __restrict__ out, u64* __restrict__ verdict) {
    typedef typename LoadOf<T>::type V;
    constexpr int N = MOD_LOAD_BYTES / sizeof(T);
    constexpr u64 TRIP = (u64)MOD_SYM_UNROLL * MOD_BLOCK;  // vectors per workgroup and trip
    const v2d* tab = stage_table<LDS_TABLE>(table, order);
    const double dorder = (double)order;
    const unsigned lane = threadIdx.x & 63;
    const u64 nvec = vec ? n / N : 0;
    u64 key = MOD_KEY_NONE;
    for (u64 b = (u64)blockIdx.x * TRIP; b < nvec; b += (u64)gridDim.x * TRIP) {  // block-uniform: every lane reaches the shuffles
        V v[MOD_SYM_UNROLL];
#pragma unroll
        for (int u = 0; u < MOD_SYM_UNROLL; ++u) {
            const u64 i = b + (u64)u * MOD_BLOCK + threadIdx.x;
            v[u] = V{};
            if (i < nvec) v[u] = __builtin_nontemporal_load((const V*)in + i);
        }
#pragma unroll
        for (int u = 0; u < MOD_SYM_UNROLL; ++u) {
            const u64 i = b + (u64)u * MOD_BLOCK + threadIdx.x;
            uint32_t mine[N];
#pragma unroll
            for (int l = 0; l < N; ++l) {
                mine[l] = MOD_NO_SYMBOL;
                if (i < nvec) {
                    uint64_t symbol = 0;
                    const unsigned code = mod_symbol_check((double)v[u][l], dorder, &symbol);
                    if (code == MOD_OK) mine[l] = (uint32_t)symbol;
                    else {
                        const u64 k = mod_key(i * N + l, code);
                        key = k < key ? k : key;
                    }
                }
            }
            const u64 chunk = (i - lane) * N;  // the first symbol of this wave's load
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int src = (64 * j + (int)lane) / N;
                uint32_t symbol = MOD_NO_SYMBOL;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint32_t theirs = (uint32_t)__shfl((int)mine[k], src);
                    if ((int)(lane % N) == k) symbol = theirs;
                }
                const u64 e = chunk + 64 * j + lane;
                if (e < nvec * N) {
                    v2d p = {0.0, 0.0};
                    if (symbol != MOD_NO_SYMBOL) p = tab[symbol];
                    __builtin_nontemporal_store(p, out + e);
                }
            }
        }
    }
    const u64 stride = (u64)gridDim.x * MOD_BLOCK;
    for (u64 i = nvec * N + (u64)blockIdx.x * MOD_BLOCK + threadIdx.x; i < n; i += stride) out[i] = symbol_point((double)in[i], dorder, tab, i, key);
    report_key(key, verdict);
}

// ---- bits: the input is a flat stream of groups of `bps` elements (input_rows is a multiple of bps), most significant bit first ----
// Per tile of MOD_BIT_TILE elements: every wave loads 64 consecutive elements at a time, one per lane - its MOD_WAVE_WORDS loads of a tile
// issued together - and its ballot of the bit values is one word in LDS; then each thread cuts the symbols of the groups whose first bit
// lies in the tile out of those words (mod_cut_symbol), looks the point up and stores 16 bytes.  The last group of a tile may reach up
// to bps - 1 elements into the next one: wave 0 loads one more word (its first MOD_BPS_MAX lanes only) for it.  Those elements are
// validated twice, with the same key.  A failed bit counts as 0: its group's symbol is still compared against the order before it
// indexes the table, and a range error it may cause carries the index of the group's last bit, so the bit's own key is the smaller one.
constexpr int MOD_WAVE_WORDS = MOD_BIT_TILE / 64 / (MOD_BLOCK / 64);
static_assert(MOD_WAVE_WORDS * (MOD_BLOCK / 64) * 64 == MOD_BIT_TILE, "the waves share a tile's words evenly");

template <class T>
__device__ __forceinline__ unsigned judged_bit(T value, u64 e, u64& key) {
    unsigned bit = 0;
    const unsigned code = mod_bit_check((double)value, &bit);
    if (code != MOD_OK) {
        const u64 k = mod_key(e, code);
        key = k < key ? k : key;
    }
    return bit;
}

template <class T, bool LDS_TABLE>
__global__ void __launch_bounds__(MOD_BLOCK) k_modulate_bits(const T* __restrict__ in, const v2d* __restrict__ table, u64 order, u64 n, unsigned bps, u64 nsym,
                                                             u64 ntiles, v2d* __restrict__ out, u64* __restrict__ verdict) {
    __shared__ uint64_t words[MOD_WORDS];
    const v2d* tab = stage_table<LDS_TABLE>(table, order);
    const double dorder = (double)order;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 key = MOD_KEY_NONE;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 base = t * MOD_BIT_TILE;
        T value[MOD_WAVE_WORDS];
#pragma unroll
        for (int j = 0; j < MOD_WAVE_WORDS; ++j) {
            const u64 e = base + (u64)(wave + j * (MOD_BLOCK / 64)) * 64 + lane;
            value[j] = (T)0;  // beyond the input: a zero bit nobody reads
            if (e < n) value[j] = __builtin_nontemporal_load(in + e);
        }
#pragma unroll
        for (int j = 0; j < MOD_WAVE_WORDS; ++j) {
            const unsigned w = wave + j * (MOD_BLOCK / 64);
            const unsigned bit = judged_bit(value[j], base + (u64)w * 64 + lane, key);
            const u64 mask = __ballot(bit != 0);
            if (lane == 0) words[w] = mask;
        }
        if (wave == 0) {  // wave-uniform
            const u64 e = base + MOD_BIT_TILE + lane;
            unsigned bit = 0;
            if (e < n && lane < (unsigned)MOD_BPS_MAX) bit = judged_bit(in[e], e, key);
            const u64 mask = __ballot(bit != 0);
            if (lane == 0) words[MOD_WORDS - 1] = mask;
        }
        __syncthreads();
        const u64 g0 = mod_tile_first_group(t, bps);
        u64 g1 = mod_tile_first_group(t + 1, bps);
        g1 = g1 < nsym ? g1 : nsym;
        for (u64 g = g0 + threadIdx.x; g < g1; g += MOD_BLOCK) {
            const u64 first = g * bps;
            const uint32_t symbol = mod_cut_symbol(words, (unsigned)(first - base), bps);
            v2d p = {0.0, 0.0};
            if ((double)symbol < dorder) p = tab[symbol];
            else {
                const u64 k = mod_key(first + bps - 1, MOD_OUT_OF_RANGE);
                key = k < key ? k : key;
            }
            __builtin_nontemporal_store(p, out + g);
        }
        __syncthreads();  // the next trip overwrites the words
    }
    report_key(key, verdict);
}

inline unsigned modulate_grid(const Context* c, u64 work_groups) {
    const u64 cap = (u64)c->num_cus * 8;  // what is resident at once; the kernels loop over the rest, staging the table once
    return (unsigned)(work_groups < 1 ? 1 : (work_groups < cap ? work_groups : cap));
}

}  // namespace

template <class T>
static int launch_symbols(Context* c, const T* in, const double* table, size_t order, size_t n, double* out, unsigned long long* verdict) {
    constexpr int N = MOD_LOAD_BYTES / sizeof(T);
    const int vec = ((uintptr_t)in & (MOD_LOAD_BYTES - 1)) == 0;
    // a workgroup's trip is MOD_SYM_UNROLL loads per thread; the scalar loop (the tail, or everything when `vec` is 0) strides by the grid
    const u64 per_group = vec ? (u64)MOD_SYM_UNROLL * MOD_BLOCK * N : (u64)MOD_BLOCK;
    const dim3 grid(modulate_grid(c, (n + per_group - 1) / per_group)), block(MOD_BLOCK);
    if (order <= MOD_TABLE_LDS_POINTS)
        hipLaunchKernelGGL((k_modulate_symbols<T, true>), grid, block, 0, c->stream, in, (const v2d*)table, (u64)order, (u64)n, vec, (v2d*)out, verdict);
    else
        hipLaunchKernelGGL((k_modulate_symbols<T, false>), grid, block, 0, c->stream, in, (const v2d*)table, (u64)order, (u64)n, vec, (v2d*)out, verdict);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    c->record_launch("modulate_symbols", {{"n", n}, {"order", order}}, {{"lds_table", order <= MOD_TABLE_LDS_POINTS ? 1u : 0u}, {"vec", (uint64_t)vec}});
    return RMHIP_OK;
}

template <class T>
static int launch_bits(Context* c, const T* in, const double* table, size_t order, size_t n, unsigned bps, double* out, unsigned long long* verdict) {
    const u64 nsym = n / bps, ntiles = (n + MOD_BIT_TILE - 1) / MOD_BIT_TILE;
    const dim3 grid(modulate_grid(c, ntiles)), block(MOD_BLOCK);
    if (order <= MOD_TABLE_LDS_POINTS)
        hipLaunchKernelGGL((k_modulate_bits<T, true>), grid, block, 0, c->stream, in, (const v2d*)table, (u64)order, (u64)n, bps, nsym, ntiles, (v2d*)out, verdict);
    else
        hipLaunchKernelGGL((k_modulate_bits<T, false>), grid, block, 0, c->stream, in, (const v2d*)table, (u64)order, (u64)n, bps, nsym, ntiles, (v2d*)out, verdict);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    c->record_launch("modulate_bits", {{"n", n}, {"order", order}, {"bps", bps}}, {{"lds_table", order <= MOD_TABLE_LDS_POINTS ? 1u : 0u}});
    return RMHIP_OK;
}

int launch_modulate_symbols(Context* c, const void* in, bool f32, const double* table, size_t order, size_t n, double* out, unsigned long long* verdict) {
    return f32 ? launch_symbols<float>(c, (const float*)in, table, order, n, out, verdict) : launch_symbols<double>(c, (const double*)in, table, order, n, out, verdict);
}

int launch_modulate_bits(Context* c, const void* in, bool f32, const double* table, size_t order, size_t n, unsigned bps, double* out, unsigned long long* verdict) {
    return f32 ? launch_bits<float>(c, (const float*)in, table, order, n, bps, out, verdict) : launch_bits<double>(c, (const double*)in, table, order, n, bps, out, verdict);
}

}  // namespace rmhip
