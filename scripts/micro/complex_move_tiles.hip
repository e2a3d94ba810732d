// Developer micro-benchmark (GPU box): the candidates of the 16-byte movers in move_kernels.h, each beside its 8-byte sibling at equal bytes.
//   transpose  8192 x 8192 complex (2 GiB moved): k_permute_tiled16 with tiles 64x64 (66 560 B of LDS), 32x64 (33 280 B), 64x32 (33 792 B) and
//              32x32 (16 896 B) against k_permute_tiled<double> on 16384 x 8192
//   circshift  by (4096, 4096) of 8192 x 8192 complex: k_index_copy<v2d, E> with E = 1, 2, 4 elements per lane against k_index_copy<double, 4>
//              on 16384 x 8192 by (8192, 4096)
// Rounds interleave every candidate (one warm-up round is dropped); per candidate the median, minimum and maximum of the per-call time over the
// rounds, and GB/s of the bytes moved (read + written) at the median.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/micro/complex_move_tiles.hip -o scripts/micro/complex_move_tiles
#include "../../runmat_amd/csrc/move_kernels.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

using namespace rmhip;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static PermParams transpose_params(unsigned long long rows, unsigned long long cols, int ti, int tj) {  // source [rows, cols] -> output [cols, rows]
    PermParams p{};
    p.rank = 2;
    p.j = 1;
    for (int d = 0; d < 8; ++d) p.shape[d] = 1;
    p.shape[0] = cols, p.shape[1] = rows;
    p.sstride[0] = rows, p.sstride[1] = 1;
    p.ostride[0] = 1, p.ostride[1] = cols;
    p.t0 = (cols + ti - 1) / ti;
    p.tj = (rows + tj - 1) / tj;
    return p;
}
static MapParams shift_params(unsigned long long rows, unsigned long long cols, unsigned long long sr, unsigned long long sc, int e) {
    MapParams p{};
    p.rank = 2;
    p.d0 = rows;
    p.id0 = 0;
    p.nchunks = (rows + 256ull * e - 1) / (256ull * e);
    for (int d = 0; d < 8; ++d) p.shape[d] = 1, p.mod[d] = 1;
    p.shape[0] = rows, p.shape[1] = cols;
    p.stride[0] = 1, p.stride[1] = rows;
    p.off[0] = (rows - sr) % rows, p.off[1] = (cols - sc) % cols;
    p.mod[0] = rows, p.mod[1] = cols;
    return p;
}
static dim3 grid_of(unsigned long long blocks) {
    const unsigned long long gx = std::min<unsigned long long>(blocks, 1048576ULL);
    return dim3((unsigned)gx, (unsigned)((blocks + gx - 1) / gx));
}

template <int TI, int TJ>
static void tiled16(const void* s, void* d, unsigned long long n, hipStream_t st) {
    const PermParams p = transpose_params(n, n, TI, TJ);
    hipLaunchKernelGGL((k_permute_tiled16<TI, TJ>), grid_of(p.t0 * p.tj), dim3(256), 0, st, (const v2d*)s, (v2d*)d, p);
}
template <class T, int E>
static void shift(const void* s, void* d, unsigned long long rows, unsigned long long cols, hipStream_t st) {
    const MapParams p = shift_params(rows, cols, rows / 2, cols / 2, E);
    hipLaunchKernelGGL((k_index_copy<T, E>), grid_of(p.nchunks * cols), dim3(256), 0, st, (const T*)s, (T*)d, p);
}

int main() {
    const unsigned long long n = 8192, bytes = n * n * 16;
    void *src, *dst;
    CHECK(hipMalloc(&src, bytes));
    CHECK(hipMalloc(&dst, bytes));
    CHECK(hipMemset(src, 0x3c, bytes));
    CHECK(hipMemset(dst, 0, bytes));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    struct Cand {
        std::string name;
        std::function<void()> run;
        std::vector<float> us;
    };
    std::vector<Cand> cands = {
        {"transpose f64 64x64 (sibling, 16384x8192)", [&] {
             const PermParams p = transpose_params(2 * n, n, 64, 64);
             hipLaunchKernelGGL((k_permute_tiled<double>), grid_of(p.t0 * p.tj), dim3(256), 0, st, (const double*)src, (double*)dst, p);
         }, {}},
        {"transpose c128 tile 64x64", [&] { tiled16<64, 64>(src, dst, n, st); }, {}},
        {"transpose c128 tile 32x64", [&] { tiled16<32, 64>(src, dst, n, st); }, {}},
        {"transpose c128 tile 64x32", [&] { tiled16<64, 32>(src, dst, n, st); }, {}},
        {"transpose c128 tile 32x32", [&] { tiled16<32, 32>(src, dst, n, st); }, {}},
        {"circshift f64 E=4 (sibling, 16384x8192)", [&] { shift<double, 4>(src, dst, 2 * n, n, st); }, {}},
        {"circshift c128 E=1", [&] { shift<v2d, 1>(src, dst, n, n, st); }, {}},
        {"circshift c128 E=2", [&] { shift<v2d, 2>(src, dst, n, n, st); }, {}},
        {"circshift c128 E=4", [&] { shift<v2d, 4>(src, dst, n, n, st); }, {}},
    };
    const int rounds = 9, reps = 10;
    for (int r = 0; r <= rounds; ++r)
        for (auto& c : cands) {
            CHECK(hipEventRecord(e0, st));
            for (int k = 0; k < reps; ++k) c.run();
            CHECK(hipEventRecord(e1, st));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipGetLastError());
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r) c.us.push_back(ms * 1000.f / reps);  // round 0 warms up
        }
    std::printf("%-44s %10s %10s %10s %10s\n", "candidate", "median us", "min us", "max us", "GB/s");
    for (auto& c : cands) {
        std::sort(c.us.begin(), c.us.end());
        const float med = c.us[c.us.size() / 2];
        std::printf("%-44s %10.1f %10.1f %10.1f %10.1f\n", c.name.c_str(), med, c.us.front(), c.us.back(), 2.0 * bytes / (med * 1e-6) / 1e9);
    }
    return 0;
}
