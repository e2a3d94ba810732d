// move_kernels.h -- the copy kernels behind repmat, permute, circshift and flip (tensor_ops.hip launches them; scripts/micro/complex_move_tiles.hip
// times the tile and per-lane candidates of the 16-byte forms).  Element types: float, double and v2d - one complex-interleaved element,
// moved by a single 16-byte load and a single 16-byte store.
#pragma once
#include <hip/hip_runtime.h>

namespace rmhip {

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {
constexpr int kBlock = 256;

struct MapParams {
    unsigned long long d0, nchunks;
    int rank;
    int id0;  // dim 0 is the identity map (off 0, mod >= extent, not reversed): no modulo per element
    unsigned long long shape[8], stride[8], off[8], mod[8];
    unsigned char rev[8];
};

__device__ __forceinline__ unsigned long long map_coord(const MapParams& p, int d, unsigned long long cd) {
    if (p.rev[d]) return p.off[d] - cd;
    unsigned long long t = p.off[d] + cd;
    if (t >= p.mod[d]) t = (t | p.mod[d]) >> 32 ? t % p.mod[d] : (unsigned long long)((unsigned)t % (unsigned)p.mod[d]);
    return t;
}

// One block: kBlock * E consecutive elements of dim 0 at one outer coordinate (E = 4, or less when dim 0 is short: a 512-element
// dim 0 on the four-element form leaves half of every block idle).
template <class T, int E>
__global__ void __launch_bounds__(kBlock) k_index_copy(const T* __restrict__ src, T* __restrict__ dst, MapParams p) {
    const unsigned long long blk = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;
    const unsigned long long chunk = blk % p.nchunks;
    const unsigned long long outer = blk / p.nchunks;
    unsigned long long base = 0, rem = outer;
    for (int d = 1; d < p.rank; ++d) {
        const unsigned long long cd = rem % p.shape[d];
        rem /= p.shape[d];
        base += map_coord(p, d, cd) * p.stride[d];
    }
    if (rem != 0) return;
    const unsigned long long obase = outer * p.d0;
    const unsigned long long i0 = chunk * (unsigned long long)(kBlock * E) + threadIdx.x;
    T v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned long long i = i0 + (unsigned long long)e * kBlock;
        if (i < p.d0) v[e] = src[base + (p.id0 ? i : map_coord(p, 0, i)) * p.stride[0]];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned long long i = i0 + (unsigned long long)e * kBlock;
        if (i < p.d0) dst[obase + i] = v[e];
    }
}

// Short dim 0 with many outer coordinates (repmat of a 1 x N row to 8 x N): flat threads over the output, 32-bit decode.
template <class T>
__global__ void __launch_bounds__(kBlock) k_index_copy_flat(const T* __restrict__ src, T* __restrict__ dst, MapParams p, unsigned n) {
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned idx = blockIdx.x * kBlock + threadIdx.x; idx < n; idx += stride) {
        unsigned rem = idx;
        unsigned long long s = 0;
        for (int d = 0; d < p.rank; ++d) {
            const unsigned sd = (unsigned)p.shape[d];
            const unsigned q = rem / sd, cd = rem - q * sd;
            rem = q;
            s += map_coord(p, d, cd) * p.stride[d];
        }
        dst[idx] = src[s];
    }
}

// ---- permutation that moves source dim 0 to output dim j > 0 -----------------------------------------------------------
// Tile = TI (output dim 0; source stride s0) x TJ (output dim j = source dim 0, stride 1).  Loads run along the source's
// contiguous dimension, stores along the output's; the transposition happens in LDS (row padding: no bank conflicts).
struct PermParams {
    int rank, j;
    unsigned long long shape[8];    // output extents
    unsigned long long sstride[8];  // source stride of every output dim (sstride[j] == 1)
    unsigned long long ostride[8];  // output strides
    unsigned long long t0, tj;      // tiles along dim 0 / dim j
};
template <class T>
__global__ void __launch_bounds__(256) k_permute_tiled(const T* __restrict__ src, T* __restrict__ dst, PermParams p) {
    __shared__ T tile[64][65];
    unsigned long long blk = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;
    // consecutive workgroups advance along the SOURCE's contiguous dimension (output dim j): their loads continue each other's 512-byte
    // row pieces (the other order - along the output's contiguous dimension - measured 275 us against 225 for 8192^2)
    const unsigned long long bj = blk % p.tj;
    blk /= p.tj;
    const unsigned long long b0 = blk % p.t0;
    unsigned long long rem = blk / p.t0;
    unsigned long long sbase = 0, obase = 0;
    for (int d = 1; d < p.rank; ++d) {
        if (d == p.j) continue;
        const unsigned long long cd = rem % p.shape[d];
        rem /= p.shape[d];
        sbase += cd * p.sstride[d];
        obase += cd * p.ostride[d];
    }
    if (rem != 0) return;
    const unsigned long long i0 = b0 * 64, j0 = bj * 64;  // tile origin: output dim 0, output dim j
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
    // load: tx runs along source dim 0 (= output dim j).  All 16 loads are issued before the first one is used (indices clamped into
    // the tensor instead of a branch per load - a guarded loop waits for every load before it issues the next: 268 us against 225 for
    // 8192^2), the stores are guarded.
    const unsigned long long jj = j0 + tx;
    const unsigned long long jc = jj < p.shape[p.j] ? jj : p.shape[p.j] - 1;
    T v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned long long ii = i0 + ty + 4 * q;
        const unsigned long long ic = ii < p.shape[0] ? ii : p.shape[0] - 1;
        v[q] = src[sbase + jc + ic * p.sstride[0]];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) tile[ty + 4 * q][tx] = v[q];
    __syncthreads();
    // store: tx runs along output dim 0
    const unsigned long long io = i0 + tx;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned long long jo = j0 + ty + 4 * q;
        if (io < p.shape[0] && jo < p.shape[p.j]) dst[obase + io + jo * p.ostride[p.j]] = tile[tx][ty + 4 * q];
    }
}

// The same pass for 16-byte elements, the tile a parameter (TI and TJ divide 256).  A row pitch of TJ + 1 elements is odd in 16-byte
// units, so the column read of the store phase (ds_read_b128: four groups of 16 lanes, each lane TJ + 1 slots after its neighbour)
// meets 16 distinct slots per group, and the row-contiguous write is conflict free as well.  What the 8-byte kernel was measured to
// need is kept: workgroups advance along the source's contiguous dimension, and every load of a thread is issued, on clamped
// indices, before the first one is used.
template <int TI, int TJ>
__global__ void __launch_bounds__(256) k_permute_tiled16(const v2d* __restrict__ src, v2d* __restrict__ dst, PermParams p) {
    constexpr int Q = TI * TJ / 256, LR = 256 / TJ, SR = 256 / TI;  // elements per thread; tile rows per load pass / per store pass
    static_assert(TI * TJ % 256 == 0 && 256 % TI == 0 && 256 % TJ == 0, "tile must split over 256 threads");
    __shared__ v2d tile[TI][TJ + 1];
    unsigned long long blk = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;
    const unsigned long long bj = blk % p.tj;
    blk /= p.tj;
    const unsigned long long b0 = blk % p.t0;
    unsigned long long rem = blk / p.t0;
    unsigned long long sbase = 0, obase = 0;
    for (int d = 1; d < p.rank; ++d) {
        if (d == p.j) continue;
        const unsigned long long cd = rem % p.shape[d];
        rem /= p.shape[d];
        sbase += cd * p.sstride[d];
        obase += cd * p.ostride[d];
    }
    if (rem != 0) return;
    const unsigned long long i0 = b0 * TI, j0 = bj * TJ;
    const int tx = threadIdx.x % TJ, ty = threadIdx.x / TJ;
    const unsigned long long jj = j0 + tx;
    const unsigned long long jc = jj < p.shape[p.j] ? jj : p.shape[p.j] - 1;
    v2d v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const unsigned long long ii = i0 + ty + LR * q;
        const unsigned long long ic = ii < p.shape[0] ? ii : p.shape[0] - 1;
        v[q] = src[sbase + jc + ic * p.sstride[0]];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) tile[ty + LR * q][tx] = v[q];
    __syncthreads();
    const int sx = threadIdx.x % TI, sy = threadIdx.x / TI;
    const unsigned long long io = i0 + sx;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const unsigned long long jo = j0 + sy + SR * q;
        if (io < p.shape[0] && jo < p.shape[p.j]) dst[obase + io + jo * p.ostride[p.j]] = tile[sx][sy + SR * q];
    }
}

}  // namespace
}  // namespace rmhip
