// signal_ops.hip -- convolutions and window generators of the signal builtins.
//   conv1d            crates/runmat-accelerate-api/src/lib.rs:2535-2542   (builtins/math/signal/conv.rs:481-517; simple_provider.rs:1780-1842, 6015-6064)
//   conv2d            lib.rs:2543-2550    (builtins/math/signal/conv2.rs:595-640; simple_provider.rs:6065-6154)
//   hann_window / hamming_window / blackman_window   lib.rs:1797-1807   (simple_provider.rs:95-120, 6453-6472)
//   iir_filter        lib.rs:2551-2559    (builtins/math/signal/filter.rs:1119-1222, 1311-1319, 1370-1460)
//   imfilter          lib.rs:1809-1817    (builtins/image/filters/imfilter.rs:476-545, 620-783)
//   interp1           lib.rs:2458-2463    (runmat-accelerate/src/simple_provider.rs:1396-1472, 8135-8204)
//   polyval           lib.rs:1652-1660    (builtins/math/poly/polyval.rs:886-905, 352-435)
//   moving_window     lib.rs:2852-2857    (builtins/math/reduction/moving.rs:737-825, 929-1003, 1198-1237, 1282-1323)
//   signal_envelope   lib.rs:310-329, 2566-2571   (builtins/math/signal/envelope.rs)
// The convolutions are DIRECT sums in the CPU's order (output n receives a[i] * b[n - i] for i ascending, every product rounded before it
// is added - this file keeps contraction off): bit-exact against the oracle.  One thread per output point, neighbouring threads read
// neighbouring signal points, the kernel operand is staged in LDS when it fits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "move_kernels.h"
#include "row_keys.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
constexpr int kB = 256;
constexpr u64 LDS_TAPS = 4096;  // kernel operands up to this many points are staged in LDS (32 KiB)

// out[o] = sum over i ascending of a[i] * b[n - i], n = start + o
__global__ void __launch_bounds__(kB) k_conv1d(const double* __restrict__ a, u64 la, const double* __restrict__ b, u64 lb, u64 start, u64 len, int b_in_lds,
                                               double* __restrict__ out) {
    extern __shared__ double taps[];
    if (b_in_lds) {
        for (u64 j = threadIdx.x; j < lb; j += kB) taps[j] = b[j];
        __syncthreads();
    }
    const double* bb = b_in_lds ? taps : b;
    const u64 o = (u64)blockIdx.x * kB + threadIdx.x;
    if (o >= len) return;
    const u64 n = start + o;
    const u64 lo = n >= lb - 1 ? n - (lb - 1) : 0, hi = n < la - 1 ? n : la - 1;
    double acc = 0.0;
    // (32-bit trip count, two running pointers: the loop was 20 instructions per tap with 64-bit index arithmetic)
    const double* ap = a + lo;
    const double* bp = bb + (n - lo);
    const unsigned cnt = (unsigned)(hi - lo + 1);
#pragma unroll 4
    for (unsigned k = 0; k < cnt; ++k) {
        const double p = ap[k] * *(bp - k);
        acc = acc + p;
    }
    out[o] = acc;
}

// out(r, c) of the window starting at (r0, c0) of the full result: sum over ac, ar ascending of a(ar, ac) * b(B_r - 1 - (R - ar), B_c - 1 - (C - ac))
__global__ void __launch_bounds__(kB) k_conv2d(const double* __restrict__ a, u64 ar_n, u64 ac_n, const double* __restrict__ b, u64 br_n, u64 bc_n, u64 r0, u64 c0,
                                               u64 rows, u64 cols, int b_in_lds, double* __restrict__ out) {
    extern __shared__ double taps[];
    if (b_in_lds) {
        for (u64 j = threadIdx.x; j < br_n * bc_n; j += kB) taps[j] = b[j];
        __syncthreads();
    }
    const double* bb = b_in_lds ? taps : b;
    const u64 o = (u64)blockIdx.x * kB + threadIdx.x;
    if (o >= rows * cols) return;
    u64 R, Cc;
    if (rows * cols <= 0xffffffffull) {
        const unsigned q = (unsigned)o / (unsigned)rows;
        R = r0 + ((unsigned)o - q * (unsigned)rows), Cc = c0 + q;
    } else {
        R = r0 + o % rows, Cc = c0 + o / rows;
    }
    const u64 ac_lo = Cc >= bc_n - 1 ? Cc - (bc_n - 1) : 0, ac_hi = Cc < ac_n - 1 ? Cc : ac_n - 1;
    const u64 ar_lo = R >= br_n - 1 ? R - (br_n - 1) : 0, ar_hi = R < ar_n - 1 ? R : ar_n - 1;
    double acc = 0.0;
    const unsigned ncol = (unsigned)(ac_hi - ac_lo + 1), nrow = (unsigned)(ar_hi - ar_lo + 1);
    const double* acol = a + ac_lo * ar_n + ar_lo;
    const double* bcol = bb + (bc_n - 1 - (Cc - ac_lo)) * br_n + (br_n - 1 - (R - ar_lo));  // the tap of (ar_lo, ac_lo); rows and columns both ascend
    for (unsigned c = 0; c < ncol; ++c) {
#pragma unroll 4
        for (unsigned k = 0; k < nrow; ++k) {
            const double p = acol[k] * bcol[k];
            acc = acc + p;
        }
        acol += ar_n;
        bcol += br_n;
    }
    out[o] = acc;
}

// The same sums on an LDS-staged patch (see k_imfilter_tile below for why): 64 rows x 16 columns of outputs per workgroup, four per thread.  A
// term whose sample lies outside `a` is skipped, not added as a zero - the CPU never forms that product (0 * Inf would be NaN).
constexpr int CONV_TX = 64, CONV_TY = 16;
__global__ void __launch_bounds__(kB) k_conv2d_tile(const double* __restrict__ a, u64 ar_n, u64 ac_n, const double* __restrict__ b, int br_n, int bc_n, u64 r0, u64 c0,
                                                    u64 rows, u64 cols, double* __restrict__ out) {
    extern __shared__ double patch[];
    const int W = CONV_TX + br_n - 1, H = CONV_TY + bc_n - 1;
    // full-result coordinates of this tile's first output, and the sample its first tap reads (negative: outside)
    const long long R0 = (long long)(r0 + (u64)blockIdx.x * CONV_TX), C0 = (long long)(c0 + (u64)blockIdx.y * CONV_TY);
    const long long ar0 = R0 - (br_n - 1), ac0 = C0 - (bc_n - 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ly = wave; ly < H; ly += kB / 64) {
        const long long ac = ac0 + ly;
        const bool col_in = ac >= 0 && ac < (long long)ac_n;
        for (int lx = lane; lx < W; lx += 64) {
            const long long ar = ar0 + lx;
            patch[ly * W + lx] = (col_in && ar >= 0 && ar < (long long)ar_n) ? a[(u64)ac * ar_n + (u64)ar] : 0.0;
        }
    }
    __syncthreads();
    constexpr int OUTS = CONV_TY / (kB / 64);
    double acc[OUTS];
#pragma unroll
    for (int j = 0; j < OUTS; ++j) acc[j] = 0.0;
    // the taps whose sample exists: kr in [kr_lo, kr_hi] for this thread's row, kc in [kc_lo, kc_hi] for each of its columns
    const long long ar_first = ar0 + lane;
    const int kr_lo = ar_first < 0 ? (int)(-ar_first) : 0;
    const long long kr_room = (long long)ar_n - 1 - ar_first;
    const int kr_hi = kr_room < br_n - 1 ? (int)kr_room : br_n - 1;
    for (int kc = 0; kc < bc_n; ++kc) {
        bool col_ok[OUTS];
#pragma unroll
        for (int j = 0; j < OUTS; ++j) {
            const long long ac = ac0 + wave + j * (kB / 64) + kc;
            col_ok[j] = ac >= 0 && ac < (long long)ac_n;
        }
        const double* row = patch + (wave + kc) * W + lane;
        for (int kr = 0; kr < br_n; ++kr) {
            const double bv = b[kc * br_n + kr];  // uniform: a scalar load
            const bool row_ok = kr >= kr_lo && kr <= kr_hi;
#pragma unroll
            for (int j = 0; j < OUTS; ++j) {
                const double p = row[j * (kB / 64) * W + kr] * bv;
                const double next = acc[j] + p;
                acc[j] = (row_ok && col_ok[j]) ? next : acc[j];
            }
        }
    }
    const u64 orow = (u64)blockIdx.x * CONV_TX + lane;
    if (orow >= rows) return;
#pragma unroll
    for (int j = 0; j < OUTS; ++j) {
        const u64 ocol = (u64)blockIdx.y * CONV_TY + wave + j * (kB / 64);
        if (ocol < cols) out[ocol * rows + orow] = acc[j];
    }
}

__global__ void __launch_bounds__(kB) k_window(int kind, u64 len, double denom, double* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * kB + threadIdx.x;
    if (i >= len) return;
    const double phase = 2.0 * 3.14159265358979323846 * (double)i / denom;
    double v;
    if (kind == 0) v = 0.5 - 0.5 * cos(phase);
    else if (kind == 1) v = 0.54 - 0.46 * cos(phase);
    else v = 0.42 - 0.5 * cos(phase) + 0.08 * cos(2.0 * phase);
    out[i] = v;
}

// moving-window statistics (moving.rs:737-825, 929-1003, 1198-1237, 1282-1323): one thread per output element walks its window in
// ascending position - the CPU's order, every operation rounded as written (sums fold from -0.0, products from 1.0, Welford's running
// mean / M2 for std and var) - so results are bit-exact.  Neighbouring threads are neighbouring lines: coalesced for a window along any
// dimension but the first; along the first, neighbouring outputs share all but two window points (cache hits).
constexpr int MED_MAX = 64;  // median: the window's values are insertion-sorted in a per-thread array
struct MovingArgs {
    u64 pre, len, post, out_len, before, after, total;
    int op, endpoints, nan_omit, population;
    double fill;
};

__device__ __forceinline__ double kth_fill(const double* sorted, int n, double fill, u64 fill_count, u64 k) {
    int less = 0;
    while (less < n && sorted[less] < fill) ++less;
    int equal = 0;
    while (less + equal < n && sorted[less + equal] == fill) ++equal;
    if (k < (u64)less) return sorted[k];
    if (k < (u64)(less + equal) + fill_count) return fill;
    return sorted[k - fill_count];
}

template <int OP>
__global__ void __launch_bounds__(kB) k_moving(const double* __restrict__ x, MovingArgs A, double* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * kB + threadIdx.x;
    if (e >= A.total) return;
    u64 i, p, o;
    if (A.total <= 0xffffffffull) {  // 32-bit divisions when the output has fewer than 2^32 elements (a 64-bit one is ~40 instructions)
        const unsigned e32 = (unsigned)e, pre32 = (unsigned)A.pre, ol32 = (unsigned)A.out_len, r32 = e32 / pre32;
        i = e32 - r32 * pre32, o = r32 / ol32, p = r32 - (unsigned)o * ol32;
    } else {
        const u64 r = e / A.pre;
        i = e % A.pre, p = r % A.out_len, o = r / A.out_len;
    }
    const long long center = (long long)(A.endpoints == 1 ? p + A.before : p);
    const long long start = center - (long long)A.before, end = center + (long long)A.after;
    long long s0 = start < 0 ? 0 : start, e0 = end + 1;
    if (s0 > (long long)A.len) s0 = (long long)A.len;
    if (e0 < 0) e0 = 0;
    if (e0 > (long long)A.len) e0 = (long long)A.len;
    u64 fc = 0;
    if (A.endpoints == 2) fc = (u64)(start < 0 ? -start : 0) + (u64)(end >= (long long)A.len ? end - (long long)A.len + 1 : 0);
    const double* src = x + i + o * A.pre * A.len;
    double sum = -0.0, prod = 1.0, mn = INFINITY, mx = -INFINITY, mean = 0.0, m2 = 0.0;
    double med[OP == 5 ? MED_MAX : 1];
    unsigned n = 0;  // (window lengths fit 32 bits: checked by the entry point)
    bool saw_nan = false;
    const double* wp = src + (u64)s0 * A.pre;  // a running pointer and a 32-bit trip count instead of 64-bit index arithmetic per point
    const unsigned wlen = (unsigned)(e0 - s0);
    // the window in batches of eight loads issued together: with one load per trip every point waited out a memory latency (the NaN test
    // between two loads keeps the compiler from batching them itself)
    for (unsigned w0 = 0; w0 < wlen && !saw_nan; w0 += 8, wp += 8 * A.pre) {
        double batch[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) batch[u] = w0 + u < wlen ? wp[(u64)u * A.pre] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
        if (saw_nan || w0 + u >= wlen) continue;
        const double v = batch[u];
        if (isnan(v)) {
            if (!A.nan_omit) saw_nan = true;
            continue;
        }
        ++n;
        if (OP == 0 || OP == 1) sum = sum + v;
        if (OP == 2) prod = prod * v;
        if (OP == 3) mn = fmin(mn, v);
        if (OP == 4) mx = fmax(mx, v);
        if (OP == 5) {  // insertion into the sorted prefix (a stable sort of non-NaN values: equal values keep their order, as the CPU's)
            int k = (int)n - 1;
            while (k > 0 && med[k - 1] > v) med[k] = med[k - 1], --k;
            med[k] = v;
        }
        if (OP == 6 || OP == 7) {
            const double d = v - mean;
            mean = mean + d / (double)n;
            const double d2 = v - mean;
            m2 = m2 + d * d2;
        }
    }
    }
    double res;
    if (fc && (saw_nan || (isnan(A.fill) && !A.nan_omit))) {
        res = NAN;
    } else {
        if (fc && isnan(A.fill)) fc = 0, saw_nan = false;  // omitted NaN padding: the values alone
        if (saw_nan) {
            res = NAN;
        } else if (n == 0 && fc == 0) {
            res = OP == 0 ? 0.0 : (OP == 2 ? 1.0 : NAN);
        } else if (OP == 0) {
            res = fc ? sum + A.fill * (double)fc : sum;
        } else if (OP == 1) {
            res = fc ? (sum + A.fill * (double)fc) / (double)(n + fc) : sum / (double)n;
        } else if (OP == 2) {
            res = fc ? prod * A.fill : prod;  // (the entry point only lets fills through whose power is the fill itself: 0, 1)
        } else if (OP == 3) {
            res = fc ? fmin(mn, A.fill) : mn;
        } else if (OP == 4) {
            res = fc ? fmax(mx, A.fill) : mx;
        } else if (OP == 5) {
            const u64 total = n + fc, mid = total / 2;
            if (fc == 0) res = total % 2 ? med[mid] : (med[mid - 1] + med[mid]) / 2.0;
            else res = total % 2 ? kth_fill(med, (int)n, A.fill, fc, mid) : (kth_fill(med, (int)n, A.fill, fc, mid - 1) + kth_fill(med, (int)n, A.fill, fc, mid)) / 2.0;
        } else {
            u64 cnt = n;
            if (fc) {
                if (cnt == 0) {
                    cnt = fc, mean = A.fill, m2 = 0.0;
                } else {
                    const u64 total = cnt + fc;
                    const double d = A.fill - mean;
                    mean = mean + d * ((double)fc / (double)total);
                    m2 = m2 + d * d * ((double)cnt * (double)fc / (double)total);
                    cnt = total;
                }
            }
            const double den = A.population ? (double)cnt : (cnt > 1 ? (double)(cnt - 1) : (double)cnt);
            res = m2 / den;
            if (OP == 6) res = sqrt(res);
        }
    }
    out[e] = res;
}

// ---- median over long windows (rmhip_moving_window_long) ---------------------------------------------------------------------------------
// The same result as k_moving<5> (moving.rs:1282-1323), found by selection instead of a per-thread sorted array.  One workgroup takes one
// line and a tile of up to MEDL_T consecutive outputs: the samples those windows cover are staged in LDS once as order-preserving keys
// (row_keys.h, the key map of k_sort_keys: both zeros one key, NaN the largest key).  Each wave then takes every fourth output and finds
// the key of the wanted rank by a most-significant-digit radix select over the window's keys: per level an 8-bit digit histogram in the
// wave's own 256 LDS counters (integer adds: the same bits on every run), a scan across the wave for the digit that holds the rank, a
// narrower prefix; it stops as soon as one candidate is left.  Level 0 reads every key, so it also counts the NaNs and, with padding, the values below / equal to the fill.  A walk
// over the window in window order then gives the POSITION of the rank's element among the candidates - the CPU's stable sort keeps equal
// values in window order - and the element's own bits: the key's inverse, or the sample itself for the one key two values share (+-0).
// For an even count the upper middle element is the next equal key in window order or else the first least key above.
constexpr unsigned MEDL_T = 1024;  // most outputs per tile
constexpr u64 MEDL_W = 4096;       // longest window: MEDL_T + MEDL_W - 1 keys and the counters are 44 KiB of a workgroup's 64 KiB of LDS
constexpr unsigned MEDL_HIST = 4 * 256 * sizeof(unsigned);  // bytes of the four waves' counters, ahead of the keys
struct MedLongArgs {
    u64 pre, len, out_len, before, after, tiles;
    unsigned T;
    int endpoints, nan_omit;
    double fill;
};

// position in window order of the k-th (from 0) key whose bits above `sh` equal `prefix`; every lane gets it
__device__ __forceinline__ unsigned medl_walk(const u64* wk, unsigned wlen, int sh, u64 prefix, unsigned k, int lane) {
    for (unsigned base = 0; base < wlen; base += 64) {
        const unsigned idx = base + lane;
        const bool m = idx < wlen && (wk[idx] >> sh) == prefix;
        const u64 mask = __ballot(m);
        const unsigned cnt = (unsigned)__popcll(mask);
        if (k < cnt) {
            const unsigned rank = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            return base + (unsigned)(__ffsll((long long)__ballot(m && rank == k)) - 1);
        }
        k -= cnt;
    }
    return 0;  // (not reached: the caller's k is below the number of such keys)
}

__global__ void __launch_bounds__(kB) k_movmed_long(const double* __restrict__ x, MedLongArgs A, u64 block0, double* __restrict__ out) {
    extern __shared__ u64 medl_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* hist = (unsigned*)medl_lds + wave * 256;
    u64* keys = medl_lds + MEDL_HIST / sizeof(u64);
    // neighbouring workgroups are neighbouring lines (the strided samples of a line along a later dimension share their cache lines with the
    // next lines'), then the tiles of a line, then the outer index
    const u64 b = block0 + blockIdx.x;
    const u64 i = b % A.pre, r = b / A.pre, tile = r % A.tiles, o = r / A.tiles;
    const u64 p0 = tile * A.T;
    const unsigned nout = (unsigned)(A.out_len - p0 < A.T ? A.out_len - p0 : A.T);
    const long long len = (long long)A.len, shift = A.endpoints == 1 ? (long long)A.before : 0;
    // the samples this tile's windows cover: [lo, hi) of the line
    long long lo = (long long)p0 + shift - (long long)A.before, hi = (long long)p0 + shift + (long long)(nout - 1) + (long long)A.after + 1;
    lo = lo < 0 ? 0 : (lo > len ? len : lo);
    hi = hi < lo ? lo : (hi > len ? len : hi);
    const double* src = x + i + o * A.pre * A.len;
    const unsigned span = (unsigned)(hi - lo);
    for (unsigned j = threadIdx.x; j < span; j += kB) keys[j] = rowkeys::key(src[((u64)lo + j) * A.pre]);
    ((uint4*)hist)[lane] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const u64 fkey = rowkeys::key(A.fill);
    const bool fill_nan = A.fill != A.fill;
    for (unsigned q = wave; q < nout; q += kB / 64) {
        const u64 p = p0 + q;
        const long long start = (long long)p + shift - (long long)A.before, end = (long long)p + shift + (long long)A.after;
        long long s0 = start < 0 ? 0 : start, e0 = end + 1;
        if (s0 > len) s0 = len;
        if (e0 < 0) e0 = 0;
        if (e0 > len) e0 = len;
        if (e0 < s0) e0 = s0;
        unsigned fc = 0;  // (a window has at most 2^31 points: checked by the entry point)
        if (A.endpoints == 2) fc = (unsigned)(start < 0 ? -start : 0) + (unsigned)(end >= len ? end - len + 1 : 0);
        const u64* wk = keys + (s0 - lo);
        const unsigned wlen = (unsigned)(e0 - s0);
        double* dst = out + i + A.pre * (p + A.out_len * o);
        // level 0: every key
        unsigned nn = 0, less_f = 0, eq_f = 0;
        for (unsigned base = 0; base < wlen; base += 64) {
            const unsigned idx = base + lane;
            const bool in = idx < wlen;
            const u64 key = in ? wk[idx] : 0ull;
            const unsigned digit = (unsigned)(key >> 56);
            nn += (unsigned)__popcll(__ballot(in && key == ~0ull));
            if (fc) {
                less_f += (unsigned)__popcll(__ballot(in && key < fkey));
                eq_f += (unsigned)__popcll(__ballot(in && key == fkey));
            }
            // the lanes that share the first lane's digit add as one (a window's top digits are mostly one value), the others singly
            const unsigned lead = (unsigned)__shfl((int)digit, 0);
            const u64 grp = __ballot(in && digit == lead);
            if (lane == 0) atomicAdd(&hist[lead], (unsigned)__popcll(grp));
            if (in && digit != lead) atomicAdd(&hist[digit], 1u);
        }
        const unsigned n = wlen - nn;
        bool nan_res = !A.nan_omit && (nn > 0 || (fc > 0 && fill_nan));
        if (fc && fill_nan) fc = 0;  // omitted NaN padding: the values alone
        if (n == 0 && fc == 0) nan_res = true;
        // the ranks wanted of the values (`sel`, and the one after it when `two`), the rest of the middle being the fill (kth_fill above)
        const unsigned total = n + fc, mid = total / 2;
        const bool even = !(total & 1);
        bool fill_a = false, fill_b = false;
        unsigned ja = even ? mid - 1 : mid, jb = mid;
        if (fc) {
            fill_a = ja >= less_f && ja < less_f + eq_f + fc;
            fill_b = jb >= less_f && jb < less_f + eq_f + fc;
            if (ja >= less_f + eq_f + fc) ja -= fc;
            if (jb >= less_f + eq_f + fc) jb -= fc;
        }
        const bool need_a = !fill_a, need_b = even && !fill_b;
        if (nan_res || !(need_a || need_b)) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            ((uint4*)hist)[lane] = make_uint4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (lane == 0) *dst = nan_res ? NAN : (even ? (A.fill + A.fill) / 2.0 : A.fill);
            continue;
        }
        const bool two = need_a && need_b;
        unsigned k = need_a ? ja : jb, cand = wlen;
        u64 prefix = 0;
        int sh = 56;
        for (int level = 0;; ++level, sh -= 8) {
            if (level > 0) {
                for (unsigned base = 0; base < wlen; base += 64) {
                    const unsigned idx = base + lane;
                    const u64 key = idx < wlen ? wk[idx] : 0ull;
                    const bool m = idx < wlen && (key >> (sh + 8)) == prefix;
                    const unsigned digit = (unsigned)(key >> sh) & 255u;
                    const u64 todo = __ballot(m);
                    if (todo) {
                        const int leader = __ffsll((long long)todo) - 1;
                        const unsigned lead = (unsigned)__shfl((int)digit, leader);
                        const u64 grp = __ballot(m && digit == lead);
                        if (lane == leader) atomicAdd(&hist[lead], (unsigned)__popcll(grp));
                        if (m && digit != lead) atomicAdd(&hist[digit], 1u);
                    }
                }
            }
            // the digit whose bin holds rank k: four bins per lane, their sums scanned across the wave
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const uint4 c4 = ((const uint4*)hist)[lane];
            ((uint4*)hist)[lane] = make_uint4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const unsigned s4 = c4.x + c4.y + c4.z + c4.w;
            unsigned incl = s4;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = (unsigned)__shfl_up((int)incl, d);
                if (lane >= d) incl += up;
            }
            const unsigned excl = incl - s4;
            const int who = __ffsll((long long)__ballot(k >= excl && k < incl)) - 1;
            const unsigned rk = k - excl;  // (meaningful in lane `who`)
            unsigned bin = 0, below = excl, cnt = c4.x;
            if (rk >= c4.x) bin = 1, below = excl + c4.x, cnt = c4.y;
            if (rk >= c4.x + c4.y) bin = 2, below = excl + c4.x + c4.y, cnt = c4.z;
            if (rk >= c4.x + c4.y + c4.z) bin = 3, below = excl + c4.x + c4.y + c4.z, cnt = c4.w;
            const unsigned digit = (unsigned)__shfl((int)(4 * lane + bin), who);
            k -= (unsigned)__shfl((int)below, who);
            cand = (unsigned)__shfl((int)cnt, who);
            prefix = (prefix << 8) | digit;
            if (cand == 1 || level == 7) break;
        }
        // the element of that rank and its bits
        const unsigned pa = medl_walk(wk, wlen, sh, prefix, k, lane);
        const u64 key_a = wk[pa];
        double va = key_a == rowkeys::KEY_ZERO ? src[((u64)s0 + pa) * A.pre] : rowkeys::value_of_key(key_a);
        double vb = va;
        if (two) {
            unsigned pb;
            u64 key_b;
            if (k + 1 < cand) {  // the next equal key in window order
                pb = medl_walk(wk, wlen, sh, prefix, k + 1, lane);
                key_b = key_a;
            } else {  // the least key above, at its first position
                u64 best = ~0ull;
                unsigned at = 0;
                for (unsigned idx = lane; idx < wlen; idx += 64) {
                    const u64 key = wk[idx];
                    if (key > key_a && key < best) best = key, at = idx;
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const u64 ok = (u64)__shfl_xor((long long)best, d);
                    const unsigned oa = (unsigned)__shfl_xor((int)at, d);
                    if (ok < best || (ok == best && oa < at)) best = ok, at = oa;
                }
                pb = at, key_b = best;
            }
            vb = key_b == rowkeys::KEY_ZERO ? src[((u64)s0 + pb) * A.pre] : rowkeys::value_of_key(key_b);
        }
        if (lane == 0) {
            double res;
            if (!even) res = va;
            else if (two) res = (va + vb) / 2.0;
            else res = need_a ? (va + A.fill) / 2.0 : (A.fill + va) / 2.0;
            *dst = res;
        }
    }
}

// polyval (builtins/math/poly/polyval.rs:886-905): Horner's rule acc = acc * x + c over the coefficients, product rounded before the sum;
// with `mu` the point is first centred and scaled the way the CPU's complex division by (scale + 0i) does it:
// ((x - mean) * scale) / (scale * scale).  The CPU runs this in complex arithmetic; for real data the real part is this recurrence as long
// as every intermediate stays finite (an infinite one makes the imaginary lane inf * 0 = NaN there): `nonfinite` records that.
__global__ void __launch_bounds__(kB) k_polyval(const double* __restrict__ coef, u64 m, const double* __restrict__ x, u64 n, int has_mu, double mean, double scale,
                                                int c_in_lds, double* __restrict__ out, int* __restrict__ nonfinite) {
    extern __shared__ double taps[];
    if (c_in_lds) {
        for (u64 j = threadIdx.x; j < m; j += kB) taps[j] = coef[j];
        __syncthreads();
    }
    const double* cc = c_in_lds ? taps : coef;
    const u64 e = (u64)blockIdx.x * kB + threadIdx.x;
    if (e >= n) return;
    double v = x[e];
    if (has_mu) {
        const double t = v - mean;
        const double num = t * scale + 0.0, den = scale * scale + 0.0;
        v = num / den;
    }
    double acc = 0.0;
    bool bad = !isfinite(v);
    for (u64 j = 0; j < m; ++j) {
        const double p = acc * v;
        acc = p + cc[j];
        bad |= !isfinite(acc);
    }
    out[e] = acc;
    if (bad) *nonfinite = 1;
}

// filter(b, a, x) along a dimension (builtins/math/signal/filter.rs:1119-1222): direct form II transposed, y = b0 x + s0,
// s[i-1] = (b[i] x + s[i]) - a[i] y - a recurrence along the dimension, so ONE THREAD PER CHANNEL walks it in order with the states in
// registers (order <= 8) or a per-thread array; neighbouring threads are neighbouring channels.  Every operation as the CPU rounds it.
template <int MAXO>
__global__ void __launch_bounds__(kB) k_iir(const double* __restrict__ x, const double* __restrict__ zi, const double* __restrict__ coef, int order, u64 leading,
                                            u64 dim_len, u64 channels, double* __restrict__ y, double* __restrict__ zf) {
    const u64 ch = (u64)blockIdx.x * kB + threadIdx.x;
    if (ch >= channels) return;
    const u64 l = ch % leading, t = ch / leading;
    const u64 state_len = (u64)order - 1;
    double bn[MAXO], an[MAXO], st[MAXO];
#pragma unroll
    for (int i = 0; i < MAXO; ++i) {
        bn[i] = i < order ? coef[i] : 0.0;
        an[i] = i < order ? coef[order + i] : 0.0;
        st[i] = (zi && (u64)i < state_len) ? zi[l + (u64)i * leading + t * leading * state_len] : 0.0;
    }
    const double* src = x + t * dim_len * leading + l;
    double* dst = y + t * dim_len * leading + l;
    // eight samples are fetched together ahead of the recurrence that consumes them: with one load per step every step waited out a memory
    // latency (4.0 ms for 8192 channels x 8192 samples)
    for (u64 s0 = 0; s0 < dim_len; s0 += 8) {
        double xb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xb[u] = s0 + u < dim_len ? src[(s0 + u) * leading] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u >= dim_len) break;
            const double xn = xb[u];
            const double yv = bn[0] * xn + st[0];
            dst[(s0 + u) * leading] = yv;
#pragma unroll
            for (int i = 1; i < MAXO; ++i) {
                if (i < order) {
                    const double next = (u64)i < state_len ? st[i] : 0.0;
                    const double p = bn[i] * xn, q = an[i] * yv;
                    st[i - 1] = (p + next) - q;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXO; ++i)
        if ((u64)i < state_len) zf[l + (u64)i * leading + t * leading * state_len] = st[i];
}

// ---- filter on long signals with few channels (rmhip_iir_filter_long) -----------------------------------------------------------------
// Every kernel below lowers *verdict to 0 when it meets a non-finite value: the CPU poisons every later sample once one appears, which
// neither the per-sample sum nor the chunked scan reproduces, so the entry point declines the request.

// FIR (every normalised a(i), i >= 2, is 0): the recurrence's states unroll into the nested sum y[n] = b0 x[n] + (b1 x[n-1] + (b2 x[n-2]
// + ...)), the chain ending in + 0.0 after order - 1 terms or in zi[n] when it reaches the start of the signal first.  One thread per
// output sample forms it from the innermost term outwards: the CPU's additions in the CPU's order.  `tiles` != 0: the dimension is the
// contiguous one, a block is one tile of kB samples of one channel and stages them with the order - 1 before them in LDS.
constexpr int FIRL_WIN = kB + 63;
__global__ void __launch_bounds__(kB) k_fir_long(const double* __restrict__ x, const double* __restrict__ zi, const double* __restrict__ coef, int order, u64 leading,
                                                 u64 dim_len, u64 total, u64 tiles, double* __restrict__ y, unsigned* __restrict__ verdict) {
    __shared__ double win[FIRL_WIN];
    const int S = order - 1;
    u64 l, n, t;
    bool live;
    if (tiles) {
        t = (u64)blockIdx.x / tiles, l = 0;
        const u64 n0 = ((u64)blockIdx.x % tiles) * kB;
        n = n0 + threadIdx.x;
        live = n < dim_len;
        const double* line = x + t * dim_len;
        for (int j = threadIdx.x; j < kB + S; j += kB) {  // win[j] is sample n0 - S + j
            const long long m = (long long)n0 - S + j;
            win[j] = (m >= 0 && (u64)m < dim_len) ? line[m] : 0.0;
        }
        __syncthreads();
    } else {
        const u64 e = (u64)blockIdx.x * kB + threadIdx.x;
        live = e < total;
        l = e % leading, n = (e / leading) % dim_len, t = e / (leading * dim_len);
    }
    if (!live) return;
    const u64 at = t * dim_len * leading + n * leading + l;
    const int K = n < (u64)S ? (int)n : S;
    double acc = (zi && n < (u64)S) ? zi[l + n * leading + t * leading * (u64)S] : 0.0;
    bool bad = !isfinite(acc);
    if (tiles) {
        const double* here = win + threadIdx.x + S;
        for (int k = K; k >= 1; --k) {
            const double p = coef[k] * *(here - k);
            acc = p + acc;
        }
    } else {
        const double* here = x + at;
        for (int k = K; k >= 1; --k) {
            const double p = coef[k] * *(here - (u64)k * leading);
            acc = p + acc;
        }
    }
    const double xn = tiles ? win[threadIdx.x + S] : x[at];
    const double p0 = coef[0] * xn;
    const double yv = p0 + acc;
    y[at] = yv;
    if (bad || !isfinite(xn) || !isfinite(yv)) *verdict = 0;
}

// its final state, one thread per (channel, state): zf[i] = b[i+1] x[N-1] + (b[i+2] x[N-2] + ...), order - 1 - i terms and + 0.0, or N terms
// and zi[i + N] when the signal is shorter than that
__global__ void __launch_bounds__(kB) k_fir_long_state(const double* __restrict__ x, const double* __restrict__ zi, const double* __restrict__ coef, int order,
                                                       u64 leading, u64 dim_len, u64 total, double* __restrict__ zf, unsigned* __restrict__ verdict) {
    const u64 w = (u64)blockIdx.x * kB + threadIdx.x;
    if (w >= total) return;
    const u64 S = (u64)order - 1;
    const u64 l = w % leading, i = (w / leading) % S, t = w / (leading * S);
    const u64 K = dim_len < S - i ? dim_len : S - i;
    double acc = (zi && i + dim_len < S) ? zi[l + (i + dim_len) * leading + t * leading * S] : 0.0;
    bool bad = zi && !isfinite(zi[w]);
    const double* end = x + t * dim_len * leading + dim_len * leading + l;  // one past the channel's last sample
    for (u64 k = K; k >= 1; --k) {
        const double p = coef[i + k] * *(end - k * leading);
        acc = p + acc;
    }
    zf[w] = acc;
    if (bad || !isfinite(acc)) *verdict = 0;
}

// Recursive filters, by chunks of `count` samples.  k_iir's recurrence, operation for operation, on one chunk per thread:
//   from_state == 0  the zero-state pass: chunk c of channel ch starts at sample first + c * count from a zero state, writes its y and
//                    leaves its closing state in states[(ch * slots + c) * S ..];
//   from_state != 0  the tail (nchunks == 1): it starts from the true entry state the state pass left in the channel's last slot, its y is
//                    final and its closing state is the filter's final state, written to zf in the signal's layout.
// Neighbouring threads are neighbouring positions of the leading dimensions, then neighbouring chunks.
template <int MAXO>
__global__ void __launch_bounds__(kB) k_iir_chunks(const double* __restrict__ x, const double* __restrict__ coef, int order, u64 leading, u64 dim_len, u64 channels,
                                                   u64 first, u64 count, u64 nchunks, u64 slots, int from_state, double* __restrict__ states, double* __restrict__ y,
                                                   double* __restrict__ zf, unsigned* __restrict__ verdict) {
    const u64 w = (u64)blockIdx.x * kB + threadIdx.x;
    if (w >= channels * nchunks) return;
    const u64 l = w % leading, cidx = (w / leading) % nchunks, t = w / (leading * nchunks);
    const u64 ch = l + t * leading;
    const u64 state_len = (u64)order - 1;
    double* slot = states + (ch * slots + (from_state ? slots - 1 : cidx)) * state_len;
    double bn[MAXO], an[MAXO], st[MAXO];
#pragma unroll
    for (int i = 0; i < MAXO; ++i) {
        bn[i] = i < order ? coef[i] : 0.0;
        an[i] = i < order ? coef[order + i] : 0.0;
        st[i] = (from_state && (u64)i < state_len) ? slot[i] : 0.0;
    }
    const u64 begin = first + cidx * count;
    const double* src = x + t * dim_len * leading + begin * leading + l;
    double* dst = y + t * dim_len * leading + begin * leading + l;
    bool bad = false;
    for (u64 s0 = 0; s0 < count; s0 += 8) {
        double xb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xb[u] = s0 + u < count ? src[(s0 + u) * leading] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u >= count) break;
            const double xn = xb[u];
            const double yv = bn[0] * xn + st[0];
            dst[(s0 + u) * leading] = yv;
            bad |= !isfinite(xn) || !isfinite(yv);
#pragma unroll
            for (int i = 1; i < MAXO; ++i) {
                if (i < order) {
                    const double next = (u64)i < state_len ? st[i] : 0.0;
                    const double p = bn[i] * xn, q = an[i] * yv;
                    st[i - 1] = (p + next) - q;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXO; ++i)
        if ((u64)i < state_len) {
            bad |= !isfinite(st[i]);
            if (zf) zf[l + (u64)i * leading + t * leading * state_len] = st[i];
            else slot[i] = st[i];
        }
    if (bad) *verdict = 0;
}

// The state pass: s(c+1) = T s(c) + sz(c), s(0) = zi, sequentially over a channel's chunks.  One wavefront per channel, lane j holds row j
// of T (T[j + S i]: state j after a chunk of zero input from unit state i) and state j; slot c holds sz(c) on entry and s(c), the state
// that really entered chunk c, on return; slot nfull receives the state after the last full chunk.  The loop is bounded by the chunk
// count and the closing states are fetched four chunks ahead of the products that consume them.
template <int MAXS>
__global__ void __launch_bounds__(64) k_iir_states(const double* __restrict__ T, const double* __restrict__ zi, int S, u64 leading, u64 nfull,
                                                   double* __restrict__ states, unsigned* __restrict__ verdict) {
    const u64 ch = blockIdx.x, l = ch % leading, t = ch / leading;
    const int lane = threadIdx.x;
    const bool mine = lane < S;
    double row[MAXS];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        row[i] = (mine && i < S) ? T[lane + S * i] : 0.0;
        bad |= !isfinite(row[i]);
    }
    double s = (zi && mine) ? zi[l + (u64)lane * leading + t * leading * (u64)S] : 0.0;
    bad |= !isfinite(s);
    double* slot = states + ch * (nfull + 1) * (u64)S + (mine ? lane : 0);
    for (u64 c0 = 0; c0 < nfull; c0 += 4) {
        double sz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) sz[u] = (mine && c0 + u < nfull) ? slot[(c0 + u) * S] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u >= nfull) break;
            if (mine) slot[(c0 + u) * S] = s;
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {
                if (i < S) {
                    const double p = row[i] * __shfl(s, i);
                    acc = acc + p;
                }
            }
            s = acc + sz[u];
            bad |= !isfinite(s);
        }
    }
    if (mine) slot[nfull * S] = s;
    if (bad) *verdict = 0;
}

// The correction: y[c L + k] += sum over i ascending of H[k + L i] * s(c)[i], over every full chunk.  A block owns IIRL_KT samples k of
// the chunk and stages their H tile (IIRL_KT x S doubles, at most 31.5 KiB) in LDS; each of its waves then walks (channel, chunk) pairs,
// its lanes on neighbouring samples.
constexpr int IIRL_KT = 64;
template <int MAXS>
__global__ void __launch_bounds__(kB) k_iir_correct(const double* __restrict__ H, int S, u64 L, u64 leading, u64 dim_len, u64 channels, u64 nfull,
                                                    const double* __restrict__ states, double* __restrict__ y, unsigned* __restrict__ verdict) {
    __shared__ double h[IIRL_KT * MAXS];
    const u64 k0 = (u64)blockIdx.x * IIRL_KT;
    bool bad = false;
    for (int j = threadIdx.x; j < IIRL_KT * S; j += kB) {
        const int kk = j % IIRL_KT, i = j / IIRL_KT;
        const double v = H[k0 + kk + L * (u64)i];
        h[j] = v;
        bad |= !isfinite(v);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 pairs = channels * nfull;
    for (u64 p = (u64)blockIdx.y * (kB / 64) + wave; p < pairs; p += (u64)gridDim.y * (kB / 64)) {
        const u64 ch = p / nfull, cidx = p % nfull;
        const u64 l = ch % leading, t = ch / leading;
        const double* s = states + (ch * (nfull + 1) + cidx) * (u64)S;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
            if (i < S) {
                const double q = h[i * IIRL_KT + lane] * s[i];
                acc = acc + q;
            }
        }
        double* at = y + t * dim_len * leading + (cidx * L + k0 + lane) * leading + l;
        const double v = *at + acc;
        *at = v;
        bad |= !isfinite(v);
    }
    if (bad) *verdict = 0;
}

// interp1 (runmat-accelerate/src/simple_provider.rs:1396-1472, 8135-8204): one thread per (series, query) - a binary search of the strictly
// increasing sample coordinates, then the CPU's four operations (linear) or its nearer-neighbour rule (ties to the left).
__device__ __forceinline__ long long interp_search(const double* __restrict__ x, u64 n, double q, bool* exact) {  // Rust's binary_search_by on distinct keys
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (x[mid] < q) lo = mid + 1;
        else hi = mid;
    }
    *exact = lo < n && x[lo] == q;
    return (long long)lo;  // Ok(lo) when exact, else Err(lo): the insertion point
}

__global__ void __launch_bounds__(kB) k_interp1(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ xq, u64 n, u64 qlen, u64 total, int nearest,
                                                int extrapolation, double fill, double* __restrict__ out) {
    const u64 o = (u64)blockIdx.x * kB + threadIdx.x;
    if (o >= total) return;
    const double q = xq[o % qlen];
    const double* ys = y + (o / qlen) * n;
    const double oor = extrapolation == 2 ? fill : NAN;  // interp1_out_of_range
    double r;
    if (!isfinite(q)) {
        r = NAN;
    } else if (!nearest) {
        long long piece = -1;
        const u64 last = n - 1;
        if (q < x[0]) piece = extrapolation == 1 ? 0 : -1;
        else if (q > x[last]) piece = extrapolation == 1 ? (long long)last - 1 : -1;
        else if (q == x[last]) piece = (long long)last - 1;
        else {
            bool exact;
            const long long idx = interp_search(x, n, q, &exact);
            if (exact) piece = idx < (long long)last - 1 ? idx : (long long)last - 1;
            else if (idx > 0 && idx < (long long)n) piece = idx - 1;
        }
        if (piece < 0) {
            r = oor;
        } else {
            const double h = x[piece + 1] - x[piece];
            const double t = (q - x[piece]) / h;
            const double d = ys[piece + 1] - ys[piece];
            const double p = t * d;
            r = ys[piece] + p;
        }
    } else if (q < x[0]) {
        r = extrapolation == 1 ? ys[0] : oor;
    } else if (q > x[n - 1]) {
        r = extrapolation == 1 ? ys[n - 1] : oor;
    } else {
        bool exact;
        const long long idx = interp_search(x, n, q, &exact);
        if (exact) {
            r = ys[idx];
        } else {
            const u64 left = idx > 0 ? (u64)idx - 1 : 0, right = (u64)idx < n - 1 ? (u64)idx : n - 1;
            r = fabs(q - x[left]) <= fabs(x[right] - q) ? ys[left] : ys[right];
        }
    }
    out[o] = r;
}

// imfilter (builtins/image/filters/imfilter.rs:476-545, 620-783): N-D correlation / convolution with the four padding rules.  One thread per
// output element walks the kernel's points in their storage order (first dimension fastest) and adds value * sample, the product rounded
// before the sum - the CPU's loop; up to four dimensions.
struct ImfArgs {
    int rank, padding, convolution;  // padding: 0 constant, 1 replicate, 2 symmetric, 3 circular
    long long img[4], ker[4], out[4], base[4], origin[4];
    u64 istride[4], kstride[4], total;
    double constant;
};

__device__ __forceinline__ long long imf_resolve(long long coord, long long len, int padding) {  // -1: outside under constant padding
    if (coord >= 0 && coord < len) return coord;
    if (padding == 0) return -1;
    if (padding == 1) return coord <= 0 ? 0 : len - 1;             // clamp_index
    if (padding == 3) {                                            // wrap_index
        long long c = coord % len;
        return c < 0 ? c + len : c;
    }
    if (len == 1) return 0;                                        // reflect_index
    const long long period = 2 * len - 2;
    long long v = coord % period;
    if (v < 0) v += period;
    return v >= len ? period - v : v;
}

__global__ void __launch_bounds__(kB) k_imfilter(const double* __restrict__ image, const double* __restrict__ kernel, ImfArgs A, int k_in_lds, double* __restrict__ out) {
    extern __shared__ double taps[];
    const u64 ktotal = (u64)(A.ker[0] * A.ker[1] * A.ker[2] * A.ker[3]);
    if (k_in_lds) {
        for (u64 j = threadIdx.x; j < ktotal; j += kB) taps[j] = kernel[j];
        __syncthreads();
    }
    const double* kk = k_in_lds ? taps : kernel;
    const u64 o = (u64)blockIdx.x * kB + threadIdx.x;
    if (o >= A.total) return;
    long long oc[4];
    u64 r = o;
    for (int d = 0; d < 4; ++d) {
        oc[d] = (long long)(r % (u64)A.out[d]) + A.base[d] - A.origin[d];  // image coordinate of kernel index 0 along d
        r /= (u64)A.out[d];
    }
    double sum = 0.0;
    bool interior = true;
    for (int d = 0; d < 4; ++d) interior = interior && oc[d] >= 0 && oc[d] + A.ker[d] <= A.img[d];
    if (interior) {
        // the kernel's footprint lies inside the image (all but a border of outputs): no padding rule to consult. The tap odometer is
        // wave-uniform, so it lives on the scalar unit (and the coefficients come by scalar loads); sixteen image loads are issued per
        // wait - one dependent load per trip waited out a full memory latency per tap. Same taps, same order.
        const unsigned n0 = (unsigned)A.ker[0], n1 = (unsigned)A.ker[1], n2 = (unsigned)A.ker[2];
        const double* ip = image + (u64)oc[0] + (u64)oc[1] * A.istride[1] + (u64)oc[2] * A.istride[2] + (u64)oc[3] * A.istride[3];
        const long long wrap1 = A.istride[1] - (long long)n0, wrap2 = A.istride[2] - (long long)n1 * A.istride[1],
                        wrap3 = A.istride[3] - (long long)n2 * A.istride[2];
        unsigned k0 = 0, k1 = 0, k2 = 0;
        long long off = 0;
        constexpr int BATCH = 16;
        for (u64 t = 0; t < ktotal; t += BATCH) {
            double v[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; ++j) {
                const bool live = t + j < ktotal;
                v[j] = ip[live ? off : 0];
                ++off;
                if (++k0 == n0) {
                    k0 = 0;
                    off += wrap1;
                    if (++k1 == n1) {
                        k1 = 0;
                        off += wrap2;
                        if (++k2 == n2) {
                            k2 = 0;
                            off += wrap3;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < BATCH; ++j)
                if (t + j < ktotal) {
                    const double p = kernel[A.convolution ? ktotal - 1 - (t + j) : t + j] * v[j];  // convolution reads the kernel back to front
                    sum = sum + p;
                }
        }
        out[o] = sum;
        return;
    }
    for (long long k3 = 0; k3 < A.ker[3]; ++k3) {
        const long long c3 = imf_resolve(oc[3] + k3, A.img[3], A.padding);
        for (long long k2 = 0; k2 < A.ker[2]; ++k2) {
            const long long c2 = imf_resolve(oc[2] + k2, A.img[2], A.padding);
            for (long long k1 = 0; k1 < A.ker[1]; ++k1) {
                const long long c1 = imf_resolve(oc[1] + k1, A.img[1], A.padding);
                const bool outside_hi = c1 < 0 || c2 < 0 || c3 < 0;
                const u64 ibase = outside_hi ? 0 : (u64)c1 * A.istride[1] + (u64)c2 * A.istride[2] + (u64)c3 * A.istride[3];
                const u64 kbase = A.convolution ? (u64)(A.ker[1] - 1 - k1) * A.kstride[1] + (u64)(A.ker[2] - 1 - k2) * A.kstride[2] + (u64)(A.ker[3] - 1 - k3) * A.kstride[3]
                                                : (u64)k1 * A.kstride[1] + (u64)k2 * A.kstride[2] + (u64)k3 * A.kstride[3];
                for (long long k0 = 0; k0 < A.ker[0]; ++k0) {
                    const long long c0 = imf_resolve(oc[0] + k0, A.img[0], A.padding);
                    const double sample = (outside_hi || c0 < 0) ? A.constant : image[ibase + (u64)c0];
                    const double kv = kk[kbase + (u64)(A.convolution ? A.ker[0] - 1 - k0 : k0)];
                    const double p = kv * sample;
                    sum = sum + p;
                }
            }
        }
    }
    out[o] = sum;
}

// The same sum for a filter of two dimensions (every image filter in practice), tiled: a workgroup stages the (64 + k0 - 1) x (16 + k1 - 1)
// patch of the image its 64 x 16 outputs read into LDS once - the padding rule is applied while staging, so the sum itself has no border case -
// and each output then reads its taps from LDS.  The one-thread-per-output kernel re-reads every sample k0*k1 times through the vector cache,
// which eight resident workgroups overflow: it ran at the L2's bandwidth (8192^2, 5x5: 1.8 ms for 13 GB of cache reads).  Taps in the CPU's order.
constexpr int IMF_TX = 64, IMF_TY = 16;
__global__ void __launch_bounds__(kB) k_imfilter_tile(const double* __restrict__ image, const double* __restrict__ kernel, ImfArgs A, double* __restrict__ out) {
    extern __shared__ double patch[];
    const int n0 = (int)A.ker[0], n1 = (int)A.ker[1], W = IMF_TX + n0 - 1, H = IMF_TY + n1 - 1;
    const long long x0 = (long long)blockIdx.x * IMF_TX, y0 = (long long)blockIdx.y * IMF_TY;
    const double* plane = image + (u64)blockIdx.z * A.istride[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ly = wave; ly < H; ly += kB / 64) {
        const long long c1 = imf_resolve(y0 + A.base[1] - A.origin[1] + ly, A.img[1], A.padding);
        for (int lx = lane; lx < W; lx += 64) {
            const long long c0 = imf_resolve(x0 + A.base[0] - A.origin[0] + lx, A.img[0], A.padding);
            patch[ly * W + lx] = (c0 < 0 || c1 < 0) ? A.constant : plane[(u64)c0 + (u64)c1 * A.istride[1]];
        }
    }
    __syncthreads();
    constexpr int ROWS = IMF_TY / (kB / 64);  // outputs per thread: rows wave, wave + 4, ...
    double sum[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) sum[j] = 0.0;
    const int ktotal = n0 * n1;
    int t = 0;
    for (int k1 = 0; k1 < n1; ++k1) {
        const double* row = patch + (wave + k1) * W + lane;
        for (int k0 = 0; k0 < n0; ++k0, ++t) {
            const double kv = kernel[A.convolution ? ktotal - 1 - t : t];  // uniform: a scalar load
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const double p = kv * row[j * (kB / 64) * W + k0];
                sum[j] = sum[j] + p;
            }
        }
    }
    const long long ox = x0 + lane;
    if (ox >= A.out[0]) return;
    double* oplane = out + (u64)blockIdx.z * (u64)A.out[0] * (u64)A.out[1];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const long long oy = y0 + wave + j * (kB / 64);
        if (oy < A.out[1]) oplane[(u64)ox + (u64)oy * (u64)A.out[0]] = sum[j];
    }
}

// polyder / polyint (simple_provider.rs:320-390, 544-585, 3137-3215): coefficient vectors, highest power first.  One thread per coefficient
// of the untrimmed result, the CPU's sums in the CPU's order (a convolution entry accumulates from 0.0 over the first operand's index
// ascending; the two rule terms are right-aligned and added - or subtracted - to 0.0 in turn).  An empty polynomial is [0].
struct PolyVec {
    const double* x;
    u64 n;  // as stored; the effective length is max(n, 1)
    __device__ u64 len() const { return n ? n : 1; }
    __device__ double at(u64 i) const { return n ? x[i] : 0.0; }
    __device__ u64 dlen() const { return n <= 1 ? 1 : n - 1; }                                      // poly_raw_derivative
    __device__ double dat(u64 i) const { return n <= 1 ? 0.0 : x[i] * (double)(n - 1 - i); }
};

template <bool DA, bool DB>  // entry k of conv(a or a', b or b')
__device__ double poly_conv_entry(const PolyVec& a, const PolyVec& b, u64 k) {
    const u64 la = DA ? a.dlen() : a.len(), lb = DB ? b.dlen() : b.len();
    const u64 lo = k >= lb - 1 ? k - (lb - 1) : 0, hi = k < la - 1 ? k : la - 1;
    double t = 0.0;
    for (u64 i = lo; i <= hi; ++i) {
        const double p = (DA ? a.dat(i) : a.at(i)) * (DB ? b.dat(k - i) : b.at(k - i));
        t = t + p;
    }
    return t;
}

// mode 0: p'; 1: p'q + pq'; 2: u'v - uv' (p = u, q = v); 3: v * v (q = v); 4: the integral of p with `constant` appended
__global__ void __launch_bounds__(kB) k_poly(PolyVec p, PolyVec q, int mode, double constant, u64 len, double* __restrict__ out) {
    const u64 k = (u64)blockIdx.x * kB + threadIdx.x;
    if (k >= len) return;
    double r = 0.0;
    if (mode == 0) {
        r = p.dat(k);
    } else if (mode == 3) {
        r = poly_conv_entry<false, false>(q, q, k);
    } else if (mode == 4) {
        r = k < p.n ? p.x[k] / (double)(p.n - k) : constant;
    } else {
        const u64 l1 = p.dlen() + q.len() - 1, l2 = p.len() + q.dlen() - 1;  // poly_add_real / poly_sub_real right-align the two terms
        if (k >= len - l1) r = r + poly_conv_entry<true, false>(p, q, k - (len - l1));
        if (k >= len - l2) {
            const double t2 = poly_conv_entry<false, true>(p, q, k - (len - l2));
            r = mode == 1 ? r + t2 : r - t2;
        }
    }
    out[k] = r;
}

// polyint of a complex-interleaved polynomial (simple_provider.rs:391-409): both parts of coefficient k over the power n - k, a true
// division each; the appended element is (constant, +0).  `r32`: a precision-32 context rounds each part through f32 on the store.
__global__ void __launch_bounds__(kB) k_polyint_cx(const v2d* __restrict__ p, u64 n, double constant, u64 len, int r32, v2d* __restrict__ out) {
    const u64 k = (u64)blockIdx.x * kB + threadIdx.x;
    if (k >= len) return;
    v2d r = {constant, 0.0};
    if (k < n) {
        const double power = (double)(n - k);
        const v2d cf = p[k];
        r.x = cf.x / power, r.y = cf.y / power;
    }
    if (r32) r.x = (double)(float)r.x, r.y = (double)(float)r.y;
    out[k] = r;
}

// poly_trim_slice: the first coefficient with |c| > 1e-12 (a NaN does not count), or len if there is none
__global__ void __launch_bounds__(kB) k_poly_first(const double* __restrict__ x, u64 len, unsigned long long* __restrict__ first) {
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = len;
    __syncthreads();
    for (u64 i = threadIdx.x; i < len && i < best; i += kB)
        if (fabs(x[i]) > 1.0e-12) {
            atomicMin(&best, (unsigned long long)i);
            break;
        }
    __syncthreads();
    if (threadIdx.x == 0) *first = best;
}

// ---- signal_envelope (lib.rs:310-329, :2566-2571; builtins/math/signal/envelope.rs) ----------------------------------------------------
// rmhip.h states the three methods.  The tensor is m channels of n consecutive samples.  k_env_stats sums every channel and looks for
// non-finite samples in the same pass; the mean goes to every later kernel as a table of m doubles.  Analytic: k_env_center writes
// x - mu, the library's own rmhip_hilbert transforms it, k_env_bounds forms mu +- |z|.  AnalyticFir / Rms: one thread per output walks
// its taps or its window in ascending order, every product rounded before it is added, over samples a workgroup staged in LDS once.
// T is the storage type read in place (f32 on a precision-32 context), TO the storage type of the results; arithmetic is f64.
typedef double env_v2d __attribute__((ext_vector_type(2)));
typedef float env_v4f __attribute__((ext_vector_type(4)));
template <class T>
struct EnvVec;
template <>
struct EnvVec<double> {
    typedef env_v2d type;
    static constexpr int N = 2;
};
template <>
struct EnvVec<float> {
    typedef env_v4f type;
    static constexpr int N = 4;
};

constexpr u64 ENV_WAVE_MAX = 4096;        // channels shorter than this are summed by one wave each, longer ones by `parts` workgroups
constexpr u64 ENV_PART_MIN = 8192;        // samples per workgroup at least, when a channel is split
constexpr u64 ENV_PARTS_MAX = 64;
constexpr size_t ENV_LDS_BYTES = 48u * 1024;  // staged samples + taps of k_env_fir / k_env_rms; beyond it they read global memory
constexpr u64 ENV_WORK_MAX = 1ull << 36;  // products of the direct FIR / RMS sums (rmhip.h: a cap, not a measurement)

// the channel of flat element e (a 64-bit division is ~40 instructions: 32-bit when the tensor has fewer than 2^32 elements)
__device__ __forceinline__ u64 env_channel(u64 e, u64 n, u64 total) {
    return total <= 0xffffffffull ? (u64)((unsigned)e / (unsigned)n) : e / n;
}

// sums[c * parts + p] = the sum of part p of channel c (divided by `divisor` when that is not 0), *verdict lowered to 0 when any
// sample is NaN or +-Inf.  A team - one wave when per_wave, else the workgroup - owns one (channel, part): scalar loads up to the first
// 16-byte boundary, 16-byte loads (four in flight per lane) from there, scalar loads for the rest; lanes are added in a fixed tree.
// Every failing team stores the same word: a plain store, no atomic.
template <class T>
__global__ void __launch_bounds__(kB) k_env_stats(const T* __restrict__ x, u64 n, u64 m, u64 parts, u64 part_len, int per_wave, double divisor,
                                                  double* __restrict__ sums, unsigned* __restrict__ verdict) {
    typedef typename EnvVec<T>::type V;
    constexpr int N = EnvVec<T>::N;
    __shared__ double wave_sum[kB / 64];
    __shared__ int wave_bad[kB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 team = per_wave ? (u64)blockIdx.x * (kB / 64) + wave : (u64)blockIdx.x;
    const unsigned tid = per_wave ? lane : threadIdx.x, tsize = per_wave ? 64 : kB;
    const bool live = team < m * parts;
    double acc = 0.0;
    bool bad = false;
    if (live) {
        const u64 c = team / parts, p = team - c * parts;
        const u64 lo = p * part_len, hi = lo + part_len < n ? lo + part_len : n;
        const T* src = x + c * n + lo;
        const u64 len = hi > lo ? hi - lo : 0;
        u64 head = ((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T);
        if (head > len) head = len;
        const u64 nvec = (len - head) / N;
        for (u64 i = tid; i < head; i += tsize) {
            const double v = (double)src[i];
            bad |= !__builtin_isfinite(v);
            acc = acc + v;
        }
        const V* body = reinterpret_cast<const V*>(src + head);
        for (u64 i0 = tid; i0 < nvec; i0 += 4ull * tsize) {
            V v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u64 i = i0 + (u64)u * tsize;
                v[u] = V{};
                if (i < nvec) v[u] = __builtin_nontemporal_load(body + i);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int l = 0; l < N; ++l) {
                    const double s = (double)v[u][l];
                    bad |= !__builtin_isfinite(s);
                    acc = acc + s;
                }
        }
        for (u64 i = head + nvec * N + tid; i < len; i += tsize) {
            const double v = (double)src[i];
            bad |= !__builtin_isfinite(v);
            acc = acc + v;
        }
    }
    int flag = bad ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc = acc + __shfl_xor(acc, o);
        flag |= __shfl_xor(flag, o);
    }
    if (!per_wave) {
        if (lane == 0) wave_sum[wave] = acc, wave_bad[wave] = flag;
        __syncthreads();
        if (threadIdx.x != 0) return;
        acc = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        flag = wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3];
    } else if (lane != 0) {
        return;
    }
    if (!live) return;
    sums[team] = divisor != 0.0 ? acc / divisor : acc;
    if (flag && verdict) *verdict = 0u;
}

template <class T>
__global__ void __launch_bounds__(kB) k_env_center(const T* __restrict__ x, const double* __restrict__ mu, u64 n, u64 total, double* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * kB + threadIdx.x;
    if (e >= total) return;
    out[e] = (double)x[e] - mu[env_channel(e, n, total)];
}

// upper = mu + |z|, lower = mu - |z|; z == nullptr (one-sample channels): |z| = 0, both are the sample itself
template <class TO>
__global__ void __launch_bounds__(kB) k_env_bounds(const double2* __restrict__ z, const double* __restrict__ mu, u64 n, u64 total, TO* __restrict__ upper,
                                                   TO* __restrict__ lower) {
    const u64 e = (u64)blockIdx.x * kB + threadIdx.x;
    if (e >= total) return;
    const double mean = mu[env_channel(e, n, total)];
    double mag = 0.0;
    if (z) {
        const double2 v = z[e];
        mag = hypot(v.x, v.y);
    }
    upper[e] = (TO)(mean + mag);
    lower[e] = (TO)(mean - mag);
}

// The samples a workgroup's kB outputs read: flat elements [base, base + count) of the tensor, base = e0 - before (not below 0), as f64
// in LDS (squared for the RMS sum).  The range is clamped to the TENSOR here, for the loads' sake; every thread clamps its own taps to
// its CHANNEL, so a sample of a neighbouring channel that happens to be staged is never read.
template <class T, bool SQUARE>
__device__ __forceinline__ u64 env_stage(const T* __restrict__ x, u64 e0, u64 before, u64 after, u64 total, double* __restrict__ tile) {
    const u64 base = e0 >= before ? e0 - before : 0;
    u64 end = e0 + kB + after;
    if (end > total) end = total;
    const unsigned count = (unsigned)(end - base);
    for (unsigned j = threadIdx.x; j < count; j += kB) {
        const double v = (double)x[base + j];
        tile[j] = SQUARE ? v * v : v;
    }
    return base;
}

// AnalyticFir: q_i = sum over t ascending of (x[i + t - half] - mu) * k[t] for the taps whose sample lies in the channel, then
// mu +- hypot(x_i - mu, q_i).  `taps` holds k[t0 .. t0 + ntaps): the only taps some output of an n-sample channel can reach.
// before / after: the halo (already limited to n - 1) staged on either side when in_lds.
template <class T, class TO>
__global__ void __launch_bounds__(kB) k_env_fir(const T* __restrict__ x, const double* __restrict__ mu, const double* __restrict__ taps, u64 n, u64 total, u64 filter_len,
                                                u64 half, u64 t0, unsigned ntaps, u64 before, u64 after, int in_lds, TO* __restrict__ upper, TO* __restrict__ lower) {
    extern __shared__ double tile[];
    const u64 e0 = (u64)blockIdx.x * kB;
    u64 base = 0;
    double* ktile = tile;
    if (in_lds) {
        base = env_stage<T, false>(x, e0, before, after, total, tile);
        ktile = tile + (kB + before + after);
        for (unsigned j = threadIdx.x; j < ntaps; j += kB) ktile[j] = taps[j];
        __syncthreads();
    }
    const u64 e = e0 + threadIdx.x;
    if (e >= total) return;
    const u64 c = env_channel(e, n, total), i = e - c * n;
    const double mean = mu[c];
    // taps t_lo .. t_hi: 0 <= i + t - half < n and t < filter_len
    const u64 t_lo = half > i ? half - i : 0;
    u64 t_hi = (n - 1 - i) + half;
    if (t_hi > filter_len - 1) t_hi = filter_len - 1;
    double q = 0.0;
    if (t_hi >= t_lo) {
        const unsigned cnt = (unsigned)(t_hi - t_lo + 1);
        const u64 first = e + t_lo - half;  // flat index of the first sample: inside the channel
        if (in_lds) {
            const double* sp = tile + (first - base);
            const double* kp = ktile + (t_lo - t0);
#pragma unroll 4
            for (unsigned k = 0; k < cnt; ++k) {
                const double p = (sp[k] - mean) * kp[k];
                q = q + p;
            }
        } else {
            const T* sp = x + first;
            const double* kp = taps + (t_lo - t0);
#pragma unroll 4
            for (unsigned k = 0; k < cnt; ++k) {
                const double p = ((double)sp[k] - mean) * kp[k];
                q = q + p;
            }
        }
    }
    const double re = (in_lds ? tile[e - base] : (double)x[e]) - mean;
    const double mag = n == 1 ? 0.0 : hypot(re, q);
    upper[e] = (TO)(mean + mag);
    lower[e] = (TO)(mean - mag);
}

// Rms: upper_i = sqrt(sum of x_j^2 over j = s .. e - 1 ascending / (e - s)), s = max(0, i - hb), e = min(n, i + ha + 1); lower = -upper.
// No mean is removed.  before / after: min(hb, n - 1) and min(ha, n - 1).
template <class T, class TO>
__global__ void __launch_bounds__(kB) k_env_rms(const T* __restrict__ x, u64 n, u64 total, u64 before, u64 after, int in_lds, TO* __restrict__ upper,
                                                TO* __restrict__ lower) {
    extern __shared__ double tile[];
    const u64 e0 = (u64)blockIdx.x * kB;
    u64 base = 0;
    if (in_lds) {
        base = env_stage<T, true>(x, e0, before, after, total, tile);
        __syncthreads();
    }
    const u64 e = e0 + threadIdx.x;
    if (e >= total) return;
    const u64 c = env_channel(e, n, total), i = e - c * n;
    const u64 s = i > before ? i - before : 0;  // (before = min(hb, n - 1): the same start)
    const u64 stop = i + after + 1 < n ? i + after + 1 : n;
    const unsigned cnt = (unsigned)(stop - s);
    const u64 first = c * n + s;
    double acc = 0.0;
    if (in_lds) {
        const double* sp = tile + (first - base);
#pragma unroll 4
        for (unsigned k = 0; k < cnt; ++k) acc = acc + sp[k];
    } else {
        const T* sp = x + first;
#pragma unroll 4
        for (unsigned k = 0; k < cnt; ++k) {
            const double v = (double)sp[k];
            const double p = v * v;
            acc = acc + p;
        }
    }
    const double r = sqrt(acc / (double)cnt);
    const TO up = (TO)r;
    upper[e] = up;
    lower[e] = -up;
}

// modified Bessel function I0 as envelope.rs sums it: at most 32 further terms, stopped when a term is <= 1e-15 of the sum
double env_bessel_i0(double x) {
    const double y = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k <= 32; ++k) {
        term *= y / (double)(k * k);
        sum += term;
        if (std::fabs(term) <= std::fabs(sum) * 1.0e-15) break;
    }
    return sum;
}

// tap t of the Kaiser-windowed (beta 8) Hilbert transformer of `len` taps (envelope.rs hilbert_fir_kernel), in its operation order
double env_fir_tap(u64 t, u64 len) {
    const double center = ((double)len - 1.0) / 2.0;
    const double k = (double)t - center;
    double ideal;
    if (std::fabs(k) <= 1.0e-12) {
        ideal = 0.0;
    } else {
        const double rounded = std::round(k);
        if (std::fabs(rounded - k) <= 1.0e-12 && std::fmod(std::fabs(rounded), 2.0) == 0.0) ideal = 0.0;
        else ideal = 2.0 / (3.14159265358979323846 * k);
    }
    double window = 1.0;
    if (len > 1) {
        const double ratio = 2.0 * (double)t / (double)(len - 1) - 1.0;
        const double argument = 8.0 * std::sqrt(std::max(1.0 - ratio * ratio, 0.0));
        window = env_bessel_i0(argument) / env_bessel_i0(8.0);
    }
    return ideal * window;
}

struct EnvPrecision64 {  // the analytic path's transform runs in f64 on a precision-32 context too (rmhip.h): held for the nested call
    Context* c;
    int saved;
    explicit EnvPrecision64(Context* ctx) : c(ctx), saved(ctx->precision) { c->precision = 64; }
    ~EnvPrecision64() { c->precision = saved; }
};

inline unsigned grid_for(u64 n) { return (unsigned)((n + kB - 1) / kB); }

// per-channel means of the [n, m] tensor into mu[0 .. m), the verdict word lowered when a sample is not finite
template <class T>
int env_means(Context* c, const T* x, u64 n, u64 m, double* mu, double* partial, u64 parts, u64 part_len, unsigned* verdict) {
    if (parts == 1) {
        const int per_wave = n < ENV_WAVE_MAX;
        const u64 blocks = per_wave ? (m + kB / 64 - 1) / (kB / 64) : m;
        hipLaunchKernelGGL(k_env_stats<T>, dim3((unsigned)blocks), dim3(kB), 0, c->stream, x, n, m, (u64)1, n, per_wave, (double)n, mu, verdict);
        c->tel.kernel_launches++;
    } else {
        hipLaunchKernelGGL(k_env_stats<T>, dim3((unsigned)(m * parts)), dim3(kB), 0, c->stream, x, n, m, parts, part_len, 0, 0.0, partial, verdict);
        // the parts of a channel, added by one wave, and the division by n
        hipLaunchKernelGGL(k_env_stats<double>, dim3((unsigned)((m + kB / 64 - 1) / (kB / 64))), dim3(kB), 0, c->stream, (const double*)partial, parts, m, (u64)1, parts, 1,
                           (double)n, mu, (unsigned*)nullptr);
        c->tel.kernel_launches += 2;
    }
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

template <class T, class TO>
int env_launch(Context* c, int method, const T* x, const double* mu, const double2* z, const double* taps, u64 n, u64 total, u64 param, u64 t0, unsigned ntaps,
               TO* upper, TO* lower) {
    const dim3 grid(grid_for(total)), block(kB);
    if (method == 0) {
        hipLaunchKernelGGL(k_env_bounds<TO>, grid, block, 0, c->stream, z, mu, n, total, upper, lower);
    } else if (method == 1) {
        const u64 half = param / 2, before = std::min<u64>(half, n - 1), after = std::min<u64>(param - 1 - half, n - 1);
        const size_t bytes = (size_t)(kB + before + after + ntaps) * sizeof(double);
        const int in_lds = bytes <= ENV_LDS_BYTES;
        hipLaunchKernelGGL((k_env_fir<T, TO>), grid, block, in_lds ? bytes : 0, c->stream, x, mu, taps, n, total, param, half, t0, ntaps, before, after, in_lds, upper, lower);
    } else {
        const u64 before = std::min<u64>((param - 1) / 2, n - 1), after = std::min<u64>(param / 2, n - 1);
        const size_t bytes = (size_t)(kB + before + after) * sizeof(double);
        const int in_lds = bytes <= ENV_LDS_BYTES;
        hipLaunchKernelGGL((k_env_rms<T, TO>), grid, block, in_lds ? bytes : 0, c->stream, x, n, total, before, after, in_lds, upper, lower);
    }
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // namespace
}  // namespace rmhip

extern "C" {

int rmhip_conv1d(rmhip_ctx* ctx, rmhip_buf signal, rmhip_buf kernel, int mode, int column, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (mode < 0 || mode > 2) return fail(RMHIP_ERR_INVALID, "conv1d: mode %d", mode);
    Buffer ab, bb;
    RMHIP_TRY(c->get(signal, &ab));
    RMHIP_TRY(c->get(kernel, &bb));
    const u64 la = ab.numel, lb = bb.numel;
    u64 start = 0, len = 0;
    if (la && lb) {
        const u64 full = la + lb - 1;
        start = 0, len = full;
        if (mode == 1) start = (lb - 1) / 2, len = la;
        if (mode == 2) {
            if (la < lb) len = 0;
            else start = lb - 1, len = la - lb + 1;
        }
        if (len && start + len > full) len = full > start ? full - start : 0;
    }
    // conv1d_output_shape (simple_provider.rs:1780-1787): [1, len] or [len, 1], an empty result keeps the orientation
    const size_t shape[2] = {column ? (size_t)len : 1, column ? 1 : (size_t)len};
    if (len > 0x7fffffffull * kB) return fail(RMHIP_ERR_UNSUPPORTED, "conv1d: %llu outputs", len);  // before the output exists
    Buffer ob;
    RMHIP_TRY(c->new_buffer(shape, 2, out, &ob));
    if (len == 0) return RMHIP_OK;
    const int in_lds = lb <= LDS_TAPS;
    hipLaunchKernelGGL(k_conv1d, dim3(grid_for(len)), dim3(kB), in_lds ? lb * sizeof(double) : 0, c->stream, ab.data(), la, bb.data(), lb, start, len, in_lds, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_conv2d(rmhip_ctx* ctx, rmhip_buf signal, rmhip_buf kernel, int mode, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (mode < 0 || mode > 2) return fail(RMHIP_ERR_INVALID, "conv2d: mode %d", mode);
    Buffer ab, bb;
    RMHIP_TRY(c->get(signal, &ab));
    RMHIP_TRY(c->get(kernel, &bb));
    for (const Buffer* x : {&ab, &bb})  // ensure_diag_shape, simple_provider.rs:2394-2400
        for (size_t d = 2; d < x->shape.size(); ++d)
            if (x->shape[d] != 1) return fail(RMHIP_ERR_INVALID, "conv2d: input must be 2-D");
    auto rows_cols = [](const Buffer& x, u64* r, u64* cc) {  // simple_provider.rs:2402-2408
        *r = x.shape.empty() ? 1 : x.shape[0];
        *cc = x.shape.size() < 2 ? 1 : x.shape[1];
    };
    u64 ar_n, ac_n, br_n, bc_n;
    rows_cols(ab, &ar_n, &ac_n);
    rows_cols(bb, &br_n, &bc_n);
    u64 r0 = 0, c0 = 0, rows = 0, cols = 0;
    if (ab.numel == 0 || bb.numel == 0) {  // simple_provider.rs:6079-6093: [0, 0], or the signal's shape for 'same' (no points either way)
        if (mode == 1) rows = ar_n, cols = ac_n;
    } else {
        rows = ar_n + br_n - 1, cols = ac_n + bc_n - 1;
        if (mode == 1) r0 = (br_n - 1) / 2, c0 = (bc_n - 1) / 2, rows = ar_n, cols = ac_n;
        if (mode == 2) {
            if (ar_n < br_n || ac_n < bc_n) rows = cols = 0;
            else r0 = br_n - 1, c0 = bc_n - 1, rows = ar_n - br_n + 1, cols = ac_n - bc_n + 1;
        }
    }
    const size_t shape[2] = {(size_t)rows, (size_t)cols};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(shape, 2, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    if (ob.numel > 0x7fffffffull * kB) {  // (the output is registered by now: released here, the caller never learns its id)
        const size_t too_many = ob.numel;
        (void)rmhip_free(ctx, *out);
        *out = 0;
        return fail(RMHIP_ERR_UNSUPPORTED, "conv2d: %zu outputs", too_many);
    }
    const size_t patch_bytes = (size_t)(CONV_TX + br_n - 1) * (size_t)(CONV_TY + bc_n - 1) * sizeof(double);
    const u64 tiles_y = (cols + CONV_TY - 1) / CONV_TY;
    if (br_n <= 64 && bc_n <= 512 && patch_bytes <= 48u * 1024 && tiles_y <= 65535) {
        const dim3 grid((unsigned)((rows + CONV_TX - 1) / CONV_TX), (unsigned)tiles_y);
        hipLaunchKernelGGL(k_conv2d_tile, grid, dim3(kB), patch_bytes, c->stream, ab.data(), ar_n, ac_n, bb.data(), (int)br_n, (int)bc_n, r0, c0, rows, cols, ob.data());
        c->tel.kernel_launches++;
        RMHIP_HIP_CHECK(hipGetLastError());
        return RMHIP_OK;
    }
    const int in_lds = bb.numel <= LDS_TAPS;
    hipLaunchKernelGGL(k_conv2d, dim3(grid_for(ob.numel)), dim3(kB), in_lds ? bb.numel * sizeof(double) : 0, c->stream, ab.data(), ar_n, ac_n, bb.data(), br_n, bc_n, r0, c0,
                       rows, cols, in_lds, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

namespace rmhip {
namespace {
// What both moving_window entry points make of a request: the operand, the geometry along `dim`, and the refusals they share, in one order
int moving_prepare(Context* c, rmhip_buf a, int dim, size_t before, size_t after, int op, int endpoints, double fill, int nan_omit, int population,
                   const size_t* out_shape, size_t out_rank, rmhip_buf* out, Buffer* ab, MovingArgs* args) {
    if (!out || (out_rank && !out_shape)) return fail(RMHIP_ERR_INVALID, "moving_window: null argument");
    if (dim < 0 || op < 0 || op > 7 || endpoints < 0 || endpoints > 2) return fail(RMHIP_ERR_INVALID, "moving_window: dim %d, op %d, endpoints %d", dim, op, endpoints);
    RMHIP_TRY(c->get(a, ab));
    std::vector<size_t> shape = ab->shape;
    if ((size_t)dim >= shape.size()) shape.resize(dim + 1, 1);  // simple_provider.rs:1266-1269
    if ((size_t)dim >= out_rank) return fail(RMHIP_ERR_INVALID, "moving_window: dimension exceeds tensor rank");
    // the caller's output shape (moving.rs:1545-1570): the input's, the dimension trimmed by before + after for 'discard'
    std::vector<size_t> want = shape;
    if (endpoints == 1) want[dim] = shape[dim] > before + after ? shape[dim] - before - after : 0;
    std::vector<size_t> given(out_shape, out_shape + out_rank), wanted = want;  // compared without trailing singleton dimensions beyond `dim`
    while (given.size() > (size_t)dim + 1 && given.back() == 1) given.pop_back();
    while (wanted.size() > (size_t)dim + 1 && wanted.back() == 1) wanted.pop_back();
    if (given != wanted) return fail(RMHIP_ERR_SHAPE, "moving_window: output shape does not match the request");
    MovingArgs& A = *args;
    A = MovingArgs{};
    A.pre = 1, A.post = 1;
    for (int k = 0; k < dim; ++k) A.pre *= shape[k];
    for (size_t k = dim + 1; k < shape.size(); ++k) A.post *= shape[k];
    A.len = shape[dim], A.out_len = want[dim], A.before = before, A.after = after;
    A.op = op, A.endpoints = endpoints, A.nan_omit = nan_omit ? 1 : 0, A.population = population ? 1 : 0, A.fill = fill;
    if (before > (1ull << 30) || after > (1ull << 30)) return fail(RMHIP_ERR_UNSUPPORTED, "moving_window: window %zu + %zu", before, after);
    return RMHIP_OK;
}
}  // namespace
}  // namespace rmhip

int rmhip_moving_window(rmhip_ctx* ctx, rmhip_buf a, int dim, size_t before, size_t after, int op, int endpoints, double fill, int nan_omit, int population,
                        const size_t* out_shape, size_t out_rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    Buffer ab;
    MovingArgs A;
    RMHIP_TRY(moving_prepare(c, a, dim, before, after, op, endpoints, fill, nan_omit, population, out_shape, out_rank, out, &ab, &A));
    if (op == 5 && std::min<u64>(A.len, before + after + 1) > (u64)MED_MAX)
        return fail(RMHIP_ERR_UNSUPPORTED, "moving_window: median over windows of more than %d points", MED_MAX);
    // prod with padding multiplies by fill^count (`powf`, moving.rs:991): only fills whose every power is the fill itself stay exact
    if (op == 2 && endpoints == 2 && !(fill == 0.0 || fill == 1.0 || std::isnan(fill)))
        return fail(RMHIP_ERR_UNSUPPORTED, "moving_window: product with a padding value other than 0, 1 or NaN");
    Buffer ob;
    RMHIP_TRY(c->new_buffer(out_shape, out_rank, out, &ob));
    A.total = ob.numel;
    if (ob.numel == 0) return RMHIP_OK;
    if (ob.numel > 0x7fffffffull * kB) {  // (the output is registered by now: released here, the caller never learns its id)
        const size_t too_many = ob.numel;
        (void)rmhip_free(ctx, *out);
        *out = 0;
        return fail(RMHIP_ERR_UNSUPPORTED, "moving_window: %zu outputs", too_many);
    }
    const dim3 grid(grid_for(ob.numel)), block(kB);
    switch (op) {
        case 0: hipLaunchKernelGGL(k_moving<0>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 1: hipLaunchKernelGGL(k_moving<1>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 2: hipLaunchKernelGGL(k_moving<2>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 3: hipLaunchKernelGGL(k_moving<3>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 4: hipLaunchKernelGGL(k_moving<4>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 5: hipLaunchKernelGGL(k_moving<5>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        case 6: hipLaunchKernelGGL(k_moving<6>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
        default: hipLaunchKernelGGL(k_moving<7>, grid, block, 0, c->stream, ab.data(), A, ob.data()); break;
    }
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_moving_window_long(rmhip_ctx* ctx, rmhip_buf a, int dim, size_t before, size_t after, int op, int endpoints, double fill, int nan_omit, int population,
                             const size_t* out_shape, size_t out_rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    Buffer ab;
    MovingArgs A;
    RMHIP_TRY(moving_prepare(c, a, dim, before, after, op, endpoints, fill, nan_omit, population, out_shape, out_rank, out, &ab, &A));
    if (op != 5) return fail(RMHIP_ERR_UNSUPPORTED, "moving_window_long: the median only; rmhip_moving_window serves op %d for every window", op);
    const u64 weff = std::min<u64>(A.len, before + after + 1);
    if (weff > MEDL_W) return fail(RMHIP_ERR_UNSUPPORTED, "moving_window_long: median over windows of more than %llu points", MEDL_W);
    const u64 lines = A.pre * A.post, outputs = lines * A.out_len;
    if (weff && outputs > (1ull << 36) / weff) return fail(RMHIP_ERR_UNSUPPORTED, "moving_window_long: %llu outputs of %llu window points", outputs, weff);
    // tiles of MEDL_T outputs, shorter ones while they would leave compute units without a workgroup
    MedLongArgs M{};
    M.T = MEDL_T;
    while (M.T > 64 && lines * ((A.out_len + M.T - 1) / M.T) < 1024) M.T /= 2;
    M.tiles = (A.out_len + M.T - 1) / M.T;
    const u64 blocks = lines * M.tiles;
    if (blocks > 0x7fffffffull) return fail(RMHIP_ERR_UNSUPPORTED, "moving_window_long: %llu workgroups", blocks);
    Buffer ob;
    RMHIP_TRY(c->new_buffer(out_shape, out_rank, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    M.pre = A.pre, M.len = A.len, M.out_len = A.out_len, M.before = before, M.after = after;
    M.endpoints = endpoints, M.nan_omit = A.nan_omit, M.fill = fill;
    const u64 span = std::min<u64>(A.len, (u64)M.T + before + after);  // the most samples a tile's windows cover
    const size_t lds = MEDL_HIST + span * sizeof(u64);
    // launches of at most 2^32 window points each, so that no single launch runs long
    const u64 per = std::max<u64>(1, (1ull << 32) / (std::min<u64>(M.T, A.out_len) * weff));
    for (u64 b0 = 0; b0 < blocks; b0 += per) {
        hipLaunchKernelGGL(k_movmed_long, dim3((unsigned)std::min<u64>(per, blocks - b0)), dim3(kB), lds, c->stream, ab.data(), M, b0, ob.data());
        c->tel.kernel_launches++;
    }
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

namespace {
using namespace rmhip;

// What both filter entry points make of a request: operands, geometry along `dim`, the state shape and the normalised coefficients
// (coef[0 .. order): b, coef[order .. 2 order): a with a(1) = 1)
struct IirRequest {
    Buffer xb, zb;
    bool has_zi = false;
    size_t order = 0, state_len = 0;
    // 2 for a complex-interleaved signal: a complex tensor of shape S filtered along `dim` is, byte for byte, the real tensor [2, S...]
    // filtered along dim + 1 (and so are zi and zf), so `leading` and `channels` are twice the logical ones and every kernel below runs
    // the real recurrence on each part - the parts never meet (simple_provider.rs:6367-6379)
    size_t lanes = 1;
    u64 leading = 1, dim_len = 0, channels = 0;
    size_t raw(const Buffer& b) const { return lanes * b.numel; }  // doubles in a signal-shaped or state-shaped tensor
    std::vector<size_t> zshape;
    std::vector<double> coef;
};

// The validation and normalisation of `iir_filter` (filter.rs:1119-1138), shared by rmhip_iir_filter and rmhip_iir_filter_long;
// `few_channels_ok`: the long form, which keeps the shapes the one-thread-per-channel form declines.  `cplx`: the call came through
// rmhip_complex_iir_filter(_long): the signal and the initial states are complex-interleaved, the coefficients real.
int iir_prepare(Context* c, bool cplx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, bool few_channels_ok, IirRequest* r) {
    Buffer bb, ab;
    if (cplx) {
        RMHIP_TRY(c->lookup(x, &r->xb));
        if (!r->xb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_iir_filter: tensor %llu is real (rmhip_iir_filter serves it)", (unsigned long long)x);
        RMHIP_TRY(c->lookup(b, &bb));
        RMHIP_TRY(c->lookup(a, &ab));
        if (bb.cplx || ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: complex filter coefficients are not supported");
        if (zi_or_0) {
            RMHIP_TRY(c->lookup(zi_or_0, &r->zb));
            if (!r->zb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: initial conditions storage must match the signal");
        }
        r->lanes = 2;
    }
    RMHIP_TRY(c->get(b, &bb));
    RMHIP_TRY(c->get(a, &ab));
    if (!cplx) RMHIP_TRY(c->get(x, &r->xb));
    const Buffer& xb = r->xb;
    const size_t nb = bb.numel, na = unit_denominator ? 1 : ab.numel;
    if (nb == 0) return fail(RMHIP_ERR_INVALID, "iir_filter: numerator coefficients must not be empty");
    if (ab.numel == 0) return fail(RMHIP_ERR_INVALID, "iir_filter: denominator coefficients must not be empty");
    if (unit_denominator && ab.numel != 1) return fail(RMHIP_ERR_INVALID, "iir_filter: unit-denominator FIR path requires scalar denominator");
    const size_t order = std::max(nb, na), state_len = order - 1;
    r->order = order, r->state_len = state_len;
    if (order > 64) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: order %zu", order);
    std::vector<size_t> shape = xb.shape;
    if ((size_t)dim >= shape.size()) shape.resize(dim + 1, 1);
    u64 leading = 1, trailing = 1;
    for (int k = 0; k < dim; ++k) leading *= shape[k];
    for (size_t k = dim + 1; k < shape.size(); ++k) trailing *= shape[k];
    const u64 dim_len = shape[dim], channels = leading * trailing;
    r->leading = leading, r->dim_len = dim_len, r->channels = channels;
    // a recurrence per channel: one thread per channel leaves the chip idle when there are few - rmhip_iir_filter_long keeps those
    if (!few_channels_ok && state_len > 0 && channels < 256 && xb.numel > 4096) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: %llu channels", channels);
    std::vector<size_t>& zshape = r->zshape;  // filter_state_shape, filter.rs:1311-1319
    zshape = shape;
    zshape[dim] = state_len;
    if (zi_or_0) {
        if (!cplx) RMHIP_TRY(c->get(zi_or_0, &r->zb));
        r->has_zi = true;
        const Buffer& zb = r->zb;
        const size_t rk = std::max(zshape.size(), zb.shape.size());
        for (size_t k = 0; k < rk; ++k)
            if ((k < zshape.size() ? zshape[k] : 1) != (k < zb.shape.size() ? zb.shape[k] : 1))
                return fail(RMHIP_ERR_SHAPE, "iir_filter: initial conditions are not compatible with the signal shape");
    }
    // coefficients: read back (<= 128 doubles), normalised as the CPU's complex division by (a0 + 0i) rounds them (filter.rs:1119-1138)
    std::vector<double> hb(nb), ha(ab.numel);
    std::vector<double>& coef = r->coef;
    coef.assign(2 * order, 0.0);
    RMHIP_HIP_CHECK(hipMemcpyAsync(hb.data(), bb.data(), nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipMemcpyAsync(ha.data(), ab.data(), ab.numel * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    const double a0 = unit_denominator ? 1.0 : ha[0];
    if (a0 == 0.0) return fail(RMHIP_ERR_INVALID, "iir_filter: denominator coefficient a(1) must be non-zero");
    const double den = a0 * a0 + 0.0;
    for (size_t i = 0; i < nb; ++i) coef[i] = (hb[i] * a0 + 0.0) / den;
    coef[order] = 1.0;
    for (size_t i = 1; i < na; ++i) coef[order + i] = (ha[i] * a0 + 0.0) / den;
    r->leading *= r->lanes, r->channels *= r->lanes;  // (the few-channels decline above counted logical channels and elements)
    return RMHIP_OK;
}

// k_iir on `channels` lines of `dim_len` samples, `coef_dev` the 2 * order normalised coefficients on the device
int iir_launch_sequential(Context* c, const double* x, const double* zi, const double* coef_dev, size_t order, u64 leading, u64 dim_len, u64 channels, double* y,
                          double* zf) {
    if (order <= 8) hipLaunchKernelGGL(k_iir<8>, dim3(grid_for(channels)), dim3(kB), 0, c->stream, x, zi, coef_dev, (int)order, leading, dim_len, channels, y, zf);
    else hipLaunchKernelGGL(k_iir<64>, dim3(grid_for(channels)), dim3(kB), 0, c->stream, x, zi, coef_dev, (int)order, leading, dim_len, channels, y, zf);
    c->tel.kernel_launches++;
    return hipGetLastError() == hipSuccess ? RMHIP_OK : fail(RMHIP_ERR_HIP, "iir_filter: launch failed");
}

// The bit-exact forms: the gain kernel without states, the initial states handed on for an empty signal, else k_iir with one thread per
// channel.  Fills the two output buffers the caller created.
int iir_run_sequential(Context* c, const IirRequest& r, const Buffer& yb, const Buffer& fb) {
    const Buffer& xb = r.xb;
    if (r.state_len == 0) {
        if (yb.numel) return launch_scalar(c, RMHIP_SMUL, xb.data(), r.coef[0], yb.data(), r.raw(yb));  // gain * x (filter.rs:1172-1176)
    } else if (r.has_zi && (r.dim_len == 0 || r.channels == 0)) {
        if (fb.numel) RMHIP_HIP_CHECK(hipMemcpyAsync(fb.data(), r.zb.data(), r.raw(fb) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    } else if (r.channels > 0) {
        std::shared_ptr<Allocation> dc;
        RMHIP_TRY(c->alloc_device(2 * r.order, &dc));
        // (pageable source: the copy is staged before the call returns, so `coef` may go out of scope)
        RMHIP_HIP_CHECK(hipMemcpyAsync(dc->ptr, r.coef.data(), 2 * r.order * sizeof(double), hipMemcpyHostToDevice, c->stream));
        const int rc = iir_launch_sequential(c, xb.data(), r.has_zi ? r.zb.data() : nullptr, dc->ptr, r.order, r.leading, r.dim_len, r.channels, yb.data(), fb.data());
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the coefficient block is released on return
        return rc;
    }
    return RMHIP_OK;
}

constexpr u64 IIRL_CHUNKS[] = {256, 512, 1024, 2048, 4096, 8192};

// FIR: the nested sum per output sample and per final state
int iir_run_fir(Context* c, const IirRequest& r, const double* coef_dev, const Buffer& yb, const Buffer& fb) {
    const double* zi = r.has_zi ? r.zb.data() : nullptr;
    const u64 tiles = r.leading == 1 ? (r.dim_len + kB - 1) / kB : 0;  // the contiguous dimension: a block per tile of a channel
    const u64 blocks = tiles ? tiles * r.channels : grid_for(r.raw(yb));
    hipLaunchKernelGGL(k_fir_long, dim3(blocks), dim3(kB), 0, c->stream, r.xb.data(), zi, coef_dev, (int)r.order, r.leading, r.dim_len, (u64)r.raw(yb), tiles,
                       yb.data(), c->verdict_word);
    hipLaunchKernelGGL(k_fir_long_state, dim3(grid_for(r.raw(fb))), dim3(kB), 0, c->stream, r.xb.data(), zi, coef_dev, (int)r.order, r.leading, r.dim_len,
                       (u64)r.raw(fb), fb.data(), c->verdict_word);
    c->tel.kernel_launches += 2;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

// Recursive: the chunked scan.  *declined: no chunk length is admissible.  *sequential: the signal is too short for two chunks of the
// first admissible length, nothing was launched on the outputs.
int iir_run_chunked(Context* c, const IirRequest& r, const double* coef_dev, const Buffer& yb, const Buffer& fb, bool* declined, bool* sequential) {
    const u64 S = r.state_len, N = r.dim_len;
    *declined = *sequential = false;
    u64 lmax = 0;
    for (u64 cand : IIRL_CHUNKS)
        if (2 * cand <= N) lmax = cand;
    // tables: S runs of the recurrence over `L` zeros from the unit states - their outputs are H (H[k + L i]), their final states T_L
    std::shared_ptr<Allocation> zeros, eye, H, T;
    RMHIP_TRY(c->alloc_device(lmax * S, &zeros));
    RMHIP_TRY(c->alloc_device(lmax * S, &H));
    RMHIP_TRY(c->alloc_device(S * S, &eye));
    RMHIP_TRY(c->alloc_device(S * S, &T));
    std::vector<double> host(S * S, 0.0);
    for (u64 i = 0; i < S; ++i) host[i + S * i] = 1.0;
    RMHIP_HIP_CHECK(hipMemsetAsync(zeros->ptr, 0, lmax * S * sizeof(double), c->stream));
    RMHIP_HIP_CHECK(hipMemcpyAsync(eye->ptr, host.data(), S * S * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // `host` is reused for T below
    u64 L = 0;
    for (u64 cand : IIRL_CHUNKS) {
        if (cand > lmax) break;
        RMHIP_TRY(iir_launch_sequential(c, zeros->ptr, eye->ptr, coef_dev, r.order, 1, cand, S, H->ptr, T->ptr));
        RMHIP_HIP_CHECK(hipMemcpyAsync(host.data(), T->ptr, S * S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
        // admissible: T_L finite and contractive in the infinity norm of |T_L| - a state error is not amplified from chunk to chunk
        double worst = 0.0;
        for (u64 j = 0; j < S; ++j) {
            double sum = 0.0;
            for (u64 i = 0; i < S; ++i) sum += std::fabs(host[j + S * i]);
            worst = std::isfinite(sum) ? std::max(worst, sum) : INFINITY;
        }
        if (worst <= 1.0) {
            L = cand;
            break;
        }
    }
    if (L == 0) {
        if (lmax == IIRL_CHUNKS[5]) *declined = true;
        else *sequential = true;
        return RMHIP_OK;
    }
    const u64 nfull = N / L, tail = N - nfull * L, slots = nfull + 1;
    std::shared_ptr<Allocation> states;
    RMHIP_TRY(c->alloc_device(r.channels * slots * S, &states));
    const double* zi = r.has_zi ? r.zb.data() : nullptr;
    const double* x = r.xb.data();
    const u64 pairs = r.channels * nfull, ktiles = L / IIRL_KT;
    const u64 wave_rows = (pairs + kB / 64 - 1) / (kB / 64);
    const unsigned gy = (unsigned)std::min<u64>(wave_rows, std::max<u64>(1, 4096 / ktiles));
    auto launch = [&](auto maxo) {  // the four phases, states and coefficients in registers up to order 8
        constexpr int MAXO = decltype(maxo)::value;
        hipLaunchKernelGGL(k_iir_chunks<MAXO>, dim3(grid_for(pairs)), dim3(kB), 0, c->stream, x, coef_dev, (int)r.order, r.leading, N, r.channels, (u64)0, L, nfull,
                           slots, 0, states->ptr, yb.data(), (double*)nullptr, c->verdict_word);
        hipLaunchKernelGGL(k_iir_states<MAXO - 1>, dim3(r.channels), dim3(64), 0, c->stream, T->ptr, zi, (int)S, r.leading, nfull, states->ptr, c->verdict_word);
        hipLaunchKernelGGL(k_iir_correct<MAXO - 1>, dim3(ktiles, gy), dim3(kB), 0, c->stream, H->ptr, (int)S, L, r.leading, N, r.channels, nfull, states->ptr,
                           yb.data(), c->verdict_word);
        hipLaunchKernelGGL(k_iir_chunks<MAXO>, dim3(grid_for(r.channels)), dim3(kB), 0, c->stream, x, coef_dev, (int)r.order, r.leading, N, r.channels, nfull * L,
                           tail, (u64)1, slots, 1, states->ptr, yb.data(), fb.data(), c->verdict_word);
    };
    if (r.order <= 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 64>{});
    c->tel.kernel_launches += 4;
    RMHIP_HIP_CHECK(hipGetLastError());
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the tables and the states are released on return
    return RMHIP_OK;
}
}  // namespace

namespace {
// A signal-shaped or state-shaped result: real, or complex-interleaved when the signal is
int iir_new_result(Context* c, const IirRequest& r, const std::vector<size_t>& shape, rmhip_buf* id, Buffer* out) {
    return r.lanes == 2 ? c->new_buffer_complex(shape.data(), shape.size(), id, out) : c->new_buffer(shape.data(), shape.size(), id, out);
}
// A precision-32 context rounds the parts of a complex result through f32 once, after the last f64 operation (real results are narrowed
// by the entry point's scope)
int iir_round_results(Context* c, const IirRequest& r, const Buffer& yb, const Buffer& fb) {
    if (r.lanes != 2 || c->precision != 32) return RMHIP_OK;
    RMHIP_TRY(launch_round_f32(c, yb.data(), r.raw(yb)));
    return launch_round_f32(c, fb.data(), r.raw(fb));
}

// `cplx`: the call came through rmhip_complex_iir_filter
int iir_filter_any(rmhip_ctx* ctx, Context* c, bool cplx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, rmhip_buf* output,
                   rmhip_buf* final_state) {
    if (!output || !final_state) return fail(RMHIP_ERR_INVALID, "iir_filter: null output");
    if (dim < 0) return fail(RMHIP_ERR_INVALID, "iir_filter: dim must be >= 0");
    *output = *final_state = 0;
    IirRequest r;
    RMHIP_TRY(iir_prepare(c, cplx, b, a, x, dim, zi_or_0, unit_denominator, false, &r));
    Buffer yb, fb;
    RMHIP_TRY(iir_new_result(c, r, r.xb.shape, output, &yb));
    int rc = iir_new_result(c, r, r.zshape, final_state, &fb);
    if (rc == RMHIP_OK) rc = iir_run_sequential(c, r, yb, fb);
    if (rc == RMHIP_OK) rc = iir_round_results(c, r, yb, fb);
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *output);
        if (*final_state) rmhip_free(ctx, *final_state);
        *output = *final_state = 0;
    }
    return rc;
}

// `cplx`: the call came through rmhip_complex_iir_filter_long
int iir_filter_long_any(rmhip_ctx* ctx, Context* c, bool cplx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator,
                        rmhip_buf* output, rmhip_buf* final_state) {
    if (!output || !final_state) return fail(RMHIP_ERR_INVALID, "iir_filter: null output");
    if (dim < 0) return fail(RMHIP_ERR_INVALID, "iir_filter: dim must be >= 0");
    *output = *final_state = 0;
    IirRequest r;
    RMHIP_TRY(iir_prepare(c, cplx, b, a, x, dim, zi_or_0, unit_denominator, true, &r));
    if (r.raw(r.xb) > 0x7fffffffull * kB) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: %zu samples", r.xb.numel);
    bool fir = true, finite = true;
    for (size_t i = 0; i < 2 * r.order; ++i) finite = finite && std::isfinite(r.coef[i]);
    for (size_t i = 1; i < r.order; ++i) fir = fir && r.coef[r.order + i] == 0.0;
    // too short to form two chunks of the shortest length, no states, nothing to filter: the bit-exact forms
    const bool plain = r.state_len == 0 || r.channels == 0 || r.dim_len < 2 * IIRL_CHUNKS[0];
    if (!plain && !finite) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: non-finite coefficients");
    Buffer yb, fb;
    RMHIP_TRY(iir_new_result(c, r, r.xb.shape, output, &yb));
    int rc = iir_new_result(c, r, r.zshape, final_state, &fb);
    auto chunked = [&]() -> int {
        if (!c->verdict_word) RMHIP_HIP_CHECK(hipMalloc((void**)&c->verdict_word, sizeof(unsigned)));
        RMHIP_HIP_CHECK(hipMemsetAsync(c->verdict_word, 0xff, sizeof(unsigned), c->stream));
        std::shared_ptr<Allocation> dc;
        RMHIP_TRY(c->alloc_device(2 * r.order, &dc));
        RMHIP_HIP_CHECK(hipMemcpyAsync(dc->ptr, r.coef.data(), 2 * r.order * sizeof(double), hipMemcpyHostToDevice, c->stream));
        bool declined = false, sequential = false;
        if (fir) RMHIP_TRY(iir_run_fir(c, r, dc->ptr, yb, fb));
        else RMHIP_TRY(iir_run_chunked(c, r, dc->ptr, yb, fb, &declined, &sequential));
        unsigned code = 0;
        RMHIP_HIP_CHECK(hipMemcpyAsync(&code, c->verdict_word, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the verdict is part of the answer; the coefficient block is released on return
        if (declined) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: filter is not contractive over a chunk");
        if (sequential) return iir_run_sequential(c, r, yb, fb);
        if (code == 0) return fail(RMHIP_ERR_UNSUPPORTED, "iir_filter: a non-finite value in the signal, the initial states or the result");
        return RMHIP_OK;
    };
    if (rc == RMHIP_OK) rc = plain ? iir_run_sequential(c, r, yb, fb) : chunked();
    if (rc == RMHIP_OK) rc = iir_round_results(c, r, yb, fb);
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *output);
        if (*final_state) rmhip_free(ctx, *final_state);
        *output = *final_state = 0;
    }
    return rc;
}
}  // namespace

int rmhip_iir_filter(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, rmhip_buf* output,
                     rmhip_buf* final_state) {
    CTX_OR_FAIL(ctx);
    return iir_filter_any(ctx, c, false, b, a, x, dim, zi_or_0, unit_denominator, output, final_state);
}
int rmhip_complex_iir_filter(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, rmhip_buf* output,
                             rmhip_buf* final_state) {
    CTX_OR_FAIL(ctx);
    return iir_filter_any(ctx, c, true, b, a, x, dim, zi_or_0, unit_denominator, output, final_state);
}
int rmhip_iir_filter_long(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, rmhip_buf* output,
                          rmhip_buf* final_state) {
    CTX_OR_FAIL(ctx);
    return iir_filter_long_any(ctx, c, false, b, a, x, dim, zi_or_0, unit_denominator, output, final_state);
}
int rmhip_complex_iir_filter_long(rmhip_ctx* ctx, rmhip_buf b, rmhip_buf a, rmhip_buf x, int dim, rmhip_buf zi_or_0, int unit_denominator, rmhip_buf* output,
                                  rmhip_buf* final_state) {
    CTX_OR_FAIL(ctx);
    return iir_filter_long_any(ctx, c, true, b, a, x, dim, zi_or_0, unit_denominator, output, final_state);
}

int rmhip_imfilter(rmhip_ctx* ctx, rmhip_buf image, rmhip_buf kernel, int padding, double constant_value, int shape_mode, int convolution, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (padding < 0 || padding > 3 || shape_mode < 0 || shape_mode > 2) return fail(RMHIP_ERR_INVALID, "imfilter: padding %d / shape %d", padding, shape_mode);
    Buffer ib, kb, ob;
    RMHIP_TRY(c->get(image, &ib));
    RMHIP_TRY(c->get(kernel, &kb));
    if (kb.numel == 0) return fail(RMHIP_ERR_INVALID, "imfilter: filter must be non-empty along every dimension");  // imfilter.rs:482-487
    std::vector<size_t> ishape = ib.shape.empty() ? std::vector<size_t>{1, 1} : ib.shape, kshape = kb.shape.empty() ? std::vector<size_t>{1, 1} : kb.shape;
    const size_t rank = std::max(ishape.size(), kshape.size());
    if (rank > 4) return fail(RMHIP_ERR_UNSUPPORTED, "imfilter: %zu dimensions", rank);
    for (size_t d = 0; d < kshape.size(); ++d) {  // validate_kernel_shape, imfilter.rs:567-593
        if (d >= ishape.size() && kshape[d] > 1)
            return fail(RMHIP_ERR_INVALID, "imfilter: filter dimension %zu is %zu, but the image has no corresponding axis", d + 1, kshape[d]);
        if ((d < ishape.size() ? ishape[d] : 1) == 0) return fail(RMHIP_ERR_INVALID, "imfilter: image must not have zero-length dimensions");
    }
    ImfArgs A{};
    A.rank = (int)rank, A.padding = padding, A.convolution = convolution ? 1 : 0, A.constant = constant_value;
    std::vector<size_t> oshape(rank);
    u64 is = 1, ks = 1;
    for (size_t d = 0; d < 4; ++d) {
        const long long img = d < ishape.size() ? (long long)ishape[d] : 1, ker = d < kshape.size() ? (long long)kshape[d] : 1;
        A.img[d] = img, A.ker[d] = ker, A.origin[d] = ker / 2;
        A.istride[d] = is, A.kstride[d] = ks;
        is *= (u64)img, ks *= (u64)ker;
        long long o = img, base = 0;                                              // same
        if (shape_mode == 1) o = img + ker - 1, base = A.origin[d] - (ker - 1);   // full
        if (shape_mode == 2) o = img >= ker ? img - ker + 1 : 0, base = A.origin[d];  // valid
        A.out[d] = o, A.base[d] = base;
        if (d < rank) oshape[d] = (size_t)o;
    }
    while (oshape.size() > ishape.size() && oshape.back() == 1) oshape.pop_back();  // imfilter.rs:526-532
    if (oshape.empty()) oshape.push_back(1);
    RMHIP_TRY(c->new_buffer(oshape.data(), oshape.size(), out, &ob));
    A.total = ob.numel;
    if (ob.numel == 0) return RMHIP_OK;
    if (ob.numel > 0x7fffffffull * kB) {  // (the output is registered by now: released here, the caller never learns its id)
        const size_t too_many = ob.numel;
        (void)rmhip_free(ctx, *out);
        *out = 0;
        return fail(RMHIP_ERR_UNSUPPORTED, "imfilter: %zu outputs", too_many);
    }
    for (int d = 0; d < 4; ++d)
        if (A.out[d] == 0) A.out[d] = 1;  // (never reached with numel > 0)
    const u64 planes = (u64)A.out[2] * (u64)A.out[3];  // with a two-dimensional filter every further image dimension is a batch of planes
    const size_t patch_bytes = (size_t)(IMF_TX + A.ker[0] - 1) * (size_t)(IMF_TY + A.ker[1] - 1) * sizeof(double);
    const u64 tiles_y = ((u64)A.out[1] + IMF_TY - 1) / IMF_TY;
    if (A.ker[2] == 1 && A.ker[3] == 1 && A.ker[0] <= 64 && patch_bytes <= 48u * 1024 && tiles_y <= 65535 && planes <= 65535) {
        const dim3 grid((unsigned)(((u64)A.out[0] + IMF_TX - 1) / IMF_TX), (unsigned)tiles_y, (unsigned)planes);
        hipLaunchKernelGGL(k_imfilter_tile, grid, dim3(kB), patch_bytes, c->stream, ib.data(), kb.data(), A, ob.data());
        c->tel.kernel_launches++;
        RMHIP_HIP_CHECK(hipGetLastError());
        return RMHIP_OK;
    }
    const int in_lds = kb.numel <= LDS_TAPS;
    hipLaunchKernelGGL(k_imfilter, dim3(grid_for(ob.numel)), dim3(kB), in_lds ? kb.numel * sizeof(double) : 0, c->stream, ib.data(), kb.data(), A, in_lds, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_interp1(rmhip_ctx* ctx, rmhip_buf x, rmhip_buf y, rmhip_buf xq, size_t sample_len, size_t series_count, size_t query_len, const size_t* output_shape,
                  size_t out_rank, int nearest, int extrapolation, double extrapolation_value, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out || (out_rank && !output_shape)) return fail(RMHIP_ERR_INVALID, "interp1: null argument");
    if (extrapolation < 0 || extrapolation > 2) return fail(RMHIP_ERR_INVALID, "interp1: extrapolation %d", extrapolation);
    if (sample_len < 2) return fail(RMHIP_ERR_INVALID, "interp1: sample_len must be at least 2");
    if (series_count < 1) return fail(RMHIP_ERR_INVALID, "interp1: series_count must be positive");
    Buffer xb, yb, qb;
    RMHIP_TRY(c->get(x, &xb));
    RMHIP_TRY(c->get(y, &yb));
    RMHIP_TRY(c->get(xq, &qb));
    u64 olen = 1;
    for (size_t d = 0; d < out_rank; ++d) olen *= output_shape[d];
    if (olen != (u64)query_len * series_count) return fail(RMHIP_ERR_SHAPE, "interp1: output shape does not match query/series count");
    if (xb.numel != sample_len) return fail(RMHIP_ERR_SHAPE, "interp1: X length does not match sample_len");
    if (yb.numel != sample_len * series_count) return fail(RMHIP_ERR_SHAPE, "interp1: Y length does not match sample/series count");
    if (qb.numel != query_len) return fail(RMHIP_ERR_SHAPE, "interp1: Xq length does not match query_len");
    Buffer ob;
    RMHIP_TRY(c->new_buffer(output_shape, out_rank, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    if (ob.numel > 0x7fffffffull * kB) {  // (the output is registered by now: released here, the caller never learns its id)
        const size_t too_many = ob.numel;
        (void)rmhip_free(ctx, *out);
        *out = 0;
        return fail(RMHIP_ERR_UNSUPPORTED, "interp1: %zu outputs", too_many);
    }
    hipLaunchKernelGGL(k_interp1, dim3(grid_for(ob.numel)), dim3(kB), 0, c->stream, xb.data(), yb.data(), qb.data(), (u64)sample_len, (u64)query_len, (u64)ob.numel, nearest ? 1 : 0,
                       extrapolation, extrapolation_value, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_polyval(rmhip_ctx* ctx, rmhip_buf coefficients, rmhip_buf points, int has_mu, double mean, double scale, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer cb, xb;
    RMHIP_TRY(c->get(coefficients, &cb));
    RMHIP_TRY(c->get(points, &xb));
    Buffer ob;
    RMHIP_TRY(c->new_buffer(xb.shape.data(), xb.shape.size(), out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    if (ob.numel > 0x7fffffffull * kB) return fail(RMHIP_ERR_UNSUPPORTED, "polyval: %zu points", ob.numel);
    std::shared_ptr<Allocation> flag;
    RMHIP_TRY(c->alloc_device(1, &flag));
    RMHIP_HIP_CHECK(hipMemsetAsync(flag->ptr, 0, sizeof(double), c->stream));
    const int in_lds = cb.numel <= LDS_TAPS;
    hipLaunchKernelGGL(k_polyval, dim3(grid_for(ob.numel)), dim3(kB), in_lds ? cb.numel * sizeof(double) : 0, c->stream, cb.data(), (u64)cb.numel, xb.data(), (u64)ob.numel,
                       has_mu ? 1 : 0, mean, scale, in_lds, ob.data(), (int*)flag->ptr);
    c->tel.kernel_launches++;
    int bad = 0;
    RMHIP_HIP_CHECK(hipMemcpyAsync(&bad, flag->ptr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (bad) {  // the CPU's complex recurrence turns these into NaN + NaN i (a complex result): the caller evaluates on the host
        rmhip_free(ctx, *out);
        *out = 0;
        return fail(RMHIP_ERR_UNSUPPORTED, "polyval: a non-finite intermediate value");
    }
    return RMHIP_OK;
}

namespace {
// poly_orientation_from_shape (simple_provider.rs:320-338): 0 scalar, 1 row, 2 column; more than one extent above 1 is not a vector
int poly_orientation(const std::vector<size_t>& shape, int* orientation) {
    int non_unit = 0;
    *orientation = 0;
    for (size_t d = 0; d < shape.size(); ++d)
        if (shape[d] > 1) ++non_unit, *orientation = d == 0 ? 2 : 1;
    return non_unit > 1 ? rmhip::fail(RMHIP_ERR_INVALID, "polyder: coefficient inputs must be vectors") : RMHIP_OK;
}

// allocate_polynomial / poly_shape_for_len (simple_provider.rs:341-348, 763-770) of work[first .. len), or of [0] when nothing is left
int poly_emit(rmhip::Context* c, const double* work, rmhip::u64 first, rmhip::u64 len, int orientation, rmhip_buf* out) {
    const rmhip::u64 kept = first < len ? len - first : 1;
    const size_t shape[2] = {orientation == 2 && kept > 1 ? (size_t)kept : 1, orientation == 2 || kept <= 1 ? 1 : (size_t)kept};
    rmhip::Buffer ob;
    RMHIP_TRY(c->new_buffer(shape, 2, out, &ob));
    if (first < len) RMHIP_HIP_CHECK(hipMemcpyAsync(ob.data(), work + first, kept * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    else RMHIP_HIP_CHECK(hipMemsetAsync(ob.data(), 0, sizeof(double), c->stream));
    return RMHIP_OK;
}

// one untrimmed result of k_poly, trimmed and emitted
int poly_run(rmhip::Context* c, const rmhip::PolyVec& p, const rmhip::PolyVec& q, int mode, rmhip::u64 len, int orientation, rmhip_buf* out) {
    using namespace rmhip;
    if (len > 0x7fffffffull * kB) return fail(RMHIP_ERR_UNSUPPORTED, "polyder: %llu coefficients", (unsigned long long)len);
    std::shared_ptr<Allocation> work;
    RMHIP_TRY(c->alloc_device(len + 1, &work));
    unsigned long long* first_dev = (unsigned long long*)(work->ptr + len);
    hipLaunchKernelGGL(k_poly, dim3(grid_for(len)), dim3(kB), 0, c->stream, p, q, mode, 0.0, len, work->ptr);
    hipLaunchKernelGGL(k_poly_first, dim3(1), dim3(kB), 0, c->stream, work->ptr, len, first_dev);
    c->tel.kernel_launches += 2;
    RMHIP_HIP_CHECK(hipGetLastError());
    unsigned long long first = 0;
    RMHIP_HIP_CHECK(hipMemcpyAsync(&first, first_dev, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the result's length is part of the answer
    return poly_emit(c, work->ptr, first, len, orientation, out);
}
}  // namespace

int rmhip_polyder(rmhip_ctx* ctx, rmhip_buf p, rmhip_buf q_or_0, int quotient, rmhip_buf* out, rmhip_buf* denominator_or_null) {
    CTX_OR_FAIL(ctx);
    if (!out || (quotient && (!q_or_0 || !denominator_or_null))) return fail(RMHIP_ERR_INVALID, "polyder: null argument");
    Buffer pb, qb;
    RMHIP_TRY(c->get(p, &pb));
    int op = 0, oq = 0;
    RMHIP_TRY(poly_orientation(pb.shape, &op));
    const PolyVec pv{pb.numel ? pb.data() : nullptr, (u64)pb.numel};
    if (!q_or_0) return poly_run(c, pv, pv, 0, pv.n <= 1 ? 1 : pv.n - 1, op, out);
    RMHIP_TRY(c->get(q_or_0, &qb));
    RMHIP_TRY(poly_orientation(qb.shape, &oq));
    const PolyVec qv{qb.numel ? qb.data() : nullptr, (u64)qb.numel};
    const u64 lp = pv.n ? pv.n : 1, lq = qv.n ? qv.n : 1, dp = pv.n <= 1 ? 1 : pv.n - 1, dq = qv.n <= 1 ? 1 : qv.n - 1;
    const u64 len = std::max(dp + lq - 1, lp + dq - 1);
    RMHIP_TRY(poly_run(c, pv, qv, quotient ? 2 : 1, len, op, out));
    if (!quotient) return RMHIP_OK;
    const int rc = poly_run(c, pv, qv, 3, 2 * lq - 1, oq, denominator_or_null);
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *out);
        *out = 0;
    }
    return rc;
}

// `cplx`: the call came through rmhip_complex_polyint, which takes complex-interleaved storage only (lengths count logical coefficients)
static int polyint_any(rmhip_ctx* ctx, Context* c, bool cplx, rmhip_buf p, double constant, rmhip_buf* out) {
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer pb;
    if (cplx) {
        *out = 0;
        RMHIP_TRY(c->lookup(p, &pb));
        if (!pb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_polyint: tensor %llu is real (rmhip_polyint serves it)", (unsigned long long)p);
    } else {
        RMHIP_TRY(c->get(p, &pb));
    }
    int orientation = 0;
    RMHIP_TRY(poly_orientation(pb.shape, &orientation));
    const u64 len = (u64)pb.numel + 1;
    if (len > 0x7fffffffull * kB) return fail(RMHIP_ERR_UNSUPPORTED, "polyint: %zu coefficients", pb.numel);
    const size_t shape[2] = {orientation == 2 && len > 1 ? (size_t)len : 1, orientation == 2 || len <= 1 ? 1 : (size_t)len};
    Buffer ob;
    if (cplx) {  // (simple_provider.rs:3205-3217: the same orientation rule on the logical length)
        RMHIP_TRY(c->new_buffer_complex(shape, 2, out, &ob));
        hipLaunchKernelGGL(k_polyint_cx, dim3(grid_for(len)), dim3(kB), 0, c->stream, reinterpret_cast<const v2d*>(pb.data()), (u64)pb.numel, constant, len,
                           c->precision == 32 ? 1 : 0, reinterpret_cast<v2d*>(ob.data()));
        c->tel.kernel_launches++;
        if (hipGetLastError() != hipSuccess) {
            rmhip_free(ctx, *out);
            *out = 0;
            return fail(RMHIP_ERR_HIP, "complex_polyint: launch failed");
        }
        return RMHIP_OK;
    }
    RMHIP_TRY(c->new_buffer(shape, 2, out, &ob));
    const PolyVec pv{pb.numel ? pb.data() : nullptr, (u64)pb.numel};
    hipLaunchKernelGGL(k_poly, dim3(grid_for(len)), dim3(kB), 0, c->stream, pv, pv, 4, constant, len, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}
int rmhip_polyint(rmhip_ctx* ctx, rmhip_buf p, double constant, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return polyint_any(ctx, c, false, p, constant, out);
}
int rmhip_complex_polyint(rmhip_ctx* ctx, rmhip_buf p, double constant, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return polyint_any(ctx, c, true, p, constant, out);
}

int rmhip_window(rmhip_ctx* ctx, int kind, size_t len, int periodic, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (kind < 0 || kind > 2) return fail(RMHIP_ERR_INVALID, "window: kind %d", kind);
    const size_t shape[2] = {len, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(shape, 2, out, &ob));
    if (len == 0) return RMHIP_OK;
    if (len == 1) return launch_fill(c, ob.data(), 1, 1.0);
    const double denom = (double)((periodic ? len + 1 : len) - 1);
    hipLaunchKernelGGL(k_window, dim3(grid_for(len)), dim3(kB), 0, c->stream, kind, (u64)len, denom, ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_signal_envelope(rmhip_ctx* ctx, rmhip_buf input, size_t channel_len, size_t channel_count, const size_t* out_shape, size_t out_rank, int method, size_t param,
                          rmhip_buf* upper, rmhip_buf* lower) {
    CTX_OR_FAIL(ctx);
    if (!upper || !lower || (out_rank && !out_shape)) return fail(RMHIP_ERR_INVALID, "signal_envelope: null argument");
    *upper = *lower = 0;
    if (method < 0 || method > 2) return fail(RMHIP_ERR_INVALID, "signal_envelope: method %d", method);
    const u64 n = channel_len, m = channel_count;
    if (n == 0 || m == 0) return fail(RMHIP_ERR_INVALID, "signal_envelope: empty signal");
    if (method != 0 && param == 0) return fail(RMHIP_ERR_INVALID, "signal_envelope: %s must be positive", method == 1 ? "filter length" : "window length");
    size_t total = 0, out_total = 1;
    if (__builtin_mul_overflow(channel_len, channel_count, &total)) return fail(RMHIP_ERR_INVALID, "signal_envelope: signal size exceeds provider limits");
    for (size_t d = 0; d < out_rank; ++d)
        if (__builtin_mul_overflow(out_total, out_shape[d], &out_total)) return fail(RMHIP_ERR_INVALID, "signal_envelope: output size exceeds provider limits");
    if (out_total != total) return fail(RMHIP_ERR_INVALID, "signal_envelope: output shape does not hold channel_len * channel_count elements");
    Buffer raw;
    RMHIP_TRY(c->lookup(input, &raw));
    if (raw.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "signal_envelope: complex input is not supported");
    if (raw.numel != total) return fail(RMHIP_ERR_INVALID, "signal_envelope: the signal holds %zu elements, the request names %zu", raw.numel, total);
    {
        const std::vector<size_t>& s = raw.shape;
        const bool matrix = s.size() == 2 && s[0] == n && s[1] == m;
        const bool vector = m == 1 && ((s.size() == 1 && s[0] == n) || (s.size() == 2 && ((s[0] == n && s[1] == 1) || (s[0] == 1 && s[1] == n))));
        if (!matrix && !vector) return fail(RMHIP_ERR_INVALID, "signal_envelope: the signal's shape is not channel_len x channel_count");
    }
    if (method == 0) {
        // what rmhip_fft_dim transforms along dimension 0: a power of two up to 2^27, any other length up to 2^23
        const bool pow2 = (n & (n - 1)) == 0;
        if (pow2 ? n > (1ull << 27) : n > (1ull << 23)) return fail(RMHIP_ERR_UNSUPPORTED, "signal_envelope: channel length %llu", n);
    } else {
        u64 work = 0;
        if (__builtin_mul_overflow(n, std::min<u64>(param, n), &work) || __builtin_mul_overflow(work, m, &work) || work > ENV_WORK_MAX)
            return fail(RMHIP_ERR_UNSUPPORTED, "signal_envelope: %llu x %llu samples under %zu taps: more than 2^36 products", n, m, param);
    }
    // a channel is summed by one wave, one workgroup, or - few long channels - by up to 64 workgroups and a second, tiny launch
    u64 parts = 1, part_len = n;
    if (n >= ENV_WAVE_MAX) {
        parts = std::min<u64>(std::min<u64>(ENV_PARTS_MAX, std::max<u64>(1, n / ENV_PART_MIN)), std::max<u64>(1, (u64)c->num_cus * 4 / m));
        part_len = (n + parts - 1) / parts;
        parts = (n + part_len - 1) / part_len;
    }
    if (total > 0x7fffffffull * kB || m * parts > 0x7fffffffull) return fail(RMHIP_ERR_UNSUPPORTED, "signal_envelope: %llu channels of %llu samples", m, n);

    Buffer xb;
    bool in32 = c->precision == 32;
    if (in32) RMHIP_TRY(get_operand(c, input, &xb, &in32));  // f32 storage read in place; anything else as f64
    else RMHIP_TRY(c->get(input, &xb));
    const bool out32 = c->precision == 32;

    std::shared_ptr<Allocation> mu, partial, taps;
    RMHIP_TRY(c->alloc_device(m, &mu));
    if (parts > 1) RMHIP_TRY(c->alloc_device(m * parts, &partial));
    if (!c->verdict_word) RMHIP_HIP_CHECK(hipMalloc((void**)&c->verdict_word, sizeof(unsigned)));
    RMHIP_HIP_CHECK(hipMemsetAsync(c->verdict_word, 0xff, sizeof(unsigned), c->stream));
    double* part_ptr = partial ? partial->ptr : nullptr;
    RMHIP_TRY(in32 ? env_means<float>(c, xb.data_f32(), n, m, mu->ptr, part_ptr, parts, part_len, c->verdict_word)
                   : env_means<double>(c, xb.data(), n, m, mu->ptr, part_ptr, parts, part_len, c->verdict_word));
    unsigned code = 0xffffffffu;  // the call's one read-back: envelope.rs raises InvalidSignal for NaN / Inf, and so does the caller's host path
    RMHIP_HIP_CHECK(hipMemcpyAsync(&code, c->verdict_word, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (code != 0xffffffffu) return fail(RMHIP_ERR_INVALID, "signal_envelope: the signal must contain finite values");

    // the taps some output can reach: t in [half - (n - 1), half + n - 1], at most 2 n - 1 of them however long the filter
    std::vector<double> host_taps;
    u64 t0 = 0;
    if (method == 1) {
        const u64 half = param / 2;
        t0 = half > n - 1 ? half - (n - 1) : 0;
        const u64 t1 = std::min<u64>(param - 1, half + (n - 1));
        host_taps.resize(t1 - t0 + 1);
        for (u64 t = t0; t <= t1; ++t) host_taps[t - t0] = env_fir_tap(t, param);
        RMHIP_TRY(c->alloc_device(host_taps.size(), &taps));
        RMHIP_HIP_CHECK(hipMemcpyAsync(taps->ptr, host_taps.data(), host_taps.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }

    Buffer ub, lb;
    int rc = out32 ? c->new_buffer_f32(out_shape, out_rank, upper, &ub) : c->new_buffer(out_shape, out_rank, upper, &ub);
    if (rc == RMHIP_OK) rc = out32 ? c->new_buffer_f32(out_shape, out_rank, lower, &lb) : c->new_buffer(out_shape, out_rank, lower, &lb);
    rmhip_buf centred = 0, analytic = 0;
    Buffer zb;
    if (rc == RMHIP_OK && method == 0 && n > 1) {
        Buffer cb;  // the centred [n, m] temporary: f64 in either precision mode, never queued for narrowing
        cb.shape = {(size_t)n, (size_t)m};
        cb.numel = total;
        rc = c->alloc_device(total, &cb.alloc);
        if (rc == RMHIP_OK) {
            if (in32) hipLaunchKernelGGL(k_env_center<float>, dim3(grid_for(total)), dim3(kB), 0, c->stream, xb.data_f32(), mu->ptr, n, (u64)total, cb.data());
            else hipLaunchKernelGGL(k_env_center<double>, dim3(grid_for(total)), dim3(kB), 0, c->stream, xb.data(), mu->ptr, n, (u64)total, cb.data());
            c->tel.kernel_launches++;
            if (hipGetLastError() != hipSuccess) rc = fail(RMHIP_ERR_HIP, "signal_envelope: launch failed");
        }
        if (rc == RMHIP_OK) rc = c->register_buffer(std::move(cb), &centred);
        if (rc == RMHIP_OK) {
            EnvPrecision64 hold(c);
            rc = rmhip_hilbert(ctx, centred, -1, 0, &analytic);
        }
        if (centred) rmhip_free(ctx, centred);
        if (rc == RMHIP_OK) rc = c->get_any(analytic, &zb);
    }
    if (rc == RMHIP_OK) {
        const double2* z = zb.alloc ? reinterpret_cast<const double2*>(zb.data()) : nullptr;
        const double* tp = taps ? taps->ptr : nullptr;
        const unsigned ntaps = (unsigned)host_taps.size();
        if (in32) rc = env_launch<float, float>(c, method, xb.data_f32(), mu->ptr, z, tp, n, total, param, t0, ntaps, ub.data_f32(), lb.data_f32());
        else if (out32) rc = env_launch<double, float>(c, method, xb.data(), mu->ptr, z, tp, n, total, param, t0, ntaps, ub.data_f32(), lb.data_f32());
        else rc = env_launch<double, double>(c, method, xb.data(), mu->ptr, z, tp, n, total, param, t0, ntaps, ub.data(), lb.data());
    }
    if (analytic) {
        zb = Buffer();
        rmhip_free(ctx, analytic);
    }
    if (rc != RMHIP_OK) {
        if (*upper) rmhip_free(ctx, *upper);
        if (*lower) rmhip_free(ctx, *lower);
        *upper = *lower = 0;
        return rc;
    }
    if (method == 0) c->record_launch("envelope", {{"channel_len", n}, {"channels", m}}, {{"analytic", 1}});
    else if (method == 1) c->record_launch("envelope", {{"channel_len", n}, {"channels", m}}, {{"analytic_fir", param}});
    else c->record_launch("envelope", {{"channel_len", n}, {"channels", m}}, {{"rms", param}});
    return RMHIP_OK;
}

}  // extern "C"
