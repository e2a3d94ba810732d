// fft.hip -- discrete Fourier transforms along one dimension of a resident tensor, and the complex-interleaved storage they produce.
//   fft_dim / ifft_dim        crates/runmat-accelerate-api/src/lib.rs:2622-2638   (semantics: the wgpu provider's host form,
//                             runmat-accelerate/src/backend/wgpu/provider/ops/fft/fallback.rs:4-150 - zero-pad / truncate to `len`,
//                             unnormalised forward transform, inverse scaled by 1 / len, complex-interleaved result)
//   fft_extract_real          lib.rs:2639-2644    (ifft(..., 'symmetric'): builtins/math/fft/ifft.rs:362-372)
//   complex_from_real(_imag)  lib.rs:1940-1959
// The reference transforms with rustfft 6.4.1 (Cargo.lock:6116-6118; not under /root/reference): parity is by tolerance against the
// DFT definition (tests/test_gpu_fft.py states it), not by bits.
//
// Kernel: `k_fft_tile` - a workgroup holds a tile of up to 4096 complex points (B lines x m points, m a power of two) in LDS as
// split re / im arrays with one pad slot per 32, runs in-place decimation-in-frequency passes of radix 8 (then 4 or 2) with ONE
// barrier per pass, and leaves through a digit-reversed LDS read, so both the loads and the stores are coalesced: along the points
// when the line is contiguous, across neighbouring lines otherwise (lines along a trailing dimension).  Lengths above the tile take
// two or three such passes, lengths that are not powers of two go through Bluestein's chirp convolution on the same kernel.
// Which passes, tiles, work buffers and tables a shape gets is decided in fft_plan.h; the drivers here execute it through launch_pass.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "fft_plan.h"

// parity here is by tolerance against the exact transform (the reference's rustfft has its own operation order): fused
// multiply-adds are allowed in this file - fewer instructions and one rounding less per complex product
#pragma clang fp contract(fast)

using namespace rmhip;

namespace rmhip {
namespace {

using namespace fft_plan;  // u64, Side, the tile constants, the routes

constexpr int FT = 256;         // threads per workgroup of the small elementwise kernels
constexpr u64 NOLINE = ~0ull;

struct FftPass {
    u64 nlines, inner, qcnt;  // line l = i + inner * (q + qcnt * o)
    const double* in;
    double* out;
    Side a, b;                // input / output addressing (in complex elements, or real elements for a real input)
    u64 in_pk, in_qk, in_len; // point p of a line with sub-index q exists iff p*in_pk + q*in_qk < in_len (else it reads as zero)
    const double2* tw;        // w_m^k = exp(-2 pi i k / m), k < m
    const double2* step_lo;   // step twiddle tables of the enclosing length (two-pass transforms), or null
    const double2* step_hi;
    const double2* mul_in;    // per-point factor on load, indexed by the point's position p*in_pk + q*in_qk (Bluestein's chirp), or null
    double scale;
    int log2m, log2b;
    int in_complex, mode, step_by_i, conj_in, conj_out, round32;  // mode: see k_fft_tile
    int nrad, rad[5];
    // k_fft_tile<NT, true> only (the spectral estimate's frames):
    const double* win;        // a REAL per-point factor on load, indexed like mul_in (the window)
};

__device__ __forceinline__ void cmul(double& xr, double& xi, double wr, double wi) {
    const double r = xr * wr - xi * wi, i = xr * wi + xi * wr;
    xr = r;
    xi = i;
}

// natural-order in, natural-order out, forward sign
template <int R>
__device__ __forceinline__ void dft_small(double (&xr)[R], double (&xi)[R]);

template <>
__device__ __forceinline__ void dft_small<2>(double (&xr)[2], double (&xi)[2]) {
    const double ar = xr[0] + xr[1], ai = xi[0] + xi[1], br = xr[0] - xr[1], bi = xi[0] - xi[1];
    xr[0] = ar, xi[0] = ai, xr[1] = br, xi[1] = bi;
}

__device__ __forceinline__ void dft4(double& r0, double& i0, double& r1, double& i1, double& r2, double& i2, double& r3, double& i3) {
    const double t0r = r0 + r2, t0i = i0 + i2, t1r = r0 - r2, t1i = i0 - i2;
    const double t2r = r1 + r3, t2i = i1 + i3;
    const double t3r = i1 - i3, t3i = -(r1 - r3);  // (a1 - a3) * (-i)
    r0 = t0r + t2r, i0 = t0i + t2i;
    r2 = t0r - t2r, i2 = t0i - t2i;
    r1 = t1r + t3r, i1 = t1i + t3i;
    r3 = t1r - t3r, i3 = t1i - t3i;
}

template <>
__device__ __forceinline__ void dft_small<4>(double (&xr)[4], double (&xi)[4]) {
    dft4(xr[0], xi[0], xr[1], xi[1], xr[2], xi[2], xr[3], xi[3]);
}

template <>
__device__ __forceinline__ void dft_small<8>(double (&xr)[8], double (&xi)[8]) {
    // even and odd halves, then X[k] = E[k] + w8^k O[k], X[k + 4] = E[k] - w8^k O[k]
    dft4(xr[0], xi[0], xr[2], xi[2], xr[4], xi[4], xr[6], xi[6]);
    dft4(xr[1], xi[1], xr[3], xi[3], xr[5], xi[5], xr[7], xi[7]);
    constexpr double h = 0.70710678118654752440;
    double er[4] = {xr[0], xr[2], xr[4], xr[6]}, ei[4] = {xi[0], xi[2], xi[4], xi[6]};
    double orr[4], oi[4];
    orr[0] = xr[1], oi[0] = xi[1];
    orr[1] = h * (xr[3] + xi[3]), oi[1] = h * (xi[3] - xr[3]);   // * (1 - i) / sqrt 2
    orr[2] = xi[5], oi[2] = -xr[5];                              // * (-i)
    orr[3] = h * (xi[7] - xr[7]), oi[3] = -h * (xr[7] + xi[7]);  // * (-1 - i) / sqrt 2
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xr[k] = er[k] + orr[k], xi[k] = ei[k] + oi[k];
        xr[k + 4] = er[k] - orr[k], xi[k + 4] = ei[k] - oi[k];
    }
}

// ---- the tile kernel ---------------------------------------------------------------------------------------------------------------
// Stockham autosort passes over a tile of B lines x m points, eight points per thread (one radix-8 butterfly, two radix-4 or four
// radix-2).  Pass s (Ns = product of the radices before it) takes butterfly j's inputs from points j + q m/R - whatever Ns is, so
// neighbouring threads always read neighbouring points -, multiplies them by w_{Ns R}^(kq), k = j mod Ns, and files result r at point
// (j - k) R + k + r Ns.  The FIRST pass therefore loads straight from global memory and the LAST one (k = j) stores straight to it,
// both coalesced; LDS only carries the exchanges in between (read all - barrier - write all - barrier: one copy of the tile).
// Thread-to-butterfly order and LDS layout follow what is contiguous in memory:
//   mode 0  points of a line are contiguous (a transform along dimension 0): threads along j, LDS index b m + point;
//   mode 1  neighbouring lines are contiguous (a trailing dimension, or the strided first step of a long transform): threads along b,
//           LDS index point B + b;
//   mode 2  contiguous points in, neighbouring lines out (the second step of a long transform - the transposition of the four-step
//           algorithm): the tile is first staged through LDS (4 points x 16 lines per wave), then as mode 1.
// One pad slot per eight keeps the exchange patterns (stride R, stride 8 R, runs of Ns) at two lanes per bank.
__device__ __forceinline__ int padi(int i) { return i + (i >> 3); }

template <int NT>
struct TileCtx {
    double* re;
    double* im;
    const u64* ibase;
    const u64* obase;
    const unsigned* lpos;
    const unsigned* lmul;
    int log2m, log2b, lines_fast;
    __device__ __forceinline__ int lidx(int b, int pt) const { return padi(lines_fast ? (pt << log2b) + b : (b << log2m) + pt); }
};

template <int R>
struct RadixLog {
    static constexpr int v = R == 8 ? 3 : (R == 4 ? 2 : 1);
};

// one pass: K = 8 / R butterflies per thread.  FIRST: inputs come from global memory (unless STAGED: from LDS, like a later pass);
// LAST: results go to global memory.  WIN: the load multiplies by the real table P.win instead of the complex P.mul_in.
template <int NT, int R, bool first_from_global, bool last, bool WIN = false>
__device__ __forceinline__ void stockham_pass(const FftPass& P, const TileCtx<NT>& T, int log2ns) {
    constexpr int LR = RadixLog<R>::v, K = 8 / R;
    const int log2m = T.log2m, log2b = T.log2b;
    const int nb = 1 << (log2m + log2b - LR);  // butterflies in the tile
    const int log2s = log2m - LR;              // input stride m / R
    double xr[K][R], xi[K][R];
    int bb[K], jj[K];
    bool live[K];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        const int id = threadIdx.x + NT * kk;
        live[kk] = id < nb;
        if (T.lines_fast) bb[kk] = id & ((1 << log2b) - 1), jj[kk] = id >> log2b;
        else jj[kk] = id & ((1 << log2s) - 1), bb[kk] = id >> log2s;
    }
    if (first_from_global) {
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            const u64 base = live[kk] ? T.ibase[bb[kk]] : NOLINE;
            const u64 lp = live[kk] ? (u64)T.lpos[bb[kk]] : 0;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int pt = jj[kk] + (q << log2s);
                const u64 pos = (u64)pt * P.in_pk + lp;
                double vr = 0.0, vi = 0.0;
                if (base != NOLINE && pos < P.in_len) {
                    const u64 off = base + (u64)pt * P.a.sp;
                    if (P.in_complex) {
                        const double2 v = reinterpret_cast<const double2*>(P.in)[off];
                        vr = v.x, vi = v.y;
                    } else {
                        vr = P.in[off];
                    }
                    if (P.conj_in) vi = -vi;
                    if constexpr (WIN) {
                        const double f = P.win[pos];
                        vr *= f, vi *= f;
                    } else {
                        if (P.mul_in) {
                            const double2 f = P.mul_in[pos];
                            cmul(vr, vi, f.x, f.y);
                        }
                    }
                }
                xr[kk][q] = vr, xi[kk][q] = vi;
            }
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int a = T.lidx(bb[kk], jj[kk] + (q << log2s));
                xr[kk][q] = live[kk] ? T.re[a] : 0.0, xi[kk][q] = live[kk] ? T.im[a] : 0.0;
            }
    }
    if (!first_from_global && log2ns > 0) {  // (the first pass has Ns = 1: no twiddles)
        const int sh = log2m - log2ns - LR;
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            const int k = jj[kk] & ((1 << log2ns) - 1);
            if (R == 8) {
                // w, w^2, w^4 from the table; w^3 = w w^2, w^5 = w w^4, w^6 = w^2 w^4, w^7 = w^3 w^4 (at most two roundings more than a
                // table entry; seven loads per butterfly were as much L1 traffic as the tile's LDS exchange)
                const double2 w1 = P.tw[k << sh], w2 = P.tw[(2 * k) << sh], w4 = P.tw[(4 * k) << sh];
                double w3r = w1.x, w3i = w1.y, w5r = w1.x, w5i = w1.y, w6r = w2.x, w6i = w2.y;
                cmul(w3r, w3i, w2.x, w2.y);
                cmul(w5r, w5i, w4.x, w4.y);
                cmul(w6r, w6i, w4.x, w4.y);
                double w7r = w3r, w7i = w3i;
                cmul(w7r, w7i, w4.x, w4.y);
                cmul(xr[kk][1], xi[kk][1], w1.x, w1.y);
                cmul(xr[kk][2], xi[kk][2], w2.x, w2.y);
                cmul(xr[kk][3], xi[kk][3], w3r, w3i);
                cmul(xr[kk][4], xi[kk][4], w4.x, w4.y);
                cmul(xr[kk][5], xi[kk][5], w5r, w5i);
                cmul(xr[kk][6], xi[kk][6], w6r, w6i);
                cmul(xr[kk][7], xi[kk][7], w7r, w7i);
            } else {
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    const double2 w = P.tw[(k * q) << sh];
                    cmul(xr[kk][q], xi[kk][q], w.x, w.y);
                }
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) dft_small<R>(xr[kk], xi[kk]);
    if (!last) {
        __syncthreads();  // every thread has read its inputs: the tile may be overwritten
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            if (!live[kk]) continue;
            const int k = jj[kk] & ((1 << log2ns) - 1);
            const int o0 = ((jj[kk] - k) << LR) + k;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int a = T.lidx(bb[kk], o0 + (r << log2ns));
                T.re[a] = xr[kk][r], T.im[a] = xi[kk][r];
            }
        }
        __syncthreads();
        return;
    }
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        if (!live[kk]) continue;
        const u64 base = T.obase[bb[kk]];
        if (base == NOLINE) continue;
        const unsigned lm = T.lmul[bb[kk]];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int pt = jj[kk] + (r << log2ns);  // (in the last pass k = j and Ns = m / R)
            double vr = xr[kk][r], vi = xi[kk][r];
            if (P.step_lo) {
                const u64 tt = (u64)pt * lm;
                const double2 wl = P.step_lo[tt & ((1u << STEP_LO) - 1)], wh = P.step_hi[tt >> STEP_LO];
                double wr = wl.x, wi = wl.y;
                cmul(wr, wi, wh.x, wh.y);
                cmul(vr, vi, wr, wi);
            }
            if (P.conj_out) vi = -vi;
            vr *= P.scale, vi *= P.scale;
            if (P.round32) vr = (double)(float)vr, vi = (double)(float)vi;
            double2 v;
            v.x = vr, v.y = vi;
            reinterpret_cast<double2*>(P.out)[base + (u64)pt * P.b.sp] = v;
        }
    }
}

template <int NT, int R, bool WIN>
__device__ __forceinline__ void run_pass(int variant, const FftPass& P, const TileCtx<NT>& T, int log2ns) {
    switch (variant) {
        case 0: stockham_pass<NT, R, false, false>(P, T, log2ns); break;
        case 1: stockham_pass<NT, R, false, true>(P, T, log2ns); break;
        case 2: stockham_pass<NT, R, true, false, WIN>(P, T, log2ns); break;
        default: stockham_pass<NT, R, true, true, WIN>(P, T, log2ns); break;
    }
}

// WIN = true is the instantiation of the spectral estimate's fused path (rmhip_spectral_estimate): frames are read straight from the
// signal through Side's strides and multiplied by the real window table; the transforms' own instantiation carries none of it.
template <int NT, bool WIN = false>
__global__ void __launch_bounds__(NT, 4) k_fft_tile(const FftPass P) {
    extern __shared__ __attribute__((aligned(16))) double fft_lds[];
    const int t = threadIdx.x;
    const int log2m = P.log2m, log2b = P.log2b, B = 1 << log2b, tile = 1 << (log2m + log2b);
    const int plane = tile + (tile >> 3) + 1;
    TileCtx<NT> T;
    T.re = fft_lds;
    T.im = T.re + plane;
    u64* const ibase = reinterpret_cast<u64*>(T.im + plane);
    u64* const obase = ibase + B;
    unsigned* const lpos = reinterpret_cast<unsigned*>(obase + B);
    unsigned* const lmul = lpos + B;
    T.ibase = ibase, T.obase = obase, T.lpos = lpos, T.lmul = lmul;
    T.log2m = log2m, T.log2b = log2b, T.lines_fast = P.mode != 0;
    for (int b = t; b < B; b += NT) {
        const u64 l = (u64)blockIdx.x * B + b;
        if (l < P.nlines) {
            const u64 i = l % P.inner, r = l / P.inner, q = r % P.qcnt, o = r / P.qcnt;
            ibase[b] = i * P.a.si + q * P.a.sq + o * P.a.so;
            obase[b] = i * P.b.si + q * P.b.sq + o * P.b.so;
            lpos[b] = (unsigned)(q * P.in_qk);
            lmul[b] = (unsigned)(P.step_by_i ? i : q);
        } else {
            ibase[b] = NOLINE, obase[b] = NOLINE, lpos[b] = 0, lmul[b] = 0;
        }
    }
    __syncthreads();
    bool from_global = true;
    if (P.mode == 2 || P.nrad == 0) {
        // staged load: a wave takes PW points x LW lines, so that a line's PW points are one contiguous piece of memory and the LW
        // lines are neighbours in the LDS layout (point B + b)
        int lpw = log2m < 2 ? log2m : 2;                       // up to four points of a line ...
        const int llw = log2b < 6 - lpw ? log2b : 6 - lpw;     // ... across up to sixteen lines (more when the lines are shorter)
        if (llw + lpw < 6) lpw = log2m < 6 - llw ? log2m : 6 - llw;
        const int cl = llw + lpw, nbb = B >> llw;              // chunk of 2^cl elements; chunks across the lines
        for (int e = t; e < tile; e += NT) {
            const int chunk = e >> cl, lane = e & ((1 << cl) - 1);
            const int b = ((chunk % nbb) << llw) + (lane >> lpw), pt = ((chunk / nbb) << lpw) + (lane & ((1 << lpw) - 1));
            double vr = 0.0, vi = 0.0;
            const u64 base = ibase[b];
            const u64 pos = (u64)pt * P.in_pk + lpos[b];
            if (base != NOLINE && pos < P.in_len) {
                const u64 off = base + (u64)pt * P.a.sp;
                if (P.in_complex) {
                    const double2 v = reinterpret_cast<const double2*>(P.in)[off];
                    vr = v.x, vi = v.y;
                } else {
                    vr = P.in[off];
                }
                if (P.conj_in) vi = -vi;
                if constexpr (WIN) {
                    const double f = P.win[pos];
                    vr *= f, vi *= f;
                } else {
                    if (P.mul_in) {
                        const double2 f = P.mul_in[pos];
                        cmul(vr, vi, f.x, f.y);
                    }
                }
            }
            const int a = T.lidx(b, pt);
            T.re[a] = vr, T.im[a] = vi;
        }
        __syncthreads();
        from_global = false;
    }
    if (P.nrad == 0) {  // one-point lines: the point itself
        for (int e = t; e < tile; e += NT) {
            const int b = e;
            if (obase[b] == NOLINE) continue;
            const int a = T.lidx(b, 0);
            double vr = T.re[a], vi = T.im[a];
            if (P.conj_out) vi = -vi;
            vr *= P.scale, vi *= P.scale;
            if (P.round32) vr = (double)(float)vr, vi = (double)(float)vi;
            double2 v;
            v.x = vr, v.y = vi;
            reinterpret_cast<double2*>(P.out)[obase[b]] = v;
        }
        return;
    }
    // the radices are (4 or 2,) 8, 8, ...: the first pass is dispatched on its radix, every later one is a radix-8 pass - the middle
    // ones in a loop of their own (one variant inside the loop: what the compiler hoists out of it stays small)
    const bool only = P.nrad == 1;
    const int variant = (from_global ? 2 : 0) | (only ? 1 : 0);
    int log2ns;
    if (P.rad[0] == 8) run_pass<NT, 8, WIN>(variant, P, T, 0), log2ns = 3;
    else if (P.rad[0] == 4) run_pass<NT, 4, WIN>(variant, P, T, 0), log2ns = 2;
    else run_pass<NT, 2, WIN>(variant, P, T, 0), log2ns = 1;
    if (only) return;
    for (int s = 1; s + 1 < P.nrad; ++s, log2ns += 3) stockham_pass<NT, 8, false, false>(P, T, log2ns);
    stockham_pass<NT, 8, false, true>(P, T, log2ns);
}

// tables ---------------------------------------------------------------------------------------------------------------------------------
// kind 0: w_n^k, k < count                 (count = n)
// kind 1: w_n^(k * 4096), k < count        (the coarse half of the step twiddle)
// kind 2: exp(-i pi k^2 / n), k < count    (Bluestein's chirp; k^2 mod 2n is taken in integers)
__global__ void __launch_bounds__(FT) k_fft_table(double2* __restrict__ out, u64 count, u64 n, int kind) {
    const u64 k = (u64)blockIdx.x * FT + threadIdx.x;
    if (k >= count) return;
    double s, co;
    if (kind == 2) {
        const u64 k2 = (unsigned long long)(((unsigned __int128)k * k) % (2 * n));
        sincospi((double)k2 / (double)n, &s, &co);
    } else {
        const u64 kk = kind == 1 ? ((k << STEP_LO) % n) : k;
        sincospi(2.0 * (double)kk / (double)n, &s, &co);
    }
    double2 v;
    v.x = co, v.y = -s;
    out[k] = v;
}

typedef std::shared_ptr<Allocation> Table;  // callers hold the reference while their launches are being queued
inline const double2* tptr(const Table& t) { return reinterpret_cast<const double2*>(t->ptr); }

int fft_table(Context* c, int kind, u64 n, u64 count, Table* out) {
    const uint64_t key = ((uint64_t)kind << 60) ^ (n << 28) ^ count;
    auto it = c->fft_tables.find(key);
    if (it == c->fft_tables.end()) {
        std::shared_ptr<Allocation> a;
        RMHIP_TRY(c->alloc_device(2 * count, &a));
        hipLaunchKernelGGL(k_fft_table, dim3((unsigned)((count + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<double2*>(a->ptr), count, n, kind);
        c->tel.kernel_launches++;
        RMHIP_HIP_CHECK(hipGetLastError());
        if (c->fft_tables.size() > 64) c->fft_tables.clear();  // bounded: a table is a few microseconds to rebuild
        it = c->fft_tables.emplace(key, a).first;
    }
    *out = it->second;
    return RMHIP_OK;
}

// What launch_pass needs beside a pass's geometry: the buffers their roles name, and what the first and the last pass carry.
struct PassIo {
    const double* in;
    int in_complex;
    double* work;
    double* out;            // complex
    bool conj_in, conj_out;
    double scale;
    bool round32;
    const double2* mul_in;  // a factor per input point (Bluestein's chirp), or null
    const double* win;      // a REAL factor per input point (the spectral estimate's window): k_fft_tile<NT, true>, or null
};

typedef void (*TileKernel)(const FftPass);
TileKernel tile_kernel(int threads, bool win) {
    static const TileKernel kernels[3][2] = {{k_fft_tile<256, false>, k_fft_tile<256, true>},
                                             {k_fft_tile<512, false>, k_fft_tile<512, true>},
                                             {k_fft_tile<1024, false>, k_fft_tile<1024, true>}};
    return kernels[threads == 256 ? 0 : (threads == 512 ? 1 : 2)][win ? 1 : 0];
}

// The one launcher: a pass's geometry (fft_plan.h), the buffers and the route's step tables (STEP_N's lo, hi, then STEP_N1's) become
// an FftPass; plan_tile gives its tile.
int launch_pass(Context* c, const PassGeom& g, const PassIo& io, const Table* steps = nullptr) {
    FftPass P{};
    P.nlines = g.nlines, P.inner = g.inner, P.qcnt = g.qcnt;
    P.in = g.src == FROM_INPUT ? io.in : io.work, P.in_complex = g.src == FROM_INPUT ? io.in_complex : 1;
    P.out = g.dst == TO_WORK ? io.work : io.out;
    P.a = g.a, P.b = g.b;
    P.in_pk = g.in_pk, P.in_qk = g.in_qk, P.in_len = g.in_len;
    P.log2m = g.log2m, P.mode = g.mode, P.step_by_i = g.step_by_i;
    if (g.step != STEP_NONE) {
        const Table* t = steps + (g.step == STEP_N ? 0 : 2);
        P.step_lo = tptr(t[0]), P.step_hi = tptr(t[1]);
    }
    P.scale = 1.0;
    if (g.first) P.conj_in = io.conj_in, P.mul_in = io.mul_in, P.win = io.win;
    if (g.last) P.conj_out = io.conj_out, P.scale = io.scale, P.round32 = io.round32;
    const TilePlan t = plan_tile(g.log2m, g.mode, g.nlines);
    P.log2b = t.log2b, P.nrad = t.nrad;
    std::copy(t.rad, t.rad + t.nrad, P.rad);
    const u64 m = 1ull << g.log2m;
    Table tw;
    RMHIP_TRY(fft_table(c, 0, m, m, &tw));
    P.tw = tptr(tw);
    if (t.refused) return fail(RMHIP_ERR_UNSUPPORTED, "fft: %llu lines", P.nlines);
    hipLaunchKernelGGL(tile_kernel(t.threads, P.win != nullptr), dim3((unsigned)t.blocks), dim3(t.threads), t.lds, c->stream, P);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

struct Lines {  // a LineShape with its buffers
    const double* in;
    int in_complex;
    LineShape shape;
    double* out;  // complex, n points per line, same layout
};

// forward transform of conj^a(x), conjugated b times (a = b = 1: the unscaled inverse) - power-of-two length n along the lines; `scale` multiplies the result.
// `mul_in` (or null): a factor per input point k (Bluestein's chirp); points from `valid` on read as zero whatever the input holds.
int fft_pow2(Context* c, const Lines& L, u64 n, bool conj_in, bool conj_out, double scale, bool round32, const double2* mul_in = nullptr, u64 valid = ~0ull) {
    const Pow2Route r = plan_pow2(L.shape, n, valid);
    if (r.npass == 0) return fail(RMHIP_ERR_UNSUPPORTED, "fft: length %llu", n);
    std::shared_ptr<Allocation> work;
    if (r.work) RMHIP_TRY(c->alloc_device(2 * r.work, &work));
    Table steps[4];
    for (int k = 0; k < r.ntables; ++k) RMHIP_TRY(fft_table(c, r.tables[k].kind, r.tables[k].n, r.tables[k].count, &steps[k]));
    const PassIo io{L.in, L.in_complex, work ? work->ptr : nullptr, L.out, conj_in, conj_out, scale, round32, mul_in, nullptr};
    for (int k = 0; k < r.npass; ++k) RMHIP_TRY(launch_pass(c, r.pass[k], io, steps));
    return RMHIP_OK;
}

// Bluestein: X[j] = conj-chirp[j] * sum_k (x[k] chirp[k]) * conj(chirp)[j - k], chirp[k] = exp(-i pi k^2 / n); the convolution by
// power-of-two transforms of length M >= 2n - 1.  G = FFT_M(g), g[k] = conj(chirp[|k|]) wrapped, is computed once per (n, M).
__global__ void __launch_bounds__(FT) k_bluestein_kernel(const double2* __restrict__ chirp, u64 n, u64 M, double2* __restrict__ g) {
    const u64 k = (u64)blockIdx.x * FT + threadIdx.x;
    if (k >= M) return;
    double2 v;
    v.x = 0.0, v.y = 0.0;
    if (k < n) v.x = chirp[k].x, v.y = -chirp[k].y;
    else if (M - k < n) v.x = chirp[M - k].x, v.y = -chirp[M - k].y;
    g[k] = v;
}

// y(i, k, o) *= G[k] (in place; tensor layout with M points per line)
__global__ void __launch_bounds__(FT) k_line_mul(double2* __restrict__ a, const double2* __restrict__ g, u64 inner, u64 M, u64 total) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e >= total) return;
    double2 v = a[e];
    const double2 w = g[(e / inner) % M];
    cmul(v.x, v.y, w.x, w.y);
    a[e] = v;
}

// out(i, j, o) = scale * op(chirp[j] * y(i, j, o)) for j < n: the first n points of the M-long lines
__global__ void __launch_bounds__(FT) k_bluestein_finish(const double2* __restrict__ y, const double2* __restrict__ chirp, u64 inner, u64 n, u64 M, u64 total,
                                                         double scale, int conj_out, int round32, double2* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;  // output element i + inner * (j + n * o)
    if (e >= total) return;
    const u64 i = e % inner, r = e / inner, j = r % n, o = r / n;
    double2 v = y[i + inner * (j + M * o)];
    const double2 w = chirp[j];
    cmul(v.x, v.y, w.x, w.y);
    if (conj_out) v.y = -v.y;
    v.x *= scale, v.y *= scale;
    if (round32) v.x = (double)(float)v.x, v.y = (double)(float)v.y;
    out[e] = v;
}

int fft_bluestein(Context* c, const Lines& L, u64 n, bool inverse, double scale, bool round32) {
    const ChirpPlan p = plan_chirp(L.shape, n);
    const u64 M = p.M, inner = L.shape.inner, len_in = L.shape.len_in;
    if (p.refused == CHIRP_LENGTH) return fail(RMHIP_ERR_UNSUPPORTED, "fft: length %llu", n);
    Table chirp;
    RMHIP_TRY(fft_table(c, 2, n, n, &chirp));
    // G = FFT_M of the wrapped conjugate chirp, kept beside the tables (kind 3)
    const uint64_t gkey = (3ull << 60) ^ (n << 28) ^ M;
    Table G;
    auto it = c->fft_tables.find(gkey);
    if (it != c->fft_tables.end()) {
        G = it->second;
    } else {
        Table g;
        RMHIP_TRY(c->alloc_device(2 * M, &g));
        RMHIP_TRY(c->alloc_device(2 * M, &G));
        hipLaunchKernelGGL(k_bluestein_kernel, dim3((unsigned)((M + FT - 1) / FT)), dim3(FT), 0, c->stream, tptr(chirp), n, M, reinterpret_cast<double2*>(g->ptr));
        c->tel.kernel_launches++;
        Lines gl{g->ptr, 1, {1, 1, M}, G->ptr};
        RMHIP_TRY(fft_pow2(c, gl, M, false, false, 1.0, false));
        c->fft_tables[gkey] = G;
    }
    if (p.refused == CHIRP_SLAB) return fail(RMHIP_ERR_UNSUPPORTED, "fft: %llu lines of chirp length %llu along a trailing dimension", inner, M);
    Table A, Y;  // the two work tensors [inner, M, outer_per]
    RMHIP_TRY(c->alloc_device(2 * p.slab * p.outer_per, &A));
    RMHIP_TRY(c->alloc_device(2 * p.slab * p.outer_per, &Y));
    for (u64 k = 0; k < p.nslabs; ++k) {
        const Slab s = chirp_slab(p, L.shape.outer, k);
        const u64 total = s.oc * p.slab;
        const double* in = L.in + (L.in_complex ? 2 : 1) * (s.o0 * len_in * inner);
        double* out = L.out + 2 * (s.o0 * n * inner);
        Lines f{in, L.in_complex, {inner, s.oc, len_in}, A->ptr};  // a = op(x) .* chirp, zero-extended to M, transformed
        RMHIP_TRY(fft_pow2(c, f, M, inverse, false, 1.0, false, tptr(chirp), p.valid));
        hipLaunchKernelGGL(k_line_mul, dim3((unsigned)((total + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<double2*>(A->ptr), tptr(G), inner, M, total);
        Lines b{A->ptr, 1, {inner, s.oc, M}, Y->ptr};
        RMHIP_TRY(fft_pow2(c, b, M, true, true, 1.0 / (double)M, false));
        const u64 ototal = s.oc * inner * n;
        hipLaunchKernelGGL(k_bluestein_finish, dim3((unsigned)((ototal + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<const double2*>(Y->ptr), tptr(chirp),
                           inner, n, M, ototal, scale, inverse ? 1 : 0, round32 ? 1 : 0, reinterpret_cast<double2*>(out));
        c->tel.kernel_launches += 2;
        RMHIP_HIP_CHECK(hipGetLastError());
    }
    return RMHIP_OK;
}

// a failed entry hands back no handle: the results it had made leave the table and their ids read 0
void drop_outputs(Context* c, std::initializer_list<rmhip_buf*> ids) {
    std::lock_guard<std::mutex> lk(c->mu);
    for (rmhip_buf* id : ids) {
        Buffer victim;
        auto it = c->table.find(*id);
        if (*id && it != c->table.end()) victim = std::move(it->second), c->table.erase(it);
        *id = 0;
    }
}

int fft_entry(Context* c, rmhip_buf a, long long len_or_neg, int dim, bool inverse, rmhip_buf* out) {
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (dim < 0) return fail(RMHIP_ERR_INVALID, "fft: dim must be >= 0");
    Buffer ab;
    RMHIP_TRY(c->get_any(a, &ab));
    std::vector<size_t> shape = ab.shape;
    if (shape.empty()) shape.push_back(ab.numel);  // fallback.rs:20-29
    const size_t origin_rank = shape.size();
    while (shape.size() <= (size_t)dim) shape.push_back(1);
    const u64 cur = shape[dim], n = len_or_neg < 0 ? cur : (u64)len_or_neg;
    u64 inner = 1, outer = 1;
    for (int k = 0; k < dim; ++k) inner *= shape[k];
    for (size_t k = dim + 1; k < shape.size(); ++k) outer *= shape[k];
    std::vector<size_t> oshape = shape;
    oshape[dim] = n;
    // fft_trim_trailing_ones(out_shape, max(origin_rank, dim + 1)) (mod.rs:14-19): nothing beyond that rank was added, so only the
    // scalar normalisation is left
    (void)origin_rank;
    bool scalar = true;
    for (size_t e : oshape) scalar = scalar && e == 1;
    if (scalar) oshape = {1, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer_complex(oshape.data(), oshape.size(), out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    const bool r32 = c->precision == 32;
    const Lines L{ab.data(), ab.cplx ? 1 : 0, {inner, outer, cur}, ob.data()};
    const double scale = inverse ? 1.0 / (double)n : 1.0;
    int rc = RMHIP_OK;
    switch (plan_entry(cur, n)) {
        case ENTRY_ZERO_FILL: RMHIP_HIP_CHECK(hipMemsetAsync(ob.data(), 0, 2 * ob.numel * sizeof(double), c->stream)); break;
        case ENTRY_ONE_POINT: rc = launch_pass(c, one_point_pass(L.shape), PassIo{L.in, L.in_complex, nullptr, L.out, false, false, scale, r32, nullptr, nullptr}); break;
        case ENTRY_POW2: rc = fft_pow2(c, L, n, inverse, inverse, scale, r32); break;
        case ENTRY_CHIRP: rc = fft_bluestein(c, L, n, inverse, scale, r32); break;
    }
    if (rc != RMHIP_OK) drop_outputs(c, {out});
    return rc;
}

// ---- framed spectra: uniform_spectral_estimate (lib.rs:266-307, :2560-2565) ---------------------------------------------------------------
// spectrogram / pwelch / periodogram hand over a signal, a window and a framing rule (rmhip.h states it) and take back the selected
// rows of every frame's spectrum, `s`, and their scaled powers, `ps`.  The wgpu provider runs four passes over a materialised
// [nfft, frames] complex buffer (frame, transform, select, power).  Here a power-of-two frame that one tile holds is loaded by
// k_fft_tile straight from the signal - a hop-strided, windowed, zero-padded line is what Side, `win` and `in_len` address - and
// one kernel reads the spectrum once for the selection / rotation and the power.  Folded frames, Bluestein lengths, lengths of
// several passes and frames that reach past input_len are written out by k_spectral_frame first.
struct SpectralFrames {
    u64 input_len, window_len, nfft, hop, input_rows, fpc;
    int mode, x_complex;
};

// frame c, point r of the [nfft, frames] complex frame buffer; a source index >= input_len contributes zero
__global__ void __launch_bounds__(FT) k_spectral_frame(const double* __restrict__ x, const double* __restrict__ w, const SpectralFrames F, u64 total, double2* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e >= total) return;
    const u64 r = e % F.nfft, c = e / F.nfft;
    const u64 base = F.mode == 0 ? c * F.hop : (F.mode == 1 ? (c / F.fpc) * F.input_rows + (c % F.fpc) * F.hop : c * F.input_rows);
    // modes 0 and 1 truncate the window at nfft (one term); mode 2 folds it: r, r + nfft, ... in ascending order
    const u64 end = F.mode == 2 ? F.window_len : (r < F.window_len ? r + 1 : 0);
    double vr = 0.0, vi = 0.0;
    for (u64 rr = r; rr < end; rr += F.nfft) {
        const u64 src = base + rr;
        if (src >= F.input_len) break;  // (src grows with rr)
        const double f = w[rr];
        if (F.x_complex) {
            const double2 v = reinterpret_cast<const double2*>(x)[src];
            vr += v.x * f, vi += v.y * f;
        } else {
            vr += x[src] * f;
        }
    }
    double2 v;
    v.x = vr, v.y = vi;
    out[e] = v;
}

// row r of frame c: s = S[src(r)] (src = r, or (r + shift) mod nfft for the centered range), ps = |s|^2 * scale / denominator with
// scale = 2 on the one-sided rows that stand for two frequencies.  `s_out` is null when the transform wrote `s` itself (two-sided) and
// equals `spec` when only its values are to be rounded (two-sided on a precision-32 context): every thread then rewrites the element it read.
__global__ void __launch_bounds__(FT) k_spectral_finish(const double2* spec, u64 nfft, u64 rows, u64 total, int range, u64 shift, double denominator, int round32,
                                                        double2* s_out, double* __restrict__ ps) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e >= total) return;
    const u64 r = e % rows, c = e / rows;
    u64 src = r;
    if (range == 2) {
        src = r + shift;
        if (src >= nfft) src -= nfft;
    }
    double2 v = spec[c * nfft + src];
    const double scale = range == 0 && r != 0 && !(nfft % 2 == 0 && r == rows - 1) ? 2.0 : 1.0;
    ps[e] = (v.x * v.x + v.y * v.y) * scale / denominator;
    if (s_out) {
        if (round32) v.x = (double)(float)v.x, v.y = (double)(float)v.y;
        s_out[e] = v;
    }
}

inline bool mul_ovf(u64 a, u64 b, u64* out) { return __builtin_mul_overflow(a, b, out); }
inline bool add_ovf(u64 a, u64 b, u64* out) { return __builtin_add_overflow(a, b, out); }

struct SpectralArgs {
    size_t input_len, window_len, nfft, frame_count, hop, input_rows, fpc;
    int input_complex, mode, range;
    double denominator;
    const double* window;
};

// validate_uniform_spectral_request (lib.rs:368-424): true when the request is refused
bool spectral_invalid(const SpectralArgs& a) {
    if (!a.window || a.window_len == 0 || a.nfft == 0 || a.frame_count == 0) return true;
    if (!std::isfinite(a.denominator) || a.denominator <= 0.0) return true;
    u64 req = 0;
    if (a.mode == 0) {
        if (a.hop == 0) return true;
        return mul_ovf(a.frame_count - 1, a.hop, &req) || add_ovf(req, a.window_len, &req) || req > a.input_len;
    }
    if (a.mode == 1) {
        if (a.hop == 0 || a.input_rows == 0 || a.fpc == 0) return true;
        const u64 last = a.frame_count - 1;
        u64 step = 0;
        return mul_ovf(last / a.fpc, a.input_rows, &req) || mul_ovf(last % a.fpc, a.hop, &step) || add_ovf(req, step, &req) || add_ovf(req, a.window_len, &req) ||
               req > a.input_len;
    }
    return a.input_rows == 0 || mul_ovf(a.input_rows, a.frame_count, &req) || req > a.input_len;
}

int spectral_entry(Context* c, rmhip_buf input, const SpectralArgs& a, rmhip_buf* s, rmhip_buf* ps, size_t* rows_out, size_t* cols_out) {
    if (!s || !ps || !rows_out || !cols_out) return fail(RMHIP_ERR_INVALID, "uniform_spectral_estimate: null output");
    *s = 0, *ps = 0;
    if (a.mode < 0 || a.mode > 2 || a.range < 0 || a.range > 2) return fail(RMHIP_ERR_INVALID, "uniform_spectral_estimate: unknown frame mode or range");
    if (spectral_invalid(a)) return fail(RMHIP_ERR_INVALID, "uniform_spectral_estimate: invalid request");
    Buffer xb;
    RMHIP_TRY(c->get_any(input, &xb));
    if (a.input_len > xb.numel) return fail(RMHIP_ERR_INVALID, "uniform_spectral_estimate: input_len %zu exceeds the tensor's %zu elements", a.input_len, xb.numel);
    if ((a.input_complex != 0) != xb.cplx) return fail(RMHIP_ERR_INVALID, "uniform_spectral_estimate: input_complex disagrees with the handle's storage");
    const u64 nfft = a.nfft, fc = a.frame_count;
    if (!length_served(nfft, 1)) return fail(RMHIP_ERR_UNSUPPORTED, "uniform_spectral_estimate: nfft %zu", a.nfft);
    u64 total = 0, bytes = 0, top = 0;
    if (mul_ovf(nfft, fc, &total) || mul_ovf(total, 2 * sizeof(double), &bytes) || (total + FT - 1) / FT > 0x7fffffffull)
        return fail(RMHIP_ERR_UNSUPPORTED, "uniform_spectral_estimate: %zu frames of %zu points", a.frame_count, a.nfft);
    // `top`: one past the largest source index any frame forms - the coverage rule above only looks at the last frame
    const u64 wl = spectral_window_points(a.mode, a.window_len, nfft);
    bool ovf = false;
    if (a.mode == 0) ovf = mul_ovf(fc - 1, a.hop, &top);
    else if (a.mode == 2) ovf = mul_ovf(fc - 1, a.input_rows, &top);
    else {
        const u64 full = fc / a.fpc, rem = fc % a.fpc;  // whole columns, and the frames of a partial last one
        u64 base = 0, step = 0;
        if (full) ovf = mul_ovf(full - 1, a.input_rows, &base) || mul_ovf(a.fpc - 1, a.hop, &step) || add_ovf(base, step, &top);
        if (rem && !ovf) {
            ovf = mul_ovf(full, a.input_rows, &base) || mul_ovf(rem - 1, a.hop, &step) || add_ovf(base, step, &base);
            top = std::max(top, base);
        }
    }
    if (ovf || add_ovf(top, wl, &top)) return fail(RMHIP_ERR_UNSUPPORTED, "uniform_spectral_estimate: index overflow");
    const SpectralPlan sp = plan_spectral(a.mode, a.range, nfft, top, a.input_len);
    const u64 rows = sp.rows;
    const bool r32 = c->precision == 32, direct = sp.direct;

    Table win, frames, spec;
    RMHIP_TRY(c->alloc_device(a.window_len, &win));
    RMHIP_HIP_CHECK(hipMemcpyAsync(win->ptr, a.window, a.window_len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (sp.alloc_frames) RMHIP_TRY(c->alloc_device(2 * total, &frames));
    if (sp.alloc_spec) RMHIP_TRY(c->alloc_device(2 * total, &spec));
    const size_t oshape[2] = {(size_t)rows, (size_t)fc};
    Buffer sb, pb;
    RMHIP_TRY(c->new_buffer_complex(oshape, 2, s, &sb));
    int rc = c->new_buffer(oshape, 2, ps, &pb);
    double* const spec_ptr = direct ? sb.data() : (spec ? spec->ptr : frames->ptr);
    if (rc == RMHIP_OK && sp.fused) {
        const PassIo io{xb.data(), xb.cplx ? 1 : 0, nullptr, spec_ptr, false, false, 1.0, false, nullptr, win->ptr};
        rc = launch_pass(c, spectral_frame_pass(a.mode, fc, a.fpc, a.hop, a.input_rows, nfft, wl), io);
    } else if (rc == RMHIP_OK) {
        const SpectralFrames F{a.input_len, a.window_len, nfft, a.hop, a.input_rows, a.fpc ? a.fpc : 1, a.mode, xb.cplx ? 1 : 0};
        double* const fout = sp.own_spectrum ? spec_ptr : frames->ptr;
        hipLaunchKernelGGL(k_spectral_frame, dim3((unsigned)((total + FT - 1) / FT)), dim3(FT), 0, c->stream, xb.data(), win->ptr, F, total, reinterpret_cast<double2*>(fout));
        c->tel.kernel_launches++;
        if (hipGetLastError() != hipSuccess) rc = fail(RMHIP_ERR_HIP, "uniform_spectral_estimate: launch failed");
        if (rc == RMHIP_OK && !sp.own_spectrum) {
            const Lines L{frames->ptr, 1, {1, fc, nfft}, spec_ptr};
            rc = is_pow2(nfft) ? fft_pow2(c, L, nfft, false, false, 1.0, false) : fft_bluestein(c, L, nfft, false, 1.0, false);
        }
    }
    if (rc == RMHIP_OK) {
        const u64 otot = rows * fc;
        double2* const s_out = direct ? (r32 ? reinterpret_cast<double2*>(sb.data()) : nullptr) : reinterpret_cast<double2*>(sb.data());
        hipLaunchKernelGGL(k_spectral_finish, dim3((unsigned)((otot + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<const double2*>(spec_ptr), nfft, rows, otot,
                           a.range, sp.shift, a.denominator, r32 ? 1 : 0, s_out, pb.data());
        c->tel.kernel_launches++;
        if (hipGetLastError() != hipSuccess) rc = fail(RMHIP_ERR_HIP, "uniform_spectral_estimate: launch failed");
    }
    if (rc != RMHIP_OK) {
        drop_outputs(c, {s, ps});
        return rc;
    }
    if (sp.fused) c->record_launch("spectral", {{"rows", rows}, {"frames", fc}}, {{"fused", 1}});
    else c->record_launch("spectral", {{"rows", rows}, {"frames", fc}}, {{"framed", 1}});
    *rows_out = rows, *cols_out = fc;
    return RMHIP_OK;
}

// the analytic-signal mask of hilbert (builtins/math/signal/hilbert.rs:349-412): the spectrum times 1 at frequency 0 (and at n / 2 for even n),
// 2 on the positive half, 0 on the negative half - in place, tensor layout [inner, n, outer]
__global__ void __launch_bounds__(FT) k_hilbert_mask(double2* __restrict__ a, u64 inner, u64 n, u64 total) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e >= total) return;
    const u64 f = (e / inner) % n;
    double sc;
    if (f == 0) sc = 1.0;
    else if (n % 2 == 0) sc = f < n / 2 ? 2.0 : (f == n / 2 ? 1.0 : 0.0);
    else sc = f <= n / 2 ? 2.0 : 0.0;
    double2 v = a[e];
    v.x *= sc, v.y *= sc;
    a[e] = v;
}

__global__ void __launch_bounds__(FT) k_complex_make(const double* __restrict__ re, u64 re_n, const double* __restrict__ im, u64 im_n, u64 total, int round32,
                                                     double2* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e >= total) return;
    double2 v;
    v.x = re[re_n == 1 ? 0 : e];
    v.y = im ? im[im_n == 1 ? 0 : e] : 0.0;
    if (round32) v.x = (double)(float)v.x, v.y = (double)(float)v.y;
    out[e] = v;
}

__global__ void __launch_bounds__(FT) k_complex_real(const double2* __restrict__ a, u64 total, double* __restrict__ out) {
    const u64 e = (u64)blockIdx.x * FT + threadIdx.x;
    if (e < total) out[e] = a[e].x;
}

}  // namespace
}  // namespace rmhip

extern "C" {

int rmhip_fft_dim(rmhip_ctx* ctx, rmhip_buf a, long long len_or_neg, int dim, int inverse, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return fft_entry(c, a, len_or_neg, dim, inverse != 0, out);
}

int rmhip_spectral_estimate(rmhip_ctx* ctx, rmhip_buf input, size_t input_len, int input_complex, const double* window, size_t window_len, size_t nfft, size_t frame_count,
                            int frame_mode, size_t hop, size_t input_rows, size_t frames_per_column, int range, double denominator, rmhip_buf* s, rmhip_buf* ps, size_t* rows,
                            size_t* cols) {
    CTX_OR_FAIL(ctx);
    const SpectralArgs a{input_len, window_len, nfft, frame_count, hop, input_rows, frames_per_column, input_complex, frame_mode, range, denominator, window};
    return spectral_entry(c, input, a, s, ps, rows, cols);
}

int rmhip_hilbert(rmhip_ctx* ctx, rmhip_buf a, long long len_or_neg, int dim, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (len_or_neg == 0) return fail(RMHIP_ERR_INVALID, "signal_hilbert: invalid request");  // lib.rs:492-494
    Buffer ab;
    RMHIP_TRY(c->get(a, &ab));  // (real input: a complex one is refused here)
    if (dim < 0 || (size_t)dim >= ab.shape.size()) return fail(RMHIP_ERR_INVALID, "signal_hilbert: invalid request");  // lib.rs:495-497
    // hilbert.rs: the analytic signal ifft(fft(x, n, dim) .* mask, n, dim)
    rmhip_buf spec = 0;
    RMHIP_TRY(fft_entry(c, a, len_or_neg, dim, false, &spec));
    Buffer sb;
    int rc = c->get_any(spec, &sb);
    if (rc == RMHIP_OK && sb.numel) {
        u64 inner = 1;
        for (int k = 0; k < dim; ++k) inner *= sb.shape[k];
        const u64 n = (size_t)dim < sb.shape.size() ? sb.shape[dim] : 1;
        hipLaunchKernelGGL(k_hilbert_mask, dim3((unsigned)((sb.numel + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<double2*>(sb.data()), inner, n, (u64)sb.numel);
        c->tel.kernel_launches++;
        if (hipGetLastError() != hipSuccess) rc = fail(RMHIP_ERR_HIP, "signal_hilbert: launch failed");
    }
    if (rc == RMHIP_OK) rc = fft_entry(c, spec, -1, dim, true, out);
    rmhip_free(ctx, spec);
    return rc;
}

int rmhip_complex(rmhip_ctx* ctx, rmhip_buf real, rmhip_buf imag_or_0, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer rb, ib;
    RMHIP_TRY(c->get(real, &rb));
    if (imag_or_0) RMHIP_TRY(c->get(imag_or_0, &ib));
    // complex(real, imag): equal shapes, or either operand a scalar that expands (lib.rs:1949-1959)
    const Buffer* shape_of = &rb;
    if (imag_or_0) {
        if (rb.numel == 1 && ib.numel != 1) shape_of = &ib;
        else if (ib.numel != 1 && ib.shape != rb.shape) return fail(RMHIP_ERR_SHAPE, "complex: real and imaginary parts must have the same size");
    }
    Buffer ob;
    RMHIP_TRY(c->new_buffer_complex(shape_of->shape.data(), shape_of->shape.size(), out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    hipLaunchKernelGGL(k_complex_make, dim3((unsigned)((ob.numel + FT - 1) / FT)), dim3(FT), 0, c->stream, rb.data(), (u64)rb.numel, imag_or_0 ? ib.data() : nullptr,
                       (u64)(imag_or_0 ? ib.numel : 0), (u64)ob.numel, c->precision == 32 ? 1 : 0, reinterpret_cast<double2*>(ob.data()));
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

int rmhip_zeros_complex(rmhip_ctx* ctx, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out || (rank && !shape)) return fail(RMHIP_ERR_INVALID, "zeros: null argument");
    Buffer ob;
    RMHIP_TRY(c->new_buffer_complex(shape, rank, out, &ob));
    if (ob.numel) RMHIP_HIP_CHECK(hipMemsetAsync(ob.data(), 0, 2 * ob.numel * sizeof(double), c->stream));
    return RMHIP_OK;
}

int rmhip_complex_real(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab;
    RMHIP_TRY(c->get_any(a, &ab));
    Buffer ob;
    RMHIP_TRY(c->new_buffer(ab.shape.data(), ab.shape.size(), out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    if (!ab.cplx) {  // already real: the caller frees the transform's handle and keeps this one (ifft.rs:368-371), so it is a copy
        RMHIP_HIP_CHECK(hipMemcpyAsync(ob.data(), ab.data(), ob.numel * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return RMHIP_OK;
    }
    hipLaunchKernelGGL(k_complex_real, dim3((unsigned)((ob.numel + FT - 1) / FT)), dim3(FT), 0, c->stream, reinterpret_cast<const double2*>(ab.data()), (u64)ob.numel,
                       ob.data());
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

}  // extern "C"
