// complex_ew.hip -- elementwise arithmetic on complex-interleaved operands: the second entry points of hooks ew_kernels.hip serves for
// real operands (rmhip_complex_unary / rmhip_complex_binary / rmhip_complex_scalar, rmhip_ops.cpp)
//   elem_add/sub/mul/div      CPU rules: math/elementwise/plus.rs:696-751, minus.rs:724-779, times.rs:702-784, rdivide.rs:633-690
//   scalar_add ... rdiv       the same rules with the real scalar in a kernel argument (no fill + binary)
//   unary_abs/angle/real/imag/conj/sign/sin/cos/tan/sinh/cosh/sinc
// The CPU builtins are the semantics: every part is a chain of separately rounded f64 operations (-ffp-contract=off), so everything
// built from + - * / sqrt, comparisons and negation is bit-exact; sin / cos / sinh / cosh / tanh / hypot / atan2 are the device
// library's, the ones unary_op<> and binary_op<> of ew_kernels.hip call.
// Streaming pattern of ew_kernels.hip: one complex element is one 16-byte double2 per lane, non-temporal, 1024-thread blocks on
// stream_grid with a grid-stride loop, two elements per lane per pass so that two 16-byte loads per stream are in flight.  A complex
// allocation is 16-byte aligned (alloc_device), so a complex stream has no tail case.  Two layouts:
//   tile   lane t of tile T takes elements 2 T B + t and 2 T B + B + t: every wave instruction covers 1 KiB contiguously
//   pair   lane w takes elements 2 w and 2 w + 1: a real stream beside the complex one (or a real result) is then one 16-byte v2
//          access per lane, with the scalar tail k_stream2 has for an odd count
#include "common.h"
#include "skel_common.h"

namespace rmhip {

typedef double v2 __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));

static constexpr int kCx = 1024;      // = kStream of ew_kernels.hip: stream_grid counts blocks of this size
static constexpr int kCxBcast = 256;  // broadcast kernel: a block spans kCxBcast * kCxBcastE elements of dim 0
static constexpr int kCxBcastE = 2;

enum { CX_CC = 0, CX_CR = 1, CX_RC = 2 };  // operand kinds: complex o complex, complex o real, real o complex

static bool cx_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the rules ----------------------------------------------------------------------------------------------------------------------
// num-complex Div (rdivide.rs:633-690): every term kept, also the products with a zero part of a real operand
__device__ __forceinline__ v2 cx_div(v2 a, v2 b) {
    const double d = b.x * b.x + b.y * b.y;
    v2 r = {(a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d};
    return r;
}
template <int OP>
__device__ __forceinline__ v2 cx_cc(v2 a, v2 b) {
    v2 r;
    switch (OP) {
        case RMHIP_ADD: r.x = a.x + b.x, r.y = a.y + b.y; return r;
        case RMHIP_SUB: r.x = a.x - b.x, r.y = a.y - b.y; return r;
        case RMHIP_MUL: r.x = a.x * b.x - a.y * b.y, r.y = a.x * b.y + a.y * b.x; return r;
        default: return cx_div(a, b);
    }
}
template <int OP>
__device__ __forceinline__ v2 cx_cr(v2 a, double s) {  // z op s
    v2 r;
    switch (OP) {
        case RMHIP_ADD: r.x = a.x + s, r.y = a.y; return r;
        case RMHIP_SUB: r.x = a.x - s, r.y = a.y; return r;
        case RMHIP_MUL: r.x = a.x * s, r.y = a.y * s; return r;
        default: r.x = s, r.y = 0.0; return cx_div(a, r);
    }
}
template <int OP>
__device__ __forceinline__ v2 cx_rc(double s, v2 b) {  // s op z
    v2 r;
    switch (OP) {
        case RMHIP_ADD: r.x = s + b.x, r.y = b.y; return r;
        case RMHIP_SUB: r.x = s - b.x, r.y = -b.y; return r;  // a negation: +0 -> -0
        case RMHIP_MUL: r.x = s * b.x, r.y = s * b.y; return r;
        default: r.x = s, r.y = 0.0; return cx_div(r, b);
    }
}

// sign.rs:248-278, branch for branch
__device__ __forceinline__ v2 cx_sign(double re, double im) {
    v2 r = {0.0, 0.0};
    if (re == 0.0 && im == 0.0) return r;
    if (rm_isnan(re) || rm_isnan(im)) {
        r.x = r.y = rm_nan();
        return r;
    }
    const bool re_inf = rm_isinf(re), im_inf = rm_isinf(im);
    if (re_inf || im_inf) {
        const double real = re_inf ? (re > 0.0 ? 1.0 : -1.0) : 0.0;
        const double imag = im_inf ? (im > 0.0 ? 1.0 : -1.0) : 0.0;
        const double norm = sqrt(real * real + imag * imag);
        r.x = real / norm, r.y = imag / norm;  // (norm is 1 or sqrt(2) here, never 0)
        return r;
    }
    const double scale = fmax(fabs(re), fabs(im));
    if (scale == 0.0) return r;
    const double nr = re / scale, ni = im / scale;
    const double magnitude = sqrt(nr * nr + ni * ni);
    if (magnitude == 0.0) return r;
    r.x = nr / magnitude, r.y = ni / magnitude;
    return r;
}
// signal/sinc.rs:313-327: the real rule on the real axis, otherwise sin(pi z) / (pi z) with the denominator's norm as ONE fused operation
__device__ __forceinline__ v2 cx_sinc(double re, double im) {
    v2 r;
    if (im == 0.0) {
        r.x = rm_sinc(re), r.y = 0.0;
        return r;
    }
    const double sr = 3.14159265358979323846 * re, si = 3.14159265358979323846 * im;
    const double nr = sin(sr) * cosh(si), ni = cos(sr) * sinh(si);
    const double d = __builtin_fma(sr, sr, si * si);
    r.x = (nr * sr + ni * si) / d, r.y = (ni * sr - nr * si) / d;
    return r;
}
template <int OP>
__device__ __forceinline__ v2 cx_unary(v2 z) {  // complex results
    v2 r;
    switch (OP) {
        case RMHIP_CCONJ: r.x = z.x, r.y = -z.y; return r;
        case RMHIP_CSIGN: return cx_sign(z.x, z.y);
        case RMHIP_CSIN: r.x = sin(z.x) * cosh(z.y), r.y = cos(z.x) * sinh(z.y); return r;     // sin.rs:280-287
        case RMHIP_CCOS: r.x = cos(z.x) * cosh(z.y), r.y = (-sin(z.x)) * sinh(z.y); return r;  // cos.rs:277-284
        case RMHIP_CSINH: r.x = sinh(z.x) * cos(z.y), r.y = cosh(z.x) * sin(z.y); return r;    // sinh.rs:190-197
        case RMHIP_CCOSH: r.x = cosh(z.x) * cos(z.y), r.y = sinh(z.x) * sin(z.y); return r;    // cosh.rs:190-197
        case RMHIP_CTAN: {                                                                    // tan.rs:283-291
            const double two_re = 2.0 * z.x, two_im = 2.0 * z.y;
            const double inv_cosh = 1.0 / cosh(two_im);
            const double denom = 1.0 + cos(two_re) * inv_cosh;
            r.x = (sin(two_re) * inv_cosh) / denom, r.y = tanh(two_im) / denom;
            return r;
        }
        default: return cx_sinc(z.x, z.y);
    }
}
template <int OP>
__device__ __forceinline__ double cx_unary_real(v2 z) {  // real results
    switch (OP) {
        case RMHIP_CABS: return hypot(z.x, z.y);     // abs.rs:181
        case RMHIP_CANGLE: return atan2(z.y, z.x);   // angle.rs:192
        case RMHIP_CREAL: return z.x;
        default: return z.y;
    }
}

// a complex result of a precision-32 context: each part rounded through f32 once, storage stays 2 x f64 (rmhip.h, complex section)
__device__ __forceinline__ v2 cx_round(v2 r, int r32) {
    if (r32) r.x = rm_f32(r.x), r.y = rm_f32(r.y);
    return r;
}

// ---- binary / scalar, operands of the output's shape or one-element ---------------------------------------------------------------------
// A streaming operand (AS / BS) is read per element; the other one is a single value read once: from its pointer, or - a real scalar
// of rmhip_complex_scalar, pointer null - from the kernel argument `s`.
template <int OP, int KIND>
__device__ __forceinline__ v2 cx_apply(v2 a, v2 b) {  // a real operand travels in .x
    if (KIND == CX_CC) return cx_cc<OP>(a, b);
    if (KIND == CX_CR) return cx_cr<OP>(a, b.x);
    return cx_rc<OP>(a.x, b);
}
template <bool CPLX>
__device__ __forceinline__ v2 cx_load_one(const double* p, double s) {
    v2 r = {s, 0.0};
    if (!p) return r;
    if (CPLX) return *(const v2*)p;
    r.x = p[0];
    return r;
}
template <bool CPLX>
__device__ __forceinline__ v2 cx_load(const double* p, size_t e) {
    if (CPLX) return __builtin_nontemporal_load((const v2*)p + e);
    v2 r = {__builtin_nontemporal_load(p + e), 0.0};
    return r;
}

// tile layout: no real v2 access (complex o complex, a real operand that does not stream, or real storage that is not 16-byte aligned)
template <int OP, int KIND, bool AS, bool BS>
__global__ void __launch_bounds__(kCx) k_cx_binary_tile(const double* __restrict__ a, const double* __restrict__ b, double s, double* __restrict__ out,
                                                       size_t n, int r32) {
    constexpr bool AC = KIND != CX_RC, BC = KIND != CX_CR;
    v2 x0 = cx_load_one<AC>(AS ? nullptr : a, s), y0 = cx_load_one<BC>(BS ? nullptr : b, s);
    v2 x1 = x0, y1 = y0;
    v2* __restrict__ ov = (v2*)out;
    for (size_t base = (size_t)blockIdx.x * (2 * kCx); base < n; base += (size_t)gridDim.x * (2 * kCx)) {
        const size_t e0 = base + threadIdx.x, e1 = e0 + kCx;
        const bool ok0 = e0 < n, ok1 = e1 < n;
        if (AS) {
            if (ok0) x0 = cx_load<AC>(a, e0);
            if (ok1) x1 = cx_load<AC>(a, e1);
        }
        if (BS) {
            if (ok0) y0 = cx_load<BC>(b, e0);
            if (ok1) y1 = cx_load<BC>(b, e1);
        }
        if (ok0) __builtin_nontemporal_store(cx_round(cx_apply<OP, KIND>(x0, y0), r32), ov + e0);
        if (ok1) __builtin_nontemporal_store(cx_round(cx_apply<OP, KIND>(x1, y1), r32), ov + e1);
    }
}

// pair layout: the real operand streams as one v2 per lane (KIND is CX_CR with BS, or CX_RC with AS)
template <int OP, int KIND, bool AS, bool BS>
__global__ void __launch_bounds__(kCx) k_cx_binary_pair(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out, size_t n,
                                                       int r32) {
    constexpr bool AC = KIND != CX_RC, BC = KIND != CX_CR;
    static_assert((!AC && AS) || (!BC && BS), "the pair layout is for a streaming real operand");
    const v2 xc = cx_load_one<AC>(AS ? nullptr : a, 0.0), yc = cx_load_one<BC>(BS ? nullptr : b, 0.0);
    const size_t npair = n >> 1, stride = (size_t)gridDim.x * kCx;
    v2* __restrict__ ov = (v2*)out;
    for (size_t w = (size_t)blockIdx.x * kCx + threadIdx.x; w < npair; w += stride) {
        v2 x0 = xc, x1 = xc, y0 = yc, y1 = yc;
        if (AS) {
            if (AC) x0 = cx_load<true>(a, 2 * w), x1 = cx_load<true>(a, 2 * w + 1);
            else {
                const v2 r = __builtin_nontemporal_load((const v2*)a + w);
                x0.x = r.x, x1.x = r.y;
            }
        }
        if (BS) {
            if (BC) y0 = cx_load<true>(b, 2 * w), y1 = cx_load<true>(b, 2 * w + 1);
            else {
                const v2 r = __builtin_nontemporal_load((const v2*)b + w);
                y0.x = r.x, y1.x = r.y;
            }
        }
        __builtin_nontemporal_store(cx_round(cx_apply<OP, KIND>(x0, y0), r32), ov + 2 * w);
        __builtin_nontemporal_store(cx_round(cx_apply<OP, KIND>(x1, y1), r32), ov + 2 * w + 1);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t t = n - 1;
        const v2 x = AS ? cx_load<AC>(a, t) : xc, y = BS ? cx_load<BC>(b, t) : yc;
        ov[t] = cx_round(cx_apply<OP, KIND>(x, y), r32);
    }
}

template <int OP, int KIND, bool AS, bool BS>
static int cx_binary_launch(Context* c, const double* a, const double* b, double s, double* out, size_t n) {
    const int r32 = c->precision == 32 ? 1 : 0;
    constexpr bool real_stream = (KIND == CX_CR && BS) || (KIND == CX_RC && AS);
    if constexpr (real_stream) {
        if (cx_aligned16(KIND == CX_CR ? b : a) && n >= 2) {
            hipLaunchKernelGGL((k_cx_binary_pair<OP, KIND, AS, BS>), dim3(stream_grid(c, n >> 1)), dim3(kCx), 0, c->stream, a, b, out, n, r32);
            c->tel.kernel_launches++;
            RMHIP_HIP_CHECK(hipGetLastError());
            return RMHIP_OK;
        }
    }
    hipLaunchKernelGGL((k_cx_binary_tile<OP, KIND, AS, BS>), dim3(stream_grid(c, (n + 1) >> 1)), dim3(kCx), 0, c->stream, a, b, s, out, n, r32);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}
template <int OP, int KIND>
static int cx_binary_streams(Context* c, const double* a, bool a_streams, const double* b, bool b_streams, double s, double* out, size_t n) {
    if (a_streams && b_streams) return cx_binary_launch<OP, KIND, true, true>(c, a, b, s, out, n);
    if (a_streams) return cx_binary_launch<OP, KIND, true, false>(c, a, b, s, out, n);
    return cx_binary_launch<OP, KIND, false, true>(c, a, b, s, out, n);
}
template <int OP>
static int cx_binary_kind(Context* c, int kind, const double* a, bool a_streams, const double* b, bool b_streams, double s, double* out, size_t n) {
    if (kind == CX_CC) return cx_binary_streams<OP, CX_CC>(c, a, a_streams, b, b_streams, s, out, n);
    if (kind == CX_CR) return cx_binary_streams<OP, CX_CR>(c, a, a_streams, b, b_streams, s, out, n);
    return cx_binary_streams<OP, CX_RC>(c, a, a_streams, b, b_streams, s, out, n);
}

int launch_complex_binary_same(Context* c, int op, int kind, const double* a, bool a_streams, const double* b, bool b_streams, double s, double* out,
                               size_t n) {
    if (n == 0) return RMHIP_OK;
    if (!a_streams && !b_streams) a_streams = b_streams = n == 1 && a && b;  // two one-element tensors: a one-element stream
    if (!a_streams && !b_streams) return fail(RMHIP_ERR_INVALID, "complex elementwise: no operand has the output's shape");
    switch (op) {
        case RMHIP_ADD: return cx_binary_kind<RMHIP_ADD>(c, kind, a, a_streams, b, b_streams, s, out, n);
        case RMHIP_SUB: return cx_binary_kind<RMHIP_SUB>(c, kind, a, a_streams, b, b_streams, s, out, n);
        case RMHIP_MUL: return cx_binary_kind<RMHIP_MUL>(c, kind, a, a_streams, b, b_streams, s, out, n);
        case RMHIP_DIV: return cx_binary_kind<RMHIP_DIV>(c, kind, a, a_streams, b, b_streams, s, out, n);
        default: return fail(RMHIP_ERR_UNSUPPORTED, "binary op %d is not served for complex operands", op);
    }
}

// ---- broadcasting: launch_binary_bcast's collapsed stride table, strides in elements of each operand's own kind ------------------------
// dim 0 along the threads, the outer dimensions decoded once per block with scalar arithmetic (k_bcast2 of ew_kernels.hip)
struct CxBcastParams {
    unsigned long long d0, nchunks;
    int rank;
    unsigned long long shape[8], sa[8], sb[8];
};
template <int OP, int KIND>
__global__ void __launch_bounds__(kCxBcast) k_cx_bcast(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out,
                                                      CxBcastParams p, int r32) {
    constexpr bool AC = KIND != CX_RC, BC = KIND != CX_CR;
    const unsigned long long blk = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;
    const unsigned long long chunk = blk % p.nchunks;
    const unsigned long long outer = blk / p.nchunks;
    unsigned long long offa = 0, offb = 0, rem = outer;
    for (int d = 1; d < p.rank; ++d) {
        const unsigned long long cdim = rem % p.shape[d];
        rem /= p.shape[d];
        offa += cdim * p.sa[d];
        offb += cdim * p.sb[d];
    }
    if (rem != 0) return;
    const unsigned long long obase = outer * p.d0;
    const unsigned long long i0 = chunk * (unsigned long long)(kCxBcast * kCxBcastE) + threadIdx.x;
    v2 x[kCxBcastE], y[kCxBcastE];
#pragma unroll
    for (int e = 0; e < kCxBcastE; ++e) {
        const unsigned long long i = i0 + (unsigned long long)e * kCxBcast;
        x[e].x = x[e].y = 0.0, y[e].x = 1.0, y[e].y = 0.0;
        if (i < p.d0) {
            const unsigned long long ia = offa + i * p.sa[0], ib = offb + i * p.sb[0];
            if (AC) x[e] = *((const v2*)a + ia);
            else x[e].x = a[ia];
            if (BC) y[e] = *((const v2*)b + ib);
            else y[e].x = b[ib];
        }
    }
#pragma unroll
    for (int e = 0; e < kCxBcastE; ++e) {
        const unsigned long long i = i0 + (unsigned long long)e * kCxBcast;
        if (i < p.d0) __builtin_nontemporal_store(cx_round(cx_apply<OP, KIND>(x[e], y[e]), r32), (v2*)out + obase + i);
    }
}
template <int OP, int KIND>
static int cx_bcast_launch(Context* c, const double* a, const double* b, double* out, const CxBcastParams& p, unsigned long long blocks) {
    const unsigned long long gx = blocks < 1048576ULL ? blocks : 1048576ULL;
    const unsigned long long gy = (blocks + gx - 1) / gx;
    if (gy > 65535ULL) return fail(RMHIP_ERR_UNSUPPORTED, "broadcast grid too large");
    hipLaunchKernelGGL((k_cx_bcast<OP, KIND>), dim3((unsigned)gx, (unsigned)gy), dim3(kCxBcast), 0, c->stream, a, b, out, p, c->precision == 32 ? 1 : 0);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}
template <int OP>
static int cx_bcast_kind(Context* c, int kind, const double* a, const double* b, double* out, const CxBcastParams& p, unsigned long long blocks) {
    if (kind == CX_CC) return cx_bcast_launch<OP, CX_CC>(c, a, b, out, p, blocks);
    if (kind == CX_CR) return cx_bcast_launch<OP, CX_CR>(c, a, b, out, p, blocks);
    return cx_bcast_launch<OP, CX_RC>(c, a, b, out, p, blocks);
}
int launch_complex_binary_bcast(Context* c, int op, int kind, const double* a, const double* b, double* out, size_t n, const BroadcastDesc& d) {
    if (n == 0) return RMHIP_OK;
    CxBcastParams p;
    p.rank = d.rank;
    p.d0 = d.out_shape[0];
    p.nchunks = (p.d0 + (unsigned long long)kCxBcast * kCxBcastE - 1) / ((unsigned long long)kCxBcast * kCxBcastE);
    unsigned long long outer = 1;
    for (int i = 0; i < 8; ++i) {
        p.shape[i] = i < d.rank ? d.out_shape[i] : 1;
        p.sa[i] = i < d.rank ? d.stride_a[i] : 0;
        p.sb[i] = i < d.rank ? d.stride_b[i] : 0;
        if (i >= 1 && i < d.rank) outer *= d.out_shape[i];
    }
    const unsigned long long blocks = p.nchunks * outer;
    switch (op) {
        case RMHIP_ADD: return cx_bcast_kind<RMHIP_ADD>(c, kind, a, b, out, p, blocks);
        case RMHIP_SUB: return cx_bcast_kind<RMHIP_SUB>(c, kind, a, b, out, p, blocks);
        case RMHIP_MUL: return cx_bcast_kind<RMHIP_MUL>(c, kind, a, b, out, p, blocks);
        case RMHIP_DIV: return cx_bcast_kind<RMHIP_DIV>(c, kind, a, b, out, p, blocks);
        default: return fail(RMHIP_ERR_UNSUPPORTED, "binary op %d is not served for complex operands", op);
    }
}

// ---- unary ----------------------------------------------------------------------------------------------------------------------------------
template <int OP>
__global__ void __launch_bounds__(kCx) k_cx_unary(const double* __restrict__ a, double* __restrict__ out, size_t n, int r32) {
    const v2* __restrict__ av = (const v2*)a;
    v2* __restrict__ ov = (v2*)out;
    for (size_t base = (size_t)blockIdx.x * (2 * kCx); base < n; base += (size_t)gridDim.x * (2 * kCx)) {
        const size_t e0 = base + threadIdx.x, e1 = e0 + kCx;
        const bool ok0 = e0 < n, ok1 = e1 < n;
        v2 x0 = {0.0, 0.0}, x1 = x0;
        if (ok0) x0 = __builtin_nontemporal_load(av + e0);
        if (ok1) x1 = __builtin_nontemporal_load(av + e1);
        if (ok0) __builtin_nontemporal_store(cx_round(cx_unary<OP>(x0), r32), ov + e0);
        if (ok1) __builtin_nontemporal_store(cx_round(cx_unary<OP>(x1), r32), ov + e1);
    }
}
// real results: 8 bytes per element (4 in f32 storage), two per lane in one store
template <int OP, class T>
__global__ void __launch_bounds__(kCx) k_cx_unary_real(const double* __restrict__ a, T* __restrict__ out, size_t n) {
    typedef T VT __attribute__((ext_vector_type(2)));
    const v2* __restrict__ av = (const v2*)a;
    const size_t npair = n >> 1, stride = (size_t)gridDim.x * kCx;
    for (size_t w = (size_t)blockIdx.x * kCx + threadIdx.x; w < npair; w += stride) {
        const v2 x0 = __builtin_nontemporal_load(av + 2 * w), x1 = __builtin_nontemporal_load(av + 2 * w + 1);
        VT r = {(T)cx_unary_real<OP>(x0), (T)cx_unary_real<OP>(x1)};
        __builtin_nontemporal_store(r, (VT*)out + w);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = (T)cx_unary_real<OP>(av[n - 1]);
}

template <int OP>
static int cx_unary_launch(Context* c, const double* a, double* out, size_t n) {
    hipLaunchKernelGGL((k_cx_unary<OP>), dim3(stream_grid(c, (n + 1) >> 1)), dim3(kCx), 0, c->stream, a, out, n, c->precision == 32 ? 1 : 0);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}
template <int OP>
static int cx_unary_real_launch(Context* c, const double* a, void* out, bool out_f32, size_t n) {
    const unsigned grid = stream_grid(c, (n + 1) >> 1);
    if (out_f32) hipLaunchKernelGGL((k_cx_unary_real<OP, float>), dim3(grid), dim3(kCx), 0, c->stream, a, (float*)out, n);
    else hipLaunchKernelGGL((k_cx_unary_real<OP, double>), dim3(grid), dim3(kCx), 0, c->stream, a, (double*)out, n);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

bool complex_unary_is_real(int op) { return op == RMHIP_CABS || op == RMHIP_CANGLE || op == RMHIP_CREAL || op == RMHIP_CIMAG; }

int launch_complex_unary(Context* c, int op, const double* a, void* out, bool out_f32, size_t n) {
    if (n == 0) return RMHIP_OK;
    switch (op) {
        case RMHIP_CABS: return cx_unary_real_launch<RMHIP_CABS>(c, a, out, out_f32, n);
        case RMHIP_CANGLE: return cx_unary_real_launch<RMHIP_CANGLE>(c, a, out, out_f32, n);
        case RMHIP_CREAL: return cx_unary_real_launch<RMHIP_CREAL>(c, a, out, out_f32, n);
        case RMHIP_CIMAG: return cx_unary_real_launch<RMHIP_CIMAG>(c, a, out, out_f32, n);
        case RMHIP_CCONJ: return cx_unary_launch<RMHIP_CCONJ>(c, a, (double*)out, n);
        case RMHIP_CSIGN: return cx_unary_launch<RMHIP_CSIGN>(c, a, (double*)out, n);
        case RMHIP_CSIN: return cx_unary_launch<RMHIP_CSIN>(c, a, (double*)out, n);
        case RMHIP_CCOS: return cx_unary_launch<RMHIP_CCOS>(c, a, (double*)out, n);
        case RMHIP_CTAN: return cx_unary_launch<RMHIP_CTAN>(c, a, (double*)out, n);
        case RMHIP_CSINH: return cx_unary_launch<RMHIP_CSINH>(c, a, (double*)out, n);
        case RMHIP_CCOSH: return cx_unary_launch<RMHIP_CCOSH>(c, a, (double*)out, n);
        case RMHIP_CSINC: return cx_unary_launch<RMHIP_CSINC>(c, a, (double*)out, n);
        default: return fail(RMHIP_ERR_UNSUPPORTED, "complex unary op %d not supported by provider", op);
    }
}

}  // namespace rmhip
