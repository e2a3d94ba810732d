// workload_ops.hip -- three closed-form workload hooks: several resident operands in, one expression per element, one launch each.
//   black_scholes_price   crates/runmat-accelerate-api/src/lib.rs:1572-1579   (simple_provider.rs:800-883, 2855-2920)
//   adam_update           lib.rs:1582-1587                                    (simple_provider.rs:985-1064, 2922-3009)
//   crossentropy_terms    lib.rs:1590-1597                                    (simple_provider.rs:1066-1137, 3011-3095)
// The CPU provider is the contract: every kernel keeps its operation order (the Makefile's -ffp-contract=off keeps products and sums
// separately rounded), so Adam is bit-exact and the other two differ from the CPU only through the device's log / exp / erf.
// adam_update and crossentropy_terms stream (56 and at most 40 bytes per f64 element, 16-byte accesses per lane, no LDS) and validate
// on the device: failing lanes lower one 32-bit verdict word of the context to their priority code - reduced per wave, then a single
// atomicMin - and the host reads it back once after the kernel.  black_scholes_price needs no verdict (a bad element prices to NaN).
// Precision-32 contexts: f32 loads and stores, f64 arithmetic in registers, one rounding on store.
#include <cmath>
#include <vector>

#include "common.h"
#include "host_shape.h"

using namespace rmhip;

namespace rmhip {
namespace {

typedef unsigned long long u64;
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// 16-byte vector of the storage type T
template <class T>
struct VecOf;
template <>
struct VecOf<double> {
    typedef v2d type;
    static constexpr int N = 2;
};
template <>
struct VecOf<float> {
    typedef v4f type;
    static constexpr int N = 4;
};

constexpr int kStream = 1024;  // the streaming hooks' block (ew_kernels.hip)
constexpr int kPriceBlock = 256;
constexpr unsigned kVerdictNone = 0xffffffffu;  // what the host resets the verdict word to: no lane failed

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grid of the streaming kernels: as ew_kernels.hip sizes its own (16 blocks per CU at most, a grid-stride loop for the rest)
inline unsigned stream_grid(const Context* c, size_t work_items, int block) {
    size_t want = (work_items + block - 1) / block;
    const size_t cap = (size_t)c->num_cus * 16;
    if (want < 1) want = 1;
    return (unsigned)(want < cap ? want : cap);
}

__device__ __forceinline__ bool is_finite(double x) { return __builtin_isfinite(x); }

// Every thread of the block calls this once, at the end of its kernel: the smallest code of the wave, then one atomic per failing wave.
__device__ __forceinline__ void report_verdict(unsigned code, unsigned* __restrict__ verdict) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)code, o);
        code = other < code ? other : code;
    }
    if ((threadIdx.x & 63) == 0 && code != kVerdictNone) atomicMin(verdict, code);
}

// ---- adam_update ----------------------------------------------------------------------------------------------------------------
enum : unsigned { kAdamBadInput = 0, kAdamBadOutput = 1 };  // input wins over output (simple_provider.rs:1020-1026 runs before the loop)

struct AdamScalars {
    double b1, one_minus_b1, b2, one_minus_b2, learn_rate, grad_correction, sq_grad_correction, epsilon;
};

// simple_provider.rs:1039-1053, operation for operation: true divisions and a correctly rounded square root
__device__ __forceinline__ unsigned adam_one(double p0, double g, double m0, double v0, const AdamScalars& a, double& p, double& m,
                                             double& v) {
    m = a.b1 * m0 + a.one_minus_b1 * g;
    v = a.b2 * v0 + (a.one_minus_b2 * g) * g;
    const double corrected = m / a.grad_correction;
    const double corrected_sq = v / a.sq_grad_correction;
    const double step = (a.learn_rate * corrected) / (sqrt(corrected_sq) + a.epsilon);
    p = p0 - step;
    if (!(is_finite(p0) && is_finite(g) && is_finite(m0) && is_finite(v0))) return kAdamBadInput;
    if (!(is_finite(p) && is_finite(m) && is_finite(v))) return kAdamBadOutput;
    return kVerdictNone;
}

// HM / HV: the moment is present.  An absent one is zeros (simple_provider.rs:2963, 2970) and is not read: 0.0 stands in its place,
// so b * 0.0 + x rounds exactly as the CPU's sum over a zero vector does.  `vec` == 0 (a base that is not 16-byte aligned): every
// element goes through the scalar loop, which otherwise takes the n % N tail.
template <class T, bool HM, bool HV>
__global__ void __launch_bounds__(kStream) k_adam_update(const T* __restrict__ p, const T* __restrict__ g, const T* __restrict__ m0,
                                                         const T* __restrict__ v0, T* __restrict__ po, T* __restrict__ mo,
                                                         T* __restrict__ vo, size_t n, int vec, const AdamScalars a,
                                                         unsigned* __restrict__ verdict) {
    typedef typename VecOf<T>::type V;
    constexpr int N = VecOf<T>::N;
    const size_t nvec = vec ? n / N : 0;
    const size_t stride = (size_t)gridDim.x * kStream;
    const size_t t0 = (size_t)blockIdx.x * kStream + threadIdx.x;
    unsigned code = kVerdictNone;
    for (size_t i = t0; i < nvec; i += stride) {
        const V pv = __builtin_nontemporal_load((const V*)p + i), gv = __builtin_nontemporal_load((const V*)g + i);
        V mv = {}, vv = {};
        if (HM) mv = __builtin_nontemporal_load((const V*)m0 + i);
        if (HV) vv = __builtin_nontemporal_load((const V*)v0 + i);
        V rp, rm, rv;
#pragma unroll
        for (int l = 0; l < N; ++l) {
            double pn, mn, vn;
            const unsigned e = adam_one((double)pv[l], (double)gv[l], HM ? (double)mv[l] : 0.0, HV ? (double)vv[l] : 0.0, a, pn, mn, vn);
            code = e < code ? e : code;
            rp[l] = (T)pn;
            rm[l] = (T)mn;
            rv[l] = (T)vn;
        }
        __builtin_nontemporal_store(rp, (V*)po + i);
        __builtin_nontemporal_store(rm, (V*)mo + i);
        __builtin_nontemporal_store(rv, (V*)vo + i);
    }
    for (size_t i = nvec * N + t0; i < n; i += stride) {
        double pn, mn, vn;
        const unsigned e = adam_one((double)p[i], (double)g[i], HM ? (double)m0[i] : 0.0, HV ? (double)v0[i] : 0.0, a, pn, mn, vn);
        code = e < code ? e : code;
        po[i] = (T)pn;
        mo[i] = (T)mn;
        vo[i] = (T)vn;
    }
    report_verdict(code, verdict);
}

template <class T>
int launch_adam(Context* c, const T* p, const T* g, const T* m0, const T* v0, T* po, T* mo, T* vo, size_t n, const AdamScalars& a,
                unsigned* verdict) {
    const int vec = aligned16(p) && aligned16(g) && aligned16(m0) && aligned16(v0) && aligned16(po) && aligned16(mo) && aligned16(vo);
    const dim3 grid(stream_grid(c, vec ? n / VecOf<T>::N : n, kStream)), block(kStream);
    if (m0 && v0) hipLaunchKernelGGL((k_adam_update<T, true, true>), grid, block, 0, c->stream, p, g, m0, v0, po, mo, vo, n, vec, a, verdict);
    else if (m0) hipLaunchKernelGGL((k_adam_update<T, true, false>), grid, block, 0, c->stream, p, g, m0, v0, po, mo, vo, n, vec, a, verdict);
    else if (v0) hipLaunchKernelGGL((k_adam_update<T, false, true>), grid, block, 0, c->stream, p, g, m0, v0, po, mo, vo, n, vec, a, verdict);
    else hipLaunchKernelGGL((k_adam_update<T, false, false>), grid, block, 0, c->stream, p, g, m0, v0, po, mo, vo, n, vec, a, verdict);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

// ---- crossentropy_terms ---------------------------------------------------------------------------------------------------------
// priority when several classes occur; the CPU orders the last two by element index, which one pass over the data does not reproduce
enum : unsigned { kCeBadInput = 0, kCeBadWeight = 1, kCeBadMask = 2, kCeBadTarget = 3, kCeBadLoss = 4 };

// simple_provider.rs:1110-1134
template <bool MULTI, bool HW, bool HK>
__device__ __forceinline__ unsigned ce_one(double pred, double t, double w, double k, double& loss) {
    const double eps = 1.0e-12, hi = 1.0 - eps;
    const double clipped = pred < eps ? eps : (pred > hi ? hi : pred);  // f64::clamp
    loss = (-t) * log(clipped);
    if (MULTI) loss = loss - (1.0 - t) * log(1.0 - clipped);
    if (HW) loss *= w;
    if (HK) loss *= k;
    if (!(is_finite(pred) && is_finite(t))) return kCeBadInput;
    if (HW && !(is_finite(w) && w >= 0.0)) return kCeBadWeight;
    if (HK && !(k == 0.0 || k == 1.0)) return kCeBadMask;
    if (!(t >= 0.0 && t <= 1.0)) return kCeBadTarget;
    if (!is_finite(loss)) return kCeBadLoss;
    return kVerdictNone;
}

template <class T, bool MULTI, bool HW, bool HK>
__global__ void __launch_bounds__(kStream) k_crossentropy_terms(const T* __restrict__ pred, const T* __restrict__ target,
                                                                const T* __restrict__ weight, const T* __restrict__ mask,
                                                                T* __restrict__ out, size_t n, int vec, unsigned* __restrict__ verdict) {
    typedef typename VecOf<T>::type V;
    constexpr int N = VecOf<T>::N;
    const size_t nvec = vec ? n / N : 0;
    const size_t stride = (size_t)gridDim.x * kStream;
    const size_t t0 = (size_t)blockIdx.x * kStream + threadIdx.x;
    unsigned code = kVerdictNone;
    for (size_t i = t0; i < nvec; i += stride) {
        const V pv = __builtin_nontemporal_load((const V*)pred + i), tv = __builtin_nontemporal_load((const V*)target + i);
        V wv = {}, kv = {};
        if (HW) wv = __builtin_nontemporal_load((const V*)weight + i);
        if (HK) kv = __builtin_nontemporal_load((const V*)mask + i);
        V r;
#pragma unroll
        for (int l = 0; l < N; ++l) {
            double loss;
            const unsigned e = ce_one<MULTI, HW, HK>((double)pv[l], (double)tv[l], (double)wv[l], (double)kv[l], loss);
            code = e < code ? e : code;
            r[l] = (T)loss;
        }
        __builtin_nontemporal_store(r, (V*)out + i);
    }
    for (size_t i = nvec * N + t0; i < n; i += stride) {
        double loss;
        const unsigned e = ce_one<MULTI, HW, HK>((double)pred[i], (double)target[i], HW ? (double)weight[i] : 1.0, HK ? (double)mask[i] : 1.0, loss);
        code = e < code ? e : code;
        out[i] = (T)loss;
    }
    report_verdict(code, verdict);
}

template <class T, bool MULTI>
int launch_crossentropy_mode(Context* c, const T* pred, const T* target, const T* weight, const T* mask, T* out, size_t n,
                             unsigned* verdict) {
    const int vec = aligned16(pred) && aligned16(target) && aligned16(weight) && aligned16(mask) && aligned16(out);
    const dim3 grid(stream_grid(c, vec ? n / VecOf<T>::N : n, kStream)), block(kStream);
    if (weight && mask) hipLaunchKernelGGL((k_crossentropy_terms<T, MULTI, true, true>), grid, block, 0, c->stream, pred, target, weight, mask, out, n, vec, verdict);
    else if (weight) hipLaunchKernelGGL((k_crossentropy_terms<T, MULTI, true, false>), grid, block, 0, c->stream, pred, target, weight, mask, out, n, vec, verdict);
    else if (mask) hipLaunchKernelGGL((k_crossentropy_terms<T, MULTI, false, true>), grid, block, 0, c->stream, pred, target, weight, mask, out, n, vec, verdict);
    else hipLaunchKernelGGL((k_crossentropy_terms<T, MULTI, false, false>), grid, block, 0, c->stream, pred, target, weight, mask, out, n, vec, verdict);
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

template <class T>
int launch_crossentropy(Context* c, bool multi, const T* pred, const T* target, const T* weight, const T* mask, T* out, size_t n,
                        unsigned* verdict) {
    return multi ? launch_crossentropy_mode<T, true>(c, pred, target, weight, mask, out, n, verdict)
                 : launch_crossentropy_mode<T, false>(c, pred, target, weight, mask, out, n, verdict);
}

// ---- black_scholes_price --------------------------------------------------------------------------------------------------------
// simple_provider.rs:839-883.  N(x) = 0.5 * (1 + erf(x / SQRT_2)).  erf is odd bit for bit and (-d) / SQRT_2 == -(d / SQRT_2), so
// N(-d) = 0.5 * (1 + -erf(d / SQRT_2)) reuses the erf computed for N(d): two erf evaluations per element instead of the CPU's four,
// with the same bits.
__device__ __forceinline__ void price_pair(double price, double strike, double rate, double time, double vol, double yield, double& call,
                                           double& put) {
    if (!(is_finite(price) && is_finite(strike) && is_finite(rate) && is_finite(time) && is_finite(vol) && is_finite(yield) && price >= 0.0 && strike > 0.0 &&
          time >= 0.0 && vol >= 0.0)) {
        call = put = __builtin_nan("");
        return;
    }
    const double discounted_price = price * exp((-yield) * time);
    const double discounted_strike = strike * exp((-rate) * time);
    if (time == 0.0 || vol == 0.0) {  // the intrinsic pair
        call = fmax(discounted_price - discounted_strike, 0.0);
        put = fmax(discounted_strike - discounted_price, 0.0);
        return;
    }
    const double sqrt_time = sqrt(time);
    const double d1 = (log(price / strike) + (rate - yield + 0.5 * vol * vol) * time) / (vol * sqrt_time);
    const double d2 = d1 - vol * sqrt_time;
    const double e1 = erf(d1 / 1.4142135623730951), e2 = erf(d2 / 1.4142135623730951);
    const double n_d1 = 0.5 * (1.0 + e1), n_d2 = 0.5 * (1.0 + e2);
    const double n_md1 = 0.5 * (1.0 + -e1), n_md2 = 0.5 * (1.0 + -e2);
    call = discounted_price * n_d1 - discounted_strike * n_d2;
    put = discounted_strike * n_md2 - discounted_price * n_md1;
}

template <class T>
struct PriceInputs {
    const T* p[6];  // Price, Strike, Rate, Time, Volatility, Yield
};

// Flat path: every input is output-shaped and contiguous, or one element (bit k of scalar_mask), which a thread loads once.
template <class T>
__global__ void __launch_bounds__(kPriceBlock) k_black_scholes_flat(const PriceInputs<T> in, unsigned scalar_mask, T* __restrict__ call,
                                                                    T* __restrict__ put, size_t n, int vec) {
    typedef typename VecOf<T>::type V;
    constexpr int N = VecOf<T>::N;
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = ((scalar_mask >> k) & 1u) ? (double)in.p[k][0] : 0.0;
    const size_t nvec = vec ? n / N : 0;
    const size_t stride = (size_t)gridDim.x * kPriceBlock;
    const size_t t0 = (size_t)blockIdx.x * kPriceBlock + threadIdx.x;
    for (size_t i = t0; i < nvec; i += stride) {
        V xv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            xv[k] = V{};
            if (!((scalar_mask >> k) & 1u)) xv[k] = __builtin_nontemporal_load((const V*)in.p[k] + i);
        }
        V rc, rp;
#pragma unroll
        for (int l = 0; l < N; ++l) {
            double x[6], cv, pv;
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = ((scalar_mask >> k) & 1u) ? s[k] : (double)xv[k][l];
            price_pair(x[0], x[1], x[2], x[3], x[4], x[5], cv, pv);
            rc[l] = (T)cv;
            rp[l] = (T)pv;
        }
        __builtin_nontemporal_store(rc, (V*)call + i);
        __builtin_nontemporal_store(rp, (V*)put + i);
    }
    for (size_t i = nvec * N + t0; i < n; i += stride) {
        double x[6], cv, pv;
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = ((scalar_mask >> k) & 1u) ? s[k] : (double)in.p[k][i];
        price_pair(x[0], x[1], x[2], x[3], x[4], x[5], cv, pv);
        call[i] = (T)cv;
        put[i] = (T)pv;
    }
}

// General path: provider_broadcast_index (simple_provider.rs:800-837) over the collapsed dimensions.  A dimension an input broadcasts
// carries stride 0.  The struct travels by value and is read with constant indices only (loops unrolled against kPriceRankMax), so it
// stays in the kernel-argument segment instead of a scratch copy.
constexpr int kPriceRankMax = 8;
template <class I>
struct PriceDims {  // in the index type: 57 words of 32 bits stay in scalar registers, 57 of 64 bits would not
    int rank;
    I shape[kPriceRankMax];
    I stride[6][kPriceRankMax];
};

// I = unsigned below 2^32 outputs: a 64-bit division is ~20 times the instructions of a 32-bit one (misc_ops.hip k_kron)
template <class T, class I>
__global__ void __launch_bounds__(kPriceBlock) k_black_scholes_strided(const PriceInputs<T> in, const PriceDims<I> d, T* __restrict__ call,
                                                                       T* __restrict__ put, u64 n) {
    const u64 stride = (u64)gridDim.x * kPriceBlock;
    for (u64 o = (u64)blockIdx.x * kPriceBlock + threadIdx.x; o < n; o += stride) {
        I rem = (I)o, off[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < kPriceRankMax; ++q) {
            if (q >= d.rank) break;
            I coord = rem;
            if (q + 1 < d.rank) {
                const I ext = d.shape[q], next = rem / ext;
                coord = rem - next * ext;
                rem = next;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) off[k] += coord * d.stride[k][q];
        }
        double x[6], cv, pv;
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = (double)in.p[k][off[k]];
        price_pair(x[0], x[1], x[2], x[3], x[4], x[5], cv, pv);
        call[o] = (T)cv;
        put[o] = (T)pv;
    }
}

template <class I>
PriceDims<I> price_dims(const std::vector<uint64_t>& shape, const std::vector<std::vector<uint64_t>>& strides) {
    PriceDims<I> d{};
    d.rank = (int)shape.size();
    for (size_t q = 0; q < shape.size(); ++q) {
        d.shape[q] = (I)shape[q];
        for (int k = 0; k < 6; ++k) d.stride[k][q] = (I)strides[k][q];  // below the input's element count, which is at most the output's
    }
    return d;
}

template <class T>
int launch_black_scholes(Context* c, const Buffer* in, const std::vector<uint64_t>& shape, const std::vector<std::vector<uint64_t>>& strides,
                         T* call, T* put, size_t n) {
    PriceInputs<T> pi;
    for (int k = 0; k < 6; ++k) pi.p[k] = (const T*)in[k].data();
    bool flat = shape.size() == 1;
    for (int k = 0; k < 6 && flat; ++k) flat = strides[k][0] <= 1;
    if (flat) {
        unsigned scalar_mask = 0;
        bool al = aligned16(call) && aligned16(put);
        for (int k = 0; k < 6; ++k) {
            if (strides[k][0] == 0) scalar_mask |= 1u << k;
            else al = al && aligned16(pi.p[k]);
        }
        const int vec = al ? 1 : 0;
        hipLaunchKernelGGL((k_black_scholes_flat<T>), dim3(stream_grid(c, vec ? n / VecOf<T>::N : n, kPriceBlock)), dim3(kPriceBlock), 0,
                           c->stream, pi, scalar_mask, call, put, n, vec);
    } else {
        const dim3 grid(stream_grid(c, n, kPriceBlock)), block(kPriceBlock);
        if (n <= 0xffffffffull)
            hipLaunchKernelGGL((k_black_scholes_strided<T, unsigned>), grid, block, 0, c->stream, pi, price_dims<unsigned>(shape, strides), call, put, (u64)n);
        else
            hipLaunchKernelGGL((k_black_scholes_strided<T, u64>), grid, block, 0, c->stream, pi, price_dims<u64>(shape, strides), call, put, (u64)n);
    }
    c->tel.kernel_launches++;
    RMHIP_HIP_CHECK(hipGetLastError());
    return RMHIP_OK;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// `n` operands (an id of 0: absent, left untouched) either all as plain f32 storage - a precision-32 context whose operands are all
// stored that way - or all as f64 (widened copies where needed)
int fetch_operands(Context* c, const rmhip_buf* ids, size_t n, Buffer* out, bool* f32) {
    *f32 = c->precision == 32;
    for (size_t k = 0; k < n && *f32; ++k)
        if (ids[k]) RMHIP_TRY(get_operand(c, ids[k], &out[k], f32));
    if (!*f32)
        for (size_t k = 0; k < n; ++k)
            if (ids[k]) RMHIP_TRY(c->get(ids[k], &out[k]));
    return RMHIP_OK;
}

// the context's verdict word, reset on the stream ahead of the launch that may lower it
int reset_verdict(Context* c) {
    if (!c->verdict_word) RMHIP_HIP_CHECK(hipMalloc((void**)&c->verdict_word, sizeof(unsigned)));
    RMHIP_HIP_CHECK(hipMemsetAsync(c->verdict_word, 0xff, sizeof(unsigned), c->stream));
    return RMHIP_OK;
}

// the one stream synchronisation of a validated call
int read_verdict(Context* c, unsigned* code) {
    RMHIP_HIP_CHECK(hipMemcpyAsync(code, c->verdict_word, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return RMHIP_OK;
}

bool checked_product(const size_t* shape, size_t rank, size_t* out) {
    size_t n = 1;
    for (size_t d = 0; d < rank; ++d)
        if (__builtin_mul_overflow(n, shape[d], &n)) return false;
    *out = n;
    return true;
}

}  // namespace
}  // namespace rmhip

int rmhip_black_scholes_price(rmhip_ctx* ctx, const rmhip_buf inputs[6], const size_t* input_shapes, const size_t* input_strides,
                              const size_t* output_shape, size_t rank, size_t len, rmhip_buf* call, rmhip_buf* put) {
    CTX_OR_FAIL(ctx);
    if (!inputs || !call || !put || (rank && (!input_shapes || !input_strides || !output_shape)))
        return fail(RMHIP_ERR_INVALID, "black_scholes_price: null argument");
    *call = *put = 0;
    size_t expected = 0;
    if (!checked_product(output_shape, rank, &expected)) return fail(RMHIP_ERR_INVALID, "black_scholes_price: output size exceeds provider limits");
    if (expected != len) return fail(RMHIP_ERR_INVALID, "black_scholes_price: output length does not match shape");
    // per input: storage, element count, extents (1 or the output's), and the furthest element the strides can reach
    std::vector<std::vector<uint64_t>> strides(6, std::vector<uint64_t>(rank, 0));
    for (int k = 0; k < 6; ++k) {
        Buffer raw;
        RMHIP_TRY(c->lookup(inputs[k], &raw));
        if (raw.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "black_scholes_price: complex input %d is not supported", k + 1);
        const size_t* shape = input_shapes + (size_t)k * rank;
        const size_t* stride = input_strides + (size_t)k * rank;
        size_t count = 0;
        if (!checked_product(shape, rank, &count) || count != raw.numel)
            return fail(RMHIP_ERR_INVALID, "black_scholes_price: input %d shape does not match buffer length", k + 1);
        size_t reach = 0;
        for (size_t d = 0; d < rank; ++d) {
            if (shape[d] != 1 && shape[d] != output_shape[d])
                return fail(RMHIP_ERR_INVALID, "black_scholes_price: input %d does not broadcast to the output shape (dimension %zu: %zu vs %zu)",
                            k + 1, d + 1, shape[d], output_shape[d]);
            if (shape[d] <= 1) continue;  // extent 1 maps to offset 0 whatever its stride
            size_t span = 0;
            if (__builtin_mul_overflow(shape[d] - 1, stride[d], &span) || __builtin_add_overflow(reach, span, &reach))
                return fail(RMHIP_ERR_INVALID, "black_scholes_price: broadcast offset overflow");
            strides[k][d] = stride[d];
        }
        if (len && reach >= raw.numel) return fail(RMHIP_ERR_INVALID, "black_scholes_price: input %d strides reach beyond its buffer", k + 1);
    }
    std::vector<uint64_t> oshape(output_shape, output_shape + rank);
    if (len) {
        collapse(&oshape, &strides);
        if (oshape.size() > (size_t)kPriceRankMax)
            return fail(RMHIP_ERR_INVALID, "black_scholes_price: broadcast rank %zu > %d after collapsing", oshape.size(), kPriceRankMax);
    }
    Buffer in[6], cb, pb;
    bool f32 = false;
    RMHIP_TRY(fetch_operands(c, inputs, 6, in, &f32));
    if (f32) RMHIP_TRY(c->new_buffer_f32(output_shape, rank, call, &cb));
    else RMHIP_TRY(c->new_buffer(output_shape, rank, call, &cb));
    int rc = f32 ? c->new_buffer_f32(output_shape, rank, put, &pb) : c->new_buffer(output_shape, rank, put, &pb);
    if (rc == RMHIP_OK && len)
        rc = f32 ? launch_black_scholes<float>(c, in, oshape, strides, cb.data_f32(), pb.data_f32(), len)
                 : launch_black_scholes<double>(c, in, oshape, strides, cb.data(), pb.data(), len);
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *call);
        if (*put) rmhip_free(ctx, *put);
        *call = *put = 0;
    }
    return rc;
}

int rmhip_adam_update(rmhip_ctx* ctx, rmhip_buf parameters, rmhip_buf gradient, rmhip_buf average_grad_or_0, rmhip_buf average_sq_grad_or_0,
                      unsigned long long iteration, double learn_rate, double gradient_decay, double sq_gradient_decay, double epsilon,
                      rmhip_buf out3[3]) {
    CTX_OR_FAIL(ctx);
    if (!out3) return fail(RMHIP_ERR_INVALID, "adam_update: null out3");
    out3[0] = out3[1] = out3[2] = 0;
    // simple_provider.rs:992-1013, then :2926-2988
    if (iteration == 0) return fail(RMHIP_ERR_INVALID, "adam_update: iteration must be positive");
    if (!(learn_rate > 0.0 && std::isfinite(learn_rate))) return fail(RMHIP_ERR_INVALID, "adam_update: learnRate must be positive and finite");
    if (!(gradient_decay >= 0.0 && gradient_decay < 1.0)) return fail(RMHIP_ERR_INVALID, "adam_update: gradient decay factor must be in [0, 1)");
    if (!(sq_gradient_decay >= 0.0 && sq_gradient_decay < 1.0))
        return fail(RMHIP_ERR_INVALID, "adam_update: squared gradient decay factor must be in [0, 1)");
    if (!(epsilon > 0.0 && std::isfinite(epsilon))) return fail(RMHIP_ERR_INVALID, "adam_update: epsilon must be positive and finite");
    const rmhip_buf ids[4] = {parameters, gradient, average_grad_or_0, average_sq_grad_or_0};
    Buffer raw[4];
    for (int k = 0; k < 4; ++k)
        if (ids[k] || k < 2) RMHIP_TRY(c->lookup(ids[k], &raw[k]));
    if (raw[0].numel == 0) return fail(RMHIP_ERR_INVALID, "adam_update: parameters must not be empty");
    for (int k = 1; k < 4; ++k)
        if (ids[k] && raw[k].shape != raw[0].shape) return fail(RMHIP_ERR_INVALID, "adam_update: optimizer tensors must match parameter shape");
    for (int k = 0; k < 4; ++k)
        if (ids[k] && raw[k].cplx) return fail(RMHIP_ERR_UNSUPPORTED, "adam_update: complex optimizer tensors are not supported");
    AdamScalars a;
    a.b1 = gradient_decay;
    a.one_minus_b1 = 1.0 - gradient_decay;
    a.b2 = sq_gradient_decay;
    a.one_minus_b2 = 1.0 - sq_gradient_decay;
    a.learn_rate = learn_rate;
    a.grad_correction = 1.0 - std::pow(gradient_decay, (double)iteration);
    a.sq_grad_correction = 1.0 - std::pow(sq_gradient_decay, (double)iteration);
    a.epsilon = epsilon;
    if (!(a.grad_correction > 0.0 && a.sq_grad_correction > 0.0))
        return fail(RMHIP_ERR_INVALID, "adam_update: decay factors and iteration produced invalid bias correction");
    Buffer in[4], ob[3];
    bool f32 = false;
    RMHIP_TRY(fetch_operands(c, ids, 4, in, &f32));
    const std::vector<size_t>& shape = raw[0].shape;
    int rc = RMHIP_OK;
    for (int k = 0; k < 3 && rc == RMHIP_OK; ++k)
        rc = f32 ? c->new_buffer_f32(shape.data(), shape.size(), &out3[k], &ob[k]) : c->new_buffer(shape.data(), shape.size(), &out3[k], &ob[k]);
    if (rc == RMHIP_OK) rc = reset_verdict(c);
    if (rc == RMHIP_OK)
        rc = f32 ? launch_adam<float>(c, in[0].data_f32(), in[1].data_f32(), in[2].data_f32(), in[3].data_f32(), ob[0].data_f32(), ob[1].data_f32(),
                                      ob[2].data_f32(), in[0].numel, a, c->verdict_word)
                 : launch_adam<double>(c, in[0].data(), in[1].data(), in[2].data(), in[3].data(), ob[0].data(), ob[1].data(), ob[2].data(),
                                       in[0].numel, a, c->verdict_word);
    unsigned code = kVerdictNone;
    if (rc == RMHIP_OK) rc = read_verdict(c, &code);
    if (rc == RMHIP_OK && code == kAdamBadInput) rc = fail(RMHIP_ERR_INVALID, "adam_update: inputs must contain finite values");
    else if (rc == RMHIP_OK && code != kVerdictNone) rc = fail(RMHIP_ERR_INVALID, "adam_update: update produced a non-finite value");
    if (rc != RMHIP_OK)
        for (int k = 0; k < 3; ++k) {
            if (out3[k]) rmhip_free(ctx, out3[k]);
            out3[k] = 0;
        }
    return rc;
}

int rmhip_crossentropy_terms(rmhip_ctx* ctx, rmhip_buf predictions, rmhip_buf targets, rmhip_buf weights_or_0, rmhip_buf mask_or_0,
                             int multi_label, rmhip_buf* losses) {
    CTX_OR_FAIL(ctx);
    if (!losses) return fail(RMHIP_ERR_INVALID, "crossentropy_terms: null losses");
    *losses = 0;
    const rmhip_buf ids[4] = {predictions, targets, weights_or_0, mask_or_0};
    Buffer raw[4];
    for (int k = 0; k < 4; ++k)
        if (ids[k] || k < 2) RMHIP_TRY(c->lookup(ids[k], &raw[k]));
    // simple_provider.rs:3015-3041
    if (raw[0].numel == 0) return fail(RMHIP_ERR_INVALID, "crossentropy_terms: predictions must not be empty");
    if (raw[1].shape != raw[0].shape) return fail(RMHIP_ERR_INVALID, "crossentropy_terms: targets must match prediction shape");
    for (int k = 2; k < 4; ++k)
        if (ids[k] && raw[k].shape != raw[0].shape) return fail(RMHIP_ERR_INVALID, "crossentropy_terms: weights and mask must match prediction shape");
    for (int k = 0; k < 4; ++k)
        if (ids[k] && raw[k].cplx) return fail(RMHIP_ERR_UNSUPPORTED, "crossentropy_terms: complex inputs are not supported");
    Buffer in[4], ob;
    bool f32 = false;
    RMHIP_TRY(fetch_operands(c, ids, 4, in, &f32));
    const std::vector<size_t>& shape = raw[0].shape;
    if (f32) RMHIP_TRY(c->new_buffer_f32(shape.data(), shape.size(), losses, &ob));
    else RMHIP_TRY(c->new_buffer(shape.data(), shape.size(), losses, &ob));
    int rc = reset_verdict(c);
    if (rc == RMHIP_OK)
        rc = f32 ? launch_crossentropy<float>(c, multi_label != 0, in[0].data_f32(), in[1].data_f32(), in[2].data_f32(), in[3].data_f32(),
                                              ob.data_f32(), in[0].numel, c->verdict_word)
                 : launch_crossentropy<double>(c, multi_label != 0, in[0].data(), in[1].data(), in[2].data(), in[3].data(), ob.data(),
                                               in[0].numel, c->verdict_word);
    unsigned code = kVerdictNone;
    if (rc == RMHIP_OK) rc = read_verdict(c, &code);
    if (rc == RMHIP_OK && code != kVerdictNone) {
        static const char* const kMessage[5] = {"crossentropy_terms: inputs must contain finite values",
                                                "crossentropy_terms: weights must contain finite nonnegative values",
                                                "crossentropy_terms: mask must contain binary 0 or 1 values",
                                                "crossentropy_terms: targets must be probabilities in the range [0, 1]",
                                                "crossentropy_terms: loss produced a non-finite value"};
        rc = fail(RMHIP_ERR_INVALID, "%s", kMessage[code < 5 ? code : 4]);
    }
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *losses);
        *losses = 0;
    }
    return rc;
}
