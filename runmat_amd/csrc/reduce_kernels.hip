// reduce_kernels.hip -- ahead-of-time reductions: reduce_sum / reduce_sum_dim / reduce_mean(_dim) /
// reduce_min / reduce_max / reduce_prod and dot (crates/runmat-accelerate-api/src/lib.rs:2709-2722,
// 2743-2792, 2858-2883; reference semantics crates/runmat-accelerate/src/simple_provider.rs:
// 6728-6806 and the CPU sum_tensor, runtime/.../reduction/sum.rs:996-1079).
// HBM-bound: coalesced loads, per-lane f64 accumulators, wave64 __shfl_down tree, LDS across the
// four waves of a block, deterministic two-stage combine (skel_reduce.h).
#include "common.h"
#include "reduce_plan.h"
#include "skel_common.h"
#include "skel_reduce.h"
#include "pair_load.h"

namespace rmhip {

// ---- producers: what stage 1 folds.  T = storage type (double, or float for precision-32 contexts); accumulation is f64 either way.
// A producer hands the skeletons two value functors: Val (index -> f64) and Val2, the same over 16-byte vectors (1 KiB per wave
// instruction instead of 512 B, non-temporal; the pairing changes only the deterministic summation grouping) - operator() on an
// aligned pair index, pair_at / one_at on element offsets for the ODD forms and the SHORT kernel's staging load.
template <class T>
struct IdentityVal {
    const T* __restrict__ x;
    __device__ __forceinline__ double operator()(rm_u64 idx) const { return (double)x[idx]; }
};
template <class T>
struct IdentityVal2 {
    const T* __restrict__ x;
    __device__ __forceinline__ rm_rv2 operator()(rm_u64 i2) const { return rm_load_pair(x, i2); }
    __device__ __forceinline__ rm_rv2 pair_at(rm_u64 e) const { return rm_load_pair<false>(x + e); }
    __device__ __forceinline__ double one_at(rm_u64 e) const { return (double)__builtin_nontemporal_load(x + e); }
};
template <class T>
struct Identity {
    typedef T Elem;
    typedef IdentityVal<T> Val;
    typedef IdentityVal2<T> Val2;
    static constexpr ReduceFamily FAMILY = REDUCE_PLAIN;
    static constexpr const char* NAME = "reduce";
    const T* x;
    bool aligned() const { return (((uintptr_t)x) & 15) == 0; }  // also for f32
    Val val() const { return Val{x}; }
    Val2 val2() const { return Val2{x}; }
};
// dot: the producer a.*b folded into the same skeletons (no temporary array).  No unaligned-pair forms (REDUCE_DOT).
template <class T>
struct ProductVal {
    const T* __restrict__ a;
    const T* __restrict__ b;
    __device__ __forceinline__ double operator()(rm_u64 idx) const { return (double)a[idx] * (double)b[idx]; }
};
template <class T>
struct ProductVal2 {
    const T* __restrict__ a;
    const T* __restrict__ b;
    __device__ __forceinline__ rm_rv2 operator()(rm_u64 i2) const { return rm_load_pair(a, i2) * rm_load_pair(b, i2); }
    __device__ __forceinline__ double one_at(rm_u64 e) const { return (double)__builtin_nontemporal_load(a + e) * (double)__builtin_nontemporal_load(b + e); }
};
template <class T>
struct Product {
    typedef T Elem;
    typedef ProductVal<T> Val;
    typedef ProductVal2<T> Val2;
    static constexpr ReduceFamily FAMILY = REDUCE_DOT;
    static constexpr const char* NAME = "dot";
    const T* a;
    const T* b;
    bool aligned() const { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }
    Val val() const { return Val{a, b}; }
    Val2 val2() const { return Val2{a, b}; }
};

// ---- stage 1: the skeletons of skel_reduce.h over a producer's functor, as codegen.cpp's generated kernels are
template <int OP, class F>
__global__ void __launch_bounds__(RM_ABLOCK) k_reduce_contig(F f, rm_u64 red, rm_u64 nslices, rm_u64 nsplit, double* pv, double* pn) {
    rm_reduce_contig<OP>(f, red, nslices, nsplit, pv, pn);
}
template <int OP, class F2, bool ODD = false>
__global__ void __launch_bounds__(RM_ABLOCK) k_reduce_contig_v2(F2 f2, rm_u64 red, rm_u64 nslices, rm_u64 nsplit, double* pv, double* pn) {
    rm_reduce_contig_v2<OP, ODD>(f2, red, nslices, nsplit, pv, pn);
}
template <int OP, class F>
__global__ void __launch_bounds__(RM_RBLOCK) k_reduce_strided(F f, rm_u64 pre, rm_u64 red, rm_u64 nsplit, int tx, double* pv, double* pn) {
    rm_reduce_strided<OP>(f, pre, red, nsplit, tx, pv, pn);
}
template <int OP, class F2, bool ODD = false>
__global__ void __launch_bounds__(RM_RBLOCK) k_reduce_strided_v2(F2 f2, rm_u64 pre, rm_u64 red, rm_u64 nsplit, unsigned win, double* pv, double* pn) {
    rm_reduce_strided_v2<OP, 8, ODD>(f2, pre, red, nsplit, win, pv, pn);
}

// Many SHORT contiguous slices (red < 256: sum(x,1) of a 3 x N or 32 x N matrix, dot along the 32 rows of a 32 x N pair).  Kernel A
// gives every slice a block of its own - 256 threads for a few elements, half a million blocks for a 32 x 524288 matrix: 731 us where
// the bytes take 25 (dot: 580).  Here a block takes `per_block` = min(256, 4096 / red) consecutive slices - one contiguous tile of
// per_block * red elements -, stages the producer's values in LDS with coalesced loads (one pad per 32 elements: the per-thread walks
// then fall on distinct banks) and thread t folds slice t in ascending order, the CPU's own sequence.  One partial per slice; the flat
// finalize applies the NaN / mean policy.
__device__ __forceinline__ int short_pad(int i) { return i + (i >> 5); }
template <int OP, class F2>
__global__ void __launch_bounds__(RM_RBLOCK) k_reduce_short(F2 f2, rm_u64 red, rm_u64 nslices, unsigned per_block, double* pv, double* pn) {
    __shared__ double tile[REDUCE_SHORT_TILE + REDUCE_SHORT_TILE / 32 + 1];
    const rm_u64 s0 = (rm_u64)blockIdx.x * per_block;
    const rm_u64 ns = nslices - s0 < per_block ? nslices - s0 : per_block;
    const rm_u64 count = ns * red;
    for (rm_u64 i = threadIdx.x; i < count; i += RM_RBLOCK) tile[short_pad((int)i)] = f2.one_at(s0 * red + i);
    __syncthreads();
    if (threadIdx.x >= ns) return;
    RmAcc a = rm_acc_init<OP>();
    const int b = (int)(threadIdx.x * red);
    for (int r = 0; r < (int)red; ++r) rm_acc_add<OP>(a, tile[short_pad(b + r)]);
    pv[s0 + threadIdx.x] = a.v;
    pn[s0 + threadIdx.x] = a.nan;
}

template <int OP>
__global__ void __launch_bounds__(RM_RBLOCK) k_reduce_final(const double* pv, const double* pn, rm_u64 nslices,
                                                            rm_u64 nsplit, rm_u64 red, int mean, int omitnan,
                                                            double scale, double* out) {
    rm_reduce_finalize<OP>(pv, pn, nslices, nsplit, red, mean, omitnan, scale, out);
}
template <int OP>
__global__ void __launch_bounds__(RM_RBLOCK) k_reduce_final_flat(const double* pv, const double* pn, rm_u64 nslices, rm_u64 nsplit, rm_u64 red,
                                                                 int mean, int omitnan, double scale, double* out) {
    rm_reduce_finalize_flat<OP>(pv, pn, nslices, nsplit, red, mean, omitnan, scale, out);
}

static int no_kernel(const char* what, ReduceKernel k) { return fail(RMHIP_ERR_UNSUPPORTED, "%s: no kernel for route %s", what, reduce_kernel_name(k)); }

// P: Identity<T> or Product<T>
template <int OP, class P>
static int run_reduce(Context* c, int mean, int nan_mode, const P& src, size_t pre, size_t red, size_t post, double* out) {
    if (pre == 0 || post == 0) return RMHIP_OK;  // no output slices
    // which kernel on which grid, how many partials per slice, which finalize: reduce_plan.h route_reduction
    const ReduceRoute rt = route_reduction(pre, red, post, c->num_cus, c->num_xcc, (unsigned)sizeof(typename P::Elem), src.aligned(), P::FAMILY);
    if (!rt.valid) return fail(RMHIP_ERR_UNSUPPORTED, "%s: geometry [%zu,%zu,%zu] exceeds launch limits", P::NAME, pre, red, post);
    typedef typename P::Val F;
    typedef typename P::Val2 F2;
    const rm_u64 nslices = rt.nslices, nsplit = rt.nsplit;
    const size_t nparts = (size_t)(nslices * nsplit);
    RMHIP_TRY(c->ensure_scratch(2 * nparts * sizeof(double)));
    double* pv = c->scratch;
    double* pn = c->scratch + nparts;
    const dim3 grid(rt.gx, rt.gy, rt.gz), block(rt.block);
    switch (rt.kernel) {
        case ReduceKernel::SHORT:
            hipLaunchKernelGGL((k_reduce_short<OP, F2>), grid, block, 0, c->stream, src.val2(), (rm_u64)red, nslices, rt.span, pv, pn);
            break;
        case ReduceKernel::CONTIG:
            hipLaunchKernelGGL((k_reduce_contig<OP, F>), grid, block, 0, c->stream, src.val(), (rm_u64)red, nslices, nsplit, pv, pn);
            break;
        case ReduceKernel::CONTIG_V2:
            hipLaunchKernelGGL((k_reduce_contig_v2<OP, F2>), grid, block, 0, c->stream, src.val2(), (rm_u64)red, nslices, nsplit, pv, pn);
            break;
        case ReduceKernel::CONTIG_V2_ODD:
            if constexpr (P::FAMILY.odd_pairs)
                hipLaunchKernelGGL((k_reduce_contig_v2<OP, F2, true>), grid, block, 0, c->stream, src.val2(), (rm_u64)red, nslices, nsplit, pv, pn);
            else
                return no_kernel(P::NAME, rt.kernel);
            break;
        case ReduceKernel::STRIDED:
            hipLaunchKernelGGL((k_reduce_strided<OP, F>), grid, block, 0, c->stream, src.val(), (rm_u64)pre, (rm_u64)red, nsplit, (int)rt.span, pv, pn);
            break;
        case ReduceKernel::STRIDED_V2:
            if constexpr (P::FAMILY.wide_b)
                hipLaunchKernelGGL((k_reduce_strided_v2<OP, F2>), grid, block, 0, c->stream, src.val2(), (rm_u64)pre, (rm_u64)red, nsplit, rt.span, pv, pn);
            else
                return no_kernel(P::NAME, rt.kernel);
            break;
        case ReduceKernel::STRIDED_V2_ODD:
            if constexpr (P::FAMILY.wide_b && P::FAMILY.odd_pairs)
                hipLaunchKernelGGL((k_reduce_strided_v2<OP, F2, true>), grid, block, 0, c->stream, src.val2(), (rm_u64)pre, (rm_u64)red, nsplit, rt.span, pv, pn);
            else
                return no_kernel(P::NAME, rt.kernel);
            break;
    }
    RMHIP_HIP_CHECK(hipGetLastError());
    if (rt.flat_final) {  // many slices, a handful of partials each: one thread per slice
        hipLaunchKernelGGL((k_reduce_final_flat<OP>), dim3((unsigned)ceil_div_u64(nslices, RM_RBLOCK)), dim3(RM_RBLOCK), 0, c->stream, pv, pn, nslices,
                           nsplit, (rm_u64)red, mean, nan_mode, 1.0, out);
    } else {
        const unsigned fb = (unsigned)ceil_div_u64(nslices, RM_RBLOCK / 64);
        hipLaunchKernelGGL((k_reduce_final<OP>), dim3(fb), dim3(RM_RBLOCK), 0, c->stream, pv, pn, nslices, nsplit, (rm_u64)red, mean, nan_mode, 1.0,
                           out);
    }
    RMHIP_HIP_CHECK(hipGetLastError());
    c->tel.kernel_launches += 2;
    return RMHIP_OK;
}

template <class T>
static int reduce_mid_any(Context* c, int op, int nan_mode, const T* x, size_t pre, size_t red, size_t post, double* out) {
    const Identity<T> src{x};
    switch (op) {
        case RMHIP_RSUM: return run_reduce<RM_RSUM>(c, 0, nan_mode, src, pre, red, post, out);
        case RMHIP_RMEAN: return run_reduce<RM_RSUM>(c, 1, nan_mode, src, pre, red, post, out);
        case RMHIP_RMIN: return run_reduce<RM_RMIN>(c, 0, nan_mode, src, pre, red, post, out);
        case RMHIP_RMAX: return run_reduce<RM_RMAX>(c, 0, nan_mode, src, pre, red, post, out);
        case RMHIP_RPROD: return run_reduce<RM_RPROD>(c, 0, nan_mode, src, pre, red, post, out);
        default: return fail(RMHIP_ERR_UNSUPPORTED, "reduce op %d not supported by provider", op);
    }
}
int launch_reduce_mid(Context* c, int op, int nan_mode, const double* x, size_t pre, size_t red, size_t post,
                      double* out) {
    return reduce_mid_any(c, op, nan_mode, x, pre, red, post, out);
}
int launch_reduce_mid_f32(Context* c, int op, int nan_mode, const float* x, size_t pre, size_t red, size_t post,
                          double* out) {
    return reduce_mid_any(c, op, nan_mode, x, pre, red, post, out);
}
int launch_reduce_dot(Context* c, const double* a, const double* b, size_t pre, size_t red, size_t post, double* out) {
    return run_reduce<RM_RSUM>(c, 0, 0, Product<double>{a, b}, pre, red, post, out);
}
int launch_reduce_dot_f32(Context* c, const float* a, const float* b, size_t pre, size_t red, size_t post, double* out) {
    return run_reduce<RM_RSUM>(c, 0, 0, Product<float>{a, b}, pre, red, post, out);
}

int launch_reduce_all(Context* c, int op, int nan_mode, const double* x, size_t n, double* out) {
    return launch_reduce_mid(c, op, nan_mode, x, 1, n, 1, out);
}

}  // namespace rmhip
