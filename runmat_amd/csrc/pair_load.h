// pair_load.h -- two adjacent elements of a plain tensor in one non-temporal load, widened to f64: 16 bytes of f64 storage, 8 bytes
// of f32 (a precision-32 provider; widening in registers is exact and order preserving).  For the 16-byte forms of the reduction
// kernels (reduce_kernels.hip, reduce2.hip).
#pragma once

typedef double rm_rv2 __attribute__((ext_vector_type(2)));  // (skel_reduce.h's own typedef: the same type)

template <class T>
struct RmPair;
template <>
struct RmPair<double> {
    typedef double v2 __attribute__((ext_vector_type(2)));
    typedef v2 v2u __attribute__((aligned(8)));
};
template <>
struct RmPair<float> {
    typedef float v2 __attribute__((ext_vector_type(2)));
    typedef v2 v2u __attribute__((aligned(4)));
};
// The pair that starts at element pointer p.  ALIGNED: p is a multiple of the pair's size; otherwise it is only element-aligned (odd
// extents: every other line starts half a pair off) and the hardware splits the loads that straddle.
template <bool ALIGNED, class T>
__device__ __forceinline__ rm_rv2 rm_load_pair(const T* p) {
    typedef typename RmPair<T>::v2 V;
    typedef typename RmPair<T>::v2u VU;
    V v;
    if constexpr (ALIGNED) v = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
    else v = (V)__builtin_nontemporal_load(reinterpret_cast<const VU*>(p));
    return rm_rv2{(double)v.x, (double)v.y};
}
// Pair number i2 of a tensor whose base is pair-aligned.
template <class T>
__device__ __forceinline__ rm_rv2 rm_load_pair(const T* x, unsigned long long i2) {
    return rm_load_pair<true>(reinterpret_cast<const T*>(reinterpret_cast<const typename RmPair<T>::v2*>(x) + i2));
}
