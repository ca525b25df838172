// Wave and workgroup folds for every kernel outside the FFT engine.  Device-only and self-contained.  The ORDER of each fold is
// part of the project's results (float64 tests, bit-identity between kernel paths, reproducible partials), so it is a contract
// (DESIGN.md "Reductions and their order"; tests/test_gpu_reduce_orders.py holds this header to the lines below):
//
//   wave_reduce     xor butterfly over the 64 lanes: for d = 32, 16, 8, 4, 2, 1: v = op(v, v of lane ^ d); every lane returns the same bits
//   wave_totals     wave_reduce, lane 0 of wave w writes red[w], barrier
//   block_reduce    wave_totals, then thread 0 folds left to right: op(op(op(red[0], red[1]), red[2]), ...); valid on thread 0
//   block_reduce_n  N values at once: wave_reduce each, red[w * N + k], barrier, thread k < N folds column k left to right over
//                   the waves into out[k], barrier
//   tree_reduce     red[t] = v, barrier, for o = NT/2, NT/4, ..., 1: threads t < o do red[t] = op(red[t], red[t + o]), barrier;
//                   the result is red[0], returned to every thread
//
// The caller declares the LDS and starts every thread from the op's identity (0, +-inf, {-inf, n}); a thread with no data holds it.
// Several values are reduced by one call per value.  block_reduce and tree_reduce read red after their last barrier: a caller
// that writes red again (a loop over items, a second fold into the same array) passes REUSE = true for a trailing barrier.
#pragma once

#include <hip/hip_runtime.h>

namespace bh {

// ------------------------------------------------------------------------------------------------------------------- ops
struct op_sum {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
// floating point: fmin / fmax semantics, a NaN operand is ignored; integers: plain comparison
struct op_min {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct op_max {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? b : a; }
};

// a value and its flat index; np.argmax semantics under first_max: the larger value wins, on equal values the smaller index
template <typename V>
struct ValIdx {
    V v;
    long long i;
};
template <typename V>
struct first_max {
    __device__ __forceinline__ ValIdx<V> operator()(ValIdx<V> a, ValIdx<V> b) const { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
};

// ----------------------------------------------------------------------------------------------------------------- folds
template <typename T>
__device__ __forceinline__ T lane_xor(T v, int d) { return __shfl_xor(v, d); }
template <typename V>
__device__ __forceinline__ ValIdx<V> lane_xor(ValIdx<V> p, int d) { return ValIdx<V>{__shfl_xor(p.v, d), __shfl_xor(p.i, d)}; }

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, lane_xor(v, d));
    return v;
}

template <int NW, typename T, typename Op>
__device__ __forceinline__ void wave_totals(T v, Op op, T (&red)[NW]) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
}

template <int NW, bool REUSE = false, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T (&red)[NW]) {
    wave_totals<NW>(v, op, red);
    if (threadIdx.x == 0) {
        v = red[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v = op(v, red[w]);
    }
    if (REUSE) __syncthreads();
    return v;
}

// red holds NW * N values; out may be LDS (the trailing barrier publishes it) or global memory
template <int NW, int N, typename T, typename Op>
__device__ __forceinline__ void block_reduce_n(const T (&a)[N], Op op, T* red, T* out) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T v = wave_reduce(a[k], op);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * N + k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        T s = red[threadIdx.x];
        for (int w = 1; w < NW; ++w) s = op(s, red[w * N + threadIdx.x]);
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

template <int NT, bool REUSE = false, typename T, typename Op>
__device__ __forceinline__ T tree_reduce(T v, Op op, T (&red)[NT]) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = op(red[t], red[t + o]);
        __syncthreads();
    }
    const T r = red[0];
    if (REUSE) __syncthreads();
    return r;
}

}  // namespace bh
