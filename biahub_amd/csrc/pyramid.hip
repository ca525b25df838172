// Multiscale pyramid levels (biahub/pyramid.py: iohub's Position.compute_pyramid): level k of a (Z, Y, X) volume has extents
// n_k = ceil(n_{k-1} / 2) and voxel (z, y, x) reduces the block [2z, min(2z + 2, n)) x [2y, ...) x [2x, ...) of level k-1 AS
// STORED (rounded to the dtype): 1, 2, 4 or 8 elements, partial blocks at the upper edges unpadded.  Methods:
// stride (the block's first element), mean (integers: exact sum, quotient rounded to nearest, ties to even, the sum of uint32
// held in 64 bits; float32 and float16: float64 sum in (z, y, x) order, one rounding from float64 to the dtype), min, max, median
// (the lower one: sorted[(count - 1) / 2]), mode (most frequent, smallest among ties).  float16 compares as float32 does.
//
// One launch reads its source level once and writes the next D <= 3 levels.  A thread owns an aligned source box of
// 2^D (z) x 2^D (y) x E (x) voxels, E = max(2^D, 16 B / element): the cascade nests because ceil nests, so every block of every
// level it writes lies inside the box.  It walks the box's rows recursively: a level-k row of E >> k voxels is reduced from the
// four level-(k-1) rows under it, stored, and handed up; at most 4 rows per level are live.  A workgroup is 4 boxes along y by
// 64 along x, so a wave reads 64 * E contiguous elements per row.  Boxes wholly inside the source skip every per-voxel test;
// rows whose byte offsets are not multiples of the access width go element by element (a per-level, launch-uniform flag).
#include <type_traits>

#include "common.hpp"

namespace bh {

enum { DS_STRIDE = BH_DS_STRIDE, DS_MEAN = BH_DS_MEAN, DS_MIN = BH_DS_MIN, DS_MAX = BH_DS_MAX, DS_MEDIAN = BH_DS_MEDIAN,
       DS_MODE = BH_DS_MODE };

struct PyrArgs {
    const void* in;
    void* out[3];
    int64_t Z[4], Y[4], X[4];  // extents of levels 0 (the source) .. D of this launch
    int64_t tx, ty, tz;        // tiles along x, y, z
    int vec;                   // bit k: rows of level k may be accessed with vector loads / stores
};

template <typename T>
struct Lim;
template <> struct Lim<uint8_t> { __device__ static uint8_t hi() { return 0xFF; } };
template <> struct Lim<uint16_t> { __device__ static uint16_t hi() { return 0xFFFF; } };
template <> struct Lim<int16_t> { __device__ static int16_t hi() { return 0x7FFF; } };
template <> struct Lim<float> { __device__ static float hi() { return INFINITY; } };
template <> struct Lim<_Float16> { __device__ static _Float16 hi() { return (_Float16)INFINITY; } };
template <> struct Lim<uint32_t> { __device__ static uint32_t hi() { return 0xFFFFFFFFu; } };

template <typename T>
constexpr bool is_floating = std::is_same<T, float>::value || std::is_same<T, _Float16>::value;

// N elements at p: 16-, 8-, 4- or 2-byte accesses when `vec` (the row offset is a multiple of min(N * sizeof(T), 16) bytes),
// element by element otherwise
template <typename T, int N>
__device__ __forceinline__ void load_row(const T* __restrict__ p, T (&v)[N], bool vec) {
    constexpr int B = N * (int)sizeof(T);
    if (vec && B >= 2) {
        if constexpr (B >= 16) {
#pragma unroll
            for (int i = 0; i < B / 16; ++i) {
                const uint4 w = reinterpret_cast<const uint4*>(p)[i];
                __builtin_memcpy(&v[i * (16 / (int)sizeof(T))], &w, 16);
            }
        } else if constexpr (B == 8) {
            const uint2 w = *reinterpret_cast<const uint2*>(p);
            __builtin_memcpy(v, &w, 8);
        } else if constexpr (B == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
            __builtin_memcpy(v, &w, 4);
        } else if constexpr (B == 2) {
            const uint16_t w = *reinterpret_cast<const uint16_t*>(p);
            __builtin_memcpy(v, &w, 2);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[i];
}

template <typename T, int N>
__device__ __forceinline__ void store_row(T* __restrict__ p, const T (&v)[N], bool vec) {
    constexpr int B = N * (int)sizeof(T);
    if (vec && B >= 2) {
        if constexpr (B >= 16) {
#pragma unroll
            for (int i = 0; i < B / 16; ++i) {
                uint4 w;
                __builtin_memcpy(&w, &v[i * (16 / (int)sizeof(T))], 16);
                reinterpret_cast<uint4*>(p)[i] = w;
            }
        } else if constexpr (B == 8) {
            uint2 w;
            __builtin_memcpy(&w, v, 8);
            *reinterpret_cast<uint2*>(p) = w;
        } else if constexpr (B == 4) {
            uint32_t w;
            __builtin_memcpy(&w, v, 4);
            *reinterpret_cast<uint32_t*>(p) = w;
        } else if constexpr (B == 2) {
            uint16_t w;
            __builtin_memcpy(&w, v, 2);
            *reinterpret_cast<uint16_t*>(p) = w;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = v[i];
}

template <typename T>
__device__ __forceinline__ void cswap(T& a, T& b) {
    const T lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo, b = hi;
}

// v: the block in (z, y, x) order; element i is valid iff (i >> 2) < cz && ((i >> 1) & 1) < cy && (i & 1) < cx.  A box inside
// the source passes cz = cy = cx = 2 as constants and every test folds away.  Blocks with no valid element return 0 (unstored).
template <typename T, int M>
__device__ __forceinline__ T reduce_block(const T (&v)[8], int cz, int cy, int cx) {
    bool ok[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ok[i] = (i >> 2) < cz && ((i >> 1) & 1) < cy && (i & 1) < cx;
    if constexpr (M == DS_STRIDE) {
        return v[0];
    } else if constexpr (M == DS_MIN || M == DS_MAX) {
        T r = v[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (ok[i] && (M == DS_MIN ? v[i] < r : r < v[i])) r = v[i];
        return r;
    } else if constexpr (M == DS_MEAN) {
        if (cz <= 0 || cy <= 0 || cx <= 0) return T(0);
        if constexpr (is_floating<T>) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (ok[i]) s += (double)v[i];
            const double q = s / (double)(cz * cy * cx);
            // float64 -> binary16 directly, ONE rounding: through float32, 1 + 2^-11 + 2^-27 goes to 1 + 2^-11 and then, a tie,
            // to 1, while the nearest binary16 is 1 + 2^-10.  gfx950 has no such instruction; the compiler expands the cast in
            // integer arithmetic on the float64's words (no fast-math: DESIGN.md §3.6).  For finite float16 inputs the sum and
            // the quotient (count 1, 2, 4, 8) are exact, so this is the exact mean rounded once.
            return (T)q;
        } else {
            using S = typename std::conditional<sizeof(T) == 4, int64_t, int>::type;  // eight uint32 overflow an int
            S s = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (ok[i]) s += (S)v[i];
            const int sh = (cz - 1) + (cy - 1) + (cx - 1);  // count = 2^sh
            S q = s >> sh;                                   // floor, also for negative sums
            if (sh > 0) {
                const S r = s - (q << sh), half = S(1) << (sh - 1);
                q += (r > half) | ((r == half) & (q & 1));  // to nearest, ties to even
            }
            return (T)q;
        }
    } else if constexpr (M == DS_MEDIAN) {
        T w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = ok[i] ? v[i] : Lim<T>::hi();  // invalid elements sort last
        // Batcher's odd-even merge sort of 8 (19 compare-exchanges)
        cswap(w[0], w[1]), cswap(w[2], w[3]), cswap(w[4], w[5]), cswap(w[6], w[7]);
        cswap(w[0], w[2]), cswap(w[1], w[3]), cswap(w[4], w[6]), cswap(w[5], w[7]);
        cswap(w[1], w[2]), cswap(w[5], w[6]);
        cswap(w[0], w[4]), cswap(w[1], w[5]), cswap(w[2], w[6]), cswap(w[3], w[7]);
        cswap(w[2], w[4]), cswap(w[3], w[5]);
        cswap(w[1], w[2]), cswap(w[3], w[4]), cswap(w[5], w[6]);
        const int k = (cz * cy * cx - 1) >> 1;
        T r = w[0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (k == i) r = w[i];
        return r;
    } else {  // DS_MODE: pairwise equality counts (each of the 28 pairs once), the smallest value among the most frequent
        int c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = ok[i] ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = i + 1; j < 8; ++j) {
                const int e = (ok[i] && ok[j] && v[i] == v[j]) ? 1 : 0;
                c[i] += e, c[j] += e;
            }
        T best = v[0];
        int bc = c[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (c[i] > bc || (c[i] == bc && ok[i] && v[i] < best)) best = v[i], bc = c[i];
        return best;
    }
}

// elements of a block along one axis: the level below has n - 2i of them from the block's first one on
__device__ __forceinline__ int clamp2(int64_t n) { return n >= 2 ? 2 : (n > 0 ? (int)n : 0); }

template <typename T, int M, int E, bool EDGE>
struct Walk {
    const PyrArgs& a;
    int64_t x0;  // the box's first source column

    // level-K row (zk, yk) of the box: E >> K voxels from column x0 >> K, stored (K >= 1) and returned in `out`
    template <int K>
    __device__ __forceinline__ void row(int64_t zk, int64_t yk, T (&out)[E >> K]) const {
        constexpr int N = E >> K;
        const int64_t xk = x0 >> K;
        if constexpr (K == 0) {
            const T* p = static_cast<const T*>(a.in) + (zk * a.Y[0] + yk) * a.X[0] + xk;
            if constexpr (!EDGE) {
                load_row(p, out, a.vec & 1);
            } else {
#pragma unroll
                for (int i = 0; i < N; ++i) out[i] = T(0);
                if (zk < a.Z[0] && yk < a.Y[0]) {
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        if (xk + i < a.X[0]) out[i] = p[i];
                }
            }
        } else {
            constexpr int P = E >> (K - 1);
            T r[4][P];
            row<K - 1>(2 * zk, 2 * yk, r[0]);
            row<K - 1>(2 * zk, 2 * yk + 1, r[1]);
            row<K - 1>(2 * zk + 1, 2 * yk, r[2]);
            row<K - 1>(2 * zk + 1, 2 * yk + 1, r[3]);
            int cz = 2, cy = 2;
            if constexpr (EDGE) {
                cz = clamp2(a.Z[K - 1] - 2 * zk);
                cy = clamp2(a.Y[K - 1] - 2 * yk);
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const T v[8] = {r[0][2 * j], r[0][2 * j + 1], r[1][2 * j], r[1][2 * j + 1],
                                r[2][2 * j], r[2][2 * j + 1], r[3][2 * j], r[3][2 * j + 1]};
                int cx = 2;
                if constexpr (EDGE) cx = clamp2(a.X[K - 1] - 2 * (xk + j));
                out[j] = reduce_block<T, M>(v, cz, cy, cx);
            }
            T* q = static_cast<T*>(a.out[K - 1]) + (zk * a.Y[K] + yk) * a.X[K] + xk;
            if constexpr (!EDGE) {
                store_row(q, out, (a.vec >> K) & 1);
            } else if (zk < a.Z[K] && yk < a.Y[K]) {
#pragma unroll
                for (int i = 0; i < N; ++i)
                    if (xk + i < a.X[K]) q[i] = out[i];
            }
        }
    }
};

template <typename T, int D>
constexpr int box_x() {
    return (1 << D) > 16 / (int)sizeof(T) ? (1 << D) : 16 / (int)sizeof(T);
}

template <typename T, int M, int D>
__global__ __launch_bounds__(256) void pyramid_kernel(const PyrArgs a) {
    constexpr int C = 1 << D, E = box_x<T, D>();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int64_t tiles = a.tx * a.ty * a.tz;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t bx = t % a.tx, by = (t / a.tx) % a.ty, bz = t / (a.tx * a.ty);
        const int64_t x0 = (bx * 64 + lx) * E, y0 = (by * 4 + ly) * C, z0 = bz * C;
        if (x0 >= a.X[0] || y0 >= a.Y[0]) continue;
        T top[E >> D];
        if (z0 + C <= a.Z[0] && y0 + C <= a.Y[0] && x0 + E <= a.X[0]) {
            const Walk<T, M, E, false> w{a, x0};
            w.template row<D>(z0 >> D, y0 >> D, top);
        } else {
            const Walk<T, M, E, true> w{a, x0};
            w.template row<D>(z0 >> D, y0 >> D, top);
        }
    }
}

template <typename T, int M, int D>
int launch_depth(bh_ctx* ctx, const PyrArgs& a0) {
    PyrArgs a = a0;
    constexpr int C = 1 << D, E = box_x<T, D>();
    a.tx = ceil_div(a.X[0], 64 * E), a.ty = ceil_div(a.Y[0], 4 * C), a.tz = ceil_div(a.Z[0], C);
    a.vec = 0;
    for (int k = 0; k <= D; ++k) {  // a level-k row chunk is (E >> k) elements at an element offset that is a multiple of it
        const int64_t bytes = std::min<int64_t>(16, (int64_t)(E >> k) * (int64_t)sizeof(T));
        const void* base = k == 0 ? a.in : a.out[k - 1];
        if ((a.X[k] * (int64_t)sizeof(T)) % bytes == 0 && (reinterpret_cast<uintptr_t>(base) % (uintptr_t)bytes) == 0)
            a.vec |= 1 << k;
    }
    const int64_t tiles = a.tx * a.ty * a.tz;
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)1 << 20);
    hipLaunchKernelGGL((pyramid_kernel<T, M, D>), dim3(grid), dim3(256), 0, ctx->stream, a);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

template <typename T, int M>
int launch_method(bh_ctx* ctx, const PyrArgs& a, int depth) {
    switch (depth) {
        case 1: return launch_depth<T, M, 1>(ctx, a);
        case 2: return launch_depth<T, M, 2>(ctx, a);
        default: return launch_depth<T, M, 3>(ctx, a);
    }
}

template <typename T>
int launch_dtype(bh_ctx* ctx, const PyrArgs& a, int method, int depth) {
    switch (method) {
        case DS_STRIDE: return launch_method<T, DS_STRIDE>(ctx, a, depth);
        case DS_MEAN: return launch_method<T, DS_MEAN>(ctx, a, depth);
        case DS_MIN: return launch_method<T, DS_MIN>(ctx, a, depth);
        case DS_MAX: return launch_method<T, DS_MAX>(ctx, a, depth);
        case DS_MEDIAN: return launch_method<T, DS_MEDIAN>(ctx, a, depth);
        default: return launch_method<T, DS_MODE>(ctx, a, depth);
    }
}

}  // namespace bh

using namespace bh;

extern "C" int bh_pyramid_downsample(bh_ctx* ctx, const void* in, int dtype, int64_t Z, int64_t Y, int64_t X, int method, int n,
                                     void* const* out) {
    BH_REQUIRE(dtype == BH_DT_U8 || dtype == BH_DT_U16 || dtype == BH_DT_I16 || dtype == BH_DT_F32 || dtype == BH_DT_F16 ||
                   dtype == BH_DT_U32,
               "bh_pyramid_downsample: unsupported dtype code %d (uint8, uint16, int16, float32, float16, uint32)", dtype);
    BH_REQUIRE(method >= BH_DS_STRIDE && method <= BH_DS_MODE, "bh_pyramid_downsample: unknown method code %d", method);
    BH_REQUIRE(n >= 1, "bh_pyramid_downsample: n = %d levels to write (>= 1)", n);
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0, "bh_pyramid_downsample: bad shape (%lld, %lld, %lld)", (long long)Z, (long long)Y,
               (long long)X);
    BH_REQUIRE(ctx && in && out, "bh_pyramid_downsample: null argument");
    for (int k = 0; k < n; ++k) BH_REQUIRE(out[k], "bh_pyramid_downsample: out[%d] is null", k);
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    // launches of depth 3 from the last level written, the remainder last: 4 levels = 3, 5 = 3 + 1, 7 = 3 + 3
    const void* src = in;
    int64_t z = Z, y = Y, x = X;
    for (int k = 0; k < n;) {
        const int depth = std::min(3, n - k);
        PyrArgs a{};
        a.in = src;
        a.Z[0] = z, a.Y[0] = y, a.X[0] = x;
        for (int d = 1; d <= depth; ++d) {
            a.out[d - 1] = out[k + d - 1];
            a.Z[d] = (a.Z[d - 1] + 1) / 2, a.Y[d] = (a.Y[d - 1] + 1) / 2, a.X[d] = (a.X[d - 1] + 1) / 2;
        }
        switch (dtype) {
            case BH_DT_U8: BH_TRY(launch_dtype<uint8_t>(ctx, a, method, depth)); break;
            case BH_DT_U16: BH_TRY(launch_dtype<uint16_t>(ctx, a, method, depth)); break;
            case BH_DT_I16: BH_TRY(launch_dtype<int16_t>(ctx, a, method, depth)); break;
            case BH_DT_F32: BH_TRY(launch_dtype<float>(ctx, a, method, depth)); break;
            case BH_DT_F16: BH_TRY(launch_dtype<_Float16>(ctx, a, method, depth)); break;
            case BH_DT_U32: BH_TRY(launch_dtype<uint32_t>(ctx, a, method, depth)); break;
            default: BH_REQUIRE(false, "bh_pyramid_downsample: unsupported dtype code %d", dtype);
        }
        src = a.out[depth - 1];
        z = a.Z[depth], y = a.Y[depth], x = a.X[depth];
        k += depth;
    }
    return BH_OK;
}
