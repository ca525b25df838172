// Per-slice moments of a volume in one pass: the reduction under estimate-bleaching's np.mean / np.std
// (biahub/estimate_bleaching.py:42-46) and under get_empty_frame_indices (biahub/utils/array_ops.py:79-102).
//
//   moments_items_kernel   one workgroup per item = (slice z, block of `rows` consecutive rows), capped grid and grid-stride loop
//                          over the items; wave w of the workgroup takes rows w, w + 4, ... of the block, lanes along x.
//                          part[z * nblk + b] = the item's counts, min, max and the two sums
//   moments_slices_kernel  one workgroup per slice: its nblk items in a fixed order -> one bh_moments record
//
// An item is a piece of the DATA, not of the launch: which workgroup computes it changes nothing about what is added to what,
// so the float64 sums of a float32 volume are the same bits on any number of compute units, and there are no floating-point
// atomics.  Within an item every lane adds its own elements in x order, the 64 lanes combine in a butterfly, the four waves in
// order.  Which lane owns an element depends on the row's offset from a 16-byte boundary (below), so the bits belong to a view,
// not to its values alone.
//
// Rows are read with 16-byte loads at the source's own alignment: up to V - 1 head elements bring the address to a multiple of
// 16 bytes (V = 16 / sizeof(T) elements per vector), up to V - 1 tail elements finish the row, so a view that starts at an odd
// element or whose row stride is no multiple of V reads its own elements only.
//
// Integer dtypes are exact.  The vector body sums into 32-bit lane partials and flushes them into 64 bits after at most
// MOM_FLUSH vectors: 2048 vectors of 8 uint16 hold less than 2^30, of 16 uint8 less than 2^23, and the uint8 squares (at most
// 65025 each) less than 2^32.  16-bit squares go straight into 64 bits (a 32 x 32 + 64 multiply-add).  With Z Y X <= 2^32 voxels
// the sum of squares of 16-bit data stays below 2^64 (int16: 2^32 * 2^30; uint16: 2^32 * (2^16 - 1)^2 < 2^64).
#include <climits>
#include <cmath>
#include <type_traits>

#include "common.hpp"

namespace bh {

constexpr int MOM_NT = 256, MOM_WAVES = MOM_NT / 64;
constexpr int MOM_WG_PER_CU = 8;            // the cap of the items kernel's grid (tests size their wrap cases from it)
constexpr int64_t MOM_ITEM_ELEMS = 32768;   // block_rows <= 0: rows per item = ceil(this / X), at least one row per wave
constexpr int MOM_FLUSH = 2048;             // vectors a lane sums in 32 bits before it flushes

template <typename T>
struct MomAcc {  // what the two sums are kept in
    static constexpr bool is_float = std::is_same<T, float>::value;
    using S = typename std::conditional<is_float, double, long long>::type;
    using Q = typename std::conditional<is_float, double, unsigned long long>::type;
};

template <typename T>
struct MomPart {  // one item, or one slice
    unsigned long long n_nan, n_zero;
    double mn, mx;
    typename MomAcc<T>::S s;
    typename MomAcc<T>::Q q;
};

// the wave totals of a workgroup, one array per field, and the fold of the six fields: every field by block_reduce (the 64 lanes
// in a butterfly, the four waves in order), valid on thread 0; the last call's trailing barrier lets a loop fold again
template <typename T>
struct MomRed {
    unsigned long long n_nan[MOM_WAVES], n_zero[MOM_WAVES];
    double mn[MOM_WAVES], mx[MOM_WAVES];
    typename MomAcc<T>::S s[MOM_WAVES];
    typename MomAcc<T>::Q q[MOM_WAVES];
    __device__ __forceinline__ MomPart<T> fold(MomPart<T> r) {
        r.n_nan = block_reduce<MOM_WAVES>(r.n_nan, op_sum(), n_nan);
        r.n_zero = block_reduce<MOM_WAVES>(r.n_zero, op_sum(), n_zero);
        r.mn = block_reduce<MOM_WAVES>(r.mn, op_min(), mn);
        r.mx = block_reduce<MOM_WAVES>(r.mx, op_max(), mx);
        r.s = block_reduce<MOM_WAVES>(r.s, op_sum(), s);
        r.q = block_reduce<MOM_WAVES, true>(r.q, op_sum(), q);
        return r;
    }
};

// lane-private running state of one item
template <typename T>
struct MomLane {
    using S = typename MomAcc<T>::S;
    using Q = typename MomAcc<T>::Q;
    unsigned n_nan = 0, n_zero = 0;  // an item has far fewer than 2^32 elements per lane (bh_volume_moments checks)
    float fmn = INFINITY, fmx = -INFINITY;
    int imn = INT_MAX, imx = INT_MIN;
    S s = 0;
    Q q = 0;
    int s32 = 0;        // integer dtypes: the vector body's partial sum
    unsigned q32 = 0;   // uint8: the vector body's partial sum of squares

    // one element outside the vector body (head, tail)
    __device__ __forceinline__ void scalar(T x, double centre) {
        if constexpr (MomAcc<T>::is_float) {
            body(x, centre);
        } else {
            const int v = (int)x;
            n_zero += v == 0;
            imn = min(imn, v), imx = max(imx, v);
            s += (long long)v;
            q += (unsigned long long)((long long)v * (long long)v);
        }
    }
    // one element of the vector body
    __device__ __forceinline__ void body(T x, double centre) {
        if constexpr (MomAcc<T>::is_float) {
            n_nan += x != x;
            n_zero += x == 0.0f;  // -0.0 too
            fmn = fminf(fmn, x), fmx = fmaxf(fmx, x);  // a NaN operand is ignored
            const double d = (double)x - centre;
            s += d;
            q += d * d;
        } else {
            const int v = (int)x;
            n_zero += v == 0;
            imn = min(imn, v), imx = max(imx, v);
            s32 += v;
            if constexpr (sizeof(T) == 1) q32 += (unsigned)(v * v);
            else q += (unsigned long long)((long long)v * (long long)v);
        }
    }
    __device__ __forceinline__ void flush() {
        if constexpr (!MomAcc<T>::is_float) {
            s += (long long)s32;
            s32 = 0;
            if constexpr (sizeof(T) == 1) {
                q += (unsigned long long)q32;
                q32 = 0;
            }
        }
    }
};

template <typename T>
__global__ __launch_bounds__(MOM_NT) void moments_items_kernel(const T* __restrict__ vol, int64_t plane_stride, int64_t row_stride, int Y, int X,
                                                               int rows, int nblk, int64_t nitems, double centre, MomPart<T>* __restrict__ part) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    __shared__ MomRed<T> red;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t z = item / nblk;
        const int b = (int)(item - z * nblk);
        const int64_t y0 = (int64_t)b * rows, y1 = min((int64_t)Y, y0 + rows);
        MomLane<T> a;
        for (int64_t y = y0 + wave; y < y1; y += MOM_WAVES) {
            const T* src = vol + z * plane_stride + y * row_stride;
            const int mis = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & (V - 1));
            const int head = min((V - mis) & (V - 1), X);
            const int nv = (X - head) / V;
            if (lane < head) a.scalar(src[lane], centre);
            const VT* sv = reinterpret_cast<const VT*>(src + head);
            for (int v0 = 0; v0 < nv; v0 += 64 * MOM_FLUSH) {
                const int v1 = min(nv, v0 + 64 * MOM_FLUSH);
                for (int v = v0 + lane; v < v1; v += 64) {
                    const VT p = sv[v];
#pragma unroll
                    for (int k = 0; k < V; ++k) a.body(p[k], centre);
                }
                a.flush();
            }
            const int64_t t = (int64_t)head + (int64_t)nv * V + lane;  // fewer than V <= 16 tail elements
            if (t < X) a.scalar(src[t], centre);
        }
        MomPart<T> r;
        r.n_nan = a.n_nan, r.n_zero = a.n_zero;
        if constexpr (MomAcc<T>::is_float) r.mn = (double)a.fmn, r.mx = (double)a.fmx;
        else r.mn = a.imn == INT_MAX ? (double)INFINITY : (double)a.imn, r.mx = a.imx == INT_MIN ? -(double)INFINITY : (double)a.imx;
        r.s = a.s, r.q = a.q;
        r = red.fold(r);  // its trailing barrier: red is written again by the next item
        if (threadIdx.x == 0) part[item] = r;
    }
}

// slice blockIdx.x: thread t takes items t, t + 256, ..., then the same butterfly and wave order as above
template <typename T>
__global__ __launch_bounds__(MOM_NT) void moments_slices_kernel(const MomPart<T>* __restrict__ part, int nblk, bh_moments* __restrict__ out) {
    __shared__ MomRed<T> red;
    const MomPart<T>* p = part + (int64_t)blockIdx.x * nblk;
    MomPart<T> r;
    r.n_nan = 0, r.n_zero = 0, r.mn = INFINITY, r.mx = -INFINITY, r.s = 0, r.q = 0;
    for (int i = threadIdx.x; i < nblk; i += MOM_NT) {
        const MomPart<T> v = p[i];
        r.n_nan += v.n_nan, r.n_zero += v.n_zero;
        r.mn = fmin(r.mn, v.mn), r.mx = fmax(r.mx, v.mx);
        r.s += v.s, r.q += v.q;
    }
    const MomPart<T> o = red.fold(r);
    if (threadIdx.x == 0) {
        bh_moments m;
        m.n_nan = o.n_nan, m.n_zero = o.n_zero, m.min = o.mn, m.max = o.mx;
        if constexpr (MomAcc<T>::is_float) m.isum = 0, m.isumsq = 0, m.fsum = o.s, m.fsumsq = o.q;
        else m.isum = o.s, m.isumsq = o.q, m.fsum = 0.0, m.fsumsq = 0.0;
        out[blockIdx.x] = m;
    }
}

template <typename T>
static int run_moments(bh_ctx* ctx, const void* vol, int64_t Z, int64_t Y, int64_t X, int64_t plane_stride, int64_t row_stride, double centre,
                       int rows, int nblk, bh_moments* out) {
    static_assert(sizeof(MomPart<T>) == 48, "one item's partial is six 8-byte words");
    const int64_t nitems = Z * nblk;
    MomPart<T>* part = nullptr;
    bh_moments* d_out = nullptr;
    BH_TRY(get_scratch(ctx, "moments_part", (size_t)nitems * sizeof(MomPart<T>), (void**)&part));
    BH_TRY(get_scratch(ctx, "moments_out", (size_t)Z * sizeof(bh_moments), (void**)&d_out));
    const int grid = (int)std::min<int64_t>(nitems, (int64_t)ctx->num_cus * MOM_WG_PER_CU);
    {
        ScopedTimer timer(ctx, T_MOMENTS);
        hipLaunchKernelGGL((moments_items_kernel<T>), dim3(grid), dim3(MOM_NT), 0, ctx->stream, static_cast<const T*>(vol), plane_stride, row_stride,
                           (int)Y, (int)X, rows, nblk, nitems, centre, part);
        hipLaunchKernelGGL((moments_slices_kernel<T>), dim3((unsigned)Z), dim3(MOM_NT), 0, ctx->stream, (const MomPart<T>*)part, nblk, d_out);
    }
    BH_CHECK_HIP(hipGetLastError());
    BH_CHECK_HIP(hipMemcpyAsync(out, d_out, (size_t)Z * sizeof(bh_moments), hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return BH_OK;
}

}  // namespace bh

using namespace bh;

extern "C" int bh_volume_moments_plan(int64_t Y, int64_t X, int64_t block_rows, int64_t* rows, int64_t* blocks, int* wg_per_cu) {
    BH_REQUIRE(rows && blocks, "bh_volume_moments_plan: null argument");
    BH_REQUIRE(Y >= 1 && X >= 1 && Y <= (int64_t)INT_MAX && X <= (int64_t)INT_MAX, "bh_volume_moments_plan: plane (%lld, %lld): 1 to 2**31 - 1 per axis",
               (long long)Y, (long long)X);
    int64_t r = block_rows > 0 ? block_rows : std::max<int64_t>(MOM_WAVES, ceil_div(MOM_ITEM_ELEMS, X));
    r = std::min(r, Y);
    *rows = r;
    *blocks = ceil_div(Y, r);
    if (wg_per_cu) *wg_per_cu = MOM_WG_PER_CU;
    return BH_OK;
}

extern "C" int bh_volume_moments(bh_ctx* ctx, const void* vol, int dtype, int64_t Z, int64_t Y, int64_t X, int64_t plane_stride, int64_t row_stride,
                                 double centre, int64_t block_rows, bh_moments* out) {
    static_assert(sizeof(bh_moments) == 64, "bh_moments is eight 8-byte words");
    BH_REQUIRE(ctx && vol && out, "bh_volume_moments: null argument");
    BH_REQUIRE(dtype == BH_DT_U8 || dtype == BH_DT_U16 || dtype == BH_DT_I16 || dtype == BH_DT_F32,
               "bh_volume_moments: unsupported dtype code %d (uint8, uint16, int16, float32)", dtype);
    BH_REQUIRE(Z >= 1 && Z <= (int64_t)INT_MAX, "bh_volume_moments: Z = %lld (1 to 2**31 - 1)", (long long)Z);
    int64_t rows = 0, nblk = 0;
    BH_TRY(bh_volume_moments_plan(Y, X, block_rows, &rows, &nblk, nullptr));
    BH_REQUIRE(Y * X <= ((int64_t)1 << 32) && Z * (Y * X) <= ((int64_t)1 << 32),
               "bh_volume_moments: (%lld, %lld, %lld) has more than 2**32 voxels: the exact sum of squares of 16-bit data needs Z * Y * X <= 2**32 per call",
               (long long)Z, (long long)Y, (long long)X);
    BH_REQUIRE(row_stride >= X && plane_stride >= (Y - 1) * row_stride + X,
               "bh_volume_moments: strides (%lld, %lld) are smaller than the volume's extents (%lld, %lld)", (long long)plane_stride,
               (long long)row_stride, (long long)Y, (long long)X);
    const size_t esize = dtype == BH_DT_U8 ? 1 : (dtype == BH_DT_F32 ? 4 : 2);
    BH_REQUIRE(reinterpret_cast<uintptr_t>(vol) % esize == 0, "bh_volume_moments: the volume's address is not a multiple of its element size");
    BH_REQUIRE(Z * nblk <= (int64_t)INT_MAX, "bh_volume_moments: %lld slices of %lld row blocks are too many items", (long long)Z, (long long)nblk);
    BH_REQUIRE(std::isfinite(centre), "bh_volume_moments: centre must be finite");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    switch (dtype) {
        case BH_DT_U8: return run_moments<uint8_t>(ctx, vol, Z, Y, X, plane_stride, row_stride, centre, (int)rows, (int)nblk, out);
        case BH_DT_U16: return run_moments<uint16_t>(ctx, vol, Z, Y, X, plane_stride, row_stride, centre, (int)rows, (int)nblk, out);
        case BH_DT_I16: return run_moments<int16_t>(ctx, vol, Z, Y, X, plane_stride, row_stride, centre, (int)rows, (int)nblk, out);
        default: return run_moments<float>(ctx, vol, Z, Y, X, plane_stride, row_stride, centre, (int)rows, (int)nblk, out);
    }
}
