// Stitch blend (biahub/stitch.py:196-311 write_output_chunk, one chunk per mosaic): the FOVs of a well, all of
// one shape (Z, Y, X), are placed at integer offsets in a mosaic and blended with weights that fall off towards each FOV's
// (y, x) border:
//     out[o] = sum_i x_i[o] * w_i[o] / (sum_i w_i[o] + 1e-8),  w = wtab[d],  d = min(y, Y-1-y, x, X-1-x) in the FOV's own frame,
// over the FOVs covering o in list order; wtab[0] = 0, wtab[d] = d ** exponent (float64 pow on the host, rounded to float32).
// Per voxel, in float32: acc = fma(x_i, w_i, acc) and sw += w_i FOV by FOV, then one correctly rounded division.  The order of
// operations of a voxel does not depend on the region a launch writes, so any split into regions gives the same bits.
//
// One launch writes a (RZ, RY, RX) box of the mosaic.  The box's (y, x) plane is cut into tiles of ST_TY x ST_TX; the host lists,
// per tile, the FOVs whose footprint meets it (CSR: tile_off, tile_fov; FOV order kept) and stages those lists, the FOV pointers
// and offsets and the weight table into the context workspace with one copy.  A workgroup takes one tile and ST_ZC planes; each
// wave takes a row at a time, each lane ST_V consecutive x of it, and walks the tile's list (wave-uniform: scalar loads), testing
// its own voxels against every footprint.  Weights: where dy = min(y, Y-1-y) is the minimum for all of a lane's voxels (all but
// the rows' ends) the row's one weight is read once; lanes nearer the left or right border than dy read ST_V consecutive table
// entries with one vector load pair; only the lane over the FOV's centre line gathers.  A lane's ST_V voxels start where the OUTPUT address is a multiple of ST_V elements
// (the row is shifted left by its misalignment, < ST_V, which the tile lists allow for with an apron), so every store inside the
// row is one or two aligned 16-byte stores; row heads and tails are stored element by element by the same lanes.  FOV rows
// start anywhere relative to that grid: a lane wholly inside a footprint reads its ST_V elements with one (float32: two)
// element-aligned vector loads - gfx950 global loads have no alignment requirement beyond the element - and lanes that straddle
// a footprint edge read element by element.  All offsets are 64-bit.
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace bh {

constexpr int ST_V = 8;            // voxels per lane: 16 B of float16 out, 32 B of float32 out, 16 B of uint16 in
constexpr int ST_TX = 64 * ST_V;   // a wave's row
constexpr int ST_TY = 16;
constexpr int ST_ZC = 4;           // planes per workgroup

struct StitchArgs {
    int64_t Z, Y, X;           // FOV extents
    int64_t r0[3], R[3];       // region origin and extent in the mosaic
    int64_t ntx, nty, nzc;
    int64_t out_elem0;         // address of out in elements: the phase of the store grid
    int nd1;                   // the last index of the weight table proper: (min(Y, X) - 1) / 2
};

template <typename TI>
__device__ __forceinline__ void load_vec(const TI* __restrict__ p, float (&v)[ST_V]) {
    TI raw[ST_V];
    __builtin_memcpy(raw, p, sizeof(raw));  // element-aligned: the back end emits unaligned dwordx4 / dwordx2 loads
#pragma unroll
    for (int i = 0; i < ST_V; ++i) v[i] = (float)raw[i];
}

__device__ __forceinline__ void store_vec(float* __restrict__ q, const float (&r)[ST_V]) {
    reinterpret_cast<float4*>(q)[0] = make_float4(r[0], r[1], r[2], r[3]);
    reinterpret_cast<float4*>(q)[1] = make_float4(r[4], r[5], r[6], r[7]);
}

__device__ __forceinline__ void store_vec(_Float16* __restrict__ q, const float (&r)[ST_V]) {
    _Float16 h[ST_V];
#pragma unroll
    for (int i = 0; i < ST_V; ++i) h[i] = (_Float16)r[i];  // to nearest even, overflow to +-inf
    uint4 w;
    __builtin_memcpy(&w, h, 16);
    *reinterpret_cast<uint4*>(q) = w;
}

// tile_off (nty * ntx + 1) / tile_fov: the tiles' FOV lists; fov: n_fov device pointers; off: n_fov x 3 (z, y, x); wtab: the
// (min(Y, X) - 1) / 2 + 1 weights followed by ST_V copies of the last one.  The tables are separate restrict parameters so that
// the wave-uniform reads become scalar loads.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void stitch_kernel(const StitchArgs a, const int32_t* __restrict__ tile_off,
                                                     const int32_t* __restrict__ tile_fov, const void* const* __restrict__ fov,
                                                     const int64_t* __restrict__ off, const float* __restrict__ wtab,
                                                     TO* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Y = (int)a.Y, X = (int)a.X;
    const int64_t RZ = a.R[0], RY = a.R[1], RX = a.R[2];
    const int64_t total = a.ntx * a.nty * a.nzc;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t tx = t % a.ntx, ty = (t / a.ntx) % a.nty, zc = t / (a.ntx * a.nty);
        const int j0 = tile_off[ty * a.ntx + tx], j1 = tile_off[ty * a.ntx + tx + 1];
        for (int item = wave; item < ST_ZC * ST_TY; item += 4) {
            const int64_t zr = zc * ST_ZC + item / ST_TY, yr = ty * ST_TY + item % ST_TY;
            if (zr >= RZ || yr >= RY) continue;
            const int64_t row = (zr * RY + yr) * RX;                                      // first element of the output row
            const int64_t xs = tx * ST_TX - ((a.out_elem0 + row) & (ST_V - 1)) + (int64_t)lane * ST_V;  // region-relative
            if (xs >= RX || xs + ST_V <= 0) continue;
            const int64_t zm = a.r0[0] + zr, ym = a.r0[1] + yr, xm = a.r0[2] + xs;
            float acc[ST_V], sw[ST_V];
#pragma unroll
            for (int i = 0; i < ST_V; ++i) acc[i] = 0.f, sw[i] = 0.f;
            for (int j = j0; j < j1; ++j) {
                const int f = tile_fov[j];
                const int64_t zz = zm - off[3 * f], yy64 = ym - off[3 * f + 1];
                if (zz < 0 || zz >= a.Z || yy64 < 0 || yy64 >= Y) continue;               // wave-uniform
                const int64_t xx64 = xm - off[3 * f + 2];
                if (xx64 >= X || xx64 + ST_V <= 0) continue;
                const int yy = (int)yy64, xx0 = (int)xx64;
                const int dy = min(yy, Y - 1 - yy);
                const TI* p = static_cast<const TI*>(fov[f]) + ((zz * Y + yy) * (int64_t)X + xx0);
                if (xx0 >= 0 && xx0 + ST_V <= X) {
                    float v[ST_V], w[ST_V];
                    load_vec(p, v);
                    // d = min(dy, dx), dx = min(xx, X-1-xx).  dl / dr: dx of the lane's first element were it in the left half,
                    // of its last one were it in the right half
                    const float wy = wtab[min(dy, a.nd1)];  // dy > nd1 only where X < Y, and there dx < dy: wy is not used
                    const int dl = xx0, dr = X - ST_V - xx0;
                    if (min(dl, dr) >= dy) {  // rows' heads and tails aside, most lanes: one weight, read once per row
#pragma unroll
                        for (int i = 0; i < ST_V; ++i) w[i] = wy;
                    } else if (dl + ST_V - 1 <= dr) {  // wholly in the left half: dx = dl + i, ST_V consecutive weights
                        float tw[ST_V];
                        __builtin_memcpy(tw, wtab + dl, sizeof(tw));  // dl < dy: inside the padded table
#pragma unroll
                        for (int i = 0; i < ST_V; ++i) w[i] = dl + i < dy ? tw[i] : wy;
                    } else if (dr + ST_V - 1 <= dl) {  // wholly in the right half: dx = dr + ST_V - 1 - i
                        float tw[ST_V];
                        __builtin_memcpy(tw, wtab + dr, sizeof(tw));
#pragma unroll
                        for (int i = 0; i < ST_V; ++i) w[i] = dr + ST_V - 1 - i < dy ? tw[ST_V - 1 - i] : wy;
                    } else {  // the lane over the FOV's centre line
#pragma unroll
                        for (int i = 0; i < ST_V; ++i) w[i] = wtab[min(dy, min(xx0 + i, X - 1 - xx0 - i))];
                    }
#pragma unroll
                    for (int i = 0; i < ST_V; ++i) {
                        acc[i] = __builtin_fmaf(v[i], w[i], acc[i]);
                        sw[i] += w[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < ST_V; ++i) {
                        const int xx = xx0 + i;
                        if (xx >= 0 && xx < X) {
                            const float w = wtab[min(dy, min(xx, X - 1 - xx))];
                            acc[i] = __builtin_fmaf((float)p[i], w, acc[i]);
                            sw[i] += w;
                        }
                    }
                }
            }
            float r[ST_V];
#pragma unroll
            for (int i = 0; i < ST_V; ++i) r[i] = acc[i] / (sw[i] + 1e-8f);
            TO* q = out + (row + xs);
            if (xs >= 0 && xs + ST_V <= RX) {
                store_vec(q, r);
            } else {
#pragma unroll
                for (int i = 0; i < ST_V; ++i)
                    if (xs + i >= 0 && xs + i < RX) q[i] = (TO)r[i];
            }
        }
    }
}

// Tiles of the region's (y, x) plane and, per tile, the FOVs whose footprint meets it, in FOV order.  Tile (ty, tx) is rows
// [ty * ST_TY, (ty + 1) * ST_TY) and columns [tx * ST_TX - (ST_V - 1), (tx + 1) * ST_TX) of the region, clipped to it: the
// apron on the left is how far a row can be shifted to put its stores on the 16-byte grid.  FOVs whose z range misses the region
// are in no list.
struct TileLists {
    int64_t nty = 0, ntx = 0;
    std::vector<int32_t> off, fov;
};

static void tile_range(int64_t o, int64_t n, int64_t r0, int64_t R, int64_t tile, int64_t apron, int64_t nt, int64_t* lo, int64_t* hi) {
    const int64_t a = std::max<int64_t>(o - r0, 0), b = std::min<int64_t>(o + n - r0, R);  // the footprint inside the region
    if (b <= a) {
        *lo = 1, *hi = 0;
        return;
    }
    *lo = a / tile;
    *hi = std::min<int64_t>((b - 1 + apron) / tile, nt - 1);
}

static TileLists build_tile_lists(int n_fov, const int64_t* off, int64_t Z, int64_t Y, int64_t X, const int64_t r0[3], const int64_t R[3]) {
    TileLists t;
    t.nty = ceil_div(R[1], ST_TY);
    t.ntx = ceil_div(R[2] + ST_V - 1, ST_TX);
    std::vector<int32_t> count((size_t)(t.nty * t.ntx), 0);
    for (int pass = 0; pass < 2; ++pass) {
        for (int f = 0; f < n_fov; ++f) {
            if (off[3 * f] >= r0[0] + R[0] || off[3 * f] + Z <= r0[0]) continue;
            int64_t y0, y1, x0, x1;
            tile_range(off[3 * f + 1], Y, r0[1], R[1], ST_TY, 0, t.nty, &y0, &y1);
            tile_range(off[3 * f + 2], X, r0[2], R[2], ST_TX, ST_V - 1, t.ntx, &x0, &x1);
            for (int64_t ty = y0; ty <= y1; ++ty)
                for (int64_t tx = x0; tx <= x1; ++tx) {
                    if (pass == 0) ++count[(size_t)(ty * t.ntx + tx)];
                    else t.fov[(size_t)count[(size_t)(ty * t.ntx + tx)]++] = f;
                }
        }
        if (pass == 0) {  // counts -> offsets; `count` becomes the fill cursor
            t.off.assign(count.size() + 1, 0);
            for (size_t i = 0; i < count.size(); ++i) t.off[i + 1] = t.off[i] + count[i];
            for (size_t i = 0; i < count.size(); ++i) count[i] = t.off[i];
            t.fov.assign((size_t)t.off.back(), 0);
        }
    }
    return t;
}

static int check_geometry(const char* who, int n_fov, const int64_t* off, int64_t Z, int64_t Y, int64_t X, const int64_t* r0, const int64_t* R) {
    BH_REQUIRE(n_fov >= 1, "%s: n_fov = %d (>= 1)", who, n_fov);
    BH_REQUIRE(off && r0 && R, "%s: null argument", who);
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0, "%s: bad FOV shape (%lld, %lld, %lld)", who, (long long)Z, (long long)Y, (long long)X);
    BH_REQUIRE(Y < (1 << 30) && X < (1 << 30), "%s: FOV plane (%lld, %lld) too large", who, (long long)Y, (long long)X);
    BH_REQUIRE(R[0] > 0 && R[1] > 0 && R[2] > 0, "%s: bad region extent (%lld, %lld, %lld)", who, (long long)R[0], (long long)R[1], (long long)R[2]);
    BH_REQUIRE(r0[0] >= 0 && r0[1] >= 0 && r0[2] >= 0, "%s: negative region origin", who);
    for (int i = 0; i < 3 * n_fov; ++i) BH_REQUIRE(off[i] >= 0, "%s: negative offset %lld of FOV %d", who, (long long)off[i], i / 3);
    BH_REQUIRE(ceil_div(R[1], ST_TY) * ceil_div(R[2] + ST_V - 1, ST_TX) < (int64_t)1 << 30, "%s: region plane too large", who);
    return BH_OK;
}

struct StitchTables {
    const int32_t *tile_off, *tile_fov;
    const void* const* fov;
    const int64_t* off;
    const float* wtab;
};

template <typename TI>
static void launch_in(const StitchArgs& a, const StitchTables& t, int out_dtype, void* out, int grid, hipStream_t s) {
    if (out_dtype == BH_DT_F16)
        hipLaunchKernelGGL((stitch_kernel<TI, _Float16>), dim3(grid), dim3(256), 0, s, a, t.tile_off, t.tile_fov, t.fov, t.off, t.wtab,
                           static_cast<_Float16*>(out));
    else
        hipLaunchKernelGGL((stitch_kernel<TI, float>), dim3(grid), dim3(256), 0, s, a, t.tile_off, t.tile_fov, t.fov, t.off, t.wtab,
                           static_cast<float*>(out));
}

}  // namespace bh

using namespace bh;

extern "C" int bh_stitch_tile_lists(int n_fov, const int64_t* offset_zyx, int64_t Z, int64_t Y, int64_t X, const int64_t region_origin[3],
                                    const int64_t region_extent[3], int64_t tiling[5], int32_t* tile_off, int32_t* tile_fov,
                                    int64_t capacity, int64_t* n_entries) {
    BH_TRY(check_geometry("bh_stitch_tile_lists", n_fov, offset_zyx, Z, Y, X, region_origin, region_extent));
    BH_REQUIRE(tiling && n_entries, "bh_stitch_tile_lists: null argument");
    const TileLists t = build_tile_lists(n_fov, offset_zyx, Z, Y, X, region_origin, region_extent);
    tiling[0] = ST_TY, tiling[1] = ST_TX, tiling[2] = ST_V - 1, tiling[3] = t.nty, tiling[4] = t.ntx;
    *n_entries = (int64_t)t.fov.size();
    if (tile_off) std::memcpy(tile_off, t.off.data(), t.off.size() * sizeof(int32_t));
    if (tile_fov) {
        BH_REQUIRE(capacity >= (int64_t)t.fov.size(), "bh_stitch_tile_lists: tile_fov holds %lld entries, %lld needed", (long long)capacity,
                   (long long)t.fov.size());
        if (!t.fov.empty()) std::memcpy(tile_fov, t.fov.data(), t.fov.size() * sizeof(int32_t));
    }
    return BH_OK;
}

extern "C" int bh_stitch_blend(bh_ctx* ctx, int n_fov, const void* const* fov, const int64_t* offset_zyx, int in_dtype, int64_t Z, int64_t Y,
                               int64_t X, double blending_exponent, const int64_t region_origin[3], const int64_t region_extent[3],
                               int out_dtype, void* out) {
    BH_TRY(check_geometry("bh_stitch_blend", n_fov, offset_zyx, Z, Y, X, region_origin, region_extent));
    BH_REQUIRE(ctx && fov && out, "bh_stitch_blend: null argument");
    for (int i = 0; i < n_fov; ++i) BH_REQUIRE(fov[i], "bh_stitch_blend: fov[%d] is null", i);
    BH_REQUIRE(in_dtype == BH_DT_U8 || in_dtype == BH_DT_U16 || in_dtype == BH_DT_I16 || in_dtype == BH_DT_F32,
               "bh_stitch_blend: unsupported input dtype code %d (uint8, uint16, int16, float32)", in_dtype);
    BH_REQUIRE(out_dtype == BH_DT_F32 || out_dtype == BH_DT_F16, "bh_stitch_blend: unsupported output dtype code %d (float32, float16)",
               out_dtype);
    BH_REQUIRE(blending_exponent >= 0.0, "bh_stitch_blend: blending_exponent %g (>= 0)", blending_exponent);  // false for NaN too
    const size_t osize = out_dtype == BH_DT_F16 ? 2 : 4;
    BH_REQUIRE(reinterpret_cast<uintptr_t>(out) % osize == 0, "bh_stitch_blend: out is not aligned to its element size");
    const int64_t nd = (std::min(Y, X) - 1) / 2 + 1;
    std::vector<float> wtab((size_t)nd + ST_V, 0.f);  // ST_V copies of the last weight follow: the kernel reads ST_V at a time
    for (int64_t d = 1; d < nd; ++d) wtab[(size_t)d] = (float)std::pow((double)d, blending_exponent);
    for (int64_t d = nd; d < nd + ST_V; ++d) wtab[(size_t)d] = wtab[(size_t)nd - 1];
    BH_REQUIRE(std::isfinite(wtab.back()), "bh_stitch_blend: %lld ** %g overflows float32", (long long)(nd - 1), blending_exponent);

    const TileLists t = build_tile_lists(n_fov, offset_zyx, Z, Y, X, region_origin, region_extent);
    // one staging block: pointers | offsets | tile offsets | tile FOVs | weights (8-byte items first)
    const size_t b_ptr = (size_t)n_fov * sizeof(void*), b_off = (size_t)n_fov * 3 * sizeof(int64_t), b_to = t.off.size() * sizeof(int32_t),
                 b_tf = t.fov.size() * sizeof(int32_t), b_w = wtab.size() * sizeof(float);
    std::vector<unsigned char> blob(b_ptr + b_off + b_to + b_tf + b_w);
    unsigned char* h = blob.data();
    std::memcpy(h, fov, b_ptr);
    std::memcpy(h + b_ptr, offset_zyx, b_off);
    std::memcpy(h + b_ptr + b_off, t.off.data(), b_to);
    if (b_tf) std::memcpy(h + b_ptr + b_off + b_to, t.fov.data(), b_tf);
    std::memcpy(h + b_ptr + b_off + b_to + b_tf, wtab.data(), b_w);

    BH_CHECK_HIP(hipSetDevice(ctx->device));
    unsigned char* d = nullptr;
    BH_TRY(get_scratch(ctx, "stitch_tab", blob.size(), (void**)&d));
    // pageable source: the runtime has taken the bytes when this returns, and the copy is ordered after earlier launches that
    // still read the block
    BH_CHECK_HIP(hipMemcpyAsync(d, h, blob.size(), hipMemcpyHostToDevice, ctx->stream));
    StitchArgs a{};
    StitchTables tb{};
    tb.fov = reinterpret_cast<const void* const*>(d);
    tb.off = reinterpret_cast<const int64_t*>(d + b_ptr);
    tb.tile_off = reinterpret_cast<const int32_t*>(d + b_ptr + b_off);
    tb.tile_fov = reinterpret_cast<const int32_t*>(d + b_ptr + b_off + b_to);
    tb.wtab = reinterpret_cast<const float*>(d + b_ptr + b_off + b_to + b_tf);
    a.Z = Z, a.Y = Y, a.X = X;
    for (int k = 0; k < 3; ++k) a.r0[k] = region_origin[k], a.R[k] = region_extent[k];
    a.ntx = t.ntx, a.nty = t.nty, a.nzc = ceil_div(region_extent[0], ST_ZC);
    a.out_elem0 = (int64_t)(reinterpret_cast<uintptr_t>(out) / osize);
    a.nd1 = (int)(nd - 1);
    const int grid = (int)std::min<int64_t>(a.ntx * a.nty * a.nzc, (int64_t)1 << 20);
    switch (in_dtype) {
        case BH_DT_U8: launch_in<uint8_t>(a, tb, out_dtype, out, grid, ctx->stream); break;
        case BH_DT_U16: launch_in<uint16_t>(a, tb, out_dtype, out, grid, ctx->stream); break;
        case BH_DT_I16: launch_in<int16_t>(a, tb, out_dtype, out, grid, ctx->stream); break;
        default: launch_in<float>(a, tb, out_dtype, out, grid, ctx->stream); break;
    }
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}
