// Geometry and float32 coordinate arithmetic of the deskew, written once for the GPU kernels (deskew.hip, deskew_rows.inc) and
// the host form (host_deskew.hip): what the two compute from, so that they agree by construction.
#pragma once

#include "common.hpp"

#include <cmath>

namespace bh {

struct DeskewGeom {
    int Z, Y, X;     // input
    int Za, Xp;      // output (Za, X, Xp)
    int N;           // average_n_slices
    float px, pxct, offset, zm1;
    int ZC;          // max z-window length of the launched configuration (rows per averaged slice of the LDS tile)
    // fused overhang-fill prologue (FILL kernels): zero-mask bits + per-block sums
    uint32_t* mask0;  // [Za*X][W32] one bit per output voxel (1 = exact zero)
    double* psum;     // per-block partial sums of the outputs
    int W32;          // mask words per output row (even)
    const int* enable;  // FILL kernels, may be null: device flag, 0 = nothing to do (the conditional pass behind the one-pass path)
    // one-pass fill (deskew_pers_kernel<NK, 2>): the geometry's zero pattern and its dilation, one bit per (a, x'), WB words per a;
    // the fill value (already final) and the fallback flag live in *st
    const uint32_t* gbits;
    const uint32_t* dgbits;
    int WB;
    FillStats* st;
};

// Shapes and the four coordinate constants, each rounded to float32 once; every pointer of *g null.
inline int deskew_geometry(int64_t Z, int64_t Y, int64_t X, double angle, double ratio, int keep_overhang, int n, DeskewGeom* g,
                           int64_t out_shape[3]) {
    double voxel[3];
    BH_TRY(bh_deskew_shape(Z, Y, X, angle, ratio, keep_overhang, n, 1.0, out_shape, voxel));
    // un-averaged geometry drives the shear offset (deskew.py:499-503: Z_out_full = Y)
    const double ct = std::cos(angle * M_PI / 180.0);
    const double px = ratio;
    const int64_t Xp = out_shape[2];
    const double offset = px * ct * (double)(Y - 1) / 2 - px * (double)(Xp - 1) / 2 + (double)(Z - 1) / 2;
    *g = DeskewGeom{};
    g->Z = (int)Z;
    g->Y = (int)Y;
    g->X = (int)X;
    g->Za = (int)out_shape[0];
    g->Xp = (int)Xp;
    g->N = n;
    g->px = (float)px;
    g->pxct = (float)(px * ct);
    g->offset = (float)offset;
    g->zm1 = (float)(Z - 1);
    return BH_OK;
}

// The reference's sample position along the scan axis, in its float32 operation order:
//   in_z = px*x - (px*ct)*zo + offset ; g = 2*in_z/(Z-1) - 1 ; ix = ((g+1)/2)*(Z-1)
__host__ __device__ inline float deskew_ix(float px, float pxct, float offset, float zm1, int xo, int zo) {
#pragma clang fp contract(off)
    float t1 = px * (float)xo;
    float t2 = pxct * (float)zo;
    float in_z = (t1 - t2) + offset;
    float g = (2.0f * in_z) / zm1 - 1.0f;
    float ix = ((g + 1.0f) / 2.0f) * zm1;
    return ix;
}

// The two taps of output (xo, zo): the lower input row z0 = floor(ix) (the upper one is z0 + 1; either may lie outside
// [0, Z)) and their weights.  w0 > 0 always; w1 == 0 where ix is an integer.
struct DeskewTaps {
    int z0;
    float w0, w1;
};
__host__ __device__ inline DeskewTaps deskew_taps(const DeskewGeom& g, int xo, int zo) {
#pragma clang fp contract(off)
    const float ix = deskew_ix(g.px, g.pxct, g.offset, g.zm1, xo, zo);
    const float fl = floorf(ix);
    DeskewTaps t;
    t.z0 = (int)fl;
    t.w1 = ix - fl;
    t.w0 = (fl + 1.0f) - ix;
    return t;
}

// z window covering every tap of the N averaged slices of slab a over the x' chunk [xo0, min(xo0 + XC, Xp)): ix is monotone
// in xo and zo.  zcnt is NOT clamped: the kernels clamp it to g.ZC (which the host sized with the same function, so the clamp
// is a memory-safety net only); a window one row short would be an out-of-range LDS read, not a wrong digit.
struct DeskewWindow {
    int zlo, zcnt;
};
__host__ __device__ inline DeskewWindow deskew_window(const DeskewGeom& g, int N, int a, int xo0, int XC) {
#pragma clang fp contract(off)
    const int zo0 = a * N;
    const int xoN = XC < g.Xp - xo0 ? XC : g.Xp - xo0;  // x' in the chunk
    const float ix_min = deskew_ix(g.px, g.pxct, g.offset, g.zm1, xo0, zo0 + N - 1);
    const float ix_max = deskew_ix(g.px, g.pxct, g.offset, g.zm1, xo0 + xoN - 1, zo0);
    DeskewWindow w;
    w.zlo = (int)floorf(ix_min);
    w.zcnt = (int)floorf(ix_max) + 2 - w.zlo;
    return w;
}

// a / N, N a small positive integer: q = a*(1/N) corrected by one fused residual step
// (r = a - q*N is exact in fma), which is the correctly rounded quotient for these operands.
__host__ __device__ __forceinline__ float div_small(float a, float n, float rn) {
    const float q = a * rn;
    const float r = __builtin_fmaf(-q, n, a);
    return __builtin_fmaf(r, rn, q);
}

// The deskew's input types: f(const T* in) for the element type `in_dtype` names, its status returned; an unknown code is an
// error here, whatever f would have done.
template <typename F>
inline int deskew_dispatch_dtype(const void* in, int in_dtype, F&& f) {
    switch (in_dtype) {
        case BH_DT_F32: return f((const float*)in);
        case BH_DT_U16: return f((const uint16_t*)in);
        case BH_DT_U8: return f((const uint8_t*)in);
        case BH_DT_I16: return f((const int16_t*)in);
    }
    set_error("unsupported input dtype code %d", in_dtype);
    return BH_ERR_INVALID;
}

}  // namespace bh
