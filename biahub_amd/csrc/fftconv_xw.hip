// The wave-private X passes of the fused FFT engine (fftconv.hip): rows of 512 / 1024 / 2048 voxels (fftconv_xw.inc) and of
// 1536 / 3072 voxels (fftconv_x3.inc) on the row-pair frame they share (fftconv_xrows.inc), their launchers and tables.
#include "fftconv_dev.hpp"

namespace bh {

#include "fftconv_regfft.inc"
#include "fftconv_xrows.inc"
#include "fftconv_xw.inc"
#include "fftconv_x3.inc"

void xw_tables(int64_t X, std::vector<cf>& tab, std::vector<int>& col) {
    if (X == 3072) x3::make_tables<9>(tab, col);
    else if (X == 1536) x3::make_tables<8>(tab, col);
    else if (X == 2048) xw::make_tables<10>(tab, col);
    else if (X == 1024) xw::make_tables<9>(tab, col);
    else xw::make_tables<8>(tab, col);
}

// the mode table of a family: NS = its namespace, KERN = its kernel template over (LOG, mode)
#define BH_XW_CASE(NS, KERN, MODE_) \
    case xw::MODE_: return launch_lds(ctx, NS::KERN<LOG, xw::MODE_>, grid, NS::NT, NS::Geo<LOG>::LDS_BYTES, p);
#define BH_XW_LAUNCHER(NAME, NS, KERN, FAMILY_MODES)                                                           \
    template <int LOG>                                                                                         \
    static int NAME(bh_ctx* ctx, const xw::Params& p, int mode, int* grid_out = nullptr) {                     \
        const long npairs = (long)p.Z * (p.Y / 2);                                                             \
        const int grid = (int)std::min<long>(ceil_div(npairs, (long)NS::NW * NS::Geo<LOG>::PAIRS), ctx->num_cus); \
        if (grid_out) *grid_out = grid;                                                                        \
        switch (mode) {                                                                                        \
            BH_XW_CASE(NS, KERN, FWD)                                                                          \
            BH_XW_CASE(NS, KERN, INV_STORE)                                                                    \
            BH_XW_CASE(NS, KERN, INV_RATIO)                                                                    \
            BH_XW_CASE(NS, KERN, INV_UPDATE)                                                                   \
            BH_XW_CASE(NS, KERN, FUSED_RATIO)                                                                  \
            BH_XW_CASE(NS, KERN, FUSED_UPDATE)                                                                 \
            BH_XW_CASE(NS, KERN, FUSED_RATIO_WRAP)                                                             \
            BH_XW_CASE(NS, KERN, FUSED_UPDATE_WRAP)                                                            \
            BH_XW_CASE(NS, KERN, INV_UPDATE_CROP)                                                              \
            FAMILY_MODES                                                                                       \
        }                                                                                                      \
        set_error("internal: " #KERN " has no mode %d", mode);                                                 \
        return BH_ERR_INVALID;                                                                                 \
    }
BH_XW_LAUNCHER(launch_xw_m, xw, xw_kernel, BH_XW_CASE(xw, xw_kernel, INV_ARGMAX))  // 3 row lengths x 10 modes
BH_XW_LAUNCHER(launch_x3_m, x3, x3_kernel, )                                       // 2 row lengths x 9 modes: no arg-max search
#undef BH_XW_LAUNCHER
#undef BH_XW_CASE

// the launch of `mode` by the plan's row length
static int launch_rows(bh_ctx* ctx, const ConvPlan& pl, const xw::Params& p, int mode, int* grid_out = nullptr) {
    if (pl.x3) return pl.d.M == 1536 ? launch_x3_m<9>(ctx, p, mode, grid_out) : launch_x3_m<8>(ctx, p, mode, grid_out);
    return pl.d.M == 1024 ? launch_xw_m<10>(ctx, p, mode, grid_out)
                          : (pl.d.M == 512 ? launch_xw_m<9>(ctx, p, mode, grid_out) : launch_xw_m<8>(ctx, p, mode, grid_out));
}

// what every pass takes from the plan and its buffers; the options (norm_mean, rowsum, S_out, wrap geometry) are off
static xw::Params plan_params(const ConvPlan& pl, const float* in, cf* S, float* out, const float* aux, float eps) {
    xw::Params p;
    p.in = in;
    p.S = S;
    p.out = out;
    p.aux = aux;
    p.tab = pl.xw_tab;
    p.twy = pl.twy;
    p.Z = pl.d.Z;
    p.Y = pl.d.Y;
    p.XP = pl.d.XP;
    p.eps = eps;
    p.norm_mean = nullptr;
    p.rowsum = nullptr;
    p.S_out = nullptr;
    p.wz = p.wx = xw::Params::Wrap{0, 0, 0, 0};
    return p;
}

int launch_xw(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out, const float* aux,
              float eps, bool fuse_fwd, const double* norm_mean) {
    xw::Params p = plan_params(pl, in, S, out, aux, eps);
    p.norm_mean = norm_mean;
    const int mode = !inverse ? xw::FWD
                     : epi == XE_STORE ? xw::INV_STORE
                     : epi == XE_RATIO ? (fuse_fwd ? xw::FUSED_RATIO : xw::INV_RATIO)
                                       : (fuse_fwd ? xw::FUSED_UPDATE : xw::INV_UPDATE);
    if (mode == xw::INV_UPDATE && !pl.x3 && pl.rl_rowsums != nullptr) {
        p.rowsum = pl.rl_rowsums;
        const_cast<ConvPlan&>(pl).rl_rowsums_done = true;
    }
    return launch_rows(ctx, pl, p, mode);
}

// inverse X pass that keeps only the first occurrence of max |.| (xw::INV_ARGMAX): `partial` receives *npartial entries
int launch_xw_argmax(bh_ctx* ctx, const ConvPlan& pl, cf* S, ArgMax* partial, int* npartial) {
    const xw::Params p = plan_params(pl, nullptr, S, reinterpret_cast<float*>(partial), nullptr, 0.f);
    int grid = 0;
    BH_TRY(launch_rows(ctx, pl, p, xw::INV_ARGMAX, &grid));
    *npartial = grid * xw::NW;
    return BH_OK;
}

// the out-of-place passes of Richardson-Lucy at a wrap-padded box (mode: one of the xw::*_WRAP modes or xw::INV_UPDATE_CROP)
int launch_xw_wrap(bh_ctx* ctx, const ConvPlan& pl, int mode, const cf* S_in, cf* S_out, float* out, const float* aux, float eps,
                   xw::Params::Wrap wz, xw::Params::Wrap wx) {
    xw::Params p = plan_params(pl, nullptr, const_cast<cf*>(S_in), out, aux, eps);
    p.S_out = S_out;
    p.wz = wz;
    p.wx = wx;
    return launch_rows(ctx, pl, p, mode);
}

}  // namespace bh
