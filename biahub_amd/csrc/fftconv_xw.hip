// The wave-private X passes of the fused FFT engine (fftconv.hip): rows of 512 / 1024 / 2048 voxels (fftconv_xw.inc) and of
// 1536 / 3072 voxels (fftconv_x3.inc), their launchers and tables.
#include "fftconv_dev.hpp"

namespace bh {

#include "fftconv_xw.inc"
#include "fftconv_x3.inc"

void xw_tables(int64_t X, std::vector<cf>& tab, std::vector<int>& col) {
    if (X == 3072) x3::make_tables<9>(tab, col);
    else if (X == 1536) x3::make_tables<8>(tab, col);
    else if (X == 2048) xw::make_tables<10>(tab, col);
    else if (X == 1024) xw::make_tables<9>(tab, col);
    else xw::make_tables<8>(tab, col);
}

template <int LOGM>
static int launch_xw_m(bh_ctx* ctx, const xw::Params& p, int mode, int* grid_out = nullptr) {
    using G = xw::Geo<LOGM>;
    const long npairs = (long)p.Z * (p.Y / 2);
    const int grid = (int)std::min<long>(ceil_div(npairs, (long)xw::NW * G::PAIRS), ctx->num_cus);
    if (grid_out) *grid_out = grid;
    auto run = [&](auto kern) { return launch_lds(ctx, kern, grid, xw::NT, G::LDS_BYTES, p); };
    switch (mode) {
        case xw::FWD: return run(xw::xw_kernel<LOGM, xw::FWD>);
        case xw::INV_STORE: return run(xw::xw_kernel<LOGM, xw::INV_STORE>);
        case xw::INV_RATIO: return run(xw::xw_kernel<LOGM, xw::INV_RATIO>);
        case xw::INV_UPDATE: return run(xw::xw_kernel<LOGM, xw::INV_UPDATE>);
        case xw::FUSED_RATIO: return run(xw::xw_kernel<LOGM, xw::FUSED_RATIO>);
        case xw::FUSED_RATIO_WRAP: return run(xw::xw_kernel<LOGM, xw::FUSED_RATIO_WRAP>);
        case xw::FUSED_UPDATE_WRAP: return run(xw::xw_kernel<LOGM, xw::FUSED_UPDATE_WRAP>);
        case xw::INV_UPDATE_CROP: return run(xw::xw_kernel<LOGM, xw::INV_UPDATE_CROP>);
        case xw::INV_ARGMAX: return run(xw::xw_kernel<LOGM, xw::INV_ARGMAX>);
        default: return run(xw::xw_kernel<LOGM, xw::FUSED_UPDATE>);
    }
}

template <int LOGL>
static int launch_x3_m(bh_ctx* ctx, const xw::Params& p, int mode) {
    using G = x3::Geo<LOGL>;
    const long npairs = (long)p.Z * (p.Y / 2);
    const int grid = (int)std::min<long>(ceil_div(npairs, (long)x3::NW * G::PAIRS), ctx->num_cus);
    auto run = [&](auto kern) { return launch_lds(ctx, kern, grid, x3::NT, G::LDS_BYTES, p); };
    switch (mode) {
        case xw::FWD: return run(x3::x3_kernel<LOGL, xw::FWD>);
        case xw::INV_STORE: return run(x3::x3_kernel<LOGL, xw::INV_STORE>);
        case xw::INV_RATIO: return run(x3::x3_kernel<LOGL, xw::INV_RATIO>);
        case xw::INV_UPDATE: return run(x3::x3_kernel<LOGL, xw::INV_UPDATE>);
        case xw::FUSED_RATIO: return run(x3::x3_kernel<LOGL, xw::FUSED_RATIO>);
        case xw::FUSED_RATIO_WRAP: return run(x3::x3_kernel<LOGL, xw::FUSED_RATIO_WRAP>);
        case xw::FUSED_UPDATE_WRAP: return run(x3::x3_kernel<LOGL, xw::FUSED_UPDATE_WRAP>);
        case xw::INV_UPDATE_CROP: return run(x3::x3_kernel<LOGL, xw::INV_UPDATE_CROP>);
        default: return run(x3::x3_kernel<LOGL, xw::FUSED_UPDATE>);
    }
}

int launch_xw(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out, const float* aux,
              float eps, bool fuse_fwd, const double* norm_mean) {
    xw::Params p;
    p.norm_mean = norm_mean;
    p.rowsum = nullptr;
    p.S_out = nullptr;
    p.wz = p.wx = xw::Params::Wrap{0, 0, 0, 0};
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
    const int mode = !inverse ? xw::FWD
                     : epi == XE_STORE ? xw::INV_STORE
                     : epi == XE_RATIO ? (fuse_fwd ? xw::FUSED_RATIO : xw::INV_RATIO)
                                       : (fuse_fwd ? xw::FUSED_UPDATE : xw::INV_UPDATE);
    if (mode == xw::INV_UPDATE && !pl.x3 && pl.rl_rowsums != nullptr) {
        p.rowsum = pl.rl_rowsums;
        const_cast<ConvPlan&>(pl).rl_rowsums_done = true;
    }
    if (pl.x3) return pl.d.M == 1536 ? launch_x3_m<9>(ctx, p, mode) : launch_x3_m<8>(ctx, p, mode);
    return pl.d.M == 1024 ? launch_xw_m<10>(ctx, p, mode) : (pl.d.M == 512 ? launch_xw_m<9>(ctx, p, mode) : launch_xw_m<8>(ctx, p, mode));
}

// inverse X pass that keeps only the first occurrence of max |.| (xw::INV_ARGMAX): `partial` receives *npartial entries
int launch_xw_argmax(bh_ctx* ctx, const ConvPlan& pl, cf* S, ArgMax* partial, int* npartial) {
    xw::Params p;
    p.norm_mean = nullptr;
    p.rowsum = nullptr;
    p.S_out = nullptr;
    p.wz = p.wx = xw::Params::Wrap{0, 0, 0, 0};
    p.in = nullptr;
    p.S = S;
    p.out = reinterpret_cast<float*>(partial);
    p.aux = nullptr;
    p.tab = pl.xw_tab;
    p.twy = pl.twy;
    p.Z = pl.d.Z;
    p.Y = pl.d.Y;
    p.XP = pl.d.XP;
    p.eps = 0.f;
    int grid = 0;
    BH_TRY(pl.d.M == 1024 ? launch_xw_m<10>(ctx, p, xw::INV_ARGMAX, &grid)
                          : (pl.d.M == 512 ? launch_xw_m<9>(ctx, p, xw::INV_ARGMAX, &grid) : launch_xw_m<8>(ctx, p, xw::INV_ARGMAX, &grid)));
    *npartial = grid * xw::NW;
    return BH_OK;
}

// the out-of-place passes of Richardson-Lucy at a wrap-padded box (mode: one of the xw::*_WRAP modes or xw::INV_UPDATE_CROP)
int launch_xw_wrap(bh_ctx* ctx, const ConvPlan& pl, int mode, const cf* S_in, cf* S_out, float* out, const float* aux, float eps,
                   xw::Params::Wrap wz, xw::Params::Wrap wx) {
    xw::Params p;
    p.norm_mean = nullptr;
    p.rowsum = nullptr;
    p.in = nullptr;
    p.S = const_cast<cf*>(S_in);
    p.S_out = S_out;
    p.out = out;
    p.aux = aux;
    p.tab = pl.xw_tab;
    p.twy = pl.twy;
    p.Z = pl.d.Z;
    p.Y = pl.d.Y;
    p.XP = pl.d.XP;
    p.eps = eps;
    p.wz = wz;
    p.wx = wx;
    if (!pl.x3) return pl.d.M == 1024 ? launch_xw_m<10>(ctx, p, mode) : (pl.d.M == 512 ? launch_xw_m<9>(ctx, p, mode) : launch_xw_m<8>(ctx, p, mode));
    return pl.d.M == 1536 ? launch_x3_m<9>(ctx, p, mode) : launch_x3_m<8>(ctx, p, mode);
}

}  // namespace bh
