// The register-stage column passes of the fused FFT engine (fftconv.hip) and the choice among all column kernels: colw
// (columns of 256 / 512 / 1024 points), colz (512-point Z passes with a spectral product), colz3 (384 / 768 points) and the
// direct Z pass with compact taps; what none of them takes goes to col_pass_kernel (fftconv_col.hip).
#include "fftconv_dev.hpp"

namespace bh {

#include "fftconv_regfft.inc"  // the in-register butterflies (xw::reg_fft), xw::brev_c and xw::opaque_i
#include "fftconv_colw.inc"
#include "fftconv_colz.inc"
#include "fftconv_colz3.inc"
#include "fftconv_zdirect.inc"

bool colw_tables(int64_t n, std::vector<cf>& tab) {
    if (n == 256) colw::make_tables<8>(tab);
    else if (n == 512) colw::make_tables<9>(tab);
    else if (n == 1024) colw::make_tables<10>(tab);
    else return false;
    return true;
}
bool colz_tables(const ConvDims& d, std::vector<cf>& tab) {
    if (d.Z != colz::N || d.XP < colz::W) return false;
    colz::make_tables(tab);
    return true;
}
bool colz3_tables(const ConvDims& d, std::vector<cf>& tab) {
    if (d.Z == 384 && d.XP >= 32) colz3::make_tables<7>(tab);
    else if (d.Z == 768 && d.XP >= 16) colz3::make_tables<8>(tab);
    else return false;
    return true;
}

template <int LOGN>
static int launch_colw(bh_ctx* ctx, ColParams p, int mode) {
    using G = colw::Geo<LOGN>;
    p.W = G::W;
    p.ncoltiles = (int)ceil_div(p.XP, p.W);
    const long ntiles = (long)p.nouter * p.ncoltiles;
    const int grid = (int)std::min<long>(ntiles, (long)ctx->num_cus * (512 / colw::NT));
    auto run = [&](auto kern) { return launch_lds(ctx, kern, grid, colw::NT, G::LDS_BYTES, p); };
    switch (mode) {
        case COL_FWD: return run(colw::colw_kernel<LOGN, COL_FWD>);
        case COL_INV: return run(colw::colw_kernel<LOGN, COL_INV>);
        case COL_FWD_SCALE: return run(colw::colw_kernel<LOGN, COL_FWD_SCALE>);
        case COL_CONV: return run(colw::colw_kernel<LOGN, COL_CONV>);
        case COL_FILTER: return run(colw::colw_kernel<LOGN, COL_FILTER>);
        case COL_CONV16: return run(colw::colw_kernel<LOGN, COL_CONV16>);
        default: return run(colw::colw_kernel<LOGN, COL_CORR>);
    }
}

int launch_col(bh_ctx* ctx, const ConvPlan& pl, int mode, bool zaxis, cf* S, const cf* otf, float scale, int pcc_norm, int pcc_swap,
               cf* otf_out) {
    ColParams p;
    p.pcc_norm = pcc_norm;
    p.pcc_swap = pcc_swap;
    p.otf_out = otf_out;
    p.S = S;
    p.otf = otf;
    p.XP = pl.d.XP;
    p.scale = scale;
    if (!zaxis) {
        p.N = pl.d.Y / 2;
        p.logN = pl.d.logYh;
        p.W = pl.Wy;
        p.tw = pl.tw_y;
        p.ntw = pl.ntw_y;
        p.L = pl.Lyh;
        p.tw3 = pl.tw3_y;
        p.row_stride = pl.d.XP;
        p.outer_stride = (long)pl.d.Y * pl.d.XP;
        p.sub_stride = (long)(pl.d.Y / 2) * pl.d.XP;
        p.nsub = 2;
        p.nouter = pl.d.Z * 2;
    } else {
        p.N = pl.d.Z;
        p.logN = pl.d.logZ;
        p.W = pl.Wz;
        p.tw = pl.tw_z;
        p.ntw = pl.ntw_z;
        p.L = pl.Lz;
        p.tw3 = pl.tw3_z;
        p.row_stride = (long)pl.d.Y * pl.d.XP;
        p.outer_stride = pl.d.XP;
        p.sub_stride = 0;
        p.nsub = 1;
        p.nouter = pl.d.Y;
    }
    // 512-point Z passes with a spectral product: radix-8 register stages (BH_FC_COLZ=0 keeps the radix-4 LDS steps: A/B switch)
    if (zaxis && pl.colz && p.N == colz::N && (mode == COL_CONV || mode == COL_CORR || mode == COL_FILTER || mode == COL_CONV16 || mode == COL_PCC) &&
        !env_off("BH_FC_COLZ") &&
        p.row_stride * 8 * 64 < (1ll << 32)) {  // colz_kernel's lanes address their rows by 32-bit offsets from scalar row pointers
        p.W = colz::W;
        p.tw = pl.colz;
        p.ncoltiles = (int)ceil_div(p.XP, p.W);
        const long ntiles = (long)p.nouter * p.ncoltiles;
        const int grid = (int)std::min<long>(ntiles, (long)ctx->num_cus * (1024 / colz::NT));
        auto run = [&](auto kern) { return launch_lds(ctx, kern, grid, colz::NT, colz::LDS_BYTES, p); };
        switch (mode) {
            case COL_CONV: return run(colz::colz_kernel<COL_CONV>);
            case COL_CORR: return run(colz::colz_kernel<COL_CORR>);
            case COL_FILTER: return run(colz::colz_kernel<COL_FILTER>);
            case COL_CONV16: return run(colz::colz_kernel<COL_CONV16>);
            default: return run(colz::colz_kernel<COL_PCC>);
        }
    }
    // 384- / 768-point Z passes with a spectral product (the boxes of the deskewed config-4 / config-2 volumes): register stages
    // (BH_FC_COLZ3=0: A/B switch)
    // (lane offsets are 32-bit: 64 rows of the spectrum must span less than 4 GiB, as for colz_kernel)
    if (zaxis && pl.colz3 && (p.N == 384 || p.N == 768) && (mode == COL_CONV || mode == COL_CORR || mode == COL_FILTER) &&
        p.row_stride * 8 * 64 < (1ll << 32) && !env_off("BH_FC_COLZ3")) {
        p.tw = pl.colz3;
        auto run = [&](auto kern, int w, int nt, int lds) -> int {
            p.W = w;
            p.ncoltiles = (int)ceil_div(p.XP, p.W);
            const long ntiles = (long)p.nouter * p.ncoltiles;
            const int grid = (int)std::min<long>(ntiles, ctx->num_cus);
            return launch_lds(ctx, kern, grid, nt, lds, p);
        };
#define BH_COLZ3(LOGL_)                                                                                                       \
    switch (mode) {                                                                                                           \
        case COL_CONV: return run(colz3::colz3_kernel<LOGL_, COL_CONV>, colz3::Geo<LOGL_>::W, colz3::Geo<LOGL_>::NT, colz3::Geo<LOGL_>::LDS_BYTES); \
        case COL_CORR: return run(colz3::colz3_kernel<LOGL_, COL_CORR>, colz3::Geo<LOGL_>::W, colz3::Geo<LOGL_>::NT, colz3::Geo<LOGL_>::LDS_BYTES); \
        default: return run(colz3::colz3_kernel<LOGL_, COL_FILTER>, colz3::Geo<LOGL_>::W, colz3::Geo<LOGL_>::NT, colz3::Geo<LOGL_>::LDS_BYTES);     \
    }
        if (p.N == 384) { BH_COLZ3(7) } else { BH_COLZ3(8) }
#undef BH_COLZ3
    }
    // columns of 256 / 512 / 1024 points: the register-stage kernels (BH_FC_COLW=0 keeps the LDS-stepped ones: A/B switch)
    const cf* colw_tab = zaxis ? pl.colw_z : pl.colw_y;
    // BH_FC_COLW: 0 never, 1 always, 2 the Y passes only, 3 the Z passes only; default (4): the Y passes, and the Z pass for
    // columns of 256 points (one exchange per transform).  Measured (tools/ab_env.sh): the Z pass of 512-point columns pays
    // more for its 8 barriers per tile at 8 wavefronts than it saves in LDS round trips (6.97 against 6.52 ms at config 2;
    // 5.66 ms with the barriers compiled out), the others win.
    const int colw_mode = env_int("BH_FC_COLW", 4);
    const bool colw_axis = colw_mode == 1 || (colw_mode == 2 && !zaxis) || (colw_mode == 3 && zaxis) ||
                           (colw_mode == 4 && (!zaxis || p.N == 256));
    if (colw_tab && (long)p.N * p.row_stride < (1l << 31) && colw_axis && mode != COL_PCC) {
        p.tw = colw_tab;
        return p.N == 1024 ? launch_colw<10>(ctx, p, mode) : (p.N == 512 ? launch_colw<9>(ctx, p, mode) : launch_colw<8>(ctx, p, mode));
    }
    return launch_col_pass(ctx, p, mode);
}

// ---- compact z taps (fftconv_zdirect.inc) ----
// The radius the direct Z pass runs a PSF of z-extent pz at (stage_rl_psf centres it: rows t in [-(pz / 2), pz - 1 - pz / 2]
// are nonzero, an even extent leaves tap +R zero), rounded up to a compiled radius; -1 when the full transfer function is
// needed: a PSF too tall for the taps, a column too short for them, or BH_RL_ZDIRECT=0 (read here, i.e. when a handle is created).
int fftconv_ztaps_radius(const ConvPlan& pl, int64_t pz) {
    if (env_off("BH_RL_ZDIRECT")) return -1;
    const int r = (int)(pz / 2);
    for (int rc : {4, zdirect::RMAX})
        if (r <= rc) return (pl.d.Z > 2 * rc && pl.d.Z >= rc + zdirect::D_RULE) ? rc : -1;
    return -1;
}

template <int R, bool REALQ>
static int launch_zdirect_r(bh_ctx* ctx, const zdirect::Params& p, int mode) {
    const long nwaves = ceil_div(p.ncol, 64);
    const dim3 grid((unsigned)ceil_div(nwaves, zdirect::NT / 64));
    switch (mode) {
        case COL_FILTER: hipLaunchKernelGGL((zdirect::zdirect_kernel<R, COL_FILTER, REALQ>), grid, dim3(zdirect::NT), 0, ctx->stream, p); break;
        case COL_CONV: hipLaunchKernelGGL((zdirect::zdirect_kernel<R, COL_CONV, REALQ>), grid, dim3(zdirect::NT), 0, ctx->stream, p); break;
        default: hipLaunchKernelGGL((zdirect::zdirect_kernel<R, COL_CORR, REALQ>), grid, dim3(zdirect::NT), 0, ctx->stream, p); break;
    }
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

// The Z pass of one R-L convolution (corr = false) or correlation (corr = true): with the taps of radius zr the direct pass
// (zreal: the taps are real, the kernels that drop their imaginary halves), with the full transfer function (zr < 0) the FFT
// Z pass launch_col picks
int launch_rl_z(bh_ctx* ctx, const ConvPlan& pl, bool corr, bool otf_real, int zr, bool zreal, cf* S, const cf* otf) {
    const int mode = otf_real ? COL_FILTER : (corr ? COL_CORR : COL_CONV);
    if (zr < 0) return launch_col(ctx, pl, mode, true, S, otf, 1.f);
    zdirect::Params p;
    p.S = S;
    p.taps = otf;
    p.ncol = (long)pl.d.Y * pl.d.XP;
    p.Z = pl.d.Z;
    BH_REQUIRE(p.Z > 2 * zr && p.Z >= zr + zdirect::D_RULE, "internal: %d z taps on columns of %d", 2 * zr + 1, p.Z);
    switch (zr) {
        case 4: return zreal ? launch_zdirect_r<4, true>(ctx, p, mode) : launch_zdirect_r<4, false>(ctx, p, mode);
        case zdirect::RMAX:
            return zreal ? launch_zdirect_r<zdirect::RMAX, true>(ctx, p, mode) : launch_zdirect_r<zdirect::RMAX, false>(ctx, p, mode);
        default: BH_REQUIRE(false, "internal: no direct Z pass of radius %d", zr);
    }
    return BH_OK;
}

}  // namespace bh
