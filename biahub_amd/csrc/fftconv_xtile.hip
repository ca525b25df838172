// The tile-based X passes of the fused FFT engine (fftconv.hip): real rows <-> half-spectrum rows through an LDS tile.
#include "fftconv_dev.hpp"

namespace bh {

// The X passes exist for two tile heights: 16 rows (M = X/2 up to 1024) and 8 rows (M up to 1536: a 3072-voxel row, for which
// 16 rows of LDS do not fit).  Same spectrum layout either way — the tile height only groups rows.
namespace xr16 {
#define BH_XP_XR BH_FC_XR
#define BH_XP_XNT BH_FC_XNT
#include "fftconv_xpass.inc"
#undef BH_XP_XR
#undef BH_XP_XNT
}  // namespace xr16
namespace xr8 {
#define BH_XP_XR 8
#define BH_XP_XNT BH_FC_XNT8
#include "fftconv_xpass.inc"
#undef BH_XP_XR
#undef BH_XP_XNT
}  // namespace xr8

int launch_x_tile(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out, const float* aux,
                  float eps, bool fuse_fwd) {
    return pl.xr == 8 ? xr8::launch_x(ctx, pl, inverse, epi, in, S, out, aux, eps, fuse_fwd)
                      : xr16::launch_x(ctx, pl, inverse, epi, in, S, out, aux, eps, fuse_fwd);
}

}  // namespace bh
