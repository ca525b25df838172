// Linear warps whose matrix couples z with y / x only weakly (a registration with a small out-of-plane rotation): the z walk of
// affine_zwalk.inc with per-lane source planes.  Included by affine.hip (namespace bh) after affine_zwalk.inc.
//
// A wave owns RY output rows x 64 columns and walks a chunk of output planes.  The source planes it needs — a window of at most
// three, because z' varies by less than one plane over the wave's footprint — sit in a wave-private ring of four LDS slots, each
// holding the plane's box of rows x 16-B quads that covers the wave's taps over the whole chunk (the box drifts by m[1][0] and
// m[2][0] per plane; it is sized for the chunk), filled by 1-KiB global_load_lds_dwordx4 one plane ahead.  Per voxel: the Q32.32
// coordinates advance by three 64-bit adds, the eight taps are four paired LDS reads from the slots of planes iz and iz + 1,
// lerp8 blends them — the staged-tile kernel's interior loop without its tiles, phases and barriers.  Output planes whose
// window leaves the volume, and waves whose box does (or does not fit a slot), take the staged kernel's boundary arithmetic on
// global memory (slow_voxel).  Either way a voxel is lerp8 of the same clamped taps: bit-identical to affine_kernel.
namespace zo {

using zw::QMAX;
using zw::RY;
constexpr int NS = 4;                 // LDS slots (planes) per wave: a window of three + one in flight
constexpr int NW = 4, NT = 64 * NW;   // a workgroup = four y-neighbours, as the z walk

// the staged-tile kernel's boundary loop for one voxel (affine.hip, sample_tile): float64 inside test, clamped taps cleaned on
// load, lerp8 on the Q32.32 fractions
template <typename TIN, int BOUNDARY>
__device__ __forceinline__ float slow_voxel(const TIN* __restrict__ in, const AffineParams& p, int oz, int oy, int ox) {
    long long c0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        c0[a] = p.mq[4 * a] * (long long)(oz + p.cz) + p.mq[4 * a + 1] * (long long)(oy + p.cy) +
                p.mq[4 * a + 2] * (long long)(ox + p.cx) + p.mq[4 * a + 3];
    const int dims[3] = {p.Zi, p.Yi, p.Xi};
    bool inside = true;
    {
#pragma clang fp contract(off)
        const double zd = (double)(oz + p.cz), yd = (double)(oy + p.cy), xd = (double)(ox + p.cx);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ca = p.m[4 * a] * zd + p.m[4 * a + 1] * yd + p.m[4 * a + 2] * xd + p.m[4 * a + 3];
            if (BOUNDARY == BH_BOUNDARY_ITK)
                inside = inside && ca >= -0.5 && ca < (double)dims[a] - 0.5;
            else
                inside = inside && ca >= 0.0 && ca <= (double)(dims[a] - 1);
        }
    }
    if (!inside) return p.cval;
    const int iz = (int)(c0[0] >> 32), iy = (int)(c0[1] >> 32), ix = (int)(c0[2] >> 32);
    const int z0 = max(0, min(iz, p.Zi - 1)), z1 = max(0, min(iz + 1, p.Zi - 1));
    const int y0 = max(0, min(iy, p.Yi - 1)), y1 = max(0, min(iy + 1, p.Yi - 1));
    const int x0 = max(0, min(ix, p.Xi - 1)), x1 = max(0, min(ix + 1, p.Xi - 1));
    const size_t sY = (size_t)p.Xi, sZ = (size_t)p.Yi * p.Xi;
    auto fetch = [&](int z, int y, int x) -> float { return load_clean(in + (size_t)z * sZ + (size_t)y * sY + x); };
    const f2 P0 = {fetch(z0, y0, x0), fetch(z0, y0, x1)};
    const f2 P1 = {fetch(z0, y1, x0), fetch(z0, y1, x1)};
    const f2 P2 = {fetch(z1, y0, x0), fetch(z1, y0, x1)};
    const f2 P3 = {fetch(z1, y1, x0), fetch(z1, y1, x1)};
    return lerp8_clean(P0, P1, P2, P3, (unsigned)c0[0], (unsigned)c0[1], (unsigned)c0[2]);
}

template <typename TIN, int BOUNDARY>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void zoblique_kernel(
    const TIN* __restrict__ in, float* __restrict__ out, AffineParams p, int ntx, int nty, int zchunk, int per_xcd, int nwg,
    int slot_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zo_lds[];
    const int t = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || t >= nwg) return;
    const int zc = t / (ntx * nty), rem = t - zc * (ntx * nty), yg = rem / ntx, xt = rem - yg * ntx;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ox0 = xt * 64, ox = ox0 + lane, oy0 = (yg * NW + wv) * RY;
    if (oy0 >= p.Yo) return;
    const int ka = zc * zchunk, kb = min(ka + zchunk, p.Zo);
    bool store[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) store[r] = ox < p.Xo && oy0 + r < p.Yo;
    auto slow_plane = [&](int k) {
#pragma unroll
        for (int r = 0; r < RY; ++r)
            if (store[r]) out[((size_t)k * p.Yo + oy0 + r) * p.Xo + ox] = slow_voxel<TIN, BOUNDARY>(in, p, k, oy0 + r, ox);
    };
    // the wave's source box in y and x over the whole chunk, and its z window per plane: the coordinates are affine, so their
    // extremes over the footprint sit at its corners (exact in Q32.32)
    auto coord = [&](int a, int k, int oy, int oxc) -> long long {
        return p.mq[4 * a] * (long long)(k + p.cz) + p.mq[4 * a + 1] * (long long)(oy + p.cy) + p.mq[4 * a + 2] * (long long)(oxc + p.cx) +
               p.mq[4 * a + 3];
    };
    long long lo[3], hi[3];
#pragma unroll
    for (int a = 1; a < 3; ++a) {
        lo[a] = hi[a] = coord(a, ka, oy0, ox0);
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            const long long v = coord(a, (c & 4) ? kb - 1 : ka, oy0 + ((c & 1) ? RY - 1 : 0), ox0 + ((c & 2) ? 63 : 0));
            lo[a] = v < lo[a] ? v : lo[a];
            hi[a] = v > hi[a] ? v : hi[a];
        }
    }
    const int by = (int)(lo[1] >> 32), y1 = (int)(hi[1] >> 32) + 1, x0 = (int)(lo[2] >> 32), x1 = (int)(hi[2] >> 32) + 1;
    constexpr int E = 16 / (int)sizeof(TIN);  // samples per 16-B quad (rows are 16-B aligned: Xi % E == 0)
    const int bxq = x0 & ~(E - 1), dx = ((x1 + E) & ~(E - 1)) - bxq, dy = y1 - by + 1;
    const unsigned L = (unsigned)dx / (unsigned)E, S = (unsigned)dy * L;
    if (!(by >= 0 && y1 <= p.Yi - 1 && x0 >= 0 && x1 <= p.Xi - 1 && S * 16u <= (unsigned)slot_bytes)) {
        for (int k = ka; k < kb; ++k) slow_plane(k);  // the box leaves the volume (or a slot): every voxel by the boundary rules
        return;
    }
    const int nq = (int)((S + 63u) >> 6);
    const unsigned slot0 = (unsigned)wv * (unsigned)(NS * slot_bytes), pitch = (unsigned)dx * (unsigned)sizeof(TIN);
    unsigned doff[QMAX];
#pragma unroll
    for (int i = 0; i < QMAX; ++i) {
        const unsigned q = min((unsigned)(i * 64 + lane), S - 1u);
        const unsigned row = q / L, xq = q - row * L;
        doff[i] = (((unsigned)(by + (int)row) * (unsigned)p.Xi + (unsigned)bxq) + (unsigned)E * xq) * (unsigned)sizeof(TIN);
    }
    const size_t sZ = (size_t)p.Yi * p.Xi;
    auto dma_plane = [&](int pz) {  // pz inside the volume
        const TIN* pl = in + (size_t)pz * sZ;
        const unsigned dst = slot0 + (unsigned)(pz & (NS - 1)) * (unsigned)slot_bytes;
#pragma unroll
        for (int i = 0; i < QMAX; ++i)
            if (i < nq && (unsigned)(i * 64 + lane) < S) zw::dma_quad(pl, doff[i], dst + i * 1024u);
    };
    // per-lane coordinates of the wave's rows at plane ka, relative to the box origin in y and x
    long long c[RY][3];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        c[r][0] = coord(0, ka, oy0 + r, ox);
        c[r][1] = coord(1, ka, oy0 + r, ox) - ((long long)by << 32);
        c[r][2] = coord(2, ka, oy0 + r, ox) - ((long long)bxq << 32);
    }
    // the last plane this chunk can need (run-ahead stops there)
    long long zmax = coord(0, kb - 1, oy0, ox0);
#pragma unroll
    for (int cnr = 1; cnr < 4; ++cnr) {
        const long long v = coord(0, kb - 1, oy0 + ((cnr & 1) ? RY - 1 : 0), ox0 + ((cnr & 2) ? 63 : 0));
        zmax = v > zmax ? v : zmax;
    }
    const int pz_last = min((int)(zmax >> 32) + 1, p.Zi - 1);
    int loaded = -0x40000000;  // highest plane requested so far (planes loaded - NS + 1 .. loaded are in the ring)
    for (int k = ka; k < kb; ++k) {
        long long zl = coord(0, k, oy0, ox0), zh = zl;
#pragma unroll
        for (int cnr = 1; cnr < 4; ++cnr) {
            const long long v = coord(0, k, oy0 + ((cnr & 1) ? RY - 1 : 0), ox0 + ((cnr & 2) ? 63 : 0));
            zl = v < zl ? v : zl;
            zh = v > zh ? v : zh;
        }
        const int zlo = __builtin_amdgcn_readfirstlane((int)(zl >> 32)), zhi = __builtin_amdgcn_readfirstlane((int)(zh >> 32));
        if (zlo >= 0 && zhi + 1 <= p.Zi - 1 && zhi + 2 - zlo <= NS - 1) {
            // planes zlo .. zhi + 1 are needed now; request up to zlo + NS - 1 (never a slot that still holds a needed plane)
            if (loaded < zlo - 1) loaded = zlo - 1;
            const int target = min(zlo + NS - 1, pz_last);
            while (loaded < target) {
                ++loaded;
                dma_plane(loaded);
            }
            if (loaded > zhi + 1) zw::wait_planes<1>(nq);  // at most one plane beyond the window is in flight
            else zw::wait_vm<0>();
            const unsigned char* ring = zo_lds + slot0;
            float* oplane = out + ((size_t)k * p.Yo + oy0) * p.Xo;
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                const int iz = (int)(c[r][0] >> 32), iy = (int)(c[r][1] >> 32), ix = (int)(c[r][2] >> 32);
                const unsigned off = (unsigned)(iy * dx + ix) * (unsigned)sizeof(TIN);
                const unsigned char* s0 = ring + (unsigned)(iz & (NS - 1)) * (unsigned)slot_bytes;
                const unsigned char* s1 = ring + (unsigned)((iz + 1) & (NS - 1)) * (unsigned)slot_bytes;
                const f2 P0 = zw::lds_pair<TIN>(s0, off), P1 = zw::lds_pair<TIN>(s0, off + pitch);
                const f2 P2 = zw::lds_pair<TIN>(s1, off), P3 = zw::lds_pair<TIN>(s1, off + pitch);
                float v = lerp8(P0, P1, P2, P3, (unsigned)c[r][0], (unsigned)c[r][1], (unsigned)c[r][2]);
                if (__builtin_expect(!__builtin_isfinite(v), 0))  // a NaN / inf tap: redo on np.nan_to_num'd taps
                    v = lerp8_clean(clean2(P0), clean2(P1), clean2(P2), clean2(P3), (unsigned)c[r][0], (unsigned)c[r][1], (unsigned)c[r][2]);
                if (store[r]) (oplane + (size_t)r * p.Xo)[ox] = v;
            }
        } else {
            slow_plane(k);
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            c[r][0] += p.mq[0];
            c[r][1] += p.mq[4];
            c[r][2] += p.mq[8];
        }
    }
}

// z chunk length and slot size for a matrix, or 0 when this kernel does not take it
static int plan(const AffineParams& p, int64_t* zchunk_out) {
    if (getenv("BH_AFFINE_NOZWALK") || getenv("BH_AFFINE_NOOBLIQUE")) return 0;
    if (p.interp != BH_INTERP_LINEAR || p.boundary == BH_BOUNDARY_ZEROS || !(p.x4 || p.x8) || p.mq[0] <= 0) return 0;
    if ((int64_t)p.Yi * p.Xi * 4 >= (1ll << 32) - 16) return 0;
    // z' must vary by less than one plane over a wave's 64 x RY footprint: a window of three source planes per output plane
    if (std::fabs(p.m[1]) * (RY - 1) + std::fabs(p.m[2]) * 63.0 >= 0.98) return 0;
    const int64_t ntx = ceil_div(p.Xo, 64), nty = ceil_div(p.Yo, RY * NW);
    // chunks for ~128 K waves: shorter chunks than the separable walk's, because the box of a chunk grows with the drift along it
    // and four slots of it decide how many waves fit a CU (64-plane chunks: 4.30 ms at config 2, 128-plane chunks 4.94, staged 4.9)
    const char* we = getenv("BH_ZO_WAVES");
    int64_t nchunk = std::min<int64_t>(ceil_div(we ? atoi(we) : 131072, ntx * nty * NW), ceil_div(p.Zo, 32));
    nchunk = std::max<int64_t>(nchunk, 1);
    const int64_t zchunk = ceil_div(p.Zo, nchunk);
    // the box of a wave over a chunk: footprint + drift along the chunk, whole quads; one slot holds at most QMAX KiB
    const double ey = std::floor((std::fabs(p.m[5]) * (RY - 1) + std::fabs(p.m[6]) * 63.0 + std::fabs(p.m[4]) * (double)(zchunk - 1)) * (1.0 + 1e-6)) + 3.0;
    const double ex = std::floor((std::fabs(p.m[9]) * (RY - 1) + std::fabs(p.m[10]) * 63.0 + std::fabs(p.m[8]) * (double)(zchunk - 1)) * (1.0 + 1e-6)) + 3.0;
    const double E = p.x4 ? 4.0 : 8.0, size = p.x4 ? 4.0 : 2.0;
    const double bytes = ey * (std::floor((ex + 2.0 * (E - 1.0)) / E) * E) * size;
    if (bytes > 1024.0 * QMAX) return 0;
    *zchunk_out = zchunk;
    return ((int)bytes + 15) & ~15;
}

template <typename TIN>
static int launch(bh_ctx* ctx, const TIN* in, float* out, const AffineParams& p, int slot_bytes, int64_t zchunk) {
    const int64_t ntx = ceil_div(p.Xo, 64), nty = ceil_div(p.Yo, RY * NW), nchunk = ceil_div(p.Zo, zchunk);
    const int64_t nwg = ntx * nty * nchunk;
    BH_REQUIRE(nwg < (1ll << 31) - 8, "affine output too large");
    const int per_xcd = (int)ceil_div(nwg, (int64_t)8);
    auto run = [&](auto kern) -> int {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(NT), (size_t)NW * NS * slot_bytes, ctx->stream, in, out, p, (int)ntx, (int)nty,
                           (int)zchunk, per_xcd, (int)nwg, slot_bytes);
        BH_CHECK_HIP(hipGetLastError());
        return BH_OK;
    };
    if (p.boundary == BH_BOUNDARY_ITK) return run(zoblique_kernel<TIN, BH_BOUNDARY_ITK>);
    return run(zoblique_kernel<TIN, BH_BOUNDARY_SCIPY_CONSTANT>);
}

}  // namespace zo
