// Fused 3-D real FFT convolution engine for gfx950 (power-of-two volumes) — the Richardson-Lucy hot loop.
//
// hipFFT runs a 3-D R2C/C2R of a 512x2048x2048 volume as 5-7 kernels (row FFTs + transposes + a slow
// strided z kernel), and every pointwise step between transforms is one more pass over HBM:
// ~29 ms forward + ~23 ms inverse + 4 x 5.4 ms pointwise per convolution pair (profiles/r01a_*).
// A convolution does not need the spectrum in natural order or natural layout, only a forward and an
// inverse that agree with the transformed kernel (OTF).  So this engine
//   * runs each axis as ONE in-place pass (no transposes), leaving every axis in the scrambled order its
//     decimation-in-frequency FFT produces (bit-reversed; Y additionally split even/odd by a radix-2 step
//     that is folded into the X pass so the Y pass fits LDS with 128-B row segments);
//   * fuses forward-Z, the OTF multiply and inverse-Z into one kernel (a tile is loaded once);
//   * fuses the real<->complex packing, and Richardson-Lucy's divide / multiply-clip, into the X passes.
// One convolution = 5 passes, 48 B/voxel of HBM traffic (two per R-L iteration: 96 B/voxel, against the
// 112 B/voxel of the 3-pass-per-FFT model and ~260 B/voxel measured for the hipFFT path).
//
// Layout of the half spectrum: S[z][y][p], p in [0, XP), XP = X/2 + 16 complex per row (128-B aligned
// column tiles; column X/2 holds the Nyquist bin, the remaining pad columns stay zero).
//
// Each pass is a persistent kernel (one 1024-thread workgroup per CU) that walks 128-KiB tiles:
// registers prefetch tile t+1 from HBM while the FFT of tile t runs out of LDS.
//
// This file holds the plans, the staging kernels and the drivers.  The kernels live in one translation unit per family, each
// with its launcher (fftconv_col.hip, fftconv_xtile.hip, fftconv_xw.hip, fftconv_colreg.hip); fftconv_dev.hpp is what they
// share, fftconv.hpp what the rest of the library sees.
#include "fftconv_dev.hpp"
#include "tune_rule.hpp"

#include <chrono>
#include <mutex>

namespace bh {

// rows per X-pass tile for a row length: the configured height while its LDS tile fits, 8 rows beyond M = 1024
static int x_tile_rows(int64_t X) { return X / 2 > 1024 ? 8 : BH_FC_XR; }

// Shapes the engine runs: every axis a power of two or — `radix3` — three or five times one (rows and columns then start
// with a radix-3 / radix-5 step).  Every caller asks with `radix3` today: Richardson-Lucy and phase correlation are
// order-agnostic, and the staging kernels that write a natural-order transfer function into the scrambled coefficient order
// (tikhonov_filter_rows_kernel, inverse_filter_rows_kernel: bh_tikhonov, bh_inverse_filter) compute the stored position of
// 3 * 2^k and 5 * 2^k axes too.  Without it (fftconv_supported; BH_FC_NORADIX3 for Richardson-Lucy) only powers of two pass.
bool fftconv_supported_ex(int64_t Z, int64_t Y, int64_t X, bool radix3) {
    auto pow2 = [](int64_t v) { return v > 0 && (v & (v - 1)) == 0; };
    auto ok = [&](int64_t v) { return pow2(v) || (radix3 && ((v % 3 == 0 && pow2(v / 3)) || (v % 5 == 0 && pow2(v / 5)))); };
    if (!ok(Z) || !ok(Y) || !ok(X)) return false;
    if (X < 64 || X > 3072) return false;          // M = X/2 in [32, 1536]: (M+1)*(rows+1)*8 + tables <= 160 KiB
    if (!pow2(X) && X / 2 / (X % 3 == 0 ? 3 : 5) < 32) return false;  // rows of 3 * 2^k / 5 * 2^k: parts of at least 32 complex points
    if (X / 4 > (X / 2 > 1024 ? BH_FC_XNT8 : BH_FC_XNT)) return false;  // an X-pass thread owns two complex columns of a row
    if (Y < 2 * 16 || Y / 2 > 2048) return false;   // Y/2 rows x >= 8 columns per tile, whole groups of tile rows
    if (Z < 4 || Z > 2048) return false;
    const int xr = x_tile_rows(X);
    if ((Y % xr) != 0) return false;
    if (!pow2(Z) && Z / (Z % 3 == 0 ? 3 : 5) < 8) return false;        // odd-radix columns: parts of at least 8 rows
    if (!pow2(Y) && Y / 2 / (Y % 3 == 0 ? 3 : 5) < 16) return false;
    const int M = (int)X / 2, Lm = pow2(X) ? M : (X % 3 == 0 ? M / 3 : M / 5);
    const size_t xlds = (size_t)(M + 1) * (xr + 1) * 8 + (size_t)twiddle_count(Lm) * 8 + (size_t)M * 8 + (Lm != M ? (size_t)(M / Lm - 1) * Lm * 8 : 0);
    return xlds <= 160 * 1024;
}

bool fftconv_supported(int64_t Z, int64_t Y, int64_t X) { return fftconv_supported_ex(Z, Y, X, false); }

static std::map<std::tuple<int, int64_t, int64_t, int64_t>, ConvPlan> g_plans;  // twiddle tables per (device, shape): a few KiB, never freed
static std::mutex g_plans_mu;                                                    // contexts of different threads share the cache

static int upload(const std::vector<cf>& h, cf** dptr) {
    BH_CHECK_HIP(hipMalloc(dptr, h.size() * sizeof(cf) + 16));
    BH_CHECK_HIP(hipMemcpy(*dptr, h.data(), h.size() * sizeof(cf), hipMemcpyHostToDevice));
    return BH_OK;
}

// THE predicate for "rows of X voxels (Y of them per plane) run the wave-private X passes": what fftconv_plan enables, and what
// the box chooser (engine_pad_box) and the back-end cost model (rl_plan) of deconv.hip assume when they prefer rows of
// 1536 / 3072 voxels or price a wrap-padded iteration.
// BH_FC_XW=0 keeps the tile-based X passes for every shape (A/B switch, read per call: plans of both kinds can coexist)
// rows of 512 / 1024 / 2048 voxels: fftconv_xw.inc; of 1536 / 3072: fftconv_x3.inc (BH_FC_X3=0 keeps those on the tile kernels)
bool fftconv_rows_wave_private(int64_t Y, int64_t X) {
    const bool x3_rows = (X == 1536 || X == 3072) && !env_off("BH_FC_X3");
    return !env_off("BH_FC_XW") && (X == 512 || X == 1024 || X == 2048 || x3_rows) && ((Y / 2) % 4) == 0;
}

int fftconv_plan(bh_ctx* ctx, int64_t Z, int64_t Y, int64_t X, ConvPlan** out) {
    std::lock_guard<std::mutex> lock(g_plans_mu);
    const bool xw_on = fftconv_rows_wave_private(Y, X);
    auto key = std::make_tuple(ctx->device * 2 + (xw_on ? 1 : 0), Z, Y, X);
    auto it = g_plans.find(key);
    if (it != g_plans.end()) {
        *out = &it->second;
        return BH_OK;
    }
    ConvPlan pl;
    pl.d.Z = (int)Z;
    pl.d.Y = (int)Y;
    pl.d.X = (int)X;
    pl.d.M = (int)X / 2;
    pl.d.XP = (int)X / 2 + 16;
    auto pow2part = [](int64_t n) { return (int)((n & (n - 1)) == 0 ? n : (n % 3 == 0 ? n / 3 : n / 5)); };
    pl.Lyh = pow2part(Y / 2);
    pl.Lz = pow2part(Z);
    pl.xr = x_tile_rows(X);
    pl.d.Lm = pow2part(X / 2);
    pl.d.logM = ilog2(pl.d.Lm);
    pl.d.logYh = ilog2(pl.Lyh);
    pl.d.logZ = ilog2(pl.Lz);
    pl.d.Lyh = pl.Lyh;
    pl.d.Lz = pl.Lz;
    std::vector<cf> h;
    make_twiddles(pl.d.Lm, h);
    pl.ntw_x = (int)h.size();
    BH_TRY(upload(h, &pl.tw_x));
    make_twiddles(pl.Lyh, h);
    pl.ntw_y = (int)h.size();
    BH_TRY(upload(h, &pl.tw_y));
    make_twiddles(pl.Lz, h);
    pl.ntw_z = (int)h.size();
    BH_TRY(upload(h, &pl.tw_z));
    auto radix3_twiddles = [&](int n, int L, cf** dptr) -> int {  // [w_n^(k m), k = 1 .. r - 1], m < L = n / r, r = 3 or 5
        if (L == n) return BH_OK;
        const int r = n / L;
        h.resize((size_t)(r - 1) * L);
        for (int m = 0; m < L; ++m)
            for (int k = 1; k < r; ++k) {
                const double a = -2.0 * M_PI * (double)m * k / (double)n;
                h[(size_t)(r - 1) * m + k - 1] = make_float2((float)std::cos(a), (float)std::sin(a));
            }
        return upload(h, dptr);
    };
    BH_TRY(radix3_twiddles((int)Y / 2, pl.Lyh, &pl.tw3_y));
    BH_TRY(radix3_twiddles((int)Z, pl.Lz, &pl.tw3_z));
    BH_TRY(radix3_twiddles(pl.d.M, pl.d.Lm, &pl.tw3_x));
    h.resize(pl.d.M);
    for (int pp = 0; pp < pl.d.M; ++pp) {
        // frequency stored at position pp: bit-reversed within the (single, or one of three) length-Lm transform(s)
        const int third = pp / pl.d.Lm, r = pp % pl.d.Lm;
        int k = 0;
        for (int b = 0; b < pl.d.logM; ++b)
            if (r & (1 << b)) k |= 1 << (pl.d.logM - 1 - b);
        if (pl.d.Lm != pl.d.M) k = (pl.d.M / pl.d.Lm) * k + third;
        const double a = -2.0 * M_PI * k / (double)X;
        h[pp] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    BH_TRY(upload(h, &pl.untangle));
    h.resize(Y / 2);
    for (int y = 0; y < (int)Y / 2; ++y) {
        const double a = -2.0 * M_PI * y / (double)Y;
        h[y] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    BH_TRY(upload(h, &pl.twy));
    auto tile_w = [&](int64_t N) {
        int w = 1;
        while (2 * w * N <= FC_TILE) w *= 2;  // widest power-of-two tile of N rows in 128 KiB
        if (w > 64) w = 64;       // 512-B row segments are plenty
        if (w > pl.d.XP) w = 16;
        return w < 2 ? 2 : w;
    };
    pl.Wy = tile_w(Y / 2);
    pl.Wz = tile_w(Z);
    if (colw_tables(Y / 2, h)) BH_TRY(upload(h, &pl.colw_y));
    if (colw_tables(Z, h)) BH_TRY(upload(h, &pl.colw_z));
    if (colz_tables(pl.d, h)) BH_TRY(upload(h, &pl.colz));
    if (colz3_tables(pl.d, h)) BH_TRY(upload(h, &pl.colz3));
    if (xw_on) {
        std::vector<int> col;
        xw_tables(X, h, col);
        pl.x3 = X == 3072 || X == 1536;
        BH_TRY(upload(h, &pl.xw_tab));
        BH_CHECK_HIP(hipMalloc(&pl.xw_col, col.size() * sizeof(int)));
        BH_CHECK_HIP(hipMemcpy(pl.xw_col, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice));
        pl.xw = true;
    }
    auto ins = g_plans.emplace(key, pl);
    *out = &ins.first->second;
    return BH_OK;
}

int fftconv_plan_tag(const ConvPlan& pl) { return pl.xw ? 1 : 0; }
// the last update pass of the next fftconv_richardson_lucy leaves the float64 row sums of its result at `dst` (wave-private X
// passes of 512 / 1024 / 2048-voxel rows only); fftconv_rowsums_taken says whether a pass did, and disarms the plan
void fftconv_arm_rowsums(ConvPlan& pl, double* dst) {
    pl.rl_rowsums = dst;
    pl.rl_rowsums_done = false;
}
bool fftconv_rowsums_taken(ConvPlan& pl) {
    const bool done = pl.rl_rowsums_done;
    pl.rl_rowsums = nullptr;
    pl.rl_rowsums_done = false;
    return done;
}

size_t fftconv_spectrum_elems(const ConvPlan& pl) {
    return (size_t)pl.d.Z * pl.d.Y * pl.d.XP + 64;  // slack: a ragged last column tile reads past its row
}

static int launch_x(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out,
                    const float* aux, float eps, bool fuse_fwd = false) {
    if (pl.xw) return launch_xw(ctx, pl, inverse, epi, in, S, out, aux, eps, fuse_fwd);
    return launch_x_tile(ctx, pl, inverse, epi, in, S, out, aux, eps, fuse_fwd);
}

// OTF (scrambled order, scaled by 2/V so that forward -> multiply -> inverse is a normalised convolution)
int fftconv_make_otf(bh_ctx* ctx, const ConvPlan& pl, const float* padded_psf, cf* otf) {
    const double V = (double)pl.d.Z * pl.d.Y * pl.d.X;
    BH_TRY(launch_x(ctx, pl, false, 0, padded_psf, otf, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, otf, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD_SCALE, true, otf, nullptr, (float)(2.0 / V)));
    return BH_OK;
}

// complex elements of the taps of radius R: R + 1 Hermitian planes or 2R + 1 general ones, each one z-row of the spectrum
size_t fftconv_ztaps_elems(const ConvPlan& pl, int R, bool hermitian) {
    return (size_t)(hermitian ? R + 1 : 2 * R + 1) * pl.d.Y * pl.d.XP;
}

// taps from Q = the PSF transformed along x and y (z natural), scaled by 2 Z / V: the factor fftconv_make_otf puts in H (2 / V)
// times the Z of the unnormalised inverse Z transform the direct pass no longer runs.  Hermitian: t = 0..R as
// (Q(t) + conj(Q(-t))) / 2 — exactly the taps whose transform is Re(H), the real transfer function of the FFT path.
// zreal: Q is real (rl_probe_psf), the imaginary halves the transforms leave are round-off and are written as zero; the planes
// keep their layout, the real-tap kernels of the direct pass read the real halves only.
__global__ void ztaps_extract_kernel(const cf* __restrict__ Q, cf* __restrict__ taps, long ncol, int Z, int R, int hermitian, int zreal,
                                     float scale) {
    const int nq = hermitian ? R + 1 : 2 * R + 1;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)nq * ncol; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i / ncol);
        const long j = i - (long)k * ncol;
        cf v;
        if (hermitian) {
            const cf a = Q[(long)k * ncol + j], b = Q[(long)((Z - k) % Z) * ncol + j];
            v = make_float2(0.5f * (a.x + b.x) * scale, 0.5f * (a.y - b.y) * scale);
        } else {
            const int t = k - R;
            v = cscale(Q[(long)((t + Z) % Z) * ncol + j], scale);
        }
        if (zreal) v.y = 0.f;
        taps[i] = v;
    }
}

// `work`: a spectrum-sized scratch (fftconv_spectrum_elems), overwritten
int fftconv_make_ztaps(bh_ctx* ctx, const ConvPlan& pl, const float* padded_psf, bool hermitian, bool zreal, int R, cf* work, cf* taps) {
    const double V = (double)pl.d.Z * pl.d.Y * pl.d.X;
    const long ncol = (long)pl.d.Y * pl.d.XP;
    BH_TRY(launch_x(ctx, pl, false, 0, padded_psf, work, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, work, nullptr, 1.f));
    const long n = (long)(hermitian ? R + 1 : 2 * R + 1) * ncol;
    hipLaunchKernelGGL(ztaps_extract_kernel, dim3((unsigned)std::min<long>(ceil_div(n, 256), 65535)), dim3(256), 0, ctx->stream, work,
                       taps, ncol, pl.d.Z, R, hermitian ? 1 : 0, zreal ? 1 : 0, (float)(2.0 * pl.d.Z / V));
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

// out = epilogue( irfft( rfft(in) * OTF or conj(OTF) ) )
int fftconv_apply(bh_ctx* ctx, const ConvPlan& pl, const float* in, const cf* otf, bool correlate, cf* spec,
                  int epilogue, const float* aux, float eps, float* out) {
    BH_TRY(launch_x(ctx, pl, false, 0, in, spec, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, correlate ? COL_CORR : COL_CONV, true, spec, otf, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, epilogue, nullptr, spec, out, aux, eps));
    return BH_OK;
}


// Tikhonov filter H/(H^2 + reg) * 2/V from the reference's natural-order full-spectrum H, written in the
// engine's scrambled half-spectrum layout.  One workgroup per spectrum row: coalesced read of tf[kz][ky][0..M],
// bit-reversal permutation through LDS, coalesced write of filt[zs][ys][0..XP).
__global__ __launch_bounds__(256) void tikhonov_filter_rows_kernel(const float* __restrict__ tf, float* __restrict__ filt,
                                                                   ConvDims d, float reg, float scale,
                                                                   const int* __restrict__ xcol) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];  // [XP]
    constexpr int PT = 8;  // columns per thread: XP <= 2048 (X <= 3072: XP = 1552)
    const int Yh = d.Y / 2;
    // a thread's columns kx = tid + 256 j and where they go in the stored row do not depend on the row
    int ps[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int kx = threadIdx.x + 256 * j;
        int q = kx;  // Nyquist and pad columns keep their place
        if (kx < d.M) {
            const int rx = d.M / d.Lm, jx = kx / rx, tx = kx - rx * jx;
            q = tx * d.Lm + (int)(__brev((unsigned)jx) >> (32 - d.logM));
            if (xcol) q = xcol[q];  // the wave-private X passes store position q in column xcol[q]
        }
        ps[j] = kx < d.XP ? q : -1;
    }
    auto source_row = [&](long row) -> const float* {
        const int zs = (int)(row / d.Y), ys = (int)(row - (long)zs * d.Y);
        // stored position -> frequency: a 3 * 2^k column holds X[3 j + t] in third t at the bit-reversed j
        const int tz = zs / d.Lz, rz = zs - tz * d.Lz;
        const int jz = (int)(__brev((unsigned)rz) >> (32 - d.logZ));
        const int kz = (d.Z / d.Lz) * jz + tz;  // Z / Lz = 1, 3 or 5: frequency r j + t sits in part t at the bit-reversed j
        const int half = ys / Yh, r = ys - half * Yh;
        const int ty = r / d.Lyh, ry = r - ty * d.Lyh;
        const int jy = (int)(__brev((unsigned)ry) >> (32 - d.logYh));
        const int ky = 2 * ((Yh / d.Lyh) * jy + ty) + half;
        return tf + ((long)kz * d.Y + ky) * d.X;
    };
    const long nrows = (long)d.Z * d.Y;
    float h[PT];
    auto load_row = [&](long row) {  // unconditional, clamped: the values of columns past M are not used
        const float* src = source_row(row < nrows ? row : nrows - 1);
#pragma unroll
        for (int j = 0; j < PT; ++j) h[j] = src[min((int)threadIdx.x + 256 * j, d.M)];
    };
    long row = blockIdx.x;
    if (row < nrows) load_row(row);
    for (; row < nrows; row += gridDim.x) {
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int kx = threadIdx.x + 256 * j;
            if (ps[j] >= 0) rowbuf[ps[j]] = kx <= d.M ? (h[j] / (h[j] * h[j] + reg)) * scale : 0.0f;
        }
        load_row(row + gridDim.x);  // the next row travels behind this row's permutation and store
        __syncthreads();
        float4* dst = reinterpret_cast<float4*>(filt + row * d.XP);  // XP % 4 == 0, rows 16-B aligned
        for (int q = threadIdx.x; q < d.XP / 4; q += 256) dst[q] = reinterpret_cast<const float4*>(rowbuf)[q];
        __syncthreads();
    }
}

// Inverse filter of a general transfer function H (natural order, full spectrum (Z, Y, X), complex64 or float32), staged in
// the engine's scrambled half-spectrum layout:  F = conj(H) / (|H|^2 + reg) * scale.  The real part of ifftn(fftn(x) F) is
// what the reference keeps (waveorder: `.real` of the filtered inverse transform), i.e. only the Hermitian part
// F_h(k) = (F(k) + conj(F(-k))) / 2 acts on a real volume — that is what a half-spectrum product can and does apply.
// One workgroup per stored spectrum row; `bf16`: the staged value is rounded to bfloat16 pairs (round to nearest even).
__device__ __forceinline__ unsigned int f32_to_bf16_bits(float f) {
    const unsigned int u = __float_as_uint(f);
    if ((u & 0x7f800000u) == 0x7f800000u) return u >> 16;  // inf / nan: truncate (a quiet-nan payload bit survives)
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
template <bool CPLX>
__global__ __launch_bounds__(256) void inverse_filter_rows_kernel(const void* __restrict__ tf, void* __restrict__ filt,
                                                                  ConvDims d, float reg, float scale, int bf16,
                                                                  const int* __restrict__ xcol) {
    extern __shared__ cf rowc[];  // [XP]
    const int Yh = d.Y / 2;
    for (long row = blockIdx.x; row < (long)d.Z * d.Y; row += gridDim.x) {
        const int zs = (int)(row / d.Y), ys = (int)(row - (long)zs * d.Y);
        const int tz = zs / d.Lz, rz = zs - tz * d.Lz;
        const int kz = (d.Z / d.Lz) * (int)(__brev((unsigned)rz) >> (32 - d.logZ)) + tz;
        const int half = ys / Yh, r = ys - half * Yh;
        const int ty = r / d.Lyh, ry = r - ty * d.Lyh;
        const int ky = 2 * ((Yh / d.Lyh) * (int)(__brev((unsigned)ry) >> (32 - d.logYh)) + ty) + half;
        const int mz = kz ? d.Z - kz : 0, my = ky ? d.Y - ky : 0;  // -k
        const long src = ((long)kz * d.Y + ky) * d.X, msrc = ((long)mz * d.Y + my) * d.X;
        for (int kx = threadIdx.x; kx < d.XP; kx += 256) {
            cf f = make_float2(0.f, 0.f);
            if (kx <= d.M) {
                const int mx = kx ? d.X - kx : 0;
                cf h, hm;
                if (CPLX) {
                    h = reinterpret_cast<const cf*>(tf)[src + kx];
                    hm = reinterpret_cast<const cf*>(tf)[msrc + mx];
                } else {
                    h = make_float2(reinterpret_cast<const float*>(tf)[src + kx], 0.f);
                    hm = make_float2(reinterpret_cast<const float*>(tf)[msrc + mx], 0.f);
                }
                const float q = 1.0f / (h.x * h.x + h.y * h.y + reg), qm = 1.0f / (hm.x * hm.x + hm.y * hm.y + reg);
                // F(k) = conj(h) q ; conj(F(-k)) = hm qm
                f = make_float2(0.5f * (h.x * q + hm.x * qm) * scale, 0.5f * (-h.y * q + hm.y * qm) * scale);
            }
            int ps = kx;  // Nyquist and pad columns keep their place
            if (kx < d.M) {
                const int rx = d.M / d.Lm, jx = kx / rx, tx = kx - rx * jx;
                ps = tx * d.Lm + (int)(__brev((unsigned)jx) >> (32 - d.logM));
                if (xcol) ps = xcol[ps];
            }
            rowc[ps] = f;
        }
        __syncthreads();
        for (int ps = threadIdx.x; ps < d.XP; ps += 256) {
            const cf f = rowc[ps];
            if (bf16)
                reinterpret_cast<unsigned int*>(filt)[row * d.XP + ps] = f32_to_bf16_bits(f.x) | (f32_to_bf16_bits(f.y) << 16);
            else
                reinterpret_cast<cf*>(filt)[row * d.XP + ps] = f;
        }
        __syncthreads();
    }
}

// filt: NS complex (f32) or NS 32-bit words (bf16 pairs), NS = fftconv_spectrum_elems
int fftconv_stage_inverse_filter(bh_ctx* ctx, const ConvPlan& pl, const void* tf, bool tf_complex, float reg, bool bf16,
                                 void* filt) {
    const double V = (double)pl.d.Z * pl.d.Y * pl.d.X;
    const int grid = ctx->num_cus * 8;
    const int* xcol = pl.xw ? pl.xw_col : nullptr;
    if (tf_complex)
        hipLaunchKernelGGL(inverse_filter_rows_kernel<true>, dim3(grid), dim3(256), pl.d.XP * sizeof(cf), ctx->stream, tf, filt,
                           pl.d, reg, (float)(2.0 / V), bf16 ? 1 : 0, xcol);
    else
        hipLaunchKernelGGL(inverse_filter_rows_kernel<false>, dim3(grid), dim3(256), pl.d.XP * sizeof(cf), ctx->stream, tf, filt,
                           pl.d, reg, (float)(2.0 / V), bf16 ? 1 : 0, xcol);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

// whether fftconv_apply_staged_filter can take the x / mean - 1 normalisation into its first pass
bool fftconv_fuses_normalisation(const ConvPlan& pl) { return pl.xw; }

// out = irfft( rfft(in) * staged filter ): 5 passes, the product rides in the Z pass.  norm_mean (device, may be null; only
// when fftconv_fuses_normalisation): the forward X pass transforms in / *norm_mean - 1.
int fftconv_apply_staged_filter(bh_ctx* ctx, const ConvPlan& pl, const float* in, const void* filt, bool bf16, cf* spec,
                                float* out, const double* norm_mean) {
    if (norm_mean) {
        BH_REQUIRE(pl.xw, "internal: fused normalisation needs the wave-private X passes");
        BH_TRY(launch_xw(ctx, pl, false, 0, in, spec, nullptr, nullptr, 0.f, false, norm_mean));
    } else
    BH_TRY(launch_x(ctx, pl, false, 0, in, spec, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, bf16 ? COL_CONV16 : COL_CONV, true, spec, reinterpret_cast<const cf*>(filt), 1.f));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, XE_STORE, nullptr, spec, out, nullptr, 0.f));
    return BH_OK;
}

// Richardson-Lucy iterations with the X passes of consecutive convolutions fused:
//   S = Xfwd(est);  repeat { Y, Z*OTF, Yinv ; [Xinv -> d/max(.,eps) -> Xfwd] ; Y, Z*conj(OTF), Yinv ;
//                            [Xinv -> est = max(est*.,0) (stored) -> Xfwd] }   (last iteration: no trailing Xfwd)
// 8 passes and 84 B/voxel per iteration instead of 10 passes and 96 B/voxel.
// `est` is output only: the first pass fills it with max(d, 0).
// zr >= 0: `otf` holds the compact z taps of that radius (fftconv_make_ztaps) and the Z passes are direct convolutions;
// zreal: those taps are real (their imaginary halves were written as zero) and the real-tap kernels run.
int fftconv_richardson_lucy(bh_ctx* ctx, const ConvPlan& pl, const float* d, const cf* otf, bool otf_real, int zr, bool zreal, cf* spec,
                            int iterations, float eps, float* est) {
    if (iterations <= 0) return BH_OK;
    // otf_real: `otf` holds one float per bin (the transfer function of a point-symmetric PSF); convolution and correlation
    // are then the same real product
    BH_TRY(launch_x(ctx, pl, false, 0, d, spec, est, nullptr, 0.f));  // est = max(d, 0) written by the same pass
    for (int it = 0; it < iterations; ++it) {
        BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
        BH_TRY(launch_rl_z(ctx, pl, false, otf_real, zr, zreal, spec, otf));
        BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
        BH_TRY(launch_x(ctx, pl, true, XE_RATIO, nullptr, spec, nullptr, d, eps, true));
        BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
        BH_TRY(launch_rl_z(ctx, pl, true, otf_real, zr, zreal, spec, otf));
        BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
        BH_TRY(launch_x(ctx, pl, true, XE_UPDATE, nullptr, spec, est, est, eps, it + 1 < iterations));
    }
    return BH_OK;
}

// Where the driver puts the spectrum matters to the passes that stream it.  A process's R-L iteration lands on one of two levels
// (profiles/zdirect_real_taps_ab.txt, r04ai_box_state_ab.txt: Y pass 2.99 or 3.50 ms, Z +8 %, the X passes +8-11 %), and most of
// the difference sits in the passes that touch nothing but the spectrum.  So a new spectrum allocation is auditioned once: the
// launches that touch only the candidate (Y forward, the Z pass of the plan, Y inverse) run twice on the zero-filled block, the
// second repetition is its time, and further candidates are drawn and HELD AT THE SAME TIME (so that the driver hands out other
// physical chunks) until the rule of tune_rule.hpp says stop; the fastest stays, the others are freed.  What profiles/
// spectrum_audition.txt measured of it (levels, share of slow draws, cost) is in DESIGN.md 2.
//   BH_FC_TUNE_ALLOC=0 / 1   never / always audition (the default is kTuneDefaultOn below)
//   BH_FC_TUNE_MIN_VOXELS=n  smallest volume that is auditioned (default 2^28: below it the passes run out of the caches)
//   BH_DEBUG_SCRATCH=1       one "[bh tune]" line per audition: every candidate's time and the choice
//   BH_FC_TUNE_SURVEY=1      measurement only: no early stop, the fused update X pass timed as well (it reads and writes `est`),
//                            every launch printed per candidate, and three more blocks that are never kept: two with the same
//                            permutation seed (they differ in their physical chunks only) and one of 16-MiB chunks
// A candidate is drawn only while free memory after it stays at least twice its size (the result and the deskew output are
// still to be allocated in the same step).  A failed allocation ends the draws with its error cleared; a failed probe ends
// them and is returned, after the best candidate so far took the block's place.
// `est` is any V-float buffer the caller is about to overwrite, `bytes` the allocation size, `otf` ... `zreal` what the
// iteration's Z pass will be launched with.
constexpr int kTuneDefaultOn = 1;
int fftconv_tune_spectrum(bh_ctx* ctx, const ConvPlan& pl, const cf* otf, bool otf_real, int zr, bool zreal, float* est, size_t bytes,
                          cf** spec) {
    const double V = (double)pl.d.Z * pl.d.Y * pl.d.X;
    const char* min_env = getenv("BH_FC_TUNE_MIN_VOXELS");
    const double min_voxels = min_env ? atof(min_env) : (double)(1u << 28);
    const bool survey = env_int("BH_FC_TUNE_SURVEY", 0) != 0;
    // pl.xw: every shape the audition was measured on runs the wave-private X passes
    if (!pl.xw || V < min_voxels || env_int("BH_FC_TUNE_ALLOC", kTuneDefaultOn) == 0) return BH_OK;
    struct Events {
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t ev : e)
                if (ev) (void)hipEventDestroy(ev);
        }
    } ev;
    for (hipEvent_t& e : ev.e) BH_CHECK_HIP(hipEventCreate(&e));
    struct Probe {
        float t[4] = {0.f, 0.f, 0.f, 0.f};  // Y forward, Z, Y inverse, fused update X (survey only)
        float ms() const { return t[0] + t[1] + t[2]; }
    };
    hipStream_t st = ctx->stream;
    auto probe = [&](cf* s, Probe* p) -> int {
        BH_CHECK_HIP(hipMemsetAsync(s, 0, bytes, st));
        for (int rep = 0; rep < 2; ++rep) {  // the second repetition is the measurement
            BH_CHECK_HIP(hipEventRecord(ev.e[0], st));
            BH_TRY(launch_col(ctx, pl, COL_FWD, false, s, nullptr, 1.f));
            BH_CHECK_HIP(hipEventRecord(ev.e[1], st));
            BH_TRY(launch_rl_z(ctx, pl, false, otf_real, zr, zreal, s, otf));
            BH_CHECK_HIP(hipEventRecord(ev.e[2], st));
            BH_TRY(launch_col(ctx, pl, COL_INV, false, s, nullptr, 1.f));
            BH_CHECK_HIP(hipEventRecord(ev.e[3], st));
            if (survey) BH_TRY(launch_x(ctx, pl, true, XE_UPDATE, nullptr, s, est, est, 1e-6f, true));
            BH_CHECK_HIP(hipEventRecord(ev.e[4], st));
            BH_CHECK_HIP(hipEventSynchronize(ev.e[4]));
            for (int k = 0; k < 4; ++k) BH_CHECK_HIP(hipEventElapsedTime(&p->t[k], ev.e[k], ev.e[k + 1]));
        }
        return BH_OK;
    };
    auto room_for_one_more = [&]() {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return free_b >= 3 * bytes;
    };
    const auto t_begin = std::chrono::steady_clock::now();
    TuneRule rule = kTuneRuleDefault;
    if (survey) rule = {6, 0.f};  // six candidates, and no second level is ever "seen": all of them are drawn
    constexpr int NC = 16;
    if (rule.max_candidates > NC) rule.max_candidates = NC;
    cf* cand[NC] = {*spec};
    float ms[NC] = {0.f};
    Probe pr[NC];
    int n = 0, rc = BH_OK;
    TuneDecision dec = {false, 0};
    while (!dec.stop) {
        if (n > 0) {  // candidate 0 is the allocation the caller came with
            if (!room_for_one_more()) break;
            if (dev_alloc(ctx->device, bytes, (void**)&cand[n]) != hipSuccess) {
                (void)hipGetLastError();
                cand[n] = nullptr;
                ms[n++] = 0.f;  // a candidate without a time: the rule stops on it
                dec = tune_decide(rule, ms, n);
                break;
            }
        }
        rc = probe(cand[n], &pr[n]);
        ms[n] = rc == BH_OK ? pr[n].ms() : 0.f;
        ++n;
        dec = tune_decide(rule, ms, n);
        if (rc != BH_OK) break;
    }
    const bool debug = getenv("BH_DEBUG_SCRATCH") != nullptr;
    if (survey && debug && rc == BH_OK) {
        for (int i = 0; i < n; ++i)
            if (cand[i])
                fprintf(stderr, "[bh tune survey] #%d Y fwd %.3f  Z %.3f  Y inv %.3f  update X %.3f ms  (%s)\n", i, pr[i].t[0], pr[i].t[1],
                        pr[i].t[2], pr[i].t[3], i ? "drawn" : "the caller's");
        if (dev_block_is_vmm(cand[0])) {
            const struct { size_t chunk; const char* what; } extra[3] = {{(size_t)2 << 20, "2-MiB chunks, seed 12345"},
                                                                          {(size_t)2 << 20, "2-MiB chunks, seed 12345 again: other chunks only"},
                                                                          {(size_t)16 << 20, "16-MiB chunks, seed 12345"}};
            cf* xb[3] = {nullptr, nullptr, nullptr};
            for (int i = 0; i < 3 && rc == BH_OK && room_for_one_more(); ++i) {
                if (dev_alloc_variant(ctx->device, bytes, extra[i].chunk, 12345, (void**)&xb[i]) != hipSuccess) {
                    (void)hipGetLastError();
                    xb[i] = nullptr;
                    break;
                }
                Probe p;
                if ((rc = probe(xb[i], &p)) == BH_OK)
                    fprintf(stderr, "[bh tune survey] +%d Y fwd %.3f  Z %.3f  Y inv %.3f  update X %.3f ms  (%s)\n", i, p.t[0], p.t[1], p.t[2],
                            p.t[3], extra[i].what);
            }
            for (cf* b : xb)
                if (b) (void)dev_free(b);
        }
    }
    for (int i = 0; i < n; ++i)
        if (i != dec.keep && cand[i]) (void)dev_free(cand[i]);
    if (debug) {
        char line[512];
        int at = 0;
        for (int i = 0; i < n && at < (int)sizeof(line) - 16; ++i) at += snprintf(line + at, sizeof(line) - at, " %.3f", ms[i]);
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        fprintf(stderr, "[bh tune] Y fwd + Z + Y inv on %d spectrum allocation(s) of %.2f GB:%s ms -> #%d  (audition %.0f ms)\n", n,
                bytes / 1e9, line, dec.keep, wall);
    }
    *spec = cand[dec.keep];
    return rc;
}

// The transform passes of one Richardson-Lucy iteration on a volume the CALLER keeps padded (deconv.hip:
// richardson_lucy_engine_padded): forward X of est_p, convolution, [inverse X -> d_p / max(., eps) -> forward X] fused,
// correlation, inverse X stored to corr_p.  est_p is wrap-extended so that the convolution is right on the volume's own box;
// d_p is zero outside that box, which zeroes the ratio there, so corr_p is the LINEAR correlation of the zero-padded ratio:
// the caller folds its wrapped-around tails back, multiplies, and rebuilds est_p.  9 transform passes (8 when nothing is
// padded and update -> forward can stay fused).
int fftconv_rl_iteration_padded(bh_ctx* ctx, const ConvPlan& pl, const float* est_p, const float* d_p, const cf* otf,
                                bool otf_real, int zr, bool zreal, cf* spec, float eps, float* corr_p) {
    BH_TRY(launch_x(ctx, pl, false, 0, est_p, spec, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_rl_z(ctx, pl, false, otf_real, zr, zreal, spec, otf));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, XE_RATIO, nullptr, spec, nullptr, d_p, eps, true));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_rl_z(ctx, pl, true, otf_real, zr, zreal, spec, otf));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, XE_STORE, nullptr, spec, corr_p, nullptr, 0.f));
    return BH_OK;
}

// Richardson-Lucy at a wrap-padded box WITHOUT a fold pass (rows the wave-private X passes take: fftconv_xw.inc / fftconv_x3.inc;
// Y unpadded).
// The estimate going into the convolution is wrap-extended by (lo below, hi above) the volume on the padded axes (z, x); the
// ratio going into the correlation is wrap-extended too — by (hi below, lo above), the mirror image, which is what the
// correlation's taps reach — instead of zero-padded, so the correlation is already the circular one on the volume's own box
// and nothing has to be folded back.  Both extensions are made by the fused X pass that produces the values: along x inside
// the row (two strips of at most K - 1 floats through LDS), along z by letting the wavefront of a margin plane re-read the
// spectrum and the epilogue operand of the plane it mirrors and redo that plane's row — no pass over memory of its own.  Because
// a margin plane reads what another wavefront overwrites, the X passes run out of place here (two spectrum buffers, two
// estimate buffers).  One iteration = the 8 passes of the unpadded path instead of 9 transform passes + a fold / rewrap pass.
bool fftconv_rl_wrap_supported(const ConvPlan& pl, const int64_t N[3], const int64_t K[3], const int64_t P[3]) {
    // any wave-private row length, Y unpadded; the two x strips (K - 1 floats) travel through the head of a row's LDS buffer
    return pl.xw && N[1] == P[1] && K[2] <= 256 && getenv("BH_RL_NOWRAP") == nullptr;
}

// d_p: the data on the box, wrap-extended like the estimate (lo below, hi above): the first pass clips it into est_a
// (e0 = max(d, 0)) and transforms it in one go.  est_a / est_b alternate; the last update is stored straight into `out`, the
// UNPADDED (N[0], N[1], N[2]) result volume.
int fftconv_richardson_lucy_wrap(bh_ctx* ctx, const ConvPlan& pl, const float* d_p, const cf* otf, bool otf_real, int zr, bool zreal, cf* spec_a,
                                 cf* spec_b, float* est_a, float* est_b, const int64_t N[3], const int64_t K[3], int iterations,
                                 float eps, float* out) {
    const int64_t P[3] = {pl.d.Z, pl.d.Y, pl.d.X};
    xw::Params::Wrap we[3], wr[3];  // extension of the estimate (lo below, hi above) and of the ratio (hi below, lo above)
    for (int a = 0; a < 3; ++a) {
        const bool padded = P[a] != N[a];
        const int lo = padded ? (int)(K[a] - 1 - K[a] / 2) : 0, hi = padded ? (int)(K[a] / 2) : 0;
        we[a] = xw::Params::Wrap{(int)N[a], lo, lo, hi};
        wr[a] = xw::Params::Wrap{(int)N[a], lo, hi, lo};
    }
    float *cur = est_a, *nxt = est_b;
    BH_TRY(launch_x(ctx, pl, false, 0, d_p, spec_a, cur, nullptr, 0.f));  // est = max(d, 0) written by the same pass
    for (int it = 0; it < iterations; ++it) {
        BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec_a, nullptr, 1.f));
        BH_TRY(launch_rl_z(ctx, pl, false, otf_real, zr, zreal, spec_a, otf));
        BH_TRY(launch_col(ctx, pl, COL_INV, false, spec_a, nullptr, 1.f));
        BH_TRY(launch_xw_wrap(ctx, pl, xw::FUSED_RATIO_WRAP, spec_a, spec_b, nullptr, d_p, eps, wr[0], wr[2]));
        BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec_b, nullptr, 1.f));
        BH_TRY(launch_rl_z(ctx, pl, true, otf_real, zr, zreal, spec_b, otf));
        BH_TRY(launch_col(ctx, pl, COL_INV, false, spec_b, nullptr, 1.f));
        if (it + 1 == iterations) {  // the last update is needed on the volume's own voxels only: stored cropped
            BH_TRY(launch_xw_wrap(ctx, pl, xw::INV_UPDATE_CROP, spec_b, nullptr, out, cur, eps, we[0], we[2]));
        } else {
            BH_TRY(launch_xw_wrap(ctx, pl, xw::FUSED_UPDATE_WRAP, spec_b, spec_a, nxt, cur, eps, we[0], we[2]));
            std::swap(cur, nxt);
        }
    }
    return BH_OK;
}

// Bare transform pair for callers that do their own spectral arithmetic (phase cross-correlation): forward leaves the
// true DFT coefficients in the engine's scrambled half-spectrum layout, inverse returns real space scaled by V/2
// (multiply the spectrum by 2/V first for a normalised irfftn).  Any element-wise operation that treats both spectra
// alike is layout-agnostic.
int fftconv_forward(bh_ctx* ctx, const ConvPlan& pl, const float* in, cf* spec) {
    BH_TRY(launch_x(ctx, pl, false, 0, in, spec, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, true, spec, nullptr, 1.f));
    return BH_OK;
}
int fftconv_inverse(bh_ctx* ctx, const ConvPlan& pl, cf* spec, float* out) {
    BH_TRY(launch_col(ctx, pl, COL_INV, true, spec, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, XE_STORE, nullptr, spec, out, nullptr, 0.f));
    return BH_OK;
}

// corr = irfft( rfft(ref) * conj(rfft(mov)) / norm ) with the product inside the Z pass of ONE image's transform, the other
// image's finished spectrum (fftconv_forward) being the multiplier: 5 passes per call once that spectrum is in hand, 8 with
// it (instead of 10 for two forward transforms, a product pass and an inverse transform).  Spectrum layout and scaling as
// fftconv_forward / fftconv_inverse: scale = 2 / V.
// fixed: the finished spectrum of the stored image; fixed_is_mov says whether that image is the product's second (conjugated)
// factor.  roll: the Z pass also writes img's forward spectrum over `fixed` (each thread replaces the rows it has just read), so
// that img is the stored image of the next call — the "previous timepoint" reference of the stabilisation estimate for one
// extra store stream.  corr == nullptr (rows the wave-private xw kernels take: fftconv_pcc_peak_only): the correlation volume
// is not stored — the last pass leaves *npartial argmax candidates of |corr| in `partial` (at most 8 per compute unit) for the
// caller's final reduction.
bool fftconv_pcc_peak_only(const ConvPlan& pl) { return pl.xw && !pl.x3 && getenv("BH_PCC_NO_FUSED_PEAK") == nullptr; }
int fftconv_pcc_apply(bh_ctx* ctx, const ConvPlan& pl, const float* img, cf* fixed, bool fixed_is_mov, bool roll, cf* s2, int norm,
                      float scale, float* corr, ArgMax* partial, int* npartial) {
    BH_REQUIRE(corr || (partial && npartial && fftconv_pcc_peak_only(pl)), "internal: correlation volume or peak buffer required");
    BH_TRY(launch_x(ctx, pl, false, 0, img, s2, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, s2, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_PCC, true, s2, fixed, scale, norm, fixed_is_mov ? 1 : 0, roll ? fixed : nullptr));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, s2, nullptr, 1.f));
    if (!corr) return launch_xw_argmax(ctx, pl, s2, partial, npartial);
    BH_TRY(launch_x(ctx, pl, true, XE_STORE, nullptr, s2, corr, nullptr, 0.f));
    return BH_OK;
}
int fftconv_pcc(bh_ctx* ctx, const ConvPlan& pl, const float* ref, const float* mov, cf* s1, cf* s2, int norm, float scale, float* corr,
                ArgMax* partial, int* npartial) {
    BH_TRY(fftconv_forward(ctx, pl, ref, s1));
    return fftconv_pcc_apply(ctx, pl, mov, s1, false, false, s2, norm, scale, corr, partial, npartial);
}

// out = irfft( rfft(in) * H/(H^2+reg) ), H = tf_full (natural order, real, even)
int fftconv_tikhonov(bh_ctx* ctx, const ConvPlan& pl, const float* in, const float* tf_full, float reg, cf* spec,
                     float* filt, float* out) {
    const double V = (double)pl.d.Z * pl.d.Y * pl.d.X;
    const int grid = ctx->num_cus * 8;
    hipLaunchKernelGGL(tikhonov_filter_rows_kernel, dim3(grid), dim3(256), pl.d.XP * sizeof(float), ctx->stream, tf_full,
                       filt, pl.d, reg, (float)(2.0 / V), pl.xw ? pl.xw_col : nullptr);
    BH_CHECK_HIP(hipGetLastError());
    BH_TRY(launch_x(ctx, pl, false, 0, in, spec, nullptr, nullptr, 0.f));
    BH_TRY(launch_col(ctx, pl, COL_FWD, false, spec, nullptr, 1.f));
    BH_TRY(launch_col(ctx, pl, COL_FILTER, true, spec, reinterpret_cast<const cf*>(filt), 1.f));
    BH_TRY(launch_col(ctx, pl, COL_INV, false, spec, nullptr, 1.f));
    BH_TRY(launch_x(ctx, pl, true, XE_STORE, nullptr, spec, out, nullptr, 0.f));
    return BH_OK;
}

}  // namespace bh
