// Focus finding by mid-band power (waveorder focus.compute_midband_power, the primitive under the reference's
// estimate_stabilization.py:948, track.py:310 and estimate_registration.py:114-138).  For a window (Z, Y, X) read in
// place from a larger volume, slice chunk by slice chunk:
//
//   focus_stage_kernel        uint8 / uint16 / int16 / float32 rows -> contiguous float32 planes, and the window's float64 sum
//   hipFFT                    real-to-complex float32, 2-D, batched over the chunk's slices
//   focus_band_rows_kernel    one wavefront per (slice, band row): sum of w |F| over the row's interval of the half spectrum
//   focus_band_slices_kernel  one workgroup per slice: the rows' partial sums, in a fixed order
//
// The band is a table computed on the host in float64 (bh_focus_band_table): by symmetry the bins of a row of the half spectrum
// that lie in the annulus are one interval, and the mirrored columns X/2 < c < X of the full plane carry the same magnitudes as
// columns X - c of row -ky, whose row is in the band exactly when ky's is: columns 0 < kx < X/2 count twice.  Every reduction has
// a fixed order and there are no floating-point atomics: a repeated call returns the same bits.
#include <climits>
#include <cmath>

#include "common.hpp"

// the band's predicate is the restatement's, operation by operation: no fused multiply-add
#pragma clang fp contract(off)

namespace bh {

constexpr size_t FOCUS_WS_BYTES = (size_t)512 << 20;  // float32 planes + half spectra of one chunk (100 slices of 800 x 800)
constexpr int FOCUS_MAX_BATCH = 32768;                // slices per chunk: the band kernels' grid.y
constexpr int FOCUS_STAGE_WG_PER_CU = 8;

struct BandRow {
    int ky, lo, hi;  // row of the half spectrum, its columns [lo, hi)
};

struct BandTable {
    std::vector<int32_t> lo, hi;
    int64_t n_bins = 0;
};

// The mask of one bin exactly as the float64 restatement evaluates it: fy = s_y / Y / p, fx = s_x / X / p,
// frr = sqrt(fy^2 + fx^2), cut_lo < frr < cut_hi.  Along a row frr does not decrease with kx (every operation is correctly
// rounded, hence monotone), so both edges are found by bisection with the very predicate the mask uses.
static int band_table(int64_t Y, int64_t X, double pixel_size, double NA_det, double lambda_ill, double frac_lo, double frac_hi, BandTable* t) {
    BH_REQUIRE(Y >= 16 && X >= 16 && Y % 2 == 0 && X % 2 == 0, "focus band: window (%lld, %lld): Y and X must be even and at least 16",
               (long long)Y, (long long)X);
    BH_REQUIRE(Y <= (int64_t)INT_MAX && X <= (int64_t)INT_MAX && Y * X <= (int64_t)INT_MAX, "focus band: a (%lld, %lld) plane is beyond hipFFT's int", (long long)Y, (long long)X);
    BH_REQUIRE(std::isfinite(pixel_size) && pixel_size > 0 && std::isfinite(NA_det) && NA_det > 0 && std::isfinite(lambda_ill) && lambda_ill > 0,
               "focus band: pixel_size %g, NA_det %g, lambda_ill %g must be finite and positive", pixel_size, NA_det, lambda_ill);
    BH_REQUIRE(std::isfinite(frac_lo) && std::isfinite(frac_hi) && frac_lo < frac_hi, "focus band: midband fractions (%g, %g): lo < hi", frac_lo, frac_hi);
    const double cutoff = 2.0 * NA_det / lambda_ill;
    const double cut_lo = cutoff * frac_lo, cut_hi = cutoff * frac_hi;
    const int half = (int)(X / 2);
    t->lo.assign((size_t)Y, 0);
    t->hi.assign((size_t)Y, 0);
    t->n_bins = 0;
    for (int64_t ky = 0; ky < Y; ++ky) {
        const int64_t sy = ky < Y / 2 ? ky : ky - Y;
        const double fy = (double)sy / (double)Y / pixel_size;
        const double fy2 = fy * fy;
        auto frr = [&](int kx) {
            const double fx = (double)kx / (double)X / pixel_size;
            const double fx2 = fx * fx;
            return std::sqrt(fy2 + fx2);
        };
        // first kx in [0, half + 1) with pred true (pred is false, ..., false, true, ..., true)
        auto first = [&](auto pred) {
            int a = 0, b = half + 1;
            while (a < b) {
                const int m = (a + b) / 2;
                if (pred(m)) b = m;
                else a = m + 1;
            }
            return a;
        };
        const int lo = first([&](int k) { return frr(k) > cut_lo; });
        const int hi = std::max(lo, first([&](int k) { return !(frr(k) < cut_hi); }));
        t->lo[(size_t)ky] = lo, t->hi[(size_t)ky] = hi;
        for (int k = lo; k < hi; ++k) t->n_bins += (k == 0 || k == half) ? 1 : 2;
    }
    return BH_OK;
}

// One wavefront per row of the chunk.  Loads are 4-element vectors at the source's own alignment: up to 3 head elements bring
// the row's address to a multiple of the vector, up to 3 tail elements finish it, so a window that starts at an odd element, or
// whose row stride is no multiple of 4, reads only its own elements.  part[blockIdx.x] = this workgroup's share of the sum.
template <typename TI>
__global__ __launch_bounds__(256) void focus_stage_kernel(const TI* __restrict__ win, int64_t plane_stride, int64_t row_stride, int nz, int Y, int X,
                                                          float* __restrict__ out, double* __restrict__ part) {
    typedef TI V4 __attribute__((ext_vector_type(4)));
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)nz * Y;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t z = r / Y, y = r % Y;
        const TI* src = win + z * plane_stride + y * row_stride;
        float* dst = out + r * X;
        const int mis = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(TI)) & 3);
        const int head = min((4 - mis) & 3, X);
        const int nv = (X - head) >> 2;
        if (lane < head) {
            const float v = (float)src[lane];
            dst[lane] = v;
            acc += (double)v;
        }
        const V4* sv = reinterpret_cast<const V4*>(src + head);
        float* dv = dst + head;
        for (int v = lane; v < nv; v += 64) {
            const V4 q = sv[v];
            const float f0 = (float)q.x, f1 = (float)q.y, f2 = (float)q.z, f3 = (float)q.w;
            dv[4 * v] = f0, dv[4 * v + 1] = f1, dv[4 * v + 2] = f2, dv[4 * v + 3] = f3;
            acc += ((double)f0 + (double)f1) + ((double)f2 + (double)f3);
        }
        const int t = head + 4 * nv + lane;
        if (t < X) {
            const float v = (float)src[t];
            dst[t] = v;
            acc += (double)v;
        }
    }
    acc = block_reduce<4>(acc, op_sum(), red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// n values -> out[0], one workgroup, fixed order
__global__ __launch_bounds__(256) void focus_sum_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
    acc = block_reduce<4>(acc, op_sum(), red);
    if (threadIdx.x == 0) out[0] = acc;
}

// spec: (nb, Y, nh) half spectra.  Wavefront (r, slice): rowpart[slice * nr + r] = sum over rows[r]'s interval of w |F|,
// w = 2 for 0 < kx < half and 1 for kx = 0 and kx = half; |F| from the float32 components in float64 (the squares are exact).
__global__ __launch_bounds__(256) void focus_band_rows_kernel(const float2* __restrict__ spec, const BandRow* __restrict__ rows, int nr, int Y, int nh,
                                                              int half, double* __restrict__ rowpart) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nr) return;  // a whole wavefront
    const BandRow b = rows[r];
    const float2* p = spec + ((int64_t)blockIdx.y * Y + b.ky) * nh;
    double acc = 0.0;
    for (int k = b.lo + lane; k < b.hi; k += 64) {
        const float2 f = p[k];
        const double m = sqrt((double)f.x * (double)f.x + (double)f.y * (double)f.y);
        acc += (k == 0 || k == half) ? m : 2.0 * m;
    }
    acc = wave_reduce(acc, op_sum());
    if (lane == 0) rowpart[(int64_t)blockIdx.y * nr + r] = acc;
}

__global__ __launch_bounds__(256) void focus_band_slices_kernel(const double* __restrict__ rowpart, int nr, double* __restrict__ power) {
    __shared__ double red[4];
    const double* p = rowpart + (int64_t)blockIdx.x * nr;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nr; i += 256) acc += p[i];
    acc = block_reduce<4>(acc, op_sum(), red);
    if (threadIdx.x == 0) power[blockIdx.x] = acc;
}

// The batched 2-D real float32 plan of nb (Y, X) slices: one cached set per (nb, Y, X), so a shorter last chunk has its own.
static int get_focus_plan(bh_ctx* ctx, int64_t nb, int64_t Y, int64_t X, FftPlans** out) {
    const FftDesc d = fft_batched_2d(HIPFFT_R2C, nb, Y, X);
    return cached_plans(ctx, "bh_focus_band_power", FftKey{FftFamily::SlicesF32, nb, Y, X}, &d, 1, out);
}

template <typename TI>
static void launch_stage(const void* win, int64_t ps, int64_t rs, int nz, int Y, int X, float* out, double* part, int grid, hipStream_t s) {
    hipLaunchKernelGGL((focus_stage_kernel<TI>), dim3(grid), dim3(256), 0, s, static_cast<const TI*>(win), ps, rs, nz, Y, X, out, part);
}

}  // namespace bh

using namespace bh;

extern "C" int bh_focus_band_table(int64_t Y, int64_t X, double pixel_size, double NA_det, double lambda_ill, double frac_lo, double frac_hi,
                                   int32_t* kx_lo, int32_t* kx_hi, int64_t* n_bins) {
    BH_REQUIRE(kx_lo && kx_hi && n_bins, "bh_focus_band_table: null argument");
    BandTable t;
    BH_TRY(band_table(Y, X, pixel_size, NA_det, lambda_ill, frac_lo, frac_hi, &t));
    std::copy(t.lo.begin(), t.lo.end(), kx_lo);
    std::copy(t.hi.begin(), t.hi.end(), kx_hi);
    *n_bins = t.n_bins;
    return BH_OK;
}

extern "C" int bh_focus_band_power(bh_ctx* ctx, const void* window, int dtype, int64_t Z, int64_t Y, int64_t X, int64_t plane_stride,
                                   int64_t row_stride, double pixel_size, double NA_det, double lambda_ill, double frac_lo, double frac_hi,
                                   int max_batch, double* power, double* sum) {
    BH_REQUIRE(ctx && window && power, "bh_focus_band_power: null argument");
    BH_REQUIRE(dtype == BH_DT_U8 || dtype == BH_DT_U16 || dtype == BH_DT_I16 || dtype == BH_DT_F32,
               "bh_focus_band_power: unsupported dtype code %d (uint8, uint16, int16, float32)", dtype);
    BH_REQUIRE(Z >= 1 && Z <= (int64_t)INT_MAX, "bh_focus_band_power: Z = %lld (1 to 2**31 - 1)", (long long)Z);
    BandTable t;
    BH_TRY(band_table(Y, X, pixel_size, NA_det, lambda_ill, frac_lo, frac_hi, &t));
    BH_REQUIRE(row_stride >= X && plane_stride >= (Y - 1) * row_stride + X,
               "bh_focus_band_power: strides (%lld, %lld) are smaller than the window's extents (%lld, %lld)", (long long)plane_stride,
               (long long)row_stride, (long long)Y, (long long)X);
    std::vector<BandRow> rows;
    for (int64_t ky = 0; ky < Y; ++ky)
        if (t.lo[(size_t)ky] < t.hi[(size_t)ky]) rows.push_back(BandRow{(int)ky, t.lo[(size_t)ky], t.hi[(size_t)ky]});
    const int nr = (int)rows.size();
    const int64_t nh = X / 2 + 1, per = Y * X, sper = Y * nh;
    int64_t nb = std::min<int64_t>({Z, (int64_t)(FOCUS_WS_BYTES / (size_t)(per * 4 + sper * 8)), (int64_t)INT_MAX / per, (int64_t)FOCUS_MAX_BATCH});
    nb = std::max<int64_t>(nb, 1);
    if (max_batch > 0) nb = std::min<int64_t>(nb, max_batch);
    const int64_t nchunks = ceil_div(Z, nb);
    const int sgrid = (int)std::min<int64_t>(ceil_div(nb * Y, 4), (int64_t)ctx->num_cus * FOCUS_STAGE_WG_PER_CU);
    BH_REQUIRE(nchunks * sgrid <= (int64_t)INT_MAX, "bh_focus_band_power: %lld chunks of %lld slices are too many", (long long)nchunks, (long long)nb);

    BH_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    float* d_real = nullptr;
    float2* d_spec = nullptr;
    BandRow* d_rows = nullptr;
    double *d_rowpart = nullptr, *d_part = nullptr, *d_out = nullptr;  // d_out: Z powers, then the sum
    BH_TRY(get_scratch(ctx, "focus_real", (size_t)(nb * per) * sizeof(float), (void**)&d_real));
    BH_TRY(get_scratch(ctx, "focus_part", (size_t)(nchunks * sgrid) * sizeof(double), (void**)&d_part));
    BH_TRY(get_scratch(ctx, "focus_out", (size_t)(Z + 1) * sizeof(double), (void**)&d_out));
    if (nr) {
        BH_TRY(get_scratch(ctx, "focus_spec", (size_t)(nb * sper) * sizeof(float2), (void**)&d_spec));
        BH_TRY(get_scratch(ctx, "focus_rows", (size_t)nr * sizeof(BandRow), (void**)&d_rows));
        BH_TRY(get_scratch(ctx, "focus_rowpart", (size_t)(nb * nr) * sizeof(double), (void**)&d_rowpart));
        BH_CHECK_HIP(hipMemcpyAsync(d_rows, rows.data(), (size_t)nr * sizeof(BandRow), hipMemcpyHostToDevice, s));  // pageable: taken when this returns
    } else {
        BH_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)Z * sizeof(double), s));  // a band without bins: every power is 0
    }
    const size_t esize = dtype == BH_DT_U8 ? 1 : (dtype == BH_DT_F32 ? 4 : 2);
    int nparts = 0;
    for (int64_t z0 = 0; z0 < Z; z0 += nb) {
        const int nz = (int)std::min<int64_t>(nb, Z - z0);
        const void* w = static_cast<const unsigned char*>(window) + (size_t)(z0 * plane_stride) * esize;
        const int grid = (int)std::min<int64_t>(ceil_div((int64_t)nz * Y, 4), sgrid);
        switch (dtype) {
            case BH_DT_U8: launch_stage<uint8_t>(w, plane_stride, row_stride, nz, (int)Y, (int)X, d_real, d_part + nparts, grid, s); break;
            case BH_DT_U16: launch_stage<uint16_t>(w, plane_stride, row_stride, nz, (int)Y, (int)X, d_real, d_part + nparts, grid, s); break;
            case BH_DT_I16: launch_stage<int16_t>(w, plane_stride, row_stride, nz, (int)Y, (int)X, d_real, d_part + nparts, grid, s); break;
            default: launch_stage<float>(w, plane_stride, row_stride, nz, (int)Y, (int)X, d_real, d_part + nparts, grid, s); break;
        }
        nparts += grid;
        if (!nr) continue;
        FftPlans* pl = nullptr;
        BH_TRY(get_focus_plan(ctx, nz, Y, X, &pl));
        BH_CHECK_FFT(hipfftExecR2C(pl->h[FFT_FWD], d_real, (hipfftComplex*)d_spec));
        hipLaunchKernelGGL(focus_band_rows_kernel, dim3((unsigned)ceil_div(nr, 4), (unsigned)nz), dim3(256), 0, s, (const float2*)d_spec,
                           (const BandRow*)d_rows, nr, (int)Y, (int)nh, (int)(X / 2), d_rowpart);
        hipLaunchKernelGGL(focus_band_slices_kernel, dim3((unsigned)nz), dim3(256), 0, s, (const double*)d_rowpart, nr, d_out + z0);
    }
    hipLaunchKernelGGL(focus_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)d_part, nparts, d_out + Z);
    BH_CHECK_HIP(hipGetLastError());
    std::vector<double> res((size_t)Z + 1);
    BH_CHECK_HIP(hipMemcpyAsync(res.data(), d_out, res.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    BH_CHECK_HIP(hipStreamSynchronize(s));
    std::copy(res.begin(), res.begin() + Z, power);
    if (sum) *sum = res[(size_t)Z];
    return BH_OK;
}
