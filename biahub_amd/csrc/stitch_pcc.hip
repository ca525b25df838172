// Pairwise registration of neighbouring FOVs on their overlap strips (biahub/vendor/stitch/tile.py offset,
// _dexp_shim.py register_translation_nd).  bh_stitch_edge_shifts takes all edges of a well; the edges of one
// relation (b below a / b right of a) share a strip shape (n0, n1) and go through the device together:
//
//   strip_min_kernel     signed and float dtypes: the minimum of every strip (subtracted when negative)
//   strip_prepare_kernel Gaussian sigma 1.5 (reflect) -> log1p, log1p -> |sobel 0| + |sobel 1| (reflect) -> sqrt-hann window,
//                        from the tile in place: the strip is a window of the tile and the flips are index arithmetic
//   hipFFT               real-to-complex, batched over the 2n strips
//   cross_power_kernel   R = Fa conj(Fb) / (|Fa conj(Fb)| + 1e-6), scaled by 1 / (n0 n1)
//   hipFFT               complex-to-real, batched over the n edges; the fftshift is index arithmetic in every reader below
//   noise_floor_kernel   the 0.999 quantile of every 16th element of the shifted correlation's corner (ranked in LDS)
//   wrap_gauss_kernel    max(x, floor) - floor on the crop [c - r, c + r), then Gaussian sigma 1.5 (wrap), axis 0 then axis 1
//   peak_argmax_kernel, peak_background_kernel
//                        first maximum in C order; the largest value outside the peak's window (numpy slice rule)
//
// Arithmetic is float64 from the tile's elements to the confidence (float64 hipFFT plans included); only the two optional test
// outputs are rounded to float32.  The reference evaluates the same formula in float32, and its confidence moves by 1e-5 with the
// rounding of its intermediates: (peak - background) / peak amplifies the correlation's error by the peak's loss under the
// sigma 1.5 smoothing.  In float64 the result is that of the float64 restatement the tests hold it to, and
// the strips are small enough (2 x 0.6 Mpixel per edge at 2048 x 300) for the wider type not to matter.
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace bh {

constexpr int SP_R = 6;                 // Gaussian radius: int(4 * 1.5 + 0.5)
constexpr int SP_H = SP_R + 1;          // halo per side: Gaussian plus Sobel
constexpr int SP_TX = 64, SP_TY = 16;   // output tile: a wave's row is 64 consecutive doubles (32 lanes = one 256-byte LDS bank row)
constexpr int SP_IW = SP_TX + 2 * SP_H, SP_IH = SP_TY + 2 * SP_H;  // staged input
constexpr int SP_GW = SP_TX + 2, SP_GH = SP_TY + 2;                // smoothed, log-compressed tile with the Sobel ring
constexpr int SP_MAX_SEL = 4096;        // noise-floor selection held in LDS (a 2048 x 300 strip has 97 values)

struct GaussW {
    double w[SP_R + 1];  // w[0] centre .. w[6] outermost
};

struct StripGeom {
    int Y, X;          // tile
    int n0, n1;        // strip
    int a_oy, a_ox;    // strip origin of tile a in the flipped tile (b's is (0, 0))
    int flipud, fliplr;
    int use_min;
};

// scipy.ndimage "reflect" (d c b a | a b c d | d c b a) for one overhang, then held inside [0, n): partial tiles index past
// the ring and those values are never used
__device__ __forceinline__ int reflect_idx(int c, int n) {
    c = c < 0 ? -c - 1 : (c >= n ? 2 * n - 1 - c : c);
    return min(max(c, 0), n - 1);
}

// monotone map float -> uint32 (for atomicMin)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the minimum of a strip does not depend on the flips: it is taken over the unflipped window
template <typename TI>
__global__ __launch_bounds__(256) void strip_min_kernel(const StripGeom g, const void* const* __restrict__ tiles, unsigned* __restrict__ keys) {
    const int s = blockIdx.y;
    const TI* t = static_cast<const TI*>(tiles[s]);
    int oy = (s & 1) ? 0 : g.a_oy, ox = (s & 1) ? 0 : g.a_ox;
    if (g.flipud) oy = g.Y - g.n0 - oy;
    if (g.fliplr) ox = g.X - g.n1 - ox;
    const int64_t n = (int64_t)g.n0 * g.n1;
    float m = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / g.n1), x = (int)(i % g.n1);
        const float v = (float)t[(int64_t)(oy + y) * g.X + ox + x];
        m = v < m ? v : m;  // a NaN is never the minimum
    }
    m = wave_reduce(m, op_min());
    if ((threadIdx.x & 63) == 0) atomicMin(&keys[s], f2key(m));
}

template <typename TI>
__global__ __launch_bounds__(256) void strip_prepare_kernel(const StripGeom g, const GaussW gw, const void* const* __restrict__ tiles,
                                                            const unsigned* __restrict__ keys, const double* __restrict__ win0,
                                                            const double* __restrict__ win1, double* __restrict__ out) {
    __shared__ double s_in[SP_IH][SP_IW];
    __shared__ double s_v[SP_GH][SP_IW];
    __shared__ double s_l[SP_GH][SP_GW];
    const int s = blockIdx.z;
    const TI* t = static_cast<const TI*>(tiles[s]);
    const int oy = (s & 1) ? 0 : g.a_oy, ox = (s & 1) ? 0 : g.a_ox;
    const int y0 = blockIdx.y * SP_TY, x0 = blockIdx.x * SP_TX;
    double sub = 0.0;
    if (g.use_min) {
        const float m = key2f(keys[s]);  // an element of the strip: exact
        sub = m < 0.f ? (double)m : 0.0;
    }
    // stage: row j <-> strip row y0 - 7 + j, reflected at the strip's edge
    for (int i = threadIdx.x; i < SP_IH * SP_IW; i += 256) {
        const int j = i / SP_IW, k = i % SP_IW;
        int ty = oy + reflect_idx(y0 - SP_H + j, g.n0), tx = ox + reflect_idx(x0 - SP_H + k, g.n1);
        if (g.flipud) ty = g.Y - 1 - ty;
        if (g.fliplr) tx = g.X - 1 - tx;
        s_in[j][k] = (double)t[(int64_t)ty * g.X + tx] - sub;
    }
    __syncthreads();
    // Gaussian along axis 0 at the rows the Sobel ring needs: ring row j <-> strip row clamp(y0 - 1 + j) (the second reflect
    // rule, radius 1, is a clamp), whose taps are staged rows (that row) - (y0 - 7) + k
    for (int i = threadIdx.x; i < SP_GH * SP_IW; i += 256) {
        const int j = i / SP_IW, k = i % SP_IW;
        const int c = min(max(y0 - 1 + j, 0), g.n0 - 1) - (y0 - SP_H);
        double acc = s_in[c][k] * gw.w[0];
#pragma unroll
        for (int d = SP_R; d >= 1; --d) acc += (s_in[c - d][k] + s_in[c + d][k]) * gw.w[d];
        s_v[j][k] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SP_GH * SP_GW; i += 256) {
        const int j = i / SP_GW, k = i % SP_GW;
        const int c = min(max(x0 - 1 + k, 0), g.n1 - 1) - (x0 - SP_H);
        double acc = s_v[j][c] * gw.w[0];
#pragma unroll
        for (int d = SP_R; d >= 1; --d) acc += (s_v[j][c - d] + s_v[j][c + d]) * gw.w[d];
        s_l[j][k] = log1p(log1p(acc));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SP_TY * SP_TX; i += 256) {
        const int j = i / SP_TX, k = i % SP_TX;
        const int y = y0 + j, x = x0 + k;
        if (y >= g.n0 || x >= g.n1) continue;
        const int a = j + 1, b = k + 1;
        // sobel along 0: derivative [-1, 0, 1] over rows, then [1, 2, 1] over columns; along 1 the other way round
        const double d0m = s_l[a + 1][b - 1] - s_l[a - 1][b - 1], d0c = s_l[a + 1][b] - s_l[a - 1][b], d0p = s_l[a + 1][b + 1] - s_l[a - 1][b + 1];
        const double s0 = d0c * 2.0 + (d0m + d0p);
        const double d1m = s_l[a - 1][b + 1] - s_l[a - 1][b - 1], d1c = s_l[a][b + 1] - s_l[a][b - 1], d1p = s_l[a + 1][b + 1] - s_l[a + 1][b - 1];
        const double s1 = d1c * 2.0 + (d1m + d1p);
        out[((int64_t)s * g.n0 + y) * g.n1 + x] = (fabs(s0) + fabs(s1)) * (win0[y] * win1[x]);
    }
}

// spec: (2n, n0, nh) half spectra, a and b of an edge adjacent; R: (n, n0, nh)
__global__ __launch_bounds__(256) void cross_power_kernel(const double2* __restrict__ spec, double2* __restrict__ R, int64_t per, int64_t total,
                                                          double scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i / per, k = i % per;
        const double2 a = spec[(2 * e) * per + k], b = spec[(2 * e + 1) * per + k];
        const double re = a.x * b.x + a.y * b.y, im = a.y * b.x - a.x * b.y;
        const double nrm = hypot(re, im) + 1e-6;
        R[i] = make_double2(re / nrm * scale, im / nrm * scale);
    }
}

struct PeakGeom {
    int n0, n1;    // strip / correlation
    int c0, c1;    // centre n / 2
    int r0, r1;    // int(0.45 n)
    int m0, m1;    // half window of the confidence mask
    int nsel;      // values in the noise-floor selection
    double qpos;   // 0.999 * (nsel - 1)
};

// element (i, j) of fftshift(corr)
__device__ __forceinline__ double corr_shifted_at(const double* __restrict__ corr, const PeakGeom& p, int i, int j) {
    int a = i - p.c0, b = j - p.c1;
    a += a < 0 ? p.n0 : 0;
    b += b < 0 ? p.n1 : 0;
    return corr[(int64_t)a * p.n1 + b];
}

// the optional outputs: float32 copies of the shifted correlation and of a prepared strip
__global__ __launch_bounds__(256) void fftshift_kernel(const PeakGeom p, const double* __restrict__ corr, float* __restrict__ out) {
    const int64_t n = (int64_t)p.n0 * p.n1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = (float)corr_shifted_at(corr, p, (int)(i / p.n1), (int)(i % p.n1));
}

__global__ __launch_bounds__(256) void narrow_kernel(const double* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (float)in[i];
}

// One block per edge.  The selection is every 16th element, in C order, of shifted[0 : c0 - r0, 0 : c1 - r1]; the quantile is
// numpy's "linear" method: sorted[k] and sorted[k + 1] for k = floor(qpos), found by ranking every value against all others
// (ties by position), interpolated as numpy does.
__global__ __launch_bounds__(256) void noise_floor_kernel(const PeakGeom p, const double* __restrict__ corr, int64_t edge_stride,
                                                          double* __restrict__ floors) {
    __shared__ double v[SP_MAX_SEL];
    __shared__ double pick[2];
    __shared__ int bad;
    __shared__ double part[256];
    const double* c = corr + (int64_t)blockIdx.x * edge_stride;
    const int w = p.c1 - p.r1;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    double sum = 0.0;
    for (int i = threadIdx.x; i < p.nsel; i += 256) {
        const int64_t f = (int64_t)i * 16;
        const double x = corr_shifted_at(c, p, (int)(f / w), (int)(f % w));
        v[i] = x;
        sum += x;
        if (!isfinite(x)) bad = 1;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (bad) {  // the quantile of a selection with a NaN or an infinity is not finite: the selection's mean stands in
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int i = 0; i < 256; ++i) t += part[i];
            floors[blockIdx.x] = t / (double)p.nsel;
        }
        return;
    }
    const int k0 = (int)floor(p.qpos), k1 = min(k0 + 1, p.nsel - 1);
    for (int i = threadIdx.x; i < p.nsel; i += 256) {
        const double x = v[i];
        int rank = 0;
        for (int j = 0; j < p.nsel; ++j) {
            const double y = v[j];
            rank += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        if (rank == k0) pick[0] = x;
        if (rank == k1) pick[1] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = p.qpos - (double)k0, a = pick[0], b = pick[1], d = b - a;
        floors[blockIdx.x] = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
    }
}

// axis 0: src is the correlation (shifted, cropped and clipped on the fly); axis 1: src is the first pass's output
template <int AXIS>
__global__ __launch_bounds__(256) void wrap_gauss_kernel(const PeakGeom p, const GaussW gw, const double* __restrict__ src, int64_t src_stride,
                                                         const double* __restrict__ floors, double* __restrict__ dst) {
    const int h = 2 * p.r0, w = 2 * p.r1;
    const int64_t n = (int64_t)h * w;
    const int e = blockIdx.y;
    const double* s = src + (int64_t)e * src_stride;
    const double fl = AXIS == 0 ? floors[e] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        auto at = [&](int d) -> double {
            if (AXIS == 0) {
                int yy = y + d;
                yy += yy < 0 ? h : (yy >= h ? -h : 0);
                return fmax(corr_shifted_at(s, p, p.c0 - p.r0 + yy, p.c1 - p.r1 + x), fl) - fl;
            }
            int xx = x + d;
            xx += xx < 0 ? w : (xx >= w ? -w : 0);
            return s[(int64_t)y * w + xx];
        };
        double acc = at(0) * gw.w[0];
#pragma unroll
        for (int d = SP_R; d >= 1; --d) acc += (at(-d) + at(d)) * gw.w[d];
        dst[(int64_t)e * n + i] = acc;
    }
}

using PeakMax = ValIdx<double>;  // a running argmax under first_max<double>: the FIRST occurrence of the maximum wins

constexpr int SP_PB = 32;  // workgroups per edge in the two peak kernels

struct PeakOut {
    double peak;
    unsigned long long background_bits;  // a non-negative double: such doubles order like their bit patterns (atomicMax)
    long long index;                     // flat index of the peak in the crop
};

// Workgroup (k, e) takes slice k of edge e's smoothed crop: its first maximum in C order, to part[e][k].
__global__ __launch_bounds__(256) void peak_argmax_kernel(const PeakGeom p, const double* __restrict__ sm, PeakMax* __restrict__ part) {
    __shared__ PeakMax red[4];
    const int64_t n = (int64_t)(2 * p.r0) * (2 * p.r1), chunk = (n + SP_PB - 1) / SP_PB;
    const int64_t lo = blockIdx.x * chunk, hi = min(lo + chunk, n);
    const double* s = sm + (int64_t)blockIdx.y * n;
    PeakMax m{-INFINITY, (long long)n};
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const double v = s[i];
        if (v > m.v) m.v = v, m.i = i;  // ascending i per thread: the first occurrence stays
    }
    m = block_reduce<4>(m, first_max<double>(), red);
    if (threadIdx.x == 0) part[blockIdx.y * SP_PB + blockIdx.x] = m;
}

// The edge's peak from the slices' maxima, then the largest value of this workgroup's slice outside [p - m, p + m) per axis, the
// window read as a numpy slice: a negative start counts from the end (and is held at 0), the stop is held at the length,
// start >= stop is empty.  The window's elements are zeroed, not removed, and the crop is non-negative (clipped at the noise
// floor, smoothed with positive weights), so the background starts from the 0 that out[] is cleared to.
__global__ __launch_bounds__(256) void peak_background_kernel(const PeakGeom p, const double* __restrict__ sm, const PeakMax* __restrict__ part,
                                                              PeakOut* __restrict__ out) {
    __shared__ double red[4];
    const int h = 2 * p.r0, w = 2 * p.r1;
    const int64_t n = (int64_t)h * w, chunk = (n + SP_PB - 1) / SP_PB;
    const int64_t lo = blockIdx.x * chunk, hi = min(lo + chunk, n);
    const double* s = sm + (int64_t)blockIdx.y * n;
    PeakMax best = part[blockIdx.y * SP_PB];
    for (int k = 1; k < SP_PB; ++k) best = first_max<double>()(best, part[blockIdx.y * SP_PB + k]);
    if (best.i >= n) best.i = 0;  // nothing compared greater than -inf (all NaN): np.argmax would name a NaN; index 0 stands in
    const int py = (int)(best.i / w), px = (int)(best.i % w);
    auto lo_of = [](int q, int m_, int len) { return q - m_ < 0 ? max(q - m_ + len, 0) : min(q - m_, len); };
    const int ylo = lo_of(py, p.m0, h), yhi = min(py + p.m0, h), xlo = lo_of(px, p.m1, w), xhi = min(px + p.m1, w);
    const bool window = ylo < yhi && xlo < xhi;
    double bg = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        if (window && y >= ylo && y < yhi && x >= xlo && x < xhi) continue;
        bg = fmax(bg, s[i]);
    }
    bg = block_reduce<4>(bg, op_max(), red);
    if (threadIdx.x == 0) {
        if (bg > 0.0) atomicMax(&out[blockIdx.y].background_bits, (unsigned long long)__double_as_longlong(bg));
        if (blockIdx.x == 0) out[blockIdx.y].peak = best.v, out[blockIdx.y].index = best.i;
    }
}

// Batched 2-D real float64 plans of (n0, n1) strips, one cached set per (n_edges, n0, n1): FFT_FWD transforms the 2 n_edges strips,
// FFT_INV the n_edges cross-power spectra.
static int get_strip_plans(bh_ctx* ctx, int64_t n_edges, int64_t n0, int64_t n1, FftPlans** out) {
    const FftDesc d[2] = {fft_batched_2d(HIPFFT_D2Z, 2 * n_edges, n0, n1), fft_batched_2d(HIPFFT_Z2D, n_edges, n0, n1)};
    return cached_plans(ctx, "bh_stitch_edge_shifts", FftKey{FftFamily::StripsF64, n_edges, n0, n1}, d, 2, out);
}

static GaussW gauss_weights() {  // scipy.ndimage._gaussian_kernel1d(sigma = 1.5, order 0, radius 6)
    GaussW g;
    double phi[2 * SP_R + 1], sum = 0;
    for (int i = -SP_R; i <= SP_R; ++i) sum += phi[i + SP_R] = std::exp(-0.5 / (1.5 * 1.5) * i * i);
    for (int d = 0; d <= SP_R; ++d) g.w[d] = phi[SP_R + d] / sum;
    return g;
}

static void sqrt_hann(int n, double* w) {  // hann(n, periodic = False) ** 0.5
    for (int i = 0; i < n; ++i) {
        const double h = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / (double)(n - 1));
        w[i] = std::sqrt(h < 0.0 ? 0.0 : h);
    }
}

template <typename TI>
static void launch_prepare(const StripGeom& g, const GaussW& gw, int nstrips, const void* const* tiles, unsigned* keys, const double* win0,
                           const double* win1, double* real, hipStream_t s) {
    if (g.use_min) {
        const int chunks = (int)std::min<int64_t>(ceil_div((int64_t)g.n0 * g.n1, 256 * 16), 64);
        hipLaunchKernelGGL((strip_min_kernel<TI>), dim3(chunks, nstrips), dim3(256), 0, s, g, tiles, keys);
    }
    hipLaunchKernelGGL((strip_prepare_kernel<TI>), dim3((unsigned)ceil_div(g.n1, SP_TX), (unsigned)ceil_div(g.n0, SP_TY), nstrips), dim3(256), 0, s,
                       g, gw, tiles, (const unsigned*)keys, win0, win1, real);
}

struct GroupBuffers {
    unsigned char* tab;  // pointers | windows | minimum keys
    double *real, *corr;
    double2 *spec, *R;
    double* floors;
    PeakMax* part;   // SP_PB slice maxima per edge of the group
    PeakOut* peaks;  // the group's edges, cleared by the caller
};

// all edges of one relation; idx: their positions in the caller's arrays
static int run_group(bh_ctx* ctx, const GroupBuffers& B, int relation, const std::vector<int>& idx, const void* const* tile_a,
                     const void* const* tile_b, int dtype, int64_t Y, int64_t X, int64_t overlap, int flipud, int fliplr,
                     float* const* prepared, float* const* corr_shifted, PeakGeom* pg_out) {
    const int n = (int)idx.size(), ns = 2 * n;
    hipStream_t s = ctx->stream;
    StripGeom g{};
    g.Y = (int)Y, g.X = (int)X;
    g.n0 = relation == BH_STITCH_BELOW ? (int)overlap : (int)Y;
    g.n1 = relation == BH_STITCH_BELOW ? (int)X : (int)overlap;
    g.a_oy = (int)Y - g.n0, g.a_ox = (int)X - g.n1;
    g.flipud = flipud, g.fliplr = fliplr;
    g.use_min = dtype == BH_DT_I16 || dtype == BH_DT_F32;
    const int64_t per = (int64_t)g.n0 * g.n1, nh = g.n1 / 2 + 1, sper = (int64_t)g.n0 * nh;
    const GaussW gw = gauss_weights();

    const size_t b_ptr = (size_t)ns * sizeof(void*), b_win = (size_t)(g.n0 + g.n1) * sizeof(double);
    std::vector<unsigned char> blob(b_ptr + b_win);
    for (int k = 0; k < n; ++k) {
        reinterpret_cast<const void**>(blob.data())[2 * k] = tile_a[idx[k]];
        reinterpret_cast<const void**>(blob.data())[2 * k + 1] = tile_b[idx[k]];
    }
    double* hw = reinterpret_cast<double*>(blob.data() + b_ptr);
    sqrt_hann(g.n0, hw);
    sqrt_hann(g.n1, hw + g.n0);
    BH_CHECK_HIP(hipMemcpyAsync(B.tab, blob.data(), blob.size(), hipMemcpyHostToDevice, s));  // pageable: taken when this returns
    const void* const* d_tiles = reinterpret_cast<const void* const*>(B.tab);
    const double* d_win0 = reinterpret_cast<const double*>(B.tab + b_ptr);
    unsigned* d_keys = reinterpret_cast<unsigned*>(B.tab + b_ptr + b_win);
    if (g.use_min) BH_CHECK_HIP(hipMemsetAsync(d_keys, 0xff, (size_t)ns * sizeof(unsigned), s));
    switch (dtype) {
        case BH_DT_U8: launch_prepare<uint8_t>(g, gw, ns, d_tiles, d_keys, d_win0, d_win0 + g.n0, B.real, s); break;
        case BH_DT_U16: launch_prepare<uint16_t>(g, gw, ns, d_tiles, d_keys, d_win0, d_win0 + g.n0, B.real, s); break;
        case BH_DT_I16: launch_prepare<int16_t>(g, gw, ns, d_tiles, d_keys, d_win0, d_win0 + g.n0, B.real, s); break;
        default: launch_prepare<float>(g, gw, ns, d_tiles, d_keys, d_win0, d_win0 + g.n0, B.real, s); break;
    }
    BH_CHECK_HIP(hipGetLastError());
    if (prepared)
        for (int k = 0; k < ns; ++k)
            hipLaunchKernelGGL(narrow_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(per, 256), 4096)), dim3(256), 0, s,
                               (const double*)(B.real + (int64_t)k * per), prepared[2 * idx[k / 2] + (k & 1)], per);

    FftPlans* pl = nullptr;
    BH_TRY(get_strip_plans(ctx, n, g.n0, g.n1, &pl));
    BH_CHECK_FFT(hipfftExecD2Z(pl->h[FFT_FWD], B.real, (hipfftDoubleComplex*)B.spec));
    const int64_t total = (int64_t)n * sper;
    const int egrid = (int)std::min<int64_t>(ceil_div(total, 256), (int64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL(cross_power_kernel, dim3(egrid), dim3(256), 0, s, (const double2*)B.spec, B.R, sper, total, 1.0 / (double)per);
    BH_CHECK_FFT(hipfftExecZ2D(pl->h[FFT_INV], (hipfftDoubleComplex*)B.R, B.corr));

    PeakGeom p{};
    p.n0 = g.n0, p.n1 = g.n1;
    p.c0 = g.n0 / 2, p.c1 = g.n1 / 2;
    p.r0 = (int)(0.45 * g.n0), p.r1 = (int)(0.45 * g.n1);
    const int h = 2 * p.r0, w = 2 * p.r1;
    p.m0 = std::max(8, (int)std::pow((double)h, 0.9) / 8);
    p.m1 = std::max(8, (int)std::pow((double)w, 0.9) / 8);
    const int64_t region = (int64_t)(p.c0 - p.r0) * (p.c1 - p.r1);
    p.nsel = (int)ceil_div(region, 16);
    p.qpos = 0.999 * (double)(p.nsel - 1);
    BH_REQUIRE(p.nsel >= 1 && p.nsel <= SP_MAX_SEL, "bh_stitch_edge_shifts: the noise-floor selection of a (%d, %d) strip has %lld values (1 to %d)",
               g.n0, g.n1, (long long)ceil_div(region, 16), SP_MAX_SEL);
    if (corr_shifted)
        for (int k = 0; k < n; ++k)
            hipLaunchKernelGGL(fftshift_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(per, 256), 4096)), dim3(256), 0, s, p,
                               (const double*)(B.corr + (int64_t)k * per), corr_shifted[idx[k]]);
    hipLaunchKernelGGL(noise_floor_kernel, dim3(n), dim3(256), 0, s, p, (const double*)B.corr, per, B.floors);
    const int64_t cn = (int64_t)h * w;
    const dim3 wgrid((unsigned)std::min<int64_t>(ceil_div(cn, 256), 4096), n);
    double* pass0 = B.real;                             // the strips have been transformed: their buffer takes the first pass,
    double* pass1 = reinterpret_cast<double*>(B.spec);  // the spectra's the second
    hipLaunchKernelGGL((wrap_gauss_kernel<0>), wgrid, dim3(256), 0, s, p, gw, (const double*)B.corr, per, (const double*)B.floors, pass0);
    hipLaunchKernelGGL((wrap_gauss_kernel<1>), wgrid, dim3(256), 0, s, p, gw, (const double*)pass0, cn, (const double*)B.floors, pass1);
    // the group's results land contiguously; the caller scatters them
    hipLaunchKernelGGL(peak_argmax_kernel, dim3(SP_PB, n), dim3(256), 0, s, p, (const double*)pass1, B.part);
    hipLaunchKernelGGL(peak_background_kernel, dim3(SP_PB, n), dim3(256), 0, s, p, (const double*)pass1, (const PeakMax*)B.part, B.peaks);
    BH_CHECK_HIP(hipGetLastError());
    *pg_out = p;
    return BH_OK;
}

}  // namespace bh

using namespace bh;

extern "C" int bh_stitch_edge_shifts(bh_ctx* ctx, int n_edges, const void* const* tile_a, const void* const* tile_b, const int32_t* relation,
                                     int dtype, int64_t Y, int64_t X, int64_t overlap, int flipud, int fliplr, double* shift,
                                     double* confidence, float* const* prepared, float* const* corr_shifted) {
    BH_REQUIRE(n_edges >= 1, "bh_stitch_edge_shifts: n_edges = %d (>= 1)", n_edges);
    BH_REQUIRE(ctx && tile_a && tile_b && relation && shift && confidence, "bh_stitch_edge_shifts: null argument");
    BH_REQUIRE(dtype == BH_DT_U8 || dtype == BH_DT_U16 || dtype == BH_DT_I16 || dtype == BH_DT_F32,
               "bh_stitch_edge_shifts: unsupported dtype code %d (uint8, uint16, int16, float32)", dtype);
    BH_REQUIRE(Y >= 16 && X >= 16 && Y < (1 << 24) && X < (1 << 24), "bh_stitch_edge_shifts: tile (%lld, %lld): each extent must be 16 to 2**24 - 1",
               (long long)Y, (long long)X);
    std::vector<int> groups[2];
    for (int e = 0; e < n_edges; ++e) {
        BH_REQUIRE(tile_a[e] && tile_b[e], "bh_stitch_edge_shifts: a tile of edge %d is null", e);
        BH_REQUIRE(relation[e] == BH_STITCH_BELOW || relation[e] == BH_STITCH_RIGHT, "bh_stitch_edge_shifts: relation %d of edge %d", relation[e], e);
        BH_REQUIRE(!prepared || (prepared[2 * e] && prepared[2 * e + 1]), "bh_stitch_edge_shifts: prepared[%d] is null", 2 * e);
        BH_REQUIRE(!corr_shifted || corr_shifted[e], "bh_stitch_edge_shifts: corr_shifted[%d] is null", e);
        groups[relation[e]].push_back(e);
    }
    for (int r = 0; r < 2; ++r) {
        if (groups[r].empty()) continue;
        const int64_t extent = r == BH_STITCH_BELOW ? Y : X;
        BH_REQUIRE(overlap >= 16 && overlap <= extent, "bh_stitch_edge_shifts: overlap %lld (16 to the tile's extent %lld along the strip axis)",
                   (long long)overlap, (long long)extent);
        const int64_t per = overlap * (r == BH_STITCH_BELOW ? X : Y);
        BH_REQUIRE(per * 2 * (int64_t)groups[r].size() < (1ll << 31), "bh_stitch_edge_shifts: %zu strips of %lld elements are too many for one batch",
                   2 * groups[r].size(), (long long)per);
    }
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    // one set of buffers, sized for the larger group; the second group's work is ordered after the first's on the stream
    size_t b_tab = 0, b_real = 0, b_spec = 0;
    for (int r = 0; r < 2; ++r) {
        const size_t n = groups[r].size();
        if (!n) continue;
        const size_t n0 = (size_t)(r == BH_STITCH_BELOW ? overlap : Y), n1 = (size_t)(r == BH_STITCH_BELOW ? X : overlap);
        b_tab = std::max(b_tab, 2 * n * sizeof(void*) + (n0 + n1) * sizeof(double) + 2 * n * sizeof(unsigned));
        b_real = std::max(b_real, 2 * n * n0 * n1 * sizeof(double));
        b_spec = std::max(b_spec, 2 * n * n0 * (n1 / 2 + 1) * sizeof(double2));
    }
    GroupBuffers B{};
    PeakOut* d_peaks = nullptr;
    BH_TRY(get_scratch(ctx, "spcc_tab", b_tab, (void**)&B.tab));
    BH_TRY(get_scratch(ctx, "spcc_real", b_real, (void**)&B.real));
    BH_TRY(get_scratch(ctx, "spcc_spec", b_spec, (void**)&B.spec));
    BH_TRY(get_scratch(ctx, "spcc_R", b_spec / 2, (void**)&B.R));
    BH_TRY(get_scratch(ctx, "spcc_corr", b_real / 2, (void**)&B.corr));
    BH_TRY(get_scratch(ctx, "spcc_floor", (size_t)n_edges * sizeof(double), (void**)&B.floors));
    BH_TRY(get_scratch(ctx, "spcc_peak", (size_t)n_edges * sizeof(PeakOut), (void**)&d_peaks));
    BH_TRY(get_scratch(ctx, "spcc_part", (size_t)n_edges * SP_PB * sizeof(PeakMax), (void**)&B.part));
    BH_CHECK_HIP(hipMemsetAsync(d_peaks, 0, (size_t)n_edges * sizeof(PeakOut), ctx->stream));
    PeakGeom pg[2] = {};
    int first[2] = {0, 0};
    int done = 0;
    for (int r = 0; r < 2; ++r) {
        if (groups[r].empty()) continue;
        first[r] = done;
        B.peaks = d_peaks + done;
        BH_TRY(run_group(ctx, B, r, groups[r], tile_a, tile_b, dtype, Y, X, overlap, flipud, fliplr, prepared, corr_shifted, &pg[r]));
        done += (int)groups[r].size();
    }
    std::vector<PeakOut> res((size_t)n_edges);
    BH_CHECK_HIP(hipMemcpyAsync(res.data(), d_peaks, res.size() * sizeof(PeakOut), hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < 2; ++r)
        for (size_t k = 0; k < groups[r].size(); ++k) {
            const int e = groups[r][k];
            const PeakOut& o = res[(size_t)first[r] + k];
            const int w = 2 * pg[r].r1;
            shift[2 * e] = (double)(o.index / w - pg[r].r0) + (r == BH_STITCH_BELOW ? (double)(Y - overlap) : 0.0);
            shift[2 * e + 1] = (double)(o.index % w - pg[r].r1) + (r == BH_STITCH_RIGHT ? (double)(X - overlap) : 0.0);
            double background;
            std::memcpy(&background, &o.background_bits, sizeof(background));
            confidence[e] = (o.peak - background) / (1e-6 + o.peak);
        }
    return BH_OK;
}
