// StackReg translation on gfx950: TurboReg's translation mode for a batch of frame pairs.
//
//   bh_stackreg_translation   pystackreg's StackReg(TRANSLATION).register_stack as biahub/estimate_stabilization.py:755-756
//                             calls it, restated (bhcore.h has the definition; tests/stackreg_ref.py restates it in numpy).
//
// Everything is float64.  Per call:
//
//   sr_convert_kernel         frames (any dtype, strided) -> level 0 of every frame's pyramid, clipped below at 0
//   sr_reduce_kernel          level l -> level l + 1: [1 4 6 4 1] / 16 along x, then y, mirror, even indices
//   sr_prefilter_*_kernel     cubic B-spline coefficients of every level: one thread per line, y lines then x lines
//   sr_flat_kernel            one workgroup per frame: the level-0 gradient matrix and energy -> a "flat" flag
//   per level, coarsest first: sr_begin_kernel, then MAX_ITER + 1 rounds of
//     sr_eval_kernel          grid (tiles, pairs): the seven sums over Omega(d) of one 64 x 64 tile at the pair's attempt
//     sr_step_kernel          one thread per pair: folds the tiles left to right, accepts or rejects, forms the next attempt
//
// The host enqueues all of it without reading back; a pair whose level has ended leaves its workgroups at once.  A translation
// moves every pixel by the same d, so the 4 + 4 tap weights are uniform and a lane that walks down a column needs one new
// row-filtered value (4 loads) per pixel: the three above it stay in registers.  The 64 lanes of a wave hold neighbouring
// columns of one row, so a coefficient row is read once per wave and the row pointers are wave-uniform.
#include "common.hpp"

#include <algorithm>
#include <cmath>

namespace bh {
namespace {

constexpr int TILE = 64, EV_THREADS = 256, EV_WAVES = EV_THREADS / 64, ROWS_PER_WAVE = TILE / EV_WAVES;
constexpr int NSUM = 7;  // count, r.r, r.gy, r.gx, gy.gy, gy.gx, gx.gx
constexpr int MAX_LEVELS = 16;
constexpr int PREFILTER_HORIZON = 64;  // |pole|^64 = 2.5e-37: the causal initialisation's later terms are below an ulp
constexpr double POLE = -0.26794919243112270647;  // sqrt(3) - 2

struct PairState {
    double d[2], trial[2], lambda, cur[NSUM];
    int active, small, dead, capped, iters, pad;
};

struct Level {
    int H, W;
    long long off;  // of the level in a frame's pyramid, in doubles
};

// whole-sample mirror (-1 -> 1, n -> n - 2), then clamped: a pixel of Omega needs one reflection, any other index stays inside
__device__ __forceinline__ int mirror(int i, int n) {
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ bool usable(double hyy, double hyx, double hxx) {
    return isfinite(hyy + hyx + hxx) && hyy > 0.0 && hxx > 0.0 && hyy * hxx - hyx * hyx > BH_STACKREG_COND_REL * hyy * hxx;
}

// ------------------------------------------------------------------------------------------------------------- pyramid
template <typename TI>
__global__ __launch_bounds__(256) void sr_convert_kernel(const TI* __restrict__ frames, long long frame_stride, long long row_stride, int H, int W,
                                                         long long P, double* __restrict__ V) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    const double v = (double)frames[(long long)blockIdx.y * frame_stride + (long long)y * row_stride + x];
    V[(long long)blockIdx.y * P + i] = v > 0.0 ? v : 0.0;
}

__global__ __launch_bounds__(256) void sr_reduce_kernel(double* __restrict__ V, long long P, Level src, Level dst) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)dst.H * dst.W) return;
    const int y = (int)(i / dst.W), x = (int)(i % dst.W);
    const double* in = V + (long long)blockIdx.y * P + src.off;
    constexpr double k[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    int cx[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) cx[b] = mirror(2 * x + b - 2, src.W);
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const double* row = in + (long long)mirror(2 * y + a - 2, src.H) * src.W;
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < 5; ++b) t += k[b] * row[cx[b]];
        s += k[a] * t;
    }
    V[(long long)blockIdx.y * P + dst.off + i] = s;
}

// scipy's spline_filter1d(order=3, mode="mirror") along one line of n >= 2 samples, `stride` doubles apart; src may be dst
__device__ void prefilter_line(const double* src, double* dst, int n, long long stride) {
    const double z = POLE, gain = (1.0 - z) * (1.0 - 1.0 / z);
    const double zn1 = pow(z, (double)(n - 1));
    double c = gain * src[0] + zn1 * (gain * src[(long long)(n - 1) * stride]);
    double zi = z;
    const int horizon = min(n - 1, PREFILTER_HORIZON);
    for (int i = 1; i < horizon; ++i) {
        c += zi * (gain * src[(long long)i * stride] + zn1 * (gain * src[(long long)(n - 1 - i) * stride]));
        zi *= z;
    }
    c /= 1.0 - zn1 * zn1;
    for (int i = 1; i < n; ++i) {  // in place: nothing is written before the sum above is complete, and src[i] is read before dst[i]
        const double next = gain * src[(long long)i * stride] + z * c;
        dst[(long long)(i - 1) * stride] = c;
        c = next;
    }
    dst[(long long)(n - 1) * stride] = c;
    c = (z * dst[(long long)(n - 2) * stride] + c) * z / (z * z - 1.0);
    dst[(long long)(n - 1) * stride] = c;
    for (int i = n - 2; i >= 0; --i) {
        c = z * (c - dst[(long long)i * stride]);
        dst[(long long)i * stride] = c;
    }
}

// one thread per (frame, column): values -> coefficients along y; neighbouring lanes hold neighbouring columns
__global__ __launch_bounds__(256) void sr_prefilter_cols_kernel(const double* __restrict__ V, double* __restrict__ Cf, long long P, Level lv, int T) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * lv.W) return;
    const long long base = (i / lv.W) * P + lv.off + i % lv.W;
    prefilter_line(V + base, Cf + base, lv.H, lv.W);
}

// one thread per (frame, row): in place along x
__global__ __launch_bounds__(256) void sr_prefilter_rows_kernel(double* __restrict__ Cf, long long P, Level lv, int T) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * lv.H) return;
    double* line = Cf + (i / lv.H) * P + lv.off + (i % lv.H) * lv.W;
    prefilter_line(line, line, lv.W, 1);
}

// flat[t] = level 0 of frame t carries no usable gradient
__global__ __launch_bounds__(EV_THREADS) void sr_flat_kernel(const double* __restrict__ V, const double* __restrict__ Cf, long long P, int H, int W,
                                                             int* __restrict__ flat) {
    __shared__ double red[EV_WAVES * 4], tot[4];
    const double* v = V + (long long)blockIdx.x * P;
    const double* c = Cf + (long long)blockIdx.x * P;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < (long long)H * W; i += EV_THREADS) {
        const int y = (int)(i / W), x = (int)(i % W);
        const double gy = 0.5 * (c[(long long)mirror(y + 1, H) * W + x] - c[(long long)mirror(y - 1, H) * W + x]);
        const double gx = 0.5 * (c[(long long)y * W + mirror(x + 1, W)] - c[(long long)y * W + mirror(x - 1, W)]);
        acc[0] += gy * gy, acc[1] += gy * gx, acc[2] += gx * gx, acc[3] += v[i] * v[i];
    }
    block_reduce_n<EV_WAVES, 4>(acc, op_sum(), red, tot);
    if (threadIdx.x == 0)
        flat[blockIdx.x] = !(usable(tot[0], tot[1], tot[2]) && isfinite(tot[3]) && fmin(tot[0], tot[2]) > BH_STACKREG_FLAT_REL * tot[3]);
}

// ------------------------------------------------------------------------------------------------------------- descent
__global__ __launch_bounds__(64) void sr_begin_kernel(PairState* __restrict__ st, const int* __restrict__ pairs, const int* __restrict__ flat, int n,
                                                      int first) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    PairState& s = st[p];
    if (first) {
        s.d[0] = s.d[1] = 0.0;
        for (int k = 0; k < NSUM; ++k) s.cur[k] = 0.0;
        s.dead = flat[pairs[2 * p]] || flat[pairs[2 * p + 1]];
        s.capped = 0, s.iters = 0, s.pad = 0;
    } else {
        s.d[0] *= 2.0, s.d[1] *= 2.0;
    }
    s.trial[0] = s.d[0], s.trial[1] = s.d[1];
    s.lambda = BH_STACKREG_LAMBDA0;
    s.small = 0;
    s.active = !s.dead;
}

struct EvalArgs {
    const double* V;
    const double* Cf;
    long long P;
    Level lv;
    int tiles_x, ntiles;
    const int* pairs;
    const PairState* st;
    double* part;  // pairs x ntiles x NSUM
};

__device__ __forceinline__ void tap_weights(double f, double (&w)[4]) {
    const double g = 1.0 - f;
    w[0] = g * g * g / 6.0;
    w[1] = (3.0 * f * f * f - 6.0 * f * f + 4.0) / 6.0;
    w[2] = (-3.0 * f * f * f + 3.0 * f * f + 3.0 * f + 1.0) / 6.0;
    w[3] = f * f * f / 6.0;
}

__global__ __launch_bounds__(EV_THREADS) void sr_eval_kernel(EvalArgs a) {
    __shared__ double red[EV_WAVES * NSUM];
    const int p = blockIdx.y, tile = blockIdx.x;
    const PairState& s = a.st[p];
    if (!s.active) return;  // the whole workgroup: the step kernel does not read this pair's partials either
    const int H = a.lv.H, W = a.lv.W;
    const double dy = s.trial[0], dx = s.trial[1];
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    // an attempt off the level (or not a number) has an empty Omega; the bound also keeps the index arithmetic in int
    if (fabs(dy) < (double)H && fabs(dx) < (double)W) {
        const double fly = floor(dy), flx = floor(dx);
        const int iy0 = (int)fly, ix0 = (int)flx;
        const bool integer = dy == fly && dx == flx;
        double wy[4] = {0.0, 1.0, 0.0, 0.0}, wx[4] = {0.0, 1.0, 0.0, 0.0};
        if (!integer) tap_weights(dy - fly, wy), tap_weights(dx - flx, wx);
        const long long fm = (long long)a.pairs[2 * p] * a.P + a.lv.off, fr = (long long)a.pairs[2 * p + 1] * a.P + a.lv.off;
        const double* mov = (integer ? a.V : a.Cf) + fm;  // the spline interpolates the values: an integer d reads them
        const double* vr = a.V + fr;
        const double* cr = a.Cf + fr;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int x = (tile % a.tiles_x) * TILE + lane, y0 = (tile / a.tiles_x) * TILE + wave * ROWS_PER_WAVE;
        const int xc = min(x, W - 1), xl = mirror(xc - 1, W), xr = mirror(xc + 1, W);
        const bool xin = x < W && (double)x + dx >= 0.0 && (double)x + dx <= (double)(W - 1);
        int cx[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) cx[l] = mirror(xc + ix0 + l - 1, W);
        auto rowf = [&](int j) {
            const double* row = mov + (long long)mirror(j, H) * W;
            return wx[0] * row[cx[0]] + wx[1] * row[cx[1]] + wx[2] * row[cx[2]] + wx[3] * row[cx[3]];
        };
        const int rows = min(ROWS_PER_WAVE, H - y0);  // <= 0 for a wave below the level
        if (rows > 0) {
            const int j = y0 + iy0 - 1;
            double h0 = rowf(j), h1 = rowf(j + 1), h2 = rowf(j + 2);
            for (int i = 0; i < rows; ++i) {
                const int y = y0 + i;
                const double h3 = rowf(j + 3 + i);
                if (xin && (double)y + dy >= 0.0 && (double)y + dy <= (double)(H - 1)) {
                    const double m = wy[0] * h0 + wy[1] * h1 + wy[2] * h2 + wy[3] * h3;
                    const double r = m - vr[(long long)y * W + xc];
                    const double gy = 0.5 * (cr[(long long)mirror(y + 1, H) * W + xc] - cr[(long long)mirror(y - 1, H) * W + xc]);
                    const double gx = 0.5 * (cr[(long long)y * W + xr] - cr[(long long)y * W + xl]);
                    acc[0] += 1.0, acc[1] += r * r, acc[2] += r * gy, acc[3] += r * gx;
                    acc[4] += gy * gy, acc[5] += gy * gx, acc[6] += gx * gx;
                }
                h0 = h1, h1 = h2, h2 = h3;
            }
        }
    }
    block_reduce_n<EV_WAVES, NSUM>(acc, op_sum(), red, a.part + ((long long)p * a.ntiles + tile) * NSUM);
}

__device__ __forceinline__ void kill_pair(PairState& s) {
    s.dead = 1, s.active = 0;
}

// round 0 takes the sums at the level's start; round k >= 1 judges attempt k
__global__ __launch_bounds__(64) void sr_step_kernel(PairState* __restrict__ st, const double* __restrict__ part, int n, int ntiles, int round) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    PairState& s = st[p];
    if (!s.active) return;
    double t[NSUM];
    const double* q = part + (long long)p * ntiles * NSUM;
    for (int k = 0; k < NSUM; ++k) t[k] = q[k];
    for (int i = 1; i < ntiles; ++i)
        for (int k = 0; k < NSUM; ++k) t[k] += q[(long long)i * NSUM + k];
    bool finite = true;
    for (int k = 0; k < NSUM; ++k) finite = finite && isfinite(t[k]);
    if (round == 0) {
        if (!(t[0] > 0.0) || !finite || !usable(t[4], t[5], t[6])) return kill_pair(s);
        for (int k = 0; k < NSUM; ++k) s.cur[k] = t[k];
    } else {
        ++s.iters;
        const bool ok = t[0] > 0.0 && finite && t[1] / t[0] < s.cur[1] / s.cur[0];
        if (ok && !usable(t[4], t[5], t[6])) return kill_pair(s);
        if (ok) {
            s.d[0] = s.trial[0], s.d[1] = s.trial[1];
            for (int k = 0; k < NSUM; ++k) s.cur[k] = t[k];
            s.lambda /= BH_STACKREG_LAMBDA_FACTOR;
        } else {
            s.lambda *= BH_STACKREG_LAMBDA_FACTOR;
        }
        if (s.small || round == BH_STACKREG_MAX_ITER) {
            s.capped = !s.small;
            s.active = 0;
            return;
        }
    }
    const double a = s.cur[4] * (1.0 + s.lambda), b = s.cur[5], c = s.cur[6] * (1.0 + s.lambda), det = a * c - b * b;
    const double uy = (c * s.cur[2] - b * s.cur[3]) / det, ux = (a * s.cur[3] - b * s.cur[2]) / det;
    s.trial[0] = s.d[0] - uy, s.trial[1] = s.d[1] - ux;
    s.small = hypot(uy, ux) < BH_STACKREG_EPS;
}

template <typename TI>
void launch_convert(const void* frames, int64_t fs, int64_t rs, int T, int H, int W, long long P, double* V, hipStream_t s) {
    const unsigned gx = (unsigned)(((long long)H * W + 255) / 256);
    hipLaunchKernelGGL(sr_convert_kernel<TI>, dim3(gx, T), dim3(256), 0, s, static_cast<const TI*>(frames), (long long)fs, (long long)rs, H, W, P, V);
}

}  // namespace
}  // namespace bh

using namespace bh;

extern "C" int bh_stackreg_translation(bh_ctx* ctx, const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int64_t frame_stride,
                                       int64_t row_stride, const int32_t* pairs, int n, double* shift_yx, double* mse, int32_t* status,
                                       int32_t* iterations) {
    BH_REQUIRE(ctx && frames && n >= 0, "null argument");
    BH_REQUIRE(n == 0 || (pairs && shift_yx && mse && status && iterations), "null argument");
    BH_REQUIRE(dtype == BH_DT_U8 || dtype == BH_DT_U16 || dtype == BH_DT_I16 || dtype == BH_DT_F32,
               "stackreg reads uint8, uint16, int16 and float32 frames, got dtype %d", dtype);
    BH_REQUIRE(T >= 1 && T <= 65535 && n <= 65535, "stackreg takes 1 to 65535 frames and up to 65535 pairs in a call");
    BH_REQUIRE(H >= 8 && W >= 8 && H <= 32768 && W <= 32768, "stackreg frames are 8 to 32768 pixels a side, got (%lld, %lld)", (long long)H, (long long)W);
    BH_REQUIRE(row_stride >= W && (T == 1 || frame_stride >= (H - 1) * row_stride + W), "stackreg: rows or frames overlap");
    for (int p = 0; p < 2 * n; ++p) BH_REQUIRE(pairs[p] >= 0 && pairs[p] < T, "stackreg: pair %d names frame %d of %lld", p / 2, pairs[p], (long long)T);
    if (n == 0) return BH_OK;

    Level lv[MAX_LEVELS];
    int L = 1;
    lv[0] = Level{(int)H, (int)W, 0};
    long long P = (long long)H * W;
    while (std::min(lv[L - 1].H, lv[L - 1].W) >= BH_STACKREG_MIN_SIDE_FOR_NEXT && L < MAX_LEVELS) {
        lv[L] = Level{(lv[L - 1].H + 1) / 2, (lv[L - 1].W + 1) / 2, P};
        P += (long long)lv[L].H * lv[L].W;
        ++L;
    }
    const int tiles_x0 = (int)ceil_div(W, TILE), ntiles0 = tiles_x0 * (int)ceil_div(H, TILE);

    BH_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    double *V, *Cf, *part;
    PairState* st;
    int *d_pairs, *d_flat;
    BH_TRY(get_scratch(ctx, "stackreg_values", sizeof(double) * (size_t)T * P, (void**)&V));
    BH_TRY(get_scratch(ctx, "stackreg_coefs", sizeof(double) * (size_t)T * P, (void**)&Cf));
    BH_TRY(get_scratch(ctx, "stackreg_part", sizeof(double) * (size_t)n * ntiles0 * NSUM, (void**)&part));
    BH_TRY(get_scratch(ctx, "stackreg_state", sizeof(PairState) * (size_t)n, (void**)&st));
    BH_TRY(get_scratch(ctx, "stackreg_pairs", sizeof(int) * 2 * (size_t)n, (void**)&d_pairs));
    BH_TRY(get_scratch(ctx, "stackreg_flat", sizeof(int) * (size_t)T, (void**)&d_flat));
    BH_CHECK_HIP(hipMemcpyAsync(d_pairs, pairs, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, s));

    switch (dtype) {
        case BH_DT_U8: launch_convert<uint8_t>(frames, frame_stride, row_stride, (int)T, (int)H, (int)W, P, V, s); break;
        case BH_DT_U16: launch_convert<uint16_t>(frames, frame_stride, row_stride, (int)T, (int)H, (int)W, P, V, s); break;
        case BH_DT_I16: launch_convert<int16_t>(frames, frame_stride, row_stride, (int)T, (int)H, (int)W, P, V, s); break;
        default: launch_convert<float>(frames, frame_stride, row_stride, (int)T, (int)H, (int)W, P, V, s); break;
    }
    for (int l = 1; l < L; ++l) {
        const unsigned gx = (unsigned)(((long long)lv[l].H * lv[l].W + 255) / 256);
        hipLaunchKernelGGL(sr_reduce_kernel, dim3(gx, (unsigned)T), dim3(256), 0, s, V, P, lv[l - 1], lv[l]);
    }
    for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(sr_prefilter_cols_kernel, dim3((unsigned)ceil_div(T * lv[l].W, 256)), dim3(256), 0, s, V, Cf, P, lv[l], (int)T);
        hipLaunchKernelGGL(sr_prefilter_rows_kernel, dim3((unsigned)ceil_div(T * lv[l].H, 256)), dim3(256), 0, s, Cf, P, lv[l], (int)T);
    }
    hipLaunchKernelGGL(sr_flat_kernel, dim3((unsigned)T), dim3(EV_THREADS), 0, s, V, Cf, P, (int)H, (int)W, d_flat);
    BH_CHECK_HIP(hipGetLastError());

    const unsigned pair_blocks = (unsigned)ceil_div(n, 64);
    for (int l = L - 1; l >= 0; --l) {
        EvalArgs a;
        a.V = V, a.Cf = Cf, a.P = P, a.lv = lv[l];
        a.tiles_x = (int)ceil_div(lv[l].W, TILE), a.ntiles = a.tiles_x * (int)ceil_div(lv[l].H, TILE);
        a.pairs = d_pairs, a.st = st, a.part = part;
        hipLaunchKernelGGL(sr_begin_kernel, dim3(pair_blocks), dim3(64), 0, s, st, d_pairs, d_flat, n, l == L - 1 ? 1 : 0);
        for (int round = 0; round <= BH_STACKREG_MAX_ITER; ++round) {
            hipLaunchKernelGGL(sr_eval_kernel, dim3((unsigned)a.ntiles, (unsigned)n), dim3(EV_THREADS), 0, s, a);
            hipLaunchKernelGGL(sr_step_kernel, dim3(pair_blocks), dim3(64), 0, s, st, part, n, a.ntiles, round);
        }
        BH_CHECK_HIP(hipGetLastError());
    }
    std::vector<PairState> host((size_t)n);
    BH_CHECK_HIP(hipMemcpyAsync(host.data(), st, sizeof(PairState) * (size_t)n, hipMemcpyDeviceToHost, s));
    BH_CHECK_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < n; ++p) {
        const PairState& r = host[(size_t)p];
        shift_yx[2 * p] = r.dead ? 0.0 : r.d[0], shift_yx[2 * p + 1] = r.dead ? 0.0 : r.d[1];
        mse[p] = r.dead ? 0.0 : r.cur[1] / r.cur[0];
        status[p] = r.dead ? BH_STACKREG_DEGENERATE : (r.capped ? BH_STACKREG_ITERCAP : BH_STACKREG_CONVERGED);
        iterations[p] = r.iters;
    }
    return BH_OK;
}
