// Gaussian fits of every bead of a slide in one batched solve on gfx950.
//
//   bh_psf_fit   analyze_psf's per-bead loop (biahub/characterize_psf.py:234-246 -> vendor/napari_psf_analysis PSF.analyze):
//                a 1-D Gaussian on the z column through the patch centre (fit_1d.py: bg, amp, mu, sigma), a 2-D Gaussian on
//                the centre plane (fit_2d.py: bg, amp, mu_y, mu_x, cyy, cyx, cxx) and a 3-D Gaussian on the whole patch
//                (fit_3d.py: bg, amp, mu_z, mu_y, mu_x, czz, czy, czx, cyy, cyx, cxx).  The covariance ENTRIES are the
//                parameters; the model uses the inverse matrix, as the reference's does.
//
// One workgroup per (bead, fit), everything in float64.  The sample is re-derived from the float32 volume on every read:
// v = (int32) max((x + offset) * gain, 0), truncated (np.clip(...).astype(np.int32)).  psf_bg_kernel selects the patch's
// median (radix select on the 32-bit sample, 8 bits per pass, integer LDS histogram); the fit kernels form the reference's
// initial guesses from exact int64 moments and run Levenberg-Marquardt with the analytic Jacobian:
//
//   u = C^-1 d, e = exp(-d.u / 2);  d/dbg = 1, d/damp = e, d/dmu = amp e u, d/dC_ii = amp e u_i^2 / 2, d/dC_ij = amp e u_i u_j
//   (1-D, parameter sigma: d/dsigma = amp e d^2 / sigma^3)
//
// J^T J (upper triangle), J^T r and r.r are accumulated in a fixed order -- per-thread strided partial sums, wave shuffles,
// then LDS across the waves in wave order -- with no float atomics, so a call returns the same bits every time.  Thread 0
// solves (A_s + lambda I) delta_s = g_s by Cholesky, A_s = D A D with D = diag(A)^-1/2 (Marquardt's scaling), the block
// re-evaluates at the trial point (its A and g are kept when the step is accepted, so an iteration is one pass over the
// sample), lambda is divided or multiplied by 10.  A fit has converged when the relative change of r.r over an iteration is
// <= 1e-12 AND the undamped Gauss-Newton step at the current point is <= 1e-8 standard errors in every parameter (or
// <= 1e-11 of the parameter vector; both in the scaled variables; rounding leaves such a step at about 1e-10 standard errors
// for a bead of a few thousand counts).  Then cov = A^-1 r.r / (M - p) (scipy's absolute_sigma=False).
#include "common.hpp"

#include <algorithm>
#include <cmath>

namespace bh {
namespace {

constexpr int FIT_THREADS = 256, FIT_WAVES = FIT_THREADS / 64;
constexpr int COL0[3] = {0, 9, 27};  // first column of the z, yx, zyx records in a row of BH_PSF_NCOL
constexpr int NCOLS[3] = {9, 18, 28};
constexpr int GUESS0[3] = {0, 4, 11};  // first entry of a fit's initial guess in a row of BH_PSF_NGUESS
constexpr double FWHM = 2.3548200450309493;  // 2 sqrt(2 ln 2)
constexpr double FTOL = 1e-12, STEP_SDE = 1e-8, STEP_REL = 1e-11, LAMBDA0 = 1e-3, LAMBDA_MIN = 1e-12, LAMBDA_MAX = 1e16;
// r.r resolves a step only down to sqrt(1e-16 (M - p)) standard errors, the Gauss-Newton step is good far below that: a trial
// point whose r.r rose by rounding only is accepted
constexpr double ACCEPT_SLACK = 1e-13;

struct FitArgs {
    const float* vol;
    int Z, Y, X;
    const int* starts;  // device, 3 per bead
    const int* shapes;  // device, 3 per bead
    double sp[3];
    double offset, gain;
    int f32math;  // the reference's (patch + offset) * gain stays float32 for a float32 store, float64 for integer ones
    int max_iter;
    int* bg;        // device, per bead: uint16 median, or -1 (median >= 65536)
    double* rows;   // device, n x BH_PSF_NCOL
    double* guess;  // device, n x BH_PSF_NGUESS
    int* status;    // device, n x 3
    int* iters;     // device, n x 3
};

__device__ __forceinline__ int sample_of(const FitArgs& a, float x) {
    double t;
    if (a.f32math) {
        const float s = x + (float)a.offset;
        t = (double)(s * (float)a.gain);
    } else {
        const double s = (double)x + a.offset;
        t = s * a.gain;
    }
    if (!(t > 0.0)) return 0;
    return t >= 2147483647.0 ? 2147483647 : (int)t;
}

struct Patch {
    const float* base;  // volume at the patch origin
    int sz, sy, sx;
};

__device__ __forceinline__ Patch patch_of(const FitArgs& a, int b) {
    const int* st = a.starts + 3 * b;
    const int* sh = a.shapes + 3 * b;
    return Patch{a.vol + ((size_t)st[0] * a.Y + st[1]) * a.X + st[2], sh[0], sh[1], sh[2]};
}

__device__ __forceinline__ int voxel(const FitArgs& a, const Patch& p, int z, int y, int x) {
    return sample_of(a, p.base[((size_t)z * a.Y + y) * a.X + x]);
}

// -------------------------------------------------------------------------------------------------- median -> background
// rank-k element (0-based) of the patch's samples: 4 passes of 8 bits, most significant first
__device__ unsigned select_rank(const FitArgs& a, const Patch& p, int M, int k, unsigned* hist, unsigned* sh) {
    unsigned prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += FIT_THREADS) hist[i] = 0;
        __syncthreads();
        for (int m = threadIdx.x; m < M; m += FIT_THREADS) {
            const int x = m % p.sx, t = m / p.sx;
            const unsigned v = (unsigned)voxel(a, p, t / p.sy, t % p.sy, x);
            if (shift == 24 || (v >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned cum = 0;
            int bin = 0;
            for (; bin < 255; ++bin) {
                if (cum + hist[bin] > (unsigned)k) break;
                cum += hist[bin];
            }
            sh[0] = prefix | ((unsigned)bin << shift);
            sh[1] = (unsigned)k - cum;
        }
        __syncthreads();
        prefix = sh[0];
        k = (int)sh[1];
        __syncthreads();
    }
    return prefix;
}

// np.median(patch).astype(np.uint16): an even count takes the mean of the two middle values, then truncates
__global__ __launch_bounds__(FIT_THREADS) void psf_bg_kernel(FitArgs a) {
    __shared__ unsigned hist[256], sh[2];
    const int b = blockIdx.x;
    const Patch p = patch_of(a, b);
    const int M = p.sz * p.sy * p.sx;
    const unsigned hi = select_rank(a, p, M, M / 2, hist, sh);
    const unsigned lo = (M & 1) ? hi : select_rank(a, p, M, M / 2 - 1, hist, sh);
    if (threadIdx.x == 0) {
        const unsigned long long med = ((unsigned long long)lo + hi) >> 1;
        a.bg[b] = med < 65536ull ? (int)med : -1;
    }
}

// ------------------------------------------------------------------------------------------------------------ the models
template <int D>
struct Dim {
    static constexpr int P = D == 1 ? 4 : (D == 2 ? 7 : 11);
    static constexpr int NA = P * (P + 1) / 2;  // upper triangle of J^T J
    static constexpr int NACC = NA + P + 1;     // + J^T r + r.r
    static constexpr int NQ = D == 1 ? 1 : (D == 2 ? 3 : 6);
    static constexpr int M_NMOM = 1 + 2 * D;    // sum w, sum w i, sum w i^2
    static constexpr int AX0 = D == 1 ? 0 : 3 - D;  // first volume axis of the fit's coordinates
};

// sample m of fit D: integer coordinates along the fit's axes and the value
template <int D>
__device__ __forceinline__ int sample_at(const FitArgs& a, const Patch& p, int m, int (&idx)[D]) {
    if constexpr (D == 1) {
        idx[0] = m;
        return voxel(a, p, m, p.sy / 2, p.sx / 2);
    } else if constexpr (D == 2) {
        idx[0] = m / p.sx, idx[1] = m % p.sx;
        return voxel(a, p, p.sz / 2, idx[0], idx[1]);
    } else {
        const int t = m / p.sx;
        idx[0] = t / p.sy, idx[1] = t % p.sy, idx[2] = m % p.sx;
        return voxel(a, p, idx[0], idx[1], idx[2]);
    }
}

// what a pass over the sample needs of the parameters: the inverse covariance (1-D: 1 / sigma^2, and sigma)
template <int D>
struct Pre {
    double bg, amp, mu[D], q[Dim<D>::NQ], sigma;
};

template <int D>
__device__ __forceinline__ Pre<D> prepare(const double* p) {
    Pre<D> r;
    r.bg = p[0], r.amp = p[1];
    for (int i = 0; i < D; ++i) r.mu[i] = p[2 + i];
    r.sigma = 0;
    if constexpr (D == 1) {
        r.sigma = p[3];
        r.q[0] = 1.0 / (p[3] * p[3]);
    } else if constexpr (D == 2) {
        const double a = p[4], b = p[5], c = p[6], det = a * c - b * b;
        r.q[0] = c / det, r.q[1] = -b / det, r.q[2] = a / det;
    } else {
        const double a = p[5], b = p[6], c = p[7], d = p[8], e = p[9], f = p[10];  // [[a b c] [b d e] [c e f]]
        const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
        const double det = a * c00 + b * c01 + c * c02;
        r.q[0] = c00 / det, r.q[1] = c01 / det, r.q[2] = c02 / det;
        r.q[3] = (a * f - c * c) / det, r.q[4] = (b * c - a * e) / det, r.q[5] = (a * d - b * b) / det;
    }
    return r;
}

// model value and Jacobian row at the coordinates c
template <int D>
__device__ __forceinline__ double model(const Pre<D>& r, const double (&c)[D], double (&J)[Dim<D>::P]) {
    if constexpr (D == 1) {
        const double d = c[0] - r.mu[0], u = d * r.q[0], e = exp(-0.5 * d * u), ae = r.amp * e;
        J[0] = 1.0, J[1] = e, J[2] = ae * u, J[3] = ae * u * u * r.sigma;
        return ae + r.bg;
    } else if constexpr (D == 2) {
        const double d0 = c[0] - r.mu[0], d1 = c[1] - r.mu[1];
        const double u0 = r.q[0] * d0 + r.q[1] * d1, u1 = r.q[1] * d0 + r.q[2] * d1;
        const double e = exp(-0.5 * (d0 * u0 + d1 * u1)), ae = r.amp * e;
        J[0] = 1.0, J[1] = e, J[2] = ae * u0, J[3] = ae * u1;
        J[4] = 0.5 * ae * u0 * u0, J[5] = ae * u0 * u1, J[6] = 0.5 * ae * u1 * u1;
        return ae + r.bg;
    } else {
        const double d0 = c[0] - r.mu[0], d1 = c[1] - r.mu[1], d2 = c[2] - r.mu[2];
        const double u0 = r.q[0] * d0 + r.q[1] * d1 + r.q[2] * d2, u1 = r.q[1] * d0 + r.q[3] * d1 + r.q[4] * d2,
                     u2 = r.q[2] * d0 + r.q[4] * d1 + r.q[5] * d2;
        const double e = exp(-0.5 * (d0 * u0 + d1 * u1 + d2 * u2)), ae = r.amp * e;
        J[0] = 1.0, J[1] = e, J[2] = ae * u0, J[3] = ae * u1, J[4] = ae * u2;
        J[5] = 0.5 * ae * u0 * u0, J[6] = ae * u0 * u1, J[7] = ae * u0 * u2;
        J[8] = 0.5 * ae * u1 * u1, J[9] = ae * u1 * u2, J[10] = 0.5 * ae * u2 * u2;
        return ae + r.bg;
    }
}

// out (LDS, NACC) = [upper triangle of J^T J by rows | J^T r | r.r] at the parameters p (LDS), r = data - model
template <int D>
__device__ void accumulate(const FitArgs& a, const Patch& pt, int M, const double* p, double* red, double* out) {
    constexpr int P = Dim<D>::P, NA = Dim<D>::NA, NACC = Dim<D>::NACC;
    const Pre<D> pre = prepare<D>(p);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (int m = threadIdx.x; m < M; m += FIT_THREADS) {
        int idx[D];
        const int v = sample_at<D>(a, pt, m, idx);
        double c[D], J[P];
#pragma unroll
        for (int i = 0; i < D; ++i) c[i] = (double)idx[i] * a.sp[Dim<D>::AX0 + i];
        const double r = (double)v - model<D>(pre, c, J);
        int k = 0;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = i; j < P; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
        for (int i = 0; i < P; ++i) acc[NA + i] += J[i] * r;
        acc[NA + P] += r * r;
    }
    block_reduce_n<FIT_WAVES, NACC>(acc, op_sum(), red, out);
}

// ------------------------------------------------------------------------------------- the small dense algebra (thread 0)
template <int P>
__device__ __forceinline__ int tri(int i, int j) {  // index of (i, j), i <= j, in the packed upper triangle
    return i * P - i * (i - 1) / 2 + (j - i);
}

// in-place Cholesky of the lower triangle of the P x P matrix Mx (row-major); false on a pivot that is not positive and finite
template <int P>
__device__ bool cholesky(double* Mx) {
    for (int j = 0; j < P; ++j) {
        double s = Mx[j * P + j];
        for (int k = 0; k < j; ++k) s -= Mx[j * P + k] * Mx[j * P + k];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double l = sqrt(s);
        Mx[j * P + j] = l;
        for (int i = j + 1; i < P; ++i) {
            double t = Mx[i * P + j];
            for (int k = 0; k < j; ++k) t -= Mx[i * P + k] * Mx[j * P + k];
            Mx[i * P + j] = t / l;
        }
    }
    return true;
}

template <int P>
__device__ void cholesky_solve(const double* L, double* b) {
    for (int i = 0; i < P; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i * P + k] * b[k];
        b[i] = s / L[i * P + i];
    }
    for (int i = P - 1; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < P; ++k) s -= L[k * P + i] * b[k];
        b[i] = s / L[i * P + i];
    }
}

// L (P x P) = Cholesky factor of D A D + lambda I, dscale = sqrt(diag A); false when A is not usable
template <int P>
__device__ bool factor_scaled(const double* acc, double lambda, double* L, double* dscale) {
    for (int i = 0; i < P; ++i) {
        const double d = acc[tri<P>(i, i)];
        if (!(d > 0.0) || !isfinite(d)) return false;
        dscale[i] = sqrt(d);
    }
    for (int i = 0; i < P; ++i)
        for (int j = 0; j <= i; ++j) L[i * P + j] = i == j ? 1.0 + lambda : acc[tri<P>(j, i)] / (dscale[i] * dscale[j]);
    return cholesky<P>(L);
}

// eigenvalues of the symmetric 3 x 3 matrix by cyclic Jacobi rotations (m: 9 entries, destroyed); ev in no order
__device__ void jacobi3(double* m, double* ev) {
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = m[1] * m[1] + m[2] * m[2] + m[5] * m[5];
        if (!(off > 0.0)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = m[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (m[q * 3 + q] - m[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {  // columns p, q
                    const double kp = m[k * 3 + p], kq = m[k * 3 + q];
                    m[k * 3 + p] = c * kp - s * kq, m[k * 3 + q] = s * kp + c * kq;
                }
                for (int k = 0; k < 3; ++k) {  // rows p, q
                    const double pk = m[p * 3 + k], qk = m[q * 3 + k];
                    m[p * 3 + k] = c * pk - s * qk, m[q * 3 + k] = s * pk + c * qk;
                }
            }
    }
    ev[0] = m[0], ev[1] = m[4], ev[2] = m[8];
}

// the reference's record of fit D (records.py, fitter.py) into row: parameters, FWHMs, standard errors
template <int D>
__device__ void write_record(const double* p, const double* sde, double* row) {
    if constexpr (D == 1) {
        row[0] = p[0], row[1] = p[1], row[2] = p[2], row[3] = fabs(p[3]), row[4] = FWHM * fabs(p[3]);
        for (int i = 0; i < 4; ++i) row[5 + i] = sde[i];
    } else if constexpr (D == 2) {
        for (int i = 0; i < 7; ++i) row[i] = p[i];
        row[7] = FWHM * sqrt(p[4]), row[8] = FWHM * sqrt(p[6]);
        const double h = 0.5 * (p[4] + p[6]), r = hypot(0.5 * (p[4] - p[6]), p[5]);
        row[9] = FWHM * sqrt(h + r), row[10] = FWHM * sqrt(h - r);
        for (int i = 0; i < 6; ++i) row[11 + i] = sde[i];
        row[17] = sde[5];  // yx_cxx_sde = error[5], as the reference writes it
    } else {
        for (int i = 0; i < 11; ++i) row[i] = p[i];
        row[11] = FWHM * sqrt(p[5]), row[12] = FWHM * sqrt(p[8]), row[13] = FWHM * sqrt(p[10]);
        double m[9] = {p[5], p[6], p[7], p[6], p[8], p[9], p[7], p[9], p[10]}, ev[3];
        jacobi3(m, ev);
        if (ev[0] < ev[1]) { const double t = ev[0]; ev[0] = ev[1], ev[1] = t; }
        if (ev[1] < ev[2]) { const double t = ev[1]; ev[1] = ev[2], ev[2] = t; }
        if (ev[0] < ev[1]) { const double t = ev[0]; ev[0] = ev[1], ev[1] = t; }
        for (int i = 0; i < 3; ++i) row[14 + i] = FWHM * sqrt(ev[i]);  // a negative eigenvalue gives NaN, as np.sqrt does
        for (int i = 0; i < 11; ++i) row[17 + i] = sde[i];
    }
}

// ---------------------------------------------------------------------------------------------------------- the fit kernel
template <int D>
__global__ __launch_bounds__(FIT_THREADS) void psf_fit_kernel(FitArgs a) {
    constexpr int P = Dim<D>::P, NA = Dim<D>::NA, NACC = Dim<D>::NACC, NMOM = Dim<D>::M_NMOM, KIND = D - 1;
    __shared__ double red[FIT_WAVES * NACC], cur[NACC], trial[NACC];
    __shared__ double par[P], par_t[P], L[P * P], dscale[P], delta[P], sde[P];
    __shared__ long long mred[FIT_WAVES * NMOM], mom[NMOM];
    __shared__ int vmax_w[FIT_WAVES];
    __shared__ int s_status, s_iters;
    __shared__ double s_lambda;

    const int b = blockIdx.x;
    const Patch pt = patch_of(a, b);
    const int M = D == 1 ? pt.sz : (D == 2 ? pt.sy * pt.sx : pt.sz * pt.sy * pt.sx);
    const int bg = a.bg[b];
    double* row = a.rows + (size_t)b * BH_PSF_NCOL + COL0[KIND];
    double* guess = a.guess + (size_t)b * BH_PSF_NGUESS + GUESS0[KIND];

    // initial guess (fit/estimator.py): exact integer moments of the raw sample, finished in float64
    long long m_[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) m_[k] = 0;
    int vmax = 0;
    for (int m = threadIdx.x; m < M; m += FIT_THREADS) {
        int idx[D];
        const long long v = sample_at<D>(a, pt, m, idx);
        vmax = max(vmax, (int)v);
        m_[0] += v;
#pragma unroll
        for (int i = 0; i < D; ++i) m_[1 + i] += v * idx[i], m_[1 + D + i] += v * idx[i] * idx[i];
    }
    vmax = block_reduce<FIT_WAVES>(vmax, op_max(), vmax_w);
    block_reduce_n<FIT_WAVES, NMOM>(m_, op_sum(), mred, mom);
    if (threadIdx.x == 0) {
        int status = -1;
        if (bg < 0 || mom[0] == 0) {
            status = bg < 0 ? BH_PSF_NONFINITE : BH_PSF_EMPTY;
            for (int i = 0; i < P; ++i) par[i] = NAN;
        } else {
            const double sw = (double)mom[0];
            par[0] = (double)bg;
            par[1] = (double)((long long)vmax - bg);
            for (int i = 0; i < D; ++i) {
                const double s = a.sp[Dim<D>::AX0 + i], swi = (double)mom[1 + i], swii = (double)mom[1 + D + i];
                par[2 + i] = swi / sw * s;
                const double var = (swii - swi * swi / sw) / (sw - 1.0) * s * s;  // np.cov(fweights=w): normaliser sum w - 1
                if (D == 1) par[3] = sqrt(var);
                else par[2 + D + (D == 2 ? 2 * i : (i == 0 ? 0 : (i == 1 ? 3 : 5)))] = var;
            }
            if (D == 2) par[5] = 0.0;
            if (D == 3) par[6] = par[7] = par[9] = 0.0;
            for (int i = 0; i < P; ++i)
                if (!isfinite(par[i])) status = BH_PSF_NONFINITE;
            if (M <= P) status = BH_PSF_SINGULAR;  // no degrees of freedom left for the covariance
        }
        for (int i = 0; i < P; ++i) guess[i] = par[i];
        s_status = status, s_iters = 0, s_lambda = LAMBDA0;
    }
    __syncthreads();

    if (s_status < 0) {
        accumulate<D>(a, pt, M, par, red, cur);
        if (threadIdx.x == 0 && !isfinite(cur[NA + P])) s_status = BH_PSF_NONFINITE;
    }
    while (true) {
        if (threadIdx.x == 0 && s_status < 0) {
            if (s_iters >= a.max_iter) s_status = BH_PSF_ITERCAP;
            else if (!factor_scaled<P>(cur, s_lambda, L, dscale)) s_status = BH_PSF_SINGULAR;
            else {
                for (int i = 0; i < P; ++i) delta[i] = cur[NA + i] / dscale[i];
                cholesky_solve<P>(L, delta);
                for (int i = 0; i < P; ++i) par_t[i] = par[i] + delta[i] / dscale[i];
                ++s_iters;
            }
        }
        __syncthreads();
        if (s_status >= 0) break;
        accumulate<D>(a, pt, M, par_t, red, trial);
        if (threadIdx.x == 0) {
            const double ssr = cur[NA + P], ssr_t = trial[NA + P];
            const bool finite_t = isfinite(ssr_t);
            const double ds = ssr > 0.0 ? (ssr - ssr_t) / ssr : 0.0;
            if (finite_t && ssr_t <= ssr * (1.0 + ACCEPT_SLACK)) {
                for (int k = 0; k < NACC; ++k) cur[k] = trial[k];
                for (int i = 0; i < P; ++i) par[i] = par_t[i];
                s_lambda = fmax(s_lambda * 0.1, LAMBDA_MIN);
            } else {
                s_lambda = fmin(s_lambda * 10.0, LAMBDA_MAX);
            }
            if (finite_t && fabs(ds) <= FTOL && factor_scaled<P>(cur, 0.0, L, dscale)) {
                // the undamped step from where we stand, in the scaled variables: delta_s = delta * sqrt(A_ii) >= delta / sde * s
                for (int i = 0; i < P; ++i) delta[i] = cur[NA + i] / dscale[i];
                cholesky_solve<P>(L, delta);
                double smax = 0.0, s2 = 0.0, p2 = 0.0;
                for (int i = 0; i < P; ++i) {
                    smax = fmax(smax, fabs(delta[i]));
                    s2 += delta[i] * delta[i], p2 += par[i] * dscale[i] * par[i] * dscale[i];
                }
                const double s_hat = sqrt(cur[NA + P] / (double)(M - P));
                if (smax <= STEP_SDE * s_hat || s2 <= STEP_REL * STEP_REL * p2) s_status = BH_PSF_CONVERGED;
            }
        }
        // the next round's thread-0 work is ordered after this one's by program order; the barrier behind it publishes both
    }

    if (threadIdx.x == 0) {
        if (s_status == BH_PSF_CONVERGED) {
            // cov = A^-1 r.r / (M - p); A^-1 = D^-1 (D A D)^-1 D^-1, L still holds the factor of D A D
            const double s2 = cur[NA + P] / (double)(M - P);
            for (int i = 0; i < P; ++i) {
                for (int k = 0; k < P; ++k) delta[k] = k == i ? 1.0 : 0.0;
                cholesky_solve<P>(L, delta);
                sde[i] = sqrt(delta[i] / (dscale[i] * dscale[i]) * s2);
            }
            write_record<D>(par, sde, row);
        } else {
            for (int i = 0; i < NCOLS[KIND]; ++i) row[i] = NAN;
        }
        a.status[3 * b + KIND] = s_status;
        a.iters[3 * b + KIND] = s_iters;
    }
}

}  // namespace
}  // namespace bh

using namespace bh;

extern "C" int bh_psf_fit(bh_ctx* ctx, const float* in, int64_t Z, int64_t Y, int64_t X, const int* starts, const int* shapes,
                          int n, const double spacing[3], double offset, double gain, int float32_math, int max_iterations,
                          double* rows, double* guesses, int* status, int* iterations) {
    BH_REQUIRE(ctx && in && spacing && n >= 0, "null argument");
    BH_REQUIRE(n == 0 || (starts && shapes && rows && guesses && status && iterations), "null argument");
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0 && Z < (1ll << 31) && Y < (1ll << 31) && X < (1ll << 31), "bad shape");
    BH_REQUIRE(spacing[0] > 0 && spacing[1] > 0 && spacing[2] > 0 && std::isfinite(spacing[0] + spacing[1] + spacing[2]),
               "spacing must be positive");
    BH_REQUIRE(std::isfinite(offset) && std::isfinite(gain), "offset and gain must be finite");
    BH_REQUIRE(max_iterations >= 1, "max_iterations must be >= 1");
    const int64_t N[3] = {Z, Y, X};
    for (int b = 0; b < n; ++b) {
        int64_t vox = 1, longest = 1;
        for (int k = 0; k < 3; ++k) {
            const int64_t s = starts[3 * b + k], e = shapes[3 * b + k];
            BH_REQUIRE(s >= 0 && e >= 1 && s + e <= N[k], "patch %d is empty or not inside the volume", b);
            vox *= e, longest = std::max(longest, e);
        }
        // int64 moments: sum w i^2 <= 2^31 * voxels * longest^2
        BH_REQUIRE(vox * longest * longest < (1ll << 32), "patch %d is too large for exact 64-bit moments", b);
    }
    if (n == 0) return BH_OK;
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const size_t nz = (size_t)n;
    const size_t o_shapes = sizeof(int) * 3 * nz, o_bg = 2 * o_shapes, o_status = o_bg + sizeof(int) * nz,
                 o_iters = o_status + sizeof(int) * 3 * nz, o_rows = (o_iters + sizeof(int) * 3 * nz + 7) & ~(size_t)7,
                 o_guess = o_rows + sizeof(double) * BH_PSF_NCOL * nz, total = o_guess + sizeof(double) * BH_PSF_NGUESS * nz;
    char* buf;
    BH_TRY(get_scratch(ctx, "psf_fit", total, (void**)&buf));
    BH_CHECK_HIP(hipMemcpyAsync(buf, starts, o_shapes, hipMemcpyHostToDevice, ctx->stream));
    BH_CHECK_HIP(hipMemcpyAsync(buf + o_shapes, shapes, o_shapes, hipMemcpyHostToDevice, ctx->stream));
    FitArgs a;
    a.vol = in, a.Z = (int)Z, a.Y = (int)Y, a.X = (int)X;
    a.starts = reinterpret_cast<const int*>(buf), a.shapes = reinterpret_cast<const int*>(buf + o_shapes);
    for (int k = 0; k < 3; ++k) a.sp[k] = spacing[k];
    a.offset = offset, a.gain = gain, a.f32math = float32_math != 0, a.max_iter = max_iterations;
    a.bg = reinterpret_cast<int*>(buf + o_bg), a.status = reinterpret_cast<int*>(buf + o_status);
    a.iters = reinterpret_cast<int*>(buf + o_iters);
    a.rows = reinterpret_cast<double*>(buf + o_rows), a.guess = reinterpret_cast<double*>(buf + o_guess);
    hipLaunchKernelGGL(psf_bg_kernel, dim3(n), dim3(FIT_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(psf_fit_kernel<1>, dim3(n), dim3(FIT_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(psf_fit_kernel<2>, dim3(n), dim3(FIT_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(psf_fit_kernel<3>, dim3(n), dim3(FIT_THREADS), 0, ctx->stream, a);
    BH_CHECK_HIP(hipGetLastError());
    BH_CHECK_HIP(hipMemcpyAsync(rows, a.rows, sizeof(double) * BH_PSF_NCOL * nz, hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipMemcpyAsync(guesses, a.guess, sizeof(double) * BH_PSF_NGUESS * nz, hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipMemcpyAsync(status, a.status, sizeof(int) * 3 * nz, hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipMemcpyAsync(iterations, a.iters, sizeof(int) * 3 * nz, hipMemcpyDeviceToHost, ctx->stream));
    BH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return BH_OK;
}
