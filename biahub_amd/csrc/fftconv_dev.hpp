// Internal header of the fused FFT engine: what its translation units share — fftconv.hip (plans, staging kernels, drivers)
// and the kernel families fftconv_col.hip, fftconv_xtile.hip, fftconv_xw.hip and fftconv_colreg.hip.  Device code common to the
// families (complex helpers, the LDS-stepped FFT), the parameter structs of the kernels, the launch helper and the switch
// readers, and the families' launchers and table builders.
#pragma once
#include "fftconv.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace bh {

#ifndef BH_FC_NT
#define BH_FC_NT 1024
#endif
constexpr int FC_NT = BH_FC_NT;    // threads per workgroup
constexpr int FC_TILE = 16384;     // complex elements per column tile (128 KiB)
#ifndef BH_FC_XR
#define BH_FC_XR 16
#endif
#ifndef BH_FC_XNT
#define BH_FC_XNT BH_FC_NT
#endif
#ifndef BH_FC_XNT8
#define BH_FC_XNT8 768  // threads per workgroup of the 8-row X passes (rows of 3072 voxels: one thread per float4 of a row;
                        // 1.40 s against 1.44 s with 1024 threads for R-L x10 at the box (768,2048,3072))
#endif

__device__ __forceinline__ cf cadd(cf a, cf b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cf csub(cf a, cf b) { return make_float2(a.x - b.x, a.y - b.y); }
// Complex products as TWO packed instructions (v_pk_mul_f32 + v_pk_fma_f32 with op_sel / neg modifiers picking the halves):
// the compiler's own lowering spends four to six instructions on them, a quarter of the arithmetic of the register FFT stages
// being v_mov shuffles that line operands up for packed adds.  BH_FC_PK_CMUL=0 keeps the plain C form (A/B switch).
#ifndef BH_FC_PK_CMUL
#define BH_FC_PK_CMUL 1
#endif
typedef float v2f_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf cmul(cf a, cf b) {
#if BH_FC_PK_CMUL
    v2f_t av = {a.x, a.y}, bv = {b.x, b.y}, t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(av), "v"(bv));                     // (a.x b.x, a.x b.y)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(av), "v"(bv), "v"(t));  // (-a.y b.y, a.y b.x) + t
    return make_float2(r.x, r.y);
#else
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
#endif
}
__device__ __forceinline__ cf cmulc(cf a, cf b) {  // a * conj(b)
#if BH_FC_PK_CMUL
    v2f_t av = {a.x, a.y}, bv = {b.x, b.y}, t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(av), "v"(bv));         // (a.x b.x, -a.x b.y)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(av), "v"(bv), "v"(t));      // (a.y b.y, a.y b.x) + t
    return make_float2(r.x, r.y);
#else
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
#endif
}
// a - i b and a + i b as ONE packed add each: v_pk_add_f32 takes either half of each source for each half of the result and can
// negate it.  The compiler's own lowering materialises (-i) b with two moves first — a fifth of the register FFT stages'
// instructions were such moves (fftconv_regfft.inc reg_fft, fftconv_colz.inc fwd8p / inv8p fold every rotation by -i / +i into
// the add or subtract that consumes it).
__host__ __device__ __forceinline__ cf add_mi(cf a, cf b) {
#if defined(__HIP_DEVICE_COMPILE__)
    v2f_t av = {a.x, a.y}, bv = {b.x, b.y}, r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(av), "v"(bv));
    return make_float2(r.x, r.y);
#else
    return make_float2(a.x + b.y, a.y - b.x);
#endif
}
__host__ __device__ __forceinline__ cf add_pi(cf a, cf b) {
#if defined(__HIP_DEVICE_COMPILE__)
    v2f_t av = {a.x, a.y}, bv = {b.x, b.y}, r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(av), "v"(bv));
    return make_float2(r.x, r.y);
#else
    return make_float2(a.x - b.y, a.y + b.x);
#endif
}
__device__ __forceinline__ cf cconj(cf a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ cf mul_mi(cf a) { return make_float2(a.y, -a.x); }  // a * (-i)
__device__ __forceinline__ cf mul_pi(cf a) { return make_float2(-a.y, a.x); }  // a * (+i)
__device__ __forceinline__ cf cscale(cf a, float s) { return make_float2(a.x * s, a.y * s); }

// ------------------------------------------------------------------------------------------------
// In-LDS, in-place FFT of W interleaved columns: element (n, c) at buf[n * P + c].
// Forward = decimation in frequency, natural in -> bit-reversed out.  Inverse = the mirrored
// decimation in time with conjugate twiddles, bit-reversed in -> natural out, unnormalised (x N).
// Radix-4 steps are two fused radix-2 levels; an odd log2(N) adds one radix-2 step (first fwd / last inv).
// Twiddle table (see make_twiddles): [radix-2: w_N^j, j < N/2 (only if log2 N odd)] then for each
// radix-4 step of half-size h (descending) and j < h/2: w_2h^j, w_2h^2j, w_2h^3j.
// ------------------------------------------------------------------------------------------------
// CPT = complex columns per thread (1: float2 accesses, any pitch; 2: float4 accesses, pitch even and
// 16-B aligned).  BPT = butterflies per thread and step, fully unrolled so that every LDS read of a step
// is in flight before the first butterfly is computed.
template <int CPT>
struct CV;
template <>
struct CV<1> {
    cf a;
    __device__ __forceinline__ static CV ld(const cf* p) { return CV{*p}; }
    __device__ __forceinline__ void st(cf* p) const { *p = a; }
};
template <>
struct CV<2> {
    cf a, b;
    __device__ __forceinline__ static CV ld(const cf* p) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        return CV{make_float2(v.x, v.y), make_float2(v.z, v.w)};
    }
    __device__ __forceinline__ void st(cf* p) const { *reinterpret_cast<float4*>(p) = make_float4(a.x, a.y, b.x, b.y); }
};

#define BH_CV_OP1(name, f)                                                                  \
    template <int CPT>                                                                      \
    __device__ __forceinline__ CV<CPT> name(const CV<CPT>& x);                              \
    template <>                                                                             \
    __device__ __forceinline__ CV<1> name<1>(const CV<1>& x) { return CV<1>{f(x.a)}; }      \
    template <>                                                                             \
    __device__ __forceinline__ CV<2> name<2>(const CV<2>& x) { return CV<2>{f(x.a), f(x.b)}; }
#define BH_CV_OP2(name, f)                                                                                    \
    template <int CPT>                                                                                        \
    __device__ __forceinline__ CV<CPT> name(const CV<CPT>& x, const CV<CPT>& y);                              \
    template <>                                                                                               \
    __device__ __forceinline__ CV<1> name<1>(const CV<1>& x, const CV<1>& y) { return CV<1>{f(x.a, y.a)}; }   \
    template <>                                                                                               \
    __device__ __forceinline__ CV<2> name<2>(const CV<2>& x, const CV<2>& y) {                                \
        return CV<2>{f(x.a, y.a), f(x.b, y.b)};                                                               \
    }
#define BH_CV_OPT(name, f)                                                                             \
    template <int CPT>                                                                                 \
    __device__ __forceinline__ CV<CPT> name(const CV<CPT>& x, cf t);                                   \
    template <>                                                                                        \
    __device__ __forceinline__ CV<1> name<1>(const CV<1>& x, cf t) { return CV<1>{f(x.a, t)}; }        \
    template <>                                                                                        \
    __device__ __forceinline__ CV<2> name<2>(const CV<2>& x, cf t) { return CV<2>{f(x.a, t), f(x.b, t)}; }
BH_CV_OP2(vadd, cadd)
BH_CV_OP2(vsub, csub)
BH_CV_OP1(vmul_mi, mul_mi)
BH_CV_OP1(vmul_pi, mul_pi)
BH_CV_OPT(vmul, cmul)
BH_CV_OPT(vmulc, cmulc)
#undef BH_CV_OP1
#undef BH_CV_OP2
#undef BH_CV_OPT

template <bool INV, int BPT, int CPT, int NT = FC_NT>
__device__ __forceinline__ void radix4_step(cf* buf, int N, int logW, int P, int h, const cf* t, int tid) {
    const int q = h >> 1;
    const int lw = logW - (CPT == 2 ? 1 : 0);       // log2 of column groups per row
    const int total = (N >> 2) << lw;
    const size_t qP = (size_t)q * P;
    // all threads run the same number of groups; ragged tails clamp the index and skip the store
    const bool ragged = (total % (BPT * NT)) != 0;
    for (int g0 = 0; g0 < total; g0 += BPT * NT) {
    CV<CPT> x0[BPT], x1[BPT], x2[BPT], x3[BPT];
    cf t1[BPT], t2[BPT], t3[BPT];
    cf* p0[BPT];
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        const int idx = min(g0 + tid + k * NT, total - 1);
        const int c = (idx & ((1 << lw) - 1)) * CPT;
        const int b = idx >> lw;
        const int j = b & (q - 1);
        const int i = ((b - j) << 2) + j;  // (b / q) * 2h + j
        p0[k] = buf + (size_t)i * P + c;
        x0[k] = CV<CPT>::ld(p0[k]);
        x1[k] = CV<CPT>::ld(p0[k] + qP);
        x2[k] = CV<CPT>::ld(p0[k] + 2 * qP);
        x3[k] = CV<CPT>::ld(p0[k] + 3 * qP);
        t1[k] = t[3 * j];
        t2[k] = t[3 * j + 1];
        t3[k] = t[3 * j + 2];
    }
    if (ragged) __syncthreads();  // clamped duplicates must all read before anyone writes
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        if (g0 + tid + k * NT < total) {
            if (!INV) {
                const CV<CPT> s02 = vadd<CPT>(x0[k], x2[k]), d02 = vsub<CPT>(x0[k], x2[k]);
                const CV<CPT> s13 = vadd<CPT>(x1[k], x3[k]), d13 = vmul_mi<CPT>(vsub<CPT>(x1[k], x3[k]));
                vadd<CPT>(s02, s13).st(p0[k]);
                vmul<CPT>(vsub<CPT>(s02, s13), t2[k]).st(p0[k] + qP);
                vmul<CPT>(vadd<CPT>(d02, d13), t1[k]).st(p0[k] + 2 * qP);
                vmul<CPT>(vsub<CPT>(d02, d13), t3[k]).st(p0[k] + 3 * qP);
            } else {
                const CV<CPT> u1 = vmulc<CPT>(x1[k], t2[k]), u2 = vmulc<CPT>(x2[k], t1[k]), u3 = vmulc<CPT>(x3[k], t3[k]);
                const CV<CPT> A = vadd<CPT>(x0[k], u1), B = vsub<CPT>(x0[k], u1);
                const CV<CPT> C = vadd<CPT>(u2, u3), D = vmul_pi<CPT>(vsub<CPT>(u2, u3));
                vadd<CPT>(A, C).st(p0[k]);
                vsub<CPT>(A, C).st(p0[k] + 2 * qP);
                vadd<CPT>(B, D).st(p0[k] + qP);
                vsub<CPT>(B, D).st(p0[k] + 3 * qP);
            }
        }
    }
    if (ragged) __syncthreads();
    }
}

// `rows` >= N: the buffer holds rows / N independent length-N sequences one after the other (see fft_lds)
template <bool INV, int BPT, int CPT, int NT = FC_NT>
__device__ __forceinline__ void radix2_step(cf* buf, int N, int logW, int P, const cf* t, int tid, int rows) {
    const int h = N >> 1;
    const int lw = logW - (CPT == 2 ? 1 : 0);
    const int total = (rows >> 1) << lw;
    const size_t hP = (size_t)h * P;
    constexpr int B2 = 2 * BPT;  // a radix-2 step has twice the butterflies of a radix-4 step
    const bool ragged = (total % (B2 * NT)) != 0;
    for (int g0 = 0; g0 < total; g0 += B2 * NT) {
    CV<CPT> a[B2], b[B2];
    cf w[B2];
    cf* pa[B2];
#pragma unroll
    for (int k = 0; k < B2; ++k) {
        const int idx = min(g0 + tid + k * NT, total - 1);
        const int c = (idx & ((1 << lw) - 1)) * CPT;
        const int jj = idx >> lw;
        const int j = jj & (h - 1);                 // butterfly within its sequence
        pa[k] = buf + (size_t)(((jj - j) << 1) + j) * P + c;
        a[k] = CV<CPT>::ld(pa[k]);
        b[k] = CV<CPT>::ld(pa[k] + hP);
        w[k] = t[j];
    }
    if (ragged) __syncthreads();
#pragma unroll
    for (int k = 0; k < B2; ++k) {
        if (g0 + tid + k * NT < total) {
            if (!INV) {
                vadd<CPT>(a[k], b[k]).st(pa[k]);
                vmul<CPT>(vsub<CPT>(a[k], b[k]), w[k]).st(pa[k] + hP);
            } else {
                const CV<CPT> ub = vmulc<CPT>(b[k], w[k]);
                vadd<CPT>(a[k], ub).st(pa[k]);
                vsub<CPT>(a[k], ub).st(pa[k] + hP);
            }
        }
    }
    if (ragged) __syncthreads();
    }
}

// Radix-3 step for a column of N = 3 L rows (L a power of two), two complex columns per thread.  Forward (decimation in
// frequency): rows (m, m + L, m + 2L) -> the three length-L sequences y_k[m] = (x[m] + w3^k x[m+L] + w3^2k x[m+2L]) w_N^(k m),
// left in rows [k L, (k + 1) L); their length-L transforms are X[3 j + k].  Inverse: the mirror image with conjugate
// twiddles, unnormalised.  t3[2 m] = w_N^m, t3[2 m + 1] = w_N^2m.
template <int CPT>
__device__ __forceinline__ CV<CPT> vscale(const CV<CPT>& x, float f);
template <>
__device__ __forceinline__ CV<1> vscale<1>(const CV<1>& x, float f) { return CV<1>{make_float2(x.a.x * f, x.a.y * f)}; }
template <>
__device__ __forceinline__ CV<2> vscale<2>(const CV<2>& x, float f) {
    return CV<2>{make_float2(x.a.x * f, x.a.y * f), make_float2(x.b.x * f, x.b.y * f)};
}
template <bool INV, int CPT = 2, int NT = FC_NT>
__device__ __forceinline__ void radix3_step(cf* buf, int L, int logW, int P, const cf* t3, int tid) {
    const int lw = logW - (CPT == 2 ? 1 : 0);
    const int total = L << lw;
    const size_t LP = (size_t)L * P;
    const float S3 = 0.86602540378443865f;
    for (int idx = tid; idx < total; idx += NT) {
        const int c = (idx & ((1 << lw) - 1)) * CPT;
        const int m = idx >> lw;
        cf* p0 = buf + (size_t)m * P + c;
        const CV<CPT> a = CV<CPT>::ld(p0);
        CV<CPT> b = CV<CPT>::ld(p0 + LP), cc = CV<CPT>::ld(p0 + 2 * LP);
        const cf w1 = t3[2 * m], w2 = t3[2 * m + 1];
        if (INV) {
            b = vmulc<CPT>(b, w1);
            cc = vmulc<CPT>(cc, w2);
        }
        const CV<CPT> sm = vadd<CPT>(b, cc), df = vsub<CPT>(b, cc);
        const CV<CPT> base = vsub<CPT>(a, vscale<CPT>(sm, 0.5f));
        const CV<CPT> rot = vscale<CPT>(INV ? vmul_pi<CPT>(df) : vmul_mi<CPT>(df), S3);
        vadd<CPT>(a, sm).st(p0);
        if (!INV) {
            vmul<CPT>(vadd<CPT>(base, rot), w1).st(p0 + LP);
            vmul<CPT>(vsub<CPT>(base, rot), w2).st(p0 + 2 * LP);
        } else {
            vadd<CPT>(base, rot).st(p0 + LP);
            vsub<CPT>(base, rot).st(p0 + 2 * LP);
        }
    }
}

// Radix-5 step, same conventions: rows (m, m + L, .., m + 4L) <-> the five length-L sequences y_k[m] = (sum_j x[m + jL] w5^jk) w_N^(k m)
// in rows [k L, (k + 1) L); t5[4 m + k - 1] = w_N^(k m), k = 1..4.
template <bool INV, int CPT = 2, int NT = FC_NT>
__device__ __forceinline__ void radix5_step(cf* buf, int L, int logW, int P, const cf* t5, int tid) {
    const int lw = logW - (CPT == 2 ? 1 : 0);
    const int total = L << lw;
    const size_t LP = (size_t)L * P;
    const float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f;  // cos(2 pi / 5), cos(4 pi / 5)
    const float S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;   // sin(2 pi / 5), sin(4 pi / 5)
    for (int idx = tid; idx < total; idx += NT) {
        const int c = (idx & ((1 << lw) - 1)) * CPT;
        const int m = idx >> lw;
        cf* p0 = buf + (size_t)m * P + c;
        const CV<CPT> x0 = CV<CPT>::ld(p0);
        CV<CPT> x1 = CV<CPT>::ld(p0 + LP), x2 = CV<CPT>::ld(p0 + 2 * LP), x3 = CV<CPT>::ld(p0 + 3 * LP), x4 = CV<CPT>::ld(p0 + 4 * LP);
        const cf w1 = t5[4 * m], w2 = t5[4 * m + 1], w3 = t5[4 * m + 2], w4 = t5[4 * m + 3];
        if (INV) {
            x1 = vmulc<CPT>(x1, w1);
            x2 = vmulc<CPT>(x2, w2);
            x3 = vmulc<CPT>(x3, w3);
            x4 = vmulc<CPT>(x4, w4);
        }
        const CV<CPT> t1 = vadd<CPT>(x1, x4), t2 = vadd<CPT>(x2, x3), t3 = vsub<CPT>(x1, x4), t4 = vsub<CPT>(x2, x3);
        const CV<CPT> a1 = vadd<CPT>(x0, vadd<CPT>(vscale<CPT>(t1, C1), vscale<CPT>(t2, C2)));
        const CV<CPT> a2 = vadd<CPT>(x0, vadd<CPT>(vscale<CPT>(t1, C2), vscale<CPT>(t2, C1)));
        const CV<CPT> b1 = vadd<CPT>(vscale<CPT>(t3, S1), vscale<CPT>(t4, S2));
        const CV<CPT> b2 = vsub<CPT>(vscale<CPT>(t3, S2), vscale<CPT>(t4, S1));
        const CV<CPT> r1 = INV ? vmul_pi<CPT>(b1) : vmul_mi<CPT>(b1), r2 = INV ? vmul_pi<CPT>(b2) : vmul_mi<CPT>(b2);
        vadd<CPT>(x0, vadd<CPT>(t1, t2)).st(p0);
        if (!INV) {
            vmul<CPT>(vadd<CPT>(a1, r1), w1).st(p0 + LP);
            vmul<CPT>(vadd<CPT>(a2, r2), w2).st(p0 + 2 * LP);
            vmul<CPT>(vsub<CPT>(a2, r2), w3).st(p0 + 3 * LP);
            vmul<CPT>(vsub<CPT>(a1, r1), w4).st(p0 + 4 * LP);
        } else {
            vadd<CPT>(a1, r1).st(p0 + LP);
            vadd<CPT>(a2, r2).st(p0 + 2 * LP);
            vsub<CPT>(a2, r2).st(p0 + 3 * LP);
            vsub<CPT>(a1, r1).st(p0 + 4 * LP);
        }
    }
}

// the odd first (forward) / last (inverse) step of an axis of rdx * 2^k, rdx = 3 or 5
template <bool INV, int CPT, int NT, int RDX>
__device__ __forceinline__ void odd_step(cf* buf, int L, int logW, int P, const cf* t, int tid) {
    if (RDX == 3) radix3_step<INV, CPT, NT>(buf, L, logW, P, t, tid);
    if (RDX == 5) radix5_step<INV, CPT, NT>(buf, L, logW, P, t, tid);
}

// SKIP2: leave out the h = 2 radix-4 step (last forward / first inverse; its twiddles are all 1) — the convolution
// passes run it fused with the spectral multiply in registers (the BH_MID macro of col_pass_kernel, fftconv_col.hip).
// rows: total rows in the buffer when it holds several length-N sequences back to back (the thirds of a 3 * 2^k column
// after radix3_step); every step then runs over all of them at once — the step functions take their butterfly count from
// `rows` and their geometry from the half-size h.  0 = one sequence.
template <bool INV, int BPT, int CPT, bool SKIP2 = false, int NT = FC_NT>
__device__ __forceinline__ void fft_lds(cf* buf, int N, int logN, int logW, int P, const cf* tw, int tid, int rows = 0) {
    if (rows == 0) rows = N;
    const bool odd = logN & 1;
    const int H0 = odd ? (N >> 2) : (N >> 1);
    const cf* t4 = tw + (odd ? (N >> 1) : 0);
    if (!INV) {
        if (odd) {
            radix2_step<false, BPT, CPT, NT>(buf, N, logW, P, tw, tid, rows);
            __syncthreads();
        }
        for (int h = H0; h >= (SKIP2 ? 8 : 2); h >>= 2) {
            radix4_step<false, BPT, CPT, NT>(buf, rows, logW, P, h, t4 + (2 * H0 - 2 * h), tid);
            __syncthreads();
        }
    } else {
        int h = SKIP2 ? 8 : 2;
        while (h <= H0) {
            radix4_step<true, BPT, CPT, NT>(buf, rows, logW, P, h, t4 + (2 * H0 - 2 * h), tid);
            __syncthreads();
            h <<= 2;
        }
        if (odd) {
            radix2_step<true, BPT, CPT, NT>(buf, N, logW, P, tw, tid, rows);
            __syncthreads();
        }
    }
}

inline int twiddle_count(int N) {
    int logN = 0;
    while ((1 << logN) < N) ++logN;
    const bool odd = logN & 1;
    const int H0 = odd ? N / 4 : N / 2;
    int n = odd ? N / 2 : 0;
    for (int h = H0; h >= 2; h /= 4) n += 3 * (h / 2);
    return n;
}

inline void make_twiddles(int N, std::vector<cf>& out) {
    int logN = 0;
    while ((1 << logN) < N) ++logN;
    const bool odd = logN & 1;
    const int H0 = odd ? N / 4 : N / 2;
    out.clear();
    if (odd)
        for (int j = 0; j < N / 2; ++j) {
            const double a = -2.0 * M_PI * j / N;
            out.push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
        }
    for (int h = H0; h >= 2; h /= 4)
        for (int j = 0; j < h / 2; ++j)
            for (int m = 1; m <= 3; ++m) {
                const double a = -2.0 * M_PI * (double)j * m / (2.0 * h);
                out.push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
            }
}

// position of frequency (M - k) when frequency k sits at bit-reversed position p
__device__ __forceinline__ int mirror_pos(int p) {
    if (p < 2) return p;
    const int top = 31 - __clz(p);
    return 3 * (1 << top) - 1 - p;
}

// ================================================================================================
// Column passes (Y: two length-Y/2 halves per z; Z: fused forward x OTF x inverse)
// ================================================================================================
// COL_CONV16: COL_CONV with the multiplier stored as bfloat16 pairs (4 B per complex bin, widened in registers, f32 products)
// COL_PCC: the phase cross-correlation product in the Z pass — tile <- otf * conj(tile) / norm * scale between the forward and
// the inverse transform (otf = the reference image's finished spectrum; norm per ColParams::pcc_norm)
enum ColMode { COL_FWD = 0, COL_INV = 1, COL_FWD_SCALE = 2, COL_CONV = 3, COL_CORR = 4, COL_FILTER = 5, COL_CONV16 = 6, COL_PCC = 7 };

// one bin of the phase cross-correlation product (estimate_stabilization.py:233-238): a * conj(b) / norm * scale
__device__ __forceinline__ float2 pcc_bin(float2 a, float2 b, int mode, float scale) {
    const float eps = 1.1920929e-07f;  // np.finfo(complex64).eps
    float2 p = make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
    if (mode == BH_PCC_NORM_NONE) return make_float2(p.x * scale, p.y * scale);
    if (mode == BH_PCC_NORM_CLASSIC) {
        const float nrm = hypotf(a.x, a.y) * hypotf(b.x, b.y);
        return make_float2((p.x / nrm) * scale, (p.y / nrm) * scale);
    }
    // magnitude: p / max(|p|, eps).  |p|^2 leaves the float range for the low frequencies of a large volume, so p is brought to
    // q = p 2^-e with max(|q.x|, |q.y|) in [1/2, 1) first: p / |p| = q / |q| is one reciprocal square root (1 ulp) and two
    // products instead of hypotf and two correctly rounded divisions — a fifth of the instructions, in the Z pass whose
    // arithmetic showed (6.5 ms against 5.1 ms for the complex product on the same bytes)
    const float big = fmaxf(fabsf(p.x), fabsf(p.y));
    const int e = big > 0.0f ? __builtin_amdgcn_frexp_expf(big) : 0;
    const float qx = __builtin_amdgcn_ldexpf(p.x, -e), qy = __builtin_amdgcn_ldexpf(p.y, -e);
    const float qq = qx * qx + qy * qy;  // in [1/4, 2) unless p == 0
    const float rs = __builtin_amdgcn_rsqf(qq);
    const float mag = __builtin_amdgcn_ldexpf(qq * rs, e);  // |p| (inf beyond the float range: still >= eps)
    if (mag >= eps) return make_float2(qx * (rs * scale), qy * (rs * scale));
    const float s = scale / eps;
    return make_float2(p.x * s, p.y * s);
}

struct ColParams {
    cf* S;
    const cf* otf;
    const cf* tw;       // twiddles for length N
    int ntw;
    int N, logN, W, logW;  // column length (rows of the tile), log2 of its power-of-two part L, tile width (complex columns)
    int L;              // N (power of two) or N / 3: the radix-3 step splits a 3 * 2^k column into three length-L transforms
    const cf* tw3;      // radix-3 twiddles (2 L entries) when L != N
    int XP;             // valid columns per row
    long row_stride;    // complex elements between consecutive n
    long outer_stride;  // base(o) = (o / nsub) * outer_stride + (o % nsub) * sub_stride
    long sub_stride;
    int nsub;
    int nouter;         // number of o values
    int ncoltiles;
    float scale;
    int midfuse;        // fuse the unit-twiddle steps around the spectral product (BH_FC_NOZMID=1 turns it off)
    int pcc_norm;       // COL_PCC: BH_PCC_NORM_* of the product (`scale` multiplies it)
    int pcc_swap;       // COL_PCC: 0 = otf * conj(column) (otf holds the FIRST image's spectrum), 1 = column * conj(otf)
    cf* otf_out;        // COL_PCC, may be null: the column's forward spectrum replaces the multiplier rows it has just read
                        // (the image becomes the stored one for the next call: bh_phase_cross_corr_apply's `roll`)
};

// ================================================================================================
// X passes: real rows <-> half-spectrum rows, with the Y radix-2 step across row pairs (y, y + Y/2)
// ================================================================================================
struct XParams {
    const float* in;      // forward: real input volume
    cf* S;                // spectrum
    float* out;           // inverse: real output volume
    const float* aux;     // inverse: d (ratio) or est (update)
    const cf* tw;         // twiddles for length M
    const cf* untangle;   // w_X^{brev(p)}, p < M
    const cf* twy;        // w_Y^y, y < Y/2
    const cf* tw3;        // radix-3 twiddles of the row transform (2 Lm entries) when M = 3 Lm
    int ntw;
    ConvDims d;
    float eps;
};

// modes and parameters of the wave-private X passes (kernels: fftconv_xw.inc, fftconv_x3.inc; what a mode implies:
// ModeOf in fftconv_xrows.inc); here because the drivers of fftconv.hip name the modes and build the wrap geometry
namespace xw {

// the _WRAP modes (both kernel families): Richardson-Lucy at a wrap-padded box without a fold pass — the epilogue's result is
// wrap-extended along x inside the row and along z by re-reading the source plane, out of place (Params::S_out, Params::wz / wx)
// INV_UPDATE_CROP: the last update of that loop — max(est * ., 0) stored straight into the UNPADDED output volume (rows of
// wx.n floats at any 4-byte alignment; planes / columns outside the volume are not stored): no crop pass
// INV_ARGMAX: the inverse transform is not stored at all — every wavefront keeps the first occurrence of max |.| of the rows it
// produced and writes one ArgMax to Params::out (an ArgMax[gridDim.x * NW] there): the phase cross-correlation's peak search
// without the correlation volume ever reaching memory
enum Mode { FWD = 0, INV_STORE = 1, INV_RATIO = 2, INV_UPDATE = 3, FUSED_RATIO = 4, FUSED_UPDATE = 5, FUSED_RATIO_WRAP = 6, FUSED_UPDATE_WRAP = 7,
            INV_UPDATE_CROP = 8, INV_ARGMAX = 9 };

struct Params {
    const float* in;   // FWD: real rows
    cf* S;             // spectrum rows (pitch XP)
    float* out;        // FWD: optional max(in, 0) copy; INV_*: real output; FUSED_UPDATE: the estimate; INV_ARGMAX: ArgMax partials
    const float* aux;  // d (ratio) or est (update)
    const cf* tab;     // [tw1 | tw2 | ut | ut1] (make_tables)
    const cf* twy;     // w_Y^y, y < Y/2
    int Z, Y, XP;
    float eps;
    const double* norm_mean;  // FWD only, may be null: transform x / mean - 1 instead of x (inten_normalization_3D fused into the load)
    double* rowsum;           // INV_UPDATE only, may be null: rowsum[z * Y + y] = sum over x of the row just stored (float64) — what
                              // the one-pass overhang fill of a deskew that follows needs of this volume (deskew_rows.inc)
    // _WRAP modes: the spectrum rows are read from S and written to S_out (a second buffer: a margin plane re-reads the plane it
    // mirrors, which another wavefront is overwriting), and the wrap geometry of the padded axes: the volume's N voxels sit at
    // box positions [off, off + N); the result is defined on rel = pos - off (pos - off - P when that is >= N + mhi) in
    // [-mlo, N + mhi) as the value at rel mod N, and is zero elsewhere
    cf* S_out;
    struct Wrap {
        int n, off, mlo, mhi;
    } wz, wx;
};

}  // namespace xw

// ================================================================================================
// host side
// ================================================================================================

inline int ilog2(long v) {
    int l = 0;
    while ((1l << l) < v) ++l;
    return l;
}

// A/B switches of the environment: env_off = the variable is set to 0, env_int = its integer value, or `dflt` when unset
inline bool env_off(const char* name) {
    const char* v = getenv(name);
    return v && atoi(v) == 0;
}
inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// launch `kern` on the context's stream with `lds` bytes of dynamic LDS (more than the 64 KiB a kernel gets unasked)
template <typename K, typename P>
int launch_lds(bh_ctx* ctx, K kern, int grid, int threads, size_t lds, const P& p) {
    BH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, ctx->stream, p);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

// ---- the kernel families: one translation unit each ----
// fftconv_col.hip: col_pass_kernel on a tile geometry filled in by launch_col
int launch_col_pass(bh_ctx* ctx, ColParams p, int mode);
// fftconv_colreg.hip: the column pass of an axis (picks colz / colz3 / colw, else launch_col_pass), the Z pass of one R-L
// convolution or correlation (direct z taps when zr >= 0), and the tables of the register-stage kernels: false = no such
// kernel for that column length
int launch_col(bh_ctx* ctx, const ConvPlan& pl, int mode, bool zaxis, cf* S, const cf* otf, float scale, int pcc_norm = 0,
               int pcc_swap = 0, cf* otf_out = nullptr);
int launch_rl_z(bh_ctx* ctx, const ConvPlan& pl, bool corr, bool otf_real, int zr, bool zreal, cf* S, const cf* otf);
bool colw_tables(int64_t n, std::vector<cf>& tab);
bool colz_tables(const ConvDims& d, std::vector<cf>& tab);
bool colz3_tables(const ConvDims& d, std::vector<cf>& tab);
// fftconv_xtile.hip: the tile-based X passes (xr16 / xr8 by ConvPlan::xr)
int launch_x_tile(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out, const float* aux,
                  float eps, bool fuse_fwd);
// fftconv_xw.hip: the wave-private X passes (xw / x3 by ConvPlan::x3), their tables and stored column order
void xw_tables(int64_t X, std::vector<cf>& tab, std::vector<int>& col);
int launch_xw(bh_ctx* ctx, const ConvPlan& pl, bool inverse, int epi, const float* in, cf* S, float* out, const float* aux,
              float eps, bool fuse_fwd, const double* norm_mean = nullptr);
int launch_xw_argmax(bh_ctx* ctx, const ConvPlan& pl, cf* S, ArgMax* partial, int* npartial);
int launch_xw_wrap(bh_ctx* ctx, const ConvPlan& pl, int mode, const cf* S_in, cf* S_out, float* out, const float* aux, float eps,
                   xw::Params::Wrap wz, xw::Params::Wrap wx);

}  // namespace bh
