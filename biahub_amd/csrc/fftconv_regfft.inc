// In-register butterflies and the small helpers every register-stage kernel family of the fused FFT engine uses: the
// wave-private X passes (fftconv_xw.inc, fftconv_x3.inc; included by fftconv_xw.hip) and the register-stage column passes
// (fftconv_colw.inc, fftconv_colz.inc, fftconv_colz3.inc; included by fftconv_colreg.hip).  The namespace is the X passes',
// where this code began; tools/xw_model.py checks the algebra of reg_fft.
namespace xw {

__host__ __device__ constexpr int parity(int v) {
    int p = 0;
    for (int b = 0; b < 16; ++b) p ^= (v >> b) & 1;
    return p;
}

__host__ __device__ __forceinline__ void xw_fence() {
    // LDS operations of one wavefront execute in order; this only pins the compiler's schedule around an exchange
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_wave_barrier();
#endif
    asm volatile("" ::: "memory");
}

// d * exp(-/+ 2 pi i k / 16), k in [0, 8) a compile-time constant after unrolling
template <bool INV>
__host__ __device__ __forceinline__ cf mulw16(cf d, int k) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R = 0.70710678118654752f;
    switch (k) {
        case 0: return d;
        case 4: return INV ? mul_pi(d) : mul_mi(d);
        case 2: return INV ? make_float2((d.x - d.y) * R, (d.x + d.y) * R) : make_float2((d.x + d.y) * R, (d.y - d.x) * R);
        case 6: return INV ? make_float2((-d.x - d.y) * R, (d.x - d.y) * R) : make_float2((d.y - d.x) * R, (-d.x - d.y) * R);
        default: {
            const float c = k == 1 ? C1 : (k == 3 ? S1 : (k == 5 ? -S1 : -C1));
            const float s = (k == 1 || k == 7) ? S1 : C1;
            return INV ? make_float2(d.x * c - d.y * s, d.x * s + d.y * c) : make_float2(d.x * c + d.y * s, d.y * c - d.x * s);
        }
    }
}

// in-register radix-2^LOGR transform of x[BASE + i * STRIDE], i < 2^LOGR.  Forward: decimation in frequency, natural in ->
// bit-reversed out; inverse: the mirrored decimation in time with conjugate twiddles, bit-reversed in -> natural out.
// reg_fft_levels is the definition (radix-2 levels with the rotations w_16^k applied one by one); reg_fft (BH_XW_PKROT, default)
// computes the same values with every rotation by -i / +i folded into the packed add / subtract that consumes it (add_mi /
// add_pi: one instruction instead of two moves and an add) and the eighth roots as (1 -+ i) R: the order of the outputs is
// unchanged, the results agree to rounding (tools/xw_model.py checks the algebra).
#ifndef BH_XW_PKROT
#define BH_XW_PKROT 1
#endif
template <int LOGR, int BASE, int STRIDE, bool INV, int NX>
__host__ __device__ __forceinline__ void reg_fft_levels(cf (&x)[NX]) {
    constexpr int R = 1 << LOGR;
    if (!INV) {
#pragma unroll
        for (int lh = LOGR - 1; lh >= 0; --lh) {
            const int h = 1 << lh;
#pragma unroll
            for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
                for (int j = 0; j < h; ++j) {
                    const int ia = BASE + (blk + j) * STRIDE, ib = BASE + (blk + j + h) * STRIDE;
                    const cf a = x[ia], b = x[ib];
                    x[ia] = cadd(a, b);
                    x[ib] = mulw16<false>(csub(a, b), j * (8 / h));
                }
            }
        }
    } else {
#pragma unroll
        for (int lh = 0; lh < LOGR; ++lh) {
            const int h = 1 << lh;
#pragma unroll
            for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
                for (int j = 0; j < h; ++j) {
                    const int ia = BASE + (blk + j) * STRIDE, ib = BASE + (blk + j + h) * STRIDE;
                    const cf a = x[ia], b = mulw16<true>(x[ib], j * (8 / h));
                    x[ia] = cadd(a, b);
                    x[ib] = csub(a, b);
                }
            }
        }
    }
}

constexpr float RQ = 0.70710678118654752f;
// radix-4 / radix-8 butterflies on four / eight values; ROT: the upper half of the inputs carries a pending factor -i
template <bool ROT>
__host__ __device__ __forceinline__ void r4_dif(cf& x0, cf& x1, cf& x2, cf& x3) {
    const cf s0 = ROT ? add_mi(x0, x2) : cadd(x0, x2), d0 = ROT ? add_pi(x0, x2) : csub(x0, x2);
    const cf s1 = ROT ? add_mi(x1, x3) : cadd(x1, x3), d1 = ROT ? add_pi(x1, x3) : csub(x1, x3);
    x0 = cadd(s0, s1);
    x1 = csub(s0, s1);
    x2 = add_mi(d0, d1);
    x3 = add_pi(d0, d1);
}
template <bool ROT>
__host__ __device__ __forceinline__ void r8_dif(cf& x0, cf& x1, cf& x2, cf& x3, cf& x4, cf& x5, cf& x6, cf& x7) {
    cf s0 = ROT ? add_mi(x0, x4) : cadd(x0, x4), d0 = ROT ? add_pi(x0, x4) : csub(x0, x4);
    cf s1 = ROT ? add_mi(x1, x5) : cadd(x1, x5), d1 = ROT ? add_pi(x1, x5) : csub(x1, x5);
    cf s2 = ROT ? add_mi(x2, x6) : cadd(x2, x6), d2 = ROT ? add_pi(x2, x6) : csub(x2, x6);
    cf s3 = ROT ? add_mi(x3, x7) : cadd(x3, x7), d3 = ROT ? add_pi(x3, x7) : csub(x3, x7);
    r4_dif<false>(s0, s1, s2, s3);
    cf f1 = cscale(add_mi(d1, d1), RQ), f3 = cscale(add_mi(d3, d3), RQ);  // w_8^1 d1, and i w_8^3 d3
    r4_dif<true>(d0, f1, d2, f3);
    x0 = s0, x1 = s1, x2 = s2, x3 = s3, x4 = d0, x5 = f1, x6 = d2, x7 = f3;
}
__host__ __device__ __forceinline__ void r4_dit(cf& x0, cf& x1, cf& x2, cf& x3) {
    const cf p0 = cadd(x0, x1), q0 = csub(x0, x1), p1 = cadd(x2, x3), q1 = csub(x2, x3);
    x0 = cadd(p0, p1);
    x1 = add_pi(q0, q1);
    x2 = csub(p0, p1);
    x3 = add_mi(q0, q1);
}
__host__ __device__ __forceinline__ void r8_dit(cf& x0, cf& x1, cf& x2, cf& x3, cf& x4, cf& x5, cf& x6, cf& x7) {
    r4_dit(x0, x1, x2, x3);
    r4_dit(x4, x5, x6, x7);
    const cf y1 = cscale(add_pi(x5, x5), RQ), e3 = cscale(add_pi(x7, x7), RQ);  // conj(w_8^1) x5, and -i conj(w_8^3) x7
    const cf u0 = x0, u1 = x1, u2 = x2, u3 = x3, v0 = x4, v2 = x6;
    x0 = cadd(u0, v0);
    x4 = csub(u0, v0);
    x1 = cadd(u1, y1);
    x5 = csub(u1, y1);
    x2 = add_pi(u2, v2);
    x6 = add_mi(u2, v2);
    x3 = add_pi(u3, e3);
    x7 = add_mi(u3, e3);
}

template <int LOGR, int BASE, int STRIDE, bool INV, int NX>
__host__ __device__ __forceinline__ void reg_fft(cf (&x)[NX]) {  // NX = 16 (fftconv_xw.inc, fftconv_colw.inc) or 24 (fftconv_x3.inc)
#define BH_X(i) x[BASE + (i) * STRIDE]
    if constexpr (!BH_XW_PKROT || LOGR < 2 || LOGR > 4) {
        reg_fft_levels<LOGR, BASE, STRIDE, INV, NX>(x);
    } else if constexpr (LOGR == 2) {
        if constexpr (!INV) r4_dif<false>(BH_X(0), BH_X(1), BH_X(2), BH_X(3));
        else r4_dit(BH_X(0), BH_X(1), BH_X(2), BH_X(3));
    } else if constexpr (LOGR == 3) {
        if constexpr (!INV) r8_dif<false>(BH_X(0), BH_X(1), BH_X(2), BH_X(3), BH_X(4), BH_X(5), BH_X(6), BH_X(7));
        else r8_dit(BH_X(0), BH_X(1), BH_X(2), BH_X(3), BH_X(4), BH_X(5), BH_X(6), BH_X(7));
    } else if constexpr (!INV) {
        // radix 16, forward: sums -> radix 8; differences d_j w_16^j -> radix 8 whose upper four inputs carry -i (w_16^(j+4) = -i w_16^j)
        cf d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const cf a = BH_X(j), b = BH_X(j + 8);
            BH_X(j) = cadd(a, b);
            d[j] = csub(a, b);
        }
        r8_dif<false>(BH_X(0), BH_X(1), BH_X(2), BH_X(3), BH_X(4), BH_X(5), BH_X(6), BH_X(7));
        d[1] = mulw16<false>(d[1], 1);
        d[5] = mulw16<false>(d[5], 1);
        d[2] = cscale(add_mi(d[2], d[2]), RQ);
        d[6] = cscale(add_mi(d[6], d[6]), RQ);
        d[3] = mulw16<false>(d[3], 3);
        d[7] = mulw16<false>(d[7], 3);
        r8_dif<true>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#pragma unroll
        for (int j = 0; j < 8; ++j) BH_X(j + 8) = d[j];
    } else {
        // radix 16, inverse: two radix-8 halves, then the upper one times conj(w_16^j), its elements 4..7 with the extra +i folded
        r8_dit(BH_X(0), BH_X(1), BH_X(2), BH_X(3), BH_X(4), BH_X(5), BH_X(6), BH_X(7));
        r8_dit(BH_X(8), BH_X(9), BH_X(10), BH_X(11), BH_X(12), BH_X(13), BH_X(14), BH_X(15));
        cf v[8];
        v[0] = BH_X(8);
        v[4] = BH_X(12);
        v[1] = mulw16<true>(BH_X(9), 1);
        v[5] = mulw16<true>(BH_X(13), 1);
        v[2] = cscale(add_pi(BH_X(10), BH_X(10)), RQ);
        v[6] = cscale(add_pi(BH_X(14), BH_X(14)), RQ);
        v[3] = mulw16<true>(BH_X(11), 3);
        v[7] = mulw16<true>(BH_X(15), 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const cf l = BH_X(j), l4 = BH_X(j + 4);
            BH_X(j) = cadd(l, v[j]);
            BH_X(j + 8) = csub(l, v[j]);
            BH_X(j + 4) = add_pi(l4, v[j + 4]);
            BH_X(j + 12) = add_mi(l4, v[j + 4]);
        }
    }
#undef BH_X
}

__host__ __device__ constexpr int brev_c(int v, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b)
        if (v >> b & 1) r |= 1 << (bits - 1 - b);
    return r;
}

__host__ __device__ __forceinline__ float4 pack2(cf a, cf b) { return make_float4(a.x, a.y, b.x, b.y); }

__device__ __forceinline__ int opaque_i(int v) {
    asm volatile("" : "+v"(v));  // the value looks loop-variant: address arithmetic built on it is not hoisted into registers
    return v;
}

}  // namespace xw
