// Wave-private X passes of the fused FFT engine (rows of 512, 1024 or 2048 voxels) — included by fftconv_xw.hip after
// fftconv_regfft.inc (the in-register butterflies) and fftconv_xrows.inc (the row-pair frame shared with fftconv_x3.inc: mode
// predicates, the rows of a pair, access addresses, Richardson-Lucy's value step).
//
// The tile-based X passes (fftconv_xpass.inc) keep 16 rows in one LDS tile and run every radix-4 step as an LDS round trip
// with a workgroup barrier: 14 round trips per fused pass, LDS- and barrier-bound at 38-50 % of the HBM rate
// (profiles/r01w_pmc_lds_conflicts.csv).  Here ONE WAVEFRONT owns a row pair (y, y + Y/2) from load to store:
//   * every lane keeps 16 complex points of each of the two rows in registers;
//   * the length-M transform (M = X/2) is three in-register stages — radix-8 over the top three index bits, radix-M/64 over
//     the middle bits, radix-8 over the low three — joined by two exchanges through a wave-private LDS buffer, so a
//     transform costs 2 LDS round trips instead of 5-6 and the kernel has no workgroup barrier at all (LDS operations of
//     one wavefront execute in order; `xw_fence` only stops the compiler from reordering across an exchange);
//   * untangle (real <-> packed complex), the Y radix-2 step across the row pair and the Richardson-Lucy epilogue run in
//     registers, in distributions chosen so that their partners sit in the same lane: at the spectrum end a lane holds an
//     8-point group of positions and the group holding the mirrored frequencies (M - k);
//   * global accesses are 16 B per lane and lane-contiguous at both ends.  The spectrum end achieves that by storing the
//     row in the order (register pair, lane): a fixed permutation of the columns [0, M) which only these kernels, the OTF
//     they produce and Tikhonov's filter staging (ConvPlan::xw_col) ever see.
// tools/xw_model.py is the executable specification of every index map, LDS address and twiddle table below (checked
// against numpy's FFT, with the LDS bank conflicts of every exchange priced by the rules of MI355X_MICROARCH.md).
namespace xw {

// (enum Mode and struct Params: fftconv_dev.hpp)
constexpr int NT = 512;       // 8 wavefronts per workgroup, one workgroup per CU, up to 256 VGPRs per lane
constexpr int NW = NT / 64;

template <int LOGM>
struct Geo {
    static constexpr int M = 1 << LOGM;
    static constexpr int LG = M / 16;            // lanes per row pair
    static constexpr int LOGLG = LOGM - 4;
    static constexpr int MIDBITS = LOGM - 6;     // middle stage: radix 16 (M = 1024) or 8 (M = 512)
    static constexpr int R2 = 1 << MIDBITS;
    static constexpr int NREP = 16 / R2;         // middle-stage groups per lane
    static constexpr int BLK = M / 8;            // points per top-3-bit block
    // + 8 words of padding per block; M = 256 runs four row pairs per wavefront, whose 64 padded row buffers would not fit
    // the 160 KiB of LDS: no padding there (1.2x the LDS cycles by tools/xw_model.py, rows of 512 voxels are small volumes)
    static constexpr int PADW = LOGM == 8 ? 0 : 8;
    static constexpr int BSTRIDE = BLK + PADW;
    static constexpr int ROWWORDS = 8 * BSTRIDE; // complex words per row buffer
    static constexpr int PAIRS = 64 / LG;        // row pairs per wavefront
    static constexpr int NTW1 = 7 * BLK, NTW2 = (R2 - 1) * 8, NUT = 8 * LG + 8;
    static constexpr int NTAB = NTW1 + NTW2 + NUT + (NTW2 & 1);  // keeps the row buffers 16-B aligned
    static constexpr size_t LDS_BYTES = ((size_t)NTAB + (size_t)NW * PAIRS * 2 * ROWWORDS) * 8;
};

// XOR swizzle of the four 16-B chunks of an 8-point group (tools/xw_model.py: `swz`)
__host__ __device__ constexpr int swz(int g) { return parity(g & 6) | (parity(g & 59) << 1); }

// complex-word address of array index i inside a row buffer
template <int LOGM>
__host__ __device__ __forceinline__ constexpr int lds_word(int i) {
    using G = Geo<LOGM>;
    const int blk = i >> (LOGM - 3), w = i & (G::BLK - 1);
    const int g = w >> 3, n = w & 7;
    const int gg = blk * (G::BLK / 8) + g;
    return blk * G::BSTRIDE + g * 8 + 2 * ((n >> 1) ^ swz(gg)) + (n & 1);
}

// the 8-point group a lane holds in slot sigma at the spectrum end: lane 0 owns the self-mirrored groups 0 and 1, lane
// lam >= 1 a group of the octave [2^(u+1), 2^(u+2)), u = floor(log2 lam), and the group of the mirrored frequencies
__host__ __device__ __forceinline__ constexpr int group_of(int lam, int sigma) {
    if (lam == 0) return sigma;
    int u = 0;
    while ((2 << u) <= lam) ++u;
    const int low = lam - (1 << u);
    return sigma == 0 ? ((2 << u) | low) : ((2 << u) | (1 << u) | (~low & ((1 << u) - 1)));
}
__host__ __device__ __forceinline__ int group_of_dev(int lam, int sigma) {
    if (lam == 0) return sigma;
    const int u = 31 - __builtin_clz((unsigned)lam);
    const int low = lam - (1 << u);
    return sigma == 0 ? ((2 << u) | low) : ((2 << u) | (1 << u) | (~low & ((1 << u) - 1)));
}

// array index held by (lane l, register rho) in the three distributions
template <int LOGM>
__host__ __device__ __forceinline__ int idx_dr(int l, int rho) {  // real side: rho = 2 r + b
    return (rho >> 1) * Geo<LOGM>::BLK + 2 * l + (rho & 1);
}
template <int LOGM>
__host__ __device__ __forceinline__ int idx_d2(int l, int rho) {  // middle stage: registers = middle bits (+ the top bit when R2 = 8)
    using G = Geo<LOGM>;
    constexpr int NX = 4 - G::MIDBITS;  // top-3 bits held in registers
    const int top = ((rho >> G::MIDBITS) << (3 - NX)) | (l >> 3);
    return top * G::BLK + (rho & (G::R2 - 1)) * 8 + (l & 7);
}
template <int LOGM>
__host__ __device__ __forceinline__ int idx_d3(int l, int rho) {  // spectrum end: rho = 8 sigma + n
    return 8 * group_of_dev(l, rho >> 3) + (rho & 7);
}

// ---- the three stages on the 16 registers of one row; `tw` tables live in LDS ----
// stage over the top three bits (real-side distribution): registers 2 r + b
template <int LOGM, bool INV>
__host__ __device__ __forceinline__ void stage_top1(cf (&x)[16], const cf* tw1, int l) {
    using G = Geo<LOGM>;
    if (!INV) {
        reg_fft<3, 0, 2, false>(x);
        reg_fft<3, 1, 2, false>(x);
    }
#pragma unroll
    for (int rp = 1; rp < 8; ++rp) {
        const int k = brev_c(rp, 3);
        const float4 w = *reinterpret_cast<const float4*>(tw1 + (k - 1) * G::BLK + 2 * l);  // w_M^(t k), t = 2 l and 2 l + 1
        const cf w0 = make_float2(w.x, w.y), w1 = make_float2(w.z, w.w);
        x[2 * rp] = INV ? cmulc(x[2 * rp], w0) : cmul(x[2 * rp], w0);
        x[2 * rp + 1] = INV ? cmulc(x[2 * rp + 1], w1) : cmul(x[2 * rp + 1], w1);
    }
    if (INV) {
        reg_fft<3, 0, 2, true>(x);
        reg_fft<3, 1, 2, true>(x);
    }
}
template <int LOGM, bool INV>
__host__ __device__ __forceinline__ void stage_top(cf (&xa)[16], cf (&xb)[16], const cf* tw1, int l) {
    using G = Geo<LOGM>;
    if (!INV) {
        reg_fft<3, 0, 2, false>(xa);
        reg_fft<3, 1, 2, false>(xa);
        reg_fft<3, 0, 2, false>(xb);
        reg_fft<3, 1, 2, false>(xb);
    }
#pragma unroll
    for (int rp = 1; rp < 8; ++rp) {
        const int k = brev_c(rp, 3);
        const float4 w = *reinterpret_cast<const float4*>(tw1 + (k - 1) * G::BLK + 2 * l);  // w_M^(t k), t = 2 l and 2 l + 1
        const cf w0 = make_float2(w.x, w.y), w1 = make_float2(w.z, w.w);
        if (!INV) {
            xa[2 * rp] = cmul(xa[2 * rp], w0);
            xa[2 * rp + 1] = cmul(xa[2 * rp + 1], w1);
            xb[2 * rp] = cmul(xb[2 * rp], w0);
            xb[2 * rp + 1] = cmul(xb[2 * rp + 1], w1);
        } else {
            xa[2 * rp] = cmulc(xa[2 * rp], w0);
            xa[2 * rp + 1] = cmulc(xa[2 * rp + 1], w1);
            xb[2 * rp] = cmulc(xb[2 * rp], w0);
            xb[2 * rp + 1] = cmulc(xb[2 * rp + 1], w1);
        }
    }
    if (INV) {
        reg_fft<3, 0, 2, true>(xa);
        reg_fft<3, 1, 2, true>(xa);
        reg_fft<3, 0, 2, true>(xb);
        reg_fft<3, 1, 2, true>(xb);
    }
}

template <int LOGM, bool INV, int REP>
__host__ __device__ __forceinline__ void stage_mid_fft(cf (&x)[16]) {
    using G = Geo<LOGM>;
    reg_fft<G::MIDBITS, REP * G::R2, 1, INV>(x);
    if constexpr (REP + 1 < G::NREP) stage_mid_fft<LOGM, INV, REP + 1>(x);
}
template <int LOGM, bool INV>
__host__ __device__ __forceinline__ void stage_mid(cf (&xa)[16], cf (&xb)[16], const cf* tw2, int l) {
    using G = Geo<LOGM>;
    if (!INV) {
        stage_mid_fft<LOGM, false, 0>(xa);
        stage_mid_fft<LOGM, false, 0>(xb);
    }
#pragma unroll
    for (int mp = 1; mp < G::R2; ++mp) {
        const int k1 = brev_c(mp, G::MIDBITS);
        const cf w = tw2[(k1 - 1) * 8 + (l & 7)];  // w_{M/8}^(n0 k1)
#pragma unroll
        for (int rep = 0; rep < G::NREP; ++rep) {
            const int i = rep * G::R2 + mp;
            xa[i] = INV ? cmulc(xa[i], w) : cmul(xa[i], w);
            xb[i] = INV ? cmulc(xb[i], w) : cmul(xb[i], w);
        }
    }
    if (INV) {
        stage_mid_fft<LOGM, true, 0>(xa);
        stage_mid_fft<LOGM, true, 0>(xb);
    }
}

template <bool INV>
__host__ __device__ __forceinline__ void stage_low(cf (&xa)[16], cf (&xb)[16]) {
    reg_fft<3, 0, 1, INV>(xa);
    reg_fft<3, 8, 1, INV>(xa);
    reg_fft<3, 0, 1, INV>(xb);
    reg_fft<3, 8, 1, INV>(xb);
}

// ---- exchanges through the wave-private row buffers ----
// Per-lane address state, in bytes from the start of row buffer a (row b = + ROWWORDS * 8).  The swizzle is XOR-linear in
// the group index, so every address is base + constant + ((constant chunk << 4) ^ lane chunk << 4): one v_xad_u32 per
// access instead of a hoisted address register per access.
struct LaneAddr {
    int dr_base, dr_c4;         // real side
    int d2_base, d2_c4;         // middle stage
    int d3_base[2], d3_c4[2];   // spectrum end, slots 0 / 1
};
template <int LOGM>
__host__ __device__ __forceinline__ LaneAddr lane_addr(int l) {
    using G = Geo<LOGM>;
    LaneAddr a;
    a.dr_base = (l >> 2) * 64;
    a.dr_c4 = ((l & 3) ^ swz(l >> 2)) << 4;
    a.d2_base = ((l >> 3) * G::BSTRIDE) * 8 + (l & 1) * 8;
    a.d2_c4 = (((l & 7) >> 1) ^ swz((l >> 3) * (G::BLK / 8))) << 4;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int g = group_of_dev(l, s);
        a.d3_base[s] = ((g >> (LOGM - 6)) * G::BSTRIDE + (g & (G::BLK / 8 - 1)) * 8) * 8;
        a.d3_c4[s] = swz(g) << 4;
    }
    return a;
}
template <int LOGM>
__host__ __device__ __forceinline__ int off_dr(const LaneAddr& a, int r) {  // 16 B: registers (2 r, 2 r + 1)
    using G = Geo<LOGM>;
    return a.dr_base + r * G::BSTRIDE * 8 + ((swz(r * (G::BLK / 8)) << 4) ^ a.dr_c4);
}
template <int LOGM>
__host__ __device__ __forceinline__ int off_d2(const LaneAddr& a, int rho) {  // 8 B: register rho
    using G = Geo<LOGM>;
    constexpr int NX = 4 - G::MIDBITS;
    const int toph = (rho >> G::MIDBITS) << (3 - NX), mid = rho & (G::R2 - 1);
    return a.d2_base + (toph * G::BSTRIDE + mid * 8) * 8 + (((swz(mid) ^ swz(toph * (G::BLK / 8))) << 4) ^ a.d2_c4);
}
__host__ __device__ __forceinline__ int off_d3(const LaneAddr& a, int c) {  // 16 B: registers (2 c, 2 c + 1), c = 4 sigma + q
    return a.d3_base[c >> 2] + (((c & 3) << 4) ^ a.d3_c4[c >> 2]);
}

template <int LOGM>
__host__ __device__ __forceinline__ void put_dr(unsigned char* buf, const cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int r = 0; r < 8; ++r) *reinterpret_cast<float4*>(buf + off_dr<LOGM>(a, r)) = pack2(x[2 * r], x[2 * r + 1]);
}
template <int LOGM>
__host__ __device__ __forceinline__ void get_dr(const unsigned char* buf, cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(buf + off_dr<LOGM>(a, r));
        x[2 * r] = make_float2(v.x, v.y);
        x[2 * r + 1] = make_float2(v.z, v.w);
    }
}
template <int LOGM>
__host__ __device__ __forceinline__ void put_d2(unsigned char* buf, const cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) *reinterpret_cast<cf*>(buf + off_d2<LOGM>(a, rho)) = x[rho];
}
template <int LOGM>
__host__ __device__ __forceinline__ void get_d2(const unsigned char* buf, cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) x[rho] = *reinterpret_cast<const cf*>(buf + off_d2<LOGM>(a, rho));
}
template <int LOGM>
__host__ __device__ __forceinline__ void put_d3(unsigned char* buf, const cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int c = 0; c < 8; ++c) *reinterpret_cast<float4*>(buf + off_d3(a, c)) = pack2(x[2 * c], x[2 * c + 1]);
}
template <int LOGM>
__host__ __device__ __forceinline__ void get_d3(const unsigned char* buf, cf (&x)[16], const LaneAddr& a) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(buf + off_d3(a, c));
        x[2 * c] = make_float2(v.x, v.y);
        x[2 * c + 1] = make_float2(v.z, v.w);
    }
}

// ---- untangle of the packed real transform in the spectrum-end registers (formulas: untangle_lds in fftconv_xpass.inc) ----
template <bool INV>
__host__ __device__ __forceinline__ void ut_pair(cf& a, cf& b, cf w) {
    const cf E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));   // (a + conj b) / 2
    const cf Dm = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));  // (a - conj b) / 2
    if (!INV) {
        const cf wO = cmul(w, mul_mi(Dm));
        a = cadd(E, wO);
        b = cconj(csub(E, wO));
    } else {
        const cf iO = mul_pi(cmulc(Dm, w));
        a = cadd(E, iO);
        b = cconj(csub(E, iO));
    }
}
// slot 0 register n pairs with slot 1 register 7 - n; lane 0 holds the two self-mirrored groups (positions 0..15).
// nyq: forward OUT (x = M bin, real), inverse IN.
template <int LOGM, bool INV>
__host__ __device__ __forceinline__ void untangle(cf (&x)[16], const cf* ut, int l, float& nyq) {
    using G = Geo<LOGM>;
    cf w[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) w[n] = ut[n * G::LG + l];  // w_X^f of the slot-0 positions
    if (l != 0) {
#pragma unroll
        for (int n = 0; n < 8; ++n) ut_pair<INV>(x[n], x[15 - n], w[n]);
    } else {
        const cf* u1 = ut + 8 * G::LG;  // w_X^f of positions 8..11
        if (!INV) {
            const cf z0 = x[0];
            x[0] = make_float2(z0.x + z0.y, 0.0f);
            nyq = z0.x - z0.y;
        } else {
            const float x0 = x[0].x;
            x[0] = make_float2(0.5f * (x0 + nyq), 0.5f * (x0 - nyq));
        }
        x[1] = cconj(x[1]);  // k = M/2
        ut_pair<INV>(x[2], x[3], w[2]);
        ut_pair<INV>(x[4], x[7], w[4]);
        ut_pair<INV>(x[5], x[6], w[5]);
        ut_pair<INV>(x[8], x[15], u1[0]);
        ut_pair<INV>(x[9], x[14], u1[1]);
        ut_pair<INV>(x[10], x[13], u1[2]);
        ut_pair<INV>(x[11], x[12], u1[3]);
    }
}

// forward: real-side registers -> spectrum-end registers; the inverse is split in two so that the kernel can issue the
// epilogue's global loads between the halves (their registers are then live across one stage, not three)
template <int LOGM>
__host__ __device__ __forceinline__ void transform_fwd(cf (&xa)[16], cf (&xb)[16], unsigned char* ba, const cf* tw1, const cf* tw2,
                                              int l, const LaneAddr& a) {
    unsigned char* bb = ba + Geo<LOGM>::ROWWORDS * 8;
    stage_top1<LOGM, false>(xa, tw1, l);  // row by row: the scheduler would otherwise interleave both rows' butterflies and
    put_dr<LOGM>(ba, xa, a);              // run out of registers next to the prefetched pair
    xw_fence();
    stage_top1<LOGM, false>(xb, tw1, l);
    put_dr<LOGM>(bb, xb, a);
    xw_fence();
    get_d2<LOGM>(ba, xa, a);
    get_d2<LOGM>(bb, xb, a);
    xw_fence();
    stage_mid<LOGM, false>(xa, xb, tw2, l);
    put_d2<LOGM>(ba, xa, a);
    put_d2<LOGM>(bb, xb, a);
    xw_fence();
    get_d3<LOGM>(ba, xa, a);
    get_d3<LOGM>(bb, xb, a);
    xw_fence();
    stage_low<false>(xa, xb);
}
template <int LOGM>
__host__ __device__ __forceinline__ void transform_inv_head(cf (&xa)[16], cf (&xb)[16], unsigned char* ba, const cf* tw2, int l,
                                                   const LaneAddr& a) {
    unsigned char* bb = ba + Geo<LOGM>::ROWWORDS * 8;
    stage_low<true>(xa, xb);
    put_d3<LOGM>(ba, xa, a);
    put_d3<LOGM>(bb, xb, a);
    xw_fence();
    get_d2<LOGM>(ba, xa, a);
    get_d2<LOGM>(bb, xb, a);
    xw_fence();
    stage_mid<LOGM, true>(xa, xb, tw2, l);
    put_d2<LOGM>(ba, xa, a);
    put_d2<LOGM>(bb, xb, a);
    xw_fence();
}
template <int LOGM>
__host__ __device__ __forceinline__ void transform_inv_tail(cf (&xa)[16], cf (&xb)[16], const unsigned char* ba, const cf* tw1,
                                                   int l, const LaneAddr& a) {
    const unsigned char* bb = ba + Geo<LOGM>::ROWWORDS * 8;
    get_dr<LOGM>(ba, xa, a);
    get_dr<LOGM>(bb, xb, a);
    xw_fence();
    stage_top<LOGM, true>(xa, xb, tw1, l);
}

// One row pair, register to register: the body of the kernel between its global loads and stores, shared with the host
// check (tools/xw_host_check.hip runs it lane by lane).  Phases are separate functions because a CPU emulation has to run
// each one for all lanes before the next; the kernel calls them back to back.
//
// inverse head: spectrum-end registers of rows A / B (as loaded) -> undo the Y step, untangle, first two inverse stages
template <int LOGM>
__host__ __device__ __forceinline__ void pair_inv_head(cf (&xa)[16], cf (&xb)[16], cf nya, cf nyb, cf wy, unsigned char* ba,
                                              const cf* tw2, const cf* ut, int l, const LaneAddr& a) {
    // X_a = A + conj(w) B, X_b = A - conj(w) B
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const cf u = cmulc(xb[i], wy), s = xa[i];
        xa[i] = cadd(s, u);
        xb[i] = csub(s, u);
    }
    const cf un = cmulc(nyb, wy);
    float na = nya.x + un.x, nb = nya.x - un.x;
    untangle<LOGM, true>(xa, ut, l, na);
    untangle<LOGM, true>(xb, ut, l, nb);
    transform_inv_head<LOGM>(xa, xb, ba, tw2, l, a);
}
// forward tail: spectrum-end registers after the forward transform -> untangle, Y step; returns the Nyquist bins of A / B
template <int LOGM>
__host__ __device__ __forceinline__ void pair_fwd_tail(cf (&xa)[16], cf (&xb)[16], cf& nyA, cf& nyB, cf wy, const cf* ut, int l) {
    float na = 0.f, nb = 0.f;
    untangle<LOGM, false>(xa, ut, l, na);
    untangle<LOGM, false>(xb, ut, l, nb);
    // A = X_a + X_b, B = (X_a - X_b) w_Y^y
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const cf s = cadd(xa[i], xb[i]), d = cmul(csub(xa[i], xb[i]), wy);
        xa[i] = s;
        xb[i] = d;
    }
    nyA = make_float2(na + nb, 0.f);
    nyB = cmul(make_float2(na - nb, 0.f), wy);
}

template <int LOGM, int MODE>
__global__ __launch_bounds__(NT) void xw_kernel(Params p) {
    using G = Geo<LOGM>;
    using MD = ModeOf<MODE>;
    constexpr int M = G::M, LG = G::LG, X = 2 * M;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* tab = reinterpret_cast<cf*>(smem);
    const int tid = threadIdx.x;
    for (int i = tid; i < G::NTW1 + G::NTW2 + G::NUT; i += NT) tab[i] = p.tab[i];
    __syncthreads();  // the only workgroup barrier: the twiddle tables are shared, everything else is wave-private
    const cf* tw1 = tab;
    const cf* tw2 = tab + G::NTW1;
    const cf* ut = tw2 + G::NTW2;
    // wave-uniform values stay in scalar registers: the wave index is made provably uniform, so the pair index, the row
    // pointers and the loop control below cost no vector registers; a lane adds its own byte offset to a scalar base
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int grp = lane / LG, l = lane % LG;
    unsigned char* ba = smem + (size_t)G::NTAB * 8 + (size_t)((wave * G::PAIRS + grp) * 2) * G::ROWWORDS * 8;
    const LaneAddr a0 = lane_addr<LOGM>(l);

    const int Yh = p.Y >> 1, XP = p.XP;
    const int npairs = p.Z * Yh;                    // host: < 2^31
    const int pstep = (int)gridDim.x * NW * G::PAIRS;
    // a wavefront's PAIRS row pairs are neighbours in y (Yh is a multiple of PAIRS): rows ra0 + grp and rb0 + grp
    const int laneS = grp * XP * 8 + l * 16;        // byte offset into a spectrum row pair
    const int laneR = grp * X * 4 + l * 16;         // byte offset into a real row pair
    cf* const Sdst = MD::WRAP ? p.S_out : p.S;

    // prefetch registers: the pair's two rows (spectrum rows for the inverse-first modes, real rows for FWD) + Nyquist bins
    float4 sa[8], sb[8];
    cf nya = make_float2(0.f, 0.f), nyb = nya;
    auto load_pair = [&](int pb) {
        const Rows r = rows_of<MD::WRAP>(p, pb, Yh);
        if (MD::HAS_INV) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                sa[c] = *at<float4>(p.S, r.sa_, XP * 8, laneS, c * LG * 16);
                sb[c] = *at<float4>(p.S, r.sb_, XP * 8, laneS, c * LG * 16);
            }
            nya = *reinterpret_cast<const cf*>(reinterpret_cast<const unsigned char*>(p.S) + r.sa_ * XP * 8 + (grp * XP * 8 + M * 8));
            nyb = *reinterpret_cast<const cf*>(reinterpret_cast<const unsigned char*>(p.S) + r.sb_ * XP * 8 + (grp * XP * 8 + M * 8));
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                sa[c] = *at<float4>(p.in, r.ra, X * 4, laneR, c * (G::BLK / 2) * 16);
                sb[c] = *at<float4>(p.in, r.rb, X * 4, laneR, c * (G::BLK / 2) * 16);
            }
        }
    };

    float best_v = -1.0f;  // INV_ARGMAX: this lane's running maximum of |.| and its flat index
    long best_i = 0;
    int pb = (blockIdx.x * NW + wave) * G::PAIRS;
    if (pb < npairs) load_pair(pb);
    for (; pb < npairs; pb += pstep) {
        LaneAddr a = a0;
        a.dr_c4 = opaque_i(a.dr_c4);
        a.d2_c4 = opaque_i(a.d2_c4);
        a.d3_c4[0] = opaque_i(a.d3_c4[0]);
        a.d3_c4[1] = opaque_i(a.d3_c4[1]);
        const Rows rw = rows_of<MD::WRAP>(p, pb, Yh);
        const cf wy = p.twy[rw.yy + grp];
        // the prefetch is unconditional (the last round re-reads its own pair): a conditional one would keep the old
        // registers alive through the whole body
        const int pnext = pb + pstep < npairs ? pb + pstep : pb;
        cf xa[16], xb[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {  // both layouts: float4 c holds registers (2 c, 2 c + 1)
            xa[2 * c] = make_float2(sa[c].x, sa[c].y);
            xa[2 * c + 1] = make_float2(sa[c].z, sa[c].w);
            xb[2 * c] = make_float2(sb[c].x, sb[c].y);
            xb[2 * c + 1] = make_float2(sb[c].z, sb[c].w);
        }
        if (MD::HAS_INV) {
            const cf nya_cur = nya, nyb_cur = nyb;  // this pair's Nyquist bins: the prefetch below overwrites the carried ones
            if (MODE == INV_STORE || MD::ARGMAX) load_pair(pnext);  // no epilogue operand: the next pair rides behind the whole inverse
            // this pair's d / est rows ride behind the inverse transform, ahead of its last stage
            float4 auxa[8], auxb[8];
            auto load_aux_a = [&]() {
#pragma unroll
                for (int r = 0; r < 8; ++r) auxa[r] = *at<float4>(p.aux, rw.sa_, X * 4, laneR, r * (G::BLK / 2) * 16);
            };
            auto load_aux_b = [&]() {
#pragma unroll
                for (int r = 0; r < 8; ++r) auxb[r] = *at<float4>(p.aux, rw.sb_, X * 4, laneR, r * (G::BLK / 2) * 16);
            };
            pair_inv_head<LOGM>(xa, xb, nya_cur, nyb_cur, wy, ba, tw2, ut, l, a);
            if (MD::RATIO || MD::UPDATE) {
                load_aux_a();
                load_aux_b();
            }
            // last inverse stage and epilogue, one row at a time: row b waits in its LDS buffer while row a's registers and
            // epilogue operands are live (natural order, real-side distribution: registers (2 r, 2 r + 1) = four
            // consecutive reals)
            const bool zero_plane = rw.zero;
            auto tail_row = [&](cf (&x)[16], const float4 (&aux)[8], const unsigned char* buf, long row) {
                // CROP: this row's plane and row inside the unpadded output volume (64-bit division once per row, not per store)
                const int zq = MD::CROP ? (int)(row / p.Y) - p.wz.off : 0;
                const long yq = MD::CROP ? row % p.Y + grp : 0;
                get_dr<LOGM>(buf, x, a);
                xw_fence();
                stage_top1<LOGM, true>(x, tw1, l);
                xw_fence();
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    float4 v = pack2(x[2 * r], x[2 * r + 1]);
                    if (MD::RATIO || MD::UPDATE) v = value_op<MODE>(v, aux[r], p.eps);
                    if (MD::ARGMAX) {
                        // four consecutive reals of row `row + grp`; a lane's indices do not ascend from pair to pair (row b
                        // lies Y/2 rows above row a), so ties are settled by the index
                        const float ax = fabsf(v.x), ay = fabsf(v.y), az = fabsf(v.z), aw = fabsf(v.w);
                        const float m = fmaxf(fmaxf(ax, ay), fmaxf(az, aw));
                        if (m >= best_v) {  // rare once a few rows have been seen
                            const int e = ax == m ? 0 : (ay == m ? 1 : (az == m ? 2 : 3));
                            const long i = (row + grp) * X + (2 * r * G::BLK + 4 * l + e);
                            if (m > best_v || i < best_i) {
                                best_v = m;
                                best_i = i;
                            }
                        }
                    }
                    if (MD::CROP) {
                        // row = z Y + y of the box; the volume's plane z - wz.off, same y (Y is not padded), columns - wx.off
                        const int xq = 2 * r * G::BLK + 4 * l - p.wx.off;
                        if (zq >= 0 && zq < p.wz.n) {
                            float* dst = p.out + ((long)zq * p.Y + yq) * p.wx.n + xq;
                            typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                            if (xq >= 0 && xq + 3 < p.wx.n) {
                                *reinterpret_cast<f4u*>(dst) = f4u{v.x, v.y, v.z, v.w};
                            } else {
                                const float v4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (xq + e >= 0 && xq + e < p.wx.n) dst[e] = v4[e];
                            }
                        }
                    } else if (MD::STORE_REAL && !MD::WRAP) *at_w<float4>(p.out, row, X * 4, laneR, r * (G::BLK / 2) * 16) = v;
                    x[2 * r] = make_float2(v.x, v.y);
                    x[2 * r + 1] = make_float2(v.z, v.w);
                }
                if (MODE == INV_UPDATE && p.rowsum != nullptr) {  // (wave-uniform) the stored row's sum: LG lanes hold it
                    // summed in float64 from the first value on: each stored float is exact in double, so the row sum is
                    // est.double().sum(-1) to float64 rounding, and the same as the deskew's own row_sums_kernel computes
                    double sd = 0.0;
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        sd += ((double)x[2 * r].x + (double)x[2 * r].y) + ((double)x[2 * r + 1].x + (double)x[2 * r + 1].y);
#pragma unroll
                    for (int o = LG / 2; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
                    if (l == 0) p.rowsum[row + grp] = sd;
                }
                if (MD::WRAP) {
                    // Wrap-extension along x inside the row, as in fftconv_x3.inc and kept in step with it (why it is written out
                    // per family: fftconv_xrows.inc): the epilogue's values are right on the volume's
                    // own voxels (box positions [off, off + n)); a margin position rel = pos - off in [-mlo, 0) takes the value
                    // of voxel rel + n, rel in [n, n + mhi) that of voxel rel - n, everything else is zero.  The two source
                    // strips travel through the start of the row's LDS buffer, free between the inverse's last read and the
                    // forward's first write; register pairs (2 r, 2 r + 1) hold the four reals 2 r BLK + 4 l .. + 3.
                    const int n = p.wx.n, off = p.wx.off, mlo = p.wx.mlo, mhi = p.wx.mhi;
                    float* scr = reinterpret_cast<float*>(const_cast<unsigned char*>(buf));
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int n0 = 2 * r * G::BLK - off, n1 = n0 + 2 * G::BLK;  // voxels of this register pair's block
                        if ((n1 > n - mlo && n0 < n) || (n0 < mhi && n1 > 0)) {
                            const float v4[4] = {x[2 * r].x, x[2 * r].y, x[2 * r + 1].x, x[2 * r + 1].y};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int nn = n0 + 4 * l + e;
                                if (nn >= n - mlo && nn < n) scr[nn - (n - mlo)] = v4[e];
                                if (nn >= 0 && nn < mhi) scr[mlo + nn] = v4[e];
                            }
                        }
                    }
                    xw_fence();
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int n0 = 2 * r * G::BLK - off, n1 = n0 + 2 * G::BLK;
                        if (n0 < 0 || n1 > n) {  // the block reaches outside the volume
                            float v4[4] = {x[2 * r].x, x[2 * r].y, x[2 * r + 1].x, x[2 * r + 1].y};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                int rel = n0 + 4 * l + e;
                                if (rel >= n + mhi) rel -= X;
                                const bool inside = rel >= 0 && rel < n, low = rel >= -mlo && rel < 0, high = rel >= n && rel < n + mhi;
                                const float m = scr[low ? rel + mlo : (high ? mlo + rel - n : 0)];
                                v4[e] = inside ? v4[e] : ((low || high) ? m : 0.0f);
                            }
                            x[2 * r] = make_float2(v4[0], v4[1]);
                            x[2 * r + 1] = make_float2(v4[2], v4[3]);
                        }
                    }
                    if (zero_plane) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) x[i] = make_float2(0.f, 0.f);
                    }
                    xw_fence();  // the scratch strips are read before the forward transform overwrites them
                    if (MD::STORE_REAL) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) *at_w<float4>(p.out, row, X * 4, laneR, r * (G::BLK / 2) * 16) = pack2(x[2 * r], x[2 * r + 1]);
                    }
                }
                xw_fence();
            };
            tail_row(xa, auxa, ba, rw.ra);
            tail_row(xb, auxb, ba + G::ROWWORDS * 8, rw.rb);
            if (MODE == INV_RATIO || MODE == INV_UPDATE || MD::CROP) load_pair(pnext);
        } else if (p.norm_mean) {  // phase reconstruction: x / mean - 1 on the way in
            const float inv = (float)(1.0 / *p.norm_mean);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                xa[i] = make_float2(xa[i].x * inv - 1.0f, xa[i].y * inv - 1.0f);
                xb[i] = make_float2(xb[i].x * inv - 1.0f, xb[i].y * inv - 1.0f);
            }
        } else if (p.out) {  // Richardson-Lucy start: e0 = max(d, 0) is stored and transformed in one pass
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                xa[2 * r] = make_float2(fmaxf(xa[2 * r].x, 0.f), fmaxf(xa[2 * r].y, 0.f));
                xa[2 * r + 1] = make_float2(fmaxf(xa[2 * r + 1].x, 0.f), fmaxf(xa[2 * r + 1].y, 0.f));
                xb[2 * r] = make_float2(fmaxf(xb[2 * r].x, 0.f), fmaxf(xb[2 * r].y, 0.f));
                xb[2 * r + 1] = make_float2(fmaxf(xb[2 * r + 1].x, 0.f), fmaxf(xb[2 * r + 1].y, 0.f));
                *at_w<float4>(p.out, rw.ra, X * 4, laneR, r * (G::BLK / 2) * 16) = pack2(xa[2 * r], xa[2 * r + 1]);
                *at_w<float4>(p.out, rw.rb, X * 4, laneR, r * (G::BLK / 2) * 16) = pack2(xb[2 * r], xb[2 * r + 1]);
            }
        }
        if (MD::HAS_FWD) {
            xw_fence();  // not earlier: above the epilogue these 64 registers would sit on top of its operands
            load_pair(pnext);  // the next pair's rows ride behind the forward transform
            xw_fence();
            transform_fwd<LOGM>(xa, xb, ba, tw1, tw2, l, a);
            cf nyA, nyB;
            pair_fwd_tail<LOGM>(xa, xb, nyA, nyB, wy, ut, l);
            // rows stored in (register pair, lane) order
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                *at_w<float4>(Sdst, rw.ra, XP * 8, laneS, c * LG * 16) = pack2(xa[2 * c], xa[2 * c + 1]);
                *at_w<float4>(Sdst, rw.rb, XP * 8, laneS, c * LG * 16) = pack2(xb[2 * c], xb[2 * c + 1]);
            }
            if (l < 16) {  // Nyquist column (lane 0) + the zero pad columns of the row pitch
                const cf zero = make_float2(0.f, 0.f);
                unsigned char* S8 = reinterpret_cast<unsigned char*>(Sdst);
                const int off = grp * XP * 8 + (M + l) * 8;
                *reinterpret_cast<cf*>(S8 + rw.ra * XP * 8 + off) = l == 0 ? nyA : zero;
                *reinterpret_cast<cf*>(S8 + rw.rb * XP * 8 + off) = l == 0 ? nyB : zero;
            }
        }
    }
    if (MD::ARGMAX) {  // every wavefront writes its slot (one that had no pair: {-1, 0})
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best_v, o);
            const long oi = ((long)__shfl_xor((int)(best_i >> 32), o) << 32) | (unsigned int)__shfl_xor((int)best_i, o);
            if (ov > best_v || (ov == best_v && oi < best_i)) {
                best_v = ov;
                best_i = oi;
            }
        }
        if (lane == 0) reinterpret_cast<ArgMax*>(p.out)[blockIdx.x * NW + wave] = ArgMax{best_v, (long long)best_i};
    }
}

// host: [tw1 [7][BLK] | tw2 [R2 - 1][8] | ut [8][LG] | ut1 [8]] and the stored column of every position
template <int LOGM>
static void make_tables(std::vector<cf>& tab, std::vector<int>& col_of_pos) {
    using G = Geo<LOGM>;
    constexpr int M = G::M;
    tab.assign(G::NTW1 + G::NTW2 + G::NUT, make_float2(0.f, 0.f));
    auto w = [](double num, double den) {
        const double a = -2.0 * M_PI * num / den;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int k = 1; k < 8; ++k)
        for (int t = 0; t < G::BLK; ++t) tab[(size_t)(k - 1) * G::BLK + t] = w((double)t * k, M);
    for (int k1 = 1; k1 < G::R2; ++k1)
        for (int n0 = 0; n0 < 8; ++n0) tab[G::NTW1 + (size_t)(k1 - 1) * 8 + n0] = w((double)n0 * k1, G::BLK);
    auto utw = [&](int pos) { return w((double)brev_c(pos, LOGM), 2.0 * M); };  // w_X^f, f = the frequency at position pos
    for (int n = 0; n < 8; ++n)
        for (int lam = 0; lam < G::LG; ++lam) tab[G::NTW1 + G::NTW2 + (size_t)n * G::LG + lam] = utw(8 * group_of(lam, 0) + n);
    for (int k = 0; k < 4; ++k) tab[G::NTW1 + G::NTW2 + 8 * G::LG + k] = utw(8 + k);
    col_of_pos.assign(M, 0);
    for (int lam = 0; lam < G::LG; ++lam)
        for (int sigma = 0; sigma < 2; ++sigma)
            for (int n = 0; n < 8; ++n)
                col_of_pos[8 * group_of(lam, sigma) + n] = 2 * ((4 * sigma + (n >> 1)) * G::LG + lam) + (n & 1);
}

}  // namespace xw
