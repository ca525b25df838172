// Radix-3 wave-private X passes of the fused FFT engine: rows of 1536 or 3072 voxels (packed complex transforms of
// M = 3 L points, L = 256 or 512) — included by fftconv_xw.hip after fftconv_regfft.inc (the in-register butterflies) and
// fftconv_xrows.inc (the row-pair frame shared with fftconv_xw.inc: mode predicates, the rows of a pair, access addresses,
// Richardson-Lucy's value step).
//
// A deskewed volume never has power-of-two rows: the wrap-padded engine box of BASELINE config 4's (342, 1024, 1517) volume is
// (384, 1024, 1536), that of config 2's (683, 2048, 3034) is (768, 2048, 3072).  Those rows used to take the tile kernels of
// fftconv_xpass.inc (LDS- and barrier-bound, 26 % of the LDS cycles in bank conflicts).  Here, as in fftconv_xw.inc, ONE
// WAVEFRONT owns a row pair (y, y + Y/2) from load to store:
//   * LG = L / 8 lanes (32 or 64) hold a row as 3 thirds x 8 registers; elements m, m + L, m + 2 L sit in one lane, so the
//     decimation-in-frequency radix-3 step that splits the row into three length-L transforms is register arithmetic;
//   * each third then takes three in-register stages — radix-8 over the top three index bits, radix-8 (L = 512) or radix-4
//     (L = 256) over the middle bits, radix-8 over the low three — joined by two exchanges through a wave-private LDS
//     buffer (no workgroup barrier: LDS operations of one wavefront execute in order);
//   * third t ends up holding the frequencies 3 j + t at the bit-reversed position of j — the order the tile kernels leave
//     such rows in, so the column passes, OTFs and staged filters do not see which kernel family ran (ConvPlan::xw_col maps
//     positions to stored columns);
//   * at the spectrum end a lane holds ONE 8-point group of each third.  The untangle of the packed real transform pairs
//     frequency f with M - f: thirds 1 and 2 mirror into each other (position p <-> L - 1 - p), so the lane that holds
//     group g of third 1 holds group LG - 1 - g of third 2; third 0 mirrors into itself, and its groups are dealt out so that
//     the mirrored group sits in the neighbouring lane (lane ^ 1: one DPP quad-permute per register; lanes 0 and 1 hold the
//     two self-mirrored groups 0 and 1 and pair inside the lane);
//   * spectrum rows are stored 16 B per lane, lane-contiguous, in (third, register pair, lane) order; real rows move 8 B per
//     lane (one complex = two consecutive reals of each of the lane's 24 block positions), 256 / 512 contiguous bytes per
//     wave instruction.
// tools/x3_model.py is the executable specification (index maps, LDS addresses with their bank-conflict prices, twiddle
// tables, untangle pairing, stored column order), checked against numpy's FFT in the CPU suite.
namespace x3 {

// modes, parameters, the butterflies of fftconv_regfft.inc and the row-pair frame of fftconv_xrows.inc; what this file
// declares under the same name as fftconv_xw.inc (Geo, LaneAddr, swz, reg_fft, untangle, ...) hides that one here
using namespace xw;

#ifndef BH_X3_NW
#define BH_X3_NW 4  // wavefronts per workgroup (one workgroup per CU): 6 row buffers of 4.5 KiB per pair leave room for 4-5
#endif
constexpr int NW = BH_X3_NW;
constexpr int NT = NW * 64;

template <int LOGL>
struct Geo {
    static constexpr int L = 1 << LOGL;
    static constexpr int M = 3 * L;
    static constexpr int LG = L / 8;              // lanes per row pair
    static constexpr int BLK = L / 8;             // points per top-3-bit block (lane l <-> element l of a block)
    static constexpr int MIDBITS = LOGL - 6;      // middle stage: radix 8 (L = 512) or 4 (L = 256)
    static constexpr int R2 = 1 << MIDBITS;
    static constexpr int NREP = 8 / R2;           // middle-stage groups per lane and third
    static constexpr int BSTRIDE = BLK + 8;       // + 8 words of padding per block
    static constexpr int ROWWORDS = 8 * BSTRIDE;  // complex words of one third of one row
    static constexpr int ROWB = ROWWORDS * 8;     // ... in bytes
    static constexpr int PAIRS = 64 / LG;         // row pairs per wavefront
    static constexpr int NTW1 = 7 * BLK, NTW2 = (R2 - 1) * 8, NTW3 = 2 * L, NUT = 8 * LG;
    static constexpr int NTAB = NTW1 + NTW2 + NTW3 + 2 * NUT;  // [tw1 | tw2 | tw3 | ut0 | ut1]; even: row buffers 16-B aligned
    static constexpr size_t LDS_BYTES = ((size_t)NTAB + (size_t)NW * PAIRS * 6 * ROWWORDS) * 8;
};

// XOR swizzle of the four 16-B chunks of an 8-point group (tools/x3_model.py: found by search per L)
template <int LOGL>
__host__ __device__ constexpr int swz(int g) {
    return LOGL == 8 ? (parity(g & 1) | (parity(g & 2) << 1)) : (parity(g & 2) | (parity(g & 20) << 1));
}

// lane -> 8-point group of third t at the spectrum end
__host__ __device__ constexpr int group0_c(int l) {
    if (l < 2) return l;
    const int k = l >> 1;
    int v = 0;
    while ((1 << v) <= k) ++v;  // floor(log2 k) + 1
    const int low = k - (1 << (v - 1));
    return (l & 1) == 0 ? ((1 << v) + low) : ((2 << v) - 1 - low);
}
__host__ __device__ __forceinline__ int group0_dev(int l) {
    if (l < 2) return l;
    const int k = l >> 1;
    const int v = 32 - __builtin_clz((unsigned)k);
    const int low = k - (1 << (v - 1));
    return (l & 1) == 0 ? ((1 << v) + low) : ((2 << v) - 1 - low);
}
template <int LOGL>
__host__ __device__ __forceinline__ int group_of(int t, int l) {
    return t == 0 ? group0_dev(l) : (t == 1 ? l : Geo<LOGL>::LG - 1 - l);
}

// in-register radix-2^LOGR transform of x[BASE + i * STRIDE]: xw::reg_fft on a 24-register row
template <int LOGR, int BASE, int STRIDE, bool INV>
__host__ __device__ __forceinline__ void reg_fft(cf (&x)[24]) {
    xw::reg_fft<LOGR, BASE, STRIDE, INV, 24>(x);
}

// ---- per-lane LDS byte offsets inside one third's buffer (thirds of row a at t * ROWB, of row b at (3 + t) * ROWB) ----
struct LaneAddr {
    int da_base, da_c4;        // real side / stage A
    int db_base, db_c4;        // stage B
    int dc_base[3], dc_c4[3];  // spectrum end, per third
};
template <int LOGL>
__host__ __device__ __forceinline__ LaneAddr lane_addr(int l) {
    using G = Geo<LOGL>;
    LaneAddr a;
    a.da_base = (l >> 3) * 64 + (l & 1) * 8;
    a.da_c4 = (((l & 7) >> 1) ^ swz<LOGL>(l >> 3)) << 4;
    a.db_base = ((l >> 3) * G::BSTRIDE) * 8 + (l & 1) * 8;
    a.db_c4 = (((l & 7) >> 1) ^ swz<LOGL>((l >> 3) * (G::BLK / 8))) << 4;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int g = group_of<LOGL>(t, l);
        a.dc_base[t] = ((g / (G::BLK / 8)) * G::BSTRIDE + (g % (G::BLK / 8)) * 8) * 8;
        a.dc_c4[t] = swz<LOGL>(g) << 4;
    }
    return a;
}
template <int LOGL>
__host__ __device__ __forceinline__ int off_da(const LaneAddr& a, int rho) {  // 8 B: register rho
    using G = Geo<LOGL>;
    return a.da_base + rho * G::BSTRIDE * 8 + ((swz<LOGL>(rho * (G::BLK / 8)) << 4) ^ a.da_c4);
}
template <int LOGL>
__host__ __device__ __forceinline__ int off_db(const LaneAddr& a, int rho) {  // 8 B: register rho
    using G = Geo<LOGL>;
    constexpr int NX = 3 - G::MIDBITS;  // top bits held in registers
    const int toph = (rho >> G::MIDBITS) << (3 - NX), mid = rho & (G::R2 - 1);
    return a.db_base + (toph * G::BSTRIDE + mid * 8) * 8 + (((swz<LOGL>(mid) ^ swz<LOGL>(toph * (G::BLK / 8))) << 4) ^ a.db_c4);
}
__host__ __device__ __forceinline__ int off_dc(const LaneAddr& a, int t, int q) {  // 16 B: registers (2 q, 2 q + 1) of third t
    return a.dc_base[t] + ((q << 4) ^ a.dc_c4[t]);
}

// thirds t of one row: registers x[8 t .. 8 t + 7]; buf = the row's first third buffer
template <int LOGL>
__host__ __device__ __forceinline__ void put_da(unsigned char* buf, const cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) *reinterpret_cast<cf*>(buf + t * Geo<LOGL>::ROWB + off_da<LOGL>(a, rho)) = x[8 * t + rho];
}
template <int LOGL>
__host__ __device__ __forceinline__ void get_da(const unsigned char* buf, cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) x[8 * t + rho] = *reinterpret_cast<const cf*>(buf + t * Geo<LOGL>::ROWB + off_da<LOGL>(a, rho));
}
template <int LOGL>
__host__ __device__ __forceinline__ void put_db(unsigned char* buf, const cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) *reinterpret_cast<cf*>(buf + t * Geo<LOGL>::ROWB + off_db<LOGL>(a, rho)) = x[8 * t + rho];
}
template <int LOGL>
__host__ __device__ __forceinline__ void get_db(const unsigned char* buf, cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) x[8 * t + rho] = *reinterpret_cast<const cf*>(buf + t * Geo<LOGL>::ROWB + off_db<LOGL>(a, rho));
}
template <int LOGL>
__host__ __device__ __forceinline__ void put_dc(unsigned char* buf, const cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(buf + t * Geo<LOGL>::ROWB + off_dc(a, t, q)) = pack2(x[8 * t + 2 * q], x[8 * t + 2 * q + 1]);
}
template <int LOGL>
__host__ __device__ __forceinline__ void get_dc(const unsigned char* buf, cf (&x)[24], const LaneAddr& a, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(buf + t * Geo<LOGL>::ROWB + off_dc(a, t, q));
        x[8 * t + 2 * q] = make_float2(v.x, v.y);
        x[8 * t + 2 * q + 1] = make_float2(v.z, v.w);
    }
}

// ---- stages on the 8 registers of third T of one row ----
// stage A: radix-8 over the top three bits; outer twiddle w_L^(l k), k = brev3(register), handed in as wA[k - 1]
template <int T, bool INV>
__host__ __device__ __forceinline__ void stage_a(cf (&x)[24], const cf (&wA)[7]) {
    if (!INV) reg_fft<3, 8 * T, 1, false>(x);
#pragma unroll
    for (int rp = 1; rp < 8; ++rp) {
        const cf w = wA[brev_c(rp, 3) - 1];
        x[8 * T + rp] = INV ? cmulc(x[8 * T + rp], w) : cmul(x[8 * T + rp], w);
    }
    if (INV) reg_fft<3, 8 * T, 1, true>(x);
}
// stage B: radix-R2 over the middle bits (NREP groups); outer twiddle w_BLK^(n0 k1) = wB[k1 - 1]
template <int LOGL, int T, bool INV>
__host__ __device__ __forceinline__ void stage_b(cf (&x)[24], const cf (&wB)[7]) {
    using G = Geo<LOGL>;
    if (!INV) {
        reg_fft<G::MIDBITS, 8 * T, 1, false>(x);
        if constexpr (G::NREP == 2) reg_fft<G::MIDBITS, 8 * T + 4, 1, false>(x);
    }
#pragma unroll
    for (int mp = 1; mp < G::R2; ++mp) {
        const cf w = wB[brev_c(mp, G::MIDBITS) - 1];
#pragma unroll
        for (int rep = 0; rep < G::NREP; ++rep) {
            const int i = 8 * T + rep * G::R2 + mp;
            x[i] = INV ? cmulc(x[i], w) : cmul(x[i], w);
        }
    }
    if (INV) {
        reg_fft<G::MIDBITS, 8 * T, 1, true>(x);
        if constexpr (G::NREP == 2) reg_fft<G::MIDBITS, 8 * T + 4, 1, true>(x);
    }
}
template <int T, bool INV>
__host__ __device__ __forceinline__ void stage_c(cf (&x)[24]) {
    reg_fft<3, 8 * T, 1, INV>(x);
}

// radix-3 step across the thirds on the real-side registers: rho-th element m = rho BLK + l of every third.
// Forward: (x[m], x[m + L], x[m + 2L]) -> (y0, y1 w_M^m, y2 w_M^2m); inverse: the mirror image with conjugate twiddles
// (unnormalised).  tw3[m] = w_M^m, tw3[L + m] = w_M^2m.
template <int LOGL, bool INV>
__host__ __device__ __forceinline__ void radix3(cf (&x)[24], const cf* tw3, int l) {
    using G = Geo<LOGL>;
    const float S3 = 0.86602540378443865f;
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) {
        const int m = rho * G::BLK + l;
        const cf w1 = tw3[m], w2 = tw3[G::L + m];
        const cf a = x[rho];
        cf b = x[8 + rho], c = x[16 + rho];
        if (INV) {
            b = cmulc(b, w1);
            c = cmulc(c, w2);
        }
        const cf sm = cadd(b, c), df = csub(b, c);
        const cf base = make_float2(a.x - 0.5f * sm.x, a.y - 0.5f * sm.y);
        const cf r0 = INV ? mul_pi(df) : mul_mi(df);
        const cf rot = make_float2(r0.x * S3, r0.y * S3);
        x[rho] = cadd(a, sm);
        if (!INV) {
            x[8 + rho] = cmul(cadd(base, rot), w1);
            x[16 + rho] = cmul(csub(base, rot), w2);
        } else {
            x[8 + rho] = cadd(base, rot);
            x[16 + rho] = csub(base, rot);
        }
    }
}

// ---- untangle of the packed real transform in the spectrum-end registers ----
// own element a (frequency f), mirrored element b (frequency M - f), w = w_X^f: the new a (both lanes of a pair run this on
// their own element: tools/x3_model.py own_fwd / own_inv)
template <bool INV>
__host__ __device__ __forceinline__ cf ut_own(cf a, cf b, cf w) {
    const cf E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));   // (a + conj b) / 2
    const cf Dm = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));  // (a - conj b) / 2
    if (!INV) return cadd(E, cmul(w, mul_mi(Dm)));
    return cadd(E, mul_pi(cmulc(Dm, w)));
}
// both elements of an in-lane pair at once (xw::ut_pair): a at frequency f, b at M - f
template <bool INV>
__host__ __device__ __forceinline__ void ut_pair(cf& a, cf& b, cf w) {
    const cf E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const cf Dm = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));
    const cf o = INV ? mul_pi(cmulc(Dm, w)) : cmul(w, mul_mi(Dm));
    a = cadd(E, o);
    b = cconj(csub(E, o));
}
// the value of `v` in lane ^ 1 (DPP quad_perm [1, 0, 3, 2]); on the host (tools) the caller supplies the partner itself
__device__ __forceinline__ float swap1(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
// nyq: forward OUT (the x = M bin, real), inverse IN.  w0[n]: w_X^f of this lane's element n of third 0; w1[n]: of third 1.
template <bool INV>
__device__ __forceinline__ void untangle(cf (&x)[24], const cf (&w0)[8], const cf (&w1)[8], int l, float& nyq) {
    // thirds 1 <-> 2: register n of third 1 pairs with register 7 - n of third 2, in this lane
#pragma unroll
    for (int n = 0; n < 8; ++n) ut_pair<INV>(x[8 + n], x[16 + 7 - n], w1[n]);
    // third 0: the mirrored element is register 7 - n of lane ^ 1 ...
    cf b[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) b[n] = make_float2(swap1(x[7 - n].x), swap1(x[7 - n].y));
    const cf x0 = x[0], x1 = x[1];
    if (l < 2) {  // ... except in lanes 0 / 1, which hold the self-mirrored groups 0 / 1 (positions 0..7 / 8..15)
        if (l == 1) {
#pragma unroll
            for (int n = 0; n < 8; ++n) b[n] = x[7 - n];
        } else {
            b[2] = x[3], b[3] = x[2], b[4] = x[7], b[5] = x[6], b[6] = x[5], b[7] = x[4];
        }
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = ut_own<INV>(x[n], b[n], w0[n]);
    if (l == 0) {  // position 0: the DC / Nyquist pair packed into one complex value; position 1: f = M / 2
        if (!INV) {
            x[0] = make_float2(x0.x + x0.y, 0.0f);
            nyq = x0.x - x0.y;
        } else {
            x[0] = make_float2(0.5f * (x0.x + nyq), 0.5f * (x0.x - nyq));
        }
        x[1] = cconj(x1);
    }
}

template <int LOGL, int MODE>
__global__ __launch_bounds__(NT) void x3_kernel(Params p) {
    using G = Geo<LOGL>;
    using MD = ModeOf<MODE>;
    constexpr int M = G::M, LG = G::LG, X = 2 * M, L = G::L;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* tab = reinterpret_cast<cf*>(smem);
    const int tid = threadIdx.x;
    for (int i = tid; i < G::NTAB; i += NT) tab[i] = p.tab[i];
    __syncthreads();  // the only workgroup barrier: the tables are shared, everything else is wave-private
    const cf* tw1 = tab;
    const cf* tw2 = tw1 + G::NTW1;
    const cf* tw3 = tw2 + G::NTW2;
    const cf* ut0 = tw3 + G::NTW3;
    const cf* ut1 = ut0 + G::NUT;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int grp = lane / LG, l = lane % LG;
    unsigned char* ba = smem + (size_t)G::NTAB * 8 + (size_t)((wave * G::PAIRS + grp) * 6) * G::ROWB;  // row a; row b = + 3 ROWB
    unsigned char* bb = ba + 3 * G::ROWB;
    const LaneAddr a0 = lane_addr<LOGL>(l);

    const int Yh = p.Y >> 1, XP = p.XP;
    const int npairs = p.Z * Yh;  // host: < 2^31
    const int pstep = (int)gridDim.x * NW * G::PAIRS;
    const int laneS = grp * XP * 8 + l * 16;  // byte offset into a spectrum row pair
    const int laneR = grp * X * 4 + l * 8;    // byte offset into a real row pair
    cf* const Sdst = MD::WRAP ? p.S_out : p.S;
    // real-side element (third t, register rho) = complex index t L + rho BLK + l: byte offset in the row beyond laneR
    auto imm_r = [](int i) { return ((i >> 3) * L + (i & 7) * G::BLK) * 8; };

    // prefetch registers: spectrum rows (12 float4 each: float4 c = 4 t + q holds registers (8 t + 2 q, + 1)) for the
    // inverse-first modes, real rows (24 float2 each) for FWD
    float4 sa[12], sb[12];
    float2 ra_[24], rb_[24];
    cf nya = make_float2(0.f, 0.f), nyb = nya;
    auto load_pair = [&](int pb) {
        const Rows r = rows_of<MD::WRAP>(p, pb, Yh);
        if (MD::HAS_INV) {
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                sa[c] = *at<float4>(p.S, r.sa_, XP * 8, laneS, c * LG * 16);
                sb[c] = *at<float4>(p.S, r.sb_, XP * 8, laneS, c * LG * 16);
            }
            nya = *reinterpret_cast<const cf*>(reinterpret_cast<const unsigned char*>(p.S) + r.sa_ * XP * 8 + (grp * XP * 8 + M * 8));
            nyb = *reinterpret_cast<const cf*>(reinterpret_cast<const unsigned char*>(p.S) + r.sb_ * XP * 8 + (grp * XP * 8 + M * 8));
        } else {
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                ra_[i] = *at<float2>(p.in, r.ra, X * 4, laneR, imm_r(i));
                rb_[i] = *at<float2>(p.in, r.rb, X * 4, laneR, imm_r(i));
            }
        }
    };

    int pb = (blockIdx.x * NW + wave) * G::PAIRS;
    if (pb < npairs) load_pair(pb);
    for (; pb < npairs; pb += pstep) {
        LaneAddr a = a0;
        a.da_c4 = opaque_i(a.da_c4);
        a.db_c4 = opaque_i(a.db_c4);
        a.dc_c4[0] = opaque_i(a.dc_c4[0]);
        a.dc_c4[1] = opaque_i(a.dc_c4[1]);
        a.dc_c4[2] = opaque_i(a.dc_c4[2]);
        const Rows rw = rows_of<MD::WRAP>(p, pb, Yh);
        const cf wy = p.twy[rw.yy + grp];
        const int pnext = pb + pstep < npairs ? pb + pstep : pb;  // unconditional prefetch: the last round re-reads its own pair
        cf xa[24], xb[24];
        // twiddles shared by the stages of both rows (LDS tables)
        cf wA[7], wB[7];
#pragma unroll
        for (int k = 1; k < 8; ++k) wA[k - 1] = tw1[(k - 1) * G::BLK + l];
#pragma unroll
        for (int k = 1; k < 8; ++k) wB[k - 1] = k < G::R2 ? tw2[(k - 1) * 8 + (l & 7)] : make_float2(0.f, 0.f);

        // forward half 1 of one row: real-side registers -> radix-3 -> stage A -> LDS (its own three buffers)
        auto fwd_row_head = [&](cf (&x)[24], unsigned char* buf) {
            radix3<LOGL, false>(x, tw3, l);
            stage_a<0, false>(x, wA);
            put_da<LOGL>(buf, x, a, 0);
            stage_a<1, false>(x, wA);
            put_da<LOGL>(buf, x, a, 1);
            stage_a<2, false>(x, wA);
            put_da<LOGL>(buf, x, a, 2);
            xw_fence();
        };

        if (MD::HAS_INV) {
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                xa[2 * c] = make_float2(sa[c].x, sa[c].y);
                xa[2 * c + 1] = make_float2(sa[c].z, sa[c].w);
                xb[2 * c] = make_float2(sb[c].x, sb[c].y);
                xb[2 * c + 1] = make_float2(sb[c].z, sb[c].w);
            }
            const cf nya_cur = nya, nyb_cur = nyb;
            if (MODE == INV_STORE) load_pair(pnext);  // no epilogue operand: the next pair rides behind the whole inverse
            // ---- inverse head: undo the Y step, untangle, stages C and B of every third ----
            // X_a = A + conj(w) B, X_b = A - conj(w) B
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const cf u = cmulc(xb[i], wy), s = xa[i];
                xa[i] = cadd(s, u);
                xb[i] = csub(s, u);
            }
            const cf un = cmulc(nyb_cur, wy);
            float na = nya_cur.x + un.x, nb = nya_cur.x - un.x;
            {
                cf w0[8], w1[8];
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    w0[n] = ut0[n * LG + l];
                    w1[n] = ut1[n * LG + l];
                }
                untangle<true>(xa, w0, w1, l, na);
                untangle<true>(xb, w0, w1, l, nb);
            }
            stage_c<0, true>(xa);
            stage_c<1, true>(xa);
            stage_c<2, true>(xa);
            put_dc<LOGL>(ba, xa, a, 0);
            put_dc<LOGL>(ba, xa, a, 1);
            put_dc<LOGL>(ba, xa, a, 2);
            stage_c<0, true>(xb);
            stage_c<1, true>(xb);
            stage_c<2, true>(xb);
            put_dc<LOGL>(bb, xb, a, 0);
            put_dc<LOGL>(bb, xb, a, 1);
            put_dc<LOGL>(bb, xb, a, 2);
            xw_fence();
            get_db<LOGL>(ba, xa, a, 0);
            get_db<LOGL>(ba, xa, a, 1);
            get_db<LOGL>(ba, xa, a, 2);
            get_db<LOGL>(bb, xb, a, 0);
            get_db<LOGL>(bb, xb, a, 1);
            get_db<LOGL>(bb, xb, a, 2);
            xw_fence();
            stage_b<LOGL, 0, true>(xa, wB);
            stage_b<LOGL, 1, true>(xa, wB);
            stage_b<LOGL, 2, true>(xa, wB);
            put_db<LOGL>(ba, xa, a, 0);
            put_db<LOGL>(ba, xa, a, 1);
            put_db<LOGL>(ba, xa, a, 2);
            stage_b<LOGL, 0, true>(xb, wB);
            stage_b<LOGL, 1, true>(xb, wB);
            stage_b<LOGL, 2, true>(xb, wB);
            put_db<LOGL>(bb, xb, a, 0);
            put_db<LOGL>(bb, xb, a, 1);
            put_db<LOGL>(bb, xb, a, 2);
            xw_fence();
            // this pair's d / est rows ride behind the last inverse stage
            float2 auxa[24], auxb[24];
            if (MD::RATIO || MD::UPDATE) {
#pragma unroll
                for (int i = 0; i < 24; ++i) auxa[i] = *at<float2>(p.aux, rw.sa_, X * 4, laneR, imm_r(i));
#pragma unroll
                for (int i = 0; i < 24; ++i) auxb[i] = *at<float2>(p.aux, rw.sb_, X * 4, laneR, imm_r(i));
            }
            // ---- last inverse stage, inverse radix-3 and epilogue, one row at a time; a fused pass sends the row straight on
            // into the first half of its forward transform (the row's LDS buffers are free again once it is in registers) ----
            const bool zero_plane = rw.zero;
            auto tail_row = [&](cf (&x)[24], const float2 (&aux)[24], unsigned char* buf, long row) {
                // CROP: this row's plane and row inside the unpadded output volume (64-bit division once per row, not per store)
                const int zq = MD::CROP ? (int)(row / p.Y) - p.wz.off : 0;
                const long yq = MD::CROP ? row % p.Y + grp : 0;
                get_da<LOGL>(buf, x, a, 0);
                get_da<LOGL>(buf, x, a, 1);
                get_da<LOGL>(buf, x, a, 2);
                xw_fence();
                stage_a<0, true>(x, wA);
                stage_a<1, true>(x, wA);
                stage_a<2, true>(x, wA);
                radix3<LOGL, true>(x, tw3, l);
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    float2 v = x[i];
                    if (MD::RATIO || MD::UPDATE) v = value_op<MODE>(v, aux[i], p.eps);
                    if (MD::CROP) {
                        const int xq = 2 * ((i >> 3) * L + (i & 7) * G::BLK + l) - p.wx.off;
                        if (zq >= 0 && zq < p.wz.n) {
                            float* dst = p.out + ((long)zq * p.Y + yq) * p.wx.n + xq;
                            typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
                            if (xq >= 0 && xq + 1 < p.wx.n) {
                                *reinterpret_cast<f2u*>(dst) = f2u{v.x, v.y};
                            } else {
                                if (xq >= 0 && xq < p.wx.n) dst[0] = v.x;
                                if (xq + 1 >= 0 && xq + 1 < p.wx.n) dst[1] = v.y;
                            }
                        }
                    } else if (MD::STORE_REAL && !MD::WRAP) *at_w<float2>(p.out, row, X * 4, laneR, imm_r(i)) = v;
                    x[i] = v;
                }
                if (MD::WRAP) {
                    // Wrap-extension along x inside the row.  The epilogue's values are right on the volume's own voxels
                    // (box positions [off, off + n)); margin position rel = pos - off in [-mlo, 0) takes the value of voxel
                    // rel + n, rel in [n, n + mhi) that of voxel rel - n, everything else is zero.  The two source strips
                    // (at most K - 1 floats together) travel through the start of the row's LDS buffers, which are free
                    // between the last read of the inverse and the first write of the forward transform.  Blocks of 2 BLK
                    // floats that lie inside the volume are skipped by scalar tests.
                    const int n = p.wx.n, off = p.wx.off, mlo = p.wx.mlo, mhi = p.wx.mhi;
                    float* scr = reinterpret_cast<float*>(buf);
#pragma unroll
                    for (int i = 0; i < 24; ++i) {
                        const int n0 = 2 * ((i >> 3) * L + (i & 7) * G::BLK) - off, n1 = n0 + 2 * G::BLK;  // voxels of this register's block
                        if ((n1 > n - mlo && n0 < n) || (n0 < mhi && n1 > 0)) {
                            const int nn = n0 + 2 * l;
                            if (nn >= n - mlo && nn < n) scr[nn - (n - mlo)] = x[i].x;
                            if (nn + 1 >= n - mlo && nn + 1 < n) scr[nn + 1 - (n - mlo)] = x[i].y;
                            if (nn >= 0 && nn < mhi) scr[mlo + nn] = x[i].x;
                            if (nn + 1 >= 0 && nn + 1 < mhi) scr[mlo + nn + 1] = x[i].y;
                        }
                    }
                    xw_fence();
#pragma unroll
                    for (int i = 0; i < 24; ++i) {
                        const int n0 = 2 * ((i >> 3) * L + (i & 7) * G::BLK) - off, n1 = n0 + 2 * G::BLK;
                        if (n0 < 0 || n1 > n) {  // the block reaches outside the volume
                            float v2[2] = {x[i].x, x[i].y};
#pragma unroll
                            for (int b = 0; b < 2; ++b) {
                                int rel = n0 + 2 * l + b;
                                if (rel >= n + mhi) rel -= X;
                                const bool inside = rel >= 0 && rel < n, low = rel >= -mlo && rel < 0, high = rel >= n && rel < n + mhi;
                                const float m = scr[low ? rel + mlo : (high ? mlo + rel - n : 0)];
                                v2[b] = inside ? v2[b] : ((low || high) ? m : 0.0f);
                            }
                            x[i] = make_float2(v2[0], v2[1]);
                        }
                    }
                    if (zero_plane) {
#pragma unroll
                        for (int i = 0; i < 24; ++i) x[i] = make_float2(0.f, 0.f);
                    }
                    xw_fence();  // the scratch strips are read before the forward transform overwrites them
                    if (MD::STORE_REAL) {
#pragma unroll
                        for (int i = 0; i < 24; ++i) *at_w<float2>(p.out, row, X * 4, laneR, imm_r(i)) = x[i];
                    }
                }
                if (MD::HAS_FWD) fwd_row_head(x, buf);
            };
            tail_row(xa, auxa, ba, rw.ra);
            tail_row(xb, auxb, bb, rw.rb);
            if (MODE == INV_RATIO || MODE == INV_UPDATE || MD::CROP) load_pair(pnext);
        } else {
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                xa[i] = ra_[i];
                xb[i] = rb_[i];
            }
            if (p.norm_mean) {  // phase reconstruction: x / mean - 1 on the way in
                const float inv = (float)(1.0 / *p.norm_mean);
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    xa[i] = make_float2(xa[i].x * inv - 1.0f, xa[i].y * inv - 1.0f);
                    xb[i] = make_float2(xb[i].x * inv - 1.0f, xb[i].y * inv - 1.0f);
                }
            } else if (p.out) {  // Richardson-Lucy start: e0 = max(d, 0) is stored and transformed in one pass
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    xa[i] = make_float2(fmaxf(xa[i].x, 0.f), fmaxf(xa[i].y, 0.f));
                    xb[i] = make_float2(fmaxf(xb[i].x, 0.f), fmaxf(xb[i].y, 0.f));
                    *at_w<float2>(p.out, rw.ra, X * 4, laneR, imm_r(i)) = xa[i];
                    *at_w<float2>(p.out, rw.rb, X * 4, laneR, imm_r(i)) = xb[i];
                }
            }
            xw_fence();
            load_pair(pnext);  // the next pair's rows ride behind the forward transform
            xw_fence();
            fwd_row_head(xa, ba);
            fwd_row_head(xb, bb);
        }
        if (MD::HAS_FWD) {
            if (MD::HAS_INV) {
                xw_fence();
                load_pair(pnext);  // the next pair's spectrum rows ride behind the rest of the forward transform
                xw_fence();
            }
            // ---- forward half 2: stages B and C of every third, untangle, Y step, store ----
            get_db<LOGL>(ba, xa, a, 0);
            get_db<LOGL>(ba, xa, a, 1);
            get_db<LOGL>(ba, xa, a, 2);
            get_db<LOGL>(bb, xb, a, 0);
            get_db<LOGL>(bb, xb, a, 1);
            get_db<LOGL>(bb, xb, a, 2);
            xw_fence();
            stage_b<LOGL, 0, false>(xa, wB);
            stage_b<LOGL, 1, false>(xa, wB);
            stage_b<LOGL, 2, false>(xa, wB);
            put_db<LOGL>(ba, xa, a, 0);
            put_db<LOGL>(ba, xa, a, 1);
            put_db<LOGL>(ba, xa, a, 2);
            stage_b<LOGL, 0, false>(xb, wB);
            stage_b<LOGL, 1, false>(xb, wB);
            stage_b<LOGL, 2, false>(xb, wB);
            put_db<LOGL>(bb, xb, a, 0);
            put_db<LOGL>(bb, xb, a, 1);
            put_db<LOGL>(bb, xb, a, 2);
            xw_fence();
            get_dc<LOGL>(ba, xa, a, 0);
            get_dc<LOGL>(ba, xa, a, 1);
            get_dc<LOGL>(ba, xa, a, 2);
            get_dc<LOGL>(bb, xb, a, 0);
            get_dc<LOGL>(bb, xb, a, 1);
            get_dc<LOGL>(bb, xb, a, 2);
            xw_fence();
            stage_c<0, false>(xa);
            stage_c<1, false>(xa);
            stage_c<2, false>(xa);
            stage_c<0, false>(xb);
            stage_c<1, false>(xb);
            stage_c<2, false>(xb);
            float na = 0.f, nb = 0.f;
            {
                cf w0[8], w1[8];
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    w0[n] = ut0[n * LG + l];
                    w1[n] = ut1[n * LG + l];
                }
                untangle<false>(xa, w0, w1, l, na);
                untangle<false>(xb, w0, w1, l, nb);
            }
            // A = X_a + X_b, B = (X_a - X_b) w_Y^y
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const cf s = cadd(xa[i], xb[i]), d = cmul(csub(xa[i], xb[i]), wy);
                xa[i] = s;
                xb[i] = d;
            }
            const cf nyA = make_float2(na + nb, 0.f), nyB = cmul(make_float2(na - nb, 0.f), wy);
#pragma unroll
            for (int c = 0; c < 12; ++c) {
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
}

// host: [tw1 [7][BLK] | tw2 [R2 - 1][8] | tw3 [2][L] | ut0 [8][LG] | ut1 [8][LG]] and the stored column of every position
// q = t L + p (third t, bit-reversed position p: frequency 3 brev(p) + t)
template <int LOGL>
static void make_tables(std::vector<cf>& tab, std::vector<int>& col_of_pos) {
    using G = Geo<LOGL>;
    constexpr int M = G::M, L = G::L;
    tab.assign(G::NTAB, make_float2(0.f, 0.f));
    auto w = [](double num, double den) {
        const double a = -2.0 * M_PI * num / den;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int k = 1; k < 8; ++k)
        for (int t = 0; t < G::BLK; ++t) tab[(size_t)(k - 1) * G::BLK + t] = w((double)t * k, L);
    for (int k1 = 1; k1 < G::R2; ++k1)
        for (int n0 = 0; n0 < 8; ++n0) tab[G::NTW1 + (size_t)(k1 - 1) * 8 + n0] = w((double)n0 * k1, G::BLK);
    for (int k = 1; k < 3; ++k)
        for (int m = 0; m < L; ++m) tab[G::NTW1 + G::NTW2 + (size_t)(k - 1) * L + m] = w((double)k * m, M);
    auto utw = [&](int t, int pos) { return w(3.0 * brev_c(pos, LOGL) + t, 2.0 * M); };  // w_X^f, f = the frequency at (t, pos)
    const size_t u0 = G::NTW1 + G::NTW2 + G::NTW3;
    for (int n = 0; n < 8; ++n)
        for (int lam = 0; lam < G::LG; ++lam) {
            tab[u0 + (size_t)n * G::LG + lam] = utw(0, 8 * group_of<LOGL>(0, lam) + n);
            tab[u0 + G::NUT + (size_t)n * G::LG + lam] = utw(1, 8 * group_of<LOGL>(1, lam) + n);
        }
    col_of_pos.assign(M, 0);
    for (int t = 0; t < 3; ++t)
        for (int lam = 0; lam < G::LG; ++lam)
            for (int n = 0; n < 8; ++n)
                col_of_pos[(size_t)t * L + 8 * group_of<LOGL>(t, lam) + n] = 2 * ((4 * t + (n >> 1)) * G::LG + lam) + (n & 1);
}

}  // namespace x3
