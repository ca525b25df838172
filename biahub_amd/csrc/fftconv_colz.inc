// Z pass of 512-point columns with radix-8 register stages: forward transform, spectral product, inverse transform of a
// 512 x 32 column tile in FOUR LDS round trips and four barriers (col_pass_kernel: ten and eleven).  Included by fftconv_colreg.hip
// (namespace bh).
//
// The LDS store path moves ~80 B/clk per CU whatever the store width (MI355X_MICROARCH.md, LDS): a 128-KiB tile costs ~1640
// cycles per full write, and the radix-4 kernel writes it ten times per tile (6.8 us of its 21.8 us; the tile's HBM time is
// 15 us) — the pass is bound by its own LDS traffic and barriers, not by memory.  Here a thread keeps 8 rows x 2 columns in
// registers and runs three decimation-in-frequency levels at a time — the same nine in-place radix-2 levels as fft_lds, so the
// spectrum keeps its bit-reversed order and every transfer function staged for the old pass fits unchanged:
//   A  (spans 256,128,64)  rows g + 64 i        <- the prefetch registers (the rows arrive in exactly this distribution)
//   B  (spans 32,16,8)     rows 64 (g/8) + g%8 + 8 i
//   C  (spans 4,2,1)       rows 8 g + i         + the spectral product + C' of the inverse, all in registers
//   B', A' mirrored with conjugate twiddles; A' hands its rows to the global stores.
// A' reads and the next tile's A writes the same LDS words of the same thread, so no barrier separates two tiles.
namespace colz {

#ifndef BH_COLZ_W
#define BH_COLZ_W 32  // complex columns per tile: 32 = one 1024-thread workgroup and one 128-KiB tile per CU; 16 = two 512-thread
                      // workgroups with 64-KiB tiles (128-B row segments; one workgroup's loads under the other's steps) — measured
                      // on the shuffled layout: 5.01 against 4.32 ms per launch (tools/prof_variant.sh), so 32 stays
#endif
constexpr int N = 512, W = BH_COLZ_W, NT = 32 * W, CP = W / 2;  // rows, complex columns, threads, column pairs (float4) per row
constexpr int LOGCP = W == 32 ? 4 : 3;
static_assert(W == 32 || W == 16, "BH_COLZ_W must be 16 or 32");
constexpr int LDS_BYTES = N * W * 8 + (64 + 8) * 3 * 8;

struct C2 {  // the two columns of a thread
    cf a, b;
};
__device__ __forceinline__ C2 operator+(C2 x, C2 y) { return C2{cadd(x.a, y.a), cadd(x.b, y.b)}; }
__device__ __forceinline__ C2 operator-(C2 x, C2 y) { return C2{csub(x.a, y.a), csub(x.b, y.b)}; }
__device__ __forceinline__ C2 mulw(C2 x, cf w) { return C2{cmul(x.a, w), cmul(x.b, w)}; }
__device__ __forceinline__ C2 mulwc(C2 x, cf w) { return C2{cmulc(x.a, w), cmulc(x.b, w)}; }  // x * conj(w)
__device__ __forceinline__ C2 mi(C2 x) { return C2{mul_mi(x.a), mul_mi(x.b)}; }
__device__ __forceinline__ C2 pi(C2 x) { return C2{mul_pi(x.a), mul_pi(x.b)}; }
constexpr float RH = 0.70710678118654752f;
__device__ __forceinline__ cf w8_1(cf x) { return make_float2((x.x + x.y) * RH, (x.y - x.x) * RH); }   // * (1 - i) / sqrt 2
__device__ __forceinline__ cf w8_3(cf x) { return make_float2((x.y - x.x) * RH, -(x.x + x.y) * RH); }  // * (-1 - i) / sqrt 2
__device__ __forceinline__ cf w8_1c(cf x) { return make_float2((x.x - x.y) * RH, (x.x + x.y) * RH); }  // * (1 + i) / sqrt 2
__device__ __forceinline__ cf w8_3c(cf x) { return make_float2(-(x.x + x.y) * RH, (x.x - x.y) * RH); } // * (-1 + i) / sqrt 2
__device__ __forceinline__ C2 w81(C2 x) { return C2{w8_1(x.a), w8_1(x.b)}; }
__device__ __forceinline__ C2 w83(C2 x) { return C2{w8_3(x.a), w8_3(x.b)}; }
__device__ __forceinline__ C2 w81c(C2 x) { return C2{w8_1c(x.a), w8_1c(x.b)}; }
__device__ __forceinline__ C2 w83c(C2 x) { return C2{w8_3c(x.a), w8_3c(x.b)}; }

// Three forward (decimation-in-frequency) levels on x[i] = element at position p + i s of a block of 8 s rows:
// w1 = w_{8s}^p, w2 = w_{4s}^p, w3 = w_{2s}^p (TW = false: p = 0, s = 1, the unit-twiddle last step).
template <bool TW>
__device__ __forceinline__ void fwd8(C2 (&x)[8], cf w1, cf w2, cf w3) {
    {  // span 4 s: (i, i + 4), twiddle w1 * w_8^i
        const C2 d0 = x[0] - x[4], d1 = x[1] - x[5], d2 = x[2] - x[6], d3 = x[3] - x[7];
        x[0] = x[0] + x[4];
        x[1] = x[1] + x[5];
        x[2] = x[2] + x[6];
        x[3] = x[3] + x[7];
        x[4] = d0;
        x[5] = w81(d1);
        x[6] = mi(d2);
        x[7] = w83(d3);
        if (TW) {
#pragma unroll
            for (int i = 4; i < 8; ++i) x[i] = mulw(x[i], w1);
        }
    }
#pragma unroll
    for (int b = 0; b < 8; b += 4) {  // span 2 s: (i, i + 2) in each half, twiddle w2 * w_4^i
        const C2 d0 = x[b] - x[b + 2], d1 = x[b + 1] - x[b + 3];
        x[b] = x[b] + x[b + 2];
        x[b + 1] = x[b + 1] + x[b + 3];
        x[b + 2] = d0;
        x[b + 3] = mi(d1);
        if (TW) {
            x[b + 2] = mulw(x[b + 2], w2);
            x[b + 3] = mulw(x[b + 3], w2);
        }
    }
#pragma unroll
    for (int b = 0; b < 8; b += 2) {  // span s: (i, i + 1), twiddle w3
        const C2 d = x[b] - x[b + 1];
        x[b] = x[b] + x[b + 1];
        x[b + 1] = TW ? mulw(d, w3) : d;
    }
}
// the mirrored decimation-in-time levels with conjugate twiddles
template <bool TW>
__device__ __forceinline__ void inv8(C2 (&x)[8], cf w1, cf w2, cf w3) {
#pragma unroll
    for (int b = 0; b < 8; b += 2) {
        const C2 y = TW ? mulwc(x[b + 1], w3) : x[b + 1];
        x[b + 1] = x[b] - y;
        x[b] = x[b] + y;
    }
#pragma unroll
    for (int b = 0; b < 8; b += 4) {
        C2 y0 = x[b + 2], y1 = x[b + 3];
        if (TW) {
            y0 = mulwc(y0, w2);
            y1 = mulwc(y1, w2);
        }
        y1 = pi(y1);
        x[b + 2] = x[b] - y0;
        x[b] = x[b] + y0;
        x[b + 3] = x[b + 1] - y1;
        x[b + 1] = x[b + 1] + y1;
    }
    {
        C2 y0 = x[4], y1 = x[5], y2 = x[6], y3 = x[7];
        if (TW) {
            y0 = mulwc(y0, w1);
            y1 = mulwc(y1, w1);
            y2 = mulwc(y2, w1);
            y3 = mulwc(y3, w1);
        }
        y1 = w81c(y1);
        y2 = pi(y2);
        y3 = w83c(y3);
        x[4] = x[0] - y0;
        x[0] = x[0] + y0;
        x[5] = x[1] - y1;
        x[1] = x[1] + y1;
        x[6] = x[2] - y2;
        x[2] = x[2] + y2;
        x[7] = x[3] - y3;
        x[3] = x[3] + y3;
    }
}

// ---- the same butterflies with the rotations by -i / +i and by the eighth roots folded into packed-add operand selects and
// into the twiddle products (BH_COLZ_PKROT, default 1): v_pk_add_f32 can take either half of each source for each half of the
// result and negate it, so a + (-i) b = (a.x + b.y, a.y - b.x) is ONE instruction; the compiler materialises (-i) b with two
// moves first (a third of the first version's non-packed vector instructions were such moves).  Same values up to the
// rounding of R folded into a twiddle (w R instead of (. R) w).
#ifndef BH_COLZ_PKROT
#define BH_COLZ_PKROT 1
#endif
typedef float v2f __attribute__((ext_vector_type(2)));
// (add_mi / add_pi: fftconv_dev.hpp)
__device__ __forceinline__ cf cmul_mi(cf a, cf w) {  // a * (-i w) = (a.x w.y + a.y w.x, a.y w.y - a.x w.x)
    v2f av = {a.x, a.y}, wv = {w.x, w.y}, t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(t) : "v"(av), "v"(wv));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(av), "v"(wv), "v"(t));
    return make_float2(r.x, r.y);
}
__device__ __forceinline__ cf cmulc_pi(cf a, cf w) {  // a * i conj(w) = (a.x w.y - a.y w.x, a.x w.x + a.y w.y)
    v2f av = {a.x, a.y}, wv = {w.x, w.y}, t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,0]" : "=v"(t) : "v"(av), "v"(wv));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(av), "v"(wv), "v"(t));
    return make_float2(r.x, r.y);
}
__device__ __forceinline__ C2 addmi(C2 x, C2 y) { return C2{add_mi(x.a, y.a), add_mi(x.b, y.b)}; }
__device__ __forceinline__ C2 addpi(C2 x, C2 y) { return C2{add_pi(x.a, y.a), add_pi(x.b, y.b)}; }
__device__ __forceinline__ C2 mulwmi(C2 x, cf w) { return C2{cmul_mi(x.a, w), cmul_mi(x.b, w)}; }
__device__ __forceinline__ C2 mulwcpi(C2 x, cf w) { return C2{cmulc_pi(x.a, w), cmulc_pi(x.b, w)}; }
__device__ __forceinline__ C2 scl2(C2 x, float s) { return C2{cscale(x.a, s), cscale(x.b, s)}; }

template <bool TW>
__device__ __forceinline__ void fwd8p(C2 (&x)[8], cf w1, cf w2, cf w3) {
    const C2 d0 = x[0] - x[4], d1 = x[1] - x[5], d2 = x[2] - x[6], d3 = x[3] - x[7];
    x[0] = x[0] + x[4];
    x[1] = x[1] + x[5];
    x[2] = x[2] + x[6];
    x[3] = x[3] + x[7];
    const C2 e1 = addmi(d1, d1), e3 = addmi(d3, d3);  // (1 - i) d: w_8^1 d = R e1, w_8^3 d = -i R e3
    if (TW) {
        const cf w1r = cscale(w1, RH);
        x[4] = mulw(d0, w1);
        x[5] = mulw(e1, w1r);
        x[6] = mulwmi(d2, w1);
        x[7] = mulwmi(e3, w1r);
        // span 2 s with its twiddle
        {
            const C2 a0 = x[0] - x[2], a1 = x[1] - x[3];
            x[0] = x[0] + x[2];
            x[1] = x[1] + x[3];
            x[2] = mulw(a0, w2);
            x[3] = mulwmi(a1, w2);
            const C2 b0 = x[4] - x[6], b1 = x[5] - x[7];
            x[4] = x[4] + x[6];
            x[5] = x[5] + x[7];
            x[6] = mulw(b0, w2);
            x[7] = mulwmi(b1, w2);
        }
#pragma unroll
        for (int b = 0; b < 8; b += 2) {
            const C2 d = x[b] - x[b + 1];
            x[b] = x[b] + x[b + 1];
            x[b + 1] = mulw(d, w3);
        }
    } else {
        // unit twiddles: every rotation rides in the add / subtract that consumes it
        const C2 f1 = scl2(e1, RH), f3 = scl2(e3, RH);  // w_8^1 d1, and i w_8^3 d3
        // lower half (0..3): span 2 then span 1
        const C2 a0 = x[0] - x[2], a1 = x[1] - x[3];      // x[3] would be -i a1
        const C2 s0 = x[0] + x[2], s1 = x[1] + x[3];
        x[0] = s0 + s1;
        x[1] = s0 - s1;
        x[2] = addmi(a0, a1);
        x[3] = addpi(a0, a1);
        // upper half: (4, 6) and (5, 7) where element 6 = -i d2, element 7 = -i f3
        const C2 b0 = addpi(d0, d2), b1 = addpi(f1, f3);  // 4 - 6, 5 - 7
        const C2 t0 = addmi(d0, d2), t1 = addmi(f1, f3);  // 4 + 6, 5 + 7
        x[4] = t0 + t1;
        x[5] = t0 - t1;
        x[6] = addmi(b0, b1);
        x[7] = addpi(b0, b1);
    }
}
template <bool TW>
__device__ __forceinline__ void inv8p(C2 (&x)[8], cf w1, cf w2, cf w3) {
    if (TW) {
#pragma unroll
        for (int b = 0; b < 8; b += 2) {
            const C2 y = mulwc(x[b + 1], w3);
            x[b + 1] = x[b] - y;
            x[b] = x[b] + y;
        }
#pragma unroll
        for (int b = 0; b < 8; b += 4) {
            const C2 y0 = mulwc(x[b + 2], w2), y1 = mulwcpi(x[b + 3], w2);
            x[b + 2] = x[b] - y0;
            x[b] = x[b] + y0;
            x[b + 3] = x[b + 1] - y1;
            x[b + 1] = x[b + 1] + y1;
        }
        const cf w1r = cscale(w1, RH);
        const C2 y0 = mulwc(x[4], w1), t1 = mulwc(x[5], w1r), y2 = mulwcpi(x[6], w1), t3 = mulwc(x[7], w1r);
        const C2 y1 = addpi(t1, t1), e3 = addpi(t3, t3);  // (1 + i) t: conj(w_8^1) y = y1, conj(w_8^3) y = i e3
        x[4] = x[0] - y0;
        x[0] = x[0] + y0;
        x[5] = x[1] - y1;
        x[1] = x[1] + y1;
        x[6] = x[2] - y2;
        x[2] = x[2] + y2;
        x[7] = addmi(x[3], e3);
        x[3] = addpi(x[3], e3);
    } else {
        // span 1
        const C2 p0 = x[0] + x[1], q0 = x[0] - x[1], p1 = x[2] + x[3], q1 = x[2] - x[3];
        const C2 p2 = x[4] + x[5], q2 = x[4] - x[5], p3 = x[6] + x[7], q3 = x[6] - x[7];
        // span 2: (0, 2), (1, 3) with element 3 rotated by +i
        const C2 u0 = p0 + p1, u2 = p0 - p1, u1 = addpi(q0, q1), u3 = addmi(q0, q1);
        const C2 v0 = p2 + p3, v2 = p2 - p3, v1 = addpi(q2, q3), v3 = addmi(q2, q3);
        // span 4: y0 = v0, y1 = conj(w_8^1) v1, y2 = i v2, y3 = conj(w_8^3) v3 = i (1 + i) R v3
        const C2 y1 = scl2(addpi(v1, v1), RH), e3 = scl2(addpi(v3, v3), RH);
        x[0] = u0 + v0;
        x[4] = u0 - v0;
        x[1] = u1 + y1;
        x[5] = u1 - y1;
        x[2] = addpi(u2, v2);
        x[6] = addmi(u2, v2);
        x[3] = addpi(u3, e3);
        x[7] = addmi(u3, e3);
    }
}
#if BH_COLZ_PKROT
#define fwd8 fwd8p
#define inv8 inv8p
#endif

__device__ __forceinline__ C2 unpack(float4 v) { return C2{make_float2(v.x, v.y), make_float2(v.z, v.w)}; }
__device__ __forceinline__ float4 pack(C2 x) { return make_float4(x.a.x, x.a.y, x.b.x, x.b.y); }

// the spectral product of one row of the thread's two columns; o = the multiplier as loaded for MODE
template <int MODE>
__device__ __forceinline__ C2 spec_mul(C2 x, float4 o, int pcc_norm, float scale) {
    if (MODE == COL_FILTER) return C2{make_float2(x.a.x * o.x, x.a.y * o.x), make_float2(x.b.x * o.y, x.b.y * o.y)};
    if (MODE == COL_CORR) return C2{cmulc(x.a, make_float2(o.x, o.y)), cmulc(x.b, make_float2(o.z, o.w))};
    if (MODE == COL_PCC) {  // first * conj(second); pcc_norm's bit 8 = the stored spectrum o is the second factor (ColParams::pcc_swap)
        const bool swap = (pcc_norm & 256) != 0;
        const float2 oa = make_float2(o.x, o.y), ob = make_float2(o.z, o.w);
        return C2{pcc_bin(swap ? x.a : oa, swap ? oa : x.a, pcc_norm & 255, scale), pcc_bin(swap ? x.b : ob, swap ? ob : x.b, pcc_norm & 255, scale)};
    }
    return C2{cmul(x.a, make_float2(o.x, o.y)), cmul(x.b, make_float2(o.z, o.w))};  // COL_CONV, COL_CONV16
}

// Addresses: every global access is (wave-uniform row pointer) + (32-bit byte offset of the lane).  A wavefront holds GPW
// consecutive g (tid >> LOGCP), so row g + 64 u = (GPW wave + 64 u) + gl and row 8 g + i = (8 GPW wave + i) + 8 gl: the
// first parts are scalar (tile base, wave, u / i), the lane parts (gl rows + its column pair) are two loop-invariant VGPRs.
// The first version formed a 64-bit address per lane and access: ~120 vector instructions per tile, a third of them
// quarter-rate 64-bit multiply-adds, and enough live address registers to keep the kernel at its 128-VGPR limit.
// The host checks that 64 rows of the spectrum span less than 4 GiB (launch_col: otherwise col_pass_kernel runs).
// pins a wave-uniform element offset in scalar registers at the point of use (the pointer it is added to is a kernel argument:
// it keeps its address space): without it the compiler folds the lane's offset into eight loop-invariant 64-bit VGPR addresses
// per distribution and adds the tile's base to each of them per tile
__device__ __forceinline__ long scalar_off(long v) {
    unsigned int lo = (unsigned int)(unsigned long long)v, hi = (unsigned int)((unsigned long long)v >> 32);
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (long)(((unsigned long long)hi << 32) | lo);
}

template <int MODE>
__global__ __launch_bounds__(NT, 1024 / NT) void colz_kernel(ColParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);               // [N][CP]
    cf* ta = reinterpret_cast<cf*>(smem + (size_t)N * W * 8);     // [64][3]: w_512^g, w_256^g, w_128^g
    cf* tb = ta + 64 * 3;                                         // [8][3]:  w_64^q,  w_32^q,  w_16^q
    const int tid = threadIdx.x;
    for (int i = tid; i < (64 + 8) * 3; i += NT) ta[i] = p.tw[i];
    constexpr int GPW = 64 / CP;  // g values per wavefront
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cp = tid & (CP - 1), gl = (tid & 63) >> LOGCP, g = GPW * wave + gl;
    const int ncoltiles = p.ncoltiles, XP = p.XP;
    const long outer_stride = p.outer_stride, row_stride = p.row_stride;
    const long ntiles = (long)p.nouter * ncoltiles;
    // bytes per multiplier element: one float (real transfer function), one packed bf16 pair, or a complex float
    constexpr int OB = (MODE == COL_FILTER || MODE == COL_CONV16) ? 4 : 8;
    const unsigned laneA = (unsigned)(((long)gl * row_stride + 2 * cp) * 8);        // spectrum, rows g + 64 u
    const unsigned laneC_ = (unsigned)(((long)(8 * gl) * row_stride + 2 * cp) * OB);  // multiplier, rows 8 g + i
    const unsigned laneC8_ = (unsigned)(((long)(8 * gl) * row_stride + 2 * cp) * 8);  // spectrum, rows 8 g + i (COL_PCC roll)
    // the tile's (outer index, column tile) pair advances by (gridDim.x / ncoltiles, gridDim.x % ncoltiles) with one carry
    const int step_ou = (int)(gridDim.x / (unsigned)ncoltiles), step_ct = (int)(gridDim.x % (unsigned)ncoltiles);
    int cur_ou = (int)(blockIdx.x / (unsigned)ncoltiles), cur_ct = (int)(blockIdx.x % (unsigned)ncoltiles);
    auto base_of = [=](int ou, int ct) -> long { return (long)ou * outer_stride + (long)(ct * W); };  // wave-uniform
    auto rowA_ptr = [=](long base, int u) { return reinterpret_cast<const unsigned char*>(p.S + scalar_off(base + (long)(GPW * wave + 64 * u) * row_stride)); };
    float4 v[8];
    // (the lane offsets pass through xw::opaque_i where they are used: their zero-extension then sits in the block of the access,
    // which is what lets instruction selection fold them into the scalar-base addressing mode)
    auto load_tile = [&](long base) {
        const unsigned la = (unsigned)xw::opaque_i((int)laneA);
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(rowA_ptr(base, u) + la);
    };
    float4 o[8];
    auto load_otf = [&](long base) {
        const unsigned laneC = (unsigned)xw::opaque_i((int)laneC_);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned char* rp = reinterpret_cast<const unsigned char*>(p.otf) + scalar_off((base + (long)(8 * GPW * wave + i) * row_stride) * OB);
            if (MODE == COL_FILTER) {
                const float2 f = *reinterpret_cast<const float2*>(rp + laneC);
                o[i] = make_float4(f.x, f.y, 0.f, 0.f);
            } else if (MODE == COL_CONV16) {
                const uint2 h = *reinterpret_cast<const uint2*>(rp + laneC);
                o[i] = make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xffff0000u), __uint_as_float(h.y << 16),
                                   __uint_as_float(h.y & 0xffff0000u));
            } else {
                o[i] = *reinterpret_cast<const float4*>(rp + laneC);
            }
        }
    };
    long t = blockIdx.x;
    if (t < ntiles) load_tile(base_of(cur_ou, cur_ct));
    __syncthreads();  // twiddle tables
    for (; t < ntiles; t += gridDim.x) {
        // opaque: LDS addresses and twiddles are recomputed / re-read where they are used instead of being hoisted out of the
        // tile loop into long-lived registers (the kernel lives at the 128-VGPR limit of a 1024-thread workgroup)
        const int go = xw::opaque_i(g);
        // LDS rows of the three distributions (float4 index = row * CP + cp)
        const int rowA = go, rowB = (go >> 3) * 64 + (go & 7), rowC = go * 8;
        int nxt_ou = cur_ou + step_ou, nxt_ct = cur_ct + step_ct;
        if (nxt_ct >= ncoltiles) {
            nxt_ct -= ncoltiles;
            ++nxt_ou;
        }
        const long base = base_of(cur_ou, cur_ct), base_n = base_of(nxt_ou, nxt_ct);
        const long tn = t + gridDim.x;
        const int ct = cur_ct;
        cur_ou = nxt_ou;
        cur_ct = nxt_ct;
        C2 x[8];
        const cf a1 = ta[go * 3], a2 = ta[go * 3 + 1], a3 = ta[go * 3 + 2];
        // ---- A: straight from the prefetch registers
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = unpack(v[u]);
        fwd8<true>(x, a1, a2, a3);
#pragma unroll
        for (int u = 0; u < 8; ++u) tile[(rowA + 64 * u) * CP + cp] = pack(x[u]);
        // this tile's multiplier rows (distribution C) ride behind steps A and B
        load_otf(base);
        __syncthreads();
        // ---- B
        const cf b1 = tb[(go & 7) * 3], b2 = tb[(go & 7) * 3 + 1], b3 = tb[(go & 7) * 3 + 2];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowB + 8 * i) * CP + cp]);
        fwd8<true>(x, b1, b2, b3);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[(rowB + 8 * i) * CP + cp] = pack(x[i]);
        __syncthreads();
        // ---- C, the spectral product, C'
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowC + i) * CP + cp]);
        fwd8<false>(x, a1, a1, a1);
        if (MODE == COL_PCC && p.otf_out && ct * W + 2 * cp < XP) {  // roll: this image is the stored one next time
            const unsigned laneC8 = (unsigned)xw::opaque_i((int)laneC8_);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<float4*>(reinterpret_cast<unsigned char*>(p.otf_out + scalar_off(base + (long)(8 * GPW * wave + i) * row_stride)) + laneC8) = pack(x[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = spec_mul<MODE>(x[i], o[i], p.pcc_norm | (p.pcc_swap << 8), p.scale);
        inv8<false>(x, a1, a1, a1);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[(rowC + i) * CP + cp] = pack(x[i]);
        __syncthreads();
        // the next tile's rows travel behind B' and A'
        if (tn < ntiles) load_tile(base_n);
        // ---- B'
        {
            const int gq = xw::opaque_i(go) & 7;
            const cf c1 = tb[gq * 3], c2 = tb[gq * 3 + 1], c3 = tb[gq * 3 + 2];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowB + 8 * i) * CP + cp]);
            inv8<true>(x, c1, c2, c3);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[(rowB + 8 * i) * CP + cp] = pack(x[i]);
        __syncthreads();
        // ---- A' and out (the same LDS words this thread overwrites in the next tile's A: no barrier in between)
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = unpack(tile[(rowA + 64 * u) * CP + cp]);
        {
            const int ga = xw::opaque_i(go);
            inv8<true>(x, ta[ga * 3], ta[ga * 3 + 1], ta[ga * 3 + 2]);
        }
        if (ct * W + 2 * cp < XP) {  // pad columns of a ragged last tile are never stored
            const unsigned la = (unsigned)xw::opaque_i((int)laneA);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                *reinterpret_cast<float4*>(const_cast<unsigned char*>(rowA_ptr(base, u)) + la) = pack(x[u]);
        }
    }
}

// host: [64][3] w_512^g, w_256^g, w_128^g then [8][3] w_64^q, w_32^q, w_16^q (forward sign)
static void make_tables(std::vector<cf>& tab) {
    tab.clear();
    auto w = [](int n, int k) {
        const double a = -2.0 * M_PI * (double)k / (double)n;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int g = 0; g < 64; ++g) {
        tab.push_back(w(512, g));
        tab.push_back(w(256, g));
        tab.push_back(w(128, g));
    }
    for (int q = 0; q < 8; ++q) {
        tab.push_back(w(64, q));
        tab.push_back(w(32, q));
        tab.push_back(w(16, q));
    }
}

}  // namespace colz
