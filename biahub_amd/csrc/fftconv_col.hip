// The LDS-stepped column pass of the fused FFT engine (fftconv.hip): col_pass_kernel, any supported column length, every
// spectral product.  The register-stage kernels of fftconv_colreg.hip take the lengths they are built for.
#include "fftconv_dev.hpp"

namespace bh {

// The prefetch registers are sixteen named float4, of which ROUNDS are used (not an array: hipcc keeps a loop-carried
// float4[] in scratch memory here even with every index constant).  BH_FOR8 applies a macro to all of them.
#define BH_FOR8(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)

// RDX: 1 for power-of-two columns, 3 / 5 for columns of 3 * 2^k / 5 * 2^k rows (their own instantiations: the odd step's
// registers would otherwise push the power-of-two kernels into scratch)
template <int MODE, int ROUNDS, int RDX = 1>
__global__ __launch_bounds__(FC_NT) void col_pass_kernel(ColParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* buf = reinterpret_cast<cf*>(smem);                         // [N][W]
    cf* tw = reinterpret_cast<cf*>(smem + (size_t)p.N * p.W * 8);  // twiddles
    const int tid = threadIdx.x;
    for (int i = tid; i < p.ntw; i += FC_NT) tw[i] = p.tw[i];
    const int L_ = RDX == 1 ? p.N : p.L;
    constexpr bool r3 = RDX != 1;
    cf* tw3 = tw + p.ntw;
    if (r3)
        for (int i = tid; i < (RDX - 1) * L_; i += FC_NT) tw3[i] = p.tw3[i];
    // column transform = [radix-3 step] + power-of-two transform of the 1 or 3 length-L sequences
#define BH_FFT_FWD(...)                                                     \
    {                                                                       \
        if (r3) {                                                           \
            odd_step<false, 2, FC_NT, RDX>(buf, L_, logW, W_, tw3, tid);                \
            __syncthreads();                                                \
        }                                                                   \
        fft_lds<false, __VA_ARGS__>(buf, L_, logN, logW, W_, tw, tid, N_);  \
    }
#define BH_FFT_INV(...)                                                     \
    {                                                                       \
        fft_lds<true, __VA_ARGS__>(buf, L_, logN, logW, W_, tw, tid, N_);   \
        if (r3) {                                                           \
            odd_step<true, 2, FC_NT, RDX>(buf, L_, logW, W_, tw3, tid);                 \
            __syncthreads();                                                \
        }                                                                   \
    }

    const int LPS = p.W >> 1;           // lanes per row segment (float4 = 2 complex)
    const int RPR = FC_NT / LPS;        // rows per round
    const int lane = tid % LPS;
    const int r0 = tid / LPS;
    const long ntiles = (long)p.nouter * p.ncoltiles;
    constexpr bool HAS_OTF = (MODE == COL_CONV || MODE == COL_CORR || MODE == COL_FILTER || MODE == COL_CONV16 || MODE == COL_PCC);
    const int ncoltiles = p.ncoltiles, nsub = p.nsub, W_ = p.W, N_ = p.N, logN = p.logN, logW = p.logW, XP = p.XP;
    const long outer_stride = p.outer_stride, sub_stride = p.sub_stride, row_stride = p.row_stride;
    cf* const S = p.S;
    const cf* const otf = p.otf;
    const float scale = p.scale;
    const int pcc_norm = p.pcc_norm, pcc_swap = p.pcc_swap;
    cf* const otf_out = p.otf_out;
    auto tile_base = [=](long tt) -> long {
        const long ou = tt / ncoltiles;
        const int ct = (int)(tt - ou * ncoltiles);
        return (ou / nsub) * outer_stride + (ou % nsub) * sub_stride + (long)ct * W_ + 2 * lane;
    };

    float4 v0, v1, v2, v3, v4, v5, v6, v7, v8, v9, v10, v11, v12, v13, v14, v15;
    v0 = v1 = v2 = v3 = v4 = v5 = v6 = v7 = make_float4(0.f, 0.f, 0.f, 0.f);
    v8 = v9 = v10 = v11 = v12 = v13 = v14 = v15 = v0;
    // unconditional, clamped row loads (see deskew.hip on predicated loads)
#define BH_LD(u) \
    if (u < ROUNDS) v##u = *reinterpret_cast<const float4*>(src_ + (long)min(r0 + u * RPR, N_ - 1) * row_stride);
#define BH_LOAD_TILE(SRC, T)                     \
    {                                            \
        const cf* src_ = (SRC) + tile_base(T);   \
        BH_FOR8(BH_LD)                           \
    }
    // real filter (Tikhonov): one float per complex element, same [z][y][p] indexing
#define BH_LDF(u)                                                                                          \
    if (u < ROUNDS) {                                                                                      \
        const float2 f_ = *reinterpret_cast<const float2*>(fsrc_ + (long)min(r0 + u * RPR, N_ - 1) * row_stride); \
        v##u = make_float4(f_.x, f_.x, f_.y, f_.y);                                                        \
    }
#define BH_LOAD_FILTER(T)                                                      \
    {                                                                          \
        const float* fsrc_ = reinterpret_cast<const float*>(otf) + tile_base(T); \
        BH_FOR8(BH_LDF)                                                        \
    }
    // complex multiplier stored as bfloat16 pairs (COL_CONV16): one 32-bit word per complex element
#define BH_LDH(u)                                                                                          \
    if (u < ROUNDS) {                                                                                      \
        const uint2 h_ = *reinterpret_cast<const uint2*>(hsrc_ + (long)min(r0 + u * RPR, N_ - 1) * row_stride); \
        v##u = make_float4(__uint_as_float(h_.x << 16), __uint_as_float(h_.x & 0xffff0000u),               \
                           __uint_as_float(h_.y << 16), __uint_as_float(h_.y & 0xffff0000u));              \
    }
#define BH_LOAD_FILTER16(T)                                                            \
    {                                                                                  \
        const unsigned int* hsrc_ = reinterpret_cast<const unsigned int*>(otf) + tile_base(T); \
        BH_FOR8(BH_LDH)                                                                \
    }
#define BH_TO_LDS(u)                                                                            \
    if (u < ROUNDS && r0 + u * RPR < N_)                                                        \
        *reinterpret_cast<float4*>(buf + (size_t)(r0 + u * RPR) * W_ + 2 * lane) = v##u;
#define BH_OTF_MUL(u)                                                                           \
    if (u < ROUNDS && r0 + u * RPR < N_) {                                                      \
        float4* q_ = reinterpret_cast<float4*>(buf + (size_t)(r0 + u * RPR) * W_ + 2 * lane);   \
        const float4 a = *q_;                                                                   \
        const float4 b = v##u;                                                                  \
        float4 c;                                                                               \
        if (MODE == COL_FILTER) {                                                               \
            c.x = a.x * b.x;                                                                    \
            c.y = a.y * b.y;                                                                    \
            c.z = a.z * b.z;                                                                    \
            c.w = a.w * b.w;                                                                    \
        } else if (MODE == COL_PCC) { /* first * conj(second) / norm * scale, as pcc_product_kernel; b = the stored spectrum */ \
            const float2 f0 = make_float2(pcc_swap ? a.x : b.x, pcc_swap ? a.y : b.y), s0 = make_float2(pcc_swap ? b.x : a.x, pcc_swap ? b.y : a.y); \
            const float2 f1 = make_float2(pcc_swap ? a.z : b.z, pcc_swap ? a.w : b.w), s1 = make_float2(pcc_swap ? b.z : a.z, pcc_swap ? b.w : a.w); \
            const float2 p0 = pcc_bin(f0, s0, pcc_norm, scale);                                 \
            const float2 p1 = pcc_bin(f1, s1, pcc_norm, scale);                                 \
            c = make_float4(p0.x, p0.y, p1.x, p1.y);                                            \
            if (otf_out && col_ok) *reinterpret_cast<float4*>(otf_out + base + (long)(r0 + u * RPR) * row_stride) = a; \
        } else if (MODE == COL_CONV || MODE == COL_CONV16) {                                    \
            c.x = a.x * b.x - a.y * b.y;                                                        \
            c.y = a.x * b.y + a.y * b.x;                                                        \
            c.z = a.z * b.z - a.w * b.w;                                                        \
            c.w = a.z * b.w + a.w * b.z;                                                        \
        } else {                                                                                \
            c.x = a.x * b.x + a.y * b.y;                                                        \
            c.y = a.y * b.x - a.x * b.y;                                                        \
            c.z = a.z * b.z + a.w * b.w;                                                        \
            c.w = a.w * b.z - a.z * b.w;                                                        \
        }                                                                                       \
        *q_ = c;                                                                                \
    }
#define BH_STORE(u)                                                                                        \
    if (u < ROUNDS && r0 + u * RPR < N_ && col_ok) {                                                       \
        float4 a = *reinterpret_cast<const float4*>(buf + (size_t)(r0 + u * RPR) * W_ + 2 * lane);         \
        if (MODE == COL_FWD_SCALE) {                                                                       \
            a.x *= scale;                                                                                  \
            a.y *= scale;                                                                                  \
            a.z *= scale;                                                                                  \
            a.w *= scale;                                                                                  \
        }                                                                                                  \
        *reinterpret_cast<float4*>(S + base + (long)(r0 + u * RPR) * row_stride) = a;                      \
    }

    long t = blockIdx.x;
    if (t < ntiles) BH_LOAD_TILE(S, t)
    for (; t < ntiles; t += gridDim.x) {
        BH_FOR8(BH_TO_LDS)  // registers -> LDS
        const long base = tile_base(t);
        const int ct = (int)(t % ncoltiles);
        const bool col_ok = (ct * W_ + 2 * lane) < XP;  // pad columns of a ragged last tile are never stored
        __syncthreads();
        const long tn = t + gridDim.x;
        if (HAS_OTF && MODE != COL_PCC && p.midfuse) {
            // This tile's OTF arrives behind the forward FFT, fetched in the order the fused middle step wants it:
            // butterfly b = tid / LPS + s * RPR (s = 0, 1) covers rows 4b .. 4b + 3 of this lane's two columns.
            // The h = 2 radix-4 steps at the end of the forward and the start of the inverse transform have unit
            // twiddles and touch the same four rows, so forward step, spectral multiply and inverse step happen in
            // registers: one LDS round trip and one barrier instead of three.
            const int nbf = N_ >> 2;  // butterflies per column
            {
                const long tb_ = tile_base(t);
#define BH_LDM(u)                                                                                                  \
    {                                                                                                              \
        const int row_ = min(4 * (r0 + (u >> 2) * RPR) + (u & 3), N_ - 1);                                         \
        if (MODE == COL_FILTER) {                                                                                  \
            const float2 f_ = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(otf) + tb_ + (long)row_ * row_stride); \
            v##u = make_float4(f_.x, f_.x, f_.y, f_.y);                                                            \
        } else if (MODE == COL_CONV16) {                                                                           \
            const uint2 h_ = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned int*>(otf) + tb_ + (long)row_ * row_stride); \
            v##u = make_float4(__uint_as_float(h_.x << 16), __uint_as_float(h_.x & 0xffff0000u),                   \
                               __uint_as_float(h_.y << 16), __uint_as_float(h_.y & 0xffff0000u));                  \
        } else {                                                                                                   \
            v##u = *reinterpret_cast<const float4*>(otf + tb_ + (long)row_ * row_stride);                          \
        }                                                                                                          \
    }
                BH_LDM(0) BH_LDM(1) BH_LDM(2) BH_LDM(3) BH_LDM(4) BH_LDM(5) BH_LDM(6) BH_LDM(7)
#undef BH_LDM
            }
            BH_FFT_FWD(1, 2, true)
#define BH_SPEC_MUL(a, b)                                                                                          \
    (MODE == COL_FILTER ? make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w)                                  \
     : (MODE == COL_CONV || MODE == COL_CONV16) ? make_float4(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x, a.z * b.z - a.w * b.w, \
                                      a.z * b.w + a.w * b.z)                                                       \
                        : make_float4(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y, a.z * b.z + a.w * b.w,         \
                                      a.w * b.z - a.z * b.w))
#define BH_MID(S_, O0, O1, O2, O3)                                                                                 \
    if (r0 + S_ * RPR < nbf) {                                                                                     \
        float4* q_ = reinterpret_cast<float4*>(buf + (size_t)(4 * (r0 + S_ * RPR)) * W_ + 2 * lane);              \
        const int st_ = W_ >> 1; /* float4 units per row */                                                        \
        const float4 x0 = q_[0], x1 = q_[st_], x2 = q_[2 * st_], x3 = q_[3 * st_];                                 \
        /* forward h = 2 step, unit twiddles: rows 4b .. 4b + 3 <- s02+s13, s02-s13, d02+d13, d02-d13 */         \
        const float4 s02 = make_float4(x0.x + x2.x, x0.y + x2.y, x0.z + x2.z, x0.w + x2.w);                       \
        const float4 d02 = make_float4(x0.x - x2.x, x0.y - x2.y, x0.z - x2.z, x0.w - x2.w);                       \
        const float4 s13 = make_float4(x1.x + x3.x, x1.y + x3.y, x1.z + x3.z, x1.w + x3.w);                       \
        const float4 e13 = make_float4(x1.x - x3.x, x1.y - x3.y, x1.z - x3.z, x1.w - x3.w);                       \
        const float4 d13 = make_float4(e13.y, -e13.x, e13.w, -e13.z); /* * (-i) */                                 \
        const float4 f0 = make_float4(s02.x + s13.x, s02.y + s13.y, s02.z + s13.z, s02.w + s13.w);                 \
        const float4 f1 = make_float4(s02.x - s13.x, s02.y - s13.y, s02.z - s13.z, s02.w - s13.w);                 \
        const float4 f2 = make_float4(d02.x + d13.x, d02.y + d13.y, d02.z + d13.z, d02.w + d13.w);                 \
        const float4 f3 = make_float4(d02.x - d13.x, d02.y - d13.y, d02.z - d13.z, d02.w - d13.w);                 \
        const float4 y0 = BH_SPEC_MUL(f0, O0), y1 = BH_SPEC_MUL(f1, O1), y2 = BH_SPEC_MUL(f2, O2),                 \
                     y3 = BH_SPEC_MUL(f3, O3);                                                                     \
        /* inverse h = 2 step, unit twiddles: rows <- A+C, B+D, A-C, B-D */                                        \
        const float4 A = make_float4(y0.x + y1.x, y0.y + y1.y, y0.z + y1.z, y0.w + y1.w);                          \
        const float4 B = make_float4(y0.x - y1.x, y0.y - y1.y, y0.z - y1.z, y0.w - y1.w);                          \
        const float4 Cc = make_float4(y2.x + y3.x, y2.y + y3.y, y2.z + y3.z, y2.w + y3.w);                         \
        const float4 e23 = make_float4(y2.x - y3.x, y2.y - y3.y, y2.z - y3.z, y2.w - y3.w);                       \
        const float4 D = make_float4(-e23.y, e23.x, -e23.w, e23.z); /* * (+i) */                                   \
        q_[0] = make_float4(A.x + Cc.x, A.y + Cc.y, A.z + Cc.z, A.w + Cc.w);                                       \
        q_[st_] = make_float4(B.x + D.x, B.y + D.y, B.z + D.z, B.w + D.w);                                         \
        q_[2 * st_] = make_float4(A.x - Cc.x, A.y - Cc.y, A.z - Cc.z, A.w - Cc.w);                                 \
        q_[3 * st_] = make_float4(B.x - D.x, B.y - D.y, B.z - D.z, B.w - D.w);                                     \
    }
            BH_MID(0, v0, v1, v2, v3)
            BH_MID(1, v4, v5, v6, v7)
#undef BH_MID
#undef BH_SPEC_MUL
            __syncthreads();
            if (tn < ntiles) BH_LOAD_TILE(S, tn)
            BH_FFT_INV(1, 2, true)
        } else if (HAS_OTF) {
            // this tile's OTF arrives behind the forward FFT; the next tile's data behind the inverse FFT
            if (MODE == COL_FILTER) BH_LOAD_FILTER(t) else if (MODE == COL_CONV16) BH_LOAD_FILTER16(t) else BH_LOAD_TILE(otf, t)
            BH_FFT_FWD(1, 2)
            BH_FOR8(BH_OTF_MUL)
            __syncthreads();
            if (tn < ntiles) BH_LOAD_TILE(S, tn)
            BH_FFT_INV(1, 2)
        } else {
            if (tn < ntiles) BH_LOAD_TILE(S, tn)  // prefetch the next tile behind the FFT
            if (MODE == COL_INV) {
                BH_FFT_INV(1, 2)
            } else {
                BH_FFT_FWD(1, 2)
            }
        }
        BH_FOR8(BH_STORE)  // LDS -> global
        __syncthreads();
    }
#undef BH_FFT_FWD
#undef BH_FFT_INV
#undef BH_LD
#undef BH_LDF
#undef BH_LOAD_FILTER
#undef BH_LDH
#undef BH_LOAD_FILTER16
#undef BH_LOAD_TILE
#undef BH_TO_LDS
#undef BH_OTF_MUL
#undef BH_STORE
}

int launch_col_pass(bh_ctx* ctx, ColParams p, int mode) {
    p.logW = ilog2(p.W);
    p.midfuse = getenv("BH_FC_NOZMID") == nullptr;
    p.ncoltiles = (int)ceil_div(p.XP, p.W);
    BH_REQUIRE((long)p.N * p.W <= FC_TILE && (long)p.N * (p.W / 2) <= 16l * FC_NT && (FC_NT % (p.W / 2)) == 0,
               "internal: column tile %dx%d unsupported", p.N, p.W);
    const size_t lds = (size_t)p.N * p.W * 8 + (size_t)p.ntw * 8 + (p.L != p.N ? (size_t)(p.N / p.L - 1) * p.L * 8 : 0);
    const long ntiles = (long)p.nouter * p.ncoltiles;
    const int grid = (int)std::min<long>(ntiles, ctx->num_cus);
    auto run = [&](auto kern) { return launch_lds(ctx, kern, grid, FC_NT, lds, p); };
    const long per_round = (long)(FC_NT / (p.W / 2));
    const int rounds = (int)ceil_div(p.N, per_round);
#define BH_COL_DISPATCH_(R, RDX)                                           \
    switch (mode) {                                                        \
        case COL_FWD: return run(col_pass_kernel<COL_FWD, R, RDX>);        \
        case COL_INV: return run(col_pass_kernel<COL_INV, R, RDX>);        \
        case COL_FWD_SCALE: return run(col_pass_kernel<COL_FWD_SCALE, R, RDX>); \
        case COL_CONV: return run(col_pass_kernel<COL_CONV, R, RDX>);      \
        case COL_FILTER: return run(col_pass_kernel<COL_FILTER, R, RDX>);  \
        case COL_CONV16: return run(col_pass_kernel<COL_CONV16, R, RDX>);  \
        case COL_PCC: return run(col_pass_kernel<COL_PCC, R, RDX>);        \
        default: return run(col_pass_kernel<COL_CORR, R, RDX>);            \
    }
#define BH_COL_DISPATCH(R)                                 \
    if (p.N / p.L == 3) { BH_COL_DISPATCH_(R, 3) }         \
    else if (p.N / p.L == 5) { BH_COL_DISPATCH_(R, 5) }    \
    else { BH_COL_DISPATCH_(R, 1) }
    if (rounds <= 1) { BH_COL_DISPATCH(1) }
    if (rounds <= 2) { BH_COL_DISPATCH(2) }
    if (rounds <= 4) { BH_COL_DISPATCH(4) }
    if (rounds <= 8) { BH_COL_DISPATCH(8) }
    BH_COL_DISPATCH(16)
#undef BH_COL_DISPATCH
#undef BH_COL_DISPATCH_
}

}  // namespace bh
