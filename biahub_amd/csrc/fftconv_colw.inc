// Register-stage column passes of the fused FFT engine (columns of 256, 512 or 1024 points) — included by fftconv_colreg.hip.
//
// col_pass_kernel keeps a 128-KiB tile (N rows x W columns) in LDS and runs every radix-4 step of the column transform as
// an LDS round trip behind a workgroup barrier (5 per transform; the Z pass, forward x OTF x inverse, 9 with its fused
// middle step).  Here a 512-thread workgroup owns the same tile, but every thread keeps 16 rows x 2 adjacent columns in
// registers and the length-N transform is three register stages — radix-16 over the top four row-index bits, radix-16 over
// the next four, radix-N/256 over the rest — joined by TWO exchanges through the LDS tile (the in-register butterflies are
// those of the wave-private X passes, xw::reg_fft).  Rows travel between HBM and registers directly, in the distribution of
// the first stage, so the tile in LDS is only ever an exchange buffer.  The Z pass runs forward stage 3, the spectral
// product and inverse stage 3 on the same 16 consecutive rows without touching LDS: 4 exchanges instead of 9 round trips.
// Row positions stay what the in-place decimation-in-frequency transform leaves (bit-reversed), as col_pass_kernel has them:
// OTFs, filters and the other passes do not see which kernel family ran.
// tools/colw_model.py is the executable specification (index maps, the transform against numpy, and the LDS bank conflicts
// of every exchange access: none, with 128 B of padding per 32 rows).
namespace colw {

#ifndef BH_COLW_NT
#define BH_COLW_NT 512
#endif
constexpr int NT = BH_COLW_NT;       // 512: 8 wavefronts, one workgroup and one 128-KiB tile per CU (256: two workgroups with 64-KiB
                                     // tiles, i.e. half as wide row segments — measured slower, tools/ab_variant.sh)
constexpr int TILE_CF = 32 * NT;     // complex points per tile: 16 rows x 2 columns per thread

template <int LOGN>
struct Geo {
    static constexpr int N = 1 << LOGN;
    static constexpr int W = TILE_CF / N;    // complex columns per tile
    static constexpr int CPN = W / 2;        // column pairs (float4) per row
    static constexpr int N16 = N / 16, NQ = N / 256;
    static constexpr int LOWBITS = LOGN - 8; // last stage: radix 4 (N = 1024), 2 (512), none (256)
    static constexpr int RC = 1 << LOWBITS;
    static constexpr int TILE_F4 = N * CPN + (N >> 5) * 8;
    static constexpr int NTA = 15 * N16, NTB = 15 * NQ;
    static constexpr size_t LDS_BYTES = (size_t)TILE_F4 * 16 + (size_t)(NTA + NTB) * 8;
};

template <int LOGN>
__host__ __device__ __forceinline__ constexpr int f4addr(int row, int cp) {
    return row * Geo<LOGN>::CPN + (row >> 5) * 8 + cp;
}

// row held in register r by the thread with row id `rest` in the three distributions
template <int LOGN>
__host__ __device__ __forceinline__ constexpr int row_a(int rest, int r) { return r * Geo<LOGN>::N16 + rest; }
template <int LOGN>
__host__ __device__ __forceinline__ constexpr int row_b(int rest, int r) {
    using G = Geo<LOGN>;
    return (rest / G::NQ) * G::N16 + r * G::NQ + (rest % G::NQ);
}
template <int LOGN>
__host__ __device__ __forceinline__ constexpr int row_c(int rest, int r) { return 16 * rest + r; }

template <int LOGN, int DIST>
__host__ __device__ __forceinline__ constexpr int row_of(int rest, int r) {
    return DIST == 0 ? row_a<LOGN>(rest, r) : (DIST == 1 ? row_b<LOGN>(rest, r) : row_c<LOGN>(rest, r));
}

template <int LOGN, int DIST>
__device__ __forceinline__ void put(float4* tile, const cf (&x0)[16], const cf (&x1)[16], int rest, int cp) {
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[f4addr<LOGN>(row_of<LOGN, DIST>(rest, r), cp)] = make_float4(x0[r].x, x0[r].y, x1[r].x, x1[r].y);
}
template <int LOGN, int DIST>
__device__ __forceinline__ void get(const float4* tile, cf (&x0)[16], cf (&x1)[16], int rest, int cp) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float4 v = tile[f4addr<LOGN>(row_of<LOGN, DIST>(rest, r), cp)];
        x0[r] = make_float2(v.x, v.y);
        x1[r] = make_float2(v.z, v.w);
    }
}

// external twiddles of a radix-16 stage: register rp holds sub-frequency brev4(rp); tw[(k - 1) * stride + id] = w^(id k)
template <bool INV>
__device__ __forceinline__ void twiddle16(cf (&x0)[16], cf (&x1)[16], const cf* tw, int stride, int id) {
#pragma unroll
    for (int rp = 1; rp < 16; ++rp) {
        const cf w = tw[(xw::brev_c(rp, 4) - 1) * stride + id];
        x0[rp] = INV ? cmulc(x0[rp], w) : cmul(x0[rp], w);
        x1[rp] = INV ? cmulc(x1[rp], w) : cmul(x1[rp], w);
    }
}
template <int LOGN, bool INV, int G0 = 0>
__device__ __forceinline__ void stage_c(cf (&x)[16]) {
    using G = Geo<LOGN>;
    if constexpr (G::LOWBITS > 0) {
        xw::reg_fft<G::LOWBITS, G0 * G::RC, 1, INV>(x);
        if constexpr ((G0 + 1) * G::RC < 16) stage_c<LOGN, INV, G0 + 1>(x);
    }
}

// forward: registers in distribution A -> registers in distribution C (B when N = 256); two exchanges
template <int LOGN>
__device__ __forceinline__ void forward(cf (&x0)[16], cf (&x1)[16], float4* tile, const cf* ta, const cf* tb, int rest, int cp) {
    using G = Geo<LOGN>;
    xw::reg_fft<4, 0, 1, false>(x0);
    xw::reg_fft<4, 0, 1, false>(x1);
    twiddle16<false>(x0, x1, ta, G::N16, rest);
    put<LOGN, 0>(tile, x0, x1, rest, cp);
    __syncthreads();
    get<LOGN, 1>(tile, x0, x1, rest, cp);
    xw::reg_fft<4, 0, 1, false>(x0);
    xw::reg_fft<4, 0, 1, false>(x1);
    if constexpr (G::LOWBITS > 0) {
        twiddle16<false>(x0, x1, tb, G::NQ, rest % G::NQ);
        __syncthreads();  // every thread has read exchange 1 before anyone writes exchange 2
        put<LOGN, 1>(tile, x0, x1, rest, cp);
        __syncthreads();
        get<LOGN, 2>(tile, x0, x1, rest, cp);
        stage_c<LOGN, false>(x0);
        stage_c<LOGN, false>(x1);
    }
}
// inverse: the mirror image, distribution C (B) -> A
template <int LOGN>
__device__ __forceinline__ void inverse(cf (&x0)[16], cf (&x1)[16], float4* tile, const cf* ta, const cf* tb, int rest, int cp) {
    using G = Geo<LOGN>;
    if constexpr (G::LOWBITS > 0) {
        stage_c<LOGN, true>(x0);
        stage_c<LOGN, true>(x1);
        put<LOGN, 2>(tile, x0, x1, rest, cp);
        __syncthreads();
        get<LOGN, 1>(tile, x0, x1, rest, cp);
        twiddle16<true>(x0, x1, tb, G::NQ, rest % G::NQ);
    }
    xw::reg_fft<4, 0, 1, true>(x0);
    xw::reg_fft<4, 0, 1, true>(x1);
    if constexpr (G::LOWBITS > 0) __syncthreads();
    put<LOGN, 1>(tile, x0, x1, rest, cp);
    __syncthreads();
    get<LOGN, 0>(tile, x0, x1, rest, cp);
    twiddle16<true>(x0, x1, ta, G::N16, rest);
    xw::reg_fft<4, 0, 1, true>(x0);
    xw::reg_fft<4, 0, 1, true>(x1);
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(NT, 2) void colw_kernel(ColParams p) {
    using G = Geo<LOGN>;
    constexpr bool HAS_OTF = MODE == COL_CONV || MODE == COL_CORR || MODE == COL_FILTER || MODE == COL_CONV16;
    constexpr bool LOAD_A = MODE != COL_INV;               // rows arrive in distribution A, except for the inverse pass
    constexpr int DSPEC = G::LOWBITS > 0 ? 2 : 1;          // distribution at the spectrum end
    constexpr int DLOAD = LOAD_A ? 0 : DSPEC;
    constexpr int DSTORE = (MODE == COL_FWD || MODE == COL_FWD_SCALE) ? DSPEC : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);
    cf* ta = reinterpret_cast<cf*>(smem + (size_t)G::TILE_F4 * 16);
    cf* tb = ta + G::NTA;
    const int tid = threadIdx.x;
    for (int i = tid; i < G::NTA + G::NTB; i += NT) ta[i] = p.tw[i];
    __syncthreads();
    const int cp = tid % G::CPN;
    const int ncoltiles = p.ncoltiles, nsub = p.nsub, XP = p.XP;
    const long outer_stride = p.outer_stride, sub_stride = p.sub_stride, row_stride = p.row_stride;
    const int ntiles = p.nouter * ncoltiles;  // host: < 2^31 (32-bit tile arithmetic: the 64-bit division is a software loop)
    auto tile_base = [=](int tt) -> long {
        const int ou = tt / ncoltiles;
        const int ct = tt - ou * ncoltiles;
        return (long)(ou / nsub) * outer_stride + (long)(ou % nsub) * sub_stride + (long)ct * G::W + 2 * cp;
    };
    // unconditional loads (a ragged last column tile reads into the slack behind its row; those columns are never stored)
    // per-thread row offsets are 32-bit element counts from the (wave-uniform, 64-bit) tile base: N * row_stride < 2^31 (host)
    const int rs = (int)row_stride;
    float4 pre[16];
    auto load_rows = [&](int tt, int rest) {
        const cf* src = p.S + tile_base(tt);
#pragma unroll
        for (int r = 0; r < 16; ++r) pre[r] = *reinterpret_cast<const float4*>(src + row_of<LOGN, DLOAD>(rest, r) * rs);
    };
    const int rest0 = tid / G::CPN;
    const int tstep = (int)gridDim.x;
    int t = (int)blockIdx.x;
    if (t < ntiles) load_rows(t, rest0);
    for (; t < ntiles; t += tstep) {
        // opaque: the row offsets and LDS addresses derived from it are recomputed where they are used instead of being
        // hoisted out of the loop into (three sets of sixteen) long-lived registers
        const int rest = xw::opaque_i(rest0);
        const long base = tile_base(t);
        const int tn = t + tstep < ntiles ? t + tstep : t;  // unconditional prefetch (the last round re-reads its tile)
        cf x0[16], x1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            x0[r] = make_float2(pre[r].x, pre[r].y);
            x1[r] = make_float2(pre[r].z, pre[r].w);
        }
        if (MODE == COL_INV) {
            load_rows(tn, rest);
            inverse<LOGN>(x0, x1, tile, ta, tb, rest, cp);
        } else if (!HAS_OTF) {
            load_rows(tn, rest);
            forward<LOGN>(x0, x1, tile, ta, tb, rest, cp);
            if (MODE == COL_FWD_SCALE) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    x0[r] = make_float2(x0[r].x * p.scale, x0[r].y * p.scale);
                    x1[r] = make_float2(x1[r].x * p.scale, x1[r].y * p.scale);
                }
            }
        } else {
            // this tile's multiplier rows (spectrum-end distribution) ride behind the forward transform
            float4 o[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long off = base + row_of<LOGN, DSPEC>(rest, r) * rs;
                if (MODE == COL_FILTER) {
                    const float2 f = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(p.otf) + off);
                    o[r] = make_float4(f.x, f.x, f.y, f.y);
                } else if (MODE == COL_CONV16) {
                    const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned int*>(p.otf) + off);
                    o[r] = make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xffff0000u), __uint_as_float(h.y << 16),
                                       __uint_as_float(h.y & 0xffff0000u));
                } else {
                    o[r] = *reinterpret_cast<const float4*>(p.otf + off);
                }
            }
            forward<LOGN>(x0, x1, tile, ta, tb, rest, cp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const cf a0 = x0[r], a1 = x1[r];
                if (MODE == COL_FILTER) {
                    x0[r] = make_float2(a0.x * o[r].x, a0.y * o[r].y);
                    x1[r] = make_float2(a1.x * o[r].z, a1.y * o[r].w);
                } else if (MODE == COL_CORR) {
                    x0[r] = cmulc(a0, make_float2(o[r].x, o[r].y));
                    x1[r] = cmulc(a1, make_float2(o[r].z, o[r].w));
                } else {
                    x0[r] = cmul(a0, make_float2(o[r].x, o[r].y));
                    x1[r] = cmul(a1, make_float2(o[r].z, o[r].w));
                }
            }
            asm volatile("" ::: "memory");  // the next tile's rows only now: above, they would sit on top of the multiplier rows
            load_rows(tn, rest);
            __syncthreads();  // exchange 2 of the forward transform has been read by everyone
            inverse<LOGN>(x0, x1, tile, ta, tb, rest, cp);
        }
        const bool col_ok = ((t % ncoltiles) * G::W + 2 * cp) < XP;
        if (col_ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                *reinterpret_cast<float4*>(p.S + base + row_of<LOGN, DSTORE>(rest, r) * rs) =
                    make_float4(x0[r].x, x0[r].y, x1[r].x, x1[r].y);
        }
        __syncthreads();  // the last exchange of this tile has been read before the next tile writes the buffer
    }
}

// host: [ta [15][N/16]: w_N^(q k) | tb [15][N/256]: w_{N/16}^(qq k)]
template <int LOGN>
static void make_tables(std::vector<cf>& tab) {
    using G = Geo<LOGN>;
    tab.assign(G::NTA + G::NTB, make_float2(0.f, 0.f));
    for (int k = 1; k < 16; ++k) {
        for (int q = 0; q < G::N16; ++q) {
            const double a = -2.0 * M_PI * (double)q * k / (double)G::N;
            tab[(size_t)(k - 1) * G::N16 + q] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        for (int q = 0; q < G::NQ; ++q) {
            const double a = -2.0 * M_PI * (double)q * k / (double)G::N16;
            tab[G::NTA + (size_t)(k - 1) * G::NQ + q] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    }
}

}  // namespace colw
