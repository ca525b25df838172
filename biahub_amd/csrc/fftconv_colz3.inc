// Z pass of 384- and 768-point columns (3 x 128, 3 x 256) with register stages — the deskewed volumes of BASELINE config 4,
// (342, 1024, 1517), and config 2, (683, 2048, 3034), run Richardson-Lucy at the boxes (384, 1024, 1536) and (768, 2048, 3072).
// Included by fftconv_colreg.hip after fftconv_colz.inc, whose radix-8 butterflies it reuses.
//
// col_pass_kernel runs such a column as a radix-3 step, a radix-2 step and three radix-4 steps through LDS, forward and back:
// ten LDS round trips and eleven barriers per 96-KiB tile (1.89 ms per pass at that box, 3.3 TB/s).  Here, as in colz_kernel,
// a 1024-thread workgroup keeps the rows in registers between FOUR round trips:
//   A   radix-3 across the thirds + the first radix-2 level(s) of each third  6 / 12 rows per thread: L j + 64 i + m  (1024 / 512 threads;
//       L = 128: one level, 32-column tiles; L = 256: two levels, 16-column tiles — the tile is 96 KiB either way)
//   B   radix-8 (spans 32, 16, 8) inside each 64-row block                    8 rows per thread: block + 8 u + r      ( 768 threads)
//   C   radix-8 (spans 4, 2, 1) + the spectral product + C' of the inverse    8 consecutive rows                      ( 768 threads)
//   B', A' mirrored with conjugate twiddles; A' hands its rows to the global stores, the next tile's rows arrive in A's
//   distribution behind B' and A'.
// Every level is the in-place decimation-in-frequency level col_pass_kernel runs (radix3_step, then the seven radix-2 levels of
// a 128-point third), so the row order — third k holds the frequencies 3 j + k at the bit-reversed position of j — and every
// transfer function staged for the old pass fit unchanged.
namespace colz3 {

using colz::C2;
using colz::fwd8;
using colz::inv8;
using colz::pack;
using colz::spec_mul;
using colz::unpack;

template <int LOGL>
struct Geo {
    static constexpr int L = 1 << LOGL, N = 3 * L;          // rows per third, rows
    static constexpr int NLEV = LOGL - 6;                   // radix-2 levels step A runs on every third (the rest: two radix-8 steps)
    static constexpr int RPT = 1 << NLEV;                   // rows per thread and third in step A
    static constexpr int W = 12288 / N, CP = W / 2;         // complex columns per tile (32 / 16), column pairs (float4) per row
    static constexpr int NTA = 64 * CP;                     // threads of step A (3 RPT rows x 2 columns each)
    static constexpr int NBC = (N / 8) * CP;                // threads of steps B and C (8 rows x 2 columns each): 768
    static constexpr int NT = NTA > NBC ? NTA : NBC;
    static constexpr int NTAB = 2 * L + (NLEV == 2 ? 128 : 0) + 64 + 8 * 3;  // [w_N^m | w_N^2m | (w_256^m, m < 128) | w_128^m, m < 64 | w_64^q, w_32^q, w_16^q]
    static constexpr int LDS_BYTES = N * W * 8 + NTAB * 8;
};
constexpr int N = 384, W = 32;  // the smaller geometry (host-side dispatch names)

__device__ __forceinline__ C2 scale(C2 x, float f) { return C2{make_float2(x.a.x * f, x.a.y * f), make_float2(x.b.x * f, x.b.y * f)}; }

template <int LOGL, int MODE>
__global__ __launch_bounds__(Geo<LOGL>::NT) void colz3_kernel(ColParams p) {
    using G = Geo<LOGL>;
    constexpr int L = G::L, N = G::N, W = G::W, CP = G::CP, NT = G::NT, RPT = G::RPT, RA = 3 * RPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);             // [N][CP]
    cf* t3 = reinterpret_cast<cf*>(smem + (size_t)N * W * 8);   // w_N^m, then w_N^2m (m < L)
    cf* t1 = t3 + 2 * L;                                        // L = 256 only: w_256^m, m < 128 (the span-128 level)
    cf* t2 = t1 + (G::NLEV == 2 ? 128 : 0);                     // w_128^m, m < 64 (the span-64 level)
    cf* tb = t2 + 64;                                           // [8][3]: w_64^q, w_32^q, w_16^q
    const int tid = threadIdx.x;
    for (int i = tid; i < G::NTAB; i += NT) t3[i] = p.tw[i];
    const int cp = tid % CP, g = tid / CP;
    const bool ta = tid < G::NTA;                               // takes part in step A (g < 64)
    const bool bc = tid < G::NBC;                               // takes part in steps B and C (g < N / 8)
    const int ncoltiles = p.ncoltiles, XP = p.XP;
    const long outer_stride = p.outer_stride, row_stride = p.row_stride;
    const long ntiles = (long)p.nouter * ncoltiles;
    // Addresses as in colz_kernel: a wave-uniform row pointer (tile base + the wavefront's first row + the access's row: scalar
    // registers, pinned by colz::scalar_off) plus ONE loop-invariant 32-bit lane offset per distribution (the lane's row inside
    // the wavefront and its column pair), instead of a 64-bit multiply-add per lane and access; the tile's (outer, column tile)
    // pair advances by additions instead of two 64-bit divisions per tile.  The host checks that 64 rows span less than 4 GiB.
    constexpr int GPW = 64 / CP;  // g values per wavefront
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gl = (tid & 63) / CP;
    constexpr int OB = MODE == COL_FILTER ? 4 : 8;  // bytes per multiplier element
    const unsigned laneA_ = (unsigned)(((long)gl * row_stride + 2 * cp) * 8);          // spectrum, rows (wave's first) + gl
    const unsigned laneC_ = (unsigned)(((long)(8 * gl) * row_stride + 2 * cp) * OB);   // multiplier, rows 8 g + i
    const int step_ou = (int)(gridDim.x / (unsigned)ncoltiles), step_ct = (int)(gridDim.x % (unsigned)ncoltiles);
    int cur_ou = (int)(blockIdx.x / (unsigned)ncoltiles), cur_ct = (int)(blockIdx.x % (unsigned)ncoltiles);
    auto base_of = [=](int ou, int ct) -> long { return (long)ou * outer_stride + (long)(ct * W); };  // wave-uniform
    // distribution A: register RPT j + i holds row L j + 64 i + g (third j, i-th 64-row block of the third)
    auto row_a = [](int gg, int u) { return L * (u / RPT) + 64 * (u % RPT) + gg; };
    auto rowA_ptr = [=](long base, int u) {
        return reinterpret_cast<const unsigned char*>(p.S + colz::scalar_off(base + (long)row_a(GPW * wave, u) * row_stride));
    };
    float4 v[RA];
    long t = blockIdx.x;
    if (t < ntiles && ta) {
        const long base0 = base_of(cur_ou, cur_ct);
        const unsigned la = (unsigned)xw::opaque_i((int)laneA_);
#pragma unroll
        for (int u = 0; u < RA; ++u) v[u] = *reinterpret_cast<const float4*>(rowA_ptr(base0, u) + la);
    }
    __syncthreads();  // twiddle tables
    const float S3 = 0.86602540378443865f;
    for (; t < ntiles; t += gridDim.x) {
        const int go = xw::opaque_i(g);
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
        // rows of distributions B and C (threads < NBC): 64-row block go / 8, r = go % 8
        const int rowB = (go >> 3) * 64 + (go & 7), rowC = go * 8;
        // ---- A: radix-3 across the thirds (twiddles w_N^(k m')), then the span-128 (L = 256) and span-64 levels of every third
        if (ta) {
            C2 x[RA];
#pragma unroll
            for (int u = 0; u < RA; ++u) x[u] = unpack(v[u]);
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int mp = go + 64 * i;  // position inside the third
                const C2 a = x[i], b = x[RPT + i], c = x[2 * RPT + i];
                const C2 sm = b + c, df = b - c;
                const C2 bs = a - scale(sm, 0.5f);
                const C2 rot = scale(colz::mi(df), S3);
                x[i] = a + sm;
                x[RPT + i] = colz::mulw(bs + rot, t3[mp]);
                x[2 * RPT + i] = colz::mulw(bs - rot, t3[L + mp]);
            }
            if (G::NLEV == 2) {  // span 128: blocks (0, 2) and (1, 3) of every third, twiddle w_256^(64 (i & 1) + g)
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const cf w = t1[go + 64 * i];
                        const C2 s = x[RPT * k + i] + x[RPT * k + i + 2], d = x[RPT * k + i] - x[RPT * k + i + 2];
                        x[RPT * k + i] = s;
                        x[RPT * k + i + 2] = colz::mulw(d, w);
                    }
            }
            const cf w = t2[go];  // span 64: neighbouring blocks
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < RPT; i += 2) {
                    const C2 s = x[RPT * k + i] + x[RPT * k + i + 1], d = x[RPT * k + i] - x[RPT * k + i + 1];
                    x[RPT * k + i] = s;
                    x[RPT * k + i + 1] = colz::mulw(d, w);
                }
#pragma unroll
            for (int u = 0; u < RA; ++u) tile[row_a(go, u) * CP + cp] = pack(x[u]);
        }
        // this tile's multiplier rows (distribution C) ride behind steps A and B
        float4 o[8];
        if (bc) {
            const unsigned laneC = (unsigned)xw::opaque_i((int)laneC_);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned char* rp = reinterpret_cast<const unsigned char*>(p.otf) +
                                          colz::scalar_off((base + (long)(8 * GPW * wave + i) * row_stride) * OB);
                if (MODE == COL_FILTER) {
                    const float2 f = *reinterpret_cast<const float2*>(rp + laneC);
                    o[i] = make_float4(f.x, f.y, 0.f, 0.f);
                } else {
                    o[i] = *reinterpret_cast<const float4*>(rp + laneC);
                }
            }
        }
        __syncthreads();
        C2 x[8];
        if (bc) {
            // ---- B: spans 32, 16, 8 of the 64-row block
            const cf b1 = tb[(go & 7) * 3], b2 = tb[(go & 7) * 3 + 1], b3 = tb[(go & 7) * 3 + 2];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowB + 8 * i) * CP + cp]);
            fwd8<true>(x, b1, b2, b3);
#pragma unroll
            for (int i = 0; i < 8; ++i) tile[(rowB + 8 * i) * CP + cp] = pack(x[i]);
        }
        __syncthreads();
        if (bc) {
            // ---- C, the spectral product, C'
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowC + i) * CP + cp]);
            const cf one = make_float2(1.f, 0.f);
            fwd8<false>(x, one, one, one);
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = spec_mul<MODE>(x[i], o[i], 0, 1.f);
            inv8<false>(x, one, one, one);
#pragma unroll
            for (int i = 0; i < 8; ++i) tile[(rowC + i) * CP + cp] = pack(x[i]);
        }
        __syncthreads();
        // the next tile's rows travel behind B' and A'
        if (tn < ntiles && ta) {
            const unsigned la = (unsigned)xw::opaque_i((int)laneA_);
#pragma unroll
            for (int u = 0; u < RA; ++u) v[u] = *reinterpret_cast<const float4*>(rowA_ptr(base_n, u) + la);
        }
        if (bc) {
            // ---- B'
            const int gq = xw::opaque_i(go) & 7;
            const cf c1 = tb[gq * 3], c2 = tb[gq * 3 + 1], c3 = tb[gq * 3 + 2];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = unpack(tile[(rowB + 8 * i) * CP + cp]);
            inv8<true>(x, c1, c2, c3);
#pragma unroll
            for (int i = 0; i < 8; ++i) tile[(rowB + 8 * i) * CP + cp] = pack(x[i]);
        }
        __syncthreads();
        // ---- A' and out (the same LDS words this thread overwrites in the next tile's A: no barrier in between)
        if (ta) {
            C2 y[RA];
#pragma unroll
            for (int u = 0; u < RA; ++u) y[u] = unpack(tile[(row_a(go, u)) * CP + cp]);
            const int ga = xw::opaque_i(go);
            const cf w = t2[ga];
#pragma unroll
            for (int k = 0; k < 3; ++k)  // inverse span-64 level: (a, b) <- (a + b conj(w), a - b conj(w))
#pragma unroll
                for (int i = 0; i < RPT; i += 2) {
                    const C2 u = colz::mulwc(y[RPT * k + i + 1], w);
                    const C2 a = y[RPT * k + i];
                    y[RPT * k + i] = a + u;
                    y[RPT * k + i + 1] = a - u;
                }
            if (G::NLEV == 2) {  // inverse span-128 level
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const C2 u = colz::mulwc(y[RPT * k + i + 2], t1[ga + 64 * i]);
                        const C2 a = y[RPT * k + i];
                        y[RPT * k + i] = a + u;
                        y[RPT * k + i + 2] = a - u;
                    }
            }
#pragma unroll
            for (int i = 0; i < RPT; ++i) {  // inverse radix-3 (unnormalised)
                const int mp = ga + 64 * i;
                const C2 a = y[i];
                const C2 b = colz::mulwc(y[RPT + i], t3[mp]), c = colz::mulwc(y[2 * RPT + i], t3[L + mp]);
                const C2 sm = b + c, df = b - c;
                const C2 bs = a - scale(sm, 0.5f);
                const C2 rot = scale(colz::pi(df), S3);
                y[i] = a + sm;
                y[RPT + i] = bs + rot;
                y[2 * RPT + i] = bs - rot;
            }
            if (ct * W + 2 * cp < XP) {  // pad columns of a ragged last tile are never stored
                const unsigned la = (unsigned)xw::opaque_i((int)laneA_);
#pragma unroll
                for (int u = 0; u < RA; ++u) *reinterpret_cast<float4*>(const_cast<unsigned char*>(rowA_ptr(base, u)) + la) = pack(y[u]);
            }
        }
    }
}

// host: [w_N^m, m < L | w_N^2m | (L = 256: w_256^m, m < 128) | w_128^m, m < 64 | [8][3] w_64^q, w_32^q, w_16^q] (forward sign)
template <int LOGL>
static void make_tables(std::vector<cf>& tab) {
    using G = Geo<LOGL>;
    tab.clear();
    auto w = [](int n, int k) {
        const double a = -2.0 * M_PI * (double)k / (double)n;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int m = 0; m < G::L; ++m) tab.push_back(w(G::N, m));
    for (int m = 0; m < G::L; ++m) tab.push_back(w(G::N, 2 * m));
    if (G::NLEV == 2)
        for (int m = 0; m < 128; ++m) tab.push_back(w(256, m));
    for (int m = 0; m < 64; ++m) tab.push_back(w(128, m));
    for (int q = 0; q < 8; ++q) {
        tab.push_back(w(64, q));
        tab.push_back(w(32, q));
        tab.push_back(w(16, q));
    }
}

}  // namespace colz3
