// One-pass overhang fill of the deskew (bh_deskew with a fill, every input type) — included by deskew.hip.  The reference fills in three steps on the finished volume (biahub/deskew.py:339-368): mask = (out == 0), three
// 3x3x3 dilations, fill = mean(out[~mask]) (or a constant), out[mask] = fill.  Unless the DATA holds exact zeros, all of it
// follows from the geometry and from sums of the input:
//   * out[a, y', x'] is an exact zero iff the N taps of (a, x') all fall outside the scanned range — a pattern G[a][x'] that does
//     not depend on y' (geom_bits_kernel, from the float32 sample positions of the resampling kernel itself);
//   * its radius-3 Chebyshev dilation in 3-D is the 2-D dilation DG[a][x'] of that pattern (dilate_bits_kernel);
//   * sum over the valid voxels: the taps' weights depend on (a, k, x') only and every y' of the output reads another x of the
//     SAME input rows (z, y), so   sum_{y'} out[a, y', x'] = (1/N) sum_k ( w0 R[z0][y] + w1 R[z0+1][y] )   with the row sums
//     R[z][y] = sum_x in[z, y, x] (row_sums_kernel: one streaming read of the input, or handed in by the operator that produced
//     the volume) — mean_partial_kernel / mean_final_kernel evaluate it in float64 over (a, x') outside DG.
// The resampling kernel then knows the fill value when it starts and writes whole rows (deskew_pers_kernel<NK, 2>).
namespace rows {

// one thread per (a, word)
__global__ void geom_bits_kernel(DeskewGeom g, uint32_t* __restrict__ gb, int WB) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.Za * WB) return;
    const int a = i / WB, w = i - a * WB;
    uint32_t bits = 0u;
    for (int b = 0; b < 32; ++b) {
        const int xo = 32 * w + b;
        bool zero = true;
        if (xo < g.Xp) {
            for (int k = 0; k < g.N; ++k) {
                const DeskewTaps t = deskew_taps(g, xo, a * g.N + k);
                const bool lower = t.z0 >= 0 && t.z0 < g.Z;  // its weight w0 > 0 always
                const bool upper = t.z0 + 1 >= 0 && t.z0 + 1 < g.Z && t.w1 != 0.0f;
                if (lower || upper) zero = false;
            }
        }
        bits |= (zero ? 1u : 0u) << b;
    }
    gb[i] = bits;
}

// 2-D Chebyshev dilation by r: (a, x') set when a set bit lies within r in both directions; nothing enters from outside the
// array (max_pool3d pads with -inf) — pad bits past Xp are masked on read and set again on write
__global__ void dilate_bits_kernel(const uint32_t* __restrict__ gb, uint32_t* __restrict__ dg, int Za, int Xp, int WB, int r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Za * WB) return;
    const int a = i / WB, w = i - a * WB;
    auto word = [&](int aa, int ww) -> uint32_t {
        if (aa < 0 || aa >= Za || ww < 0 || ww >= WB) return 0u;
        uint32_t v = gb[aa * WB + ww];
        const int valid = Xp - 32 * ww;
        if (valid < 32) v &= (1u << valid) - 1u;
        return v;
    };
    uint32_t o = 0u;
    for (int da = -r; da <= r; ++da) {
        const uint32_t c = word(a + da, w), l = word(a + da, w - 1), h = word(a + da, w + 1);
        o |= c;
        for (int s = 1; s <= r; ++s) o |= (c << s) | (l >> (32 - s)) | (c >> s) | (h << (32 - s));
    }
    const int valid = Xp - 32 * w;
    if (valid < 32) o |= ~((1u << valid) - 1u);
    dg[i] = o;
}

// R[row] = sum_x in[row, x] in float64 (every value converted before it is added: the same sums, to float64 rounding, as the
// Richardson-Lucy update pass hands over): one wavefront per row at a time, 16 bytes per lane per load, four rows in flight
template <typename TIN>
__global__ __launch_bounds__(256) void row_sums_kernel(const TIN* __restrict__ in, double* __restrict__ R, long rows, int X) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const bool vec = sizeof(TIN) == 4 && (X & 3) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    for (long row = wave; row < rows; row += nwaves) {
        const TIN* rp = in + row * X;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (vec) {
            const float4* r4 = reinterpret_cast<const float4*>(rp);
            const int n4 = X >> 2;
            int i = lane;
            for (; i + 192 < n4; i += 256) {
                const float4 a = r4[i], b = r4[i + 64], c = r4[i + 128], d = r4[i + 192];
                s0 += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
                s1 += ((double)b.x + (double)b.y) + ((double)b.z + (double)b.w);
                s2 += ((double)c.x + (double)c.y) + ((double)c.z + (double)c.w);
                s3 += ((double)d.x + (double)d.y) + ((double)d.z + (double)d.w);
            }
            for (; i < n4; i += 64) {
                const float4 a = r4[i];
                s0 += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
            }
        } else {
            for (int i = lane; i < X; i += 64) s0 += (double)to_f32(rp[i]);
        }
        const double s = wave_reduce((s0 + s1) + (s2 + s3), op_sum());
        if (lane == 0) R[row] = s;
    }
}

// one workgroup per a: sum over x' outside DG of (1/N) sum_k (w0 R[z0][y] + w1 R[z0 + 1][y]), and the count of such x'
__global__ __launch_bounds__(256) void mean_partial_kernel(DeskewGeom g, const uint32_t* __restrict__ dg, int WB, const double* __restrict__ R,
                                                            double* __restrict__ psum, unsigned long long* __restrict__ pcnt) {
#pragma clang fp contract(off)
    const int a = blockIdx.x;
    double s = 0.0;
    unsigned long long c = 0;
    for (int xo = threadIdx.x; xo < g.Xp; xo += 256) {
        if ((dg[a * WB + (xo >> 5)] >> (xo & 31)) & 1u) continue;
        ++c;
        double t = 0.0;
        for (int k = 0; k < g.N; ++k) {
            const int zo = a * g.N + k;
            const DeskewTaps tp = deskew_taps(g, xo, zo);
            const int z0 = tp.z0;
            const int yin = g.Y - 1 - min(zo, g.Y - 1);
            if (z0 >= 0 && z0 < g.Z) t += (double)tp.w0 * R[(long)z0 * g.Y + yin];
            if (z0 + 1 >= 0 && z0 + 1 < g.Z) t += (double)tp.w1 * R[(long)(z0 + 1) * g.Y + yin];
        }
        s += t;
    }
    __shared__ double shs[4];
    __shared__ unsigned long long shc[4];
    wave_totals<4>(s, op_sum(), shs);
    c = block_reduce<4>(c, op_sum(), shc);
    if (threadIdx.x == 0) {
        psum[a] = (shs[0] + shs[1]) + (shs[2] + shs[3]);  // pairwise, not block_reduce's left to right: this order is part of the result
        pcnt[a] = c;
    }
}

// fixed-order final reduction; also arms the stats block for the resampling kernel (fallback flag cleared)
__global__ __launch_bounds__(256) void mean_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt, int n,
                                                          int N, long X, long total, int fill_mode, float fill_value, FillStats* st) {
    __shared__ double ss[256];
    __shared__ unsigned long long sc[256];
    double s = 0.0;
    unsigned long long c = 0;
    if (fill_mode == BH_FILL_MEAN) {
        for (int i = threadIdx.x; i < n; i += 256) {
            s += psum[i];
            c += pcnt[i];
        }
    }
    s = tree_reduce<256>(s, op_sum(), ss);
    c = tree_reduce<256>(c, op_sum(), sc);
    if (threadIdx.x == 0) {
        const double nvalid = (double)c * (double)X;
        st->sum_all = s / (double)N;
        st->sum_shell = 0.0;
        st->n_masked = (unsigned long long)total - (unsigned long long)(c * (unsigned long long)X);
        st->fill = fill_mode == BH_FILL_MEAN ? (float)((s / (double)N) / nvalid) : fill_value;  // 0/0 -> NaN like torch's empty mean
        st->fallback = 0;
    }
}

}  // namespace rows
