// Z pass of Richardson-Lucy as a direct circular convolution along z with compact taps.  Included by fftconv_colreg.hip (namespace bh).
//
// The Z pass of the engine computes Z-inverse(H . Z-forward(column)) for every (ky, kx) column of the half spectrum, with
// H = DFT_z(Q) and Q(t; ky, kx) the PSF transformed along x and y only.  A PSF of z-extent K makes Q nonzero for |t| <= K / 2
// only, so the pass is a circular convolution of each column with 2R + 1 taps: the column is read once (plus R wrap rows) and
// written once, and per column 2R + 1 (complex) or R + 1 (Hermitian) taps are read instead of Z transfer-function values.
// z stays in natural order: no LDS exchanges, no twiddles.  (colz_kernel reads 4.36 GB of transfer function per launch at the
// bench box; these taps are 0.29 GB.)
//
// One wavefront walks 64 consecutive columns (flattened (y, p): a z-row of the spectrum is contiguous, so every load and store
// is one 512-B row segment and only the very last strip can be ragged) down z.  Its lane keeps a ring of P = 2R + 1 + D rows in
// registers — rows z - R .. z + R for the output at z and D rows in flight — and the taps.  The walk is unrolled by P so every
// ring slot is a compile-time register: no moves rotate it.
//
// REALQ: Q is real (every z-slice of the PSF equals its own 180-degree rotation in (y, x): rl_probe_psf), so the taps' imaginary
// halves, which the transforms leave as round-off, are dropped: the real and imaginary halves of a column decouple and a tap
// costs ONE packed FMA whose multiplier is broadcast from one half of a register pair that holds two taps.  The tap planes keep
// their layout (fftconv_make_ztaps writes the imaginary halves as zero); these kernels load the real halves only.
//
// In place: output z is stored into row z once rows up to z + R + D have been requested, so no later global load reads a row
// that is already overwritten, except the wrap: outputs Z - R .. Z - 1 need the ORIGINAL rows 0 .. R - 1.  The wave keeps those
// rows in LDS (R x 512 B per wave) when it first loads them and reads them back at the end.
namespace zdirect {

constexpr int NT = 256;  // 4 wavefronts per workgroup
constexpr int RMAX = 16;  // the largest compiled radius (33 taps)
// Rows requested ahead of the one an output needs last, per variant: 16 waves x 8 x 512 B = 64 KiB of loads in flight per CU
// at 8.  The complex-tap kernels sit at their register limits with 8 (R = 16: 128 VGPRs Hermitian, 164 general).  The real,
// even kernel of radius 16 holds 17 floats of taps instead of 34 and spends the freed registers on 4 more rows in flight
// (122 VGPRs, 114 at 8; measured faster than 8 at the bench box).  The real general kernel of radius 16 fits 128 VGPRs without scratch at 6 (7 spills 12 B per
// lane): 4 waves x 6 rows per SIMD where the complex general kernel has 3 x 8.  Radius 4 keeps 8 everywhere: its rule
// (Z >= 4 + 8) promises no more.
#ifndef BH_ZD_D
#define BH_ZD_D 8
#endif
#ifndef BH_ZD_D_REAL
#define BH_ZD_D_REAL 12
#endif
#ifndef BH_ZD_D_REALG
#define BH_ZD_D_REALG 6
#endif
// What the eligibility rule (fftconv_ztaps_radius, launch_rl_z) asks of a column: Z > 2R and Z >= R + D_RULE.  The prologue
// of a variant with D rows in flight reads rows up to R + D - 1, so every variant needs R + D <= max(2R + 1, R + D_RULE).
constexpr int D_RULE = 8;
template <int R, int MODE, bool REALQ>
constexpr int depth() {
    return REALQ && R == RMAX ? (MODE == COL_FILTER ? BH_ZD_D_REAL : BH_ZD_D_REALG) : BH_ZD_D;
}

struct Params {
    cf* S;            // spectrum [Z][ncol]
    const cf* taps;   // COL_FILTER: [R + 1][ncol] Hermitian taps t = 0..R (tap -t = conj(tap t)); else [2R + 1][ncol], t = -R..R at t + R
    long ncol;        // complex columns per z-row (Y * XP)
    int Z;
};

typedef float v2 __attribute__((ext_vector_type(2)));

// acc + q.x * x
__device__ __forceinline__ v2 fma_re(v2 acc, v2 q, v2 x) {
    v2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(q), "v"(x), "v"(acc));
    return r;
}
// acc + q.y * x
__device__ __forceinline__ v2 fma_hi(v2 acc, v2 q, v2 x) {
    v2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0]" : "=v"(r) : "v"(q), "v"(x), "v"(acc));
    return r;
}
// acc + q.y * (i x) = acc + (-q.y x.y, q.y x.x)
__device__ __forceinline__ v2 fma_im(v2 acc, v2 q, v2 x) {
    v2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(q), "v"(x), "v"(acc));
    return r;
}
// acc + q.y * (-i x) = acc + (q.y x.y, -q.y x.x)
__device__ __forceinline__ v2 fma_imc(v2 acc, v2 q, v2 x) {
    v2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[0,1,0]" : "=v"(r) : "v"(q), "v"(x), "v"(acc));
    return r;
}

// f(integral_constant<int, K>) for K = 0 .. N - 1: every step of the walk its own code, every ring index a constant
template <class F, int... K>
__device__ __forceinline__ void static_for_(F&& f, std::integer_sequence<int, K...>) {
    (f(std::integral_constant<int, K>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_(f, std::make_integer_sequence<int, N>{});
}

// Addresses: (row pointer: a kernel argument plus a wave-uniform offset pinned in scalar registers, colz::scalar_off) + (the
// lane's 32-bit byte offset), which the loads and stores take as their scalar-base addressing mode.  With 64-bit per-lane
// addresses the compiler strength-reduces every step's row into a pointer of its own that lives across the walk, and spills.
__device__ __forceinline__ v2 ld_row(const cf* base, long off, unsigned lane_b) {
    const float2 f = *reinterpret_cast<const float2*>(reinterpret_cast<const unsigned char*>(base + colz::scalar_off(off)) + lane_b);
    return v2{f.x, f.y};
}
// the real half alone (REALQ taps)
__device__ __forceinline__ float ld_row_re(const cf* base, long off, unsigned lane_b) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(base + colz::scalar_off(off)) + lane_b);
}

// MODE: COL_FILTER (real transfer function: Hermitian taps, convolution = correlation), COL_CONV (out[z] = sum_t q(t) in[z - t]),
// COL_CORR (out[z] = sum_t conj(q(-t)) in[z - t]).  REALQ: the taps are real (with COL_FILTER real and even), two to a register pair.
template <int R, int MODE, bool REALQ>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT), amdgpu_waves_per_eu(MODE == COL_FILTER || REALQ ? 4 : 3)))
void zdirect_kernel(Params p) {
    constexpr int D = depth<R, MODE, REALQ>();
    static_assert(D >= 1 && R + D <= (2 * R + 1 > R + D_RULE ? 2 * R + 1 : R + D_RULE), "the prologue reads rows the eligibility rule does not promise");
    constexpr int P = 2 * R + 1 + D;
    constexpr bool HERM = MODE == COL_FILTER;
    constexpr int NT_ = HERM ? R + 1 : 2 * R + 1;           // taps per column
    constexpr int NQ = REALQ ? (NT_ + 1) / 2 : NT_;         // registers pairs of taps: REALQ holds tap j in half j & 1 of q[j / 2]
    __shared__ v2 stash[NT / 64][R][64];  // the original rows 0 .. R - 1 of the wave's columns
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long j0 = ((long)blockIdx.x * (NT / 64) + wave) * 64;  // first column of the wave (uniform)
    if (j0 >= p.ncol) return;
    const long ncol = p.ncol;
    const int Z = p.Z;
    const int nl = (int)min((long)64, ncol - j0);  // valid lanes (a ragged last strip: the others load a duplicate, store nothing)
    const int ll = min(lane, nl - 1);
    const unsigned lane_b = (unsigned)ll * 8u;  // the lane's byte offset in a row segment of the wave

    v2 q[NQ];
    if (REALQ) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            q[k].x = ld_row_re(p.taps, (long)(2 * k) * ncol + j0, lane_b);
            q[k].y = 2 * k + 1 < NT_ ? ld_row_re(p.taps, (long)(2 * k + 1) * ncol + j0, lane_b) : 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NQ; ++k) q[k] = ld_row(p.taps, (long)k * ncol + j0, lane_b);
    }
    // acc + (real tap j) * x
    auto fma_tap = [&](v2 acc, int j, v2 x) { return (j & 1) ? fma_hi(acc, q[j / 2], x) : fma_re(acc, q[j / 2], x); };

    v2 w[P];  // ring: row s lives in w[s mod P]
    auto slot = [](int s) { return ((s % P) + P) % P; };
    // prologue: rows -R .. R + D - 1 (rows below 0 wrap to Z - R ..); rows 0 .. R - 1 also go to the stash
#pragma unroll
    for (int s = -R; s < R + D; ++s) w[slot(s)] = ld_row(p.S, (long)(s < 0 ? s + Z : s) * ncol + j0, lane_b);
#pragma unroll
    for (int s = 0; s < R; ++s) stash[wave][s][lane] = w[slot(s)];

    // one step of the walk at z = z0 + k (z0 a multiple of P); TAIL: rows past the end (the stash) and outputs past Z exist
    auto step = [&](auto kc, int z0, auto tail) {
        constexpr int k = decltype(kc)::value;
        constexpr bool TAIL = decltype(tail)::value;
        const int z = z0 + k;
        if (TAIL && z >= Z) return;
        // request row z + R + D into the slot of row z - R - 1, which no output from z on needs
        const int s = z + R + D;
        if (!TAIL || s < Z) w[(k + R + D) % P] = ld_row(p.S, (long)s * ncol + j0, lane_b);
        else if (s < Z + R) w[(k + R + D) % P] = stash[wave][s - Z][lane];
        // out[z] from rows z - R .. z + R
        v2 acc;
        if (REALQ && HERM) {
            const v2 x = w[k % P];
            acc = v2{q[0].x * x.x, q[0].x * x.y};
#pragma unroll
            for (int t = 1; t <= R; ++t) acc = fma_tap(acc, t, w[(k - t + P) % P] + w[(k + t) % P]);  // q(t) (row z - t + row z + t)
        } else if (REALQ) {
            acc = v2{0.f, 0.f};
#pragma unroll
            for (int t = -R; t <= R; ++t)  // q(t) or q(-t) times row z - t
                acc = fma_tap(acc, MODE == COL_CONV ? t + R : R - t, w[(k - t + 2 * P) % P]);
        } else if (HERM) {
            const v2 x = w[k % P];
            acc = v2{q[0].x * x.x, q[0].x * x.y};
#pragma unroll
            for (int t = 1; t <= R; ++t) {
                const v2 a = w[(k - t + P) % P], b = w[(k + t) % P];  // rows z - t, z + t
                acc = fma_re(acc, q[t], a + b);                       // q(t) a + conj(q(t)) b = Re q (a + b) + i Im q (a - b)
                acc = fma_im(acc, q[t], a - b);
            }
        } else {
            acc = v2{0.f, 0.f};
#pragma unroll
            for (int t = -R; t <= R; ++t) {
                const v2 a = w[(k - t + 2 * P) % P];  // row z - t
                if (MODE == COL_CONV) {
                    const v2 qq = q[t + R];
                    acc = fma_im(fma_re(acc, qq, a), qq, a);
                } else {
                    const v2 qq = q[R - t];
                    acc = fma_imc(fma_re(acc, qq, a), qq, a);
                }
            }
        }
        // lanes of a ragged strip past the last column store their duplicate of the last column's value to that column
        *reinterpret_cast<float2*>(reinterpret_cast<unsigned char*>(p.S + colz::scalar_off((long)z * ncol + j0)) + lane_b) = make_float2(acc.x, acc.y);
        // steps stay in order: the scheduler otherwise hoists the loads of later steps, and the ring plus those loads spill
        __builtin_amdgcn_sched_barrier(0);
    };
    // whole chunks whose rows are all in the volume: straight-line code, no branch between two steps
    int z0 = 0;
#pragma unroll 1
    for (; z0 + P - 1 + R + D < Z; z0 += P) static_for<P>([&](auto kc) { step(kc, z0, std::false_type{}); });
#pragma unroll 1
    for (; z0 < Z; z0 += P) static_for<P>([&](auto kc) { step(kc, z0, std::true_type{}); });
}

}  // namespace zdirect
