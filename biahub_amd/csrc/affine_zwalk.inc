// Z-separable linear warps: every wave walks its own column of output rows through z.  Included by affine.hip (namespace bh).
//
// When the pull matrix splits into z' = a z + t (a >= 0) and (y', x') = f(y, x) — every stabilisation shift, and a
// registration whose rotation is about the z axis (biahub/register.py:202-281, stabilize.py:32-90 apply such matrices to every
// time point) — a lane's row and column taps, their fractions and its inside/outside decision in y and x are the same on every
// output plane, and the source plane index is the same for the whole wave.  A wave owns RY output rows x 64 columns and walks a
// chunk of output planes: each source plane is loaded ONCE per wave as x-pairs of the rows it needs (straight into registers,
// D planes ahead of their use, by hand-counted asm loads; no LDS, no barrier, no tile phases — the staged-tile kernel spends 2 of its 4.8 ms in phases
// that do not overlap), reduced to its y-lerped pair A and shared by the two output planes that bracket it.  The operations
// and their order are lerp8's on the same clamped taps, the Q32.32 coordinates are the same integers and the inside tests the
// same float64 expressions, so the result is bit-identical to affine_kernel's for every voxel (tests compare the two).
namespace zw {

#ifndef BH_ZW_D
#define BH_ZW_D 4
#endif
constexpr int RY = 4;                // output rows per wave
constexpr int D = BH_ZW_D;           // source planes in flight per wave (register ring)
#ifndef BH_ZW_DL
#define BH_ZW_DL 2
#endif
constexpr int DL = BH_ZW_DL;         // ... of the LDS ring (1, 2, 3 measured alike, 4 is 2 % slower)
constexpr int NSLOT = DL > 2 ? DL : 2;  // slots per wave (the first two planes of a chunk land in slots 0 and 1)
#ifndef BH_ZW_NWX  // waves of a workgroup along x and along y
#define BH_ZW_NWX 1
#endif
#ifndef BH_ZW_NWY
#define BH_ZW_NWY 4
#endif
#ifndef BH_ZW_PROBE  // measurement builds: 1 = no stores, 2 = no loads
#define BH_ZW_PROBE 0
#endif
constexpr int NWX = BH_ZW_NWX, NWY = BH_ZW_NWY, NW = NWX * NWY, NT = 64 * NW;  // a workgroup = four y-neighbours (16 rows; 1 x 4 measured 4.27 ms, 2 x 2 4.30, 4 x 1 4.38)

// A pair of neighbouring samples at byte offset `off` of a source plane (offsets are 32-bit: scalar base + lane offset
// addressing).  Pairs sit on element boundaries only, so the 8/4/2-byte loads are under-aligned by design.
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32_a2 __attribute__((aligned(2)));
typedef uint16_t u16_a1 __attribute__((aligned(1)));

// Keeps the zero-extension of a lane offset next to its use, so that the access is selected as scalar base + 32-bit lane
// offset (hoisted out of the plane loop it becomes a 64-bit lane address: two more registers and a 64-bit add per access).
__device__ __forceinline__ unsigned here(unsigned off) {
    asm volatile("" : "+v"(off));
    return off;
}

template <typename T>
__device__ __forceinline__ f2 load_pair(const T* plane, unsigned off);  // compiler-visible form (the rare redo path)
template <>
__device__ __forceinline__ f2 load_pair<float>(const float* plane, unsigned off) {
    const f2u v = *reinterpret_cast<const f2u*>(reinterpret_cast<const char*>(plane) + here(off));
    return f2{v.x, v.y};
}
template <>
__device__ __forceinline__ f2 load_pair<uint16_t>(const uint16_t* plane, unsigned off) {
    const uint32_t v = *reinterpret_cast<const u32_a2*>(reinterpret_cast<const char*>(plane) + here(off));
    return f2{(float)(v & 0xffffu), (float)(v >> 16)};
}
template <>
__device__ __forceinline__ f2 load_pair<int16_t>(const int16_t* plane, unsigned off) {
    const uint32_t v = *reinterpret_cast<const u32_a2*>(reinterpret_cast<const char*>(plane) + here(off));
    return f2{(float)(int16_t)(v & 0xffffu), (float)((int32_t)v >> 16)};
}
template <>
__device__ __forceinline__ f2 load_pair<uint8_t>(const uint8_t* plane, unsigned off) {
    const uint32_t v = *reinterpret_cast<const u16_a1*>(reinterpret_cast<const char*>(plane) + here(off));
    return f2{(float)(v & 0xffu), (float)(v >> 8)};
}

// The plane ring is loaded by hand: hipcc (ROCm 7.2) waits for a rotating register ring as if nothing newer than the stage
// being consumed were in flight (vmcnt(7) where 23 is right), which serialises the planes.  An asm load is invisible to its
// counter logic; `landed` is the matching wait — it passes the destination registers through the s_waitcnt, so no use can be
// scheduled above it — with the count of asm loads issued after the stage (stores in between only make the wait earlier).
template <typename T>
struct Raw {
    typedef uint32_t type;
};
template <>
struct Raw<float> {
    typedef f2 type;
};
template <typename T>
__device__ __forceinline__ typename Raw<T>::type issue_pair(const T* plane, unsigned off);
template <>
__device__ __forceinline__ f2 issue_pair<float>(const float* plane, unsigned off) {
    f2 v;
#ifdef BH_ZW_SPLIT  // two dword loads (twice the instructions; `landed` counts are for the single-load form, so only for D >= 2 probes)
    asm volatile("global_load_dword %0, %2, %3\n\tglobal_load_dword %1, %2, %3 offset:4" : "=&v"(v.x), "=&v"(v.y) : "v"(off), "s"(plane) : "memory");
#else
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
#endif
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_pair<uint16_t>(const uint16_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_pair<int16_t>(const int16_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_pair<uint8_t>(const uint8_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_ushort %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <typename T>
__device__ __forceinline__ f2 widen(typename Raw<T>::type v);
template <>
__device__ __forceinline__ f2 widen<float>(f2 v) {
    return v;
}
template <>
__device__ __forceinline__ f2 widen<uint16_t>(uint32_t v) {
    return f2{(float)(v & 0xffffu), (float)(v >> 16)};
}
template <>
__device__ __forceinline__ f2 widen<int16_t>(uint32_t v) {
    return f2{(float)(int16_t)(v & 0xffffu), (float)((int32_t)v >> 16)};
}
template <>
__device__ __forceinline__ f2 widen<uint8_t>(uint32_t v) {
    return f2{(float)(v & 0xffu), (float)((v >> 8) & 0xffu)};
}
template <int N, typename R>
__device__ __forceinline__ void landed(R (&d)[4][2]) {  // RY == 4
#ifdef BH_ZW_SPLIT
    constexpr int NN = 2 * N < 63 ? 2 * N : 63;
#else
    constexpr int NN = N < 63 ? N : 63;
#endif
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]), "+v"(d[2][0]), "+v"(d[2][1]), "+v"(d[3][0]),
                   "+v"(d[3][1])
                 : "n"(NN)
                 : "memory");
}

// nearest-neighbour walk: one element per lane and row
template <typename T>
struct Raw1 {
    typedef uint32_t type;
};
template <>
struct Raw1<float> {
    typedef float type;
};
template <typename T>
__device__ __forceinline__ typename Raw1<T>::type issue_one(const T* plane, unsigned off);
template <>
__device__ __forceinline__ float issue_one<float>(const float* plane, unsigned off) {
    float v;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_one<uint16_t>(const uint16_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_ushort %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_one<int16_t>(const int16_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_sshort %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <>
__device__ __forceinline__ uint32_t issue_one<uint8_t>(const uint8_t* plane, unsigned off) {
    uint32_t v;
    asm volatile("global_load_ubyte %0, %1, %2" : "=v"(v) : "v"(off), "s"(plane) : "memory");
    return v;
}
template <typename T>
__device__ __forceinline__ float widen_one(typename Raw1<T>::type v) {
    return (float)v;
}
template <>
__device__ __forceinline__ float widen_one<float>(float v) {
    return load_clean(&v);  // np.nan_to_num
}
template <>
__device__ __forceinline__ float widen_one<int16_t>(uint32_t v) {
    return (float)(int32_t)v;  // global_load_sshort sign-extends
}
template <int N, typename R>
__device__ __forceinline__ void landed1(R (&d)[4]) {  // RY == 4
    constexpr int NN = N < 63 ? N : 63;
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]) : "n"(NN) : "memory");
}

// edge clamp along x: the pair was read at the clamped base; sel 1 = both taps are the first (ix = -1), 2 = both the second
template <bool XEDGE>
__device__ __forceinline__ f2 fix_pair(f2 P, int sel) {
    if (XEDGE) {
        if (sel == 1) P.y = P.x;
        if (sel == 2) P.x = P.y;
    }
    return P;
}

struct Rows {  // per-lane constants of the wave's RY output rows
    unsigned off0[RY], off1[RY];  // byte offsets of the two source rows (clamped) at the clamped pair base, within a plane
    float fy[RY], fx[RY];
    int sel[RY];
    bool inside[RY], store[RY];
};

// LDS-DMA form of the plane ring (float32 / 16-bit input with 16-B aligned rows, waves whose source box lies inside the volume): the
// wave's source box of a plane — the rows and 16-B quads any of its lanes taps, the same for every plane — lands in a
// wave-private LDS slot by 1-KiB global_load_lds_dwordx4 instructions (1-4 per plane against 8 pair loads: the walk is bound
// by vector-memory instructions, not bytes), and the lanes read their pairs from there.  No barrier: the slot is only this
// wave's, ordered by its own vmcnt / lgkmcnt.
constexpr int QMAX = 4;  // DMA instructions per plane at most (a 4-KiB slot)
struct LdsBox {
    int on;                 // wave-uniform: this wave uses the LDS ring
    int nq;                 // DMA instructions per plane (1 .. QMAX)
    unsigned S;             // quads per plane
    unsigned doff[QMAX];    // per lane: byte offset of its quad of instruction i within a source plane
    unsigned loff[RY];      // per lane: byte offset of row r's first tap within a slot
    unsigned pitch;         // slot row pitch in bytes
    unsigned slot0, slot_bytes;  // LDS byte address of this wave's first slot, slot size
};

__device__ __forceinline__ void dma_quad(const void* plane, unsigned off, unsigned lds_dst) {
    unsigned keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);  // wave-uniform by construction
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(off), "s"(plane), "s"(lds_dst)
        : "memory");
}

// a lane's pair of neighbouring samples at byte offset `off` of a landed slot.  16-bit samples: the two aligned words that hold
// the pair, funnel-shifted (2-byte LDS reads measured 7.3 ms per 8.6-Gvoxel volume against 4.7 ms for the register ring)
template <typename T>
__device__ __forceinline__ f2 lds_pair(const unsigned char* slot, unsigned off);
template <>
__device__ __forceinline__ f2 lds_pair<float>(const unsigned char* slot, unsigned off) {
    const float* t = reinterpret_cast<const float*>(slot + off);
    return f2{t[0], t[1]};
}
__device__ __forceinline__ uint32_t lds_pair16(const unsigned char* slot, unsigned off) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(slot + (off & ~3u));
    return __builtin_amdgcn_alignbit(w[1], w[0], (off & 2u) * 8u);
}
template <>
__device__ __forceinline__ f2 lds_pair<uint16_t>(const unsigned char* slot, unsigned off) {
    const uint32_t v = lds_pair16(slot, off);
    return f2{(float)(v & 0xffffu), (float)(v >> 16)};
}
template <>
__device__ __forceinline__ f2 lds_pair<int16_t>(const unsigned char* slot, unsigned off) {
    const uint32_t v = lds_pair16(slot, off);
    return f2{(float)(int16_t)(v & 0xffffu), (float)((int32_t)v >> 16)};
}
template <>
__device__ __forceinline__ f2 lds_pair<uint8_t>(const unsigned char* slot, unsigned off) {  // never used: 8-bit input keeps the register ring
    return f2{(float)slot[off], (float)slot[off + 1]};
}

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < 63 ? N : 63) : "memory");
}
// all but the newest n * nq DMA instructions have landed (nq is wave-uniform)
template <int NPL>
__device__ __forceinline__ void wait_planes(int nq) {
    if (nq == 1) wait_vm<NPL * 1>();
    else if (nq == 2) wait_vm<NPL * 2>();
    else if (nq == 3) wait_vm<NPL * 3>();
    else wait_vm<NPL * 4>();
}

template <typename TIN, int BOUNDARY, bool XEDGE, bool LDS = false>
__device__ __forceinline__ void walk(const TIN* __restrict__ in, float* __restrict__ out, const AffineParams& p, const Rows& R,
                                     int ox, int oy0, int ka, int kb, const LdsBox& bx = LdsBox{}) {
    const size_t sZ = (size_t)p.Yi * p.Xi;
    const long long a = p.mq[0];
    // planes past the last one this chunk samples are never used: the ring's run-ahead re-requests that plane instead
    const int pz_last = (int)((a * (long long)(kb - 1 + p.cz) + p.mq[3]) >> 32) + 1;
    auto plane_ptr = [&](int pz) -> const TIN* { return in + (size_t)max(0, min(min(pz, pz_last), p.Zi - 1)) * sZ; };
    typedef typename Raw<TIN>::type raw_t;
    constexpr int LP = 2 * RY;  // loads per plane
    auto load_plane = [&](int pz, raw_t (&dst)[RY][2]) {
        const TIN* pl = plane_ptr(pz);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
#if BH_ZW_PROBE == 2
            dst[r][0] = dst[r][1] = typename Raw<TIN>::type{};
            asm volatile("" : "+v"(dst[r][0]), "+v"(dst[r][1]));
#else
            dst[r][0] = issue_pair<TIN>(pl, R.off0[r]);
            dst[r][1] = issue_pair<TIN>(pl, R.off1[r]);
#endif
        }
    };
    auto ylerp = [&](const raw_t (&src)[RY][2], f2 (&A)[RY]) {
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const f2 P0 = fix_pair<XEDGE>(widen<TIN>(src[r][0]), R.sel[r]), P1 = fix_pair<XEDGE>(widen<TIN>(src[r][1]), R.sel[r]);
            const f2 fy = {R.fy[r], R.fy[r]};
            A[r] = __builtin_elementwise_fma(fy, P1 - P0, P0);
        }
    };
    constexpr int DR = LDS ? DL : D;  // ring depth of this form
    extern __shared__ __attribute__((aligned(16))) unsigned char zw_lds[];
    auto dma_plane = [&](int pz, int slot) {  // LDS ring: request a source plane's box into a slot
        const TIN* pl = plane_ptr(pz);
        const unsigned dst = bx.slot0 + (unsigned)slot * bx.slot_bytes;
#pragma unroll
        for (int i = 0; i < QMAX; ++i)
            if (i < bx.nq && (unsigned)(i * 64 + (threadIdx.x & 63)) < bx.S) dma_quad(pl, bx.doff[i], dst + i * 1024u);
    };
    auto lds_take = [&](int slot, f2 (&A)[RY]) {  // y-lerped pairs of a landed plane
        const unsigned char* sl = zw_lds + (bx.slot0 + (unsigned)slot * bx.slot_bytes);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const f2 P0 = lds_pair<TIN>(sl, bx.loff[r]), P1 = lds_pair<TIN>(sl, bx.loff[r] + bx.pitch);
            const f2 fy = {R.fy[r], R.fy[r]};
            A[r] = __builtin_elementwise_fma(fy, P1 - P0, P0);
        }
    };
    long long cz = a * (long long)(ka + p.cz) + p.mq[3];
    int pz = (int)(cz >> 32);
    f2 Alo[RY], Ahi[RY];
    raw_t ring[LDS ? 1 : D][RY][2];
    if constexpr (LDS) {
        dma_plane(pz, 0);
        dma_plane(pz + 1, 1);
        wait_vm<0>();
        lds_take(0, Alo);
        lds_take(1, Ahi);
#pragma unroll
        for (int s = 0; s < DL; ++s) dma_plane(pz + 2 + s, s);
    } else {
        raw_t t0[RY][2], t1[RY][2];
        load_plane(pz, t0);
        load_plane(pz + 1, t1);
#pragma unroll
        for (int s = 0; s < D; ++s) load_plane(pz + 2 + s, ring[s]);
        landed<(D + 1) * LP>(t0);
        ylerp(t0, Alo);
        landed<D * LP>(t1);
        ylerp(t1, Ahi);
    }
    int k = ka;
    auto emit = [&]() {  // output plane k from the source planes pz, pz + 1
        const float fzf = (float)(unsigned)cz * 2.3283064365386963e-10f;
        const f2 fz = {fzf, fzf};
        bool zin;
        {
#pragma clang fp contract(off)
            const double c = p.m[0] * (double)(k + p.cz) + p.m[3];
            zin = BOUNDARY == BH_BOUNDARY_ITK ? (c >= -0.5 && c < (double)p.Zi - 0.5) : (c >= 0.0 && c <= (double)(p.Zi - 1));
        }
        char* oplane = reinterpret_cast<char*>(out + ((size_t)k * p.Yo + oy0) * p.Xo);
        float v[RY];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const f2 B = __builtin_elementwise_fma(fz, Ahi[r] - Alo[r], Alo[r]);
            v[r] = __builtin_fmaf(R.fx[r], B.y - B.x, B.x);
            bad = bad || !__builtin_isfinite(v[r]);
        }
#ifndef BH_ZW_NORARE
        if (__builtin_expect(bad, 0)) {  // a NaN / inf tap somewhere: redo those voxels on np.nan_to_num'd taps
            const TIN *pl0 = plane_ptr(pz), *pl1 = plane_ptr(pz + 1);
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                if (!__builtin_isfinite(v[r])) {
                    const f2 P0 = clean2(fix_pair<XEDGE>(load_pair<TIN>(pl0, R.off0[r]), R.sel[r]));
                    const f2 P1 = clean2(fix_pair<XEDGE>(load_pair<TIN>(pl0, R.off1[r]), R.sel[r]));
                    const f2 P2 = clean2(fix_pair<XEDGE>(load_pair<TIN>(pl1, R.off0[r]), R.sel[r]));
                    const f2 P3 = clean2(fix_pair<XEDGE>(load_pair<TIN>(pl1, R.off1[r]), R.sel[r]));
                    v[r] = lerp8f_clean(P0, P1, P2, P3, fzf, R.fy[r], R.fx[r]);
                }
            }
        }
#endif
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (!(zin && R.inside[r])) v[r] = p.cval;
#if BH_ZW_PROBE == 1
            if (v[r] == 1.2345e-30f)
#endif
            if (R.store[r]) *reinterpret_cast<float*>(oplane + (size_t)r * p.Xo * 4 + here((unsigned)(ox * 4))) = v[r];
        }
    };
    bool done = false;
    while (!done) {
#pragma unroll
        for (int s = 0; s < DR; ++s) {
            if (!done) {
                while (k < kb && (int)(cz >> 32) <= pz) {  // wave-uniform: 0, 1 or 2 output planes per source plane
                    emit();
                    ++k;
                    cz += a;
                }
                if (k >= kb) {
                    done = true;
                } else {  // next source plane: its pairs were requested D planes ago
                    ++pz;
#pragma unroll
                    for (int r = 0; r < RY; ++r) Alo[r] = Ahi[r];
                    if constexpr (LDS) {
                        wait_planes<DL - 1>(bx.nq);
                        lds_take(s, Ahi);
                        dma_plane(pz + 1 + DL, s);
                    } else {
                        landed<(D - 1) * LP>(ring[s]);
                        ylerp(ring[s], Ahi);
                        load_plane(pz + 1 + D, ring[s]);
                    }
                }
            }
        }
    }
}

// Nearest neighbour: the source element of a lane's row is fixed in y and x, the source plane is wave-uniform; the float64
// coordinates, the inside rule and floor(c + 0.5) are affine_kernel's, evaluated once per lane and row (y, x) and once per
// plane (z).  Output plane k + DN is requested while plane k is stored.
constexpr int DN = 6;
template <typename TIN, int BOUNDARY>
__device__ __forceinline__ void walk_nearest(const TIN* __restrict__ in, float* __restrict__ out, const AffineParams& p,
                                             const unsigned (&off)[RY], const bool (&ok)[RY], const bool (&store)[RY], int ox,
                                             int oy0, int ka, int kb) {
    typedef typename Raw1<TIN>::type raw_t;
    const size_t sZ = (size_t)p.Yi * p.Xi;
    auto zplane = [&](int k, bool& zok) -> const TIN* {  // source plane of output plane k (clamped to a valid one)
#pragma clang fp contract(off)
        const double c = p.m[0] * (double)(min(k, kb - 1) + p.cz) + p.m[3];
        const bool inside = BOUNDARY == BH_BOUNDARY_ITK ? (c >= -0.5 && c < (double)p.Zi - 0.5) : (c >= 0.0 && c <= (double)(p.Zi - 1));
        int iz = inside ? (int)floor(c + 0.5) : 0;
        zok = inside && (BOUNDARY == BH_BOUNDARY_ITK || (iz >= 0 && iz < p.Zi));
        iz = max(0, min(iz, p.Zi - 1));
        return in + (size_t)iz * sZ;
    };
    auto load_plane = [&](int k, raw_t (&dst)[RY]) {
        bool zok;
        const TIN* pl = zplane(k, zok);
#pragma unroll
        for (int r = 0; r < RY; ++r) dst[r] = issue_one<TIN>(pl, off[r]);
    };
    raw_t ring[DN][RY];
#pragma unroll
    for (int s = 0; s < DN; ++s) load_plane(ka + s, ring[s]);
    for (int k0 = ka; k0 < kb; k0 += DN) {
#pragma unroll
        for (int s = 0; s < DN; ++s) {
            const int k = k0 + s;
            if (k < kb) {
                bool zok;
                zplane(k, zok);
                landed1<(DN - 1) * RY>(ring[s]);
                char* oplane = reinterpret_cast<char*>(out + ((size_t)k * p.Yo + oy0) * p.Xo);
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const float v = (zok && ok[r]) ? widen_one<TIN>(ring[s][r]) : p.cval;
                    if (store[r]) *reinterpret_cast<float*>(oplane + (size_t)r * p.Xo * 4 + here((unsigned)(ox * 4))) = v;
                }
                load_plane(k + DN, ring[s]);
            }
        }
    }
}

template <typename TIN, int INTERP, int BOUNDARY>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void zwalk_kernel(const TIN* __restrict__ in, float* __restrict__ out, AffineParams p,
                                                  int ntx, int nxg, int nty, int zchunk, int per_xcd, int nwg) {
    const int t = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || t >= nwg) return;
    const int zc = t / (nxg * nty), rem = t - zc * (nxg * nty), yg = rem / nxg, xg = rem - yg * nxg;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xt = xg * NWX + wv % NWX;
    if (xt >= ntx) return;
    const int ox = xt * 64 + (threadIdx.x & 63), oy0 = (yg * NWY + wv / NWX) * RY;
    if (oy0 >= p.Yo) return;
    const int ka = zc * zchunk, kb = min(ka + zchunk, p.Zo);
    if (INTERP == BH_INTERP_NEAREST) {
        unsigned off[RY];
        bool ok[RY], store[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int oy = oy0 + r;
            store[r] = ox < p.Xo && oy < p.Yo;
            bool inside;
            int iy = 0, ix = 0;
            {
#pragma clang fp contract(off)
                const double yd = (double)(oy + p.cy), xd = (double)(ox + p.cx);
                const double cy = (p.m[5] * yd + p.m[6] * xd) + p.m[7], cx = (p.m[9] * yd + p.m[10] * xd) + p.m[11];
                if (BOUNDARY == BH_BOUNDARY_ITK)
                    inside = cy >= -0.5 && cy < (double)p.Yi - 0.5 && cx >= -0.5 && cx < (double)p.Xi - 0.5;
                else
                    inside = cy >= 0.0 && cy <= (double)(p.Yi - 1) && cx >= 0.0 && cx <= (double)(p.Xi - 1);
                if (inside) {
                    iy = (int)floor(cy + 0.5);
                    ix = (int)floor(cx + 0.5);
                }
            }
            ok[r] = inside && (BOUNDARY == BH_BOUNDARY_ITK || (iy >= 0 && iy < p.Yi && ix >= 0 && ix < p.Xi));
            iy = max(0, min(iy, p.Yi - 1));
            ix = max(0, min(ix, p.Xi - 1));
            off[r] = ((unsigned)iy * (unsigned)p.Xi + (unsigned)ix) * (unsigned)sizeof(TIN);
        }
        walk_nearest<TIN, BOUNDARY>(in, out, p, off, ok, store, ox, oy0, ka, kb);
        return;
    }
    Rows R;
    bool edge = false;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int oy = oy0 + r;
        R.store[r] = ox < p.Xo && oy < p.Yo;
        const long long cyq = p.mq[5] * (long long)(oy + p.cy) + p.mq[6] * (long long)(ox + p.cx) + p.mq[7];
        const long long cxq = p.mq[9] * (long long)(oy + p.cy) + p.mq[10] * (long long)(ox + p.cx) + p.mq[11];
        const int iy = (int)(cyq >> 32), ix = (int)(cxq >> 32);
        R.fy[r] = (float)(unsigned)cyq * 2.3283064365386963e-10f;  // the Q0.32 fractions, as lerp8 widens them
        R.fx[r] = (float)(unsigned)cxq * 2.3283064365386963e-10f;
        const int y0 = max(0, min(iy, p.Yi - 1)), y1 = max(0, min(iy + 1, p.Yi - 1));
        const int xb = max(0, min(ix, p.Xi - 2));
        R.sel[r] = ix < 0 ? 1 : (ix >= p.Xi - 1 ? 2 : 0);
        edge = edge || R.sel[r] != 0;
        R.off0[r] = ((unsigned)y0 * (unsigned)p.Xi + (unsigned)xb) * (unsigned)sizeof(TIN);
        R.off1[r] = ((unsigned)y1 * (unsigned)p.Xi + (unsigned)xb) * (unsigned)sizeof(TIN);
        bool inside = true;
        {  // the float64 decision of the staged-tile kernel's boundary loop (m[4], m[8] are exact zeros here)
#pragma clang fp contract(off)
            const double yd = (double)(oy + p.cy), xd = (double)(ox + p.cx);
            const double cy = (p.m[5] * yd + p.m[6] * xd) + p.m[7], cx = (p.m[9] * yd + p.m[10] * xd) + p.m[11];
            if (BOUNDARY == BH_BOUNDARY_ITK)
                inside = cy >= -0.5 && cy < (double)p.Yi - 0.5 && cx >= -0.5 && cx < (double)p.Xi - 0.5;
            else
                inside = cy >= 0.0 && cy <= (double)(p.Yi - 1) && cx >= 0.0 && cx <= (double)(p.Xi - 1);
        }
        R.inside[r] = inside;
    }
    if (__builtin_amdgcn_ballot_w64(edge) != 0ull) {
        walk<TIN, BOUNDARY, true>(in, out, p, R, ox, oy0, ka, kb);
        return;
    }
    if ((sizeof(TIN) == 4 || sizeof(TIN) == 2) && p.zslot > 0) {
        constexpr int E = 16 / (int)sizeof(TIN);  // samples per 16-B quad
        // Source box of the wave's 64 x RY outputs (exact: the Q32.32 coordinates are affine, extremes sit at the corners);
        // the LDS ring takes it when it lies inside the volume and fits a slot.
        const int ox0 = xt * 64;
        long long ylo = 0, yhi = 0, xlo = 0, xhi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long oyc = oy0 + ((c & 1) ? RY - 1 : 0) + p.cy, oxc = ox0 + ((c & 2) ? 63 : 0) + p.cx;
            const long long cyq = p.mq[5] * oyc + p.mq[6] * oxc + p.mq[7], cxq = p.mq[9] * oyc + p.mq[10] * oxc + p.mq[11];
            ylo = c ? (cyq < ylo ? cyq : ylo) : cyq;
            yhi = c ? (cyq > yhi ? cyq : yhi) : cyq;
            xlo = c ? (cxq < xlo ? cxq : xlo) : cxq;
            xhi = c ? (cxq > xhi ? cxq : xhi) : cxq;
        }
        const int by = (int)(ylo >> 32), y1 = (int)(yhi >> 32) + 1, x0 = (int)(xlo >> 32), x1 = (int)(xhi >> 32) + 1;
        if (by >= 0 && y1 <= p.Yi - 1 && x0 >= 0 && x1 <= p.Xi - 1) {
            // whole quads (Xi % E == 0 keeps them in the row)
            const int bxq = x0 & ~(E - 1), dx = ((x1 + E) & ~(E - 1)) - bxq, dy = y1 - by + 1;
            const unsigned L = (unsigned)dx / (unsigned)E, S = (unsigned)dy * L;
            if (S * 16u <= (unsigned)p.zslot) {
                LdsBox B;
                B.on = 1;
                B.S = S;
                B.nq = (int)((S + 63u) >> 6);
                B.pitch = (unsigned)dx * (unsigned)sizeof(TIN);
                B.slot_bytes = (unsigned)p.zslot;
                B.slot0 = (unsigned)wv * (unsigned)(NSLOT * p.zslot);
#pragma unroll
                for (int i = 0; i < QMAX; ++i) {
                    const unsigned q = min((unsigned)(i * 64 + (threadIdx.x & 63)), S - 1u);
                    const unsigned row = q / L, xq = q - row * L;
                    B.doff[i] = (((unsigned)(by + (int)row) * (unsigned)p.Xi + (unsigned)bxq) + (unsigned)E * xq) * (unsigned)sizeof(TIN);
                }
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const long long cyq = p.mq[5] * (long long)(oy0 + r + p.cy) + p.mq[6] * (long long)(ox + p.cx) + p.mq[7];
                    const long long cxq = p.mq[9] * (long long)(oy0 + r + p.cy) + p.mq[10] * (long long)(ox + p.cx) + p.mq[11];
                    // lanes past the output's last column stay inside the box (their results are never stored)
                    const int iy = min(max((int)(cyq >> 32), by), y1 - 1), ix = min(max((int)(cxq >> 32), bxq), bxq + dx - 2);
                    B.loff[r] = (unsigned)((iy - by) * dx + (ix - bxq)) * (unsigned)sizeof(TIN);
                }
                walk<TIN, BOUNDARY, false, true>(in, out, p, R, ox, oy0, ka, kb, B);
                return;
            }
        }
    }
    walk<TIN, BOUNDARY, false>(in, out, p, R, ox, oy0, ka, kb);
}

// the matrices this kernel takes: exact zeros couple z with (y, x) in neither direction, z scale >= 0, planes addressable
// with 32-bit byte offsets
static bool takes(const AffineParams& p) {
    const bool zeros = p.m[1] == 0.0 && p.m[2] == 0.0 && p.m[4] == 0.0 && p.m[8] == 0.0 && p.mq[0] >= 0;
    return zeros && p.boundary != BH_BOUNDARY_ZEROS && p.Xi >= 2 &&
           (int64_t)p.Yi * p.Xi * 4 < (1ll << 32) - 16 && (int64_t)p.Xo * 4 < (1ll << 31) &&
           getenv("BH_AFFINE_NOZWALK") == nullptr;
}

template <typename TIN>
static int launch(bh_ctx* ctx, const TIN* in, float* out, const AffineParams& p) {
    const int64_t ntx = ceil_div(p.Xo, 64), nxg = ceil_div(ntx, NWX), nty = ceil_div(p.Yo, RY * NWY);
    // enough z chunks for ~64 K waves (16 rounds of the chip), none shorter than 32 planes (each chunk re-reads D + 2)
    const char* we = getenv("BH_ZW_WAVES");
    int64_t nchunk = std::min<int64_t>(ceil_div(we ? atoi(we) : 65536, ntx * nty * NWY), ceil_div(p.Zo, 32));
    nchunk = std::max<int64_t>(nchunk, 1);
    const int64_t zchunk = ceil_div(p.Zo, nchunk);
    nchunk = ceil_div(p.Zo, zchunk);
    const int64_t nwg = nxg * nty * nchunk;
    BH_REQUIRE(nwg < (1ll << 31) - 8, "affine output too large");
    const int per_xcd = (int)ceil_div(nwg, (int64_t)8);
    auto run = [&](auto kern) -> int {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(NT), (size_t)NW * NSLOT * p.zslot, ctx->stream, in, out, p, (int)ntx, (int)nxg, (int)nty,
                           (int)zchunk, per_xcd, (int)nwg);
        BH_CHECK_HIP(hipGetLastError());
        return BH_OK;
    };
    if (p.interp == BH_INTERP_NEAREST) {
        if (p.boundary == BH_BOUNDARY_ITK) return run(zwalk_kernel<TIN, BH_INTERP_NEAREST, BH_BOUNDARY_ITK>);
        return run(zwalk_kernel<TIN, BH_INTERP_NEAREST, BH_BOUNDARY_SCIPY_CONSTANT>);
    }
    if (p.boundary == BH_BOUNDARY_ITK) return run(zwalk_kernel<TIN, BH_INTERP_LINEAR, BH_BOUNDARY_ITK>);
    return run(zwalk_kernel<TIN, BH_INTERP_LINEAR, BH_BOUNDARY_SCIPY_CONSTANT>);
}

}  // namespace zw
