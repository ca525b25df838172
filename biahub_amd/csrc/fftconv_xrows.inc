// The row-pair frame of the wave-private X passes — included by fftconv_xw.hip after fftconv_regfft.inc and ahead of
// fftconv_xw.inc (rows of 512 / 1024 / 2048 voxels) and fftconv_x3.inc (rows of 1536 / 3072), which both build their kernels
// on it: what a mode means, which rows a pair reads and writes (the z wrap geometry and the mirrored source plane included),
// the address of a lane's access in a row, and Richardson-Lucy's value step on one access.  Nothing here asks which family is
// calling.
//
// A family file brings its geometry, index maps, LDS address plan, register stages, untangle, tables and the kernel skeleton:
// the loop over row pairs, where the prefetches sit, and the loads and stores themselves.  The stores of the real-side
// epilogue (cropped store, wrap extension along x, the FWD prologue) and of the spectrum row also stay written out in each
// family: the two write the same steps over different index expressions (16-B accesses at 2 r BLK + 4 l against 8-B accesses
// at 2 (t L + rho BLK + l)), the compiler's address folding and schedule follow the written expression tree, and one generic
// text over a layout description compiled to different instruction counts in one family or the other
// (profiles/xrows_refactor_isa.txt).  A change to one of those steps is made in both files.
namespace xw {

// ---- what a mode means ----
template <int MODE>
struct ModeOf {
    static constexpr bool WRAP = MODE == FUSED_RATIO_WRAP || MODE == FUSED_UPDATE_WRAP;  // fftconv_richardson_lucy_wrap
    static constexpr bool HAS_INV = MODE != FWD;
    static constexpr bool HAS_FWD = MODE == FWD || MODE == FUSED_RATIO || MODE == FUSED_UPDATE || WRAP;
    static constexpr bool RATIO = MODE == INV_RATIO || MODE == FUSED_RATIO || MODE == FUSED_RATIO_WRAP;
    static constexpr bool CROP = MODE == INV_UPDATE_CROP;  // the last update, stored straight into the unpadded output volume
    static constexpr bool UPDATE = MODE == INV_UPDATE || MODE == FUSED_UPDATE || MODE == FUSED_UPDATE_WRAP || CROP;
    static constexpr bool ARGMAX = MODE == INV_ARGMAX;  // fftconv_xw.inc only: the mode table of x3_kernel has no such case
    static constexpr bool STORE_REAL = MODE != FUSED_RATIO && MODE != FUSED_RATIO_WRAP && !ARGMAX;  // the ratio of a fused pass never leaves the chip
};

// ---- the rows of a wavefront's pairs ----
struct Rows {
    long ra, rb;    // first row of the wavefront's pairs (uniform): where results go
    long sa_, sb_;  // the rows read (WRAP: those of the plane this plane mirrors)
    int yy;
    bool zero;      // WRAP: a plane beyond the wrap margins holds zeros
};
template <bool WRAP>
__device__ __forceinline__ Rows rows_of(const Params& p, int pb, int Yh) {
    Rows r;
    const int z = pb / Yh;
    r.yy = pb - z * Yh;
    r.ra = (long)z * p.Y + r.yy;
    r.rb = r.ra + Yh;
    r.sa_ = r.ra;
    r.sb_ = r.rb;
    r.zero = false;
    if (WRAP) {
        int rel = z - p.wz.off;
        if (rel >= p.wz.n + p.wz.mhi) rel -= p.Z;
        r.zero = rel < -p.wz.mlo || rel >= p.wz.n + p.wz.mhi;
        rel += rel < 0 ? p.wz.n : (rel >= p.wz.n ? -p.wz.n : 0);
        const int zs = r.zero ? z : rel + p.wz.off;
        r.sa_ = (long)zs * p.Y + r.yy;
        r.sb_ = r.sa_ + Yh;
    }
    return r;
}

// address of a V (float4 / float2): uniform row base + (the lane's byte offset + a compile-time immediate)
template <typename V>
__device__ __forceinline__ const V* at(const void* base, long row, int pitch_bytes, int lane_off, int imm) {
    return reinterpret_cast<const V*>(static_cast<const unsigned char*>(base) + row * pitch_bytes + (lane_off + imm));
}
template <typename V>
__device__ __forceinline__ V* at_w(void* base, long row, int pitch_bytes, int lane_off, int imm) {
    return reinterpret_cast<V*>(static_cast<unsigned char*>(base) + row * pitch_bytes + (lane_off + imm));
}

// ---- the value step of an inverse pass's epilogue on one access: v = the reals the transform left, aux = d or est there ----
__device__ __forceinline__ void to_arr(const float2& v, float (&a)[2]) { a[0] = v.x, a[1] = v.y; }
__device__ __forceinline__ void to_arr(const float4& v, float (&a)[4]) { a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w; }
__device__ __forceinline__ float2 to_vec(const float (&a)[2]) { return make_float2(a[0], a[1]); }
__device__ __forceinline__ float4 to_vec(const float (&a)[4]) { return make_float4(a[0], a[1], a[2], a[3]); }
template <int MODE, typename V>
__device__ __forceinline__ V value_op(V v, const V& aux, float eps) {
    using MD = ModeOf<MODE>;
    if constexpr (MD::RATIO || MD::UPDATE) {
        constexpr int NV = sizeof(V) / 4;
        float a[NV], o[NV];
        to_arr(v, a);
        to_arr(aux, o);
#pragma unroll
        for (int e = 0; e < NV; ++e) a[e] = MD::RATIO ? rl_ratio(o[e], a[e], eps) : rl_update(o[e], a[e]);
        v = to_vec(a);
    }
    return v;
}

}  // namespace xw
