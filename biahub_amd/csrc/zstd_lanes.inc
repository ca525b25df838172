// The lane vocabulary of the zstd decoder (zstd_frame.inc) and encoder (zstd_enc.inc), which are written once and compiled
// twice: for a wavefront (64 lanes; lane 0 runs what is serial) and for the host (one lane).  Included inside a namespace:
//     #define ZS_TARGET_DEVICE (or ZS_TARGET_HOST), #include "zstd_lanes.inc"  -> the macros and helpers below
//     ... the code written in them ...
//     #define ZS_TARGET_END, #include "zstd_lanes.inc"                          -> the macros are gone again
//   ZS_FN            function qualifier            ZS_CONST   storage of a constant table
//   ZS_LANE_DECL     declares `lane`               ZS_SERIAL  guards what lane 0 alone runs
//   ZS_WIDTH         lanes (stride of wide loops)  ZS_SYNC()  producer -> consumer hand-off through the wave's record
#if defined(ZS_TARGET_END)
#undef ZS_FN
#undef ZS_CONST
#undef ZS_LANE_DECL
#undef ZS_SERIAL
#undef ZS_WIDTH
#undef ZS_SYNC
#undef ZS_TARGET_DEVICE
#undef ZS_TARGET_HOST
#undef ZS_TARGET_END
#elif defined(ZS_TARGET_DEVICE)
#define ZS_FN __device__
#define ZS_CONST __constant__
#define ZS_LANE_DECL const uint32_t lane = threadIdx.x & 63u
#define ZS_SERIAL if (lane == 0)
#define ZS_WIDTH 64u
#define ZS_SYNC()                                              \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

// this wave's earlier global stores have landed (a match or a literal read-back may reach them)
__device__ __forceinline__ void zs_wait_own_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// a byte this wave wrote earlier: read past the vector cache
__device__ __forceinline__ uint8_t zs_load_own(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// exclusive prefix sum of v over the wavefront's lanes (all active); *total: the sum
__device__ __forceinline__ uint32_t zs_scan_excl(uint32_t v, uint32_t* total) {
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += t;
    }
    *total = (uint32_t)__shfl((int)incl, 63, 64);
    return incl - v;
}
__device__ __forceinline__ void zs_atomic_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ void zs_atomic_inc(uint32_t* p) { atomicAdd(p, 1u); }
#elif defined(ZS_TARGET_HOST)
#define ZS_FN
#define ZS_CONST static const
#define ZS_LANE_DECL const uint32_t lane = 0
#define ZS_SERIAL if (lane == 0)
#define ZS_WIDTH 1u
#define ZS_SYNC() ((void)0)
static inline void zs_wait_own_stores() {}
static inline uint8_t zs_load_own(const uint8_t* p) { return *p; }
static inline uint32_t zs_scan_excl(uint32_t v, uint32_t* total) {
    *total = v;
    return 0;
}
static inline void zs_atomic_or(uint32_t* p, uint32_t v) { *p |= v; }
static inline void zs_atomic_inc(uint32_t* p) { ++*p; }
#else
#error "define ZS_TARGET_DEVICE, ZS_TARGET_HOST or ZS_TARGET_END before including zstd_lanes.inc"
#endif
