// Zstandard compression of Blosc-1 blocks on gfx950: the write side of iohub stores, whose chunks are Blosc frames with zstd
// inside (level 1, bit shuffle; reference biahub/deskew.py:608-640).  csrc/zstd.hip reads them on the device; here they are
// written there, so a device-resident volume crosses PCIe compressed in the store's DEFAULT format (csrc/lz4.hip does the same
// for stores opted into the lz4 inner codec).
//
// One wavefront encodes one Blosc block (256 KiB of already permuted bytes) as one complete zstd frame — what c-blosc's
// ZSTD_compressCCtx call per block gives: single segment, content size recorded, no checksum — persistent wavefronts stride
// over the blocks, and the frames are assembled by the codec-independent kernels of csrc/blosc_frame.hpp.  The encoder itself
// is csrc/zstd_enc.inc, compiled twice: for the wavefront (lane 0 runs what is serial, all 64 lanes what is wide) and, with
// one-lane macros, for the host (bh_host_zstd_compress), which the CPU tests hold to libzstd.
#include "blosc_frame.hpp"

#include <cstring>
#include <vector>

namespace bh {
namespace zstd_enc {

namespace dev {

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
#define ZSE_DEVICE 1

// this wave's earlier global stores have landed (the literal scratch is read back by other lanes)
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

#include "zstd_enc.inc"

#undef ZS_FN
#undef ZS_CONST
#undef ZS_LANE_DECL
#undef ZS_SERIAL
#undef ZS_WIDTH
#undef ZS_SYNC
#undef ZSE_DEVICE

}  // namespace dev

namespace host {

#define ZS_FN
#define ZS_CONST static const
#define ZS_LANE_DECL const uint32_t lane = 0
#define ZS_SERIAL if (lane == 0)
#define ZS_WIDTH 1u
#define ZS_SYNC() \
    do {          \
    } while (0)

static inline void zs_wait_own_stores() {}
static inline uint8_t zs_load_own(const uint8_t* p) { return *p; }
static inline uint32_t zs_scan_excl(uint32_t v, uint32_t* total) {
    *total = v;
    return 0;
}
static inline void zs_atomic_or(uint32_t* p, uint32_t v) { *p |= v; }
static inline void zs_atomic_inc(uint32_t* p) { ++*p; }

#include "zstd_enc.inc"

#undef ZS_FN
#undef ZS_CONST
#undef ZS_LANE_DECL
#undef ZS_SERIAL
#undef ZS_WIDTH
#undef ZS_SYNC

}  // namespace host

constexpr int WAVES = 4;  // wavefronts per workgroup; 4 x sizeof(zse::Work) of dynamic LDS (66 KiB: two workgroups per CU)
constexpr size_t LDS_BYTES = WAVES * sizeof(dev::zse::Work);
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups' records exceed the CU's LDS");

// sizes[b] = bytes of block b's zstd frame at dst + b * slot (== the block's length when the frame is not smaller: the block is
// then copied raw, the Blosc container's mark for a stored block).  Block numbering as in lz4::compress_kernel.
__global__ __launch_bounds__(64 * WAVES) void compress_kernel(const uint8_t* __restrict__ src, uint32_t cbytes, uint32_t nb, uint32_t blocksize,
                                                             uint8_t* __restrict__ dst, uint64_t slot, uint32_t* __restrict__ sizes,
                                                             uint32_t nblocks, uint8_t* __restrict__ lits_all, uint64_t* __restrict__ seqs_all) {
    extern __shared__ __attribute__((aligned(16))) uint8_t work_lds[];
    dev::zse::Work* work = reinterpret_cast<dev::zse::Work*>(work_lds);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    dev::zse::Work* W = &work[wave];
    const uint64_t wid = (uint64_t)blockIdx.x * WAVES + wave;
    uint8_t* lits = lits_all + wid * dev::zse::BLOCK_MAX;
    uint64_t* seqs = seqs_all + wid * dev::zse::MAXSEQ;
    for (uint32_t b = blockIdx.x * WAVES + wave; b < nblocks; b += gridDim.x * WAVES) {
        const uint32_t fr = b / nb, jb = b - fr * nb;
        const uint8_t* in = src + (uint64_t)fr * cbytes + (uint64_t)jb * blocksize;
        const uint32_t n = min(blocksize, cbytes - jb * blocksize);  // (jb * blocksize < cbytes < 2^32)
        uint8_t* out = dst + (uint64_t)b * slot;
        uint32_t cs = dev::zse::encode_frame(in, n, out, lits, seqs, W);
        if (cs >= n) {  // stored block
            blosc_frame::wave_copy(out, in, n, lane);
            cs = n;
        }
        if (lane == 0) sizes[b] = cs;
    }
}

// the slot of one block: every byte a frame of `blocksize` bytes may write (zse::frame_bound, derived in zstd_enc.inc), which
// also holds the block stored raw
static uint64_t slot_bytes(uint32_t blocksize) { return (dev::zse::frame_bound(blocksize) + 15) & ~(uint64_t)15; }

}  // namespace zstd_enc
}  // namespace bh

extern "C" {

// Upper bound of the packed frames.  A block never takes more than its own length in a frame (a zstd frame that is not smaller
// is replaced by the raw bytes), so a frame is at most 16 (header) + nb * (4 (start) + 4 (size)) + cbytes bytes, rounded up to
// the 16-byte alignment of the next frame: the same bound as the lz4 writer's.
uint64_t bh_blosc_zstd_bound(uint32_t nframes, uint32_t cbytes, uint32_t blocksize) {
    const uint64_t nb = (cbytes + (uint64_t)blocksize - 1) / blocksize;
    return (uint64_t)nframes * ((16 + 8 * nb + cbytes + 15) & ~(uint64_t)15);
}

// src: nframes * cbytes permuted bytes (chunks back to back); out: packed Blosc frames (inner codec zstd); foff (device,
// nframes + 1 uint64): the frames' offsets in `out` and the total.  out must hold bh_blosc_zstd_bound(nframes, cbytes, blocksize).
int bh_blosc_zstd_compress(bh_ctx* ctx, const void* src, uint32_t nframes, uint32_t cbytes, uint32_t blocksize, uint32_t typesize,
                           int shuffle_mode, void* out, uint64_t* foff) {
    using namespace bh;
    BH_REQUIRE(ctx && src && out && foff, "NULL argument");
    BH_REQUIRE(nframes > 0 && cbytes >= 128 && blocksize >= 128 && blocksize <= (1u << 30), "invalid frame geometry");
    BH_REQUIRE(typesize >= 1 && typesize <= 255, "invalid typesize %u", typesize);
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const uint32_t nb = (uint32_t)(((uint64_t)cbytes + blocksize - 1) / blocksize);
    BH_REQUIRE((uint64_t)nframes * nb < (1ull << 31), "too many blocks");
    const uint32_t nblocks = nframes * nb;
    const uint64_t slot = zstd_enc::slot_bytes(blocksize);
    const int grid = (int)std::min<uint64_t>(((uint64_t)nblocks + zstd_enc::WAVES - 1) / zstd_enc::WAVES, (uint64_t)ctx->num_cus * 2);
    uint8_t *slots, *lits;
    uint64_t* seqs;
    uint32_t *sizes, *bstarts, *fbytes;
    BH_TRY(get_scratch(ctx, "zstd_enc_slots", (uint64_t)nblocks * slot, (void**)&slots));
    BH_TRY(get_scratch(ctx, "zstd_enc_sizes", (uint64_t)nblocks * 4, (void**)&sizes));
    BH_TRY(get_scratch(ctx, "zstd_enc_bstarts", (uint64_t)nblocks * 4, (void**)&bstarts));
    BH_TRY(get_scratch(ctx, "zstd_enc_fbytes", (uint64_t)nframes * 4, (void**)&fbytes));
    // per wave of the grid: the literals and the sequences of one zstd block
    BH_TRY(get_scratch(ctx, "zstd_enc_literals", (uint64_t)grid * zstd_enc::WAVES * zstd_enc::dev::zse::BLOCK_MAX, (void**)&lits));
    BH_TRY(get_scratch(ctx, "zstd_enc_sequences", (uint64_t)grid * zstd_enc::WAVES * zstd_enc::dev::zse::MAXSEQ * 8, (void**)&seqs));
    hipStream_t s = ctx->stream;
    BH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(zstd_enc::compress_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)zstd_enc::LDS_BYTES));
    hipLaunchKernelGGL(zstd_enc::compress_kernel, dim3(grid), dim3(64 * zstd_enc::WAVES), zstd_enc::LDS_BYTES, s, (const uint8_t*)src, cbytes, nb, blocksize, slots,
                       slot, sizes, nblocks, lits, seqs);
    // flags: blocks never split, inner codec zstd (4), the permutation the caller applied
    const uint32_t flags = 0x10u | (4u << 5) | (shuffle_mode == BH_BLOSC_SHUFFLE ? 0x1u : (shuffle_mode == BH_BLOSC_BITSHUFFLE ? 0x4u : 0u));
    blosc_frame::launch_frame_assembly(s, slots, slot, sizes, bstarts, fbytes, nb, nframes, cbytes, blocksize, typesize, flags, (uint8_t*)out, foff);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

// The encoder on the host (no GPU, no context): src[0, n) -> one zstd frame in dst[0, *csize), or — when the frame would not
// be smaller than n — the n bytes themselves (*csize == n, the container's mark for a stored block).  cap >= n.
int bh_host_zstd_compress(const void* src, uint64_t n, void* dst, uint64_t cap, uint64_t* csize) {
    using namespace bh;
    namespace zse = zstd_enc::host::zse;
    BH_REQUIRE(src && dst && csize, "NULL argument");
    BH_REQUIRE(n >= 1 && n <= (1u << 30), "invalid length");
    BH_REQUIRE(cap >= n, "the destination holds fewer than n bytes");
    std::vector<uint8_t> frame(zse::frame_bound(n)), lits(zse::BLOCK_MAX);
    std::vector<uint64_t> seqs(zse::MAXSEQ);
    std::vector<zse::Work> work(1);
    const uint32_t cs = zse::encode_frame((const uint8_t*)src, (uint32_t)n, frame.data(), lits.data(), seqs.data(), &work[0]);
    if (cs >= n) {
        std::memcpy(dst, src, n);
        *csize = n;
    } else {
        std::memcpy(dst, frame.data(), cs);
        *csize = cs;
    }
    return BH_OK;
}

}  // extern "C"
