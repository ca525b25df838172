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
#define ZS_TARGET_DEVICE
#include "zstd_lanes.inc"
#include "zstd_enc.inc"
#define ZS_TARGET_END
#include "zstd_lanes.inc"
}  // namespace dev

namespace host {
#define ZS_TARGET_HOST
#include "zstd_lanes.inc"
#include "zstd_enc.inc"
#define ZS_TARGET_END
#include "zstd_lanes.inc"
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

// The zstd writer's pair of the container: contract in blosc_frame::bound / compress_frames.
uint64_t bh_blosc_zstd_bound(uint32_t nframes, uint32_t cbytes, uint32_t blocksize) { return bh::blosc_frame::bound(nframes, cbytes, blocksize); }

int bh_blosc_zstd_compress(bh_ctx* ctx, const void* src, uint32_t nframes, uint32_t cbytes, uint32_t blocksize, uint32_t typesize,
                           int shuffle_mode, void* out, uint64_t* foff) {
    using namespace bh;
    namespace zse = zstd_enc::dev::zse;
    auto launch = [&](uint8_t* slots, uint64_t slot, uint32_t* sizes, uint32_t nb, uint32_t nblocks) -> int {
        const int grid = wave_grid(ctx, nblocks, zstd_enc::WAVES);
        uint8_t* lits;
        uint64_t* seqs;
        // per wave of the grid: the literals and the sequences of one zstd block
        BH_TRY(get_scratch(ctx, "zstd_enc_literals", (uint64_t)grid * zstd_enc::WAVES * zse::BLOCK_MAX, (void**)&lits));
        BH_TRY(get_scratch(ctx, "zstd_enc_sequences", (uint64_t)grid * zstd_enc::WAVES * zse::MAXSEQ * 8, (void**)&seqs));
        BH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(zstd_enc::compress_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)zstd_enc::LDS_BYTES));
        hipLaunchKernelGGL(zstd_enc::compress_kernel, dim3(grid), dim3(64 * zstd_enc::WAVES), zstd_enc::LDS_BYTES, ctx->stream, (const uint8_t*)src,
                           cbytes, nb, blocksize, slots, slot, sizes, nblocks, lits, seqs);
        return BH_OK;
    };
    return blosc_frame::compress_frames(ctx, src, nframes, cbytes, blocksize, typesize, shuffle_mode, 4, "zstd_enc", zstd_enc::slot_bytes(blocksize), launch,
                                        out, foff);
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
