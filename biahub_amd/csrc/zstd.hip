// Zstandard decompression of Blosc-1 blocks on gfx950: the read side of iohub stores, whose chunks are Blosc frames with zstd
// inside (level 1, bit shuffle; reference biahub/deskew.py:608-640).  c-blosc compresses every block (or split) with one
// ZSTD_compressCCtx call, so each stream is one complete zstd frame (RFC 8878) with its content size in the header, and a
// volume holds thousands of them: one wavefront decodes one frame, persistent wavefronts stride over the streams.
//
// Inside a frame (zstd_frame.inc, zstd_block.inc): lane 0 parses headers and table descriptions and decodes the sequence
// bitstream into an LDS batch of up to 128 sequences; Huffman literals are decoded one lane per stream (1 or 4) into a
// per-wave global scratch of one block (128 KiB); then all 64 lanes copy the batch's literals (a running sum of LL and ML gives
// every output position) and run its matches in order, reading the frame's own output back from global memory after waiting
// for this wave's stores.  Every lane hand-off through LDS goes through a wavefront fence and barrier.
// The decoder is compiled twice, under the two macro sets of zstd_lanes.inc: for the wavefront (the kernel below) and with one
// lane for the host (bh_host_zstd_decompress: no GPU, for tests and debugging only).
#include "common.hpp"

#include <cstring>
#include <vector>

namespace bh {
namespace zstd {

namespace dev {
#define ZS_TARGET_DEVICE
#include "zstd_lanes.inc"
#include "zstd_frame.inc"
#define ZS_TARGET_END
#include "zstd_lanes.inc"
}  // namespace dev

namespace host {
#define ZS_TARGET_HOST
#include "zstd_lanes.inc"
#include "zstd_frame.inc"
#define ZS_TARGET_END
#include "zstd_lanes.inc"
}  // namespace host

constexpr int WAVES = 4;  // wavefronts per workgroup; 4 x sizeof(dev::zs::Lds) of static LDS

__global__ __launch_bounds__(64 * WAVES) void decompress_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ soff,
                                                               const uint32_t* __restrict__ csize, const uint64_t* __restrict__ doff,
                                                               const uint32_t* __restrict__ dlen, uint32_t nstreams,
                                                               uint8_t* __restrict__ dst, uint8_t* __restrict__ scratch,
                                                               unsigned* __restrict__ status) {
    __shared__ dev::zs::Lds lds[WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    dev::zs::Lds* L = &lds[wave];
    uint8_t* lit = scratch + (uint64_t)(blockIdx.x * WAVES + wave) * dev::zs::LIT_SCRATCH;
    for (uint32_t b = blockIdx.x * WAVES + wave; b < nstreams; b += gridDim.x * WAVES) {
        const uint8_t* in = src + soff[b];
        const uint32_t cs = csize[b], n = dlen[b];
        uint8_t* out = dst + doff[b];
        if (cs == n) {  // a block c-blosc stored raw
            for (uint32_t j = lane; j < n; j += 64) out[j] = in[j];
            continue;
        }
        if (!dev::zs::decode_frame(in, cs, out, n, lit, L) && lane == 0) atomicMin(status, b);
    }
}

}  // namespace zstd
}  // namespace bh

extern "C" {

// zstd frames back to bytes on the device: stream i = csize[i] bytes at src + soff[i] -> dlen[i] bytes at dst + doff[i] (four
// device arrays of nstreams entries; csize == dlen marks a stored stream).  Synchronises; BH_ERR_INVALID names the first
// corrupt stream.
int bh_zstd_decompress_streams(bh_ctx* ctx, const void* src, const uint64_t* soff, const uint32_t* csize, const uint64_t* doff,
                               const uint32_t* dlen, uint32_t nstreams, void* dst) {
    using namespace bh;
    BH_REQUIRE(ctx && src && soff && csize && doff && dlen && dst, "NULL argument");
    BH_REQUIRE(nstreams > 0, "no streams");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const int grid = wave_grid(ctx, nstreams, zstd::WAVES);
    unsigned* status;
    uint8_t* scratch;
    BH_TRY(get_scratch(ctx, "zstd_status", sizeof(unsigned), (void**)&status));
    BH_TRY(get_scratch(ctx, "zstd_literals", (uint64_t)grid * zstd::WAVES * zstd::dev::zs::LIT_SCRATCH, (void**)&scratch));
    hipStream_t s = ctx->stream;
    BH_CHECK_HIP(hipMemsetAsync(status, 0xff, sizeof(unsigned), s));
    hipLaunchKernelGGL(zstd::decompress_kernel, dim3(grid), dim3(64 * zstd::WAVES), 0, s, (const uint8_t*)src, soff, csize, doff, dlen,
                       nstreams, (uint8_t*)dst, scratch, status);
    BH_CHECK_HIP(hipGetLastError());
    unsigned h = 0;
    BH_CHECK_HIP(hipMemcpyAsync(&h, status, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    BH_CHECK_HIP(hipStreamSynchronize(s));
    BH_REQUIRE(h == 0xffffffffu, "corrupt zstd stream %u", h);
    return BH_OK;
}

// The decoder on the host (no GPU, no context), one stream under the device entry's contract: src[0, csize) -> dst[0, n).
// csize == n: a stored stream; else one complete frame of exactly n bytes.  BH_ERR_INVALID on a corrupt frame.
int bh_host_zstd_decompress(const void* src, uint64_t csize, void* dst, uint64_t n) {
    using namespace bh;
    namespace zs = zstd::host::zs;
    BH_REQUIRE(src && dst, "NULL argument");
    BH_REQUIRE(csize < (1ull << 31) && n < (1ull << 31), "invalid length");
    if (csize == n) {
        std::memcpy(dst, src, n);
        return BH_OK;
    }
    std::vector<zs::Lds> lds(1);
    std::vector<uint8_t> lit(zs::LIT_SCRATCH);
    BH_REQUIRE(zs::decode_frame((const uint8_t*)src, (uint32_t)csize, (uint8_t*)dst, (uint32_t)n, lit.data(), &lds[0]), "corrupt zstd stream");
    return BH_OK;
}

}  // extern "C"
