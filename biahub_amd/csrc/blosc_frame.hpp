// What the device writers of the Blosc-1 container share (csrc/lz4.hip, csrc/zstd_enc.hip): the codec's kernel leaves every
// block's bytes in a slot of its own and its size in `sizes` (== the block's length: stored raw); compress_frames is the whole
// entry around that kernel, three kernels turn slots and sizes into packed frames, and wave_extend is the matchers' wave-wide
// match extension.  Nothing here depends on the inner codec but its number in the `flags` byte.
#pragma once
#include "common.hpp"

#include <string>

namespace bh {
namespace blosc_frame {

__host__ __device__ __forceinline__ unsigned ld32(const uint8_t* p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__host__ __device__ __forceinline__ void st32(uint8_t* p, unsigned v) { __builtin_memcpy(p, &v, 4); }

// Length of the match between in + mp and its candidate in + mc (mc < mp), whose first four bytes are known to be equal, ending
// at or before `limit`: the wavefront compares 256 bytes per step as dwords, a ballot finds the first lane that differs (or
// runs out of range), ctz the byte inside its dword; within four bytes of the limit, bytes.
__device__ __forceinline__ unsigned wave_extend(const uint8_t* in, unsigned mp, unsigned mc, unsigned limit, int lane) {
    unsigned len = 4;
    for (;;) {
        const unsigned q = mp + len + 4 * lane;
        const bool in_range = q + 4 <= limit;
        const unsigned a = in_range ? ld32(in + q) : 0u, c = in_range ? ld32(in + (mc + len + 4 * lane)) : 1u;
        const unsigned x = a ^ c;
        const unsigned long long neq = __ballot(x != 0u || !in_range);
        if (neq == 0ull) {
            len += 256;
            continue;
        }
        const int fl = __builtin_ctzll(neq);
        len += 4 * fl;
        // the lane that stopped the run: a differing byte inside its dword, or the end of the comparable range
        if (mp + len + 4 <= limit) {
            const unsigned xf = (unsigned)__builtin_amdgcn_readlane((int)x, fl);
            len += (unsigned)__builtin_ctz(xf) >> 3;
        } else {
            while (mp + len < limit && in[mp + len] == in[mc + len]) ++len;  // at most three bytes (uniform loop)
        }
        break;
    }
    return len;
}

// copy n bytes (any alignment, non-overlapping), the wavefront together: 256 bytes per step as dwords, the tail by bytes
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, unsigned n, int lane) {
    unsigned i = 0;
    for (; i + 256 <= n; i += 256) st32(dst + i + 4 * lane, ld32(src + i + 4 * lane));
    for (unsigned j = i + lane; j < n; j += 64) dst[j] = src[j];
}

// Blosc-1 frames of `nframes` chunks of `cbytes` permuted bytes each (the last block of a chunk may be short), blocks never
// split (flag 0x10): frame f = 16-byte header, nb block starts, then per block an int32 size and the payload.
//   scan_kernel : one workgroup per frame — block starts (exclusive scan of 4 + size) and the frame's total
//   offsets     : frame f starts at foff[f] (16-byte aligned) in the packed output; foff[nframes] = total bytes
static __global__ __launch_bounds__(256) void frame_scan_kernel(const uint32_t* __restrict__ sizes, uint32_t nb, uint32_t* __restrict__ bstarts,
                                                         uint32_t* __restrict__ fbytes) {
    __shared__ uint32_t part[256];
    const uint32_t f = blockIdx.x;
    const uint32_t* s = sizes + (uint64_t)f * nb;
    uint32_t* bs = bstarts + (uint64_t)f * nb;
    const uint32_t per = (nb + 255) / 256, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    uint32_t acc = 0;
    for (uint32_t b = b0; b < b1; ++b) acc += 4 + s[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 16 + 4 * nb;
        for (int i = 0; i < 256; ++i) {
            const uint32_t t = part[i];
            part[i] = run;
            run += t;
        }
        fbytes[f] = run;
    }
    __syncthreads();
    uint32_t pos = part[threadIdx.x];
    for (uint32_t b = b0; b < b1; ++b) {
        bs[b] = pos;
        pos += 4 + s[b];
    }
}
static __global__ void frame_offsets_kernel(const uint32_t* __restrict__ fbytes, uint32_t nframes, uint64_t* __restrict__ foff) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t run = 0;
        for (uint32_t f = 0; f < nframes; ++f) {
            foff[f] = run;
            run += ((uint64_t)fbytes[f] + 15) & ~(uint64_t)15;
        }
        foff[nframes] = run;
    }
}
// one wavefront per block copies its payload into place; the first wavefront of a frame also writes header and table
static __global__ __launch_bounds__(256) void frame_pack_kernel(const uint8_t* __restrict__ slots, uint64_t slot, const uint32_t* __restrict__ sizes,
                                                         const uint32_t* __restrict__ bstarts, const uint32_t* __restrict__ fbytes,
                                                         const uint64_t* __restrict__ foff, uint32_t nb, uint32_t nframes, uint32_t cbytes,
                                                         uint32_t blocksize, uint32_t typesize, uint32_t flags, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (uint64_t)nframes * nb) return;
    const uint32_t f = (uint32_t)(w / nb), b = (uint32_t)(w - (uint64_t)f * nb);
    uint8_t* fr = out + foff[f];
    if (b == 0) {
        if (lane == 0) {
            fr[0] = 2;  // blosc format version
            fr[1] = 1;  // inner codec format version
            fr[2] = (uint8_t)flags;
            fr[3] = (uint8_t)typesize;
            st32(fr + 4, cbytes);
            st32(fr + 8, min(blocksize, cbytes));  // c-blosc refuses a block size beyond the buffer (a chunk smaller than one block)
            st32(fr + 12, fbytes[f]);
        }
        for (uint32_t j = lane; j < nb; j += 64) st32(fr + 16 + 4 * j, bstarts[(uint64_t)f * nb + j]);
    }
    const uint32_t cs = sizes[w], pos = bstarts[w];
    if (lane == 0) st32(fr + pos, cs);
    wave_copy(fr + pos + 4, slots + w * slot, cs, lane);
}

// sizes / slots of nframes * nb blocks -> packed frames in `out`, their offsets (and the total) in foff; bstarts and fbytes are
// scratch of nframes * nb and nframes words
static inline void launch_frame_assembly(hipStream_t s, const uint8_t* slots, uint64_t slot, const uint32_t* sizes, uint32_t* bstarts,
                                         uint32_t* fbytes, uint32_t nb, uint32_t nframes, uint32_t cbytes, uint32_t blocksize,
                                         uint32_t typesize, uint32_t flags, uint8_t* out, uint64_t* foff) {
    const uint64_t nblocks = (uint64_t)nframes * nb;
    hipLaunchKernelGGL(frame_scan_kernel, dim3(nframes), dim3(256), 0, s, sizes, nb, bstarts, fbytes);
    hipLaunchKernelGGL(frame_offsets_kernel, dim3(1), dim3(64), 0, s, fbytes, nframes, foff);
    hipLaunchKernelGGL(frame_pack_kernel, dim3((unsigned)((nblocks + 3) / 4)), dim3(256), 0, s, slots, slot, sizes, bstarts, fbytes, foff, nb,
                       nframes, cbytes, blocksize, typesize, flags, out);
}

// Upper bound of the packed frames.  A block that does not shrink is stored raw, so a frame is at most 16 (header) + nb * (4
// (start) + 4 (size)) + cbytes bytes, rounded up to the 16-byte alignment of the next frame.
static inline uint64_t bound(uint32_t nframes, uint32_t cbytes, uint32_t blocksize) {
    const uint64_t nb = (cbytes + (uint64_t)blocksize - 1) / blocksize;
    return (uint64_t)nframes * ((16 + 8 * nb + cbytes + 15) & ~(uint64_t)15);
}

// The body of bh_blosc_<codec>_compress.  src: nframes * cbytes permuted bytes (chunks back to back); out: packed Blosc frames,
// bound(...) bytes; foff (device, nframes + 1 uint64): the frames' offsets in `out` and the total.  codec_id: the container's
// number of the inner codec; `prefix` names this codec's scratch blocks (one codec's calls do not resize another's); slot: bytes
// per block.  launch_blocks(slots, slot, sizes, nb, nblocks) launches the codec's kernel over every block and returns a status.
template <class Launch>
static int compress_frames(bh_ctx* ctx, const void* src, uint32_t nframes, uint32_t cbytes, uint32_t blocksize, uint32_t typesize, int shuffle_mode,
                           uint32_t codec_id, const char* prefix, uint64_t slot, Launch launch_blocks, void* out, uint64_t* foff) {
    BH_REQUIRE(ctx && src && out && foff, "NULL argument");
    BH_REQUIRE(nframes > 0 && cbytes >= 128 && blocksize >= 128 && blocksize <= (1u << 30), "invalid frame geometry");
    BH_REQUIRE(typesize >= 1 && typesize <= 255, "invalid typesize %u", typesize);
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const uint32_t nb = (uint32_t)(((uint64_t)cbytes + blocksize - 1) / blocksize);
    BH_REQUIRE((uint64_t)nframes * nb < (1ull << 31), "too many blocks");
    const uint32_t nblocks = nframes * nb;
    const std::string p(prefix);
    uint8_t* slots;
    uint32_t *sizes, *bstarts, *fbytes;
    BH_TRY(get_scratch(ctx, (p + "_slots").c_str(), (uint64_t)nblocks * slot, (void**)&slots));
    BH_TRY(get_scratch(ctx, (p + "_sizes").c_str(), (uint64_t)nblocks * 4, (void**)&sizes));
    BH_TRY(get_scratch(ctx, (p + "_bstarts").c_str(), (uint64_t)nblocks * 4, (void**)&bstarts));
    BH_TRY(get_scratch(ctx, (p + "_fbytes").c_str(), (uint64_t)nframes * 4, (void**)&fbytes));
    BH_TRY(launch_blocks(slots, slot, sizes, nb, nblocks));
    // flags: blocks never split, the inner codec, the permutation the caller applied
    const uint32_t flags = 0x10u | (codec_id << 5) | (shuffle_mode == BH_BLOSC_SHUFFLE ? 0x1u : (shuffle_mode == BH_BLOSC_BITSHUFFLE ? 0x4u : 0u));
    launch_frame_assembly(ctx->stream, slots, slot, sizes, bstarts, fbytes, nb, nframes, cbytes, blocksize, typesize, flags, (uint8_t*)out, foff);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}

}  // namespace blosc_frame
}  // namespace bh
