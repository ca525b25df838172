// Shared host-side plumbing for libbhcore (context, errors, workspace, timing).
#pragma once

#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "bhcore.h"
#include "reduce.hpp"

namespace bh {

void set_error(const char* fmt, ...);

#define BH_CHECK_HIP(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            bh::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                          __LINE__);                                                         \
            return _e == hipErrorOutOfMemory ? BH_ERR_NOMEM : BH_ERR_HIP;                    \
        }                                                                                    \
    } while (0)

#define BH_CHECK_FFT(expr)                                                                   \
    do {                                                                                     \
        hipfftResult _r = (expr);                                                            \
        if (_r != HIPFFT_SUCCESS) {                                                          \
            bh::set_error("%s failed: hipfftResult %d (%s:%d)", #expr, (int)_r, __FILE__,    \
                          __LINE__);                                                         \
            return _r == HIPFFT_ALLOC_FAILED ? BH_ERR_NOMEM : BH_ERR_HIP;                    \
        }                                                                                    \
    } while (0)

#define BH_REQUIRE(cond, ...)              \
    do {                                   \
        if (!(cond)) {                     \
            bh::set_error(__VA_ARGS__);    \
            return BH_ERR_INVALID;         \
        }                                  \
    } while (0)

#define BH_TRY(expr)                 \
    do {                             \
        int _s = (expr);             \
        if (_s != BH_OK) return _s;  \
    } while (0)

enum TimerSlot { T_DESKEW = 0, T_FILL, T_RL_TOTAL, T_TIKHONOV, T_AFFINE, T_CROPFLIP, T_RL_ITER, T_TF, T_FLATFIELD, T_MOMENTS, T_EDGECOST, T_COUNT };

// One hipFFT plan.  `volume`: the 3-D real transform of (n[0], n[1], n[2]) through hipfftMakePlan3d (the entry point the
// self-check of get_plans exists for), `type` R2C or C2R.  Otherwise one hipfftMakePlanMany call, the members in the order of
// its arguments; with `embed`, n is passed as inembed and onembed too (hipFFT reads strides and distances only then).
struct FftDesc {
    bool volume = false;
    int rank = 3;
    int64_t n[3] = {0, 0, 0};
    bool embed = false;
    int64_t istride = 1, idist = 0, ostride = 1, odist = 0;
    hipfftType type = HIPFFT_R2C;
    int64_t batch = 1;
};
// `batch` contiguous images of (n0, n1), real <-> half spectrum of (n0, n1/2+1): type R2C, C2R, D2Z or Z2D
inline FftDesc fft_batched_2d(hipfftType type, int64_t batch, int64_t n0, int64_t n1) {
    const bool forward = type == HIPFFT_R2C || type == HIPFFT_D2Z;
    const int64_t real = n0 * n1, spec = n0 * (n1 / 2 + 1);
    return FftDesc{false, 2, {n0, n1}, false, 1, forward ? real : spec, 1, forward ? spec : real, type, batch};
}

enum { FFT_FWD = 0, FFT_INV = 1, FFT_ZY = 2, FFT_MAX_PLANS = 3 };  // slots of FftPlans::h
// A cached set of up to three plans (build_plans): one work area from dev_alloc shared by all of them (they never run
// concurrently on one stream), auto-allocation off, every handle on the context's stream.  h[] is in the order of the
// descriptions the set was built from, unused slots 0; by convention the forward transform first, its inverse second.
// Volume sets, the 3-D real transform of (Z, Y, X): shapes with a non-power-of-two extent (what reaches the library in
// production: the fused engine in fftconv.hip takes the power-of-two ones) use hipfftPlan3d.  All-power-of-two shapes (only
// here when BH_FFT_BACKEND=hipfft forces it, or beyond the engine's size limits) are decomposed into batched 1-D real
// transforms along x and one strided batched 2-D complex transform over (z, y): rocFFT 1.0.36 (ROCm 7.2) returns wrong 3-D
// real transforms for some power-of-two shapes once 3-D plans of certain other power-of-two shapes exist in the process
// (tools/hipfft_two_plans.cpp; tools/hipfft_plan3d_sweep.cpp: 8 of 131 power-of-two plans wrong, 0 of 319 mixed-radix ones);
// the decomposition is immune (tools/hipfft_separable_probe.cpp) but ~2.5x slower at large sizes.
struct FftPlans {
    bool separable = false;  // volume sets: the decomposed triple (volume_descs in context.hip) instead of the 3-D pair
    hipfftHandle h[FFT_MAX_PLANS] = {};
    void* work = nullptr;
    size_t work_bytes = 0;
};
// What a cached set transforms: its family and the family's integers (volume: Z, Y, X; strips and slices: batch, n0, n1).
enum class FftFamily { Volume, StripsF64, SlicesF32 };
using FftKey = std::tuple<FftFamily, int64_t, int64_t, int64_t>;

// Named, grow-only device scratch buffers owned by the context.
struct Scratch {
    void* ptr = nullptr;
    size_t bytes = 0;
};

}  // namespace bh

struct bh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    hipEvent_t ev[2 * bh::T_COUNT] = {};
    bool ev_valid[bh::T_COUNT] = {};
    float ms_override[bh::T_COUNT] = {};
    std::map<bh::FftKey, bh::FftPlans> plans;  // owned by context.hip: cached_plans, destroy_plans, stream_plans
    std::map<std::string, bh::Scratch> scratch;
    int num_cus = 256;
    int deskew_path = 0;     // how the last bh_deskew filled the overhang: 0 mask pipeline (or no fill), 1 one-pass (deskew_rows.inc)
    int affine_path = -1;    // the launch of the last bh_affine: 0 staged tiles, 1 compact blocks, 2 z walk, 3 oblique walk, 4 cubic
    // the launches of the last cubic bh_affine (or bh_spline_prefilter alone: bit 128 only), -1 like affine_path: 1 global gather,
    // 2 tiles of 8 planes, 4 tiles of 4 planes; for tiles 8 plane combining (ZUNI), 16 quad staging, 32 pitch of 32 words, 64 512
    // threads; 128 the x pass's VEC form
    int spline_path = -1;
    int plans_replaced = 0;  // 3-D library plans that failed their self-check and were rebuilt decomposed (context.hip)
    // One-shot Richardson-Lucy on the engine box: the handle of the last call, its transfer function in scratch "fc_otf" /
    // "fc_otf_real" (not owned), built from the PSF kept in "rl_psf_kept" (compared byte for byte on every call).  Whoever
    // overwrites or frees that scratch calls rl_oneshot_drop first.
    bh_rl* rl_oneshot = nullptr;
    void* spec_tuned = nullptr;  // the "fc_spec" allocation fftconv_tune_spectrum chose (or accepted) for this context
};

namespace bh {

// grid of a kernel whose persistent wavefronts take one of n items (blocks, streams) at a time, `waves` wavefronts per workgroup
inline int wave_grid(const bh_ctx* ctx, uint64_t n, int waves) {
    return (int)std::min<uint64_t>((n + waves - 1) / waves, (uint64_t)ctx->num_cus * 2);
}
// returns a device buffer of at least `bytes`, cached under `name`
int get_scratch(bh_ctx* ctx, const char* name, size_t bytes, void** out);
int free_scratch(bh_ctx* ctx, const char* name);
// the workspace's allocator (hipMalloc, or the virtual-memory API under BH_ALLOC_VMM_MB: context.hip)
hipError_t dev_alloc(int device, size_t bytes, void** out);
hipError_t dev_free(void* p);
hipError_t dev_alloc_variant(int device, size_t bytes, size_t chunk_bytes, long long seed, void** out);  // survey blocks
bool dev_alloc_is_shuffled();  // the default layout is in force (not switched off by BH_ALLOC_VMM_MB=0)
bool dev_block_is_vmm(const void* p);  // this block was built from mapped chunks (large enough for the layout)
// The set cached under `key`, or built from the n (1 to 3) descriptions and inserted.  All or nothing: on failure nothing is
// left behind, the status is BH_ERR_INVALID (a value that does not fit hipFFT's int), BH_ERR_NOMEM or BH_ERR_HIP, and the
// message names `who` and the transform.
int cached_plans(bh_ctx* ctx, const char* who, const FftKey& key, const FftDesc* descs, int n, FftPlans** out);
int get_plans(bh_ctx* ctx, int64_t Z, int64_t Y, int64_t X, FftPlans** out);
// real (Z,Y,X) -> half spectrum (Z,Y,X/2+1), unnormalised
int fft_forward(const FftPlans* pl, const float* real, float2* spec);
// half spectrum -> real, unnormalised; the spectrum buffer is overwritten
int fft_inverse(const FftPlans* pl, float2* spec, float* real);

struct ScopedTimer {
    bh_ctx* ctx;
    int slot;
    ScopedTimer(bh_ctx* c, int s) : ctx(c), slot(s) {
        if (ctx->timing) {
            ctx->ev_valid[slot] = false;
            (void)hipEventRecord(ctx->ev[2 * slot], ctx->stream);
        }
    }
    ~ScopedTimer() {
        if (ctx->timing) {
            (void)hipEventRecord(ctx->ev[2 * slot + 1], ctx->stream);
            ctx->ev_valid[slot] = true;
        }
    }
};

// One iteration's share of the span it lives through, into ms_override[slot] (read back by bh_last_elapsed_ms): the slot's
// own event pair, so nothing to create, destroy or leak on an error path.  With timing off, or nothing to iterate, it does
// nothing; with timing on its end waits for the stream.
struct ScopedIterTimer {
    bh_ctx* ctx;
    int slot, n;
    ScopedIterTimer(bh_ctx* c, int s, int iterations) : ctx(c), slot(s), n(c->timing ? iterations : 0) {
        if (n > 0) (void)hipEventRecord(ctx->ev[2 * slot], ctx->stream);
    }
    ~ScopedIterTimer() {
        float ms = 0;
        if (n > 0 && hipEventRecord(ctx->ev[2 * slot + 1], ctx->stream) == hipSuccess &&
            hipEventSynchronize(ctx->ev[2 * slot + 1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ctx->ev[2 * slot], ctx->ev[2 * slot + 1]) == hipSuccess)
            ctx->ms_override[slot] = ms / n;
    }
};

// forgets the one-shot Richardson-Lucy handle of the context (deconv.hip): its transfer function's scratch is about to change
void rl_oneshot_drop(bh_ctx* ctx);

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Gigabyte blocks that prepared handles own (staged inverse filters, Richardson-Lucy transfer functions): released blocks are
// kept per (device, size) for the next handle of that size, bh_inverse_filter_trim() returns them to the driver (invtf.hip).
void* filter_pool_take(int device, size_t bytes);
void filter_pool_give(int device, size_t bytes, void* p);

// Device-resident result of the overhang fill's reductions (fill.hip; the one-pass deskew of deskew.hip writes `fill` before
// its resampling kernel starts and raises `fallback` when it meets an exact zero that geometry does not explain).
struct FillStats {
    double sum_all;               // sum of every voxel (zeros contribute nothing)
    double sum_shell;             // sum over dilated & ~zero
    unsigned long long n_masked;  // voxels in the dilated mask
    float fill;                   // value written
    int fallback;                 // one-pass deskew: 1 = a data-dependent zero was seen, the mask pipeline re-runs the volume
};

// |value| and flat index of a running argmax (np.argmax semantics, first_max<float> of reduce.hpp: the FIRST occurrence of the
// maximum wins).  The FFT engine's fused peak search writes these 16 bytes.
using ArgMax = ValIdx<float>;
static_assert(sizeof(ArgMax) == 16 && offsetof(ArgMax, v) == 0 && offsetof(ArgMax, i) == 8, "ArgMax: a float at 0, a long long at 8");

}  // namespace bh
