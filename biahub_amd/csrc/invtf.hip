// apply-inv-tf / compute-tf (BASELINE config 5): the per-volume inverse-transfer-function step and the transfer functions
// it consumes.
//
// Reference boundary: biahub/apply_inverse_transfer_function.py:158-170 submits waveorder's
// `apply_inverse_transfer_function_single_position` per position; biahub/compute_transfer_function.py:16-38 and
// reconstruct.py:27-78 call waveorder's `compute_transfer_function_cli`.  The arithmetic is waveorder 3.0.5's
// (uv.lock:6062-6063), which is NOT in /root/reference: everything below restates its published algorithm as recalled
// (waveorder/models/phase_thick_3d.py, isotropic_fluorescent_thick_3d.py, optics.py, filter.py) — PARITY UNPINNED.
//
//   apply:   out = crop_z( Re ifftn( fftn( pad_z( normalise(x) ) ) * conj(H) / (|H|^2 + reg) ) )
//            Volumes the fused engine takes run as its 5 passes with the filter multiplied inside the Z pass
//            (fftconv_apply_staged_filter; the staged filter may be kept as bfloat16 pairs: COL_CONV16); other shapes
//            run hipFFT R2C -> one pointwise kernel -> C2R.
//   compute: phase (weak-object transfer function of a thick 3-D sample) and fluorescence (|PSF|^2 spectrum) transfer
//            functions from the optical parameters, on hipFFT complex transforms.
#include "common.hpp"
#include "fftconv.hpp"

#include <cstring>
#include <mutex>

namespace bh {

static dim3 grid_for(bh_ctx* ctx, int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    const int64_t cap = (int64_t)ctx->num_cus * 16;
    return dim3((unsigned)(g < 1 ? 1 : (g > cap ? cap : g)));
}

// ------------------------------------------------------------------------------------------------ apply
// sum of a float volume in float64 (per-block partials, fixed-order finish): the mean of inten_normalization_3D
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
    __shared__ double sh[256];
    // 16-B loads, four of them in flight per lane and four independent float64 chains (one 4-B load per trip: 2.3 TB/s)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t n4 = vec ? n >> 2 : 0, stride = (int64_t)gridDim.x * 256;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 u = x4[i], v = x4[i + stride], w = x4[i + 2 * stride], t = x4[i + 3 * stride];
        a0 += ((double)u.x + (double)u.y) + ((double)u.z + (double)u.w);
        a1 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        a2 += ((double)w.x + (double)w.y) + ((double)w.z + (double)w.w);
        a3 += ((double)t.x + (double)t.y) + ((double)t.z + (double)t.w);
    }
    for (; i < n4; i += stride) {
        const float4 u = x4[i];
        a0 += ((double)u.x + (double)u.y) + ((double)u.z + (double)u.w);
    }
    for (int64_t j = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) a1 += (double)x[j];
    const double acc = (a0 + a1) + (a2 + a3);
    const double t = tree_reduce<256>(acc, op_sum(), sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void sum_finish_kernel(double* part, int nblocks, int64_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < nblocks; ++i) t += part[i];
        part[nblocks] = t / (double)n;  // mean
    }
}
// padded[z + pad] = n(x)[z], n(x) = normalise ? x / mean - 1 : x.  The padding planes follow waveorder 3.0.5's
// util.pad_zyx_along_z (recalled; parity unpinned): with z_padding < Z they mirror the volume's own edge planes (plane pad - 1 - z
// below, plane Z - 1 - k for the k-th plane above), otherwise they are constant 0.  UNVERIFIED against waveorder (absent from
// the reference tree): BH_INVTF_ZPAD=zeros restores constant-zero pad planes (the rounds-1-2 behaviour), read per call.
__global__ __launch_bounds__(256) void normalize_pad_kernel(const float* __restrict__ x, float* __restrict__ padded, int64_t nin,
                                                            int64_t plane, int64_t pad, int64_t ntotal,
                                                            const double* __restrict__ mean, int normalize, int mirror_planes) {
    const float inv = normalize ? (float)(1.0 / *mean) : 1.0f;
    const float sub = normalize ? 1.0f : 0.0f;
    const int64_t Z = nin / plane;
    const bool mirror = pad < Z && mirror_planes;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ntotal; i += (int64_t)gridDim.x * 256) {
        const int64_t zp = i / plane, r = i - zp * plane;
        int64_t z = zp - pad;
        bool inside = z >= 0 && z < Z;
        if (!inside && mirror) {
            z = z < 0 ? -1 - z : 2 * Z - 1 - z;
            inside = true;
        }
        padded[i] = inside ? x[z * plane + r] * inv - sub : 0.0f;
    }
}

}  // namespace bh

using namespace bh;

// A prepared inverse filter: the transfer function staged once (engine: the scrambled half-spectrum filter; library: the
// Hermitian part on the (Z', Y, X/2+1) half spectrum), applied to any number of volumes of the same shape — a position's
// time points, a plate's positions.  Staging reads the transfer function twice (k and -k) and is a quarter of a one-shot call.
struct bh_filter {
    int device = 0;
    int64_t Z = 0, Y = 0, X = 0, z_padding = 0;
    bool engine = false, bf16 = false;
    bh::ConvPlan* plan = nullptr;   // engine
    void* filt = nullptr;           // the staged filter
    size_t filt_bytes = 0;
    bool owned = true;              // false: `filt` is the context's scratch (one-shot form), not released with the handle
};

namespace bh {
// Staged filters are gigabytes; hipMalloc / hipFree of such blocks cost hundreds of milliseconds (page-table work) — more
// than reconstructing a position's time points.  Released blocks are therefore kept per (device, size) and handed to the next
// handle of that size: a plate's positions all ask for the same size.  bh_ctx_release_workspace does not touch them;
// they live until the process ends or bh_inverse_filter_trim() is called.
static std::mutex g_filter_pool_mu;
static std::map<std::pair<int, size_t>, std::vector<void*>> g_filter_pool;
void* filter_pool_take(int device, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_filter_pool_mu);
    auto it = g_filter_pool.find({device, bytes});
    if (it == g_filter_pool.end() || it->second.empty()) return nullptr;
    void* p = it->second.back();
    it->second.pop_back();
    return p;
}
void filter_pool_give(int device, size_t bytes, void* p) {
    std::lock_guard<std::mutex> lock(g_filter_pool_mu);
    g_filter_pool[{device, bytes}].push_back(p);
}

// library path: the staged filter is one complex factor per half-spectrum bin (incl. 1/V)
template <bool CPLX>
__global__ void inverse_filter_stage_library_kernel(cf* __restrict__ filt, const void* __restrict__ tf, int64_t Z, int64_t Y,
                                                    int64_t X, float reg, float inv_v) {
    const int64_t Xh = X / 2 + 1, n = Z * Y * Xh;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x = i % Xh, zy = i / Xh, y = zy % Y, z = zy / Y;
        const int64_t mz = z ? Z - z : 0, my = y ? Y - y : 0, mx = x ? X - x : 0;
        cf h, hm;
        if (CPLX) {
            h = reinterpret_cast<const cf*>(tf)[(z * Y + y) * X + x];
            hm = reinterpret_cast<const cf*>(tf)[(mz * Y + my) * X + mx];
        } else {
            h = make_float2(reinterpret_cast<const float*>(tf)[(z * Y + y) * X + x], 0.f);
            hm = make_float2(reinterpret_cast<const float*>(tf)[(mz * Y + my) * X + mx], 0.f);
        }
        const float q = 1.0f / (h.x * h.x + h.y * h.y + reg), qm = 1.0f / (hm.x * hm.x + hm.y * hm.y + reg);
        filt[i] = make_float2(0.5f * (h.x * q + hm.x * qm) * inv_v, 0.5f * (-h.y * q + hm.y * qm) * inv_v);
    }
}
__global__ void cmul_inplace_kernel(cf* __restrict__ spec, const cf* __restrict__ f, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf c = spec[i], g = f[i];
        spec[i] = make_float2(c.x * g.x - c.y * g.y, c.x * g.y + c.y * g.x);
    }
}
}  // namespace bh

static int inverse_filter_create_impl(bh_ctx* ctx, const void* tf, int tf_is_complex, int64_t Z, int64_t Y, int64_t X,
                                      int64_t z_padding, double regularization_strength, int filter_storage, bool use_scratch,
                                      bh_filter** out) {
    BH_REQUIRE(ctx && tf && out, "NULL argument");
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0 && z_padding >= 0, "invalid shape");
    BH_REQUIRE(filter_storage == BH_FILTER_F32 || filter_storage == BH_FILTER_BF16, "filter_storage must be BH_FILTER_F32 or BH_FILTER_BF16");
    BH_REQUIRE(regularization_strength >= 0, "regularization_strength must be >= 0");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const int64_t Zp = Z + 2 * z_padding;
    bh_filter* f = new bh_filter;
    f->device = ctx->device;
    f->Z = Z;
    f->Y = Y;
    f->X = X;
    f->z_padding = z_padding;
    f->bf16 = filter_storage == BH_FILTER_BF16;
    f->engine = fftconv_supported_ex(Zp, Y, X, true) && !(getenv("BH_FFT_BACKEND") && !strcmp(getenv("BH_FFT_BACKEND"), "hipfft"));
    f->owned = !use_scratch;
    auto fail = [&](int rc) {
        if (f->filt && f->owned) filter_pool_give(f->device, f->filt_bytes, f->filt);
        delete f;
        return rc;
    };
    // device memory of the staged filter: the handle's own, or (one-shot form: hipMalloc / hipFree of gigabytes cost far more
    // than the filter pass itself) the context's grow-only scratch
    auto alloc = [&](size_t bytes) -> int {
        f->filt_bytes = bytes;
        if (use_scratch) return get_scratch(ctx, "itf_filter", bytes, &f->filt);
        if ((f->filt = filter_pool_take(ctx->device, bytes)) != nullptr) return BH_OK;
        if (dev_alloc(ctx->device, bytes, &f->filt) != hipSuccess) {
            f->filt = nullptr;
            set_error("out of device memory for the staged inverse filter (%zu bytes)", bytes);
            return BH_ERR_NOMEM;
        }
        return BH_OK;
    };
    if (f->engine) {
        int rc = fftconv_plan(ctx, Zp, Y, X, &f->plan);
        if (rc != BH_OK) return fail(rc);
        const size_t NS = fftconv_spectrum_elems(*f->plan);
        rc = alloc(NS * (f->bf16 ? 4 : sizeof(cf)));
        if (rc != BH_OK) return fail(rc);
        rc = fftconv_stage_inverse_filter(ctx, *f->plan, tf, tf_is_complex != 0, (float)regularization_strength, f->bf16, f->filt);
        if (rc != BH_OK) return fail(rc);
    } else {
        if (f->bf16) {
            set_error("the bfloat16 filter needs a shape the fused FFT engine takes (got %lld x %lld x %lld)", (long long)Zp,
                      (long long)Y, (long long)X);
            return fail(BH_ERR_INVALID);
        }
        const int64_t NS = Zp * Y * (X / 2 + 1);
        const int rc = alloc((size_t)NS * sizeof(cf));
        if (rc != BH_OK) return fail(rc);
        const float inv_v = (float)(1.0 / ((double)Zp * Y * X));
        if (tf_is_complex)
            hipLaunchKernelGGL(inverse_filter_stage_library_kernel<true>, grid_for(ctx, NS), dim3(256), 0, ctx->stream,
                               reinterpret_cast<cf*>(f->filt), tf, Zp, Y, X, (float)regularization_strength, inv_v);
        else
            hipLaunchKernelGGL(inverse_filter_stage_library_kernel<false>, grid_for(ctx, NS), dim3(256), 0, ctx->stream,
                               reinterpret_cast<cf*>(f->filt), tf, Zp, Y, X, (float)regularization_strength, inv_v);
        if (hipGetLastError() != hipSuccess) {
            set_error("inverse filter staging kernel failed to launch");
            return fail(BH_ERR_HIP);
        }
    }
    *out = f;
    return BH_OK;
}

extern "C" int bh_inverse_filter_create(bh_ctx* ctx, const void* tf, int tf_is_complex, int64_t Z, int64_t Y, int64_t X,
                                        int64_t z_padding, double regularization_strength, int filter_storage,
                                        bh_filter** out) {
    return inverse_filter_create_impl(ctx, tf, tf_is_complex, Z, Y, X, z_padding, regularization_strength, filter_storage, false, out);
}

extern "C" int bh_inverse_filter_destroy(bh_filter* f) {
    if (!f) return BH_OK;
    // the block goes back to the pool, not to the driver; work already enqueued on it is ordered before any reuse as long
    // as handles of one device are used on one stream at a time (the contexts of this library are)
    if (f->filt && f->owned) filter_pool_give(f->device, f->filt_bytes, f->filt);
    delete f;
    return BH_OK;
}

extern "C" int bh_inverse_filter_trim(void) {
    std::lock_guard<std::mutex> lock(g_filter_pool_mu);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto& kv : g_filter_pool) {
        (void)hipSetDevice(kv.first.first);
        for (void* p : kv.second) (void)dev_free(p);
    }
    if (prev >= 0) (void)hipSetDevice(prev);  // the caller's device stays current
    g_filter_pool.clear();
    return BH_OK;
}

static int inverse_filter_apply_impl(bh_ctx* ctx, const bh_filter* f, const float* in, int normalize, float* out) {
    hipStream_t s = ctx->stream;
    const int64_t Z = f->Z, Y = f->Y, X = f->X, z_padding = f->z_padding;
    const int64_t Zp = Z + 2 * z_padding, plane = Y * X, V = Z * plane, Vp = Zp * plane;
    const float* src = in;
    float* padded = nullptr;
    double* part = nullptr;
    const int nb = 1024;
    if (normalize) {
        BH_TRY(get_scratch(ctx, "itf_partials", (nb + 1) * sizeof(double), (void**)&part));
        hipLaunchKernelGGL(sum_partials_kernel, dim3(nb), dim3(256), 0, s, in, V, part);
        hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(1), 0, s, part, nb, V);
    }
    // x / mean - 1 rides in the forward X pass when nothing has to be padded and the plan's X passes can take it
    const bool fuse_norm = normalize && z_padding == 0 && f->engine && fftconv_fuses_normalisation(*f->plan);
    const bool staged_input = (normalize != 0 && !fuse_norm) || z_padding != 0;
    if (staged_input) {
        BH_TRY(get_scratch(ctx, "itf_padded", Vp * sizeof(float), (void**)&padded));
        if (!part) BH_TRY(get_scratch(ctx, "itf_partials", (nb + 1) * sizeof(double), (void**)&part));
        const char* zp = getenv("BH_INVTF_ZPAD");
        const int mirror_planes = !(zp && strcmp(zp, "zeros") == 0);
        hipLaunchKernelGGL(normalize_pad_kernel, grid_for(ctx, Vp), dim3(256), 0, s, in, padded, V, plane, z_padding, Vp,
                           (const double*)(part + nb), normalize ? 1 : 0, mirror_planes);
        BH_CHECK_HIP(hipGetLastError());
        src = padded;
    }
    // the transforms write a full padded volume: straight into `out` when there is nothing to crop
    float* dst = z_padding ? padded : out;
    if (f->engine) {
        const size_t NS = fftconv_spectrum_elems(*f->plan);
        cf* spec;
        BH_TRY(get_scratch(ctx, "fc_spec", NS * sizeof(cf), (void**)&spec));
        BH_TRY(fftconv_apply_staged_filter(ctx, *f->plan, src, f->filt, f->bf16, spec, dst, fuse_norm ? part + nb : nullptr));
    } else {
        FftPlans* pl;
        BH_TRY(get_plans(ctx, Zp, Y, X, &pl));
        const int64_t NS = Zp * Y * (X / 2 + 1);
        cf* spec;
        BH_TRY(get_scratch(ctx, "fft_spec", NS * sizeof(cf), (void**)&spec));
        BH_TRY(fft_forward(pl, src, spec));
        hipLaunchKernelGGL(cmul_inplace_kernel, grid_for(ctx, NS), dim3(256), 0, s, spec, reinterpret_cast<const cf*>(f->filt), NS);
        BH_CHECK_HIP(hipGetLastError());
        BH_TRY(fft_inverse(pl, spec, dst));
    }
    if (z_padding)
        BH_CHECK_HIP(hipMemcpyAsync(out, padded + z_padding * plane, V * sizeof(float), hipMemcpyDeviceToDevice, s));
    return BH_OK;
}

extern "C" int bh_inverse_filter_apply(bh_ctx* ctx, const bh_filter* f, const float* in, int normalize, float* out) {
    BH_REQUIRE(ctx && f && in && out, "NULL argument");
    BH_REQUIRE(f->device == ctx->device, "the filter was prepared on device %d, the context is on device %d", f->device, ctx->device);
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    ScopedTimer timer(ctx, T_TIKHONOV);
    return inverse_filter_apply_impl(ctx, f, in, normalize, out);
}

// one-shot form: prepare, apply, release (timed as a whole)
extern "C" int bh_inverse_filter(bh_ctx* ctx, const float* in, const void* tf, int tf_is_complex, int64_t Z, int64_t Y,
                                 int64_t X, int64_t z_padding, double regularization_strength, int normalize,
                                 int filter_storage, float* out) {
    BH_REQUIRE(ctx && in && tf && out, "NULL argument");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    bh_filter* f = nullptr;
    ScopedTimer timer(ctx, T_TIKHONOV);
    BH_TRY(inverse_filter_create_impl(ctx, tf, tf_is_complex, Z, Y, X, z_padding, regularization_strength, filter_storage, true, &f));
    const int rc = inverse_filter_apply_impl(ctx, f, in, normalize, out);
    (void)bh_inverse_filter_destroy(f);  // the staged filter lives in the context's scratch: nothing to free, nothing to wait for
    return rc;
}

// ------------------------------------------------------------------------------------------------ compute
namespace bh {

struct OpticsGeo {
    int Zt, Y, X;            // Zt = Z + 2 z_padding
    double yx_px, z_px;      // pixel sizes
    double inv_lamb;         // 1 / (wavelength / index of refraction)
    double cut_ill, cut_det; // NA / wavelength
    int invert;              // z positions flipped (invert_phase_contrast)
};

// np.fft.fftfreq / torch.fft.fftfreq: k * (1 / (n d)), the reciprocal rounded first (k / (n d) is an ulp off at some k)
__device__ __forceinline__ double fft_freq(int i, int n, double d) {
#pragma clang fp contract(off)
    const double step = 1.0 / ((double)n * d);
    return (double)(i < (n + 1) / 2 ? i : i - n) * step;
}
// Radial frequency of plane bin (y, x), waveorder util.generate_radial_frequencies: sqrt(fy^2 + fx^2) with each square rounded
// on its own, as numpy forms it.  A bin sits inside a pupil when this is < NA / wavelength, and a cut-off may land exactly on
// one of these values: a fused multiply-add (which the compiler forms wherever contraction is allowed, __dmul_rn / __dadd_rn
// included) moves the sum by an ulp at many bins and such a bin to the other side of the comparison — and with it the pupil
// count that scales every bin of the result.  The one helper of every kernel that asks for pupil membership.
__device__ __forceinline__ double radial_freq(int y, int x, int Y, int X, double yx_px) {
#pragma clang fp contract(off)
    const double fy = fft_freq(y, Y, yx_px), fx = fft_freq(x, X, yx_px);
    const double yy = fy * fy, xx = fx * fx;
    return sqrt(yy + xx);
}
// z position of plane zi: ifftshift((arange(Zt) - Zt // 2) * dz), optionally flipped
__device__ __forceinline__ double z_position(int zi, const OpticsGeo& g) {
    if (g.invert) zi = g.Zt - 1 - zi;
    const int c = g.Zt / 2;
    const int k = (zi + c) % g.Zt;  // ifftshift: out[i] = in[(i + n // 2) % n]
    return (double)(k - c) * g.z_px;
}

// A = illumination pupil * propagation kernel, B = detection pupil * Green's function (phase); fluorescence: A = propagation
// kernel only.  waveorder/optics.py: generate_pupil, generate_propagation_kernel, generate_greens_function_z (recalled).
// The phases 2 pi z nu_z reach hundreds of radians: they are formed in float64 (a set-up step, run once per plate).
__global__ __launch_bounds__(256) void optics_planes_kernel(cf* __restrict__ A, cf* __restrict__ B, OpticsGeo g, int phase) {
    const int64_t plane = (int64_t)g.Y * g.X, n = plane * g.Zt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int zi = (int)(i / plane);
        const int64_t r = i - (int64_t)zi * plane;
        const int y = (int)(r / g.X), x = (int)(r - (int64_t)y * g.X);
        const double frr = radial_freq(y, x, g.Y, g.X, g.yx_px);
        const double det = frr < g.cut_det ? 1.0 : 0.0, ill = frr < g.cut_ill ? 1.0 : 0.0;
        const double lamb = 1.0 / g.inv_lamb;
        const double ob = sqrt(fmax(1.0 - lamb * lamb * frr * frr, 0.0) * det) * g.inv_lamb;  // oblique factor
        const double z = z_position(zi, g);
        double sn, cs;
        sincos(6.283185307179586 * z * ob, &sn, &cs);
        if (!phase) {
            A[i] = make_float2((float)(det * cs), (float)(det * sn));
            continue;
        }
        A[i] = make_float2((float)(ill * det * cs), (float)(ill * det * sn));
        // G = -i / (4 pi) * det * exp(i 2 pi |z| ob) / (ob + 1e-15)
        sincos(6.283185307179586 * fabs(z) * ob, &sn, &cs);
        const double k = det / (12.566370614359172 * (ob + 1e-15));
        B[i] = make_float2((float)(det * k * sn), (float)(-det * k * cs));
    }
}
// C = conj(A) * B ; A = A * conj(B)
__global__ void wotf_products_kernel(cf* __restrict__ A, const cf* __restrict__ B, cf* __restrict__ C, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf a = A[i], b = B[i];
        C[i] = make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
        A[i] = make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
    }
}
// v *= window(z) / (Y X)  (the 1/(YX) of the unnormalised inverse 2-D transform); window = ifftshift(hann(Zt, periodic=False))
__global__ void window_kernel(cf* __restrict__ a, cf* __restrict__ c, int Zt, int64_t plane) {
    const int64_t n = plane * Zt;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int zi = (int)(i / plane);
        const int k = (zi + Zt / 2) % Zt;
        const float w = Zt > 1 ? 0.5f - 0.5f * cosf(6.283185307179586f * (float)k / (float)(Zt - 1)) : 1.0f;
        const float s = w / (float)plane;
        cf v = a[i];
        a[i] = make_float2(v.x * s, v.y * s);
        v = c[i];
        c[i] = make_float2(v.x * s, v.y * s);
    }
}
// real = (H1 + H2) f ; imag = i (H1 - H2) f   with H1 = c, H2 = a, f = z_px / direct intensity
__global__ void wotf_combine_kernel(const cf* __restrict__ a, const cf* __restrict__ c, cf* __restrict__ re, cf* __restrict__ im,
                                    int64_t n, float z_px, const unsigned long long* __restrict__ count) {
    const float f = z_px / (float)(*count);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf h1 = c[i], h2 = a[i];
        re[i] = make_float2((h1.x + h2.x) * f, (h1.y + h2.y) * f);
        const cf d = make_float2((h1.x - h2.x) * f, (h1.y - h2.y) * f);
        im[i] = make_float2(-d.y, d.x);
    }
}
// direct intensity = sum(ill * ill * det * conj(det)): the number of pixels inside both pupils
__global__ void pupil_count_kernel(OpticsGeo g, unsigned long long* count) {
    const int64_t plane = (int64_t)g.Y * g.X;
    unsigned long long c = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < plane; r += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(r / g.X), x = (int)(r - (int64_t)y * g.X);
        const double frr = radial_freq(y, x, g.Y, g.X, g.yx_px);
        c += (frr < g.cut_det && frr < g.cut_ill) ? 1ull : 0ull;
    }
    if (c) atomicAdd(count, c);
}
// psf = |a / (Y X)|^2 as a complex array
__global__ void abs2_kernel(cf* __restrict__ a, int64_t n, float inv_plane) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf v = a[i];
        a[i] = make_float2((v.x * v.x + v.y * v.y) * inv_plane * inv_plane, 0.0f);
    }
}
__global__ void absmax_kernel(const cf* __restrict__ a, int64_t n, unsigned int* __restrict__ mx) {
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, sqrtf(a[i].x * a[i].x + a[i].y * a[i].y));
    m = wave_reduce(m, op_max());
    if ((threadIdx.x & 63) == 0) atomicMax(mx, __float_as_uint(m));  // non-negative floats order like their bit patterns
}
__global__ void scale_by_max_kernel(const cf* __restrict__ a, cf* __restrict__ out, int64_t n, const unsigned int* __restrict__ mx) {
    const float inv = 1.0f / __uint_as_float(*mx);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = make_float2(a[i].x * inv, a[i].y * inv);
}

// dst (n) = the low-frequency corners of src (N >= n), both in FFT order: index i < ceil(n/2) stays, the rest maps to the
// top of the source axis (waveorder sampling.nd_fourier_central_cuboid, recalled)
__global__ void central_cuboid_kernel(const cf* __restrict__ src, cf* __restrict__ dst, int64_t NZ, int64_t NY, int64_t NX,
                                      int64_t nz, int64_t ny, int64_t nx) {
    const int64_t n = nz * ny * nx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x = i % nx, zy = i / nx, y = zy % ny, z = zy / ny;
        const int64_t sz = z < (nz + 1) / 2 ? z : NZ - nz + z;
        const int64_t sy = y < (ny + 1) / 2 ? y : NY - ny + y;
        const int64_t sx = x < (nx + 1) / 2 ? x : NX - nx + x;
        dst[i] = src[(sz * NY + sy) * NX + sx];
    }
}

struct C2CPlans {
    hipfftHandle yx = 0, z = 0;
    ~C2CPlans() {
        if (yx) (void)hipfftDestroy(yx);
        if (z) (void)hipfftDestroy(z);
    }
};
static int make_c2c_plans(C2CPlans& pl, int Zt, int Y, int X, hipStream_t s) {
    int n2[2] = {Y, X};
    BH_CHECK_FFT(hipfftPlanMany(&pl.yx, 2, n2, nullptr, 1, Y * X, nullptr, 1, Y * X, HIPFFT_C2C, Zt));
    BH_CHECK_FFT(hipfftSetStream(pl.yx, s));
    int n1[1] = {Zt};
    int embed[1] = {Zt};
    // transforms along z: element stride Y X, one batch entry per (y, x)
    BH_CHECK_FFT(hipfftPlanMany(&pl.z, 1, n1, embed, Y * X, 1, embed, Y * X, 1, HIPFFT_C2C, Y * X));
    BH_CHECK_FFT(hipfftSetStream(pl.z, s));
    return BH_OK;
}

}  // namespace bh

extern "C" int bh_phase_transfer_function_3d(bh_ctx* ctx, int64_t Z, int64_t Y, int64_t X, double yx_pixel_size,
                                             double z_pixel_size, double wavelength_illumination, int64_t z_padding,
                                             double index_of_refraction_media, double numerical_aperture_illumination,
                                             double numerical_aperture_detection, int invert_phase_contrast,
                                             void* real_potential_tf, void* imag_potential_tf) {
    BH_REQUIRE(ctx && real_potential_tf && imag_potential_tf, "NULL argument");
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0 && z_padding >= 0, "invalid shape");
    BH_REQUIRE(yx_pixel_size > 0 && z_pixel_size > 0 && wavelength_illumination > 0 && index_of_refraction_media > 0 &&
                   numerical_aperture_illumination > 0 && numerical_aperture_detection > 0,
               "optical parameters must be positive");
    BH_REQUIRE(Y * X < (1ll << 31) && Z + 2 * z_padding < (1ll << 31), "volume too large for the library transforms");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    OpticsGeo g;
    g.Zt = (int)(Z + 2 * z_padding);
    g.Y = (int)Y;
    g.X = (int)X;
    g.yx_px = yx_pixel_size;
    g.z_px = z_pixel_size;
    g.inv_lamb = index_of_refraction_media / wavelength_illumination;
    g.cut_ill = numerical_aperture_illumination / wavelength_illumination;
    g.cut_det = numerical_aperture_detection / wavelength_illumination;
    g.invert = invert_phase_contrast ? 1 : 0;
    const int64_t n = (int64_t)g.Zt * Y * X;
    cf *A, *B, *C;
    unsigned long long* count;
    BH_TRY(get_scratch(ctx, "optics_a", n * sizeof(cf), (void**)&A));
    BH_TRY(get_scratch(ctx, "optics_b", n * sizeof(cf), (void**)&B));
    BH_TRY(get_scratch(ctx, "optics_c", n * sizeof(cf), (void**)&C));
    BH_TRY(get_scratch(ctx, "optics_count", 64, (void**)&count));
    C2CPlans pl;
    BH_TRY(make_c2c_plans(pl, g.Zt, g.Y, g.X, s));
    BH_CHECK_HIP(hipMemsetAsync(count, 0, 64, s));
    hipLaunchKernelGGL(pupil_count_kernel, grid_for(ctx, Y * X), dim3(256), 0, s, g, count);
    hipLaunchKernelGGL(optics_planes_kernel, grid_for(ctx, n), dim3(256), 0, s, A, B, g, 1);
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, A, A, HIPFFT_FORWARD));   // SPHz_hat
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, B, B, HIPFFT_FORWARD));   // PG_hat
    hipLaunchKernelGGL(wotf_products_kernel, grid_for(ctx, n), dim3(256), 0, s, A, B, C, n);
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, C, C, HIPFFT_BACKWARD));  // H1 (x Y X)
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, A, A, HIPFFT_BACKWARD));  // H2 (x Y X)
    hipLaunchKernelGGL(window_kernel, grid_for(ctx, n), dim3(256), 0, s, A, C, g.Zt, (int64_t)Y * X);
    BH_CHECK_FFT(hipfftExecC2C(pl.z, C, C, HIPFFT_FORWARD));
    BH_CHECK_FFT(hipfftExecC2C(pl.z, A, A, HIPFFT_FORWARD));
    hipLaunchKernelGGL(wotf_combine_kernel, grid_for(ctx, n), dim3(256), 0, s, A, C, reinterpret_cast<cf*>(real_potential_tf),
                       reinterpret_cast<cf*>(imag_potential_tf), n, (float)g.z_px, count);
    BH_CHECK_HIP(hipGetLastError());
    BH_CHECK_HIP(hipStreamSynchronize(s));  // the plans die with this scope
    return BH_OK;
}

extern "C" int bh_fluorescence_transfer_function_3d(bh_ctx* ctx, int64_t Z, int64_t Y, int64_t X, double yx_pixel_size,
                                                    double z_pixel_size, double wavelength_emission, int64_t z_padding,
                                                    double index_of_refraction_media, double numerical_aperture_detection,
                                                    void* optical_transfer_function) {
    BH_REQUIRE(ctx && optical_transfer_function, "NULL argument");
    BH_REQUIRE(Z > 0 && Y > 0 && X > 0 && z_padding >= 0, "invalid shape");
    BH_REQUIRE(yx_pixel_size > 0 && z_pixel_size > 0 && wavelength_emission > 0 && index_of_refraction_media > 0 &&
                   numerical_aperture_detection > 0,
               "optical parameters must be positive");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    OpticsGeo g;
    g.Zt = (int)(Z + 2 * z_padding);
    g.Y = (int)Y;
    g.X = (int)X;
    g.yx_px = yx_pixel_size;
    g.z_px = z_pixel_size;
    g.inv_lamb = index_of_refraction_media / wavelength_emission;
    g.cut_ill = 0.0;
    g.cut_det = numerical_aperture_detection / wavelength_emission;
    g.invert = 0;
    const int64_t n = (int64_t)g.Zt * Y * X;
    cf* A;
    unsigned int* mx;
    BH_TRY(get_scratch(ctx, "optics_a", n * sizeof(cf), (void**)&A));
    BH_TRY(get_scratch(ctx, "optics_count", 64, (void**)&mx));
    C2CPlans pl;
    BH_TRY(make_c2c_plans(pl, g.Zt, g.Y, g.X, s));
    BH_CHECK_HIP(hipMemsetAsync(mx, 0, 64, s));
    hipLaunchKernelGGL(optics_planes_kernel, grid_for(ctx, n), dim3(256), 0, s, A, (cf*)nullptr, g, 0);
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, A, A, HIPFFT_BACKWARD));  // ifft2 (x Y X)
    hipLaunchKernelGGL(abs2_kernel, grid_for(ctx, n), dim3(256), 0, s, A, n, (float)(1.0 / ((double)Y * X)));
    BH_CHECK_FFT(hipfftExecC2C(pl.yx, A, A, HIPFFT_FORWARD));   // fftn = fft2 + fft along z
    BH_CHECK_FFT(hipfftExecC2C(pl.z, A, A, HIPFFT_FORWARD));
    hipLaunchKernelGGL(absmax_kernel, grid_for(ctx, n), dim3(256), 0, s, A, n, mx);
    hipLaunchKernelGGL(scale_by_max_kernel, grid_for(ctx, n), dim3(256), 0, s, A, reinterpret_cast<cf*>(optical_transfer_function), n, mx);
    BH_CHECK_HIP(hipGetLastError());
    BH_CHECK_HIP(hipStreamSynchronize(s));
    return BH_OK;
}

extern "C" int bh_fourier_central_cuboid(bh_ctx* ctx, const void* src, int64_t NZ, int64_t NY, int64_t NX, void* dst,
                                         int64_t nz, int64_t ny, int64_t nx) {
    BH_REQUIRE(ctx && src && dst, "NULL argument");
    BH_REQUIRE(nz > 0 && ny > 0 && nx > 0 && NZ >= nz && NY >= ny && NX >= nx, "the target must fit inside the source");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(central_cuboid_kernel, grid_for(ctx, nz * ny * nx), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const cf*>(src), reinterpret_cast<cf*>(dst), NZ, NY, NX, nz, ny, nx);
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}
