// Interface of the fused FFT-convolution engine (fftconv.hip and the kernel families it drives) to the rest of the library:
// the plan, the epilogues of the inverse X pass, and every fftconv_* entry point another translation unit calls.
#pragma once
#include "common.hpp"

namespace bh {

typedef float2 cf;

// shape of one engine volume and the lengths derived from it (handed to kernels by value)
struct ConvDims {
    int Z, Y, X;   // real volume
    int M;         // X / 2 (complex FFT length along x)
    int XP;        // spectrum row pitch in complex elements
    int logM, logYh, logZ;  // log2 of M and of the power-of-two parts of Y/2 and Z
    int Lyh, Lz;            // those parts: Y/2 and Z themselves, or a third of them (radix-3 column passes)
    int Lm;                 // M or M / 3 (radix-3 first step of the row transforms)
};

// the device-side tables of one (device, shape), cached by fftconv_plan; callers outside the engine only pass it on
struct ConvPlan {
    ConvDims d;
    cf *tw_x = nullptr, *tw_y = nullptr, *tw_z = nullptr, *untangle = nullptr, *twy = nullptr;
    int ntw_x = 0, ntw_y = 0, ntw_z = 0;
    int Wy = 0, Wz = 0;
    int Lyh = 0, Lz = 0;                      // power-of-two part of Y/2 and Z (== them, or a third of them)
    cf *tw3_y = nullptr, *tw3_z = nullptr;    // radix-3 twiddles where the axis is 3 * 2^k
    cf* tw3_x = nullptr;                      // same for the rows (M = 3 Lm)
    int xr = 0;                               // rows per X-pass tile: which instantiation of the X passes runs
    // wave-private X passes (fftconv_xw.inc) for rows of 1024 / 2048 voxels: their tables, and the stored column of every
    // bit-reversed position (they keep the spectrum row in their own column order)
    // set by bh_richardson_lucy_apply_rows for the duration of one call: where the LAST update pass leaves the row sums of the
    // estimate it stores (xw::Params::rowsum); rl_rowsums_done says that a pass took it
    double* rl_rowsums = nullptr;
    bool rl_rowsums_done = false;
    bool xw = false;
    bool x3 = false;  // rows of 1536 / 3072 voxels: the radix-3 kernels of fftconv_x3.inc (same role, tables and column map)
    cf* xw_tab = nullptr;
    int* xw_col = nullptr;
    // register-stage column passes (fftconv_colw.inc) for columns of 256 / 512 / 1024 points: their twiddle tables
    cf *colw_y = nullptr, *colw_z = nullptr;
    cf* colz = nullptr;  // radix-8 register-stage Z pass of 512-point columns (fftconv_colz.inc)
    cf* colz3 = nullptr;  // register-stage Z pass of 384-point columns (fftconv_colz3.inc)
};

// what the inverse X pass does with the real rows it produces (fftconv_apply's `epilogue`)
enum XEpilogue { XE_STORE = 0, XE_RATIO = 1, XE_UPDATE = 2 };

// Richardson-Lucy's two pointwise steps, as every kernel that applies them (X-pass epilogues, deconv.hip) computes them:
// a true divide, and a product that is rounded before the clamp
__device__ __forceinline__ float rl_ratio(float d, float blur, float eps) { return d / fmaxf(blur, eps); }
__device__ __forceinline__ float rl_update(float est, float corr) { return fmaxf(est * corr, 0.0f); }

// ---- shapes and plans ----
bool fftconv_supported(int64_t Z, int64_t Y, int64_t X);
bool fftconv_supported_ex(int64_t Z, int64_t Y, int64_t X, bool radix3);
bool fftconv_rows_wave_private(int64_t Y, int64_t X);
int fftconv_plan(bh_ctx* ctx, int64_t Z, int64_t Y, int64_t X, ConvPlan** out);
int fftconv_plan_tag(const ConvPlan& pl);
size_t fftconv_spectrum_elems(const ConvPlan& pl);
int fftconv_tune_spectrum(bh_ctx* ctx, const ConvPlan& pl, const cf* otf, bool otf_real, int zr, bool zreal, float* est, size_t bytes,
                          cf** spec);
void fftconv_arm_rowsums(ConvPlan& pl, double* dst);
bool fftconv_rowsums_taken(ConvPlan& pl);

// ---- transfer functions, z taps, staged filters ----
int fftconv_make_otf(bh_ctx* ctx, const ConvPlan& pl, const float* padded_psf, cf* otf);
int fftconv_ztaps_radius(const ConvPlan& pl, int64_t pz);
size_t fftconv_ztaps_elems(const ConvPlan& pl, int R, bool hermitian);
int fftconv_make_ztaps(bh_ctx* ctx, const ConvPlan& pl, const float* padded_psf, bool hermitian, bool zreal, int R, cf* work, cf* taps);
int fftconv_stage_inverse_filter(bh_ctx* ctx, const ConvPlan& pl, const void* tf, bool tf_complex, float reg, bool bf16,
                                 void* filt);

// ---- convolutions ----
int fftconv_apply(bh_ctx* ctx, const ConvPlan& pl, const float* in, const cf* otf, bool correlate, cf* spec,
                  int epilogue, const float* aux, float eps, float* out);
bool fftconv_fuses_normalisation(const ConvPlan& pl);
int fftconv_apply_staged_filter(bh_ctx* ctx, const ConvPlan& pl, const float* in, const void* filt, bool bf16, cf* spec,
                                float* out, const double* norm_mean);
int fftconv_tikhonov(bh_ctx* ctx, const ConvPlan& pl, const float* in, const float* tf_full, float reg, cf* spec,
                     float* filt, float* out);

// ---- Richardson-Lucy ----
int fftconv_richardson_lucy(bh_ctx* ctx, const ConvPlan& pl, const float* d, const cf* otf, bool otf_real, int zr, bool zreal, cf* spec,
                            int iterations, float eps, float* est);
int fftconv_rl_iteration_padded(bh_ctx* ctx, const ConvPlan& pl, const float* est_p, const float* d_p, const cf* otf,
                                bool otf_real, int zr, bool zreal, cf* spec, float eps, float* corr_p);
bool fftconv_rl_wrap_supported(const ConvPlan& pl, const int64_t N[3], const int64_t K[3], const int64_t P[3]);
int fftconv_richardson_lucy_wrap(bh_ctx* ctx, const ConvPlan& pl, const float* d_p, const cf* otf, bool otf_real, int zr, bool zreal, cf* spec_a,
                                 cf* spec_b, float* est_a, float* est_b, const int64_t N[3], const int64_t K[3], int iterations,
                                 float eps, float* out);

// ---- bare transforms and phase cross-correlation ----
int fftconv_forward(bh_ctx* ctx, const ConvPlan& pl, const float* in, cf* spec);
int fftconv_inverse(bh_ctx* ctx, const ConvPlan& pl, cf* spec, float* out);
bool fftconv_pcc_peak_only(const ConvPlan& pl);
int fftconv_pcc_apply(bh_ctx* ctx, const ConvPlan& pl, const float* img, cf* fixed, bool fixed_is_mov, bool roll, cf* s2, int norm,
                      float scale, float* corr, ArgMax* partial, int* npartial);
int fftconv_pcc(bh_ctx* ctx, const ConvPlan& pl, const float* ref, const float* mov, cf* s1, cf* s2, int norm, float scale, float* corr,
                ArgMax* partial, int* npartial);

}  // namespace bh
