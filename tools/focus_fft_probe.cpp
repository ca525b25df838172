// Probe for DESIGN.md §3.8: the two forms of the focus transform on Z slices of (Y, X) float32, timed interleaved in one process.
//   plain      one batched 2-D real-to-complex plan over the Z slices (what csrc/focus.hip runs)
//   separable  a batched 1-D real-to-complex plan over all Z * Y rows, then per slice a strided 1-D complex plan along y over the
//              first K columns of the half spectrum only (the band needs columns below max(kx_hi): K = 162 of 401 at 800 x 800,
//              default optics, 0.1494 um)
// Prints the median of the rounds in ms per form, and the largest |difference| of the two spectra over the K columns relative to
// the largest magnitude.  hipcc --offload-arch=gfx950 -O2 tools/focus_fft_probe.cpp -lhipfft -o focus_fft_probe; args: Z Y X K rounds
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                      \
    do {                                                           \
        if ((int)(x) != 0) {                                       \
            printf("FAILED %s (%d) line %d\n", #x, (int)(x), __LINE__); \
            return 1;                                              \
        }                                                          \
    } while (0)

int main(int argc, char** argv) {
    const int Z = argc > 1 ? atoi(argv[1]) : 100, Y = argc > 2 ? atoi(argv[2]) : 800, X = argc > 3 ? atoi(argv[3]) : 800;
    const int K = argc > 4 ? atoi(argv[4]) : 162, rounds = argc > 5 ? atoi(argv[5]) : 11;
    const int nh = X / 2 + 1;
    if (Z < 1 || Y < 2 || X < 2 || K < 1 || K > nh || rounds < 1) return 2;
    const size_t nreal = (size_t)Z * Y * X, nspec = (size_t)Z * Y * nh;
    float* d_real;
    hipfftComplex *d_a, *d_b;
    CK(hipMalloc(&d_real, nreal * sizeof(float)));
    CK(hipMalloc(&d_a, nspec * sizeof(hipfftComplex)));
    CK(hipMalloc(&d_b, nspec * sizeof(hipfftComplex)));
    {
        std::vector<float> h(nreal);
        srand(7);
        for (auto& v : h) v = 100.f + (float)(rand() % 4096);
        CK(hipMemcpy(d_real, h.data(), nreal * sizeof(float), hipMemcpyHostToDevice));
    }
    hipfftHandle plain, rows, cols;
    int n2[2] = {Y, X}, nx[1] = {X}, ny[1] = {Y};
    CK(hipfftPlanMany(&plain, 2, n2, nullptr, 1, Y * X, nullptr, 1, Y * nh, HIPFFT_R2C, Z));
    CK(hipfftPlanMany(&rows, 1, nx, nullptr, 1, X, nullptr, 1, nh, HIPFFT_R2C, Z * Y));
    CK(hipfftPlanMany(&cols, 1, ny, ny, nh, 1, ny, nh, 1, HIPFFT_C2C, K));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto run_plain = [&]() { return (int)hipfftExecR2C(plain, d_real, d_a); };
    auto run_sep = [&]() {
        int r = (int)hipfftExecR2C(rows, d_real, d_b);
        for (int z = 0; z < Z && r == 0; ++z) r = (int)hipfftExecC2C(cols, d_b + (size_t)z * Y * nh, d_b + (size_t)z * Y * nh, HIPFFT_FORWARD);
        return r;
    };
    std::vector<float> t_plain, t_sep;
    for (int i = 0; i < rounds + 3; ++i) {  // three warm-up rounds
        float ms = 0;
        CK(hipEventRecord(e0, 0));
        CK(run_plain());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 3) t_plain.push_back(ms);
        CK(hipEventRecord(e0, 0));
        CK(run_sep());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 3) t_sep.push_back(ms);
    }
    std::sort(t_plain.begin(), t_plain.end());
    std::sort(t_sep.begin(), t_sep.end());
    // the two forms agree on the K columns (slice 0 and the last slice)
    double worst = 0, big = 0;
    std::vector<hipfftComplex> ha((size_t)Y * nh), hb((size_t)Y * nh);
    for (int z : {0, Z - 1}) {
        CK(hipMemcpy(ha.data(), d_a + (size_t)z * Y * nh, ha.size() * sizeof(hipfftComplex), hipMemcpyDeviceToHost));
        CK(hipMemcpy(hb.data(), d_b + (size_t)z * Y * nh, hb.size() * sizeof(hipfftComplex), hipMemcpyDeviceToHost));
        for (int y = 0; y < Y; ++y)
            for (int k = (y == 0 ? 1 : 0); k < K; ++k) {  // without the DC bin
                const hipfftComplex a = ha[(size_t)y * nh + k], b = hb[(size_t)y * nh + k];
                worst = std::max(worst, std::hypot((double)a.x - b.x, (double)a.y - b.y));
                big = std::max(big, std::hypot((double)a.x, (double)a.y));
            }
    }
    printf("{\"shape\": [%d, %d, %d], \"K\": %d, \"rounds\": %d, \"plain_ms\": %.4f, \"separable_ms\": %.4f, \"plain_min_ms\": %.4f, "
           "\"separable_min_ms\": %.4f, \"max_diff_rel\": %.3e}\n",
           Z, Y, X, K, rounds, t_plain[t_plain.size() / 2], t_sep[t_sep.size() / 2], t_plain[0], t_sep[0], worst / big);
    return 0;
}
