// Stand-alone probe of biahub_amd/csrc/reduce.hpp (tests/test_gpu_reduce_orders.py): one kernel per helper, one workgroup each.
// Reads records from the file named on the command line and prints one line of hex bit patterns per record.
//
//   record   int32 helper, type, op, count, then `count` values of the type (ValIdx: the 16-byte struct)
//   helper   0 wave_reduce, 64 threads, every lane printed     1 wave_totals<4>, red[0..4) printed
//            2 block_reduce<4>                                  3 block_reduce<4, true> twice in one kernel, 2 x 256 values
//            4 block_reduce_n<4, 3>, 3 x 256 values             5 tree_reduce<256>, thread 0's and thread 255's return value
//            6 tree_reduce<1024>, threads 0 and 1023            7 tree_reduce<256, true> twice in one kernel, 2 x 256 values
//   type     0 float, 1 double, 2 int, 3 unsigned long long, 4 ValIdx<float>, 5 ValIdx<double>
//   op       0 sum, 1 min, 2 max, 3 first_max
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "reduce.hpp"

using namespace bh;

constexpr int kThreads[8] = {64, 256, 256, 256, 256, 256, 1024, 256};
constexpr int kInputs[8] = {64, 256, 256, 512, 768, 256, 1024, 512};
constexpr int kOutputs[8] = {64, 4, 1, 2, 3, 2, 2, 2};

template <int H, typename T, typename Op>
__global__ void probe_kernel(const T* __restrict__ in, T* __restrict__ out) {
    const int t = threadIdx.x;
    Op op;
    if constexpr (H == 0) {
        out[t] = wave_reduce(in[t], op);
    } else if constexpr (H == 1) {
        __shared__ T red[4];
        wave_totals<4>(in[t], op, red);
        if (t < 4) out[t] = red[t];
    } else if constexpr (H == 2) {
        __shared__ T red[4];
        const T r = block_reduce<4>(in[t], op, red);
        if (t == 0) out[0] = r;
    } else if constexpr (H == 3) {
        __shared__ T red[4];
        for (int k = 0; k < 2; ++k) {
            const T r = block_reduce<4, true>(in[k * 256 + t], op, red);
            if (t == 0) out[k] = r;
        }
    } else if constexpr (H == 4) {
        __shared__ T red[4 * 3], res[3];
        const T a[3] = {in[t], in[256 + t], in[512 + t]};
        block_reduce_n<4, 3>(a, op, red, res);
        if (t == 255)  // reads what threads 0, 1, 2 wrote: the trailing barrier
            for (int k = 0; k < 3; ++k) out[k] = res[k];
    } else if constexpr (H == 5 || H == 6) {
        constexpr int NT = H == 5 ? 256 : 1024;
        __shared__ T red[NT];
        const T r = tree_reduce<NT>(in[t], op, red);
        if (t == 0) out[0] = r;
        if (t == NT - 1) out[1] = r;
    } else {
        __shared__ T red[256];
        for (int k = 0; k < 2; ++k) {
            const T r = tree_reduce<256, true>(in[k * 256 + t], op, red);
            if (t == 255 * k) out[k] = r;
        }
    }
}

static void print_one(float v) { uint32_t u; memcpy(&u, &v, 4); printf(" %08x", u); }
static void print_one(double v) { uint64_t u; memcpy(&u, &v, 8); printf(" %016llx", (unsigned long long)u); }
static void print_one(int v) { printf(" %08x", (unsigned)v); }
static void print_one(unsigned long long v) { printf(" %016llx", v); }
template <typename V>
static void print_one(ValIdx<V> p) {
    print_one(p.v);
    printf(":%lld", p.i);
}

#define HIP_OK(expr)                                                                  \
    do {                                                                              \
        const hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));                \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

template <int H, typename T, typename Op>
static int launch(const T* d_in, T* d_out) {
    hipLaunchKernelGGL((probe_kernel<H, T, Op>), dim3(1), dim3(kThreads[H]), 0, 0, d_in, d_out);
    return 0;
}

template <typename T, typename Op>
static int run(int helper, FILE* f, int count) {
    if (count != kInputs[helper]) return 3;
    std::vector<T> in(count), out(kOutputs[helper]);
    if (fread(in.data(), sizeof(T), count, f) != (size_t)count) return 3;
    T *d_in = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc((void**)&d_in, in.size() * sizeof(T)));
    HIP_OK(hipMalloc((void**)&d_out, out.size() * sizeof(T)));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(T), hipMemcpyHostToDevice));
    switch (helper) {
        case 0: launch<0, T, Op>(d_in, d_out); break;
        case 1: launch<1, T, Op>(d_in, d_out); break;
        case 2: launch<2, T, Op>(d_in, d_out); break;
        case 3: launch<3, T, Op>(d_in, d_out); break;
        case 4: launch<4, T, Op>(d_in, d_out); break;
        case 5: launch<5, T, Op>(d_in, d_out); break;
        case 6: launch<6, T, Op>(d_in, d_out); break;
        default: launch<7, T, Op>(d_in, d_out); break;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    for (const T& v : out) print_one(v);
    printf("\n");
    return 0;
}

template <typename T>
static int run_arith(int helper, int op, FILE* f, int count) {
    if (op == 0) return run<T, op_sum>(helper, f, count);
    if (op == 1) return run<T, op_min>(helper, f, count);
    if (op == 2) return run<T, op_max>(helper, f, count);
    return 3;
}

int main(int argc, char** argv) {
    if (argc != 2) return 3;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[4];
    int n = 0;
    while (fread(h, sizeof(int32_t), 4, f) == 4) {
        const int helper = h[0], type = h[1], op = h[2], count = h[3];
        if (helper < 0 || helper > 7) return 3;
        printf("%d", n++);
        int s = 3;
        if (type == 0) s = run_arith<float>(helper, op, f, count);
        if (type == 1) s = run_arith<double>(helper, op, f, count);
        if (type == 2) s = run_arith<int>(helper, op, f, count);
        if (type == 3 && op == 0) s = run<unsigned long long, op_sum>(helper, f, count);
        if (type == 4 && op == 3) s = run<ValIdx<float>, first_max<float>>(helper, f, count);
        if (type == 5 && op == 3) s = run<ValIdx<double>, first_max<double>>(helper, f, count);
        if (s != 0) {
            fprintf(stderr, "record %d (helper %d, type %d, op %d, count %d): status %d\n", n - 1, helper, type, op, count, s);
            return s;
        }
    }
    fclose(f);
    return 0;
}
