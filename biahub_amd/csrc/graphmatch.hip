// Edge-consistency cost of bead graph matching: the loop of GraphMatcher._compute_edge_consistency_cost
// (biahub/core/graph_matching.py:518-571).  For every pair (moving node i, reference node j) the reference fills a k_i x k_j
// table C[p][q] = float32(|a_p - b_q|) from the attributes of the two nodes' edges, solves it with linear_sum_assignment and
// keeps the mean of the matched entries: n * m tiny assignment problems, one per element of the cost matrix.
//
// The table is |a - b| on a line, so an optimal matching never crosses: with both rows sorted, equal counts pair in order, and
// unequal counts are the monotone dynamic programme over the sorted rows (s the shorter row, l the longer one)
//     f[p][q] = min(f[p][q - 1], f[p - 1][q - 1] + C[p][q]),    f[-1][.] = 0,    f[p][q] = +inf for q < p,
// the cheapest way to match s_0 .. s_p inside l_0 .. l_q, O(k_i * k_j) with one rolling row f[.] that is updated in place for
// ascending p while `prev` carries f[p - 1] of the previous q.
//
//   edge_cost_kernel   a workgroup of 256 threads takes tiles of GM_TI x GM_TJ = 16 x 64 pairs (capped grid, grid-stride loop over
//                      the tiles).  Per tile it stages the 16 rows of a and the 64 rows of b in LDS once (coalesced: the rows of
//                      a tile are one contiguous piece of the input), threads 0 .. 79 sort one row each in place (insertion
//                      sort, at most 16 entries), then lane x of wave w computes the pairs (i0 + w + 4 r, j0 + x), r = 0 .. 3:
//                      one thread per pair, four pairs in turn, 64 consecutive j per store.
//
// LDS rows have a pitch of 17 words: lane x reads word x * 17 + q of the b rows, 32 different banks for the 32 lanes of a
// group; the a row of a wave is one address for all lanes (a broadcast).  A pair whose b row is the shorter one swaps the
// roles, so a group may meet the a row's bank once more: two-way at worst.  The shorter row and the rolling row live in
// registers and are indexed by unrolled loops only, the longer row is read from LDS, so nothing goes to scratch.
//
// Arithmetic as the reference stores it: an entry is formed in double and rounded to float32; the matched entries are summed
// and divided by their number in float64 (exact for sixteen float32 terms of like magnitude) and rounded once.  No atomics,
// one writer per element: the same bytes on every run and on any number of compute units.
#include <climits>
#include <cmath>

#include "common.hpp"

namespace bh {

constexpr int GM_NT = 256, GM_WAVES = GM_NT / 64;
constexpr int GM_K = BH_GRAPH_KMAX;      // most attributes per node
constexpr int GM_TI = 16, GM_TJ = 64;    // pairs of a tile: rows of a, rows of b
constexpr int GM_PITCH = GM_K + 1;       // words per LDS row
constexpr int GM_WG_PER_CU = 4;          // the cap of the grid: what 122 VGPRs let a compute unit hold (tests size their wrap case from it)
static_assert(GM_TJ == 64 && GM_TI % GM_WAVES == 0, "a wave is one row of a against the 64 rows of b");
static_assert(GM_TI + GM_TJ <= GM_NT, "one thread sorts one row");

__device__ __forceinline__ float gm_entry(float a, float b) { return (float)fabs((double)a - (double)b); }

// rows sorted ascending, ka, kb in 0 .. GM_K
__device__ __forceinline__ float gm_pair(const float* ra, int ka, const float* rb, int kb, float default_cost) {
    if (ka == 0 || kb == 0) return default_cost;
    const bool a_short = ka <= kb;
    const float* s = a_short ? ra : rb;
    const float* l = a_short ? rb : ra;
    const int ks = a_short ? ka : kb, kl = a_short ? kb : ka;
    double total = 0.0;
    if (ks == kl) {
#pragma unroll
        for (int p = 0; p < GM_K; ++p)
            if (p < ks) total += (double)gm_entry(s[p], l[p]);
    } else {
        float sv[GM_K];
        double f[GM_K];
#pragma unroll
        for (int p = 0; p < GM_K; ++p) {
            sv[p] = p < ks ? s[p] : 0.0f;
            f[p] = (double)INFINITY;
        }
        for (int q = 0; q < kl; ++q) {
            const float lq = l[q];
            double prev = 0.0;
#pragma unroll
            for (int p = 0; p < GM_K; ++p) {
                if (p < ks) {
                    const double old = f[p];
                    const double c = prev + (double)gm_entry(sv[p], lq);
                    f[p] = old < c ? old : c;
                    prev = old;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < GM_K; ++p)
            if (p == ks - 1) total = f[p];
    }
    return (float)(total / (double)ks);
}

__global__ __launch_bounds__(GM_NT) void edge_cost_kernel(const float* __restrict__ attr_a, const int* __restrict__ cnt_a, int64_t n,
                                                          const float* __restrict__ attr_b, const int* __restrict__ cnt_b, int64_t m,
                                                          int kmax, float default_cost, int64_t tiles_j, int64_t ntiles,
                                                          float* __restrict__ cost) {
    __shared__ float rows[(GM_TI + GM_TJ) * GM_PITCH];  // the tile's a rows, then its b rows
    __shared__ int cnt[GM_TI + GM_TJ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t ti = tile / tiles_j, tj = tile - ti * tiles_j;
        const int64_t i0 = ti * GM_TI, j0 = tj * GM_TJ;
        const int na = (int)min((int64_t)GM_TI, n - i0), nb = (int)min((int64_t)GM_TJ, m - j0);
        // stage: the na (nb) rows are na * kmax (nb * kmax) consecutive floats of the input
        for (int e = threadIdx.x; e < na * kmax; e += GM_NT) rows[(e / kmax) * GM_PITCH + e % kmax] = attr_a[i0 * kmax + e];
        for (int e = threadIdx.x; e < nb * kmax; e += GM_NT) rows[(GM_TI + e / kmax) * GM_PITCH + e % kmax] = attr_b[j0 * kmax + e];
        if (threadIdx.x < GM_TI + GM_TJ) {
            const int r = threadIdx.x;
            int c = 0;  // rows past the matrix's edge are empty; a count outside 0 .. kmax is clamped, never followed
            if (r < GM_TI) {
                if (r < na) c = cnt_a[i0 + r];
            } else if (r - GM_TI < nb) {
                c = cnt_b[j0 + r - GM_TI];
            }
            cnt[r] = max(0, min(c, kmax));
        }
        __syncthreads();
        if (threadIdx.x < GM_TI + GM_TJ) {
            float* row = rows + threadIdx.x * GM_PITCH;
            const int c = cnt[threadIdx.x];
            for (int u = 1; u < c; ++u) {
                const float v = row[u];
                int w = u;
                while (w > 0 && row[w - 1] > v) {
                    row[w] = row[w - 1];
                    --w;
                }
                row[w] = v;
            }
        }
        __syncthreads();
        const int kb = cnt[GM_TI + lane];
        const float* rb = rows + (GM_TI + lane) * GM_PITCH;
        for (int r = 0; r < GM_TI / GM_WAVES; ++r) {
            const int li = wave + GM_WAVES * r;
            if (li < na && lane < nb) cost[(i0 + li) * m + j0 + lane] = gm_pair(rows + li * GM_PITCH, cnt[li], rb, kb, default_cost);
        }
        __syncthreads();  // the next tile overwrites rows and cnt
    }
}

}  // namespace bh

using namespace bh;

extern "C" int bh_edge_consistency_plan(int64_t n, int64_t m, int64_t* tile_n, int64_t* tile_m, int64_t* tiles, int* wg_per_cu) {
    BH_REQUIRE(tile_n && tile_m && tiles, "bh_edge_consistency_plan: null argument");
    BH_REQUIRE(n >= 0 && m >= 0 && n <= (int64_t)INT_MAX && m <= (int64_t)INT_MAX, "bh_edge_consistency_plan: (%lld, %lld) nodes: 0 to 2**31 - 1 a side",
               (long long)n, (long long)m);
    *tile_n = GM_TI;
    *tile_m = GM_TJ;
    *tiles = ceil_div(n, GM_TI) * ceil_div(m, GM_TJ);
    if (wg_per_cu) *wg_per_cu = GM_WG_PER_CU;
    return BH_OK;
}

extern "C" int bh_edge_consistency_cost(bh_ctx* ctx, const float* attr_a, const int32_t* cnt_a, int64_t n, const float* attr_b, const int32_t* cnt_b,
                                        int64_t m, int kmax, float default_cost, float* cost) {
    BH_REQUIRE(ctx, "bh_edge_consistency_cost: null context");
    BH_REQUIRE(kmax >= 1 && kmax <= GM_K, "bh_edge_consistency_cost: kmax = %d (1 to %d attributes per node)", kmax, GM_K);
    int64_t tn = 0, tm = 0, ntiles = 0;
    BH_TRY(bh_edge_consistency_plan(n, m, &tn, &tm, &ntiles, nullptr));
    if (ntiles == 0) return BH_OK;
    BH_REQUIRE(attr_a && cnt_a && attr_b && cnt_b && cost, "bh_edge_consistency_cost: null argument");
    BH_CHECK_HIP(hipSetDevice(ctx->device));
    const int grid = (int)std::min<int64_t>(ntiles, (int64_t)ctx->num_cus * GM_WG_PER_CU);
    {
        ScopedTimer timer(ctx, T_EDGECOST);
        hipLaunchKernelGGL(edge_cost_kernel, dim3(grid), dim3(GM_NT), 0, ctx->stream, attr_a, cnt_a, n, attr_b, cnt_b, m, kmax, default_cost,
                           ceil_div(m, GM_TJ), ntiles, cost);
    }
    BH_CHECK_HIP(hipGetLastError());
    return BH_OK;
}
