// Track identities for gfx950 (DESIGN.md 4b'-link "the identity rule"; tracks.py is the caller): the pairwise distance between the
// descriptors of two tracks, and a weighted mean over groups of rows.
//
//   track_affinity    one wave per ordered pair (a, b), four pairs per workgroup.  Lane l takes texels l, l + 64, ... of the two atlases
//                     in raster order (part, i, j); a texel is one 16-byte load per side.  Per lane: S = sum m, D = sum m |rgb_a - rgb_b|^2
//                     in double, n = #{m > 0}, u = #{wa > w_min or wb > w_min}; the 64 partials are combined by a fixed xor butterfly.
//                     The colours of a texel with m = 0 never enter the arithmetic (a branch, not a product with 0), so a NaN there
//                     does not spread.  d_shape is ten sequential double terms, the same in every lane.
//   track_group_mean  one lane per (group, column), adjacent lanes adjacent columns, sequential over the group's rows through a CSR:
//                     sum c x / sum c in double over the rows with c > 0 (rows with c = 0 are never read), rounded to fp32 once; with
//                     write_back the rounded mean goes into that column of every row of the group.  A group without weight reports
//                     status 1, mean 0, and its rows are not touched.
//
// No atomics, no LDS, no grid barrier; a lane reads only its own pair or group, so a result does not depend on its neighbours in the
// launch, and two runs give the same bits.  Compiled with -ffp-contract=off: tests/link_oracle.py restates the operations.
#include <vector>

#include "common.h"
#include "video_sizes.h"

using namespace danet;

namespace {

constexpr int kWave = 64;
constexpr int kPairsPerBlock = 4;
constexpr double kWMin = 1e-3;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__global__ __launch_bounds__(kWave * kPairsPerBlock) void track_affinity_kernel(const float* __restrict__ shape, const float4* __restrict__ atlas,
                                                                                int K, int texels, const int32_t* __restrict__ pairs, int C,
                                                                                float4* __restrict__ out)
{
    const int p = blockIdx.x * kPairsPerBlock + (int)(threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    if (p >= C) return;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= K || b < 0 || b >= K) {                                   // (the host has refused such a table already)
        if (lane == 0) out[p] = make_float4(NAN, NAN, NAN, NAN);
        return;
    }
    const float4* A = atlas + (size_t)a * texels;
    const float4* B = atlas + (size_t)b * texels;
    double S = 0.0, D = 0.0;
    int n = 0, u = 0;
    for (int x = lane; x < texels; x += kWave) {
        const float4 ta = A[x], tb = B[x];
        const bool ia = (double)ta.w > kWMin, ib = (double)tb.w > kWMin;
        u += (ia || ib) ? 1 : 0;
        if (ia && ib) {
            const double m = (ta.w < 1.0f ? (double)ta.w : 1.0) * (tb.w < 1.0f ? (double)tb.w : 1.0);
            const double dr = (double)ta.x - (double)tb.x, dg = (double)ta.y - (double)tb.y, db = (double)ta.z - (double)tb.z;
            S += m;
            D += m * ((dr * dr + dg * dg) + db * db);
            n += 1;
        }
    }
    S = wave_sum(S);
    D = wave_sum(D);
    n = wave_sum(n);
    u = wave_sum(u);
    if (lane != 0) return;
    double ds = 0.0;
#pragma unroll
    for (int i = 0; i < kNB; ++i) {
        const double d = (double)shape[(size_t)a * kNB + i] - (double)shape[(size_t)b * kNB + i];
        ds += d * d;
    }
    const double d_app = n > 0 ? D / (3.0 * S) : 0.0;
    const double overlap = u > 0 ? (double)n / (double)u : 0.0;
    out[p] = make_float4((float)(ds / (double)kNB), (float)d_app, (float)overlap, (float)S);
}

__global__ __launch_bounds__(kWave) void track_group_mean_kernel(float* __restrict__ rows, const float* __restrict__ conf,
                                                                 const int32_t* __restrict__ group_start, const int32_t* __restrict__ group_rows,
                                                                 int G, int N, int col0, int ncol, float* __restrict__ mean,
                                                                 int32_t* __restrict__ status, int write_back)
{
    const long idx = (long)blockIdx.x * kWave + threadIdx.x;
    if (idx >= (long)G * ncol) return;
    const int g = (int)(idx / ncol), j = (int)(idx % ncol);
    const int s = group_start[g], e = group_start[g + 1];
    if (s < 0 || e > N || s > e) return;                                       // (refused on the host already)
    float* x = rows + col0 + j;
    double sc = 0.0, sy = 0.0;
    for (int r = s; r < e; ++r) {
        const int row = group_rows[r];
        if (row < 0 || row >= N) continue;
        const float c = conf[row];
        if (c > 0.0f) {
            sc += (double)c;
            sy += (double)c * (double)x[(size_t)row * kParaRow];
        }
    }
    const bool has = sc > 0.0;
    if (j == 0) status[g] = has ? 0 : 1;
    const float m = has ? (float)(sy / sc) : 0.0f;
    mean[(size_t)g * ncol + j] = m;
    if (!write_back || !has) return;
    for (int r = s; r < e; ++r) {
        const int row = group_rows[r];
        if (row < 0 || row >= N) continue;
        x[(size_t)row * kParaRow] = m;
    }
}

}  // namespace

extern "C" int danet_track_affinity(const float* shape, const float* atlas, int K, int T, const int32_t* pairs, const int32_t* pairs_host,
                                    long C, float* out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(C >= 0 && C < (1L << 31) - kPairsPerBlock, "track_affinity: bad pair count C=%ld", C);
    if (C == 0) return DANET_OK;
    DANET_CHECK_ARG(K >= 1 && T >= 2 && T <= 4096, "track_affinity: bad sizes K=%d T=%d (T in [2, 4096])", K, T);
    DANET_CHECK_ARG(shape && atlas && pairs && pairs_host && out, "track_affinity: null pointer");
    DANET_CHECK_ARG((reinterpret_cast<uintptr_t>(atlas) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                    "track_affinity: atlas and out must be 16-byte aligned");
    for (long c = 0; c < 2 * C; ++c)
        DANET_CHECK_ARG(pairs_host[c] >= 0 && pairs_host[c] < K, "track_affinity: pair %ld names track %d of %d", c / 2, pairs_host[c], K);
    const int texels = kParts * T * T;
    hipLaunchKernelGGL(track_affinity_kernel, dim3(danet::cdiv(C, kPairsPerBlock)), dim3(kWave * kPairsPerBlock), 0, (hipStream_t)stream, shape,
                       (const float4*)atlas, K, texels, pairs, (int)C, (float4*)out);
    DANET_CHECK_LAUNCH("track_affinity_kernel");
    return DANET_OK;
}

extern "C" int danet_track_group_mean(float* rows, const float* conf, const int32_t* group_start, const int32_t* group_start_host,
                                      const int32_t* group_rows, const int32_t* group_rows_host, int G, long N, int col0, int ncol,
                                      float* mean, int32_t* status, int write_back, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(G >= 0 && N >= 0 && N < (1L << 31), "track_group_mean: bad sizes G=%d N=%ld", G, N);
    if (G == 0 || N == 0) return DANET_OK;
    DANET_CHECK_ARG(col0 >= 0 && ncol >= 1 && col0 + ncol <= kParaRow, "track_group_mean: columns %d .. %d of %d", col0, col0 + ncol, kParaRow);
    DANET_CHECK_ARG(rows && conf && group_start && group_start_host && group_rows && group_rows_host && mean && status,
                    "track_group_mean: null pointer");
    DANET_CHECK_OFFSETS("track_group_mean", "group_start", group_start_host, G, N);
    std::vector<unsigned char> seen((size_t)N, 0);                             // every row in exactly one group: no two lanes share a row
    for (long r = 0; r < N; ++r) {
        const int32_t row = group_rows_host[r];
        DANET_CHECK_ARG(row >= 0 && row < N && !seen[(size_t)row], "track_group_mean: group_rows[%ld] = %d (a permutation of 0 .. %ld expected)", r,
                        row, N - 1);
        seen[(size_t)row] = 1;
    }
    DANET_CHECK_ARG((long)G * ncol / kWave + 1 < (1L << 31), "track_group_mean: G=%d groups of %d columns exceed the grid", G, ncol);
    hipLaunchKernelGGL(track_group_mean_kernel, dim3(danet::cdiv((long)G * ncol, kWave)), dim3(kWave), 0, (hipStream_t)stream, rows, conf,
                       group_start, group_rows, G, (int)N, col0, ncol, mean, status, write_back ? 1 : 0);
    DANET_CHECK_LAUNCH("track_group_mean_kernel");
    return DANET_OK;
}
