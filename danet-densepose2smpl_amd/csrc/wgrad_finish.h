// The split-K finish of the weight-gradient kernels: dW = beta * dW + the sum of a problem's partial blocks.
//
// Every MFMA weight-gradient kernel that splits the pixel axis leaves part[split][g][tap][cout][cin] (fp32) in a workspace and wants
// the torch layout dW[g][cout][cin][tap].  With cc = cout * Cin_g + cin and CC = Cout_g * Cin_g that is, per group, the plain transpose
// [tap][CC] -> [CC][tap]: a run of L consecutive cc is `taps` contiguous source runs of L floats and ONE contiguous destination run of
// L * taps floats.  A workgroup owns such a run: it reads the partials with 16-byte loads (taps x 4 splits in flight per thread), parks
// the sums in LDS as [cc][tap] and writes the destination as consecutive 16-byte stores.  (49 taps do not fit a thread's registers: a
// workgroup then takes seven of them and writes rows of seven floats; the regressor stems' gradient is 0.8 MB behind 118 MB of partials,
// and what that needs is workgroups: with all 49 taps in one workgroup the launch took 105 us, with seven 25 us.)
//
// The order of the additions is fixed and is the one the element-per-thread reduce kernels before this one used:
//     s = 0;  for each full group of four splits  s += (v0 + v1) + (v2 + v3);  then the remaining splits one by one;  then beta.
// A problem with many splits and few elements (a 16 -> 16 layer behind 256 splits) would be a handful of workgroups walking a long
// chain of dependent loads, so the 256 threads of a workgroup are T = L / 4 element threads x P split lanes: in a round, lane p computes
// the group sum (v0 + v1) + (v2 + v3) of group r P + p -- those are independent -- and leaves it in LDS, then one thread per element
// adds the round's P sums to s IN GROUP ORDER.  The bits do not depend on P.
#pragma once
#include <cstdint>
#include "common.h"
#include "conv_common.h"

namespace danet_conv {
namespace {          // (every translation unit that includes this gets a kernel of its own)

constexpr int FIN_NP = 32;                          // problems per finish launch (by-value descriptors: 1.2 KB)
// Pending partial sums a multi-problem call may leave behind its MFMA launches before it finishes them: about half the 256 MB infinity
// cache, so that a finish launch still finds most of what it reads there, and several small launch groups share one finish launch.
constexpr size_t FIN_BUDGET_BYTES = (size_t)128 << 20;

struct FinishArgs {
    const float* part[FIN_NP]; float* dw[FIN_NP];
    int CC[FIN_NP], G[FIN_NP], ms[FIN_NP], lp[FIN_NP];          // lp: log2 of the split lanes P
    int start[FIN_NP + 1];                                      // first workgroup of each problem
    int n; float beta;
};

template <int TAPS> constexpr int fin_tc() { return TAPS == 49 ? 7 : TAPS; }      // taps a thread carries at a time

__device__ __forceinline__ float4 fin_add(const float4 a, const float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

template <int TAPS>
__global__ __launch_bounds__(256) void wgrad_finish_kernel(FinishArgs a)
{
    constexpr int TC = fin_tc<TAPS>();
    static_assert(TAPS % TC == 0, "tap chunks");
    extern __shared__ __attribute__((aligned(16))) float fin_smem[];
    const int t = threadIdx.x, b = (int)blockIdx.x;
    int i = 0;
    while (i + 1 < a.n && b >= a.start[i + 1]) ++i;
    const int CC = a.CC[i], ms = a.ms[i], lp = a.lp[i];
    const int P = 1 << lp, T = 256 >> lp, L = T * 4;
    constexpr int NCH = TAPS / TC;                               // tap chunks: a workgroup takes one of them
    const int tpg = (CC + L - 1) / L;                            // runs per group
    const int tile = (b - a.start[i]) / NCH, t0 = ((b - a.start[i]) - tile * NCH) * TC;
    const int g = tile / tpg, cc0 = (tile - g * tpg) * L;
    const int run = min(L, CC - cc0);                            // floats of this run per tap (a multiple of 4)
    const size_t total = (size_t)a.G[i] * TAPS * CC;             // floats of one split
    const float* const src = a.part[i] + (size_t)g * TAPS * CC + cc0;
    float* const tileS = fin_smem;                               // [run][TC]
    float4* const red = reinterpret_cast<float4*>(fin_smem + L * TC);        // [P][TC][T] group sums of a round (P > 1)

    const int it = t & (T - 1), pl = t >> (8 - lp);
    const bool lane_on = it * 4 < run;
    const int ng = ms >> 2, rem = ms & 3;
    // the sums a thread carries: chain c = t + 256 j < T * TC is tap tc = c / T of element thread ci = c % T (P = 1: its own loads)
    int ctc[TC], cci[TC];
    bool con[TC];
#pragma unroll
    for (int j = 0; j < TC; ++j) {
        const int c = t + 256 * j;
        ctc[j] = c >> (8 - lp); cci[j] = c & (T - 1);
        con[j] = ctc[j] < TC && cci[j] * 4 < run;
    }
    {
        float4 s[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) s[j] = float4{0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < ng; r0 += P) {
            const int k = r0 + pl;
            const bool on = k < ng && lane_on;
            float4 gs[TC];
            if (on) {
                const float* const q = src + (size_t)(4 * k) * total + (size_t)t0 * CC + 4 * it;
                float4 v[4][TC];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tc = 0; tc < TC; ++tc) v[u][tc] = *reinterpret_cast<const float4*>(q + (size_t)u * total + (size_t)tc * CC);
#pragma unroll
                for (int tc = 0; tc < TC; ++tc) gs[tc] = fin_add(fin_add(v[0][tc], v[1][tc]), fin_add(v[2][tc], v[3][tc]));
            }
            if (P == 1) {
                if (on) {
#pragma unroll
                    for (int j = 0; j < TC; ++j) s[j] = fin_add(s[j], gs[j]);
                }
                continue;
            }
            if (on) {
#pragma unroll
                for (int tc = 0; tc < TC; ++tc) red[(pl * TC + tc) * T + it] = gs[tc];
            }
            __syncthreads();
            const int np = min(P, ng - r0);
#pragma unroll
            for (int j = 0; j < TC; ++j)
                if (con[j])
                    for (int q0 = 0; q0 < np; q0 += 4) {         // four LDS reads in flight, added in group order
                        float4 r[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (q0 + u < np) r[u] = red[((q0 + u) * TC + ctc[j]) * T + cci[j]];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (q0 + u < np) s[j] = fin_add(s[j], r[u]);
                    }
            __syncthreads();
        }
        if (rem) {
            float4 w[3][TC];
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int j = 0; j < TC; ++j)
                    if (u < rem && con[j])
                        w[u][j] = *reinterpret_cast<const float4*>(src + (size_t)(4 * ng + u) * total + (size_t)(t0 + ctc[j]) * CC + 4 * cci[j]);
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int j = 0; j < TC; ++j)
                    if (u < rem && con[j]) s[j] = fin_add(s[j], w[u][j]);
        }
#pragma unroll
        for (int j = 0; j < TC; ++j)
            if (con[j]) {
                float* const o = tileS + (cci[j] * 4) * TC + ctc[j];
                o[0] = s[j].x; o[TC] = s[j].y; o[2 * TC] = s[j].z; o[3 * TC] = s[j].w;
            }
    }
    __syncthreads();
    float* const dst = a.dw[i] + ((size_t)g * CC + cc0) * TAPS + t0;      // TC == TAPS: the run's run * TAPS consecutive floats
    const int nf = run * TC;
    const float beta = a.beta;
    if (TC != TAPS) {                                            // a tap chunk of 49: rows of TC floats (the gradient is a few hundred KB)
        for (int q = t; q < nf; q += 256) {
            float* const d = dst + (q / TC) * TAPS + q % TC;
            *d = beta != 0.f ? *d * beta + tileS[q] : tileS[q];
        }
    } else if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const float4* const t4 = reinterpret_cast<const float4*>(tileS);
        float4* const d4 = reinterpret_cast<float4*>(dst);
        for (int q = t; q < nf / 4; q += 256) {
            float4 v = t4[q];
            if (beta != 0.f) {
                const float4 d = d4[q];
                v.x = d.x * beta + v.x; v.y = d.y * beta + v.y; v.z = d.z * beta + v.z; v.w = d.w * beta + v.w;
            }
            d4[q] = v;
        }
    } else {                                                     // a gradient view that is not 16-byte aligned: consecutive 4-byte stores
        for (int q = t; q < nf; q += 256) dst[q] = beta != 0.f ? dst[q] * beta + tileS[q] : tileS[q];
    }
}

inline int finish_tiles(int G, int CC, int taps, int lp) {
    const int L = 1024 >> lp;
    return G * ((CC + L - 1) / L) * (taps == 49 ? 7 : 1);
}
// Split lanes of a problem (log2): a lane walks up to four groups of four splits, and a problem of few elements gives the threads its
// run does not fill to the splits.  Behind 64 splits or more, a problem that would still be fewer than 64 workgroups (a 16 -> 16 layer
// behind 256 splits, a 7x7 stem behind 147) halves its runs further, down to 16 elements, while every lane keeps a group of its own.
// (Measured with the same halving for every problem of fewer than 64 workgroups -- the 96-channel layers behind 8-16 splits then go
// through the LDS rounds in smaller runs instead of one register chain -- and eight LDS reads in flight in the ordered add: the step's
// 3x3 finish launches took 385 us against 317 us; profiles/wgrad_finish_INDEX.md.)
inline int finish_lanes_log2(int G, int CC, int ms, int taps) {
    int lp = 0;
    while (lp < 4 && (16 << lp) < ms) ++lp;
    while (lp < 4 && (1024 >> (lp + 1)) >= CC) ++lp;
    while (ms >= 64 && lp < 6 && finish_tiles(G, CC, taps, lp) < 64 && (2 << lp) <= (ms >> 2)) ++lp;
    return lp;
}

// The problems waiting for one finish launch.  add() after the launch that writes the problem's partials has been issued; flush<TAPS>()
// launches what is pending (nothing: no launch).
struct FinishQueue {
    FinishArgs a;
    size_t lds, bytes;
    explicit FinishQueue(float beta) : lds(0), bytes(0) { a.n = 0; a.start[0] = 0; a.beta = beta; }
    bool full() const { return a.n == FIN_NP; }
    bool over_budget() const { return bytes >= FIN_BUDGET_BYTES; }
    // part [ms][G][taps][CC] (16-byte aligned), dw [G][CC][taps]
    int add(const float* part, float* dw, int G, int CC, int ms, int taps) {
        if (full() || !part || !dw || G < 1 || CC < 4 || CC % 4 != 0 || ms < 1 || (reinterpret_cast<uintptr_t>(part) & 15) != 0)
            return danet::fail(DANET_ERR_ARG, "wgrad finish: bad problem (%d groups, %d elements, %d splits; partials must be 16-byte aligned)", G, CC, ms);
        if (taps != 9 && taps != 49) return danet::fail(DANET_ERR_ARG, "wgrad finish: no kernel for %d taps", taps);
        const int lp = finish_lanes_log2(G, CC, ms, taps), L = 1024 >> lp, tc = taps == 49 ? 7 : taps;
        const int k = a.n++;
        a.part[k] = part; a.dw[k] = dw; a.CC[k] = CC; a.G[k] = G; a.ms[k] = ms; a.lp[k] = lp;
        a.start[k + 1] = a.start[k] + finish_tiles(G, CC, taps, lp);
        const size_t l = ((size_t)L * tc + (lp ? 256 * tc * 4 : 0)) * sizeof(float);
        if (l > lds) lds = l;
        bytes += (size_t)ms * G * taps * CC * sizeof(float);
        return DANET_OK;
    }
    template <int TAPS> int flush(hipStream_t st) {
        if (a.n == 0) return DANET_OK;
        hipLaunchKernelGGL((wgrad_finish_kernel<TAPS>), dim3((unsigned)a.start[a.n]), dim3(256), lds, st, a);
        a.n = 0; lds = 0; bytes = 0;
        DANET_CHECK_LAUNCH("wgrad_finish_kernel");
        return DANET_OK;
    }
};

}  // namespace
}  // namespace danet_conv
