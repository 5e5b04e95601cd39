// The fit kernel of kp_fit.hip and dense_fit.hip (DESIGN.md "fit rule", "the dense fit rule"), stated once.  ONE launch per fit, ONE
// workgroup of 256 threads per person, every iteration inside the kernel: the unknowns, the Adam moments and every intermediate of an
// iteration live in LDS and registers; global memory sees the read-only tables, the inputs, the outputs and the caller-owned workspace
// (written in the forward sweep and read back by the same workgroup).  No atomics, every reduction in a fixed order: a person's result
// does not depend on the other people of the batch, and two runs give the same bits.
//
//   fit_kernel<false, danet_kp_fit_args>      the keypoint fit   (kp_fit.hip)
//   fit_kernel<true, danet_dense_fit_args>    the dense fit      (dense_fit.hip)
//
// Per iteration:
//   rotations   24 lanes: 6D -> R (rot6d.h, shared with geometry.hip)
//   chain       rest joints J = J_template + J_shapedirs beta, the 24-joint chain, A_j = [Rg_j | Jp_j - Rg_j J_j]
//   forward     tiles of 128 support vertices: v_posed = v_template + basis^T f, f = (R_1..23 - I, beta) -- one lane per
//               coordinate streams its basis column (coalesced rows); skinning, one lane per vertex; landmark picks and the
//               extra joints' partial sums (tile after tile, fixed order)
//   energy      one lane per joint of the 49: projection, Geman-McClure, d/d joint and d/d cam; butterfly sums in wave order
//   reverse     the same tiles: seed per vertex, d v_posed, dA (one lane per (joint, row), vertices in order), d f = basisT g
//               (one lane per feature streams its basisT column); then the chain's reverse pass, the priors, 6D backward
//   update      Adam on the stage's groups, s clamped
// LDS does not grow with the support: the tile arrays are fixed.  Values are stored in fp32; sums are accumulated in double (with
// fp32 accumulators an 8-iteration trajectory sat at up to 6 x the error of a float32 run of the oracle, with double at 1.1 x).
//
// Only these are the dense fit's own, each behind `if constexpr (DENSE)`; everything else is one text for both:
//   1. the doubled workspace stride (v_posed of the support, then the skinned support), the LDS arrays sRed, sGl and sWl (one element
//      each in the keypoint fit, unreferenced there: its LDS stays at 42 288 bytes, the dense fit's at 56 240);
//   2. forward: the skinned tile also goes to the workspace;
//   3. energy: a landmark's three corners may fall in different tiles, so its point is made after the sweep: a lane per landmark (lane t
//      takes landmarks t, t + 256, ...; M <= 864) gathers the corners from the workspace and adds w0 v0 + w1 v1 + w2 v2 in double, in
//      that order.  (Carrying the corners, weights and partial sums in registers through the sweep instead cost 60 VGPRs in the
//      streaming loops, which then ran at 1.6 ms per iteration: DESIGN.md.)  At x_0 the gate is decided from the same corners (the
//      texture rule's facing test), once, and held.  Then projection, Geman-McClure with sigma_dense, d/d point into LDS (sGl), the
//      lane's share of E and d/d cam in registers (eL, gcL);
//   4. the sum of E and d/d cam.  The two fits sum in different orders and tests pin both: the keypoint fit's wave 0 takes
//      sE[lane] + sE[lane + 64] and waves 1-3 take sGc; the dense fit sums its 256 lanes together with the 49 keypoint lanes by a
//      butterfly per wave, then the four waves in order (sRed);
//   5. reverse: a vertex's seed adds w * sGl[l] over the vertex -> (landmark, weight) CSR, ascending landmark.
// Fields that only danet_dense_fit_args has are read inside those blocks alone.  The body is the kernel itself and not a device
// function called from two kernels: inlined that way the streaming loops unrolled differently and the registers ran over into AGPRs.
#pragma once
#include <type_traits>
#include "common.h"
#include "rot6d.h"

namespace danet_fit {

constexpr int NJ = 24;
constexpr int NPB = 207;
constexpr int NT = 256;
constexpr int TV = 128;            // support vertices per tile
constexpr int TC = TV * 3;
constexpr int WPAD = 25;
constexpr int NB_MAX = 16;
constexpr int NE_MAX = 16;
constexpr int NL_MAX = 32;
constexpr int NKP = 224;           // padded feature count (207 + NB_MAX = 223)
constexpr int NJ_MAX = NJ + NL_MAX + NE_MAX;
constexpr int NXP = 3 + NB_MAX + 144 + 1;
constexpr int NK49 = 49;
constexpr int M_MAX = 864;         // 24 G^2, G <= 6
#ifndef KP_UNROLL
#define KP_UNROLL 16             // rows of the basis in flight per lane in the streaming loops (measured at P = 8 / 32: 8 -> 126 us per iteration, 16 -> 120, 32 -> 285)
#endif

__device__ __forceinline__ double wave_sum(double v) {        // every lane ends with the same sum, in a fixed order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool DENSE, typename Args>
__global__ __launch_bounds__(NT) void fit_kernel(const Args a)
{
    const int p = blockIdx.x, t = threadIdx.x;
    const int NB = a.NB, NL = a.NL, NE = a.NE, NK = NPB + NB, NX = 3 + NB + 144, OA = 3 + NB, PW = 3 + NB + 216;
    const int NJ54 = NJ + NL + NE, T = a.T;
    const size_t S3p = (size_t)a.Sp * 3;
    const int ntiles = a.Sp / TV;
    const float* __restrict__ row = a.para + (size_t)p * PW;
    float* ws = a.ws + (size_t)p * (DENSE ? 2 : 1) * S3p;  // v_posed of the support; DENSE: then the skinned support
    float* wsv = ws + S3p;
    int M = 0;                                              // DENSE: the landmarks
    if constexpr (DENSE) M = a.M;

    __shared__ float sx[NXP], sm[NXP], sv[NXP], sxb[NXP], sg[NXP];
    __shared__ float sB0[NB_MAX];
    __shared__ float sR0[216], sR[216], sRg[216], sJ[72], sJp[72];
    __shared__ __attribute__((aligned(16))) float sA[288];
    __shared__ float sF[NKP];
    __shared__ float sJ54[NJ_MAX * 3], sGj[NJ_MAX * 3];
    __shared__ float sKp[NK49 * 3], sG49[NK49 * 3];
    __shared__ int sMap[NK49], sLm[NL_MAX], sPar[NJ];
    __shared__ float sE[128], sGc[3][64], sScal[4];
    __shared__ double sRed[DENSE ? 4 : 1][4];
    __shared__ float gRg[216], gR[216], gJp[72], gJ[72], gtt[72], gF[NKP];
    __shared__ float sVp[TC], sVt[TC], sGvp[TC];            // tile: v_posed, skinned vertex / its seed, d v_posed
    __shared__ float sJx[NE_MAX][TV];
    __shared__ float sW[TV][WPAD];
    __shared__ float sGl[DENSE ? M_MAX * 3 : 1];             // d E / d landmark point
    __shared__ float sWl[DENSE ? M_MAX : 1];                 // w_dense (g c)^2 of every landmark, set at x_0

    // ---- inputs ------------------------------------------------------------------------------------------------------------------
    if (t < NX) {
        float v;
        if (t < OA) v = row[t];
        else { const int q = t - OA, j = q / 6, e = q - j * 6; v = row[OA + j * 9 + (e >> 1) * 3 + (e & 1)]; }     // first two columns, [3,2] row-major
        sx[t] = v;
    }
    if (t < NB) sB0[t] = row[3 + t];
    for (int i = t; i < NK49 * 3; i += NT) sKp[i] = a.kp[(size_t)p * NK49 * 3 + i];
    if (t < NK49) sMap[t] = a.jmap[t];
    if (t < NL_MAX) sLm[t] = t < NL ? a.lm[t] : -1;
    if (t < NJ) sPar[t] = a.parents[t];
    if (t < 128) sE[t] = 0.f;
    if (t < 192) sGc[t >> 6][t & 63] = 0.f;
    const float* __restrict__ obs = nullptr;                // DENSE: this person's observations of the landmarks
    if constexpr (DENSE) obs = a.obs + (size_t)p * M * 3;
    __syncthreads();
    const float s0 = sx[0];

    float bestE = 0.f;
    int besti = 0, status = 0, it = 0;
    for (int st = 0; st <= a.nstages && !status; ++st) {
        const bool last = st == a.nstages;
        const int n = last ? 1 : a.stage_iters[st], mask = last ? 0 : a.stage_mask[st];
        if (t < NXP) { sm[t] = 0.f; sv[t] = 0.f; }
        double b1p = 1.0, b2p = 1.0;          // beta^step in double: 1 - 0.999^k in fp32 loses four digits to cancellation
        for (int k = 0; k < n; ++k, ++it) {
            const bool need_grad = !last || (a.grad0 && it == 0);
            // ---- rotations, features, rest joints ---------------------------------------------------------------------------------
            if (t < NJ) danet::rot6d_fwd(&sx[OA + t * 6], &sR[t * 9]);
            __syncthreads();
            if (it == 0 && t < 216) sR0[t] = sR[t];
            if (t < NKP) {
                float f = 0.f;
                if (t < NPB) { const int e = t % 9; f = sR[9 + t] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f); }
                else if (t < NK) f = sx[3 + t - NPB];
                sF[t] = f;
            }
            if (t < 72) {
                double s = a.J_template[t];
                for (int l = 0; l < NB; ++l) s += (double)a.J_shapedirs[t * NB + l] * sx[3 + l];
                sJ[t] = (float)s;
            }
            __syncthreads();
            // ---- chain (the recurrence of smpl_prep_kernel / smpl_fused_fwd_kernel in smpl_lbs.hip, one item, sums in double: keep in step) ----
            for (int i = 0; i < NJ; ++i) {
                const int pa = sPar[i];
                if (t < 9) {
                    const int r = t / 3, cc = t - r * 3;
                    sRg[i * 9 + t] = pa < 0 ? sR[i * 9 + t]
                                            : (float)((double)sRg[pa * 9 + r * 3 + 0] * sR[i * 9 + 0 + cc] + (double)sRg[pa * 9 + r * 3 + 1] * sR[i * 9 + 3 + cc] +
                                                      (double)sRg[pa * 9 + r * 3 + 2] * sR[i * 9 + 6 + cc]);
                } else if (t < 12) {
                    const int r = t - 9;
                    double s;
                    if (pa < 0) s = sJ[i * 3 + r];
                    else {
                        s = sJp[pa * 3 + r];
                        for (int m = 0; m < 3; ++m) s += (double)sRg[pa * 9 + r * 3 + m] * ((double)sJ[i * 3 + m] - (double)sJ[pa * 3 + m]);
                    }
                    sJp[i * 3 + r] = (float)s;
                }
                __syncthreads();
            }
            for (int idx = t; idx < 288; idx += NT) {
                const int j = idx / 12, e = idx - j * 12, r = e / 4, cc = e - r * 4;
                double v;
                if (cc < 3) v = sRg[j * 9 + r * 3 + cc];
                else {
                    v = sJp[j * 3 + r];
                    for (int m = 0; m < 3; ++m) v -= (double)sRg[j * 9 + r * 3 + m] * sJ[j * 3 + m];
                }
                sA[idx] = (float)v;
            }
            if (t < 72) sJ54[t] = sJp[t];
            __syncthreads();
            // ---- forward sweep over the support ------------------------------------------------------------------------------------
            double jacc = 0.0;
            for (int tile = 0; tile < ntiles; ++tile) {
                const int v0 = tile * TV;
                const size_t c0 = (size_t)v0 * 3;
                for (int i = t; i < NE * TV; i += NT) { const int e = i / TV, vv = i - e * TV; sJx[e][vv] = a.jx[(size_t)e * a.Sp + v0 + vv]; }
                for (int i = t; i < TV * NJ; i += NT) { const int vv = i / NJ, j = i - vv * NJ; sW[vv][j] = a.weights[(size_t)v0 * NJ + i]; }
                for (int c = t; c < TC; c += NT) {
                    const float* col = a.basis + c0 + c;
                    double s = a.v_template[c0 + c];
#pragma unroll KP_UNROLL
                    for (int q = 0; q < NK; ++q) s += (double)col[(size_t)q * S3p] * sF[q];
                    sVp[c] = (float)s;
                    ws[c0 + c] = (float)s;
                }
                __syncthreads();
                if (t < TV) {
                    double Tm[12];
#pragma unroll
                    for (int e = 0; e < 12; ++e) Tm[e] = 0.0;
                    for (int j = 0; j < NJ; ++j) {
                        const double w = sW[t][j];
                        const float4* a4 = reinterpret_cast<const float4*>(&sA[j * 12]);
#pragma unroll
                        for (int e4 = 0; e4 < 3; ++e4) {
                            const float4 q = a4[e4];
                            Tm[e4 * 4 + 0] += w * q.x; Tm[e4 * 4 + 1] += w * q.y; Tm[e4 * 4 + 2] += w * q.z; Tm[e4 * 4 + 3] += w * q.w;
                        }
                    }
                    const double x = sVp[t * 3 + 0], y = sVp[t * 3 + 1], z = sVp[t * 3 + 2];
#pragma unroll
                    for (int r = 0; r < 3; ++r) sVt[t * 3 + r] = (float)(Tm[r * 4 + 0] * x + Tm[r * 4 + 1] * y + Tm[r * 4 + 2] * z + Tm[r * 4 + 3]);
                }
                __syncthreads();
                if constexpr (DENSE)
                    for (int c = t; c < TC; c += NT) wsv[c0 + c] = sVt[c];
                if (t < NE * 3) {
                    const int e = t / 3, kk = t - e * 3;
                    double s = 0.0;
#pragma unroll KP_UNROLL
                    for (int vv = 0; vv < TV; ++vv) s += (double)sJx[e][vv] * sVt[vv * 3 + kk];
                    jacc += s;
                } else if (t >= 64 && t < 64 + NL) {
                    const int l = t - 64, li = sLm[l] - v0;
                    if (li >= 0 && li < TV)
                        for (int kk = 0; kk < 3; ++kk) sJ54[(NJ + l) * 3 + kk] = sVt[li * 3 + kk];
                }
                __syncthreads();
            }
            if (t < NE * 3) sJ54[(NJ + NL) * 3 + t] = (float)jacc;
            __syncthreads();                  // (DENSE also: the skinned support in the workspace is visible to the workgroup)
            // ---- energy -----------------------------------------------------------------------------------------------------------
            double eL = 0.0, gcL[3] = {0.0, 0.0, 0.0};          // DENSE: the lane's landmarks' share of E and d/d cam
            {
                const double s = sx[0], tx = sx[1], ty = sx[2];
                const double den = (double)a.res * s + 1e-9;
                const double tz = 2.0 * a.focal / den, kap = a.kappa, sg2 = (double)a.sigma * a.sigma;
                const double dz_ds = -2.0 * a.focal * a.res / (den * den);
                if constexpr (DENSE) {
                    const double sd2 = (double)a.sigma_dense * a.sigma_dense;
                    for (int l = t; l < M; l += NT) {           // the lane's landmarks: the point from its three corners, in their order
                        double c3[3][3], lp[3] = {0.0, 0.0, 0.0};
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float* v = wsv + (size_t)a.lm_corner[l * 3 + c] * 3;
                            const double w = a.lm_w[l * 3 + c];
                            c3[c][0] = v[0]; c3[c][1] = v[1]; c3[c][2] = v[2];
                            lp[0] += w * c3[c][0]; lp[1] += w * c3[c][1]; lp[2] += w * c3[c][2];
                        }
                        if (it == 0) {            // the gate, once: the texture rule's facing test on the landmark's face at x_0
                            const double t0x = c3[0][0] + tx, t0y = c3[0][1] + ty, t0z = c3[0][2] + tz;
                            const double e1x = (c3[1][0] + tx) - t0x, e1y = (c3[1][1] + ty) - t0y, e1z = (c3[1][2] + tz) - t0z;
                            const double e2x = (c3[2][0] + tx) - t0x, e2y = (c3[2][1] + ty) - t0y, e2z = (c3[2][2] + tz) - t0z;
                            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                            const double Px = lp[0] + tx, Py = lp[1] + ty, Pz = lp[2] + tz;
                            const double nl = sqrt(nx * nx + ny * ny + nz * nz), pl = sqrt(Px * Px + Py * Py + Pz * Pz);
                            const bool g = nl > 0.0 && pl > 0.0 && -(nx * Px + ny * Py + nz * Pz) / (nl * pl) > (double)a.min_cos;
                            a.gate[(size_t)p * M + l] = g ? 1 : 0;
                            const float c = obs[l * 3 + 2];
                            sWl[l] = g ? a.w_dense * (c * c) : 0.f;            // w_dense (g c)^2, read by this lane alone
                        }
                        const double D = lp[2] + tz;
                        const double w = sWl[l];
                        double gX = 0.0, gY = 0.0, gZ = 0.0;
                        if (!(D <= 1e-6)) {
                            const double u = kap * (lp[0] + tx) / D, v = kap * (lp[1] + ty) / D;
                            const double eu = u - (double)obs[l * 3 + 0], ev = v - (double)obs[l * 3 + 1];
                            const double r2 = eu * eu + ev * ev;
                            const double qq = sd2 + r2;
                            eL += w * (sd2 * r2 / qq);
                            const double dr = w * (sd2 / qq) * (sd2 / qq) * 2.0;
                            const double gu = dr * eu, gv = dr * ev;
                            gX = gu * kap / D;
                            gY = gv * kap / D;
                            gZ = -(gu * u + gv * v) / D;
                            gcL[0] += gZ * dz_ds; gcL[1] += gX; gcL[2] += gY;
                        }
                        sGl[l * 3 + 0] = (float)gX; sGl[l * 3 + 1] = (float)gY; sGl[l * 3 + 2] = (float)gZ;
                    }
                }
                if (t < NK49) {
                    const int j = sMap[t];
                    const double X = sJ54[j * 3 + 0], Y = sJ54[j * 3 + 1], Z = sJ54[j * 3 + 2];
                    const double D = Z + tz;
                    const double c = sKp[t * 3 + 2];
                    double E = 0.0, gX = 0.0, gY = 0.0, gZ = 0.0;
                    if (!(D <= 1e-6)) {           // (a NaN depth is NOT skipped: it makes E(x_0) non-finite, status 1)
                        const double u = kap * (X + tx) / D, v = kap * (Y + ty) / D;
                        const double eu = u - (double)sKp[t * 3 + 0], ev = v - (double)sKp[t * 3 + 1];
                        const double r2 = eu * eu + ev * ev;
                        const double q = sg2 + r2;
                        const double c2 = c * c;
                        E = c2 * (sg2 * r2 / q);
                        const double dr = c2 * (sg2 / q) * (sg2 / q) * 2.0;      // c^2 rho'(r2) 2
                        const double gu = dr * eu, gv = dr * ev;
                        gX = gu * kap / D;
                        gY = gv * kap / D;
                        gZ = -(gu * u + gv * v) / D;
                    }
                    sE[t] = (float)E;
                    sG49[t * 3 + 0] = (float)gX; sG49[t * 3 + 1] = (float)gY; sG49[t * 3 + 2] = (float)gZ;
                    sGc[0][t] = (float)(gZ * dz_ds);
                    sGc[1][t] = (float)gX;
                    sGc[2][t] = (float)gY;
                } else if (t >= 64 && t < 64 + NJ) {
                    const int j = t - 64;
                    float s2 = 0.f;
#pragma unroll
                    for (int e = 0; e < 9; ++e) { const float d = sR[j * 9 + e] - sR0[j * 9 + e]; s2 += d * d; }
                    sE[t] = (j == 0 ? a.w_orient : a.w_pose) * s2;
                } else if (t == 96) {
                    float s2 = 0.f;
                    for (int l = 0; l < NB; ++l) { const float d = sx[3 + l] - sB0[l]; s2 += d * d; }
                    sE[t] = a.w_shape * s2;
                }
            }
            __syncthreads();
            {
                const int w = t >> 6, lane = t & 63;
                if constexpr (DENSE) {
                    const double vE = wave_sum((t < 128 ? (double)sE[t] : 0.0) + eL);
                    const double v0 = wave_sum((w == 0 ? (double)sGc[0][lane] : 0.0) + gcL[0]);
                    const double v1 = wave_sum((w == 0 ? (double)sGc[1][lane] : 0.0) + gcL[1]);
                    const double v2 = wave_sum((w == 0 ? (double)sGc[2][lane] : 0.0) + gcL[2]);
                    if (lane == 0) { sRed[w][0] = vE; sRed[w][1] = v0; sRed[w][2] = v1; sRed[w][3] = v2; }
                    __syncthreads();
                    if (t < 4) sScal[t] = (float)(((sRed[0][t] + sRed[1][t]) + sRed[2][t]) + sRed[3][t]);
                } else {
                    const double v = w == 0 ? (double)sE[lane] + (double)sE[lane + 64] : (double)sGc[w - 1][lane];
                    const double s = wave_sum(v);
                    if (lane == 0) sScal[w] = (float)s;
                }
            }
            __syncthreads();
            const float E = sScal[0];
            if (t == 0) a.history[(size_t)p * (T + 1) + it] = E;
            const bool fin = __builtin_isfinite(E);
            if (it == 0 && !fin) { status = 1; break; }
            if (fin && (it == 0 || E < bestE)) {
                bestE = E; besti = it;
                if (t < NX) sxb[t] = sx[t];
            }
            if (!need_grad) continue;
            // ---- d joints54: the 49 gathered back in the map's order --------------------------------------------------------------
            if (t < NJ54 * 3) {
                const int j = t / 3, kk = t - j * 3;
                double s = 0.0;
                for (int q = 0; q < NK49; ++q)
                    if (sMap[q] == j) s += sG49[q * 3 + kk];
                sGj[t] = (float)s;
            }
            __syncthreads();
            // ---- reverse sweep over the support -----------------------------------------------------------------------------------
            double accA[4] = {0.0, 0.0, 0.0, 0.0};
            double accF = 0.0;
            for (int tile = 0; tile < ntiles; ++tile) {
                const int v0 = tile * TV;
                const size_t c0 = (size_t)v0 * 3;
                for (int i = t; i < NE * TV; i += NT) { const int e = i / TV, vv = i - e * TV; sJx[e][vv] = a.jx[(size_t)e * a.Sp + v0 + vv]; }
                for (int i = t; i < TV * NJ; i += NT) { const int vv = i / NJ, j = i - vv * NJ; sW[vv][j] = a.weights[(size_t)v0 * NJ + i]; }
                for (int c = t; c < TC; c += NT) sVp[c] = ws[c0 + c];
                __syncthreads();
                if (t < TV) {
                    double g[3] = {0.0, 0.0, 0.0};
                    for (int l = 0; l < NL; ++l)
                        if (sLm[l] - v0 == t) { g[0] += sGj[(NJ + l) * 3 + 0]; g[1] += sGj[(NJ + l) * 3 + 1]; g[2] += sGj[(NJ + l) * 3 + 2]; }
                    for (int e = 0; e < NE; ++e) {
                        const double w = sJx[e][t];
                        g[0] += w * sGj[(NJ + NL + e) * 3 + 0]; g[1] += w * sGj[(NJ + NL + e) * 3 + 1]; g[2] += w * sGj[(NJ + NL + e) * 3 + 2];
                    }
                    if constexpr (DENSE) {
                        const int q0 = a.csr_off[v0 + t], q1 = a.csr_off[v0 + t + 1];
                        for (int q = q0; q < q1; ++q) {             // the vertex's landmarks, ascending
                            const int l = a.csr_lm[q];
                            const double w = a.csr_w[q];
                            g[0] += w * sGl[l * 3 + 0]; g[1] += w * sGl[l * 3 + 1]; g[2] += w * sGl[l * 3 + 2];
                        }
                    }
                    double Tm[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) Tm[e] = 0.0;
                    for (int j = 0; j < NJ; ++j) {
                        const double w = sW[t][j];
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int cc = 0; cc < 3; ++cc) Tm[r * 3 + cc] += w * sA[j * 12 + r * 4 + cc];
                    }
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) sGvp[t * 3 + cc] = (float)(Tm[0 * 3 + cc] * g[0] + Tm[1 * 3 + cc] * g[1] + Tm[2 * 3 + cc] * g[2]);
                    sVt[t * 3 + 0] = (float)g[0]; sVt[t * 3 + 1] = (float)g[1]; sVt[t * 3 + 2] = (float)g[2];
                }
                __syncthreads();
                if (t < 72) {                       // dA: lane (joint, row), the tile's vertices in order
                    const int j = t / 3, r = t - j * 3;
                    for (int vv = 0; vv < TV; ++vv) {
                        const double wg = (double)sW[vv][j] * sVt[vv * 3 + r];
                        accA[0] += wg * sVp[vv * 3 + 0]; accA[1] += wg * sVp[vv * 3 + 1]; accA[2] += wg * sVp[vv * 3 + 2]; accA[3] += wg;
                    }
                }
                if (t < NKP) {                      // d f: lane per feature, the tile's coordinates in order (basisT rows are coalesced)
                    const float* colT = a.basisT + c0 * NKP + t;
#pragma unroll KP_UNROLL
                    for (int c = 0; c < TC; ++c) accF += (double)colT[(size_t)c * NKP] * sGvp[c];
                }
                __syncthreads();
            }
            if (t < 72) {
                const int j = t / 3, r = t - j * 3;
                gRg[j * 9 + r * 3 + 0] = (float)accA[0]; gRg[j * 9 + r * 3 + 1] = (float)accA[1]; gRg[j * 9 + r * 3 + 2] = (float)accA[2];
                gtt[t] = (float)accA[3];
            }
            if (t < NKP) gF[t] = (float)accF;
            __syncthreads();
            // ---- the chain's reverse pass (tt_j = Jp_j - Rg_j J_j; finalize_bwd_body of smpl_lbs.hip, sums in double: keep in step) ------
            if (t < 216) {
                const int j = t / 9, r = (t % 9) / 3, cc = t % 3;
                gRg[t] -= gtt[j * 3 + r] * sJ[j * 3 + cc];
            }
            if (t < 72) {
                const int j = t / 3, cc = t - j * 3;
                gJ[t] = -(sRg[j * 9 + 0 + cc] * gtt[j * 3 + 0] + sRg[j * 9 + 3 + cc] * gtt[j * 3 + 1] + sRg[j * 9 + 6 + cc] * gtt[j * 3 + 2]);
                gJp[t] = sGj[t] + gtt[t];
            }
            __syncthreads();
            for (int i = NJ - 1; i >= 1; --i) {
                const int pa = sPar[i];
                if (t < 9) {
                    const int r = t / 3, cc = t - r * 3;
                    double s = 0.0, s2 = 0.0;
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        s += (double)sRg[pa * 9 + m * 3 + r] * gRg[i * 9 + m * 3 + cc];
                        s2 += (double)gRg[i * 9 + r * 3 + m] * sR[i * 9 + cc * 3 + m];
                    }
                    gR[i * 9 + t] = (float)s;
                    gRg[pa * 9 + t] = (float)((double)gRg[pa * 9 + t] + s2 + (double)gJp[i * 3 + r] * ((double)sJ[i * 3 + cc] - (double)sJ[pa * 3 + cc]));
                } else if (t < 12) {
                    const int cc = t - 9;
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 3; ++m) s += (double)sRg[pa * 9 + m * 3 + cc] * gJp[i * 3 + m];
                    gJ[i * 3 + cc] = (float)(gJ[i * 3 + cc] + s);
                    gJ[pa * 3 + cc] = (float)(gJ[pa * 3 + cc] - s);
                    gJp[pa * 3 + cc] += gJp[i * 3 + cc];
                }
                __syncthreads();
            }
            if (t < 9) gR[t] = gRg[t];
            if (t < 3) gJ[t] += gJp[t];
            __syncthreads();
            // ---- pose features, priors, 6D backward ---------------------------------------------------------------------------------
            if (t < 216) {
                const float w2 = 2.f * (t < 9 ? a.w_orient : a.w_pose);
                gR[t] += (t >= 9 ? gF[t - 9] : 0.f) + w2 * (sR[t] - sR0[t]);
            }
            if (t < NB) {
                double s = gF[NPB + t] + 2.0 * a.w_shape * ((double)sx[3 + t] - (double)sB0[t]);
                for (int i = 0; i < 72; ++i) s += (double)a.J_shapedirs[i * NB + t] * gJ[i];
                sg[3 + t] = (float)s;
            }
            if (t >= 64 && t < 67) sg[t - 64] = sScal[1 + t - 64];
            __syncthreads();
            if (t < NJ) danet::rot6d_bwd(&sx[OA + t * 6], &gR[t * 9], &sg[OA + t * 6]);
            __syncthreads();
            if (a.grad0 && it == 0 && t < NX) a.grad0[(size_t)p * NX + t] = sg[t];
            if (last) continue;
            // ---- Adam on the stage's groups ----------------------------------------------------------------------------------------
            b1p *= 0.9; b2p *= 0.999;
            const float bc1 = (float)(1.0 - b1p), bc2 = (float)(1.0 - b2p);
            if (t < NX) {
                const int grp = t < 3 ? 1 : t < OA ? 8 : t < OA + 6 ? 2 : 4;
                if (mask & grp) {
                    const float g = sg[t];
                    const float m = 0.9f * sm[t] + 0.1f * g;
                    const float v = 0.999f * sv[t] + 0.001f * g * g;
                    sm[t] = m; sv[t] = v;
                    const float mh = m / bc1, vh = v / bc2;
                    float x = sx[t] - a.lr * mh / (sqrtf(vh) + 1e-8f);
                    if (t == 0) x = fmaxf(x, 0.1f * s0);
                    sx[t] = x;
                }
            }
            __syncthreads();
        }
    }
    // ---- outputs -----------------------------------------------------------------------------------------------------------------
    __syncthreads();                // (the best iterate's lanes have written it)
    float* out = a.para_fit + (size_t)p * PW;
    if (status || besti == 0) {
        for (int i = t; i < PW; i += NT) out[i] = row[i];
    } else {
        if (t < OA) out[t] = sxb[t];
        if (t < NJ) {
            float Rm[9];
            danet::rot6d_fwd(&sxb[OA + t * 6], Rm);
#pragma unroll
            for (int e = 0; e < 9; ++e) out[OA + t * 9 + e] = Rm[e];
        }
    }
    if (status) {
        for (int i = 1 + t; i <= T; i += NT) a.history[(size_t)p * (T + 1) + i] = __builtin_nanf("");
        if (a.grad0 && t < NX) a.grad0[(size_t)p * NX + t] = 0.f;
    }
    if (t == 0) { a.best_iter[p] = besti; a.status[p] = status; }
}

// The argument checks of danet_kp_fit and danet_dense_fit; the first that fails is the one reported.  `op` opens every message
// ("kp_fit", "dense_fit").  The dense arguments' own fields (M, the landmark tables, sigma_dense) are checked at their place in that
// order, which callers' messages depend on; the w_dense check follows in dense_fit.hip.
template <typename Args>
int fit_check_args(const char* op, const Args* a)
{
    constexpr bool DENSE = std::is_same_v<Args, danet_dense_fit_args>;
    DANET_CHECK_ARG(a, "%s: null arguments", op);
    DANET_CHECK_ARG(a->P > 0, "%s: P=%d", op, a->P);
    DANET_CHECK_ARG(a->NB >= 1 && a->NB <= NB_MAX, "%s: NB=%d unsupported (1..%d)", op, a->NB, NB_MAX);
    DANET_CHECK_ARG(a->NL >= 0 && a->NL <= NL_MAX && a->NE >= 0 && a->NE <= NE_MAX, "%s: NL=%d NE=%d unsupported", op, a->NL, a->NE);
    DANET_CHECK_ARG(a->S >= 1 && a->Sp >= a->S && a->Sp % TV == 0, "%s: S=%d Sp=%d (Sp: a multiple of %d, >= S)", op, a->S, a->Sp, TV);
    if constexpr (DENSE) DANET_CHECK_ARG(a->M >= 1 && a->M <= M_MAX, "%s: M=%d (1..%d)", op, a->M, M_MAX);
    DANET_CHECK_ARG(a->nstages >= 0 && a->nstages <= 4, "%s: %d stages (0..4)", op, a->nstages);
    long total = 0;
    for (int i = 0; i < a->nstages; ++i) {
        DANET_CHECK_ARG(a->stage_iters[i] >= 0 && a->stage_iters[i] <= 100000 && a->stage_mask[i] >= 0 && a->stage_mask[i] < 16,
                        "%s: stage %d: %d iterations, groups %d", op, i, a->stage_iters[i], a->stage_mask[i]);
        total += a->stage_iters[i];
    }
    DANET_CHECK_ARG(total == a->T, "%s: T=%d, the stages sum to %ld", op, a->T, total);
    DANET_CHECK_ARG(a->para && a->kp && a->J_template && a->J_shapedirs && a->parents && a->v_template && a->basis && a->basisT &&
                    a->weights && a->jmap && a->ws && a->para_fit && a->history && a->best_iter && a->status, "%s: null pointer", op);
    DANET_CHECK_ARG((a->NE == 0 || a->jx) && (a->NL == 0 || a->lm), "%s: joint tables missing", op);
    if constexpr (DENSE) {
        DANET_CHECK_ARG(a->lm_corner && a->lm_w && a->csr_off && a->csr_lm && a->csr_w && a->obs && a->gate, "%s: landmark tables, obs or gate missing", op);
        DANET_CHECK_ARG(a->sigma > 0.f && a->sigma_dense > 0.f && a->res > 0.f && a->focal > 0.f,
                        "%s: sigma, sigma_dense, res and focal must be positive", op);
    } else {
        DANET_CHECK_ARG(a->sigma > 0.f && a->res > 0.f && a->focal > 0.f, "%s: sigma, res and focal must be positive", op);
    }
    return DANET_OK;
}

}  // namespace danet_fit
