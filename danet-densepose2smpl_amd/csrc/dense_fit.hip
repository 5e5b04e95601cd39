// Dense fit for gfx950 (DESIGN.md "the dense fit rule"): SMPL rows refined on the predicted IUV image, alone or together with 2D
// keypoints.  Two kernels.
//
// dense_landmarks_kernel   the observation: for each landmark (a mapped texel of the texel map at T = G) the Gaussian-weighted
//                          mean position of the pixels of its part whose (U, V) lie near the landmark's chart coordinate.  One
//                          wave per landmark; lane k takes pixels k, k + 64, ... in raster order, the lanes are summed by a
//                          butterfly: a fixed order, double arithmetic, no atomics, nothing shared between people.
// fit_kernel<true, danet_dense_fit_args>   the fit: the keypoint fit's kernel (fit_kernel.h: ONE launch per fit, ONE workgroup of 256
//                          per person, every iteration inside) with the dense term switched on.  fit_kernel.h lists what that adds to
//                          an iteration; the rest is the one text kp_fit.hip launches as fit_kernel<false, danet_kp_fit_args>.
// The landmark tables stay in global memory (read-only, a few KB, cached); LDS holds what the keypoint fit holds plus the landmark
// seeds and weights, 56 240 bytes in all: no opt-in.  Values are stored in fp32, sums are accumulated in double.
#include "fit_kernel.h"

using namespace danet_fit;

namespace {

// ---- the observation ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void dense_landmarks_kernel(const float* __restrict__ iuv, const int32_t* __restrict__ cell, int P, int M,
                                                             int S, int G, double tau, double w_min, float* __restrict__ obs,
                                                             float* __restrict__ wsum)
{
    const int l = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = blockIdx.y;
    if (l >= M) return;                                       // (whole waves leave; there is no barrier below)
    const int part = cell[l * 3 + 0];
    const double ul = ((double)cell[l * 3 + 2] + 0.5) / (double)G, vl = ((double)cell[l * 3 + 1] + 0.5) / (double)G;
    const size_t SS = (size_t)S * S;
    const float* pi = iuv + (size_t)p * 3 * SS;
    const float* pu = pi + SS;
    const float* pv = pu + SS;
    const double t2 = tau * tau, cut = 9.0 * t2, inv = 1.0 / (2.0 * t2), px = 2.0 / (double)S;
    double W = 0.0, sx = 0.0, sy = 0.0;
    for (size_t q = lane; q < SS; q += 64) {
        double pf = floor(24.0 * (double)pi[q] + 0.5);
        pf = pf < 0.0 ? 0.0 : (pf > 24.0 ? 24.0 : pf);        // (a NaN compares false twice and matches no part)
        if (pf != (double)part) continue;
        const double du = (double)pu[q] - ul, dv = (double)pv[q] - vl;
        const double d2 = du * du + dv * dv;
        if (!(d2 <= cut)) continue;
        const double w = exp(-d2 * inv);
        const int r = (int)(q / S), c = (int)(q - (size_t)r * S);
        W += w;
        sx += w * (((double)c + 0.5) * px - 1.0);
        sy += w * (((double)r + 0.5) * px - 1.0);
    }
    W = wave_sum(W); sx = wave_sum(sx); sy = wave_sum(sy);
    if (lane == 0) {
        const bool ok = W >= w_min;
        float* o = obs + ((size_t)p * M + l) * 3;
        o[0] = ok ? (float)(sx / W) : 0.f;
        o[1] = ok ? (float)(sy / W) : 0.f;
        o[2] = ok ? (float)(W < 1.0 ? W : 1.0) : 0.f;
        if (wsum) wsum[(size_t)p * M + l] = (float)W;
    }
}

}  // namespace

extern "C" int danet_dense_landmarks(const float* iuv, const int32_t* cell, int P, int M, int S, int G, double tau, double w_min,
                                     float* obs, float* wsum, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(P > 0 && P <= 65535, "dense_landmarks: P=%d (1..65535)", P);
    DANET_CHECK_ARG(G >= 2 && G <= 6, "dense_landmarks: G=%d (2..6)", G);
    DANET_CHECK_ARG(M >= 1 && M <= 24 * G * G, "dense_landmarks: M=%d (1..%d at G=%d)", M, 24 * G * G, G);
    DANET_CHECK_ARG(S >= 1 && S <= 4096, "dense_landmarks: S=%d (1..4096)", S);
    DANET_CHECK_ARG(iuv && cell && obs, "dense_landmarks: null pointer");
    DANET_CHECK_ARG(tau > 0.0 && w_min > 0.0, "dense_landmarks: tau and w_min must be positive");
    hipLaunchKernelGGL(dense_landmarks_kernel, dim3(danet::cdiv(M, NT / 64), P), dim3(NT), 0, (hipStream_t)stream, iuv, cell, P, M, S, G, tau,
                       w_min, obs, wsum);
    DANET_CHECK_LAUNCH("dense_landmarks_kernel");
    return DANET_OK;
}

extern "C" size_t danet_dense_fit_ws_floats(int P, int Sp) {
    return P > 0 && Sp > 0 ? (size_t)P * (size_t)Sp * 6 : 0;
}

extern "C" int danet_dense_fit(const danet_dense_fit_args* a, size_t ws_floats, void* stream)
{
    DANET_ENTER();
    if (const int e = fit_check_args("dense_fit", a)) return e;
    DANET_CHECK_ARG(a->w_dense >= 0.f, "dense_fit: w_dense=%g", (double)a->w_dense);
    if (ws_floats < danet_dense_fit_ws_floats(a->P, a->Sp))
        return danet::fail(DANET_ERR_WORKSPACE, "dense_fit: workspace %zu < %zu floats", ws_floats, danet_dense_fit_ws_floats(a->P, a->Sp));
    hipLaunchKernelGGL((fit_kernel<true, danet_dense_fit_args>), dim3(a->P), dim3(NT), 0, (hipStream_t)stream, *a);
    DANET_CHECK_LAUNCH("fit_kernel<true, danet_dense_fit_args> (dense_fit)");
    return DANET_OK;
}
