// The temporal layer for gfx950 (DESIGN.md 4b'-track "the track rule"; tracks.py is the caller): a confidence-weighted smoother
// over the rows of a track, and the acceleration measure.
//
//   track_factor    one lane per (track, lam group), sequential in t: the banded L D L^T factor of the pentadiagonal normal
//                   equations.  The factor depends on (track, lam pair, conf) only, so it is computed once and stored (l1, l2, D:
//                   3 N doubles per group), not once per channel.
//   track_solve     one lane per (track, channel), sequential in t; the lanes of a wave take adjacent channels of the same row,
//                   so every step's load and store is one coalesced access and the factor is a broadcast load.  Three passes:
//                   the weighted mean in ascending t, the forward pass in ascending t (z kept in the workspace, N C doubles),
//                   the back substitution in descending t.  Double inside, rounded to fp32 once.
//   track_rot       the para form only: one lane per (row, joint) takes the six rounded numbers of the joint, which track_solve
//                   left in the first two columns of the output matrix, through danet::rot6d_fwd.
//   track_accel     one wave per track: the mean norm of the second difference, per-lane double partials over a fixed set of
//                   (row, joint) pairs, then a fixed shuffle tree.
//
// No grid barrier, no atomics; a lane reads only its own track's rows, so a track's result does not depend on its neighbours in the
// launch, and two runs give the same bits.  Compiled with -ffp-contract=off: tests/track_oracle.py restates the factor and the two
// substitutions operation by operation; they are shared with track_stream.hip (track_rule.h).
#include "common.h"
#include "rot6d.h"
#include "track_rule.h"

using namespace danet;

namespace {

constexpr int kWave = 64;

__global__ __launch_bounds__(kWave) void track_factor_kernel(const float* __restrict__ conf, const int32_t* __restrict__ track_start, int K,
                                                             int G, Lams lam, double* __restrict__ ws, size_t N)
{
    const long idx = (long)blockIdx.x * kWave + threadIdx.x;
    if (idx >= (long)K * G) return;
    const int k = (int)(idx / G), g = (int)(idx % G);
    const int s = track_start[k], T = track_start[k + 1] - s;
    const double lv = lam.vel[g], la = lam.acc[g];
    double* l1 = ws + (size_t)g * 3 * N + s;
    double* l2 = l1 + N;
    double* D = l2 + N;
    double Dm1 = 0.0, Dm2 = 0.0, l1m1 = 0.0;
    for (int t = 0; t < T; ++t) {
        const FactorRow f = factor_row(t, T, (double)conf[s + t] + kEps, lv, la, Dm1, Dm2, l1m1);
        l1[t] = f.L1; l2[t] = f.L2; D[t] = f.Dt;
        Dm2 = Dm1; Dm1 = f.Dt; l1m1 = f.L1;
    }
}

template <bool kPara>
__global__ __launch_bounds__(kWave) void track_solve_kernel(const float* __restrict__ values, const float* __restrict__ conf,
                                                            const int32_t* __restrict__ track_start, int C, int cblocks, int shared_shape,
                                                            double* __restrict__ ws, size_t N, float* __restrict__ out,
                                                            int32_t* __restrict__ status)
{
    const int k = blockIdx.x / cblocks;
    const int ch = (blockIdx.x % cblocks) * kWave + threadIdx.x;
    if (ch >= C) return;
    const int s = track_start[k], T = track_start[k + 1] - s;
    const int stride = kPara ? kParaRow : C;
    const int col = channel_col<kPara>(ch);
    const int g = channel_group<kPara>(ch);
    const float* x = values + (size_t)s * stride + col;
    float* y = out + (size_t)s * stride + col;
    const float* c = conf + s;

    double sc = 0.0, sy = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int t = 0; t < T; ++t) {
        const float ct = c[t];
        if (ct > 0.0f) {
            const float v = x[(size_t)t * stride];
            sc += (double)ct;
            sy += (double)ct * (double)v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    if (ch == 0) status[k] = sc > 0.0 ? 0 : 1;
    if (!(sc > 0.0)) {                                                         // nothing observed: the rows come back bit for bit
        for (int t = 0; t < T; ++t) y[(size_t)t * stride] = x[(size_t)t * stride];
        return;
    }
    const double mean = sy / sc;
    if (kPara && g == 1 && shared_shape) {
        const float m = (float)mean;
        for (int t = 0; t < T; ++t) y[(size_t)t * stride] = m;
        return;
    }
    const double* l1 = ws + (size_t)g * 3 * N + s;
    const double* l2 = l1 + N;
    const double* D = l2 + N;
    double* z = ws + (size_t)kGroups * 3 * N + (size_t)s * C + ch;
    double zm1 = 0.0, zm2 = 0.0;
    for (int t = 0; t < T; ++t) {
        const float ct = c[t];
        const double w = (double)ct + kEps;
        const double yt = ct > 0.0f ? (double)x[(size_t)t * stride] : mean;
        const double zt = forward_step(w * yt, l1[t], zm1, l2[t], zm2);
        z[(size_t)t * C] = zt;
        zm2 = zm1; zm1 = zt;
    }
    double xp1 = 0.0, xp2 = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        const double a1 = t + 1 < T ? l1[t + 1] : 0.0;
        const double a2 = t + 2 < T ? l2[t + 2] : 0.0;
        const double xt = backward_step(z[(size_t)t * C], D[t], a1, xp1, a2, xp2);
        float r = (float)xt;
        if (kPara && ch == 0) r = r < lo ? lo : (r > hi ? hi : r);             // (a NaN stays a NaN)
        y[(size_t)t * stride] = r;
        xp2 = xp1; xp1 = xt;
    }
}

__global__ __launch_bounds__(kWave) void track_rot_kernel(const float* __restrict__ para, const int32_t* __restrict__ track_start, int K,
                                                          size_t N, const int32_t* __restrict__ status, float* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (idx >= N * 24) return;
    const size_t n = idx / 24;
    const int j = (int)(idx % 24);
    int a = 0, b = K;                                                          // the track of row n: track_start[a] <= n < track_start[a + 1]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if ((size_t)track_start[m] <= n) a = m; else b = m;
    }
    float* o = out + n * kParaRow + 3 + kNB + j * 9;
    if (status[a] != 0) {
        const float* p = para + n * kParaRow + 3 + kNB + j * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) o[i] = p[i];
        return;
    }
    const float p6[6] = {o[0], o[1], o[3], o[4], o[6], o[7]};
    float R[9];
    danet::rot6d_fwd(p6, R);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = R[i];
}

__global__ __launch_bounds__(kWave) void track_accel_kernel(const float* __restrict__ joints, const float* __restrict__ ref,
                                                            const int32_t* __restrict__ track_start, int J, double* __restrict__ accel,
                                                            int32_t* __restrict__ count)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const int s = track_start[k], T = track_start[k + 1] - s;
    const long items = T >= 3 ? (long)(T - 2) * J : 0;
    double acc = 0.0;
    for (long i = lane; i < items; i += kWave) {
        const size_t t = (size_t)(i / J) + 1;
        const size_t base = ((size_t)s + t) * J * 3 + (size_t)(i % J) * 3;
        const size_t row = (size_t)J * 3;
        double n2 = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double xm = (double)joints[base - row + d], x0 = (double)joints[base + d], xp = (double)joints[base + row + d];
            if (ref) { xm -= (double)ref[base - row + d]; x0 -= (double)ref[base + d]; xp -= (double)ref[base + row + d]; }
            const double a = (xp - 2.0 * x0) + xm;
            n2 += a * a;
        }
        acc += sqrt(n2);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if (lane == 0) {
        accel[k] = items > 0 ? acc / (double)items : 0.0;
        count[k] = (int32_t)items;
    }
}

int check_common(const char* op, const void* values, const float* conf, const int32_t* track_start, const int32_t* track_start_host,
                 long N, int C, int K, const void* out, const int32_t* status, const void* ws, size_t ws_bytes)
{
    DANET_CHECK_ARG(N >= 1 && C >= 1 && K >= 1 && N < (1L << 31), "%s: bad sizes N=%ld C=%d K=%d", op, N, C, K);
    DANET_CHECK_ARG(values && conf && track_start && track_start_host && out && status && ws, "%s: null pointer", op);
    DANET_CHECK_ARG(values != out, "%s: the output must not alias the input", op);
    DANET_CHECK_OFFSETS(op, "track_start", track_start_host, K, N);
    DANET_CHECK_ARG((long)K * danet::cdiv(C, kWave) < (1L << 31), "%s: K=%d tracks of C=%d channels exceed the grid", op, K, C);
    if (ws_bytes < danet_track_smooth_ws_bytes(N, C))
        return ::danet::fail(DANET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", op, ws_bytes, danet_track_smooth_ws_bytes(N, C));
    return DANET_OK;
}

}  // namespace

extern "C" size_t danet_track_smooth_ws_bytes(long N, int C)
{
    if (N < 1 || C < 1) return 0;
    return ((size_t)kGroups * 3 * (size_t)N + (size_t)N * (size_t)C) * sizeof(double);
}

extern "C" int danet_track_smooth(const float* values, const float* conf, const int32_t* track_start, const int32_t* track_start_host,
                                  long N, int C, int K, double lam_vel, double lam_acc, float* out, int32_t* status, void* ws,
                                  size_t ws_bytes, void* stream)
{
    DANET_ENTER();
    const int rc = check_common("track_smooth", values, conf, track_start, track_start_host, N, C, K, out, status, ws, ws_bytes);
    if (rc != DANET_OK) return rc;
    DANET_CHECK_ARG(lam_ok(lam_vel) && lam_ok(lam_acc), "track_smooth: lam_vel=%g lam_acc=%g (finite and not negative)", lam_vel, lam_acc);
    Lams lam = {};
    lam.vel[0] = lam_vel; lam.acc[0] = lam_acc;
    const int cb = danet::cdiv(C, kWave);
    hipLaunchKernelGGL(track_factor_kernel, dim3(danet::cdiv(K, kWave)), dim3(kWave), 0, (hipStream_t)stream, conf, track_start, K, 1, lam,
                       (double*)ws, (size_t)N);
    DANET_CHECK_LAUNCH("track_factor_kernel");
    hipLaunchKernelGGL(track_solve_kernel<false>, dim3((unsigned)((long)K * cb)), dim3(kWave), 0, (hipStream_t)stream, values, conf, track_start,
                       C, cb, 0, (double*)ws, (size_t)N, out, status);
    DANET_CHECK_LAUNCH("track_solve_kernel");
    return DANET_OK;
}

extern "C" int danet_track_smooth_para(const float* para, const float* conf, const int32_t* track_start, const int32_t* track_start_host,
                                       long N, int K, const double* lam, int shared_shape, float* out, int32_t* status, void* ws,
                                       size_t ws_bytes, void* stream)
{
    DANET_ENTER();
    const int rc = check_common("track_smooth_para", para, conf, track_start, track_start_host, N, kParaCh, K, out, status, ws, ws_bytes);
    if (rc != DANET_OK) return rc;
    Lams l = {};
    if (const int e = read_lams("track_smooth_para", lam, l)) return e;
    DANET_CHECK_ARG(N * 24 / kWave + 1 < (1L << 31), "track_smooth_para: N=%ld rows exceed the grid", N);
    const int cb = danet::cdiv(kParaCh, kWave);
    hipLaunchKernelGGL(track_factor_kernel, dim3(danet::cdiv((long)K * kGroups, kWave)), dim3(kWave), 0, (hipStream_t)stream, conf, track_start,
                       K, kGroups, l, (double*)ws, (size_t)N);
    DANET_CHECK_LAUNCH("track_factor_kernel");
    hipLaunchKernelGGL(track_solve_kernel<true>, dim3((unsigned)((long)K * cb)), dim3(kWave), 0, (hipStream_t)stream, para, conf, track_start,
                       kParaCh, cb, shared_shape ? 1 : 0, (double*)ws, (size_t)N, out, status);
    DANET_CHECK_LAUNCH("track_solve_kernel");
    hipLaunchKernelGGL(track_rot_kernel, dim3(danet::cdiv(N * 24, kWave)), dim3(kWave), 0, (hipStream_t)stream, para, track_start, K, (size_t)N,
                       status, out);
    DANET_CHECK_LAUNCH("track_rot_kernel");
    return DANET_OK;
}

extern "C" int danet_track_accel(const float* joints, const float* joints_ref, const int32_t* track_start, const int32_t* track_start_host,
                                 long N, int J, int K, double* accel, int32_t* count, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(N >= 1 && J >= 1 && K >= 1 && N < (1L << 31), "track_accel: bad sizes N=%ld J=%d K=%d", N, J, K);
    DANET_CHECK_ARG(joints && track_start && track_start_host && accel && count, "track_accel: null pointer");
    DANET_CHECK_OFFSETS("track_accel", "track_start", track_start_host, K, N);
    hipLaunchKernelGGL(track_accel_kernel, dim3(K), dim3(kWave), 0, (hipStream_t)stream, joints, joints_ref, track_start, J, accel, count);
    DANET_CHECK_LAUNCH("track_accel_kernel");
    return DANET_OK;
}
