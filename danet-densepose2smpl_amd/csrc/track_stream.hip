// The streaming form of the track smoother for gfx950 (DESIGN.md 4b'-stream "the stream rule"; tracks.StreamSmoother is the caller):
// rows arrive a few at a time, and the value emitted for row g of a slot is what track_ops.hip gives on the rows the slot has seen so
// far, read at row g, for g at most `lag` rows behind the newest.
//
//   track_stream_kernel   one launch per step, one workgroup per slot.
//     phase 1   lane g < G (one per lam group) recomputes the factor rows t0 = T0 - 2 .. T - 1 (T0 rows before the step, T after)
//               with the stencils of the new length: rows <= T - 3 of the banded L D L^T do not depend on T, so everything older
//               is final and is kept.  The same lane carries zB, the forward pass of the gap rows' (c + eps), which depends on the
//               group only.
//     phase 2   a lane per channel: the running sum c y, the right-hand side (c + eps) y of the new rows, the forward pass zA of
//               rows t0 .. T - 1, then, where a row is asked for, z = zA + mean zB (the forward pass is linear in the right-hand
//               side, and the gap rows' target is the prefix's current mean) and the back substitution from T - 1 down to the row.
//     phase 3   the para form only: the six rounded numbers of a joint meet in LDS, 24 lanes take them through danet::rot6d_fwd.
//
// The rings hold R = lag + max_new + 4 rows: the back substitution reaches lag rows back, the refactoring max_new + 4.  A lane
// touches only its own slot's state, rows and output: a slot's bits do not depend on its neighbours.  No atomics, no grid barrier,
// nothing read on the host.  Compiled with -ffp-contract=off: the factor row and the substitution steps are shared with
// track_ops.hip (track_rule.h) and restated in tests/track_oracle.py.
#include "common.h"
#include "rot6d.h"
#include "track_rule.h"

using namespace danet;

namespace {

constexpr int kWave = 64;
constexpr int kParaBlock = 192;                  // >= kParaCh: one lane per unknown
constexpr int kMaxSlots = 1 << 20, kMaxLag = 4096, kMaxNew = 64, kMaxC = 65536;

struct SlotHeader { int32_t T; int32_t pad; float lo; float hi; double sc; };    // 24 bytes; all zero: an empty slot
static_assert(sizeof(SlotHeader) == 24, "SlotHeader");

__host__ __device__ inline int ring_rows(int lag, int max_new) { return lag + max_new + 4; }
__host__ __device__ inline size_t slot_bytes(int C, int R)
{
    const size_t Re = (size_t)((R + 1) & ~1);
    return sizeof(SlotHeader) + 4 * Re + 8 * ((size_t)kGroups * 4 * R + (size_t)C + 2 * (size_t)R * C);
}

template <bool kPara>
__global__ __launch_bounds__(256) void track_stream_kernel(unsigned char* __restrict__ state, int C, int lag, int max_new,
                                                           const int32_t* __restrict__ n_new, const int32_t* __restrict__ reset,
                                                           const float* __restrict__ rows, const float* __restrict__ conf,
                                                           const int32_t* __restrict__ emit, Lams lam, int shared_shape,
                                                           float* __restrict__ out, int32_t* __restrict__ valid)
{
    __shared__ float six[kPara ? 144 : 1];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int R = ring_rows(lag, max_new);
    const int G = kPara ? kGroups : 1;
    const int stride = kPara ? kParaRow : C;
    unsigned char* base = state + (size_t)slot * slot_bytes(C, R);
    SlotHeader* hdr = (SlotHeader*)base;
    float* cring = (float*)(base + sizeof(SlotHeader));
    double* fac = (double*)(base + sizeof(SlotHeader) + 4 * (size_t)((R + 1) & ~1));   // [kGroups][l1 | l2 | D | zB][R]
    double* sy_all = fac + (size_t)kGroups * 4 * R;                                       // [C]
    double* rA = sy_all + C;                                                              // [R][C]
    double* zA = rA + (size_t)R * C;                                                      // [R][C]

    const bool fresh = reset[slot] != 0;
    const int T0 = fresh ? 0 : hdr->T;
    int n = n_new[slot];
    n = n < 0 ? 0 : (n > max_new ? max_new : n);
    const int T = T0 + n;
    const int t0 = T0 - 2 > 0 ? T0 - 2 : 0;
    const float* cin = conf + (size_t)slot * max_new;
    const double sc0 = T0 > 0 ? hdr->sc : 0.0;

    // ---- phase 1: the factor rows t0 .. T - 1 of every group, and zB --------------------------------------------------------------
    if (tid < G && n > 0) {
        const int g = tid;
        const double lv = lam.vel[g], la = lam.acc[g];
        double* l1 = fac + (size_t)g * 4 * R;
        double* l2 = l1 + R;
        double* D = l2 + R;
        double* zB = D + R;
        double Dm1 = t0 >= 1 ? D[(t0 - 1) % R] : 0.0, Dm2 = t0 >= 2 ? D[(t0 - 2) % R] : 0.0, l1m1 = t0 >= 1 ? l1[(t0 - 1) % R] : 0.0;
        double zm1 = t0 >= 1 ? zB[(t0 - 1) % R] : 0.0, zm2 = t0 >= 2 ? zB[(t0 - 2) % R] : 0.0;
        for (int t = t0; t < T; ++t) {
            const float ct = t >= T0 ? cin[t - T0] : cring[t % R];
            const double w = (double)ct + kEps;
            const FactorRow f = factor_row(t, T, w, lv, la, Dm1, Dm2, l1m1);
            const double zt = forward_step(ct > 0.0f ? 0.0 : w, f.L1, zm1, f.L2, zm2);
            l1[t % R] = f.L1; l2[t % R] = f.L2; D[t % R] = f.Dt; zB[t % R] = zt;
            Dm2 = Dm1; Dm1 = f.Dt; l1m1 = f.L1;
            zm2 = zm1; zm1 = zt;
        }
    }
    __syncthreads();                                                            // the factor rows are visible to the slot's lanes
    if (tid == 0) {                                                             // (every lane has read the header and the old ring by now)
        double sc = sc0;
        for (int i = 0; i < n; ++i) {
            const float ct = cin[i];
            cring[(T0 + i) % R] = ct;
            if (ct > 0.0f) sc += (double)ct;
        }
        hdr->T = T;
        hdr->sc = sc;
    }

    const int g_emit = emit[slot];
    const int oldest = T - 1 - lag > 0 ? T - 1 - lag : 0;
    const bool ok = g_emit >= oldest && g_emit <= T - 1;                        // (T = 0: never)
    float* o = out + (size_t)slot * stride;
    if (tid == 0) valid[slot] = ok ? 1 : 0;

    // ---- phase 2: a lane per channel ----------------------------------------------------------------------------------------------
    for (int ch = tid; ch < C; ch += blockDim.x) {
        const int col = channel_col<kPara>(ch);
        const int g = channel_group<kPara>(ch);
        const double* l1 = fac + (size_t)g * 4 * R;
        const double* l2 = l1 + R;
        const double* D = l2 + R;
        const double* zB = D + R;
        const bool clamp = kPara && ch == 0;
        double sc = sc0, sy = T0 > 0 ? sy_all[ch] : 0.0;
        float lo = INFINITY, hi = -INFINITY;
        if (clamp && T0 > 0) { lo = hdr->lo; hi = hdr->hi; }                    // (lane 0 alone reads and writes these two)
        for (int i = 0; i < n; ++i) {
            const float ct = cin[i];
            double r = 0.0;
            if (ct > 0.0f) {
                const float v = rows[((size_t)slot * max_new + i) * stride + col];
                sc += (double)ct;
                sy += (double)ct * (double)v;
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
                r = ((double)ct + kEps) * (double)v;
            }
            rA[(size_t)((T0 + i) % R) * C + ch] = r;
        }
        if (n > 0 || fresh) sy_all[ch] = sy;
        if (clamp && (n > 0 || fresh)) { hdr->lo = lo; hdr->hi = hi; }
        if (n > 0) {
            double zm1 = t0 >= 1 ? zA[(size_t)((t0 - 1) % R) * C + ch] : 0.0, zm2 = t0 >= 2 ? zA[(size_t)((t0 - 2) % R) * C + ch] : 0.0;
            for (int t = t0; t < T; ++t) {
                const int r = t % R;
                const double zt = forward_step(rA[(size_t)r * C + ch], l1[r], zm1, l2[r], zm2);
                zA[(size_t)r * C + ch] = zt;
                zm2 = zm1; zm1 = zt;
            }
        }
        float res = 0.0f;
        if (ok) {
            const double mean = sy / sc;
            if (kPara && g == 1 && shared_shape) {
                res = (float)mean;
            } else {
                double xp1 = 0.0, xp2 = 0.0, xt = 0.0;
                for (int t = T - 1; t >= g_emit; --t) {
                    const int r = t % R;
                    const double a1 = t + 1 < T ? l1[(t + 1) % R] : 0.0;
                    const double a2 = t + 2 < T ? l2[(t + 2) % R] : 0.0;
                    const double z = zA[(size_t)r * C + ch] + mean * zB[r];
                    xt = backward_step(z, D[r], a1, xp1, a2, xp2);
                    xp2 = xp1; xp1 = xt;
                }
                res = (float)xt;
                if (clamp) res = res < lo ? lo : (res > hi ? hi : res);        // (a NaN stays a NaN)
            }
        }
        if (!kPara || ch < 3 + kNB) o[ch] = res;
        else six[ch - (3 + kNB)] = res;
    }

    // ---- phase 3: the 6D map --------------------------------------------------------------------------------------------------------
    if (kPara) {
        __syncthreads();
        if (tid < 24) {
            float* m = o + 3 + kNB + tid * 9;
            if (ok) {
                const float p6[6] = {six[tid * 6], six[tid * 6 + 1], six[tid * 6 + 2], six[tid * 6 + 3], six[tid * 6 + 4], six[tid * 6 + 5]};
                float Rm[9];
                danet::rot6d_fwd(p6, Rm);
#pragma unroll
                for (int i = 0; i < 9; ++i) m[i] = Rm[i];
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) m[i] = 0.0f;
            }
        }
    }
}

int check_common(const char* op, const void* state, size_t state_bytes, int S, int C, int lag, int max_new, const void* n_new,
                 const void* reset, const void* rows, const void* conf, const void* emit, const void* out, const void* valid)
{
    const size_t need = danet_track_stream_state_bytes(S, C, lag, max_new);
    DANET_CHECK_ARG(need > 0, "%s: bad sizes S=%d C=%d lag=%d max_new=%d", op, S, C, lag, max_new);
    DANET_CHECK_ARG(state && n_new && reset && rows && conf && emit && out && valid, "%s: null pointer", op);
    DANET_CHECK_ARG(((uintptr_t)state & 7) == 0, "%s: the state must be 8-byte aligned", op);
    DANET_CHECK_ARG(rows != out, "%s: the output must not alias the input", op);
    if (state_bytes < need) return ::danet::fail(DANET_ERR_WORKSPACE, "%s: state of %zu bytes, %zu needed", op, state_bytes, need);
    return DANET_OK;
}

}  // namespace

extern "C" size_t danet_track_stream_state_bytes(int S, int C, int lag, int max_new)
{
    if (S < 1 || C < 1 || lag < 0 || max_new < 1 || S > kMaxSlots || C > kMaxC || lag > kMaxLag || max_new > kMaxNew) return 0;
    return (size_t)S * slot_bytes(C, ring_rows(lag, max_new));
}

extern "C" int danet_track_stream_step(void* state, size_t state_bytes, int S, int C, int lag, int max_new, const int32_t* n_new,
                                       const int32_t* reset, const float* rows, const float* conf, const int32_t* emit, double lam_vel,
                                       double lam_acc, float* out, int32_t* valid, void* stream)
{
    DANET_ENTER();
    const int rc = check_common("track_stream_step", state, state_bytes, S, C, lag, max_new, n_new, reset, rows, conf, emit, out, valid);
    if (rc != DANET_OK) return rc;
    DANET_CHECK_ARG(lam_ok(lam_vel) && lam_ok(lam_acc), "track_stream_step: lam_vel=%g lam_acc=%g (finite and not negative)", lam_vel, lam_acc);
    Lams lam = {};
    lam.vel[0] = lam_vel; lam.acc[0] = lam_acc;
    const int block = C >= 256 ? 256 : danet::cdiv(C, kWave) * kWave;
    hipLaunchKernelGGL(track_stream_kernel<false>, dim3(S), dim3(block), 0, (hipStream_t)stream, (unsigned char*)state, C, lag, max_new, n_new,
                       reset, rows, conf, emit, lam, 0, out, valid);
    DANET_CHECK_LAUNCH("track_stream_kernel");
    return DANET_OK;
}

extern "C" int danet_track_stream_step_para(void* state, size_t state_bytes, int S, int lag, int max_new, const int32_t* n_new,
                                            const int32_t* reset, const float* rows, const float* conf, const int32_t* emit,
                                            const double* lam, int shared_shape, float* out, int32_t* valid, void* stream)
{
    DANET_ENTER();
    const int rc = check_common("track_stream_step_para", state, state_bytes, S, kParaCh, lag, max_new, n_new, reset, rows, conf, emit, out, valid);
    if (rc != DANET_OK) return rc;
    Lams l = {};
    if (const int e = read_lams("track_stream_step_para", lam, l)) return e;
    static_assert(kParaBlock >= kParaCh, "one lane per unknown");
    hipLaunchKernelGGL(track_stream_kernel<true>, dim3(S), dim3(kParaBlock), 0, (hipStream_t)stream, (unsigned char*)state, kParaCh, lag, max_new,
                       n_new, reset, rows, conf, emit, l, shared_shape ? 1 : 0, out, valid);
    DANET_CHECK_LAUNCH("track_stream_kernel");
    return DANET_OK;
}
