// The track rule (DESIGN.md 4b'-track): the channels of a row, the lam pairs and one row of the banded L D L^T factor with the two
// substitution steps, ONE set of functions for every caller: track_ops.hip (whole tracks) and track_stream.hip (a few rows per step,
// through rings).  The callers compile with -ffp-contract=off: every operation below is one IEEE-754 double operation in the written
// order (tests/track_oracle.py restates them), so the streamed factor is the offline one bit for bit.
#pragma once
#include "common.h"
#include "video_sizes.h"

namespace danet {

constexpr double kEps = 1e-6;                    // added to every weight: the system stays definite where nothing is observed
constexpr int kParaCh = 3 + kNB + 144;           // 157 unknowns
constexpr int kGroups = 3;                       // cam, betas, rotations

struct Lams { double vel[kGroups]; double acc[kGroups]; };

inline bool lam_ok(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }    // not negative, finite, not NaN

// the para form's six numbers (lam_vel, lam_acc per group) on the host -> l; `op` opens the messages
inline int read_lams(const char* op, const double* lam, Lams& l)
{
    DANET_CHECK_ARG(lam, "%s: null lam", op);
    for (int g = 0; g < kGroups; ++g) {
        l.vel[g] = lam[2 * g]; l.acc[g] = lam[2 * g + 1];
        DANET_CHECK_ARG(lam_ok(l.vel[g]) && lam_ok(l.acc[g]), "%s: group %d lam_vel=%g lam_acc=%g (finite and not negative)", op, g, l.vel[g],
                        l.acc[g]);
    }
    return DANET_OK;
}

// Column of channel ch in a row: the plain form is [N,C]; the para form reads and writes the fit rule's unknowns in place in a
// [N,229] row: cam, betas, and per joint the [3,2] row-major view of the first two matrix columns.
template <bool kPara> __device__ __forceinline__ int channel_col(int ch)
{
    if (!kPara || ch < 3 + kNB) return ch;
    const int r = ch - (3 + kNB), j = r / 6, i = r % 6;
    return 3 + kNB + j * 9 + (i >> 1) * 3 + (i & 1);
}

// the lam group of channel ch: the plain form has one; cam, betas, rotations in the para form
template <bool kPara> __device__ __forceinline__ int channel_group(int ch) { return !kPara ? 0 : (ch < 3 ? 0 : (ch < 3 + kNB ? 1 : 2)); }

// Row t of the factor of a track of T rows: w = c_t + kEps, (lv, la) the group's lam pair, Dm1 = D[t - 1], Dm2 = D[t - 2] and
// l1m1 = l1[t - 1] (0 where the row does not exist).  The stencils lose a term at the ends and below T = 3.
struct FactorRow { double L1, L2, Dt; };

__device__ __forceinline__ FactorRow factor_row(int t, int T, double w, double lv, double la, double Dm1, double Dm2, double l1m1)
{
    const double nv = T >= 2 ? ((t == 0 || t == T - 1) ? 1.0 : 2.0) : 0.0;
    const double na = (t + 1 <= T - 2 ? 1.0 : 0.0) + (t >= 1 && t <= T - 2 ? 4.0 : 0.0) + (t - 1 >= 1 ? 1.0 : 0.0);
    const double d = (w + lv * nv) + la * (T >= 3 ? na : 0.0);
    double L1 = 0.0, L2 = 0.0;
    if (t >= 2) L2 = la / Dm2;                                             // f_{t-2} = la
    if (t >= 1) {
        const int u = t - 1;                                               // e_u: rows (u, u + 1)
        const double ne = (u >= 1 && u <= T - 2 ? 1.0 : 0.0) + (u + 1 >= 1 && u + 1 <= T - 2 ? 1.0 : 0.0);
        const double e = -lv - 2.0 * la * ne;
        L1 = (e - (L2 * Dm2) * l1m1) / Dm1;
    }
    return FactorRow{L1, L2, (d - (L1 * L1) * Dm1) - (L2 * L2) * Dm2};
}

// one step of L z = rhs in ascending t, and of L^T x = z / D in descending t (a1 = l1[t + 1], a2 = l2[t + 2], 0 past the end)
__device__ __forceinline__ double forward_step(double rhs, double l1, double zm1, double l2, double zm2) { return (rhs - l1 * zm1) - l2 * zm2; }
__device__ __forceinline__ double backward_step(double z, double D, double a1, double xp1, double a2, double xp2)
{
    return (z / D - a1 * xp1) - a2 * xp2;
}

}  // namespace danet
