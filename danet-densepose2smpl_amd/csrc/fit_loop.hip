// The accept step of the in-loop fit for gfx950 (DESIGN.md 4d "the refresh rule"; fit_loop.py is the caller): which fitted rows
// replace their pseudo-label in FitsDict's table, and the replacement itself.
//
//   fits_accept     one launch, one workgroup of one wave per sample, a lane per joint.  A sample's CANDIDATE is what the table
//                   would take from it: the axis-angle of its 24 fitted matrices (the one rotmat_to_angle_axis of rotation.h),
//                   taken out of the augmented frame by the undo of pose_aug.h (flip_pose, then rotate_pose by -rot), and its
//                   ten betas; fp64 inside, rounded to fp32 once.  The decision reads the two data energies, the two status
//                   words, has_smpl, the betas and the candidate.  Samples that name the same table row are settled without
//                   atomics and without a second launch: each sample scans the B row numbers and works out the decision of every
//                   sample that shares its row for itself (duplicates inside a batch are rare, and a candidate costs a few
//                   hundred operations); the lowest E_new wins, the lowest sample index on ties.  So a table row is written by at
//                   most one workgroup, no workgroup reads what another writes, and the result is independent of dispatch order.
//
// Compiled with -ffp-contract=off like input_ops.hip: the same pose_row gives the same bits in both units.
#include "common.h"
#include "pose_aug.h"

namespace {

constexpr int kAcceptThreads = 64;
constexpr int kNB = 10;                  // the table's rows are 72 pose + 10 betas
constexpr int kRow = 72 + kNB;

struct SmplPerm { unsigned char smpl[24]; };

struct Scratch {                         // LDS of one workgroup
    double aa[72];                       // the fitted rotations as axis-angle, augmented frame
    double sh[72];                       // pose_row's scratch
    float cand[kRow];                    // the candidate row
};

// Candidate and decision of sample c, by the whole workgroup (every lane returns the same answer; call from uniform control
// flow).  Leaves the candidate in s.cand.
__device__ bool candidate(const danet_fits_accept_args& a, const SmplPerm& pm, int c, Scratch& s)
{
    const int tid = threadIdx.x;
    const int stride = 3 + kNB + 216;
    const float* p = a.para_fit + (size_t)c * stride;
    if (tid < 24) {
        double R[9], v[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (double)p[3 + kNB + tid * 9 + k];
        danet::rotmat_to_angle_axis<double>(R, v);
        s.aa[tid * 3 + 0] = v[0]; s.aa[tid * 3 + 1] = v[1]; s.aa[tid * 3 + 2] = v[2];
    }
    __syncthreads();
    const double rot = a.rot_flip[c * 2 + 0];
    const bool flip = a.rot_flip[c * 2 + 1] != 0.0;
    const double rad = rot * 3.141592653589793 / 180.0;                     // the undo: label_augment's inverse = 1
    danet::pose_row<double, kAcceptThreads>(s.aa, s.sh, pm.smpl, flip, true, cos(rad), sin(rad), s.cand);
    if (tid < kNB) s.cand[72 + tid] = p[3 + tid];
    __syncthreads();
    bool ok = true;
    for (int k = tid; k < kRow; k += kAcceptThreads) {
        const float v = s.cand[k];
        ok = ok && (v - v == 0.0f);                                          // finite
        if (k >= 72) ok = ok && fabsf(v) <= 3.0f;                            // prepare_batch zeroes betas beyond 3 on the way in
    }
    const int all_ok = __syncthreads_and(ok ? 1 : 0);
    const float en = a.e_new[c], eo = a.e_old[c];
    const long long row = a.rows[c];
    return all_ok != 0 && a.has_smpl[c] == 0.0f && row >= 0 && row < a.N && a.status_fit[c] == 0 && a.status_eval[c] == 0 &&
           (en - en == 0.0f) && !(eo <= en);
}

__global__ __launch_bounds__(kAcceptThreads) void fits_accept_kernel(danet_fits_accept_args a, SmplPerm pm)
{
    __shared__ Scratch own, other;
    const int b = blockIdx.x, tid = threadIdx.x;
    bool take = candidate(a, pm, b, own);
    if (take) {
        const long long row = a.rows[b];
        const float en = a.e_new[b];
        for (int c = 0; c < a.B && take; ++c) {
            if (c == b || a.rows[c] != row) continue;
            const float ec = a.e_new[c];
            if (!(ec < en || (ec == en && c < b))) continue;                  // could not beat b even if accepted
            if (candidate(a, pm, c, other)) take = false;
        }
    }
    if (take) {
        const long long row = a.rows[b];
        for (int k = tid; k < kRow; k += kAcceptThreads) a.table[(size_t)row * kRow + k] = own.cand[k];
        if (tid == 0) {
            double c2 = 0.0;
            for (int k = 0; k < 49; ++k) {
                const double cf = (double)a.kp[((size_t)b * 49 + k) * 3 + 2];
                c2 += cf * cf;
            }
            a.valid[row] = (double)a.e_new[b] < (double)a.tau * c2 ? 1 : 0;
        }
    }
    if (tid == 0) a.updated[b] = take ? 1 : 0;
}

}  // namespace

extern "C" int danet_fits_accept(const struct danet_fits_accept_args* args, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(args, "fits_accept: null arguments");
    const danet_fits_accept_args& a = *args;
    DANET_CHECK_ARG(a.B > 0 && a.B < (1 << 24) && a.N > 0 && a.NB == kNB, "fits_accept: bad sizes B=%d N=%lld NB=%d (the table holds %d betas)",
                    a.B, (long long)a.N, a.NB, kNB);
    DANET_CHECK_ARG(a.para_fit && a.e_new && a.e_old && a.status_fit && a.status_eval && a.has_smpl && a.rows && a.rot_flip && a.kp &&
                    a.table && a.valid && a.updated, "fits_accept: null pointer");
    SmplPerm pm;
    for (int j = 0; j < 24; ++j) pm.smpl[j] = danet::kSmplFlip[j];
    hipLaunchKernelGGL(fits_accept_kernel, dim3(a.B), dim3(kAcceptThreads), 0, (hipStream_t)stream, a, pm);
    DANET_CHECK_LAUNCH("fits_accept_kernel");
    return DANET_OK;
}
