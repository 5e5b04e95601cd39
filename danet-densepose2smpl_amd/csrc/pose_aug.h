// The augmentation of an axis-angle SMPL pose (augment.pose_processing: rotate_pose, then flip_pose) and its undo
// (FitsDict.__setitem__: flip_pose, then rotate_pose by -rot), ONE pair of device functions for every caller: input_ops.hip
// (the label op, both directions) and fit_loop.hip (a fitted row on its way back into the table).  fp64 inside, rounded to
// fp32 once; the callers compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "rotation.h"

namespace danet {

// constants.py SMPL_JOINTS_FLIP_PERM (host table: kernels take it by value inside an argument struct)
static const unsigned char kSmplFlip[24] = {0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22};

// imutils.py:115-127 (augment.rot_aa): the axis-angle vector aa rotated by `rad` about the camera axis
__device__ inline void rotate_global_orient(double* __restrict__ aa, double cs, double sn) {
    double ang = sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
    if (ang < 1e-12) ang = 1e-12;
    const double ax = aa[0] / ang, ay = aa[1] / ang, az = aa[2] / ang;
    const double s = sin(ang), c1 = 1.0 - cos(ang);
    double R[9];                                                                      // I + s K + (1 - c) K K
    R[0] = 1.0 + c1 * (-az * az - ay * ay); R[1] = -s * az + c1 * (ax * ay);         R[2] = s * ay + c1 * (ax * az);
    R[3] = s * az + c1 * (ax * ay);         R[4] = 1.0 + c1 * (-az * az - ax * ax);  R[5] = -s * ax + c1 * (ay * az);
    R[6] = -s * ay + c1 * (ax * az);        R[7] = s * ax + c1 * (ay * az);          R[8] = 1.0 + c1 * (-ay * ay - ax * ax);
    double Q[9];                                                                      // Rz R
    for (int k = 0; k < 3; ++k) {
        Q[k] = cs * R[k] - sn * R[3 + k];
        Q[3 + k] = sn * R[k] + cs * R[3 + k];
        Q[6 + k] = R[6 + k];
    }
    rotmat_to_angle_axis<double>(Q, aa);
}

// pose_processing (inverse = 0: rotate, then flip) or FitsDict.__setitem__'s undo (inverse = 1: flip, then rotate back) by a
// workgroup of kThreads; `in` 72 numbers of type T, `sh` 72 doubles of LDS scratch, `perm` the 24 entries of kSmplFlip, out fp32.
// (cs, sn) = cos / sin of -rot (forward) or +rot (inverse) in radians.
template <typename T, int kThreads>
__device__ inline void pose_row(const T* __restrict__ in, double* __restrict__ sh, const unsigned char* __restrict__ perm, bool flip,
                                bool inverse, double cs, double sn, float* __restrict__ out)
{
    for (int k = threadIdx.x; k < 72; k += kThreads) {
        double v;
        if (inverse && flip) {
            const int j = k / 3, a = k - j * 3;
            v = (double)in[perm[j] * 3 + a];
            if (a > 0) v = -v;
        } else {
            v = (double)in[k];
        }
        sh[k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) rotate_global_orient(sh, cs, sn);
    __syncthreads();
    for (int k = threadIdx.x; k < 72; k += kThreads) {
        double v;
        if (!inverse && flip) {
            const int j = k / 3, a = k - j * 3;
            v = sh[perm[j] * 3 + a];
            if (a > 0) v = -v;
        } else {
            v = sh[k];
        }
        out[k] = (float)v;
    }
    __syncthreads();
}

}  // namespace danet
