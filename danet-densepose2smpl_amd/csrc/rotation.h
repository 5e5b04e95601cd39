// Rotation matrix -> axis-angle under the rule of DESIGN.md ("axis-angle rule"; the convention of cv2.Rodrigues: angle in
// [0, pi]), ONE device function for every caller: eval_ops.hip (fp32, danet_rotmat_to_angle_axis), pose_aug.h (fp64, the
// global orientation of an augmented pose: input_ops.hip, fit_loop.hip) and fit_loop.hip (fp64, the 24 fitted matrices).
#pragma once
#include <hip/hip_runtime.h>

namespace danet {

__device__ __forceinline__ float rt_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double rt_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float rt_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double rt_atan2(double y, double x) { return atan2(y, x); }

// R: 9 numbers, row-major; aa: 3 numbers
template <typename T>
__device__ __forceinline__ void rotmat_to_angle_axis(const T* __restrict__ R, T* __restrict__ aa) {
    const T r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
    // matrix -> quaternion, the case of the largest of (trace, r00, r11, r22): the square root is taken of a number >= 1
    T w, x, y, z;
    const T tr = r00 + r11 + r22;
    if (tr > T(0)) {
        const T s = T(2) * rt_sqrt(tr + T(1));
        w = T(0.25) * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
    } else if (r00 >= r11 && r00 >= r22) {
        const T s = T(2) * rt_sqrt(T(1) + r00 - r11 - r22);
        w = (r21 - r12) / s; x = T(0.25) * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
    } else if (r11 >= r22) {
        const T s = T(2) * rt_sqrt(T(1) + r11 - r00 - r22);
        w = (r02 - r20) / s; x = (r01 + r10) / s; y = T(0.25) * s; z = (r12 + r21) / s;
    } else {
        const T s = T(2) * rt_sqrt(T(1) + r22 - r00 - r11);
        w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = T(0.25) * s;
    }
    if (w < T(0)) { w = -w; x = -x; y = -y; z = -z; }                        // the angle in [0, pi]
    // quaternion -> axis-angle: angle = 2 atan2(|xyz|, w), axis = xyz / |xyz|; small angles: 2 xyz / w
    const T sn = rt_sqrt(x * x + y * y + z * z);
    const T k = sn < T(1e-6) ? T(2) / w : T(2) * rt_atan2(sn, w) / sn;
    aa[0] = x * k;
    aa[1] = y * k;
    aa[2] = z * k;
}

}  // namespace danet
