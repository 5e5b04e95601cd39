// Input ops of the training pipeline for gfx950 (the reference's datasets/base_dataset.py:144-277 and train/fits_dict.py:51-119;
// datasets.py and fits_dict.py are the callers).
//
//   batch_crop      augment.rgb_processing for a whole batch as one launch: one lane per output pixel reads its four bilinear taps
//                   straight from the packed uint8 HWC source (3 bytes per tap, neighbouring lanes neighbouring pixels unless the
//                   crop is rotated), applies flip, pixel noise, the clamp, / 255 and the ImageNet normalisation and writes the
//                   three NCHW planes, consecutive lanes consecutive words.  No float copy of the source exists and nothing is
//                   padded to a common size.  The coordinates and the arithmetic are fp64 (2 M pixels at B = 32, 256 x 256: far from
//                   any fp64 limit of the chip; the kernel is bound by the gather), the result is rounded to fp32 once.
//   label_augment   the label transforms of a batch as one launch, one workgroup per sample: j2d_processing (keypoints, SMPL 2D
//                   keypoints), j3d_processing, pose_processing and FitsDict's rotate / flip of the stored fits (or its inverse),
//                   fp64 inside so that `transform`'s truncation to integers lands where augment.py puts it.
//
// Compiled with -ffp-contract=off: the tests restate the arithmetic operation by operation.
#include "common.h"
#include "pose_aug.h"

namespace {

constexpr int kCropThreads = 256;
constexpr int kCropParams = 10;          // tinv[2][3], flip, pn[3]

__global__ __launch_bounds__(kCropThreads) void batch_crop_kernel(
    const unsigned char* __restrict__ src, long long src_bytes, const long long* __restrict__ offsets,
    const int* __restrict__ shapes, const int* __restrict__ origin, const double* __restrict__ params, int res,
    float* __restrict__ out)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * kCropThreads + threadIdx.x;
    if (p >= res * res) return;
    const int v = p / res, u = p - v * res;
    const double* q = params + (size_t)b * kCropParams;
    const double sx = q[0] * u + q[1] * v + q[2];
    const double sy = q[3] * u + q[4] * v + q[5];
    const bool flip = q[6] != 0.0;
    const int H = shapes[b * 2 + 0], W = shapes[b * 2 + 1];
    const long long base = offsets[b];
    const long long room = offsets[b + 1] < src_bytes ? offsets[b + 1] : src_bytes;      // this sample's bytes end here
    double acc[3] = {0.0, 0.0, 0.0};
    // the packed rectangle starts at `origin` of the image: taps are found in whole-image pixels and moved by integers
    const double fx0 = floor(sx), fy0 = floor(sy);
    const double rx = fx0 - (double)origin[b * 2 + 0], ry = fy0 - (double)origin[b * 2 + 1];
    if (rx >= -1.0 && rx < (double)W && ry >= -1.0 && ry < (double)H && H > 0 && W > 0 && base >= 0) {       // (false for NaN)
        const int x0 = (int)rx, y0 = (int)ry;
        const double ax = sx - fx0, ay = sy - fy0;
        const double wx[2] = {1.0 - ax, ax}, wy[2] = {1.0 - ay, ay};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = x0 + dx, y = y0 + dy;
                if (x < 0 || x >= W || y < 0 || y >= H) continue;                        // a tap outside the image contributes zero
                const long long at = base + ((long long)y * W + x) * 3;
                if (at + 3 > room) continue;
                const double w = wy[dy] * wx[dx];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += w * (double)src[at + c];
            }
    }
    const int uo = flip ? res - 1 - u : u;
    const double mean[3] = {0.485, 0.456, 0.406}, stdev[3] = {0.229, 0.224, 0.225};    // constants.IMG_NORM_MEAN / IMG_NORM_STD
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double t = acc[c] * q[7 + c];
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        t = t / 255.0;
        out[(((size_t)b * 3 + c) * res + v) * res + uo] = (float)((t - mean[c]) / stdev[c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kLabelThreads = 128;

struct Perms {                            // constants.py: J49_FLIP_PERM, J24_FLIP_PERM, SMPL_JOINTS_FLIP_PERM
    unsigned char j49[49], j24[24], smpl[24];
};

__device__ __forceinline__ double trunc1(double x) { return trunc(x) + 1.0; }

// base_dataset.py:160-167 for one keypoint (before the flip): crop transform with truncation, normalisation to [-1, 1]
__device__ __forceinline__ void j2d_point(const double* __restrict__ t, const double* __restrict__ kp, int res, double* __restrict__ o) {
    const double px = (kp[0] + 1.0) - 1.0, py = (kp[1] + 1.0) - 1.0;               // transform(kp + 1): 1-based in, 0-based inside
    const double nx = t[0] * px + t[1] * py + t[2], ny = t[3] * px + t[4] * py + t[5];
    o[0] = 2.0 * trunc1(nx) / res - 1.0;
    o[1] = 2.0 * trunc1(ny) / res - 1.0;
    o[2] = kp[2];
}

__global__ __launch_bounds__(kLabelThreads) void label_augment_kernel(
    const double* __restrict__ xform, const double* __restrict__ rot_flip, const double* __restrict__ keypoints,
    const double* __restrict__ smpl_2dkps, const double* __restrict__ pose_3d, const double* __restrict__ pose,
    const float* __restrict__ fits, Perms pm, int res, int inverse,
    float* __restrict__ keypoints_out, float* __restrict__ smpl_2dkps_out, float* __restrict__ pose_3d_out,
    float* __restrict__ pose_out, float* __restrict__ fits_pose_out, float* __restrict__ fits_betas_out)
{
    __shared__ double sh[72];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double rot = rot_flip[b * 2 + 0];
    const bool flip = rot_flip[b * 2 + 1] != 0.0;
    const double rad = (inverse ? rot : -rot) * 3.141592653589793 / 180.0;        // ("to match direction of rotation from cropping")
    const double sn = sin(rad), cs = cos(rad);
    const double* t = xform ? xform + (size_t)b * 6 : nullptr;
    if (keypoints && t) {
        for (int j = tid; j < 49; j += kLabelThreads) {
            const int s = flip ? pm.j49[j] : j;
            double o[3];
            j2d_point(t, keypoints + ((size_t)b * 49 + s) * 3, res, o);
            if (flip) o[0] = -o[0];
            float* dst = keypoints_out + ((size_t)b * 49 + j) * 3;
            dst[0] = (float)o[0]; dst[1] = (float)o[1]; dst[2] = (float)o[2];
        }
    }
    if (smpl_2dkps && t) {
        for (int j = tid; j < 24; j += kLabelThreads) {
            const int s = flip ? pm.smpl[j] : j;
            double o[3];
            j2d_point(t, smpl_2dkps + ((size_t)b * 24 + s) * 3, res, o);
            if (o[2] == 0.0) o[0] = o[1] = 0.0;                                         // base_dataset.py:260
            if (flip) o[0] = -o[0];
            float* dst = smpl_2dkps_out + ((size_t)b * 24 + j) * 3;
            dst[0] = (float)o[0]; dst[1] = (float)o[1]; dst[2] = (float)o[2];
        }
    }
    if (pose_3d) {
        for (int j = tid; j < 24; j += kLabelThreads) {
            const int s = flip ? pm.j24[j] : j;
            const double* S = pose_3d + ((size_t)b * 24 + s) * 4;
            double x = cs * S[0] + -sn * S[1] + 0.0 * S[2];
            const double y = sn * S[0] + cs * S[1] + 0.0 * S[2];
            if (flip) x = -x;
            float* dst = pose_3d_out + ((size_t)b * 24 + j) * 4;
            dst[0] = (float)x; dst[1] = (float)y; dst[2] = (float)S[2]; dst[3] = (float)S[3];
        }
    }
    if (pose) danet::pose_row<double, kLabelThreads>(pose + (size_t)b * 72, sh, pm.smpl, flip, inverse != 0, cs, sn, pose_out + (size_t)b * 72);
    if (fits) {
        danet::pose_row<float, kLabelThreads>(fits + (size_t)b * 82, sh, pm.smpl, flip, inverse != 0, cs, sn, fits_pose_out + (size_t)b * 72);
        if (tid < 10) fits_betas_out[(size_t)b * 10 + tid] = fits[(size_t)b * 82 + 72 + tid];
    }
}

const unsigned char kJ24Flip[24] = {5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22};
const unsigned char kJ25Flip[25] = {0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21};

}  // namespace

extern "C" int danet_batch_crop(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* shapes, const int32_t* origin,
                                const double* params, int B, int res, float* out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < 65536 && res > 0 && res <= 4096 && src_bytes > 0, "batch_crop: bad sizes B=%d res=%d src_bytes=%lld", B, res,
                    (long long)src_bytes);
    DANET_CHECK_ARG(src && offsets && shapes && origin && params && out, "batch_crop: null pointer");
    hipLaunchKernelGGL(batch_crop_kernel, dim3(danet::cdiv((long)res * res, kCropThreads), B), dim3(kCropThreads), 0, (hipStream_t)stream,
                       src, (long long)src_bytes, (const long long*)offsets, shapes, origin, params, res, out);
    DANET_CHECK_LAUNCH("batch_crop_kernel");
    return DANET_OK;
}

extern "C" int danet_label_augment(const double* xform, const double* rot_flip, const double* keypoints, const double* smpl_2dkps,
                                   const double* pose_3d, const double* pose, const float* fits, int B, int res, int inverse,
                                   float* keypoints_out, float* smpl_2dkps_out, float* pose_3d_out, float* pose_out,
                                   float* fits_pose_out, float* fits_betas_out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < (1 << 24) && res > 0, "label_augment: bad sizes B=%d res=%d", B, res);
    DANET_CHECK_ARG(rot_flip, "label_augment: null rot_flip");
    DANET_CHECK_ARG(!(keypoints || smpl_2dkps) || xform, "label_augment: 2D keypoints need the crop transform");
    DANET_CHECK_ARG((!keypoints || keypoints_out) && (!smpl_2dkps || smpl_2dkps_out) && (!pose_3d || pose_3d_out) && (!pose || pose_out) &&
                    (!fits || (fits_pose_out && fits_betas_out)), "label_augment: an input without its output");
    DANET_CHECK_ARG(keypoints || smpl_2dkps || pose_3d || pose || fits, "label_augment: nothing to do");
    Perms pm;
    for (int j = 0; j < 25; ++j) pm.j49[j] = kJ25Flip[j];
    for (int j = 0; j < 24; ++j) { pm.j49[25 + j] = (unsigned char)(25 + kJ24Flip[j]); pm.j24[j] = kJ24Flip[j]; pm.smpl[j] = danet::kSmplFlip[j]; }
    hipLaunchKernelGGL(label_augment_kernel, dim3(B), dim3(kLabelThreads), 0, (hipStream_t)stream, xform, rot_flip, keypoints, smpl_2dkps,
                       pose_3d, pose, fits, pm, res, inverse, keypoints_out, smpl_2dkps_out, pose_3d_out, pose_out, fits_pose_out, fits_betas_out);
    DANET_CHECK_LAUNCH("label_augment_kernel");
    return DANET_OK;
}
