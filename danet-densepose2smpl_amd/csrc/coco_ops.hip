// COCO keypoint evaluation ops for gfx950 (the reference's eval_coco.py; evaluate_coco.py is the caller).
//
//   coco_keypoints      eval_coco.py:114-145 for a batch as one launch, one lane per (sample, COCO joint): the joint is picked out of the
//                       49 SMPL joints, translated by the weak-perspective camera's (tx, ty, 2 f / (img_res s + 1e-9)), projected through
//                       a pinhole with identity rotation and a zero principal point, moved by img_res / 2 and taken back into the
//                       original image by the inverse crop affine, which for rot = 0 is a uniform scale of 200 scale / img_res about
//                       the crop centre (DESIGN.md 4c "closed-form affine").  fp32 in, fp64 inside, one rounding to fp32 at the end.
//   coco_oks_match      the per-image part of the COCO keypoint rule for the WHOLE dataset as one launch, one workgroup
//                       per image: the (at most 20) x G matrix of object keypoint similarities in fp64 into LDS, one lane per pair; the
//                       ground truths ordered non-ignored first (stable) per area range; then one lane per (area range, threshold) runs
//                       the greedy matching over its own row of matched flags; then one lane per (detection, range) packs the ten
//                       threshold bits into one 16-bit word.  Launch-bound by design: what matters is that no similarity flips across a
//                       threshold.  Flags are written with plain vector stores.
#include "common.h"

namespace {

constexpr int kCocoJ = 17;
constexpr int kSmplJ = 49;                                     // joints of the SMPL layer; the last 24 are the ground-truth set
constexpr int kMaxDets = DANET_COCO_MAX_DETS;                  // 20
constexpr int kMaxGt = DANET_COCO_MAX_GT;                      // 256
constexpr int kNT = 10;                                        // thresholds
constexpr int kNA = 3;                                         // area ranges
constexpr int kThreads = 256;

__constant__ int kJ24ToCoco[kCocoJ] = {19, 20, 21, 22, 23, 9, 8, 10, 7, 11, 6, 3, 2, 4, 1, 5, 0};      // constants.J24_TO_JCOCO
// (2 sigma)^2 of the COCO keypoint sigmas / 10 is taken in the kernel from these
__constant__ double kSigma[kCocoJ] = {.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89};
__constant__ double kAreaLo[kNA] = {0.0, 32.0 * 32.0, 96.0 * 96.0};
__constant__ double kAreaHi[kNA] = {1e10, 96.0 * 96.0, 1e10};

__global__ void coco_keypoints_kernel(const float* __restrict__ joints, const float* __restrict__ camera,
                                      const float* __restrict__ center, const float* __restrict__ scale,
                                      int B, double img_res, double focal, float* __restrict__ preds)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * kCocoJ) return;
    const int b = i / kCocoJ, j = i - b * kCocoJ;
    const float* p = joints + ((size_t)b * kSmplJ + (kSmplJ - 24) + kJ24ToCoco[j]) * 3;
    const double s = (double)camera[b * 3 + 0];
    const double tz = 2.0 * focal / (img_res * s + 1e-9);
    const double z = (double)p[2] + tz;
    const double u = focal * (((double)p[0] + (double)camera[b * 3 + 1]) / z) + 0.5 * img_res;      // crop pixels
    const double v = focal * (((double)p[1] + (double)camera[b * 3 + 2]) / z) + 0.5 * img_res;
    const double k = 200.0 * (double)scale[b] / img_res;
    preds[(size_t)i * 2 + 0] = (float)((double)center[b * 2 + 0] + (u - 0.5 * img_res) * k);
    preds[(size_t)i * 2 + 1] = (float)((double)center[b * 2 + 1] + (v - 0.5 * img_res) * k);
}

struct Thresholds { double t[kNT]; };

__device__ double oks_pair(const float* __restrict__ d, const double* __restrict__ g, double area, const double* __restrict__ bb) {
    int k1 = 0;
    for (int j = 0; j < kCocoJ; ++j) k1 += g[j * 3 + 2] > 0.0 ? 1 : 0;
    const double x0 = bb[0] - bb[2], x1 = bb[0] + 2.0 * bb[2], y0 = bb[1] - bb[3], y1 = bb[1] + 2.0 * bb[3];
    const double den = area + 2.220446049250313e-16;
    double sum = 0.0;
    for (int j = 0; j < kCocoJ; ++j) {
        const double xd = (double)d[j * 2 + 0], yd = (double)d[j * 2 + 1];
        double dx, dy;
        if (k1 > 0) {
            if (!(g[j * 3 + 2] > 0.0)) continue;
            dx = xd - g[j * 3 + 0];
            dy = yd - g[j * 3 + 1];
        } else {
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
            dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        const double sg = 2.0 * (kSigma[j] / 10.0);
        const double e = (dx * dx + dy * dy) / (sg * sg) / den / 2.0;
        sum += exp(-e);
    }
    return sum / (double)(k1 > 0 ? k1 : kCocoJ);
}

__global__ __launch_bounds__(kThreads) void coco_oks_match_kernel(
    const float* __restrict__ dt_kpts, const double* __restrict__ dt_area, const long long* __restrict__ dt_offsets, long long N,
    const double* __restrict__ gt_kpts, const double* __restrict__ gt_area, const double* __restrict__ gt_bbox,
    const unsigned char* __restrict__ gt_ignore, const unsigned char* __restrict__ gt_iscrowd, const long long* __restrict__ gt_offsets,
    long long M, Thresholds thr, unsigned short* __restrict__ dt_match, unsigned short* __restrict__ dt_ignore, int* __restrict__ gt_count)
{
    __shared__ double oks[kMaxDets * kMaxGt];                            // 40 KB
    __shared__ unsigned char gtm[kNA * kNT][kMaxGt];                     // matched flags, one row per (range, threshold) lane
    __shared__ unsigned char g_ig[kNA][kMaxGt], g_crowd[kMaxGt];
    __shared__ unsigned short order[kNA][kMaxGt];
    __shared__ unsigned char d_m[kNA * kNT][kMaxDets], d_ig[kNA * kNT][kMaxDets];
    const int img = blockIdx.x, tid = threadIdx.x;
    const long long d0 = dt_offsets[img], d1 = dt_offsets[img + 1], g0 = gt_offsets[img], g1 = gt_offsets[img + 1];
    // the host has checked the offsets it was told about (ascending, inside N / M, at most kMaxGt ground truths per image); an image
    // whose offsets on the device say otherwise is left alone rather than read out of bounds (uniform over the block)
    if (d0 < 0 || d1 < d0 || d1 > N || g0 < 0 || g1 < g0 || g1 > M || g1 - g0 > kMaxGt) return;
    const int D = (int)(d1 - d0 < kMaxDets ? d1 - d0 : kMaxDets), G = (int)(g1 - g0);

    for (int k = tid; k < kNA * kNT * kMaxGt; k += kThreads) (&gtm[0][0])[k] = 0;
    if (tid < G) {
        const double a = gt_area[g0 + tid];
        const bool ig = gt_ignore[g0 + tid] != 0;
        g_crowd[tid] = gt_iscrowd[g0 + tid] != 0;
        for (int r = 0; r < kNA; ++r) g_ig[r][tid] = (ig || a < kAreaLo[r] || a > kAreaHi[r]) ? 1 : 0;
    }
    for (int p = tid; p < D * G; p += kThreads) {
        const int d = p / G, g = p - d * G;
        oks[d * kMaxGt + g] = oks_pair(dt_kpts + (size_t)(d0 + d) * kCocoJ * 2, gt_kpts + (size_t)(g0 + g) * kCocoJ * 3,
                                       gt_area[g0 + g], gt_bbox + (size_t)(g0 + g) * 4);
    }
    __syncthreads();
    // stable order, non-ignored first: a ground truth's place is the number of its kind before it (+ all non-ignored, if ignored)
    if (tid < G) {
        for (int r = 0; r < kNA; ++r) {
            int before_keep = 0, before_ig = 0, keep = 0;
            for (int k = 0; k < G; ++k) {
                const int ig = g_ig[r][k];
                keep += 1 - ig;
                if (k < tid) { before_keep += 1 - ig; before_ig += ig; }
            }
            order[r][g_ig[r][tid] ? keep + before_ig : before_keep] = (unsigned short)tid;
            if (tid == 0) gt_count[(size_t)img * kNA + r] = keep;
        }
    }
    if (G == 0 && tid < kNA) gt_count[(size_t)img * kNA + tid] = 0;
    __syncthreads();
    if (tid < kNA * kNT) {
        const int r = tid / kNT, t = tid - r * kNT;
        for (int d = 0; d < D; ++d) {
            double best = fmin(thr.t[t], 1.0 - 1e-10);
            int m = -1;
            for (int k = 0; k < G; ++k) {
                const int g = order[r][k];
                if (gtm[tid][g] && !g_crowd[g]) continue;
                if (m >= 0 && !g_ig[r][m] && g_ig[r][g]) break;
                const double v = oks[d * kMaxGt + g];
                if (v < best) continue;
                best = v;
                m = g;
            }
            if (m >= 0) {
                gtm[tid][m] = 1;
                d_m[tid][d] = 1;
                d_ig[tid][d] = g_ig[r][m];
            } else {
                const double a = dt_area[d0 + d];
                d_m[tid][d] = 0;
                d_ig[tid][d] = (a < kAreaLo[r] || a > kAreaHi[r]) ? 1 : 0;
            }
        }
    }
    __syncthreads();
    if (tid < D * kNA) {
        const int d = tid / kNA, r = tid - d * kNA;
        unsigned mt = 0, ig = 0;
        for (int t = 0; t < kNT; ++t) {
            mt |= (unsigned)d_m[r * kNT + t][d] << t;
            ig |= (unsigned)d_ig[r * kNT + t][d] << t;
        }
        dt_match[(size_t)(d0 + d) * kNA + r] = (unsigned short)mt;
        dt_ignore[(size_t)(d0 + d) * kNA + r] = (unsigned short)ig;
    }
    // a detection past the first kMaxDets of its image: matched nowhere, ignored at every threshold (it counts neither way)
    for (long long p = (long long)D * kNA + tid; p < (d1 - d0) * kNA; p += kThreads) {
        dt_match[(size_t)d0 * kNA + p] = 0;
        dt_ignore[(size_t)d0 * kNA + p] = (unsigned short)((1u << kNT) - 1);
    }
}

}  // namespace

extern "C" int danet_coco_keypoints(const float* joints, const float* camera, const float* center, const float* scale, int B,
                                    int img_res, float focal_length, float* preds, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < (1 << 24) && img_res > 0 && focal_length > 0.0f, "coco_keypoints: bad sizes B=%d img_res=%d focal=%g", B,
                    img_res, (double)focal_length);
    DANET_CHECK_ARG(joints && camera && center && scale && preds, "coco_keypoints: null pointer");
    hipLaunchKernelGGL(coco_keypoints_kernel, dim3(danet::cdiv((long)B * kCocoJ, 256)), dim3(256), 0, (hipStream_t)stream, joints, camera,
                       center, scale, B, (double)img_res, (double)focal_length, preds);
    DANET_CHECK_LAUNCH("coco_keypoints_kernel");
    return DANET_OK;
}

extern "C" int danet_coco_oks_match(const float* dt_kpts, const double* dt_area, const int64_t* dt_offsets, int64_t N,
                                    const double* gt_kpts, const double* gt_area, const double* gt_bbox, const uint8_t* gt_ignore,
                                    const uint8_t* gt_iscrowd, const int64_t* gt_offsets, int64_t M, int num_images, int max_gt,
                                    uint16_t* dt_match, uint16_t* dt_ignore, int32_t* gt_count, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(num_images > 0 && num_images < (1 << 30) && N >= 0 && M >= 0 && max_gt >= 0, "coco_oks_match: bad sizes images=%d N=%lld M=%lld max_gt=%d",
                    num_images, (long long)N, (long long)M, max_gt);
    DANET_CHECK_ARG(max_gt <= kMaxGt, "coco_oks_match: an image has %d ground truths; the similarity matrix in LDS holds at most %d per image",
                    max_gt, kMaxGt);
    DANET_CHECK_ARG(dt_offsets && gt_offsets && gt_count, "coco_oks_match: null pointer");
    DANET_CHECK_ARG(N == 0 || (dt_kpts && dt_area && dt_match && dt_ignore), "coco_oks_match: null detection pointer with N=%lld", (long long)N);
    DANET_CHECK_ARG(M == 0 || (gt_kpts && gt_area && gt_bbox && gt_ignore && gt_iscrowd), "coco_oks_match: null ground-truth pointer with M=%lld", (long long)M);
    Thresholds thr;                                                         // numpy.linspace(0.5, 0.95, 10), operation by operation
    const double step = (0.95 - 0.5) / 9.0;
    for (int t = 0; t < kNT; ++t) thr.t[t] = t == kNT - 1 ? 0.95 : 0.5 + t * step;
    hipLaunchKernelGGL(coco_oks_match_kernel, dim3(num_images), dim3(kThreads), 0, (hipStream_t)stream, dt_kpts, dt_area,
                       (const long long*)dt_offsets, (long long)N, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd,
                       (const long long*)gt_offsets, (long long)M, thr, dt_match, dt_ignore, gt_count);
    DANET_CHECK_LAUNCH("coco_oks_match_kernel");
    return DANET_OK;
}
