// Ground-truth part crops of DANET.INPUT_MODE 'iuv_gt' (/root/reference/models/danet/iuv_estimator.py:64-89): the 3-channel IUV
// image is split into 24 per-joint 7-class maps (part_iuv_simp) and each is resampled by its joint's affine theta (affine_grid +
// grid_sample, bilinear, zero padding).  In this mode theta is NOT detached, so the crops carry a gradient with respect to theta --
// the only path by which the 24 learned ratios / offsets are trained.
//
//   part_gt_kernel       x24[b*24+j, h, w, 0:21] = keep[b,j,c] * resampled (U | V | I) of class c, as bf16 NHWC, channels 21..23 = 0:
//                        the limb regressor's zero-padded first-conv operand (the layout part_ops.hip's part_clean writes).
//                        Extra workgroups of the same launch write the body operand [B,H,W,80] bf16 = [U | V | I | 5 zeros] of
//                        iuvmap_clean(keep25 * iuv_img2map(image)) (the global maps of danet.py:194-205,247).
//   part_gt_bwd_kernel   d theta [B,24,2,3] from d x24: one 1024-thread workgroup per (b, joint), fixed-order reduction (no atomics):
//                        d theta = sum over pixels of (d L / d grid) x (xn, yn, 1), d L / d grid as grid_sample's backward defines it.
//
// The sampling coordinate is computed by ONE helper (sample_coord) in both directions, with FMA contraction off: the forward's
// bilinear weights and the backward's cell choice come from the same bits, and a host-side fp32 emulation reproduces them exactly.
#include "common.h"
#include "conv_common.h"

namespace {

using namespace danet_conv;

constexpr int NJ = 24, NC = 7, NP = 25, MAPC = 80;

struct Coord { float xn, yn, ix, iy; };

// normalised output coordinate of pixel (oh, ow), the sampling grid point theta . (xn, yn, 1), and its unnormalised image
// coordinate -- every operation rounded on its own, in this order
__device__ inline Coord sample_coord(const float* __restrict__ th, int H, int W, int oh, int ow, int align)
{
#pragma clang fp contract(off)
    Coord c;
    if (align) {
        c.xn = W > 1 ? -1.0f + (2.0f * (float)ow) / (float)(W - 1) : 0.0f;
        c.yn = H > 1 ? -1.0f + (2.0f * (float)oh) / (float)(H - 1) : 0.0f;
    } else {
        c.xn = (2.0f * (float)ow + 1.0f) / (float)W - 1.0f;
        c.yn = (2.0f * (float)oh + 1.0f) / (float)H - 1.0f;
    }
    const float gx = th[0] * c.xn + th[1] * c.yn + th[2];
    const float gy = th[3] * c.xn + th[4] * c.yn + th[5];
    if (align) {
        c.ix = (gx + 1.0f) * 0.5f * (float)(W - 1);
        c.iy = (gy + 1.0f) * 0.5f * (float)(H - 1);
    } else {
        c.ix = ((gx + 1.0f) * (float)W - 1.0f) * 0.5f;
        c.iy = ((gy + 1.0f) * (float)H - 1.0f) * 0.5f;
    }
    return c;
}

// the image pixel (xx, yy) as the joint's 7-class simplified maps see it: bit c set = class c (1..6) is the pixel's part
// (sel may name a part twice); class 0 (none of the six) when no bit is set
__device__ inline unsigned tap_classes(float i0, const int* s)
{
    int part = (int)rintf(i0 * 24.f);
    part = part < 0 ? 0 : (part > 24 ? 24 : part);
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) m |= (s[c] == part) ? (2u << c) : 0u;
    return m ? m : 1u;
}

__global__ __launch_bounds__(256) void part_gt_kernel(const float* __restrict__ img, const float* __restrict__ theta,
                                                      const int* __restrict__ sel, const float* __restrict__ keep,
                                                      const float* __restrict__ keep25, int B, int H, int W, int align, int part_blocks,
                                                      bf16_t* __restrict__ x24, bf16_t* __restrict__ body)
{
    const int HW = H * W;
    if ((int)blockIdx.x >= part_blocks) {
        // body operand: one thread per (b, pixel)
        const long i = (long)(blockIdx.x - part_blocks) * 256 + threadIdx.x;
        if (i >= (long)B * HW) return;
        const int b = (int)(i / HW), hw = (int)(i - (long)b * HW);
        const float* im = img + (size_t)b * 3 * HW;
        int part = (int)rintf(im[hw] * 24.f);
        part = part < 0 ? 0 : (part > 24 ? 24 : part);
        const bool kept = keep25 == nullptr || keep25[(size_t)b * NP + part] != 0.f;
        // iuvmap_clean of the dropped maps: a dropped part leaves an all-zero index row, whose arg-max is class 0 (U = V = 0 there)
        const int am = kept ? part : 0;
        const float u = kept ? im[HW + hw] : 0.f, v = kept ? im[2 * HW + hw] : 0.f;
        const float k = kept ? 1.f : 0.f;
        float o[MAPC];
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            o[c] = c == am ? u * k : 0.f;
            o[NP + c] = c == am ? v * k : 0.f;
            o[2 * NP + c] = c == am ? 1.f : 0.f;
        }
#pragma unroll
        for (int c = 3 * NP; c < MAPC; ++c) o[c] = 0.f;
        uint4* dst = reinterpret_cast<uint4*>(body + (size_t)i * MAPC);
#pragma unroll
        for (int q = 0; q < MAPC / 8; ++q) {
            uint4 r;
            r.x = f2bf_pk(o[q * 8 + 0], o[q * 8 + 1]); r.y = f2bf_pk(o[q * 8 + 2], o[q * 8 + 3]);
            r.z = f2bf_pk(o[q * 8 + 4], o[q * 8 + 5]); r.w = f2bf_pk(o[q * 8 + 6], o[q * 8 + 7]);
            dst[q] = r;
        }
        return;
    }
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * NJ * HW) return;
    const int bj = (int)(i / HW), hw = (int)(i - (long)bj * HW);
    const int b = bj / NJ, j = bj - b * NJ;
    const float* im = img + (size_t)b * 3 * HW;
    int s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = sel[j * 6 + c];
    const Coord cd = sample_coord(theta + (size_t)bj * 6, H, W, hw / W, hw % W, align);
    const float fx = floorf(cd.ix), fy = floorf(cd.iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = cd.ix - fx, wy1 = cd.iy - fy;
    float o[24];
#pragma unroll
    for (int c = 0; c < 24; ++c) o[c] = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int xx = x0 + (n & 1), yy = y0 + (n >> 1);
        if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) continue;
        const float wgt = ((n & 1) ? wx1 : 1.f - wx1) * ((n >> 1) ? wy1 : 1.f - wy1);
        const int p = yy * W + xx;
        const unsigned m = tap_classes(im[p], s);
        const float u = im[HW + p], v = im[2 * HW + p];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (m & (1u << c)) {
                if (c > 0) { o[c] += wgt * u; o[NC + c] += wgt * v; }
                o[2 * NC + c] += wgt;
            }
    }
    if (keep) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float k = keep[(size_t)bj * NC + c];
            o[c] *= k; o[NC + c] *= k; o[2 * NC + c] *= k;
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(x24 + (size_t)i * 24);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint4 r;
        r.x = f2bf_pk(o[q * 8 + 0], o[q * 8 + 1]); r.y = f2bf_pk(o[q * 8 + 2], o[q * 8 + 3]);
        r.z = f2bf_pk(o[q * 8 + 4], o[q * 8 + 5]); r.w = f2bf_pk(o[q * 8 + 6], o[q * 8 + 7]);
        dst[q] = r;
    }
}

// one workgroup of BWD_THREADS per (b, joint) (16 waves: B * 24 workgroups alone leave too few waves per compute unit to hide the
// gather latency); thread t walks pixels t, t + BWD_THREADS, ... in order, then a fixed butterfly within each wave and a fixed order over
// the waves: the result does not depend on scheduling (bitwise reproducible, also under graph replay)
constexpr int BWD_THREADS = 1024, BWD_WAVES = BWD_THREADS / 64;

__global__ __launch_bounds__(BWD_THREADS) void part_gt_bwd_kernel(const float* __restrict__ img, const float* __restrict__ theta,
                                                          const int* __restrict__ sel, const float* __restrict__ keep,
                                                          const bf16_t* __restrict__ g24, int H, int W, int align,
                                                          float* __restrict__ dtheta)
{
    const int HW = H * W, bj = blockIdx.x, b = bj / NJ, j = bj - b * NJ, t = threadIdx.x;
    const float* im = img + (size_t)b * 3 * HW;
    const float* th = theta + (size_t)bj * 6;
    int s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = sel[j * 6 + c];
    float k[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) k[c] = keep ? keep[(size_t)bj * NC + c] : 1.f;
    const float mx = align ? 0.5f * (float)(W - 1) : 0.5f * (float)W;       // d ix / d gx
    const float my = align ? 0.5f * (float)(H - 1) : 0.5f * (float)H;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int hw = t; hw < HW; hw += BWD_THREADS) {
        const Coord cd = sample_coord(th, H, W, hw / W, hw % W, align);
        const float fx = floorf(cd.ix), fy = floorf(cd.iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float wx1 = cd.ix - fx, wy1 = cd.iy - fy;
        // d x24 of this pixel, times keep: gU / gV / gI per class
        const uint4* q = reinterpret_cast<const uint4*>(g24 + ((size_t)bj * HW + hw) * 24);
        const uint4 a0 = q[0], a1 = q[1], a2 = q[2];
        const unsigned w[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        float g[24];
#pragma unroll
        for (int e = 0; e < 12; ++e) { g[2 * e] = __builtin_bit_cast(float, w[e] << 16); g[2 * e + 1] = __builtin_bit_cast(float, w[e] & 0xffff0000u); }
        float gix = 0.f, giy = 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int xx = x0 + (n & 1), yy = y0 + (n >> 1);
            if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) continue;
            const int p = yy * W + xx;
            const unsigned m = tap_classes(im[p], s);
            const float u = im[HW + p], v = im[2 * HW + p];
            // d L / d (this tap's weight): the tap's source values dotted with d x24
            float st = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (m & (1u << c)) st += k[c] * (c > 0 ? g[c] * u + g[NC + c] * v + g[2 * NC + c] : g[2 * NC + c]);
            // weight = wx * wy; d wx / d ix = -1 (left tap) / +1 (right tap), likewise for y
            const float wx = (n & 1) ? wx1 : 1.f - wx1, wy = (n >> 1) ? wy1 : 1.f - wy1;
            gix += ((n & 1) ? wy : -wy) * st;
            giy += ((n >> 1) ? wx : -wx) * st;
        }
        const float ggx = gix * mx, ggy = giy * my;
        acc[0] += ggx * cd.xn; acc[1] += ggx * cd.yn; acc[2] += ggx;
        acc[3] += ggy * cd.xn; acc[4] += ggy * cd.yn; acc[5] += ggy;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int e = 0; e < 6; ++e) acc[e] += __shfl_xor(acc[e], o);
    __shared__ float red[6][BWD_WAVES];
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 6; ++e) red[e][wave] = acc[e];
    }
    __syncthreads();
    if (t < 6) {
        float r[BWD_WAVES];
#pragma unroll
        for (int w = 0; w < BWD_WAVES; ++w) r[w] = red[t][w];
#pragma unroll
        for (int n = BWD_WAVES / 2; n >= 1; n >>= 1)
#pragma unroll
            for (int w = 0; w < n; ++w) r[w] += r[w + n];
        dtheta[(size_t)bj * 6 + t] = r[0];
    }
}

}  // namespace

extern "C" int danet_part_gt_forward(const float* iuv_img, const float* theta, const int* sel, const float* keep, const float* keep25,
                                     int B, int H, int W, int align, void* x24, void* body, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(iuv_img && theta && sel && x24 && B > 0 && H > 0 && W > 0, "part_gt_forward: bad arguments");
    DANET_CHECK_ARG((long)B * NJ * H * W < (1L << 31), "part_gt_forward: B*24*H*W too large");
    const int part_blocks = danet::cdiv((long)B * NJ * H * W, 256);
    const int body_blocks = body ? danet::cdiv((long)B * H * W, 256) : 0;
    hipLaunchKernelGGL(part_gt_kernel, dim3((unsigned)(part_blocks + body_blocks)), dim3(256), 0, (hipStream_t)stream,
                       iuv_img, theta, sel, keep, keep25, B, H, W, align, part_blocks, (bf16_t*)x24, (bf16_t*)body);
    DANET_CHECK_LAUNCH("part_gt_kernel");
    return DANET_OK;
}

extern "C" int danet_part_gt_backward(const float* iuv_img, const float* theta, const int* sel, const float* keep, const void* g24,
                                      int B, int H, int W, int align, float* dtheta, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(iuv_img && theta && sel && g24 && dtheta && B > 0 && H > 0 && W > 0, "part_gt_backward: bad arguments");
    hipLaunchKernelGGL(part_gt_bwd_kernel, dim3((unsigned)(B * NJ)), dim3(BWD_THREADS), 0, (hipStream_t)stream,
                       iuv_img, theta, sel, keep, (const bf16_t*)g24, H, W, align, dtheta);
    DANET_CHECK_LAUNCH("part_gt_bwd_kernel");
    return DANET_OK;
}
