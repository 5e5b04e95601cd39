// DensePose-COCO point supervision of the estimator (/root/reference/models/danet/iuv_estimator.py:343-419, called at :106-117) as one
// launch per pass instead of ~25 tensor ops forward and several times that backward:
//
//   dp_losses_fwd   bilinear pooling (grid_sample, zero padding, both align_corners modes) of the U, V and index heads at the <= 196
//                   annotated points of each sample; smooth-L1 of U, V with inside = outside = point weights; 25-way cross-entropy over
//                   all 196 point slots; dense 15-way cross-entropy of the Ann head over the S x S pixels.  Every workgroup writes its
//                   four partial sums as doubles to a row of its own (no atomics, no memset): glue.hip loss_finalize adds the rows in
//                   index order and applies the weights and divisors.
//   dp_losses_bwd   the gradient w.r.t. the four head outputs, every element written (pad channels, pixels without a point, samples
//                   without labels: zeros).  Several points may share a pixel, and no floating-point atomics are used: one workgroup
//                   owns a strip of rows of one sample, keeps the strip's U / V / index gradient in LDS, and one THREAD owns one
//                   (map, channel) column of it -- it walks the sample's 196 points in index order and adds the taps that land in the
//                   strip, so every address sees its additions in a fixed order from a single thread.  The Ann gradient is per pixel.
//
// Head tensors are fp32 NHWC with the conv epilogue's padded channel stride (32 floats for U / V / index, 16 for Ann): a tap is 32
// contiguous floats.  A sample with has_dp <= 0 contributes exact zeros to the sums and gets exact zero gradients.
// (compiled with -ffp-contract=off: the sampling coordinates follow grid_sample's arithmetic operation by operation)
#include "common.h"

namespace {

constexpr int NP = 25, NA = 15, NPT = 196, LD = 32, LDA = 16;
constexpr int FWD_PIX = 1024;                 // Ann pixels per forward workgroup (256 threads x 4)
constexpr int BWD_THREADS = 128;              // 96 column owners (3 maps x 32 channels) + 32 that only help with the copy-out

__device__ inline float smooth_l1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ inline float smooth_l1_grad(float d) { return d >= 1.f ? 1.f : (d <= -1.f ? -1.f : d); }

// pixel coordinate of an annotated point -> first tap index and the two tap weights along one axis: grid = (p - S/2) * (2/S)
// (iuv_estimator.py:372-374), then grid_sample's un-normalisation and its (i0 + 1 - i, i - i0) weights.  i0 is clamped to [-2, S]:
// beyond that no tap is inside the map (and the weights are never used); a NaN coordinate lands there too.
__device__ inline void axis_taps(float p, int S, int align, int& i0, float& w0, float& w1)
{
    const float g = (p - (float)S / 2.f) * (2.f / (float)S);
    const float i = align ? ((g + 1.f) / 2.f) * (float)(S - 1) : ((g + 1.f) * (float)S - 1.f) / 2.f;
    const float f = fminf(fmaxf(floorf(i), -2.f), (float)S);
    i0 = (int)f;
    w0 = (f + 1.f) - i;
    w1 = i - f;
}

struct Taps {
    int off[4];          // pixel index y * S + x of the nw, ne, sw, se taps; -1: outside the map
    float w[4];
    int y0;
};

__device__ inline Taps point_taps(float x, float y, int S, int align)
{
    int x0, y0;
    float wx[2], wy[2];
    axis_taps(x, S, align, x0, wx[0], wx[1]);
    axis_taps(y, S, align, y0, wy[0], wy[1]);
    Taps t;
    t.y0 = y0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dx = k & 1, dy = k >> 1, xx = x0 + dx, yy = y0 + dy;
        t.off[k] = (xx >= 0 && xx < S && yy >= 0 && yy < S) ? yy * S + xx : -1;
        t.w[k] = wx[dx] * wy[dy];
    }
    return t;
}

// the 25 pooled channels of one map at one point (map: the sample's [S*S][LD] rows)
__device__ inline void pool25(const float* __restrict__ map, const Taps& t, float* o)
{
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        float4 a{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.off[k] >= 0) {
                const float4 f = reinterpret_cast<const float4*>(map + (size_t)t.off[k] * LD)[q];
                a.x += f.x * t.w[k]; a.y += f.y * t.w[k]; a.z += f.z * t.w[k]; a.w += f.w * t.w[k];
            }
        o[4 * q] = a.x;
        if (q < 6) { o[4 * q + 1] = a.y; o[4 * q + 2] = a.z; o[4 * q + 3] = a.w; }
    }
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void dp_losses_fwd_kernel(
    const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ ix, const float* __restrict__ an,
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ I, const float* __restrict__ TU,
    const float* __restrict__ TV, const float* __restrict__ PW, const int* __restrict__ ann_labels, const float* __restrict__ has_dp,
    int S, int align, int nchunks, double* __restrict__ partial /* [B * nchunks][4] */)
{
    __shared__ double sred[4][4];
    const int b = blockIdx.x / nchunks, c = blockIdx.x - b * nchunks, t = threadIdx.x;
    const int HW = S * S;
    double l[4] = {0., 0., 0., 0.};
    if (has_dp[b] > 0.f) {                                           // (uniform per workgroup)
        const int ppb = (NPT + nchunks - 1) / nchunks, p = c * ppb + t;
        if (t < ppb && p < NPT) {
            const Taps tp = point_taps(X[b * NPT + p], Y[b * NPT + p], S, align);
            const size_t mo = (size_t)b * HW * LD;
            const float* pw = PW + (size_t)b * NP * NPT + p;
            float val[NP];
            pool25(u + mo, tp, val);
            const float* tg = TU + (size_t)b * NP * NPT + p;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < NP; ++k) { const float wk = pw[k * NPT]; s += wk * smooth_l1(wk * val[k] - wk * tg[k * NPT]); }
            l[0] = s;
            pool25(v + mo, tp, val);
            tg = TV + (size_t)b * NP * NPT + p;
            s = 0.f;
#pragma unroll
            for (int k = 0; k < NP; ++k) { const float wk = pw[k * NPT]; s += wk * smooth_l1(wk * val[k] - wk * tg[k * NPT]); }
            l[1] = s;
            pool25(ix + mo, tp, val);
            const int lab = clampi((int)I[b * NPT + p], 0, NP - 1);
            float m = val[0], at = 0.f, se = 0.f;
#pragma unroll
            for (int k = 1; k < NP; ++k) m = fmaxf(m, val[k]);
#pragma unroll
            for (int k = 0; k < NP; ++k) { se += expf(val[k] - m); if (k == lab) at = val[k]; }
            l[2] = (m + logf(se)) - at;
        }
        float sa = 0.f;
#pragma unroll
        for (int q = 0; q < FWD_PIX / 256; ++q) {
            const int pix = c * FWD_PIX + q * 256 + t;
            if (pix < HW) {
                const float4* row = reinterpret_cast<const float4*>(an + ((size_t)b * HW + pix) * LDA);
                const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
                const float A[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
                const int lab = clampi(ann_labels[(size_t)b * HW + pix], 0, NA - 1);
                float m = A[0], at = 0.f, se = 0.f;
#pragma unroll
                for (int k = 1; k < NA; ++k) m = fmaxf(m, A[k]);
#pragma unroll
                for (int k = 0; k < NA; ++k) { se += expf(A[k] - m); if (k == lab) at = A[k]; }
                sa += (m + logf(se)) - at;
            }
        }
        l[3] = sa;
    }
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double s = wave_sum(l[i]); if (lane == 0) sred[wv][i] = s; }
    __syncthreads();
    if (t < 4) partial[(size_t)blockIdx.x * 4 + t] = (sred[0][t] + sred[1][t]) + (sred[2][t] + sred[3][t]);
}

extern __shared__ __attribute__((aligned(16))) float dp_smem[];

__global__ __launch_bounds__(BWD_THREADS) void dp_losses_bwd_kernel(
    const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ ix, const float* __restrict__ an,
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ I, const float* __restrict__ TU,
    const float* __restrict__ TV, const float* __restrict__ PW, const int* __restrict__ ann_labels, const float* __restrict__ has_dp,
    const float* __restrict__ coef, int S, int align, int R, int nstrips,
    float* __restrict__ du, float* __restrict__ dv, float* __restrict__ di, float* __restrict__ da)
{
    const int b = blockIdx.x / nstrips, st = blockIdx.x - b * nstrips, t = threadIdx.x;
    const int HW = S * S, r0 = st * R, rows = min(R, S - r0), npix = rows * S;
    const size_t p0 = (size_t)b * HW + (size_t)r0 * S;               // first pixel of the strip
    float4* const outs[3] = {reinterpret_cast<float4*>(du + p0 * LD), reinterpret_cast<float4*>(dv + p0 * LD), reinterpret_cast<float4*>(di + p0 * LD)};
    float4* const oa = reinterpret_cast<float4*>(da + p0 * LDA);
    if (!(has_dp[b] > 0.f)) {                                        // (uniform per workgroup) no labels: exact zeros
        const float4 z{0.f, 0.f, 0.f, 0.f};
        for (int i = t; i < npix * (LD / 4); i += BWD_THREADS) { outs[0][i] = z; outs[1][i] = z; outs[2][i] = z; }
        for (int i = t; i < npix * (LDA / 4); i += BWD_THREADS) oa[i] = z;
        return;
    }
    float* const g = dp_smem;                                        // [3][R * S][LD]
    float* const sX = dp_smem + (size_t)3 * R * S * LD;
    float* const sY = sX + NPT;
    int* const sL = reinterpret_cast<int*>(sY + NPT);
    {
        float4* g4 = reinterpret_cast<float4*>(g);
        const float4 z{0.f, 0.f, 0.f, 0.f};
        for (int i = t; i < 3 * R * S * (LD / 4); i += BWD_THREADS) g4[i] = z;
        for (int i = t; i < NPT; i += BWD_THREADS) {
            sX[i] = X[b * NPT + i];
            sY[i] = Y[b * NPT + i];
            sL[i] = clampi((int)I[b * NPT + i], 0, NP - 1);
        }
    }
    __syncthreads();
    {
        const int m = t >> 5, ch = t & 31, mm = m < 2 ? m : 2;       // threads 96..127 shadow the index group and store nothing
        const float* map = (mm == 0 ? u : (mm == 1 ? v : ix)) + (size_t)b * HW * LD + ch;
        const float* tgt = (mm == 0 ? TU : TV) + (size_t)b * NP * NPT + (size_t)(ch < NP ? ch : 0) * NPT;
        const float* pwp = PW + (size_t)b * NP * NPT + (size_t)(ch < NP ? ch : 0) * NPT;
        const float cf = coef[mm];
        float* const gcol = g + (size_t)mm * R * S * LD + ch;
        for (int p = 0; p < NPT; ++p) {
            const Taps tp = point_taps(sX[p], sY[p], S, align);
            if (tp.y0 + 1 < r0 || tp.y0 >= r0 + rows) continue;       // (uniform) neither tap row in this strip
            float val = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (tp.off[k] >= 0) val += map[(size_t)tp.off[k] * LD] * tp.w[k];
            float gp = 0.f;
            if ((t >> 6) == 0) {                                     // U and V: smooth-L1 with inside = outside = the point weights
                if (ch < NP) { const float wk = pwp[p]; gp = cf * wk * wk * smooth_l1_grad(wk * val - wk * tgt[p]); }
            } else {                                                 // index: softmax over the group's 25 valid lanes
                const float z = ch < NP ? val : -3.0e38f;
                float mx = z;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
                const float e = ch < NP ? expf(z - mx) : 0.f;
                float se = e;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) se += __shfl_xor(se, o, 32);
                if (ch < NP) gp = cf * (e / se - (ch == sL[p] ? 1.f : 0.f));
            }
            if (m < 3) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int yy = tp.y0 + (k >> 1);
                    if (tp.off[k] >= 0 && yy >= r0 && yy < r0 + rows) gcol[(size_t)(tp.off[k] - r0 * S) * LD] += tp.w[k] * gp;
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int mp = 0; mp < 3; ++mp) {
        const float4* src = reinterpret_cast<const float4*>(g + (size_t)mp * R * S * LD);
        for (int i = t; i < npix * (LD / 4); i += BWD_THREADS) outs[mp][i] = src[i];
    }
    const float ca = coef[3];
    for (int pix = t; pix < npix; pix += BWD_THREADS) {
        const float4* row = reinterpret_cast<const float4*>(an + (p0 + pix) * LDA);
        const float4 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
        float A[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
        const int lab = clampi(ann_labels[p0 + pix], 0, NA - 1);
        float m = A[0], se = 0.f;
#pragma unroll
        for (int k = 1; k < NA; ++k) m = fmaxf(m, A[k]);
#pragma unroll
        for (int k = 0; k < NA; ++k) { A[k] = expf(A[k] - m); se += A[k]; }
#pragma unroll
        for (int k = 0; k < NA; ++k) A[k] = ca * (A[k] / se - (k == lab ? 1.f : 0.f));
        A[15] = 0.f;
        float4* o = oa + (size_t)pix * (LDA / 4);
        o[0] = float4{A[0], A[1], A[2], A[3]}; o[1] = float4{A[4], A[5], A[6], A[7]};
        o[2] = float4{A[8], A[9], A[10], A[11]}; o[3] = float4{A[12], A[13], A[14], A[15]};
    }
}

inline int strip_rows(int S) { return S >= 128 ? 1 : 128 / S; }       // 3 maps x R x S x 128 bytes <= 48 KiB of LDS

}  // namespace

extern "C" int danet_dp_point_losses_rows(int B, int S)
{
    return (B > 0 && S > 0) ? B * danet::cdiv((long)S * S, FWD_PIX) : 0;
}

extern "C" int danet_dp_point_losses_forward(const float* u, const float* v, const float* ix, const float* an, int ld, int lda,
                                             const float* X, const float* Y, const float* I, const float* TU, const float* TV, const float* PW,
                                             const int* ann_labels, const float* has_dp, int B, int S, int align, double* partial, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(u && v && ix && an && X && Y && I && TU && TV && PW && ann_labels && has_dp && partial && B > 0 && S > 0 && S <= 4096,
                    "dp_point_losses_forward: bad arguments");
    DANET_CHECK_ARG(ld == LD && lda == LDA, "dp_point_losses_forward: channel strides %d / %d (32 / 16 expected)", ld, lda);
    const int nchunks = danet::cdiv((long)S * S, FWD_PIX);
    hipLaunchKernelGGL(dp_losses_fwd_kernel, dim3(B * nchunks), dim3(256), 0, (hipStream_t)stream, u, v, ix, an, X, Y, I, TU, TV, PW,
                       ann_labels, has_dp, S, align ? 1 : 0, nchunks, partial);
    DANET_CHECK_LAUNCH("dp_losses_fwd_kernel");
    return DANET_OK;
}

extern "C" int danet_dp_point_losses_backward(const float* u, const float* v, const float* ix, const float* an, int ld, int lda,
                                              const float* X, const float* Y, const float* I, const float* TU, const float* TV, const float* PW,
                                              const int* ann_labels, const float* has_dp, const float* coef, int B, int S, int align,
                                              float* du, float* dv, float* di, float* da, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(u && v && ix && an && X && Y && I && TU && TV && PW && ann_labels && has_dp && coef && du && dv && di && da && B > 0 && S > 0,
                    "dp_point_losses_backward: bad arguments");
    DANET_CHECK_ARG(ld == LD && lda == LDA, "dp_point_losses_backward: channel strides %d / %d (32 / 16 expected)", ld, lda);
    DANET_CHECK_ARG(S <= 128, "dp_point_losses_backward: map size %d (a row of the three gradient maps must fit 48 KiB of LDS: S <= 128)", S);
    const int R = strip_rows(S), nstrips = danet::cdiv(S, R);
    const size_t lds = ((size_t)3 * R * S * LD + 3 * NPT) * sizeof(float);
    hipLaunchKernelGGL(dp_losses_bwd_kernel, dim3(B * nstrips), dim3(BWD_THREADS), lds, (hipStream_t)stream, u, v, ix, an, X, Y, I, TU, TV, PW,
                       ann_labels, has_dp, coef, S, align ? 1 : 0, R, nstrips, du, dv, di, da);
    DANET_CHECK_LAUNCH("dp_losses_bwd_kernel");
    return DANET_OK;
}
