// Scoring ops of the evaluation pipeline for gfx950 (the reference's eval.py; evaluate.py is the caller).
//
//   pose_eval           eval.py:183-216 + utils/pose_utils.py:10-58 as one launch, one workgroup per sample: the 17 x V joint
//                       regression as a block reduction (every lane walks vertices tid, tid + 256, ...: the regressor rows and the
//                       vertices are read as consecutive words by consecutive lanes; the regressor stays in L2 across workgroups),
//                       then one lane centres, maps, takes the MPJPE and solves the Procrustes problem in fp64: Jacobi on the
//                       symmetric K^T K gives V and the order of the singular values, U follows from K V, and the last singular
//                       pair takes the sign that makes det R = +1 (the reference's Z).  HBM / latency bound, no MFMA.
//   vertex_eval         the PVE rule of DESIGN.md 4c as one launch, one workgroup per sample: three passes over the two meshes (they
//                       stay in L2: 2 x 82.7 KB at V = 6890), every sum in fp64 through the block sum pose_eval uses -- pelvis dot
//                       products and centroids; K, var1 and the pelvis-centred distance (PVE); one lane solves the Procrustes problem
//                       with pose_eval's solver and publishes s R and t through LDS; the aligned distance (PA-PVE).
//   seg_confusion       eval.py:222-266 for a batch as one launch: one lane per label pixel looks its predicted value up through
//                       the paste rectangle and the two nearest-neighbour index tables of the uncrop rule, so no
//                       uncropped image exists.  Counts are wave ballots + popcounts kept in wave-uniform registers over the
//                       block's pixel chunk, then one LDS atomic per counter and wave, then one global atomic per counter and
//                       block.  All sums are integers: the result does not depend on the order.
//   rotmat_to_angle_axis  the inverse of batch_rodrigues under the rule of DESIGN.md ("axis-angle rule"), one lane per matrix.
#include "common.h"
#include "rotation.h"

namespace {

constexpr int kNJ = 17;                 // rows of the H36M joint regressor
constexpr int kPoseThreads = 256;

struct Mapper { int idx[kNJ]; };

// sum over the 64 lanes of a wave; the result is valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sums of N values per lane over the block, in fp64: every lane reads them from out[0..N) afterwards.  `red` holds 4 x N doubles
// and may be reused by the next call (the closing barrier orders its reads before the next writes).
template <int N, typename Acc, typename Out>
__device__ __forceinline__ void block_sum(const Acc* __restrict__ acc, double* __restrict__ red, Out* __restrict__ out) {
    static_assert(N <= kPoseThreads, "one lane per sum adds the four waves' partial sums");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double s = wave_sum((double)acc[k]);
        if (lane == 0) red[wave * N + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        out[k] = (Out)(red[k] + red[N + k] + red[2 * N + k] + red[3 * N + k]);
    }
    __syncthreads();
}

__device__ void regress17(const float* __restrict__ verts, const float* __restrict__ Jr, int V, double* __restrict__ red /* [4][51] */,
                          float* __restrict__ out /* LDS [51] */)
{
    float acc[kNJ * 3];
#pragma unroll
    for (int k = 0; k < kNJ * 3; ++k) acc[k] = 0.0f;
    for (int v = threadIdx.x; v < V; v += kPoseThreads) {
        const float x = verts[v * 3 + 0], y = verts[v * 3 + 1], z = verts[v * 3 + 2];
#pragma unroll
        for (int j = 0; j < kNJ; ++j) {
            const float w = Jr[(size_t)j * V + v];
            acc[j * 3 + 0] += w * x;
            acc[j * 3 + 1] += w * y;
            acc[j * 3 + 2] += w * z;
        }
    }
    block_sum<kNJ * 3>(acc, red, out);
}

// eigenvectors of the symmetric 3 x 3 matrix A (destroyed) by cyclic Jacobi rotations: A -> diagonal, E -> columns
__device__ void jacobi3(double A[3][3], double E[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) E[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {                       // A <- A G
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {                       // A <- G^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double ekp = E[k][p], ekq = E[k][q];
                    E[k][p] = c * ekp - s * ekq;
                    E[k][q] = s * ekp + c * ekq;
                }
            }
    }
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ bool normalize3(double* a) {
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (!(n > 0.0)) return false;
    a[0] /= n; a[1] /= n; a[2] /= n;
    return true;
}

// a unit vector orthogonal to the unit vector a
__device__ __forceinline__ void any_orthogonal(const double* a, double* o) {
    const int k = fabs(a[0]) <= fabs(a[1]) ? (fabs(a[0]) <= fabs(a[2]) ? 0 : 2) : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
    double e[3] = {0.0, 0.0, 0.0};
    e[k] = 1.0;
    cross3(a, e, o);
    normalize3(o);
}

// steps 4-6 of pose_utils.py:10-58 on one lane: from K = X1 X2^T, var1 = sum |X1|^2 and the two centroids the rotation R with
// det R = +1, the translation t and (returned) the scale of the best similarity transform of set 1 onto set 2
__device__ double similarity_solve(const double K[3][3], double var1, const double* mu1, const double* mu2, double R[3][3], double* t) {
    // K = U S V^T: V and S^2 from K^T K
    double A[3][3], E[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[a][b] = K[0][a] * K[0][b] + K[1][a] * K[1][b] + K[2][a] * K[2][b];
    jacobi3(A, E);
    int o0 = 0, o1 = 1, o2 = 2;                                             // descending eigenvalues
    if (A[o0][o0] < A[o1][o1]) { const int s = o0; o0 = o1; o1 = s; }
    if (A[o0][o0] < A[o2][o2]) { const int s = o0; o0 = o2; o2 = s; }
    if (A[o1][o1] < A[o2][o2]) { const int s = o1; o1 = o2; o2 = s; }
    double v0[3] = {E[0][o0], E[1][o0], E[2][o0]}, v1[3] = {E[0][o1], E[1][o1], E[2][o1]}, v2[3];
    cross3(v0, v1, v2);
    double u0[3], u1[3], u2[3];
    for (int a = 0; a < 3; ++a) {
        u0[a] = K[a][0] * v0[0] + K[a][1] * v0[1] + K[a][2] * v0[2];
        u1[a] = K[a][0] * v1[0] + K[a][1] * v1[1] + K[a][2] * v1[2];
    }
    if (!normalize3(u0)) { u0[0] = 1.0; u0[1] = 0.0; u0[2] = 0.0; }          // K = 0: any rotation is optimal
    const double d = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
    for (int a = 0; a < 3; ++a) u1[a] -= d * u0[a];
    if (!normalize3(u1)) any_orthogonal(u0, u1);                            // rank one
    cross3(u0, u1, u2);
    // R = V Z U^T with det R = +1: both triples are right-handed, so the third pair carries the sign of Z
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[a][b] = v0[a] * u0[b] + v1[a] * u1[b] + v2[a] * u2[b];
    double tr = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) tr += R[a][b] * K[b][a];                // trace(R K)
    const double scale = tr / var1;
    for (int a = 0; a < 3; ++a) t[a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
    return scale;
}

// pose_utils.py:10-58 for S1, S2 [J][3] fp32 (J <= 17): the mean distance between S2 and S1 under the best similarity transform
__device__ double procrustes_error(const float* __restrict__ S1, const float* __restrict__ S2, int J) {
    double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int k = 0; k < 3; ++k) { mu1[k] += (double)S1[j * 3 + k]; mu2[k] += (double)S2[j * 3 + k]; }
    for (int k = 0; k < 3; ++k) { mu1[k] /= J; mu2[k] /= J; }
    double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
    for (int j = 0; j < J; ++j) {
        double x1[3], x2[3];
        for (int k = 0; k < 3; ++k) { x1[k] = (double)S1[j * 3 + k] - mu1[k]; x2[k] = (double)S2[j * 3 + k] - mu2[k]; }
        for (int a = 0; a < 3; ++a) {
            var1 += x1[a] * x1[a];
            for (int b = 0; b < 3; ++b) K[a][b] += x1[a] * x2[b];          // K = X1 X2^T
        }
    }
    double R[3][3], t[3];
    const double scale = similarity_solve(K, var1, mu1, mu2, R, t);
    double err = 0.0;
    for (int j = 0; j < J; ++j) {
        double e2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double h = scale * (R[a][0] * (double)S1[j * 3 + 0] + R[a][1] * (double)S1[j * 3 + 1] + R[a][2] * (double)S1[j * 3 + 2]) + t[a];
            const double df = h - (double)S2[j * 3 + a];
            e2 += df * df;
        }
        err += sqrt(e2);
    }
    return err / J;
}

__global__ __launch_bounds__(kPoseThreads) void pose_eval_kernel(
    const float* __restrict__ pred_vertices, const float* __restrict__ Jr, Mapper mapper, int J,
    const float* __restrict__ gt_kp, const float* __restrict__ gt_vertices, int V,
    float* __restrict__ mpjpe, float* __restrict__ recon, float* __restrict__ joints17)
{
    __shared__ double red[4 * kNJ * 3];
    __shared__ float pj[kNJ * 3], gj[kNJ * 3];
    __shared__ float s1[kNJ * 3], s2[kNJ * 3];
    const int b = blockIdx.x;
    regress17(pred_vertices + (size_t)b * V * 3, Jr, V, red, pj);
    if (threadIdx.x < kNJ * 3) joints17[(size_t)b * kNJ * 3 + threadIdx.x] = pj[threadIdx.x];
    if (gt_vertices) regress17(gt_vertices + (size_t)b * V * 3, Jr, V, red, gj);
    if (threadIdx.x < J * 3) {
        const int j = threadIdx.x / 3, k = threadIdx.x - j * 3;
        const int m = mapper.idx[j];
        s1[threadIdx.x] = pj[m * 3 + k] - pj[k];                              // centred on the regressed pelvis (joint 0)
        s2[threadIdx.x] = gt_vertices ? gj[m * 3 + k] - gj[k] : gt_kp[(size_t)b * J * 3 + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int j = 0; j < J; ++j) {
            double e2 = 0.0;
            for (int k = 0; k < 3; ++k) { const double df = (double)s1[j * 3 + k] - (double)s2[j * 3 + k]; e2 += df * df; }
            e += sqrt(e2);
        }
        mpjpe[b] = (float)(e / J);
        recon[b] = (float)procrustes_error(s1, s2, J);
    }
}

// The PVE rule.  P, G: the sample's two meshes, pel: row 0 of the H36M regressor.
__global__ __launch_bounds__(kPoseThreads) void vertex_eval_kernel(
    const float* __restrict__ pred_vertices, const float* __restrict__ gt_vertices, const float* __restrict__ pel, int V,
    float* __restrict__ pve, float* __restrict__ pa_pve)
{
    __shared__ double red[4 * 12];
    __shared__ double s1[12], s2[11], s3[1];
    __shared__ double xf[12];                                                // s R (row-major), then t
    const int b = blockIdx.x;
    const float* __restrict__ P = pred_vertices + (size_t)b * V * 3;
    const float* __restrict__ G = gt_vertices + (size_t)b * V * 3;
    // pass 1: pel . P, pel . G, sum P, sum G
    double a1[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a1[k] = 0.0;
    for (int v = threadIdx.x; v < V; v += kPoseThreads) {
        const double w = (double)pel[v];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = (double)P[v * 3 + k], g = (double)G[v * 3 + k];
            a1[k] += w * p;
            a1[3 + k] += w * g;
            a1[6 + k] += p;
            a1[9 + k] += g;
        }
    }
    block_sum<12>(a1, red, s1);
    double pp[3], gp[3], mu1[3], mu2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pp[k] = s1[k]; gp[k] = s1[3 + k]; mu1[k] = s1[6 + k] / V; mu2[k] = s1[9 + k] / V; }
    // pass 2: K = sum (p - mu1)(g - mu2)^T, var1 = sum |p - mu1|^2, and the distance of the pelvis-centred meshes
    double a2[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) a2[k] = 0.0;
    for (int v = threadIdx.x; v < V; v += kPoseThreads) {
        double x1[3], x2[3], e2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = (double)P[v * 3 + k], g = (double)G[v * 3 + k];
            x1[k] = p - mu1[k];
            x2[k] = g - mu2[k];
            const double df = (p - pp[k]) - (g - gp[k]);
            e2 += df * df;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a2[9] += x1[i] * x1[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) a2[i * 3 + j] += x1[i] * x2[j];
        }
        a2[10] += sqrt(e2);
    }
    block_sum<11>(a2, red, s2);
    if (threadIdx.x == 0) {
        pve[b] = (float)(s2[10] / V);
        double K[3][3], R[3][3], t[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) K[i][j] = s2[i * 3 + j];
        const double scale = similarity_solve(K, s2[9], mu1, mu2, R, t);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) xf[i * 3 + j] = scale * R[i][j];
            xf[9 + i] = t[i];
        }
    }
    __syncthreads();
    // pass 3: the distance after the alignment
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = xf[k];
    double a3[1] = {0.0};
    for (int v = threadIdx.x; v < V; v += kPoseThreads) {
        const double x = (double)P[v * 3 + 0], y = (double)P[v * 3 + 1], z = (double)P[v * 3 + 2];
        double e2 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double df = (m[i * 3 + 0] * x + m[i * 3 + 1] * y + m[i * 3 + 2] * z + m[9 + i]) - (double)G[v * 3 + i];
            e2 += df * df;
        }
        a3[0] += sqrt(e2);
    }
    block_sum<1>(a3, red, s3);
    if (threadIdx.x == 0) pa_pve[b] = (float)(s3[0] / V);
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kSegThreads = 256;
constexpr int kSegChunk = 4096;           // label pixels per block
constexpr int kNC = 32;                   // counters (include/danet_hip.h DANET_SEG_*)

__device__ __forceinline__ int popc(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(kSegThreads) void seg_confusion_kernel(
    const float* __restrict__ mask, const long long* __restrict__ parts,
    const unsigned char* __restrict__ gt_mask, const unsigned char* __restrict__ gt_parts, long long label_bytes,
    const long long* __restrict__ offsets, const int* __restrict__ shapes, const int* __restrict__ rects,
    const int* __restrict__ tables, int table_len, int res, unsigned long long* __restrict__ counters)
{
    __shared__ int blk[kNC];
    const int b = blockIdx.y;
    const int H = shapes[b * 2 + 0], W = shapes[b * 2 + 1];
    const long long npix = (long long)H * W;
    const long long first = (long long)blockIdx.x * kSegChunk;
    if (first >= npix || H <= 0 || W <= 0) return;                           // (uniform over the block)
    if (threadIdx.x < kNC) blk[threadIdx.x] = 0;
    __syncthreads();
    const long long base = offsets[b];
    const int y0 = rects[b * 6 + 0], y1 = rects[b * 6 + 1], x0 = rects[b * 6 + 2], x1 = rects[b * 6 + 3];
    const int* rt = tables + rects[b * 6 + 4];
    const int* ct = tables + rects[b * 6 + 5];
    const int rt_room = table_len - rects[b * 6 + 4], ct_room = table_len - rects[b * 6 + 5];
    int cnt[kNC];                                                            // wave-uniform
#pragma unroll
    for (int k = 0; k < kNC; ++k) cnt[k] = 0;
    for (int it = 0; it < kSegChunk / kSegThreads; ++it) {
        const long long p = first + it * kSegThreads + threadIdx.x;
        const bool live = p < npix && base >= 0 && base + p < label_bytes;
        if (!__any(live)) break;
        int sy = -1, sx = -1;                                                // source pixel of the rendered images, -1: outside the paste
        if (live) {
            const int y = (int)(p / W), x = (int)(p - (long long)y * W);
            if (y >= y0 && y < y1 && x >= x0 && x < x1 && rects[b * 6 + 4] >= 0 && rects[b * 6 + 5] >= 0 &&
                y - y0 < rt_room && x - x0 < ct_room) {
                sy = rt[y - y0];
                sx = ct[x - x0];
                if (sy < 0 || sy >= res || sx < 0 || sx >= res) sy = sx = -1;
            }
        }
        const size_t src = (size_t)b * res * res + (sy >= 0 ? sy * res + sx : 0);
        if (gt_mask) {
            const bool g = live && gt_mask[base + p] > 0;
            const bool q = live && sy >= 0 && mask[src] > 0.0f;
            const int n11 = popc(g && q), n10 = popc(g && !q), n01 = popc(live && !g && q), n00 = popc(live && !g && !q);
            cnt[DANET_SEG_TP + 0] += n00; cnt[DANET_SEG_FP + 0] += n10; cnt[DANET_SEG_FN + 0] += n01;
            cnt[DANET_SEG_TP + 1] += n11; cnt[DANET_SEG_FP + 1] += n01; cnt[DANET_SEG_FN + 1] += n10;
            cnt[DANET_SEG_ACC] += n00 + n11;
        }
        if (gt_parts) {
            const int g = live ? (int)gt_parts[base + p] : -1;
            const int q = live ? (sy >= 0 ? (int)(unsigned char)parts[src] : 0) : -2;     // (astype(uint8), as eval.py:250)
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const bool cg = g == c, cp = q == c && g != 255;
                cnt[DANET_SEG_PARTS_TP + c] += popc(cg && cp);
                cnt[DANET_SEG_PARTS_FP + c] += popc(live && !cg && cp);
                cnt[DANET_SEG_PARTS_FN + c] += popc(cg && !cp);
            }
            cnt[DANET_SEG_PARTS_ACC] += popc(live && (g == 255 ? 0 : g) == (q == 255 ? 0 : q));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kNC; ++k)
            if (cnt[k]) atomicAdd(&blk[k], cnt[k]);
    }
    __syncthreads();
    if (threadIdx.x < kNC) {
        unsigned long long v = (unsigned long long)blk[threadIdx.x];
        if (blockIdx.x == 0) {                                               // the image's size once per sample
            if (threadIdx.x == DANET_SEG_PIXELS && gt_mask) v = (unsigned long long)npix;
            if (threadIdx.x == DANET_SEG_PARTS_PIXELS && gt_parts) v = (unsigned long long)npix;
        }
        if (v) atomicAdd(&counters[threadIdx.x], v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ void rotmat_to_angle_axis_kernel(const float* __restrict__ Rm, int N, float* __restrict__ aa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    danet::rotmat_to_angle_axis<float>(Rm + (size_t)i * 9, aa + (size_t)i * 3);      // (rotation.h: shared with input_ops.hip)
}

}  // namespace

extern "C" int danet_pose_eval(const float* pred_vertices, const float* J_regressor, const int32_t* joint_mapper, int J,
                               const float* gt_keypoints_3d, const float* gt_vertices, int B, int V,
                               float* mpjpe, float* recon_err, float* pred_joints17, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < (1 << 24) && V > 0 && V < (1 << 24), "pose_eval: bad sizes B=%d V=%d", B, V);
    DANET_CHECK_ARG(J >= 3 && J <= kNJ, "pose_eval: %d mapped joints (3..17)", J);
    DANET_CHECK_ARG(pred_vertices && J_regressor && joint_mapper && mpjpe && recon_err && pred_joints17, "pose_eval: null pointer");
    DANET_CHECK_ARG((gt_keypoints_3d != nullptr) != (gt_vertices != nullptr), "pose_eval: give exactly one of gt_keypoints_3d / gt_vertices");
    Mapper m;
    for (int j = 0; j < kNJ; ++j) m.idx[j] = 0;
    for (int j = 0; j < J; ++j) {
        DANET_CHECK_ARG(joint_mapper[j] >= 0 && joint_mapper[j] < kNJ, "pose_eval: joint_mapper[%d] = %d", j, joint_mapper[j]);
        m.idx[j] = joint_mapper[j];
    }
    hipLaunchKernelGGL(pose_eval_kernel, dim3(B), dim3(kPoseThreads), 0, (hipStream_t)stream, pred_vertices, J_regressor, m, J,
                       gt_keypoints_3d, gt_vertices, V, mpjpe, recon_err, pred_joints17);
    DANET_CHECK_LAUNCH("pose_eval_kernel");
    return DANET_OK;
}

extern "C" int danet_vertex_eval(const float* pred_vertices, const float* gt_vertices, const float* pelvis_row, int B, int V,
                                 float* pve, float* pa_pve, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < (1 << 24) && V > 0 && V < (1 << 24), "vertex_eval: bad sizes B=%d V=%d", B, V);
    DANET_CHECK_ARG(pred_vertices && gt_vertices && pelvis_row && pve && pa_pve, "vertex_eval: null pointer");
    hipLaunchKernelGGL(vertex_eval_kernel, dim3(B), dim3(kPoseThreads), 0, (hipStream_t)stream, pred_vertices, gt_vertices, pelvis_row, V,
                       pve, pa_pve);
    DANET_CHECK_LAUNCH("vertex_eval_kernel");
    return DANET_OK;
}

extern "C" int danet_seg_confusion(const float* mask, const int64_t* parts, const uint8_t* gt_mask, const uint8_t* gt_parts,
                                   int64_t label_bytes, const int64_t* offsets, const int32_t* shapes, const int32_t* rects,
                                   const int32_t* tables, int table_len, int B, int res, int max_pixels, int64_t* counters, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < 65536 && res > 0 && res <= 4096 && max_pixels > 0 && label_bytes > 0 && table_len > 0,
                    "seg_confusion: bad sizes B=%d res=%d max_pixels=%d label_bytes=%lld table_len=%d", B, res, max_pixels, (long long)label_bytes, table_len);
    DANET_CHECK_ARG(mask && parts && offsets && shapes && rects && tables && counters, "seg_confusion: null pointer");
    DANET_CHECK_ARG(gt_mask || gt_parts, "seg_confusion: no label images");
    hipLaunchKernelGGL(seg_confusion_kernel, dim3(danet::cdiv(max_pixels, kSegChunk), B), dim3(kSegThreads), 0, (hipStream_t)stream,
                       mask, (const long long*)parts, gt_mask, gt_parts, (long long)label_bytes, (const long long*)offsets, shapes, rects,
                       tables, table_len, res, (unsigned long long*)counters);
    DANET_CHECK_LAUNCH("seg_confusion_kernel");
    return DANET_OK;
}

extern "C" int danet_rotmat_to_angle_axis(const float* R, int N, float* angle_axis, void* stream) {
    DANET_ENTER();
    DANET_CHECK_ARG(R && angle_axis && N > 0, "rotmat_to_angle_axis: bad arguments");
    hipLaunchKernelGGL(rotmat_to_angle_axis_kernel, dim3(danet::cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, R, N, angle_axis);
    DANET_CHECK_LAUNCH("rotmat_to_angle_axis_kernel");
    return DANET_OK;
}
