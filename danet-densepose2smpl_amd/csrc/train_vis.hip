// Sheet kernels of the training visualisation for gfx950 (train_vis.py is the caller).  Forward only.
//
//   vis_grid     the sheet rule: torchvision's make_grid(tensor [B,C,H,W], nrow, padding, pad_value) as ONE launch, one lane per
//                sheet pixel (consecutive lanes on consecutive columns: every plane store is a coalesced row), three planes per lane.
//                Optional, in this order: de-normalise with the ImageNet constants (/root/reference/train/trainer.py:251-253),
//                overlay a nearest-upsampled low-resolution image per ELEMENT (`img[iuv > 0] = iuv[iuv > 0]`, trainer.py:271-273),
//                normalise with the batch's min / max (make_grid(normalize=True) as utils/vis.py:367 calls it); two sources may be
//                interleaved a0, b0, a1, b1, ... (utils/renderer.py:39-50).
//   vis_joints   the marker rule: the 5-pixel plus of every visible joint, in place on the fp32 sheet.  One lane per sheet pixel;
//                the sheet positions of all joints pass through LDS 256 at a time and every lane keeps the LAST joint (tile order,
//                then joint order: the reference's draw order) whose plus covers its pixel -- no lane stores outside its own
//                pixel, so overlaps are deterministic and nothing can be written outside the sheet.
//
// Both are HBM- and launch-bound (a 32 x 3 x 256 x 256 batch is 25 MB read, 25 MB written); the scan of vis_joints is B * J
// broadcast LDS reads per lane.  Compiled with -ffp-contract=off: x * std + mean and (x - lo) / (hi - lo + 1e-5) are the written
// IEEE-754 binary32 operations, which is what the tests' oracle restates.  No atomics, no workspace, no inline assembly.
#include "common.h"

namespace {

struct View4 { long long sb, sc, sh, sw; };      // element strides of a [B, C, H, W] view

template <typename T> __device__ __forceinline__ float ld(const T* p, long long i);
template <> __device__ __forceinline__ float ld<float>(const float* p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float ld<unsigned short>(const unsigned short* p, long long i) {     // bf16 bits
    return __uint_as_float((unsigned int)p[i] << 16);
}

struct GridGeom {
    int N, C, H, W;              // tiles on the sheet (B, or 2 B when interleaved), channels and size of a tile
    int xmaps, pad, Hs, Ws;
    int oh, ow, f;               // overlay size and its integer upsampling factor
    int flags;
    float pad_value;
};

template <typename T>
__global__ __launch_bounds__(256) void vis_grid_kernel(
    const T* __restrict__ a, const T* __restrict__ b, View4 sa, View4 sb, GridGeom g,
    const float* __restrict__ over, const float* __restrict__ lohi, float* __restrict__ out)
{
    const int npix = g.Hs * g.Ws;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const int y = pix / g.Ws, x = pix - y * g.Ws;
    float v[3] = {g.pad_value, g.pad_value, g.pad_value};
    const int cy = y - g.pad, cx = x - g.pad;
    if (cy >= 0 && cx >= 0) {
        const int ch = g.H + g.pad, cw = g.W + g.pad;
        const int ty = cy / ch, iy = cy - ty * ch;
        const int tx = cx / cw, ix = cx - tx * cw;
        const int k = ty * g.xmaps + tx;
        if (iy < g.H && ix < g.W && tx < g.xmaps && k < g.N) {
            const bool second = b != nullptr && (k & 1);
            const int n = b != nullptr ? (k >> 1) : k;
            const T* src = second ? b : a;
            const View4 s = second ? sb : sa;
            const long long base = n * s.sb + iy * s.sh + ix * s.sw;
            const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
            float lo = 0.0f, den = 1.0f;
            if (g.flags & DANET_VIS_NORMALIZE) { lo = lohi[0]; den = (lohi[1] - lo) + 1e-5f; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = ld<T>(src, base + (g.C == 1 ? 0 : c) * s.sc);
                if (g.flags & DANET_VIS_DENORM) t = t * stdv[c] + mean[c];
                if (over) {
                    const float o = over[(((size_t)n * 3 + c) * g.oh + iy / g.f) * g.ow + ix / g.f];
                    if (o > 0.0f) t = o;
                }
                if (g.flags & DANET_VIS_NORMALIZE) {
                    t = (t - lo) / den;
                    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                }
                v[c] = t;
            }
        }
    }
    out[pix] = v[0];
    out[(size_t)npix + pix] = v[1];
    out[2 * (size_t)npix + pix] = v[2];
}

constexpr int kFar = -(1 << 30);      // a position no sheet pixel is near (sheets are at most 32768 pixels a side)

__global__ __launch_bounds__(256) void vis_joints_kernel(
    float* __restrict__ sheet, int Hs, int Ws, const float* __restrict__ joints, long long jb, long long jj, long long jc,
    const float* __restrict__ vis, long long vb, long long vj, int B, int J, int xmaps, int cellh, int cellw, int pad)
{
    __shared__ int px[256], py[256];
    const int npix = Hs * Ws;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < npix;
    const int y = pix / Ws, x = pix - y * Ws;
    const int total = B * J;
    int win = -1;
    for (int base = 0; base < total; base += 256) {
        const int i = base + (int)threadIdx.x;
        int qx = kFar, qy = kFar;
        if (i < total) {
            const int k = i / J, j = i - k * J;
            const float fx = (float)((k % xmaps) * cellw + pad) + joints[k * jb + j * jj];
            const float fy = (float)((k / xmaps) * cellh + pad) + joints[k * jb + j * jj + jc];
            const bool seen = vis == nullptr || vis[k * vb + j * vj] != 0.0f;
            // (false for NaN and inf; a finite position this far out touches no sheet pixel either)
            if (seen && fabsf(fx) < 1e9f && fabsf(fy) < 1e9f) { qx = (int)fx; qy = (int)fy; }      // truncation toward zero
        }
        px[threadIdx.x] = qx;
        py[threadIdx.x] = qy;
        __syncthreads();
        const int n = total - base < 256 ? total - base : 256;
        if (live)
            for (int t = 0; t < n; ++t)
                if (abs(x - px[t]) + abs(y - py[t]) <= 1) win = base + t;
        __syncthreads();
    }
    if (live && win >= 0) {
        const bool odd = (win % J) & 1;
        sheet[pix] = odd ? 1.0f : 0.0f;
        sheet[(size_t)npix + pix] = odd ? 0.0f : 1.0f;
        sheet[2 * (size_t)npix + pix] = 0.0f;
    }
}

// the sheet rule's size; false when a sheet side passes 32768 pixels
bool sheet_size(int N, int H, int W, int nrow, int pad, int& xmaps, int& Hs, int& Ws) {
    xmaps = nrow < N ? nrow : N;
    const long ymaps = (N + xmaps - 1) / xmaps;
    const long hs = ymaps * ((long)H + pad) + pad, ws = (long)xmaps * ((long)W + pad) + pad;
    Hs = (int)hs;
    Ws = (int)ws;
    return hs <= 32768 && ws <= 32768;
}

}  // namespace

extern "C" int danet_vis_grid(const void* a, const void* b, const int64_t* strides, int dtype, int B, int C, int H, int W,
                              int nrow, int padding, float pad_value, int flags, const float* overlay, int oh, int ow,
                              const float* lohi, float* out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B <= 16384 && (C == 1 || C == 3) && H > 0 && W > 0 && H <= 32768 && W <= 32768 && nrow > 0 &&
                    padding >= 0 && padding <= 1024, "vis_grid: bad sizes B=%d C=%d H=%d W=%d nrow=%d padding=%d", B, C, H, W, nrow, padding);
    DANET_CHECK_ARG(a && strides && out, "vis_grid: null pointer");
    DANET_CHECK_ARG(dtype == 0 || dtype == 1, "vis_grid: dtype %d (0 = fp32, 1 = bf16)", dtype);
    DANET_CHECK_ARG((flags & ~(DANET_VIS_DENORM | DANET_VIS_NORMALIZE)) == 0, "vis_grid: unknown flags %d", flags);
    DANET_CHECK_ARG(!(flags & DANET_VIS_DENORM) || C == 3, "vis_grid: de-normalising needs 3 channels, got %d", C);
    DANET_CHECK_ARG(!(flags & DANET_VIS_NORMALIZE) || lohi, "vis_grid: normalising needs the (min, max) buffer");
    for (int i = 0; i < (b ? 8 : 4); ++i) DANET_CHECK_ARG(strides[i] >= 0, "vis_grid: negative stride");
    GridGeom g;
    g.N = b ? 2 * B : B; g.C = C; g.H = H; g.W = W; g.pad = padding; g.flags = flags; g.pad_value = pad_value;
    g.oh = g.ow = 0; g.f = 1;
    if (overlay) {
        DANET_CHECK_ARG(!b, "vis_grid: an overlay and a second source exclude each other");
        DANET_CHECK_ARG(oh > 0 && ow > 0 && H % oh == 0 && W % ow == 0 && H / oh == W / ow,
                        "vis_grid: the overlay (%d x %d) must divide the tile (%d x %d) by one integer factor", oh, ow, H, W);
        g.oh = oh; g.ow = ow; g.f = H / oh;
    }
    DANET_CHECK_ARG(sheet_size(g.N, H, W, nrow, padding, g.xmaps, g.Hs, g.Ws), "vis_grid: the sheet passes 32768 pixels a side");
    const View4 sa{strides[0], strides[1], strides[2], strides[3]};
    const View4 sb = b ? View4{strides[4], strides[5], strides[6], strides[7]} : sa;
    const dim3 grid(danet::cdiv((long)g.Hs * g.Ws, 256));
    if (dtype == 0)
        hipLaunchKernelGGL(vis_grid_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)a, (const float*)b, sa, sb, g,
                           overlay, lohi, out);
    else
        hipLaunchKernelGGL(vis_grid_kernel<unsigned short>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)a,
                           (const unsigned short*)b, sa, sb, g, overlay, lohi, out);
    DANET_CHECK_LAUNCH("vis_grid_kernel");
    return DANET_OK;
}

extern "C" int danet_vis_joints(float* sheet, int Hs, int Ws, const float* joints, const int64_t* joint_strides, const float* vis,
                                const int64_t* vis_strides, int B, int J, int H, int W, int nrow, int padding, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B <= 16384 && J > 0 && J <= 4096 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && nrow > 0 && padding >= 0 &&
                    padding <= 1024, "vis_joints: bad sizes B=%d J=%d H=%d W=%d nrow=%d padding=%d", B, J, H, W, nrow, padding);
    DANET_CHECK_ARG(sheet && joints && joint_strides && (!vis || vis_strides), "vis_joints: null pointer");
    for (int i = 0; i < 3; ++i) DANET_CHECK_ARG(joint_strides[i] >= 0, "vis_joints: negative stride");
    for (int i = 0; vis && i < 2; ++i) DANET_CHECK_ARG(vis_strides[i] >= 0, "vis_joints: negative stride");
    int xmaps, hs, ws;
    DANET_CHECK_ARG(sheet_size(B, H, W, nrow, padding, xmaps, hs, ws), "vis_joints: the sheet passes 32768 pixels a side");
    DANET_CHECK_ARG(hs == Hs && ws == Ws, "vis_joints: a %d x %d sheet, the sheet rule gives %d x %d", Hs, Ws, hs, ws);
    hipLaunchKernelGGL(vis_joints_kernel, dim3(danet::cdiv((long)Hs * Ws, 256)), dim3(256), 0, (hipStream_t)stream, sheet, Hs, Ws, joints,
                       (long long)joint_strides[0], (long long)joint_strides[1], (long long)joint_strides[2], vis,
                       vis ? (long long)vis_strides[0] : 0LL, vis ? (long long)vis_strides[1] : 0LL, B, J, xmaps, H + padding, W + padding, padding);
    DANET_CHECK_LAUNCH("vis_joints_kernel");
    return DANET_OK;
}
