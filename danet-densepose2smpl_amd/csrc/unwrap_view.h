// One view of the texture rule (DESIGN.md "texture rule"): the rasteriser's camera, what one photograph adds to the running sums of a
// texel, and the finished texel, ONE set of device functions for every caller: texture_ops.hip (unwrap loops add_view over a person's
// views; the draw takes the camera) and track_reid.hip (the online descriptor adds one view per step and reads the same texel).  The
// callers compile with -ffp-contract=off: every operation below is one IEEE-754 operation in the written order (the tests restate
// them), so the two units give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace danet {

// the rasteriser's intrinsics (iuv_raster.hip raster_project_kernel): for orig != 224 the principal point is scaled too
struct Camera { float fx, cx, tz; };

__device__ __forceinline__ Camera camera(float focal, float orig, float s) {
    Camera k;
    k.fx = focal; k.cx = orig / 2.0f;
    if (orig != 224.0f) { const float sc = orig / 224.0f; k.fx = k.fx * sc; k.cx = k.cx * sc; }
    k.tz = (2.0f * focal) / (orig * s + 1e-9f);
    return k;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the frames a texel is unwrapped from: [N,3,H,H] photographs, [N,NV,3] meshes, [N,3] cameras, [N,H,H] rasteriser depth planes
struct ViewInputs {
    const float *images, *verts, *cam, *depth;
    int NV, H;
    float focal, depth_tol, min_cos;
};

// View n of the surface point with barycentrics (w0, w1, w2) on the mesh vertices (i0, i1, i2), all three inside [0, NV): the point
// is projected with the rasteriser's camera (raster_project_kernel, operation by operation), tested against the rasteriser's depth
// plane and the facing cosine cs, and the photograph is sampled bilinearly; (sr, sg, sb, sw) += cs (r, g, b, 1).  A view that does
// not see the point adds nothing.
__device__ __forceinline__ void add_view(const ViewInputs& a, int n, int i0, int i1, int i2, float w0, float w1, float w2, float& sr,
                                         float& sg, float& sb, float& sw)
{
    const int H = a.H;
    const float orig = (float)H;
    const size_t npix = (size_t)H * H;
    const float* vb = a.verts + (size_t)n * a.NV * 3;
    const float tx = a.cam[n * 3 + 1], ty = a.cam[n * 3 + 2];
    const Camera k = camera(a.focal, orig, a.cam[n * 3 + 0]);
    const float ax = vb[i0 * 3 + 0], ay = vb[i0 * 3 + 1], az = vb[i0 * 3 + 2];
    const float bx = vb[i1 * 3 + 0], by = vb[i1 * 3 + 1], bz = vb[i1 * 3 + 2];
    const float cx = vb[i2 * 3 + 0], cy = vb[i2 * 3 + 1], cz = vb[i2 * 3 + 2];
    // the surface point, then the rasteriser's projection of it
    const float X = w0 * ax + w1 * bx + w2 * cx, Y = w0 * ay + w1 * by + w2 * cy, Z = w0 * az + w1 * bz + w2 * cz;
    const float px = X + tx, py = Y + ty, pz = Z + k.tz;
    const float zz = pz + 1e-9f;
    const float x = px / zz, y = py / zz;
    const float c = k.fx * x + k.cx - 0.5f, r = k.fx * y + k.cx - 0.5f;
    const float rn = floorf(r + 0.5f), cn = floorf(c + 0.5f);
    if (!(rn >= 0.0f && rn < orig && cn >= 0.0f && cn < orig)) return;
    const float d = a.depth[(size_t)n * npix + (size_t)(int)rn * H + (int)cn];
    if (!(d < __builtin_inff()) || !(pz <= d + a.depth_tol)) return;
    // facing: the normal of the camera-space corners against the direction to the camera
    const float t0x = ax + tx, t0y = ay + ty, t0z = az + k.tz;
    const float ux = (bx + tx) - t0x, uy = (by + ty) - t0y, uz = (bz + k.tz) - t0z;
    const float vx = (cx + tx) - t0x, vy = (cy + ty) - t0y, vz = (cz + k.tz) - t0z;
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float nl = sqrtf(nx * nx + ny * ny + nz * nz), pl = sqrtf(px * px + py * py + pz * pz);
    if (!(nl > 0.0f && pl > 0.0f)) return;
    const float cs = (0.0f - (nx * px + ny * py + nz * pz)) / (nl * pl);
    if (!(cs > a.min_cos)) return;
    // bilinear, pixel centres at integers, edge clamp
    const float rf = floorf(r), cf = floorf(c);
    const float lr = r - rf, lc = c - cf;
    const int r0 = clampi((int)rf, H - 1), r1 = clampi((int)rf + 1, H - 1);
    const int c0 = clampi((int)cf, H - 1), c1 = clampi((int)cf + 1, H - 1);
    const float* img = a.images + (size_t)n * 3 * npix;
    float col[3];
    for (int ch = 0; ch < 3; ++ch) {
        const float* plane = img + ch * npix;
        const float top = (1.0f - lc) * plane[(size_t)r0 * H + c0] + lc * plane[(size_t)r0 * H + c1];
        const float bot = (1.0f - lc) * plane[(size_t)r1 * H + c0] + lc * plane[(size_t)r1 * H + c1];
        col[ch] = (1.0f - lr) * top + lr * bot;
    }
    sr += cs * col[0]; sg += cs * col[1]; sb += cs * col[2]; sw += cs;
}

// the texel of the sums: the weighted mean colour and the weight, or zeros where no view saw it
__device__ __forceinline__ float4 texel(float sr, float sg, float sb, float sw)
{
    return sw > 0.0f ? float4{sr / sw, sg / sw, sb / sw, sw} : float4{0.0f, 0.0f, 0.0f, 0.0f};
}

}  // namespace danet
