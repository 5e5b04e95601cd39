// Texture atlases over the DensePose charts for gfx950 (DESIGN.md "texture rule"): a texel -> surface map, the unwrap of
// photographs into the 24 charts and the textured draw.
//
//   map      one lane per texel (part, i, j): the faces of the part are walked in ascending index (a CSR by part); the first
//            face whose UV triangle holds the texel centre wins.  Edge functions in double from the f32 UV table, so the
//            float64 restatement of the tests reproduces face and barycentrics bit for bit.  Made once per topology and T.
//   unwrap   one lane per (person, texel): loops over the person's views in order; per view the surface point is projected
//            with the rasteriser's camera (iuv_raster.hip raster_project_kernel, operation by operation), tested against the
//            rasteriser's depth plane and the facing cosine, and the photograph is sampled bilinearly.  One 16-byte store.
//   render   one lane per pixel: the winning face comes from the rasteriser's face-index plane; barycentrics as
//            mesh_shade_pixel_kernel (vis_ops.hip) computes them; a valid-aware bilinear sample of the face's chart.
//
// Compiled with -ffp-contract=off: every operation below is one IEEE-754 operation in the written order (the tests restate
// them).  No LDS, no atomics, no inline assembly.
#include "common.h"

namespace {

constexpr int PARTS = 24;

__global__ __launch_bounds__(256) void texture_map_kernel(
    const float* __restrict__ uv, const int* __restrict__ faces, const int* __restrict__ part_off,
    const int* __restrict__ part_faces, int T, int* __restrict__ face, float* __restrict__ bary)
{
    const int p = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T * T) return;
    const int i = t / T, j = t - i * T;
    const double u = ((double)j + 0.5) / (double)T, v = ((double)i + 0.5) / (double)T;
    int win = -1;
    double b0 = 0.0, b1 = 0.0;
    const int q1 = part_off[p + 1];
    for (int q = part_off[p]; q < q1; ++q) {
        const int f = part_faces[q];
        const int ia = faces[f * 3 + 0], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
        const double au = uv[ia * 2 + 0], av = uv[ia * 2 + 1];
        const double bu = uv[ib * 2 + 0], bv = uv[ib * 2 + 1];
        const double cu = uv[ic * 2 + 0], cv = uv[ic * 2 + 1];
        const double e0 = (bu - u) * (cv - v) - (bv - v) * (cu - u);
        const double e1 = (cu - u) * (av - v) - (cv - v) * (au - u);
        const double e2 = (au - u) * (bv - v) - (av - v) * (bu - u);
        const double area = e0 + e1 + e2;
        if (area == 0.0) continue;
        if ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0)) {
            win = f; b0 = e0 / area; b1 = e1 / area;
            break;
        }
    }
    const size_t o = (size_t)p * T * T + t;
    face[o] = win;
    bary[o * 2 + 0] = (float)b0;
    bary[o * 2 + 1] = (float)b1;
}

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

__global__ __launch_bounds__(256) void texture_unwrap_kernel(
    const float* __restrict__ images, const float* __restrict__ verts, const float* __restrict__ cam,
    const float* __restrict__ depth, int NV, int H, const int* __restrict__ view_off,
    const int* __restrict__ vert_mapping, const int* __restrict__ faces, int F, const int* __restrict__ map_face,
    const float* __restrict__ map_bary, int ntex, float focal, float depth_tol, float min_cos, float4* __restrict__ atlas)
{
    const int p = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntex) return;
    float4 out = float4{0.0f, 0.0f, 0.0f, 0.0f};
    const int f = map_face[t];
    if (f >= 0 && f < F) {
        const float w0 = map_bary[t * 2 + 0], w1 = map_bary[t * 2 + 1];
        const float w2 = 1.0f - w0 - w1;
        const int i0 = vert_mapping[faces[f * 3 + 0]], i1 = vert_mapping[faces[f * 3 + 1]], i2 = vert_mapping[faces[f * 3 + 2]];
        const float orig = (float)H;
        const size_t npix = (size_t)H * H;
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
        const int n1 = view_off[p + 1];
        for (int n = view_off[p]; n < n1; ++n) {
            const float* vb = verts + (size_t)n * NV * 3;
            const float tx = cam[n * 3 + 1], ty = cam[n * 3 + 2];
            const Camera k = camera(focal, orig, cam[n * 3 + 0]);
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
            if (!(rn >= 0.0f && rn < orig && cn >= 0.0f && cn < orig)) continue;
            const float d = depth[(size_t)n * npix + (size_t)(int)rn * H + (int)cn];
            if (!(d < __builtin_inff()) || !(pz <= d + depth_tol)) continue;
            // facing: the normal of the camera-space corners against the direction to the camera
            const float t0x = ax + tx, t0y = ay + ty, t0z = az + k.tz;
            const float ux = (bx + tx) - t0x, uy = (by + ty) - t0y, uz = (bz + k.tz) - t0z;
            const float vx = (cx + tx) - t0x, vy = (cy + ty) - t0y, vz = (cz + k.tz) - t0z;
            const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const float nl = sqrtf(nx * nx + ny * ny + nz * nz), pl = sqrtf(px * px + py * py + pz * pz);
            if (!(nl > 0.0f && pl > 0.0f)) continue;
            const float cs = (0.0f - (nx * px + ny * py + nz * pz)) / (nl * pl);
            if (!(cs > min_cos)) continue;
            // bilinear, pixel centres at integers, edge clamp
            const float rf = floorf(r), cf = floorf(c);
            const float lr = r - rf, lc = c - cf;
            const int r0 = clampi((int)rf, H - 1), r1 = clampi((int)rf + 1, H - 1);
            const int c0 = clampi((int)cf, H - 1), c1 = clampi((int)cf + 1, H - 1);
            const float* img = images + (size_t)n * 3 * npix;
            float col[3];
            for (int ch = 0; ch < 3; ++ch) {
                const float* plane = img + ch * npix;
                const float top = (1.0f - lc) * plane[(size_t)r0 * H + c0] + lc * plane[(size_t)r0 * H + c1];
                const float bot = (1.0f - lc) * plane[(size_t)r1 * H + c0] + lc * plane[(size_t)r1 * H + c1];
                col[ch] = (1.0f - lr) * top + lr * bot;
            }
            sr += cs * col[0]; sg += cs * col[1]; sb += cs * col[2]; sw += cs;
        }
        if (sw > 0.0f) out = float4{sr / sw, sg / sw, sb / sw, sw};
    }
    atlas[(size_t)p * ntex + t] = out;
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

struct Fill { float c[3]; };

__global__ __launch_bounds__(256) void texture_render_kernel(
    const float* __restrict__ rverts, const float* __restrict__ cam, int NV, const int* __restrict__ vert_mapping,
    const int* __restrict__ faces, int F, const float* __restrict__ uv, const int* __restrict__ face_part,
    const int* __restrict__ fidx, const float4* __restrict__ atlas, int T, const int* __restrict__ atlas_index,
    const float* __restrict__ images, float focal, int S, Fill fill, float* __restrict__ rgb, float* __restrict__ alpha)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int npix = S * S;
    if (pix >= npix) return;
    const size_t o = (size_t)b * 3 * npix + pix;
    const int f = fidx[(size_t)b * npix + pix];
    if (f < 0 || f >= F) {
        rgb[o] = images ? images[o] : 0.0f;
        rgb[o + npix] = images ? images[o + npix] : 0.0f;
        rgb[o + 2 * (size_t)npix] = images ? images[o + 2 * (size_t)npix] : 0.0f;
        alpha[(size_t)b * npix + pix] = 0.0f;
        return;
    }
    // barycentrics exactly as mesh_shade_pixel_kernel (vis_ops.hip): on the normalised image plane, clamped, renormalised,
    // perspective-correct through 1 / z
    const int r = pix / S, cc = pix - r * S;
    const float Sf = (float)S, orig = (float)S;
    const Camera k = camera(focal, orig, cam[b * 3 + 0]);
    const float tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    const float half = orig / 2.0f;
    const float xp = (2.0f * (float)cc + 1.0f - Sf) / Sf, yp = (Sf - 1.0f - 2.0f * (float)r) / Sf;
    const float X = (xp * half + half - k.cx) / k.fx;
    const float Y = (orig - half - k.cx - yp * half) / k.fx;
    const int d0 = faces[f * 3 + 0], d1 = faces[f * 3 + 1], d2 = faces[f * 3 + 2];
    const int i0 = vert_mapping[d0], i1 = vert_mapping[d1], i2 = vert_mapping[d2];
    const float* vb = rverts + (size_t)b * NV * 3;
    const float z0 = vb[i0 * 3 + 2] + k.tz, z1 = vb[i1 * 3 + 2] + k.tz, z2 = vb[i2 * 3 + 2] + k.tz;
    const float x0 = (vb[i0 * 3 + 0] + tx) / (z0 + 1e-9f) - X, y0 = (vb[i0 * 3 + 1] + ty) / (z0 + 1e-9f) - Y;
    const float x1 = (vb[i1 * 3 + 0] + tx) / (z1 + 1e-9f) - X, y1 = (vb[i1 * 3 + 1] + ty) / (z1 + 1e-9f) - Y;
    const float x2 = (vb[i2 * 3 + 0] + tx) / (z2 + 1e-9f) - X, y2 = (vb[i2 * 3 + 1] + ty) / (z2 + 1e-9f) - Y;
    float w0 = x1 * y2 - y1 * x2, w1 = x2 * y0 - y2 * x0, w2 = x0 * y1 - y0 * x1;
    const float area = w0 + w1 + w2;
    w0 = clamp01(w0 / area); w1 = clamp01(w1 / area); w2 = clamp01(w2 / area);
    float ws = w0 + w1 + w2;
    if (!(ws > 0.0f)) { w0 = w1 = w2 = 1.0f; ws = 3.0f; }
    w0 /= ws; w1 /= ws; w2 /= ws;
    const float p0 = w0 / z0, p1 = w1 / z1, p2 = w2 / z2;
    const float ps = p0 + p1 + p2;
    const float u = (p0 * uv[d0 * 2 + 0] + p1 * uv[d1 * 2 + 0] + p2 * uv[d2 * 2 + 0]) / ps;
    const float v = (p0 * uv[d0 * 2 + 1] + p1 * uv[d1 * 2 + 1] + p2 * uv[d2 * 2 + 1]) / ps;
    // chart coordinates; the four taps are clamped to the chart, a tap nothing was unwrapped to does not count
    const float x = u * (float)T - 0.5f, y = v * (float)T - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    const float lx = x - xf, ly = y - yf;
    float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
    if (xf == xf && yf == yf) {                     // (a NaN from a degenerate projection draws as fill)
        const float hi = (float)(T - 1);
        const int j0 = (int)fminf(fmaxf(xf, 0.0f), hi), j1 = (int)fminf(fmaxf(xf + 1.0f, 0.0f), hi);
        const int r0 = (int)fminf(fmaxf(yf, 0.0f), hi), r1 = (int)fminf(fmaxf(yf + 1.0f, 0.0f), hi);
        const int part = face_part[f];
        const float4* chart = atlas + ((size_t)atlas_index[b] * PARTS + part) * T * T;
        const int ti[4] = {r0 * T + j0, r0 * T + j1, r1 * T + j0, r1 * T + j1};
        const float tb[4] = {(1.0f - ly) * (1.0f - lx), (1.0f - ly) * lx, ly * (1.0f - lx), ly * lx};
        for (int q = 0; q < 4; ++q) {
            const float4 tex = chart[ti[q]];
            if (tex.w > 0.0f) {
                num[0] += tb[q] * tex.x; num[1] += tb[q] * tex.y; num[2] += tb[q] * tex.z;
                den += tb[q];
            }
        }
    }
    const bool seen = den > 0.0f;
    rgb[o] = seen ? num[0] / den : fill.c[0];
    rgb[o + npix] = seen ? num[1] / den : fill.c[1];
    rgb[o + 2 * (size_t)npix] = seen ? num[2] / den : fill.c[2];
    alpha[(size_t)b * npix + pix] = 1.0f;
}

}  // namespace

extern "C" int danet_texture_map(const float* uv, int NDV, const int32_t* faces, int F, const int32_t* part_off,
                                 const int32_t* part_faces, int T, int32_t* face, float* bary, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(NDV > 0 && F > 0 && T >= 2 && T <= 4096, "texture_map: bad sizes NDV=%d F=%d T=%d (T >= 2)", NDV, F, T);
    DANET_CHECK_ARG(uv && faces && part_off && part_faces && face && bary, "texture_map: null pointer");
    hipLaunchKernelGGL(texture_map_kernel, dim3(danet::cdiv((long)T * T, 256), PARTS), dim3(256), 0, (hipStream_t)stream, uv, faces,
                       part_off, part_faces, T, face, bary);
    DANET_CHECK_LAUNCH("texture_map_kernel");
    return DANET_OK;
}

extern "C" int danet_texture_unwrap(const float* images, const float* verts, const float* cam, const float* depth, int N, int NV,
                                    int H, const int32_t* view_off, const int32_t* host_view_off, int P,
                                    const int32_t* vert_mapping, int NDV, const int32_t* faces, int F, const int32_t* map_face,
                                    const float* map_bary, int T, float focal, float depth_tol, float min_cos, float* atlas,
                                    void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(N >= 0 && N < 65536 && NV > 0 && NDV > 0 && F > 0 && H > 0 && H <= 4096 && P > 0 && P < 65536 && T >= 2 && T <= 4096,
                    "texture_unwrap: bad sizes N=%d NV=%d NDV=%d F=%d H=%d P=%d T=%d", N, NV, NDV, F, H, P, T);
    DANET_CHECK_ARG(view_off && host_view_off && vert_mapping && faces && map_face && map_bary && atlas, "texture_unwrap: null pointer");
    DANET_CHECK_ARG(N == 0 || (images && verts && cam && depth), "texture_unwrap: null pointer");
    DANET_CHECK_ARG((long)PARTS * T * T < (1L << 30), "texture_unwrap: T=%d is too large", T);
    DANET_CHECK_ARG(((uintptr_t)atlas & 15) == 0, "texture_unwrap: atlas must be 16-byte aligned");
    DANET_CHECK_ARG(host_view_off[0] == 0 && host_view_off[P] == N, "texture_unwrap: view_off must run from 0 to N=%d", N);
    for (int p = 0; p < P; ++p)
        DANET_CHECK_ARG(host_view_off[p] <= host_view_off[p + 1], "texture_unwrap: view_off must be non-decreasing");
    const int ntex = PARTS * T * T;
    hipLaunchKernelGGL(texture_unwrap_kernel, dim3(danet::cdiv(ntex, 256), P), dim3(256), 0, (hipStream_t)stream, images, verts, cam,
                       depth, NV, H, view_off, vert_mapping, faces, F, map_face, map_bary, ntex, focal, depth_tol, min_cos,
                       (float4*)atlas);
    DANET_CHECK_LAUNCH("texture_unwrap_kernel");
    return DANET_OK;
}

extern "C" int danet_texture_render(const float* rverts, const float* cam, int N, int NV, const int32_t* vert_mapping, int NDV,
                                    const int32_t* faces, int F, const float* uv, const int32_t* face_part,
                                    const int32_t* face_idx, const float* atlas, int P, int T, const int32_t* atlas_index,
                                    const int32_t* host_atlas_index, const float* images, float focal, int S, const float* fill,
                                    float* rgb, float* alpha, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(N > 0 && N < 65536 && NV > 0 && NDV > 0 && F > 0 && S > 0 && S <= 4096 && P > 0 && T >= 2 && T <= 4096,
                    "texture_render: bad sizes N=%d NV=%d NDV=%d F=%d S=%d P=%d T=%d", N, NV, NDV, F, S, P, T);
    DANET_CHECK_ARG(rverts && cam && vert_mapping && faces && uv && face_part && face_idx && atlas && atlas_index && host_atlas_index &&
                    fill && rgb && alpha, "texture_render: null pointer");
    DANET_CHECK_ARG(((uintptr_t)atlas & 15) == 0, "texture_render: atlas must be 16-byte aligned");
    for (int n = 0; n < N; ++n)
        DANET_CHECK_ARG(host_atlas_index[n] >= 0 && host_atlas_index[n] < P, "texture_render: atlas_index[%d] = %d outside [0, %d)", n,
                        host_atlas_index[n], P);
    const Fill fl = Fill{{fill[0], fill[1], fill[2]}};
    hipLaunchKernelGGL(texture_render_kernel, dim3(danet::cdiv((long)S * S, 256), N), dim3(256), 0, (hipStream_t)stream, rverts, cam, NV,
                       vert_mapping, faces, F, uv, face_part, face_idx, (const float4*)atlas, T, atlas_index, images, focal, S, fl, rgb,
                       alpha);
    DANET_CHECK_LAUNCH("texture_render_kernel");
    return DANET_OK;
}
