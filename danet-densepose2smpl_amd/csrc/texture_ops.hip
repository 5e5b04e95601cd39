// Texture atlases over the DensePose charts for gfx950 (DESIGN.md "texture rule"): a texel -> surface map, the unwrap of
// photographs into the 24 charts and the textured draw.
//
//   map      one lane per texel (part, i, j): the faces of the part are walked in ascending index (a CSR by part); the first
//            face whose UV triangle holds the texel centre wins.  Edge functions in double from the f32 UV table, so the
//            float64 restatement of the tests reproduces face and barycentrics bit for bit.  Made once per topology and T.
//   unwrap   one lane per (person, texel): loops danet::add_view (unwrap_view.h, shared with track_reid.hip) over the person's
//            views in order and stores danet::texel of the sums.  One 16-byte store.
//   render   one lane per pixel: the winning face comes from the rasteriser's face-index plane; barycentrics as
//            mesh_shade_pixel_kernel (vis_ops.hip) computes them; a valid-aware bilinear sample of the face's chart.
//
// Compiled with -ffp-contract=off: every operation below is one IEEE-754 operation in the written order (the tests restate
// them).  No LDS, no atomics, no inline assembly.
#include "common.h"
#include "unwrap_view.h"
#include "video_sizes.h"

using namespace danet;

namespace {

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

__global__ __launch_bounds__(256) void texture_unwrap_kernel(
    const ViewInputs in, const int* __restrict__ view_off, const int* __restrict__ vert_mapping, const int* __restrict__ faces, int F,
    const int* __restrict__ map_face, const float* __restrict__ map_bary, int ntex, float4* __restrict__ atlas)
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
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
        const int n1 = view_off[p + 1];
        for (int n = view_off[p]; n < n1; ++n) add_view(in, n, i0, i1, i2, w0, w1, w2, sr, sg, sb, sw);
        out = texel(sr, sg, sb, sw);
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
        const float4* chart = atlas + ((size_t)atlas_index[b] * kParts + part) * T * T;
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
    hipLaunchKernelGGL(texture_map_kernel, dim3(danet::cdiv((long)T * T, 256), kParts), dim3(256), 0, (hipStream_t)stream, uv, faces,
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
    DANET_CHECK_ARG((long)kParts * T * T < (1L << 30), "texture_unwrap: T=%d is too large", T);
    DANET_CHECK_ARG(((uintptr_t)atlas & 15) == 0, "texture_unwrap: atlas must be 16-byte aligned");
    DANET_CHECK_OFFSETS("texture_unwrap", "view_off", host_view_off, P, N);
    const int ntex = kParts * T * T;
    const ViewInputs in = {images, verts, cam, depth, NV, H, focal, depth_tol, min_cos};
    hipLaunchKernelGGL(texture_unwrap_kernel, dim3(danet::cdiv(ntex, 256), P), dim3(256), 0, (hipStream_t)stream, in, view_off,
                       vert_mapping, faces, F, map_face, map_bary, ntex, (float4*)atlas);
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
