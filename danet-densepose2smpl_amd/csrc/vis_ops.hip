// Visualisation ops of the demo pipeline for gfx950: IUV decode, shaded mesh view, result-panel composition.
//
//   iuv_map2img   /root/reference/utils/iuvmap.py:41-100 (uv_rois=None): arg-max over the K index channels, optional Ann gate,
//                 plane 0 = index / (K - 1) or a table entry, planes 1 / 2 = U / V of the winning channel.  One lane per
//                 (map, pixel); consecutive lanes on consecutive pixels, so every channel-plane read is a coalesced row.
//   mesh shading  the rule of DESIGN.md ("shading rule"; opendr is absent and unpinned): a per-vertex kernel (rotation about y,
//                 area-weighted normals through a vertex -> face table walked in table order, three Lambertian point lights)
//                 and a per-pixel kernel (perspective-correct barycentric mix of the winning face's vertex colours; the winning
//                 face comes from the rasteriser's face-index plane, there is no second z-buffer here).  No atomics.
//   compose       /root/reference/demo.py:115-177: bilinear x4 resize of the two IUV images, overlay, 4 x 6 part grid, clip,
//                 RGBA interleave -- one lane per panel pixel, one 16-byte store each.
//
// Compiled with -ffp-contract=off: every float operation is one IEEE-754 binary32 operation in the written order (the rotation
// and the bilinear weights are restated operation by operation in the tests).  No LDS, no inline assembly.
#include "common.h"

namespace {

struct View5 { long long sb, sj, sk, sh, sw; };      // element strides of a [NB, J, K, H, W] view

template <typename T> __device__ __forceinline__ float ld(const T* p, long long i);
template <> __device__ __forceinline__ float ld<float>(const float* p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float ld<unsigned short>(const unsigned short* p, long long i) {     // bf16 bits
    return __uint_as_float((unsigned int)p[i] << 16);
}

// first maximum in channel order; a NaN counts as the maximum (torch.argmax)
template <typename T>
__device__ __forceinline__ int argmax_k(const T* p, long long base, long long sk, int K) {
    float best = ld<T>(p, base);
    int bi = 0;
    for (int k = 1; k < K; ++k) {
        const float v = ld<T>(p, base + k * sk);
        if (v > best || (v != v && best == best)) { best = v; bi = k; }
    }
    return bi;
}

template <typename T>
__global__ __launch_bounds__(256) void iuv_map2img_kernel(
    const T* __restrict__ U, const T* __restrict__ V, const T* __restrict__ I, const T* __restrict__ A,
    View5 su, View5 sv, View5 si, View5 sa, int J, int K, int KA, int H, int W,
    const float* __restrict__ table, float* __restrict__ out)
{
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int npix = H * W;
    if (pix >= npix) return;
    const int b = n / J, j = n - b * J;
    const int y = pix / W, x = pix - y * W;
    int idx = argmax_k<T>(I, b * si.sb + j * si.sj + y * si.sh + x * si.sw, si.sk, K);
    if (A) {
        const int a = argmax_k<T>(A, b * sa.sb + j * sa.sj + y * sa.sh + x * sa.sw, sa.sk, KA);
        if (a == 0) idx = 0;
    }
    float u = 0.0f, v = 0.0f;
    if (idx >= 1) {
        u = ld<T>(U, b * su.sb + j * su.sj + idx * su.sk + y * su.sh + x * su.sw);
        v = ld<T>(V, b * sv.sb + j * sv.sj + idx * sv.sk + y * sv.sh + x * sv.sw);
    }
    const float p0 = table ? table[j * K + idx] : (float)idx / (float)(K - 1);
    float* o = out + (size_t)n * 3 * npix + pix;
    o[0] = p0;
    o[npix] = u;
    o[2 * (size_t)npix] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct Lights { float pos[3][3]; float col[3][3]; };

__device__ __forceinline__ void rot_y(const float* __restrict__ p, float c, float s, float& x, float& y, float& z) {
    // row vector times rotateY(angle) (/root/reference/utils/renderer.py:97-104)
    const float px = p[0], py = p[1], pz = p[2];
    x = px * c - pz * s;
    y = py;
    z = px * s + pz * c;
}

__global__ __launch_bounds__(256) void mesh_shade_vertex_kernel(
    const float* __restrict__ verts, int NV, const int* __restrict__ faces, const int* __restrict__ csr_off,
    const int* __restrict__ csr_face, Lights L, float c, float s, float albedo,
    float* __restrict__ rverts, float* __restrict__ vcol)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NV) return;
    const float* vb = verts + (size_t)b * NV * 3;
    float x, y, z;
    rot_y(vb + i * 3, c, s, x, y, z);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    const int e0 = csr_off[i], e1 = csr_off[i + 1];
    for (int e = e0; e < e1; ++e) {
        const int f = csr_face[e];
        float ax, ay, az, bx, by, bz, cx, cy, cz;
        rot_y(vb + faces[f * 3 + 0] * 3, c, s, ax, ay, az);
        rot_y(vb + faces[f * 3 + 1] * 3, c, s, bx, by, bz);
        rot_y(vb + faces[f * 3 + 2] * 3, c, s, cx, cy, cz);
        const float ux = bx - ax, uy = by - ay, uz = bz - az;
        const float wx = cx - ax, wy = cy - ay, wz = cz - az;
        nx += uy * wz - uz * wy;
        ny += uz * wx - ux * wz;
        nz += ux * wy - uy * wx;
    }
    const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
    if (nl > 0.0f) { nx /= nl; ny /= nl; nz /= nl; } else { nx = ny = nz = 0.0f; }
    float r = 0.0f, g = 0.0f, bl = 0.0f;
    for (int l = 0; l < 3; ++l) {
        float dx = L.pos[l][0] - x, dy = L.pos[l][1] - y, dz = L.pos[l][2] - z;
        const float dl = sqrtf(dx * dx + dy * dy + dz * dz);
        float d = 0.0f;
        if (dl > 0.0f) d = nx * (dx / dl) + ny * (dy / dl) + nz * (dz / dl);
        d = d > 0.0f ? d : 0.0f;
        r += albedo * L.col[l][0] * d;
        g += albedo * L.col[l][1] * d;
        bl += albedo * L.col[l][2] * d;
    }
    float* ro = rverts + ((size_t)b * NV + i) * 3;
    ro[0] = x; ro[1] = y; ro[2] = z;
    float* co = vcol + ((size_t)b * NV + i) * 3;
    co[0] = r; co[1] = g; co[2] = bl;
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__global__ __launch_bounds__(256) void mesh_shade_pixel_kernel(
    const float* __restrict__ rverts, const float* __restrict__ vcol, const float* __restrict__ cam, int NV,
    const int* __restrict__ faces2, int F2, const int* __restrict__ fidx, const float* __restrict__ images,
    float focal, float orig, int S, float* __restrict__ rgb, float* __restrict__ alpha)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int npix = S * S;
    if (pix >= npix) return;
    const size_t o = (size_t)b * 3 * npix + pix;
    const int f = fidx[(size_t)b * npix + pix];
    if (f < 0 || f >= F2) {
        rgb[o] = images ? images[o] : 0.0f;
        rgb[o + npix] = images ? images[o + npix] : 0.0f;
        rgb[o + 2 * (size_t)npix] = images ? images[o + 2 * (size_t)npix] : 0.0f;
        alpha[(size_t)b * npix + pix] = 0.0f;
        return;
    }
    const int r = pix / S, cc = pix - r * S;
    const float Sf = (float)S;
    // the rasteriser's camera (iuv_raster.hip): pixel centre (xp, yp) in NDC, carried back to the normalised image plane
    // x / z, where barycentrics are the same (the map between the two is affine) and the edge functions lose less
    float fx = focal, cx = orig / 2.0f;
    if (orig != 224.0f) { const float sc = orig / 224.0f; fx = fx * sc; cx = cx * sc; }
    const float half = orig / 2.0f;
    const float xp = (2.0f * (float)cc + 1.0f - Sf) / Sf, yp = (Sf - 1.0f - 2.0f * (float)r) / Sf;
    const float X = (xp * half + half - cx) / fx;
    const float Y = (orig - half - cx - yp * half) / fx;
    const float sc0 = cam[b * 3 + 0], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    const float tz = (2.0f * focal) / (orig * sc0 + 1e-9f);
    const int i0 = faces2[f * 3 + 0], i1 = faces2[f * 3 + 1], i2 = faces2[f * 3 + 2];
    const float* vb = rverts + (size_t)b * NV * 3;
    const float z0 = vb[i0 * 3 + 2] + tz, z1 = vb[i1 * 3 + 2] + tz, z2 = vb[i2 * 3 + 2] + tz;
    // vertex positions relative to the pixel centre
    const float x0 = (vb[i0 * 3 + 0] + tx) / (z0 + 1e-9f) - X, y0 = (vb[i0 * 3 + 1] + ty) / (z0 + 1e-9f) - Y;
    const float x1 = (vb[i1 * 3 + 0] + tx) / (z1 + 1e-9f) - X, y1 = (vb[i1 * 3 + 1] + ty) / (z1 + 1e-9f) - Y;
    const float x2 = (vb[i2 * 3 + 0] + tx) / (z2 + 1e-9f) - X, y2 = (vb[i2 * 3 + 1] + ty) / (z2 + 1e-9f) - Y;
    float w0 = x1 * y2 - y1 * x2, w1 = x2 * y0 - y2 * x0, w2 = x0 * y1 - y0 * x1;
    const float area = w0 + w1 + w2;
    w0 = clamp01(w0 / area); w1 = clamp01(w1 / area); w2 = clamp01(w2 / area);
    float ws = w0 + w1 + w2;
    if (!(ws > 0.0f)) { w0 = w1 = w2 = 1.0f; ws = 3.0f; }      // (degenerate projection: the plain mean)
    w0 /= ws; w1 /= ws; w2 /= ws;
    const float p0 = w0 / z0, p1 = w1 / z1, p2 = w2 / z2;
    const float ps = p0 + p1 + p2;
    const float* cb = vcol + (size_t)b * NV * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const float v = (p0 * cb[i0 * 3 + ch] + p1 * cb[i1 * 3 + ch] + p2 * cb[i2 * 3 + ch]) / ps;
        rgb[o + ch * (size_t)npix] = clamp01(v);
    }
    alpha[(size_t)b * npix + pix] = 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// bilinear, half-pixel centres, edge clamp, scale S / hm (F.interpolate(mode='bilinear', align_corners=False))
__device__ __forceinline__ void lin_tap(int d, float scale, int n, int& i0, int& i1, float& l0, float& l1) {
    float src = ((float)d + 0.5f) * scale - 0.5f;
    if (src < 0.0f) src = 0.0f;
    i0 = (int)src;
    if (i0 > n - 1) i0 = n - 1;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

__device__ __forceinline__ float bilin(const float* __restrict__ p, int hm, int i0, int i1, int j0, int j1,
                                       float h0, float h1, float w0, float w1) {
    return h0 * (w0 * p[i0 * hm + j0] + w1 * p[i0 * hm + j1]) + h1 * (w0 * p[i1 * hm + j0] + w1 * p[i1 * hm + j1]);
}

__global__ __launch_bounds__(256) void demo_compose_kernel(
    const float* __restrict__ images, const float* __restrict__ glob, const float* __restrict__ part,
    const float* __restrict__ riuv, const float* __restrict__ mesh, const float* __restrict__ side,
    const float* __restrict__ side_alpha, int S, int hm, int Wt, float4* __restrict__ out)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * Wt) return;
    const int y = i / Wt, xt = i - y * Wt;
    const size_t sp = (size_t)S * S, hp = (size_t)hm * hm;
    const int wpart = 6 * hm;
    float c[3], a = 1.0f;
    if (xt < S) {
        for (int ch = 0; ch < 3; ++ch) c[ch] = images[((size_t)b * 3 + ch) * sp + (size_t)y * S + xt];
    } else if (xt < 2 * S || (xt >= 2 * S + wpart && xt < 3 * S + wpart)) {
        const bool over = xt >= 2 * S;
        const int x = over ? xt - 2 * S - wpart : xt - S;
        const float scale = (float)hm / (float)S;
        int i0, i1, j0, j1;
        float h0, h1, w0, w1;
        lin_tap(y, scale, hm, i0, i1, h0, h1);
        lin_tap(x, scale, hm, j0, j1, w0, w1);
        const float* src = (over ? riuv : glob) + (size_t)b * 3 * hp;
        for (int ch = 0; ch < 3; ++ch) {
            const float v = bilin(src + ch * hp, hm, i0, i1, j0, j1, h0, h1, w0, w1);
            c[ch] = (over && !(v > 0.0f)) ? images[((size_t)b * 3 + ch) * sp + (size_t)y * S + x] : v;
        }
    } else if (xt < 2 * S + wpart) {
        const int x = xt - 2 * S;
        const int j = (y / hm) * 6 + x / hm;
        const size_t q = (size_t)(y % hm) * hm + x % hm;
        for (int ch = 0; ch < 3; ++ch) c[ch] = part[(((size_t)b * 24 + j) * 3 + ch) * hp + q];
    } else if (xt < 4 * S + wpart) {
        const int x = xt - 3 * S - wpart;
        for (int ch = 0; ch < 3; ++ch) c[ch] = mesh[((size_t)b * 3 + ch) * sp + (size_t)y * S + x];
    } else {
        const int x = xt - 4 * S - wpart;
        for (int ch = 0; ch < 3; ++ch) c[ch] = side[((size_t)b * 3 + ch) * sp + (size_t)y * S + x];
        a = side_alpha[(size_t)b * sp + (size_t)y * S + x];
    }
    out[(size_t)b * S * Wt + i] = float4{clamp01(c[0]), clamp01(c[1]), clamp01(c[2]), clamp01(a)};
}

View5 view5(const int64_t* s) { return View5{s[0], s[1], s[2], s[3], s[4]}; }

}  // namespace

extern "C" int danet_iuv_map2img_forward(const void* U, const void* V, const void* I, const void* A, const int64_t* strides,
                                         int NB, int J, int K, int KA, int H, int W, int dtype, const float* table,
                                         float* out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(NB > 0 && J > 0 && (long)NB * J < 65536 && K >= 2 && K <= 256 && H > 0 && W > 0 && (long)H * W < (1L << 30),
                    "iuv_map2img_forward: bad sizes NB=%d J=%d K=%d H=%d W=%d", NB, J, K, H, W);
    DANET_CHECK_ARG(U && V && I && strides && out, "iuv_map2img_forward: null pointer");
    DANET_CHECK_ARG(!A || (KA >= 1 && KA <= 256), "iuv_map2img_forward: bad Ann channel count %d", KA);
    DANET_CHECK_ARG(dtype == 0 || dtype == 1, "iuv_map2img_forward: dtype %d (0 = fp32, 1 = bf16)", dtype);
    for (int i = 0; i < 20; ++i) DANET_CHECK_ARG(strides[i] >= 0, "iuv_map2img_forward: negative stride");
    const dim3 grid(danet::cdiv((long)H * W, 256), NB * J);
    hipStream_t st = (hipStream_t)stream;
    const View5 su = view5(strides), sv = view5(strides + 5), si = view5(strides + 10), sa = view5(strides + 15);
    if (dtype == 0)
        hipLaunchKernelGGL(iuv_map2img_kernel<float>, grid, dim3(256), 0, st, (const float*)U, (const float*)V, (const float*)I,
                           (const float*)A, su, sv, si, sa, J, K, KA, H, W, table, out);
    else
        hipLaunchKernelGGL(iuv_map2img_kernel<unsigned short>, grid, dim3(256), 0, st, (const unsigned short*)U,
                           (const unsigned short*)V, (const unsigned short*)I, (const unsigned short*)A, su, sv, si, sa, J, K, KA,
                           H, W, table, out);
    DANET_CHECK_LAUNCH("iuv_map2img_kernel");
    return DANET_OK;
}

// workspace: the rotated vertices [B,V,3] f32 followed by the vertex colours [B,V,3] f32
extern "C" size_t danet_mesh_shade_ws_bytes(int B, int V) { return (size_t)2 * B * V * 3 * sizeof(float); }

extern "C" int danet_mesh_shade_vertices(const float* verts, int B, int V, const int32_t* faces, int F, const int32_t* csr_off,
                                         const int32_t* csr_face, const float* lights, float cos_y, float sin_y, float albedo,
                                         void* ws, size_t ws_bytes, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < 65536 && V > 0 && F > 0, "mesh_shade_vertices: bad sizes B=%d V=%d F=%d", B, V, F);
    DANET_CHECK_ARG(verts && faces && csr_off && csr_face && lights && ws, "mesh_shade_vertices: null pointer");
    if (ws_bytes < danet_mesh_shade_ws_bytes(B, V))
        return danet::fail(DANET_ERR_WORKSPACE, "mesh_shade_vertices: workspace %zu < %zu bytes", ws_bytes, danet_mesh_shade_ws_bytes(B, V));
    Lights L;
    for (int l = 0; l < 3; ++l)
        for (int k = 0; k < 3; ++k) { L.pos[l][k] = lights[l * 3 + k]; L.col[l][k] = lights[9 + l * 3 + k]; }
    float* rverts = (float*)ws;
    float* vcol = rverts + (size_t)B * V * 3;
    hipLaunchKernelGGL(mesh_shade_vertex_kernel, dim3(danet::cdiv(V, 256), B), dim3(256), 0, (hipStream_t)stream, verts, V, faces,
                       csr_off, csr_face, L, cos_y, sin_y, albedo, rverts, vcol);
    DANET_CHECK_LAUNCH("mesh_shade_vertex_kernel");
    return DANET_OK;
}

extern "C" int danet_mesh_shade_pixels(const void* ws, const float* cam, int B, int V, const int32_t* faces2, int F2,
                                       const int32_t* face_idx, const float* images, float focal, float orig, int S,
                                       float* rgb, float* alpha, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < 65536 && V > 0 && F2 > 0 && S > 0 && S <= 4096, "mesh_shade_pixels: bad sizes B=%d V=%d F2=%d S=%d", B, V, F2, S);
    DANET_CHECK_ARG(ws && cam && faces2 && face_idx && rgb && alpha, "mesh_shade_pixels: null pointer");
    const float* rverts = (const float*)ws;
    const float* vcol = rverts + (size_t)B * V * 3;
    hipLaunchKernelGGL(mesh_shade_pixel_kernel, dim3(danet::cdiv((long)S * S, 256), B), dim3(256), 0, (hipStream_t)stream, rverts, vcol,
                       cam, V, faces2, F2, face_idx, images, focal, orig, S, rgb, alpha);
    DANET_CHECK_LAUNCH("mesh_shade_pixel_kernel");
    return DANET_OK;
}

extern "C" int danet_demo_compose(const float* images, const float* glob, const float* part, const float* riuv, const float* mesh,
                                  const float* side, const float* side_alpha, int B, int S, int hm, float* out, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(B > 0 && B < 65536 && S > 0 && S <= 4096 && hm > 0 && 4 * hm == S, "demo_compose: bad sizes B=%d S=%d hm=%d (4 hm = S)", B, S, hm);
    DANET_CHECK_ARG(images && glob && part && riuv && out, "demo_compose: null pointer");
    DANET_CHECK_ARG((mesh != nullptr) == (side != nullptr) && (mesh != nullptr) == (side_alpha != nullptr),
                    "demo_compose: the two mesh panels come together");
    DANET_CHECK_ARG(((uintptr_t)out & 15) == 0, "demo_compose: out must be 16-byte aligned");
    const int Wt = (mesh ? 4 : 2) * S + 6 * hm + S;
    hipLaunchKernelGGL(demo_compose_kernel, dim3(danet::cdiv((long)S * Wt, 256), B), dim3(256), 0, (hipStream_t)stream, images, glob, part,
                       riuv, mesh, side, side_alpha, S, hm, Wt, (float4*)out);
    DANET_CHECK_LAUNCH("demo_compose_kernel");
    return DANET_OK;
}
