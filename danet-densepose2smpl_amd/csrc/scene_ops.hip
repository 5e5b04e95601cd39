// Scene rasteriser for gfx950: every person's shaded mesh drawn into the uncropped photograph it was found in, one depth order
// per photograph (scene.py / tools/demo_scene.py are the callers).
//
// The rule is the one of DESIGN.md ("scene rule").  It is iuv_raster.hip's raster rule moved from one square S x S image per
// sample to frame pixels: each person carries an affine map `proj` from the normalised image plane to pixel index coordinates of
// its frame, the frames are packed uint8 HWC rectangles of different sizes (batch_crop's layout), and all people of a frame share
// that frame's 64-bit depth/id buffer, with depths made comparable between people by `dscale`.
//
// This translation unit is compiled with -ffp-contract=off: every float operation below is one IEEE-754 binary32 operation in
// the written order (tests/scene_oracle.py restates them), so the integer id plane is reproducible.
//
// Mapping (three launches, a straight chain; nothing is serial per frame or per person):
//   project  one lane per (person, vertex): translate, divide, apply `proj`, store (col, row, Z + tz) in the workspace; the same
//            launch resets the depth/id buffer of every frame pixel.
//   faces    one lane per (person, face): set-up, candidate pixel range with 0.01 pixel of slack clipped to the frame, and a 64-bit
//            atomic min of (depth bits << 32 | person * F2 + face) per covered pixel centre -- depth > 0, so the unsigned order is
//            the float order and a tie falls to the lower id.  The minimum does not depend on the order lanes arrive in.
//   resolve  one lane per frame pixel: an empty pixel copies its three source bytes; a covered one mixes the winning face's vertex
//            colours perspective-correctly (vis_ops.hip's mesh_shade_pixel_kernel, in frame pixels relative to the pixel centre)
//            and stores three bytes.  One extra row of blocks copies the bytes the buffer holds after the last frame.
#include "common.h"

namespace {

constexpr float SCENE_NEAR = 0.1f;
constexpr unsigned long long EMPTY = 0xFFFFFFFFFFFFFFFFull;
constexpr float INF = __builtin_inff();

__global__ __launch_bounds__(256) void scene_project_kernel(
    const float* __restrict__ verts, const float* __restrict__ cam_t, const float* __restrict__ proj, long long PV, int V,
    long long npix, float* __restrict__ pv, unsigned long long* __restrict__ zbuf)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) zbuf[i] = EMPTY;
    if (i >= PV) return;
    const int p = (int)(i / V);
    const float* t = cam_t + (size_t)p * 3;
    const float* q = proj + (size_t)p * 6;
    const float* x = verts + (size_t)i * 3;
    const float z = x[2] + t[2];
    const float xn = (x[0] + t[0]) / z, yn = (x[1] + t[1]) / z;
    float* o = pv + (size_t)i * 3;
    o[0] = (q[0] * xn + q[1] * yn) + q[2];
    o[1] = (q[3] * xn + q[4] * yn) + q[5];
    o[2] = z;
}

__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return fabsf(a) < INF && fabsf(b) < INF && fabsf(c) < INF;       // (false for NaN)
}

__global__ __launch_bounds__(256) void scene_faces_kernel(
    const float* __restrict__ pv, int V, const int* __restrict__ faces2, int F2, const float* __restrict__ dscale,
    const int* __restrict__ person_frame, const long long* __restrict__ offsets, const int* __restrict__ shapes, int N,
    unsigned long long* __restrict__ zbuf)
{
    const int p = blockIdx.y;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F2) return;
    const int n = person_frame[p];
    if ((unsigned)n >= (unsigned)N) return;
    const int H = shapes[n * 2 + 0], W = shapes[n * 2 + 1];
    const int i0 = faces2[(size_t)f * 3 + 0], i1 = faces2[(size_t)f * 3 + 1], i2 = faces2[(size_t)f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
    const float* vb = pv + (size_t)p * V * 3;
    const float x0 = vb[(size_t)i0 * 3 + 0], y0 = vb[(size_t)i0 * 3 + 1], z0 = vb[(size_t)i0 * 3 + 2];
    const float x1 = vb[(size_t)i1 * 3 + 0], y1 = vb[(size_t)i1 * 3 + 1], z1 = vb[(size_t)i1 * 3 + 2];
    const float x2 = vb[(size_t)i2 * 3 + 0], y2 = vb[(size_t)i2 * 3 + 1], z2 = vb[(size_t)i2 * 3 + 2];
    if (!(z0 > SCENE_NEAR && z1 > SCENE_NEAR && z2 > SCENE_NEAR)) return;
    const float ds = dscale[p];
    if (!finite3(x0, x1, x2) || !finite3(y0, y1, y2) || !finite3(z0, z1, z2) || !(fabsf(ds) < INF)) return;
    const float area2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    if (!(area2 > 0.0f) || !(area2 < INF)) return;
    const float xmin = fminf(x0, fminf(x1, x2)), xmax = fmaxf(x0, fmaxf(x1, x2));
    const float ymin = fminf(y0, fminf(y1, y2)), ymax = fmaxf(y0, fmaxf(y1, y2));
    // pixel centres sit at integer (col, row); conservative candidate range (0.01 px slack >> rounding), clipped to the frame
    float cl = ceilf(xmin - 0.01f), ch = floorf(xmax + 0.01f);
    float rl = ceilf(ymin - 0.01f), rh = floorf(ymax + 0.01f);
    const float Wm = (float)(W - 1), Hm = (float)(H - 1);
    if (cl < 0.0f) cl = 0.0f;
    if (rl < 0.0f) rl = 0.0f;
    if (ch > Wm) ch = Wm;
    if (rh > Hm) rh = Hm;
    if (!(cl <= ch) || !(rl <= rh)) return;
    const int c0 = (int)cl, c1 = (int)ch, r0 = (int)rl, r1 = (int)rh;
    unsigned long long* zb = zbuf + (offsets[n] - offsets[0]) / 3;
    const unsigned int id = (unsigned int)p * (unsigned int)F2 + (unsigned int)f;
    for (int r = r0; r <= r1; ++r) {
        const float yp = (float)r;
        for (int cc = c0; cc <= c1; ++cc) {
            const float xp = (float)cc;
            const float e0 = (x1 - xp) * (y2 - yp) - (y1 - yp) * (x2 - xp);
            const float e1 = (x2 - xp) * (y0 - yp) - (y2 - yp) * (x0 - xp);
            const float e2 = (x0 - xp) * (y1 - yp) - (y0 - yp) * (x1 - xp);
            if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) continue;
            const float w0 = e0 / area2, w1 = e1 / area2, w2 = e2 / area2;
            const float zp = 1.0f / (w0 / z0 + w1 / z1 + w2 / z2);
            const float d = zp * ds;
            if (!(d > 0.0f && d < INF)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | id;
            atomicMin(&zb[(size_t)r * W + cc], key);
        }
    }
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__global__ __launch_bounds__(256) void scene_resolve_kernel(
    const unsigned long long* __restrict__ zbuf, const float* __restrict__ pv, const float* __restrict__ vcol, int V,
    const int* __restrict__ faces2, int F2, const unsigned char* __restrict__ src, long long src_bytes,
    const long long* __restrict__ offsets, const int* __restrict__ shapes, int N,
    unsigned char* __restrict__ out, int* __restrict__ ids, float* __restrict__ depth)
{
    const int n = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n == N) {                                        // what the buffer holds after the last frame (crop_params pads it)
        const long long at = offsets[N] + i;
        if (at < src_bytes) out[at] = src[at];
        return;
    }
    const int W = shapes[n * 2 + 1];
    if (i >= (long long)shapes[n * 2 + 0] * W) return;
    const long long g = (offsets[n] - offsets[0]) / 3 + i;                  // this pixel in the id / depth / key planes
    const long long at = offsets[n] + i * 3;
    const unsigned long long key = zbuf[g];
    if (key == EMPTY) {
        out[at + 0] = src[at + 0];
        out[at + 1] = src[at + 1];
        out[at + 2] = src[at + 2];
        if (ids) ids[g] = -1;
        if (depth) depth[g] = INF;
        return;
    }
    const unsigned int id = (unsigned int)(key & 0xFFFFFFFFull);
    const int p = (int)(id / (unsigned int)F2), f = (int)(id - (unsigned int)p * (unsigned int)F2);
    const int r = (int)(i / W), cc = (int)(i - (long long)r * W);
    const float xp = (float)cc, yp = (float)r;
    const int i0 = faces2[(size_t)f * 3 + 0], i1 = faces2[(size_t)f * 3 + 1], i2 = faces2[(size_t)f * 3 + 2];
    const float* vb = pv + (size_t)p * V * 3;
    const float z0 = vb[(size_t)i0 * 3 + 2], z1 = vb[(size_t)i1 * 3 + 2], z2 = vb[(size_t)i2 * 3 + 2];
    // vertex positions relative to the pixel centre
    const float x0 = vb[(size_t)i0 * 3 + 0] - xp, y0 = vb[(size_t)i0 * 3 + 1] - yp;
    const float x1 = vb[(size_t)i1 * 3 + 0] - xp, y1 = vb[(size_t)i1 * 3 + 1] - yp;
    const float x2 = vb[(size_t)i2 * 3 + 0] - xp, y2 = vb[(size_t)i2 * 3 + 1] - yp;
    float w0 = x1 * y2 - y1 * x2, w1 = x2 * y0 - y2 * x0, w2 = x0 * y1 - y0 * x1;
    const float area = w0 + w1 + w2;
    w0 = clamp01(w0 / area); w1 = clamp01(w1 / area); w2 = clamp01(w2 / area);
    float ws = w0 + w1 + w2;
    if (!(ws > 0.0f)) { w0 = w1 = w2 = 1.0f; ws = 3.0f; }      // (degenerate projection: the plain mean)
    w0 /= ws; w1 /= ws; w2 /= ws;
    const float p0 = w0 / z0, p1 = w1 / z1, p2 = w2 / z2;
    const float ps = p0 + p1 + p2;
    const float* cb = vcol + (size_t)p * V * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float v = (p0 * cb[(size_t)i0 * 3 + ch] + p1 * cb[(size_t)i1 * 3 + ch] + p2 * cb[(size_t)i2 * 3 + ch]) / ps;
        out[at + ch] = (unsigned char)rintf(clamp01(v) * 255.0f);           // round half to even
    }
    if (ids) ids[g] = (int)id;
    if (depth) depth[g] = __uint_as_float((unsigned int)(key >> 32));
}

size_t pv_bytes(int P, int V) { return ((size_t)P * V * 3 * sizeof(float) + 7) / 8 * 8; }

}  // namespace

// workspace: the projected vertices [P,V,3] f32 (col, row, Z + tz) followed by the 64-bit depth/id buffer, one word per frame pixel
extern "C" size_t danet_scene_render_ws_bytes(int P, int V, int64_t num_pixels) {
    if (P < 0 || V < 0 || num_pixels < 0) return 0;
    return pv_bytes(P, V) + (size_t)num_pixels * 8;
}

extern "C" int danet_scene_render(const float* verts, const float* vcol, int P, int V, const int32_t* faces2, int F2,
                                  const float* cam_t, const float* proj, const float* dscale, const int32_t* person_frame,
                                  const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* shapes, int N,
                                  const int32_t* host_person_frame, const int64_t* host_offsets, const int32_t* host_shapes,
                                  uint8_t* out, int32_t* ids, float* depth, void* ws, size_t ws_bytes, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(P >= 0 && P < 65535 && V > 0 && F2 > 0 && N > 0 && N < 65535 && src_bytes > 0,
                    "scene_render: bad sizes P=%d V=%d F2=%d N=%d src_bytes=%lld", P, V, F2, N, (long long)src_bytes);
    DANET_CHECK_ARG((long long)P * F2 < (1LL << 31), "scene_render: P * F2 = %lld does not fit the 31-bit id (person * F2 + face)",
                    (long long)P * F2);
    DANET_CHECK_ARG((long long)P * V < (1LL << 31), "scene_render: P * V = %lld vertices", (long long)P * V);
    DANET_CHECK_ARG(src && offsets && shapes && host_offsets && host_shapes && out && ws, "scene_render: null pointer");
    DANET_CHECK_ARG(P == 0 || (verts && vcol && faces2 && cam_t && proj && dscale && person_frame && host_person_frame),
                    "scene_render: null pointer with P=%d", P);
    DANET_CHECK_ARG(src != out, "scene_render: out must not be src (uncovered pixels are copied)");
    DANET_CHECK_ARG(((uintptr_t)ws & 7) == 0, "scene_render: workspace must be 8-byte aligned");
    DANET_CHECK_ARG(host_offsets[0] == 0, "scene_render: offsets[0] = %lld (the frames are packed from byte 0)", (long long)host_offsets[0]);
    long long maxpix = 0;
    for (int n = 0; n < N; ++n) {
        const long long H = host_shapes[n * 2 + 0], W = host_shapes[n * 2 + 1];
        DANET_CHECK_ARG(H > 0 && W > 0 && H * W < (1LL << 31), "scene_render: frame %d is %lld x %lld", n, H, W);
        DANET_CHECK_ARG(host_offsets[n + 1] - host_offsets[n] == 3 * H * W,
                        "scene_render: offsets[%d..%d] = %lld..%lld do not hold the %lld x %lld x 3 bytes of frame %d", n, n + 1,
                        (long long)host_offsets[n], (long long)host_offsets[n + 1], H, W, n);
        if (H * W > maxpix) maxpix = H * W;
    }
    DANET_CHECK_ARG(host_offsets[N] <= src_bytes, "scene_render: the frames end at byte %lld of %lld", (long long)host_offsets[N],
                    (long long)src_bytes);
    for (int p = 0; p < P; ++p) {
        DANET_CHECK_ARG(host_person_frame[p] >= 0 && host_person_frame[p] < N, "scene_render: person_frame[%d] = %d outside [0, %d)", p,
                        host_person_frame[p], N);
        DANET_CHECK_ARG(p == 0 || host_person_frame[p] >= host_person_frame[p - 1], "scene_render: person_frame decreases at %d", p);
    }
    const long long npix = (host_offsets[N] - host_offsets[0]) / 3;
    if (ws_bytes < danet_scene_render_ws_bytes(P, V, npix))
        return danet::fail(DANET_ERR_WORKSPACE, "scene_render: workspace %zu < %zu bytes", ws_bytes, danet_scene_render_ws_bytes(P, V, npix));
    hipStream_t st = (hipStream_t)stream;
    float* pv = (float*)ws;
    unsigned long long* zbuf = (unsigned long long*)((char*)ws + pv_bytes(P, V));
    const long long PV = (long long)P * V;
    const long long n1 = PV > npix ? PV : npix;
    hipLaunchKernelGGL(scene_project_kernel, dim3(danet::cdiv(n1, 256)), dim3(256), 0, st, verts, cam_t, proj, PV, V, npix, pv, zbuf);
    DANET_CHECK_LAUNCH("scene_project_kernel");
    if (P > 0) {
        hipLaunchKernelGGL(scene_faces_kernel, dim3(danet::cdiv(F2, 256), P), dim3(256), 0, st, pv, V, faces2, F2, dscale, person_frame,
                           (const long long*)offsets, shapes, N, zbuf);
        DANET_CHECK_LAUNCH("scene_faces_kernel");
    }
    const long long tail = src_bytes - host_offsets[N];
    const long long n3 = maxpix > tail ? maxpix : tail;
    hipLaunchKernelGGL(scene_resolve_kernel, dim3(danet::cdiv(n3, 256), N + 1), dim3(256), 0, st, zbuf, pv, vcol, V, faces2, F2, src,
                       (long long)src_bytes, (const long long*)offsets, shapes, N, out, ids, depth);
    DANET_CHECK_LAUNCH("scene_resolve_kernel");
    return DANET_OK;
}
