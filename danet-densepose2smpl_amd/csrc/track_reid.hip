// Streaming identities for gfx950 (DESIGN.md 4b'-reid "the causal identity rule"; tracks.StreamDescriptor is the caller): the descriptor
// of a track (tracks.descriptors: its weighted mean shape and the texture fused over its observed rows) kept as running sums, one frame
// at a time, for S slots.
//
//   track_desc_step   one lane per (person of the frame, texel).  The lane loads the four unnormalised sums (sum cs r, sum cs g, sum cs b,
//                     sum cs) of its texel of the person's slot (one 16-byte load), adds this frame's view with danet::add_view
//                     (unwrap_view.h), the function texture_unwrap_kernel (texture_ops.hip) loops, and stores them (one 16-byte store).  The
//                     sums after n views are the registers of texture_unwrap_kernel after the same n views: dividing them gives its bits.
//                     Eleven lanes of each person's first workgroup add the row to the shape sums as track_group_mean_kernel
//                     (track_link.hip) adds it: sum_c += (double)c, sum_y += (double)c * (double)beta, only where c > 0.  A gap row
//                     (observed 0) adds to the shape alone: its image, mesh and depth are never read.  S further rows of workgroups empty the
//                     slots named in `reset` that hold no person of this frame; a person's lanes empty their own slot by starting from 0.
//   track_desc_read   one lane per (pair, texel): the descriptor of a slot goes into a row of the table, unwrap's danet::texel for the skin,
//                     (float)(sum_y / sum_c) for the shape; the raw shape sums go beside it in double.
//   track_desc_shape  one lane per (row, shape column): the betas of an emitted row become (float)((carry_y + sum_y) / (carry_c + sum_c)).
//
// No atomics, no LDS, no grid barrier, no inline assembly; no slot appears twice in a launch (refused on the host), so every state word
// has one reader and writer.  Compiled with -ffp-contract=off.
#include <vector>

#include "common.h"
#include "unwrap_view.h"
#include "video_sizes.h"

using namespace danet;

namespace {

constexpr int kShapeWords = 12;                       // sum_y [10], sum_c, one spare: a slot's shape sums are 96 bytes

__device__ __forceinline__ float4* slot_acc(void* state, int s, int ntex) { return (float4*)state + (size_t)s * ntex; }

__device__ __forceinline__ double* slot_shape(void* state, int S, int s, int ntex)
{
    return (double*)((float4*)state + (size_t)S * ntex) + (size_t)s * kShapeWords;
}

struct StepArgs {
    ViewInputs view;                                                         // the chunk's frames: person p is view p
    const float *para, *conf, *map_bary;
    const int32_t *slot, *observed, *reset, *vert_mapping, *faces, *map_face;
    int S, P, NDV, F, ntex;
};

__global__ __launch_bounds__(256) void track_desc_step_kernel(void* __restrict__ state, const StepArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if ((int)blockIdx.y >= a.P) {                                            // the rows of workgroups that only empty a slot
        const int s = (int)blockIdx.y - a.P;
        if (s >= a.S || a.reset[s] == 0) return;
        for (int q = 0; q < a.P; ++q)
            if (a.slot[q] == s) return;                                      // (its person's lanes do it)
        if (t < a.ntex) slot_acc(state, s, a.ntex)[t] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        if (blockIdx.x == 0 && threadIdx.x < kShapeWords) slot_shape(state, a.S, s, a.ntex)[threadIdx.x] = 0.0;
        return;
    }
    const int p = blockIdx.y;
    const int s = a.slot[p];
    if (s < 0 || s >= a.S) return;
    const bool fresh = a.reset[s] != 0;
    const bool seen = a.observed[p] != 0;
    if (blockIdx.x == 0 && threadIdx.x <= kNB) {                             // the shape sums: lanes 0 .. 9 a column each, lane 10 the weight
        double* sh = slot_shape(state, a.S, s, a.ntex) + threadIdx.x;
        double v = fresh ? 0.0 : *sh;
        const float c = a.conf[p];
        if (c > 0.0f) v += threadIdx.x < kNB ? (double)c * (double)a.para[(size_t)p * kParaRow + 3 + threadIdx.x] : (double)c;
        if (fresh || c > 0.0f) *sh = v;
    }
    if (t >= a.ntex || !(seen || fresh)) return;
    float4* acc = slot_acc(state, s, a.ntex) + t;
    float4 sum = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if (!fresh) sum = *acc;
    const int f = a.map_face[t];
    if (seen && f >= 0 && f < a.F) {
        float sr = sum.x, sg = sum.y, sb = sum.z, sw = sum.w;
        const float w0 = a.map_bary[t * 2 + 0], w1 = a.map_bary[t * 2 + 1];
        const float w2 = 1.0f - w0 - w1;
        const int d0 = a.faces[f * 3 + 0], d1 = a.faces[f * 3 + 1], d2 = a.faces[f * 3 + 2];
        const bool named = d0 >= 0 && d0 < a.NDV && d1 >= 0 && d1 < a.NDV && d2 >= 0 && d2 < a.NDV;
        const int i0 = named ? a.vert_mapping[d0] : -1, i1 = named ? a.vert_mapping[d1] : -1, i2 = named ? a.vert_mapping[d2] : -1;
        const int NV = a.view.NV;
        if (i0 >= 0 && i0 < NV && i1 >= 0 && i1 < NV && i2 >= 0 && i2 < NV)      // (anything else is refused on the host already)
            add_view(a.view, p, i0, i1, i2, w0, w1, w2, sr, sg, sb, sw);          // the frame's one view: person p of the chunk
        sum = float4{sr, sg, sb, sw};
    }
    *acc = sum;
}

__global__ __launch_bounds__(256) void track_desc_read_kernel(const void* __restrict__ state, int S, int ntex, const int32_t* __restrict__ pairs,
                                                              int n, int R, float* __restrict__ desc_shape, float4* __restrict__ desc_atlas,
                                                              double* __restrict__ desc_sums, int32_t* __restrict__ status)
{
    const int q = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int s = pairs[2 * q], row = pairs[2 * q + 1];
    if (s < 0 || s >= S || row < 0 || row >= R) return;                     // (refused on the host already)
    if (blockIdx.x == 0 && threadIdx.x <= kNB) {
        const double* sh = slot_shape(const_cast<void*>(state), S, s, ntex);
        const double sc = sh[kNB];
        const double v = sh[threadIdx.x];
        desc_sums[(size_t)row * (kNB + 1) + threadIdx.x] = v;
        if (threadIdx.x < kNB) desc_shape[(size_t)row * kNB + threadIdx.x] = sc > 0.0 ? (float)(v / sc) : 0.0f;
        else status[row] = sc > 0.0 ? 0 : 1;
    }
    if (t >= ntex) return;
    const float4 sum = slot_acc(const_cast<void*>(state), s, ntex)[t];
    desc_atlas[(size_t)row * ntex + t] = texel(sum.x, sum.y, sum.z, sum.w);
}

__global__ __launch_bounds__(64) void track_desc_shape_kernel(const void* __restrict__ state, int S, int ntex, float* __restrict__ rows,
                                                              const int32_t* __restrict__ slot, const double* __restrict__ carry,
                                                              const int32_t* __restrict__ use, int P)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= P * kNB) return;
    const int p = idx / kNB, j = idx - p * kNB;
    const int s = slot[p];
    if (use[p] == 0 || s < 0 || s >= S) return;
    const double* sh = slot_shape(const_cast<void*>(state), S, s, ntex);
    const double den = carry[(size_t)p * (kNB + 1) + kNB] + sh[kNB];
    if (!(den > 0.0)) return;
    rows[(size_t)p * kParaRow + 3 + j] = (float)((carry[(size_t)p * (kNB + 1) + j] + sh[j]) / den);
}

bool sizes_ok(int S, int T) { return S >= 1 && S <= 4096 && T >= 2 && T <= 4096 && (long)kParts * T * T < (1L << 24); }

size_t state_bytes(int S, int T) { return (size_t)S * ((size_t)kParts * T * T * 16 + (size_t)kShapeWords * 8); }

}  // namespace

extern "C" size_t danet_track_desc_state_bytes(int S, int T) { return sizes_ok(S, T) ? state_bytes(S, T) : 0; }

extern "C" int danet_track_desc_step(void* state, size_t state_nbytes, int S, int T, const float* images, const float* verts, const float* cam,
                                     const float* depth, int P, int NV, int H, const float* para, const float* conf, const int32_t* slot,
                                     const int32_t* slot_host, const int32_t* observed, const int32_t* reset, const int32_t* vert_mapping,
                                     int NDV, const int32_t* faces, int F, const int32_t* map_face, const float* map_bary, float focal,
                                     float depth_tol, float min_cos, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(sizes_ok(S, T), "track_desc_step: bad sizes S=%d T=%d", S, T);
    DANET_CHECK_ARG(P >= 0 && P < 32768, "track_desc_step: bad chunk P=%d", P);
    if (P == 0) return DANET_OK;
    DANET_CHECK_ARG(NV > 0 && NDV > 0 && F > 0 && H > 0 && H <= 4096, "track_desc_step: bad sizes NV=%d NDV=%d F=%d H=%d", NV, NDV, F, H);
    DANET_CHECK_ARG(state && state_nbytes >= state_bytes(S, T), "track_desc_step: the state holds %zu bytes, %zu needed", state_nbytes,
                    state_bytes(S, T));
    DANET_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 15) == 0, "track_desc_step: the state must be 16-byte aligned");
    DANET_CHECK_ARG(images && verts && cam && depth && para && conf && slot && slot_host && observed && reset && vert_mapping && faces &&
                    map_face && map_bary, "track_desc_step: null pointer");
    std::vector<unsigned char> taken((size_t)S, 0);                            // no slot twice: one reader and writer per state word
    for (int p = 0; p < P; ++p) {
        const int32_t s = slot_host[p];
        DANET_CHECK_ARG(s >= -1 && s < S, "track_desc_step: slot[%d] = %d outside [-1, %d)", p, s, S);
        if (s < 0) continue;
        DANET_CHECK_ARG(!taken[(size_t)s], "track_desc_step: slot %d appears twice", s);
        taken[(size_t)s] = 1;
    }
    StepArgs a;
    a.view = ViewInputs{images, verts, cam, depth, NV, H, focal, depth_tol, min_cos};
    a.para = para; a.conf = conf; a.map_bary = map_bary;
    a.slot = slot; a.observed = observed; a.reset = reset; a.vert_mapping = vert_mapping; a.faces = faces; a.map_face = map_face;
    a.S = S; a.P = P; a.NDV = NDV; a.F = F; a.ntex = kParts * T * T;
    hipLaunchKernelGGL(track_desc_step_kernel, dim3(danet::cdiv(a.ntex, 256), P + S), dim3(256), 0, (hipStream_t)stream, state, a);
    DANET_CHECK_LAUNCH("track_desc_step_kernel");
    return DANET_OK;
}

extern "C" int danet_track_desc_read(const void* state, size_t state_nbytes, int S, int T, const int32_t* pairs, const int32_t* pairs_host,
                                     int n, int R, float* desc_shape, float* desc_atlas, double* desc_sums, int32_t* status, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(sizes_ok(S, T), "track_desc_read: bad sizes S=%d T=%d", S, T);
    DANET_CHECK_ARG(n >= 0 && n < 32768 && R >= 1 && R < (1 << 20), "track_desc_read: bad sizes n=%d R=%d", n, R);
    if (n == 0) return DANET_OK;
    DANET_CHECK_ARG(state && state_nbytes >= state_bytes(S, T), "track_desc_read: the state holds %zu bytes, %zu needed", state_nbytes,
                    state_bytes(S, T));
    DANET_CHECK_ARG(pairs && pairs_host && desc_shape && desc_atlas && desc_sums && status, "track_desc_read: null pointer");
    DANET_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 15) == 0 && (reinterpret_cast<uintptr_t>(desc_atlas) & 15) == 0,
                    "track_desc_read: the state and desc_atlas must be 16-byte aligned");
    std::vector<unsigned char> written((size_t)R, 0);
    for (int q = 0; q < n; ++q) {
        const int32_t s = pairs_host[2 * q], row = pairs_host[2 * q + 1];
        DANET_CHECK_ARG(s >= 0 && s < S && row >= 0 && row < R, "track_desc_read: pair %d = (slot %d, row %d) outside [0, %d) x [0, %d)", q, s,
                        row, S, R);
        DANET_CHECK_ARG(!written[(size_t)row], "track_desc_read: row %d is written twice", row);
        written[(size_t)row] = 1;
    }
    const int ntex = kParts * T * T;
    hipLaunchKernelGGL(track_desc_read_kernel, dim3(danet::cdiv(ntex, 256), n), dim3(256), 0, (hipStream_t)stream, state, S, ntex, pairs, n, R,
                       desc_shape, (float4*)desc_atlas, desc_sums, status);
    DANET_CHECK_LAUNCH("track_desc_read_kernel");
    return DANET_OK;
}

extern "C" int danet_track_desc_shape(const void* state, size_t state_nbytes, int S, int T, float* rows, const int32_t* slot,
                                      const int32_t* slot_host, const double* carry, const int32_t* use, int P, void* stream)
{
    DANET_ENTER();
    DANET_CHECK_ARG(sizes_ok(S, T), "track_desc_shape: bad sizes S=%d T=%d", S, T);
    DANET_CHECK_ARG(P >= 0 && P < 32768, "track_desc_shape: bad chunk P=%d", P);
    if (P == 0) return DANET_OK;
    DANET_CHECK_ARG(state && state_nbytes >= state_bytes(S, T), "track_desc_shape: the state holds %zu bytes, %zu needed", state_nbytes,
                    state_bytes(S, T));
    DANET_CHECK_ARG(rows && slot && slot_host && carry && use, "track_desc_shape: null pointer");
    for (int p = 0; p < P; ++p)
        DANET_CHECK_ARG(slot_host[p] >= -1 && slot_host[p] < S, "track_desc_shape: slot[%d] = %d outside [-1, %d)", p, slot_host[p], S);
    hipLaunchKernelGGL(track_desc_shape_kernel, dim3(danet::cdiv((long)P * kNB, 64)), dim3(64), 0, (hipStream_t)stream, state, S,
                       kParts * T * T, rows, slot, carry, use, P);
    DANET_CHECK_LAUNCH("track_desc_shape_kernel");
    return DANET_OK;
}
