// The LSTM tree refinement of REFINE_STRATEGY 'lstm' / 'lstm_direct' (/root/reference/models/danet/smpl_regressor.py:742-822) as
// one op: pos [B,24,128] -> pos' [B,24,256].  Five bidirectional nn.LSTM(128, 128) run along six chains of the SMPL kinematic tree:
//   c0 = (0,3,6,9)         LSTM 0, zero state; its final (h_n, c_n) is H0
//   c1 = (12,15)           LSTM 0, initial state H0
//   c2 = (9,13,16,18,20,22) LSTM 1, H0         c3 = (9,14,17,19,21,23) LSTM 2, H0
//   c4 = (0,1,4,7,10)      LSTM 3, zero        c5 = (0,2,5,8,11)       LSTM 4, zero
// pos'[j] = cat(pos[j], pos[j]) + the output of the chain position that owns joint j: the last chain (c0 .. c5 order) holding j,
// except that joint 0 stays c0's.  H0 per direction: the forward direction's state after t = T-1, the reverse direction's after t = 0.
//
// Schedule.  A workgroup owns one (chain, direction, tile of BT batch rows).  Forward: phase A runs c0, c4, c5, phase B c1, c2, c3
// (which read c0's final state from the workspace) -- two launches.  In a workgroup every thread owns one gate row g of the 512: it
// holds W_ih[g,:] in registers for the input projection of every step (written to the workspace), then W_hh[g,:] in registers for
// the recurrence, reading h of the BT rows from LDS (broadcast).  Gate nonlinearities, c and h run one (row, unit) pair per thread.
// Backward: phase B' (c1, c2, c3; the gradients of their initial state go to separate slots), phase A' (c0 sums those three slots in
// a fixed order into the gradient of its final state), then one launch for the weight gradients (a chain-major, step-major, row-major
// fixed-order sum over the chains of each LSTM) and for d pos.  In the backward recurrence a thread owns one column e of W_hh for a
// quarter of the gate rows; the four quarters are summed in a fixed order.  fp32 operands, fp32 FMA accumulation, no atomics, no
// grid barrier: results are bitwise reproducible.
#include "common.h"

namespace {

constexpr int H = 128, G = 4 * H, NT = 512, BT = 8, NPOS = 28, ROW = G + 2 * H, NC = 6, NL = 5, TMAX = 6;
constexpr int GB = 16, RT = 256;            // reduction launch: gate rows per workgroup, threads per workgroup

__constant__ int kLen[NC] = {4, 2, 6, 6, 5, 5};
__constant__ int kOff[NC] = {0, 4, 6, 12, 18, 23};
__constant__ int kLstm[NC] = {0, 0, 1, 2, 3, 4};
__constant__ int kJoint[NPOS] = {0, 3, 6, 9, 12, 15, 9, 13, 16, 18, 20, 22, 9, 14, 17, 19, 21, 23, 0, 1, 4, 7, 10, 0, 2, 5, 8, 11};
__constant__ int kOwns[NPOS] = {1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1};

typedef danet_lstm_tree_args Args;

// workspace (forward -> backward): per (direction, chain position, batch row) the activated gates i, f, g, o, then c, then h
__device__ __forceinline__ size_t wsi(int d, int p, int b, int B) { return (((size_t)d * NPOS + p) * B + b) * ROW; }
// backward scratch: pre-activation gate gradients [2][28][B][512], input gradients [2][28][B][128], initial-state gradients of
// c1..c3 [3][2][B][256] (h then c)
__host__ __device__ __forceinline__ size_t sc_dx(int B) { return (size_t)2 * NPOS * B * G; }
__host__ __device__ __forceinline__ size_t sc_dinit(int B) { return sc_dx(B) + (size_t)2 * NPOS * B * H; }
__host__ __device__ __forceinline__ size_t sc_total(int B) { return sc_dinit(B) + (size_t)3 * 2 * B * 2 * H; }

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// chain of workgroup column ci in a phase: A = c0, c4, c5; B = c1, c2, c3
__device__ __forceinline__ int chain_of(int phase, int ci) { return phase ? ci + 1 : (ci == 0 ? 0 : ci + 3); }
// position whose state precedes position tt of a chain in direction d (-1: the initial state)
__device__ __forceinline__ int prev_pos(int d, int tt, int T) { const int p = d ? tt + 1 : tt - 1; return (p < 0 || p >= T) ? -1 : p; }
// c0's final-state position in direction d
__device__ __forceinline__ int c0_final(int d) { return d ? 0 : 3; }

__device__ __forceinline__ void load_row(float (&w)[H], const float* __restrict__ src) {
#pragma unroll
    for (int e = 0; e < H; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + e);
        w[e] = v.x; w[e + 1] = v.y; w[e + 2] = v.z; w[e + 3] = v.w;
    }
}

// acc[r] = sum_e w[e] * s[r][e] over the BT rows of an LDS matrix of stride H (all lanes read the same address: broadcast)
__device__ __forceinline__ void rows_dot(float (&acc)[BT], const float (&w)[H], const float* s) {
#pragma unroll
    for (int e = 0; e < H; e += 4) {
#pragma unroll
        for (int r = 0; r < BT; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(s + r * H + e);
            acc[r] = fmaf(w[e], v.x, acc[r]);
            acc[r] = fmaf(w[e + 1], v.y, acc[r]);
            acc[r] = fmaf(w[e + 2], v.z, acc[r]);
            acc[r] = fmaf(w[e + 3], v.w, acc[r]);
        }
    }
}

__global__ __launch_bounds__(NT) void lstm_tree_fwd_kernel(Args a, int phase)
{
    __shared__ __attribute__((aligned(16))) float xs[TMAX][BT][H];
    __shared__ __attribute__((aligned(16))) float hs[BT][H];
    __shared__ float gl[BT][G];
    const int t = threadIdx.x, B = a.B;
    const int c = chain_of(phase, blockIdx.x >> 1), d = blockIdx.x & 1;
    const int T = kLen[c], off = kOff[c], k = kLstm[c];
    const int b0 = blockIdx.y * BT;
    for (int i = t; i < T * BT * H; i += NT) {
        const int tt = i / (BT * H), r = (i / H) % BT, e = i % H, b = b0 + r;
        xs[tt][r][e] = b < B ? a.pos[((size_t)b * 24 + kJoint[off + tt]) * H + e] : 0.f;
    }
    // (row, unit) pairs of this thread: rows r0 and r0 + 4, unit e
    const int e = t & (H - 1), r0 = t >> 7;
    float cst[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = r0 + 4 * q, b = b0 + r;
        float h0 = 0.f, c0 = 0.f;
        if (phase && b < B) {
            const size_t s = wsi(d, c0_final(d), b, B);
            c0 = a.ws[s + G + e];
            h0 = a.ws[s + G + H + e];
        }
        cst[q] = c0;
        hs[r][e] = h0;
    }
    __syncthreads();

    // input projection of every step (+ both biases) into the gate slots of the workspace; thread t = gate row g
    // (W_ih streamed from L2 / the cache here: off the recurrence's critical path, and it keeps the registers for W_hh)
    const int g = t;
    const float bias = a.b_ih[k][d][g] + a.b_hh[k][d][g];
    const float* wih = a.w_ih[k][d] + (size_t)g * H;
    for (int tt = 0; tt < T; ++tt) {
        float acc[BT];
#pragma unroll
        for (int r = 0; r < BT; ++r) acc[r] = bias;
#pragma unroll 4
        for (int e4 = 0; e4 < H; e4 += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(wih + e4);
#pragma unroll
            for (int r = 0; r < BT; ++r) {
                const float4 v = *reinterpret_cast<const float4*>(&xs[tt][r][e4]);
                acc[r] = fmaf(wv.x, v.x, acc[r]);
                acc[r] = fmaf(wv.y, v.y, acc[r]);
                acc[r] = fmaf(wv.z, v.z, acc[r]);
                acc[r] = fmaf(wv.w, v.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < BT; ++r)
            if (b0 + r < B) a.ws[wsi(d, off + tt, b0 + r, B) + g] = acc[r];
    }
    float w[H];
    load_row(w, a.w_hh[k][d] + (size_t)g * H);

    for (int s = 0; s < T; ++s) {
        const int tt = d ? T - 1 - s : s;
        float acc[BT];
#pragma unroll
        for (int r = 0; r < BT; ++r) acc[r] = b0 + r < B ? a.ws[wsi(d, off + tt, b0 + r, B) + g] : 0.f;
        rows_dot(acc, w, &hs[0][0]);
#pragma unroll
        for (int r = 0; r < BT; ++r) gl[r][g] = acc[r];
        __syncthreads();
        const int j = kJoint[off + tt];
        const bool owns = kOwns[off + tt];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = r0 + 4 * q, b = b0 + r;
            const float gi = sigm(gl[r][e]), gf = sigm(gl[r][H + e]), gg = tanhf(gl[r][2 * H + e]), go = sigm(gl[r][3 * H + e]);
            const float cn = fmaf(gf, cst[q], gi * gg);
            const float hn = go * tanhf(cn);
            cst[q] = cn;
            hs[r][e] = hn;
            if (b < B) {
                float* o = a.ws + wsi(d, off + tt, b, B);
                o[e] = gi; o[H + e] = gf; o[2 * H + e] = gg; o[3 * H + e] = go;
                o[G + e] = cn; o[G + H + e] = hn;
                if (owns) a.out[((size_t)b * 24 + j) * (2 * H) + d * H + e] = xs[tt][r][e] + hn;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void lstm_tree_bwd_kernel(Args a, int phase)
{
    __shared__ __attribute__((aligned(16))) float dg[BT][G];
    __shared__ float part[4][BT][H];
    const int t = threadIdx.x, B = a.B;
    const int c = chain_of(phase, blockIdx.x >> 1), d = blockIdx.x & 1;
    const int T = kLen[c], off = kOff[c], k = kLstm[c];
    const int b0 = blockIdx.y * BT;
    const int e = t & (H - 1), r0 = t >> 7;        // (row, unit) pairs: rows r0, r0 + 4; matrix role: column e, gate quarter r0
    float* dgates = a.scratch;
    float* dxs = a.scratch + sc_dx(B);
    float* dinit = a.scratch + sc_dinit(B);

    float dh_next[2], dc_next[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int b = b0 + r0 + 4 * q;
        float dh = 0.f, dc = 0.f;
        if (c == 0 && b < B) {
            for (int cc = 0; cc < 3; ++cc) {          // c1, c2, c3 in order
                const float* s = dinit + (((size_t)cc * 2 + d) * B + b) * (2 * H);
                dh += s[e];
                dc += s[H + e];
            }
        }
        dh_next[q] = dh; dc_next[q] = dc;
    }
    // column e of W_hh over the gate rows [128 * r0, 128 * r0 + 128)
    float w[H];
    {
        const float* src = a.w_hh[k][d] + (size_t)(r0 * H) * H + e;
#pragma unroll
        for (int i = 0; i < H; ++i) w[i] = src[(size_t)i * H];
    }
    for (int s = 0; s < T; ++s) {
        const int tt = d ? s : T - 1 - s;
        const int tp = prev_pos(d, tt, T);
        const int j = kJoint[off + tt];
        const bool owns = kOwns[off + tt];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = r0 + 4 * q, b = b0 + r;
            float dai = 0.f, daf = 0.f, dag = 0.f, dao = 0.f;
            if (b < B) {
                const float* o = a.ws + wsi(d, off + tt, b, B);
                const float gi = o[e], gf = o[H + e], gg = o[2 * H + e], go = o[3 * H + e], cn = o[G + e];
                float cp = 0.f;
                if (tp >= 0) cp = a.ws[wsi(d, off + tp, b, B) + G + e];
                else if (phase) cp = a.ws[wsi(d, c0_final(d), b, B) + G + e];
                float dh = dh_next[q];
                if (owns) dh += a.g_out[((size_t)b * 24 + j) * (2 * H) + d * H + e];
                const float tc = tanhf(cn);
                const float dc = fmaf(dh * go, 1.f - tc * tc, dc_next[q]);
                dao = dh * tc * go * (1.f - go);
                dai = dc * gg * gi * (1.f - gi);
                daf = dc * cp * gf * (1.f - gf);
                dag = dc * gi * (1.f - gg * gg);
                dc_next[q] = dc * gf;
                float* so = dgates + (((size_t)d * NPOS + off + tt) * B + b) * G;
                so[e] = dai; so[H + e] = daf; so[2 * H + e] = dag; so[3 * H + e] = dao;
            }
            dg[r][e] = dai; dg[r][H + e] = daf; dg[r][2 * H + e] = dag; dg[r][3 * H + e] = dao;
        }
        __syncthreads();
        {
            float acc[BT];
#pragma unroll
            for (int r = 0; r < BT; ++r) acc[r] = 0.f;
            // d h_prev[r][e] (quarter r0) = sum_i dg[r][128 r0 + i] W_hh[128 r0 + i][e]
#pragma unroll
            for (int i = 0; i < H; i += 4) {
#pragma unroll
                for (int r = 0; r < BT; ++r) {
                    const float4 v = *reinterpret_cast<const float4*>(&dg[r][r0 * H + i]);
                    acc[r] = fmaf(w[i], v.x, acc[r]);
                    acc[r] = fmaf(w[i + 1], v.y, acc[r]);
                    acc[r] = fmaf(w[i + 2], v.z, acc[r]);
                    acc[r] = fmaf(w[i + 3], v.w, acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < BT; ++r) part[r0][r][e] = acc[r];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = r0 + 4 * q;
            dh_next[q] = ((part[0][r][e] + part[1][r][e]) + part[2][r][e]) + part[3][r][e];
        }
    }
    if (phase) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int b = b0 + r0 + 4 * q;
            if (b < B) {
                float* s = dinit + (((size_t)(c - 1) * 2 + d) * B + b) * (2 * H);
                s[e] = dh_next[q];
                s[H + e] = dc_next[q];
            }
        }
    }
    // input gradients of every step: dx_t = dgates_t . W_ih (column e, quarter r0; quarters summed in order)
    __syncthreads();
    {
        const float* src = a.w_ih[k][d] + (size_t)(r0 * H) * H + e;
#pragma unroll
        for (int i = 0; i < H; ++i) w[i] = src[(size_t)i * H];
    }
    for (int tt = 0; tt < T; ++tt) {
        for (int i = t; i < BT * G; i += NT) {
            const int r = i / G, gg = i % G, b = b0 + r;
            dg[r][gg] = b < B ? dgates[(((size_t)d * NPOS + off + tt) * B + b) * G + gg] : 0.f;
        }
        __syncthreads();
        float acc[BT];
#pragma unroll
        for (int r = 0; r < BT; ++r) acc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < H; i += 4) {
#pragma unroll
            for (int r = 0; r < BT; ++r) {
                const float4 v = *reinterpret_cast<const float4*>(&dg[r][r0 * H + i]);
                acc[r] = fmaf(w[i], v.x, acc[r]);
                acc[r] = fmaf(w[i + 1], v.y, acc[r]);
                acc[r] = fmaf(w[i + 2], v.z, acc[r]);
                acc[r] = fmaf(w[i + 3], v.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < BT; ++r) part[r0][r][e] = acc[r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = r0 + 4 * q, b = b0 + r;
            if (b < B)
                dxs[(((size_t)d * NPOS + off + tt) * B + b) * H + e] = ((part[0][r][e] + part[1][r][e]) + part[2][r][e]) + part[3][r][e];
        }
        __syncthreads();
    }
}

// Workgroups [0, NL * 2 * G / GB): weight and bias gradients of one (LSTM, direction, block of GB gate rows); thread = column:
// [0, 128) of W_ih (the input x), [128, 256) of W_hh (the previous h).  The rest: d pos, one element per thread.
__global__ __launch_bounds__(RT) void lstm_tree_wgrad_kernel(Args a)
{
    __shared__ float sdg[32][GB];
    const int t = threadIdx.x, B = a.B;
    const int nw = NL * 2 * (G / GB);
    const float* dgates = a.scratch;
    if ((int)blockIdx.x >= nw) {
        const size_t idx = (size_t)(blockIdx.x - nw) * RT + t;
        if (idx >= (size_t)B * 24 * H) return;
        const int e = idx % H, j = (idx / H) % 24;
        const size_t b = idx / (24 * H);
        const float* go = a.g_out + (b * 24 + j) * (2 * H);
        float v = go[e] + go[H + e];
        const float* dxs = a.scratch + sc_dx(B);
        for (int p = 0; p < NPOS; ++p) {
            if (kJoint[p] != j) continue;
            for (int d = 0; d < 2; ++d) v += dxs[(((size_t)d * NPOS + p) * B + b) * H + e];
        }
        a.g_pos[idx] = v;
        return;
    }
    const int k = blockIdx.x / (2 * (G / GB)), d = (blockIdx.x / (G / GB)) & 1, g0 = (blockIdx.x % (G / GB)) * GB;
    const int col = t & (H - 1);
    const bool hcol = t >= H;
    float acc[GB];
#pragma unroll
    for (int i = 0; i < GB; ++i) acc[i] = 0.f;
    float bacc = 0.f;
    for (int c = 0; c < NC; ++c) {
        if (kLstm[c] != k) continue;
        const int T = kLen[c], off = kOff[c];
        for (int tt = 0; tt < T; ++tt) {
            const int tp = prev_pos(d, tt, T);
            const int j = kJoint[off + tt];
            for (int bb = 0; bb < B; bb += 32) {
                const int nb = min(32, B - bb);
                __syncthreads();
                for (int i = t; i < 32 * GB; i += RT) {
                    const int r = i / GB, gg = i % GB;
                    sdg[r][gg] = r < nb ? dgates[(((size_t)d * NPOS + off + tt) * B + bb + r) * G + g0 + gg] : 0.f;
                }
                __syncthreads();
                for (int r = 0; r < nb; ++r) {
                    const int b = bb + r;
                    float v;
                    if (!hcol) v = a.pos[((size_t)b * 24 + j) * H + col];
                    else if (tp >= 0) v = a.ws[wsi(d, off + tp, b, B) + G + H + col];
                    else if (c >= 1 && c <= 3) v = a.ws[wsi(d, c0_final(d), b, B) + G + H + col];
                    else v = 0.f;
#pragma unroll
                    for (int i = 0; i < GB; ++i) acc[i] = fmaf(sdg[r][i], v, acc[i]);
                    if (t < GB) bacc += sdg[r][t];
                }
            }
        }
    }
    float* gw = hcol ? a.g_w_hh[k][d] : a.g_w_ih[k][d];
#pragma unroll
    for (int i = 0; i < GB; ++i) gw[(size_t)(g0 + i) * H + col] = acc[i];
    if (t < GB) {
        a.g_b_ih[k][d][g0 + t] = bacc;
        a.g_b_hh[k][d][g0 + t] = bacc;
    }
}

int check_args(const Args* a, const char* what) {
    DANET_CHECK_ARG(a && a->pos && a->ws && a->B >= 1 && a->B <= (1 << 20), "%s: bad arguments (1 <= B <= 2^20)", what);
    for (int k = 0; k < NL; ++k)
        for (int d = 0; d < 2; ++d)
            DANET_CHECK_ARG(a->w_ih[k][d] && a->w_hh[k][d] && a->b_ih[k][d] && a->b_hh[k][d], "%s: LSTM %d direction %d lacks a parameter", what, k, d);
    return DANET_OK;
}

}  // namespace

extern "C" int danet_lstm_tree_ok(int B) { return B >= 1 && B <= (1 << 20); }
extern "C" size_t danet_lstm_tree_ws_floats(int B) { return B < 1 ? 0 : (size_t)2 * NPOS * B * ROW; }
extern "C" size_t danet_lstm_tree_scratch_floats(int B) { return B < 1 ? 0 : sc_total(B); }

extern "C" int danet_lstm_tree_forward(const void* args, void* stream)
{
    DANET_ENTER();
    const Args* a = (const Args*)args;
    if (int e = check_args(a, "lstm_tree_forward")) return e;
    DANET_CHECK_ARG(a->out, "lstm_tree_forward: missing output");
    const dim3 grid(2 * 3, danet::cdiv(a->B, BT));
    for (int phase = 0; phase < 2; ++phase) {
        hipLaunchKernelGGL(lstm_tree_fwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, *a, phase);
        DANET_CHECK_LAUNCH("lstm_tree_fwd_kernel");
    }
    return DANET_OK;
}

extern "C" int danet_lstm_tree_backward(const void* args, void* stream)
{
    DANET_ENTER();
    const Args* a = (const Args*)args;
    if (int e = check_args(a, "lstm_tree_backward")) return e;
    DANET_CHECK_ARG(a->g_out && a->g_pos && a->scratch, "lstm_tree_backward: missing gradient buffers");
    for (int k = 0; k < NL; ++k)
        for (int d = 0; d < 2; ++d)
            DANET_CHECK_ARG(a->g_w_ih[k][d] && a->g_w_hh[k][d] && a->g_b_ih[k][d] && a->g_b_hh[k][d],
                            "lstm_tree_backward: LSTM %d direction %d lacks a gradient buffer", k, d);
    const dim3 grid(2 * 3, danet::cdiv(a->B, BT));
    for (int phase = 1; phase >= 0; --phase) {
        hipLaunchKernelGGL(lstm_tree_bwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, *a, phase);
        DANET_CHECK_LAUNCH("lstm_tree_bwd_kernel");
    }
    const int nw = NL * 2 * (G / GB) + danet::cdiv((long)a->B * 24 * H, RT);
    hipLaunchKernelGGL(lstm_tree_wgrad_kernel, dim3(nw), dim3(RT), 0, (hipStream_t)stream, *a);
    DANET_CHECK_LAUNCH("lstm_tree_wgrad_kernel");
    return DANET_OK;
}
