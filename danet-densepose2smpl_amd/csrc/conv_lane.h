// Lane primitives and epilogue pieces of the convolution kernels, each written once.  Included after conv_common.h.
// Everything here is inlined into its caller and compiles the same with and without -amdgpu-mfma-vgpr-form.  What stays per kernel,
// on purpose: the hand-counted weight rings (the *_KSTEP macros, load_a / refill / issue_mine, conv3x3s.hip's ring), every barrier,
// and the pieces that compiled to other code when shared (named where they would stand below).
#pragma once
#include "conv_common.h"

namespace danet_conv {

typedef __attribute__((ext_vector_type(4))) int i32x4;               // 16 bytes of a buffer load / store, a raw buffer descriptor
typedef __attribute__((ext_vector_type(2))) int i32x2;               // 8 bytes: four bf16 values
typedef __attribute__((ext_vector_type(2))) unsigned v2u;            // a transposing LDS read's result
typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr int OOB = 0x7fffffff;      // a buffer offset beyond every buffer (sizes are checked to be < 2^31 bytes): zeros in, nothing out

// ---- primitives --------------------------------------------------------------------------------------------------------------------
// n / d for n < 2^24 (checked by the host) with rcp = 1.0f / d: a float reciprocal and a fix-up (every gather and tile index of the conv kernels).
__device__ __forceinline__ unsigned udiv24(unsigned n, unsigned d, float rcp) {
    unsigned q = (unsigned)((float)n * rcp);
    const int r = (int)(n - q * d);
    if (r < 0) --q; else if (r >= (int)d) ++q;
    return q;
}
// Workgroup barrier that orders LDS traffic only: global stores of an epilogue keep draining across it (__syncthreads() would wait
// for them: its fence covers every address space).  The LDS-tile, streamed and stem kernels.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// v + (v of the lane DPP control CTRL names); row_sum16: the sum over the 16 lanes of a DPP row, in every lane (xor 1, xor 2,
// half-row mirror, row mirror).  Every per-channel statistic of a conv kernel leaves its 16 pixel lanes through these.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, o);
}
__device__ __forceinline__ float row_sum16(float v) {
    v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);     // row_half_mirror
    v = dpp_add<0x140>(v);     // row_mirror
    return v;
}
// One LDS-DMA copy instruction: 64 lanes x 16 bytes from desc[voff + soff] to the 1 KB piece at LDS address lds_addr; an out-of-range
// lane writes zeros.  M0 is written in the statement that uses it: the compiler does not preserve it.  conv3x3s / conv3x3a / the stem kernels.
__device__ __forceinline__ void dma16(unsigned lds_addr, int voff, const i32x4& desc, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(lds_addr), "v"(voff), "s"(desc), "s"(soff) : "memory");
}
// Raw buffer descriptor (stride 0, num_records in bytes) as the four scalars inline-asm buffer loads take.  The same kernels.
__device__ __forceinline__ i32x4 raw_desc(const void* base, int bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    return i32x4{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu)),
                 __builtin_amdgcn_readfirstlane(bytes), 0x00020000};
}
// Transposing LDS read (ds_read_b64_tr_b16): four bf16 of an MFMA operand from a tile staged as it lies in memory.  The weight-gradient kernels.
__device__ __forceinline__ v2u tr_read(unsigned lds_byte_addr) {
    v2u r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(lds_byte_addr) : "memory");
    return r;
}

// ---- epilogue pieces ---------------------------------------------------------------------------------------------------------------
// Four packed bf16 values as fp32 (exact).  The statistics of the rounded output (conv3x3a, conv_stem), the BatchNorm tail's operands
// (conv3x3s).  (conv_fast / conv3x3 unpack their BatchNorm-backward operands into float[4]: as f32x4 values their code changed.)
__device__ __forceinline__ f32x4 bf16x4_to_f32(i32x2 q) {
    return f32x4{__uint_as_float((unsigned)q.x << 16), __uint_as_float((unsigned)q.x & 0xffff0000u),
                 __uint_as_float((unsigned)q.y << 16), __uint_as_float((unsigned)q.y & 0xffff0000u)};
}
// v + a bf16x4 addend (the residual branch's tensor, added before the output is rounded).  Every kernel with an `addend` argument.
// (By value, `v = add_bf16x4(v, q)`: through a reference conv_fast.hip compiled to other code.)
__device__ __forceinline__ f32x4 add_bf16x4(f32x4 v, i32x2 q) {
    v[0] += __uint_as_float((unsigned)q.x << 16); v[1] += __uint_as_float((unsigned)q.x & 0xffff0000u);
    v[2] += __uint_as_float((unsigned)q.y << 16); v[3] += __uint_as_float((unsigned)q.y & 0xffff0000u);
    return v;
}
// s1 += v, s2 += v * v on a lane's four channels, two values per instruction (v_pk_add_f32, v_pk_fma_f32).  conv3x3a / conv_stem feed
// it the bf16-ROUNDED output (bf16x4_to_f32 of the packed pairs), conv3x3s the accumulator.  (conv_pw.hip keeps the same text with its
// validity mask multiplied in: through this function its instruction order changed, and one layer measured slower.)
__device__ __forceinline__ void sums_add(float (&s1)[4], float (&s2)[4], f32x4 v) {
    f32x2_ lo = {v[0], v[1]}, hi = {v[2], v[3]};
    f32x2_& a0 = *reinterpret_cast<f32x2_*>(&s1[0]); f32x2_& a1 = *reinterpret_cast<f32x2_*>(&s1[2]);
    f32x2_& q0 = *reinterpret_cast<f32x2_*>(&s2[0]); f32x2_& q1 = *reinterpret_cast<f32x2_*>(&s2[2]);
    a0 += lo; a1 += hi;
    q0 = __builtin_elementwise_fma(lo, lo, q0); q1 = __builtin_elementwise_fma(hi, hi, q1);
}
// A lane's four fp32 values rounded to two bf16 pairs (what the statistics of the rounded output are taken from).
__device__ __forceinline__ i32x2 pack_bf16x4(f32x4 v) { return i32x2{(int)f2bf_pk(v[0], v[1]), (int)f2bf_pk(v[2], v[3])}; }
// v_permlane16_swap trades lane rows 1 <-> 0 and 3 <-> 2 between the packed registers of two sixteen-channel blocks a and b: from
// (block a: channels 4 lg .. + 3, block b: the same) a lane ends up with EIGHT consecutive channels -- rows 0 / 2 block a's channels
// 0-7 / 8-15, rows 1 / 3 block b's -- and stores 16 bytes instead of two 8-byte pieces 32 bytes apart.  With a = block np, b = block np + 1
// the lane's run starts at channel  c8 = (np + (lg & 1)) * 16 + (lg >> 1) * 8.  conv_pw / conv3x3a / conv3x3s / the stem kernels.
__device__ __forceinline__ i32x4 swap8(i32x2 pa, i32x2 pb) {
    const auto sx = __builtin_amdgcn_permlane16_swap((unsigned)pa.x, (unsigned)pb.x, false, false);
    const auto sy = __builtin_amdgcn_permlane16_swap((unsigned)pa.y, (unsigned)pb.y, false, false);
    return i32x4{(int)sx[0], (int)sy[0], (int)sx[1], (int)sy[1]};
}
__device__ __forceinline__ i32x4 pack_swap8(f32x4 va, f32x4 vb) { return swap8(pack_bf16x4(va), pack_bf16x4(vb)); }

// The replica flush behind the row sums: scratch [4 waves][2][NT * 16] in LDS holds every wave's row sums (lane 0 of each DPP row wrote
// them; the caller's barrier lies between).  The four partials are ALWAYS added (w0 + w1) + (w2 + w3) -- the order the kernels and the
// tests' oracles agree on --, then one atomic per channel into replica rep of dst [BN_NCOPY][2][Ctot]: channel cbase + n0 + c for
// n0 + c < climit.  t = threadIdx.x.  No barrier inside: the callers' differ.  conv3x3 / conv3x3s (conv_fast.hip keeps the same sum on its
// static array, conv_pw.hip sums the nsub waves of a group).  The first half -- row_sum16 of s1 / s2[nt][r], lane 0 writes -- stays in
// each kernel: as a function taking the two arrays it changed the code of conv_pw, conv_fast and conv3x3s.
template <int NT>
__device__ __forceinline__ void scratch_to_replicas(const float* scratch, float* __restrict__ dst, int rep, int Ctot, int cbase, int n0, int climit, int t) {
    if (t < 2 * NT * 16) {
        const int which = t / (NT * 16), c = t - which * (NT * 16);
        const float v = (scratch[(0 * 2 + which) * (NT * 16) + c] + scratch[(1 * 2 + which) * (NT * 16) + c]) +
                        (scratch[(2 * 2 + which) * (NT * 16) + c] + scratch[(3 * 2 + which) * (NT * 16) + c]);
        if (n0 + c < climit) bn_acc_add(dst, rep, which, Ctot, cbase + n0 + c, v);
    }
}

// ---- the stem machinery: conv3x3a / conv_stem / conv_stem_dgrad (256 threads = 2 pixel halves x 2 K halves, 8 x NT accumulator tiles
// per wave in AGPRs behind inline-asm MFMAs, 64 output channels) ----------------------------------------------------------------------
// (The K-half exchange through LDS stays written out in each of the three: as a function taking the AGPR accumulator array it cost
// conv3x3a a VGPR and an AGPR and changed conv_stem_dgrad's code.)
// BatchNorm-backward sums of the BatchNorm that produced the convolution's input, on a lane's eight channels c8 .. c8 + 7 after swap8:
// q = the ROUNDED gradient, xq = that BatchNorm's input, yq = its output (the ReLU gate: positive = passed); sMean = [2][64] mean, invstd
// in LDS.  s1row += g, s2row += g * (x - mean) * invstd with g = yv > 0 ? gv : 0.  conv3x3a (which decodes its byte mask into yq first)
// and conv_stem_dgrad.
__device__ __forceinline__ void bn_bwd_sums8(const i32x4& q, const i32x4& xq, const i32x4& yq, const float* sMean, int c8, float (&s1row)[8], float (&s2row)[8]) {
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(sMean + c8), m1 = *reinterpret_cast<const f32x4*>(sMean + c8 + 4);
    const f32x4 i0 = *reinterpret_cast<const f32x4*>(sMean + 64 + c8), i1 = *reinterpret_cast<const f32x4*>(sMean + 64 + c8 + 4);
    const float mean[8] = {m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2], m1[3]};
    const float invs[8] = {i0[0], i0[1], i0[2], i0[3], i1[0], i1[1], i1[2], i1[3]};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned gw = (unsigned)q[k >> 1], xw = (unsigned)xq[k >> 1], yw = (unsigned)yq[k >> 1];
        const float gv0 = (k & 1) ? __uint_as_float(gw & 0xffff0000u) : __uint_as_float(gw << 16);
        const float xv = (k & 1) ? __uint_as_float(xw & 0xffff0000u) : __uint_as_float(xw << 16);
        const float yv = (k & 1) ? __uint_as_float(yw & 0xffff0000u) : __uint_as_float(yw << 16);
        const float gv = yv > 0.f ? gv0 : 0.f;
        s1row[k] += gv;
        s2row[k] += gv * (xv - mean[k]) * invs[k];
    }
}
// A tile's statistics s1 / s2[nt][r] (channels nt * 16 + lg * 4 + r) -> the 16 pixel lanes (DPP) -> this wave's own copy of the
// workgroup's accumulators sAcc [wave][2][64] in LDS (a copy per wave: the order of LDS atomics is not fixed).  conv3x3a / conv_stem.
template <int NT>
__device__ __forceinline__ void acc_tile_sums(float* sAcc, int wave, int li, int lg, float (*s1)[4], float (*s2)[4]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = row_sum16(s1[nt][r]), bq = row_sum16(s2[nt][r]);
            if (li == 0) { sAcc[wave * 128 + nt * 16 + lg * 4 + r] += a; sAcc[wave * 128 + 64 + nt * 16 + lg * 4 + r] += bq; }
        }
}
// sAcc [4 waves][2][64], behind a __syncthreads() of the caller: (w0 + w1) + (w2 + w3), one atomic per channel into replica rep of
// dst [BN_NCOPY][2][Ctot].  The three kernels' only way out for statistics.
__device__ __forceinline__ void acc_to_replicas64(const float* sAcc, float* dst, int rep, int Ctot, int t) {
    if (t < 128) {
        const int which = t >> 6, c = t & 63;
        bn_acc_add(dst, rep, which, Ctot, c, (sAcc[t] + sAcc[128 + t]) + (sAcc[256 + t] + sAcc[384 + t]));
    }
}
// Every inline-asm load into the weight ring A[D][4] has landed (s_waitcnt vmcnt(0) with the ring as "+v" operands: the compiler knows
// nothing of loads in flight and would hand their registers on).  Before a publishing barrier, and behind a tile's / the last refills.
template <int D>
__device__ __forceinline__ void ring_wait_all(bf16x8 (&A)[D][4]) {
#pragma unroll
    for (int d = 0; d < D; ++d) asm volatile("s_waitcnt vmcnt(0)" : "+v"(A[d][0]), "+v"(A[d][1]), "+v"(A[d][2]), "+v"(A[d][3]));
}

}  // namespace danet_conv
