"""Float64 restatements of csrc/norm_act.hip -- BatchNorm (+ residual) (+ ReLU) forward / backward, the per-channel sum and the
HRNet fuse sum with its window-sum gradients --, the rounding bounds of the kernels' arithmetic, the launch geometry of make_map
and of the one-pass planner restated in Python, and the case tables of tests/test_gpu_norm_oracle.py.  numpy only: no torch, no
GPU, nothing of the package under test.  tests/test_norm_oracle_host.py checks all of it on the CPU.

Every function takes float64 arrays whose LAST axis is the channel (NHWC; the BatchNorm functions flatten the rest to M rows)
and that hold exactly the values of the device tensor (bf16: rounded first, round_bf16).

Bounds.  u = 2^-24 is the unit roundoff of fp32, first order in u throughout (k u < 2^-17 for every k below).  A channel's n = M
values are summed in three stages (bn_stats_kernel, bn_bwd_reduce, channel_sum_kernel, the one-pass kernel):
  1. every lane adds the k1 = ceil(M / rstep) rows it walks, one after the other, in fp32     (k1 - 1 roundings)
  2. block_channel_reduce adds the k2 = span / CV lanes of a channel vector in a fixed order  (k2 - 1 roundings)
  3. the workgroups' partial sums are added as doubles (exact to 2^-53), reduce_replicas rounds the total to fp32 once,
     and the consumer multiplies by the rounded 1.0f / M                                      (3 roundings)
so a sum of terms t_i divided by M is within k u mean|t_i| of the exact one, k = k1 + k2 + 2 (one unit to spare).
  mean, bf16     |mean_k - mean| <= dm = k u mean|x|
  var, bf16      the kernel forms max(E2 - mean^2, 0) with E2 = sum x^2 / M (the squares of bf16 values are exact in fp32):
                 k u E2 for the sum, 2 |mean| dm + dm^2 + u mean^2 for the rounded square of the kernel's mean, u (E2 + mean^2)
                 for the subtraction:       dvar = u ((k + 1) E2 + 2 mean^2) + 2 |mean| dm + dm^2
                 -- relative to E[x^2], NOT to var: a channel whose mean is 16 times its spread loses 2^8 of it.
  mean/var, fp32 the fp32 build sums d = x - x[row 0] (one rounding each: u |d|; d d has 3 u): with d in the place of x
                 dmd = (k + 1) u mean|d|,  dm = dmd + u |mean| (the addition of x[row 0]),
                 dvar = u ((k + 4) E[d^2] + 2 mean(d)^2) + 2 |mean(d)| dmd + dmd^2
  invstd         a = var + eps is rounded once more: relative error rho = dvar / a + u; (1 - rho)^-1/2 - 1 >= rho / 2 is carried
                 exactly (rho capped at 1/2).  The root itself: bf16 build rsqrtf, ASSUMED accurate to RSQRT_ULPS = 2 units in
                 the last place = 4 u relative (the ROCm device-library documentation is not at hand; the published HIP math table
                 says 1); fp32 build 1.0f / sqrtf, both correctly rounded (hipcc's default): 2 u.
  y              sc = invstd gamma: dsc = |gamma| dinv + u |sc|.  sh = fma(-mean, sc, beta) and v = fma(x, sc, sh) use the SAME
                 sc, so v = (x - mean_k) sc_k + beta up to the two fma roundings:
                     |v_k - v| <= |x - mean| dsc + (|sc| + dsc) dm + u |sh| + u (|x sc| + |sh|)   [+ u |v| for `+ res`]
                 bf16: + 2^-8 |ref| for the one round-to-nearest-even of f2bf_pk (half a unit in the last of 8 significant
                 bits; truncation would need 2^-7: not admitted.  2^-8 of the fp32 error itself is left to the spare unit of k).
                 ReLU needs no exclusion: |relu(a) - relu(b)| <= |a - b|.
  running        rm' = (1 - mom) rm + mom mean: mom dm + u (3 |(1 - mom) rm| + 2 |mom mean|) (1 - mom, the product, the sum; the
                 product, the sum); rv' likewise with mom var unbias, unbias = M / (M - 1) rounded: 4 roundings on that term.
  backward       with the kernel's OWN saved mean / invstd as inputs (saved is checked separately) and g = dy gate,
                 xhat = (x - mean) invstd (3 roundings per product g xhat):
                     |dbeta_k - dbeta| <= k u sum|g|,           |dgamma_k - dgamma| <= (k + 3) u sum|g xhat|
                     dm1 = (k + 2) u mean|g|,  dm2 = (k + 5) u mean|g xhat|     (m1 = dbeta / M, m2 = dgamma / M)
                     |dx_k - dx| <= |k0| (dm1 + |xhat| dm2 + u (|A| + 3 |B| + |A - B|)) + 2 u |dx|     [bf16: + 2^-8 |dx|]
                 with k0 = gamma invstd, A = g - m1, B = xhat m2.  dres = g is stored as it is: exact.
  fuse sum       n terms added in fp32: (n - 1) u sum|terms| [+ 2^-8 |ref|]; a 2^s x 2^s window sum: at most 4^s - 1 roundings
                 (the per-shift kernel adds in a row; the all-shifts kernel in a tree of depth 3 per level, which is fewer).
Integer-valued inputs whose partial sums stay below 2^24 make every one of these sums exact: see exact_sum_ok."""
import collections

import numpy as np

U = 2.0 ** -24
UB = 2.0 ** -8
RSQRT_ULPS = 2.0                    # assumed (see above)
VW, UNR, SLAB, NCOPY = 4, 4, 1024, 32
BLOCK_BYTES = 24576                 # danet_bn_set_block_bytes default
OP_ROWS, OP_ROWS_BIG, OP_NV, OP_NV_BIG, OP_MAX_BLOCKS = 25, 29, 10, 14, 512
ES = {'bf16': 2, 'fp32': 4}


class Obj(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def round_bf16(a):
    """Round-to-nearest-even to bf16, returned as float64."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7fff)
    return ((b + r) & np.uint64(0xffff0000)).astype(np.uint32).view(np.float32).astype(np.float64)


def as_dtype(a, dtype_name):
    """The float64 values an fp32 / bf16 device tensor made from `a` holds."""
    return round_bf16(a) if dtype_name == 'bf16' else np.asarray(a, dtype=np.float32).astype(np.float64)


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, a.shape[-1])


def _vec(p, C, fill):
    return np.full(C, fill, dtype=np.float64) if p is None else np.asarray(p, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ the operations
def _apply(x, res, gamma, beta, mean, var, eps, relu):
    C = x.shape[-1]
    invstd = 1.0 / np.sqrt(var + eps)
    v = (x - mean) * (invstd * _vec(gamma, C, 1.0)) + _vec(beta, C, 0.0)
    if res is not None:
        v = v + np.asarray(res, dtype=np.float64)
    return Obj(v=v, y=np.maximum(v, 0.0) if relu else v, mean=mean, var=var, invstd=invstd)


def bn_forward(x, res, gamma, beta, eps, relu):
    """Training mode -> v (before the ReLU), y, mean, var (biased), invstd."""
    x = np.asarray(x, dtype=np.float64)
    x2 = _rows(x)
    mean = x2.mean(0)
    var = ((x2 - mean) ** 2).mean(0)
    return _apply(x, res, gamma, beta, mean, var, float(eps), relu)


def bn_eval(x, res, gamma, beta, rm, rv, eps, relu):
    return _apply(np.asarray(x, dtype=np.float64), res, gamma, beta, np.asarray(rm, np.float64), np.asarray(rv, np.float64), float(eps), relu)


def running_update(rm, rv, mean, var, M, momentum):
    unb = M / (M - 1.0) if M > 1 else 1.0
    return (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * var * unb


def bn_backward(dy, x, gate, gamma, mean, invstd):
    """-> dx, dres, dbeta, dgamma; gate (bool), mean and invstd are inputs (the kernel's own, in the GPU tests)."""
    dy = np.asarray(dy, dtype=np.float64)
    g = dy * np.asarray(gate, dtype=np.float64)
    xhat = (np.asarray(x, np.float64) - mean) * invstd
    g2, h2 = _rows(g), _rows(xhat)
    M = g2.shape[0]
    dbeta, dgamma = g2.sum(0), (g2 * h2).sum(0)
    dx = _vec(gamma, dy.shape[-1], 1.0) * invstd * (g - dbeta / M - xhat * (dgamma / M))
    return Obj(dx=dx, dres=g, dbeta=dbeta, dgamma=dgamma, xhat=xhat, g=g)


def channel_sum(x):
    return _rows(x).sum(0)


def upsample(t, s, H, W):
    return t[:, np.arange(H) >> s][:, :, np.arange(W) >> s]


def fuse_sum(terms, shifts, relu):
    """terms[i]: [B, H >> s_i, W >> s_i, C] -> v, y of [B, H, W, C]: nearest upsampling as the index arithmetic h >> s, w >> s."""
    B, Ht, Wt, C = terms[0].shape
    H, W = Ht << shifts[0], Wt << shifts[0]
    v = np.zeros((B, H, W, C))
    for t, s in zip(terms, shifts):
        assert t.shape == (B, H >> s, W >> s, C)
        v = v + upsample(np.asarray(t, np.float64), s, H, W)
    return Obj(v=v, y=np.maximum(v, 0.0) if relu else v)


def window_sum(g, s):
    B, H, W, C = g.shape
    f = 1 << s
    return g.reshape(B, H >> s, f, W >> s, f, C).sum(axis=(2, 4))


def fuse_sum_backward(gy, y_gate, shifts_wanted):
    """{s: [B, H >> s, W >> s, C] window sums of gy * gate}."""
    g = np.asarray(gy, np.float64) * np.asarray(y_gate, np.float64)
    return {s: window_sum(g, s) for s in shifts_wanted}


def mask_bytes(v):
    """The ReLU byte mask of ldmask / stmask: byte i covers the flat elements 4i .. 4i + 3, bit j = element 4i + j positive."""
    b = (np.asarray(v).reshape(-1, VW) > 0).astype(np.uint8)
    return (b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- launch geometry
def ceil_div(a, b):
    return -(-a // b)


def slabs(C):
    return [(c0, min(SLAB, C - c0)) for c0 in range(0, C, SLAB)]


def wide_slabs(C):
    return C // SLAB if (C > SLAB and C % SLAB == 0 and C // SLAB <= 12) else 1


def bn_ncopy(C):
    return max((32 if C <= 64 else 16 if C <= 128 else 8 if C <= 256 else 4) // 2, 4)


def slab_plan(M, Cs, es, block_bytes=None, cap=1024):
    """make_map for one slab of Cs channels (the workgroup count does not depend on the full width)."""
    block_bytes = block_bytes or BLOCK_BYTES
    CV = Cs // VW
    span = (256 // CV) * CV
    rpb = span // CV
    blocks = max(1, min(ceil_div(M * CV, span), ceil_div(M * Cs * es, block_bytes), 1024, cap))
    rstep = span * blocks // CV
    return Obj(Cs=Cs, CV=CV, span=span, rpb=rpb, idle=256 - span, blocks=blocks, rstep=rstep, k1=ceil_div(M, rstep), k2=rpb)


def plan(M, C, dtype_name, block_bytes=None, cap=1024):
    return [slab_plan(M, Cs, ES[dtype_name], block_bytes, cap) for _, Cs in slabs(C)]


def k_of(plans, k1=None):
    """Per channel: k = k1 + k2 + 2 of the slab it lies in (k1: the rows per lane of another launch form, if given)."""
    return np.concatenate([np.full(p.Cs, (p.k1 if k1 is None else k1) + p.k2 + 2.0) for p in plans])


def onepass_plan(M, C, budget=0, device_blocks=OP_MAX_BLOCKS):
    """onepass_plan of ONE job -> None (two kernels) or (rows per lane the instantiation holds, workgroups per slab)."""
    if not (C <= SLAB or wide_slabs(C) > 1):
        return None
    max_blocks = min(budget, device_blocks) if budget > 0 else device_blocks

    def rows_plan(rows):
        launches, used, per = 0, None, []
        for _ in range(wide_slabs(C)):
            rpb = slab_plan(M, min(C, SLAB), 2).rpb
            blocks = max(1, ceil_div(M, rpb * rows))
            if blocks > max_blocks:
                return 0, per
            if used is None or used + blocks > max_blocks:
                launches, used = launches + 1, 0
            used += blocks
            per.append(blocks)
        return launches, per
    (ns, ps), (nb, pb) = rows_plan(OP_ROWS), rows_plan(OP_ROWS_BIG)
    if ns > 0 and (nb == 0 or ns <= nb):
        return OP_ROWS, ps
    return (OP_ROWS_BIG, pb) if nb > 0 else None


def onepass_k1(M, C, budget=0):
    """Rows a lane of the one-pass launch walks (None: the launch does not qualify)."""
    p = onepass_plan(M, C, budget)
    if p is None:
        return None
    return ceil_div(M, slab_plan(M, min(C, SLAB), 2).rpb * p[1][0])


# ---------------------------------------------------------------------------------------------------------------- bounds
def stats_bound(x, dtype_name, k):
    """-> dm, dvar per channel (see the module docstring)."""
    x2 = _rows(x)
    if dtype_name == 'bf16':
        mabs, md, e2 = np.abs(x2).mean(0), x2.mean(0), (x2 * x2).mean(0)
        dm = k * U * mabs
        return dm, U * ((k + 1) * e2 + 2 * md * md) + 2 * np.abs(md) * dm + dm * dm
    d = x2 - x2[0]
    mabs, md, e2 = np.abs(d).mean(0), d.mean(0), (d * d).mean(0)
    dmd = (k + 1) * U * mabs
    return dmd + U * np.abs(x2.mean(0)), U * ((k + 4) * e2 + 2 * md * md) + 2 * np.abs(md) * dmd + dmd * dmd


def invstd_bound(var, eps, dvar, dtype_name):
    a = var + eps
    rho = np.minimum(dvar / a + U, 0.5)
    half = 1.0 / np.sqrt(1.0 - rho) - 1.0
    fn = 2.0 * RSQRT_ULPS * U if dtype_name == 'bf16' else 2.0 * U
    return (half + fn + half * fn) / np.sqrt(a)


def forward_bound(x, res, gamma, beta, o, dm, dinv, dtype_name):
    """|y_kernel - o.y| elementwise; also the bound on the value the ReLU gate is taken from (without the bf16 term: fp32_only)."""
    C = x.shape[-1]
    g, b = _vec(gamma, C, 1.0), _vec(beta, C, 0.0)
    sc = o.invstd * g
    sh = b - o.mean * sc
    dsc = np.abs(g) * dinv + U * np.abs(sc)
    e = np.abs(x - o.mean) * dsc + (np.abs(sc) + dsc) * dm + U * np.abs(sh) + U * (np.abs(x * sc) + np.abs(sh))
    if res is not None:
        e = e + U * np.abs(o.v)
    if dtype_name == 'bf16':
        e = e + UB * np.abs(o.y)
    return e


def running_bound(rm, rv, mean, var, M, momentum, dm, dvar):
    unb = M / (M - 1.0) if M > 1 else 1.0
    brm = momentum * dm + U * (3 * np.abs((1 - momentum) * rm) + 2 * np.abs(momentum * mean))
    brv = momentum * unb * dvar + U * (3 * np.abs((1 - momentum) * rv) + 4 * np.abs(momentum * var * unb))
    return brm, brv


def backward_bound(gamma, invstd, bw, k, dtype_name):
    """-> bounds on dx (elementwise), dbeta, dgamma (per channel); bw = bn_backward(...) with the kernel's saved statistics."""
    g2, h2 = _rows(bw.g), _rows(bw.xhat)
    M, C = g2.shape
    s1, s2 = np.abs(g2).sum(0), np.abs(g2 * h2).sum(0)
    dm1, dm2 = (k + 2) * U * s1 / M, (k + 5) * U * s2 / M
    k0 = _vec(gamma, C, 1.0) * invstd
    A, B = bw.g - bw.dbeta / M, bw.xhat * (bw.dgamma / M)
    e = np.abs(k0) * (dm1 + np.abs(bw.xhat) * dm2 + U * (np.abs(A) + 3 * np.abs(B) + np.abs(A - B))) + 2 * U * np.abs(bw.dx)
    if dtype_name == 'bf16':
        e = e + UB * np.abs(bw.dx)
    return Obj(dx=e, dbeta=k * U * s1, dgamma=(k + 3) * U * s2)


def channel_sum_bound(x, k1, k2):
    return (k1 + k2) * U * np.abs(_rows(x)).sum(0)


def fuse_forward_bound(terms, shifts, o, dtype_name):
    B, H, W, C = o.v.shape
    e = (len(terms) - 1) * U * sum(upsample(np.abs(t), s, H, W) for t, s in zip(terms, shifts))
    return e + UB * np.abs(o.y) if dtype_name == 'bf16' else e


def fuse_backward_bound(gy, y_gate, ref, dtype_name):
    a = np.abs(np.asarray(gy, np.float64) * np.asarray(y_gate, np.float64))
    return {s: (4 ** s - 1) * U * window_sum(a, s) + (UB * np.abs(r) if dtype_name == 'bf16' else 0.0) for s, r in ref.items()}


def exact_sum_ok(values):
    """Every partial sum of these integer values, in whatever order, is an integer below 2^24: exact in fp32."""
    v = _rows(values)
    return bool((v == np.rint(v)).all()) and float(np.abs(v).sum(0).max()) < 2.0 ** 24


def ratio(err, bound):
    """max err / bound; where the bound is zero the error must be zero."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    z = bound == 0
    if z.any() and np.asarray(err)[z].any():
        return float('inf')
    return float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0


# ------------------------------------------------------------------------------------------------------------ case tables
EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.1))
BnCase = collections.namedtuple('BnCase', 'name C M knob why expect')     # expect: per slab (Cs, span, rpb, workgroups, rows per lane)

BN_CASES = [
    BnCase('c4_m2', 4, 2, None, 'one channel vector, rpb 256 > M: less than one trip of UNR rows, lanes M.. past the end', [(4, 256, 256, 1, 1)]),
    BnCase('c4_m3', 4, 3, None, 'as c4_m2, odd M', [(4, 256, 256, 1, 1)]),
    BnCase('c4_m5', 4, 5, None, 'as c4_m2, M one more than UNR', [(4, 256, 256, 1, 1)]),
    BnCase('c12_m85', 12, 85, None, 'span 255 (lane 255 idle), rpb 85: exactly one step of rows', [(12, 255, 85, 1, 1)]),
    BnCase('c12_m86', 12, 86, None, 'one row more than a step: lane 0..2 walk two rows', [(12, 255, 85, 1, 2)]),
    BnCase('c12_m341', 12, 341, None, 'one row more than a full trip of UNR = 4 steps: a second trip', [(12, 255, 85, 1, 5)]),
    BnCase('c40_m51', 40, 51, None, 'span 250: six idle lanes', [(40, 250, 25, 1, 3)]),
    BnCase('c1024_m5', 1024, 5, None, 'CV 256, rpb 1', [(1024, 256, 1, 1, 5)]),
    BnCase('c1028_m6', 1028, 6, None, 'slab loop 1024 + 4: neither wide nor one-pass', [(1024, 256, 1, 1, 6), (4, 256, 256, 1, 1)]),
    BnCase('c1536_m4', 1536, 4, None, 'slabs 1024 + 512', [(1024, 256, 1, 1, 4), (512, 256, 2, 1, 2)]),
    BnCase('c2048_m8', 2048, 8, None, 'wide_slabs 2: the multi-kernel launch forward and backward', [(1024, 256, 1, 1, 8)] * 2),
    BnCase('c3072_m8', 3072, 8, None, 'wide_slabs 3', [(1024, 256, 1, 1, 8)] * 3),
    BnCase('c2052_m4', 2052, 4, None, 'slab loop 1024 + 1024 + 4 (not a whole number of slabs: not wide)', [(1024, 256, 1, 1, 4)] * 2 + [(4, 256, 256, 1, 1)]),
    BnCase('c48_m700_k512', 48, 700, 512, 'block bytes 512: 34 workgroups, more than the bn_ncopy(48) = 16 replicas', [(48, 252, 21, 34, 1)]),
    BnCase('c48_cap_k64', 48, 1024 * 21 + 5, 64, 'block bytes 64: the 1024-workgroup cap binds, rstep from the cap, the first lanes walk two rows',
           [(48, 252, 21, 1024, 2)]),
]
BN_BY_NAME = {c.name: c for c in BN_CASES}
WIDE = {'c2048_m8': 2, 'c3072_m8': 3}
# fp32: 8 rows of a 1024-channel slab are 32 KB > BLOCK_BYTES: two workgroups of four rows
EXPECT_FP32 = {'c2048_m8': [(1024, 256, 1, 2, 4)] * 2, 'c3072_m8': [(1024, 256, 1, 2, 4)] * 3}

OFFSET_CASE = ('c12_m512_offset', 12, 512)       # M a power of two: the constant channel's statistics are exact

# channel_sum: (name, C, M, knob, ncopy, workgroups, rows per lane)
CHSUM_CASES = [('c4_m5', 4, 5, None, 1, 1, 1), ('c12_m341', 12, 341, None, 1, 1, 5), ('c40_m51', 40, 51, None, 4, 1, 3),
               ('c1028_m6', 1028, 6, None, 1, 1, 6), ('c48_cap_ncopy1', 48, 1024 * 21 + 5, 64, 1, 256, 5), ('c48_cap_ncopy16', 48, 1024 * 21 + 5, 64, 16, 1024, 2)]

# integer-exact BatchNorm: M a power of two (the mean is exact)
INT_CASES = [('c4_m2', 4, 2, None), ('c12_m512', 12, 512, None), ('c48_m1024_k512', 48, 1024, 512), ('c1028_m8', 1028, 8, None), ('c2048_m8', 2048, 8, None)]
INT_X, INT_DY = 8, 8               # |x| <= 8, |dy| <= 8

# one-pass backward (bf16, C = 48: rpb 21): (M, budget, rows of the instantiation or None = two kernels, workgroups, rows per lane, why)
ONEPASS_CASES = [(210, 0, 25, 1, 10, 'registers only'), (211, 0, 25, 1, 11, 'first LDS row'), (525, 0, 25, 1, 25, 'all 25 rows'),
                 (526, 0, 25, 2, 13, 'second workgroup'), (526, 1, 29, 1, 26, 'budget 1: the 29-row instantiation'),
                 (609, 1, 29, 1, 29, 'budget 1: all 29 rows'), (610, 1, None, 0, 0, 'budget 1: does not qualify, two kernels')]
ONEPASS_WIDE = [(2048, 8), (3072, 8)]
MULTI_BN = [(48, 526), (12, 341), (40, 51), (4, 5)]

FuseCase = collections.namedtuple('FuseCase', 'name B H W C shifts wanted')
FUSE_CASES = [
    FuseCase('c4_8x24_1t', 1, 8, 24, 4, (0,), [(0,)]),
    FuseCase('c12_16x8_b3_2t', 3, 16, 8, 12, (0, 1), [(0, 1), (1,)]),
    FuseCase('c12_8x24_b3_3t', 3, 8, 24, 12, (0, 1, 2), [(0, 1, 2), (0, 2), (2,)]),
    FuseCase('c4_16x8_rep', 1, 16, 8, 4, (0, 0, 1, 2), [(0, 1, 2)]),
    FuseCase('c12_8x24_b3_4t', 3, 8, 24, 12, (0, 1, 2, 3), [(0, 1, 2, 3), (1, 3), (0,), (3,)]),
]
FUSE_BIG = FuseCase('c48_256x352', 1, 256, 352, 48, (0, 1), [(0,), (0, 1)])      # 4224 > 4096 workgroups: a second grid-stride trip
FUSE_BY_NAME = {c.name: c for c in FUSE_CASES + [FUSE_BIG]}
FUSE_MULTI = ['c12_8x24_b3_4t', 'c4_16x8_rep', 'c12_16x8_b3_2t', 'c4_8x24_1t']
FUSE_TERM, FUSE_GY = 4, 3          # |term| <= 4 (a sum of 4 is <= 16), |gy| <= 3 (a sum of 64 is <= 192 < 256: exact in bf16)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def ints(rs, shape, m):
    return rs.randint(-m, m + 1, size=shape).astype(np.float64)


def bn_inputs(C, M, name, dtype_name, use_res, kind='normal'):
    """The inputs of one BatchNorm case as the device holds them.  kind: 'normal'; 'offset': every channel's mean 16 times its
    spread, channel 1 constant; 'int': integer x.  dy is integer-valued everywhere (|dy| <= INT_DY), so dbeta is exact."""
    rs = np.random.RandomState(_seed(name))
    if kind == 'int':
        x = ints(rs, (M, C), INT_X)
    else:
        spread = 0.5 + rs.rand(C)
        x = rs.standard_normal((M, C)) * spread + (16.0 * spread if kind == 'offset' else 0.3 * rs.standard_normal(C))
        if kind == 'offset':
            x[:, 1] = 2.0
    res = rs.standard_normal((M, C)) if use_res else None
    return Obj(x=as_dtype(x, dtype_name), res=None if res is None else as_dtype(res, dtype_name), dy=ints(rs, (M, C), INT_DY),
               gamma=as_dtype(0.5 + rs.rand(C), 'fp32'), beta=as_dtype(0.3 * rs.standard_normal(C) + 0.05, 'fp32'),
               rm=as_dtype(0.1 * rs.standard_normal(C), 'fp32'), rv=as_dtype(0.5 + rs.rand(C), 'fp32'))


def fuse_inputs(case, dtype_name, integer=True):
    rs = np.random.RandomState(_seed(case.name))
    shp = lambda s: (case.B, case.H >> s, case.W >> s, case.C)
    if integer:
        return [ints(rs, shp(s), FUSE_TERM) for s in case.shifts], ints(rs, shp(0), FUSE_GY)
    return [as_dtype(rs.standard_normal(shp(s)), dtype_name) for s in case.shifts], as_dtype(rs.standard_normal(shp(0)), dtype_name)
