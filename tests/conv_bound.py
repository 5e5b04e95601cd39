"""The rounding bound the convolution-epilogue tests check against (tests/test_gpu_infer.py, tests/test_gpu_infer_layers.py,
tests/test_infer_fold.py) and, with reference_dgrad / reference_wgrad / int_operands, the backward-pass tests
(tests/test_gpu_conv_grad.py, tests/test_conv_bound_host.py).  Not a test module: a helper they import.

A launch computes y = round(relu(acc + b[c] + res)) with acc = conv(x, Wq) accumulated in fp32 over exact products of its operands and
round() the output type's round-to-nearest.  With r the same expression evaluated in fp64 on the same operands (`reference`),

    |y - r| <= u * |r|  +  c * 2^-24 * sqrt(K) * S          (elementwise)

where u bounds the relative error of the output rounding (2^-8 for bf16: half an ulp is at most 2^-8 of the value), K = Cin per group
* R * S_kernel is the length of the dot product and S = conv(|x|, |Wq|) + |b| + |res| the scale its fp32 roundings are relative to.
A launch that rounds the convolution before a separate sum / ReLU kernel adds u * |r_conv| (r_conv: the reference before the residual
and the ReLU).

The per-channel check looks for what rounding cannot explain.  It compares y with the reference rounded the way the launch rounds
(`rounded`: once, or the convolution first and then the sum), so that only the accumulation error is left, which flips a result to its
neighbour now and then in either direction.  The signed mean of y - rounded(r) per output channel must stay within MEAN_FACTOR times
u * mean|r| / sqrt(n) (plus u * mean|r_conv| / sqrt(n) for two roundings) plus the accumulation term's mean.  That is the check that
sees a bias applied to the wrong channel or an addend dropped on a few tiles where |r| is large enough to hide them elementwise.  (The
unrounded r will not do for it: where the addend dominates -- a deep residual stream -- y rounds back onto the addend's own bf16 grid,
and y - r is then minus the convolution's contribution, a per-channel bias, not noise.)"""
import collections
import math

import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -22
C_ACC = 8.0
MEAN_FACTOR = 4.0

Reference = collections.namedtuple('Reference', 'r r_conv S K res relu')
_ROUNDED_TYPE = {U_BF16: torch.bfloat16, U_F32: torch.float32}


def reference(x, w, b=None, res=None, relu=False, stride=1, pad=0, dil=1, groups=1, transposed=False, outpad=0):
    """fp64 [relu](conv(x, w) + b + res) on the operands as given (cast them to what the kernel consumed first), with the
    accumulation scale S and the dot-product length K.  w: [Cout, Cin/groups, R, S] (conv) or [Cin, Cout, R, S] (transposed)."""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    if transposed:
        fn = lambda a, ww, bb: F.conv_transpose2d(a, ww, bb, stride, pad, outpad, 1, dil)
        K = w.shape[0] * w.shape[2] * w.shape[3]
    else:
        fn = lambda a, ww, bb: F.conv2d(a, ww, bb, stride, pad, dil, groups)
        K = w.shape[1] * w.shape[2] * w.shape[3]
    r_conv = fn(x, w, b)
    S = fn(x.abs(), w.abs(), None if b is None else b.abs())
    r = r_conv
    if res is not None:
        res = res.double()
        r = r + res
        S = S + res.abs()
    if relu:
        r = F.relu(r)
    return Reference(r, r_conv, S, K, res, bool(relu))


def reference_dgrad(x_shape, w, gy, stride=1, pad=0, dil=1, groups=1, addend=None):
    """The backward pass's data gradient (tests/test_gpu_conv_grad.py): fp64 d conv2d(x, w) / dx applied to gy, plus `addend` (the
    residual branch's gradient, fused into the epilogue), on the operands as given.  w: the forward weight [Cout, Cin/groups, R, S],
    gy [B, Cout, OH, OW], x_shape = (B, Cin, H, W).  K = Cout/groups * R * S bounds the dot-product length from above: at stride s an
    input pixel meets only the taps of its parity class, about K / s^2 of them, so the accumulation term -- the small one -- is up to
    s times too generous, never too tight."""
    w, gy = w.double(), gy.double()
    fn = lambda ww, gg: torch.nn.grad.conv2d_input(tuple(x_shape), ww, gg, stride, pad, dil, groups)
    r_conv = fn(w, gy)
    S = fn(w.abs(), gy.abs())
    K = w.shape[0] // groups * w.shape[2] * w.shape[3]
    r = r_conv
    if addend is not None:
        addend = addend.double()
        r = r + addend
        S = S + addend.abs()
    return Reference(r, r_conv, S, K, addend, False)


def reference_wgrad(x, gy, w_shape, stride=1, pad=0, dil=1, groups=1):
    """The weight gradient: fp64 d conv2d(x, w) / dw applied to gy, [Cout, Cin/groups, R, S] (for `ratios` its "channels" are dim 1,
    the input channels of a group); K = B * OH * OW, the pixels every element sums over."""
    x, gy = x.double(), gy.double()
    fn = lambda xx, gg: torch.nn.grad.conv2d_weight(xx, tuple(w_shape), gg, stride, pad, dil, groups)
    r = fn(x, gy)
    S = fn(x.abs(), gy.abs())
    return Reference(r, r, S, gy.shape[0] * gy.shape[2] * gy.shape[3], None, False)


def int_operands(shape, lo, hi, generator):
    """Integers of [lo, hi] as an fp32 tensor; |values| <= 256, so each one is a bf16 number (8 significant bits) and sums of products
    of such operands are exact in fp32, in any order, as long as they stay below 2^24."""
    if not -256 <= lo <= hi <= 256:
        raise ValueError('int_operands: [%d, %d] is not exactly representable in bf16' % (lo, hi))
    t = torch.randint(lo, hi + 1, tuple(shape), generator=generator).float()
    assert torch.equal(t.bfloat16().float(), t)
    return t


def rounded(ref, u, rounded_conv=False):
    """The reference rounded as the launch rounds its result (u = U_BF16: to bf16, U_F32: to fp32): once, or (rounded_conv) the
    convolution on its own and then the sum / ReLU."""
    dt = _ROUNDED_TYPE[u]
    if not rounded_conv:
        return ref.r.to(dt).double()
    z = ref.r_conv.to(dt).double()
    if ref.res is not None:
        z = z + ref.res
    if ref.relu:
        z = F.relu(z)
    return z.to(dt).double()


def bound(ref, u, rounded_conv=False, c=C_ACC):
    """(elementwise bound, its accumulation term) for a result rounded once (rounded_conv: twice, the convolution on its own first)."""
    acc = (c * 2.0 ** -24 * math.sqrt(ref.K)) * ref.S
    b = u * ref.r.abs() + acc
    if rounded_conv:
        b = b + u * ref.r_conv.abs()
    return b, acc


def ratios(y, ref, u, rounded_conv=False, c=C_ACC, mean_factor=MEAN_FACTOR):
    """(worst |y - r| / bound, worst per-channel |mean(y - rounded(r))| / (mean_factor * its scale)): both <= 1 when y is right.  y [B, C, H, W]
    in any float type, ref = reference(...) of the same shape."""
    if tuple(y.shape) != tuple(ref.r.shape):
        raise ValueError('shape %s != reference %s' % (tuple(y.shape), tuple(ref.r.shape)))
    d = y.double() - ref.r
    bnd, acc = bound(ref, u, rounded_conv, c)
    if not torch.isfinite(d).all():
        return math.inf, math.inf
    over = d.abs() / bnd.clamp_min(1e-300)
    elem = over.max().item()
    dims = (0, 2, 3)
    n = d.numel() // d.shape[1]
    scale = u * ref.r.abs().mean(dims) / math.sqrt(n) + acc.mean(dims)
    if rounded_conv:
        scale = scale + u * ref.r_conv.abs().mean(dims) / math.sqrt(n)
    dm = (y.double() - rounded(ref, u, rounded_conv)).mean(dims)
    mean = (dm.abs() / (mean_factor * scale).clamp_min(1e-300)).max().item()
    return elem, mean


def check(y, ref, u, what, rounded_conv=False, c=C_ACC, mean_factor=MEAN_FACTOR):
    """ratios(...) asserted <= 1; returns them for record()."""
    elem, mean = ratios(y, ref, u, rounded_conv, c, mean_factor)
    assert elem <= 1.0 and mean <= 1.0, (what, {'elem': elem, 'chan_mean': mean})
    return elem, mean
