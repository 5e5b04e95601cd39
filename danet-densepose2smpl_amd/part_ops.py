"""Fused partial-IUV ("limb") element-wise path on HIP kernels (csrc/part_ops.hip).

`part_clean`  = part drop + iuvmap_clean of the 24 partial maps (/root/reference/models/danet/danet.py:264-283)
                producing directly the zero-padded 24-channel NHWC bf16 operand of the limb regressor's first conv.
`part_losses` = part_iuv_simp + affine_grid/grid_sample of the ground truth + body_uv_losses summed over the
                24 joints (/root/reference/models/danet/iuv_estimator.py:206-246), as three raw sums.
Both take the grouped conv's output [B, 24*21, H, W] (bf16, channels_last) as it is.
"""
import torch

from . import _lib
from ._lib import ptr, check, stream, f32c, require_gpu
from .conv import nhwc_bf16, nptr, _empty_nhwc, ARENA
from .glue import loss_finalize

NJ, NC = 24, 7


def _cpj(C):
    """channels per joint in memory: 21, or 24 for the grouped conv's zero-padded output"""
    if C not in (NJ * 21, NJ * 24):
        raise ValueError('partial IUV prediction must have %d or %d channels, got %d' % (NJ * 21, NJ * 24, C))
    return C // NJ


def padded_view6(pp):
    """[B, 24*24, H, W] group-padded prediction -> its [B,24,3,7,H,W] view (no copy); the padded tensor rides along
    as `._padded` so that part_clean / part_losses read it directly."""
    B, C, H, W = pp.shape
    v = pp.permute(0, 2, 3, 1).reshape(B, H, W, NJ, C // NJ)[..., :21].reshape(B, H, W, NJ, 3, NC).permute(0, 3, 4, 5, 1, 2)
    v._padded = pp
    return v


def _flat(pred):
    """The [B, 24*21 | 24*24, H, W] prediction behind a [B,24,3,7,H,W] view: the group-padded tensor riding along as `._padded`, a
    reshape otherwise; a 4-D prediction as it is."""
    if pred.dim() == 6:
        B, J, T, K, H, W = pred.shape
        padded = getattr(pred, '_padded', None)
        pred = padded if padded is not None else pred.reshape(B, J * T * K, H, W)
    _cpj(pred.shape[1])
    return pred


def _gt_args(op, iuv_img, theta, sel, sample_w=None, BHW=None):
    """(iuv_img, theta, sample_w | None, sel) cast for the kernels and checked against (B, H, W) (None: the IUV image's own)."""
    img, th, w = f32c(iuv_img), f32c(theta), f32c(sample_w)
    sel = sel.to(torch.int32).contiguous()
    if BHW is None:
        B, _, H, W = img.shape
    else:
        B, H, W = BHW
    if img.shape != (B, 3, H, W) or th.shape != (B, NJ, 2, 3) or sel.shape != (NJ, 6):
        raise ValueError('%s: bad shapes %s %s %s' % (op, tuple(img.shape), tuple(th.shape), tuple(sel.shape)))
    return img, th, w, sel


# One function per C entry point of csrc/part_ops.hip.  pred, g24: bf16 channels_last; gt = _gt_args' (img, th, w, sel).

def _clean_fwd(pred, k):
    B, C, H, W = pred.shape
    x24 = _empty_nhwc(B * NJ, 24, H, W, torch.bfloat16, pred.device)
    check(_lib.lib().danet_part_clean_forward(nptr(pred), ptr(k), B, H, W, _cpj(C), nptr(x24), stream()), 'danet_part_clean_forward')
    return x24


def _clean_bwd(g24, pred, k):
    B, C, H, W = pred.shape
    gp = _empty_nhwc(B, C, H, W, torch.bfloat16, pred.device)
    check(_lib.lib().danet_part_clean_backward(nptr(g24), nptr(pred), ptr(k), B, H, W, _cpj(C), nptr(gp), stream()), 'danet_part_clean_backward')
    return gp


def _loss_fwd(pred, gt, align):
    B, C, H, W = pred.shape
    sums = ARENA.zeros(32 * 3 * 2, pred.device)              # [32][3] doubles: exact, order-independent adds of the workgroups' partial sums
    check(_lib.lib().danet_part_loss_forward(nptr(pred), *[ptr(t) for t in gt], B, H, W, align, _cpj(C), ptr(sums), stream()),
          'danet_part_loss_forward')
    return sums


def _loss_bwd(pred, gt, scale, align):
    B, C, H, W = pred.shape
    gp = _empty_nhwc(B, C, H, W, torch.bfloat16, pred.device)
    check(_lib.lib().danet_part_loss_backward(nptr(pred), *[ptr(t) for t in gt], ptr(scale), B, H, W, align, _cpj(C), nptr(gp), stream()),
          'danet_part_loss_backward')
    return gp


def _fused_bwd(pred, gt, scale, g24, k, align):
    B, C, H, W = pred.shape
    gp = _empty_nhwc(B, C, H, W, torch.bfloat16, pred.device)
    check(_lib.lib().danet_part_backward_fused(nptr(pred), *[ptr(t) for t in gt], ptr(scale), nptr(g24), ptr(k), B, H, W, align, _cpj(C),
                                               nptr(gp), stream()), 'danet_part_backward_fused')
    return gp


class PartCleanFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, keep):
        pred, k = nhwc_bf16(pred), f32c(keep)
        ctx.save_for_backward(pred, k)
        return _clean_fwd(pred, k)

    @staticmethod
    def backward(ctx, g24):
        pred, k = ctx.saved_tensors
        return _clean_bwd(nhwc_bf16(g24), pred, k), None


def part_clean(pred, keep=None):
    """pred [B,504,H,W] (or its [B,24,3,7,H,W] view), keep [B,24,7] or None ->
    (part_iuv_map [B,24,3,7,H,W] bf16 view, x24 [B*24,24,H,W] bf16 channels_last: channels 21..23 are zero)."""
    require_gpu(pred, 'part_clean')
    x24 = PartCleanFunction.apply(_flat(pred), keep)
    return padded_part_view(x24), x24


def padded_part_view(x24):
    """x24 [B*24, 24, H, W] (channels 21..23 zero) -> its [B,24,3,7,H,W] strided view (no copy)."""
    BJ, _, H, W = x24.shape
    return x24[:, :21].reshape(BJ // NJ, NJ, 3, NC, H, W)


class PartLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, iuv_img, theta, sample_w, sel, align, scales=None):
        pred = nhwc_bf16(pred)
        B, _, H, W = pred.shape
        gt = _gt_args('part_losses', iuv_img, theta, sel, sample_w, (B, H, W))
        ctx.align, ctx.scales = int(align), scales
        sums = _loss_fwd(pred, gt, ctx.align)
        ctx.save_for_backward(pred, *gt)
        if scales is not None:               # the three finished losses, one launch (glue.loss_finalize; see iuv_ops.IuvGlobalFunction)
            out = loss_finalize(3, scales, gt[2], B, sums=sums, rows=32)
            ctx.set_materialize_grads(False)
            return out[0:1], out[1:2], out[2:3]
        return sums.view(torch.float64).view(32, 3).sum(dim=0, dtype=torch.float64).float()

    @staticmethod
    def backward(ctx, *grads):
        pred, *gt = ctx.saved_tensors
        if ctx.scales is not None:
            if all(g is None for g in grads):
                return (None,) * 7
            scale = loss_finalize(3, ctx.scales, gt[2], pred.shape[0], grads=list(grads))
        else:
            scale = f32c(grads[0])
        return (_loss_bwd(pred, gt, scale, ctx.align),) + (None,) * 6


def part_losses(pred, iuv_img, theta, sample_w, sel, align, scales=None):
    """-> tensor [3]: sum over (b, joint, class, pixel) of fg * smooth_l1(U), same for V, and the sum over
    (b, joint, pixel) of w_b * cross-entropy of the index map; ground truth = the 3-channel IUV image
    resampled per joint by `theta` [B,24,2,3] (sel [24,6]: DensePose parts of each joint).
    scales = ((a, b),) * 3: the three FINISHED losses sums_i * a_i / (max(sum w, 1) * b_i) as a tuple of one-element tensors instead."""
    require_gpu(pred, 'part_losses')
    return PartLossFunction.apply(_flat(pred), iuv_img, theta, sample_w, sel, align, scales)


class PartJointFunction(torch.autograd.Function):
    """part_clean AND part_losses of one prediction as ONE autograd node (round 6): the prediction has two consumers -- the three losses and
    the regressor's cleaned operand -- and autograd summed their gradients with an add over three 151 MB tensors after two separate
    backward kernels; here the backward is one launch (danet_part_backward_fused) that reads the prediction once and writes its gradient once.
    Outputs: (x24, loss_pU, loss_pV, loss_pIndexUV) -- the finished losses (`scales`, see part_losses)."""

    @staticmethod
    def forward(ctx, pred, keep, iuv_img, theta, sample_w, sel, align, scales):
        pred, k = nhwc_bf16(pred), f32c(keep)
        B, _, H, W = pred.shape
        gt = _gt_args('part_joint', iuv_img, theta, sel, sample_w, (B, H, W))
        ctx.align, ctx.scales = int(align), scales
        x24 = _clean_fwd(pred, k)
        out = loss_finalize(3, scales, gt[2], B, sums=_loss_fwd(pred, gt, ctx.align), rows=32)
        ctx.save_for_backward(pred, k, *gt)
        ctx.set_materialize_grads(False)
        return x24, out[0:1], out[1:2], out[2:3]

    @staticmethod
    def backward(ctx, g24, *gl):
        pred, k, *gt = ctx.saved_tensors
        have_loss = any(g is not None for g in gl)
        if g24 is None and not have_loss:
            return (None,) * 8
        if g24 is not None:
            g24 = nhwc_bf16(g24)
        if not have_loss:
            gp = _clean_bwd(g24, pred, k)
        else:
            scale = loss_finalize(3, ctx.scales, gt[2], pred.shape[0], grads=list(gl))
            if g24 is None:
                gp = _loss_bwd(pred, gt, scale, ctx.align)
            elif _cpj(pred.shape[1]) != 24:              # (the unpadded layout: two kernels and an add, as autograd would)
                gp = _loss_bwd(pred, gt, scale, ctx.align) + _clean_bwd(g24, pred, k)
            else:
                gp = _fused_bwd(pred, gt, scale, g24, k, ctx.align)
        return (gp,) + (None,) * 7


def part_joint(pred, keep, iuv_img, theta, sample_w, sel, align, scales):
    """-> (x24, lU, lV, lI): part_clean(pred, keep)[1] and part_losses(..., scales=scales) as one autograd node."""
    require_gpu(pred, 'part_joint')
    return PartJointFunction.apply(_flat(pred), keep, iuv_img, theta, sample_w, sel, align, scales)


class PartGtFunction(torch.autograd.Function):
    """Ground-truth part crops of DANET.INPUT_MODE 'iuv_gt' (csrc/part_gt.hip), differentiable in theta:
    (iuv_img [B,3,H,W], theta [B,24,2,3], sel [24,6], keep [B,24,7] | None, keep25 [B,25] | None, align, body) ->
    x24 [B*24,24,H,W] bf16 channels_last (channels 21..23 zero) and, when `body`, the body operand [B,80,H,W] bf16 channels_last
    (no gradient).  Backward: d theta, all six entries (the IUV image carries no gradient)."""

    @staticmethod
    def forward(ctx, iuv_img, theta, sel, keep, keep25, align, body):
        img, th, _, sel = _gt_args('part_gt', iuv_img, theta, sel)
        B, _, H, W = img.shape
        k, k25 = f32c(keep), f32c(keep25)
        if (k is not None and k.shape != (B, NJ, NC)) or (k25 is not None and k25.shape != (B, 25)):
            raise ValueError('part_gt: bad keep shapes')
        x24 = torch.empty(B * NJ, H, W, 24, dtype=torch.bfloat16, device=img.device)
        mp = torch.empty(B, H, W, 80, dtype=torch.bfloat16, device=img.device) if body else None
        check(_lib.lib().danet_part_gt_forward(ptr(img), ptr(th), ptr(sel), ptr(k), ptr(k25), B, H, W, int(bool(align)), ptr(x24), ptr(mp),
                                               stream()), 'danet_part_gt_forward')
        ctx.save_for_backward(img, th, sel, k)
        ctx.align = int(bool(align))
        ctx.theta_dtype = theta.dtype
        ctx.set_materialize_grads(False)
        if mp is None:
            return x24.permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(mp)
        return x24.permute(0, 3, 1, 2), mp.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g24, *_):
        if g24 is None or not ctx.needs_input_grad[1]:
            return (None,) * 7
        img, th, sel, k = ctx.saved_tensors
        B, _, H, W = img.shape
        g24 = nhwc_bf16(g24)
        dth = torch.empty(B, NJ, 2, 3, dtype=torch.float32, device=img.device)
        check(_lib.lib().danet_part_gt_backward(ptr(img), ptr(th), ptr(sel), ptr(k), nptr(g24), B, H, W, ctx.align,
                                                ptr(dth), stream()), 'danet_part_gt_backward')
        return None, dth.to(ctx.theta_dtype), None, None, None, None, None


def part_gt(iuv_img, theta, sel, keep=None, keep25=None, align=True, body=False):
    """x24 [B*24,24,H,W] bf16 channels_last = keep * (part_iuv_simp + affine_grid/grid_sample of the IUV image by theta), channels 21..23
    zero (the regressor's limb operand, as part_clean makes it); with body=True also the body operand [B,80,H,W] (iuvmap_clean of the
    keep25-dropped iuv_img2map, [U | V | I | 5 zeros]).  Differentiable in theta.  GPU only."""
    require_gpu(iuv_img, 'part_gt')
    return PartGtFunction.apply(iuv_img, theta, sel, keep, keep25, align, body)
