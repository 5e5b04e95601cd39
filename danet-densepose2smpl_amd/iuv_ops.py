"""Global (25-class) IUV glue on HIP kernels (csrc/iuv_ops.hip): the estimator's `iuv_img2map` + `body_uv_losses`
(/root/reference/models/danet/iuv_estimator.py:95-104,304-341, utils/iuvmap.py:103-147) and DaNet.forward's part drop +
`iuvmap_clean` + concat (models/danet/danet.py:194-205,247, utils/iuvmap.py:6-38) as ONE op per pass, and the
soft-argmax of the joint heat-maps (utils/keypoints.py:334-394); and the DensePose-COCO point supervision
(models/danet/iuv_estimator.py:343-419) as one launch per pass (csrc/dp_losses.hip).  GPU only; the tensor-op forms in iuvmap.py /
geometry.py remain as the CPU-checkable statement of the same arithmetic (tests pin both against the reference's
golden vectors)."""
import torch

from . import _lib
from ._lib import ptr, check, stream, f32c, require_gpu
from .glue import loss_finalize

NP, NA, MAPC = 25, 15, 80
LDP, LDA = 32, 16          # leading width (floats per pixel row) of the U / V / Index heads and of the Ann head
VALID, LDS = (NP, NP, NP, NA), (LDP, LDP, LDP, LDA)
PADDED_BASES = bool(int(__import__('os').environ.get('DANET_IUV_PADDED_BASES', '1')))       # A-B knob


def _rows(t, valid, ld):
    """[B,C,H,W] fp32 head output -> (tensor whose memory is [B*H*W][ld] floats with the `valid` channels first, ld).
    The conv epilogue's zero-padded NHWC output qualifies as it is (a view); anything else is copied into that form."""
    B, C, H, W = t.shape
    if t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(3) == ld and t.stride(2) == W * ld and t.stride(0) == H * W * ld:
        return t
    buf = torch.zeros(B, H, W, ld, dtype=torch.float32, device=t.device)
    buf[..., :valid] = t[:, :valid].permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :valid]


def _head_rows(heads):
    """The four head outputs (u, v, index, ann) -> (their four row tensors, `full` flags).  full: the input IS the conv epilogue's
    padded output (all 32 / 16 channels: _padded_bases hands those over when it can) and gets its gradient back at that width -- no
    slice-backward (a fill + a copy of the padded tensor per head) in between."""
    return [_rows(t, n, ld) for t, n, ld in zip(heads, VALID, LDS)], tuple(t.shape[1] == ld for t, ld in zip(heads, LDS))


def _grad_buffers(B, H, W, device):
    """The four heads' gradient buffers, NHWC at the leading widths (fully written by the kernels: no memset)."""
    du = torch.empty(B, H, W, LDP, dtype=torch.float32, device=device)
    return du, torch.empty_like(du), torch.empty_like(du), torch.empty(B, H, W, LDA, dtype=torch.float32, device=device)


def _head_grads(bufs, full):
    """Gradient buffers + `full` -> the four returned gradients: at full width for padded bases, the valid channels otherwise."""
    return tuple(t.permute(0, 3, 1, 2) if f else t.permute(0, 3, 1, 2)[:, :n] for t, n, f in zip(bufs, VALID, full))


class IuvGlobalFunction(torch.autograd.Function):
    """(u, v, index, ann, gt_img | None, w | None, keep25 | None) -> (sums[4], iuv_map [B,80,H,W] bf16 channels_last,
    argmax [B,H,W] uint8 of the raw index logits)."""

    @staticmethod
    def forward(ctx, u, v, ix, an, gt, w, keep, scales=None):
        """scales (round 6) = four (a, b) pairs: the op returns the four FINISHED losses sum_i * a_i / (max(sum w, 1) * b_i) (b_i = 0: no
        division) as separate one-element tensors instead of the raw sum vector -- one launch (glue.loss_finalize) where the selects,
        multiplications / divisions, their backward and the select-backward fills cost ~6 launches per loss and pass."""
        L = _lib.lib()
        B, _, H, W = u.shape
        (u, v, ix, an), ctx.full = _head_rows((u, v, ix, an))
        want = gt is not None
        gtc, wc, kc = f32c(gt), f32c(w), f32c(keep)
        dev = u.device
        mp = torch.empty(B, H, W, MAPC, dtype=torch.bfloat16, device=dev)
        am_raw = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        am_drop = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        sums = torch.zeros(4, dtype=torch.float64, device=dev)         # double accumulators: exact, order-independent adds of the workgroups' partial sums
        check(L.danet_iuv_global_forward(u.data_ptr(), v.data_ptr(), ix.data_ptr(), an.data_ptr(), LDP, LDA, ptr(gtc), ptr(wc), ptr(kc),
                                         B, H, W, int(want), ptr(mp), ptr(am_raw), ptr(am_drop), ptr(sums), stream()), 'danet_iuv_global_forward')
        ctx.save_for_backward(u, v, ix, an, gtc, wc, kc, am_drop)
        ctx.want = want
        ctx.scales = scales
        ctx.mark_non_differentiable(am_raw)
        if scales is not None:
            out = loss_finalize(4, scales, wc, B, sums=sums, rows=1)
            ctx.set_materialize_grads(False)
            return out[0:1], out[1:2], out[2:3], out[3:4], mp.permute(0, 3, 1, 2), am_raw
        return sums.float(), mp.permute(0, 3, 1, 2), am_raw

    @staticmethod
    def backward(ctx, *grads):
        L = _lib.lib()
        u, v, ix, an, gtc, wc, kc, am_drop = ctx.saved_tensors
        B, _, H, W = u.shape
        dev = u.device
        if ctx.scales is not None:
            g4, gmap = grads[:4], grads[4]
            gsums = None
            if ctx.want and any(g is not None for g in g4):
                gsums = loss_finalize(4, ctx.scales, wc, B, grads=list(g4))
        else:
            gsums, gmap = grads[0], grads[1]
        bufs = _grad_buffers(B, H, W, dev)
        coef = None
        if ctx.want:
            coef = torch.zeros(4, dtype=torch.float32, device=dev) if gsums is None else gsums.to(torch.float32).contiguous()
        gm = None
        if gmap is not None:
            gm = gmap.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        check(L.danet_iuv_global_backward(u.data_ptr(), v.data_ptr(), ix.data_ptr(), an.data_ptr(), LDP, LDA, ptr(gtc), ptr(wc), ptr(kc),
                                          ptr(am_drop), ptr(gm), ptr(coef), B, H, W, int(ctx.want and coef is not None),
                                          *[ptr(t) for t in bufs], stream()), 'danet_iuv_global_backward')
        return _head_grads(bufs, ctx.full) + (None,) * 4


def iuv_global(u, v, ix, an, gt=None, w=None, keep=None, scales=None):
    """sums = (sum smooth-L1 U, sum smooth-L1 V, sum CE index, sum CE ann) over the batch, weighted per sample by w
    (zeros when gt is None); iuv_map = [U_clean | V_clean | one-hot | 5 zero channels] as a bf16 channels_last
    [B,80,H,W] tensor (the body regressor's padded first-conv operand); argmax = uint8 [B,H,W] of the raw index head.
    scales = ((a, b),) * 4: the first result is the tuple of the four finished losses sums_i * a_i / (max(sum w, 1) * b_i) instead."""
    require_gpu(u, 'iuv_global')
    u, v, ix, an = _padded_bases(u, v, ix, an)
    return _pack(IuvGlobalFunction.apply(u, v, ix, an, gt, w, keep, scales), scales)


def _padded_bases(u, v, ix, an):
    """The hand-over rule of iuv_global and dp_point_losses: -> the four `_padded_base` tensors when all four head outputs carry one
    that qualifies (and gradients are being recorded), the tensors as they came otherwise.  Head outputs that are [:, :25] / [:, :15]
    views of the conv epilogue's zero-padded fp32 NHWC output carry that tensor along (conv.conv2d `_padded_base`): taking IT as the
    differentiable input keeps autograd's slice-backward out of the backward pass."""
    if PADDED_BASES and torch.is_grad_enabled():
        bases = [getattr(t, '_padded_base', None) for t in (u, v, ix, an)]
        ok = all(b is not None and b.dtype == torch.float32 and b.shape[0] == t.shape[0] and b.shape[2:] == t.shape[2:] and
                 b.data_ptr() == t.data_ptr() and b.shape[1] == ld for b, t, ld in zip(bases, (u, v, ix, an), LDS))
        if ok and all(_rows(b, n, ld) is b for b, n, ld in zip(bases, VALID, LDS)):
            return bases
    return u, v, ix, an


def _pack(out, scales):
    """(sums, map, argmax), with `scales` the four finished losses as a tuple in place of the sum vector."""
    return out if scales is None else (tuple(out[:4]), out[4], out[5])


class SoftArgmaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, scale):
        L = _lib.lib()
        B, J, H, W = hm.shape
        ld = (J + 3) // 4 * 4
        rows = _rows(hm, J, ld)
        out = torch.empty(B, J, 2, dtype=torch.float32, device=hm.device)
        saved = torch.empty(B, J, 4, dtype=torch.float32, device=hm.device)
        check(L.danet_softargmax_forward(rows.data_ptr(), ld, B, J, H, W, float(scale), ptr(out), ptr(saved), stream()), 'danet_softargmax_forward')
        ctx.save_for_backward(rows, saved)
        ctx.cfg = (ld, float(scale))
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        rows, saved = ctx.saved_tensors
        B, J, H, W = rows.shape
        ld, scale = ctx.cfg
        d = torch.empty(B, H, W, J, dtype=torch.float32, device=rows.device)
        check(L.danet_softargmax_backward(rows.data_ptr(), ld, B, J, H, W, scale, ptr(saved), ptr(g.to(torch.float32).contiguous()), ptr(d), stream()),
              'danet_softargmax_backward')
        return d.permute(0, 3, 1, 2), None


def softargmax(hm, scale=1.0):
    """Expected (x, y) pixel index of softmax(scale * hm) over each joint's map: [B,J,H,W] -> [B,J,2]
    (= softmax_integral_tensor(scale * hm, J, H, W) of geometry.py)."""
    require_gpu(hm, 'softargmax')
    return SoftArgmaxFunction.apply(hm, scale)


NPT = 196          # DensePose point slots per sample (datasets/base_dataset.py:228-232)


class DpPointLossesFunction(torch.autograd.Function):
    """(u, v, index, ann, X, Y, I, U, V, point weights, ann labels, w [B] in {0, 1}, align, scales) -> the four finished losses
    (csrc/dp_losses.hip + glue.loss_finalize); the gradients come back at the inputs' width (32 / 16 channels for padded bases)."""

    @staticmethod
    def forward(ctx, u, v, ix, an, X, Y, I, TU, TV, PW, labels, w, align, scales):
        L = _lib.lib()
        B, _, H, W = u.shape
        if H != W:
            raise RuntimeError('dp_point_losses: square maps expected, got %d x %d' % (H, W))
        (u, v, ix, an), ctx.full = _head_rows((u, v, ix, an))
        rows = L.danet_dp_point_losses_rows(B, H)
        partial = torch.empty(rows, 4, dtype=torch.float64, device=u.device)      # one row of double sums per workgroup, every row written
        check(L.danet_dp_point_losses_forward(u.data_ptr(), v.data_ptr(), ix.data_ptr(), an.data_ptr(), LDP, LDA, ptr(X), ptr(Y), ptr(I), ptr(TU),
                                              ptr(TV), ptr(PW), ptr(labels), ptr(w), B, H, int(bool(align)), ptr(partial), stream()),
              'danet_dp_point_losses_forward')
        ctx.save_for_backward(u, v, ix, an, X, Y, I, TU, TV, PW, labels, w)
        ctx.align, ctx.scales = bool(align), scales
        ctx.set_materialize_grads(False)
        out = loss_finalize(4, scales, w, B, sums=partial, rows=rows)
        return out[0:1], out[1:2], out[2:3], out[3:4]

    @staticmethod
    def backward(ctx, *g4):
        L = _lib.lib()
        u, v, ix, an, X, Y, I, TU, TV, PW, labels, w = ctx.saved_tensors
        B, _, H, W = u.shape
        if all(g is None for g in g4):
            return (None,) * 14
        coef = loss_finalize(4, ctx.scales, w, B, grads=list(g4))
        bufs = _grad_buffers(B, H, W, u.device)
        check(L.danet_dp_point_losses_backward(u.data_ptr(), v.data_ptr(), ix.data_ptr(), an.data_ptr(), LDP, LDA, ptr(X), ptr(Y), ptr(I), ptr(TU),
                                               ptr(TV), ptr(PW), ptr(labels), ptr(w), ptr(coef), B, H, int(ctx.align),
                                               *[ptr(t) for t in bufs], stream()), 'danet_dp_point_losses_backward')
        return _head_grads(bufs, ctx.full) + (None,) * 10


def dp_point_losses(u, v, index, ann, dp, has_dp=None, align=True):
    """IUV_Estimator.dp_uvia_losses (the CPU-checkable statement of this arithmetic) as one HIP launch per pass: the heads' [B,25|15,S,S]
    outputs (or their zero-padded bases), the 9 DensePose blobs `dp` of a batch, has_dp [B] or None (= all labelled) ->
    (loss_Udp, loss_Vdp, loss_IndexUVdp, loss_segAnndp), one-element tensors.  Every sample is evaluated and weighted by
    has_dp > 0; an all-zero has_dp gives exact zeros.  The backward pass uses no floating-point atomics: two runs are bitwise equal."""
    from .config import cfg
    require_gpu(u, 'dp_point_losses')
    B, S = u.shape[0], u.shape[-1]
    f32 = lambda k, n: dp[k].detach().reshape(B, n).to(torch.float32).contiguous()                   # noqa: E731
    w = torch.ones(B, device=u.device) if has_dp is None else (has_dp.detach().reshape(B) > 0).to(torch.float32)
    scales = ((cfg.DANET.POINT_REGRESSION_WEIGHTS, 0.), (cfg.DANET.POINT_REGRESSION_WEIGHTS, 0.),
              (cfg.DANET.PART_WEIGHTS, float(NPT)), (cfg.DANET.INDEX_WEIGHTS, float(S * S)))
    u, v, index, ann = _padded_bases(u, v, index, ann)
    return DpPointLossesFunction.apply(u, v, index, ann, f32('body_uv_X_points', NPT), f32('body_uv_Y_points', NPT), f32('body_uv_I_points', NPT),
                                       f32('body_uv_U_points', NP * NPT), f32('body_uv_V_points', NP * NPT), f32('body_uv_point_weights', NP * NPT),
                                       dp['body_uv_ann_labels'].detach().reshape(B, S * S).to(torch.int32).contiguous(), w, align, scales)
