"""Generates the fixtures of DANET.INPUT_MODE 'iuv_gt' by IMPORTING the reference, like make_golden.py (whose parameter and input formulas
it reuses): g23_iuvgt_{train,eval}.npz (B = 4) and g23_iuvgt_b32.npz (B = 32, train).  The reference's IUV_Estimator in 'iuv_gt' mode
(iuv_estimator.py:64-89: the 24 crops of the ground-truth IUV image, differentiable in the crop ratios) feeds its DecomposedPredictor
together with iuvmap_clean(iuv_img2map(image)) (danet.py:245-262,314-323; jitters and part drop 0), forward and backward, in double and in
single precision.  Re-run:  python tests/golden/make_golden_iuvgt.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref_env, formula_params, g19_inputs, g19_grad_sample, save   # noqa: E402

ENV = {'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.INPUT_MODE': 'iuv_gt', 'DANET.USE_LEARNED_RATIO': False,
       'DANET.PART_UVI_SCALE': 1.0, 'DANET.PART_UVI_LR_OFFSET': 0.1, 'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0.,
       'DANET.PARTDROP_RATE': 0.}
SKIP = ('mean_', 'I_n', 'A_link', 'A_mask', 'A', 'r2p_A', 'p2r_A')
GRAD_NAMES = ('limb_net.0.weight', 'body_net.3.layer4.1.conv2.weight', 'pose_regressors.1.1.weight')
RELU_ZERO = (5, 7)          # learned_ratio[5] < 0 and learned_offset[7] < 0: the ReLU passes no gradient there


def ratio_offset():
    """Closed-form crop ratios / offsets (one negative entry of each)."""
    j = torch.arange(24, dtype=torch.float64)
    ratio = 0.55 + 0.025 * j
    offset = 0.06 + 0.004 * j
    ratio[RELU_ZERO[0]] = -0.3
    offset[RELU_ZERO[1]] = -0.02
    return ratio.float(), offset.float()


def _mean():
    pose6 = torch.tensor([1., 0., 0., 1., 0., 0.]).repeat(24).unsqueeze(0)
    return torch.tensor([[0.9, 0., 0.]]), torch.zeros(1, 10), pose6


def loss_weights(para):
    return torch.cos(torch.arange(para.numel(), dtype=para.dtype).view_as(para) * 0.37)


def _run(B, train):
    ref_env(ENV)
    import torch.nn.functional as F
    ag, gs = F.affine_grid, F.grid_sample
    # the reference was written for torch 1.1 (align_corners=True semantics) -- as g19 / g17
    F.affine_grid = lambda theta, size, align_corners=None: ag(theta, size, align_corners=True)
    F.grid_sample = lambda x, grid, mode='bilinear', padding_mode='zeros', align_corners=None: gs(x.to(grid.dtype), grid, mode, padding_mode, align_corners=True)
    try:
        from models.danet.iuv_estimator import IUV_Estimator
        from models.danet.smpl_regressor import DecomposedPredictor
        from utils.iuvmap import iuv_img2map, iuvmap_clean
        _, gt, kps = g19_inputs(B, 64)
        ratio, offset = ratio_offset()
        res = {}
        for dt in (torch.float64, torch.float32):
            torch.manual_seed(0)
            est = IUV_Estimator(pretrained=False)
            assert not hasattr(est, 'iuv_est')
            with torch.no_grad():
                est.learned_ratio.copy_(ratio)
                est.learned_offset.copy_(offset)
            pred = DecomposedPredictor(None, _mean(), pretrained=False)
            formula_params(pred, skip=SKIP)
            est, pred = est.to(dt).train(train), pred.to(dt).train(train)
            torch.set_default_dtype(dt)
            try:
                with torch.set_grad_enabled(train):
                    # (the estimator's scale_box path and affine_para as the reference runs them; thetas are captured by a wrapper)
                    thetas = []
                    ap = est.affine_para

                    def tap(c, part_hidden=None):
                        th, sc = ap(c, part_hidden)
                        thetas.append(torch.stack(th, 1))
                        return th, sc
                    est.affine_para = tap
                    rd = est(None, gt.to(dt), kps.to(dt))
                    part = rd['part_iuv_gt']
                    u, v, i, _ = iuvmap_clean(*iuv_img2map(gt.to(dt)))
                    out = pred(torch.cat([u, v, i], 1), part)
                    if train:
                        para = out['para']
                        loss = (para * loss_weights(para)).sum() + sum(t.sum() for t in out['joint_position']) + out['joint_rotation'][0].sum()
                        loss.backward()
            finally:
                torch.set_default_dtype(torch.float32)
            o = {'theta': thetas[0].detach(), 'part_iuv_gt': part.detach(), 'para': out['para'].detach()}
            if train:
                pd = dict(pred.named_parameters())
                o['d_ratio'] = est.learned_ratio.grad.clone()
                o['d_offset'] = est.learned_offset.grad.clone()
                for n in GRAD_NAMES:
                    o['grad__' + n.replace('.', '__')] = pd[n].grad.clone()
            res[dt] = o
        return res, gt, kps, ratio, offset
    finally:
        F.affine_grid, F.grid_sample = ag, gs


def _part_sub(t, B):
    """A sub-sample of [B,24,3,7,64,64]: every 3rd joint and 4th pixel (B = 4); every 4th sample, 6th joint and 8th pixel (B = 32)."""
    return t[:, ::3, :, :, ::4, ::4].contiguous() if B <= 4 else t[::4, ::6, :, :, ::8, ::8].contiguous()


def _make(name, B, train):
    res, gt, kps, ratio, offset = _run(B, train)
    r64, r32 = res[torch.float64], res[torch.float32]
    arrs = {'ratio': ratio, 'offset': offset, 'relu_zero': np.array(RELU_ZERO)}
    for k in r64:
        ref = r64[k]
        if k == 'part_iuv_gt':
            arrs['part_iuv_gt'] = _part_sub(ref, B).float()
        elif k.startswith('grad__'):
            arrs['grad64__' + k[6:]] = g19_grad_sample(ref.float())
        else:
            arrs[k + '64'] = ref.float()
            arrs[k + '32'] = r32[k]
        arrs['floor__' + k] = ((r32[k].double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30)).float()
        print(name, k, 'fp32 reference vs fp64: %.3g of scale' % float(arrs['floor__' + k]))
    if train:
        assert float(r64['d_ratio'][RELU_ZERO[0]]) == 0.0 and float(r64['d_offset'][RELU_ZERO[1]]) == 0.0
    save(name, **arrs)


def g23():
    _make('g23_iuvgt_train', 4, True)
    _make('g23_iuvgt_eval', 4, False)


def g23_b32():
    _make('g23_iuvgt_b32', 32, True)


if __name__ == '__main__':
    which = sys.argv[1:] or ['g23', 'g23_b32']
    for w in which:
        globals()[w]()
