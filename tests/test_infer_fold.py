"""BatchNorm folding of the inference engine (danet_densepose2smpl_amd/inference.py) on the CPU: the fold math in fp64 against
F.batch_norm(conv(x)) for every layer kind the models have, and the fold plan of both backbones."""
import pytest
import torch
import torch.nn.functional as F

from danet_densepose2smpl_amd.inference import fold_conv_bn, fold_plan


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) * 2 + 0.1)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) * 3 + 0.05)
    return bn


def _rel(a, b):
    return float((a - b).detach().abs().max() / b.detach().abs().max())


@pytest.mark.parametrize('cin,cout,k,stride,pad,groups,with_bias', [
    (16, 32, 3, 1, 1, 1, False),
    (16, 32, 3, 2, 1, 1, True),
    (64, 64, 7, 2, 3, 1, False),        # the regressors' stems
    (75, 64, 1, 1, 0, 1, False),        # _StemNet's 1x1 on the IUV maps
    (24 * 8, 24 * 16, 3, 2, 1, 24, False),      # LimbResLayers: groups = 24
    (24 * 4, 24 * 4, 3, 1, 1, 24, True),
])
def test_fold_conv_bn_matches_conv_then_eval_batchnorm(cin, cout, k, stride, pad, groups, with_bias):
    g = torch.Generator().manual_seed(cin * 7 + cout + groups)
    x = torch.randn(2, cin, 12, 12, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin // groups, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64) if with_bias else None
    bn = _bn(cout, cout + k)
    ref = bn(F.conv2d(x, w, b, stride, pad, 1, groups))
    w2, b2 = fold_conv_bn(w, b, bn)
    assert w2.dtype == torch.float64 and w2.shape == w.shape and b2.shape == (cout,)
    assert _rel(F.conv2d(x, w2, b2, stride, pad, 1, groups), ref) <= 1e-12


@pytest.mark.parametrize('with_bias', [False, True])
def test_fold_conv_transpose_k4_s2_p1(with_bias):
    """PoseResNet's deconvolution stack: the output channel of a ConvTranspose2d weight is dim 1."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 6, 6, generator=g, dtype=torch.float64)
    w = torch.randn(32, 24, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(24, generator=g, dtype=torch.float64) if with_bias else None
    bn = _bn(24, 11)
    ref = bn(F.conv_transpose2d(x, w, b, 2, 1))
    w2, b2 = fold_conv_bn(w, b, bn, transposed=True)
    assert _rel(F.conv_transpose2d(x, w2, b2, 2, 1), ref) <= 1e-12


def test_fold_padded_width_bottleneck():
    """The heat-map head's Bottleneck(48, 12) (inner width 12, run at 16 by resnet.Bottleneck._forward_padded): the folded block with
    zero-padded folded weights equals the module's own eval-mode forward math."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 48, 10, 10, generator=g, dtype=torch.float64)
    ws = [torch.randn(12, 48, 1, 1, generator=g, dtype=torch.float64), torch.randn(12, 12, 3, 3, generator=g, dtype=torch.float64),
          torch.randn(48, 12, 1, 1, generator=g, dtype=torch.float64)]
    bns = [_bn(12, 1), _bn(12, 2), _bn(48, 3)]
    ref = F.relu(bns[0](F.conv2d(x, ws[0])))
    ref = F.relu(bns[1](F.conv2d(ref, ws[1], None, 1, 1)))
    ref = F.relu(bns[2](F.conv2d(ref, ws[2])) + x)
    f = [fold_conv_bn(w, None, bn) for w, bn in zip(ws, bns)]
    pad = lambda t, dims: F.pad(t, dims)
    w1, b1 = pad(f[0][0], (0, 0, 0, 0, 0, 0, 0, 4)), pad(f[0][1], (0, 4))        # 12 -> 16 output channels, zero rows
    w2, b2 = pad(f[1][0], (0, 0, 0, 0, 0, 4, 0, 4)), pad(f[1][1], (0, 4))
    w3, b3 = pad(f[2][0], (0, 0, 0, 0, 0, 4)), f[2][1]
    out = F.relu(F.conv2d(x, w1, b1))
    out = F.relu(F.conv2d(out, w2, b2, 1, 1))
    out = F.relu(F.conv2d(out, w3, b3) + x)
    assert _rel(out, ref) <= 1e-12


def test_fold_keeps_inputs_and_stores_fp32():
    bn = _bn(8, 4).float()
    w = torch.randn(8, 4, 3, 3)
    w0 = w.clone()
    sd = {k: v.clone() for k, v in bn.state_dict().items()}
    w2, b2 = fold_conv_bn(w, None, bn)
    assert w2.dtype == torch.float32 and b2.dtype == torch.float32
    assert torch.equal(w, w0) and all(torch.equal(v, bn.state_dict()[k]) for k, v in sd.items())
    s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
    assert torch.equal(w2, (w.double() * s.view(-1, 1, 1, 1)).float())


@pytest.mark.parametrize('regressor,n_img,n_total', [('hrnet', 301, 343), ('resnet', 65, 107)])
def test_fold_plan_pairs_every_batchnorm_of_both_backbones(regressor, n_img, n_total):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    from danet_densepose2smpl_amd.nn import BatchNorm2d
    from danet_densepose2smpl_amd.deconv import ConvTranspose2d
    reset_cfg()
    try:
        cfg_from_dict({'DANET.IUV_REGRESSOR': regressor})
        model = DaNet(default_options(2), None, pretrained=False)
    finally:
        reset_cfg()
    plan = fold_plan(model)
    assert plan.unfolded == []
    assert len(plan) == n_total
    assert sum(p.bn_name.startswith('img2iuv.') for p in plan.pairs) == n_img
    assert n_total - n_img == 42
    assert all(isinstance(p.bn, BatchNorm2d) for p in plan.pairs)
    assert len({id(p.bn) for p in plan.pairs}) == n_total and len({id(p.conv) for p in plan.pairs}) == n_total
    assert all(p.transposed == isinstance(p.conv, ConvTranspose2d) for p in plan.pairs)
    assert sum(p.transposed for p in plan.pairs) == (3 if regressor == 'resnet' else 0)
    # the reference's unused rot2pos / pos2rot BatchNorms are skipped, not folded
    assert plan.skipped and all('.rot2pos.' in n or '.pos2rot.' in n for n in plan.skipped)
