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


# ---- the epilogue checker itself (tests/conv_bound.py), on a simulated bf16 launch --------------------------------------------------
# y = bf16(relu(acc + b[c] + res)) with acc the fp32 convolution of bf16 operands: what a folded launch computes.  The checker must
# accept it at every layer kind the engine launches and reject each of the faults a subtly wrong epilogue would make.

def _launch(B, Cin, Cout, H, k, stride, groups, transposed, with_res, relu, seed, fault=None, two_roundings=False, res_scale=1.):
    """(simulated result, fp64 reference on the same operands) -- `fault` plants one epilogue error in the result."""
    from conv_bound import reference
    g = torch.Generator().manual_seed(seed)
    pad = (k - 1) // 2 if not transposed else 1
    x = torch.randn(B, Cin, H, H, generator=g).bfloat16()
    if transposed:
        w = (torch.randn(Cin, Cout, k, k, generator=g) / (Cin * k * k / stride ** 2) ** 0.5).bfloat16()
        acc = F.conv_transpose2d(x.float(), w.float(), None, stride, pad)
    else:
        w = (torch.randn(Cout, Cin // groups, k, k, generator=g) / (Cin // groups * k * k) ** 0.5).bfloat16()
        acc = F.conv2d(x.float(), w.float(), None, stride, pad, 1, groups)
    b = torch.randn(Cout, generator=g) * 0.5
    res = (torch.randn(acc.shape, generator=g) * res_scale).bfloat16() if with_res else None
    ref = reference(x, w, b, res, relu, stride, pad, 1, groups, transposed)
    bb = b.clone()
    if fault == 'bias_shift':              # one channel's bias off by 1 % of that channel's output RMS
        c = int(ref.r.pow(2).mean((0, 2, 3)).argmax())
        bb[c] += 0.01 * ref.r[:, c].pow(2).mean().sqrt().item()
    elif fault == 'group_bias':            # group 0's bias applied to group 1
        n = Cout // groups
        bb[n:2 * n] = b[:n]
    z = acc + bb.view(1, -1, 1, 1)
    if two_roundings:                      # the convolution rounded on its own, then the sum / ReLU kernel
        z = z.bfloat16().float()
    if res is not None:
        add = res.float().clone()
        if fault == 'addend_tail':         # the addend missing on the last 4 x 4 tile of the last batch item
            add[-1, :, -4:, -4:] = 0
        z = (F.relu(z) if fault == 'relu_first' else z) + add
    y = (F.relu(z) if relu else z).bfloat16()
    return y, ref


_LAYERS = [            # (B, Cin, Cout, H, k, stride, groups, transposed)
    (3, 16, 32, 12, 3, 1, 1, False),
    (3, 64, 64, 16, 7, 2, 1, False),       # the regressors' stem
    (2, 256, 48, 8, 1, 1, 1, False),       # pointwise, long dot product
    (4, 96, 96, 8, 3, 1, 24, False),       # LimbResLayers: groups = 24
    (2, 192, 384, 8, 3, 2, 24, False),
    (3, 32, 24, 6, 4, 2, 1, True),         # PoseResNet's deconvolutions: k4 / s2 / p1
]


@pytest.mark.parametrize('layer', _LAYERS, ids=lambda l: 'B%d_%dx%d_k%d_s%d_g%d%s' % (l[0], l[1], l[2], l[4], l[5], l[6], '_T' if l[7] else ''))
@pytest.mark.parametrize('with_res,relu', [(False, False), (False, True), (True, True), (True, False)])
def test_epilogue_bound_accepts_a_correct_bf16_launch(layer, with_res, relu):
    from conv_bound import U_BF16, check
    y, ref = _launch(*layer, with_res, relu, seed=sum(layer[:6]) + 2 * with_res + relu)
    check(y, ref, U_BF16, ('single', layer))
    if with_res or relu:                   # a separate sum / ReLU launch after a rounded convolution: within the two-rounding bound
        y2, ref2 = _launch(*layer, with_res, relu, seed=sum(layer[:6]) + 2 * with_res + relu, two_roundings=True)
        check(y2, ref2, U_BF16, ('two', layer), rounded_conv=True)


@pytest.mark.parametrize('layer', [(3, 16, 32, 12, 3, 1, 1, False), (2, 256, 48, 8, 1, 1, 1, False), (4, 96, 96, 8, 3, 1, 24, False)])
def test_epilogue_bound_accepts_an_addend_dominated_launch(layer):
    """A residual stream much larger than the convolution (deep residual blocks): y rounds back onto the addend's bf16 grid, so y - r
    per channel is close to minus the convolution's mean, a bias.  The per-channel check compares against the rounded reference, so it
    does not count that bias as an error."""
    from conv_bound import U_BF16, check
    for res_scale in (16., 64.):
        y, ref = _launch(*layer, True, False, seed=17, res_scale=res_scale)
        check(y, ref, U_BF16, ('addend-dominated', layer, res_scale))


@pytest.mark.parametrize('fault,layer', [
    ('bias_shift', (3, 64, 64, 16, 7, 2, 1, False)),
    ('bias_shift', (3, 16, 32, 12, 3, 1, 1, False)),
    ('bias_shift', (4, 96, 96, 8, 3, 1, 24, False)),
    ('bias_shift', (3, 32, 24, 6, 4, 2, 1, True)),
    ('addend_tail', (3, 16, 32, 12, 3, 1, 1, False)),
    ('addend_tail', (2, 256, 48, 8, 1, 1, 1, False)),
    ('relu_first', (3, 16, 32, 12, 3, 1, 1, False)),
    ('relu_first', (4, 96, 96, 8, 3, 1, 24, False)),
    ('group_bias', (4, 96, 96, 8, 3, 1, 24, False)),
    ('group_bias', (2, 192, 384, 8, 3, 2, 24, False)),
])
def test_epilogue_bound_rejects_planted_faults(fault, layer):
    from conv_bound import U_BF16, ratios
    seed = sum(layer[:6]) + 3
    y, ref = _launch(*layer, True, True, seed=seed)
    assert max(ratios(y, ref, U_BF16)) <= 1.0
    yf, ref = _launch(*layer, True, True, seed=seed, fault=fault)
    elem, mean = ratios(yf, ref, U_BF16)
    assert max(elem, mean) > 1.0, (fault, elem, mean)
    if fault == 'bias_shift':               # the per-channel mean is what sees a 1 % bias error
        assert mean > 1.0, (elem, mean)


def test_fp32_bound_accepts_the_fp32_mode_and_rejects_a_bf16_rounding():
    """The fp32 verification mode's bound (u = 2^-22, the conv rounded before the sum / ReLU kernel) holds for an fp32 launch and is
    far below one bf16 rounding of the same result."""
    from conv_bound import U_F32, reference, ratios
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 48, 16, 16, generator=g)
    w = torch.randn(48, 48, 3, 3, generator=g) / (48 * 9) ** 0.5
    b = torch.randn(48, generator=g) * 0.5
    res = torch.randn(3, 48, 16, 16, generator=g)
    ref = reference(x, w, b, res, True, 1, 1)
    y = F.relu(F.conv2d(x, w, b, 1, 1) + res)
    assert max(ratios(y, ref, U_F32, rounded_conv=True)) <= 1.0
    assert max(ratios(y.bfloat16(), ref, U_F32, rounded_conv=True)) > 1.0
