"""DANET.INPUT_MODE 'iuv_gt' on the device: the ground-truth crop op (csrc/part_gt.hip) against the fp64 oracle (tests/part_gt_oracle.py)
in both directions, its bitwise reproducibility eager and under graph replay, the estimator + predictor path against the reference's own
results (g23), train steps (eager and captured) that move the learned crop ratios as Adam says, infer_net, and that the default mode
never calls the new op."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, record

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import formula_params, g19_inputs, g19_grad_sample    # noqa: E402
from make_golden_iuvgt import SKIP, loss_weights                         # noqa: E402
import part_gt_oracle as orc                                             # noqa: E402

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(kw)


@pytest.fixture(autouse=True)
def _reset():
    from danet_densepose2smpl_amd import nn as dnn
    prev = dnn.ONEPASS_STREAM
    yield
    from danet_densepose2smpl_amd.config import reset_cfg
    reset_cfg()
    dnn.ONEPASS_STREAM = prev


def _sel():
    from danet_densepose2smpl_amd.iuv_estimator import DP2SMPL_MAPPING
    return torch.tensor(DP2SMPL_MAPPING, dtype=torch.int32)


def _keep(B, seed):
    k = (torch.rand(B, 24, 7, generator=torch.Generator().manual_seed(seed)) > 0.3).float()
    k[..., 0] = 1
    return k


def _keep25(B, seed):
    k = (torch.rand(B, 25, generator=torch.Generator().manual_seed(seed)) > 0.3).float()
    k[:, 0] = 1
    return k


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,keep,align', [(1, 64, False, 1), (3, 56, True, 1), (3, 64, True, 0), (1, 56, False, 0), (32, 64, True, 1)])
def test_op_forward_vs_fp64_oracle(B, H, keep, align):
    from danet_densepose2smpl_amd import part_ops
    W = H
    img = orc.make_image(B, H, W, 10 + B)
    th = orc.make_thetas(B, 20 + H)
    sel = _sel()
    k = _keep(B, 3) if keep else None
    k25 = _keep25(B, 4) if keep else None
    x24, body = part_ops.part_gt(img.cuda(), th.cuda(), sel.cuda(), None if k is None else k.cuda(), None if k25 is None else k25.cuda(),
                                 align, body=True)
    torch.cuda.synchronize()
    assert x24.shape == (B * 24, 24, H, W) and x24.dtype == torch.bfloat16
    x = x24.float().cpu().reshape(B, 24, 24, H, W)
    assert torch.count_nonzero(x[:, :, 21:]) == 0
    worst, outside = 0.0, 0
    for b in range(B):
        r, S = orc.forward_sample(img[b].numpy(), th[b].numpy(), sel.numpy(), None if k is None else k[b].numpy(), align)
        err = np.abs(x[b, :, :21].double().numpy() - r)
        bound = 2.0 ** -8 * np.abs(r) + 8 * U32 * S
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        _, _, ix, iy = orc.coords(th[b].numpy(), H, W, align, True)
        outside += int(((ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)).sum())
    record('part_gt_fwd_B%d_H%d_keep%d_align%d' % (B, H, keep, align), {'worst_err_over_bound': worst, 'outside_points': outside})
    assert worst <= 1.0, worst
    assert outside > 0                                   # sampling points outside the image are covered
    # the body operand: iuvmap_clean(keep25 * iuv_img2map(img)), [U | V | I | 5 zeros]
    from danet_densepose2smpl_amd.iuvmap import iuv_img2map, iuvmap_clean
    u, v, i, _ = iuv_img2map(img)
    if k25 is not None:
        k4 = k25.view(B, 25, 1, 1)
        u, v, i = u * k4, v * k4, i * k4
    u, v, i, _ = iuvmap_clean(u, v, i)
    want = torch.cat([u, v, i, torch.zeros(B, 5, H, W)], 1).to(torch.bfloat16)
    assert body.shape == (B, 80, H, W) and torch.equal(body.cpu(), want)


def _bwd_case(B, H, align, seed):
    from danet_densepose2smpl_amd import part_ops
    W = H
    img = orc.make_image(B, H, W, seed)
    th = orc.make_thetas(B, seed + 1)
    sel = _sel()
    k = _keep(B, seed + 2)
    g = torch.randn(B, 24, 21, H, W, generator=torch.Generator().manual_seed(seed + 3))
    # tie pixels (a sampling coordinate within 1e-4 of an integer: the bilinear gradient jumps there) get no upstream gradient
    g = g * torch.from_numpy(~orc.tie_mask(th, H, W, align)).unsqueeze(2)
    g24 = torch.zeros(B, 24, 24, H, W)
    g24[:, :, :21] = g
    g24 = g24.to(torch.bfloat16)                                   # the op's input precision: the oracle uses the same values
    tc = th.cuda().requires_grad_(True)
    x24 = part_ops.part_gt(img.cuda(), tc, sel.cuda(), k.cuda(), None, align)
    x24.backward(g24.reshape(B * 24, 24, H, W).cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    return img, th, sel, k, g24, tc.grad.cpu().double()


@pytest.mark.parametrize('B,H,align', [(1, 64, 1), (3, 56, 1), (3, 64, 0), (8, 64, 1)])
def test_op_backward_vs_fp64_autograd(B, H, align):
    """d theta against fp64 autograd through affine_grid / grid_sample (tests/part_gt_oracle.torch_reference), from the same bf16 g24.
    Bound, per entry, derived from how the kernel computes it (not fitted):
      coordinates: the kernel's fp32 sampling coordinate differs from the exact one by delta (the oracle computes both); gix / giy are
        sums of +-w * s with |d w / d coord| = 1, so they move by <= A * delta (A = sum over taps and channels of |k g src| x dix/dgx);
      arithmetic: ~12 fp32 roundings per pixel term (products, the tap and channel sums): 12 u * A * |base|;
      summation: each thread adds HW / 256 terms in order, then an 8-level butterfly / tree: (HW / 256 + 10) u * sum |term|."""
    img, th, sel, k, g24, got = _bwd_case(B, H, align, seed=100 + B + H + align)
    W = H
    t64 = th.double().requires_grad_(True)
    out = orc.torch_reference(img.double(), t64, sel.long().numpy(), k.double(), bool(align))
    (out.reshape(B, 24, 21, H, W) * g24[:, :, :21].double()).sum().backward()
    ref = t64.grad
    worst = 0.0
    nseq = (H * W + 255) // 256
    for b in range(B):
        _, T, A = orc.dtheta_sample(img[b].numpy(), th[b].numpy(), sel.numpy(), g24[b, :, :21].double().numpy(), k[b].numpy(), align, False)
        xn, yn, ix64, iy64 = orc.coords(th[b].numpy(), H, W, align, False)
        _, _, ix32, iy32 = orc.coords(th[b].numpy(), H, W, align, True)
        delta = np.abs(ix32 - ix64) + np.abs(iy32 - iy64)                          # [24,H,W]
        base = [np.abs(xn).reshape(1, 1, W) + 0 * delta, np.abs(yn).reshape(1, H, 1) + 0 * delta, np.ones_like(delta)] * 2
        bound = np.stack([(A * (delta + 12 * U32) * bs).sum((1, 2)) for bs in base], 1) + (nseq + 10) * U32 * T
        err = np.abs(got[b].reshape(24, 6).numpy() - ref[b].reshape(24, 6).numpy())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    record('part_gt_bwd_B%d_H%d_align%d' % (B, H, align), {'worst_err_over_bound': worst,
                                                           'max_abs_err': float((got - ref).abs().max()), 'scale': float(ref.abs().max())})
    assert worst <= 1.0, worst


def test_op_reproducible_eager_and_graph():
    from danet_densepose2smpl_amd import part_ops
    B, H = 32, 64
    img = orc.make_image(B, H, H, 1).cuda()
    th = orc.make_thetas(B, 2).cuda()
    sel = _sel().cuda()
    k = _keep(B, 3).cuda()
    k25 = _keep25(B, 4).cuda()
    g24 = torch.randn(B * 24, 24, H, H, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last)

    def run():
        t = th.clone().requires_grad_(True)
        x, body = part_ops.part_gt(img, t, sel, k, k25, True, body=True)
        x.backward(g24)
        return x.detach().clone(), body.clone(), t.grad.clone()

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    tt = th.clone().requires_grad_(True)
    with torch.cuda.graph(graph):
        x, body = part_ops.part_gt(img, tt, sel, k, k25, True, body=True)
        x.backward(g24)
    reps = []
    for _ in range(2):
        tt.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        reps.append((x.detach().clone(), body.clone(), tt.grad.clone()))
    for r in reps:
        for u, v in zip(a, r):
            assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------------------
def _port(B, train):
    """The project's IUV_Estimator ('iuv_gt') and DecomposedPredictor with g23's parameters."""
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    from danet_densepose2smpl_amd.smpl_regressor import DecomposedPredictor
    _cfg(**{'DANET.INPUT_MODE': 'iuv_gt', 'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.STN_CENTER_JITTER': 0.,
            'DANET.STN_SCALE_JITTER': 0., 'DANET.PARTDROP_RATE': 0.})
    g = golden('g23_iuvgt_b32' if B == 32 else 'g23_iuvgt_%s' % ('train' if train else 'eval'))
    est = IUV_Estimator(pretrained=False)
    with torch.no_grad():
        est.learned_ratio.copy_(torch.from_numpy(g['ratio']))
        est.learned_offset.copy_(torch.from_numpy(g['offset']))
    pose6 = torch.tensor([1., 0., 0., 1., 0., 0.]).repeat(24).unsqueeze(0)
    pred = DecomposedPredictor(None, (torch.tensor([[0.9, 0., 0.]]), torch.zeros(1, 10), pose6), pretrained=False)
    formula_params(pred, skip=SKIP)
    return est.cuda().train(train), pred.cuda().train(train), g


def _path(est, pred, B, train, fp32):
    from danet_densepose2smpl_amd import conv, part_ops
    from danet_densepose2smpl_amd.iuvmap import iuv_img2map, iuvmap_clean
    import contextlib
    _, gt, kps = g19_inputs(B, 64)
    gt, kps = gt.cuda(), kps.cuda()
    with (conv.precision('fp32') if fp32 else contextlib.nullcontext()), torch.set_grad_enabled(train):
        rd = est(None, gt, kps, part_clean=None if fp32 else (None,))
        if fp32:
            u, v, i, _ = iuvmap_clean(*iuv_img2map(gt))
            out = pred(torch.cat([u, v, i], 1), rd['part_iuv_gt'])
        else:
            part = part_ops.padded_part_view(rd['part_x24'])
            part._nhwc_padded = rd['part_x24']
            out = pred(rd['iuv_map'], part)
        if train:
            para = out['para'].float()
            loss = (para * loss_weights(para.cpu()).to(para.device)).sum() + sum(t.float().sum() for t in out['joint_position']) + out['joint_rotation'][0].float().sum()
            loss.backward()
            conv.flush_wgrads()
    torch.cuda.synchronize()
    return out


def _bn_fp64_two_pass(self, x, res=None, relu=False, link=None):
    """A training-mode BatchNorm with exact statistics (torch, fp64, two-pass variance): isolates the crops' gradient path from the
    project's fp32 BatchNorm, whose one-pass shifted variance loses digits on these piecewise-constant inputs."""
    import torch.nn.functional as F
    C = self.num_features
    y = F.batch_norm(x[:, :C].double(), None, None, self.weight.double(), self.bias.double(), True, 0.1, self.eps).float()
    if res is not None:
        y = y + res[:, :C].float()
    return F.relu(y) if relu else y


@pytest.mark.parametrize('mode', ['fp32', 'fp32_exact_bn', 'bf16'])
def test_path_vs_reference_g23_b32(mode, monkeypatch):
    B = 32
    est, pred, g = _port(B, True)
    if mode == 'fp32_exact_bn':
        from danet_densepose2smpl_amd import nn as dnn
        monkeypatch.setattr(dnn.BatchNorm2d, 'forward', _bn_fp64_two_pass)
    out = _path(est, pred, B, True, mode != 'bf16')
    para = out['para'].detach().float().cpu().numpy()
    rel = lambda a, r: float(np.abs(a - r).max() / np.abs(r).max())     # noqa: E731
    cos = lambda a, r: float((a * r).sum() / (np.linalg.norm(a) * np.linalg.norm(r)))     # noqa: E731
    dr, do = est.learned_ratio.grad.cpu().numpy(), est.learned_offset.grad.cpu().numpy()
    meas = {'para': rel(para, g['para64']), 'd_ratio': rel(dr, g['d_ratio64']), 'd_offset': rel(do, g['d_offset64']),
            'cos_d_ratio': cos(dr, g['d_ratio64']), 'cos_d_offset': cos(do, g['d_offset64']),
            'floor_para': float(g['floor__para']), 'floor_d_ratio': float(g['floor__d_ratio']), 'floor_d_offset': float(g['floor__d_offset'])}
    pd = dict(pred.named_parameters())
    for key in g.files:
        if key.startswith('grad64__'):
            n = key[8:]
            gw = g19_grad_sample(pd[n.replace('__', '.')].grad.float()).cpu().numpy()
            meas['grad__' + n] = rel(gw, g[key])
            meas['floor_grad__' + n] = float(g['floor__grad__' + n])
    record('iuv_gt_path_b32_%s_vs_reference' % mode, meas)
    rz = g['relu_zero']
    assert dr[int(rz[0])] == 0.0 and do[int(rz[1])] == 0.0
    assert np.isfinite(dr).all() and np.isfinite(do).all()
    if mode == 'fp32_exact_bn':
        # with exact BatchNorm statistics every compared quantity is within a small multiple of the reference's own fp32-vs-fp64
        # distance (measured on MI355X: 0.46x / 0.50x for d ratio / d offset, 0.61x / 0.84x / 0.95x for the three sentinel gradients)
        for k in ('para', 'd_ratio', 'd_offset') + tuple(k for k in meas if k.startswith('grad__')):
            fl = meas['floor_' + k]
            assert meas[k] <= 3 * fl + 1e-6, (k, meas)
    elif mode == 'fp32':
        # para: within a small multiple of the reference's fp32 floor (measured 1.07x).  The gradients through the two ResNets are
        # further off (measured d ratio / d offset 0.035 / 0.039, body layer4 0.055): the cause is the project's fp32 BatchNorm, whose
        # one-pass shifted variance E[(x-k)^2] - E[x-k]^2 (csrc/norm_act.hip) cancels on these piecewise-constant label inputs --
        # the same run with exact statistics ('fp32_exact_bn') is at the floor.  Bounded here at the measured level with margin.
        assert meas['para'] <= 10 * meas['floor_para'] + 1e-6, meas
        assert meas['d_ratio'] <= 0.06 and meas['d_offset'] <= 0.06, meas
        assert meas['grad__body_net__3__layer4__1__conv2__weight'] <= 0.08, meas
    else:
        # bf16 operands through two ResNets; measured on MI355X: para 0.018 of scale; d ratio / d offset cosines 0.990 / 0.989, their
        # max deviations 1.18 / 1.36 of scale (a few small entries: d ratio is a sum with heavy cancellation, and the limb net's bf16
        # backward is noisy -- g20's limb_net.0 gradient has cosine 0.89)
        assert meas['para'] <= 5e-2, meas
        assert meas['cos_d_ratio'] > 0.95 and meas['cos_d_offset'] > 0.95, meas


def test_infer_net_vs_reference_g23_eval():
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    est, pred, g = _port(4, False)
    torch.manual_seed(0)
    model = DaNet(default_options(4), None, pretrained=False)
    model.img2iuv.load_state_dict(est.state_dict())
    model.iuv2smpl.smpl_para_Outs.load_state_dict(pred.state_dict())
    model = model.cuda().eval()
    img, gt, kps = g19_inputs(4, 64)
    rd = model.infer_net((img.cuda(), gt.cuda(), kps.cuda()))
    d = float(np.abs(rd['para'].float().cpu().numpy() - g['para64']).max() / np.abs(g['para64']).max())
    # the same path in fp32 mode
    from danet_densepose2smpl_amd import conv
    with conv.precision('fp32'):
        rd32 = model.infer_net((img.cuda(), gt.cuda(), kps.cuda()))
    d32 = float(np.abs(rd32['para'].float().cpu().numpy() - g['para64']).max() / np.abs(g['para64']).max())
    record('iuv_gt_infer_net_vs_g23_eval', {'bf16': d, 'fp32': d32, 'floor': float(g['floor__para'])})
    assert d32 <= 10 * float(g['floor__para']) + 1e-6, d32
    assert d <= 5e-2, d


def test_train_step_eager_and_captured():
    _cfg(**{'DANET.INPUT_MODE': 'iuv_gt', 'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.PARTDROP_RATE': 0.,
            'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0.})
    from danet_densepose2smpl_amd.trainer import Trainer, synthetic_in_dict, default_options
    dev = torch.device('cuda')
    torch.manual_seed(0)
    tr = Trainer(default_options(32), device=dev, distributed=False, lr=1e-30)
    batch = synthetic_in_dict(tr.model, 32, dev, seed=3)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        _, le = tr.train_step(batch)
        runs.append({k: float(v.sum()) for k, v in le.items()})
    e = runs[0]
    torch.manual_seed(11)
    tr.capture(batch, warmup=1)
    torch.manual_seed(11)
    _, l1 = tr.train_step_graphed()
    g1 = {k: float(v.sum()) for k, v in l1.items()}
    torch.cuda.synchronize()
    # exactly the reference's regressor-only loss set (smpl_regressor.py:139-226 in the default configuration: gcn with intermediate
    # position supervision, ORTHOGONAL_WEIGHTS = 0): no estimator loss
    want = {'joint_rotation0', 'joint_position0', 'joint_position1', 'keypoints_2d', 'keypoints_3d', 'smpl_pose', 'smpl_betas',
            'smpl_verts', 'cam'}
    assert set(e) == want, sorted(e)
    assert set(g1) == want
    record('train_step_iuv_gt', {'eager': e, 'graph': g1, 'keys': sorted(e)})
    for k in e:
        assert np.isfinite(e[k]) and np.isfinite(g1[k]), (k, e[k], g1[k])
        # lr 1e-30: the replayed step runs the same kernels on the same data as the eager ones (measured on MI355X: identical)
        assert runs[1][k] == e[k], (k, runs)
        assert abs(g1[k] - e[k]) <= 2 * np.spacing(np.float32(abs(e[k]))), (k, e[k], g1[k])


def test_adam_moves_the_crop_ratios():
    _cfg(**{'DANET.INPUT_MODE': 'iuv_gt', 'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.PARTDROP_RATE': 0.,
            'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0.})
    from danet_densepose2smpl_amd.trainer import Trainer, synthetic_in_dict, default_options
    dev = torch.device('cuda')
    torch.manual_seed(0)
    lr = 1e-3
    tr = Trainer(default_options(8), device=dev, distributed=False, lr=lr)
    est = tr.model.img2iuv
    assert any(p is est.learned_ratio for p in tr.params) and any(p is est.learned_offset for p in tr.params)
    batch = synthetic_in_dict(tr.model, 8, dev, seed=4)
    p0 = [est.learned_ratio.detach().clone(), est.learned_offset.detach().clone()]
    tr.train_step(batch)
    torch.cuda.synchronize()
    b1, b2, eps = 0.9, 0.999, 1e-8
    for p, before in zip((est.learned_ratio, est.learned_offset), p0):
        g = p.grad.detach().cpu().numpy().astype(np.float32)
        assert np.count_nonzero(g) >= 20
        # Adam's first step (csrc/adam.hip, torch.optim.Adam's formula) in fp32 on the host
        f = np.float32
        m, v = (f(1) - f(b1)) * g, (f(1) - f(b2)) * g * g
        step_size, inv_sqrt_bc2 = f(lr) / (f(1) - f(b1)), f(1) / np.sqrt(f(1) - f(b2))
        want = before.cpu().numpy() - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + f(eps))
        got = p.detach().cpu().numpy()
        assert np.abs(got - before.cpu().numpy()).max() > 0.5 * lr
        assert np.abs(got - want).max() <= 4 * np.spacing(np.abs(want)).max(), np.abs(got - want).max()


def test_default_mode_never_calls_the_new_op(monkeypatch):
    from danet_densepose2smpl_amd import part_ops
    _cfg(**{'DANET.INIMG_SIZE': 128, 'DANET.HEATMAP_SIZE': 32, 'DANET.IUV_REGRESSOR': 'resnet'})

    def boom(*a, **k):
        raise AssertionError('part_gt called in the default mode')
    monkeypatch.setattr(part_ops, 'part_gt', boom)
    monkeypatch.setattr(part_ops.PartGtFunction, 'apply', boom)
    calls = []
    orig = part_ops.part_joint
    monkeypatch.setattr(part_ops, 'part_joint', lambda *a, **k: calls.append(1) or orig(*a, **k))
    from danet_densepose2smpl_amd.trainer import Trainer, synthetic_in_dict, default_options
    dev = torch.device('cuda')
    torch.manual_seed(0)
    tr = Trainer(default_options(2), device=dev, distributed=False, lr=1e-30)
    _, le = tr.train_step(synthetic_in_dict(tr.model, 2, dev, seed=5))
    torch.cuda.synchronize()
    assert calls, 'the default train step no longer takes part_joint'
    assert 'loss_pU' in le and all(np.isfinite(float(v.sum())) for v in le.values())
