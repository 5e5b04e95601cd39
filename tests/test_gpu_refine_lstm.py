"""REFINE_STRATEGY 'lstm' / 'lstm_direct' on the device: the LSTM tree op (csrc/lstm_tree.hip) against the fp64 oracle
(tests/lstm_oracle.py, torch's nn.LSTM on the CPU) -- values and every gradient --, its bitwise reproducibility eager and under graph
replay, the predictor against the reference's own results (g21, g22), full train steps eager and captured, the inference engine, and
that nothing runs torch's LSTM."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, record

sys.path.insert(0, GOLDEN)
from make_golden import formula_params, g19_grad_sample, g20_inputs    # noqa: E402
from lstm_oracle import lstm_tree_ref, make_lstms    # noqa: E402

pytestmark = pytest.mark.gpu


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
    dnn.ONEPASS_STREAM = prev           # (a Trainer confines the one-pass launches to its own stream: later tests expect the default)


def _lstms(seed):
    from danet_densepose2smpl_amd.lstm_tree import LimbLSTM
    torch.manual_seed(seed)
    return [LimbLSTM(128, 128) for _ in range(5)]


def _op_case(B, seed=0):
    from danet_densepose2smpl_amd.lstm_tree import lstm_tree
    mods = _lstms(seed)
    g = torch.Generator().manual_seed(seed + 1)
    pos = torch.randn(B, 24, 128, generator=g) * 0.7
    wout = torch.randn(B, 24, 256, generator=g)
    # fp64 oracle on the CPU
    ref_mods = make_lstms([m.state_dict() for m in mods])
    p64 = pos.double().requires_grad_(True)
    r64 = lstm_tree_ref(p64, ref_mods)
    (r64 * wout.double()).sum().backward()
    # the op
    dmods = [m.cuda() for m in mods]
    pd = pos.cuda().requires_grad_(True)
    out = lstm_tree(pd, dmods)
    (out * wout.cuda()).sum().backward()
    torch.cuda.synchronize()
    meas = {'fwd_max_abs': float((out.detach().cpu().double() - r64.detach()).abs().max()),
            'dpos_rel_max': float((pd.grad.cpu().double() - p64.grad).abs().max() / p64.grad.abs().max())}
    worst = 0.0
    n = 0
    for m, rm in zip(dmods, ref_mods):
        got = dict(m.named_parameters())
        for name, p in rm.named_parameters():
            ga, gr = got[name].grad.cpu().double(), p.grad
            worst = max(worst, float((ga - gr).abs().max() / gr.abs().max()))
            n += 1
    meas['param_grad_rel_max'] = worst
    meas['n_param_grads'] = n
    return meas


@pytest.mark.parametrize('B', [1, 3, 32, 33])
def test_op_matches_fp64_oracle(B):
    meas = _op_case(B, seed=B)
    record('lstm_tree_op_vs_fp64_B%d' % B, meas)
    assert meas['n_param_grads'] == 40
    # fp32 FMA chains of 128 terms through <= 10 dependent steps: a few 1e-6 is the expected size
    assert meas['fwd_max_abs'] < 1e-4, meas
    assert meas['dpos_rel_max'] < 1e-4 and meas['param_grad_rel_max'] < 1e-4, meas


def test_op_is_bitwise_reproducible_eager_and_under_graph_replay():
    from danet_densepose2smpl_amd.lstm_tree import lstm_tree
    mods = [m.cuda() for m in _lstms(7)]
    g = torch.Generator().manual_seed(3)
    pos = (torch.randn(32, 24, 128, generator=g) * 0.7).cuda()
    wout = torch.randn(32, 24, 256, generator=g).cuda()
    params = [p for m in mods for p in m.parameters()]

    def run(x):
        for p in params:
            p.grad = None
        xr = x.detach().requires_grad_(True)
        out = lstm_tree(xr, mods)
        (out * wout).sum().backward()
        return [out.detach().clone(), xr.grad.clone()] + [p.grad.clone() for p in params]

    a = run(pos)
    b = run(pos)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    static = pos.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)                                   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for p in params:
        p.grad = None
    with torch.cuda.graph(graph):
        xr = static.detach().requires_grad_(True)
        out = lstm_tree(xr, mods)
        (out * wout).sum().backward()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    c = [out, xr.grad] + [p.grad for p in params]
    assert all(torch.equal(u, v) for u, v in zip(a, c))


def _port_predictor(strategy, train):
    from danet_densepose2smpl_amd.smpl_regressor import DecomposedPredictor
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.REFINE_STRATEGY': strategy})
    pose6 = torch.tensor([1., 0., 0., 1., 0., 0.]).repeat(24).unsqueeze(0)
    net = DecomposedPredictor(None, (torch.tensor([[0.9, 0., 0.]]), torch.zeros(1, 10), pose6), pretrained=False)
    formula_params(net, skip=('mean_',))
    return net.cuda().train(train)


def _outs(rd):
    o = {'para': rd['para']}
    for i, t in enumerate(rd['joint_rotation']):
        o['jr%d' % i] = t
    for i, t in enumerate(rd.get('joint_position', [])):
        o['jp%d' % i] = t
    return o


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
@pytest.mark.parametrize('train', [True, False])
def test_predictor_vs_reference_g21(strategy, train, mode):
    import contextlib
    from danet_densepose2smpl_amd import conv
    g = golden('g21_predictor_%s_%s' % (strategy, 'train' if train else 'eval'))
    net = _port_predictor(strategy, train)
    iuv, part = (t.cuda() for t in g20_inputs(4))
    with (conv.precision('fp32') if mode == 'fp32' else contextlib.nullcontext()), torch.no_grad():
        rd = net(iuv, part)
    torch.cuda.synchronize()
    outs = _outs(rd)
    keys = [k for k in g.files if k in ('para', 'jr0', 'jp0', 'jp1')]
    assert sorted(outs) == sorted(keys)
    meas = {k: {'max_abs': float(np.abs(outs[k].float().cpu().numpy() - g[k]).max()), 'reference_fp32_floor': float(g['floor__' + k])}
            for k in keys}
    record('predictor_g21_%s_%s_%s' % (strategy, 'train' if train else 'eval', mode), meas)
    if mode == 'fp32':
        # measured on MI355X: within 1.2 x the reference's own floor except 'lstm' train, where BatchNorm over 4 rows through the 9
        # rot2pos levels amplifies rounding (the reference's fp32 floor is 0.009 there): 3.1 x
        assert all(meas[k]['max_abs'] <= max(5.0 * meas[k]['reference_fp32_floor'], 2e-4) for k in keys), meas
    elif strategy == 'lstm' and train:
        # (bf16 activations through those same 4-row BatchNorms: measured 0.83 on para -- only the head before them is compared)
        assert meas['jr0']['max_abs'] < 0.1 and all(np.isfinite(meas[k]['max_abs']) for k in keys), meas
    else:
        assert all(meas[k]['max_abs'] < 0.15 for k in keys), meas           # measured <= 0.035


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_predictor_train_pass_vs_reference_g22(mode):
    import contextlib
    from danet_densepose2smpl_amd import conv
    g = golden('g22_predictor_lstm_b32')
    net = _port_predictor('lstm', True)
    iuv, part = (t.cuda() for t in g20_inputs())
    with (conv.precision('fp32') if mode == 'fp32' else contextlib.nullcontext()):
        rd = net(iuv, part)
        w = torch.cos(torch.arange(rd['para'].numel(), dtype=torch.float32, device='cuda').view_as(rd['para']) * 0.37)
        loss = (rd['para'].float() * w).sum() + sum(t.float().sum() for t in rd['joint_position']) + rd['joint_rotation'][0].float().sum()
        loss.backward()
        conv.flush_wgrads()
    torch.cuda.synchronize()
    outs = _outs(rd)
    meas = {k: {'max_abs': float(np.abs(outs[k].detach().float().cpu().numpy() - g[k]).max()), 'reference_fp32_floor': float(g['floor__' + k])}
            for k in ('para', 'jr0', 'jp0', 'jp1')}
    pd = dict(net.named_parameters())
    grads = []
    for k in g.files:
        if k.startswith('grad64__'):
            gw = g19_grad_sample(pd[k[8:].replace('__', '.')].grad.float()).cpu().flatten().double()
            r = torch.from_numpy(g[k]).flatten().double()
            meas['grad__' + k[8:]] = {'rel_max': float((gw - r).abs().max() / r.abs().max()), 'cos': float((gw * r).sum() / (gw.norm() * r.norm())),
                                      'norm_ratio': float(gw.norm() / r.norm()), 'reference_fp32_floor': float(g['gfloor__' + k[8:]])}
            grads.append('grad__' + k[8:])
    record('predictor_g22_lstm_b32_%s' % mode, meas)
    assert len(grads) == 5
    outk = ('para', 'jr0', 'jp0', 'jp1')
    if mode == 'fp32':
        # measured on MI355X: outputs within 3.7 x the reference's floor (para 3.9e-4 against 3.6e-4); gradient samples within 3.4 x
        # their floor in max relative error (LSTM 1.6e-3 / 9.3e-3), cosines >= 0.99988
        assert all(meas[k]['max_abs'] <= max(3.0 * meas[k]['reference_fp32_floor'], 2e-4) for k in outk), meas
        assert all(meas[k]['rel_max'] <= max(5.0 * meas[k]['reference_fp32_floor'], 5e-3) and meas[k]['cos'] > 0.9998 for k in grads), meas
    else:
        # bf16 activations through 9 levels of per-joint MLPs with BatchNorm: measured para 0.42, positions 0.29, rotation 0.061; LSTM
        # and head gradient cosines 0.91 .. 0.99, the deep rot2pos / pos2rot gradients 0.37 / 0.85 (norms within 10 %)
        assert all(meas[k]['max_abs'] < 0.6 for k in outk), meas
        assert all(0.85 < meas[k]['norm_ratio'] < 1.15 for k in grads), meas
        assert all(meas[k]['cos'] > 0.85 for k in grads if 'rot2pos' not in k and 'pos2rot' not in k), meas


@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
def test_train_step_eager_and_captured(strategy):
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.PARTDROP_RATE': 0., 'DANET.REFINE_STRATEGY': strategy,
            'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0.})
    from danet_densepose2smpl_amd.trainer import Trainer, synthetic_in_dict, default_options
    dev = torch.device('cuda')
    torch.manual_seed(0)
    tr = Trainer(default_options(32), device=dev, distributed=False, lr=1e-30)
    batch = synthetic_in_dict(tr.model, 32, dev, seed=3)
    runs = []
    for _ in range(2):
        _, le = tr.train_step(batch)
        runs.append({k: float(v.sum()) for k, v in le.items()})
    e = runs[0]
    spread = {k: abs(runs[0][k] - runs[1][k]) for k in e}
    tr.capture(batch, warmup=1)
    _, l1 = tr.train_step_graphed()
    g1 = {k: float(v.sum()) for k, v in l1.items()}
    torch.cuda.synchronize()
    want = {'joint_rotation0', 'joint_position0', 'joint_position1'} if strategy == 'lstm' else {'joint_rotation0'}
    assert want <= set(e) and not ({'joint_position0', 'joint_position1'} - want) & set(e)
    assert set(g1) == set(e)
    record('train_step_%s' % strategy, {'eager': e, 'graph': g1})
    for k in e:
        assert np.isfinite(e[k]) and np.isfinite(g1[k]), (k, e[k], g1[k])
        assert min(abs(g1[k] - r[k]) for r in runs) <= 5e-2 * abs(e[k]) + 2 * spread[k] + 1e-4, (k, e[k], g1[k], spread[k])


@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
def test_inference_engine(strategy):
    from danet_densepose2smpl_amd import conv
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.IUV_REGRESSOR': 'resnet', 'DANET.REFINE_STRATEGY': strategy})
    B = 4
    torch.manual_seed(0)
    model = DaNet(default_options(B), None, pretrained=False).cuda().eval()
    img = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(2)).cuda()
    ref = model.infer_net(img)
    eng = model.inference_engine(B)
    conv.TRACE = []
    try:
        eager = eng.eager(img)['para'].clone()
        trace = list(conv.TRACE)
    finally:
        conv.TRACE = None
    assert not [t for t in trace if t[0].startswith('bn')], trace[:3]
    out = eng(img)['para']
    assert torch.equal(out, eager)
    d = (out - ref['para']).abs().max().item()
    record('infer_engine_%s' % strategy, {'para_max_abs': d, 'launches': dict(eng.launches)})
    # measured on MI355X: 6.3e-5 ('lstm') and 1.9e-5 ('lstm_direct') -- bf16 rounding of the folded w * s, as for 'gcn'
    assert d < 1e-3, d
    eng.close()


@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
def test_torch_lstm_never_runs(strategy, monkeypatch):
    def boom(*a, **k):
        raise AssertionError('torch.nn.LSTM.forward called')
    monkeypatch.setattr(torch.nn.LSTM, 'forward', boom)
    net = _port_predictor(strategy, True)
    iuv, part = g20_inputs(2)
    rd = net(iuv.cuda().requires_grad_(True), part.cuda().requires_grad_(True))
    loss = rd['para'].float().sum() + sum(t.float().sum() for t in rd['joint_rotation'])
    loss.backward()
    torch.cuda.synchronize()
    assert all(m.weight_hh_l0.grad is not None and torch.isfinite(m.weight_hh_l0.grad).all() for m in net.limb_lstm[0])
