"""Generates the fixtures of the LSTM refinement strategies (DANET.REFINE_STRATEGY 'lstm' / 'lstm_direct') by IMPORTING the
reference, like make_golden.py (whose parameter and input formulas it reuses): g21_predictor_lstm*.npz (B = 4, train and eval) and
g22_predictor_lstm_b32.npz (B = 32, 'lstm' train pass, forward and backward).  Re-run:  python tests/golden/make_golden_refine.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref_env, formula_params, g19_grad_sample, g20_inputs, save   # noqa: E402

SKIP = ('mean_',)
ENV = {'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64}


def _mean():
    pose6 = torch.tensor([1., 0., 0., 1., 0., 0.]).repeat(24).unsqueeze(0)
    return torch.tensor([[0.9, 0., 0.]]), torch.zeros(1, 10), pose6


def _build(strategy, dt):
    ref_env(dict(ENV, **{'DANET.REFINE_STRATEGY': strategy}))
    from models.danet.smpl_regressor import DecomposedPredictor
    torch.manual_seed(0)
    net = DecomposedPredictor(None, _mean(), pretrained=False)
    formula_params(net, skip=SKIP)
    return net.to(dt)


def _taps(net, strategy):
    taps = {}
    hs = [net.limb_reslayer.register_forward_hook(lambda m, i, o: taps.__setitem__('rot_feats', o.detach())),
          net.pose_regressors[1].register_forward_pre_hook(lambda m, i: taps.__setitem__('prehead', i[0].detach()))]
    if strategy == 'lstm':
        hs.append(net.pos2rot[0].register_forward_pre_hook(lambda m, i: taps.__setitem__('tri', i[0].detach())))
    return taps, hs


def _run(strategy, train, B, backward=False, grad_names=()):
    iuv, part = g20_inputs(B)
    res = {}
    for dt in (torch.float64, torch.float32):
        net = _build(strategy, dt)
        net.train(train)
        taps, hs = _taps(net, strategy)
        torch.set_default_dtype(dt)
        try:
            with torch.set_grad_enabled(backward):
                rd = net(iuv.to(dt), part.to(dt))
                if backward:
                    w = torch.cos(torch.arange(rd['para'].numel(), dtype=dt).view_as(rd['para']) * 0.37)
                    loss = (rd['para'] * w).sum() + sum(t.sum() for t in rd.get('joint_position', [])) + \
                        sum(t.sum() for t in rd['joint_rotation'])
                    loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        for h in hs:
            h.remove()
        out = {'para': rd['para'].detach()}
        for i, t in enumerate(rd['joint_rotation']):
            out['jr%d' % i] = t.detach()
        for i, t in enumerate(rd.get('joint_position', [])):
            out['jp%d' % i] = t.detach()
        nb = B
        out['rot_feats'] = taps['rot_feats'].reshape(nb, 24, -1)
        out['prehead'] = taps['prehead'].reshape(nb, 24, -1)
        if 'tri' in taps:
            out['tri'] = taps['tri'].reshape(24, nb, -1).transpose(0, 1)         # [B,24,768]
        pd = dict(net.named_parameters())
        res[dt] = (out, {n: pd[n].grad.clone() for n in grad_names}, net)
    return res


def _keys(net):
    sd = net.state_dict()
    shapes = np.full((len(sd), 4), -1, np.int64)
    for i, t in enumerate(sd.values()):
        shapes[i, :t.dim()] = t.shape
    return np.array(list(sd.keys())), shapes


def _degeneracy(out):
    """How much of pos' is the LSTM's contribution: |pos' - cat(pos, pos)| / |pos'| (pos' = the input of the final head)."""
    pos = out['rot_feats'] if 'tri' not in out else None
    ref = out['prehead'] if 'tri' not in out else out['tri'][:, :, 256:512]
    if pos is None:
        return None
    return float((ref - torch.cat([pos, pos], 2)).norm() / ref.norm())


def g21():
    for strategy in ('lstm', 'lstm_direct'):
        for train in (True, False):
            res = _run(strategy, train, 4)
            out64, _, net = res[torch.float64]
            out32 = res[torch.float32][0]
            arrs = {k: v.float() for k, v in out64.items()}
            for k in out64:
                arrs['floor__' + k] = (out32[k].double() - out64[k]).abs().max().float()
            keys, shapes = _keys(net)
            arrs['sd_keys'], arrs['sd_shapes'] = keys, shapes
            name = 'g21_predictor_%s_%s' % (strategy, 'train' if train else 'eval')
            print(name, {k: round(float(v), 6) for k, v in arrs.items() if k.startswith('floor__')}, 'lstm share', _degeneracy(out64))
            for k in ('rot_feats', 'prehead', 'tri'):
                if k in arrs:
                    arrs[k] = arrs[k].numpy()
            save(name, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()})


G22_NAMES = ('limb_lstm.0.1.weight_hh_l0', 'limb_lstm.0.0.weight_ih_l0_reverse', 'rot2pos.0.9.0.weight', 'pos2rot.0.3.weight',
             'pose_regressors.1.1.weight')


def g22():
    res = _run('lstm', True, 32, backward=True, grad_names=G22_NAMES)
    out64, g64, _ = res[torch.float64]
    out32, g32, _ = res[torch.float32]
    arrs = {}
    for k in ('para', 'jr0', 'jp0', 'jp1'):
        arrs[k] = out64[k].float().numpy()
        arrs['floor__' + k] = (out32[k].double() - out64[k]).abs().max().float().numpy()
        print(k, 'fp32 vs fp64 reference: max abs %.3g' % float(arrs['floor__' + k]))
    for n in G22_NAMES:
        key = n.replace('.', '__')
        arrs['grad64__' + key] = g19_grad_sample(g64[n].float()).numpy()
        arrs['gfloor__' + key] = ((g32[n].double() - g64[n]).abs().max() / g64[n].abs().max()).float().numpy()
        print(n, 'fp32 reference gradient vs fp64: %.3g of scale' % float(arrs['gfloor__' + key]))
    save('g22_predictor_lstm_b32', **arrs)


def check_stack2():
    """STACK_NUM = 2 fails in the reference itself for both strategies (why the port refuses it)."""
    iuv, part = g20_inputs(2)
    for strategy, train in (('lstm_direct', False), ('lstm', True)):
        ref_env(dict(ENV, **{'DANET.REFINE_STRATEGY': strategy, 'DANET.REFINEMENT.STACK_NUM': 2}))
        from models.danet.smpl_regressor import DecomposedPredictor
        net = DecomposedPredictor(None, _mean(), pretrained=False).train(train)
        try:
            with torch.no_grad():
                net(iuv, part)
            print(strategy, 'STACK_NUM=2: ran')
        except Exception as e:      # noqa: BLE001 -- reporting what the reference does
            print(strategy, 'STACK_NUM=2: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:160]))
    ref_env(dict(ENV, **{'DANET.REFINEMENT.STACK_NUM': 1}))


if __name__ == '__main__':
    which = sys.argv[1:] or ['check_stack2', 'g21', 'g22']
    for w in which:
        globals()[w]()
