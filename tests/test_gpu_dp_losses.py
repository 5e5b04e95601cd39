"""iuv_ops.dp_point_losses (csrc/dp_losses.hip): the DensePose point supervision as one launch per pass, against the reference's
golden vectors (g11), against IUV_Estimator.dp_uvia_losses in float64 on edge cases, its determinism, graph capture and wiring."""
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSSES = ('loss_Udp', 'loss_Vdp', 'loss_IndexUVdp', 'loss_segAnndp')


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(kw)


def _padded(t, ld):
    """[B,C,S,S] -> the conv epilogue's zero-padded fp32 NHWC tensor seen as [B,ld,S,S] (what iuv_ops._rows takes as it is)."""
    B, C, H, W = t.shape
    buf = torch.zeros(B, H, W, ld, dtype=torch.float32, device=t.device)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)


def _run_op(preds, dp, has_dp, align, weights=(1., 2., 3., 4.), padded=False):
    """-> (four losses as floats, the four gradients at [B,25|15,S,S]) of iuv_ops.dp_point_losses."""
    from danet_densepose2smpl_amd import iuv_ops
    ins = []
    for t, ld in zip(preds, (32, 32, 32, 16)):
        t = t.detach().to(DEV)
        ins.append((_padded(t, ld) if padded else t.clone()).requires_grad_(True))
    out = iuv_ops.dp_point_losses(*ins, {k: v.to(DEV) for k, v in dp.items()}, None if has_dp is None else has_dp.to(DEV), bool(align))
    assert all(o.shape == (1,) and o.dtype == torch.float32 for o in out)
    sum(o * w for o, w in zip(out, weights)).sum().backward()
    grads = [t.grad for t in ins]
    if padded:
        for g, n in zip(grads, (25, 25, 25, 15)):
            assert g.shape[1] in (32, 16) and float(g[:, n:].abs().max()) == 0.0          # gradients at padded width, pad channels zero
        grads = [g[:, :n] for g, n in zip(grads, (25, 25, 25, 15))]
    return [float(o.detach()) for o in out], [g.detach().cpu() for g in grads]


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('align', [0, 1])
def test_dp_point_losses_vs_reference_golden(align, padded):
    """Golden g11 (B = 4, S = 16, has_dp = [1,0,1,1], 150 used slots, loss weights 1, 2, 3, 4) with the bounds tests/test_host_logic.py
    holds the torch form to; plain [B,25,S,S] inputs and padded-base inputs."""
    _cfg(**{'DANET.HEATMAP_SIZE': 16})
    g = golden('g11_dp_losses_align%d' % align)
    preds = [torch.from_numpy(g[k]) for k in ('u', 'v', 'idx', 'ann')]
    dp = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('dp__')}
    has_dp = torch.from_numpy(g['has_dp'])
    losses, grads = _run_op(preds, dp, has_dp, align, padded=padded)
    for ours, k in zip(losses, LOSSES):
        print('%s ours %.8g golden %.8g' % (k, ours, float(g[k])))
        assert abs(ours - float(g[k])) <= 1e-5 * max(1.0, abs(float(g[k]))), k
    for t, k in zip(grads, ('gu', 'gv', 'gidx', 'gann')):
        print('%s max err %.3e of %.3e' % (k, np.abs(t.numpy() - g[k]).max(), np.abs(g[k]).max()))
        np.testing.assert_allclose(t.numpy(), g[k], atol=1e-6 + 1e-5 * np.abs(g[k]).max())
        assert float(t[1].abs().max()) == 0.0, k                        # sample 1 has no labels: exactly zero rows
    # no labelled sample at all: four exact zeros and zero gradients (iuv_estimator.py:118-121)
    losses, grads = _run_op(preds, dp, torch.zeros(4), align, padded=padded)
    assert losses == [0.0] * 4
    assert all(float(t.abs().max()) == 0.0 for t in grads)


def _edge_case(S=64, B=3, seed=7):
    """Seeded edge inputs: exact integer coordinates, points within half a pixel of every border (taps outside the map), eight points
    sharing one pixel, a sample with no used slot."""
    g = torch.Generator().manual_seed(seed)
    preds = [torch.randn(B, 25, S, S, generator=g) for _ in range(3)] + [torch.randn(B, 15, S, S, generator=g)]
    X = torch.rand(B, 196, generator=g) * (S - 1.0) + 0.3
    Y = torch.rand(B, 196, generator=g) * (S - 1.0) + 0.3
    X[0, :6] = torch.tensor([0., 5., 17., float(S - 1), 31., float(S)])              # exact integers, the last one on the far border
    Y[0, :6] = torch.tensor([0., 9., 17., float(S - 1), float(S), 12.])
    X[0, 6:14] = torch.tensor([0.05, 0.45, S - 0.05, S - 0.45, 20.3, 33.7, 0.2, S - 0.3])    # within half a pixel of a border
    Y[0, 6:14] = torch.tensor([11.2, 0.1, 40.6, S - 0.2, 0.3, S - 0.1, S - 0.4, 0.25])
    X[1, 10:18] = 23.0 + torch.rand(8, generator=g) * 0.4 + 0.55                      # eight points inside one pixel's taps
    Y[1, 10:18] = 41.0 + torch.rand(8, generator=g) * 0.4 + 0.55
    I = torch.randint(1, 25, (B, 196), generator=g)
    I[:, 160:] = 0
    I[2] = 0                                                                          # sample 2: no used slot
    X[2], Y[2] = 0., 0.
    wts = torch.nn.functional.one_hot(I, 25).permute(0, 2, 1).float() * (I > 0).float().unsqueeze(1)
    dp = {'body_uv_X_points': X, 'body_uv_Y_points': Y, 'body_uv_Ind_points': torch.zeros(B, 196), 'body_uv_I_points': I.float(),
          'body_uv_U_points': (torch.rand(B, 25, 196, generator=g) * wts).reshape(B, 4900),
          'body_uv_V_points': (torch.rand(B, 25, 196, generator=g) * 3.0 * wts).reshape(B, 4900),       # (some residuals beyond 1: the linear branch)
          'body_uv_point_weights': wts.reshape(B, 4900),
          'body_uv_ann_labels': torch.randint(0, 15, (B, S * S), generator=g).to(torch.int32),
          'body_uv_ann_weights': torch.ones(B, S * S)}
    return preds, dp, torch.ones(B)


def _torch_form(preds, dp, has_dp, align, device, double):
    """IUV_Estimator.dp_uvia_losses -> (losses, gradients) with loss weights 1, 2, 3, 4.  double: evaluated in float64 -- the function
    states its arithmetic with explicit float32 casts, which are pointed at float64 for the duration of the call."""
    import contextlib
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    dt = torch.float64 if double else torch.float32
    ins = [t.detach().to(device=device, dtype=dt).requires_grad_(True) for t in preds]
    d = {k: (v.to(device) if v.dtype == torch.int32 else v.to(device=device, dtype=dt)) for k, v in dp.items()}
    with contextlib.ExitStack() as es:
        if double:
            es.enter_context(mock.patch.object(torch, 'float32', torch.float64))
            es.enter_context(mock.patch.object(torch.Tensor, 'float', torch.Tensor.double))
        out = IUV_Estimator.dp_uvia_losses(*ins, d, has_dp.to(device), bool(align))
        assert all(o.dtype == dt for o in out)
        sum(o * w for o, w in zip(out, (1., 2., 3., 4.))).backward()
    return [float(o.detach()) for o in out], [t.grad.detach().cpu().double() for t in ins]


@pytest.fixture(scope='module')
def edge():
    _cfg(**{'DANET.HEATMAP_SIZE': 64})
    preds, dp, has_dp = _edge_case()
    return {'in': (preds, dp, has_dp), 'oracle': {a: _torch_form(preds, dp, has_dp, a, 'cpu', True) for a in (0, 1)}}


@pytest.mark.parametrize('align', [0, 1])
def test_edge_cases_against_the_float64_torch_form(edge, align):
    """B = 3, S = 64: e_new (the HIP op) <= 2 * e_old (dp_uvia_losses on the GPU in fp32) + 1e-7 against dp_uvia_losses on the CPU in
    float64, for every loss and every gradient tensor (max abs error).
    Measured on MI355X: see DESIGN.md 4d."""
    _cfg(**{'DANET.HEATMAP_SIZE': 64})
    preds, dp, has_dp = edge['in']
    want_l, want_g = edge['oracle'][align]
    old_l, old_g = _torch_form(preds, dp, has_dp, align, DEV, False)
    new_l, new_g = _run_op(preds, dp, has_dp, align)
    rows = []
    for k, w, o, n in zip(LOSSES, want_l, old_l, new_l):
        rows.append((k, abs(n - w), abs(o - w)))
    for k, w, o, n in zip(('grad u', 'grad v', 'grad index', 'grad ann'), want_g, old_g, new_g):
        rows.append((k, float((n.double() - w).abs().max()), float((o - w).abs().max())))
    for k, e_new, e_old in rows:
        print('align %d %-14s e_new %.3e e_old %.3e' % (align, k, e_new, e_old))
    for k, e_new, e_old in rows:
        assert e_new <= 2 * e_old + 1e-7, (k, e_new, e_old)
    assert all(np.isfinite(x) for x in new_l) and new_l[2] > 0 and new_l[3] > 0
    assert float(new_g[0][2].abs().max()) == 0.0 and float(new_g[2][2].abs().max()) > 0      # no used slot: no U gradient, the index CE still runs


def test_backward_is_bitwise_reproducible(edge):
    preds, dp, has_dp = edge['in']
    _cfg(**{'DANET.HEATMAP_SIZE': 64})
    a = _run_op(preds, dp, has_dp, 1)
    b = _run_op(preds, dp, has_dp, 1)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_op_captures_and_replays_bit_for_bit(edge):
    from danet_densepose2smpl_amd import iuv_ops
    _cfg(**{'DANET.HEATMAP_SIZE': 64})
    preds, dp, has_dp = edge['in']
    ins = [_padded(t.to(DEV), ld).requires_grad_(True) for t, ld in zip(preds, (32, 32, 32, 16))]
    d = {k: v.to(DEV) for k, v in dp.items()}
    w = has_dp.to(DEV)

    def step():
        out = iuv_ops.dp_point_losses(*ins, d, w, False)
        return [o.clone() for o in out], list(torch.autograd.grad(sum(o * c for o, c in zip(out, (1., 2., 3., 4.))).sum(), ins))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(static[0], eager[0]))
        assert all(torch.equal(a, b) for a, b in zip(static[1], eager[1]))


def test_cpu_tensors_are_refused():
    from danet_densepose2smpl_amd import iuv_ops
    preds, dp, has_dp = _edge_case()
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        iuv_ops.dp_point_losses(*preds, dp, has_dp, True)


def test_estimator_dispatches_to_the_op_and_fp32_mode_to_the_torch_form(monkeypatch):
    sys.path.insert(0, GOLDEN)
    from make_golden import formula_params
    from danet_densepose2smpl_amd import conv
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    _cfg(**{'DANET.INIMG_SIZE': 64, 'DANET.HEATMAP_SIZE': 16, 'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0., 'DANET.PARTDROP_RATE': 0.})
    g, gd = golden('g7_estimator_align1'), golden('g11_dp_losses_align1')
    est = IUV_Estimator(pretrained=False)
    formula_params(est, skip=('learned_ratio', 'learned_offset', '_'))
    est = est.cuda().train()
    t = lambda k: torch.from_numpy(g[k]).cuda()                                       # noqa: E731
    dp = {k[4:]: torch.from_numpy(gd[k])[:2].cuda() for k in gd.files if k.startswith('dp__')}
    has_dp = torch.tensor([1., 0.], device=DEV)

    class Reached(Exception):
        pass

    def boom(*a, **k):
        raise Reached()
    monkeypatch.setattr(IUV_Estimator, 'dp_uvia_losses', staticmethod(boom))
    rd = est(t('img'), t('iuv_gt'), t('kps'), uvia_dp_gt=dp, has_iuv=torch.ones(2, device=DEV), has_dp=has_dp)
    assert all(torch.isfinite(rd['losses'][k]).all() and float(rd['losses'][k]) > 0 for k in LOSSES)
    sum(v.sum() for v in rd['losses'].values()).backward()
    assert est.iuv_est.final_pred.predict_ann_index.weight.grad.abs().sum() > 0
    with conv.precision('fp32'), pytest.raises(Reached):
        est(t('img'), t('iuv_gt'), t('kps'), uvia_dp_gt=dp, has_iuv=torch.ones(2, device=DEV), has_dp=has_dp)


def test_padded_base_hand_over_is_bit_equal_to_plain_heads():
    """B = 3, S = 16: dp_point_losses on leaf [B,25|15,S,S] heads and on [:, :25] / [:, :15] views carrying the `_padded_base` of leaf NHWC
    [B,32|16,S,S] buffers (same values, zeros behind): the losses bit-equal, the gradient on the base at full width with exactly zero
    pad channels and its leading channels bit-equal -- both runs feed the kernels the same row buffers."""
    from danet_densepose2smpl_amd import iuv_ops
    _cfg(**{'DANET.HEATMAP_SIZE': 16})
    preds, dp, has_dp = _edge_case(S=16, B=3)
    d, w = {k: v.to(DEV) for k, v in dp.items()}, has_dp.to(DEV)
    plain = [t.to(DEV).clone().requires_grad_(True) for t in preds]
    bases = [_padded(t.to(DEV), ld).requires_grad_(True) for t, ld in zip(preds, (32, 32, 32, 16))]
    views = []
    for b, t in zip(bases, preds):
        v = b[:, :t.shape[1]]
        v._padded_base = b
        views.append(v)
    res = []
    for ins in (plain, views):
        out = iuv_ops.dp_point_losses(*ins, d, w, True)
        sum(o * c for o, c in zip(out, (1., 2., 3., 4.))).sum().backward()
        res.append(torch.cat(out).detach())
    assert torch.equal(res[0], res[1]) and float(res[0].abs().min()) > 0
    for p, b, n in zip(plain, bases, (25, 25, 25, 15)):
        assert b.grad is not None and b.grad.shape == b.shape
        assert float(b.grad[:, n:].abs().max()) == 0.0
        assert torch.equal(b.grad[:, :n], p.grad)
