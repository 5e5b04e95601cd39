"""tests/stn_oracle.py against torch's own affine_grid + grid_sample on the CPU in float64 (autograd gives the backward), so
that the oracle is trusted before csrc/stn.hip is judged by it (tests/test_gpu_stn.py).  Both sides are float64 evaluations of
the same definition in different operation orders: they must agree to 1e-12 of the tensors' scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stn_oracle as so

CASES = ['pc1', 'out_hw', 'oh1', 'ow1', 'idle', 'sheared']


def _torch_ref(x, theta, OH, OW, align, gy):
    """x [B,H,W,C], theta [B,P,2,3] float32, gy [B,OH,OW,P*C] -> (y, dx) in the oracle's layouts, from torch in float64."""
    B, H, W, C = x.shape
    P = theta.shape[1]
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    th = torch.from_numpy(theta).double()
    outs = [F.grid_sample(xt, F.affine_grid(th[:, p], [B, C, OH, OW], align_corners=align), mode='bilinear', padding_mode='zeros',
                          align_corners=align) for p in range(P)]
    y = torch.cat(outs, 1)                                                  # [B, P*C, OH, OW]
    g, = torch.autograd.grad(y, xt, torch.from_numpy(gy).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).numpy(), g.permute(0, 2, 3, 1).numpy()


def _inputs(case):
    B, P, C, H, W, OH, OW = so.SHAPES['out_hw' if case == 'sheared' else case]
    rs = np.random.RandomState(11)
    x = rs.standard_normal((B, H, W, C))
    gy = rs.standard_normal((B, OH, OW, P * C))
    if case == 'sheared':
        return x, gy, [so.sheared_thetas(B, P, 5)]
    # enough phases for every kind of theta (negative scale, far-outside centre, ...) to occur at this B * P
    return x, gy, [so.thetas(B, P, 5 + ph, ph)[0] for ph in range(0, 8, min(8, B * P))]


@pytest.mark.filterwarnings('ignore:Since version 1.3.0, affine_grid')      # OH == 1 / OW == 1 on purpose
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_oracle_vs_torch_float64(case, align):
    x, gy, ths = _inputs(case)
    B, H, W, C = x.shape
    OH, OW = gy.shape[1:3]
    for th in ths:
        y_t, dx_t = _torch_ref(x, th, OH, OW, align, gy)
        y = so.forward(x, th, OH, OW, align)
        dx = so.backward(gy, th, H, W, align)
        assert y.shape == y_t.shape and dx.shape == dx_t.shape
        assert np.abs(y - y_t).max() <= 1e-12 * max(np.abs(y_t).max(), 1.0)
        assert np.abs(dx - dx_t).max() <= 1e-12 * max(np.abs(dx_t).max(), 1.0)


def test_oracle_backward_is_the_transpose():
    """<forward(x), gy> == <x, backward(gy)> in float64, sheared thetas included."""
    B, P, C, H, W, OH, OW = so.SHAPES['out_hw']
    rs = np.random.RandomState(3)
    x, gy = rs.standard_normal((B, H, W, C)), rs.standard_normal((B, OH, OW, P * C))
    for th in (so.thetas(B, P, 1)[0], so.sheared_thetas(B, P, 2)):
        for align in (False, True):
            y = so.forward(x, th, OH, OW, align)
            a, b = np.sum(y * gy), np.sum(x * so.backward(gy, th, H, W, align))
            assert abs(a - b) <= 1e-12 * np.sum(np.abs(y * gy))


def test_candidates_bracket_the_transpose():
    """candidates() counts every sample with a non-zero tent weight at weight 1: backward(|gy|) <= candidates(|gy|, delta = 0)
    elementwise, the count grows with delta, and a part whose samples all miss the map adds nothing to either."""
    B, P, C, H, W, OH, OW = so.SHAPES['idle']
    rs = np.random.RandomState(4)
    g = np.abs(rs.standard_normal((B, OH, OW, P * C)))
    for ph in (0, 6):
        th, kinds = so.thetas(B, P, 9, ph)
        for align in (False, True):
            R = so.backward(g, th, H, W, align)
            T0, T1 = so.candidates(g, th, H, W, align, 0.0), so.candidates(g, th, H, W, align, 0.25)
            assert (R <= T0 + 1e-12).all() and (T0 <= T1).all() and (T1 > T0).any()
            empty = np.isin(kinds, so.EMPTY_KINDS)
            ge = g.reshape(B, OH, OW, P, C) * empty[:, None, None, :, None]
            assert empty.any() and not so.candidates(ge.reshape(g.shape), th, H, W, align, 0.25).any()


def test_thetas_cover_every_kind_and_stay_in_range():
    for name, (B, P, C, H, W, OH, OW) in so.SHAPES.items():
        seen = set()
        for ph in range(0, 8, min(8, B * P)):
            th, kinds = so.thetas(B, P, 7 + ph, ph)
            seen |= set(kinds.ravel())
            assert th.dtype == np.float32 and (th[:, :, 0, 1] == 0).all() and (th[:, :, 1, 0] == 0).all()
            assert (np.abs(th[:, :, 0, 0]) + np.abs(th[:, :, 0, 2]) <= 8).all() and (np.abs(th[:, :, 1, 1]) + np.abs(th[:, :, 1, 2]) <= 8).all()
            flat = th.reshape(B * P, 6)
            varied = kinds.ravel() != 'identity'
            assert len({tuple(r) for r in flat[varied]}) == varied.sum(), 'a different theta for every (b, p)'
        assert seen == set(so.KINDS), name
