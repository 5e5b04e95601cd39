"""The backward-pass instruments of tests/conv_bound.py (reference_dgrad, reference_wgrad, int_operands) shown sound and sharp on the
CPU, before any kernel is involved: torch's own fp32 gradients stand in for a correct kernel and must pass; the same gradients with
ONE product removed -- at one corner pixel of the data gradient, from one element of the weight gradient -- stand in for a subtly
wrong kernel and must fail the elementwise bound (today's 1e-2 * max|ref| comparison passes seven of the eight).  And the integer
operands of tests/test_gpu_conv_grad.py meet, on every shape listed there, the conditions its exact comparison rests on."""
import math

import pytest
import torch
import torch.nn.functional as F

from conv_bound import U_BF16, U_F32, check, int_operands, ratios, reference_dgrad, reference_wgrad    # noqa: E402
import test_gpu_conv_grad as G    # noqa: E402  (its tables and operand generators; nothing in it touches a GPU on import)

# forward conv (B, Cin, Cout, k, stride, pad, groups, H, W, bf16 addend on the data gradient)
SHAPES = [(2, 48, 48, 3, 1, 1, 1, 16, 16, False), (4, 96, 64, 3, 2, 1, 1, 17, 17, False), (3, 64, 128, 1, 2, 0, 1, 15, 15, False),
          (2, 64, 64, 7, 2, 3, 1, 32, 32, False), (4, 96, 48, 3, 1, 1, 2, 8, 8, False), (8, 256, 256, 3, 1, 1, 1, 4, 4, False),
          (2, 384, 384, 3, 1, 1, 1, 8, 8, False), (2, 64, 256, 1, 1, 0, 1, 12, 10, True)]
_CACHE = {}


def _fp32_gradients(shape):
    """bf16-valued operands, torch's fp32 gradients of the convolution on them, and the fp64 references (computed once per shape)."""
    if shape not in _CACHE:
        B, Cin, Cout, k, stride, pad, groups, H, W, with_add = shape
        g = torch.Generator().manual_seed(sum(shape[:9]))
        x = torch.randn(B, Cin, H, W, generator=g).bfloat16().float().requires_grad_(True)
        w = (torch.randn(Cout, Cin // groups, k, k, generator=g) / math.sqrt(k * k * Cin / groups)).bfloat16().float().requires_grad_(True)
        y = F.conv2d(x, w, None, stride, pad, 1, groups)
        gy = torch.randn(y.shape, generator=g).bfloat16().float()
        add = torch.randn(x.shape, generator=g).bfloat16().float() if with_add else None
        gx, gw = torch.autograd.grad(y, (x, w), gy)
        x, w = x.detach(), w.detach()
        _CACHE[shape] = (x, w, gy, add, gx, gw, reference_dgrad(x.shape, w, gy, stride, pad, 1, groups, add),
                         reference_wgrad(x, gy, w.shape, stride, pad, 1, groups))
    return _CACHE[shape]


_ids = lambda s: 'x'.join(str(int(v)) for v in s)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_fp32_data_gradient_passes_and_one_dropped_product_fails(shape):
    x, w, gy, add, gx, _, ref, _ = _fp32_gradients(shape)
    pad = shape[5]
    out = lambda t: (t if add is None else t + add).bfloat16()          # the epilogue: addend in fp32, one rounding to bf16
    elem, mean = check(out(gx), ref, U_BF16, shape)
    assert elem <= 1.0 and mean <= 1.0
    # corner pixel (0, 0) of image 0, input channel 0 meets output pixel (0, 0) through tap (pad, pad): drop output channel 0's product
    bad = gx.clone()
    bad[0, 0, 0, 0] -= w[0, 0, pad, pad] * gy[0, 0, 0, 0]
    e_bad = ratios(out(bad), ref, U_BF16)[0]
    assert e_bad > 1.0, (shape, e_bad, float(w[0, 0, pad, pad] * gy[0, 0, 0, 0]))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_fp32_weight_gradient_passes_and_one_dropped_product_fails(shape):
    x, w, gy, _, _, gw, _, ref = _fp32_gradients(shape)
    pad = shape[5]
    assert ref.K == gy.shape[0] * gy.shape[2] * gy.shape[3]
    elem = ratios(gw, ref, U_F32)[0]
    assert elem <= 1.0, (shape, elem)
    bad = gw.clone()
    bad[0, 0, pad, pad] -= x[0, 0, 0, 0] * gy[0, 0, 0, 0]               # tap (pad, pad) pairs input pixel (0, 0) with output pixel (0, 0)
    e_bad = ratios(bad, ref, U_F32)[0]
    assert e_bad > 1.0, (shape, e_bad)


def test_references_handle_groups_and_agree_with_autograd_on_doubles():
    B, Cin, Cout, k, stride, pad, groups, H, W = 2, 12, 8, 3, 2, 1, 4, 9, 7
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin // groups, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride, pad, 1, groups)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    add = torch.randn(x.shape, generator=g, dtype=torch.float64)
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    rd = reference_dgrad(x.shape, w.detach(), gy, stride, pad, 1, groups, add)
    rw = reference_wgrad(x.detach(), gy, w.shape, stride, pad, 1, groups)
    assert torch.allclose(rd.r_conv, gx, rtol=1e-12, atol=1e-12) and torch.allclose(rd.r, gx + add, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rw.r, gw, rtol=1e-12, atol=1e-12)
    assert rd.K == Cout // groups * k * k and rw.K == B * y.shape[2] * y.shape[3]
    assert (rd.S >= rd.r.abs() - 1e-12).all() and (rw.S >= rw.r.abs() - 1e-12).all()


def test_int_operands_are_bf16_integers():
    g = torch.Generator().manual_seed(1)
    t = int_operands((4, 5, 6), -2, 2, g)
    assert t.dtype == torch.float32 and torch.equal(t, t.round()) and torch.equal(t.bfloat16().float(), t)
    assert set(t.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    with pytest.raises(ValueError):
        int_operands((2,), -300, 300, g)


@pytest.mark.parametrize('c', G.DGRAD, ids=G._did)
def test_integer_data_gradients_are_exact_in_fp32_and_mostly_bf16_numbers(c):
    """2 (Cout / groups) R S < 2^24, and at most 1 % of the exact gradient lies beyond 256 -- with the addend and without."""
    w, gy, add = G.dgrad_operands(c, 'int')
    assert 2 * (c.cout // c.groups) * c.k * c.k + 2 < 2 ** 24
    idx = G.sample_images(c)[:2]
    for a in (None, add):
        exact, small, unreached = G.int_dgrad_exact(c, w, gy, a, idx)
        assert torch.equal(exact, exact.round()) and exact.abs().max().item() < 2 ** 24
        assert (~small).double().mean().item() <= 0.01
        assert torch.equal(exact[unreached], (torch.zeros_like(exact) if a is None else a[idx].double())[unreached])


@pytest.mark.parametrize('c', G.WGRAD + [G.W('small_map', 'multi3', ci, co, 3, st, 1, 1, gr, s * st, s * st, B) for B, ci, co, gr, s, st in G.PAIRS]
                         + [G.W('pw_multi', 'multi', ci, co, 1, 1, 0, 1, 1, h, w, b) for ci, co, h, w, b in G.PW_MULTI], ids=G._wid)
def test_integer_weight_gradients_are_exact_in_fp32(c):
    d = G.wgrad_dims(c)
    assert 4 * c.B * d[4] * d[5] + 3 < 2 ** 24
