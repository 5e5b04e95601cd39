"""The backward pass's convolution kernels -- every data-gradient and weight-gradient family of csrc/conv*.hip, and the bias gradient --
against an fp64 reference of the same operation on the same bf16 operands (tests/conv_bound.py reference_dgrad / reference_wgrad).

Every case first asserts, with the library's own predicate, that the kernel family it is meant for is the one that runs, and is then
checked twice:

(a) 'rand': x, gy ~ N(0, 1), w ~ N(0, 1 / K_fwd), rounded to bf16; the result must stay within the elementwise rounding bound
    |y - r| <= u |r| + C_ACC 2^-24 sqrt(K) S and (data gradients) the per-channel mean check, with the constants the inference-engine
    tests use (u = 2^-8 for the bf16 data gradients, rounded once, the residual addend fused; u = 2^-22 for the fp32 weight gradients;
    the beta = 1 form rounds the sum and then the accumulation: rounded_conv).  The measured ratios go to record('conv_grad_bound').
(b) 'int': x, gy, addend in {-2 .. 2}, w in {-1, 0, 1}.  Every product and partial sum is an integer below 2^24 (asserted from the
    shape), so fp32 accumulation is exact in any order, through split-K partials and atomics alike: weight gradients must EQUAL the
    exact result, data gradients must equal it wherever |exact| <= 256 (a bf16 number: no rounding rule enters; at most 1 % of the
    elements may lie beyond), and positions the gradient never reaches must hold exactly the addend (zero without one).

What the tables found about the routing (asserted below, so it stays true):
  * a stride-2 data gradient whose gathered channels per group are no multiple of 32 has no parity classes and runs on
    conv_igemm_kernel (id % 10 == 0); that is the one way the training pass reaches that kernel -- conv.conv2d pads every other
    width to a multiple of 8, so the (48 -> 25) and (12 -> 12) layers run at (48 -> 32) on the LDS 3x3 kernel and at (16 -> 16) on
    the gather kernel, and are kept here for the pad-and-crop route of their gradients;
  * the streamed kernel takes grouped problems forward only (conv3x3s.hip), so with conv_g3 switched off the 24-group head's data
    gradient runs on the grouped gather kernel (id % 10 == 1), not on id % 10 == 4;
  * 512 -> 512 on 2 x 2 maps is no LDS 3x3 problem at any batch size (gather kernel); 40 -> 72 has no pointwise weight-gradient
    plan and runs on conv_wgrad_kernel<4, 3, 1>.
References are computed on the CPU in fp64, for a sample of images (first and last included) where the batch is large."""
import collections
import ctypes
import math

import pytest
import torch

from conftest import record
from conv_bound import U_BF16, U_F32, Reference, int_operands, ratios, reference_dgrad, reference_wgrad    # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ('rand', 'int')
_WORST = collections.defaultdict(lambda: [0.0, 0.0])


def _note(family, case, elem, mean=0.0):
    w = _WORST[family]
    w[0], w[1] = max(w[0], elem), max(w[1], mean)
    record('conv_grad_bound', {'family': family, 'case': case, 'elem': elem, 'chan_mean': mean, 'family_worst': list(w)})


def osz(n, k, stride, pad, dil=1):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ---- data gradients --------------------------------------------------------------------------------------------------------------
# the FORWARD convolution (cin -> cout, k, stride, pad, groups) on a [B, cin, H, W] input; route: how the kernel is called; kid: the last
# digit danet_conv_forward_kernel must report for the data gradient (routes raw / conv2d); addend: also run with the fused addend;
# knobs: library switches held during the launch; force: (MT, KW) register tiling of the LDS-tile kernel that must be honoured
D = collections.namedtuple('D', 'family route cin cout k stride pad groups H W B kid addend knobs force', defaults=(None, False, {}, None))
_TILE = {'c3s_enable': 0}          # streamed kernel off: conv3x3_tile_kernel runs what it would have taken
_C3 = [(16, 16, 8, 8, 2), (48, 32, 20, 12, 3), (80, 48, 16, 16, 5), (384, 384, 7, 7, 2)]
_G = 24
DGRAD = [
    D('gather', 'raw', 256, 64, 1, 1, 0, 1, 24, 20, 4, 1, True),
    D('gather_s2_parity', 'raw', 96, 64, 3, 2, 1, 1, 17, 17, 4, 1, True),
    D('gather_s2_parity', 'raw', 64, 128, 1, 2, 0, 1, 15, 15, 3, 1, True),
    D('igemm_s2_no_parity', 'raw', 96, 48, 3, 2, 1, 1, 16, 16, 3, 0),
    D('padded_widths', 'conv2d', 48, 25, 3, 1, 1, 1, 12, 12, 2, 2),
    D('padded_widths', 'conv2d', 12, 12, 3, 1, 1, 1, 12, 12, 2, 1),
    D('gather', 'raw', 512, 512, 3, 1, 1, 1, 2, 2, 8, 1, True),
] + [D('lds3x3_planner', 'raw', ci, co, 3, 1, 1, 1, h, w, b, 2, True) for ci, co, h, w, b in _C3] \
  + [D('lds3x3_tile', 'raw', ci, co, 3, 1, 1, 1, h, w, b, 2, True, _TILE) for ci, co, h, w, b in _C3] \
  + [D('lds3x3_tile_forced', 'raw', 48, 32, 3, 1, 1, 1, 20, 12, 3, 2, True, _TILE, f) for f in ((8, 2), (8, 4), (4, 1), (4, 2), (4, 4))] + [
    D('conv_pw', 'raw', 96, 192, 1, 1, 0, 1, 24, 20, 18, 3, True),
    D('conv_pw', 'raw', 128, 128, 1, 1, 0, 1, 33, 31, 9, 3, True),
    D('conv_pw', 'raw', 40, 72, 1, 1, 0, 1, 50, 50, 4, 3, True),
    D('gather_grouped', 'raw', _G * 48, _G * 24, 3, 1, 1, _G, 32, 32, 3, 1, True, {'g3': 0}),
    D('conv_g3', 'raw', _G * 48, _G * 24, 3, 1, 1, _G, 7, 16, 2, 5),
    D('conv_g3', 'raw', _G * 48, _G * 24, 3, 1, 1, _G, 20, 48, 2, 5),
    D('conv_stem_dgrad', 'stem', 64, 64, 7, 2, 3, 1, 64, 64, 64),
    D('conv_stem_dgrad', 'stem', 64, 64, 7, 2, 3, 1, 64, 64, 70),
    D('conv3x3a', 'c3a', 64, 64, 3, 1, 1, 1, 64, 64, 20, None, True),
    D('conv3x3a', 'c3a', 64, 64, 3, 1, 1, 1, 32, 16, 140, None, True),
]


def _did(c):
    return '%s-%s' % (c.family, 'x'.join(str(v) for v in c[2:11])) + ('' if c.force is None else '-mt%d_kw%d' % c.force)


def sample_images(c):
    """The images a case's reference is computed for: all of a small batch, else four that include the first and the last."""
    macs = c.B * osz(c.H, c.k, c.stride, c.pad) * osz(c.W, c.k, c.stride, c.pad) * c.cout * (c.cin // c.groups) * c.k * c.k
    return list(range(c.B)) if macs <= 4e8 else sorted(set(int(round(i * (c.B - 1) / 3.0)) for i in range(4)))


def dgrad_operands(c, kind):
    """(w [cout, cin/groups, k, k], gy [B, cout, OH, OW], addend [B, cin, H, W]) on the CPU, fp32 holding bf16 numbers."""
    g = torch.Generator().manual_seed(sum(int(v) for v in c[2:11]) + (1 if kind == 'int' else 0))
    ws, gs = (c.cout, c.cin // c.groups, c.k, c.k), (c.B, c.cout, osz(c.H, c.k, c.stride, c.pad), osz(c.W, c.k, c.stride, c.pad))
    xs = (c.B, c.cin, c.H, c.W)
    if kind == 'int':
        return int_operands(ws, -1, 1, g), int_operands(gs, -2, 2, g), int_operands(xs, -2, 2, g)
    w = (torch.randn(ws, generator=g) / math.sqrt(c.k * c.k * c.cin / c.groups)).bfloat16().float()
    return w, torch.randn(gs, generator=g).bfloat16().float(), torch.randn(xs, generator=g).bfloat16().float()


def int_dgrad_exact(c, w, gy, add, idx):
    """The exact integer data gradient of the sampled images, the mask of its bf16-exact elements (|.| <= 256) and the mask of the
    positions no tap reaches.  Sums stay below 2^24: |w| <= 1, |gy| <= 2, at most cout/groups * k * k products, |addend| <= 2."""
    assert 2 * (c.cout // c.groups) * c.k * c.k + 2 < 2 ** 24
    shape = (len(idx), c.cin, c.H, c.W)
    ref = reference_dgrad(shape, w, gy[idx], c.stride, c.pad, 1, c.groups, None if add is None else add[idx])
    reach = reference_dgrad(shape, torch.ones_like(w), torch.ones_like(gy[idx]), c.stride, c.pad, 1, c.groups).r
    return ref.r, ref.r.abs() <= 256, reach == 0


def _launch_dgrad(c, w, gy, add):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    OH, OW = gy.shape[2], gy.shape[3]
    tdims = (c.B, OH, OW, c.cout, c.H, c.W, c.cin, c.k, c.k, c.stride, c.pad, 1, c.groups)       # as the kernels take a data gradient
    if c.route == 'raw':
        dconv.stream_tables(gy.device)
        knobs = dict(c.knobs)
        if c.force is not None:
            knobs.update(c3_mt=c.force[0], c3_kw=c.force[1])
        with _lib.knobs(**knobs):
            kid = L.danet_conv_forward_kernel(*tdims, 1, 0)
            assert kid % 10 == c.kid, (kid, c)
            if c.family == 'gather_s2_parity':
                assert (c.cout // c.groups) % 32 == 0             # gathered channels per group: the parity classes exist
            if c.family.startswith('lds3x3'):
                plan = L.danet_conv3x3_stream_plan(c.B, c.H, c.W, c.cout, c.cin, 1)
                assert c.family == 'lds3x3_planner' or plan == 0, plan       # ('tile': the streamed kernel must be out of the way)
            if c.force is not None:
                assert (kid // 1000, (kid // 10) % 10) == c.force, (kid, c.force)
            y = dconv._conv_fwd_raw(gy, dconv.pack_weight(w, c.groups, 1), None, *tdims, True, False, False, None, None, add)
            torch.cuda.synchronize()
        return y
    if c.route == 'stem':
        assert add is None and L.danet_conv_stem_dgrad_ok(c.B, c.H, c.W, c.cin, OH, OW, c.cout, c.k, c.k, c.stride, c.pad, 1, c.groups) == 1
        return dconv._conv_stem_dgrad_raw(gy, dconv.pack_weight(w, 1, 1, 16), c.B, c.H, c.W, c.cin, OH, OW, c.cout, None)
    if c.route == 'c3a':
        assert L.danet_conv3x3a_ok(c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, 1, c.groups) == 1
        return dconv._conv3x3a_raw(gy, dconv.pack_weight(w, 1, 1, 16), c.B, c.H, c.W, True, None, None, add)
    raise ValueError(c.route)


def _check_dgrad(c, kind, y, w, gy, add, idx, what):
    yy = y[idx].float().cpu()
    if kind == 'rand':
        ref = reference_dgrad(yy.shape, w, gy[idx], c.stride, c.pad, 1, c.groups, None if add is None else add[idx])
        elem, mean = ratios(yy, ref, U_BF16)                      # (conv_bound.check's assertion, the figures written down first)
        _note(c.family, what, elem, mean)
        assert elem <= 1.0 and mean <= 1.0, (what, {'elem': elem, 'chan_mean': mean})
        return
    exact, small, unreached = int_dgrad_exact(c, w, gy, add, idx)
    assert (~small).double().mean().item() <= 0.01, what
    assert torch.equal(yy.double()[small], exact[small]), (what, int((yy.double() != exact)[small].sum()))
    rest = torch.zeros_like(exact) if add is None else add[idx].double()
    assert torch.equal(yy.double()[unreached], rest[unreached]), what
    if c.k == 1 and c.stride == 2:
        assert unreached.double().mean().item() > 0.7               # three of four pixels, and the last row / column


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', [c for c in DGRAD if c.route != 'conv2d'], ids=_did)
def test_data_gradient(c, kind):
    from danet_densepose2smpl_amd import conv as dconv
    w, gy, add = dgrad_operands(c, kind)
    idx = sample_images(c)
    gyd, wd = dconv.nhwc_bf16(gy.cuda()), w.cuda()
    for a in ((None, add) if c.addend else (None,)):
        y = _launch_dgrad(c, wd, gyd, None if a is None else dconv.nhwc_bf16(a.cuda()))
        torch.cuda.synchronize()
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (c.B, c.cin, c.H, c.W)
        _check_dgrad(c, kind, y, w, gy, a, idx, _did(c) + ('+addend' if a is not None else ''))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', [c for c in DGRAD if c.route == 'conv2d'], ids=_did)
def test_data_gradient_at_padded_widths_through_autograd(c, kind):
    """Widths that are no multiple of 8 through conv.conv2d: the layer runs zero-padded (48 -> 32 with a bias, 16 -> 16), the data
    gradient on the kernel the library names for the PADDED problem, cropped back by autograd; the weight and bias gradients of the
    same backward call are held to their references as well."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    w, gy, _ = dgrad_operands(c, kind)
    bias = c.cout % 8 != 0
    padc, _, padn = dconv.channel_padding(c.cin, c.cin, c.cout, 1)
    assert L.danet_conv_forward_kernel(c.B, c.H, c.W, c.cout + padn, c.H, c.W, c.cin + padc, 3, 3, 1, 1, 1, 1, 1, 0) % 10 == c.kid
    g = torch.Generator().manual_seed(c.cin)
    x = int_operands((c.B, c.cin, c.H, c.W), -2, 2, g) if kind == 'int' else torch.randn(c.B, c.cin, c.H, c.W, generator=g).bfloat16().float()
    xt = x.cuda().requires_grad_(True)
    wt = w.cuda().requires_grad_(True)
    bt = torch.zeros(c.cout, device='cuda', requires_grad=True) if bias else None
    y = dconv.conv2d(xt, wt, bt, 1, 1)
    y.backward(gy.cuda().bfloat16())
    torch.cuda.synchronize()
    idx = list(range(c.B))
    _check_dgrad(c, kind, xt.grad, w, gy, None, idx, _did(c))
    ref = reference_wgrad(x, gy, w.shape, 1, 1)
    bref = bias_reference(gy)
    if kind == 'int':
        assert torch.equal(wt.grad.cpu().double(), ref.r)
        assert not bias or torch.equal(bt.grad.cpu().double().view_as(bref.r), bref.r)
    else:
        elem = ratios(wt.grad.cpu(), ref, U_F32)[0]
        _note('padded_widths_wgrad', _did(c), elem)
        assert elem <= 1.0
        assert not bias or ratios(bt.grad.cpu().view_as(bref.r), bref, U_F32)[0] <= 1.0


@pytest.mark.parametrize('kind', KINDS)
def test_four_branch_data_gradient_launch(kind):
    """danet_conv_forward_multi, transposed, on the four HRNet branch widths in ONE launch of conv3x3_stream_kernel: at the smallest
    maps and batch where the planner still takes the streamed kernel for the set (384 channels on 4 x 4 or 2 x 2 maps are no LDS
    3x3 problem at any batch size, so the search moves on to larger maps)."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    chans = (48, 96, 192, 384)
    dev = torch.device('cuda')
    dconv.stream_tables(dev)

    def table(B, sizes, tensors=None):
        jobs = (_lib.ConvJob * 4)()
        for i, (j, ch, s) in enumerate(zip(jobs, chans, sizes)):
            if tensors is None:
                j.x = j.wp = j.y = 4096                     # (the planner reads the geometry only)
                dconv._job_geometry(j, (B, s, s, ch, s, s, ch, 3, 3, 1, 1, 1, 1), True)
            else:
                dconv._conv_job(j, tensors[i][0], tensors[i][1], tensors[i][2], (B, s, s, ch, s, s, ch, 3, 3, 1, 1, 1, 1), True)
        return jobs
    found = None
    for sizes in ((16, 8, 4, 2), (32, 16, 8, 4), (64, 32, 16, 8)):
        for B in (4, 8, 16, 32):
            if found is None and L.danet_conv_forward_multi_kernel(ctypes.addressof(table(B, sizes)), 4) == 3:
                found = (B, sizes)
    assert found is not None, 'no four-branch set runs on the streamed kernel'
    B, sizes = found
    cases = [D('four_branch_multi', 'multi', ch, ch, 3, 1, 1, 1, s, s, B) for ch, s in zip(chans, sizes)]
    ops = [dgrad_operands(c, kind) for c in cases]
    tensors = [(dconv.nhwc_bf16(gy.cuda()), dconv.pack_weight(w.cuda(), 1, 1), dconv._empty_nhwc(B, c.cin, c.H, c.W, torch.bfloat16, dev))
               for c, (w, gy, _) in zip(cases, ops)]
    jobs = table(B, sizes, tensors)
    assert L.danet_conv_forward_multi_kernel(ctypes.addressof(jobs), 4) == 3
    dconv.check(L.danet_conv_forward_multi(ctypes.addressof(jobs), 4, _lib.stream()), 'danet_conv_forward_multi')
    torch.cuda.synchronize()
    for c, (w, gy, _), t in zip(cases, ops, tensors):
        _check_dgrad(c, kind, t[2], w, gy, None, sample_images(c), 'four-branch %d @ %d, B = %d' % (c.cin, c.H, B))


# ---- weight gradients ------------------------------------------------------------------------------------------------------------
# the forward convolution again; route: generic (danet_conv_wgrad: conv_wgrad_kernel<CT, NI, TG>, kid = its id, or the pointwise kernel,
# kid None), w3 (danet_conv_wgrad3x3; ms: 'one' / 'many' partial blocks), rows (danet_conv_wgrad_rows)
W = collections.namedtuple('W', 'family route cin cout k stride pad dil groups H W B kid ms', defaults=(None, None))
WGRAD = [
    # 3x3 shapes danet_conv_wgrad3x3_ok refuses, 16 .. 64 channels per group: 1, 2, 3 and 4 (-> 2) tiles of 16 on either side
    W('conv_wgrad_9', 'generic', 16, 24, 3, 2, 1, 1, 1, 17, 17, 3, 219),
    W('conv_wgrad_9', 'generic', 32, 48, 3, 1, 2, 2, 1, 12, 12, 2, 329),
    W('conv_wgrad_9', 'generic', 64, 16, 3, 1, 1, 1, 1, 10, 12, 2, 149),
    W('conv_wgrad_9', 'generic', 48, 64, 3, 1, 1, 1, 1, 9, 9, 2, 239),
    W('conv_wgrad_9', 'generic', 64, 64, 3, 2, 1, 1, 1, 17, 17, 2, 249),
    W('conv_wgrad_9', 'generic', 16, 64, 7, 2, 3, 1, 1, 16, 16, 4, 419),
    W('conv_wgrad_9', 'generic', 96, 128, 3, 1, 1, 1, 4, 10, 10, 2, 229),
    W('conv_wgrad_1', 'generic', 64, 128, 1, 2, 0, 1, 1, 15, 15, 3, 441),
    W('conv_wgrad_1', 'generic', 40, 72, 1, 1, 0, 1, 1, 32, 32, 4, 431),
    W('conv_pw_wgrad', 'generic', 64, 256, 1, 1, 0, 1, 1, 32, 32, 4),
    W('conv_pw_wgrad', 'generic', 24, 64, 1, 1, 0, 1, 1, 32, 32, 4),
    W('conv_wgrad3x3', 'w3', 16, 16, 3, 1, 1, 1, 1, 4, 8, 2, None, 'one'),
    W('conv_wgrad3x3', 'w3', 16, 16, 3, 2, 1, 1, 1, 16, 16, 4, None, 'many'),
    W('conv_wgrad3x3', 'w3', 48, 96, 3, 1, 1, 1, 1, 8, 8, 2, None, 'one'),
    W('conv_wgrad3x3', 'w3', 48, 96, 3, 1, 1, 1, 1, 4, 8, 8, None, 'many'),
    W('conv_wgrad3x3', 'w3', 48, 96, 3, 2, 1, 1, 1, 24, 32, 2, None, 'many'),
    W('conv_wgrad3x3', 'w3', 80, 48, 3, 1, 1, 1, 2, 12, 16, 1, None, 'one'),
    W('conv_wgrad3x3', 'w3', 80, 48, 3, 2, 1, 1, 2, 8, 16, 8, None, 'many'),
    W('conv_wgrad3x3', 'w3', 256, 96, 3, 1, 1, 1, 1, 8, 8, 4, None, 'many'),
    W('conv_wgrad3x3', 'w3', 256, 96, 3, 2, 1, 1, 1, 8, 16, 3, None, 'one'),
    W('conv_wgrad3x3', 'w3', 256, 96, 3, 1, 1, 1, 1, 12, 16, 3, None, 'many'),
    # the predicate's minimum B * OH * OW = 65536: the narrowest widths the launcher accepts (half a 16-channel tile in, one out), and
    # one 16-channel slab in with all four 16-channel tiles of a block out
    W('conv_wgrad_rows', 'rows', 8, 16, 7, 2, 3, 1, 1, 64, 64, 64),
    W('conv_wgrad_rows', 'rows', 16, 64, 7, 2, 3, 1, 1, 64, 64, 64),
]
# (B, cin, cout, groups, output map side, stride): 4 x 4 outputs pair images, 2 x 2 outputs take eight per chunk
PAIRS = [(2, 16, 16, 1, 4, 1), (6, 64, 32, 1, 4, 2), (8, 64, 32, 1, 2, 1), (8, 48, 48, 1, 2, 2), (4, 96, 48, 2, 4, 1), (6, 96, 48, 2, 4, 2)]
PW_MULTI = [(64, 256, 32, 32, 4), (24, 64, 32, 32, 4), (40, 72, 32, 32, 4), (64, 24, 64, 32, 2)]         # (cin, cout, H, W, B), 1x1 / stride 1


def _wid(c):
    return '%s-%s' % (c.family, 'x'.join(str(v) for v in c[2:12]))


def wgrad_dims(c):
    return (c.B, c.H, c.W, c.cin, osz(c.H, c.k, c.stride, c.pad, c.dil), osz(c.W, c.k, c.stride, c.pad, c.dil), c.cout, c.k, c.k,
            c.stride, c.pad, c.dil, c.groups)


def wgrad_operands(c, kind):
    """(x [B, cin, H, W], gy [B, cout, OH, OW], the beta = 1 run's initial dW) on the CPU."""
    d = wgrad_dims(c)
    g = torch.Generator().manual_seed(sum(int(v) for v in c[2:12]) + (1 if kind == 'int' else 0))
    xs, gs, ws = (c.B, c.cin, c.H, c.W), (c.B, c.cout, d[4], d[5]), (c.cout, c.cin // c.groups, c.k, c.k)
    if kind == 'int':
        assert 4 * c.B * d[4] * d[5] + 3 < 2 ** 24                    # |x|, |gy| <= 2 over B * OH * OW pixels, |init| <= 3
        return int_operands(xs, -2, 2, g), int_operands(gs, -2, 2, g), int_operands(ws, -3, 3, g)
    return torch.randn(xs, generator=g).bfloat16().float(), torch.randn(gs, generator=g).bfloat16().float(), torch.randn(ws, generator=g)


def _three_ways(cases, kind, launch):
    """launch(xs, gys, outs, beta) runs the weight gradients of `cases` (device tensors: bf16 NHWC operands, fp32 outputs): into
    NaN-filled outputs with beta = 0, a second time (bit-identical), and with beta = 1 onto a known tensor."""
    from danet_densepose2smpl_amd import conv as dconv
    ops = [wgrad_operands(c, kind) for c in cases]
    xs = [dconv.nhwc_bf16(o[0].cuda()) for o in ops]
    gys = [dconv.nhwc_bf16(o[1].cuda()) for o in ops]

    def run(beta):
        outs = [o[2].cuda() if beta else torch.full(o[2].shape, float('nan'), device='cuda') for o in ops]
        launch(xs, gys, outs, beta)
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]
    a, b, acc = run(0.0), run(0.0), run(1.0)
    for c, (x, gy, init), ya, yb, yc in zip(cases, ops, a, b, acc):
        what = _wid(c)
        ref = reference_wgrad(x, gy, init.shape, c.stride, c.pad, c.dil, c.groups)
        assert torch.isfinite(ya).all() and torch.equal(ya, yb), what
        if kind == 'int':
            assert torch.equal(ya.double(), ref.r), (what, int((ya.double() != ref.r).sum()))
            assert torch.equal(yc.double(), ref.r + init.double()), what
        else:
            elem = ratios(ya, ref, U_F32)[0]
            racc = ref._replace(r=ref.r + init.double(), S=ref.S + init.double().abs(), res=init.double())
            elem1 = ratios(yc, racc, U_F32, rounded_conv=True)[0]
            _note(c.family, what, elem)
            _note(c.family + '_beta1', what, elem1)
            assert elem <= 1.0 and elem1 <= 1.0, (what, elem, elem1)


def _wg_table(cases, xs, gys, outs):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    jobs = (_lib.WgJob * len(cases))()
    for j, c, x, gy, o in zip(jobs, cases, xs, gys, outs):
        j.x, j.dy, j.dw = (4096, 4096, 4096) if x is None else (dconv.nptr(x), dconv.nptr(gy), o.data_ptr())
        dconv._fill_wg(j, wgrad_dims(c))
    return jobs


def _pointwise(c):
    """Whether csrc/conv_pw_wgrad.hip takes the problem: its partial sums are the part of danet_conv_wgrad_multi's workspace that
    needs no zeroing, so a one-problem table has a non-zero zero_from exactly then."""
    from danet_densepose2smpl_amd import _lib
    jobs = _wg_table([c], [None], [None], [None])
    return _lib.lib().danet_conv_wgrad_multi_ws_zero_from(ctypes.addressof(jobs), 1) > 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', WGRAD, ids=_wid)
def test_weight_gradient(c, kind):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib.lib()
    d = wgrad_dims(c)
    ok3 = L.danet_conv_wgrad3x3_ok(c.H, c.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, c.dil, c.groups)
    rows = L.danet_conv_wgrad_rows_ok(*d)
    cgw = c.cout * (c.cin // c.groups) * c.k * c.k
    if c.route == 'generic':
        assert not ok3 and not rows and _pointwise(c) == (c.kid is None), c
        assert c.kid is None or L.danet_conv_wgrad_kernel_id(c.cin, c.cout, c.groups, c.k * c.k) == c.kid
        nws = L.danet_conv_wgrad_ws_floats_for(*d)

        def launch(xs, gys, outs, beta):
            ws = torch.full((nws,), float('nan'), device='cuda')          # (not zeroed: the call must clear what it accumulates into)
            dconv.check(L.danet_conv_wgrad(dconv.nptr(xs[0]), dconv.nptr(gys[0]), ptr(outs[0]), ptr(ws), nws, *d, beta, 0, stream()), 'danet_conv_wgrad')
    elif c.route == 'w3':
        assert ok3 == 1
        nws = L.danet_conv_wgrad3x3_ws_floats(c.B, c.H, c.W, c.cin, c.cout, c.groups, c.stride)
        assert nws % cgw == 0 and (nws // cgw == 1) == (c.ms == 'one'), (nws // cgw, c)

        def launch(xs, gys, outs, beta):
            ws = torch.full((nws,), float('nan'), device='cuda')
            dconv.check(L.danet_conv_wgrad3x3(dconv.nptr(xs[0]), dconv.nptr(gys[0]), ptr(outs[0]), ptr(ws), nws, c.B, c.H, c.W, c.cin, c.cout,
                                              c.groups, c.stride, beta, 0, stream()), 'danet_conv_wgrad3x3')
    else:
        assert rows == 1 and c.B * d[4] * d[5] == 65536
        nws = L.danet_conv_wgrad_rows_ws_floats(c.B, d[4], d[5], c.cin, c.cout, c.k, c.k, c.groups)

        def launch(xs, gys, outs, beta):
            ws = torch.full((nws,), float('nan'), device='cuda')
            dconv.check(L.danet_conv_wgrad_rows(dconv.nptr(xs[0]), dconv.nptr(gys[0]), ptr(outs[0]), ptr(ws), nws, c.B, c.H, c.W, c.cin, d[4], d[5],
                                                c.cout, c.k, c.k, c.stride, c.pad, c.groups, beta, stream()), 'danet_conv_wgrad_rows')
    _three_ways([c], kind, launch)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,cin,cout,groups,side,stride', PAIRS, ids=lambda v: str(v))
def test_weight_gradient_small_map_mode(B, cin, cout, groups, side, stride, kind):
    """conv_wgrad3x3.hip with two (4 x 4 outputs) or eight (2 x 2) images per chunk, through danet_conv_wgrad3x3_multi, with an ordinary
    8 x 8 job of the same widths in the same call."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib.lib()
    cases = [W('conv_wgrad3x3_small_map', 'multi3', cin, cout, 3, stride, 1, 1, groups, side * stride, side * stride, B),
             W('conv_wgrad3x3_multi', 'multi3', cin, cout, 3, stride, 1, 1, groups, 8 * stride, 8 * stride, 4)]
    s = cases[0]
    assert L.danet_conv_wgrad3x3_pair_ok(s.B, s.H, s.W, cin, cout, 3, 3, stride, 1, 1, groups) == 1
    assert L.danet_conv_wgrad3x3_ok(s.H, s.W, cin, cout, 3, 3, stride, 1, 1, groups) == 0
    assert L.danet_conv_wgrad3x3_ok(cases[1].H, cases[1].W, cin, cout, 3, 3, stride, 1, 1, groups) == 1

    def launch(xs, gys, outs, beta):
        jobs = (_lib.Wg3Job * 2)()
        for j, c, x, gy, o in zip(jobs, cases, xs, gys, outs):
            j.x, j.dy, j.dw = dconv.nptr(x), dconv.nptr(gy), o.data_ptr()
            dconv._fill_wg3(j, wgrad_dims(c))
        need = L.danet_conv_wgrad3x3_multi_ws_floats(ctypes.addressof(jobs), 2)
        ws = torch.full((max(int(need), 1),), float('nan'), device='cuda')
        dconv.check(L.danet_conv_wgrad3x3_multi(ctypes.addressof(jobs), 2, ptr(ws), need, beta, stream()), 'danet_conv_wgrad3x3_multi')
    _three_ways(cases, kind, launch)


@pytest.mark.parametrize('kind', KINDS)
def test_pointwise_weight_gradients_in_one_call(kind):
    """Several 1x1 / stride-1 layers in one danet_conv_wgrad_multi call: three on csrc/conv_pw_wgrad.hip, 40 -> 72 (no pointwise plan) on
    the generic kernel next to them."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib.lib()
    cases = [W('conv_pw_wgrad_multi' if (ci, co) != (40, 72) else 'conv_wgrad_1_multi', 'multi', ci, co, 1, 1, 0, 1, 1, h, w, b) for ci, co, h, w, b in PW_MULTI]
    assert [_pointwise(c) for c in cases] == [True, True, False, True]

    def launch(xs, gys, outs, beta):
        jobs = _wg_table(cases, xs, gys, outs)
        need = L.danet_conv_wgrad_multi_ws_floats(ctypes.addressof(jobs), len(cases))
        zero_from = L.danet_conv_wgrad_multi_ws_zero_from(ctypes.addressof(jobs), len(cases))
        assert 0 < zero_from < need
        ws = torch.full((need,), float('nan'), device='cuda')           # the pointwise partial sums need no zeroing ...
        ws[zero_from:].zero_()                                          # ... the packed accumulators behind them do (include/danet_hip.h)
        dconv.check(L.danet_conv_wgrad_multi(ctypes.addressof(jobs), len(cases), ptr(ws), need, beta, stream()), 'danet_conv_wgrad_multi')
    _three_ways(cases, kind, launch)


# ---- bias gradient ---------------------------------------------------------------------------------------------------------------
BIAS = [(5, 32, 33, 17), (3, 24, 9, 7), (4, 64, 96, 96)]          # the last: 2 359 296 elements, past the 2^21 replica threshold


def bias_reference(gy):
    """gy.sum(dim = (0, 2, 3)) in fp64 as a Reference [1, C, 1, 1]: K = B * H * W terms, S = sum |gy|."""
    r = gy.double().sum(dim=(0, 2, 3)).view(1, -1, 1, 1)
    return Reference(r, r, gy.double().abs().sum(dim=(0, 2, 3)).view(1, -1, 1, 1), gy.shape[0] * gy.shape[2] * gy.shape[3], None, False)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', BIAS, ids=lambda s: 'x'.join(map(str, s)))
def test_bias_gradient(shape, kind):
    """conv.channel_sum (csrc/norm_act.hip channel_sum_kernel: fp32 partial sums per thread, combined in double accumulators, 16
    replicas for large maps) against the fp64 sum: equal on integers, within the bound of a sum of K = B * H * W terms (u = U_F32)
    on random operands."""
    from danet_densepose2smpl_amd import conv as dconv
    g = torch.Generator().manual_seed(sum(shape))
    assert (shape[0] * shape[1] * shape[2] * shape[3] >= 1 << 21) == (shape == BIAS[-1])
    gy = int_operands(shape, -2, 2, g) if kind == 'int' else torch.randn(shape, generator=g).bfloat16().float()
    out = dconv.channel_sum(dconv.nhwc_bf16(gy.cuda())).cpu()
    ref = bias_reference(gy)
    assert out.dtype == torch.float32 and out.numel() == shape[1]
    if kind == 'int':
        assert 2 * shape[0] * shape[2] * shape[3] < 2 ** 24 and torch.equal(out.double().view_as(ref.r), ref.r)
    else:
        elem = ratios(out.view_as(ref.r), ref, U_F32)[0]
        _note('channel_sum', 'x'.join(map(str, shape)), elem)
        assert elem <= 1.0
