"""The split-K finish of the weight-gradient kernels (csrc/wgrad_finish.h): dW = beta * dW + the partial blocks, summed in a fixed order
and written in the torch layout.

(a) Exact order.  danet_conv_wgrad3x3 with phase = 1 leaves part[split][g][tap][cout][cin] in the workspace; the expected dW is built
    from those partials in torch, in fp32 on the device, with the association the kernel promises --
        s = 0;  s += (v0 + v1) + (v2 + v3) for each full group of four splits;  then the remaining splits one by one;  then beta
    -- and phase = 2 must give the same bits (torch.equal).  The split count is set with DANET_WGRAD3_BLOCKS.  The planner caps it at a
    quarter of the 4 x 8-pixel chunks, so B = 2 with 8 x 8 and 8 x 16 maps reaches one and two splits only; the splits 3, 4, 7 and 36
    (the group-of-four tail and the split lanes of a workgroup) run on 48 x 48 maps (144 chunks).
(b) Exact integers.  Operands in {-2 .. 2}: every partial and every sum is an integer below 2^24, exact in fp32 in any order, so dW must
    EQUAL the fp64 gradient of F.conv2d's autograd -- for 45 jobs in one danet_conv_wgrad3x3_multi call (several MFMA launch groups,
    direct and split jobs, more problems than one finish launch takes), for a pointwise queue and a 7x7 / stride-2 problem through
    danet_conv_wgrad_multi, and for the filter-row kernel; twice, with identical bits, and with beta = 1 onto a known tensor.
(c) Destination edges.  Element counts Cout_g * Cin_g one 64-element step short of a workgroup's run and one step over it, gradients
    that are and are not 16-byte aligned, inside a poisoned guard band that must stay untouched."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

POISON = -12345.0


def _lib_():
    from danet_densepose2smpl_amd import _lib
    return _lib.lib()


class _Blocks:
    """DANET_WGRAD3_BLOCKS for the duration of a block (the planner reads it at every call)."""
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get('DANET_WGRAD3_BLOCKS')
        os.environ['DANET_WGRAD3_BLOCKS'] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            del os.environ['DANET_WGRAD3_BLOCKS']
        else:
            os.environ['DANET_WGRAD3_BLOCKS'] = self.old


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def _autograd_wgrad(x, gy, wshape, stride, pad, groups):
    """fp64 d conv2d(x, w) / dw applied to gy, on the CPU."""
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, stride, pad, 1, groups).backward(gy.double())
    return w.grad


def _guarded(n, offset_floats=0):
    """An n-float gradient inside a poisoned buffer: (buffer, view, first index); offset_floats shifts it off 16-byte alignment."""
    guard = 64 + offset_floats
    buf = torch.full((n + 2 * guard,), POISON, device='cuda')
    return buf, buf[guard:guard + n], guard


def _band_intact(buf, first, n):
    return bool((buf[:first] == POISON).all()) and bool((buf[first + n:] == POISON).all())


def _ordered_sum(part):
    """part [split, ...] -> the finish kernel's sum, fp32 on the device."""
    s = torch.zeros_like(part[0])
    ms = part.shape[0]
    k = 0
    while k + 4 <= ms:
        s = s + ((part[k] + part[k + 1]) + (part[k + 2] + part[k + 3]))
        k += 4
    while k < ms:
        s = s + part[k]
        k += 1
    return s


# ---- (a) exact order --------------------------------------------------------------------------------------------------------------
CHANNELS = [(16, 16, 1), (40, 24, 1), (96, 48, 2)]
# (H, W, wanted splits)
ORDER = [(8, 8, 1), (8, 16, 1), (8, 16, 2), (48, 48, 1), (48, 48, 3), (48, 48, 4), (48, 48, 7), (48, 48, 36)]


def _blocks_for(L, B, H, W, cin, cout, groups, want):
    """DANET_WGRAD3_BLOCKS that makes the planner split `want` ways: it takes ceil(blocks / channel blocks) splits."""
    cgw = cout * (cin // groups) * 9
    with _Blocks(1 << 20):
        cap = L.danet_conv_wgrad3x3_ws_floats(B, H, W, cin, cout, groups, 1) // cgw
    assert want <= cap, (want, cap)
    for blocks in range(1, 64 * want + 1):
        with _Blocks(blocks):
            if L.danet_conv_wgrad3x3_ws_floats(B, H, W, cin, cout, groups, 1) // cgw == want:
                return blocks
    raise AssertionError('no DANET_WGRAD3_BLOCKS gives %d splits' % want)


@pytest.mark.parametrize('beta', [0.0, 1.0])
@pytest.mark.parametrize('H,W,ms', ORDER, ids=lambda v: str(v))
@pytest.mark.parametrize('cin,cout,groups', CHANNELS, ids=lambda v: str(v))
def test_finish_sums_the_partials_in_the_promised_order(cin, cout, groups, H, W, ms, beta):
    from danet_densepose2smpl_amd import conv as dconv
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib_()
    B = 2
    assert L.danet_conv_wgrad3x3_ok(H, W, cin, cout, 3, 3, 1, 1, 1, groups) == 1
    g = torch.Generator().manual_seed(cin + cout + H + W + ms)
    x = dconv.nhwc_bf16(torch.randn((B, cin, H, W), generator=g).cuda())
    gy = dconv.nhwc_bf16(torch.randn((B, cout, H, W), generator=g).cuda())
    cin_g, cout_g = cin // groups, cout // groups
    n = cout * cin_g * 9
    init = torch.randn((n,), generator=g).cuda()
    with _Blocks(_blocks_for(L, B, H, W, cin, cout, groups, ms)):
        nws = L.danet_conv_wgrad3x3_ws_floats(B, H, W, cin, cout, groups, 1)
        assert nws == ms * n
        for off in (0, 1):                                       # a 16-byte aligned gradient and one that is not
            ws = torch.full((nws,), float('nan'), device='cuda')
            buf, dw, first = _guarded(n, off)
            dw.copy_(init if beta else torch.full_like(init, float('nan')))
            args = (dconv.nptr(x), dconv.nptr(gy), ptr(dw), ptr(ws), nws, B, H, W, cin, cout, groups, 1, beta)
            dconv.check(L.danet_conv_wgrad3x3(*args, 1, stream()), 'danet_conv_wgrad3x3')
            torch.cuda.synchronize()
            part = ws.clone().view(ms, groups, 9, cout_g, cin_g)
            assert torch.isfinite(part).all()
            dconv.check(L.danet_conv_wgrad3x3(*args, 2, stream()), 'danet_conv_wgrad3x3')
            torch.cuda.synchronize()
            s = _ordered_sum(part).permute(0, 2, 3, 1).reshape(n)           # [g][cout][cin][tap]
            want = init * beta + s if beta else s
            assert torch.equal(dw, want), (off, int((dw != want).sum()))
            assert _band_intact(buf, first, n), off


# ---- (b) exact integers through the multi-problem paths ---------------------------------------------------------------------------
# (B, cin, cout, groups, input side, stride)
def _multi3_jobs():
    jobs = []
    for c in (16, 48, 96, 192):
        jobs += [(2, c, c, 1, 16, 1), (2, c, c, 1, 8, 1), (2, c, c, 1, 16, 2)]                 # split, direct (4 chunks), stride 2
    jobs += [(2, 96, 48, 2, 16, 1), (2, 96, 48, 2, 16, 2), (2, 48, 16, 1, 16, 1), (2, 16, 48, 1, 16, 1), (2, 40, 24, 1, 16, 1)]
    jobs += [(8, 16, 16, 1, 4, 1), (8, 48, 48, 1, 4, 1), (8, 64, 32, 1, 8, 2), (8, 96, 48, 2, 4, 1)]      # 4 x 4 outputs: image pairs
    jobs += [(8, 64, 32, 1, 2, 1), (8, 48, 48, 1, 4, 2), (8, 96, 96, 1, 2, 1)]                             # 2 x 2 outputs: eight per chunk
    jobs += [(2, 24, 40, 1, 16, 1), (2, 136, 8, 1, 16, 1), (2, 8, 136, 1, 16, 1), (4, 16, 16, 1, 32, 1), (4, 16, 16, 1, 32, 2)]
    k = 0
    while len(jobs) < 45:                                                                                   # more of the narrow layers
        jobs.append((2 + 2 * (k % 2), (16, 32, 48)[k % 3], (16, 24, 32, 48)[k % 4], 1, 16, 1 + k % 2))
        k += 1
    return jobs


def _run_multi3(specs, xs, gys, inits, beta, offset):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib.lib()
    jobs = (_lib.Wg3Job * len(specs))()
    held = []
    for j, (B, cin, cout, groups, side, stride), x, gy, init in zip(jobs, specs, xs, gys, inits):
        n = init.numel()
        buf, dw, first = _guarded(n, offset)
        dw.copy_(init.cuda().view(-1) if beta else torch.full((n,), float('nan'), device='cuda'))
        held.append((buf, dw, first, n))
        j.x, j.dy, j.dw = dconv.nptr(x), dconv.nptr(gy), dw.data_ptr()
        j.B, j.H, j.W, j.Cin, j.Cout, j.groups, j.stride = B, side, side, cin, cout, groups, stride
    need = L.danet_conv_wgrad3x3_multi_ws_floats(ctypes.addressof(jobs), len(specs))
    ws = torch.full((max(int(need), 1),), float('nan'), device='cuda')
    dconv.check(L.danet_conv_wgrad3x3_multi(ctypes.addressof(jobs), len(specs), ptr(ws), need, beta, stream()), 'danet_conv_wgrad3x3_multi')
    torch.cuda.synchronize()
    for buf, dw, first, n in held:
        assert _band_intact(buf, first, n)
    return [h[1].cpu() for h in held]


def test_exact_integers_through_45_jobs_in_one_3x3_call():
    from danet_densepose2smpl_amd import conv as dconv
    L = _lib_()
    specs = _multi3_jobs()
    assert len(specs) == 45
    g = torch.Generator().manual_seed(45)
    xs, gys, inits, refs = [], [], [], []
    for B, cin, cout, groups, side, stride in specs:
        assert L.danet_conv_wgrad3x3_ok(side, side, cin, cout, 3, 3, stride, 1, 1, groups) or \
            L.danet_conv_wgrad3x3_pair_ok(B, side, side, cin, cout, 3, 3, stride, 1, 1, groups), (B, cin, cout, groups, side, stride)
        o = side // stride
        assert 4 * B * o * o + 3 < 2 ** 24
        x, gy = _ints((B, cin, side, side), -2, 2, g), _ints((B, cout, o, o), -2, 2, g)
        wshape = (cout, cin // groups, 3, 3)
        refs.append(_autograd_wgrad(x, gy, wshape, stride, 1, groups))
        inits.append(_ints(wshape, -3, 3, g))
        xs.append(dconv.nhwc_bf16(x.cuda()))
        gys.append(dconv.nhwc_bf16(gy.cuda()))
    a = _run_multi3(specs, xs, gys, inits, 0.0, 0)              # (beta = 0: the jobs of one split go straight into dW)
    b = _run_multi3(specs, xs, gys, inits, 0.0, 1)
    acc = _run_multi3(specs, xs, gys, inits, 1.0, 0)            # (beta = 1: all 45 through the finish kernel, two launches)
    for spec, ya, yb, yc, ref, init in zip(specs, a, b, acc, refs, inits):
        assert torch.equal(ya, yb), spec
        assert torch.equal(ya.double().view_as(ref), ref), (spec, int((ya.double().view_as(ref) != ref).sum()))
        assert torch.equal(yc.double().view_as(ref), ref + init.double()), spec


# (cin, cout, k, stride, pad, H, W, B): a pointwise queue (the last has no pointwise plan) and one 7x7 / stride-2 problem
GENERIC = [(64, 256, 1, 1, 0, 32, 32, 4), (24, 64, 1, 1, 0, 32, 32, 4), (64, 24, 1, 1, 0, 64, 32, 2), (40, 72, 1, 1, 0, 32, 32, 4),
           (16, 64, 7, 2, 3, 16, 16, 2)]


def _run_generic(specs, xs, gys, inits, beta, offset):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib.lib()
    jobs = (_lib.WgJob * len(specs))()
    held = []
    for j, (cin, cout, k, stride, pad, H, W, B), x, gy, init in zip(jobs, specs, xs, gys, inits):
        n = init.numel()
        buf, dw, first = _guarded(n, offset)
        dw.copy_(init.cuda().view(-1) if beta else torch.full((n,), float('nan'), device='cuda'))
        held.append((buf, dw, first, n))
        j.x, j.dy, j.dw = dconv.nptr(x), dconv.nptr(gy), dw.data_ptr()
        dconv._fill_wg(j, (B, H, W, cin, gy.shape[2], gy.shape[3], cout, k, k, stride, pad, 1, 1))
    need = L.danet_conv_wgrad_multi_ws_floats(ctypes.addressof(jobs), len(specs))
    zero_from = L.danet_conv_wgrad_multi_ws_zero_from(ctypes.addressof(jobs), len(specs))
    ws = torch.full((need,), float('nan'), device='cuda')
    ws[zero_from:].zero_()
    dconv.check(L.danet_conv_wgrad_multi(ctypes.addressof(jobs), len(specs), ptr(ws), need, beta, stream()), 'danet_conv_wgrad_multi')
    torch.cuda.synchronize()
    for buf, dw, first, n in held:
        assert _band_intact(buf, first, n)
    return [h[1].cpu() for h in held]


def test_exact_integers_through_a_pointwise_queue_and_a_7x7_problem():
    from danet_densepose2smpl_amd import conv as dconv
    g = torch.Generator().manual_seed(7)
    xs, gys, inits, refs = [], [], [], []
    for cin, cout, k, stride, pad, H, W, B in GENERIC:
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        assert 4 * B * oh * ow + 3 < 2 ** 24
        x, gy = _ints((B, cin, H, W), -2, 2, g), _ints((B, cout, oh, ow), -2, 2, g)
        refs.append(_autograd_wgrad(x, gy, (cout, cin, k, k), stride, pad, 1))
        inits.append(_ints((cout, cin, k, k), -3, 3, g))
        xs.append(dconv.nhwc_bf16(x.cuda()))
        gys.append(dconv.nhwc_bf16(gy.cuda()))
    a = _run_generic(GENERIC, xs, gys, inits, 0.0, 0)
    b = _run_generic(GENERIC, xs, gys, inits, 0.0, 1)
    acc = _run_generic(GENERIC, xs, gys, inits, 1.0, 0)
    for spec, ya, yb, yc, ref, init in zip(GENERIC, a, b, acc, refs, inits):
        assert torch.equal(ya, yb), spec
        assert torch.equal(ya.double().view_as(ref), ref), spec
        assert torch.equal(yc.double().view_as(ref), ref + init.double()), spec


def test_exact_integers_through_the_filter_row_kernel():
    """7x7 / stride 2 at the smallest size danet_conv_wgrad_rows takes (B * OH * OW = 65536): 49 taps, 147 splits."""
    from danet_densepose2smpl_amd import conv as dconv
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib_()
    B, cin, cout, H = 64, 8, 16, 64
    oh = 32
    assert L.danet_conv_wgrad_rows_ok(B, H, H, cin, oh, oh, cout, 7, 7, 2, 3, 1, 1) == 1 and 4 * B * oh * oh + 3 < 2 ** 24
    g = torch.Generator().manual_seed(49)
    x, gy, init = _ints((B, cin, H, H), -2, 2, g), _ints((B, cout, oh, oh), -2, 2, g), _ints((cout, cin, 7, 7), -3, 3, g)
    ref = _autograd_wgrad(x, gy, init.shape, 2, 3, 1)
    xd, gyd = dconv.nhwc_bf16(x.cuda()), dconv.nhwc_bf16(gy.cuda())
    nws = L.danet_conv_wgrad_rows_ws_floats(B, oh, oh, cin, cout, 7, 7, 1)
    n = init.numel()
    assert nws // n > 32                                          # (the split lanes of the finish kernel are in use)
    outs = []
    for beta, off in ((0.0, 0), (0.0, 1), (1.0, 0)):
        buf, dw, first = _guarded(n, off)
        dw.copy_(init.cuda().view(-1) if beta else torch.full((n,), float('nan'), device='cuda'))
        ws = torch.full((nws,), float('nan'), device='cuda')
        dconv.check(L.danet_conv_wgrad_rows(dconv.nptr(xd), dconv.nptr(gyd), ptr(dw), ptr(ws), nws, B, H, H, cin, oh, oh, cout, 7, 7, 2, 3, 1,
                                            beta, stream()), 'danet_conv_wgrad_rows')
        torch.cuda.synchronize()
        assert _band_intact(buf, first, n)
        outs.append(dw.cpu().double().view_as(ref))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ref) and torch.equal(outs[2], ref + init.double())


# ---- (c) destination edges --------------------------------------------------------------------------------------------------------
# Cout_g * Cin_g against a workgroup's run of 1024 elements (two splits: one split lane) and of 128 (36 splits: eight lanes): one
# 64-element step short of a multiple (960 = 40 x 24), one step over (1088 = 8 x 136 and 136 x 8), and across groups
EDGES = [(24, 40, 1), (40, 24, 1), (136, 8, 1), (8, 136, 1), (80, 48, 2), (16, 16, 1), (24, 8, 1)]


@pytest.mark.parametrize('ms', [2, 36])
@pytest.mark.parametrize('cin,cout,groups', EDGES, ids=lambda v: str(v))
def test_destination_edges_inside_a_guard_band(cin, cout, groups, ms):
    from danet_densepose2smpl_amd import conv as dconv
    from danet_densepose2smpl_amd._lib import ptr, stream
    L = _lib_()
    B, H, W = 2, 48, 48
    assert 4 * B * H * W + 3 < 2 ** 24
    g = torch.Generator().manual_seed(cin * cout + ms)
    x, gy = _ints((B, cin, H, W), -2, 2, g), _ints((B, cout, H, W), -2, 2, g)
    wshape = (cout, cin // groups, 3, 3)
    init = _ints(wshape, -3, 3, g)
    ref = _autograd_wgrad(x, gy, wshape, 1, 1, groups)
    xd, gyd = dconv.nhwc_bf16(x.cuda()), dconv.nhwc_bf16(gy.cuda())
    n = init.numel()
    with _Blocks(_blocks_for(L, B, H, W, cin, cout, groups, ms)):
        nws = L.danet_conv_wgrad3x3_ws_floats(B, H, W, cin, cout, groups, 1)
        assert nws == ms * n
        for beta, off in ((0.0, 0), (0.0, 3), (1.0, 0), (1.0, 2)):
            buf, dw, first = _guarded(n, off)
            dw.copy_(init.cuda().view(-1) if beta else torch.full((n,), float('nan'), device='cuda'))
            ws = torch.full((nws,), float('nan'), device='cuda')
            dconv.check(L.danet_conv_wgrad3x3(dconv.nptr(xd), dconv.nptr(gyd), ptr(dw), ptr(ws), nws, B, H, W, cin, cout, groups, 1, beta, 0,
                                              stream()), 'danet_conv_wgrad3x3')
            torch.cuda.synchronize()
            assert _band_intact(buf, first, n), (beta, off)
            want = ref + init.double() if beta else ref
            assert torch.equal(dw.cpu().double().view_as(ref), want), (beta, off)
