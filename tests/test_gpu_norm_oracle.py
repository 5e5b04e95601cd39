"""csrc/norm_act.hip -- BatchNorm (+ residual) (+ ReLU) forward and backward (two kernels and one pass), the per-channel sum and
the HRNet fuse sum with its window-sum gradients, bf16 and fp32 builds -- against the float64 restatements of
tests/norm_oracle.py (checked against torch in tests/test_norm_oracle_host.py), at the shapes where make_map, the slab loop and
the one-pass planner branch (norm_oracle.BN_CASES, ONEPASS_CASES, FUSE_CASES: one line each on what a case exists for; the host
test recomputes every such claim).

Bounded tests assert err <= bound elementwise with the bounds of norm_oracle's docstring -- derived from the kernels' arithmetic,
nothing tuned; rsqrtf is ASSUMED accurate to 2 units in the last place -- and record max(err / bound) through
conftest.record('norm_oracle').  Exact tests use `==`: integer inputs whose partial sums stay below 2^24 (dy is integer-valued in
EVERY BatchNorm case, so dbeta and dres are exact everywhere), the saved mean at power-of-two M, the fuse sums, the byte mask
wherever |v_ref| exceeds the forward bound, and the three ReLU gate sources against each other in one-workgroup launches.

The forward, the two-kernel backward, danet_channel_sum and the fuse kernels are called through their C entry points, so that the
test owns the outputs: each sits between two guard bands of sentinel elements and starts out as NaN (bytes: 0xFF); after the launch
the guards are intact and nothing is left unwritten -- the out-of-range offsets of rows past the end are dropped by the hardware.
The one-pass kernel is reached only the way the library reaches it: nn.BatchNorm2d / nn.multi_batch_norm under nn.ONEPASS and
nn.ONEPASS_MAX_BLOCKS, with the path that ran asserted from conv.FUSION['bn_bwd_onepass'] and the barrier's error word clear.

Measured on an MI355X, max err / bound over the cases of a group (bf16 | fp32):
                        mean          invstd        y             running mean  running var   dx            dgamma
  direct, C <= 40       0.018 | 0.071 0.065 | 0.092 0.981 | 0.104 0.081 | 0.125 0.466 | 0.328 0.987 | 0.175 0.051 | 0.052
  direct, C = 48 grids  0.041 | 0.053 0.064 | 0.074 0.996 | 0.249 0.193 | 0.092 0.400 | 0.356 0.996 | 0.290 0.009 | 0.013
  direct, C >= 1024     0.148 | 0.510 0.200 | 0.296 0.996 | 0.313 0.492 | 0.443 0.670 | 0.709 0.996 | 0.380 0.223 | 0.300
  offset statistics     0.000 | 0.112 0.012 | 0.280 0.872 | 0.142 0.016 | 0.194 0.012 | 0.095 0.988 | 0.072 0.006 | 0.006
  one pass (bf16)       -             -             0.995         -             -             0.996         0.154
  multi_batch_norm      0.031         0.071         0.990         -             -             0.994         0.066
  eval mode y 0.946 | 0.661; channel_sum 0.003 | 0.286; fuse sum y 0.996 | 0.573, window sums 0.981 | 0.622; excluded gates <= 0.08 %.
bf16 y / dx / window sums sit just below 1 because the 2^-8 |ref| term IS the rounding of the stored value (half a unit in the last
place is attained; truncation measures 1.98).  The statistics of the narrow tensors sit at a few percent: k counts the rpb = 85 or 256
lanes of block_channel_reduce as worst-case roundings that add up, where they behave as a random walk, and sums of 8-bit bf16 values in
24-bit accumulators mostly do not round at all (channel_sum 0.003).  The constant channel's invstd is within 0.23 (bf16) / 0.35 (fp32)
of the root's own allowance: rsqrtf measured below one unit in the last place, two assumed.  Under a mean of 16 spreads the bf16
build's invstd is off by 2.5e-5 relative, the fp32 build's by 8.5e-7."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from conftest import record
import norm_oracle as no

pytestmark = pytest.mark.gpu

GUARD = 4096
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
BIG_KNOB = 1 << 30          # block bytes above every tensor here: one workgroup per launch


def _L():
    from danet_densepose2smpl_amd import _lib
    return _lib.lib()


def _entry(name, dtype):
    return getattr(_L(), name + ('_f32' if dtype == torch.float32 else ''))


def _call(name, dtype, *args):
    from danet_densepose2smpl_amd._lib import check, stream
    check(_entry(name, dtype)(*args, stream()), name)
    torch.cuda.synchronize()


def _p(t):
    from danet_densepose2smpl_amd._lib import ptr
    return ptr(t.out if isinstance(t, Guarded) else t)


class Guarded(object):
    """An output of `shape` between two sentinel bands; floats start as NaN, bytes as 0xFF (a written mask byte is < 16); `init`
    (in-place updated buffers) starts as a copy of it."""

    def __init__(self, shape, dtype, init=None):
        self.n = int(np.prod(shape))
        self.bytes = dtype == torch.uint8
        self.sentinel = 0xA5 if self.bytes else -7.0
        self.buf = torch.full((self.n + 2 * GUARD,), self.sentinel, dtype=dtype, device='cuda')
        self.out = self.buf[GUARD:GUARD + self.n].view(*shape)
        if init is not None:
            self.out.copy_(init)
        else:
            self.out.fill_(0xFF if self.bytes else float('nan'))

    def written(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n:] == self.sentinel).all()), 'a guard band was written'
        if self.bytes:
            assert bool((self.out < 16).all()), 'a mask byte was never written'
        else:
            assert not bool(torch.isnan(self.out).any()), 'an output element was never written'
        return self.out


def _device(a, dtype):
    """float64 values -> the device tensor of `dtype`, which must hold exactly these values (the oracle's own rounding)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).cuda()
    assert np.array_equal(_h64(t), a), 'the device tensor does not hold the values the oracle was given'
    return t


def _h64(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype != torch.float64 else t.cpu().numpy()


@contextlib.contextmanager
def block_bytes(knob):
    """The BatchNorm kernels' bytes-per-workgroup knob at `knob` (None: the default the oracle's plans assume) inside, restored after."""
    L = _L()
    prev = L.danet_bn_set_block_bytes(knob or no.BLOCK_BYTES)
    try:
        yield
    finally:
        L.danet_bn_set_block_bytes(prev)


def _ws(C):
    return torch.empty(_L().danet_bn_ws_floats(C), dtype=torch.float32, device='cuda')


def bn_fwd(x, res, gamma, beta, rm, rv, training, relu, want_mask, M, C):
    """Direct launch of danet_bn_forward -> y, saved [2, C] (training), mask bytes, running mean / var (all guarded, checked)."""
    y = Guarded((M, C), x.dtype)
    saved = Guarded((2, C), torch.float32) if training else None
    mask = Guarded((M * C // 4,), torch.uint8) if want_mask else None
    grm = None if rm is None else Guarded((C,), torch.float32, init=rm)
    grv = None if rv is None else Guarded((C,), torch.float32, init=rv)
    _call('danet_bn_forward', x.dtype, _p(x), None if res is None else _p(res), _p(y), M, C, None if gamma is None else _p(gamma),
          None if beta is None else _p(beta), None if grm is None else _p(grm), None if grv is None else _p(grv),
          None if saved is None else _p(saved), _p(_ws(C)) if training else None, 0, no.MOMENTUM, no.EPS, int(training), int(relu),
          None if mask is None else _p(mask))
    return no.Obj(y=y.written(), saved=None if saved is None else saved.written(), mask=None if mask is None else mask.written(),
                  rm=None if grm is None else grm.written(), rv=None if grv is None else grv.written())


def bn_bwd(dy, x, y, gamma, beta, saved, relu, mask_mode, mask, want_dres, M, C):
    """Direct launch of danet_bn_backward (reduce + apply kernels) -> dx, dres, dparam [2, C]."""
    dx = Guarded((M, C), x.dtype)
    dres = Guarded((M, C), x.dtype) if want_dres else None
    dparam = Guarded((2, C), torch.float32)
    _call('danet_bn_backward', x.dtype, _p(dy), _p(x), None if y is None else _p(y), M, C, None if gamma is None else _p(gamma), _p(saved),
          int(relu), _p(dx), None if dres is None else _p(dres), _p(dparam), _p(_ws(C)), 0, int(mask_mode), None if mask is None else _p(mask),
          None if beta is None else _p(beta))
    return no.Obj(dx=dx.written(), dres=None if dres is None else dres.written(), dparam=dparam.written())


def _finish(meas):
    record('norm_oracle', meas)
    print('norm_oracle %s' % meas)
    bad = ['%s err / bound = %.3g' % (k, v) for k, v in meas.items() if isinstance(v, float) and k != 'excluded' and v > 1.0]
    assert not bad, '%s: %s' % (meas['case'], '; '.join(bad))


def check_forward(i, o, fw, k, dtype_name, M, relu, meas):
    """The training forward's saved statistics, y, running statistics and byte mask against the oracle `o`."""
    dm, dvar = no.stats_bound(i.x, dtype_name, k)
    dinv = no.invstd_bound(o.var, no.EPS, dvar, dtype_name)
    saved = _h64(fw.saved)
    meas['mean'] = no.ratio(np.abs(saved[0] - o.mean), dm)
    meas['invstd'] = no.ratio(np.abs(saved[1] - o.invstd), dinv)
    bound = no.forward_bound(i.x, i.res, i.gamma, i.beta, o, dm, dinv, dtype_name)
    meas['y'] = no.ratio(np.abs(_h64(fw.y) - o.y), bound)
    nrm, nrv = no.running_update(i.rm, i.rv, o.mean, o.var, M, no.MOMENTUM)
    brm, brv = no.running_bound(i.rm, i.rv, o.mean, o.var, M, no.MOMENTUM, dm, dvar)
    meas['running_mean'] = no.ratio(np.abs(_h64(fw.rm) - nrm), brm)
    meas['running_var'] = no.ratio(np.abs(_h64(fw.rv) - nrv), brv)
    if fw.mask is not None:
        sure = (np.abs(o.v) > bound).reshape(-1, 4).all(1)
        meas['excluded'] = float(1.0 - (np.abs(o.v) > bound).mean())
        assert meas['excluded'] <= 0.01
        got = fw.mask.cpu().numpy()
        assert np.array_equal(got[sure], no.mask_bytes(o.v)[sure]), 'a ReLU mask byte differs where the reference is not in doubt'
        if relu:
            assert np.array_equal(got, no.mask_bytes(_h64(fw.y))), 'the byte mask is not the gate of the written y'


def check_backward(i, dy, x, gate, saved, bwd, k, dtype_name, meas, dparam=None):
    """dx (bounded), dbeta (exact: dy is integer-valued), dgamma (bounded), dres (exact), with the kernel's own saved statistics."""
    sv = _h64(saved)
    bw = no.bn_backward(i.dy, i.x, gate, i.gamma, sv[0], sv[1])
    bb = no.backward_bound(i.gamma, sv[1], bw, k, dtype_name)
    meas['dx'] = no.ratio(np.abs(_h64(bwd.dx) - bw.dx), bb.dx)
    dp = _h64(bwd.dparam if dparam is None else dparam)
    assert no.exact_sum_ok(bw.g)
    assert np.array_equal(dp[0], bw.dbeta), 'dbeta is a sum of integers: exact'
    meas['dgamma'] = no.ratio(np.abs(dp[1] - bw.dgamma), bb.dgamma)
    if bwd.dres is not None:
        assert torch.equal(bwd.dres, dy * torch.from_numpy(gate).to(dy.dtype).cuda()), 'dres is dy * gate, exactly'
    return bw


def _to_dev(i, dtype):
    f = lambda a: None if a is None else _device(a, torch.float32)
    return no.Obj(x=_device(i.x, dtype), res=None if i.res is None else _device(i.res, dtype), dy=_device(i.dy, dtype),
                  gamma=f(i.gamma), beta=f(i.beta), rm=f(i.rm), rv=f(i.rv))


def run_bn_case(C, M, name, knob, dtype_name, relu, use_res, kind='normal'):
    dtype = DTYPES[dtype_name]
    i = no.bn_inputs(C, M, name, dtype_name, use_res, kind)
    d = _to_dev(i, dtype)
    meas = {'case': '%s-%s%s%s%s' % (name, dtype_name, '-relu' if relu else '', '-res' if use_res else '', '' if kind == 'normal' else '-' + kind)}
    k = no.k_of(no.plan(M, C, dtype_name, knob))
    # the gate source of the backward: the byte mask with a residual, otherwise recomputed from x (bf16) or read from y (fp32)
    mode = 0 if not relu else 1 if use_res else 2 if dtype_name == 'bf16' else 0
    with block_bytes(knob):
        fw = bn_fwd(d.x, d.res, d.gamma, d.beta, d.rm, d.rv, True, relu, relu, M, C)
        bwd = bn_bwd(d.dy, d.x, fw.y if mode == 0 and relu else None, d.gamma, d.beta, fw.saved, relu, mode, fw.mask if mode == 1 else None,
                     use_res, M, C)
    o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, relu)
    check_forward(i, o, fw, k, dtype_name, M, relu, meas)
    gate = _h64(fw.y) > 0 if relu else np.ones((M, C), dtype=bool)
    check_backward(i, d.dy, d.x, gate, fw.saved, bwd, k, dtype_name, meas)
    return i, o, fw, meas


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('use_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case', no.BN_CASES, ids=lambda c: c.name)
def test_bn_vs_oracle(case, relu, use_res, dtype_name):
    _, _, _, meas = run_bn_case(case.C, case.M, case.name, case.knob, dtype_name, relu, use_res)
    _finish(meas)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('use_res', [False, True], ids=['nores', 'res'])
def test_bn_statistics_under_offset(use_res, dtype_name):
    """Every channel's mean is 16 times its spread (E[x^2] = 257 var: the bf16 build's E[x^2] - mean^2 cancels, the fp32 build's
    shifted sums do not), channel 1 is constant and M a power of two: its sums are exact, var = 0 and invstd = rsqrt(eps)."""
    name, C, M = no.OFFSET_CASE
    i, o, fw, meas = run_bn_case(C, M, name, None, dtype_name, True, use_res, 'offset')
    assert o.var[1] == 0.0 and (np.abs(o.mean / np.sqrt(o.var + 1e-30))[np.arange(C) != 1] > 8).all()
    sv = _h64(fw.saved)
    assert sv[0][1] == 2.0, 'the mean of 2^n equal powers of two is exact'
    fn = (2 * no.RSQRT_ULPS if dtype_name == 'bf16' else 2.0) * no.U           # the root alone: var + eps = eps exactly
    meas['invstd_const'] = float(abs(sv[1][1] * np.sqrt(no.EPS) - 1.0) / fn)
    meas['invstd_relerr'] = float(np.abs(sv[1] / o.invstd - 1.0).max())            # the figure itself, not a ratio: how much the path cancels
    _finish(meas)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'null_gamma_beta'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_bn_eval_mode_and_null_affine(training, affine, dtype_name):
    """Eval mode (running statistics, nothing saved, the buffers untouched) and NULL gamma / beta through the direct entry point."""
    C, M, name = 12, 86, 'c12_m86'
    dtype = DTYPES[dtype_name]
    i = no.bn_inputs(C, M, name + ('' if affine else '-na'), dtype_name, True)
    if not affine:
        i.gamma = i.beta = None
    d = _to_dev(i, dtype)
    meas = {'case': '%s-%s-%s-%s' % (name, dtype_name, 'train' if training else 'eval', 'affine' if affine else 'noaffine')}
    fw = bn_fwd(d.x, d.res, d.gamma, d.beta, d.rm, d.rv, training, True, training, M, C)
    if training:
        o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, True)
        k = no.k_of(no.plan(M, C, dtype_name))
        check_forward(i, o, fw, k, dtype_name, M, True, meas)
        bwd = bn_bwd(d.dy, d.x, None, d.gamma, d.beta, fw.saved, True, 1, fw.mask, True, M, C)
        check_backward(i, d.dy, d.x, _h64(fw.y) > 0, fw.saved, bwd, k, dtype_name, meas)
    else:
        o = no.bn_eval(i.x, i.res, i.gamma, i.beta, i.rm, i.rv, no.EPS, True)
        dinv = no.invstd_bound(o.var, no.EPS, 0.0, dtype_name)
        meas['y'] = no.ratio(np.abs(_h64(fw.y) - o.y), no.forward_bound(i.x, i.res, i.gamma, i.beta, o, 0.0, dinv, dtype_name))
        assert torch.equal(fw.rm, d.rm) and torch.equal(fw.rv, d.rv), 'eval mode must not touch the running statistics'
    _finish(meas)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', no.INT_CASES, ids=lambda c: c[0])
def test_bn_integer_inputs_exact(case, dtype_name):
    """Integer x, M a power of two: the saved mean is float32(mean64) bit for bit; dbeta and dres are exact (check_backward)."""
    name, C, M, knob = case
    dtype = DTYPES[dtype_name]
    i = no.bn_inputs(C, M, name, dtype_name, True, 'int')
    assert no.exact_sum_ok(i.x) and no.exact_sum_ok(i.x - i.x[0])
    d = _to_dev(i, dtype)
    with block_bytes(knob):
        fw = bn_fwd(d.x, d.res, d.gamma, d.beta, d.rm, d.rv, True, True, True, M, C)
        bwd = bn_bwd(d.dy, d.x, fw.y, d.gamma, d.beta, fw.saved, True, 0, None, True, M, C)
    mean32 = torch.from_numpy(i.x.mean(0).astype(np.float32)).cuda()
    assert torch.equal(fw.saved[0].view(torch.int32), mean32.view(torch.int32)), 'the mean of integers over 2^n rows is exact'
    meas = {'case': '%s-int-%s' % (name, dtype_name)}
    check_backward(i, d.dy, d.x, _h64(fw.y) > 0, fw.saved, bwd, no.k_of(no.plan(M, C, dtype_name, knob)), dtype_name, meas)
    _finish(meas)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('name', ['c12_m341', 'c48_m700_k512', 'c1028_m6'])
def test_bn_gate_sources_bit_identical(name, dtype_name):
    """One workgroup per launch (block bytes above the tensor size: the sums have a fixed order): the backward with the gate read
    from y, from the byte mask and recomputed from x gives bit-identical dx, dres and dparam."""
    c = no.BN_BY_NAME[name]
    dtype = DTYPES[dtype_name]
    i = no.bn_inputs(c.C, c.M, name, dtype_name, False)
    d = _to_dev(i, dtype)
    assert all(p.blocks == 1 for p in no.plan(c.M, c.C, dtype_name, BIG_KNOB))
    before = _L().knob('bn_block_bytes')
    with block_bytes(BIG_KNOB):
        fw = bn_fwd(d.x, None, d.gamma, d.beta, d.rm, d.rv, True, True, True, c.M, c.C)
        b0 = bn_bwd(d.dy, d.x, fw.y, d.gamma, d.beta, fw.saved, True, 0, None, True, c.M, c.C)
        b1 = bn_bwd(d.dy, d.x, None, d.gamma, d.beta, fw.saved, True, 1, fw.mask, True, c.M, c.C)
        b2 = bn_bwd(d.dy, d.x, None, d.gamma, d.beta, fw.saved, True, 2, None, False, c.M, c.C)
    as_bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    for other in (b1, b2):
        assert torch.equal(as_bits(b0.dx), as_bits(other.dx)) and torch.equal(as_bits(b0.dparam), as_bits(other.dparam))
    assert torch.equal(as_bits(b0.dres), as_bits(b1.dres))
    assert _L().knob('bn_block_bytes') == before, 'the block-bytes knob was not restored'


# ---------------------------------------------------------------------------------------------------------------- channel sum
@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', no.CHSUM_CASES, ids=lambda c: c[0])
def test_channel_sum_exact_and_bounded(case, dtype_name):
    name, C, M, knob, ncopy, blocks, k1 = case
    dtype = DTYPES[dtype_name]
    p = no.plan(M, C, dtype_name, knob, cap=1024 if ncopy >= 4 else 256)
    meas = {'case': 'chsum-%s-%s' % (name, dtype_name)}
    for kind in ('int', 'normal'):
        i = no.bn_inputs(C, M, name, dtype_name, False, kind)
        x = _device(i.x, dtype)
        out = Guarded((ncopy, C), torch.float64)
        with block_bytes(knob):
            _call('danet_channel_sum', dtype, _p(x), M, C, _p(out), 0, ncopy)
        got = out.written().cpu().numpy().sum(0)
        if kind == 'int':
            assert no.exact_sum_ok(i.x) and np.array_equal(got, no.channel_sum(i.x)), 'a sum of integers below 2^24 is exact'
        else:
            bound = np.concatenate([no.channel_sum_bound(i.x[:, c0:c0 + q.Cs], q.k1, q.k2) for (c0, _), q in zip(no.slabs(C), p)])
            meas['sum'] = no.ratio(np.abs(got - no.channel_sum(i.x)), bound)
    _finish(meas)


# ------------------------------------------------------------------------------------------------------------------ one pass
@contextlib.contextmanager
def onepass(budget, on=True):
    from danet_densepose2smpl_amd import nn as dnn
    prev = (dnn.ONEPASS, dnn.ONEPASS_MAX_BLOCKS, dnn.ONEPASS_STREAM, dnn.RELU_MASK)
    dnn.ONEPASS, dnn.ONEPASS_MAX_BLOCKS, dnn.ONEPASS_STREAM, dnn.RELU_MASK = on, budget, None, True
    try:
        yield dnn
    finally:
        dnn.ONEPASS, dnn.ONEPASS_MAX_BLOCKS, dnn.ONEPASS_STREAM, dnn.RELU_MASK = prev


def _nchw(t, M, C):
    """[M, C] rows -> the [1, C, M, 1] tensor whose NHWC storage they are."""
    return t.view(1, M, 1, C).permute(0, 3, 1, 2)


def _module(dnn, i, C):
    bn = dnn.BatchNorm2d(C, momentum=no.MOMENTUM, eps=no.EPS).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(i.gamma)); bn.bias.copy_(torch.from_numpy(i.beta))
        bn.running_mean.copy_(torch.from_numpy(i.rm)); bn.running_var.copy_(torch.from_numpy(i.rv))
    return bn


def _rows_of(t, M, C):
    return t.permute(0, 2, 3, 1).contiguous().reshape(M, C)


def _check_module_backward(i, d, y, xt, rt, bn, M, C, k, meas, relu):
    sv = y._bn_ctx.saved
    gate = _h64(_rows_of(y.detach(), M, C)) > 0 if relu else np.ones((M, C), dtype=bool)
    bwd = no.Obj(dx=_rows_of(xt.grad, M, C), dres=None if rt is None else _rows_of(rt.grad, M, C))
    check_backward(i, d.dy, d.x, gate, sv, bwd, k, 'bf16', meas, dparam=torch.stack([bn.bias.grad, bn.weight.grad]))


def run_onepass_case(C, M, budget, expect_onepass, k1, relu, use_res, name):
    from danet_densepose2smpl_amd import conv as dconv
    i = no.bn_inputs(C, M, name, 'bf16', use_res)
    d = _to_dev(i, torch.bfloat16)
    meas = {'case': '%s-b%d-bf16%s%s' % (name, budget, '-relu' if relu else '', '-res' if use_res else '')}
    with onepass(budget) as dnn:
        bn = _module(dnn, i, C)
        xt = _nchw(d.x, M, C).clone(memory_format=torch.preserve_format).requires_grad_(True)
        rt = _nchw(d.res, M, C).clone(memory_format=torch.preserve_format).requires_grad_(True) if use_res else None
        before = dconv.FUSION['bn_bwd_onepass']
        y = bn(xt, res=rt, relu=relu)
        y.backward(_nchw(d.dy, M, C))
        torch.cuda.synchronize()
        assert dconv.FUSION['bn_bwd_onepass'] - before == int(expect_onepass), 'the backward took the other path'
        assert not dnn.onepass_error()
    o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, relu)
    kf = no.k_of(no.plan(M, C, 'bf16'))
    dm, dvar = no.stats_bound(i.x, 'bf16', kf)
    dinv = no.invstd_bound(o.var, no.EPS, dvar, 'bf16')
    meas['y'] = no.ratio(np.abs(_h64(_rows_of(y.detach(), M, C)) - o.y), no.forward_bound(i.x, i.res, i.gamma, i.beta, o, dm, dinv, 'bf16'))
    k = no.k_of(no.plan(M, C, 'bf16'), k1 if expect_onepass else None)
    _check_module_backward(i, d, y, xt, rt, bn, M, C, k, meas, relu)
    _finish(meas)


@pytest.mark.parametrize('use_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case', no.ONEPASS_CASES, ids=lambda c: 'm%d_b%d' % (c[0], c[1]))
def test_onepass_row_budget(case, relu, use_res):
    M, budget, rows, blocks, k1, why = case
    assert (no.onepass_plan(M, 48, budget) is not None) == (rows is not None)
    run_onepass_case(48, M, budget, rows is not None, k1, relu, use_res, 'op48_m%d' % M)


@pytest.mark.parametrize('use_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('CM', no.ONEPASS_WIDE, ids=lambda c: 'c%d_m%d' % c)
def test_onepass_wide_slabs(CM, use_res):
    C, M = CM
    assert no.onepass_k1(M, C) == M
    run_onepass_case(C, M, 0, True, M, True, use_res, 'c%d_m%d' % (C, M))


def test_multi_batch_norm_four_jobs():
    """nn.multi_batch_norm over four tensors of different C and M (bn_apply_multi_kernel, one one-pass launch of four jobs)."""
    from danet_densepose2smpl_amd import conv as dconv
    ins = [no.bn_inputs(C, M, 'multi_c%d_m%d' % (C, M), 'bf16', q % 2 == 1) for q, (C, M) in enumerate(no.MULTI_BN)]
    ds = [_to_dev(i, torch.bfloat16) for i in ins]
    with onepass(0) as dnn:
        bns = [_module(dnn, i, C) for i, (C, M) in zip(ins, no.MULTI_BN)]
        xs = [_nchw(d.x, M, C).clone(memory_format=torch.preserve_format).requires_grad_(True) for d, (C, M) in zip(ds, no.MULTI_BN)]
        rs = [None if d.res is None else _nchw(d.res, M, C).clone(memory_format=torch.preserve_format).requires_grad_(True)
              for d, (C, M) in zip(ds, no.MULTI_BN)]
        before = dconv.FUSION['bn_bwd_onepass']
        ys = dnn.multi_batch_norm(bns, xs, rs, relu=True)
        torch.autograd.backward(ys, [_nchw(d.dy, M, C) for d, (C, M) in zip(ds, no.MULTI_BN)])
        torch.cuda.synchronize()
        assert dconv.FUSION['bn_bwd_onepass'] - before == 4 and not dnn.onepass_error()
    for q, (C, M) in enumerate(no.MULTI_BN):
        i, meas = ins[q], {'case': 'multi-c%d_m%d-bf16' % (C, M)}
        o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, True)
        kf = no.k_of(no.plan(M, C, 'bf16'))
        dm, dvar = no.stats_bound(i.x, 'bf16', kf)
        dinv = no.invstd_bound(o.var, no.EPS, dvar, 'bf16')
        sv = _h64(ys[q]._bn_ctx.saved)
        meas['mean'], meas['invstd'] = no.ratio(np.abs(sv[0] - o.mean), dm), no.ratio(np.abs(sv[1] - o.invstd), dinv)
        meas['y'] = no.ratio(np.abs(_h64(_rows_of(ys[q].detach(), M, C)) - o.y), no.forward_bound(i.x, i.res, i.gamma, i.beta, o, dm, dinv, 'bf16'))
        k = no.k_of(no.plan(M, C, 'bf16'), no.onepass_k1(M, C))
        _check_module_backward(i, ds[q], ys[q], xs[q], rs[q], bns[q], M, C, k, meas, True)
        _finish(meas)


# ------------------------------------------------------------------------------------------------------------------ fuse sum
def _shape(c, s):
    return (c.B, c.H >> s, c.W >> s, c.C)


def fuse_fwd(terms, c, relu, dtype):
    n = len(terms)
    y = Guarded(_shape(c, 0), dtype)
    _call('danet_sum_relu_forward', dtype, (ctypes.c_void_p * n)(*[_p(t) for t in terms]), (ctypes.c_int * n)(*c.shifts), n,
          c.B, c.H, c.W, c.C, int(relu), _p(y))
    return y.written()


def fuse_bwd_all(gy, y, c, relu, wanted, dtype):
    d = {s: Guarded(_shape(c, s), dtype) for s in wanted}
    _call('danet_sum_relu_backward_all', dtype, _p(gy), _p(y), c.B, c.H, c.W, c.C, int(relu), *[_p(d[s]) if s in d else None for s in range(4)])
    return {s: g.written() for s, g in d.items()}


def fuse_bwd_one(gy, y, c, relu, s, dtype):
    d = Guarded(_shape(c, s), dtype)
    _call('danet_sum_relu_backward', dtype, _p(gy), _p(y), c.B, c.H, c.W, c.C, s, int(relu), _p(d))
    return d.written()


def _same(t, ref):
    return np.array_equal(_h64(t), ref)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'lin'])
@pytest.mark.parametrize('case', no.FUSE_CASES + [no.FUSE_BIG], ids=lambda c: c.name)
def test_fuse_sum_integer_exact(case, relu, dtype_name):
    """Small integers: the sum of <= 4 terms and every window sum of <= 64 gated gradients equal the oracle with ==; the all-shifts
    kernel with every wanted subset (NULL outputs in between) and the per-shift kernel on the same inputs."""
    c, dtype = case, DTYPES[dtype_name]
    terms, gy = no.fuse_inputs(c, dtype_name)
    dts, dgy = [_device(t, dtype) for t in terms], _device(gy, dtype)
    y = fuse_fwd(dts, c, relu, dtype)
    o = no.fuse_sum(terms, c.shifts, relu)
    assert _same(y, o.y)
    gate = o.y > 0 if relu else np.ones_like(o.y, dtype=bool)
    ref = no.fuse_sum_backward(gy, gate, sorted(set(c.shifts)))
    for wanted in c.wanted:
        got = fuse_bwd_all(dgy, y, c, relu, wanted, dtype)
        for s in wanted:
            assert _same(got[s], ref[s]), 'all-shifts kernel, wanted %s, shift %d' % (wanted, s)
    for s in sorted(set(c.shifts)):
        assert _same(fuse_bwd_one(dgy, y, c, relu, s, dtype), ref[s]), 'per-shift kernel, shift %d' % s


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_fuse_sum_module_paths_integer_exact(dtype_name):
    """nn.sum_relu through autograd with nn.SUM_BWD_ALL on and off (the per-shift launches) on a four-term case."""
    from danet_densepose2smpl_amd import conv as dconv, nn as dnn
    c = no.FUSE_BY_NAME['c12_8x24_b3_4t']
    terms, gy = no.fuse_inputs(c, dtype_name)
    o = no.fuse_sum(terms, c.shifts, True)
    ref = no.fuse_sum_backward(gy, o.y > 0, c.shifts)
    prev = dnn.SUM_BWD_ALL
    try:
        for mode in (True, False):
            dnn.SUM_BWD_ALL = mode
            with dconv.precision(dtype_name):
                ts = [_device(t, DTYPES[dtype_name]).permute(0, 3, 1, 2).requires_grad_(True) for t in terms]
                y = dnn.sum_relu(ts, list(c.shifts), relu=True)
                y.backward(_device(gy, DTYPES[dtype_name]).permute(0, 3, 1, 2))
            assert _same(y.detach().permute(0, 2, 3, 1), o.y)
            for t, s in zip(ts, c.shifts):
                assert _same(t.grad.permute(0, 2, 3, 1), ref[s])
    finally:
        dnn.SUM_BWD_ALL = prev


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_fuse_sum_multi_four_jobs_integer_exact(dtype_name):
    """One sum_relu_multi_kernel launch and one sum_relu_bwd_all_multi_kernel launch over four jobs of different sizes."""
    from danet_densepose2smpl_amd import _lib
    dtype = DTYPES[dtype_name]
    cases = [no.FUSE_BY_NAME[n] for n in no.FUSE_MULTI]
    fj, bj = (_lib.SumFwdJob * 4)(), (_lib.SumBwdJob * 4)()
    keep, ys, ds, refs = [], [], [], []
    for q, c in enumerate(cases):
        terms, gy = no.fuse_inputs(c, dtype_name)
        dts, dgy = [_device(t, dtype) for t in terms], _device(gy, dtype)
        y = Guarded(_shape(c, 0), dtype)
        for n, (t, s) in enumerate(zip(dts, c.shifts)):
            fj[q].terms[n], fj[q].shifts[n] = _p(t), s
        fj[q].nterms, fj[q].B, fj[q].H, fj[q].W, fj[q].C, fj[q].relu, fj[q].y = len(dts), c.B, c.H, c.W, c.C, 1, _p(y)
        o = no.fuse_sum(terms, c.shifts, True)
        wanted = c.wanted[min(1, len(c.wanted) - 1)]
        d = {s: Guarded(_shape(c, s), dtype) for s in wanted}
        bj[q].gy, bj[q].y, bj[q].B, bj[q].H, bj[q].W, bj[q].C, bj[q].relu = _p(dgy), _p(y), c.B, c.H, c.W, c.C, 1
        for s in range(4):
            bj[q].d[s] = _p(d[s]) if s in d else None
        keep += [dts, dgy]; ys.append(y); ds.append(d)
        refs.append((o, no.fuse_sum_backward(gy, o.y > 0, wanted)))
    _call('danet_sum_relu_forward_multi', dtype, ctypes.addressof(fj), 4)
    for y, (o, _) in zip(ys, refs):
        assert _same(y.written(), o.y)
    _call('danet_sum_relu_backward_all_multi', dtype, ctypes.addressof(bj), 4)
    for d, (_, ref) in zip(ds, refs):
        for s, g in d.items():
            assert _same(g.written(), ref[s])


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_fuse_sum_bounded(dtype_name):
    """Real-valued terms: the fp32 sum and the window sums within their rounding bounds (bf16: + 2^-8 |ref|)."""
    c, dtype = no.FUSE_BY_NAME['c12_8x24_b3_4t'], DTYPES[dtype_name]
    terms, gy = no.fuse_inputs(c, dtype_name, integer=False)
    dts, dgy = [_device(t, dtype) for t in terms], _device(gy, dtype)
    y = fuse_fwd(dts, c, True, dtype)
    o = no.fuse_sum(terms, c.shifts, True)
    meas = {'case': 'fuse-%s-%s' % (c.name, dtype_name)}
    meas['y'] = no.ratio(np.abs(_h64(y) - o.y), no.fuse_forward_bound(terms, c.shifts, o, dtype_name))
    gate = _h64(y) > 0
    ref = no.fuse_sum_backward(gy, gate, c.shifts)
    bound = no.fuse_backward_bound(gy, gate, ref, dtype_name)
    got = fuse_bwd_all(dgy, y, c, True, c.shifts, dtype)
    for s in c.shifts:
        meas['d%d' % s] = no.ratio(np.abs(_h64(got[s]) - ref[s]), bound[s])
        meas['d%d_per_shift' % s] = no.ratio(np.abs(_h64(fuse_bwd_one(dgy, y, c, True, s, dtype)) - ref[s]), bound[s])
    _finish(meas)
