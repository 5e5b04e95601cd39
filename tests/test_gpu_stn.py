"""csrc/stn.hip -- the joint-centric part gather and its gather-form backward -- against the float64 restatement of
tests/stn_oracle.py (itself checked against torch in tests/test_stn_host.py), at the shapes where its index arithmetic
branches (stn_oracle.SHAPES) and over thetas that differ for every (b, p) and cycle through stn_oracle.KINDS.  The C entry
points are called directly, so that the test owns the output buffers: each sits between two guard bands of 4096 sentinel
elements and starts out as NaN; after a launch no NaN may be left (an unreached dx pixel is an exact zero) and the guards
must be untouched.  Every launch is repeated into a second buffer and must reproduce bit for bit (no atomics anywhere).

Bounds (derived from the kernels' arithmetic, not tuned; err / bound is recorded through conftest.record('stn_oracle')).
  * The kernel forms a sample coordinate in fp32 in at most 8 rounded operations (the division and the addition of
    norm_coord, two products and two additions of theta . (xn, yn, 1), the addition and the scaling of unnorm_coord) on
    magnitudes up to M = 8 * max(H, W) pixels: |centre| + |scale| <= 8 keeps |g| <= 8, and unnorm_coord scales by at most
    max(H, W) / 2.  Each rounding is at most 2^-24 relative, so the coordinate is within delta = 8 * 2^-24 * M pixels of the
    oracle's.
  * Bilinear interpolation is continuous in the coordinate with a slope per axis of at most 2 * max|x| (the difference of two
    neighbouring pixels), so a coordinate off by delta on both axes -- a different floor() decision included -- moves a
    sample by at most 4 * delta * max|x|.  The weights (1 - f, products) and the four-term sum add a few 2^-24 * max|x|:
        forward, fp32    |y - ref| <= 4 * delta * max|x| + 2^-20 * max|x|
  * In the backward each candidate's weight tent(ix - xx) * tent(iy - yy) has slope <= 1 per axis and factors <= 1, so it
    moves by at most 2 * delta; T = candidates(|gy|, delta) sums |gy| over every sample that can have a non-zero weight on
    either side, R = backward(|gy|) scales the rounding of the products and of the running sum:
        backward, fp32   |dx - ref| <= 2 * delta * T + 2^-20 * R
  * bf16: the same plus 2^-8 * |ref|: one rounding of the fp32 accumulator to bf16's 8 significant bits.  f2bf_pk rounds to
    nearest even (conv_common.h), so the error is at most half a unit in the last place, 2^-8 of the binade's lower end and
    so of the value.  (Truncation would need 2^-7; this bound does not admit it.  The accumulator itself is off ref by the
    fp32 term, and 2^-8 of THAT is left to the fp32 term's own margin.)
A part whose samples all miss the map (EMPTY_KINDS) must give exact zeros in y, and exact zeros in dx from its gy alone.

Adjoint identity (fp32): <stn_fwd(x), gy> and <x, stn_bwd(gy)>, both summed in float64 from the kernels' outputs, agree to
2^-18 of sum |y * gy| -- the backward is the forward's transpose, without help from any reference.

The DANET_STN_V1 kernels (read once per process) run the same case function in a fresh child process: this file as a script."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record
import stn_oracle as so

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -7.0
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}


def _entry(name, dtype):
    from danet_densepose2smpl_amd import _lib
    return getattr(_lib.lib(), name + ('_f32' if dtype == torch.float32 else ''))


class Guarded(object):
    """A NaN-filled output of n elements between two sentinel bands."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
        self.out = self.buf[GUARD:GUARD + self.n].view(*shape)
        self.out.fill_(float('nan'))

    def untouched(self):
        return bool(torch.isnan(self.out).all()) and self.guards_intact()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def written(self):
        assert self.guards_intact(), 'a guard band was written'
        assert not bool(torch.isnan(self.out).any()), 'an output element was never written'
        return self.out


def _launch(which, src, theta, dims, align, out_shape):
    from danet_densepose2smpl_amd._lib import ptr, check, stream
    B, P, C, H, W, OH, OW = dims
    assert src.is_contiguous() and theta.is_contiguous() and theta.dtype == torch.float32
    g = Guarded(out_shape, src.dtype)
    check(_entry('danet_stn_gather_' + which, src.dtype)(ptr(src), ptr(theta), B, H, W, C, P, OH, OW, int(align), ptr(g.out), stream()), which)
    torch.cuda.synchronize()
    return g


def stn_fwd(x, theta, dims, align):
    """Direct forward launch, twice: guards, no NaN left, bitwise reproducible.  x [B,H,W,C] -> y [B,OH,OW,P*C]."""
    B, P, C, H, W, OH, OW = dims
    y = _launch('forward', x, theta, dims, align, (B, OH, OW, P * C)).written()
    assert torch.equal(y, _launch('forward', x, theta, dims, align, (B, OH, OW, P * C)).written()), 'forward is not deterministic'
    return y


def stn_bwd(gy, theta, dims, align):
    B, P, C, H, W, OH, OW = dims
    dx = _launch('backward', gy, theta, dims, align, (B, H, W, C)).written()
    assert torch.equal(dx, _launch('backward', gy, theta, dims, align, (B, H, W, C)).written()), 'backward is not deterministic'
    return dx


def _device(a, dtype):
    """fp32 values -> the device tensor of `dtype` and the float64 values it holds (bf16: rounded first)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).cuda()
    return t, t.float().cpu().numpy().astype(np.float64)


def _h64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _delta(H, W):
    return 8.0 * 2.0 ** -24 * 8.0 * max(H, W)


def check_forward(x, xh, theta, dims, align, empty=None):
    """-> max err / bound of the forward at these thetas."""
    B, P, C, H, W, OH, OW = dims
    y = _h64(stn_fwd(x, torch.from_numpy(theta).cuda(), dims, align))
    ref = so.forward(xh, theta, OH, OW, align)
    xmax = np.abs(xh).max()
    bound = 4.0 * _delta(H, W) * xmax + 2.0 ** -20 * xmax
    if x.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    ratio = float((np.abs(y - ref) / bound).max())
    if empty is not None and empty.any():
        ye = y.reshape(B, OH, OW, P, C).transpose(0, 3, 1, 2, 4)[empty]
        assert not ye.any(), 'a part that misses the map must give exact zeros'
    return ratio, y


def check_backward(gy, gh, theta, dims, align, empty):
    B, P, C, H, W, OH, OW = dims
    th = torch.from_numpy(theta).cuda()
    dx = _h64(stn_bwd(gy, th, dims, align))
    ref = so.backward(gh, theta, H, W, align)
    delta = _delta(H, W)
    T = so.candidates(np.abs(gh), theta, H, W, align, delta)
    R = so.backward(np.abs(gh), theta, H, W, align)
    bound = 2.0 * delta * T + 2.0 ** -20 * R
    if gy.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    err = np.abs(dx - ref)
    assert not err[bound == 0].any(), 'a pixel no sample reaches must be an exact zero'
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    if empty.any():
        mask = torch.from_numpy(np.repeat(empty, C, axis=1)).cuda()                      # [B, P*C]
        dxe = stn_bwd(gy * mask[:, None, None, :].to(gy.dtype), th, dims, align)
        assert not bool(dxe.any()), 'the gradient of a part that misses the map must be exact zeros'
    return ratio, dx


def run_case(name, align, dtype_name, report=None):
    """One shape at one align mode and element type over enough theta phases for every kind to occur; asserts the bounds and
    returns the measured err / bound maxima."""
    dims = so.SHAPES[name]
    B, P, C, H, W, OH, OW = dims
    dtype = DTYPES[dtype_name]
    rs = np.random.RandomState(sum(map(ord, name)))
    x, xh = _device(rs.standard_normal((B, H, W, C)), dtype)
    gy, gh = _device(rs.standard_normal((B, OH, OW, P * C)), dtype)
    meas = {'case': '%s-align%d-%s' % (name, int(align), dtype_name), 'fwd': 0.0, 'bwd': 0.0}
    if dtype == torch.float32:
        meas['adjoint'] = 0.0
    fails = []
    for phase in range(0, len(so.KINDS), min(len(so.KINDS), B * P)):
        theta, kinds = so.thetas(B, P, 100 + phase, phase)
        empty = np.isin(kinds, so.EMPTY_KINDS)
        rf, y = check_forward(x, xh, theta, dims, align, empty)
        rb, dx = check_backward(gy, gh, theta, dims, align, empty)
        meas['fwd'], meas['bwd'] = max(meas['fwd'], rf), max(meas['bwd'], rb)
        if dtype == torch.float32:
            lhs, rhs, scale = np.sum(y * gh), np.sum(xh * dx), np.sum(np.abs(y * gh))
            ra = float(abs(lhs - rhs) / (2.0 ** -18 * scale))
            meas['adjoint'] = max(meas['adjoint'], ra)
    if report is not None:
        report(meas)
    print('stn_oracle %s' % meas)
    for k in ('fwd', 'bwd', 'adjoint'):
        if meas.get(k, 0.0) > 1.0:
            fails.append('%s err / bound = %.3g' % (k, meas[k]))
    assert not fails, '%s: %s' % (meas['case'], '; '.join(fails))
    return meas


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('align', [0, 1])
@pytest.mark.parametrize('name', list(so.SHAPES))
def test_stn_vs_oracle(name, align, dtype_name):
    run_case(name, align, dtype_name, report=lambda m: record('stn_oracle', m))


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('align', [0, 1])
def test_stn_forward_sheared(align, dtype_name):
    """The forward honours th[0][1] and th[1][0] (the backward does not: forward only)."""
    dims = so.SHAPES['out_hw']
    B, P, C, H, W, OH, OW = dims
    rs = np.random.RandomState(77)
    x, xh = _device(rs.standard_normal((B, H, W, C)), DTYPES[dtype_name])
    theta = so.sheared_thetas(B, P, 78)
    assert (theta[:, :, 0, 1] != 0).all() and (theta[:, :, 1, 0] != 0).all()
    ratio, _ = check_forward(x, xh, theta, dims, align)
    record('stn_oracle', {'case': 'sheared-align%d-%s' % (align, dtype_name), 'fwd': ratio})
    assert ratio <= 1.0, 'forward err / bound = %.3g' % ratio


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('align', [0, 1])
def test_stn_wrapper_equals_direct_call(align, dtype_name):
    """nn.stn_gather(..., out_hw=(8, 24)) and autograd on an NCHW-contiguous x and a non-contiguous gy == the direct launches
    on NHWC buffers, bit for bit: the permutes and nhwc_as of the wrapper."""
    from danet_densepose2smpl_amd import conv, nn as dnn
    dims = so.SHAPES['out_hw']
    B, P, C, H, W, OH, OW = dims
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g).to(dtype).cuda()                          # NCHW-contiguous
    gy = torch.randn(B, P * C, OH, 2 * OW, generator=g).to(dtype).cuda()[:, :, :, ::2]  # NCHW, every other column
    assert x.is_contiguous() and not gy.is_contiguous() and not gy.permute(0, 2, 3, 1).is_contiguous()
    theta = torch.from_numpy(so.thetas(B, P, 9)[0]).cuda()
    y_d = stn_fwd(x.permute(0, 2, 3, 1).contiguous(), theta, dims, align)
    dx_d = stn_bwd(gy.permute(0, 2, 3, 1).contiguous(), theta, dims, align)
    xt = x.clone().requires_grad_(True)
    with conv.precision('fp32' if dtype == torch.float32 else 'bf16'):
        y = dnn.stn_gather(xt, theta, out_hw=(OH, OW), align_corners=bool(align))
        dx, = torch.autograd.grad(y, xt, gy)
    assert y.dtype == dtype and tuple(y.shape) == (B, P * C, OH, OW) and tuple(dx.shape) == (B, C, H, W)
    assert torch.equal(y.permute(0, 2, 3, 1), y_d)
    assert torch.equal(dx.permute(0, 2, 3, 1), dx_d)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_stn_size_rejections(dtype_name):
    """The host-side argument checks return an error before any launch and leave the output alone.  (Every buffer has the full
    size the arguments describe.)"""
    from danet_densepose2smpl_amd._lib import ptr, check, stream
    dtype = DTYPES[dtype_name]
    theta = torch.from_numpy(so.thetas(1, 24, 3)[0]).cuda()

    def rejected(which, dims, src_shape, out_shape):
        B, P, C, H, W, OH, OW = dims
        src = torch.zeros(src_shape, dtype=dtype, device='cuda')
        out = Guarded(out_shape, dtype)
        with pytest.raises(RuntimeError, match='stn_gather_' + which):
            check(_entry('danet_stn_gather_' + which, dtype)(ptr(src), ptr(theta[:, :P].contiguous()), B, H, W, C, P, OH, OW, 1, ptr(out.out),
                                                             stream()), which)
        torch.cuda.synchronize()
        assert out.untouched()

    # C = 12: not a multiple of the 8 channels a lane moves
    rejected('forward', (1, 2, 12, 4, 4, 4, 4), (1, 4, 4, 12), (1, 4, 4, 24))
    rejected('backward', (1, 2, 12, 4, 4, 4, 4), (1, 4, 4, 24), (1, 4, 4, 12))
    # a forward row of 2^20 items
    rejected('forward', (1, 1, 8, 1, 1, 1, 1 << 20), (1, 1, 1, 8), (1, 1, 1 << 20, 8))
    # backward coordinate tables of 24 * (256 + 256 + 4 + 256) * 4 bytes = 74 112 > 60 KB
    rejected('backward', (1, 24, 8, 1, 256, 256, 256), (1, 256, 256, 24 * 8), (1, 1, 256, 8))
    # OW >= 32768 in the backward (the column windows are packed into 16 bits each)
    rejected('backward', (1, 1, 8, 1, 1, 1, 32768), (1, 1, 32768, 8), (1, 1, 1, 8))


V1_SHAPES = ('pc1', 'out_hw', 'prod')


def test_stn_v1_kernels_in_child_process():
    """The round-1 kernels (DANET_STN_V1=1, which tools/stn_bench.py still times against) meet the same bounds."""
    env = dict(os.environ, DANET_STN_V1='1')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit('the DANET_STN_V1 child process hung: nothing more is started on this device', returncode=1)
    if r.returncode < 0:
        pytest.exit('the DANET_STN_V1 child process was killed by signal %d: nothing more is started on this device\n%s' %
                    (-r.returncode, r.stderr[-2000:]), returncode=1)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('stn_oracle') == 2 * len(V1_SHAPES), r.stdout[-3000:]


def _child():
    assert os.environ.get('DANET_STN_V1') == '1'
    for name in V1_SHAPES:
        for dtype_name in ('bf16', 'fp32'):
            run_case(name, 1, dtype_name, report=lambda m: record('stn_oracle', dict(m, case='v1-' + m['case'])))


if __name__ == '__main__':
    try:
        _child()
    except AssertionError as e:
        print('FAILED: %s' % e)
        sys.exit(1)
