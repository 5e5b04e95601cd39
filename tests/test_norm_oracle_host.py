"""CPU checks of tests/norm_oracle.py: the float64 restatements against torch in float64, the byte-mask layout against a
hand-written example, and the case tables -- every "exists for" claim recomputed from make_map's formulas as norm_oracle restates
them, the exactness conditions of the integer cases, and the share of ReLU gates the mask comparison has to leave out."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_oracle as no


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize('name,relu,use_res', [('c4_m5', True, False), ('c12_m86', True, True), ('c40_m51', False, True)])
def test_batch_norm_oracle_vs_torch_float64(name, relu, use_res):
    c = no.BN_BY_NAME[name]
    i = no.bn_inputs(c.C, c.M, name, 'bf16', use_res)
    x = _t(i.x.T[None, :, :, None]).requires_grad_(True)                       # [1, C, M, 1]
    res = _t(i.res.T[None, :, :, None]).requires_grad_(True) if use_res else None
    g, b = _t(i.gamma).requires_grad_(True), _t(i.beta).requires_grad_(True)
    rm, rv = _t(i.rm).clone(), _t(i.rv).clone()
    v = F.batch_norm(x, rm, rv, g, b, True, no.MOMENTUM, no.EPS)
    if use_res:
        v = v + res
    y = F.relu(v) if relu else v
    y.backward(_t(i.dy.T[None, :, :, None]))
    o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, relu)
    back = lambda t: t.detach()[0, :, :, 0].numpy().T
    assert np.allclose(o.y, back(y), rtol=1e-12, atol=1e-12) and np.allclose(o.v, back(v), rtol=1e-12, atol=1e-12)
    nrm, nrv = no.running_update(i.rm, i.rv, o.mean, o.var, c.M, no.MOMENTUM)
    assert np.allclose(nrm, rm.numpy(), rtol=1e-12, atol=1e-14) and np.allclose(nrv, rv.numpy(), rtol=1e-12, atol=1e-14)
    bw = no.bn_backward(i.dy, i.x, o.y > 0 if relu else np.ones_like(o.y, bool), i.gamma, o.mean, o.invstd)
    assert np.allclose(bw.dx, back(x.grad), rtol=1e-9, atol=1e-10)
    assert np.allclose(bw.dbeta, b.grad.numpy(), rtol=1e-10, atol=1e-10) and np.allclose(bw.dgamma, g.grad.numpy(), rtol=1e-10, atol=1e-10)
    if use_res:
        assert np.array_equal(bw.dres, back(res.grad))
    # eval mode with the updated running statistics
    e = no.bn_eval(i.x, i.res, i.gamma, i.beta, nrm, nrv, no.EPS, relu)
    ve = F.batch_norm(x.detach(), rm, rv, g.detach(), b.detach(), False, no.MOMENTUM, no.EPS)
    ve = ve + res.detach() if use_res else ve
    assert np.allclose(e.y, back(F.relu(ve) if relu else ve), rtol=1e-12, atol=1e-12)
    assert np.array_equal(no.channel_sum(i.x), i.x.sum(0))


def test_batch_norm_oracle_without_affine_and_single_row():
    i = no.bn_inputs(12, 7, 'noaffine', 'fp32', False)
    o = no.bn_forward(i.x, None, None, None, no.EPS, False)
    v = F.batch_norm(_t(i.x.T[None, :, :, None]), None, None, None, None, True, 0.1, no.EPS)
    assert np.allclose(o.y, v[0, :, :, 0].numpy().T, rtol=1e-12, atol=1e-12)
    rm, rv = no.running_update(np.zeros(3), np.ones(3), np.ones(3), np.full(3, 2.0), 1, 0.5)       # M == 1: the factor is 1
    assert np.array_equal(rm, np.full(3, 0.5)) and np.array_equal(rv, np.full(3, 1.5))
    rm, rv = no.running_update(np.zeros(3), np.ones(3), np.ones(3), np.full(3, 2.0), 5, 0.5)
    assert np.array_equal(rv, np.full(3, 0.5 + 0.5 * 2.0 * 5 / 4))


@pytest.mark.parametrize('name', ['c12_16x8_b3_2t', 'c4_16x8_rep', 'c12_8x24_b3_4t'])
def test_fuse_sum_oracle_vs_torch_float64(name):
    c = no.FUSE_BY_NAME[name]
    terms, gy = no.fuse_inputs(c, 'bf16', integer=False)
    ts = [_t(t).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in terms]
    v = sum(t if s == 0 else F.interpolate(t, scale_factor=2 ** s, mode='nearest') for t, s in zip(ts, c.shifts))
    y = F.relu(v)
    y.backward(_t(gy).permute(0, 3, 1, 2))
    o = no.fuse_sum(terms, c.shifts, True)
    assert np.allclose(o.y, y.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-13, atol=1e-13)
    d = no.fuse_sum_backward(gy, o.y > 0, sorted(set(c.shifts)))
    for t, s in zip(ts, c.shifts):
        assert np.allclose(d[s], t.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    lin = no.fuse_sum(terms, c.shifts, False)
    assert np.array_equal(lin.y, lin.v) and np.allclose(lin.v, v.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-13, atol=1e-13)


def test_mask_bytes_hand_written():
    v = np.array([[1.0, -1.0, 0.0, 2.0, -3.0, -4.0, 5.0, 1e-30],        # byte 0: bits 0, 3 = 9; byte 1: bits 2, 3 = 12
                  [0.0, 0.0, -0.0, 0.0, 7.0, 7.0, 7.0, 7.0]])          # byte 2: 0; byte 3: 15
    assert no.mask_bytes(v).tolist() == [9, 12, 0, 15]
    assert no.mask_bytes(v).dtype == np.uint8


def test_round_bf16_is_round_to_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, -2.5, 0.0, 255.0, 257.0])
    want = torch.from_numpy(a.astype(np.float32)).bfloat16().double().numpy()
    assert np.array_equal(no.round_bf16(a), want)
    assert no.round_bf16(np.array([1.0 + 2.0 ** -8]))[0] == 1.0 and no.round_bf16(np.array([1.0 + 3 * 2.0 ** -8]))[0] == 1.0 + 2.0 ** -6
    rs = np.random.RandomState(0)
    b = rs.standard_normal(4096) * 10.0 ** rs.randint(-6, 6, 4096)
    assert np.array_equal(no.round_bf16(b), torch.from_numpy(b.astype(np.float32)).bfloat16().double().numpy())


@pytest.mark.parametrize('case', no.BN_CASES, ids=lambda c: c.name)
def test_bn_case_takes_the_branch_it_exists_for(case):
    assert case.C % 4 == 0 and len(case.expect) == len(no.slabs(case.C))
    for dtype_name in ('bf16', 'fp32'):
        plans = no.plan(case.M, case.C, dtype_name, case.knob)
        got = [(p.Cs, p.span, p.rpb, p.blocks, p.k1) for p in plans]
        assert got == list(no.EXPECT_FP32.get(case.name, case.expect) if dtype_name == 'fp32' else case.expect), (dtype_name, got)
        for p in plans:                                  # make_map's own invariants
            assert p.span <= 256 and p.span % p.CV == 0 and p.rstep * p.k1 >= case.M and p.blocks <= 1024
    assert no.wide_slabs(case.C) == no.WIDE.get(case.name, 1)
    p0 = no.plan(case.M, case.C, 'bf16', case.knob)[0]
    if case.name.startswith('c4_'):
        assert p0.CV == 1 and case.M < p0.rpb and (case.M < no.UNR or case.name == 'c4_m5')
    if case.name.startswith('c12_'):
        assert p0.idle == 1 and case.M in (p0.rpb, p0.rpb + 1, no.UNR * p0.rpb + 1)
    if case.name == 'c40_m51':
        assert p0.idle == 6
    if case.name == 'c1024_m5':
        assert p0.CV == 256 and p0.rpb == 1
    if case.name == 'c1028_m6':
        assert [Cs for _, Cs in no.slabs(case.C)] == [1024, 4] and no.onepass_plan(case.M, case.C) is None
    if case.name == 'c1536_m4':
        assert [Cs for _, Cs in no.slabs(case.C)] == [1024, 512] and no.onepass_plan(case.M, case.C) is None
    if case.name in no.WIDE:
        assert no.onepass_plan(case.M, case.C) == (no.OP_ROWS, [1] * no.WIDE[case.name])
    if case.name == 'c2052_m4':
        assert [Cs for _, Cs in no.slabs(case.C)] == [1024, 1024, 4]
    if case.name == 'c48_m700_k512':
        assert p0.blocks == 34 > no.bn_ncopy(48) == 16
        assert no.plan(case.M, case.C, 'bf16', None)[0].blocks < p0.blocks          # it is the knob that does it
    if case.name == 'c48_cap_k64':
        assert p0.blocks == 1024 and no.ceil_div(case.M, p0.rpb) == 1025 and p0.rstep == 21 * 1024 and p0.k1 == 2
        assert case.M - p0.rstep == 5                                                # five rows' lanes walk a second row


@pytest.mark.parametrize('case', no.CHSUM_CASES, ids=lambda c: c[0])
def test_channel_sum_case_geometry(case):
    name, C, M, knob, ncopy, blocks, k1 = case
    for dtype_name in ('bf16', 'fp32'):
        p = no.plan(M, C, dtype_name, knob, cap=1024 if ncopy >= 4 else 256)[0]
        assert (p.blocks, p.k1) == (blocks, k1)
    if 'cap' in name:
        assert no.plan(M, C, 'bf16', knob)[0].blocks == 1024 and blocks == (1024 if ncopy >= 4 else 256)
        assert (k1 == no.UNR + 1) == (ncopy == 1)                                  # ncopy 1: one row more than a trip
    i = no.bn_inputs(C, M, name, 'bf16', False, 'int')
    assert no.exact_sum_ok(i.x)


@pytest.mark.parametrize('case', no.ONEPASS_CASES, ids=lambda c: 'm%d_b%d' % (c[0], c[1]))
def test_onepass_case_row_budget(case):
    M, budget, rows, blocks, k1, why = case
    p = no.onepass_plan(M, 48, budget)
    if rows is None:
        assert p is None and no.onepass_plan(M, 48, 0) is not None
        return
    assert p == (rows, [blocks]) and no.onepass_k1(M, 48, budget) == k1
    assert k1 <= rows
    if why == 'registers only':
        assert k1 == no.OP_NV
    if why == 'first LDS row':
        assert k1 == no.OP_NV + 1
    if why in ('all 25 rows', 'budget 1: all 29 rows'):
        assert k1 == rows and no.onepass_plan(M + 1, 48, budget) != p
    if budget == 1 and rows == 29:
        assert no.onepass_plan(M, 48, 0)[0] == no.OP_ROWS and k1 > no.OP_ROWS          # only the 29-row form fits one workgroup


def test_integer_cases_are_exact_in_fp32_and_bf16():
    for name, C, M, knob in no.INT_CASES:
        assert C % 4 == 0 and M & (M - 1) == 0, name                                # a power of two: mean = sum / M is exact
        i = no.bn_inputs(C, M, name, 'bf16', False, 'int')
        assert np.array_equal(i.x, no.round_bf16(i.x)) and no.exact_sum_ok(i.x) and no.exact_sum_ok(i.x - i.x[0])
        assert np.array_equal(np.float32(i.x.mean(0)).astype(np.float64) * M, i.x.sum(0))
    for c in no.BN_CASES:
        for use_res in (False, True):
            i = no.bn_inputs(c.C, c.M, c.name, 'bf16', use_res)
            assert no.exact_sum_ok(i.dy) and np.array_equal(i.dy, no.round_bf16(i.dy)) and np.abs(i.dy).max() <= no.INT_DY
    assert 4 * no.FUSE_TERM <= 256 and 64 * no.FUSE_GY <= 256                      # integers up to 256 are bf16 values
    for c in no.FUSE_CASES + [no.FUSE_BIG]:
        terms, gy = no.fuse_inputs(c, 'bf16')
        assert len(terms) <= 4 and max(c.shifts) <= 3 and c.C % 4 == 0
        assert all(np.array_equal(t, np.rint(t)) and np.abs(t).max() <= no.FUSE_TERM for t in terms)
        assert np.array_equal(gy, np.rint(gy)) and np.abs(gy).max() <= no.FUSE_GY
        assert all(c.H % (1 << s) == 0 and c.W % (1 << s) == 0 for s in c.shifts)
    c = no.FUSE_BIG
    assert no.ceil_div(c.B * c.H * c.W * (c.C // 4), 256) > 4096 and c.B * c.H * c.W * c.C * 2 < 9e6


def _gate_share(c, dtype_name, use_res, kind='normal'):
    i = no.bn_inputs(c.C, c.M, c.name, dtype_name, use_res, kind)
    o = no.bn_forward(i.x, i.res, i.gamma, i.beta, no.EPS, True)
    k = no.k_of(no.plan(c.M, c.C, dtype_name, c.knob))
    dm, dvar = no.stats_bound(i.x, dtype_name, k)
    bound = no.forward_bound(i.x, i.res, i.gamma, i.beta, o, dm, no.invstd_bound(o.var, no.EPS, dvar, dtype_name), dtype_name)
    return float((np.abs(o.v) <= bound).mean())


@pytest.mark.parametrize('case', no.BN_CASES, ids=lambda c: c.name)
def test_excluded_gate_share_is_at_most_one_percent(case):
    for use_res in (False, True):
        assert _gate_share(case, 'bf16', use_res) <= 0.01


def test_offset_case():
    name, C, M = no.OFFSET_CASE
    c = no.BnCase(name, C, M, None, '', None)
    assert M & (M - 1) == 0 and _gate_share(c, 'bf16', False, 'offset') <= 0.01 and _gate_share(c, 'bf16', True, 'offset') <= 0.01
    i = no.bn_inputs(C, M, name, 'bf16', False, 'offset')
    o = no.bn_forward(i.x, None, i.gamma, i.beta, no.EPS, True)
    assert o.var[1] == 0.0 and o.mean[1] == 2.0 and (np.delete(np.abs(o.mean) / np.sqrt(o.var + 1e-30), 1) > 8).all()


def test_bounds_catch_the_faults_the_old_tolerance_let_pass():
    """With the oracle alone: a row counted twice, a dropped tail row, a missing `unbias` and a truncation to bf16 all move the
    result by more than the derived bound (so a kernel with that fault fails the GPU test), at a grid-sizing case."""
    c = no.BN_BY_NAME['c48_m700_k512']
    i = no.bn_inputs(c.C, c.M, c.name, 'bf16', False)
    o = no.bn_forward(i.x, None, i.gamma, i.beta, no.EPS, False)
    k = no.k_of(no.plan(c.M, c.C, 'bf16', c.knob))
    dm, dvar = no.stats_bound(i.x, 'bf16', k)
    twice = np.concatenate([i.x, i.x[-1:]]).sum(0) / c.M
    dropped = i.x[:-1].sum(0) / c.M
    assert (np.abs(twice - o.mean) > dm).all() and (np.abs(dropped - o.mean) > dm).all()
    _, brv = no.running_bound(i.rm, i.rv, o.mean, o.var, c.M, no.MOMENTUM, dm, dvar)
    _, rv = no.running_update(i.rm, i.rv, o.mean, o.var, c.M, no.MOMENTUM)
    assert (np.abs((1 - no.MOMENTUM) * i.rv + no.MOMENTUM * o.var - rv) > brv).all()
    bound = no.forward_bound(i.x, None, i.gamma, i.beta, o, dm, no.invstd_bound(o.var, no.EPS, dvar, 'bf16'), 'bf16')
    b = np.ascontiguousarray(o.y, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)
    assert (np.abs(b.view(np.float32).astype(np.float64) - o.y) > bound).mean() > 0.2
    # one wrong gate bit moves dres by a whole integer gradient value and dbeta by it: the exact tests see both
    assert np.abs(i.dy).min() == 0 and (np.abs(i.dy) >= 1).mean() > 0.9


@pytest.mark.skipif(torch.cuda.is_available(), reason='its evidence is that every launch fails where there is no device, and its fake '
                                                      'pointers must never reach a GPU')
def test_refused_calls_answer_err_arg_with_their_text_and_enqueue_nothing():
    """Refused argument sets of every entry of csrc/norm_act.hip, in both instantiations: DANET_ERR_ARG and the exact text.  Without
    a device every launch attempt answers DANET_ERR_HIP (the premise, asserted first), so DANET_ERR_ARG also says that the call had
    enqueued nothing -- the zeroing kernel and bn_stats_kernel included -- when it refused."""
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    ERR_ARG, ERR_HIP, NBM, NSM = -1, -2, 12, 4
    P = ctypes.c_void_p(64)
    BIG = dict(M=1 << 22, C=512)                                   # 2^32 bytes in bf16: past the 32-bit byte offsets ("< 2 GB")
    GB2 = 'C=512 (M=4194304) unsupported'
    GATE = "bn_backward: ReLU gate: mask_mode 0 needs y, 1 the forward's byte mask, 2 (recompute from x) no residual"
    SHIFTED = 'the fp32 statistics are shifted sums (bn_stats_kernel): no pre-accumulated sums'

    def call(name, order, defaults, kw):
        a = dict(defaults, **kw)
        rc = getattr(L, name)(*[a[k] for k in order.split()])
        return rc, L.danet_last_error().decode()

    def arr(ctype, values):
        return (ctype * len(values))(*values)

    def fwd_jobs(*kws):
        jobs = (_lib.BnFwdJob * (NBM + 1))()
        for j, kw in zip(jobs, kws):
            for k in ('x', 'y', 'saved', 'sums'):
                setattr(j, k, 64)
            j.M, j.C, j.sums_state = 8, 8, 1
            for k, v in kw.items():
                setattr(j, k, v)
        return ctypes.addressof(jobs), jobs

    def bwd_jobs(*kws):
        jobs = (_lib.BnBwdJob * (NBM + 1))()
        for j, kw in zip(jobs, kws):
            for k in ('dy', 'x', 'dx', 'saved', 'red'):
                setattr(j, k, 64)
            j.M, j.C, j.red_state = 8, 8, 1
            for k, v in kw.items():
                setattr(j, k, v)
        return ctypes.addressof(jobs), jobs

    def sum_fwd_jobs(*kws):
        jobs = (_lib.SumFwdJob * (NSM + 1))()
        for j, kw in zip(jobs, kws):
            j.terms[0], j.terms[1], j.shifts[1], j.nterms, j.B, j.H, j.W, j.C, j.y = 64, 64, 1, 2, 1, 8, 8, 8, 64
            for k, v in kw.items():
                setattr(j, k, v)
        return ctypes.addressof(jobs), jobs

    def sum_bwd_jobs(*kws):
        jobs = (_lib.SumBwdJob * (NSM + 1))()
        for j, kw in zip(jobs, kws):
            j.gy, j.B, j.H, j.W, j.C = 64, 1, 8, 8, 8
            j.d[1] = 64
            for k, v in kw.items():
                setattr(j, k, v)
        return ctypes.addressof(jobs), jobs

    FWD = ('x res y M C gamma beta rm rv saved sums ws_is_zero momentum eps training relu mask stream',
           dict(x=P, res=None, y=P, M=8, C=8, gamma=None, beta=None, rm=P, rv=P, saved=P, sums=P, ws_is_zero=1, momentum=0.1, eps=1e-5,
                training=1, relu=0, mask=None, stream=None))
    BWD = ('dy x y M C gamma saved relu dx dres dparam red ws_is_zero mask_mode mask beta stream',
           dict(dy=P, x=P, y=None, M=8, C=8, gamma=None, saved=P, relu=0, dx=P, dres=None, dparam=None, red=P, ws_is_zero=1, mask_mode=0,
                mask=None, beta=None, stream=None))
    CSUM = ('x M C out out_is_zero ncopy stream', dict(x=P, M=8, C=8, out=P, out_is_zero=1, ncopy=1, stream=None))
    SFWD = ('terms shifts nterms B H W C relu y stream',
            dict(terms=arr(ctypes.c_void_p, [64, 64, 64, 64]), shifts=arr(ctypes.c_int, [0, 1, 0, 0]), nterms=2, B=1, H=8, W=8, C=8, relu=1, y=P,
                 stream=None))
    SALL = ('gy y B H W C relu d0 d1 d2 d3 stream', dict(gy=P, y=P, B=1, H=8, W=8, C=8, relu=1, d0=P, d1=None, d2=None, d3=None, stream=None))
    SBWD = ('gy y B H W C shift relu d_term stream', dict(gy=P, y=P, B=1, H=8, W=8, C=8, shift=1, relu=1, d_term=P, stream=None))

    for suffix in ('', '_f32'):
        f32 = suffix == '_f32'
        # the premise: an accepted call reaches its launch, and without a device the launch fails
        rc, msg = call('danet_bn_forward' + suffix, *FWD, dict(training=0))
        assert rc == ERR_HIP and msg.startswith('bn_apply'), (suffix, rc, msg)

        single = [
            ('danet_bn_forward', FWD, [
                (dict(x=None), 'bn_forward: bad arguments'), (dict(M=0), 'bn_forward: bad arguments'),
                (dict(saved=None), 'bn_forward: missing buffers'), (dict(training=0, rm=None), 'bn_forward: missing buffers'),
                (dict(C=6), 'bn_forward: C=6 must be a multiple of 4'),
                (dict(BIG, training=0), 'bn_forward: %s: channels must be a multiple of 4 and the tensor < 2 GB' % GB2),
                (dict(BIG, ws_is_zero=0), 'bn_forward: %s: channels must be a multiple of 4 and the tensor < 2 GB' % GB2)]
             + ([(dict(ws_is_zero=2), 'bn_forward_f32: ' + SHIFTED)] if f32 else [])),
            ('danet_bn_backward', BWD, [
                (dict(dx=None), 'bn_backward: bad arguments'),
                (dict(relu=1, mask_mode=0), GATE), (dict(relu=1, mask_mode=1, y=P), GATE), (dict(relu=1, mask_mode=2, dres=P), GATE),
                (dict(C=6), 'bn_backward: C=6 must be a multiple of 4'),
                (dict(BIG, ws_is_zero=0), 'bn_backward: %s: channels must be a multiple of 4 and the tensor < 2 GB' % GB2)]),
            ('danet_channel_sum', CSUM, [
                (dict(ncopy=0), 'channel_sum: bad arguments (C=8 must be a multiple of 4)'),
                (dict(ncopy=65), 'channel_sum: bad arguments (C=8 must be a multiple of 4)'),
                (dict(C=6), 'channel_sum: bad arguments (C=6 must be a multiple of 4)'),
                (dict(BIG, out_is_zero=0), 'channel_sum: ' + GB2)]),
            ('danet_sum_relu_forward', SFWD, [
                (dict(nterms=0), 'sum_relu_forward: bad arguments'), (dict(nterms=5), 'sum_relu_forward: bad arguments'),
                (dict(C=6), 'sum_relu_forward: bad arguments'),
                (dict(terms=arr(ctypes.c_void_p, [64, None, 64, 64])), 'sum_relu_forward: term 1'),
                (dict(H=6, shifts=arr(ctypes.c_int, [0, 2, 0, 0])), 'sum_relu_forward: term 1'),
                (dict(shifts=arr(ctypes.c_int, [-1, 1, 0, 0])), 'sum_relu_forward: term 0')]),
            ('danet_sum_relu_backward_all', SALL, [
                (dict(d0=None), 'sum_relu_backward_all: bad arguments'), (dict(y=None), 'sum_relu_backward_all: bad arguments'),
                (dict(H=6, d2=P), 'sum_relu_backward_all: bad arguments')]),
            ('danet_sum_relu_backward', SBWD, [
                (dict(shift=-1), 'sum_relu_backward: bad arguments'), (dict(d_term=None), 'sum_relu_backward: bad arguments')]),
        ]
        for name, (order, defaults), cases in single:
            for kw, text in cases:
                assert call(name + suffix, order, defaults, kw) == (ERR_ARG, text), (name + suffix, kw)

        good = {}
        multi = [
            ('danet_bn_forward_multi', fwd_jobs, NBM, lambda p, n: (p, n, 0.1, 1e-5, None), 'bn_forward_multi: 1..12 jobs', [
                # job 0 is accepted and asks for a statistics pass (sums_state 1): refusing job 1 must come before that launch
                ((good, dict(y=None)), 'bn_forward_multi: job 1: bad arguments (C <= 1024, zeroed or pre-accumulated sums required)'),
                ((good, dict(BIG)), 'bn_forward_multi: job 1: C=512 unsupported'),
                ((dict(C=2048),), 'bn_forward_multi: job 0: bad arguments (C <= 1024, zeroed or pre-accumulated sums required)')]
             + ([((dict(sums_state=2),), 'bn_forward_multi_f32: job 0: ' + SHIFTED), ((good, dict(sums_state=2)), 'bn_forward_multi_f32: job 1: ' + SHIFTED)]
                if f32 else [])),
            ('danet_bn_backward_multi', bwd_jobs, NBM, lambda p, n: (p, n, None), 'bn_backward_multi: 1..12 jobs', [
                ((good, dict(dx=None)), 'bn_backward_multi: job 1: bad arguments'),
                ((dict(C=2048),), 'bn_backward_multi: job 0: bad arguments'),
                ((good, dict(red_state=0)), 'bn_backward_multi: job 1: bad arguments'),
                ((good, dict(relu=1, mask_mode=0)), 'bn_backward_multi: job 1: ReLU gate (mask_mode 0) lacks its input'),
                ((good, dict(relu=1, mask_mode=1, y=64)), 'bn_backward_multi: job 1: ReLU gate (mask_mode 1) lacks its input'),
                ((good, dict(relu=1, mask_mode=2, dres=64)), 'bn_backward_multi: job 1: ReLU gate (mask_mode 2) lacks its input'),
                ((good, dict(BIG)), 'bn_backward_multi: job 1: C=512 unsupported')]),
            ('danet_sum_relu_forward_multi', sum_fwd_jobs, NSM, lambda p, n: (p, n, None), 'sum_relu_forward_multi: 1..4 jobs', [
                ((good, dict(y=None)), 'sum_relu_forward_multi: job 1: bad arguments'),
                ((good, dict(nterms=5)), 'sum_relu_forward_multi: job 1: bad arguments'),
                ((good, dict(H=7)), 'sum_relu_forward_multi: job 1 term 1')]),
            ('danet_sum_relu_backward_all_multi', sum_bwd_jobs, NSM, lambda p, n: (p, n, None), 'sum_relu_backward_all_multi: 1..4 jobs', [
                ((good, dict(gy=None)), 'sum_relu_backward_all_multi: job 1: bad arguments'),
                ((good, dict(relu=1)), 'sum_relu_backward_all_multi: job 1: bad arguments'),
                ((good, dict(H=7)), 'sum_relu_backward_all_multi: job 1: bad arguments')]),
        ]
        for name, make, nmax, args, count_text, cases in multi:
            fn = getattr(L, name + suffix)
            p, keep = make(*([good] * (nmax + 1)))
            for n in (0, nmax + 1):
                assert (fn(*args(p, n)), L.danet_last_error().decode()) == (ERR_ARG, count_text), (name + suffix, n)
            assert (fn(*args(None, 1)), L.danet_last_error().decode()) == (ERR_ARG, count_text), name + suffix
            for kws, text in cases:
                p, keep = make(*kws)
                assert (fn(*args(p, len(kws))), L.danet_last_error().decode()) == (ERR_ARG, text), (name + suffix, kws)
