"""Keypoint fit on the GPU (csrc/kp_fit.hip, kp_fit.py, DESIGN.md "fit rule") against the float64 oracle of kp_fit_oracle.py.

The error bound.  The kernel is fp32 and sums in its own order, so it cannot match the float64 oracle closer than single precision
allows on the same inputs.  What single precision costs is measured, not guessed: the oracle runs a second time in float32, and for
a block of outputs

    max |kernel - f64|  <=  4 * max |oracle_f32 - f64|  +  8 * 2^-23 * max |f64|           (maxima over the block)

The second term is the absolute floor: 8 roundings of the block's largest entry (an energy is a sum of some fifty terms, whose roundings
add up to about sqrt(50) = 7 of the largest), for entries that are exactly zero in float64 and for a float32 oracle run that happens to
land on the float64 value.  Of the 52 blocks of these tests one, the energy at P = 1, uses any of it (0.16 roundings).  Blocks: the energies of the batch, the camera gradients of the
batch (one and three numbers per person are too few for a maximum per person to be a stable yardstick), and per person the shape
gradient, the 6D gradient, the history, and camera / betas / rotations of para_fit.  The measured ratios max |kernel - f64| /
max |oracle_f32 - f64| are printed and recorded (conftest.record)."""
import numpy as np
import pytest
import torch

import kp_fit_oracle as ko
from conftest import record

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
SHORT = ((3, 'cam+orient'), (5, 'all'))


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope='module')
def ctx(smpl_model):
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL(smpl_model).cuda()
    m64 = ko.model_tensors(smpl_model)
    return {'smpl': smpl, 'fitter': KeypointFitter(smpl), 'm64': m64, 'm32': ko.as_tensors(m64, torch.float32), 'model': smpl_model}


def bound_block(tag, got, r64, r32, ratios):
    err, err32, scale = np.abs(got - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    bound = 4.0 * err32 + 8.0 * EPS32 * scale
    ratios.append((tag, float(err), float(err32), float(bound)))
    return err <= bound


def _report(name, ratios):
    worst = max(ratios, key=lambda r: r[1] / max(r[3], 1e-300))
    rel = [r[1] / r[2] for r in ratios if r[2] > 0]
    print('%s: %d blocks, err / err_f32 median %.2f max %.2f; tightest block %s err %.3g (f32 oracle %.3g, bound %.3g)'
          % (name, len(ratios), float(np.median(rel)), float(np.max(rel)), worst[0], worst[1], worst[2], worst[3]), flush=True)
    record(name, {'blocks': len(ratios), 'all': [[r[0], r[1], r[2], r[3]] for r in ratios], 'ratio_median': float(np.median(rel)), 'ratio_max': float(np.max(rel)),
                  'tightest': {'block': worst[0], 'err': worst[1], 'err_f32': worst[2], 'bound': worst[3]}})


def _energy_and_gradient(fitter, m64, m32, P, seed, name):
    para, kp = ko.edge_case(m64, P, seed)
    # what the case is meant to hold
    p64 = torch.as_tensor(para.astype(np.float64))
    _, D = ko.project(ko.joints49(m64, p64[:, 3:13], p64[:, 13:].reshape(P, 24, 3, 3)), p64[:, :3], 5000., 224., 2 * 5000. / 224.)
    assert (kp[:, :, 2] == 0).any() and np.isfinite(kp).all() and ((D - 1e-6).abs() > 1e-3).all()
    if P > 2:
        assert (D[2] <= 1e-6).any() and (D[2] > 1e-6).any() and (D[:2] > 1e-6).all() and para[1, 0] == np.float32(0.05)
    r64 = ko.fit(m64, para, kp, stages=())
    r32 = ko.fit(m32, para, kp, stages=(), dtype=torch.float32)
    fit, info = fitter.fit(_cu(para), _cu(kp), return_history=True, return_grad=True, stages=())
    torch.cuda.synchronize()
    E, g = info['history'].cpu().numpy().astype(np.float64), info['grad'].cpu().numpy().astype(np.float64)
    assert E.shape == (P, 1) and g.shape == (P, 157) and (info['status'].cpu().numpy() == 0).all() and (info['best_iter'].cpu().numpy() == 0).all()
    assert torch.equal(fit, _cu(para))                                   # T = 0: the row itself
    ratios, ok = [], True
    ok &= bound_block('E', E, r64['history'], r32['history'], ratios)
    ok &= bound_block('g_cam', g[:, :3], r64['grad'][:, :3], r32['grad'][:, :3], ratios)
    for p in range(P):
        ok &= bound_block('g_betas[%d]' % p, g[p, 3:13], r64['grad'][p, 3:13], r32['grad'][p, 3:13], ratios)
        ok &= bound_block('g_a[%d]' % p, g[p, 13:], r64['grad'][p, 13:], r32['grad'][p, 13:], ratios)
    _report(name, ratios)
    assert ok, ratios


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('P', [1, 3])
def test_energy_and_gradient_at_x0(ctx, P):
    _energy_and_gradient(ctx['fitter'], ctx['m64'], ctx['m32'], P, P, 'kp_fit_energy_gradient_P%d' % P)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_short_trajectory(ctx):
    P, seed = 8, 3
    star = ko.make_para(P, seed)
    init = ko.perturb(star, seed + 1, pose_sigma=0.1, shift=0.03, scale=1.05)
    kp = ko.keypoints_of(ctx['m64'], star)
    kp[:, :, 2] = np.random.default_rng(seed).uniform(0.2, 1.0, (P, 49))
    r64 = ko.fit(ctx['m64'], init, kp, stages=SHORT)
    r32 = ko.fit(ctx['m32'], init, kp, stages=SHORT, dtype=torch.float32)
    agree = r64['best_iter'] == r32['best_iter']
    assert (~agree).sum() <= P // 8                                       # the oracle alone stays within the cap
    fit, info = ctx['fitter'].fit(_cu(init), _cu(kp), return_history=True, stages=SHORT)
    torch.cuda.synchronize()
    h, bi, pf = info['history'].cpu().numpy().astype(np.float64), info['best_iter'].cpu().numpy(), fit.cpu().numpy().astype(np.float64)
    assert h.shape == (P, 9) and (info['status'].cpu().numpy() == 0).all()
    print('history[0]: %s; best_iter %s (f64 %s)' % (np.round(h[0], 5).tolist(), bi.tolist(), r64['best_iter'].tolist()), flush=True)
    assert np.array_equal(bi[agree], r64['best_iter'][agree])
    assert (h.min(1) < 0.5 * h[:, 0]).all()                               # eight steps already halve the energy
    ratios, ok = [], True
    for p in range(P):
        ok &= bound_block('history[%d]' % p, h[p], r64['history'][p], r32['history'][p], ratios)
        for tag, sl in (('cam', slice(0, 3)), ('betas', slice(3, 13)), ('rot', slice(13, 229))):
            ok &= bound_block('para_fit.%s[%d]' % (tag, p), pf[p, sl], r64['para_fit'][p, sl], r32['para_fit'][p, sl], ratios)
    _report('kp_fit_short_trajectory', ratios)
    assert ok, ratios


# ------------------------------------------------------------------------------------------------------------------ 3
def test_bit_properties(ctx):
    fitter, m64 = ctx['fitter'], ctx['m64']
    star = ko.make_para(33, 17)
    init = _cu(ko.perturb(star, 18, pose_sigma=0.1, shift=0.03, scale=1.05))
    kp = _cu(ko.keypoints_of(m64, star))
    fit = lambda p, k, **kw: fitter.fit(p, k, return_history=True, stages=kw.pop('stages', SHORT), **kw)          # noqa: E731
    # all confidences zero: nothing moves
    k0 = kp[:5].clone()
    k0[:, :, 2] = 0
    f0, i0 = fit(init[:5], k0)
    assert torch.equal(f0, init[:5]) and (i0['history'] == i0['history'][:, :1]).all() and (i0['best_iter'] == 0).all()
    # a batch is its rows; two runs are one
    f5, i5 = fit(init[:5], kp[:5])
    again, iagain = fit(init[:5], kp[:5])
    assert torch.equal(f5, again) and torch.equal(i5['history'], iagain['history']) and torch.equal(i5['best_iter'], iagain['best_iter'])
    assert (i5['best_iter'] > 0).all() and not torch.equal(f5, init[:5])
    for p in range(5):
        f1, i1 = fit(init[p:p + 1], kp[p:p + 1])
        assert torch.equal(f1[0], f5[p]) and torch.equal(i1['history'][0], i5['history'][p]) and i1['best_iter'][0] == i5['best_iter'][p]
    f33, i33 = fit(init, kp)
    assert torch.equal(f33[0], f5[0]) and torch.equal(i33['history'][0], i5['history'][0]) and torch.equal(f33[:5], f5)
    # a row of NaN: status 1, unchanged, neighbours untouched
    bad = init[:5].clone()
    bad[2] = float('nan')
    fb, ib = fit(bad, kp[:5], return_grad=True)
    assert ib['status'].tolist() == [0, 0, 1, 0, 0] and ib['best_iter'][2] == 0
    assert torch.isnan(fb[2]).all() and torch.isnan(ib['history'][2]).all() and (ib['grad'][2] == 0).all()
    keep = [0, 1, 3, 4]
    assert torch.equal(fb[keep], f5[keep]) and torch.equal(ib['history'][keep], i5['history'][keep])
    # a NaN in the camera alone: the depth of every joint is NaN, which the Z + tz guard does not skip -> E(x_0) is NaN, status 1
    bad = init[:5].clone()
    bad[1, 0] = float('nan')
    fb, ib = fit(bad, kp[:5])
    assert ib['status'].tolist() == [0, 1, 0, 0, 0] and torch.isnan(ib['history'][1]).all() and ib['best_iter'][1] == 0
    assert torch.equal(fb[1, 1:], init[1, 1:]) and torch.isnan(fb[1, 0]) and torch.equal(fb[[0, 2, 3, 4]], f5[[0, 2, 3, 4]])
    # min(history) is E(x_0) of the fitted row.  With the priors on, E(x_0) of a fresh call measures them from the fitted row, so the
    # priors are switched off here; the fitted rotations go through 6D and back once more, which costs roundings (1e-5 relative)
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    free = KeypointFitter(ctx['smpl'], w_pose=0.0, w_orient=0.0, w_shape=0.0)
    ff, fi = free.fit(init[:5], kp[:5], return_history=True, stages=SHORT)
    _, zi = free.fit(ff, kp[:5], return_history=True, stages=())
    hmin, e0 = fi['history'].min(1).values.cpu().numpy(), zi['history'][:, 0].cpu().numpy()
    print('min(history) %s, E(x_0) of para_fit %s' % (hmin.tolist(), e0.tolist()), flush=True)
    assert np.abs(hmin - e0).max() <= 1e-5 * np.abs(hmin).max()
    # with the default priors on: min(history) less the prior terms of the best iterate (measured from the start, float64 on the host
    # from the two rows) is E(x_0) of the fitted row, whose own priors are zero
    _, zd = fitter.fit(f5, kp[:5], return_history=True, stages=())
    x0, xb = ko.unpack(torch.as_tensor(init[:5].cpu().numpy().astype(np.float64))), torch.as_tensor(f5.cpu().numpy().astype(np.float64))
    dR = ((xb[:, 13:].reshape(5, 24, 3, 3) - ko.rot6d_to_rotmat(x0[:, 13:].reshape(5, 24, 3, 2))) ** 2).sum((-1, -2))
    prior = fitter.w_orient * dR[:, 0] + fitter.w_pose * dR[:, 1:].sum(1) + fitter.w_shape * ((xb[:, 3:13] - x0[:, 3:13]) ** 2).sum(1)
    hmin, e0 = i5['history'].min(1).values.cpu().numpy().astype(np.float64), zd['history'][:, 0].cpu().numpy().astype(np.float64)
    print('default priors: min(history) %s, prior %s, E(x_0) of para_fit %s' % (hmin.tolist(), prior.tolist(), e0.tolist()), flush=True)
    assert (prior.numpy() > 1e-5).all() and np.abs(hmin - prior.numpy() - e0).max() <= 1e-5 * np.abs(hmin).max()
    # ... and bit for bit where the best iterate is x_0 itself (a start that the fit cannot improve: its own keypoints)
    own = _cu(ko.keypoints_of(m64, star[:2]))
    fo, oi = free.fit(_cu(star[:2]), own, return_history=True, stages=SHORT)
    _, zo = free.fit(fo, own, return_history=True, stages=())
    assert (oi['best_iter'] == 0).all() and torch.equal(fo, _cu(star[:2]))
    assert torch.equal(oi['history'].min(1).values, zo['history'][:, 0])


# ------------------------------------------------------------------------------------------------------------------ 4
def test_large_support(ctx):
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    big = ko.spread_model(ctx['model'])
    fitter = KeypointFitter(SMPL(big).cuda())
    assert 1700 <= fitter.tables(torch.device('cuda', torch.cuda.current_device()))['S'] <= 2100
    m64 = ko.model_tensors(big)
    _energy_and_gradient(fitter, m64, ko.as_tensors(m64, torch.float32), 3, 3, 'kp_fit_energy_gradient_large_support')


# ------------------------------------------------------------------------------------------------------------------ 5
def test_recovery(ctx):
    init, kp, star = ko.recovery_case(ctx['m64'])
    fit, info = ctx['fitter'].fit(_cu(init), _cu(kp), return_history=True)
    torch.cuda.synchronize()
    h = info['history'].cpu().numpy()
    reproj = lambda p: float(np.abs(ko.keypoints_of(ctx['m64'], p)[..., :2] - kp[..., :2]).mean())        # noqa: E731
    before, after = reproj(init), reproj(fit.cpu().numpy())
    print('recovery: E_0 %s E_T %s ratio %s, best %s, mean reprojection error %.4g -> %.4g' % (h[:, 0], h[:, -1], h[:, -1] / h[:, 0],
                                                                                               info['best_iter'].tolist(), before, after), flush=True)
    record('kp_fit_recovery', {'E0': h[:, 0].tolist(), 'ET': h[:, -1].tolist(), 'reproj_before': before, 'reproj_after': after})
    assert h.shape == (2, 101) and (h[:, -1] <= 0.1 * h[:, 0]).all()
    assert after < before


# ------------------------------------------------------------------------------------------------------------------ 6
def test_capture_and_replay(ctx):
    fitter = ctx['fitter']
    star = ko.make_para(4, 23)
    init, kp = _cu(ko.perturb(star, 24, pose_sigma=0.1, shift=0.03, scale=1.05)), _cu(ko.keypoints_of(ctx['m64'], star))
    eager, ei = fitter.fit(init, kp, return_history=True, stages=SHORT)
    eager, eh = eager.clone(), ei['history'].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fitter.fit(init, kp, return_history=True, stages=SHORT)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static, si = fitter.fit(init, kp, return_history=True, stages=SHORT)
    for _ in range(2):
        static.zero_()
        si['history'].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager) and torch.equal(si['history'], eh)
    del g


# ------------------------------------------------------------------------------------------------------------------ 7
def test_scene_demo_with_and_without_the_fit(ctx):
    from danet_densepose2smpl_amd import datasets, scene
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    model = DaNet(default_options(2), None, pretrained=False).cuda().eval()
    smpl = model.iuv2smpl.smpl
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (96, 80, 3)).astype(np.uint8), rng.integers(0, 256, (64, 72, 3)).astype(np.uint8)]
    boxes = [[scene.boxes_from_xywh([5., 8., 50., 70.]), scene.boxes_from_xywh([30., 20., 45., 60.])], [scene.boxes_from_xywh([10., 6., 40., 50.])]]
    plain = scene.SceneDemo(model, smpl, 2)
    r0, p0 = plain(frames, boxes)
    # keypoints: the model's own prediction in frame pixels, moved by a few pixels
    para = np.concatenate([p['para'] for p in p0]).astype(np.float64)
    P = para.shape[0]
    assert P == 3
    m64 = ko.model_tensors(ko.model_from_layer(smpl))
    pt = torch.as_tensor(para)
    j = ko.joints49(m64, pt[:, 3:13], pt[:, 13:].reshape(P, 24, 3, 3)).numpy()
    plan = plain.prepare(frames, boxes)
    cams = scene.person_cameras(para[:, :3], plan['tinv'], plan['shapes'], plan['person_frame'], plain.res, plain.focal)
    tz = cams['cam_t'][:, 2]
    xn, yn = (j[..., 0] + para[:, None, 1]) / (j[..., 2] + tz[:, None]), (j[..., 1] + para[:, None, 2]) / (j[..., 2] + tz[:, None])
    pr = cams['proj']
    kf = np.stack([pr[:, None, 0] * xn + pr[:, None, 1] * yn + pr[:, None, 2] + rng.uniform(2.0, 4.0, (P, 1)),
                   pr[:, None, 3] * xn + pr[:, None, 4] * yn + pr[:, None, 5] - rng.uniform(2.0, 4.0, (P, 1)), np.ones((P, 49))], -1)
    print('scene: predicted cams %s' % para[:, :3].tolist(), flush=True)
    keypoints = [[kf[0], kf[1]], [kf[2]]]
    fitted = scene.SceneDemo(model, smpl, 2, fitter=KeypointFitter(smpl, res=plain.res, focal=plain.focal))
    r1, p1 = fitted(frames, boxes, keypoints)
    loss = np.concatenate([p['fit_loss'] for p in p1])
    print('scene: fit_loss %s, fit_iter %s' % (loss.tolist(), [p['fit_iter'].tolist() for p in p1]), flush=True)
    assert loss.shape == (3, 2) and (loss[:, 1] <= loss[:, 0]).all()
    for a, b in zip(p0, p1):
        assert np.array_equal(a['para'], b['para_init']) and b['fit_iter'].shape == (a['para'].shape[0],)
        assert b['para'].shape == a['para'].shape and b['vertices'].shape == a['vertices'].shape
    assert any(not np.array_equal(a, b) for a, b in zip(r0, r1))
    # no fitter, or no keypoints: today's call, bit for bit
    for demo, kw in ((fitted, {}), (plain, {'keypoints': keypoints}), (scene.SceneDemo(model, smpl, 2), {})):
        r2, p2 = demo(frames, boxes, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(r0, r2))
        for a, b in zip(p0, p2):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
