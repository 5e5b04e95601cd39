"""Dense fit on the GPU (csrc/dense_fit.hip, dense_fit.py, DESIGN.md "the dense fit rule") against the float64 oracle of
dense_fit_oracle.py.

The error bound is test_gpu_kp_fit.py's, restated: the oracle runs a second time in float32, and for a block of outputs

    max |kernel - f64|  <=  4 * max |oracle_f32 - f64|  +  8 * 2^-23 * max |f64|           (maxima over the block)

Blocks: the energies of the batch, the camera gradients of the batch, and per person the shape gradient, the 6D gradient, the
history, and camera / betas / rotations of para_fit; for the observation x, y and W of the batch over the certain landmarks.
Landmarks whose decisions a rounding could flip (dense_fit_oracle.uncertain_*) get confidence zero in the inputs of the fit and are
left out of the observation's comparison; their share stays under 5 %.  The measured ratios are printed and recorded.

Measured on the MI355X (profiles/dense_fit_parity_measured.jsonl): see DESIGN.md "the dense fit rule"."""
import numpy as np
import pytest
import torch

import dense_fit_oracle as do
import kp_fit_oracle as ko
from conftest import record

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
SHORT = ((3, 'cam+orient'), (5, 'all'))


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope='module')
def ctx(smpl_model):
    from danet_densepose2smpl_amd.dense_fit import DenseFitter
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL(smpl_model).cuda()
    m64 = ko.model_tensors(smpl_model)
    fitters = {G: DenseFitter(smpl, smpl_model=smpl_model, grid=G) for G in (2, 4, 6)}
    return {'smpl': smpl, 'fitters': fitters, 'fitter': fitters[4], 'kp_fitter': KeypointFitter(smpl), 'm64': m64,
            'm32': ko.as_tensors(m64, torch.float32), 'model': smpl_model}


def bound_block(tag, got, r64, r32, ratios):
    err, err32, scale = np.abs(got - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    bound = 4.0 * err32 + 8.0 * EPS32 * scale
    ratios.append((tag, float(err), float(err32), float(bound)))
    return err <= bound


def _report(name, ratios):
    worst = max(ratios, key=lambda r: r[1] / max(r[3], 1e-300))
    rel = [r[1] / r[2] for r in ratios if r[2] > 0] or [0.0]
    print('%s: %d blocks, err / err_f32 median %.2f max %.2f; tightest block %s err %.3g (f32 oracle %.3g, bound %.3g)'
          % (name, len(ratios), float(np.median(rel)), float(np.max(rel)), worst[0], worst[1], worst[2], worst[3]), flush=True)
    record(name, {'blocks': len(ratios), 'all': [[r[0], r[1], r[2], r[3]] for r in ratios], 'ratio_median': float(np.median(rel)), 'ratio_max': float(np.max(rel)),
                  'tightest': {'block': worst[0], 'err': worst[1], 'err_f32': worst[2], 'bound': worst[3]}})


@pytest.fixture(scope='module')
def bodies():
    """Rastered bodies shared by the tests: {S: (para [3,229], iuv [3,3,S,S] f32)}."""
    para = ko.make_para(3, 11)
    verts = do.vertices_of(do.synthetic()[0], para)
    return {S: (para, do.raster(verts, para[:, :3], S)) for S in (32, 56)}


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('S,P,G', [(32, 3, 4), (32, 3, 2), (56, 1, 4), (56, 1, 2)])
def test_observation(ctx, bodies, S, P, G):
    fitter, lt = ctx['fitters'][G], do.tables(G)
    iuv = bodies[S][1][:P].copy()
    if P == 3:
        iuv[1] = 0.0                                                     # all background
        gone = np.floor(24.0 * iuv[2, 0].astype(np.float64) + 0.5) == 2  # one image with part 2 absent
        assert gone.sum() > 0
        iuv[2][:, gone] = 0.0
    o64, W64, margin = do.extract(iuv, lt)
    o32, W32, _ = do.extract(iuv, lt, dtype=np.float32)
    unc = do.uncertain_obs(W64, margin)
    assert unc.mean() <= 0.05
    cert = ~unc
    d = _cu(iuv)
    obs, W = fitter.landmarks(d, return_weight=True)
    again, Wa = fitter.landmarks(d, return_weight=True)
    torch.cuda.synchronize()
    assert torch.equal(obs, again) and torch.equal(W, Wa)                # two runs, one result
    assert torch.equal(obs, fitter.landmarks(d))
    for p in range(P):                                                   # a batch is its rows
        o1, W1 = fitter.landmarks(d[p:p + 1], return_weight=True)
        assert torch.equal(o1[0], obs[p]) and torch.equal(W1[0], W[p])
    got, gW = obs.cpu().numpy().astype(np.float64), W.cpu().numpy().astype(np.float64)
    assert got.shape == (P, lt['M'], 3)
    seen = o64[..., 2] > 0
    assert (seen & cert).sum() > 0.25 * lt['M'] and (~seen & cert)[0].any()
    # c = 0 rows are exactly zero, on both sides
    assert (got[cert & ~seen] == 0).all() and (got[got[..., 2] == 0] == 0).all()
    assert np.array_equal(got[..., 2][cert] > 0, seen[cert])
    if P == 3:
        assert (got[1] == 0).all() and (gW[1] == 0).all()
        assert (got[2][lt['cell'][:, 0] == 2] == 0).all() and seen[0][lt['cell'][:, 0] == 2].any()
    ratios, ok = [], True
    for tag, g, a, b in (('x', got[..., 0], o64[..., 0], o32[..., 0]), ('y', got[..., 1], o64[..., 1], o32[..., 1]),
                         ('c', got[..., 2], o64[..., 2], o32[..., 2]), ('W', gW, W64, W32)):
        ok &= bound_block(tag, g[cert], a[cert], b[cert].astype(np.float64), ratios)
    _report('dense_landmarks_S%d_P%d_G%d' % (S, P, G), ratios)
    assert ok, ratios


# ------------------------------------------------------------------------------------------------------------------ 2
def _edge_case(m64, lt, P, seed):
    """ko.edge_case's rows and keypoints, and observations: the landmarks of the perturbed target projected by the rule's camera,
    confidences in [0,1] with zeros among them; row 1 (P > 1) has every c zero, row 2 (P > 2) has landmarks behind the depth guard."""
    para, kp = ko.edge_case(m64, P, seed)
    rng = np.random.default_rng(seed + 200)
    target = ko.perturb(para, seed + 1, pose_sigma=0.1, shift=0.02, scale=1.0)
    c = dict(ko.DEFAULTS, kappa=2 * 5000. / 224.)
    obs = np.zeros((P, lt['M'], 3))
    D0 = np.zeros((P, lt['M']))
    for which, rows in (('target', target), ('start', para)):
        p64 = torch.as_tensor(rows.astype(np.float64))
        verts, _ = do.lbs(m64, p64[:, 3:13], p64[:, 13:].reshape(P, 24, 3, 3))
        pts, _ = do.landmark_points(verts, lt)
        uv, D = ko.project(pts, p64[:, :3], c['focal'], c['res'], c['kappa'])
        if which == 'target':
            obs[..., :2] = np.clip(np.nan_to_num(uv.numpy(), nan=0.0, posinf=3.0, neginf=-3.0), -3.0, 3.0)
        else:
            D0 = D.numpy()
    obs[..., 2] = rng.uniform(0.0, 1.0, (P, lt['M']))
    obs[:, rng.choice(lt['M'], lt['M'] // 5, replace=False), 2] = 0.0
    obs[0, 5, :2] += 4.0                                                  # one landmark far away (saturates rho_d)
    obs[0, 5, 2] = 0.9
    if P > 1:
        obs[1, :, 2] = 0.0
    obs = obs.astype(np.float32)
    cos = do.gate_cos(m64, lt, ko.unpack(torch.as_tensor(para.astype(np.float64))), c).numpy()
    unc = do.uncertain_gate(cos) | (np.abs(D0 - 1e-6) < 1e-3)
    if P > 2:
        assert (D0[2] <= 1e-6).any() and (D0[2] > 1e-6).any() and (D0[:2] > 1e-6).all()
    return para, kp, do.certain_obs(obs, unc), unc


@pytest.mark.parametrize('P', [1, 3])
def test_energy_and_gradient_at_x0(ctx, P):
    fitter, m64, m32, lt = ctx['fitter'], ctx['m64'], ctx['m32'], do.tables(4)
    para, kp, obs, unc = _edge_case(m64, lt, P, P)
    zeros = np.zeros_like(obs)
    ratios, ok = [], True
    for mode, k, o in (('dense', None, obs), ('kp', kp, zeros), ('both', kp, obs)):
        r64 = do.fit(m64, lt, para, o, k, stages=())
        r32 = do.fit(m32, lt, para, o, k, stages=(), dtype=torch.float32)
        fit, info = fitter.fit(_cu(para), obs=_cu(o), keypoints=None if k is None else _cu(k), return_history=True, return_grad=True, stages=())
        torch.cuda.synchronize()
        E, g = info['history'].cpu().numpy().astype(np.float64), info['grad'].cpu().numpy().astype(np.float64)
        assert E.shape == (P, 1) and g.shape == (P, 157) and (info['status'].cpu().numpy() == 0).all() and (info['best_iter'].cpu().numpy() == 0).all()
        assert torch.equal(fit, _cu(para))                               # T = 0: the row itself
        gate = info['gate'].cpu().numpy()
        assert gate.shape == (P, lt['M']) and np.array_equal(gate[~unc], r64['gate'][~unc]) and 0.2 < gate[0].mean() < 0.8
        if mode == 'dense' and P > 1:                                    # the row without observations: no data term, no gradient
            assert E[1, 0] == 0 and (g[1] == 0).all()
        ok &= bound_block(mode + '.E', E, r64['history'], r32['history'], ratios)
        ok &= bound_block(mode + '.g_cam', g[:, :3], r64['grad'][:, :3], r32['grad'][:, :3], ratios)
        for p in range(P):
            if mode == 'dense' and p == 1:
                continue
            ok &= bound_block('%s.g_betas[%d]' % (mode, p), g[p, 3:13], r64['grad'][p, 3:13], r32['grad'][p, 3:13], ratios)
            ok &= bound_block('%s.g_a[%d]' % (mode, p), g[p, 13:], r64['grad'][p, 13:], r32['grad'][p, 13:], ratios)
        if mode == 'kp':
            # all landmark confidences zero: the keypoint fit's own numbers, within the same bound
            kfit, kinfo = ctx['kp_fitter'].fit(_cu(para), _cu(k), return_history=True, return_grad=True, stages=())
            kE, kg = kinfo['history'].cpu().numpy().astype(np.float64), kinfo['grad'].cpu().numpy().astype(np.float64)
            k64 = ko.fit(m64, para, k, stages=())
            assert np.array_equal(k64['history'], r64['history']) or np.abs(k64['history'] - r64['history']).max() <= 1e-12 * np.abs(k64['history']).max()
            for tag, a, b, x64, x32 in (('E', E, kE, r64['history'], r32['history']), ('g_cam', g[:, :3], kg[:, :3], r64['grad'][:, :3], r32['grad'][:, :3]),
                                        ('g_betas', g[:, 3:13], kg[:, 3:13], r64['grad'][:, 3:13], r32['grad'][:, 3:13]),
                                        ('g_a', g[:, 13:], kg[:, 13:], r64['grad'][:, 13:], r32['grad'][:, 13:])):
                bound = 4.0 * np.abs(x32 - x64).max() + 8.0 * EPS32 * np.abs(x64).max()
                d = float(np.abs(a - b).max())
                print('against KeypointFitter: %s differs by %.3g (bound %.3g)' % (tag, d, bound), flush=True)
                ok &= d <= bound
    _report('dense_fit_energy_gradient_P%d' % P, ratios)
    assert ok, ratios


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('P,G', [(4, 4), (1, 6)])
def test_short_trajectory(ctx, P, G):
    fitter, m64, m32, lt = ctx['fitters'][G], ctx['m64'], ctx['m32'], do.tables(G)
    assert lt['M'] == {4: 259, 6: 560}[G]
    seed = 3
    star = ko.make_para(P, seed)
    init = ko.perturb(star, seed + 1, pose_sigma=0.1, shift=0.03, scale=1.05)
    o, W, margin = do.extract(do.raster(do.vertices_of(ctx['model'], star), star[:, :3], 56), lt)
    cos = do.gate_cos(m64, lt, ko.unpack(torch.as_tensor(init.astype(np.float64))), dict(ko.DEFAULTS, kappa=2 * 5000. / 224.)).numpy()
    unc = do.uncertain_obs(W, margin) | do.uncertain_gate(cos)
    obs = do.certain_obs(o.astype(np.float32), unc)
    kp = ko.keypoints_of(m64, star)
    kp[:, :, 2] = np.random.default_rng(seed).uniform(0.2, 1.0, (P, 49))
    r64 = do.fit(m64, lt, init, obs, kp, stages=SHORT)
    r32 = do.fit(m32, lt, init, obs, kp, stages=SHORT, dtype=torch.float32)
    agree = r64['best_iter'] == r32['best_iter']
    assert (~agree).sum() <= P // 4                                       # the oracle alone stays within the cap
    fit, info = fitter.fit(_cu(init), obs=_cu(obs), keypoints=_cu(kp), return_history=True, stages=SHORT)
    torch.cuda.synchronize()
    h, bi, pf = info['history'].cpu().numpy().astype(np.float64), info['best_iter'].cpu().numpy(), fit.cpu().numpy().astype(np.float64)
    assert h.shape == (P, 9) and (info['status'].cpu().numpy() == 0).all()
    print('history[0]: %s; best_iter %s (f64 %s)' % (np.round(h[0], 5).tolist(), bi.tolist(), r64['best_iter'].tolist()), flush=True)
    assert np.array_equal(bi[agree], r64['best_iter'][agree]) and (bi > 0).all()
    assert np.array_equal(info['gate'].cpu().numpy()[~unc], r64['gate'][~unc])
    ratios, ok = [], True
    for p in range(P):
        ok &= bound_block('history[%d]' % p, h[p], r64['history'][p], r32['history'][p], ratios)
        for tag, sl in (('cam', slice(0, 3)), ('betas', slice(3, 13)), ('rot', slice(13, 229))):
            ok &= bound_block('para_fit.%s[%d]' % (tag, p), pf[p, sl], r64['para_fit'][p, sl], r32['para_fit'][p, sl], ratios)
    _report('dense_fit_short_trajectory_P%d_G%d' % (P, G), ratios)
    assert ok, ratios


# ------------------------------------------------------------------------------------------------------------------ 4
def test_bit_properties(ctx):
    fitter, lt = ctx['fitter'], do.tables(4)
    star = ko.make_para(5, 17)
    init = _cu(ko.perturb(star, 18, pose_sigma=0.1, shift=0.03, scale=1.05))
    iuv = _cu(do.raster(do.vertices_of(ctx['model'], star), star[:, :3], 32))
    fit = lambda p, i, **kw: fitter.fit(p, i, return_history=True, stages=SHORT, **kw)          # noqa: E731
    # zero observations and no keypoints: the input row, bit for bit
    f0, i0 = fit(init, torch.zeros_like(iuv))
    assert torch.equal(f0, init) and (i0['obs'] == 0).all() and (i0['history'] == 0).all() and (i0['best_iter'] == 0).all()
    f0, i0 = fitter.fit(init, obs=torch.zeros(5, lt['M'], 3, device='cuda'), return_history=True, stages=SHORT)
    assert torch.equal(f0, init) and (i0['best_iter'] == 0).all()
    # a batch is its rows; two runs are one
    f5, i5 = fit(init, iuv)
    again, ia = fit(init, iuv)
    for k in ('history', 'best_iter', 'gate', 'obs', 'status'):
        assert torch.equal(i5[k], ia[k]), k
    assert torch.equal(f5, again) and (i5['best_iter'] > 0).all() and not torch.equal(f5, init)
    for p in range(5):
        f1, i1 = fit(init[p:p + 1], iuv[p:p + 1])
        assert torch.equal(f1[0], f5[p]) and torch.equal(i1['history'][0], i5['history'][p]) and i1['best_iter'][0] == i5['best_iter'][p]
        assert torch.equal(i1['gate'][0], i5['gate'][p])
    # a row of NaN: status 1, unchanged, neighbours untouched
    bad = init.clone()
    bad[2] = float('nan')
    fb, ib = fitter.fit(bad, iuv, return_history=True, return_grad=True, stages=SHORT)
    assert ib['status'].tolist() == [0, 0, 1, 0, 0] and ib['best_iter'][2] == 0
    assert torch.isnan(fb[2]).all() and torch.isnan(ib['history'][2]).all() and (ib['grad'][2] == 0).all() and (ib['gate'][2] == 0).all()
    keep = [0, 1, 3, 4]
    assert torch.equal(fb[keep], f5[keep]) and torch.equal(ib['history'][keep], i5['history'][keep]) and torch.equal(ib['gate'][keep], i5['gate'][keep])


# ------------------------------------------------------------------------------------------------------------------ 5
def test_recovery(ctx):
    """The device end to end on the dense recovery case: rasteriser -> landmarks -> 100 iterations."""
    from danet_densepose2smpl_amd import ops
    fitter, m64, lt, model = ctx['fitter'], ctx['m64'], do.tables(4), ctx['model']
    case = do.dense_recovery_case()
    vm, faces, tex = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in do.synthetic()[2])
    iuv = ops.iuv_raster(_cu(case['verts_star']), _cu(case['star'][:, :3]), vm, faces, tex, 5000., 224, 56)
    init = _cu(case['init'])
    fit, info = fitter.fit(init, iuv, return_history=True)
    torch.cuda.synchronize()
    h, obs = info['history'].cpu().numpy().astype(np.float64), info['obs'].cpu().numpy()
    assert h.shape == (4, 101) and (info['status'].cpu().numpy() == 0).all()
    r64 = do.fit(m64, lt, case['init'], obs)                              # the oracle on the device's own observations
    ratio, ratio64 = h[:, -1] / h[:, 0], r64['history'][:, -1] / r64['history'][:, 0]
    before = do.mean_vertex_error(model, case['init'], case['verts_star'])
    after = do.mean_vertex_error(model, fit.cpu().numpy(), case['verts_star'])
    kp = _cu(ko.keypoints_of(m64, case['star']))
    after_kp = do.mean_vertex_error(model, ctx['kp_fitter'].fit(init, kp).cpu().numpy(), case['verts_star'])
    after_both = do.mean_vertex_error(model, fitter.fit(init, iuv, keypoints=kp).cpu().numpy(), case['verts_star'])
    print('dense recovery: E_T / E_0 %s (float64 oracle %s), best %s; mean vertex error mm %s -> %s; keypoints only %s (mean %.1f), both %s (mean %.1f)'
          % (np.round(ratio, 4).tolist(), np.round(ratio64, 4).tolist(), info['best_iter'].tolist(), np.round(before * 1e3, 1).tolist(),
             np.round(after * 1e3, 1).tolist(), np.round(after_kp * 1e3, 1).tolist(), after_kp.mean() * 1e3, np.round(after_both * 1e3, 1).tolist(),
             after_both.mean() * 1e3), flush=True)
    record('dense_fit_recovery', {'ratio': ratio.tolist(), 'ratio_f64': ratio64.tolist(), 'mve_before': before.tolist(), 'mve_after': after.tolist(),
                                  'mve_keypoints_only': after_kp.tolist(), 'mve_both': after_both.tolist()})
    assert (ratio <= 1.5 * ratio64).all()
    assert (after < before).all()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_capture_and_replay(ctx, bodies):
    fitter = ctx['fitter']
    star = bodies[32][0]
    init, iuv = _cu(ko.perturb(star, 24, pose_sigma=0.1, shift=0.03, scale=1.05)), _cu(bodies[32][1])
    eager, ei = fitter.fit(init, iuv, return_history=True, stages=SHORT)
    eager, eh, eg = eager.clone(), ei['history'].clone(), ei['gate'].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fitter.fit(init, iuv, return_history=True, stages=SHORT)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static, si = fitter.fit(init, iuv, return_history=True, stages=SHORT)
    for _ in range(2):
        static.zero_()
        si['history'].zero_()
        si['gate'].zero_()
        si['obs'].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager) and torch.equal(si['history'], eh) and torch.equal(si['gate'], eg)
    assert (ei['best_iter'] > 0).all()
    del g


# ------------------------------------------------------------------------------------------------------------------ 7
def test_scene_demo_with_a_dense_fitter(ctx):
    from danet_densepose2smpl_amd import scene
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.dense_fit import DenseFitter
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    model = DaNet(default_options(2), None, pretrained=False).cuda().eval()
    smpl = model.iuv2smpl.smpl
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (96, 80, 3)).astype(np.uint8)]
    boxes = [[scene.boxes_from_xywh([5., 8., 50., 70.]), scene.boxes_from_xywh([30., 20., 45., 60.])]]
    plain = scene.SceneDemo(model, smpl, 2)
    r0, p0 = plain(frames, boxes)
    dense = scene.SceneDemo(model, smpl, 2, fitter=DenseFitter(smpl, smpl_model=ctx['model'], res=plain.res, focal=plain.focal))
    plan = dense.prepare(frames, boxes)
    para, iuv = dense.infer(plan, return_iuv=True)
    assert torch.equal(para, plain.infer(plan)) and iuv.shape[:2] == (2, 3) and iuv.shape[2] == iuv.shape[3]
    r1, p1 = dense(frames, boxes)                                         # no keypoints at all
    loss = np.concatenate([p['fit_loss'] for p in p1])
    print('scene: fit_loss %s, fit_iter %s, IUV pixels on a body %d' % (loss.tolist(), [p['fit_iter'].tolist() for p in p1], int((iuv[:, 0] > 0).sum())), flush=True)
    assert loss.shape == (2, 2) and (loss[:, 1] <= loss[:, 0]).all()
    for a, b in zip(p0, p1):
        assert np.array_equal(a['para'], b['para_init']) and b['fit_iter'].shape == (a['para'].shape[0],)
        assert b['para'].shape == a['para'].shape and b['vertices'].shape == a['vertices'].shape
    # keypoints of confidence zero beside the image: the same fit
    r3, p3 = dense(frames, boxes, [[np.zeros((49, 3)), np.zeros((25, 3))]])
    assert all(np.array_equal(a, b) for a, b in zip(r1, r3)) and all(np.array_equal(p1[0][k], p3[0][k]) for k in p1[0])
    # an untrained network's image may hold nothing to fit, and its rows may lie anywhere: SceneDemo.fit on known rows and the image
    # of their bodies seen by a shifted camera must lower every row's energy (the scene kappa, 2 focal / 224)
    from danet_densepose2smpl_amd import ops
    vm, faces, tex = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in do.synthetic()[2])
    known = _cu(ko.make_para(2, 5))
    cam = known[:, :3].clone()
    cam[:, 1:] += 0.05
    shifted = ops.iuv_raster(dense.vertices(known), cam, vm, faces, tex, plain.focal, 224, 56)
    pf, info = dense.fit(known, plan, None, shifted)
    h, bi = info['history'].cpu().numpy(), info['best_iter'].cpu().numpy()
    print('scene: shifted camera: E_0 %s, E_best %s, best_iter %s' % (h[:, 0].tolist(), h[np.arange(2), bi].tolist(), bi.tolist()), flush=True)
    assert (h[:, 0] > 0).all() and (bi > 0).all() and (h[np.arange(2), bi] < h[:, 0]).all() and not torch.equal(pf, known)
    # without the fitter: today's outputs
    r2, p2 = scene.SceneDemo(model, smpl, 2)(frames, boxes)
    assert all(np.array_equal(a, b) for a, b in zip(r0, r2))
    for a, b in zip(p0, p2):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
