"""Keypoint fit, the checks that need no GPU: the float64 oracle against the LBS oracle, the support sub-tables against the full
tables, the 6D round trip, the keypoint conventions, the refusals, and the oracle's own recovery of the synthetic case -- the
condition the GPU recovery test relies on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kp_fit_oracle as ko
from conftest import ROOT, rand_pose_shape


def test_oracle_joints_agree_with_the_lbs_oracle(smpl_model):
    import oracle
    betas, pose = rand_pose_shape(3, seed=11)
    R = ko.rodrigues(pose.reshape(3, 24, 3))
    _, j_ref = oracle.lbs_forward(smpl_model, betas, R.reshape(3, 216), True, np.float64)       # (rotation matrices in: one Rodrigues rule)
    j = ko.joints54(ko.model_tensors(smpl_model), torch.as_tensor(betas), torch.as_tensor(R)).numpy()
    err = np.abs(j - j_ref).max()
    print('oracle joints54 against oracle.lbs_forward: %.3g' % err)
    assert err <= 1e-10


@pytest.mark.parametrize('spread', [False, True])
def test_sub_tables_give_the_joints_of_the_full_tables(smpl_model, spread):
    from danet_densepose2smpl_amd import constants
    from danet_densepose2smpl_amd.kp_fit import fit_tables, TILE
    from danet_densepose2smpl_amd.smpl import SMPL
    assert ko.JOINT_MAP_49 == constants.JOINT_MAP_49
    smpl = SMPL(ko.spread_model(smpl_model) if spread else smpl_model)
    t = fit_tables(smpl)
    S, Sp = t['S'], t['Sp']
    print('support: %d vertices, padded to %d' % (S, Sp))
    assert (300 <= S <= 21 + 9 * 32) if not spread else (1700 <= S <= 2100)       # (21 landmarks + 9 rows of 32, less the shared ones)
    assert Sp % TILE == 0 and 0 <= Sp - S < TILE and t['basis'].shape == (217, Sp * 3) and t['basisT'].shape == (Sp * 3, 224)
    assert np.array_equal(t['basisT'][:, :217], t['basis'].T) and not t['basisT'][:, 217:].any() and not t['weights'][S:].any()
    assert np.array_equal(t['support'][t['lm']], smpl.landmark_verts.numpy()) and t['basis'].dtype == np.float64
    full = ko.model_from_layer(smpl)                       # the layer's float32 buffers, folded here in float64
    V = full['v_template'].shape[0]
    Jr = full['J_regressor'].astype(np.float64)
    Jt = Jr @ full['v_template'].astype(np.float64)
    Jd = (Jr @ full['shapedirs'].astype(np.float64).reshape(V, 30)).reshape(72, 10)
    betas, pose = rand_pose_shape(4, seed=21, pose_sigma=0.4)
    R = ko.rodrigues(pose.reshape(4, 24, 3))
    j_sub = ko.joints54_from_tables(t, Jt, Jd, full['parents'], betas, R)
    j_full = ko.joints54(ko.model_tensors(full), torch.as_tensor(betas), torch.as_tensor(R)).numpy()
    err = np.abs(j_sub - j_full).max()
    print('54 joints, sub-tables against full tables: %.3g' % err)
    assert err <= 1e-12
    # the layer's own folded regression is this one rounded to float32
    assert np.abs(smpl.J_template.numpy() - Jt).max() <= 1e-7 and np.abs(smpl.J_shapedirs.numpy() - Jd).max() <= 1e-7


def test_rot6d_round_trip_of_orthonormal_matrices():
    R = torch.as_tensor(ko.rodrigues(np.random.default_rng(3).normal(0, 1.0, (5, 24, 3))))
    back = ko.rot6d_to_rotmat(R[..., :2])
    assert (back - R).abs().max() <= 1e-12
    para = torch.cat([torch.zeros(5, 13, dtype=torch.float64), R.reshape(5, 216)], 1)
    x = ko.unpack(para)
    assert x.shape == (5, 157)
    assert torch.equal(x[:, 13:].reshape(5, 24, 3, 2), R[..., :2])          # [3,2] row-major, as rot6d_to_rotmat reads x.view(-1,3,2)


def test_openpose_rows_and_the_crop_round_trip():
    from danet_densepose2smpl_amd import datasets, scene
    from danet_densepose2smpl_amd.kp_fit import openpose_to_j49
    rng = np.random.default_rng(5)
    k25 = rng.uniform(0, 100, (25, 3)).astype(np.float32)
    for src in (k25, k25.reshape(-1).tolist(), np.stack([k25, k25 + 1])):
        out = openpose_to_j49(src)
        assert out.shape[-2:] == (49, 3) and out.dtype == np.float32
        assert np.array_equal(out[..., :25, :].reshape(-1, 25, 3)[0], k25) and not out[..., 25:, :].any()
    with pytest.raises(ValueError):
        openpose_to_j49(np.zeros((18, 3)))
    # person_cameras' proj takes (x_n, y_n) to frame pixels; keypoints_to_crop takes those back to kappa (x_n, y_n), kappa = 2 f / 224
    P, res, focal = 3, 224, 5000.
    center, scale = rng.uniform(40, 200, (P, 2)), rng.uniform(0.4, 1.5, P)
    t, tinv = datasets.crop_transforms(center, scale, np.zeros(P), res)
    cams = scene.person_cameras(np.tile([0.9, 0.0, 0.0], (P, 1)), tinv, [[300, 400]], np.zeros(P, np.int64), res, focal)
    xn = rng.uniform(-0.02, 0.02, (P, 49, 2))
    pr = cams['proj']
    frame = np.stack([pr[:, None, 0] * xn[..., 0] + pr[:, None, 1] * xn[..., 1] + pr[:, None, 2],
                      pr[:, None, 3] * xn[..., 0] + pr[:, None, 4] * xn[..., 1] + pr[:, None, 5], rng.uniform(0, 1, (P, 49))], -1)
    back = scene.keypoints_to_crop(frame, t, res)
    assert np.abs(back[..., :2] - 2 * focal / 224. * xn).max() <= 1e-9 and np.array_equal(back[..., 2], frame[..., 2])
    # a res other than 224: the same normalised coordinates
    t2, tinv2 = datasets.crop_transforms(center, scale, np.zeros(P), 128)
    pr2 = scene.person_cameras(np.tile([0.9, 0.0, 0.0], (P, 1)), tinv2, [[300, 400]], np.zeros(P, np.int64), 128, focal)['proj']
    frame2 = np.stack([pr2[:, None, 0] * xn[..., 0] + pr2[:, None, 1] * xn[..., 1] + pr2[:, None, 2],
                       pr2[:, None, 3] * xn[..., 0] + pr2[:, None, 4] * xn[..., 1] + pr2[:, None, 5], np.ones((P, 49))], -1)
    assert np.abs(scene.keypoints_to_crop(frame2, t2, 128)[..., :2] - 2 * focal / 224. * xn).max() <= 1e-9


def test_cpu_tensors_are_refused(smpl_model, monkeypatch):
    from danet_densepose2smpl_amd import _lib, kp_fit
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter, parse_stages

    def no_library():
        raise AssertionError('the library was asked for before the CPU tensor was refused')
    monkeypatch.setattr(_lib, 'lib', no_library)
    from danet_densepose2smpl_amd.smpl import SMPL
    fitter = KeypointFitter(SMPL(smpl_model))
    assert fitter.iterations == 100 and parse_stages(fitter.stages) == ([30, 70], [3, 15])
    with pytest.raises(RuntimeError, match=r'GPU only \(.*got a cpu tensor\); there is no CPU path'):
        fitter.fit(torch.zeros(1, 229), torch.zeros(1, 49, 3))
    with pytest.raises(RuntimeError, match=r'GPU only \(.*got a cpu tensor\); there is no CPU path'):
        fitter.fit(torch.zeros(1, 229), torch.zeros(1, 49, 3), return_history=True, return_grad=True, stages=())
    assert not hasattr(kp_fit, 'keypoint_fit')          # the fitter is the one entry; there is no second public wrapper
    with pytest.raises(ValueError):
        KeypointFitter(SMPL(smpl_model), stages=((3, 'cam+hands'),))


@pytest.mark.parametrize('extra, message', [([], '--fit needs --keypoints_dir'), (['--boxes', 'boxes.json'], '--fit cannot be combined with --boxes'),
                                            (['--boxes', 'boxes.json', '--keypoints_dir', 'kp'], '--fit cannot be combined with --boxes')])
def test_tool_refuses_fit_without_keypoints(tmp_path, extra, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'demo_scene.py'), '--img_dir', str(tmp_path), '--fit'] + extra,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and message in r.stderr and 'unrecognized arguments' not in r.stderr, r.stderr[-2000:]


def test_oracle_recovers_the_synthetic_case(smpl_model):
    m = ko.model_tensors(smpl_model)
    init, kp, star = ko.recovery_case(m)
    r = ko.fit(m, init, kp)
    h = r['history']
    reproj = lambda p: np.abs(ko.keypoints_of(m, p)[..., :2] - kp[..., :2]).mean()           # noqa: E731
    print('E_0 %s  E_T %s  ratio %s  best %s  reprojection %.4g -> %.4g' % (h[:, 0], h[:, -1], h[:, -1] / h[:, 0], r['best_iter'], reproj(init),
                                                                         reproj(r['para_fit'])))
    assert h.shape == (2, 101) and (r['status'] == 0).all()
    assert (h[:, -1] <= 0.05 * h[:, 0]).all()
    assert reproj(r['para_fit']) < 0.25 * reproj(init)


def test_fill_args_writes_the_shared_fields_alike_into_both_structs():
    """The one fill of kp_fit.py on the two argument structs: every field they share gets the same value, and the dense struct's own
    fields come from the same call."""
    import ctypes
    from danet_densepose2smpl_amd import _lib, kp_fit
    assert ctypes.sizeof(_lib.KpFitArgs) == 18 * 8 + 8 * 4 + 8 * 4 + 8 * 4 and ctypes.sizeof(_lib.DenseFitArgs) == 25 * 8 + 8 * 4 + 9 * 4 + 11 * 4
    shared = [k for k, _ in _lib.KpFitArgs._fields_]
    assert shared == [k for k, _ in _lib.DenseFitArgs._fields_ if k in shared] and len(shared) == 36
    pointers = {k: 4096 + 64 * i for i, (k, t) in enumerate(_lib.KpFitArgs._fields_) if t is ctypes.c_void_p}
    pointers['grad0'] = None
    sizes = {'P': 3, 'NB': 10, 'S': 100, 'Sp': 128, 'NL': 21, 'NE': 9}
    floats = {'focal': 5000., 'res': 224., 'kappa': 44.625, 'sigma': 0.1, 'w_orient': 0.005, 'w_pose': 0.0025, 'w_shape': 0.002, 'lr': 0.02}
    stages = kp_fit.parse_stages(((3, 'cam+orient'), (5, 'all'), (2, 'shape')))
    a = kp_fit.fill_args(_lib.KpFitArgs(), pointers, sizes, stages, floats)
    own = {'lm_corner': 9000, 'lm_w': 9064, 'csr_off': 9128, 'csr_lm': 9192, 'csr_w': 9256, 'obs': 9320, 'gate': 9384}
    b = kp_fit.fill_args(_lib.DenseFitArgs(), dict(pointers, **own), dict(sizes, M=259), stages,
                         dict(floats, w_dense=0.25, sigma_dense=0.05, min_cos=0.125))
    for k in shared:
        va, vb = getattr(a, k), getattr(b, k)
        assert (list(va), list(vb)) == ([3, 5, 2, 0], [3, 5, 2, 0]) or (list(va), list(vb)) == ([3, 15, 8, 0], [3, 15, 8, 0]) if k.startswith('stage_') else va == vb, k
    assert a.para == 4096 and a.grad0 is None and (a.P, a.NB, a.S, a.Sp, a.NL, a.NE, a.nstages, a.T) == (3, 10, 100, 128, 21, 9, 3, 10)
    assert (a.focal, a.res, a.kappa, a.lr) == (5000., 224., 44.625, np.float32(0.02)) and a.w_pose == np.float32(0.0025)
    assert all(getattr(b, k) == v for k, v in own.items()) and b.M == 259 and (b.w_dense, b.sigma_dense, b.min_cos) == (0.25, np.float32(0.05), 0.125)
