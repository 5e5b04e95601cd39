"""Host-side checks of the dense fit (dense_fit.py, DESIGN.md "the dense fit rule"): the tables, the pixel convention of the
observation, float64 recovery of the rule itself on the dense recovery case, and the refusals that come before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import dense_fit_oracle as do
import kp_fit_oracle as ko
import texture_oracle as to

# the issue's prototype at G = 4 over landmarks with c >= 0.5: median distance between observation and projection, in pixels
RECORDED_MEDIAN_PX = {56: 0.45, 64: 0.50}


@pytest.fixture(scope='module')
def layer(smpl_model):
    from danet_densepose2smpl_amd.smpl import SMPL
    return SMPL(smpl_model)


@pytest.mark.parametrize('G,M,NV', [(3, 154, None), (4, 259, 678), (6, 560, 1306)])
def test_tables(layer, G, M, NV):
    from danet_densepose2smpl_amd import dense_fit
    at = do.synthetic()[1]
    face, bary = to.texture_map(at, G)
    t = dense_fit.dense_tables(layer, at, face, bary)
    lt = do.tables(G)
    assert t['M'] == M == lt['M'] and t['G'] == G and t['M'] <= 24 * G * G
    assert np.array_equal(t['cell'], lt['cell']) and t['cell'].dtype == np.int32
    assert (np.diff(t['cell'][:, 0] * 64 + t['cell'][:, 1] * 8 + t['cell'][:, 2]) > 0).all()              # raster order over (part, i, j)
    # weights: the map's float32 barycentrics, w2 = 1 - w0 - w1 in double; they sum to 1
    assert t['lm_w'].dtype == np.float64 and np.abs(t['lm_w'].sum(1) - 1.0).max() <= 2.0 ** -52
    assert np.array_equal(t['lm_w'], lt['w'])
    # corners: the face's own order, as positions in the support
    f = face[t['cell'][:, 0] - 1, t['cell'][:, 1], t['cell'][:, 2]]
    assert (f >= 0).all()
    want = at['vert_mapping'].astype(np.int64)[at['faces'].astype(np.int64)[f]]
    assert np.array_equal(t['support'][t['lm_corner']], want) and np.array_equal(t['lm_vert'], want)
    assert (np.diff(t['support']) > 0).all() and t['Sp'] % 128 == 0 and t['S'] <= t['Sp'] < t['S'] + 128
    if NV is not None:
        assert np.unique(want).size == NV
    # the support holds the keypoint fit's own, and lm / jx still name it
    from danet_densepose2smpl_amd.kp_fit import fit_tables
    k = fit_tables(layer)
    assert np.isin(k['support'], t['support']).all() and np.array_equal(t['support'][t['lm']], k['support'][k['lm']])
    assert t['S'] == np.union1d(k['support'], want.reshape(-1)).size
    # the CSR is the inverse: the same [Sp, M] matrix, and ascending landmarks within a vertex
    Sp = t['Sp']
    A = np.zeros((Sp, M))
    np.add.at(A, (t['lm_corner'].reshape(-1), np.repeat(np.arange(M), 3)), t['lm_w'].reshape(-1))
    B = np.zeros((Sp, M))
    off = t['csr_off']
    assert off.shape == (Sp + 1,) and off[0] == 0 and off[-1] == 3 * M and (np.diff(off) >= 0).all()
    for v in range(Sp):
        ls = t['csr_lm'][off[v]:off[v + 1]]
        assert (np.diff(ls) >= 0).all()
        np.add.at(B, (np.full(ls.size, v), ls), t['csr_w'][off[v]:off[v + 1]])
    assert np.array_equal(A, B)


@pytest.mark.parametrize('S', [56, 64])
def test_pixel_convention(S):
    """The observation of a rastered body lands on the landmarks' projections: within the recorded median for the rule's
    convention, x = (col + .5) 2 / S - 1, y = (row + .5) 2 / S - 1, and far from it with y flipped."""
    lt = do.tables(4)
    case = do.dense_recovery_case(S, 4)
    pts, _ = do.landmark_points(torch.as_tensor(case['verts_star']), lt)
    uv = do.project_points(pts.numpy(), case['star'][:, :3])
    med = {}
    for flip in (False, True):
        obs, _, _ = do.extract(case['iuv'], lt, flip_y=flip)
        ok = obs[..., 2] >= 0.5
        assert ok.sum() >= 300
        med[flip] = float(np.median(np.linalg.norm(obs[..., :2] - uv, axis=-1)[ok]) * S / 2.0)
    print('S = %d: median %.3f px, with y flipped %.3f px' % (S, med[False], med[True]))
    assert med[False] <= RECORDED_MEDIAN_PX[S]
    assert med[True] > 10 * RECORDED_MEDIAN_PX[S]


def test_float64_recovery_dense_only():
    """The rule itself, float64, the defaults, dense term only: every row's mean vertex error ends below its start."""
    model = do.synthetic()[0]
    lt = do.tables(4)
    case = do.dense_recovery_case()
    obs, W, margin = do.extract(case['iuv'], lt)
    r = do.fit(ko.model_tensors(model), lt, case['init'], obs)
    unc = do.uncertain_obs(W, margin) | do.uncertain_gate(r['cos'])
    assert unc.mean() <= 0.05                                            # the GPU tests' case stays under the cap
    before = do.mean_vertex_error(model, case['init'], case['verts_star'])
    after = do.mean_vertex_error(model, r['para_fit'], case['verts_star'])
    print('mean vertex error (mm): %s -> %s; E_T / E_0 %s' % (np.round(before * 1e3, 1).tolist(), np.round(after * 1e3, 1).tolist(),
                                                            np.round(r['history'][:, -1] / r['history'][:, 0], 4).tolist()))
    assert (r['status'] == 0).all() and (r['best_iter'] > 0).all()
    assert (after < before).all()
    # no observation, no keypoints: the row itself
    r0 = do.fit(ko.model_tensors(model), lt, case['init'][:1], np.zeros((1, lt['M'], 3)), stages=((2, 'all'),))
    assert np.array_equal(r0['para_fit'], case['init'][:1].astype(np.float64)) and r0['best_iter'][0] == 0


def test_refusals_before_any_launch(layer, smpl_model):
    from danet_densepose2smpl_amd import _lib, dense_fit
    for kw in ({'grid': 1}, {'grid': 7}, {'grid': 2.5}, {'sigma_dense': 0.0}, {'tau': -1.0}, {'w_dense': -0.1}, {'stages': ((3, 'arms'),)}):
        with pytest.raises(ValueError):
            dense_fit.DenseFitter(layer, smpl_model=smpl_model, **kw)
    fitter = dense_fit.DenseFitter(layer, smpl_model=smpl_model)
    assert fitter.tau == 1.0 / 16 and fitter.iterations == 100
    para, img = torch.zeros(2, 229), torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        fitter.fit(para, img)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        fitter.fit(para, obs=torch.zeros(2, 259, 3))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        fitter.landmarks(img)
    with pytest.raises(ValueError, match='exactly one'):
        fitter.fit(para)
    with pytest.raises(ValueError, match='exactly one'):
        fitter.fit(para, img, obs=torch.zeros(2, 259, 3))
    with pytest.raises(ValueError, match='unknown parameter group'):
        fitter.fit(para, img, stages=((1, 'legs'),))
    with pytest.raises(ValueError):
        dense_fit.dense_tables(layer, do.synthetic()[1], np.full((24, 8, 8), -1), np.zeros((24, 8, 8, 2)))
    # the entry points check their arguments before they launch
    L = _lib.lib()
    fake = ctypes.c_void_p(64)
    for args, word in (((fake, fake, 1, 10, 8, 7, 0.1, 1e-3, fake, None, None), 'G=7'), ((fake, fake, 1, 0, 8, 4, 0.1, 1e-3, fake, None, None), 'M=0'),
                       ((fake, fake, 1, 10, 8, 4, 0.0, 1e-3, fake, None, None), 'tau'), ((fake, None, 1, 10, 8, 4, 0.1, 1e-3, fake, None, None), 'null')):
        assert L.danet_dense_landmarks(*args) != 0 and word in L.danet_last_error().decode()
    a = _lib.DenseFitArgs()
    for k, _ in a._fields_[:25]:
        setattr(a, k, 64)
    a.P, a.NB, a.S, a.Sp, a.NL, a.NE, a.nstages, a.T, a.M = 1, 10, 100, 128, 21, 9, 0, 0, 259
    a.focal, a.res, a.kappa, a.sigma, a.sigma_dense, a.w_dense, a.min_cos = 5000., 224., 44.6, 0.1, 0.05, 0.25, 0.1
    nws = L.danet_dense_fit_ws_floats(1, 128)
    assert nws == 128 * 6 and L.danet_dense_fit_ws_floats(0, 128) == 0
    for field, value, word in (('M', 0, 'M=0'), ('M', 865, 'M=865'), ('sigma_dense', 0.0, 'sigma_dense'), ('obs', None, 'obs'), ('gate', None, 'gate'),
                               ('lm_corner', None, 'landmark tables'), ('Sp', 100, 'Sp=100'), ('T', 3, 'T=3')):
        old = getattr(a, field)
        setattr(a, field, value)
        assert L.danet_dense_fit(ctypes.addressof(a), nws, None) != 0 and word in L.danet_last_error().decode(), field
        setattr(a, field, old)
    assert L.danet_dense_fit(ctypes.addressof(a), nws - 1, None) != 0 and 'workspace' in L.danet_last_error().decode()
