"""Host side of the scene demo (scene.py, ops.scene_render's refusals, the ABI) and the CPU-only premises of tests/test_gpu_scene.py:
the share of pixels the oracle calls uncertain on that file's scenes, and its colour margin DELTA."""
import numpy as np
import pytest
import torch

import scene_oracle as so

from scene_oracle import DELTA


def test_colour_margin_is_four_times_the_float32_oracle_error():
    people, frames = so.main_scene()
    d = so.colour_delta(people, frames)
    print('4 x max |level32 - level64| = %.6e (DELTA %.3e)' % (d, DELTA), flush=True)
    assert 0.5 * DELTA < d <= DELTA
    for kind in so.SKIP_KINDS:
        p, f, _ = so.skip_scene(kind)
        assert so.colour_delta(p, f) <= DELTA


def test_uncertain_share_of_the_gpu_scenes_is_at_most_5_percent():
    scenes = [so.main_scene()] + [so.skip_scene(k)[:2] for k in so.SKIP_KINDS]
    for people, frames in scenes:
        cov = unc = 0
        for r in so.run(people, frames):
            c = r['ids'] >= 0
            cov += int(c.sum())
            unc += int((so.uncertain(r) & c).sum())
        print('covered %d, uncertain %d' % (cov, unc), flush=True)
        assert cov > 150 and unc <= 0.05 * cov


def test_main_scene_is_what_its_docstring_says():
    people, frames = so.main_scene()
    assert [f.shape for f in frames] == [(37, 53, 3), (64, 40, 3), (16, 16, 3)]
    col, row, z = so.project(people['verts'], people['cam_t'], people['proj'])
    assert max(np.abs(col).max(), np.abs(row).max()) < 256 and z.min() > 0.1            # the +-256 pixels of the coordinate bound
    r = so.run(people, frames)
    F2 = people['faces2'].shape[0]
    a, b, c = (so.run(people, frames, keep=[k])[0]['ids'] >= 0 for k in range(3))
    who = r[0]['ids'] // F2
    both = a & b
    assert (both & (who == 0)).sum() >= 10 and (both & (who == 1)).sum() >= 10          # interleaved depths: each wins part of the overlap
    assert c[0, 0] and c[:, 0].any() and c[0, :].any()                                  # the third hangs over the top-left corner
    assert ((a | b) & c & (who == 2)).sum() >= 5                                        # and occludes, being nearer
    assert (r[1]['ids'] // F2 == 3).sum() > 100 and (r[2]['ids'] == -1).all()
    assert np.array_equal(r[2]['out'], frames[2])
    for k in range(3):
        assert np.array_equal(r[k]['out'][r[k]['ids'] < 0], frames[k][r[k]['ids'] < 0])
    assert np.isfinite(r[0]['depth'][r[0]['ids'] >= 0]).all() and np.isinf(r[0]['depth'][r[0]['ids'] < 0]).all()


def test_skip_scenes_remove_something_that_would_have_been_drawn():
    for kind in so.SKIP_KINDS:
        people, frames, dead = so.skip_scene(kind)
        ids = so.run(people, frames)[0]['ids']
        assert not dead(ids).any() and (ids >= 0).sum() > 150
    # the unspoilt people of 'behind' / 'nan' do show the faces those cases kill, and the person of 'outside' is seen inside
    clean, frames, _ = so.skip_scene('zero_area')
    clean['faces2'] = clean['faces2'][:40]
    ids = so.run(clean, frames)[0]['ids']
    for kind in ('behind', 'nan', 'outside'):
        assert so.skip_scene(kind)[2](ids).sum() >= 10


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def _raster_rule_crop_index(X, cam, res, focal):
    """The raster rule's NDC (csrc/iuv_raster.hip, orig = S = res) of points X [n,3] for cam (s, tx, ty), read as pixel indices: a
    pixel centre c has NDC (2 c + 1 - S) / S across and (S - 1 - 2 r) / S down.  float64."""
    s, tx, ty = cam
    fx, cx = focal, res / 2.0
    if res != 224.0:
        fx, cx = fx * (res / 224.0), cx * (res / 224.0)
    half = res / 2.0
    tz = 2.0 * focal / (res * s + 1e-9)
    x, y = (X[:, 0] + tx) / (X[:, 2] + tz), (X[:, 1] + ty) / (X[:, 2] + tz)
    u, v = fx * x + cx, res - (fx * y + cx)
    u, v = 2.0 * (u - half) / res, 2.0 * (v - half) / res
    return (u * res + res - 1.0) / 2.0, (res - 1.0 - v * res) / 2.0


@pytest.mark.parametrize('res', [224, 256])
def test_person_cameras_compose_the_raster_rule_with_the_inverse_crop_transform(res):
    from danet_densepose2smpl_amd import augment, scene
    H, W = 480, 640
    # boxes hanging over the left, top, right and bottom border, one inside, one larger than the frame
    center = np.array([[10., 200.], [300., -20.], [630., 250.], [320., 470.], [300., 240.], [320., 240.]])
    scale = np.array([0.9, 1.1, 0.8, 1.3, 0.6, 4.0])
    P = center.shape[0]
    rng = np.random.default_rng(5)
    cam = np.stack([rng.uniform(0.5, 1.2, P), rng.uniform(-.2, .2, P), rng.uniform(-.2, .2, P)], 1)
    t = augment.get_transform(torch.from_numpy(center), torch.from_numpy(scale), [res, res], 0.).numpy()
    tinv = np.linalg.inv(t)
    shapes = np.array([[H, W], [333, 777]])
    pf = np.array([0, 0, 0, 1, 1, 1])
    k = scene.person_cameras(cam, tinv, shapes, pf, res)
    X = rng.normal(0, 0.5, (50, 3))
    X[0] = 0.0                                                                           # the pelvis
    for p in range(P):
        if res == 224:
            u, v = _raster_rule_crop_index(X, cam[p], float(res), 5000.)
        else:
            # (away from 224 the raster rule also scales its principal point, the reference's K[0,2] * orig / 224; the scene
            # cameras keep it at the crop's centre, as DESIGN.md says and as ops.coco_keypoints does)
            tz_ = 2.0 * 5000. / (res * cam[p, 0] + 1e-9)
            fx_ = 5000. * res / 224.
            u = fx_ * (X[:, 0] + cam[p, 1]) / (X[:, 2] + tz_) + res / 2. - 0.5
            v = fx_ * (X[:, 1] + cam[p, 2]) / (X[:, 2] + tz_) + res / 2. - 0.5
        want = tinv[p] @ np.stack([u, v, np.ones_like(u)])                               # crop index -> frame index
        tx, ty, tz = k['cam_t'][p]
        assert tz == 2.0 * 5000. / (res * cam[p, 0] + 1e-9) and (tx, ty) == (cam[p, 1], cam[p, 2])
        xn, yn = (X[:, 0] + tx) / (X[:, 2] + tz), (X[:, 1] + ty) / (X[:, 2] + tz)
        q = k['proj'][p]
        col, row = q[0] * xn + q[1] * yn + q[2], q[3] * xn + q[4] * yn + q[5]
        assert np.abs(col - want[0]).max() < 1e-9 and np.abs(row - want[1]).max() < 1e-9
        # one camera for the whole frame: focal F0, principal point the frame's centre, translation cam_t_full
        Hn, Wn = shapes[pf[p]]
        F0 = k['focal_full'][p]
        assert F0 == np.sqrt(float(Hn) ** 2 + float(Wn) ** 2)
        Fp = 5000. * res / 224. * 200. * scale[p] / res
        assert abs(k['dscale'][p] - F0 / Fp) < 1e-12 * F0 / Fp
        fx_, fy_, fz_ = k['cam_t_full'][p]
        assert abs(fz_ - tz * k['dscale'][p]) < 1e-12 * fz_
        assert abs(F0 * fx_ / fz_ + (Wn - 1) / 2.0 - col[0]) < 1e-9 and abs(F0 * fy_ / fz_ + (Hn - 1) / 2.0 - row[0]) < 1e-9
    k2 = scene.person_cameras(cam, tinv, shapes, pf, res, focal_full=1000.)
    assert (k2['focal_full'] == 1000.).all() and np.array_equal(k2['proj'], k['proj'])
    assert np.allclose(k2['dscale'] / k['dscale'], 1000. / k['focal_full'], rtol=1e-14)


def test_box_helpers_hand_worked():
    from danet_densepose2smpl_amd import scene
    c, s = scene.boxes_from_xywh([10., 20., 100., 50.])
    assert c.tolist() == [60., 45.] and s == 1.2 * 100. / 200.
    c, s = scene.boxes_from_xywh([[0., 0., 30., 60.], [5., 5., 10., 10.]], rescale=1.0)
    assert c.tolist() == [[15., 30.], [10., 10.]] and s.tolist() == [0.3, 0.05]
    kps = np.array([[100., 50., 0.9], [140., 250., 0.5], [0., 0., 0.1], [120., 100., 0.21], [999., 999., 0.2]])
    c, s = scene.boxes_from_keypoints(kps)                                               # the third and the last are not above 0.2
    assert c.tolist() == [120., 150.] and s == 1.2 * 200. / 200.
    c, s = scene.boxes_from_keypoints(kps, thresh=0.6, rescale=2.0)
    assert c.tolist() == [100., 50.] and s == 0.0
    with pytest.raises(ValueError):
        scene.boxes_from_keypoints(kps, thresh=0.95)
    c, s = scene.whole_image_box((1080, 1920, 3))
    assert c.tolist() == [959.5, 539.5] and s == 9.6


def test_pack_frames_round_trip_and_layout():
    from danet_densepose2smpl_amd import scene
    frames = so.make_frames(3)
    src, off, shp = scene.pack_frames(frames)
    assert off.tolist() == [0, 37 * 53 * 3, 37 * 53 * 3 + 64 * 40 * 3, 37 * 53 * 3 + 64 * 40 * 3 + 16 * 16 * 3] and off[1] % 4 != 0
    assert shp.tolist() == [[37, 53], [64, 40], [16, 16]] and src.size == off[-1] + 16 and src.dtype == np.uint8
    back = scene.unpack_frames(src, off, shp)
    assert all(np.array_equal(a, b) for a, b in zip(back, frames))
    with pytest.raises(ValueError):
        scene.pack_frames([np.zeros((4, 4, 3), np.float32)])


def test_write_obj_round_trip(tmp_path):
    from danet_densepose2smpl_amd import scene
    rng = np.random.default_rng(0)
    v = rng.normal(size=(12, 3)).astype(np.float32)
    _, f = so.icosahedron()
    path = str(tmp_path / 'p.obj')
    scene.write_obj(path, v, f)
    lines = open(path).read().split('\n')
    assert lines[-1] == '' and len(lines) == 12 + 20 + 1
    vs = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith('v ')], np.float64).astype(np.float32)
    fs = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith('f ')])
    assert np.array_equal(vs, v) and np.array_equal(fs, f + 1)                           # bit for bit; 1-based


def test_scene_render_refuses_cpu_tensors():
    from danet_densepose2smpl_amd import ops, scene
    people, frames = so.main_scene()
    src, off, shp = scene.pack_frames(frames)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                              # noqa: E731
    with pytest.raises(RuntimeError, match='GPU only.*no CPU path'):
        ops.scene_render(t(people['verts']), t(people['vcol']), t(people['faces2']), t(people['cam_t']), t(people['proj']), t(people['dscale']),
                         t(people['person_frame']), t(src), t(off), t(shp))


def test_scene_symbols_declared_bound_and_exported():
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    for name in ('danet_scene_render', 'danet_scene_render_ws_bytes'):
        assert name in _lib.exported_symbols() and hasattr(L, name)
    assert L.danet_scene_render_ws_bytes(2, 12, 100) == 2 * 12 * 3 * 4 + 100 * 8
    assert L.danet_scene_render_ws_bytes(1, 1, 0) == 16                                  # (12 bytes rounded up to the 8-byte buffer)


# ------------------------------------------------------------------------------------------------------------------ the demo stages' host side
def test_box_row_and_row_box_bit_for_bit():
    from danet_densepose2smpl_amd import scene
    c, s = (10.25, 7.5), 0.8
    row = scene.box_row((np.array(c), s, 0.9))                            # a confidence behind the scale is not looked at
    want = np.zeros(3, np.float32)
    want[:] = (np.float64(c[0]), np.float64(c[1]), np.log(float(s)))
    assert row.dtype == np.float32 and row.shape == (3,) and row.tobytes() == want.tobytes()
    assert scene.box_row(([[10.25], [7.5]], np.float32(0.8))).tobytes() == np.array([10.25, 7.5, np.log(float(np.float32(0.8)))], np.float32).tobytes()
    center, scale = scene.row_box(row)
    assert center.dtype == np.float64 and center.tobytes() == np.array(c, np.float64).tobytes()
    assert type(scale) is float and scale == float(np.exp(np.float64(np.float32(np.log(0.8))))) and scale != 0.8


def test_fit_record_reads_the_loss_at_the_start_and_at_the_best_iterate():
    from danet_densepose2smpl_amd import scene
    h = np.array([[5.0, 4.0, 3.0], [6.0, 2.0, 1.5], [7.0, 0.5, 0.75]], np.float32)                # P = 3, T = 2
    init = torch.arange(3 * 229, dtype=torch.float32).view(3, 229)
    info = {'history': torch.from_numpy(h), 'best_iter': torch.tensor([0, 2, 1], dtype=torch.int32), 'status': torch.zeros(3, dtype=torch.int32)}
    got_init, loss, it = scene.fit_record((init, info), 3)
    assert np.array_equal(got_init, init.numpy()) and it.dtype == np.int32 and it.tolist() == [0, 2, 1]
    assert loss.dtype == np.float32 and loss.tolist() == [[5.0, 5.0], [6.0, 1.5], [7.0, 0.5]]
    got_init, loss, it = scene.fit_record((torch.zeros(0, 229), None), 0)
    assert got_init.shape == (0, 229) and (loss.shape, loss.dtype) == ((0, 2), np.float32) and (it.shape, it.dtype) == ((0,), np.int32)
    assert scene.fit_columns(None, 3) == {}
    cols = scene.fit_columns((init, info), 3)
    assert list(cols) == ['para_init', 'fit_loss', 'fit_iter'] and cols['fit_loss'].tolist() == loss_of(h, [0, 2, 1])


def loss_of(h, it):
    return [[float(h[p, 0]), float(h[p, i])] for p, i in enumerate(it)]


def bare_demo(res=224, focal=5000., focal_full=None):
    """A SceneDemo without a model: what the host-side stages read."""
    from danet_densepose2smpl_amd import scene
    demo = object.__new__(scene.SceneDemo)
    demo.res, demo.focal, demo.focal_full, demo.fitter = res, focal, focal_full, None
    return demo


def test_people_builder_against_literal_dicts():
    from danet_densepose2smpl_amd import datasets, scene
    demo = bare_demo()
    center, scale, pf = np.array([[40., 50.], [60., 30.], [25., 35.]]), np.array([0.4, 0.3, 0.5]), np.array([0, 0, 1], np.int32)
    shapes = np.array([[96, 80], [64, 48]], np.int32)
    _, tinv = datasets.crop_transforms(center, scale, np.zeros(3), 224)
    plan = {'P': 3, 'N': 2, 'person_frame': pf, 'tinv': tinv, 'shapes': shapes, 'center': center, 'scale': scale}
    para = np.random.default_rng(0).normal(size=(3, 229)).astype(np.float32)
    para[:, 0] = (0.9, 0.8, 1.1)
    verts = np.arange(3 * 4 * 3, dtype=np.float32).reshape(3, 4, 3)
    cams = scene.person_cameras(para[:, 0:3], tinv, shapes, pf, 224, 5000., None)
    want = [{'para': para[:2], 'cam': para[:2, :3], 'cam_t_full': cams['cam_t_full'][:2], 'focal_full': cams['focal_full'][:2],
             'center': center[:2], 'scale': scale[:2], 'vertices': verts[:2]},
            {'para': para[2:], 'cam': para[2:, :3], 'cam_t_full': cams['cam_t_full'][2:], 'focal_full': cams['focal_full'][2:],
             'center': center[2:], 'scale': scale[2:], 'vertices': verts[2:]}]
    extra = {'track_id': np.array([4, 1, 4], np.int32), 'observed': np.array([True, False, True]), 'para_raw': para + 1, 'identity': np.array([0, 1, 0], np.int32),
             'prefix_end': np.array([5, 5, 6], np.int32)}
    want_extra = [dict(w, **{k: v[m] for k, v in extra.items()}) for w, m in zip(want, (slice(0, 2), slice(2, 3)))]
    assert want_extra[0]['track_id'].tolist() == [4, 1] and want_extra[1]['observed'].tolist() == [True] and want_extra[1]['para_raw'].shape == (1, 229)
    for columns, expected in (({}, want), (extra, want_extra)):
        one = demo.people(para, verts, plan, **columns)
        assert one['para'] is para and one['vertices'] is verts and one['cam'].shape == (3, 3) and one['focal_full'].shape == (3,)
        got = scene.split_people(one, plan)
        assert len(got) == 2
        for g, w in zip(got, expected):
            assert sorted(g) == sorted(w)
            for k in w:
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and g[k].tobytes() == np.ascontiguousarray(w[k]).tobytes(), k
    # no people at all: the empty columns, with their dtypes, in every frame
    empty = {'P': 0, 'N': 2, 'person_frame': np.zeros(0, np.int32), 'shapes': shapes, 'center': np.zeros((0, 2)), 'scale': np.zeros(0)}
    cols = {'track_id': np.zeros(0, np.int32), 'observed': np.zeros(0, bool), 'para_raw': np.zeros((0, 229), np.float32)}
    got = scene.split_people(demo.people(np.zeros((0, 229), np.float32), np.zeros((0, 0, 3), np.float32), empty, **cols), empty)
    want0 = {'para': ((0, 229), np.float32), 'cam': ((0, 3), np.float32), 'cam_t_full': ((0, 3), np.float64), 'focal_full': ((0,), np.float64),
             'center': ((0, 2), np.float64), 'scale': ((0,), np.float64), 'vertices': ((0, 0, 3), np.float32), 'track_id': ((0,), np.int32),
             'observed': ((0,), np.bool_), 'para_raw': ((0, 229), np.float32)}
    assert len(got) == 2
    for g in got:
        assert {k: (v.shape, v.dtype.type) for k, v in g.items()} == want0


def test_infer_and_fit_stages_decide_on_the_host():
    """P = 0 and 'nothing to fit to' never reach the network or the fitter."""
    from danet_densepose2smpl_amd import scene
    demo = bare_demo()
    demo.device = torch.device('cpu')
    para, iuv = demo.infer_stage({'P': 0})
    assert para.shape == (0, 229) and para.dtype == torch.float32 and iuv is None
    rows = torch.zeros(2, 229)
    assert demo.fit_stage(rows, {'P': 2}, [[np.zeros((49, 3))] * 2], None) == (None, rows)             # no fitter
    demo.fitter = object()                                                                           # a keypoint fitter without keypoints
    fitted, out = demo.fit_stage(rows, {'P': 2}, None, None)
    assert fitted is None and out is rows
    fitted, out = demo.fit_stage(rows[:0], {'P': 0}, [[]], None)                                      # a fit of nobody: the record of one
    assert fitted[0].shape == (0, 229) and fitted[1] is None and out.shape == (0, 229)
