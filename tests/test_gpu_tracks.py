"""The track ops (csrc/track_ops.hip, tracks.py) and the video demo (video.py) on the device, against the float64 restatement of the
track rule in tests/track_oracle.py.

Bounds.  A block is one track's rows of one lam group.  smooth, cam and betas: |kernel - f64| <= 8 x 2^-23 x max |f64| of the block
plus four times the oracle's own two-solver difference on the block (dense numpy.linalg.solve against its banded L D L^T;
tests/test_tracks_host.py bounds that difference on exactly these cases).  Rotation blocks: four times the float32 oracle's error
(the float64 solution rounded to fp32, then Gram-Schmidt in float32, against Gram-Schmidt in float64) plus 8 roundings of 1, the
bound of the fit rule.  accel: 1e-6 relative.  Every test prints the ratio measured / bound before it asserts and hands it to
conftest.record.

Shapes: T in {1 .. 6, 257} covers every size at which the stencils lose a term and one long chain; C in {1, 63, 64, 65, 157} sits on
both sides of a wave of 64 lanes and is the para form's width."""
import json
import os

import numpy as np
import pytest
import torch

import track_oracle as to
from conftest import record
from track_oracle import CONF_KINDS, FIVE, LAMS, LENGTHS, WIDTHS

pytestmark = pytest.mark.gpu

U = 2.0 ** -23


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _record(name, ratio, **kw):
    print('%s: measured / bound = %.4f %s' % (name, ratio, kw), flush=True)
    record('tracks.' + name, dict(kw, ratio=round(float(ratio), 6)))


def make_case(lengths, C, kind, seed, nan_gaps=True):
    """track_oracle.make_case with the TrackSet: -> (values [N,C] f32, TrackSet)."""
    from danet_densepose2smpl_amd import tracks
    v, conf, start = to.make_case(lengths, C, kind, seed, nan_gaps)
    frame = np.concatenate([np.arange(T) for T in lengths])
    return v, tracks.TrackSet(start, frame, np.where(conf > 0, 0, -1), conf, max(lengths))


def check_smooth(v, ts, lam, name):
    from danet_densepose2smpl_amd import tracks
    out, status = tracks.smooth(_cu(v), ts, lam[0], lam[1])
    torch.cuda.synchronize()
    got, st = out.cpu().numpy(), status.cpu().numpy()
    ref, st_ref = to.smooth(v, ts.conf, ts.track_start, lam[0], lam[1])
    gap = to.solver_gap(v, ts.conf, ts.track_start, lam[0], lam[1])
    assert got.dtype == np.float32 and np.array_equal(st, st_ref)
    worst = 0.0
    for k in range(ts.K):
        s, e = ts.track_start[k], ts.track_start[k + 1]
        if st_ref[k]:
            assert np.array_equal(got[s:e].view(np.int32), v[s:e].view(np.int32)), (name, k)         # bit for bit
            continue
        assert np.isfinite(got[s:e]).all(), (name, k)
        bound = 8 * U * np.abs(ref[s:e]).max() + 4 * gap[k]
        worst = max(worst, np.abs(got[s:e] - ref[s:e]).max() / bound)
    return worst


# ------------------------------------------------------------------------------------------------------------------ smooth
@pytest.mark.parametrize('lam', LAMS)
@pytest.mark.parametrize('C', WIDTHS)
def test_smooth_against_the_oracle(C, lam):
    worst = 0.0
    for i, kind in enumerate(CONF_KINDS):
        v, ts = make_case(LENGTHS, C, kind, to.case_seed(C, i))
        worst = max(worst, check_smooth(v, ts, lam, kind))
    _record('smooth', worst, C=C, lam=list(lam))
    assert worst <= 1.0


@pytest.mark.parametrize('lam', LAMS)
def test_smooth_five_tracks_in_one_launch(lam):
    """K = 5 tracks of lengths (1, 2, 5, 64, 257), each with its own conf pattern, the fourth without any weight."""
    from danet_densepose2smpl_amd import tracks
    lengths = [T for T, _ in FIVE]
    parts = [make_case((T,), 65, kind, 7 + i) for i, (T, kind) in enumerate(FIVE)]
    v = np.concatenate([p[0] for p in parts])
    conf = np.concatenate([p[1].conf for p in parts])
    start = np.concatenate([[0], np.cumsum(lengths)])
    ts = tracks.TrackSet(start, np.concatenate([np.arange(T) for T in lengths]), np.where(conf > 0, 0, -1), conf, 257)
    worst = check_smooth(v, ts, lam, 'five')
    _record('smooth_five_tracks', worst, lam=list(lam))
    assert worst <= 1.0
    out, status = tracks.smooth(_cu(v), ts, *lam)
    assert status.cpu().tolist() == [0, 0, 0, 1, 0]
    # each track alone: the same bits
    for k, (vk, tk) in enumerate(parts):
        alone, _ = tracks.smooth(_cu(vk), tk, *lam)
        assert np.array_equal(alone.cpu().numpy().view(np.int32), out[start[k]:start[k + 1]].cpu().numpy().view(np.int32)), k
    again, _ = tracks.smooth(_cu(v), ts, *lam)
    assert np.array_equal(again.cpu().numpy().view(np.int32), out.cpu().numpy().view(np.int32))


def test_smooth_nan_in_an_observed_row_spoils_that_track_and_channel_only():
    from danet_densepose2smpl_amd import tracks
    v, ts = make_case((5, 64, 6), 65, 'mid', 3)
    clean, _ = tracks.smooth(_cu(v), ts, 0.5, 100.0)
    bad = v.copy()
    row = int(ts.track_start[1]) + 2
    assert ts.conf[row] > 0
    bad[row, 17] = np.nan
    got, status = tracks.smooth(_cu(bad), ts, 0.5, 100.0)
    got, clean = got.cpu().numpy(), clean.cpu().numpy()
    assert status.cpu().tolist() == [0, 0, 0]
    s, e = ts.track_start[1], ts.track_start[2]
    assert not np.isfinite(got[s:e, 17]).any()
    got[s:e, 17] = clean[s:e, 17]
    assert np.isfinite(got).all() and np.array_equal(got.view(np.int32), clean.view(np.int32))


def test_refusals_launch_nothing():
    from danet_densepose2smpl_amd import tracks
    v, ts = make_case((5, 6), 3, 'ones', 1, nan_gaps=False)
    x = _cu(v)
    for bad in ((1, 5, 11), (0, 5, 10), (0, 7, 6, 11)):
        t2 = tracks.TrackSet(ts.track_start, ts.frame, ts.det, ts.conf, ts.n_frames)
        t2.track_start = np.array(bad, np.int32)
        with pytest.raises(ValueError):
            tracks.smooth(x, t2)
    t2 = tracks.TrackSet(ts.track_start, ts.frame, ts.det, ts.conf, ts.n_frames)
    t2.conf = ts.conf.copy()
    t2.conf[3] = -0.5
    with pytest.raises(ValueError):
        tracks.smooth(x, t2)
    t2.conf[3] = np.inf
    with pytest.raises(ValueError):
        tracks.smooth_para(torch.zeros(11, 229, device='cuda'), t2)
    with pytest.raises(ValueError):
        tracks.smooth(x, ts, -1.0, 0.0)
    with pytest.raises(ValueError):
        tracks.smooth(x, ts, 0.0, float('nan'))
    with pytest.raises(ValueError):
        tracks.smooth(x[:, 0], ts)
    with pytest.raises(ValueError):
        tracks.smooth_para(x, ts)
    with pytest.raises(ValueError):
        tracks.accel(x, ts)
    with pytest.raises(ValueError):
        tracks.smooth(x.to(torch.int32), ts)
    # N = 0: empty results, no launch
    empty = tracks.TrackSet([0], [], [], [], 0)
    out, status = tracks.smooth(torch.zeros(0, 4, device='cuda'), empty)
    assert out.shape == (0, 4) and status.shape == (0,)
    out, status = tracks.smooth_para(torch.zeros(0, 229, device='cuda'), empty)
    assert out.shape == (0, 229) and status.shape == (0,)
    a, n = tracks.accel(torch.zeros(0, 24, 3, device='cuda'), empty)
    assert a.shape == (0,) and n.shape == (0,)
    # the entry point itself: a workspace that is too small, a bad host track_start
    from danet_densepose2smpl_amd import _lib
    from danet_densepose2smpl_amd._lib import ptr, stream
    from danet_densepose2smpl_amd.ops import _host_i32
    L = _lib.lib()
    d_start, d_conf = ts.device(x.device)
    out = torch.full_like(x, 7.0)
    status = torch.full((2,), 7, dtype=torch.int32, device='cuda')
    ws = torch.empty(4096, dtype=torch.int64, device='cuda')
    rc = L.danet_track_smooth(ptr(x), ptr(d_conf), ptr(d_start), _host_i32(ts.track_start), 11, 3, 2, 0.0, 10.0, ptr(out), ptr(status), ptr(ws), 8, stream())
    assert rc == -3
    rc = L.danet_track_smooth(ptr(x), ptr(d_conf), ptr(d_start), _host_i32(np.array([0, 5, 12], np.int32)), 11, 3, 2, 0.0, 10.0, ptr(out), ptr(status),
                              ptr(ws), 4096 * 8, stream())
    assert rc == -1 and b'track_start' in L.danet_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((status == 7).all())


def test_device_tables_are_uploaded_once_per_device(monkeypatch):
    """'cuda' and 'cuda:<current>' are one cache entry for a TrackSet, a PairSet and a RowGroups: the same tensors, and after the
    first call nothing is uploaded."""
    from danet_densepose2smpl_amd import tracks
    ts = tracks.TrackSet([0, 1, 3], [0, 0, 1], [0, 0, 0], [1, 1, 0.5], 2)
    holders = (ts, tracks.PairSet([[0, 1]], 2), tracks.RowGroups([0, 3], [2, 0, 1]))
    named = torch.device('cuda', torch.cuda.current_device())
    first = [h.device(torch.device('cuda')) for h in holders]
    torch.cuda.synchronize()
    assert torch.equal(first[0][0].cpu(), torch.tensor([0, 1, 3], dtype=torch.int32)) and first[0][1].cpu().tolist() == [1, 1, 0.5]
    assert first[1].cpu().tolist() == [[0, 1]] and first[2][0].cpu().tolist() == [0, 3] and first[2][1].cpu().tolist() == [2, 0, 1]

    def no_upload(*a, **kw):
        raise AssertionError('a second upload')
    monkeypatch.setattr(torch, 'from_numpy', no_upload)
    for h, f in zip(holders, first):
        for dev in (named, torch.device('cuda'), named):
            again = h.device(dev)
            assert len(h._dev) == 1
            for x, y in zip(f if isinstance(f, tuple) else (f,), again if isinstance(again, tuple) else (again,)):
                assert x is y and x.data_ptr() == y.data_ptr() and x.device == named


# ------------------------------------------------------------------------------------------------------------------ smooth_para
def para_case():
    from danet_densepose2smpl_amd import tracks
    para, conf, start, rc = to.para_case()
    frame = np.concatenate([np.arange(b - a) for a, b in zip(start[:-1], start[1:])])
    return para, tracks.TrackSet(start, frame, np.where(conf > 0, 0, -1), conf, int(frame.max()) + 1), rc


@pytest.fixture(scope='module')
def para_refs():
    para, ts, rc = para_case()
    refs = {}
    for shared in (True, False):
        b = to.smooth_para(para, ts.conf, ts.track_start, to.DEFAULT_LAM, shared)
        d = to.smooth_para(para, ts.conf, ts.track_start, to.DEFAULT_LAM, shared, solver=to.solve_dense)
        refs[shared] = (b, np.abs(b['ch'] - d['ch']))
    return para, ts, rc, refs


def check_para(got, para, ts, ref, gap, name, shared):
    worst = {'cam': 0.0, 'betas': 0.0, 'rot': 0.0}
    for k in range(ts.K):
        s, e = ts.track_start[k], ts.track_start[k + 1]
        if ref['status'][k]:
            assert np.array_equal(got[s:e].view(np.int32), para[s:e].view(np.int32)), (name, k)
            continue
        assert np.isfinite(got[s:e]).all(), (name, k)                                      # gap rows are filled
        for g, sl in (('cam', slice(0, 3)), ('betas', slice(3, 13))):
            bound = 8 * U * np.abs(ref['para64'][s:e, sl]).max() + 4 * gap[s:e, sl].max()
            worst[g] = max(worst[g], np.abs(got[s:e, sl] - ref['para64'][s:e, sl]).max() / bound)
        err32 = np.abs(ref['para32'][s:e, 13:].astype(np.float64) - ref['para64'][s:e, 13:]).max()
        worst['rot'] = max(worst['rot'], np.abs(got[s:e, 13:] - ref['para64'][s:e, 13:]).max() / (4 * err32 + 8 * U))
        obs = ts.conf[s:e] > 0
        assert para[s:e, 0][obs].min() <= got[s:e, 0].min() and got[s:e, 0].max() <= para[s:e, 0][obs].max()
        if shared:
            assert (got[s:e, 3:13] == got[s, 3:13]).all()
        R = got[s:e, 13:].reshape(-1, 3, 3).astype(np.float64)
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-5 and np.abs(np.linalg.det(R) - 1).max() < 1e-5
    for g, w in worst.items():
        _record('smooth_para', w, block=g, shared_shape=shared, case=name)
    return worst


@pytest.mark.parametrize('shared', (True, False))
def test_smooth_para_against_the_oracle(para_refs, shared):
    from danet_densepose2smpl_amd import tracks
    para, ts, _, refs = para_refs
    out, status = tracks.smooth_para(_cu(para), ts, shared_shape=shared)
    torch.cuda.synchronize()
    ref, gap = refs[shared]
    assert np.array_equal(status.cpu().numpy(), ref['status']) and ref['status'].tolist() == [0, 0, 0, 0, 0, 1]
    worst = check_para(out.cpu().numpy(), para, ts, ref, gap, 'para', shared)
    assert max(worst.values()) <= 1.0


def test_recovery_case_on_the_device(para_refs):
    """The device's rows are within the parity bound of the oracle's (above), and show the oracle's strict improvement on every
    track: joint error against ground truth and acceleration error, measured with the oracle's toy joints in float64."""
    from danet_densepose2smpl_amd import tracks
    para, ts, rc, _ = para_refs
    n, st = rc['gt'].shape[0], rc['track_start']
    out, _ = tracks.smooth_para(_cu(para), ts)
    got = out.cpu().numpy()[:n].astype(np.float64)
    e0, e1 = to.joint_error(rc['obs_full'], rc['gt'], st), to.joint_error(got, rc['gt'], st)
    jg = to.toy_joints(rc['gt'])
    a0, _ = to.accel(to.toy_joints(rc['obs_full']), st, jg)
    a1, _ = to.accel(to.toy_joints(got), st, jg)
    print('recovery on the device: joint error ratio %s, acceleration error ratio %s' % ((e1 / e0).round(4).tolist(), (a1 / a0).round(4).tolist()), flush=True)
    assert (e1 < e0).all() and (a1 < a0).all()
    # the device's own measure on the same joints
    a_dev, cnt = tracks.accel(_cu(to.toy_joints(got).astype(np.float32)), tracks.TrackSet(st, ts.frame[:n], ts.det[:n], ts.conf[:n], ts.n_frames),
                              _cu(jg.astype(np.float32)))
    # (the joints went to the device as fp32: a rounding of 6e-8 of coordinates near 1 against accelerations of 1e-3 and more)
    assert np.allclose(a_dev.cpu().numpy(), a1, rtol=1e-3) and cnt.cpu().tolist() == [(b - a - 2) * 24 for a, b in zip(st[:-1], st[1:])]


def test_smooth_para_bits_alone_twice_and_under_graph_replay(para_refs):
    from danet_densepose2smpl_amd import tracks
    para, ts, _, _ = para_refs
    x = _cu(para)
    eager, st = tracks.smooth_para(x, ts)
    again, _ = tracks.smooth_para(x, ts)
    assert np.array_equal(eager.cpu().numpy().view(np.int32), again.cpu().numpy().view(np.int32))
    for k in range(ts.K):
        s, e = int(ts.track_start[k]), int(ts.track_start[k + 1])
        tk = tracks.TrackSet([0, e - s], ts.frame[s:e], ts.det[s:e], ts.conf[s:e], ts.n_frames)
        alone, _ = tracks.smooth_para(x[s:e], tk)
        assert np.array_equal(alone.cpu().numpy().view(np.int32), eager[s:e].cpu().numpy().view(np.int32)), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            tracks.smooth_para(x, ts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static, static_st = tracks.smooth_para(x, ts)
    for _ in range(2):
        static.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(static.cpu().numpy().view(np.int32), eager.cpu().numpy().view(np.int32))
        assert torch.equal(static_st, st)
    del g


# ------------------------------------------------------------------------------------------------------------------ accel
@pytest.mark.parametrize('with_ref', (False, True))
def test_accel_against_the_oracle(with_ref):
    from danet_densepose2smpl_amd import tracks
    rng = np.random.default_rng(11)
    lengths = (1, 2, 3, 65)
    start = np.concatenate([[0], np.cumsum(lengths)])
    N = int(start[-1])
    ts = tracks.TrackSet(start, np.concatenate([np.arange(T) for T in lengths]), np.zeros(N), np.ones(N), 65)
    for J in (1, 24, 49):
        x = rng.normal(0, 1, (N, J, 3)).astype(np.float32)
        r = (x + rng.normal(0, 0.05, x.shape)).astype(np.float32) if with_ref else None
        a, n = tracks.accel(_cu(x), ts, None if r is None else _cu(r))
        a_ref, n_ref = to.accel(x, start, r)
        a = a.cpu().numpy()
        assert n.cpu().tolist() == n_ref.tolist() == [0, 0, J, 63 * J] and a[0] == 0 and a[1] == 0
        rel = np.abs(a[2:] - a_ref[2:]) / a_ref[2:]
        _record('accel', rel.max() / 1e-6, J=J, with_ref=with_ref)
        assert (rel <= 1e-6).all()
        b, _ = tracks.accel(_cu(x), ts, None if r is None else _cu(r))
        assert torch.equal(b, torch.from_numpy(a).cuda())


# ------------------------------------------------------------------------------------------------------------------ video
@pytest.fixture(scope='module')
def demo_model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False).cuda().eval()


def clip(missing=True):
    """Six frames of 96 x 80, two people drifting slowly; with `missing`, person 2 has no box in frame 3."""
    from danet_densepose2smpl_amd import scene
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (96, 80, 3)).astype(np.uint8) for _ in range(6)]
    boxes = []
    for f in range(6):
        bs = [scene.boxes_from_xywh([4. + f, 8. + 0.5 * f, 44., 64.]), scene.boxes_from_xywh([32. - f, 20. + f, 42., 60.])]
        boxes.append(bs[:1] if missing and f == 3 else bs)
    return frames, boxes


def test_video_demo_end_to_end(demo_model):
    from danet_densepose2smpl_amd import video
    model = demo_model
    smpl = model.iuv2smpl.smpl
    frames, boxes = clip()
    demo = video.VideoDemo(model, smpl, 2)
    rendered, people, summary = demo(frames, boxes)
    print(summary, flush=True)
    assert summary['tracks'] == 2 and summary['rows'] == 12 and summary['gap_rows'] == 1
    assert [r.shape for r in rendered] == [f.shape for f in frames]
    assert all(p['para'].shape == (2, 229) and p['para_raw'].shape == (2, 229) for p in people)
    assert people[3]['observed'].tolist() == [True, False] and people[3]['track_id'].tolist() == [0, 1]
    gap = people[3]['para'][1]
    R = gap[13:].reshape(24, 3, 3).astype(np.float64)
    assert np.isfinite(gap).all() and np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-5
    for tid in (0, 1):                                                                   # one shape per track
        betas = np.stack([p['para'][list(p['track_id']).index(tid), 3:13] for p in people])
        assert (betas == betas[0]).all()
    # the gap person is drawn in frame 3
    _, ids, _ = demo.last['render_aux']
    off = demo.last['plan']['offsets']
    F2 = int(demo.scene.mesh.tables(demo.scene.device, people[0]['vertices'].shape[1]).faces2.shape[0])
    ids3 = ids.cpu().numpy()[off[3] // 3:off[4] // 3]
    person = np.unique(ids3[ids3 >= 0] // F2)
    gap_person = int(demo.last['tracks'].row_person[np.nonzero(demo.last['tracks'].det < 0)[0][0]])
    print('frame 3: people drawn %s, the gap row is person %d' % (person.tolist(), gap_person), flush=True)
    assert gap_person in person.tolist()
    assert summary['accel_raw'] > 0 and summary['accel'] > 0


def test_video_demo_without_smoothing_is_the_scene_demo(demo_model):
    from danet_densepose2smpl_amd import scene, video
    model = demo_model
    smpl = model.iuv2smpl.smpl
    frames, boxes = clip(missing=False)
    rendered, people, summary = video.VideoDemo(model, smpl, 2, smooth=False)(frames, boxes)
    assert summary['gap_rows'] == 0
    ref = scene.SceneDemo(model, smpl, 2)
    for n in range(len(frames)):
        r, p = ref(frames[n:n + 1], boxes[n:n + 1])
        assert np.array_equal(p[0]['para'].view(np.int32), people[n]['para'].view(np.int32)), n
        assert np.array_equal(r[0], rendered[n]), n


def test_video_demo_with_a_keypoint_fitter(demo_model):
    from danet_densepose2smpl_amd import scene, video
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    model = demo_model
    smpl = model.iuv2smpl.smpl
    plain = scene.SceneDemo(model, smpl, 2)
    frames, boxes = clip()
    rng = np.random.default_rng(4)
    kps = [[np.concatenate([rng.uniform(10, 70, (49, 2)), rng.uniform(0.3, 1.0, (49, 1))], 1) for _ in bs] for bs in boxes]
    fitter = KeypointFitter(smpl, stages=((3, 'cam+orient'), (5, 'all')), res=plain.res, focal=plain.focal)
    demo = video.VideoDemo(model, smpl, 2, fitter=fitter, rounds=2)
    rendered, people, summary = demo(frames, boxes, kps)
    assert len(rendered) == 6 and summary['gap_rows'] == 1
    for p in people:
        assert p['para_init'].shape == (2, 229) and p['fit_loss'].shape == (2, 2) and p['fit_iter'].shape == (2,)
        assert np.isfinite(p['para']).all()


def test_tool_writes_frames_tracks_and_a_json_line(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    frames, boxes = clip()
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    table = {}
    for n, (f, bs) in enumerate(zip(frames, boxes)):
        np.save(str(src / ('f%02d.npy' % n)), f)
        table['f%02d.npy' % n] = [[float(c[0] - 100 * s / 1.2), float(c[1] - 100 * s / 1.2), 200 * s / 1.2, 200 * s / 1.2] for c, s in bs]
    (tmp_path / 'boxes.json').write_text(json.dumps(table))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'demo_video.py'), '--frames_dir', str(src), '--out_dir', str(dst), '--boxes',
                        str(tmp_path / 'boxes.json'), '--batch', '2'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().split('\n')[-1])
    print(line, flush=True)
    assert line['tool'] == 'demo_video' and line['frames'] == 6 and line['tracks'] == 2 and line['rows'] == 12 and line['gap_rows'] == 1
    assert all(line['ms_per_frame'][k] > 0 for k in ('associate', 'boxes', 'prepare', 'infer', 'smooth', 'render'))
    assert sorted(n for n in os.listdir(str(dst)) if n.endswith('_scene.png')) == ['f%02d_scene.png' % n for n in range(6)]
    z = np.load(str(dst / 'tracks.npz'))
    assert z['track_start'].tolist() == [0, 6, 12] and z['frame'].shape == (12,) and z['det'].tolist().count(-1) == 1
    assert z['para_raw'].shape == (12, 229) and z['para'].shape == (12, 229) and z['boxes_raw'].shape == (12, 3) and z['boxes'].shape == (12, 3)
    assert z['accel_raw'].shape == (2,) and z['accel'].shape == (2,) and z['conf'].shape == (12,)
