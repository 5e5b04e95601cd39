"""The host side of the track rule (DESIGN.md 4b'-track): tracks.associate by known answers, the TrackSet's invariants, the argument
refusals (which need no device), and the conditions on the inputs of tests/test_gpu_tracks.py: the oracle's two solvers agree on every
case those tests use, the 6D map is well conditioned on every para case, and the recovery case improves in float64."""
import numpy as np
import pytest
import torch

import track_oracle as to

U = 2.0 ** -23


def sq(cx, cy, side, conf=None):
    """A square of the given side as a box entry (center, scale = side / 200)."""
    return (np.array([cx, cy], np.float64), side / 200.0) if conf is None else (np.array([cx, cy], np.float64), side / 200.0, conf)


def tracks_of(ts):
    """Per track the list of (frame, det)."""
    return [[(int(ts.frame[n]), int(ts.det[n])) for n in range(ts.track_start[k], ts.track_start[k + 1])] for k in range(ts.K)]


# ------------------------------------------------------------------------------------------------------------------ association
def test_iou_of_squares():
    from danet_densepose2smpl_amd import tracks
    assert tracks.square_iou([0, 0], 0.5, [0, 0], 0.5) == 1.0
    assert tracks.square_iou([0, 0], 0.5, [50, 0], 0.5) == pytest.approx(1.0 / 3.0)          # overlap 50 x 100 of two 100 x 100
    assert tracks.square_iou([0, 0], 0.5, [100, 0], 0.5) == 0.0
    assert tracks.square_iou([0, 0], 0.5, [0, 0], 1.0) == 0.25


def test_two_people_crossing():
    """Two people walk through each other, 30 px per frame, squares of 100: each step keeps IoU 0.54 with the own last square, and the
    greedy order by IoU follows each person."""
    from danet_densepose2smpl_amd import tracks
    boxes = []
    for f in range(7):
        a, b = sq(10 + 30 * f, 50, 100), sq(190 - 30 * f, 52, 100)
        boxes.append([a, b] if f % 2 == 0 else [b, a])                                       # the detector's order flips
    ts = tracks.associate(boxes)
    assert ts.K == 2 and ts.track_start.tolist() == [0, 7, 14]
    assert tracks_of(ts)[0] == [(f, 0 if f % 2 == 0 else 1) for f in range(7)]
    assert tracks_of(ts)[1] == [(f, 1 if f % 2 == 0 else 0) for f in range(7)]
    assert (ts.conf == 1).all()


def test_exact_tie_goes_to_the_lower_track_then_the_lower_detection():
    from danet_densepose2smpl_amd import tracks
    # two tracks at x = 0 and x = 80, one detection exactly between them: the same IoU with both, track 0 takes it
    ts = tracks.associate([[sq(0, 0, 100), sq(80, 0, 100)], [sq(40, 0, 100)]])
    assert tracks_of(ts) == [[(0, 0), (1, 0)], [(0, 1)]]
    # one track, two detections at the same distance on either side: detection 0 is taken, detection 1 opens a track
    ts = tracks.associate([[sq(40, 0, 100)], [sq(60, 0, 100), sq(20, 0, 100)]])
    assert tracks_of(ts) == [[(0, 0), (1, 0)], [(1, 1)]]


def test_a_track_ends_while_another_starts_in_the_same_frame():
    from danet_densepose2smpl_amd import tracks
    boxes = [[sq(0, 0, 100)], [sq(2, 0, 100)], [sq(500, 0, 100)], [sq(502, 0, 100)]]
    ts = tracks.associate(boxes)
    assert tracks_of(ts) == [[(0, 0), (1, 0)], [(2, 0), (3, 0)]]


def test_gaps_max_gap_and_the_empty_frame():
    """A track is live while its last observed frame is at most max_gap frames back: a distance of max_gap is bridged (max_gap - 1 gap
    rows, among them an empty frame), max_gap + 1 is not."""
    from danet_densepose2smpl_amd import tracks
    for dist, K in ((5, 1), (6, 2)):
        boxes = [[sq(0, 0, 100, 0.8)]] + [[] for _ in range(dist - 1)] + [[sq(3, 0, 100)]]
        ts = tracks.associate(boxes, max_gap=5)
        assert ts.K == K
        if K == 1:
            assert ts.det.tolist() == [0, -1, -1, -1, -1, 0] and ts.frame.tolist() == list(range(6))
            assert ts.conf.tolist() == [np.float32(0.8), 0, 0, 0, 0, 1]
        else:
            assert ts.track_start.tolist() == [0, 1, 2] and ts.frame.tolist() == [0, 6]
    ts = tracks.associate([[], [], []])
    assert ts.K == 0 and ts.N == 0 and ts.n_frames == 3


def test_min_iou_at_the_boundary():
    from danet_densepose2smpl_amd import tracks
    # squares of 100 shifted by 50: IoU = 1/3, in float64 5000 / 15000
    iou = tracks.square_iou([0, 0], 0.5, [50, 0], 0.5)
    boxes = [[sq(0, 0, 100)], [sq(50, 0, 100)]]
    assert tracks.associate(boxes, min_iou=iou).K == 1                                       # >= min_iou matches
    assert tracks.associate(boxes, min_iou=np.nextafter(iou, 1.0)).K == 2


def test_csr_invariants_and_the_permutation_round_trip():
    from danet_densepose2smpl_amd import tracks
    rng = np.random.default_rng(2)
    boxes = []
    for f in range(12):
        bs = [sq(20 + 3 * f, 40, 90), sq(300 - 2 * f, 60, 110), sq(600, 50 + f, 100)]
        boxes.append([b for b in bs if rng.uniform() > 0.25])
    ts = tracks.associate(boxes)
    N = ts.N
    assert ts.track_start[0] == 0 and ts.track_start[-1] == N and (np.diff(ts.track_start) >= 1).all()
    for k in range(ts.K):
        s, e = ts.track_start[k], ts.track_start[k + 1]
        assert (np.diff(ts.frame[s:e]) == 1).all() and ts.det[s] >= 0 and ts.det[e - 1] >= 0       # one row per frame of the span
        assert ((ts.conf[s:e] > 0) == (ts.det[s:e] >= 0)).all()
    seen = sorted((int(f), int(d)) for f, d in zip(ts.frame, ts.det) if d >= 0)
    assert seen == [(f, d) for f, bs in enumerate(boxes) for d in range(len(bs))]            # every detection in exactly one row
    assert (ts.det < 0).sum() > 0
    # person order: frame-major, detections in their order first, then gap rows by track
    assert np.array_equal(np.sort(ts.person_row), np.arange(N)) and np.array_equal(ts.person_row[ts.row_person], np.arange(N))
    x = rng.normal(size=(N, 3))
    assert np.array_equal(x[ts.row_person][ts.person_row], x) and np.array_equal(x[ts.person_row][ts.row_person], x)
    pf = ts.frame[ts.person_row]
    assert (np.diff(pf) >= 0).all()
    for f in range(12):
        d = ts.det[ts.person_row][pf == f]
        n = len(boxes[f])
        assert d[:n].tolist() == list(range(n)) and (d[n:] == -1).all()
        assert (np.diff(ts.track[ts.person_row][pf == f][n:]) > 0).all()
    assert tracks.associate(boxes).arrays()['det'].tolist() == ts.det.tolist()               # deterministic


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    from danet_densepose2smpl_amd import tracks
    good = tracks.TrackSet([0, 5, 11], np.arange(11), np.zeros(11), np.ones(11), 11)
    for start in ([1, 5, 11], [0, 5, 10], [0, 7, 6, 11]):
        with pytest.raises(ValueError):
            tracks.TrackSet(start, np.arange(11), np.zeros(11), np.ones(11), 11)
        bad = tracks.TrackSet([0, 5, 11], np.arange(11), np.zeros(11), np.ones(11), 11)
        bad.track_start = np.array(start, np.int32)
        with pytest.raises(ValueError):
            tracks.smooth(torch.zeros(11, 3), bad)
    for c in (-0.1, np.inf, np.nan):
        conf = np.ones(11)
        conf[4] = c
        with pytest.raises(ValueError):
            tracks.TrackSet([0, 5, 11], np.arange(11), np.zeros(11), conf, 11)
        with pytest.raises(ValueError):
            good.with_conf(conf)
    for lam in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            tracks.smooth(torch.zeros(11, 3), good, lam, 0.0)
        with pytest.raises(ValueError):
            tracks.smooth(torch.zeros(11, 3), good, 0.0, lam)
        with pytest.raises(ValueError):
            tracks.smooth_para(torch.zeros(11, 229), good, ((0, 1), (0, lam), (0, 1)))
    with pytest.raises(ValueError):
        tracks.smooth_para(torch.zeros(11, 229), good, ((0, 1), (0, 1)))
    for bad in (torch.zeros(11), torch.zeros(10, 3), torch.zeros(11, 3, dtype=torch.int32), np.zeros((11, 3))):
        with pytest.raises(ValueError):
            tracks.smooth(bad, good)
    with pytest.raises(ValueError):
        tracks.smooth_para(torch.zeros(11, 228), good)
    with pytest.raises(ValueError):
        tracks.accel(torch.zeros(11, 24, 2), good)
    with pytest.raises(ValueError):
        tracks.accel(torch.zeros(11, 24, 3), good, torch.zeros(11, 23, 3))
    with pytest.raises(ValueError):
        tracks.smooth(torch.zeros(11, 3), 'tracks')
    with pytest.raises(ValueError):
        tracks.associate([[sq(0, 0, 100, 1.5)]])
    with pytest.raises(ValueError):
        tracks.associate([[sq(0, 0, -100)]])
    # CPU tensors that are otherwise right: refused as everywhere
    for call in (lambda: tracks.smooth(torch.zeros(11, 3), good), lambda: tracks.smooth_para(torch.zeros(11, 229), good),
                 lambda: tracks.accel(torch.zeros(11, 24, 3), good)):
        with pytest.raises(RuntimeError, match='GPU only|no CPU'):
            call()


def test_workspace_query_is_host_side():
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    assert L.danet_track_smooth_ws_bytes(100, 157) == 8 * (9 * 100 + 100 * 157)
    assert L.danet_track_smooth_ws_bytes(0, 3) == 0


# ------------------------------------------------------------------------------------------------------------------ the oracle
def smooth_cases():
    for C in to.WIDTHS:
        for i, kind in enumerate(to.CONF_KINDS):
            yield ('C%d-%s' % (C, kind),) + to.make_case(to.LENGTHS, C, kind, to.case_seed(C, i))
    parts = [to.make_case((T,), 65, kind, 7 + i) for i, (T, kind) in enumerate(to.FIVE)]
    yield 'five', np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([[0], np.cumsum([T for T, _ in to.FIVE])])
    yield ('nan',) + to.make_case((5, 64, 6), 65, 'mid', 3)


def test_the_two_solvers_agree_on_every_gpu_case():
    """Within 0.25 of one fp32 rounding of the block's largest entry: a condition on the inputs, not a measurement of the kernel."""
    worst = 0.0
    for name, v, conf, start in smooth_cases():
        for lam in to.LAMS:
            a, _ = to.smooth(v, conf, start, lam[0], lam[1], to.solve_dense)
            gap = to.solver_gap(v, conf, start, lam[0], lam[1])
            for k in range(len(start) - 1):
                s, e = start[k], start[k + 1]
                if conf[s:e].sum() > 0:
                    r = gap[k] / (0.5 * U * np.abs(a[s:e]).max())
                    worst = max(worst, r)
                    assert r <= 0.25, (name, lam, k, r)
    para, conf, start, _ = to.para_case()
    for shared in (True, False):
        b = to.smooth_para(para, conf, start, to.DEFAULT_LAM, shared)
        d = to.smooth_para(para, conf, start, to.DEFAULT_LAM, shared, solver=to.solve_dense)
        for k in range(len(start) - 1):
            s, e = start[k], start[k + 1]
            if b['status'][k]:
                continue
            for sl in to.GROUPS:
                r = np.abs(b['ch'][s:e, sl] - d['ch'][s:e, sl]).max() / (0.5 * U * np.abs(d['ch'][s:e, sl]).max())
                worst = max(worst, r)
                assert r <= 0.25, ('para', shared, k, r)
    print('two solvers: at most %.4f fp32 roundings apart' % worst)


def test_the_6d_map_is_well_conditioned_on_every_para_case():
    """|a_1| >= 0.5 and |u| >= 0.5 on every smoothed column: no case is left out of the rotation bound (the cap on left-out cases is
    zero)."""
    para, conf, start, _ = to.para_case()
    for shared in (True, False):
        r = to.smooth_para(para, conf, start, to.DEFAULT_LAM, shared)
        print('6D conditioning: min |a_1| %.3f, min |u| %.3f' % (r['a1'].min(), r['u'].min()))
        assert r['a1'].min() >= 0.5 and r['u'].min() >= 0.5


def test_oracle_basics():
    """The banded factor reproduces the dense matrix; T = 1 and T = 2 lack the terms that need more rows; a constant and (with
    lam_vel = 0) a straight line pass unchanged; rows with c = 0 are never read."""
    rng = np.random.default_rng(0)
    for T in (1, 2, 3, 4, 7):
        c = rng.uniform(0.1, 1, T)
        l1, l2, D = to.factor(c, 0.7, 3.0)
        Lm = np.eye(T) + np.diag(l1[1:], -1) + (np.diag(l2[2:], -2) if T > 2 else 0)
        assert np.abs(Lm @ np.diag(D) @ Lm.T - to.system(c, 0.7, 3.0)).max() < 1e-12
    assert np.allclose(to.system([1.0], 5, 5), [[1 + to.EPS]]) and np.allclose(to.system([1, 1], 2, 9), np.array([[3, -2], [-2, 3]]) + to.EPS * np.eye(2))
    t = np.arange(9.0)
    line = np.stack([np.full(9, 3.0), 2 * t - 1], 1)
    c = np.ones(9)
    assert np.abs(to.solve_banded(line, c, 0.0, 50.0) - line).max() < 1e-9
    c[3:6] = 0
    y = line.copy()
    y[3:6] = np.nan
    x = to.solve_banded(y, c, 0.0, 50.0)
    assert np.isfinite(x).all() and np.abs(x[:, 0] - 3.0).max() < 1e-9 and np.abs(x[:, 1] - line[:, 1]).max() < 1e-3      # the gap is bridged by the line
    a, n = to.accel(np.stack([t * t, t, 0 * t], 1)[:, None, :], [0, 9])
    assert n[0] == 7 and abs(a[0] - 2.0) < 1e-12


def test_recovery_case_improves_on_every_track_in_float64():
    rc = to.recovery_case()
    st = rc['track_start']
    assert (rc['conf'] == 0).sum() >= 3 and np.isnan(rc['obs'][rc['conf'] == 0]).all()
    r = to.smooth_para(rc['obs'], rc['conf'], st, to.DEFAULT_LAM, True)
    e0, e1 = to.joint_error(rc['obs_full'], rc['gt'], st), to.joint_error(r['para64'], rc['gt'], st)
    jg = to.toy_joints(rc['gt'])
    a0, _ = to.accel(to.toy_joints(rc['obs_full']), st, jg)
    a1, _ = to.accel(to.toy_joints(r['para64']), st, jg)
    print('recovery: joint error ratio %s, acceleration error ratio %s' % ((e1 / e0).round(4).tolist(), (a1 / a0).round(4).tolist()))
    assert (e1 < e0).all() and (a1 < a0).all()
    from danet_densepose2smpl_amd import tracks
    assert tuple(map(tuple, tracks.DEFAULT_LAM)) == to.DEFAULT_LAM


# ------------------------------------------------------------------------------------------------------------------ rules stated once
def test_trackset_check_fires_from_the_constructor_and_from_the_ops():
    from danet_densepose2smpl_amd import tracks
    build = lambda start=(0, 1, 3), conf=(1, 1, 1): tracks.TrackSet(start, [0, 0, 1], [0, 0, 0], conf, 2)        # noqa: E731
    ts = build()
    assert (ts.K, ts.N) == (2, 3)
    ts.check('op')
    assert tracks._tracks(ts, 3, 'op') is ts
    ts.conf[1] = -0.5
    with pytest.raises(ValueError, match='^op: conf must be finite and not negative'):
        tracks._tracks(ts, 3, 'op')
    with pytest.raises(ValueError, match='^tracks.smooth: conf must be finite'):
        tracks.smooth(torch.zeros(3, 2), ts)
    with pytest.raises(ValueError, match='^TrackSet: conf must be finite and not negative'):
        build(conf=(1, -0.5, 1))
    ts = build()
    ts.track_start = np.array([1, 2, 3], np.int32)
    with pytest.raises(ValueError, match='^op: track_start must ascend from 0 to 3'):
        tracks._tracks(ts, 3, 'op')
    with pytest.raises(ValueError, match='^tracks.accel: track_start must ascend'):
        tracks.accel(torch.zeros(3, 24, 3), ts)
    with pytest.raises(ValueError, match='^TrackSet: track_start must ascend from 0 to 3'):
        build(start=(1, 2, 3))
    with pytest.raises(ValueError, match='^op: 4 rows, the TrackSet has 3'):
        tracks._tracks(build(), 4, 'op')
    with pytest.raises(ValueError, match='^op: a TrackSet expected, got list'):
        tracks._tracks([0, 3], 3, 'op')


def test_lam_pairs():
    from danet_densepose2smpl_amd import tracks
    assert tracks._lam_pairs(((0, 3), [0.5, 10], (1, 2.5)), 'op') == [0.0, 3.0, 0.5, 10.0, 1.0, 2.5]
    assert tracks._lam_pairs(tracks.DEFAULT_LAM, 'op') == [0.0, 3.0, 0.0, 10.0, 0.0, 10.0]
    for bad in (((0, 1), (0, 1)), ((0, 1), (0, 1, 2), (0, 1)), ((0, 1), (0, 1), (0, 1), (0, 1)), ((0, 1), (0,), (0, 1))):
        with pytest.raises(ValueError, match=r'^op: lam must hold three \(lam_vel, lam_acc\) pairs'):
            tracks._lam_pairs(bad, 'op')
    for v in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='^op: lam: .*finite and not negative'):
            tracks._lam_pairs(((0, 1), (0, v), (0, 1)), 'op')
    # the two callers share it
    with pytest.raises(ValueError, match='^tracks.StreamSmoother: lam must hold three'):
        tracks.StreamSmoother(2, 3, para=True, lam=((0, 1), (0, 1)))
    assert tracks.StreamSmoother(2, 3, para=True).lam == tracks._lam_pairs(tracks.DEFAULT_LAM, 'op')
