"""The host side of the stream rule (DESIGN.md 4b'-stream): tracks.OnlineAssociator against tracks.associate, the refusals of
tracks.StreamSmoother and video.StreamDemo (which need neither a device nor the library), the state-size query, the condition on the
inputs of tests/test_gpu_stream.py (the oracle's two solvers agree on every prefix of every streaming case), and the lag table."""
import numpy as np
import pytest
import torch

import stream_cases as sc
import track_oracle as to

U = sc.U


# ------------------------------------------------------------------------------------------------------------------ association
def random_clip(rng, frames, people, p_seen, burst):
    """People on slow random walks; each is seen with probability p_seen per frame, and now and then vanishes for `burst` frames
    (longer than max_gap: its track dies and a new one is born); some carry a confidence; now and then two of them coincide."""
    pos = rng.uniform(0, 600, (people, 2))
    side = rng.uniform(80, 140, people)
    away = np.zeros(people, int)
    boxes = []
    for f in range(frames):
        pos += rng.normal(0, 6, pos.shape)
        if rng.uniform() < 0.1:
            a, b = rng.choice(people, 2, replace=False)
            pos[b], side[b] = pos[a], side[a]                                                # an exact tie
        dets = []
        for p in rng.permutation(people):
            if away[p] > 0:
                away[p] -= 1
                continue
            if rng.uniform() < 0.05:
                away[p] = burst
                continue
            if rng.uniform() < p_seen:
                c = pos[p].copy()
                dets.append((c, side[p] / 200.0) if rng.uniform() < 0.5 else (c, side[p] / 200.0, float(rng.uniform(0.3, 1.0))))
        boxes.append(dets)
    return boxes


@pytest.mark.parametrize('max_gap,min_iou', ((5, 0.3), (1, 0.3), (3, 0.0), (2, 0.6)))
def test_online_associator_equals_associate_on_every_prefix(max_gap, min_iou):
    from danet_densepose2smpl_amd import tracks
    rng = np.random.default_rng(17 + max_gap)
    seen = {'gaps': 0, 'over': 0, 'births': 0, 'deaths': 0}
    for trial in range(6):
        boxes = random_clip(rng, 40, 4, 0.7, max_gap + 2)
        a = tracks.OnlineAssociator(max_gap, min_iou)
        died_all, last = [], {}
        for f, dets in enumerate(boxes):
            matches, died = a.push(dets)
            assert [d for _, d in matches] == list(range(len(dets)))
            for k, _ in matches:
                assert k not in died_all                                                     # a dead track is never extended
                last[k] = f
            assert sorted(died) == sorted(k for k, l in last.items() if f - l == max_gap)
            died_all += died
            if f % 7 == 3 or f == len(boxes) - 1:
                got, ref = a.trackset(), tracks.associate(boxes[:f + 1], max_gap, min_iou)
                assert got.n_frames == ref.n_frames == f + 1
                for name, arr in ref.arrays().items():
                    assert np.array_equal(got.arrays()[name], arr) and got.arrays()[name].dtype == arr.dtype, (trial, f, name)
        ts = a.trackset()
        seen['gaps'] += int((ts.det < 0).sum())
        seen['births'] += ts.K
        seen['deaths'] += len(died_all)
        seen['over'] += sum(1 for k in range(ts.K) if ts.frame[ts.track_start[k + 1] - 1] < len(boxes) - 1 - max_gap)
    print('associator cases:', seen)
    assert seen['births'] > 24 and seen['deaths'] > 0 and seen['over'] > 0 and (seen['gaps'] > 0 or max_gap == 1)


def test_online_associator_refusals():
    from danet_densepose2smpl_amd import tracks
    for kw in ({'max_gap': 0}, {'max_gap': 2.5}, {'min_iou': 1.5}, {'min_iou': -0.1}):
        with pytest.raises(ValueError):
            tracks.OnlineAssociator(**kw)
    a = tracks.OnlineAssociator()
    with pytest.raises(ValueError):
        a.push([(np.zeros(2), -1.0)])
    with pytest.raises(ValueError):
        a.push([(np.zeros(2), 1.0, 1.5)])
    assert a.trackset().K == 0


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_stream_refusals_need_neither_a_device_nor_the_library(monkeypatch):
    from danet_densepose2smpl_amd import _lib, tracks, video

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)
    for kw in ({'slots': 0}, {'lag': -1}, {'max_new': 0}, {'slots': 2.5}, {'channels': None}, {'channels': 0}, {'para': True},
               {'lam': (0.0, -1.0)}, {'lam': (np.nan, 1.0)}, {'lam': (0.0, np.inf)}, {'lam': (1.0,)}):
        with pytest.raises(ValueError):
            tracks.StreamSmoother(**dict({'slots': 2, 'lag': 3, 'channels': 4}, **kw))
    for lam in (((0, 1), (0, 1)), ((0, 1), (0, -1), (0, 1)), ((0, 1), (0, np.nan), (0, 1))):
        with pytest.raises(ValueError):
            tracks.StreamSmoother(2, 3, para=True, lam=lam)

    def fresh(rows_taken=0):
        sm = tracks.StreamSmoother(2, 3, max_new=2, channels=4)
        sm.count[:] = rows_taken                                                           # (as if that many rows had gone in)
        return sm
    rows, conf = torch.zeros(2, 2, 4), np.ones((2, 2), np.float32)
    one, none = np.array([1, 1]), np.array([-1, -1])
    bad_calls = [
        lambda sm: sm.step(one, torch.zeros(2, 2, 5), conf, none),                          # shapes
        lambda sm: sm.step(one, torch.zeros(2, 4), conf, none),
        lambda sm: sm.step(one, rows.to(torch.int32), conf, none),                          # dtypes
        lambda sm: sm.step(one, np.zeros((2, 2, 4), np.float32), conf, none),
        lambda sm: sm.step(one.astype(np.float32), rows, conf, none),
        lambda sm: sm.step(one, rows, conf.astype(np.int32), none),
        lambda sm: sm.step(one, rows, conf, none.astype(np.float64)),
        lambda sm: sm.step(one[:1], rows, conf, none),
        lambda sm: sm.step(one, rows, conf[:, :1], none),
        lambda sm: sm.step(np.array([3, 1]), rows, conf, none),                             # n_new out of range
        lambda sm: sm.step(np.array([-1, 1]), rows, conf, none),
        lambda sm: sm.step(one, rows, conf, np.array([1, -1])),                             # emit: T = 1 after the step, rows 0 .. 0
        lambda sm: sm.step(one, rows, conf, np.array([-2, -1])),
        lambda sm: sm.step(np.array([0, 1]), rows, conf, np.array([0, -1])),               # emit from an empty slot
        lambda sm: sm.step(one, rows, np.array([[0, 1], [1, 1]], np.float32), none),        # a first row without weight
        lambda sm: sm.step(one, rows, np.array([[-0.5, 1], [1, 1]], np.float32), none),     # conf
        lambda sm: sm.step(one, rows, np.array([[np.nan, 1], [1, 1]], np.float32), none),
        lambda sm: sm.step(np.array([2, 1]), rows, np.array([[1, np.inf], [1, 1]], np.float32), none),
    ]
    for i, call in enumerate(bad_calls):
        sm = fresh()
        with pytest.raises(ValueError):
            call(sm)
        assert sm.count.tolist() == [0, 0] and sm.state is None, i
    sm = fresh(10)                                                                           # T = 11 after the step: rows 7 .. 10
    for e in (6, 11):
        with pytest.raises(ValueError):
            sm.step(one, rows, conf, np.array([e, -1]))
    with pytest.raises(ValueError):
        sm.reset(2)
    # all right but on the CPU: refused as everywhere, and nothing has moved
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        sm.step(one, rows, conf, np.array([7, 10]))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        sm.launch(rows)
    assert sm.count.tolist() == [10, 10] and sm.state is None
    # a weight beyond n_new is not looked at
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        fresh().step(one, rows, np.array([[1, np.nan], [1, -3]], np.float32), none)
    # the pipeline: box_lag below max_gap cannot tell a gap row from an ended track
    for kw in ({'box_lag': 4}, {'lag': -1}, {'slots': 0}, {'gap_conf': 2.0}, {'box_lag': 2.5}):
        with pytest.raises(ValueError):
            video.StreamDemo.check_arguments(**dict({'lag': 8, 'box_lag': 8, 'slots': 32, 'max_gap': 5, 'gap_conf': 0.0}, **kw))
    video.StreamDemo.check_arguments(lag=0, box_lag=5, slots=1, max_gap=5, gap_conf=0.0)


def test_state_size_query_is_host_side():
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    # per slot: a header of 24 bytes, a ring of R = lag + max_new + 4 weights (fp32, R rounded up to even), and in doubles
    # l1, l2, D, zB [3 groups][R], sum c y [C], and the right-hand side and zA [R][C]
    assert L.danet_track_stream_state_bytes(1, 1, 0, 1) == 24 + 4 * 6 + 8 * (12 * 5 + 1 + 2 * 5 * 1) == 616
    assert L.danet_track_stream_state_bytes(32, 157, 8, 1) == 32 * (24 + 4 * 14 + 8 * (12 * 13 + 157 + 2 * 13 * 157)) == 1127680
    for bad in ((0, 3, 1, 1), (1, 0, 1, 1), (1, 3, -1, 1), (1, 3, 1, 0)):
        assert L.danet_track_stream_state_bytes(*bad) == 0


# ------------------------------------------------------------------------------------------------------------------ the oracle
def test_the_two_solvers_agree_on_every_prefix_of_every_gpu_case():
    """Within 0.25 of one fp32 rounding of the block's largest entry, the condition tests/test_tracks_host.py imposes on the offline
    cases: a condition on the inputs, not a measurement of the kernel."""
    worst, where = 0.0, None
    for C in sc.WIDTHS:
        for kind in sc.KINDS:
            for lam in to.LAMS:
                for f, (_, _, gap, dmax) in enumerate(sc.plain_refs(C, kind, lam)):
                    r = gap / (0.5 * U * dmax)
                    if r > worst:
                        worst, where = r, (C, kind, lam, f + 1)
                    assert r <= 0.25, (C, kind, lam, f + 1, r)
    for shared in (True, False):
        for k, per in enumerate(sc.para_refs(shared)):
            for f, (_, gap, dch) in enumerate(per):
                for sl in to.GROUPS:
                    r = gap[:, sl].max() / (0.5 * U * np.abs(dch[:, sl]).max())
                    if r > worst:
                        worst, where = r, ('para', shared, k, f + 1)
                    assert r <= 0.25, ('para', shared, k, f + 1, r)
    print('two solvers on prefixes: at most %.4f fp32 roundings apart, at %s' % (worst, where))


def test_the_6d_map_is_well_conditioned_on_every_prefix():
    for shared in (True, False):
        lo = min(min(b['a1'].min(), b['u'].min()) for per in sc.para_refs(shared) for b, _, _ in per)
        print('6D conditioning on prefixes: min(|a_1|, |u|) = %.3f' % lo)
        assert lo >= 0.5


def fixed_lag(rc, lag):
    """The fixed-lag estimate of every row of the recovery case in float64: row g of a track from its committed prefix at the time, the
    rows 0 .. l', l' the last observed row up to min(g + lag, T - 1) or, where that lies before g, the first one after g.  lag None:
    the offline result."""
    st = rc['track_start']
    out = np.empty((st[-1], 229))
    for k in range(len(st) - 1):
        s, T = int(st[k]), int(st[k + 1] - st[k])
        cache = {}
        for g in range(T):
            f = T - 1 if lag is None else min(g + lag, T - 1)
            while rc['conf'][s + f] == 0:                                                    # a committed prefix ends in an observed row:
                f -= 1                                                                       # the last one seen by then,
            while f < g or rc['conf'][s + f] == 0:                                           # or, for a gap row still open, the one that closes it
                f += 1
            if f not in cache:
                cache[f] = to.smooth_para(rc['obs'][s:s + f + 1], rc['conf'][s:s + f + 1], np.array([0, f + 1]), to.DEFAULT_LAM, True)['para64']
            out[s + g] = cache[f][g]
    return out


def test_lag_table():
    """Smoothed / observed per track of the recovery case: the error of the joints against ground truth and the acceleration error.
    At the default lag every track improves strictly on both."""
    from danet_densepose2smpl_amd import video
    rc = to.recovery_case()
    st = rc['track_start']
    jg = to.toy_joints(rc['gt'])
    e0 = to.joint_error(rc['obs_full'], rc['gt'], st)
    a0, _ = to.accel(to.toy_joints(rc['obs_full']), st, jg)
    print('| lag | joint error ratio | acceleration error ratio |')
    table = {}
    for lag in (0, 2, 5, 8, 16, None):
        x = fixed_lag(rc, lag)
        e1 = to.joint_error(x, rc['gt'], st)
        a1, _ = to.accel(to.toy_joints(x), st, jg)
        table[lag] = (e1 / e0, a1 / a0)
        print('| %s | %s | %s |' % ('offline' if lag is None else lag, ' '.join('%.3f' % v for v in e1 / e0), ' '.join('%.3f' % v for v in a1 / a0)))
    assert video.STREAM_LAG == 8
    assert (table[8][0] < 1).all() and (table[8][1] < 1).all()
    assert np.array_equal(table[None][1].round(2), table[8][1].round(2)) or np.abs(table[None][1] - table[8][1]).max() < 0.005
    ref = to.smooth_para(rc['obs'], rc['conf'], st, to.DEFAULT_LAM, True)['para64']
    assert np.array_equal(fixed_lag(rc, 64), ref) and np.array_equal(fixed_lag(rc, None), ref)       # lag >= T: the offline result
