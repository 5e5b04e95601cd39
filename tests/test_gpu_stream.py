"""The stream rule on the device (DESIGN.md 4b'-stream): csrc/track_stream.hip through tracks.StreamSmoother, and video.StreamDemo,
against tests/track_oracle.py run on prefixes.  The value emitted for row g of a slot that holds rows 0 .. f is the offline oracle of
those rows read at row g, under the bounds of tests/test_gpu_tracks.py, each taken on the prefix block: |kernel - f64| <=
8 x 2^-23 x max |f64| plus four times the oracle's two-solver difference; rotation blocks four times the float32 oracle's error plus 8
roundings of 1.  tests/test_stream_host.py bounds the two-solver difference on every prefix of the cases used here
(tests/stream_cases.py).  Every parity test prints measured / bound and hands it to conftest.record."""
import json
import os

import numpy as np
import pytest
import torch

import stream_cases as sc
import track_oracle as to
from conftest import record
from track_oracle import LAMS

pytestmark = pytest.mark.gpu

U = sc.U


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _record(name, ratio, **kw):
    print('%s: measured / bound = %.4f %s' % (name, ratio, kw), flush=True)
    record('stream.' + name, dict(kw, ratio=round(float(ratio), 6)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_plain(sm, tracks_in, schedule, emit_rule):
    """Stream tracks_in[s] = (values [T,C], conf [T]) through slot s of `sm`: schedule[step][s] rows per step.  emit_rule(T, s) -> the row
    to emit or -1.  -> per step (out [S,C], valid [S], emit [S], T [S]) on the host."""
    S, M, C = sm.S, sm.max_new, sm.width
    pos = np.zeros(S, int)
    log = []
    for n_new in schedule:
        rows = np.full((S, M, C), np.nan, np.float32)
        conf = np.zeros((S, M), np.float32)
        for s in range(S):
            v, c = tracks_in[s]
            rows[s, :n_new[s]] = v[pos[s]:pos[s] + n_new[s]]
            conf[s, :n_new[s]] = c[pos[s]:pos[s] + n_new[s]]
        pos += np.asarray(n_new)
        emit = np.array([emit_rule(pos[s], s) for s in range(S)])
        out, valid = sm.step(np.asarray(n_new), _cu(rows), conf, emit)
        log.append((out.cpu().numpy().copy(), valid.cpu().numpy().copy(), emit, pos.copy()))
    return log


# ------------------------------------------------------------------------------------------------------------------ parity, plain
@pytest.mark.parametrize('lam', LAMS)
@pytest.mark.parametrize('C', sc.WIDTHS)
def test_stream_against_the_oracle_on_every_prefix(C, lam):
    """One 70-row track per weight pattern, a row per step, the row `lag` behind emitted at every step and the tail flushed at the
    end: every prefix length 1 .. 70 is passed through.  With lag 70 the flush is the offline result on the whole track."""
    from danet_densepose2smpl_amd import tracks
    T = sc.T_PLAIN
    cases = [sc.plain_case(C, kind) for kind in sc.KINDS]
    refs = [sc.plain_refs(C, kind, lam) for kind in sc.KINDS]
    for lag in sc.LAGS:
        sm = tracks.StreamSmoother(len(cases), lag, channels=C, lam=lam)
        worst, emitted = 0.0, 0
        log = run_plain(sm, cases, [[1] * len(cases)] * T, lambda t, s: max(t - 1 - lag, 0))
        flush = list(range(max(T - lag, 1), T)) if lag < T else list(range(T))               # rows not yet emitted with the whole track in
        for g in flush:
            out, valid = sm.step(np.zeros(len(cases), np.int64), _cu(np.full((len(cases), 1, C), np.nan, np.float32)),
                                 np.zeros((len(cases), 1), np.float32), np.full(len(cases), g))
            log.append((out.cpu().numpy().copy(), valid.cpu().numpy().copy(), np.full(len(cases), g), np.full(len(cases), T)))
        for out, valid, emit, pos in log:
            assert valid.tolist() == [1] * len(cases)
            for s in range(len(cases)):
                x, xmax, gap, _ = refs[s][pos[s] - 1]
                assert np.isfinite(out[s]).all()
                worst = max(worst, np.abs(out[s] - x[emit[s]]).max() / (8 * U * xmax + 4 * gap))
                emitted += 1
        if lag >= T:                                                                       # the flush against the offline oracle
            for s, (v, c) in enumerate(cases):
                off, _ = to.smooth(v, c, [0, T], lam[0], lam[1])
                gap = to.solver_gap(v, c, [0, T], lam[0], lam[1])[0]
                got = np.stack([log[T + g][0][s] for g in range(T)])
                worst = max(worst, np.abs(got - off).max() / (8 * U * np.abs(off).max() + 4 * gap))
        _record('plain', worst, C=C, lam=list(lam), lag=lag, rows=emitted)
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ parity, para
@pytest.mark.parametrize('lag', (3, 40))
@pytest.mark.parametrize('shared', (True, False))
def test_stream_para_against_the_oracle_on_every_prefix(shared, lag):
    """The recovery case's three tracks and the T = 1 and T = 2 tracks, a slot each; lag 40 is every track's length, so its flush is
    the offline result."""
    from danet_densepose2smpl_amd import tracks
    trs, _ = sc.para_tracks()
    refs = sc.para_refs(shared)
    S = len(trs)
    lens = np.array([len(c) for _, c in trs])
    sm = tracks.StreamSmoother(S, lag, para=True, shared_shape=shared)
    worst = {'cam': 0.0, 'betas': 0.0, 'rot': 0.0}
    steps = [(np.minimum(f + 1, lens) - np.minimum(f, lens), False) for f in range(lens.max())]
    steps += [(np.zeros(S, int), g) for g in range(lens.max())]                              # the flush: every row once more, whole tracks in
    pos = np.zeros(S, int)
    emitted = 0
    for n_new, flush_row in steps:
        rows = np.full((S, 1, 229), np.nan, np.float32)
        conf = np.zeros((S, 1), np.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, 0], conf[s, 0] = trs[s][0][pos[s]], trs[s][1][pos[s]]
        pos += n_new
        if flush_row is False:
            emit = np.where(n_new > 0, np.maximum(pos - 1 - lag, 0), -1)
        else:
            emit = np.where((flush_row >= pos - 1 - lag) & (flush_row < pos), flush_row, -1)
        out, valid = sm.step(n_new, _cu(rows), conf, emit)
        out, valid = out.cpu().numpy(), valid.cpu().numpy()
        assert valid.tolist() == (emit >= 0).astype(int).tolist()
        for s in range(S):
            if emit[s] < 0:
                assert not out[s].any()
                continue
            ref, gap, _ = refs[s][pos[s] - 1]
            got, g = out[s], int(emit[s])
            assert np.isfinite(got).all()
            for name, r in sc.para_ratio(got, ref, gap, g).items():
                worst[name] = max(worst[name], r)
            obs = trs[s][1][:pos[s]] > 0
            assert trs[s][0][:pos[s], 0][obs].min() <= got[0] <= trs[s][0][:pos[s], 0][obs].max()
            R = got[13:].reshape(24, 3, 3).astype(np.float64)
            assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-5 and np.abs(np.linalg.det(R) - 1).max() < 1e-5
            emitted += 1
    for name, w in worst.items():
        _record('para', w, block=name, shared_shape=shared, lag=lag, rows=emitted)
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ several slots
def test_five_slots_of_different_ages_in_one_launch():
    """Five slots, max_new = 3: rows arrive 0, 1 or 3 at a time, slot 3 is reset in the middle and starts another track, slot 4 stays
    empty.  Every slot's bits are those of the same slot streamed alone."""
    from danet_densepose2smpl_amd import tracks
    C, lag, lam = 65, 3, (0.5, 100.0)
    data = [sc.plain_case(C, kind, 40, seed=50 + i) for i, kind in enumerate(('ones', 'mid', 'rand', 'rand'))]
    second = sc.plain_case(C, 'mid', 20, seed=60)
    sched = [[1, 3, 0, 1], [1, 0, 1, 3], [3, 1, 0, 0], [0, 3, 3, 1], [1, 1, 1, 0], [3, 3, 0, 1], [1, 0, 1, 3], [0, 1, 3, 3], [1, 3, 1, 1]]
    reset_at = 4                                                                             # slot 3 starts over before this step

    def run(slots):
        """slots: the subset of (0 .. 4) streamed, in a smoother of that many slots."""
        sm = tracks.StreamSmoother(len(slots), lag, max_new=3, channels=C, lam=lam)
        pos = {s: 0 for s in slots}
        src = {s: data[s] if s < 4 else None for s in slots}
        outs = []
        for i, n4 in enumerate(sched):
            n_new = np.array([n4[s] if s < 4 else 0 for s in slots])
            if i == reset_at and 3 in slots:
                sm.reset(slots.index(3))
                src[3], pos[3] = second, 0
            rows = np.full((len(slots), 3, C), np.nan, np.float32)
            conf = np.zeros((len(slots), 3), np.float32)
            emit = np.full(len(slots), -1)
            for j, s in enumerate(slots):
                if s == 4:
                    continue
                rows[j, :n_new[j]] = src[s][0][pos[s]:pos[s] + n_new[j]]
                conf[j, :n_new[j]] = src[s][1][pos[s]:pos[s] + n_new[j]]
                pos[s] += n_new[j]
                emit[j] = max(pos[s] - 1 - (i % (lag + 1)), 0) if pos[s] else -1             # a different distance every step
            out, valid = sm.step(n_new, _cu(rows), conf, emit)
            outs.append((out.cpu().numpy().copy(), valid.cpu().numpy().copy(), emit, dict(pos)))
        return outs
    together = run([0, 1, 2, 3, 4])
    assert all(v.tolist() == [1, 1, int(p[2] > 0), int(p[3] > 0), 0] for _, v, _, p in together)
    # against the oracle too: the rows are right, not only equal
    for i, (out, valid, emit, pos) in enumerate(together):
        for s in range(4):
            if emit[s] < 0:
                continue
            v, c = (second if (s == 3 and i >= reset_at) else data[s])
            ref = to.solve_banded(v[:pos[s]], c[:pos[s]], *lam)
            gap = np.abs(ref - to.solve_dense(v[:pos[s]], c[:pos[s]], *lam)).max()
            assert np.abs(out[s] - ref[emit[s]]).max() <= 8 * U * np.abs(ref).max() + 4 * gap, (i, s)
    for s in range(5):
        alone = run([s])
        for (o5, v5, _, _), (o1, v1, _, _) in zip(together, alone):
            assert v5[s] == v1[0] and np.array_equal(_bits(o5[s]), _bits(o1[0])), s
    again = run([0, 1, 2, 3, 4])
    assert all(np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(together, again))


def test_seven_tracks_through_two_slots():
    """A slot that is reset and reused gives the bits of a fresh one."""
    from danet_densepose2smpl_amd import tracks
    C, lag, lam = 64, 3, (0.0, 10.0)
    lengths = (5, 9, 1, 12, 2, 7, 6)
    data = [sc.plain_case(C, ('ones', 'rand', 'mid')[i % 3], T, seed=80 + i) for i, T in enumerate(lengths)]

    def stream(sm, slot_of, order):
        """Feed the tracks in `order`, each to slot slot_of[k], one after the other in a slot; -> per track the emitted rows."""
        got = {k: [] for k in order}
        queues = {}
        for k in order:
            queues.setdefault(slot_of[k], []).append(k)
        cur = {s: None for s in queues}
        pos = {}
        while any(queues.values()) or any(c is not None for c in cur.values()):
            n_new, emit = np.zeros(sm.S, int), np.full(sm.S, -1)
            rows, conf = np.full((sm.S, 1, C), np.nan, np.float32), np.zeros((sm.S, 1), np.float32)
            for s in cur:
                if cur[s] is None and queues[s]:
                    cur[s] = queues[s].pop(0)
                    pos[cur[s]] = 0
                    sm.reset(s)
                k = cur[s]
                if k is None:
                    continue
                v, c = data[k]
                rows[s, 0], conf[s, 0] = v[pos[k]], c[pos[k]]
                pos[k] += 1
                n_new[s], emit[s] = 1, max(pos[k] - 1 - lag, 0)
            out, valid = sm.step(n_new, _cu(rows), conf, emit)
            out = out.cpu().numpy()
            for s in cur:
                k = cur[s]
                if k is not None:
                    got[k].append(out[s].copy())
                    if pos[k] == lengths[k]:
                        cur[s] = None
        return got
    shared = stream(tracks.StreamSmoother(2, lag, channels=C, lam=lam), {k: k % 2 for k in range(7)}, list(range(7)))
    for k in range(7):
        fresh = stream(tracks.StreamSmoother(1, lag, channels=C, lam=lam), {k: 0}, [k])
        assert len(shared[k]) == lengths[k]
        assert np.array_equal(_bits(np.stack(shared[k])), _bits(np.stack(fresh[k]))), k


# ------------------------------------------------------------------------------------------------------------------ bits, capture
def test_para_step_twice_and_under_graph_replay():
    """A 30-step sequence over three slots (one reset on the way), eager twice and then as one captured launch whose commands and rows
    are static tensors refilled before every replay: the same bits each time."""
    from danet_densepose2smpl_amd import tracks
    trs, _ = sc.para_tracks()
    S, lag, steps = 3, 8, 30
    seq = []
    pos = np.zeros(S, int)
    src = [1, 0, 2]                                                                          # tracks of 40, 24 and 17 rows
    for i in range(steps):
        n_new = np.array([1, 1 if i % 3 else 0, 1])
        reset = i == 17                                                                      # slot 2 has taken its 17 rows: it starts over with track 0
        if reset:
            pos[2], src[2] = 0, 0
        rows, conf = np.full((S, 1, 229), np.nan, np.float32), np.zeros((S, 1), np.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, 0], conf[s, 0] = trs[src[s]][0][pos[s]], trs[src[s]][1][pos[s]]
        pos += n_new
        seq.append((n_new, rows, conf, np.where(pos > 0, np.maximum(pos - 1 - lag, 0), -1), reset))

    def eager():
        sm = tracks.StreamSmoother(S, lag, para=True)
        outs = []
        for n_new, rows, conf, emit, reset in seq:
            if reset:
                sm.reset(2)
            out, valid = sm.step(n_new, _cu(rows), conf, emit)
            outs.append((out.cpu().numpy().copy(), valid.cpu().numpy().copy()))
        return outs
    a, b = eager(), eager()
    assert all(np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert all(np.isfinite(x[0]).all() for x in a)

    sm = tracks.StreamSmoother(S, lag, para=True)
    static_rows = torch.zeros(S, 1, 229, device='cuda')
    sm.commands(np.zeros(S, int), np.zeros((S, 1), np.float32), np.full(S, -1))              # nothing arrives, nothing is emitted:
    side = torch.cuda.Stream()                                                               # the warm-up leaves the state as it is
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            sm.launch(static_rows)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, valid = sm.launch(static_rows)
    for i, (n_new, rows, conf, emit, reset) in enumerate(seq):
        if reset:
            sm.reset(2)
        static_rows.copy_(torch.from_numpy(rows))
        sm.commands(n_new, conf, emit)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(a[i][0])) and np.array_equal(valid.cpu().numpy(), a[i][1]), i
    del g


def test_nan_in_an_observed_row_spoils_that_slot_and_channel_only():
    from danet_densepose2smpl_amd import tracks
    C, lag, lam, T = 65, 3, (0.5, 100.0), 12
    data = [sc.plain_case(C, kind, T, seed=90 + i) for i, kind in enumerate(('ones', 'mid', 'rand'))]
    bad = [(v.copy(), c) for v, c in data]
    assert bad[1][1][2] > 0
    bad[1][0][2, 17] = np.nan

    def run(d):
        sm = tracks.StreamSmoother(3, lag, channels=C, lam=lam)
        return [o for o, _, _, _ in run_plain(sm, d, [[1, 1, 1]] * T, lambda t, s: max(t - 1 - lag, 0))]
    clean, got = run(data), run(bad)
    for i in range(T):
        x = got[i].copy()
        if i >= 2:
            assert not np.isfinite(x[1, 17])
            x[1, 17] = clean[i][1, 17]
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(clean[i])), i


# ------------------------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope='module')
def demo_model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False).cuda().eval()


def clip(missing=True):
    """The six-frame clip of tests/test_gpu_tracks.py: 96 x 80, two people drifting slowly; with `missing`, person 2 has no box in
    frame 3."""
    from danet_densepose2smpl_amd import scene
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (96, 80, 3)).astype(np.uint8) for _ in range(6)]
    boxes = []
    for f in range(6):
        bs = [scene.boxes_from_xywh([4. + f, 8. + 0.5 * f, 44., 64.]), scene.boxes_from_xywh([32. - f, 20. + f, 42., 60.])]
        boxes.append(bs[:1] if missing and f == 3 else bs)
    return frames, boxes


def test_pipeline_stream_demo_end_to_end(demo_model):
    from danet_densepose2smpl_amd import video
    model = demo_model
    smpl = model.iuv2smpl.smpl
    frames, boxes = clip()
    demo = video.StreamDemo(model, smpl, 2, lag=2, box_lag=2, max_gap=2, slots=3)
    done = []
    for f in range(6):
        out = demo.push(frames[f], boxes[f])
        assert [n for n, _, _ in out] == ([f - 4] if f >= 4 else [])                         # in order, four frames late
        done += out
    rest, summary = demo.flush()
    assert [n for n, _, _ in rest] == [2, 3, 4, 5] and demo.max_held <= 5
    done += rest
    print({k: v for k, v in summary.items() if not k.endswith('tracks')}, flush=True)
    assert summary['tracks'] == 2 and summary['rows'] == 12 and summary['gap_rows'] == 1 and summary['accel_raw'] > 0 and summary['accel'] > 0
    # track ids and observed flags are VideoDemo's
    _, ref_people, _ = video.VideoDemo(model, smpl, 2, max_gap=2)(frames, boxes)
    for n, (idx, img, p) in enumerate(done):
        assert idx == n and img.shape == frames[n].shape and img.dtype == np.uint8
        assert p['track_id'].tolist() == ref_people[n]['track_id'].tolist() and p['observed'].tolist() == ref_people[n]['observed'].tolist()
        assert p['para'].shape == (2, 229) and p['para_raw'].shape == (2, 229) and p['vertices'].shape[0] == 2 and np.isfinite(p['para']).all()
        R = p['para'][:, 13:].reshape(-1, 3, 3).astype(np.float64)
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-5
        assert p['prefix_end'].tolist() == [min(n + 2, 5)] * 2
    assert done[3][2]['observed'].tolist() == [True, False]
    # every emitted row against the oracle on the recorded raw rows up to the recorded prefix end
    worst = {'cam': 0.0, 'betas': 0.0, 'rot': 0.0}
    for tid in (0, 1):
        raw = np.stack([p['para_raw'][p['track_id'].tolist().index(tid)] for _, _, p in done])
        conf = np.array([1.0 if p['observed'][p['track_id'].tolist().index(tid)] else 0.0 for _, _, p in done], np.float32)
        for n, (_, _, p) in enumerate(done):
            i = p['track_id'].tolist().index(tid)
            e = int(p['prefix_end'][i]) + 1
            ts = np.array([0, e])
            ref = to.smooth_para(raw[:e], conf[:e], ts, to.DEFAULT_LAM, True)
            dense = to.smooth_para(raw[:e], conf[:e], ts, to.DEFAULT_LAM, True, solver=to.solve_dense)
            for name, r in sc.para_ratio(p['para'][i], ref, np.abs(ref['ch'] - dense['ch']), n).items():
                worst[name] = max(worst[name], r)
    for name, w in worst.items():
        _record('pipeline', w, block=name)
    assert max(worst.values()) <= 1.0


def test_pipeline_the_gap_person_is_drawn_in_frame_3(demo_model):
    from danet_densepose2smpl_amd import video
    model = demo_model
    frames, boxes = clip()
    demo = video.StreamDemo(model, model.iuv2smpl.smpl, 2, lag=0, box_lag=2, max_gap=2)       # a delay of two: frame 3 comes out of push 5
    for f in range(6):
        out = demo.push(frames[f], boxes[f])
    (n, _, p), last = out[0], demo.last
    assert n == 3 and last['frame'] == 3 and p['observed'].tolist() == [True, False] and p['prefix_end'].tolist() == [3, 3]
    _, ids, _ = last['render_aux']
    F2 = int(demo.scene.mesh.tables(demo.scene.device, p['vertices'].shape[1]).faces2.shape[0])
    ids3 = ids.cpu().numpy()
    person = np.unique(ids3[ids3 >= 0] // F2)
    print('frame 3: people drawn %s, the gap row is person 1' % person.tolist(), flush=True)
    assert 1 in person.tolist()


def test_pipeline_without_smoothing_is_the_scene_demo(demo_model):
    from danet_densepose2smpl_amd import scene, video
    model = demo_model
    smpl = model.iuv2smpl.smpl
    frames, boxes = clip(missing=False)
    demo = video.StreamDemo(model, smpl, 2, smooth=False, lag=2, box_lag=2, max_gap=2)
    done = []
    for f in range(6):
        done += demo.push(frames[f], boxes[f])
    rest, summary = demo.flush()
    done += rest
    assert summary['gap_rows'] == 0 and len(done) == 6
    ref = scene.SceneDemo(model, smpl, 2)
    for n in range(6):
        r, p = ref(frames[n:n + 1], boxes[n:n + 1])
        assert np.array_equal(p[0]['para'].view(np.int32), done[n][2]['para'].view(np.int32)), n
        assert np.array_equal(r[0], done[n][1]), n


def test_pipeline_refusals_and_slots(demo_model):
    from danet_densepose2smpl_amd import video
    model = demo_model
    smpl = model.iuv2smpl.smpl
    with pytest.raises(ValueError):
        video.StreamDemo(model, smpl, 2, box_lag=4)                                          # below max_gap = 5
    frames, boxes = clip()
    demo = video.StreamDemo(model, smpl, 2, lag=0, box_lag=2, max_gap=2, slots=1)
    with pytest.raises(RuntimeError, match='2|slots'):
        demo.push(frames[0], boxes[0])                                                       # two tracks, one slot
    # one slot, one person at a time: the first track ends, its slot is drawn empty and serves the second
    demo = video.StreamDemo(model, smpl, 2, lag=0, box_lag=1, max_gap=1, slots=1)
    done = []
    for f in range(6):
        done += demo.push(frames[f], [boxes[f][0]] if f < 2 else ([] if f < 4 else [boxes[f][-1]]))
    rest, summary = demo.flush()
    done += rest
    assert [n for n, _, _ in done] == list(range(6)) and summary['tracks'] == 2
    assert [p['track_id'].tolist() for _, _, p in done] == [[0], [0], [], [], [1], [1]]


def test_tool_streams_the_clip(tmp_path):
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
                        str(tmp_path / 'boxes.json'), '--batch', '2', '--stream', '--lag', '2', '--box_lag', '2'], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().split('\n')[-1])
    print(line, flush=True)
    assert line['tool'] == 'demo_video' and line['stream'] is True and line['frames'] == 6 and line['tracks'] == 2 and line['rows'] == 12
    assert line['gap_rows'] == 1 and line['delay_frames'] == 4 and line['max_frames_held'] <= 5
    assert all(line['ms_per_frame'][k] > 0 for k in ('associate', 'boxes', 'infer', 'smooth', 'render', 'total'))
    assert sorted(n for n in os.listdir(str(dst)) if n.endswith('_scene.png')) == ['f%02d_scene.png' % n for n in range(6)]
    z = np.load(str(dst / 'tracks.npz'))
    assert z['track_start'].tolist() == [0, 6, 12] and z['frame'].shape == (12,) and z['det'].tolist().count(-1) == 1
    assert z['para_raw'].shape == (12, 229) and z['para'].shape == (12, 229) and z['boxes_raw'].shape == (12, 3) and z['boxes'].shape == (12, 3)
    assert z['accel_raw'].shape == (2,) and z['accel'].shape == (2,) and z['conf'].shape == (12,)
