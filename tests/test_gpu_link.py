"""The identity ops (csrc/track_link.hip, tracks.affinity / group_mean / descriptors / share_shape) and VideoDemo(link=True) on the
device, against the float64 restatement of the identity rule in tests/link_oracle.py.

Bound, for every number of both ops: |kernel - f64| <= 4 x 2^-23 x |f64|.  The sums are double and rounded to fp32 once (half a
rounding); the oracle sums in another order, which costs about 1e-13 relative.  A number whose float64 value is exactly 0 must be
exactly 0.  No input holds a texel weight within 1e-6 relative of w_min (asserted), so no pair is left out of a comparison.  Every
test prints measured / bound before it asserts and hands it to conftest.record.

Shapes: T in {2, 5, 8} is 96, 600 and 1 536 texels -- fewer than two waves' worth, no multiple of 64, and the default; C in
{1, 3, 4, 5, 17} leaves the last workgroup of four pairs partly empty; groups of 1, 2, 64 and 257 rows in one launch, ncol 1 and 10."""
import json
import os

import numpy as np
import pytest
import torch

import link_oracle as lo
from conftest import record

pytestmark = pytest.mark.gpu

U = 2.0 ** -23


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _record(name, ratio, **kw):
    print('%s: measured / bound = %.4f %s' % (name, ratio, kw), flush=True)
    record('link.' + name, dict(kw, ratio=round(float(ratio), 6)))


def ratio(got, ref):
    """max |got - ref| / (4 U |ref|); entries whose reference is exactly 0 must be exactly 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((np.abs(got[~zero] - ref[~zero]) / (4 * U * np.abs(ref[~zero]))).max())


# ------------------------------------------------------------------------------------------------------------------ affinity
def make_atlas(rng, T, seen=None):
    """One track's atlas [24,T,T,4]: weights 0, below w_min, between w_min and 1, exactly 1 and above 1, a fifth each; the colours
    of every texel at or below w_min are NaN (such a texel is never read whoever the partner is).  seen: a bool mask over the
    24 T T texels, outside which the weight is 0."""
    n = 24 * T * T
    kind = rng.integers(0, 5, n)
    w = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0, rng.uniform(1e-5, 9e-4, n), rng.uniform(1.1e-3, 0.999, n), 1.0],
                  rng.uniform(1.001, 6.0, n))
    if seen is not None:
        w = np.where(seen, w, 0.0)
    a = np.concatenate([rng.uniform(0, 1, (n, 3)), w[:, None]], 1).astype(np.float32)
    a[a[:, 3] <= lo.W_MIN, :3] = np.nan
    return a.reshape(24, T, T, 4)


def affinity_case(K, T, C, seed):
    """-> (shape [K,10] f32, atlas [K,24,T,T,4] f32, pairs [C,2] int32).  K = 5: tracks 3 and 4 see disjoint halves of the texels,
    so the pair (3, 4) shares none; every K: a pair (a, a)."""
    rng = np.random.default_rng(seed)
    shape = rng.normal(0, 1, (K, 10)).astype(np.float32)
    n = 24 * T * T
    half = np.arange(n) < n // 2
    seen = {3: half, 4: ~half} if K == 5 else ({1: np.arange(n) >= n // 4} if K == 2 else {})
    atlas = np.stack([make_atlas(rng, T, seen.get(k)) for k in range(K)])
    first = {1: [(0, 0)], 2: [(0, 1), (1, 1), (1, 0), (0, 0)], 5: [(3, 4), (2, 2), (0, 1), (4, 3), (1, 0), (3, 3)]}[K]
    rest = [tuple(int(v) for v in rng.integers(0, K, 2)) for _ in range(C)]
    return shape, atlas, np.array((first + rest)[:C], np.int32)


def check_affinity(shape, atlas, pairs, name):
    from danet_densepose2smpl_amd import tracks
    assert not lo.near_w_min(atlas)                                          # the cap on pairs left out of the comparison is 0
    out = tracks.affinity(_cu(shape), _cu(atlas), pairs)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = lo.pair_distance(shape, atlas, pairs)
    assert got.dtype == np.float32 and got.shape == (len(pairs), 4) and np.isfinite(got).all(), name
    for c, (a, b) in enumerate(pairs.tolist()):
        if a == b:
            assert got[c, 0] == 0 and got[c, 1] == 0, (name, c)
    return ratio(got, ref), got


@pytest.mark.parametrize('C', (1, 3, 4, 5, 17))
@pytest.mark.parametrize('T', (2, 5, 8))
@pytest.mark.parametrize('K', (1, 2, 5))
def test_affinity_against_the_oracle(K, T, C):
    shape, atlas, pairs = affinity_case(K, T, C, 1000 * K + 100 * T + C)
    r, got = check_affinity(shape, atlas, pairs, (K, T, C))
    if K == 5:
        assert pairs[0].tolist() == [3, 4] and got[0, 1] == 0 and got[0, 2] == 0 and got[0, 3] == 0        # no common texel
        assert got[0, 0] > 0
    _record('affinity', r, K=K, T=T, C=C)
    assert r <= 1.0


def test_affinity_nan_in_every_texel_that_must_not_be_read():
    """Two tracks; wherever m_x = 0 BOTH sides' colours are NaN, also on a side whose own weight is large."""
    rng = np.random.default_rng(77)
    T = 5
    shape = rng.normal(0, 1, (2, 10)).astype(np.float32)
    atlas = np.stack([make_atlas(rng, T), make_atlas(rng, T)])
    clean = np.nan_to_num(atlas)
    flat = atlas.reshape(2, -1, 4)
    dead = ~((flat[0, :, 3] > lo.W_MIN) & (flat[1, :, 3] > lo.W_MIN))
    flat[:, dead, :3] = np.nan
    assert dead.sum() > 100 and (~dead).sum() > 100
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    r, got = check_affinity(shape, atlas, pairs, 'nan')
    _, got_clean = check_affinity(shape, clean, pairs, 'clean')
    assert np.array_equal(_bits(got), _bits(got_clean))
    assert np.array_equal(_bits(got[0]), _bits(got[1]))                      # the distance is symmetric, bit for bit
    _record('affinity_nan', r, T=T)
    assert r <= 1.0


def test_affinity_weights_on_both_sides_of_w_min_and_of_one():
    """One texel per case, the rest empty: known answers."""
    from danet_densepose2smpl_amd import tracks
    T = 2
    cases = [(2e-3, 0.5, 2e-3 * 0.5, 1, 1), (9e-4, 0.5, 0.0, 0, 1), (0.5, 9e-4, 0.0, 0, 1), (3.0, 0.25, 0.25, 1, 1), (3.0, 7.0, 1.0, 1, 1),
             (1.0, 1.0, 1.0, 1, 1), (9e-4, 5e-4, 0.0, 0, 0)]
    for wa, wb, S, n, u in cases:
        atlas = np.zeros((2, 24, T, T, 4), np.float32)
        atlas[0, 7, 1, 0] = (0.25, 0.5, 0.75, wa)
        atlas[1, 7, 1, 0] = (0.75, 0.25, 0.5, wb)
        out = tracks.affinity(_cu(np.zeros((2, 10), np.float32)), _cu(atlas), [[0, 1]]).cpu().numpy()[0]
        want = [0.0, ((0.5 ** 2 + 0.25 ** 2 + 0.25 ** 2) / 3.0) if n else 0.0, float(n) / u if u else 0.0,
                float(np.float64(np.float32(wa) if wa < 1 else 1.0) * np.float64(np.float32(wb) if wb < 1 else 1.0)) if n else 0.0]
        assert ratio(out, want) <= 1.0, (wa, wb, out.tolist(), want)


def test_affinity_bits_twice_alone_and_under_graph_replay():
    from danet_densepose2smpl_amd import tracks
    K, T, C = 5, 5, 17
    shape, atlas, pairs = affinity_case(K, T, C, 31)
    shape2, atlas2, _ = affinity_case(K, T, C, 32)
    s, a = _cu(shape), _cu(atlas)
    ps = tracks.PairSet(pairs, K)
    eager = tracks.affinity(s, a, ps)
    again = tracks.affinity(s, a, ps)
    assert np.array_equal(_bits(eager), _bits(again))
    for c in range(C):                                                       # each pair alone: the same bits
        alone = tracks.affinity(s, a, pairs[c:c + 1])
        assert np.array_equal(_bits(alone[0]), _bits(eager[c])), c
    eager2 = tracks.affinity(_cu(shape2), _cu(atlas2), ps)
    assert not np.array_equal(_bits(eager), _bits(eager2))
    ss, sa = s.clone(), a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            tracks.affinity(ss, sa, ps)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = tracks.affinity(ss, sa, ps)
    for sh, at, want in ((shape2, atlas2, eager2), (shape, atlas, eager)):    # refilled inputs, one capture
        ss.copy_(_cu(sh))
        sa.copy_(_cu(at))
        static.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(static), _bits(want))
    del g
    assert tracks.affinity(s, a, np.zeros((0, 2), np.int32)).shape == (0, 4)  # C = 0: nothing is launched


# ------------------------------------------------------------------------------------------------------------------ group mean
GROUP_SIZES = (1, 2, 64, 257, 3)                                             # the last group has no weight


def group_case(seed):
    """Rows [N,229] f32, conf [N] f32 and the groups over a shuffled row order: sizes 1, 2, 64, 257 and a weightless group of 3.
    About a fifth of the rows of the weighted groups have c = 0 and are NaN all over: they must never be read."""
    rng = np.random.default_rng(seed)
    N = sum(GROUP_SIZES)
    start = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int32)
    order = rng.permutation(N).astype(np.int32)
    rows = (rng.normal(0, 1, (N, 229)) * rng.uniform(0.1, 3.0, 229) + rng.normal(0, 2, 229)).astype(np.float32)
    conf = rng.uniform(0.2, 1.0, N).astype(np.float32)
    for g, n in enumerate(GROUP_SIZES):
        members = order[start[g]:start[g + 1]]
        if g == len(GROUP_SIZES) - 1:
            conf[members] = 0.0
        elif n > 2:
            off = members[rng.uniform(size=n) < 0.2]
            conf[off] = 0.0
            rows[off] = np.nan
    return rows, conf, start, order


def group_oracle(rows, conf, start, order, col0, ncol):
    G = len(start) - 1
    mean, status = np.zeros((G, ncol)), np.zeros(G, np.int32)
    for g in range(G):
        members = order[start[g]:start[g + 1]]
        m, sc = lo.weighted_mean(rows[members, col0:col0 + ncol], conf[members])
        if sc > 0:
            mean[g] = m
        else:
            status[g] = 1
    return mean, status


@pytest.mark.parametrize('write_back', (False, True))
@pytest.mark.parametrize('col0,ncol', ((3, 10), (0, 1), (228, 1), (13, 10)))
def test_group_mean_against_the_oracle(col0, ncol, write_back):
    from danet_densepose2smpl_amd import tracks
    rows, conf, start, order = group_case(10 * col0 + ncol)
    groups = tracks.RowGroups(start, order)
    x = _cu(rows)
    mean, status = tracks.group_mean(x, _cu(conf), groups, col0, ncol, write_back)
    torch.cuda.synchronize()
    ref, st_ref = group_oracle(rows, conf, start, order, col0, ncol)
    assert status.cpu().tolist() == st_ref.tolist() == [0, 0, 0, 0, 1]
    r = ratio(mean.cpu().numpy(), ref)
    _record('group_mean', r, col0=col0, ncol=ncol, write_back=write_back)
    assert r <= 1.0
    after = x.cpu().numpy()
    want = rows.copy()
    if write_back:
        m32 = mean.cpu().numpy()
        for g in range(len(GROUP_SIZES) - 1):                                # the weightless group keeps its rows bit for bit
            want[order[start[g]:start[g + 1]], col0:col0 + ncol] = m32[g][None]
    assert np.array_equal(_bits(after), _bits(want))


def test_group_mean_bits_twice_alone_and_under_graph_replay():
    from danet_densepose2smpl_amd import tracks
    rows, conf, start, order = group_case(5)
    rows2 = np.where(np.isnan(rows), np.nan, np.nan_to_num(group_case(6)[0], nan=1.0)).astype(np.float32)      # other values, the same NaN rows
    groups = tracks.RowGroups(start, order)
    c = _cu(conf)

    def run(r):
        x = _cu(r)
        m, st = tracks.group_mean(x, c, groups, 3, 10, True)
        return x, m, st
    x1, m1, st1 = run(rows)
    x1b, m1b, _ = run(rows)
    assert np.array_equal(_bits(x1), _bits(x1b)) and np.array_equal(_bits(m1), _bits(m1b))
    x2, m2, _ = run(rows2)
    for g in range(len(GROUP_SIZES)):                                        # each group alone: the same bits
        members = order[start[g]:start[g + 1]]
        xa = _cu(rows[members])
        ma, sa = tracks.group_mean(xa, _cu(conf[members]), tracks.RowGroups([0, len(members)], np.arange(len(members))), 3, 10, True)
        assert np.array_equal(_bits(ma[0]), _bits(m1[g])) and sa.cpu().tolist() == [st1.cpu().tolist()[g]], g
        assert np.array_equal(_bits(xa), _bits(x1.cpu().numpy()[members])), g
    static = _cu(rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            tracks.group_mean(static, c, groups, 3, 10, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sm, sst = tracks.group_mean(static, c, groups, 3, 10, True)
    for r, wx, wm in ((rows2, x2, m2), (rows, x1, m1)):                       # refilled inputs, one capture
        static.copy_(_cu(r))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(static), _bits(wx)) and np.array_equal(_bits(sm), _bits(wm)) and torch.equal(sst, st1)
    del g
    empty = tracks.group_mean(torch.zeros(0, 229, device='cuda'), torch.zeros(0, device='cuda'), tracks.RowGroups([0], np.zeros(0, np.int32)))
    assert empty[0].shape == (0, 10) and empty[1].shape == (0,)               # G = 0, N = 0: nothing is launched


def test_recovery_case_on_the_device():
    """descriptors, affinity, link and share_shape on the oracle's recovery case: the oracle's numbers within the bound, its links
    and identities exactly, one shape per identity."""
    from danet_densepose2smpl_amd import tracks
    case = lo.recovery_case()
    ref = lo.solve_case(case)
    ts = tracks.TrackSet(case['track_start'], case['frame'], case['det'], case['conf'], case['n_frames'])
    rows_seen = {}

    def builder(obs, off):
        rows_seen['obs'], rows_seen['off'] = obs, off
        return _cu(case['atlas'])
    para = _cu(case['para'])
    shape, atlas, status = tracks.descriptors(para, ts, builder)
    obs_ref, off_ref = lo.observed_views(case['det'], case['track_start'])
    assert np.array_equal(rows_seen['obs'], obs_ref) and np.array_equal(rows_seen['off'], off_ref) and status.cpu().tolist() == [0] * 12
    shape64, _ = lo.shape_descriptors(case['para'], case['conf'], case['track_start'])
    r_shape = ratio(shape.cpu().numpy(), shape64)
    pairs = tracks.candidates(ts)
    assert np.array_equal(pairs, ref['pairs']) and not lo.near_w_min(case['atlas'])
    dist = tracks.affinity(shape, atlas, pairs)
    r_dist = ratio(dist.cpu().numpy(), lo.pair_distance(shape.cpu().numpy(), case['atlas'], pairs))
    _record('recovery', max(r_shape, r_dist), shape=round(r_shape, 4), dist=round(r_dist, 4))
    assert r_shape <= 1.0 and r_dist <= 1.0
    res = tracks.link(ts, dist, pairs)
    assert np.array_equal(res['identity'], ref['identity']) and np.array_equal(res['links'], ref['links'])
    assert lo.score(res['links'], case) == (6, 0, 0)
    out, mean, st = tracks.share_shape(para, ts, res['identity'])
    out_ref, mean_ref, st_ref = lo.share_shape(case['para'], case['conf'], case['track_start'], ref['identity'])
    assert st.cpu().tolist() == st_ref.tolist()
    r_mean = ratio(mean.cpu().numpy(), mean_ref)
    _record('recovery_share_shape', r_mean)
    assert r_mean <= 1.0
    got = out.cpu().numpy()
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(_bits(got[:, other]), _bits(case['para'][:, other]))                     # NaN gap rows stay as they were elsewhere
    assert np.array_equal(_bits(got[:, 3:13]), _bits(mean.cpu().numpy()[res['identity'][ts.track]]))
    assert np.array_equal(_bits(para), _bits(case['para']))                                        # the input is not touched


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def demo_model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False).cuda().eval()


PRESENT = (0, 1, 2, 3, 11, 12, 13)                                           # both people are away for seven frames, max_gap is 5


def clip():
    """Fourteen frames of 96 x 80: the left half one flat colour, the right half another, a person in each half in flat-coloured
    clothing that fills their box.  Both leave after frame 3 and come back in frame 11."""
    from danet_densepose2smpl_amd import scene
    frames, boxes = [], []
    for f in range(14):
        img = np.zeros((96, 80, 3), np.uint8)
        img[:, :40] = (210, 40, 50)
        img[:, 40:] = (40, 70, 220)
        frames.append(img)
        boxes.append([scene.boxes_from_xywh([2. + 0.25 * f, 20. + 0.5 * f, 34., 56.]), scene.boxes_from_xywh([44. - 0.25 * f, 16. + 0.5 * f, 32., 60.])]
                     if f in PRESENT else [])
    return frames, boxes


@pytest.fixture(scope='module')
def linked(demo_model):
    from danet_densepose2smpl_amd import video
    frames, boxes = clip()
    demo = video.VideoDemo(demo_model, demo_model.iuv2smpl.smpl, 2, link=True)
    rendered, people, summary = demo(frames, boxes)
    return demo, rendered, people, summary


def test_video_demo_links_two_people_who_leave_and_come_back(linked):
    demo, rendered, people, summary = linked
    last = demo.last
    ts, lk = last['tracks'], last['link']
    print(summary, flush=True)
    assert summary['tracks'] == 4 and summary['rows'] == 14 and summary['gap_rows'] == 0
    rows = lk['rows'].cpu().numpy()
    conf = ts.conf
    atlas = lk['atlas'].cpu().numpy()
    assert atlas.shape == (4, 24, 8, 8, 4) and not lo.near_w_min(atlas)
    # the oracle on the recorded rows and atlases
    shape64, _ = lo.shape_descriptors(rows, conf, ts.track_start)
    r_shape = ratio(lk['shape'].cpu().numpy(), shape64)
    pairs = lo.candidates(ts.track_start, ts.frame, lo.DEFAULTS['max_absence'])
    assert np.array_equal(pairs, lk['pairs']) and pairs.tolist() == [[0, 2], [0, 3], [1, 2], [1, 3]]
    dist64 = lo.pair_distance(lk['shape'].cpu().numpy(), atlas, pairs)
    r_dist = ratio(lk['dist'], dist64)
    print('pairs %s\ndist (d_shape, d_app, overlap, S)\n%s\nspread of the betas over the tracks %s' % (
        pairs.tolist(), lk['dist'], np.abs(shape64 - shape64.mean(0)).max(0).round(5).tolist()), flush=True)
    _record('video', max(r_shape, r_dist), shape=round(r_shape, 4), dist=round(r_dist, 4))
    assert r_shape <= 1.0 and r_dist <= 1.0
    ref = lo.link(ts.track_start, ts.frame, dist64.astype(np.float32), pairs, **lo.DEFAULTS)
    assert np.array_equal(last['identity'], ref['identity']) and np.array_equal(last['links'], ref['links'])
    assert np.array_equal(last['link_cost'], ref['link_cost'])
    # each person keeps their identity across the absence
    assert last['identity'].tolist() == [0, 1, 0, 1] and last['links'].tolist() in ([[0, 2], [1, 3]], [[1, 3], [0, 2]])
    assert summary['identities'] == 2 and summary['links'] == 2
    # one shape per identity, the oracle's
    out_ref, mean_ref, st_ref = lo.share_shape(rows, conf, ts.track_start, ref['identity'])
    assert st_ref.tolist() == [0, 0]
    para = last['para']
    r_share = ratio(para[:, 3:13], mean_ref[ref['identity'][ts.track]])
    assert np.array_equal(out_ref[:, 3:13], mean_ref[ref['identity'][ts.track]].astype(np.float32))
    _record('video_share_shape', r_share)
    assert r_share <= 1.0
    for g in (0, 1):
        b = para[last['identity'][ts.track] == g, 3:13]
        assert (b == b[0]).all()
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(_bits(para[:, other]), _bits(rows[:, other]))
    for f, p in enumerate(people):
        assert p['identity'].tolist() == ([0, 1] if f in PRESENT else [])
        assert p['identity'].tolist() == last['identity'][p['track_id']].tolist()
    assert [r.shape for r in rendered] == [(96, 80, 3)] * 14


def test_video_demo_without_link_is_what_it_was(demo_model, linked):
    from danet_densepose2smpl_amd import video
    frames, boxes = clip()
    smpl = demo_model.iuv2smpl.smpl
    plain = video.VideoDemo(demo_model, smpl, 2)
    r0, p0, s0 = plain(frames, boxes)
    off = video.VideoDemo(demo_model, smpl, 2, link=False)
    r1, p1, s1 = off(frames, boxes)
    assert sorted(s0) == sorted(s1) and 'identities' not in s1 and 'identity' not in p1[0] and 'identity' not in off.last
    assert sorted(plain.last) == sorted(off.last)
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b)
    for a, b in zip(p0, p1):
        assert sorted(a) == sorted(b) and np.array_equal(_bits(a['para']), _bits(b['para']))
    for k in ('para', 'para_raw', 'boxes', 'boxes_raw'):
        assert np.array_equal(_bits(plain.last[k]), _bits(off.last[k])), k
    for k, v in plain.last['tracks'].arrays().items():
        assert np.array_equal(v, off.last['tracks'].arrays()[k]), k
    # linking touches the shape columns alone: with link=True everything else of the rows is what it is without
    demo = linked[0]
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(_bits(demo.last['para'][:, other]), _bits(plain.last['para'][:, other]))
    assert np.array_equal(_bits(demo.last['para_raw']), _bits(plain.last['para_raw']))


def test_tool_with_link_writes_identities_and_refuses_stream(tmp_path):
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
    tool = [sys.executable, os.path.join(ROOT, 'tools', 'demo_video.py'), '--frames_dir', str(src), '--out_dir', str(dst), '--boxes',
            str(tmp_path / 'boxes.json'), '--batch', '2', '--link']
    r = subprocess.run(tool + ['--stream'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and 'finished track' in r.stderr and not os.path.exists(str(dst / 'tracks.npz'))
    r = subprocess.run(tool + ['--max_absence', '20'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().split('\n')[-1])
    print(line, flush=True)
    assert line['tool'] == 'demo_video' and line['frames'] == 14 and line['tracks'] == 4 and line['rows'] == 14
    assert line['link'] is True and line['identities'] == 2 and line['links'] == 2 and line['max_absence'] == 20 and line['id_texture_size'] == 8
    assert all(line['ms_per_frame'][k] > 0 for k in ('associate', 'boxes', 'prepare', 'infer', 'smooth', 'link', 'render'))
    z = np.load(str(dst / 'tracks.npz'))
    assert z['identity'].tolist() == [0, 1, 0, 1] and z['identity'].dtype == np.int32
    assert z['links'].shape == (2, 2) and z['links'].dtype == np.int32 and z['link_cost'].shape == (2,) and z['link_cost'].dtype == np.float64
    assert z['para'].shape == (14, 229) and z['track_start'].tolist() == [0, 4, 8, 11, 14]
