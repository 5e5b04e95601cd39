"""The host side of the identity rule (DESIGN.md 4b'-link; tracks.candidates / link / identity_groups, the argument rules): known
answers, and the float64 oracle of tests/link_oracle.py on its recovery case with the chosen defaults.  No GPU."""
import numpy as np
import pytest
import torch

import link_oracle as lo


def trackset(spans, conf=None):
    """A TrackSet of tracks with the given (first, last) frames, every row observed."""
    from danet_densepose2smpl_amd import tracks
    lengths = [b - a + 1 for a, b in spans]
    start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    frame = np.concatenate([np.arange(a, b + 1) for a, b in spans]).astype(np.int32)
    N = int(start[-1])
    return tracks.TrackSet(start, frame, np.zeros(N, np.int32), np.ones(N, np.float32) if conf is None else conf, int(frame.max()) + 1)


def dist_of(cost, sigma_s):
    """[C,4] rows whose cost is `cost` through the shape term alone (overlap 1, d_app 0)."""
    c = np.asarray(cost, np.float64)
    return np.stack([c * sigma_s ** 2, np.zeros_like(c), np.ones_like(c), np.ones_like(c)], 1)


KW = dict(max_absence=10, sigma_s=0.5, sigma_a=0.5, min_overlap=0.1, no_app=0.5)


@pytest.fixture(scope='module')
def case():
    return lo.recovery_case()


@pytest.fixture(scope='module')
def solved(case):
    return lo.solve_case(case)


def test_candidates_honour_max_absence_on_both_sides():
    from danet_densepose2smpl_amd import tracks
    # track 0 ends at frame 9; the others start 0 (overlap), 1, 10 and 11 frames after that frame
    ts = trackset([(0, 9), (9, 12), (10, 12), (19, 20), (20, 22)])
    got = tracks.candidates(ts, 10)
    assert got.dtype == np.int32 and got.tolist() == [[0, 2], [0, 3], [1, 3], [1, 4], [2, 3], [2, 4]]
    assert np.array_equal(got, lo.candidates(ts.track_start, ts.frame, 10))
    assert tracks.candidates(ts, 1).tolist() == [[0, 2]]
    # link ignores a pair outside the window whatever it costs
    pairs = np.array([[0, 1], [0, 4], [0, 3], [3, 0]], np.int32)
    res = tracks.link(ts, dist_of([0.0, 0.0, 0.5, 0.0], 0.5), pairs, **KW)
    assert res['links'].tolist() == [[0, 3]] and res['admissible'].tolist() == [False, False, True, False]
    assert np.isinf(res['cost'][[0, 1, 3]]).all() and res['cost'][2] == 0.5
    assert res['identity'].tolist() == [0, 1, 2, 0, 3]


def test_tie_order_is_cost_then_a_then_b_and_linking_is_deterministic():
    from danet_densepose2smpl_amd import tracks
    ts = trackset([(0, 3), (0, 4), (6, 8), (7, 9)])
    pairs = np.array([[1, 3], [1, 2], [0, 3], [0, 2]], np.int32)
    # all four cost the same: (0, 2) is taken first, then (1, 3); (0, 3) and (1, 2) find their ends used
    res = tracks.link(ts, dist_of([0.25] * 4, 0.5), pairs, **KW)
    assert res['links'].tolist() == [[0, 2], [1, 3]] and res['link_cost'].tolist() == [0.25, 0.25]
    # a cheaper pair goes first whatever its indices
    res2 = tracks.link(ts, dist_of([0.2, 0.25, 0.25, 0.25], 0.5), pairs, **KW)
    assert res2['links'].tolist() == [[1, 3], [0, 2]]
    again = tracks.link(ts, dist_of([0.25] * 4, 0.5), pairs, **KW)
    for k in ('identity', 'links', 'link_cost', 'cost'):
        assert np.array_equal(res[k], again[k]), k
    # cost above 1 never links; cost exactly 1 does
    res3 = tracks.link(ts, dist_of([2.0, 2.0, 1.0, 1.0 + 1e-9], 0.5), pairs, **KW)
    assert res3['links'].tolist() == [[0, 3]]


def test_no_overlap_pairs_pay_no_app_instead_of_the_appearance_term():
    from danet_densepose2smpl_amd import tracks
    ts = trackset([(0, 3), (6, 8)])
    d = np.array([[0.05, 7.0, 0.05, 3.0]])                                   # overlap below min_overlap: d_app is not used
    res = tracks.link(ts, d, [[0, 1]], **KW)
    assert res['cost'][0] == 0.05 / 0.25 + 0.5 and res['links'].tolist() == [[0, 1]]
    d[0, 2] = 0.1                                                            # at min_overlap: the appearance term counts
    res = tracks.link(ts, d, [[0, 1]], **KW)
    assert res['cost'][0] == 0.05 / 0.25 + 7.0 / 0.25 and res['links'].shape == (0, 2) and res['identity'].tolist() == [0, 1]


def test_identity_numbering_follows_the_first_tracks_id():
    from danet_densepose2smpl_amd import tracks
    ts = trackset([(0, 2), (1, 3), (5, 6), (6, 8), (10, 11)])
    pairs = np.array([[1, 2], [2, 4], [0, 3]], np.int32)
    res = tracks.link(ts, dist_of([0.1, 0.2, 0.3], 0.5), pairs, **KW)
    assert res['links'].tolist() == [[1, 2], [2, 4], [0, 3]]
    assert res['identity'].tolist() == [0, 1, 1, 0, 1]
    g = tracks.identity_groups(ts, res['identity'])
    assert g.start.tolist() == [0, 6, 13]
    assert g.rows.tolist() == [0, 1, 2, 8, 9, 10] + [3, 4, 5, 6, 7, 11, 12]           # ascending (track id, t) inside an identity


def test_chains_on_the_recovery_case_are_injective_and_disjoint_in_time(case, solved):
    from danet_densepose2smpl_amd import tracks
    ts = tracks.TrackSet(case['track_start'], case['frame'], case['det'], case['conf'], case['n_frames'])
    rng = np.random.default_rng(5)
    first, last = lo.spans(case['track_start'], case['frame'])
    for trial in range(4):                                                   # random distances: the structure must hold whatever they are
        pairs = tracks.candidates(ts, 150 if trial < 2 else 400)
        d = np.stack([rng.uniform(0, 0.05, len(pairs)), rng.uniform(0, 0.02, len(pairs)), rng.uniform(0, 1, len(pairs)), np.ones(len(pairs))], 1)
        kw = dict(lo.DEFAULTS, max_absence=150 if trial < 2 else 400)
        res = tracks.link(ts, d, pairs, **kw)
        L = res['links']
        assert len(L) > 0
        assert len(set(L[:, 0].tolist())) == len(L) and len(set(L[:, 1].tolist())) == len(L)          # one successor, one predecessor
        assert ((first[L[:, 1]] - last[L[:, 0]] >= 1) & (first[L[:, 1]] - last[L[:, 0]] <= kw['max_absence'])).all()
        for g in range(int(res['identity'].max()) + 1):
            members = sorted(np.nonzero(res['identity'] == g)[0], key=lambda k: first[k])
            assert all(last[a] < first[b] for a, b in zip(members[:-1], members[1:]))                 # disjoint in time
        assert len(np.unique(res['identity'])) == ts.K - len(L)
        # a permutation of the candidate list changes nothing
        perm = rng.permutation(len(pairs))
        res_p = tracks.link(ts, d[perm], pairs[perm], **kw)
        for k in ('identity', 'links', 'link_cost'):
            assert np.array_equal(res[k], res_p[k]), k
        ref = lo.link(case['track_start'], case['frame'], d, pairs, **kw)
        for k in ('identity', 'links', 'link_cost', 'cost'):
            assert np.array_equal(res[k], ref[k]), k


def test_recovery_case_with_the_defaults_finds_every_link_and_none_wrong(case, solved):
    from danet_densepose2smpl_amd import tracks
    assert tracks.LINK_DEFAULTS == lo.DEFAULTS
    assert len(case['true_links']) == 6 and len(case['far_links']) == 2
    found, wrong, missed = lo.score(solved['links'], case)
    print('defaults: found %d wrong %d missed %d, costs %s' % (found, wrong, missed, solved['link_cost'].round(3).tolist()), flush=True)
    assert (found, wrong, missed) == (6, 0, 0)
    # some true pairs share no texel (front, then back) and are linked through no_app
    true_rows = [i for i, p in enumerate(solved['pairs'].tolist()) if tuple(p) in case['true_links']]
    assert (solved['dist'][true_rows, 2] < lo.DEFAULTS['min_overlap']).sum() >= 2
    # identities: tracklets of one person inside max_absence share one, the far third tracklets open their own
    ident = solved['identity']
    for a, b in case['true_links']:
        assert ident[a] == ident[b]
    for a, b in case['far_links']:
        assert ident[a] != ident[b]
    assert ident.max() + 1 == 12 - 6
    # the product's host code gives the same on the same distances
    ts = tracks.TrackSet(case['track_start'], case['frame'], case['det'], case['conf'], case['n_frames'])
    pairs = tracks.candidates(ts)
    assert np.array_equal(pairs, solved['pairs'])
    res = tracks.link(ts, solved['dist'], pairs)
    for k in ('identity', 'links', 'link_cost', 'cost'):
        assert np.array_equal(res[k], solved[k]), k


def _joins(links, case, people):
    return [(int(a), int(b)) for a, b in links if {int(case['person'][a]), int(case['person'][b])} == set(people)]


def test_both_terms_earn_their_place(case):
    """Appearance off: the two people of one shape are confused.  Shape off: the two people of one colouring are confused."""
    no_app = lo.solve_case(case, sigma_a=1e6, no_app=0.0)
    found, wrong, missed = lo.score(no_app['links'], case)
    print('appearance off: found %d wrong %d missed %d' % (found, wrong, missed), flush=True)
    assert wrong > 0 and len(_joins(no_app['links'], case, (0, 1))) > 0 and not _joins(no_app['links'], case, (2, 3))
    no_shape = lo.solve_case(case, sigma_s=1e6)
    found, wrong, missed = lo.score(no_shape['links'], case)
    print('shape off: found %d wrong %d missed %d' % (found, wrong, missed), flush=True)
    assert wrong > 0 and len(_joins(no_shape['links'], case, (2, 3))) > 0 and not _joins(no_shape['links'], case, (0, 1))


def test_share_shape_oracle_and_groups(case, solved):
    """The oracle's one shape per identity: every row of an identity holds the weighted mean, NaN gap rows are never read."""
    out, mean, status = lo.share_shape(case['para'], case['conf'], case['track_start'], solved['identity'])
    assert status.tolist() == [0] * 6 and np.isfinite(out[:, 3:13]).all()
    track = np.repeat(np.arange(12), np.diff(case['track_start']))
    for g in range(6):
        rows = np.nonzero(solved['identity'][track] == g)[0]
        assert (out[rows, 3:13] == mean[g].astype(np.float32)[None]).all()
        w = case['conf'][rows].astype(np.float64)
        ref = (w[:, None] * np.nan_to_num(case['para'][rows, 3:13].astype(np.float64))).sum(0) / w.sum()
        assert np.abs(mean[g] - ref).max() < 1e-12
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(out[:, other].view(np.int32), case['para'][:, other].view(np.int32))


def test_argument_refusals():
    from danet_densepose2smpl_amd import tracks
    ts = trackset([(0, 3), (6, 8)])
    d = np.zeros((1, 4))
    for bad in ([[0, 2]], [[-1, 1]]):
        with pytest.raises(ValueError, match=r'outside \[0, 2\)'):
            tracks.link(ts, d, bad)
        with pytest.raises(ValueError, match=r'outside \[0, 2\)'):
            tracks.affinity(torch.zeros(2, 10), torch.zeros(2, 24, 2, 2, 4), bad)
    with pytest.raises(ValueError, match='integers'):
        tracks.link(ts, d, np.zeros((1, 2)))
    with pytest.raises(ValueError, match=r'\[C,2\]'):
        tracks.link(ts, d, np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError, match='dist'):
        tracks.link(ts, np.zeros((2, 4)), [[0, 1]])
    with pytest.raises(ValueError, match='dist'):
        tracks.link(ts, np.zeros((1, 4), np.int32), [[0, 1]])
    with pytest.raises(ValueError, match='non-finite distance'):
        tracks.link(ts, np.full((1, 4), np.nan), [[0, 1]])
    with pytest.raises(ValueError, match='TrackSet'):
        tracks.link(None, d, [[0, 1]])
    for name in ('sigma_s', 'sigma_a', 'min_overlap', 'no_app'):
        for v in (float('nan'), float('inf'), -1.0):
            with pytest.raises(ValueError, match=name):
                tracks.link(ts, d, [[0, 1]], **{name: v})
    for name in ('sigma_s', 'sigma_a'):
        with pytest.raises(ValueError, match=name):
            tracks.link(ts, d, [[0, 1]], **{name: 0.0})
    for v in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match='max_absence'):
            tracks.link(ts, d, [[0, 1]], max_absence=v)
        with pytest.raises(ValueError, match='max_absence'):
            tracks.candidates(ts, v)
    # shapes and dtypes of the device ops, refused before the library is loaded and before the device is asked for
    with pytest.raises(ValueError, match='shape'):
        tracks.affinity(torch.zeros(2, 9), torch.zeros(2, 24, 2, 2, 4), [[0, 1]])
    with pytest.raises(ValueError, match='atlas'):
        tracks.affinity(torch.zeros(2, 10), torch.zeros(2, 24, 2, 3, 4), [[0, 1]])
    with pytest.raises(ValueError, match='atlas'):
        tracks.affinity(torch.zeros(2, 10), torch.zeros(3, 24, 2, 2, 4), [[0, 1]])
    with pytest.raises(ValueError, match='floating-point'):
        tracks.affinity(torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, 24, 2, 2, 4), [[0, 1]])
    with pytest.raises(ValueError, match='PairSet was made for'):
        tracks.affinity(torch.zeros(2, 10), torch.zeros(2, 24, 2, 2, 4), tracks.PairSet([[0, 1]], 3))
    with pytest.raises(ValueError, match='rows'):
        tracks.share_shape(torch.zeros(6, 229), ts, [0, 0])
    with pytest.raises(ValueError, match='identity'):
        tracks.share_shape(torch.zeros(7, 229), ts, [0, 2])
    with pytest.raises(ValueError, match='identity'):
        tracks.share_shape(torch.zeros(7, 229), ts, [0.0, 1.0])
    with pytest.raises(ValueError, match='229'):
        tracks.descriptors(torch.zeros(7, 228), ts)
    gaps = tracks.TrackSet([0, 2, 3], [0, 1, 5], [0, 0, -1], [1, 1, 0], 6)
    with pytest.raises(ValueError, match='without an observed row'):
        tracks.descriptors(torch.zeros(3, 229), gaps)
    with pytest.raises(ValueError, match='permutation'):
        tracks.RowGroups([0, 2, 3], [0, 0, 1])
    with pytest.raises(ValueError, match='ascend'):
        tracks.RowGroups([0, 2, 1, 3], [0, 1, 2])
    groups = tracks.RowGroups([0, 4, 7], np.arange(7))
    with pytest.raises(ValueError, match='columns'):
        tracks.group_mean(torch.zeros(7, 229), torch.ones(7), groups, col0=225, ncol=5)
    with pytest.raises(ValueError, match='rows'):
        tracks.group_mean(torch.zeros(6, 229), torch.ones(6), groups)
    # CPU tensors: there is no CPU path
    for call in (lambda: tracks.affinity(torch.zeros(2, 10), torch.zeros(2, 24, 2, 2, 4), [[0, 1]]),
                 lambda: tracks.descriptors(torch.zeros(7, 229), ts),
                 lambda: tracks.share_shape(torch.zeros(7, 229), ts, [0, 0]),
                 lambda: tracks.group_mean(torch.zeros(7, 229), torch.ones(7), groups)):
        with pytest.raises(RuntimeError, match='GPU only|no CPU'):
            call()


def test_stream_demo_refuses_link_and_video_demo_checks_its_thresholds():
    from danet_densepose2smpl_amd import video
    with pytest.raises(ValueError, match='finished track'):
        video.StreamDemo(None, None, 1, link=True)
    with pytest.raises(ValueError, match='sigma_s'):
        video.VideoDemo(None, None, 1, link=True, sigma_s=float('nan'))
    with pytest.raises(ValueError, match='max_absence'):
        video.VideoDemo(None, None, 1, link=True, max_absence=0)
    with pytest.raises(ValueError, match='chart size'):
        video.VideoDemo(None, None, 1, link=True, id_texture_size=1)
