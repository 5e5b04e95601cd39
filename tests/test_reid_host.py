"""The host side of the causal identity rule (DESIGN.md 4b'-reid; tracks.OnlineLinker, the argument rules of tracks.StreamDescriptor and
video.StreamDemo(reid=True)) against the float64 restatement of tests/reid_oracle.py, and the table the online defaults were chosen
from.  No GPU."""
import numpy as np
import pytest
import torch

import link_oracle as lo
import reid_oracle as ro
import texture_oracle as to

SEEDS = (0, 1, 2)


@pytest.fixture(scope='module')
def cases():
    return [ro.recovery_case(s) for s in SEEDS]


def run_linker(case, rows, gallery=64, **kw):
    """tracks.OnlineLinker driven frame by frame over a recovery case, the distances from the float64 oracle (rounded to fp32 once, as
    the device hands them over) -> (identity, links, link_cost, the most entries the gallery held)."""
    from danet_densepose2smpl_amd import tracks
    first, last = case['first'], case['last']
    K = len(first)
    final = [ro.descriptor(case, k) for k in range(K)]
    heads = [ro.descriptor(case, k, rows) for k in range(K)]
    lk = tracks.OnlineLinker(gallery, **dict(ro.DEFAULTS, **kw))
    peak = 0
    for d in range(int(first.min()), int(last.max()) + 1):
        born = [b for b in range(K) if first[b] == d]
        cand = lk.candidates(d, born)
        if born:
            shape = np.stack([final[k][0] for k in range(K)])
            atlas = np.stack([final[k][1] for k in range(K)])
            for b in born:
                shape[b], atlas[b] = heads[b][:2]
            dist = lo.pair_distance(shape, atlas, np.array([(a, b) for a, _, b in cand]).reshape(-1, 2)).astype(np.float32)
            lk.decide(d, born, cand, dist)
        for a in range(K):
            if last[a] == d:
                lk.retire(a, d)
        peak = max(peak, len(lk.entries))
    return lk.arrays(K) + (peak,)


def test_unbounded_heads_give_the_offline_links(cases):
    """With the whole track as its head the causal rule decides on the offline rule's descriptors: the same links, the same numbers."""
    for case in cases:
        off = lo.solve_case(case)
        res = ro.solve_case(case, rows=None, **lo.DEFAULTS)
        assert sorted(map(tuple, res['links'].tolist())) == sorted(map(tuple, off['links'].tolist()))
        assert np.array_equal(res['identity'], off['identity']) and lo.score(res['links'], case) == (6, 0, 0)
        ident, links, cost, _ = run_linker(case, None, **lo.DEFAULTS)
        assert np.array_equal(ident, res['identity']) and np.array_equal(links, res['links']) and np.array_equal(cost, res['link_cost'])


def test_sweep_table_and_the_chosen_defaults(cases):
    from danet_densepose2smpl_amd import tracks, video
    assert tracks.REID_DEFAULTS == ro.DEFAULTS and video.STREAM_LAG == ro.LAG
    table = ro.sweep(SEEDS)
    print('sigma_s sigma_a no_app | heads of %d rows | heads of 5 rows   (found / wrong / missed over seeds 0-2, 18 true links)' % (ro.LAG + 1))
    clean = {}
    for kw, res in table:
        print('%7.2f %7.2f %6.2f | %2d / %d / %d       | %2d / %d / %d' % ((kw['sigma_s'], kw['sigma_a'], kw['no_app']) + res[ro.LAG + 1] + res[5]),
              flush=True)
        clean[(kw['sigma_s'], kw['sigma_a'], kw['no_app'])] = res[ro.LAG + 1] == (18, 0, 0) and res[5] == (18, 0, 0)
    d = ro.DEFAULTS
    assert clean[(d['sigma_s'], d['sigma_a'], d['no_app'])]
    # room on both sides: the neighbours of the chosen row in the table are clean too
    for key in ((0.5, d['sigma_a'], d['no_app']), (d['sigma_s'], 0.15, d['no_app']), (d['sigma_s'], 0.3, d['no_app']), (d['sigma_s'], d['sigma_a'], 0.75)):
        assert clean[key], key
    # the offline defaults are not the online ones: at heads of nine rows they take one wrong link
    off = dict((tuple(kw[k] for k in ('sigma_s', 'sigma_a', 'no_app')), res) for kw, res in table)[(0.3, 0.15, 0.5)]
    assert off[ro.LAG + 1] == (17, 1, 1) and off[5] == (18, 0, 0)
    # each seed on its own, through the product's host code
    for case in cases:
        for rows in (ro.LAG + 1, 5):
            ident, links, cost, _ = run_linker(case, rows)
            ref = ro.solve_case(case, rows)
            assert lo.score(links, case) == (6, 0, 0)
            assert np.array_equal(ident, ref['identity']) and np.array_equal(links, ref['links']) and np.array_equal(cost, ref['link_cost'])


def test_chains_are_time_ordered_and_disjoint_and_the_window_holds(cases):
    case = cases[0]
    first, last = case['first'], case['last']
    for kw in ({}, {'max_absence': 400}, {'max_absence': 100}, {'sigma_s': 50.0, 'sigma_a': 50.0}):      # the last links whatever it can
        A = dict(ro.DEFAULTS, **kw)['max_absence']
        ident, links, cost, _ = run_linker(case, ro.LAG + 1, **kw)
        assert len(links) > 0 and len(set(links[:, 0].tolist())) == len(links) and len(set(links[:, 1].tolist())) == len(links)
        gap = first[links[:, 1]] - last[links[:, 0]]
        assert ((gap >= 1) & (gap <= A)).all()                               # a pair outside the window never links
        assert (cost <= 1.0).all()
        for g in range(int(ident.max()) + 1):
            members = sorted(np.nonzero(ident == g)[0], key=lambda k: first[k])
            assert all(last[a] < first[b] for a, b in zip(members[:-1], members[1:]))
        assert len(np.unique(ident)) == len(ident) - len(links) and ident.max() + 1 == len(np.unique(ident))
        born = np.array([k for k in range(len(ident)) if k not in set(links[:, 1].tolist())])
        assert ident[born].tolist() == list(range(len(born)))               # numbers ascend with (first frame, track id)
    ident, links, _, _ = run_linker(case, ro.LAG + 1, max_absence=100)
    far = [(a, b) for a, b in case['true_links'] if first[b] - last[a] > 100]
    assert far and all(ident[a] != ident[b] for a, b in far)


def test_eviction_changes_no_decision_and_overflow_raises(cases):
    from danet_densepose2smpl_amd import tracks
    for case in cases:
        for kw in ({}, {'max_absence': 100}):
            bounded = ro.solve_case(case, gallery=64, **kw)
            free = ro.solve_case(case, gallery=None, **kw)
            for k in ('identity', 'links', 'link_cost', 'carry', 'tot'):
                assert np.array_equal(bounded[k], free[k]), k
            ident, links, cost, peak = run_linker(case, ro.LAG + 1, **kw)
            assert np.array_equal(ident, free['identity']) and np.array_equal(links, free['links']) and np.array_equal(cost, free['link_cost'])
            assert peak <= bounded['peak'] <= free['peak']
    peak = run_linker(cases[0], ro.LAG + 1)[3]
    run_linker(cases[0], ro.LAG + 1, gallery=peak)                            # exactly enough
    with pytest.raises(RuntimeError, match=r'%d finished tracks wait in the gallery and frame \d+ retires another; the gallery holds %d' % (peak - 1, peak - 1)):
        run_linker(cases[0], ro.LAG + 1, gallery=peak - 1)
    lk = tracks.OnlineLinker(2, max_absence=5)
    lk.decide(0, [0, 1], lk.candidates(0, [0, 1]), np.zeros((0, 4)))
    assert lk.retire(0, 3) == 0 and lk.retire(1, 4) == 1
    assert lk.candidates(9, [2]) == [(1, 1, 2)] and sorted(lk.entries) == [1]       # track 0 has been away for six frames: gone


def test_carry_arithmetic_of_the_oracle(cases):
    """tot = carry + own sums along a chain, in the chain's order; the carried shape is the weighted mean over the chain so far."""
    case = cases[0]
    res = ro.solve_case(case)
    for a, b in res['links']:
        assert np.array_equal(res['carry'][b], res['tot'][a])
    for k in range(len(res['identity'])):
        own = ro.descriptor(case, k)[2]
        assert np.array_equal(res['tot'][k], res['carry'][k] + own)
    a, b = res['links'][0]
    sy, sc = ro.shape_sums(case['para'][case['track_start'][b]:case['track_start'][b] + 4, 3:13], case['conf'][case['track_start'][b]:case['track_start'][b] + 4])
    got = ro.carried_shape(res['carry'][b], sy, sc)
    rows = np.concatenate([np.arange(case['track_start'][a], case['track_start'][a + 1]), case['track_start'][b] + np.arange(4)])
    w = case['conf'][rows].astype(np.float64)
    ref = (w[:, None] * np.nan_to_num(case['para'][rows, 3:13].astype(np.float64))).sum(0) / w.sum()
    assert got.dtype == np.float32 and np.abs(got - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    assert ro.carried_shape(np.zeros(11), np.zeros(10), 0.0) is None


def _step_args(P=2, H=8, NV=12, device='cpu'):
    z = lambda *s: torch.zeros(*s, device=device)                             # noqa: E731
    return [z(P, 3, H, H), z(P, NV, 3), z(P, 3), z(P, H, H), z(P, 229), z(P)]


def test_every_refusal_comes_before_the_library_is_loaded(monkeypatch):
    from danet_densepose2smpl_amd import _lib, tracks, video
    from danet_densepose2smpl_amd.texture import TextureAtlas

    def loaded():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', loaded)
    tex = TextureAtlas(densepose=to.ico_densepose(), size=4)
    for kw, name in (({'slots': 0}, 'slots'), ({'slots': 2.5}, 'slots'), ({'gallery': -1}, 'gallery'), ({'texture': None}, 'TextureAtlas')):
        with pytest.raises(ValueError, match=name):
            tracks.StreamDescriptor(**dict({'slots': 3, 'gallery': 2, 'texture': tex}, **kw))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        tracks.StreamDescriptor(3, 2, tex, device='cpu')
    sd = tracks.StreamDescriptor(3, 2, tex)
    assert sd.R == 5 and sd.head_row(1) == 3
    for slot, name in (([0, 0], 'twice'), ([0, 3], r'-1\.\.2'), ([-2, 0], r'-1\.\.2'), ([0.0, 1.0], 'integers'), ([0], r'\[1\] integers|shape')):
        with pytest.raises(ValueError, match=name):
            sd.step(*_step_args(), slot, [1, 1])
    with pytest.raises(ValueError, match='observed'):
        sd.step(*_step_args(), [0, 1], [1, 2])
    with pytest.raises(ValueError, match='observed'):
        sd.commands([0, 1], [1])
    for i, name in ((0, 'images'), (1, 'vertices'), (2, 'cam'), (3, 'depth'), (4, 'para'), (5, 'conf')):
        bad = _step_args()
        bad[i] = bad[i][:1] if i != 4 else bad[i][:, :228]
        with pytest.raises(ValueError, match=name):
            sd.step(*bad, [0, 1], [1, 0])
        bad = _step_args()
        bad[i] = bad[i].to(torch.int32)
        with pytest.raises(ValueError, match='floating-point'):
            sd.step(*bad, [0, 1], [1, 0])
    with pytest.raises(ValueError, match='square'):
        sd.step(torch.zeros(2, 3, 8, 9), *_step_args()[1:], [0, 1], [1, 0])
    with pytest.raises(ValueError, match='12 mesh vertices'):
        sd.step(*(_step_args(NV=11)), [0, 1], [1, 0])
    sd.reset(2)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):                # CPU tensors: there is no CPU path
        sd.step(*_step_args(), [0, -1], [1, 0])
    assert sd.state is None and sd._reset.tolist() == [0, 0, 1]              # a refused step changes nothing
    with pytest.raises(ValueError, match='slot'):
        sd.reset(3)
    for slots, rows, name in (([0, 1], [2, 2], 'twice'), ([3], [0], 'slots'), ([0], [5], 'rows'), ([0, 1], [0], 'rows')):
        with pytest.raises(ValueError, match=name):
            sd.read(slots, rows)
    carry = torch.zeros(2, 11, dtype=torch.float64)
    for args, name in (((torch.zeros(2, 228), [0, 1], carry, [1, 1]), '229'), ((torch.zeros(2, 229), [0, 3], carry, [1, 1]), 'slot'),
                       ((torch.zeros(2, 229), [0, 1], carry, [1, 2]), 'use'), ((torch.zeros(2, 229), [0, 1], carry.float(), [1, 1]), 'float64'),
                       ((torch.zeros(2, 229), [0, 1], carry[:1], [1, 1]), 'carry')):
        with pytest.raises(ValueError, match=name):
            sd.apply_shape(*args)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        sd.apply_shape(torch.zeros(2, 229), [0, 1], carry, [1, 1])
    # the linker
    for kw, name in (({'gallery': 0}, 'gallery'), ({'max_absence': 0}, 'max_absence'), ({'sigma_s': 0.0}, 'sigma_s'), ({'sigma_a': float('nan')}, 'sigma_a'),
                     ({'min_overlap': -1.0}, 'min_overlap'), ({'no_app': float('inf')}, 'no_app')):
        with pytest.raises(ValueError, match=name):
            tracks.OnlineLinker(**kw)
    lk = tracks.OnlineLinker(2)
    assert lk.thr == tracks.REID_DEFAULTS
    lk.decide(0, [0], [], np.zeros((0, 4)))
    with pytest.raises(ValueError, match='decided once'):
        lk.decide(1, [0], [], np.zeros((0, 4)))
    with pytest.raises(ValueError, match='has not been decided'):
        lk.retire(5, 3)
    lk.retire(0, 2)
    cand = lk.candidates(4, [1])
    assert cand == [(0, 0, 1)]
    with pytest.raises(ValueError, match='dist'):
        lk.decide(4, [1], cand, np.zeros((2, 4)))
    with pytest.raises(ValueError, match='non-finite'):
        lk.decide(4, [1], cand, np.full((1, 4), np.nan))
    assert lk.identity == {0: 0} and lk.links == []                           # a refused decision changes nothing
    # the demo: refused before the model, the scene or the library is touched
    for kw, name in (({'gallery': 0}, 'gallery'), ({'max_absence': 0}, 'max_absence'), ({'id_texture_size': 1}, 'chart size'),
                     ({'sigma_s': -1.0}, 'sigma_s'), ({'sigma_a': 0.0}, 'sigma_a'), ({'min_overlap': float('nan')}, 'min_overlap'),
                     ({'no_app': -0.5}, 'no_app')):
        with pytest.raises(ValueError, match=name):
            video.StreamDemo(None, None, 1, reid=True, **kw)
    thr, T, G = video.StreamDemo.check_reid_arguments()
    assert thr == tracks.REID_DEFAULTS and T == tracks.ID_TEXTURE_SIZE == 8 and G == tracks.REID_GALLERY == 64


def test_stream_demo_still_refuses_link():
    from danet_densepose2smpl_amd import video
    with pytest.raises(ValueError, match='finished track'):
        video.StreamDemo.check_arguments(8, 8, 32, 5, 0.0, link=True)
    with pytest.raises(ValueError, match='finished track'):
        video.StreamDemo(None, None, 1, link=True, reid=True)
    assert 'reid=True' in video.NO_STREAM_LINK and video.NO_STREAM_LINK.index('finished track') < video.NO_STREAM_LINK.index('reid=True')
    video.StreamDemo.check_arguments(8, 8, 32, 5, 0.0)
