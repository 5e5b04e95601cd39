"""The online descriptor (csrc/track_reid.hip, tracks.StreamDescriptor) and StreamDemo(reid=True) on the device.

The descriptor: after every step read() must equal, bit for bit, what the ops the project already has give on the rows seen so far --
texture.TextureAtlas.unwrap over the slot's observed rows and tracks.descriptors' shape over all its rows -- and hold, against the
float64 oracles, the bounds those ops have in test_gpu_texture.py (observed flags equal on certain texels, weights within 1e-5
relative, colours within texture_oracle.bounds()['DELTA']) and test_gpu_link.py (|kernel - f64| <= 4 x 2^-23 x |f64|, an exact 0
exactly 0).  Shapes: the icosahedron topology and the H = 64 views of tests/texture_oracle.py, T in {2, 5, 8} (96, 600 and 1 536
texels: less than one workgroup, no multiple of 256, several workgroups), S = 3 slots, chunks of P = 3 people.

The stream (nine frames; `obs` an observed row, `gap0` a gap row with c = 0, `gapc` a gap row with c = 0.25):
slot 0 holds track A, observed in frames 0, 1, 3 (a view that leaves the frame in part), 5 and 7 (a view wholly outside the frame:
it moves the shape and not one texel) with gap rows between, then is reset in
frame 8 by the step that brings track D's first row; slot 1 holds track B (one observed row and a gap row), is reset in frame 2 by
a step that brings it no row, and is reused by track C (two observed rows) from frame 3; slot 2 stays empty."""
import json
import os

import numpy as np
import pytest
import torch

import link_oracle as lo
import reid_oracle as ro
import texture_oracle as to
from conftest import record

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
W_REL = 1e-5
S, G, P = 3, 2, 3
VIEWS = to.VIEWS + (to.VIEWS[0],)
CAMS = to.CAMS + ((3.0, 9.0, 0.85),)                                         # the fifth camera puts the whole body outside the frame
# per frame: the resets, then the chunk's entries (slot, track, kind, view) or None
FRAMES = (
    ((), ((0, 'A', 'obs', 0), (1, 'B', 'obs', 1), None)),
    ((), (None, (1, 'B', 'gapc', 0), (0, 'A', 'obs', 1))),
    ((1,), ((0, 'A', 'gap0', 0), None, None)),
    ((), ((1, 'C', 'obs', 2), (0, 'A', 'obs', 3), None)),
    ((), ((0, 'A', 'gapc', 0), (1, 'C', 'gap0', 0), None)),
    ((), ((1, 'C', 'obs', 0), None, (0, 'A', 'obs', 2))),
    ((), ((0, 'A', 'gap0', 0), None, None)),
    ((), ((0, 'A', 'obs', 4), None, None)),
    ((0,), (None, (0, 'D', 'obs', 1), None)),
)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _record(name, ratio, **kw):
    print('%s: measured / bound = %.4f %s' % (name, ratio, kw), flush=True)
    record('reid.' + name, dict(kw, ratio=round(float(ratio), 6)))


def ratio(got, ref):
    """max |got - ref| / (4 U |ref|); entries whose reference is exactly 0 must be exactly 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((np.abs(got[~zero] - ref[~zero]) / (4 * U * np.abs(ref[~zero]))).max())


def make_stream(seed=3, poison=False):
    """-> per frame dict(reset, slot [P], observed [P], track [P], images [P,3,H,H], vertices [P,12,3], cam [P,3], para [P,229],
    conf [P]).  poison: NaN in the image and mesh of every gap row and empty entry, and in the para of every row with c = 0 (the depth
    plane of those entries is made NaN by the caller)."""
    rng = np.random.default_rng(seed)
    v0, _ = to.ico_mesh()
    out = []
    for resets, entries in FRAMES:
        fr = {'reset': list(resets), 'slot': np.full(P, -1, np.int32), 'observed': np.zeros(P, np.int32), 'track': [None] * P,
              'images': np.zeros((P, 3, to.H, to.H), np.float32), 'vertices': np.zeros((P, 12, 3), np.float32),
              'cam': np.ones((P, 3), np.float32), 'para': np.zeros((P, 229), np.float32), 'conf': np.zeros(P, np.float32)}
        for p, e in enumerate(entries):
            img, para, c_obs = rng.random((3, to.H, to.H)).astype(np.float32), rng.normal(0, 1, 229).astype(np.float32), rng.uniform(0.3, 1.0)
            if e is not None:
                s, k, kind, view = e
                fr['slot'][p], fr['track'][p] = s, k
                fr['observed'][p] = kind == 'obs'
                fr['conf'][p] = {'obs': c_obs, 'gapc': 0.25, 'gap0': 0.0}[kind]
                fr['images'][p], fr['para'][p] = img, para
                fr['vertices'][p] = (v0.astype(np.float64) @ to.rot_xyz(*VIEWS[view]).T).astype(np.float32)
                fr['cam'][p] = CAMS[view]
            if poison and (e is None or e[2] != 'obs'):
                fr['images'][p], fr['vertices'][p], fr['cam'][p] = np.nan, np.nan, np.nan
            if poison and fr['conf'][p] == 0:
                fr['para'][p] = np.nan
        out.append(fr)
    return out


def feed(sd, fr, clean=None):
    """One step; the depth planes come from the clean twin of a poisoned frame and are poisoned where the frame is."""
    src = fr if clean is None else clean
    depth = sd.depth_planes(_cu(src['vertices']), _cu(src['cam']), to.H)
    if clean is not None:
        depth = torch.where(_cu(fr['observed']).bool()[:, None, None], depth, torch.full_like(depth, float('nan')))
    for s in fr['reset']:
        sd.reset(s)
    sd.step(_cu(fr['images']), _cu(fr['vertices']), _cu(fr['cam']), depth, _cu(fr['para']), _cu(fr['conf']), fr['slot'], fr['observed'])


def read_heads(sd):
    shape, atlas, status = sd.read(np.arange(S), G + np.arange(S))
    torch.cuda.synchronize()
    return shape[G:].cpu().numpy(), atlas[G:].cpu().numpy(), status[G:].cpu().numpy(), sd.desc_sums[G:].cpu().numpy()


def run_stream(T, frames, clean=None, only=None):
    """Feed the frames -> per frame (shape [S,10], atlas [S,24,T,T,4], status [S], sums [S,11]).  only: a slot; every other entry of
    the chunks is emptied (the slot streamed alone)."""
    from danet_densepose2smpl_amd import tracks
    from danet_densepose2smpl_amd.texture import TextureAtlas
    sd = tracks.StreamDescriptor(S, G, TextureAtlas(densepose=to.ico_densepose(), size=T))
    out = []
    for i, fr in enumerate(frames):
        if only is not None:
            fr = dict(fr, slot=np.where(fr['slot'] == only, fr['slot'], -1).astype(np.int32), reset=[s for s in fr['reset'] if s == only])
        feed(sd, fr, None if clean is None else clean[i])
        out.append(read_heads(sd))
    return sd, out


def prefixes(frames, upto):
    """What every slot holds after frame `upto`: {slot: [(frame, entry)]} of the rows since its last reset."""
    held = {s: [] for s in range(S)}
    for i, fr in enumerate(frames[:upto + 1]):
        for s in fr['reset']:
            held[s] = []
        for p in range(P):
            if fr['slot'][p] >= 0:
                held[int(fr['slot'][p])].append((i, p))
    return held


@pytest.fixture(scope='module')
def stream():
    return make_stream()


@pytest.fixture(scope='module', params=(2, 5, 8))
def streamed(request, stream):
    T = request.param
    sd, out = run_stream(T, stream)
    return T, sd, out


# ------------------------------------------------------------------------------------------------------------------ the descriptor
def test_every_prefix_is_bit_equal_to_unwrap_and_descriptors(stream, streamed):
    from danet_densepose2smpl_amd import tracks
    from danet_densepose2smpl_amd.texture import TextureAtlas
    T, sd, out = streamed
    tex = TextureAtlas(densepose=to.ico_densepose(), size=T)
    tb = to.tables()
    mf, mb = to.texture_map(tb, T)
    worst_shape, checked = 0.0, 0
    for i in range(len(stream)):
        shape, atlas, status, sums = out[i]
        held = prefixes(stream, i)
        obs = {s: [(f, p) for f, p in held[s] if stream[f]['observed'][p]] for s in held}
        views = [fp for s in range(S) for fp in obs[s]]
        off = np.concatenate([[0], np.cumsum([len(obs[s]) for s in range(S)])]).astype(np.int32)
        pick = lambda key: np.stack([stream[f][key][p] for f, p in views])                                    # noqa: E731
        ref = tex.unwrap(_cu(pick('images')), _cu(pick('vertices')), _cu(pick('cam')), view_offsets=off).cpu().numpy()
        assert np.array_equal(_bits(atlas), _bits(ref)), (T, i)
        assert not atlas[2].any() and status[2] == 1 and not shape[2].any() and not sums[2].any()             # the empty slot
        # the shape: tracks.descriptors over all rows of the slots that hold a track
        live = [s for s in range(S) if held[s]]
        rows = [fp for s in live for fp in held[s]]
        para = np.stack([stream[f]['para'][p] for f, p in rows])
        conf = np.array([stream[f]['conf'][p] for f, p in rows], np.float32)
        start = np.concatenate([[0], np.cumsum([len(held[s]) for s in live])]).astype(np.int32)
        det = np.array([0 if stream[f]['observed'][p] else -1 for f, p in rows], np.int32)
        ts = tracks.TrackSet(start, np.concatenate([np.arange(len(held[s])) for s in live]), det, conf, len(stream))
        ref_shape, _, ref_status = tracks.descriptors(_cu(para), ts)
        assert np.array_equal(_bits(shape[live]), _bits(ref_shape)) and status[live].tolist() == ref_status.cpu().tolist() == [0] * len(live)
        for n, s in enumerate(live):
            m64, sc = lo.weighted_mean(para[start[n]:start[n + 1], 3:13], conf[start[n]:start[n + 1]])
            worst_shape = max(worst_shape, ratio(shape[s], m64))
            sy, sc2 = ro.shape_sums(para[start[n]:start[n + 1], 3:13], conf[start[n]:start[n + 1]])
            assert np.array_equal(_bits(sums[s]), _bits(np.concatenate([sy, [sc2]])))                         # the sums themselves: exact
        if i in (1, 5, 7, 8):                                               # the skin against the float64 oracle
            a64, aux = to.texture_unwrap(tb, mf, mb, pick('images'), pick('vertices'), pick('cam'), off, np.float64)
            cert = ~to.uncertain(aux, off).reshape(a64.shape[:4]) & (mf >= 0)[None]
            got = atlas.astype(np.float64)
            seen_r, seen_g = a64[..., 3] > 0, got[..., 3] > 0
            assert np.array_equal(seen_r[cert], seen_g[cert]) and not seen_g[:, mf < 0].any() and (got[~seen_g] == 0).all()
            both = cert & seen_r
            checked += int(both.sum())
            if both.any():
                d_w = (np.abs(got[..., 3] - a64[..., 3]) / np.where(both, a64[..., 3], 1.0))[both].max()
                d_c = np.abs(got[..., :3] - a64[..., :3])[both].max()
                print('T %d frame %d: %d certain observed texels, weight rel %.3g, colour %.3g (DELTA %.3g)' % (
                    T, i, both.sum(), d_w, d_c, to.bounds()['DELTA']), flush=True)
                _record('skin', d_c / to.bounds()['DELTA'], T=T, frame=i, weight=float(d_w / W_REL))
                assert d_w <= W_REL and d_c <= to.bounds()['DELTA']
    assert checked > (0 if T == 2 else 50)
    _record('shape', worst_shape, T=T)
    assert worst_shape <= 1.0
    # a gap row with c = 0 moves nothing, one with c > 0 moves the shape alone
    assert all(np.array_equal(_bits(out[2][n][0]), _bits(out[1][n][0])) for n in (0, 1, 3))
    assert np.array_equal(_bits(out[4][1][0]), _bits(out[3][1][0])) and not np.array_equal(_bits(out[4][0][0]), _bits(out[3][0][0]))
    assert np.array_equal(_bits(out[7][1][0]), _bits(out[6][1][0])) and not np.array_equal(_bits(out[7][0][0]), _bits(out[6][0][0]))   # the view outside
    assert not out[2][1][1].any() and out[2][2][1] == 1 and out[1][1][1].any()                                # slot 1 emptied in frame 2
    assert out[7][1][0].any() and not np.array_equal(_bits(out[8][1][0]), _bits(out[7][1][0]))                # slot 0 reset and refilled


def test_unread_data_stays_unread(stream, streamed):
    T, _, out = streamed
    poisoned = make_stream(poison=True)
    assert sum(int(np.isnan(fr['para']).any(1).sum()) for fr in poisoned) >= 10
    _, got = run_stream(T, poisoned, clean=stream)
    for i in range(len(stream)):
        for a, b in zip(got[i], out[i]):
            assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b)), (T, i)


def test_bits_alone_twice_and_under_graph_replay(stream, streamed):
    from danet_densepose2smpl_amd import tracks
    from danet_densepose2smpl_amd.texture import TextureAtlas
    T, _, out = streamed
    _, again = run_stream(T, stream)
    for i in range(len(stream)):
        for a, b in zip(again[i], out[i]):
            assert np.array_equal(_bits(a), _bits(b))
    for s in range(S):                                                       # each slot streamed alone: the same bits
        _, alone = run_stream(T, stream, only=s)
        for i in range(len(stream)):
            for a, b in zip(alone[i], out[i]):
                assert np.array_equal(_bits(a[s]), _bits(b[s])), (s, i)
    # one captured step replayed over the stream with refilled inputs
    sd = tracks.StreamDescriptor(S, G, TextureAtlas(densepose=to.ico_densepose(), size=T))
    keys = ('images', 'vertices', 'cam', 'para', 'conf')
    static = {k: _cu(stream[0][k]).clone() for k in keys}
    static['depth'] = torch.zeros(P, to.H, to.H, device='cuda')
    warm = tracks.StreamDescriptor(S, G, sd.tex)                             # the warm-up runs on a descriptor of its own
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            warm.step(static['images'], static['vertices'], static['cam'], static['depth'], static['para'], static['conf'], stream[0]['slot'],
                      stream[0]['observed'])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    sd.commands(stream[0]['slot'], stream[0]['observed'])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sd.launch(static['images'], static['vertices'], static['cam'], static['depth'], static['para'], static['conf'])
    sd.state.zero_()                                                         # (the capture itself launches nothing; start from empty anyway)
    for i, fr in enumerate(stream):
        for k in keys:
            static[k].copy_(_cu(fr[k]))
        static['depth'].copy_(sd.depth_planes(static['vertices'], static['cam'], to.H))
        for s in fr['reset']:
            sd.reset(s)
        sd.commands(fr['slot'], fr['observed'])
        g.replay()
        for a, b in zip(read_heads(sd), out[i]):
            assert np.array_equal(_bits(a), _bits(b)), i
    del g
    # P = 0 launches nothing and keeps a pending reset for the next step
    sd.reset(0)
    e = torch.zeros(0, device='cuda')
    sd.step(e.view(0, 3, to.H, to.H), e.view(0, 12, 3), e.view(0, 3), e.view(0, to.H, to.H), e.view(0, 229), e, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert np.array_equal(_bits(read_heads(sd)[1]), _bits(out[-1][1]))
    feed(sd, dict(stream[2], reset=[]))
    assert not read_heads(sd)[1][0].any()


def test_apply_shape(stream, streamed):
    """Rows with use = 0, rows of an empty entry and rows without weight keep their bits; the others get the oracle's rounded value."""
    T, sd, out = streamed
    rng = np.random.default_rng(11)
    slot = np.array([0, 1, -1, 0, 2, 1], np.int32)
    use = np.array([1, 1, 1, 0, 1, 1], np.int32)
    carry = np.concatenate([rng.normal(0, 3, (6, 10)), rng.uniform(0.5, 20, (6, 1))], 1)
    carry[1] = 0.0                                                           # a zero carry: the track's own mean
    carry[4] = 0.0                                                           # the empty slot with a zero carry: no weight
    rows = rng.normal(0, 1, (6, 229)).astype(np.float32)
    x = _cu(rows)
    assert sd.apply_shape(x, slot, _cu(carry), use) is x
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    sums = out[-1][3]
    want = rows.copy()
    for p in (0, 1, 5):
        want[p, 3:13] = ro.carried_shape(carry[p], sums[slot[p], :10], sums[slot[p], 10])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[1, 3:13]), _bits(out[-1][0][1]))         # zero carry: the slot's own descriptor
    assert not np.array_equal(_bits(got[0]), _bits(rows[0]))


# ------------------------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope='module')
def demo_model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False).cuda().eval()


PRESENT = (0, 1, 2, 3, 11, 12, 13)                                           # both people are away for seven frames, max_gap is 2
STREAM_KW = dict(lag=2, box_lag=2, max_gap=2)


def clip():
    """test_gpu_link.py's clip, restated: fourteen frames of 96 x 80, the left half one flat colour, the right half another, a person
    in each half in flat-coloured clothing that fills their box.  Both leave after frame 3 and come back in frame 11."""
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


def run_clip(model, **kw):
    from danet_densepose2smpl_amd import video
    frames, boxes = clip()
    demo = video.StreamDemo(model, model.iuv2smpl.smpl, 2, **dict(STREAM_KW, **kw))
    demo.record = True
    done = []
    for f, b in zip(frames, boxes):
        done += demo.push(f, b)
    rest, summary = demo.flush()
    return demo, done + rest, summary


@pytest.fixture(scope='module')
def with_reid(demo_model):
    return run_clip(demo_model, reid=True)


@pytest.fixture(scope='module')
def without(demo_model):
    return run_clip(demo_model, reid=False)


def test_stream_demo_keeps_identities_across_an_absence(with_reid):
    demo, done, summary = with_reid
    ts, rec = demo.tracks, demo.recorded
    print(summary, flush=True)
    assert summary['tracks'] == 4 and summary['rows'] == 14 and summary['gap_rows'] == 0 and summary['identities'] == 2 and summary['links'] == 2
    assert demo.identity.tolist() == [0, 1, 0, 1] and demo.identity.dtype == np.int32
    assert demo.links.dtype == np.int32 and sorted(demo.links.tolist()) == [[0, 2], [1, 3]] and demo.link_cost.dtype == np.float64
    assert [n for n, _, _ in done] == list(range(14))
    for f, _, p in done:                                                     # from a track's first drawn frame on
        assert p['identity'].tolist() == ([0, 1] if f in PRESENT else []) and p['identity'].dtype == np.int32
        assert p['identity'].tolist() == demo.identity[p['track_id']].tolist()
    # the causal oracle on the recorded descriptors
    first, last = lo.spans(ts.track_start, ts.frame)
    assert first.tolist() == [0, 0, 11, 11] and last.tolist() == [3, 3, 13, 13] and sorted(rec['head']) == [2, 3] and sorted(rec['final']) == [0, 1, 2, 3]
    final = {k: tuple(t.cpu().numpy() for t in rec['final'][k]) for k in range(4)}
    head = {k: tuple(t.cpu().numpy() for t in rec['head'][k]) for k in (2, 3)}
    assert final[0][1].shape == (24, 8, 8, 4) and not lo.near_w_min(np.stack([final[0][1], final[1][1], head[2][1], head[3][1]]))
    ref = ro.solve(first, last, lambda k: final[k][:2], lambda k: head[k], np.stack([final[k][2] for k in range(4)]), gallery=64)
    pairs = [(0, 2), (0, 3), (1, 2), (1, 3)]
    assert sorted(rec['dist']) == pairs
    shape = np.stack([final[0][0], final[1][0], head[2][0], head[3][0]])
    atlas = np.stack([final[0][1], final[1][1], head[2][1], head[3][1]])
    dist64 = lo.pair_distance(shape, atlas, np.array(pairs))
    got = np.stack([rec['dist'][p] for p in pairs])
    r_dist = ratio(got, dist64)
    print('dist (d_shape, d_app, overlap, S)\n%s\ncosts %s' % (got, demo.link_cost), flush=True)
    _record('pipeline_dist', r_dist)
    assert r_dist <= 1.0
    assert np.array_equal(demo.identity, ref['identity']) and np.array_equal(demo.links, ref['links']) and np.array_equal(demo.link_cost, ref['link_cost'])
    # the shape sums, heads and carried means from the recorded rows, in the rule's association: exact
    para = demo.para
    for k in range(4):
        rows = [rec['rows'][(k, g)] for g in range(first[k], last[k] + 1)]
        betas = np.stack([r[0].cpu().numpy()[3:13] for r in rows])
        conf = np.array([r[1] for r in rows], np.float32)
        assert all(r[2] for r in rows)
        sy, sc = ro.shape_sums(betas, conf)
        assert np.array_equal(_bits(final[k][2]), _bits(np.concatenate([sy, [sc]])))
        assert np.array_equal(_bits(final[k][0]), _bits(ro.shape_of(sy, sc)))
        assert np.array_equal(_bits(final[k][3]), _bits(ref['carry'][k]))
        if k in head:                                                        # lag 2, three rows: the head is the rows of frames 11 .. 13
            assert np.array_equal(_bits(head[k][0]), _bits(ro.shape_of(sy, sc)))
        if k >= 2:
            assert ref['carry'][k][10] > 0
            for d in range(first[k], last[k] + 1):                           # drawn at d: the rows of frames first .. min(d + lag, last) are in
                n = min(d + STREAM_KW['lag'], last[k]) - first[k] + 1
                want = ro.carried_shape(ref['carry'][k], *ro.shape_sums(betas[:n], conf[:n]))
                row = int(ts.track_start[k]) + d - int(first[k])
                assert np.array_equal(_bits(para[row, 3:13]), _bits(want)), (k, d)
        else:
            assert not ref['carry'][k].any()


def test_stream_demo_without_reid_is_what_it_was_and_unlinked_tracks_keep_their_rows(demo_model, with_reid, without):
    from danet_densepose2smpl_amd import video
    demo, done, summary = with_reid
    off, done0, summary0 = without
    plain = video.StreamDemo(demo_model, demo_model.iuv2smpl.smpl, 2, **STREAM_KW)          # today's call: no reid argument at all
    frames, boxes = clip()
    done1 = []
    for f, b in zip(frames, boxes):
        done1 += plain.push(f, b)
    rest, summary1 = plain.flush()
    done1 += rest
    assert sorted(summary0) == sorted(summary1) and 'identities' not in summary0 and 'identity' not in done0[0][2] and not hasattr(off, 'identity')
    assert off.desc is None and off.linker is None
    for (n0, r0, p0), (n1, r1, p1) in zip(done0, done1):
        assert n0 == n1 and np.array_equal(r0, r1) and sorted(p0) == sorted(p1) and np.array_equal(_bits(p0['para']), _bits(p1['para']))
    for k in ('para', 'para_raw', 'boxes', 'boxes_raw'):
        assert np.array_equal(_bits(getattr(off, k)), _bits(getattr(plain, k))), k
    for k, v in plain.tracks.arrays().items():
        assert np.array_equal(v, off.tracks.arrays()[k]) and np.array_equal(v, demo.tracks.arrays()[k]), k
    # with reid=True: the unlinked tracks' rows and frames are what they are without; a linked track differs in its shape alone
    ts = demo.tracks
    unlinked = np.isin(ts.track, (0, 1))
    assert np.array_equal(_bits(demo.para[unlinked]), _bits(off.para[unlinked])) and np.array_equal(_bits(demo.para_raw), _bits(off.para_raw))
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(_bits(demo.para[:, other]), _bits(off.para[:, other]))
    assert not np.array_equal(_bits(demo.para[~unlinked, 3:13]), _bits(off.para[~unlinked, 3:13]))
    for (n, r, _), (_, r0, _) in zip(done, done0):
        if n < 11:
            assert np.array_equal(r, r0), n


def test_stream_demo_without_smoothing_shares_the_shape_of_linked_tracks_alone(demo_model):
    """smooth=False: the rows drawn are the network's own; a linked track gets its identity's shape, nothing else moves."""
    demo, done, summary = run_clip(demo_model, reid=True, smooth=False)
    ts = demo.tracks
    assert demo.identity.tolist() == [0, 1, 0, 1] and summary['links'] == 2
    unlinked = np.isin(ts.track, (0, 1))
    other = np.ones(229, bool)
    other[3:13] = False
    assert np.array_equal(_bits(demo.para[unlinked]), _bits(demo.para_raw[unlinked]))
    assert np.array_equal(_bits(demo.para[:, other]), _bits(demo.para_raw[:, other]))
    for k in (2, 3):
        carry = demo.recorded['final'][k][3].cpu().numpy()
        rows = [demo.recorded['rows'][(k, g)] for g in (11, 12, 13)]
        betas, conf = np.stack([r[0].cpu().numpy()[3:13] for r in rows]), np.array([r[1] for r in rows], np.float32)
        assert carry[10] > 0 and np.array_equal(_bits(betas), _bits(demo.para_raw[ts.track == k, 3:13]))    # the rows described are the rows drawn
        for d in (11, 12, 13):
            want = ro.carried_shape(carry, *ro.shape_sums(betas[:min(d + 2, 13) - 10], conf[:min(d + 2, 13) - 10]))
            assert np.array_equal(_bits(demo.para[int(ts.track_start[k]) + d - 11, 3:13]), _bits(want)), (k, d)


def test_gallery_overflow_raises_with_the_counts(demo_model):
    from danet_densepose2smpl_amd import video
    frames, boxes = clip()
    demo = video.StreamDemo(demo_model, demo_model.iuv2smpl.smpl, 2, reid=True, gallery=1, **STREAM_KW)
    for f in range(7):                                                       # frame 3, the last of both tracks, is drawn at clock 3 + 2 + 2
        demo.push(frames[f], boxes[f])
    with pytest.raises(RuntimeError, match='1 finished tracks wait in the gallery and frame 3 retires another; the gallery holds 1'):
        demo.push(frames[7], boxes[7])


def test_tool_with_stream_reid_writes_identities_and_refuses_reid_alone(tmp_path):
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
            str(tmp_path / 'boxes.json'), '--batch', '2', '--reid']
    r = subprocess.run(tool, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and '--link' in r.stderr and not os.path.exists(str(dst / 'tracks.npz'))
    r = subprocess.run(tool + ['--stream', '--lag', '2', '--box_lag', '2', '--max_absence', '20', '--gallery', '4'], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().split('\n')[-1])
    print(line, flush=True)
    assert line['tool'] == 'demo_video' and line['stream'] is True and line['frames'] == 14 and line['tracks'] == 4 and line['rows'] == 14
    assert line['reid'] is True and line['identities'] == 2 and line['links'] == 2 and line['max_absence'] == 20 and line['id_texture_size'] == 8
    assert line['gallery'] == 4 and all(line['ms_per_frame'][k] > 0 for k in ('associate', 'boxes', 'infer', 'smooth', 'reid', 'render'))
    z = np.load(str(dst / 'tracks.npz'))
    assert z['identity'].tolist() == [0, 1, 0, 1] and z['identity'].dtype == np.int32
    assert z['links'].shape == (2, 2) and z['links'].dtype == np.int32 and z['link_cost'].shape == (2,) and z['link_cost'].dtype == np.float64
    assert z['para'].shape == (14, 229) and z['track_start'].tolist() == [0, 4, 8, 11, 14]
