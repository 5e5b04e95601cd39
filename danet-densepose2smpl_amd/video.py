"""Video demo: the frames of a clip plus person boxes per frame in, the frames with every person's mesh drawn in place out, the people
followed across frames (tracks.associate), their boxes and rows smoothed along each track (tracks.smooth, tracks.smooth_para;
DESIGN.md 4b'-track "the track rule") and the frames in which a person has no box filled in.

    demo = VideoDemo(model_or_engine, smpl, batch, fitter=None)
    rendered, people, summary = demo(frames, boxes, keypoints=None)

A VideoDemo wraps a scene.SceneDemo and calls its stages; the scene demo itself is what it was.  The whole clip is one call: every
row of every track is on the device at once.  StreamDemo (below) is the same pipeline fed one frame at a time: online association, an
exact fixed-lag smoother (tracks.StreamSmoother, DESIGN.md 4b'-stream "the stream rule") and a bounded number of frames held, for
clips that do not fit on the device and for live sources.  With link=True a VideoDemo also links the tracks of one person into an
identity by body shape and fused texture (tracks.descriptors / affinity / link / share_shape, DESIGN.md 4b'-link "the identity rule").
With reid=True a StreamDemo decides a track's identity at its first drawn frame from the descriptors kept as running sums
(tracks.StreamDescriptor / OnlineLinker, DESIGN.md 4b'-reid "the causal identity rule").
Not here: video decoding, a person detector, revising an identity later, motion prediction, several ranks.
There is no CPU path."""
import numpy as np
import torch

from . import tracks as tr
from . import constants
from .ops import _int, _texture_size
from .scene import SceneDemo, box_row, fit_columns, row_box, split_people, timed, unpack_frames
from .smpl import from_para


def _gap_conf(what, v):
    """The weight of a gap row's own prediction in the smoother: finite, in [0, 1]."""
    if not (np.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError('%s: gap_conf %r (in [0, 1])' % (what, v))


def accel_summary(joints_fn, para_raw, para, ts):
    """The four acceleration entries of a summary: joints_fn(rows) gives the SMPL joints [N,J,3] of para_raw and of para on the
    device, track-major; 'accel_raw_tracks' / 'accel_tracks' [K] are tracks.accel of the two, 'accel_raw' / 'accel' their means
    weighted by the tracks' interior-row counts."""
    if ts.N:
        a0, cnt = tr.accel(joints_fn(para_raw), ts)
        a1, _ = tr.accel(joints_fn(para), ts)
        a0, a1, cnt = a0.cpu().numpy(), a1.cpu().numpy(), cnt.cpu().numpy().astype(np.float64)
    else:
        a0 = a1 = cnt = np.zeros(ts.K)
    w = cnt / cnt.sum() if cnt.sum() > 0 else cnt
    return {'accel_raw': float((a0 * w).sum()), 'accel': float((a1 * w).sum()), 'accel_raw_tracks': a0, 'accel_tracks': a1}


class VideoDemo(object):
    """VideoDemo(model_or_engine, smpl, batch, fitter=None, smooth=True, rounds=1, shared_shape=True, max_gap=5, min_iou=0.3,
    gap_conf=0., lam=tracks.DEFAULT_LAM, box_lam=tracks.BOX_LAM, **scene_kw): the first three and `fitter` as scene.SceneDemo takes
    them.  `rounds` times the rows are fitted from their current values (where there is a fitter) and then smoothed: the fitters
    take the start row both as initialisation and as prior, so the alternation is a proximal one.  gap_conf: the weight of a gap
    row's own prediction in the smoother (0: the row is filled from its neighbours alone).  With smooth = False nothing is smoothed
    (gap rows still get an interpolated box), and a clip without gap rows comes out as SceneDemo draws it, bit for bit.
    link=True (DESIGN.md 4b'-link): after the last round the tracks are linked into identities on the final rows -- a person who
    was away for up to `max_absence` frames keeps their identity --, with shared_shape every identity gets one shape, and the frames
    are drawn from those rows; max_absence, sigma_s, sigma_a, min_overlap, no_app default to tracks.LINK_DEFAULTS, id_texture_size
    (the side of a chart of the skin descriptor) to tracks.ID_TEXTURE_SIZE.  Without it every output is what it was."""

    def __init__(self, model_or_engine, smpl, batch, fitter=None, smooth=True, rounds=1, shared_shape=True, max_gap=5, min_iou=0.3,
                 gap_conf=0., lam=tr.DEFAULT_LAM, box_lam=tr.BOX_LAM, link=False, max_absence=None, id_texture_size=tr.ID_TEXTURE_SIZE,
                 sigma_s=None, sigma_a=None, min_overlap=None, no_app=None, **scene_kw):
        given = {'max_absence': max_absence, 'sigma_s': sigma_s, 'sigma_a': sigma_a, 'min_overlap': min_overlap, 'no_app': no_app}
        self.link = bool(link)
        self.link_kw = tr.link_arguments('VideoDemo', **{k: tr.LINK_DEFAULTS[k] if v is None else v for k, v in given.items()})
        self.id_texture_size = _texture_size(id_texture_size)
        self._tex = None
        self.scene = SceneDemo(model_or_engine, smpl, batch, fitter=fitter, **scene_kw)
        self.smooth, self.rounds, self.shared_shape = bool(smooth), int(rounds), bool(shared_shape)
        self.max_gap, self.min_iou, self.gap_conf = int(max_gap), float(min_iou), float(gap_conf)
        self.lam, self.box_lam = tuple(tuple(p) for p in lam), tuple(box_lam)
        if self.rounds < 1:
            raise ValueError('VideoDemo: rounds %d (>= 1)' % self.rounds)
        _gap_conf('VideoDemo', self.gap_conf)
        self.last = {}

    # ---- stages ------------------------------------------------------------------------------------------------------------------
    def track_boxes(self, boxes):
        """boxes per frame -> (TrackSet, boxes_raw [N,3] f32 = (cx, cy, log scale) per row, zeros in gap rows, boxes [N,3] f32 the rows
        after the box smoother, boxes per frame in person order with the gap rows included).  Observed rows keep their own box when
        nothing is smoothed."""
        ts = tr.associate(boxes, self.max_gap, self.min_iou)
        raw = np.zeros((ts.N, 3), np.float32)
        for n in range(ts.N):
            if ts.det[n] >= 0:
                raw[n] = box_row(boxes[ts.frame[n]][ts.det[n]])
        if ts.N == 0:
            return ts, raw, raw.copy(), [[] for _ in boxes]
        sm, _ = tr.smooth(torch.from_numpy(raw).to(self.scene.device), ts, *self.box_lam)
        sm = sm.cpu().numpy()
        per_frame = [[] for _ in boxes]
        for n in ts.person_row:
            if ts.det[n] >= 0 and not self.smooth:
                b = boxes[ts.frame[n]][ts.det[n]]
                per_frame[ts.frame[n]].append((b[0], b[1]))
            else:
                per_frame[ts.frame[n]].append(row_box(sm[n]))
        return ts, raw, sm, per_frame

    def person_keypoints(self, ts, keypoints):
        """Keypoints per frame and box -> per frame and person of the plan: a gap row has none, so it gets zeros."""
        out = [[] for _ in range(ts.n_frames)]
        for n in ts.person_row:
            f, d = int(ts.frame[n]), int(ts.det[n])
            out[f].append(np.zeros((49, 3)) if d < 0 else keypoints[f][d])
        return out

    def joints(self, para):
        return from_para(self.scene.smpl, para).smpl_joints.detach()

    def link_tracks(self, rows, ts, plan):
        """The identity rule on the rows [N,229] (track-major, on the device) of the TrackSet whose conf weighs the shape: the
        descriptors (the skin from the de-normalised crops of the observed rows, through the meshes and cameras of those rows), the
        distances of the time-admissible pairs and the linking.  -> tracks.link's dict plus 'shape' [K,10] and 'atlas' [K,24,T,T,4]
        (device) and 'dist' [C,4] (host)."""
        from .texture import TextureAtlas
        sc = self.scene
        if self._tex is None:
            self._tex = TextureAtlas(size=self.id_texture_size, focal_length=sc.focal)

        def skin(obs, view_offsets):
            mean, std = (torch.tensor(c, device=sc.device).view(1, 3, 1, 1) for c in (constants.IMG_NORM_MEAN, constants.IMG_NORM_STD))
            crops = (sc.crops(plan) * std + mean).clamp(0.0, 1.0)
            drawn = rows[torch.from_numpy(obs).to(sc.device)]
            return self._tex.unwrap(crops[torch.from_numpy(ts.row_person[obs]).to(sc.device)], sc.vertices(drawn), drawn[:, 0:3].contiguous(),
                                    view_offsets=view_offsets)
        shape, atlas, _ = tr.descriptors(rows, ts, skin)
        pairs = tr.PairSet(tr.candidates(ts, self.link_kw['max_absence']), ts.K)
        dist = tr.affinity(shape, atlas, pairs).cpu().numpy()
        res = tr.link(ts, dist, pairs, **self.link_kw)
        res.update({'shape': shape, 'atlas': atlas, 'dist': dist})
        return res

    def __call__(self, frames, boxes, keypoints=None):
        """-> (rendered frames, people: SceneDemo's dict per frame plus 'track_id' [k], 'observed' [k] and 'para_raw' [k,229] (the
        network's rows), summary: 'tracks', 'rows', 'gap_rows', 'accel_raw' and 'accel' (the mean acceleration of the SMPL joints over
        all tracks' interior rows before and after), 'accel_raw_tracks' / 'accel_tracks' [K]).  With link=True the people dicts gain
        'identity' [k], the summary 'identities' and 'links', and self.last 'identity' [K], 'links' [L,2], 'link_cost' [L] and 'link'
        (link_tracks' dict with 'rows', the rows the descriptors were made from)."""
        sc = self.scene
        if len(frames) != len(boxes) or not frames:
            raise ValueError('VideoDemo: %d frames, %d box lists' % (len(frames), len(boxes)))
        if keypoints is not None and [len(k) for k in keypoints] != [len(b) for b in boxes]:
            raise ValueError('VideoDemo: keypoints must hold one array per box of every frame')
        ts, boxes_raw, boxes_s, per_frame = self.track_boxes(boxes)
        plan = sc.prepare(frames, per_frame)
        P = plan['P']
        dev = sc.device
        to_rows = torch.from_numpy(ts.row_person).to(dev)               # x[to_rows]: people (frame-major) -> rows (track-major)
        to_people = torch.from_numpy(ts.person_row).to(dev)             # and back
        conf = ts.conf.copy()
        conf[ts.det < 0] = self.gap_conf
        ts_para = ts.with_conf(conf)
        para, iuv = sc.infer_stage(plan)
        para_raw = para
        kps = self.person_keypoints(ts, keypoints) if (sc.fitter is not None and keypoints is not None) else None
        for _ in range(self.rounds):
            fitted, para = sc.fit_stage(para, plan, kps, iuv)
            if not self.smooth or not P:
                break
            rows, _ = tr.smooth_para(para[to_rows], ts_para, self.lam, self.shared_shape)
            para = rows[to_people]
        summary = {'tracks': ts.K, 'rows': ts.N, 'gap_rows': int((ts.det < 0).sum())}
        linked = None
        if self.link:
            rows = para[to_rows] if P else para
            linked = self.link_tracks(rows, ts_para, plan) if P else tr.link(ts_para, np.zeros((0, 4)), np.zeros((0, 2), np.int32), **self.link_kw)
            linked['rows'] = rows
            if P and self.shared_shape:
                para = tr.share_shape(rows, ts_para, linked['identity'])[0][to_people]
            summary.update({'identities': int(linked['identity'].max()) + 1 if ts.K else 0, 'links': int(linked['links'].shape[0])})
        summary.update(accel_summary(lambda rows: self.joints(rows)[to_rows], para_raw, para, ts))
        verts = sc.vertices(para) if P else None
        aux = sc.render(para, plan, return_aux=True, vertices=verts)
        rendered = unpack_frames(aux[0].cpu().numpy(), plan['offsets'], plan['shapes'])
        para_h, raw_h = para.cpu().numpy(), para_raw.cpu().numpy()
        verts_h = verts.cpu().numpy() if P else np.zeros((0, 0, 3), np.float32)
        track_p = ts.track[ts.person_row]
        columns = dict({'track_id': track_p, 'observed': ts.det[ts.person_row] >= 0, 'para_raw': raw_h}, **fit_columns(fitted, P))
        if linked is not None:
            columns['identity'] = linked['identity'][track_p]
        people = split_people(sc.people(para_h, verts_h, plan, **columns), plan)
        self.last = {'tracks': ts, 'plan': plan, 'render_aux': aux, 'boxes_raw': boxes_raw, 'boxes': boxes_s,
                     'para_raw': raw_h[ts.row_person] if P else raw_h, 'para': para_h[ts.row_person] if P else para_h}
        if linked is not None:
            self.last.update({'identity': linked['identity'], 'links': linked['links'], 'link_cost': linked['link_cost'], 'link': linked})
        return rendered, people, summary


STREAM_LAG = 8          # the default lag and box_lag of StreamDemo: DESIGN.md 4b'-stream, the lag table
NO_STREAM_LINK = ('StreamDemo: link=True is not available while streaming: the descriptor of the identity rule (DESIGN.md 4b\'-link) needs a '
                  'finished track, its mean shape and the texture fused over all its observed rows; link the clip with VideoDemo.  '
                  'While streaming, reid=True decides identities causally (DESIGN.md 4b\'-reid)')


class StreamDemo(object):
    """StreamDemo(model_or_engine, smpl, batch, fitter=None, smooth=True, lag=8, box_lag=8, slots=32, shared_shape=True, max_gap=5,
    min_iou=0.3, gap_conf=0., lam=tracks.DEFAULT_LAM, box_lam=tracks.BOX_LAM, **scene_kw): VideoDemo's pipeline fed one frame at a
    time (DESIGN.md 4b'-stream "the stream rule").

        done = demo.push(frame, boxes, keypoints=None)       # [] or [(frame_index, rendered, people)]
        rest, summary = demo.flush()

    Frame f enters the association (tracks.OnlineAssociator) and the box stream; frame g = f - box_lag gets its smoothed boxes, gap
    rows included (box_lag >= max_gap is what makes "gap row or ended track" decidable for it), is cropped, inferred and, where there is
    a fitter, fitted once; its rows enter the para stream (tracks.StreamSmoother, one launch per frame for every track), and frame
    g - lag is drawn: a delay of box_lag + lag frames, at most box_lag + lag + 1 frames held.  Every value drawn is the offline rule on
    the track's committed prefix; people dicts carry VideoDemo's keys plus 'prefix_end' [k], the last frame of the prefix each row was
    computed from.  With shared_shape a track's shape is its prefix's mean and so moves over time.  A track holds one of `slots` slots
    from its first box until its last row is drawn.  There is no `rounds`: the fit / smooth alternation needs whole tracks and stays
    VideoDemo's.  With smooth = False observed rows keep their own box and row, and gap rows get the box stream's box.  Wraps a
    scene.SceneDemo and does not change it; there is no CPU path.  link=True raises ValueError: identities need finished tracks and
    are VideoDemo's.
    reid=True (DESIGN.md 4b'-reid "the causal identity rule"): every track's descriptor is kept as running sums
    (tracks.StreamDescriptor, one launch per processed frame); a track's identity is decided once, at its first drawn frame, from its
    rows so far against the finished tracks of the last `max_absence` frames (tracks.OnlineLinker; at most `gallery` of them wait), and
    never revised; with shared_shape the rows of a linked track are drawn with the shape of its identity so far.  The people dicts gain
    'identity' [k], the summary 'identities' and 'links', and after flush() the object holds identity [K], links [L,2] and link_cost
    [L].  max_absence, sigma_s, sigma_a, min_overlap, no_app default to tracks.REID_DEFAULTS.  Without it every output is what it
    was.  With `record` set, `recorded` keeps device copies of the rows, heads, final descriptors and distances the decisions were
    taken on (the tests compare them with the float64 oracle); it grows with the stream."""

    @staticmethod
    def check_arguments(lag, box_lag, slots, max_gap, gap_conf, link=False):
        if link:
            raise ValueError(NO_STREAM_LINK)
        for name, v, low in (('lag', lag, 0), ('box_lag', box_lag, 0), ('slots', slots, 1), ('max_gap', max_gap, 1)):
            _int(v, 'StreamDemo', name, low)
        if box_lag < max_gap:
            raise ValueError('StreamDemo: box_lag %d is below max_gap %d: a frame would be emitted before its gap rows are known' % (box_lag, max_gap))
        _gap_conf('StreamDemo', gap_conf)

    @staticmethod
    def check_reid_arguments(max_absence=None, id_texture_size=tr.ID_TEXTURE_SIZE, gallery=tr.REID_GALLERY, sigma_s=None, sigma_a=None,
                             min_overlap=None, no_app=None):
        """-> (the thresholds of the causal identity rule as a dict, None taking tracks.REID_DEFAULTS; the chart size; the gallery)."""
        given = {'max_absence': max_absence, 'sigma_s': sigma_s, 'sigma_a': sigma_a, 'min_overlap': min_overlap, 'no_app': no_app}
        thr = tr.link_arguments('StreamDemo', **{k: tr.REID_DEFAULTS[k] if v is None else v for k, v in given.items()})
        return thr, _texture_size(id_texture_size), _int(gallery, 'StreamDemo', 'gallery', 1, 1 << 16)

    def __init__(self, model_or_engine, smpl, batch, fitter=None, smooth=True, lag=STREAM_LAG, box_lag=STREAM_LAG, slots=32, shared_shape=True,
                 max_gap=5, min_iou=0.3, gap_conf=0., lam=tr.DEFAULT_LAM, box_lam=tr.BOX_LAM, link=False, reid=False, max_absence=None,
                 id_texture_size=tr.ID_TEXTURE_SIZE, gallery=tr.REID_GALLERY, sigma_s=None, sigma_a=None, min_overlap=None, no_app=None,
                 **scene_kw):
        self.check_arguments(lag, box_lag, slots, max_gap, gap_conf, link)
        self.reid_kw, self.id_texture_size, self.gallery = self.check_reid_arguments(max_absence, id_texture_size, gallery, sigma_s, sigma_a,
                                                                                    min_overlap, no_app)
        self.reid, self.shared_shape = bool(reid), bool(shared_shape)
        self.linker = tr.OnlineLinker(self.gallery, **self.reid_kw) if self.reid else None
        self.desc = None                     # the tracks.StreamDescriptor, made at the first use
        self._carry = self._tot = None       # the chain totals on the device (_tables)
        self.carried = set()                 # the tracks that have a predecessor
        self.record, self.recorded = False, {'rows': {}, 'head': {}, 'final': {}}       # record: keep device copies of what was decided on
        self.assoc = tr.OnlineAssociator(max_gap, min_iou, what='StreamDemo')
        self.smooth, self.lag, self.box_lag, self.slots = bool(smooth), int(lag), int(box_lag), int(slots)
        self.max_gap, self.gap_conf = int(max_gap), float(gap_conf)
        self.box_stream = tr.StreamSmoother(self.slots, self.box_lag, max_new=self.max_gap, channels=3, lam=box_lam)
        self.para_stream = tr.StreamSmoother(self.slots, self.lag, para=True, lam=lam, shared_shape=shared_shape)
        self.scene = SceneDemo(model_or_engine, smpl, batch, fitter=fitter, **scene_kw)
        self.free = list(range(self.slots))
        self.slot = {}                       # track -> slot, while it holds one
        self.boxed = {}                      # track -> the last frame whose box row went into the box stream
        self.held = {}                       # frame -> what is kept of it until it is drawn
        self.rows = {}                       # (track, frame) -> (para_raw [229], para [229]) of every row drawn, for the summary
        self.box_rows = {}                   # (track, frame) -> (box_raw [3] or None in a gap row, box [3] after the box stream)
        self.time = 0                        # frames pushed plus the flush's steps
        self.max_held = 0
        self.timing, self.ms = False, {}     # timing: a device synchronisation around every stage, milliseconds summed per stage in ms
        self.last = {}

    def _timed(self, key, f):
        return timed(self.ms, key, f) if self.timing else f()

    # ---- the three stages of one step ------------------------------------------------------------------------------------------------
    def _span(self, k):
        r = self.assoc.tracks[k]['rows']
        return r[0][0], r[-1][0]

    def _covering(self, frame):
        return [k for k in sorted(self.slot) if self._span(k)[0] <= frame <= self._span(k)[1]]

    def _box_step(self, matches, g):
        """The new committed box rows of this frame's matched tracks go in; the boxes of frame g (or None) come out: {track: [3]}."""
        st, S, M = self.box_stream, self.slots, self.max_gap
        n_new, emit = np.zeros(S, np.int64), np.full(S, -1, np.int64)
        rows, conf = np.zeros((S, M, 3), np.float32), np.zeros((S, M), np.float32)
        f = self.assoc.n_frames - 1
        for k, d in matches:
            if k not in self.slot:
                if not self.free:
                    raise RuntimeError('StreamDemo: %d tracks hold a slot and frame %d opens another; there are %d slots' % (len(self.slot), f, self.slots))
                s = self.slot[k] = self.free.pop(0)
                self.box_stream.reset(s)
                self.para_stream.reset(s)
                if self.reid:
                    self._descriptor().reset(s)
            s = self.slot[k]
            n = f - self.boxed.get(k, f - 1)                               # the gap rows this detection has resolved, then its own row
            rows[s, n - 1] = box_row(self.held[f]['boxes'][d])
            self.box_rows[(k, f)] = [rows[s, n - 1].copy(), None]
            conf[s, n - 1] = self.assoc.tracks[k]['rows'][-1][2]
            n_new[s], self.boxed[k] = n, f
        cover = self._covering(g) if g is not None else []
        for k in cover:
            emit[self.slot[k]] = g - self._span(k)[0]
        if not (n_new.any() or cover):
            return {}
        out, _ = st.step(n_new, torch.from_numpy(rows).to(self.scene.device), conf, emit)
        out = out.cpu().numpy()
        for k in cover:
            self.box_rows.setdefault((k, g), [None, None])[1] = out[self.slot[k]].copy()
        return {k: out[self.slot[k]].copy() for k in cover}

    def _process(self, g, sm_boxes):
        """Frame g with its smoothed boxes: crop, infer, fit; -> its people in VideoDemo's order (detections, then gap rows by track)."""
        sc, h = self.scene, self.held[g]
        by_det = {r[1]: k for k in sm_boxes for r in self.assoc.tracks[k]['rows'] if r[0] == g}
        order = [(by_det[d], d) for d in range(len(h['boxes']))] + [(k, -1) for k in sorted(sm_boxes) if k not in by_det.values()]
        boxes = []
        for k, d in order:
            if d >= 0 and not self.smooth:
                boxes.append((h['boxes'][d][0], h['boxes'][d][1]))
            else:
                boxes.append(row_box(sm_boxes[k]))
        plan = sc.prepare([h['frame']], [boxes])
        para, iuv = sc.infer_stage(plan)
        kps = None if h['kps'] is None else [[np.zeros((49, 3)) if d < 0 else h['kps'][d] for _, d in order]]
        h.update({'plan': plan, 'order': order, 'para_raw': para})
        h['fitted'], h['para_in'] = sc.fit_stage(para, plan, kps, iuv)
        del h['boxes'], h['kps']

    def _row_conf(self, k, det, g):
        """The weight of track k's row of frame g: its detection's confidence, gap_conf for a gap row."""
        return self.gap_conf if det < 0 else [r[2] for r in self.assoc.tracks[k]['rows'] if r[0] == g][0]

    # ---- identities (DESIGN.md 4b'-reid) -----------------------------------------------------------------------------------------------
    def _descriptor(self):
        if self.desc is None:
            from .texture import TextureAtlas
            tex = TextureAtlas(size=self.id_texture_size, focal_length=self.scene.focal)
            self.desc = tr.StreamDescriptor(self.slots, self.gallery, tex)
        return self.desc

    def _describe(self, g):
        """The rows of frame g that enter the para stream go into their tracks' descriptors: the de-normalised crops as
        VideoDemo.link_tracks makes them, the meshes and cameras of those rows, the rasteriser's depth plane.  One launch."""
        sc, h, desc = self.scene, self.held[g], self._descriptor()
        order = h['order']
        if not order:
            return
        mean, std = (torch.tensor(c, device=sc.device).view(1, 3, 1, 1) for c in (constants.IMG_NORM_MEAN, constants.IMG_NORM_STD))
        crops = (sc.crops(h['plan']) * std + mean).clamp(0.0, 1.0)
        rows = h['para_in'].contiguous()
        verts, cam = sc.vertices(rows), rows[:, 0:3].contiguous()
        conf = np.array([self._row_conf(k, det, g) for k, det in order], np.float32)
        observed = np.array([det >= 0 for _, det in order], np.int32)
        desc.step(crops, verts, cam, desc.depth_planes(verts, cam, crops.shape[2]), rows, torch.from_numpy(conf).to(sc.device),
                  np.array([self.slot[k] for k, _ in order], np.int32), observed)
        if self.record:
            for i, (k, _) in enumerate(order):
                self.recorded['rows'][(k, g)] = (rows[i].clone(), float(conf[i]), bool(observed[i]))

    def _tables(self):
        """(carry [slots,11], tot [gallery,11]) float64 on the device: the chain totals (sum c betas, sum c) a slot's track inherits and
        those of the finished tracks in the gallery."""
        if self._carry is None:
            self._carry = torch.zeros(self.slots, 11, device=self.scene.device, dtype=torch.float64)
            self._tot = torch.zeros(self.gallery, 11, device=self.scene.device, dtype=torch.float64)
        return self._carry, self._tot

    def _identify(self, d):
        """The decisions of drawn frame d: its newborn tracks against the gallery (the one host read: dist [C,4], where there are both),
        then the tracks whose last row this is go into the gallery.  -> {track: identity} of the frame's people."""
        lk, desc, order = self.linker, self._descriptor(), self.held[d]['order']
        carry, tot = self._tables()
        newborn = sorted(k for k, _ in order if self._span(k)[0] == d)
        cand = lk.candidates(d, newborn)
        if newborn:
            dist = np.zeros((0, 4))
            if cand:
                desc.read([self.slot[b] for b in newborn], [desc.head_row(self.slot[b]) for b in newborn], device=self.scene.device)
                pairs = tr.PairSet([(row, desc.head_row(self.slot[b])) for _, row, b in cand], desc.R)
                dist = tr.affinity(desc.desc_shape, desc.desc_atlas, pairs).cpu().numpy()
                if self.record:
                    for n, (a, _, b) in enumerate(cand):
                        self.recorded.setdefault('dist', {})[(a, b)] = dist[n].copy()
                    for b in newborn:
                        r = desc.head_row(self.slot[b])
                        self.recorded['head'][b] = (desc.desc_shape[r].clone(), desc.desc_atlas[r].clone())
            for b, (_, row) in lk.decide(d, newborn, cand, dist).items():
                if row is None:
                    carry[self.slot[b]].zero_()
                else:
                    carry[self.slot[b]].copy_(tot[row])
                    self.carried.add(b)
        for k in sorted(k for k, _ in order if self._span(k)[1] == d):        # before _draw frees the slot and a reset can empty it
            row = lk.retire(k, d)
            desc.read([self.slot[k]], [row], device=self.scene.device)
            tot[row].copy_(carry[self.slot[k]] + desc.desc_sums[row])
            if self.record:
                self.recorded['final'][k] = (desc.desc_shape[row].clone(), desc.desc_atlas[row].clone(), desc.desc_sums[row].clone(),
                                             carry[self.slot[k]].clone())
        return {k: lk.identity[k] for k, _ in order}

    def _para_step(self, g, d):
        """The rows of frame g (or None) go into the para stream; the rows of frame d (or None) come out: ({track: [229] on the
        device}, {track: the prefix's last frame})."""
        S = self.slots
        n_new, emit = np.zeros(S, np.int64), np.full(S, -1, np.int64)
        rows, conf = torch.zeros(S, 1, 229, device=self.scene.device), np.zeros((S, 1), np.float32)
        if g is not None and self.held[g]['order']:
            h = self.held[g]
            slots = [self.slot[k] for k, _ in h['order']]
            rows[slots, 0] = h['para_in']
            for s, (k, det) in zip(slots, h['order']):
                n_new[s] = 1
                conf[s, 0] = self._row_conf(k, det, g)
        cover = [k for k, _ in self.held[d]['order']] if d is not None else []
        for k in cover:
            emit[self.slot[k]] = d - self._span(k)[0]
        if not (n_new.any() or cover):
            return {}, {}
        out, _ = self.para_stream.step(n_new, rows, conf, emit)
        out = out.clone()
        seen = self.assoc.n_frames - 1 if g is None else g                               # the last frame whose rows have gone in
        return {k: out[self.slot[k]] for k in cover}, {k: min(seen, self._span(k)[1]) for k in cover}

    def _draw(self, d, sm_rows, ends, ident=None):
        sc, h = self.scene, self.held.pop(d)
        plan, order, P = h['plan'], h['order'], h['plan']['P']
        para = h['para_in']
        if self.smooth and P:
            para = torch.stack([sm_rows[k] for k, _ in order])
        columns = {}
        if ident is not None:
            columns['identity'] = np.array([ident[k] for k, _ in order], np.int32)
            use = np.array([k in self.carried for k, _ in order], np.int32)
            if self.shared_shape and use.any():                               # one shape per identity: the chain so far
                para = para.contiguous() if self.smooth else para.clone(memory_format=torch.contiguous_format)     # (para_in stays as it is)
                slots = np.array([self.slot[k] for k, _ in order], np.int32)
                self.desc.apply_shape(para, slots, self._carry[torch.from_numpy(slots.astype(np.int64)).to(para.device)], use)
        verts = sc.vertices(para) if P else None
        aux = sc.render(para, plan, return_aux=True, vertices=verts)
        rendered = unpack_frames(aux[0].cpu().numpy(), plan['offsets'], plan['shapes'])[0]
        para_h, raw_h = para.cpu().numpy(), h['para_raw'].cpu().numpy()
        people = sc.people(para_h, verts.cpu().numpy() if P else np.zeros((0, 0, 3), np.float32), plan,
                           track_id=np.array([k for k, _ in order], np.int32), observed=np.array([det >= 0 for _, det in order], bool),
                           para_raw=raw_h, prefix_end=np.array([ends.get(k, d) for k, _ in order], np.int32), **columns,
                           **fit_columns(h['fitted'], P))
        for i, (k, _) in enumerate(order):
            self.rows[(k, d)] = (raw_h[i], para_h[i])
            if self._span(k)[1] == d:                                      # the track's last row: its slot is free again
                self.free.append(self.slot.pop(k))
                self.free.sort()
        self.last = {'frame': d, 'plan': plan, 'render_aux': aux}
        return d, rendered, people

    def _step(self, matches):
        """One tick of the pipeline's clock: frame time - box_lag is processed, frame time - box_lag - lag is drawn."""
        F = self.assoc.n_frames
        g, d = self.time - self.box_lag, self.time - self.box_lag - self.lag
        g, d = (g if 0 <= g < F else None), (d if 0 <= d < F else None)
        sm_boxes = self._timed('boxes', lambda: self._box_step(matches, g))
        if g is not None:
            self._timed('infer', lambda: self._process(g, sm_boxes))
            if self.reid:
                self._timed('reid', lambda: self._describe(g))
        sm_rows, ends = self._timed('smooth', lambda: self._para_step(g, d))
        ident = self._timed('reid', lambda: self._identify(d)) if self.reid and d is not None else None
        self.time += 1
        return [self._timed('render', lambda: self._draw(d, sm_rows, ends, ident))] if d is not None else []

    # ---- the interface -------------------------------------------------------------------------------------------------------------------
    def push(self, frame, boxes, keypoints=None):
        """One frame [H,W,3] uint8 with its boxes (and one keypoint array per box) -> [] or [(frame_index, rendered, people)]."""
        if self.time != self.assoc.n_frames:
            raise RuntimeError('StreamDemo: push after flush')
        if keypoints is not None and len(keypoints) != len(boxes):
            raise ValueError('StreamDemo: keypoints must hold one array per box')
        f = self.assoc.n_frames
        matches, _ = self._timed('associate', lambda: self.assoc.push(boxes))
        self.held[f] = {'frame': frame, 'boxes': list(boxes), 'kps': keypoints}
        self.max_held = max(self.max_held, len(self.held))
        return self._step(matches)

    def joints(self, para, chunk=256):
        return torch.cat([from_para(self.scene.smpl, para[i:i + chunk]).smpl_joints.detach() for i in range(0, para.shape[0], chunk)], 0)

    def flush(self):
        """-> (the frames not drawn yet, in order, VideoDemo's summary of the whole stream).  self.tracks / self.para_raw / self.para
        / self.boxes_raw / self.boxes
        then hold the TrackSet and the rows of everything drawn, track-major."""
        F = self.assoc.n_frames
        rest = []
        while self.held:
            rest += self._step([])
        ts = self.assoc.trackset()
        summary = {'tracks': ts.K, 'rows': ts.N, 'gap_rows': int((ts.det < 0).sum()), 'frames': F}
        keys = list(zip(ts.track.tolist(), ts.frame.tolist()))
        raw = np.stack([self.rows[k][0] for k in keys]) if keys else np.zeros((0, 229), np.float32)
        out = np.stack([self.rows[k][1] for k in keys]) if keys else np.zeros((0, 229), np.float32)
        summary.update(accel_summary(lambda rows: self.joints(torch.from_numpy(rows).to(self.scene.device)), raw, out, ts))
        self.tracks, self.para_raw, self.para = ts, raw, out
        if self.reid:
            self.identity, self.links, self.link_cost = self.linker.arrays(ts.K)
            summary.update({'identities': self.linker.n_identities, 'links': len(self.linker.links)})
        zero = np.zeros(3, np.float32)
        self.boxes_raw = np.stack([zero if self.box_rows[k][0] is None else self.box_rows[k][0] for k in keys]) if keys else np.zeros((0, 3), np.float32)
        self.boxes = np.stack([self.box_rows[k][1] for k in keys]) if keys else np.zeros((0, 3), np.float32)
        return rest, summary
