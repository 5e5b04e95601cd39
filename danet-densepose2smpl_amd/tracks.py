"""Video tracks (DESIGN.md 4b'-track "the track rule"): boxes of the frames of a clip associated into tracks on the host, and the rows
of a track smoothed on the GPU.

    ts = associate(boxes)                                   # per frame a list of (center [2], scale[, confidence]) -> TrackSet
    boxes_s, status = smooth(values, ts, lam_vel, lam_acc)  # [N,C] rows, track-major (csrc/track_ops.hip, two launches)
    para_s, status = smooth_para(para, ts)                  # [N,229] rows: cam, betas and the 6D columns smoothed, matrices rebuilt
    a, n = accel(joints, ts)                                # [N,J,3] -> the mean second difference per track

Rows are track-major: track k owns rows track_start[k] .. track_start[k+1]-1, one per frame of its span; frames inside the span
without a detection are gap rows (det -1, conf 0), which the smoother fills.  scene.SceneDemo orders people frame-major;
TrackSet.person_row / row_person are the permutation between the two.  There is no CPU path for the three ops.

The same fed one frame at a time (DESIGN.md 4b'-stream "the stream rule"):

    a = OnlineAssociator(); matches, died = a.push(dets); a.trackset()     # associate(), a frame at a time
    sm = StreamSmoother(slots, lag, para=True)                              # csrc/track_stream.hip, one launch per step
    out, valid = sm.step(n_new, rows, conf, emit)                           # the offline rule on each slot's rows so far, read at row emit

Identities (DESIGN.md 4b'-link "the identity rule"; csrc/track_link.hip): the tracks of one person linked by shape and fused texture:

    shape, atlas, _ = descriptors(para_s, ts, atlas_builder)               # [K,10] mean betas (one launch), [K,24,T,T,4] fused texture
    pairs = candidates(ts, max_absence)                                     # host: b begins 1 .. max_absence frames after a ends
    dist = affinity(shape, atlas, pairs)                                    # [C,4] = (d_shape, d_app, overlap, S), one launch
    res = link(ts, dist, pairs)                                             # host, float64: identity [K], links [L,2], link_cost [L]
    para_i, mean, status = share_shape(para_s, ts, res['identity'])        # one shape per identity, one launch

Identities while streaming (DESIGN.md 4b'-reid "the causal identity rule"; csrc/track_reid.hip): the same descriptors as running sums:

    sd = StreamDescriptor(slots, gallery, texture_atlas)                    # per slot the unnormalised texel sums and the shape sums
    sd.step(images, vertices, cam, depth, para, conf, slot, observed)       # a frame's people, one launch; read() = descriptors() so far
    lk = OnlineLinker(gallery)                                              # host, float64: a track is decided once, at its first drawn frame"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream
from .ops import _ascending, _device_key, _f32, _host_i32, _int, _per_device, _shape, _texture_size, _typed, _workspace

PARA = 229
CHANNELS = 157
DEFAULT_LAM = ((0.0, 3.0), (0.0, 10.0), (0.0, 10.0))        # (lam_vel, lam_acc) of cam, betas, rotations: DESIGN.md, the recovery case
BOX_LAM = (0.0, 10.0)


def square_iou(ca, sa, cb, sb):
    """IoU of two squares of side 200 * scale around their centers, float64."""
    ha, hb = 100.0 * float(sa), 100.0 * float(sb)
    w = min(ca[0] + ha, cb[0] + hb) - max(ca[0] - ha, cb[0] - hb)
    h = min(ca[1] + ha, cb[1] + hb) - max(ca[1] - ha, cb[1] - hb)
    inter = max(w, 0.0) * max(h, 0.0)
    union = 4.0 * ha * ha + 4.0 * hb * hb - inter
    return inter / union if union > 0 else 0.0


class TrackSet(object):
    """K tracks over N rows.  track_start [K+1] int32 (CSR), frame [N] int32, det [N] int32 (the detection's index in its frame, -1 for
    a gap row), conf [N] float32 (0 for a gap row), n_frames.  person_row [N]: the row of SceneDemo's p-th person when every row, gap
    rows included, is a box of its frame (frame-major; inside a frame the detections in their order, then the gap rows by track);
    row_person [N] its inverse; track [N] the track of each row."""

    def __init__(self, track_start, frame, det, conf, n_frames):
        self.track_start = np.ascontiguousarray(track_start, np.int32)
        self.frame = np.ascontiguousarray(frame, np.int32)
        self.det = np.ascontiguousarray(det, np.int32)
        self.conf = np.ascontiguousarray(conf, np.float32)
        self.n_frames = int(n_frames)
        N = self.frame.size
        if self.track_start.ndim != 1 or self.track_start.size < 1 or self.det.shape != (N,) or self.conf.shape != (N,):
            raise ValueError('TrackSet: track_start [K+1], frame / det / conf [N] expected')
        self.check('TrackSet')
        self.track = np.repeat(np.arange(self.K, dtype=np.int32), np.diff(self.track_start))
        gap = self.det < 0
        self.person_row = np.lexsort((np.where(gap, self.track, self.det), gap, self.frame)).astype(np.int64)
        self.row_person = np.empty(N, np.int64)
        self.row_person[self.person_row] = np.arange(N)
        self._dev = {}
        self._groups = None                                              # track_groups' RowGroups

    def check(self, what):
        """The invariants of the fields, which are plain arrays anyone can assign to: the constructor and every op ask."""
        if self.K:
            _ascending(self.track_start, self.N, what + ': track_start', integers=True)
        elif self.N or self.track_start[0] != 0:
            raise ValueError('%s: rows without a track' % what)
        if not (np.isfinite(self.conf).all() and (self.conf >= 0).all()):
            raise ValueError('%s: conf must be finite and not negative' % what)

    @property
    def K(self):
        return self.track_start.size - 1

    @property
    def N(self):
        return self.frame.size

    @property
    def observed(self):
        return self.det >= 0

    def with_conf(self, conf):
        """The same tracks with other row weights [N] (finite, not negative)."""
        return TrackSet(self.track_start, self.frame, self.det, conf, self.n_frames)

    def device(self, device):
        """(track_start, conf) on `device`, uploaded at the first call and kept: no copy inside a captured region afterwards."""
        return _per_device(self._dev, device, lambda: (torch.from_numpy(self.track_start).to(device), torch.from_numpy(self.conf).to(device)))

    def arrays(self):
        return {'track_start': self.track_start, 'frame': self.frame, 'det': self.det, 'conf': self.conf, 'person_row': self.person_row,
                'row_person': self.row_person}


class OnlineAssociator(object):
    """The association of DESIGN.md 4b'-track fed one frame at a time (4b'-stream): greedy IoU matching of a frame's squares against
    the last observed square of the live tracks, float64, deterministic.  The rule never looks ahead, so trackset() after any number
    of frames is associate() of those frames, array for array.

        matches, died = a.push(dets)      # dets: a list of (center [2], scale) or (center, scale, confidence in (0, 1])
        ts = a.trackset()

    tracks: per track {'rows': [(frame, det, conf) of its observed rows], 'c', 's': its last square}; ids are list positions."""

    def __init__(self, max_gap=5, min_iou=0.3, what='OnlineAssociator'):
        if int(max_gap) != max_gap or max_gap < 1 or not 0.0 <= float(min_iou) <= 1.0:
            raise ValueError('%s: max_gap %r (an integer >= 1), min_iou %r (in [0, 1])' % (what, max_gap, min_iou))
        self.max_gap, self.min_iou, self.what = int(max_gap), float(min_iou), what
        self.tracks = []
        self.n_frames = 0

    def push(self, dets):
        """-> (this frame's [(track_id, det)] in detection order, the ids of the tracks that have just died: their last observed
        frame now lies max_gap frames back, so no later frame can extend them)."""
        f, tracks = self.n_frames, self.tracks
        sq = []
        for b in dets:
            c, s = np.asarray(b[0], np.float64).reshape(2), float(b[1])
            cf = float(b[2]) if len(b) > 2 else 1.0
            if not (np.isfinite(c).all() and np.isfinite(s) and s > 0 and 0.0 < cf <= 1.0):
                raise ValueError('%s: frame %d: a box needs a finite center, a positive scale and a confidence in (0, 1]' % (self.what, f))
            sq.append((c, s, cf))
        cand = []
        for k, tr in enumerate(tracks):
            if f - tr['rows'][-1][0] > self.max_gap:
                continue
            for d, (c, s, _) in enumerate(sq):
                iou = square_iou(tr['c'], tr['s'], c, s)
                if iou >= self.min_iou:
                    cand.append((-iou, k, d))
        cand.sort()
        used_k, used_d = set(), {}
        for _, k, d in cand:
            if k in used_k or d in used_d:
                continue
            used_k.add(k)
            used_d[d] = k
            tracks[k]['rows'].append((f, d, sq[d][2]))
            tracks[k]['c'], tracks[k]['s'] = sq[d][0], sq[d][1]
        for d, (c, s, cf) in enumerate(sq):
            if d not in used_d:
                used_d[d] = len(tracks)
                tracks.append({'rows': [(f, d, cf)], 'c': c, 's': s})
        self.n_frames = f + 1
        died = [k for k, tr in enumerate(tracks) if f - tr['rows'][-1][0] == self.max_gap]
        return [(used_d[d], d) for d in range(len(sq))], died

    def live(self, k):
        """Whether the next frame can still extend track k."""
        return self.n_frames - self.tracks[k]['rows'][-1][0] <= self.max_gap

    def trackset(self):
        start, frame, det, conf = [0], [], [], []
        for tr in self.tracks:
            seen = {r[0]: r for r in tr['rows']}
            for f in range(tr['rows'][0][0], tr['rows'][-1][0] + 1):
                r = seen.get(f, (f, -1, 0.0))
                frame.append(f)
                det.append(r[1])
                conf.append(r[2])
            start.append(len(frame))
        return TrackSet(start, frame, det, conf, self.n_frames)


def associate(boxes, max_gap=5, min_iou=0.3):
    """boxes: per frame a list of (center [2], scale) or (center, scale, confidence in (0, 1]) -> TrackSet.  Greedy IoU matching of
    every frame's squares against the last observed square of the live tracks (DESIGN.md 4b'-track); float64, deterministic."""
    a = OnlineAssociator(max_gap, min_iou, what='associate')
    for dets in boxes:
        a.push(dets)
    return a.trackset()


# ---- the ops ---------------------------------------------------------------------------------------------------------------------
def _trackset(x, what):
    if not isinstance(x, TrackSet):
        raise ValueError('%s: a TrackSet expected, got %s' % (what, type(x).__name__))
    return x


def _tracks(tracks, N, what):
    if _trackset(tracks, what).N != N:
        raise ValueError('%s: %d rows, the TrackSet has %d' % (what, N, tracks.N))
    tracks.check(what)
    return tracks


def _rows(t, shape, what):
    """The host-side part of the argument rule, which needs no device: a floating-point tensor of the shape pattern."""
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise ValueError('%s: a floating-point tensor expected, got %s' % (what, t.dtype if torch.is_tensor(t) else type(t).__name__))
    return _shape(t, shape, what)


def _lam(v, what):
    v = float(v)
    if not (np.isfinite(v) and v >= 0):
        raise ValueError('%s: %r (finite and not negative)' % (what, v))
    return v


def _lam_pairs(lam, what):
    """Three (lam_vel, lam_acc) pairs, for cam, betas and the rotations -> the six floats."""
    lam = [tuple(pair) for pair in lam]
    if len(lam) != 3 or any(len(pair) != 2 for pair in lam):
        raise ValueError('%s: lam must hold three (lam_vel, lam_acc) pairs' % what)
    return [_lam(x, what + ': lam') for pair in lam for x in pair]


def _smooth(what, name, rows, width, tracks, lam, channels, call):
    """smooth and smooth_para up to the entry point: rows [N,width] (None: any), lam() the checked weights (asked for after the rows
    and the TrackSet, before the device), `channels` what the workspace is sized for (None: the rows' width) and call(L, v, conf,
    start, host_start, N, C, K, lam, out, status, ws, nws) the launch."""
    N, C = _rows(rows, (None, width), '%s: %s' % (what, name)).shape
    ts = _tracks(tracks, N, what)
    lam = lam()
    if C < 1:
        raise ValueError('%s: no channel' % what)
    require_gpu(rows, what)
    v = _f32(rows, (N, C), '%s: %s' % (what, name))
    out = torch.empty_like(v)
    status = torch.empty(ts.K, device=v.device, dtype=torch.int32)
    if N == 0:
        return out, status.fill_(1) if ts.K else status
    d_start, d_conf = ts.device(v.device)
    L = _lib.lib()
    nws = L.danet_track_smooth_ws_bytes(N, channels or C)
    ws = _workspace(nws, v.device)
    call(L, ptr(v), ptr(d_conf), ptr(d_start), _host_i32(ts.track_start), N, C, ts.K, lam, ptr(out), ptr(status), ptr(ws), nws)
    return out, status


def smooth(values, tracks, lam_vel=BOX_LAM[0], lam_acc=BOX_LAM[1]):
    """values [N,C] on the GPU -> (smoothed [N,C] f32, status [K] int32: 1 where a track has no positive weight and came back as it
    was).  Two launches, no synchronisation, no allocation by data."""
    def call(L, v, conf, start, host_start, N, C, K, lam, out, status, ws, nws):
        check(L.danet_track_smooth(v, conf, start, host_start, N, C, K, lam[0], lam[1], out, status, ws, nws, stream()), 'danet_track_smooth')
    return _smooth('tracks.smooth', 'values', values, None, tracks,
                   lambda: (_lam(lam_vel, 'tracks.smooth: lam_vel'), _lam(lam_acc, 'tracks.smooth: lam_acc')), None, call)


def smooth_para(para, tracks, lam=DEFAULT_LAM, shared_shape=True):
    """para [N,229] on the GPU (cam, betas, 24 matrices) -> (smoothed [N,229] f32, status [K] int32).  `lam`: three (lam_vel, lam_acc)
    pairs, for cam, betas and the rotations.  Three launches, no synchronisation, no allocation by data."""
    def call(L, v, conf, start, host_start, N, C, K, lam, out, status, ws, nws):
        check(L.danet_track_smooth_para(v, conf, start, host_start, N, K, (ctypes.c_double * 6)(*lam), 1 if shared_shape else 0, out, status,
                                        ws, nws, stream()), 'danet_track_smooth_para')
    return _smooth('tracks.smooth_para', 'para', para, PARA, tracks, lambda: _lam_pairs(lam, 'tracks.smooth_para'), CHANNELS, call)


def accel(joints, tracks, joints_ref=None):
    """joints [N,J,3] on the GPU (and joints_ref, the same shape) -> (accel [K] f64, count [K] int32): per track the mean over
    interior rows and joints of |x_{t+1} - 2 x_t + x_{t-1}|, of joints - joints_ref with a reference; 0 and count 0 where T < 3."""
    N, J = _rows(joints, (None, None, 3), 'tracks.accel: joints').shape[:2]
    if joints_ref is not None:
        _rows(joints_ref, (N, J, 3), 'tracks.accel: joints_ref')
    ts = _tracks(tracks, N, 'tracks.accel')
    require_gpu(joints, 'tracks.accel')
    if joints_ref is not None:
        require_gpu(joints_ref, 'tracks.accel: joints_ref')
    x = _f32(joints, (N, J, 3), 'tracks.accel: joints')
    r = _f32(joints_ref, (N, J, 3), 'tracks.accel: joints_ref', optional=True)
    if r is not None and r.device != x.device:
        raise ValueError('tracks.accel: joints and joints_ref must be on one device')
    if J < 1:
        raise ValueError('tracks.accel: no joint')
    a = torch.zeros(ts.K, device=x.device, dtype=torch.float64)
    n = torch.zeros(ts.K, device=x.device, dtype=torch.int32)
    if N == 0:
        return a, n
    d_start, _ = ts.device(x.device)
    check(_lib.lib().danet_track_accel(ptr(x), ptr(r), ptr(d_start), _host_i32(ts.track_start), N, J, ts.K, ptr(a), ptr(n), stream()),
          'danet_track_accel')
    return a, n


# ---- identities (DESIGN.md 4b'-link "the identity rule"; csrc/track_link.hip) -------------------------------------------------------
PARTS = 24
W_MIN = 1e-3
# (max_absence, sigma_s, sigma_a, min_overlap, no_app): DESIGN.md 4b'-link, the default table on link_oracle.recovery_case
LINK_DEFAULTS = {'max_absence': 150, 'sigma_s': 0.3, 'sigma_a': 0.15, 'min_overlap': 0.1, 'no_app': 0.5}
ID_TEXTURE_SIZE = 8


class PairSet(object):
    """C ordered pairs (a, b) of track ids in [0, K): pairs [C,2] int32 on the host, checked here, uploaded at the first use on a
    device and kept (no copy inside a captured region afterwards)."""

    def __init__(self, pairs, K):
        p = np.asarray(pairs)
        if p.size == 0:
            p = np.zeros((0, 2), np.int32)
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError('tracks.PairSet: pairs must be [C,2] integers, got %s %s' % (p.dtype, p.shape))
        K = _int(K, 'tracks.PairSet', 'K', 0)
        if ((p < 0) | (p >= K)).any():
            c = int(np.nonzero(((p < 0) | (p >= K)).any(1))[0][0])
            raise ValueError('tracks.PairSet: pair %d = %s names a track outside [0, %d)' % (c, p[c].tolist(), K))
        self.pairs, self.K = np.ascontiguousarray(p, np.int32), K
        self._dev = {}

    @property
    def C(self):
        return self.pairs.shape[0]

    def device(self, device):
        return _per_device(self._dev, device, lambda: torch.from_numpy(self.pairs).to(device))


def _pairset(pairs, K, what):
    """pairs [C,2] host integers in [0, K), or a PairSet made for K tracks -> the PairSet."""
    ps = pairs if isinstance(pairs, PairSet) else PairSet(pairs, K)
    if ps.K != K:
        raise ValueError('%s: the PairSet was made for %d tracks, there are %d' % (what, ps.K, K))
    return ps


def _span(ts):
    """(first frame [K], last frame [K]) of the tracks of a TrackSet; every track must hold a row."""
    if (np.diff(ts.track_start) < 1).any():
        raise ValueError('tracks: a track without a row')
    return ts.frame[ts.track_start[:-1]].astype(np.int64), ts.frame[ts.track_start[1:] - 1].astype(np.int64)


def link_arguments(what, max_absence, sigma_s, sigma_a, min_overlap, no_app):
    """The checked thresholds of the identity rule as a dict: max_absence an integer >= 1, sigma_s and sigma_a finite and positive,
    min_overlap and no_app finite and not negative."""
    thr = {'max_absence': _int(max_absence, what, 'max_absence', 1)}
    for name, v, positive in (('sigma_s', sigma_s, True), ('sigma_a', sigma_a, True), ('min_overlap', min_overlap, False), ('no_app', no_app, False)):
        v = float(v)
        if not np.isfinite(v) or v < 0 or (positive and v == 0):
            raise ValueError('%s: %s %r (finite and %s)' % (what, name, v, 'positive' if positive else 'not negative'))
        thr[name] = v
    return thr


def candidates(ts, max_absence=LINK_DEFAULTS['max_absence']):
    """The ordered pairs (a, b) with 1 <= first_frame(b) - last_frame(a) <= max_absence, ascending in (a, b): [C,2] int32 (host)."""
    _trackset(ts, 'tracks.candidates')
    A = _int(max_absence, 'tracks.candidates', 'max_absence', 1)
    if ts.K == 0:
        return np.zeros((0, 2), np.int32)
    first, last = _span(ts)
    d = first[None, :] - last[:, None]
    a, b = np.nonzero((d >= 1) & (d <= A))
    return np.stack([a, b], 1).astype(np.int32)


class RowGroups(object):
    """G groups over N rows as a CSR: group_start [G+1] ascending from 0 to N, group_rows [N] a permutation of 0 .. N-1 (host int32,
    checked here); uploaded at the first use on a device and kept."""

    def __init__(self, group_start, group_rows):
        order = np.asarray(group_rows).reshape(-1)
        start = np.asarray(group_start).reshape(-1)
        N = order.size
        if not np.issubdtype(order.dtype, np.integer) or not np.issubdtype(start.dtype, np.integer) or start.size < 1:
            raise ValueError('tracks.RowGroups: group_start [G+1] and group_rows [N] must be integers')
        if start.size > 1:
            _ascending(start, N, 'tracks.RowGroups: group_start', integers=True)
        elif N or start[0] != 0:
            raise ValueError('tracks.RowGroups: rows without a group')
        if N and not np.array_equal(np.sort(order), np.arange(N)):
            raise ValueError('tracks.RowGroups: group_rows must be a permutation of 0 .. %d' % (N - 1))
        self.start, self.rows = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(order, np.int32)
        self._dev = {}

    @property
    def G(self):
        return self.start.size - 1

    @property
    def N(self):
        return self.rows.size

    def device(self, device):
        return _per_device(self._dev, device, lambda: (torch.from_numpy(self.start).to(device), torch.from_numpy(self.rows).to(device)))


def group_mean(para_rows, conf, groups, col0=3, ncol=10, write_back=False):
    """para_rows [N,229] f32 and conf [N] f32 on the GPU (the caller vouches that conf is finite and not negative), groups a
    RowGroups -> (mean [G,ncol] f32 of the columns col0 .. col0 + ncol - 1: sum c x / sum c over the group's rows with c > 0 in the
    CSR's order, double inside, rounded once; status [G] int32: 1 and mean 0 for a group without weight).  With write_back para_rows
    must be a contiguous fp32 tensor and is changed IN PLACE: every row of a group with status 0 gets the mean in those columns.
    One launch (csrc/track_link.hip); G = 0 or N = 0 launches nothing."""
    what = 'tracks.group_mean'
    N = _rows(para_rows, (None, PARA), what + ': para_rows').shape[0]
    _rows(conf, (N,), what + ': conf')
    if not isinstance(groups, RowGroups):
        raise ValueError('%s: a RowGroups expected, got %s' % (what, type(groups).__name__))
    if groups.N != N:
        raise ValueError('%s: %d rows, the groups hold %d' % (what, N, groups.N))
    for name, v in (('col0', col0), ('ncol', ncol)):
        _int(v, what, name)
    if col0 < 0 or ncol < 1 or col0 + ncol > PARA:
        raise ValueError('%s: columns %d .. %d of %d' % (what, col0, col0 + ncol, PARA))
    require_gpu(para_rows, what)
    require_gpu(conf, what + ': conf')
    if write_back:
        rows = _typed(para_rows, torch.float32, (N, PARA), what + ': para_rows (write_back)')
    else:
        rows = _f32(para_rows, (N, PARA), what + ': para_rows')
    c = _f32(conf, (N,), what + ': conf')
    if c.device != rows.device:
        raise ValueError('%s: para_rows and conf must be on one device' % what)
    G = groups.G
    mean = torch.zeros(G, int(ncol), device=rows.device, dtype=torch.float32)
    status = torch.ones(G, device=rows.device, dtype=torch.int32)
    if N == 0 or G == 0:
        return mean, status
    d_start, d_rows = groups.device(rows.device)
    check(_lib.lib().danet_track_group_mean(ptr(rows), ptr(c), ptr(d_start), _host_i32(groups.start), ptr(d_rows), _host_i32(groups.rows), G, N,
                                            int(col0), int(ncol), ptr(mean), ptr(status), 1 if write_back else 0, stream()),
          'danet_track_group_mean')
    return mean, status


def track_groups(ts):
    """Every track a group, its rows in ascending t (made once per TrackSet)."""
    if ts._groups is None:
        ts._groups = RowGroups(ts.track_start, np.arange(ts.N, dtype=np.int32))
    return ts._groups


def descriptors(para_rows, tracks, atlas_builder=None, texture_size=ID_TEXTURE_SIZE):
    """The descriptor of every track: para_rows [N,229] on the GPU, track-major -> (shape [K,10] f32: sum c betas / sum c over the
    track's rows with c > 0, c the TrackSet's conf, one launch; atlas [K,24,T,T,4] f32).  atlas_builder(rows, view_offsets) -> the
    atlas: `rows` the observed rows (det >= 0) of all tracks, track-major and ascending in t (host int64), view_offsets [K+1] host
    int32, the views of track k being rows[view_offsets[k] : view_offsets[k+1]] (texture.TextureAtlas.unwrap's convention).  None:
    no skin, an all-zero atlas of side `texture_size`, which shares no texel with anything.  -> (shape, atlas, status [K] int32)."""
    N = _rows(para_rows, (None, PARA), 'tracks.descriptors: para_rows').shape[0]
    ts = _tracks(tracks, N, 'tracks.descriptors')
    if ts.K and ((np.diff(ts.track_start) < 1).any() or (np.add.reduceat(ts.observed.astype(np.int64), ts.track_start[:-1]) < 1).any()):
        raise ValueError('tracks.descriptors: a track without an observed row')
    require_gpu(para_rows, 'tracks.descriptors')
    p = _f32(para_rows, (N, PARA), 'tracks.descriptors: para_rows')
    shape, status = group_mean(p, ts.device(p.device)[1], track_groups(ts), 3, 10, False)
    obs = np.nonzero(ts.observed)[0].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.add.reduceat(ts.observed.astype(np.int64), ts.track_start[:-1]))]).astype(np.int32) if ts.K \
        else np.zeros(1, np.int32)
    if atlas_builder is None:
        T = _texture_size(texture_size)
        atlas = torch.zeros(ts.K, PARTS, T, T, 4, device=p.device, dtype=torch.float32)
    else:
        atlas = atlas_builder(obs, off)
        if not torch.is_tensor(atlas) or atlas.dim() != 5 or tuple(atlas.shape[:2]) != (ts.K, PARTS) or atlas.shape[2] != atlas.shape[3] \
                or atlas.shape[4] != 4:
            raise ValueError('tracks.descriptors: the builder gave %s, expected [%d,24,T,T,4]' % (tuple(getattr(atlas, 'shape', ())), ts.K))
        atlas = _f32(atlas, None, 'tracks.descriptors: atlas')
    return shape, atlas, status


def affinity(shape, atlas, pairs):
    """shape [K,10], atlas [K,24,T,T,4] on the GPU, pairs: [C,2] host integers in [0, K) or a PairSet -> dist [C,4] f32 on the GPU:
    (d_shape, d_app, overlap, S) of every ordered pair (DESIGN.md 4b'-link).  One launch; C = 0 launches nothing."""
    K = _rows(shape, (None, 10), 'tracks.affinity: shape').shape[0]
    _rows(atlas, (K, PARTS, None, None, 4), 'tracks.affinity: atlas')
    T = atlas.shape[2]
    if atlas.shape[3] != T or T < 2 or T > 4096:
        raise ValueError('tracks.affinity: atlas %s, expected [K,24,T,T,4] with T in [2, 4096]' % (tuple(atlas.shape),))
    ps = _pairset(pairs, K, 'tracks.affinity')
    require_gpu(shape, 'tracks.affinity')
    require_gpu(atlas, 'tracks.affinity: atlas')
    s = _f32(shape, (K, 10), 'tracks.affinity: shape')
    a = _f32(atlas, (K, PARTS, T, T, 4), 'tracks.affinity: atlas')
    if a.device != s.device:
        raise ValueError('tracks.affinity: shape and atlas must be on one device')
    out = torch.empty(ps.C, 4, device=s.device, dtype=torch.float32)
    if ps.C == 0:
        return out
    check(_lib.lib().danet_track_affinity(ptr(s), ptr(a), K, T, ptr(ps.device(s.device)), _host_i32(ps.pairs), ps.C, ptr(out), stream()),
          'danet_track_affinity')
    return out


def link(tracks, dist, pairs, max_absence=LINK_DEFAULTS['max_absence'], sigma_s=LINK_DEFAULTS['sigma_s'], sigma_a=LINK_DEFAULTS['sigma_a'],
         min_overlap=LINK_DEFAULTS['min_overlap'], no_app=LINK_DEFAULTS['no_app']):
    """The linking of DESIGN.md 4b'-link, host, float64, deterministic.  dist [C,4] (affinity's rows; a tensor or an array) of the
    pairs [C,2].  A pair is a candidate where 1 <= first_frame(b) - last_frame(a) <= max_absence; its cost is d_shape / sigma_s^2 +
    d_app / sigma_a^2 where overlap >= min_overlap and d_shape / sigma_s^2 + no_app elsewhere; candidates with cost <= 1, sorted by
    (cost, a, b), are accepted greedily while a has no successor and b no predecessor.  -> dict: 'identity' [K] int32 (chains numbered
    by their first track's id), 'links' [L,2] int32 in acceptance order, 'link_cost' [L] float64, 'pairs' [C,2] int32, 'cost' [C]
    float64 (inf outside the time window) and 'admissible' [C] bool (inside the window)."""
    what = 'tracks.link'
    K = _trackset(tracks, what).K
    ps = _pairset(pairs, K, what)
    d = dist.detach().cpu().numpy() if torch.is_tensor(dist) else np.asarray(dist)
    if d.shape != (ps.C, 4) or not np.issubdtype(d.dtype, np.floating):
        raise ValueError('%s: dist must be [%d,4] floating point, got %s %s' % (what, ps.C, d.dtype, d.shape))
    d = d.astype(np.float64)
    thr = link_arguments(what, max_absence, sigma_s, sigma_a, min_overlap, no_app)
    A = thr['max_absence']
    p = ps.pairs.astype(np.int64)
    if K:
        first, last = _span(tracks)
        gap = first[p[:, 1]] - last[p[:, 0]]
    else:
        gap = np.zeros(0, np.int64)
    ok = (gap >= 1) & (gap <= A)
    if not np.isfinite(d[ok]).all():
        raise ValueError('%s: a non-finite distance in an admissible pair' % what)
    with np.errstate(invalid='ignore'):
        app = np.where(d[:, 2] >= thr['min_overlap'], d[:, 1] / thr['sigma_a'] ** 2, thr['no_app'])
        cost = np.where(ok, d[:, 0] / thr['sigma_s'] ** 2 + app, np.inf)
    keep = np.nonzero(cost <= 1.0)[0]
    keep = keep[np.lexsort((p[keep, 1], p[keep, 0], cost[keep]))]
    succ, pred, links, link_cost = {}, {}, [], []
    for c in keep:
        a, b = int(p[c, 0]), int(p[c, 1])
        if a in succ or b in pred:
            continue
        succ[a], pred[b] = b, a
        links.append((a, b))
        link_cost.append(cost[c])
    identity = np.full(K, -1, np.int32)
    n = 0
    for k in range(K):                                                      # chains in the order of their first track's id
        if k in pred:
            continue
        j = k
        while True:
            identity[j] = n
            if j not in succ:
                break
            j = succ[j]
        n += 1
    return {'identity': identity, 'links': np.array(links, np.int32).reshape(-1, 2), 'link_cost': np.array(link_cost, np.float64),
            'pairs': ps.pairs, 'cost': cost, 'admissible': ok}


def identity_groups(tracks, identity):
    """The rows of every identity as a RowGroups, ascending in (track id, t) inside an identity."""
    idn = np.asarray(identity)
    if idn.shape != (tracks.K,) or not np.issubdtype(idn.dtype, np.integer):
        raise ValueError('tracks.share_shape: identity must be [%d] integers, got %s %s' % (tracks.K, idn.dtype, idn.shape))
    G = int(idn.max()) + 1 if idn.size else 0
    if idn.size and (idn.min() < 0 or np.unique(idn).size != G):
        raise ValueError('tracks.share_shape: identity must use every number of 0 .. %d' % (G - 1))
    row_id = idn.astype(np.int64)[tracks.track]
    order = np.argsort(row_id, kind='stable').astype(np.int32)              # stable: rows stay ascending in (track id, t) inside a group
    start = np.concatenate([[0], np.cumsum(np.bincount(row_id, minlength=G))]).astype(np.int32)
    return RowGroups(start, order)


def share_shape(para_rows, tracks, identity):
    """One shape per identity: para_rows [N,229] on the GPU, track-major; identity [K] host integers (link's) -> (rows [N,229] f32, a
    new tensor whose betas are, per identity, sum c betas / sum c over all rows of its tracks with c > 0, in ascending (track id, t),
    c the TrackSet's conf; mean [G,10] f32; status [G] int32, 1 for an identity without weight, whose rows come back bit for bit).
    One launch."""
    N = _rows(para_rows, (None, PARA), 'tracks.share_shape: para_rows').shape[0]
    ts = _tracks(tracks, N, 'tracks.share_shape')
    groups = identity if isinstance(identity, RowGroups) else identity_groups(ts, identity)
    require_gpu(para_rows, 'tracks.share_shape')
    out = _f32(para_rows, (N, PARA), 'tracks.share_shape: para_rows').clone()
    mean, status = group_mean(out, ts.device(out.device)[1], groups, 3, 10, True)
    return out, mean, status


# ---- the stream ------------------------------------------------------------------------------------------------------------------
class StreamSmoother(object):
    """The fixed-lag smoother of DESIGN.md 4b'-stream (csrc/track_stream.hip, one launch per step): `slots` tracks whose rows arrive
    at most `max_new` per step; the row emitted for a slot is smooth / smooth_para of the rows the slot holds so far, read at a row at
    most `lag` rows behind the newest.

        sm = StreamSmoother(slots, lag, max_new=1, channels=C)                  # the plain form, lam = (lam_vel, lam_acc)
        sm = StreamSmoother(slots, lag, para=True, shared_shape=True)           # [.,229] rows, lam = three pairs
        out, valid = sm.step(n_new, rows, conf, emit)
        sm.reset(slot)

    step: n_new [S] integers in 0..max_new, conf [S,max_new] and emit [S] (the absolute row of the slot to emit, in
    [T - 1 - lag, T - 1] for a slot of T rows after the step, or -1) are HOST arrays, checked against a host mirror of every slot's
    row count (`count`); rows [S,max_new,C] (para: [S,max_new,229]) is a GPU tensor, of which rows with conf 0 are never read.
    -> (out [S,C] or [S,229] f32, valid [S] int32): the smoother's own tensors, overwritten by the next step.  Everything is checked
    before anything is launched, and a refused step changes nothing.

    Under torch.cuda.graph: capture launch(rows) on a static rows tensor, then per step refill rows, call commands(n_new, conf,
    emit) (checked as in step; it uploads into the smoother's static command tensors) and replay."""

    def __init__(self, slots, lag, max_new=1, channels=None, para=False, lam=None, shared_shape=True, device=None):
        what = 'tracks.StreamSmoother'
        for name, v, low in (('slots', slots, 1), ('lag', lag, 0), ('max_new', max_new, 1)):
            _int(v, what, name, low)
        if bool(para) == (channels is not None):
            raise ValueError('%s: either channels=C or para=True' % what)
        if not para:
            _int(channels, what, 'channels', 1)
        self.S, self.lag, self.max_new, self.para, self.shared_shape = int(slots), int(lag), int(max_new), bool(para), bool(shared_shape)
        self.C = CHANNELS if para else int(channels)
        self.width = PARA if para else self.C
        if para:
            self.lam = _lam_pairs(DEFAULT_LAM if lam is None else lam, what)
        else:
            lam = tuple(BOX_LAM if lam is None else lam)
            if len(lam) != 2:
                raise ValueError('%s: lam must be a (lam_vel, lam_acc) pair' % what)
            self.lam = [_lam(x, what + ': lam') for x in lam]
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise RuntimeError(_lib.GPU_ONLY % (what, self.device))
        self.count = np.zeros(self.S, np.int64)                          # the host mirror: rows per slot
        self._reset = np.zeros(self.S, np.int32)
        self.state = None

    # ---- host side -----------------------------------------------------------------------------------------------------------------
    def reset(self, slot):
        """Empty a slot: the next step clears it on the device before its rows are appended."""
        slot = _int(slot, 'tracks.StreamSmoother.reset', 'slot', 0, self.S - 1)
        self.count[slot] = 0
        self._reset[slot] = 1

    def _check(self, n_new, conf, emit):
        what, S, M = 'tracks.StreamSmoother.step', self.S, self.max_new
        n_new, emit, conf = np.asarray(n_new), np.asarray(emit), np.asarray(conf)
        for name, a in (('n_new', n_new), ('emit', emit)):
            if a.shape != (S,) or not np.issubdtype(a.dtype, np.integer):
                raise ValueError('%s: %s must be [%d] integers, got %s %s' % (what, name, S, a.dtype, a.shape))
        if conf.shape != (S, M) or not np.issubdtype(conf.dtype, np.floating):
            raise ValueError('%s: conf must be [%d,%d] floating point, got %s %s' % (what, S, M, conf.dtype, conf.shape))
        if ((n_new < 0) | (n_new > M)).any():
            raise ValueError('%s: n_new must lie in 0..%d, got %s' % (what, M, n_new.tolist()))
        used = np.arange(M)[None] < n_new[:, None]
        conf = np.where(used, conf, 0.0).astype(np.float32)
        if not (np.isfinite(conf).all() and (conf >= 0).all()):
            raise ValueError('%s: conf must be finite and not negative' % what)
        first = (self.count == 0) & (n_new > 0)
        if (conf[first, 0] <= 0).any():
            raise ValueError('%s: the first row of slots %s has no weight' % (what, np.nonzero(first & (conf[:, 0] <= 0))[0].tolist()))
        T = self.count + n_new
        bad = (emit != -1) & ((emit < np.maximum(T - 1 - self.lag, 0)) | (emit > T - 1))
        if bad.any():
            s = int(np.nonzero(bad)[0][0])
            raise ValueError('%s: emit %d of slot %d lies outside [%d, %d]' % (what, emit[s], s, max(T[s] - 1 - self.lag, 0), T[s] - 1))
        return n_new.astype(np.int32), conf, emit.astype(np.int32), T

    def _check_rows(self, rows):
        _rows(rows, (self.S, self.max_new, self.width), 'tracks.StreamSmoother.step: rows')

    def _alloc(self, device):
        if self.state is not None:
            if device != self.state.device:
                raise ValueError('tracks.StreamSmoother: rows on %s, the state is on %s' % (device, self.state.device))
            return
        if self.device is not None and _device_key(device) != _device_key(self.device):
            raise ValueError('tracks.StreamSmoother: rows on %s, the smoother was made for %s' % (device, self.device))
        nb = _lib.lib().danet_track_stream_state_bytes(self.S, self.C, self.lag, self.max_new)
        if nb == 0:
            raise ValueError('tracks.StreamSmoother: sizes out of range (slots %d, channels %d, lag %d, max_new %d)' % (self.S, self.C, self.lag, self.max_new))
        self.state_bytes = nb
        self.state = torch.zeros(nb // 8, device=device, dtype=torch.int64)
        self.cmd = torch.zeros(3, self.S, device=device, dtype=torch.int32)          # n_new, reset, emit
        self.cmd[2].fill_(-1)
        self.conf = torch.zeros(self.S, self.max_new, device=device, dtype=torch.float32)
        self.out = torch.zeros(self.S, self.width, device=device, dtype=torch.float32)
        self.valid = torch.zeros(self.S, device=device, dtype=torch.int32)

    def _commit(self, n_new, conf, emit, T, device):
        self._alloc(device)
        self.cmd.copy_(torch.from_numpy(np.stack([n_new, self._reset, emit])))
        self.conf.copy_(torch.from_numpy(conf))
        self.count[:] = T
        self._reset[:] = 0

    # ---- the op ----------------------------------------------------------------------------------------------------------------------
    def commands(self, n_new, conf, emit, device=None):
        """The checked half of step: the commands go into the smoother's static tensors and the mirror advances; no launch."""
        n_new, conf, emit, T = self._check(n_new, conf, emit)
        if device is None:
            device = self.state.device if self.state is not None else (self.device or torch.device('cuda', torch.cuda.current_device()))
        self._commit(n_new, conf, emit, T, torch.device(device))

    def launch(self, rows):
        """The launch alone, on the commands last given: -> (out, valid).  The caller vouches for what commands() checked."""
        self._check_rows(rows)
        require_gpu(rows, 'tracks.StreamSmoother')
        self._alloc(rows.device)
        r = _f32(rows, (self.S, self.max_new, self.width), 'tracks.StreamSmoother: rows')
        L = _lib.lib()
        if self.para:
            check(L.danet_track_stream_step_para(ptr(self.state), self.state_bytes, self.S, self.lag, self.max_new, ptr(self.cmd[0]), ptr(self.cmd[1]),
                                                 ptr(r), ptr(self.conf), ptr(self.cmd[2]), (ctypes.c_double * 6)(*self.lam),
                                                 1 if self.shared_shape else 0, ptr(self.out), ptr(self.valid), stream()),
                  'danet_track_stream_step_para')
        else:
            check(L.danet_track_stream_step(ptr(self.state), self.state_bytes, self.S, self.C, self.lag, self.max_new, ptr(self.cmd[0]),
                                            ptr(self.cmd[1]), ptr(r), ptr(self.conf), ptr(self.cmd[2]), self.lam[0], self.lam[1], ptr(self.out),
                                            ptr(self.valid), stream()), 'danet_track_stream_step')
        return self.out, self.valid

    def step(self, n_new, rows, conf, emit):
        self._check_rows(rows)
        n_new, conf, emit, T = self._check(n_new, conf, emit)
        require_gpu(rows, 'tracks.StreamSmoother.step')
        self._commit(n_new, conf, emit, T, rows.device)
        return self.launch(rows)


# ---- identities while streaming (DESIGN.md 4b'-reid "the causal identity rule"; csrc/track_reid.hip) ---------------------------------
# (max_absence, sigma_s, sigma_a, min_overlap, no_app): DESIGN.md 4b'-reid, the table at heads of lag + 1 = 9 rows on the recovery case
REID_DEFAULTS = {'max_absence': 150, 'sigma_s': 0.4, 'sigma_a': 0.2, 'min_overlap': 0.1, 'no_app': 0.5}
REID_GALLERY = 64


def _host_ints(a, n, what, low, high, unique=False):
    """A host array of n whole numbers in [low, high] (bools count as 0 / 1) -> int32; `unique`: no value >= 0 twice."""
    a = np.asarray(a)
    if a.dtype == bool:
        a = a.astype(np.int32)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s must be [%d] integers, got %s %s' % (what, n, a.dtype, a.shape))
    if ((a < low) | (a > high)).any():
        raise ValueError('%s must lie in %d..%d, got %s' % (what, low, high, a.tolist()))
    if unique:
        used = a[a >= 0]
        if np.unique(used).size != used.size:
            raise ValueError('%s names a value twice: %s' % (what, a.tolist()))
    return np.ascontiguousarray(a, np.int32)


class StreamDescriptor(object):
    """The descriptor of the identity rule (descriptors(): a track's weighted mean shape and the texture fused over its observed rows)
    kept as running sums for `slots` tracks, one frame at a time (csrc/track_reid.hip; DESIGN.md 4b'-reid).  `texture`: the
    texture.TextureAtlas whose topology, chart size T and focal length the skin uses; `gallery`: the rows of the descriptor table kept
    for finished tracks.

        sd = StreamDescriptor(slots, gallery, texture)
        sd.step(images, vertices, cam, depth, para, conf, slot, observed)     # one launch: a frame's people go into their slots
        shape, atlas, status = sd.read(slots, rows)                           # one launch: descriptors -> rows of the table
        sd.apply_shape(rows, slot, carry, use)                                # one launch: the identity's shape into emitted rows
        sd.reset(slot)                                                        # the next step empties the slot first

    step: images [P,3,H,H] in [0,1], vertices [P,NV,3], cam [P,3], depth [P,H,H] (depth_planes() makes it as TextureAtlas.unwrap does),
    para [P,229] and conf [P] are GPU tensors (the caller vouches that conf is finite and not negative); slot [P] (-1: the entry is
    empty; no slot twice) and observed [P] (0: a gap row, which adds to the shape with its conf and never to the skin; its image, mesh and
    depth are never read) are HOST arrays.  After any number of steps read() gives, bit for bit, TextureAtlas.unwrap over the observed
    rows the slot has taken in their order, and descriptors()' shape over all its rows.

    The table has gallery + slots rows: desc_shape [R,10], desc_atlas [R,24,T,T,4], status [R] (1: no weight yet) and desc_sums [R,11]
    float64, the shape sums (sum c betas, sum c) as they are.  head_row(s) = gallery + s is the row of the track in slot s, so that
    affinity() compares finished tracks with live ones through an ordinary PairSet over R.  apply_shape: rows [P,229], a contiguous
    fp32 GPU tensor changed IN PLACE: where use[p] != 0, slot[p] >= 0 and carry_c + sum_c > 0 the betas become
    (carry_y + sum_y) / (carry_c + sum_c), carry [P,11] float64 on the GPU; other rows keep their bits.

    Everything is checked before anything is launched and a refused call changes nothing.  Under torch.cuda.graph: capture
    launch(...) on static tensors, then per frame refill them, call commands(slot, observed) and replay."""

    def __init__(self, slots, gallery, texture, device=None):
        from .texture import TextureAtlas
        what = 'tracks.StreamDescriptor'
        self.S, self.G = _int(slots, what, 'slots', 1, 4096), _int(gallery, what, 'gallery', 0, 1 << 16)
        if not isinstance(texture, TextureAtlas):
            raise ValueError('%s: a texture.TextureAtlas expected, got %s' % (what, type(texture).__name__))
        self.tex, self.T, self.R = texture, texture.size, self.G + self.S
        if PARTS * self.T * self.T >= 1 << 24:
            raise ValueError('%s: chart size %d is too large' % (what, self.T))
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise RuntimeError(_lib.GPU_ONLY % (what, self.device))
        self._reset = np.zeros(self.S, np.int32)
        self.state, self._cmd = None, {}

    def head_row(self, slot):
        return self.G + int(slot)

    def reset(self, slot):
        """Empty a slot: the next step clears it on the device before its row is added."""
        self._reset[_int(slot, 'tracks.StreamDescriptor.reset', 'slot', 0, self.S - 1)] = 1

    # ---- host side -----------------------------------------------------------------------------------------------------------------
    def _check(self, slot, observed):
        what = 'tracks.StreamDescriptor.step'
        if np.asarray(slot).ndim != 1:
            raise ValueError('%s: slot must be [P] integers, got shape %s' % (what, np.asarray(slot).shape))
        P = np.asarray(slot).shape[0]
        return _host_ints(slot, P, what + ': slot', -1, self.S - 1, unique=True), _host_ints(observed, P, what + ': observed', 0, 1)

    def _check_rows(self, P, images, vertices, cam, depth, para, conf, what='tracks.StreamDescriptor.step'):
        _rows(images, (P, 3, None, None), what + ': images')
        H = images.shape[2]
        if images.shape[3] != H or H < 1 or H > 4096:
            raise ValueError('%s: images %s, expected square [P,3,H,H]' % (what, tuple(images.shape)))
        _rows(vertices, (P, None, 3), what + ': vertices')
        if vertices.shape[1] < self.tex.num_verts:
            raise ValueError('%s: vertices %s (the topology names %d mesh vertices)' % (what, tuple(vertices.shape), self.tex.num_verts))
        _rows(cam, (P, 3), what + ': cam')
        _rows(depth, (P, H, H), what + ': depth')
        _rows(para, (P, PARA), what + ': para')
        _rows(conf, (P,), what + ': conf')
        for name, t in (('images', images), ('vertices', vertices), ('cam', cam), ('depth', depth), ('para', para), ('conf', conf)):
            require_gpu(t, '%s: %s' % (what, name))
        if len(set(t.device for t in (images, vertices, cam, depth, para, conf))) != 1:
            raise ValueError('%s: the tensors must be on one device' % what)

    def _pick_device(self, device):
        if device is None:
            device = self.state.device if self.state is not None else (self.device or torch.device('cuda', torch.cuda.current_device()))
        return torch.device(device)

    def _alloc(self, device):
        if self.state is not None:
            if device != self.state.device:
                raise ValueError('tracks.StreamDescriptor: tensors on %s, the state is on %s' % (device, self.state.device))
            return
        if self.device is not None and _device_key(device) != _device_key(self.device):
            raise ValueError('tracks.StreamDescriptor: tensors on %s, the descriptor was made for %s' % (device, self.device))
        nb = _lib.lib().danet_track_desc_state_bytes(self.S, self.T)
        if nb == 0:
            raise ValueError('tracks.StreamDescriptor: sizes out of range (slots %d, chart size %d)' % (self.S, self.T))
        self.state_bytes = nb
        self.state = torch.zeros(nb // 8, device=device, dtype=torch.int64)
        self.d_reset = torch.zeros(self.S, device=device, dtype=torch.int32)
        self.desc_shape = torch.zeros(self.R, 10, device=device, dtype=torch.float32)
        self.desc_atlas = torch.zeros(self.R, PARTS, self.T, self.T, 4, device=device, dtype=torch.float32)
        self.desc_sums = torch.zeros(self.R, 11, device=device, dtype=torch.float64)
        self.status = torch.ones(self.R, device=device, dtype=torch.int32)

    def _commit(self, slot, observed, device):
        """The checked commands go into static tensors (one pair per chunk size P); the pending resets go with them."""
        P = slot.size
        if P == 0:
            return                                                        # (nothing is launched: the resets wait for the next step)
        self._alloc(device)
        if P not in self._cmd:
            self._cmd[P] = torch.zeros(2, P, device=device, dtype=torch.int32)
        self._cmd[P].copy_(torch.from_numpy(np.stack([slot, observed])))
        self.d_reset.copy_(torch.from_numpy(self._reset))
        self._host_slot = slot
        self._reset[:] = 0

    # ---- the ops ---------------------------------------------------------------------------------------------------------------------
    def depth_planes(self, vertices, cam, H):
        """The rasteriser's depth plane [P,H,H] of the meshes, as TextureAtlas.unwrap makes it."""
        from . import ops
        v = _f32(vertices, (None, None, 3), 'tracks.StreamDescriptor.depth_planes: vertices')
        c = _f32(cam, (v.shape[0], 3), 'tracks.StreamDescriptor.depth_planes: cam')
        d = self.tex._dev(v.device)
        return ops.iuv_raster(v, c, d['vert_mapping'], d['faces'], d['tex'], self.tex.focal_length, int(H), int(H), return_aux=True)[2]

    def commands(self, slot, observed, device=None):
        """The checked half of step: slot and observed go into the descriptor's static tensors; no launch."""
        slot, observed = self._check(slot, observed)
        self._commit(slot, observed, self._pick_device(device))

    def launch(self, images, vertices, cam, depth, para, conf, depth_tol=0.02, min_cos=0.1):
        """The launch alone, on the commands last given.  The caller vouches for what commands() checked."""
        P = images.shape[0] if torch.is_tensor(images) and images.dim() else -1
        self._check_rows(P, images, vertices, cam, depth, para, conf)
        if P == 0:
            return
        if P not in self._cmd or self._host_slot.size != P:
            raise ValueError('tracks.StreamDescriptor.launch: no commands for a chunk of %d' % P)
        self._alloc(images.device)
        what = 'tracks.StreamDescriptor'
        H = images.shape[2]
        img, v, c = _f32(images, (P, 3, H, H), what), _f32(vertices, (P, None, 3), what), _f32(cam, (P, 3), what)
        dp, pa, cf = _f32(depth, (P, H, H), what), _f32(para, (P, PARA), what), _f32(conf, (P,), what)
        d = self.tex._dev(img.device)
        cmd = self._cmd[P]
        check(_lib.lib().danet_track_desc_step(ptr(self.state), self.state_bytes, self.S, self.T, ptr(img), ptr(v), ptr(c), ptr(dp), P, v.shape[1], H,
                                               ptr(pa), ptr(cf), ptr(cmd[0]), _host_i32(self._host_slot), ptr(cmd[1]), ptr(self.d_reset),
                                               ptr(d['vert_mapping']), d['vert_mapping'].numel(), ptr(d['faces']), d['faces'].shape[0],
                                               ptr(d['map_face']), ptr(d['map_bary']), self.tex.focal_length, float(depth_tol), float(min_cos),
                                               stream()), 'danet_track_desc_step')

    def step(self, images, vertices, cam, depth, para, conf, slot, observed, depth_tol=0.02, min_cos=0.1):
        slot, observed = self._check(slot, observed)
        self._check_rows(slot.size, images, vertices, cam, depth, para, conf)
        self._commit(slot, observed, images.device)
        self.launch(images, vertices, cam, depth, para, conf, depth_tol, min_cos)

    def read(self, slots, rows, device=None):
        """The descriptors of `slots` (host integers in [0, S)) go into the rows `rows` (host integers in [0, R), none twice) of the
        table -> (desc_shape, desc_atlas, status): the descriptor's own tensors.  One launch; no pair launches nothing."""
        what = 'tracks.StreamDescriptor.read'
        if np.asarray(slots).ndim != 1:
            raise ValueError('%s: slots must be [n] integers' % what)
        n = np.asarray(slots).shape[0]
        s, r = _host_ints(slots, n, what + ': slots', 0, self.S - 1), _host_ints(rows, n, what + ': rows', 0, self.R - 1, unique=True)
        self._alloc(self._pick_device(device))
        if n:
            pairs = np.ascontiguousarray(np.stack([s, r], 1), np.int32)
            check(_lib.lib().danet_track_desc_read(ptr(self.state), self.state_bytes, self.S, self.T, ptr(torch.from_numpy(pairs).to(self.state.device)),
                                                   _host_i32(pairs), n, self.R, ptr(self.desc_shape), ptr(self.desc_atlas), ptr(self.desc_sums),
                                                   ptr(self.status), stream()), 'danet_track_desc_read')
        return self.desc_shape, self.desc_atlas, self.status

    def apply_shape(self, rows, slot, carry, use):
        what = 'tracks.StreamDescriptor.apply_shape'
        P = _rows(rows, (None, PARA), what + ': rows').shape[0]
        s, u = _host_ints(slot, P, what + ': slot', -1, self.S - 1), _host_ints(use, P, what + ': use', 0, 1)
        if not torch.is_tensor(carry) or carry.dtype != torch.float64 or tuple(carry.shape) != (P, 11):
            raise ValueError('%s: carry must be a float64 [%d,11] tensor' % (what, P))
        r = _typed(rows, torch.float32, (P, PARA), what + ': rows')
        cy = _typed(carry, torch.float64, (P, 11), what + ': carry')
        if cy.device != r.device:
            raise ValueError('%s: rows and carry must be on one device' % what)
        self._alloc(r.device)
        if P:
            cmd = torch.from_numpy(np.stack([s, u])).to(r.device)
            check(_lib.lib().danet_track_desc_shape(ptr(self.state), self.state_bytes, self.S, self.T, ptr(r), ptr(cmd[0]), _host_i32(s), ptr(cy),
                                                    ptr(cmd[1]), P, stream()), 'danet_track_desc_shape')
        return rows


class OnlineLinker(object):
    """The decisions of the causal identity rule (DESIGN.md 4b'-reid), host, float64, deterministic.  A finished track waits in one of
    `gallery` rows until it gets a successor or has been away for more than max_absence frames; a track is decided once, at its
    first drawn frame, and never again.

        cand = lk.candidates(d, newborn)                 # [(track a, its gallery row, track b)], ascending in (a, b); evicts first
        out = lk.decide(d, newborn, cand, dist)          # dist [C,4]: affinity's rows of cand -> {b: (identity, a's gallery row or None)}
        row = lk.retire(track, last)                     # the track's last row has been drawn: -> its gallery row

    The cost and the greedy acceptance are link()'s.  A linked b takes a's identity, and a's row is free again after decide: the caller
    copies what it keeps per row (the chain totals) before it retires a track.  identity {track: number}, links and link_cost in
    acceptance order."""

    def __init__(self, gallery=REID_GALLERY, max_absence=None, sigma_s=None, sigma_a=None, min_overlap=None, no_app=None):
        what = 'tracks.OnlineLinker'
        given = {'max_absence': max_absence, 'sigma_s': sigma_s, 'sigma_a': sigma_a, 'min_overlap': min_overlap, 'no_app': no_app}
        self.thr = link_arguments(what, **{k: REID_DEFAULTS[k] if v is None else v for k, v in given.items()})
        self.G = _int(gallery, what, 'gallery', 1, 1 << 16)
        self.entries = {}                                                # gallery row -> {'track', 'last', 'identity'}
        self.free = list(range(self.G))
        self.identity, self.links, self.link_cost = {}, [], []
        self.n_identities = 0

    def evict(self, d):
        """Entries with d - last > max_absence leave: no later frame can bring them a successor."""
        for row in [r for r, e in self.entries.items() if d - e['last'] > self.thr['max_absence']]:
            del self.entries[row]
            self.free.append(row)
        self.free.sort()

    def candidates(self, d, newborn):
        self.evict(d)
        rows = sorted((e['track'], r) for r, e in self.entries.items() if 1 <= d - e['last'] <= self.thr['max_absence'])
        return [(a, r, int(b)) for a, r in rows for b in sorted(newborn)]

    def decide(self, d, newborn, cand, dist):
        what = 'tracks.OnlineLinker.decide'
        dist = dist.detach().cpu().numpy() if torch.is_tensor(dist) else np.asarray(dist)
        if dist.shape != (len(cand), 4) or (len(cand) and not np.issubdtype(dist.dtype, np.floating)):
            raise ValueError('%s: dist must be [%d,4] floating point, got %s %s' % (what, len(cand), dist.dtype, dist.shape))
        if any(b in self.identity for b in newborn):
            raise ValueError('%s: a track is decided once' % what)
        dist = dist.astype(np.float64).reshape(-1, 4)
        if not np.isfinite(dist[:, :3]).all():
            raise ValueError('%s: a non-finite distance' % what)
        thr, keep = self.thr, []
        for c, (a, row, b) in enumerate(cand):
            app = dist[c, 1] / thr['sigma_a'] ** 2 if dist[c, 2] >= thr['min_overlap'] else thr['no_app']
            cost = dist[c, 0] / thr['sigma_s'] ** 2 + app
            if cost <= 1.0:
                keep.append((cost, a, b, row))
        keep.sort()
        succ, pred = set(), {}
        for cost, a, b, row in keep:
            if a in succ or b in pred:
                continue
            succ.add(a)
            pred[b] = (a, row)
            self.links.append((a, b))
            self.link_cost.append(cost)
        out = {}
        for b in sorted(newborn):
            if b in pred:
                a, row = pred[b]
                self.identity[b] = self.entries[row]['identity']
                del self.entries[row]
                self.free.append(row)
                out[b] = (self.identity[b], row)
            else:
                self.identity[b] = self.n_identities
                self.n_identities += 1
                out[b] = (self.identity[b], None)
        self.free.sort()
        return out

    def retire(self, track, last):
        if track not in self.identity:
            raise ValueError('tracks.OnlineLinker.retire: track %d has not been decided' % track)
        if not self.free:
            raise RuntimeError('tracks.OnlineLinker: %d finished tracks wait in the gallery and frame %d retires another; the gallery holds %d'
                               % (len(self.entries), last, self.G))
        row = self.free.pop(0)
        self.entries[row] = {'track': int(track), 'last': int(last), 'identity': self.identity[track]}
        return row

    def arrays(self, K):
        """-> (identity [K] int32, links [L,2] int32, link_cost [L] float64), link()'s dtypes."""
        return (np.array([self.identity[k] for k in range(K)], np.int32), np.array(self.links, np.int32).reshape(-1, 2),
                np.array(self.link_cost, np.float64))
