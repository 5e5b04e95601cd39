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
    out, valid = sm.step(n_new, rows, conf, emit)                           # the offline rule on each slot's rows so far, read at row emit"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream
from .ops import _ascending, _f32, _host_i32, _shape, _workspace

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
        if self.K:
            _ascending(self.track_start, N, 'TrackSet: track_start', integers=True)
        elif N or self.track_start[0] != 0:
            raise ValueError('TrackSet: rows without a track')
        if not (np.isfinite(self.conf).all() and (self.conf >= 0).all()):
            raise ValueError('TrackSet: conf must be finite and not negative')
        self.track = np.repeat(np.arange(self.K, dtype=np.int32), np.diff(self.track_start))
        gap = self.det < 0
        self.person_row = np.lexsort((np.where(gap, self.track, self.det), gap, self.frame)).astype(np.int64)
        self.row_person = np.empty(N, np.int64)
        self.row_person[self.person_row] = np.arange(N)
        self._dev = {}

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
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = (torch.from_numpy(self.track_start).to(device), torch.from_numpy(self.conf).to(device))
        return t

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
def _tracks(tracks, N, what):
    if not isinstance(tracks, TrackSet):
        raise ValueError('%s: a TrackSet expected, got %s' % (what, type(tracks).__name__))
    if tracks.N != N:
        raise ValueError('%s: %d rows, the TrackSet has %d' % (what, N, tracks.N))
    if tracks.K:
        _ascending(tracks.track_start, N, what + ': track_start', integers=True)
    if not (np.isfinite(tracks.conf).all() and (tracks.conf >= 0).all()):
        raise ValueError('%s: conf must be finite and not negative' % what)
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


def smooth(values, tracks, lam_vel=BOX_LAM[0], lam_acc=BOX_LAM[1]):
    """values [N,C] on the GPU -> (smoothed [N,C] f32, status [K] int32: 1 where a track has no positive weight and came back as it
    was).  Two launches, no synchronisation, no allocation by data."""
    N, C = _rows(values, (None, None), 'tracks.smooth: values').shape
    ts = _tracks(tracks, N, 'tracks.smooth')
    lv, la = _lam(lam_vel, 'tracks.smooth: lam_vel'), _lam(lam_acc, 'tracks.smooth: lam_acc')
    if C < 1:
        raise ValueError('tracks.smooth: no channel')
    require_gpu(values, 'tracks.smooth')
    v = _f32(values, (N, C), 'tracks.smooth: values')
    out = torch.empty_like(v)
    status = torch.empty(ts.K, device=v.device, dtype=torch.int32)
    if N == 0:
        return out, status.fill_(1) if ts.K else status
    d_start, d_conf = ts.device(v.device)
    L = _lib.lib()
    nws = L.danet_track_smooth_ws_bytes(N, C)
    ws = _workspace(nws, v.device)
    check(L.danet_track_smooth(ptr(v), ptr(d_conf), ptr(d_start), _host_i32(ts.track_start), N, C, ts.K, lv, la, ptr(out), ptr(status),
                               ptr(ws), nws, stream()), 'danet_track_smooth')
    return out, status


def smooth_para(para, tracks, lam=DEFAULT_LAM, shared_shape=True):
    """para [N,229] on the GPU (cam, betas, 24 matrices) -> (smoothed [N,229] f32, status [K] int32).  `lam`: three (lam_vel, lam_acc)
    pairs, for cam, betas and the rotations.  Three launches, no synchronisation, no allocation by data."""
    N = _rows(para, (None, PARA), 'tracks.smooth_para: para').shape[0]
    ts = _tracks(tracks, N, 'tracks.smooth_para')
    lam = [tuple(pair) for pair in lam]
    if len(lam) != 3 or any(len(pair) != 2 for pair in lam):
        raise ValueError('tracks.smooth_para: lam must hold three (lam_vel, lam_acc) pairs')
    flat = [_lam(x, 'tracks.smooth_para: lam') for pair in lam for x in pair]
    require_gpu(para, 'tracks.smooth_para')
    p = _f32(para, (N, PARA), 'tracks.smooth_para: para')
    out = torch.empty_like(p)
    status = torch.empty(ts.K, device=p.device, dtype=torch.int32)
    if N == 0:
        return out, status.fill_(1) if ts.K else status
    d_start, d_conf = ts.device(p.device)
    L = _lib.lib()
    nws = L.danet_track_smooth_ws_bytes(N, CHANNELS)
    ws = _workspace(nws, p.device)
    check(L.danet_track_smooth_para(ptr(p), ptr(d_conf), ptr(d_start), _host_i32(ts.track_start), N, ts.K, (ctypes.c_double * 6)(*flat),
                                    1 if shared_shape else 0, ptr(out), ptr(status), ptr(ws), nws, stream()), 'danet_track_smooth_para')
    return out, status


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
            if isinstance(v, bool) or int(v) != v or v < low:
                raise ValueError('%s: %s %r (an integer >= %d)' % (what, name, v, low))
        if bool(para) == (channels is not None):
            raise ValueError('%s: either channels=C or para=True' % what)
        if not para and (isinstance(channels, bool) or int(channels) != channels or channels < 1):
            raise ValueError('%s: channels %r (an integer >= 1)' % (what, channels))
        self.S, self.lag, self.max_new, self.para, self.shared_shape = int(slots), int(lag), int(max_new), bool(para), bool(shared_shape)
        self.C = CHANNELS if para else int(channels)
        self.width = PARA if para else self.C
        if para:
            lam = [tuple(pair) for pair in (DEFAULT_LAM if lam is None else lam)]
            if len(lam) != 3 or any(len(pair) != 2 for pair in lam):
                raise ValueError('%s: lam must hold three (lam_vel, lam_acc) pairs' % what)
            self.lam = [_lam(x, what + ': lam') for pair in lam for x in pair]
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
        if isinstance(slot, bool) or int(slot) != slot or not 0 <= slot < self.S:
            raise ValueError('tracks.StreamSmoother.reset: slot %r of %d' % (slot, self.S))
        self.count[int(slot)] = 0
        self._reset[int(slot)] = 1

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

    def _rows(self, rows):
        _rows(rows, (self.S, self.max_new, self.width), 'tracks.StreamSmoother.step: rows')

    def _alloc(self, device):
        if self.state is not None:
            if device != self.state.device:
                raise ValueError('tracks.StreamSmoother: rows on %s, the state is on %s' % (device, self.state.device))
            return
        if self.device is not None and torch.device(device) != torch.device(self.device.type, self.device.index if self.device.index is not None
                                                                             else torch.cuda.current_device()):
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
        self._rows(rows)
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
        self._rows(rows)
        n_new, conf, emit, T = self._check(n_new, conf, emit)
        require_gpu(rows, 'tracks.StreamSmoother.step')
        self._commit(n_new, conf, emit, T, rows.device)
        return self.launch(rows)
