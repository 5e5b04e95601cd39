"""Video tracks (DESIGN.md 4b'-track "the track rule"): boxes of the frames of a clip associated into tracks on the host, and the rows
of a track smoothed on the GPU.

    ts = associate(boxes)                                   # per frame a list of (center [2], scale[, confidence]) -> TrackSet
    boxes_s, status = smooth(values, ts, lam_vel, lam_acc)  # [N,C] rows, track-major (csrc/track_ops.hip, two launches)
    para_s, status = smooth_para(para, ts)                  # [N,229] rows: cam, betas and the 6D columns smoothed, matrices rebuilt
    a, n = accel(joints, ts)                                # [N,J,3] -> the mean second difference per track

Rows are track-major: track k owns rows track_start[k] .. track_start[k+1]-1, one per frame of its span; frames inside the span
without a detection are gap rows (det -1, conf 0), which the smoother fills.  scene.SceneDemo orders people frame-major;
TrackSet.person_row / row_person are the permutation between the two.  There is no CPU path for the three ops."""
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


def associate(boxes, max_gap=5, min_iou=0.3):
    """boxes: per frame a list of (center [2], scale) or (center, scale, confidence in (0, 1]) -> TrackSet.  Greedy IoU matching of
    every frame's squares against the last observed square of the live tracks (DESIGN.md 4b'-track); float64, deterministic."""
    if int(max_gap) != max_gap or max_gap < 1 or not 0.0 <= float(min_iou) <= 1.0:
        raise ValueError('associate: max_gap %r (an integer >= 1), min_iou %r (in [0, 1])' % (max_gap, min_iou))
    tracks = []                                                    # per track: list of (frame, det, conf), and the last square
    for f, dets in enumerate(boxes):
        sq = []
        for b in dets:
            c, s = np.asarray(b[0], np.float64).reshape(2), float(b[1])
            cf = float(b[2]) if len(b) > 2 else 1.0
            if not (np.isfinite(c).all() and np.isfinite(s) and s > 0 and 0.0 < cf <= 1.0):
                raise ValueError('associate: frame %d: a box needs a finite center, a positive scale and a confidence in (0, 1]' % f)
            sq.append((c, s, cf))
        cand = []
        for k, tr in enumerate(tracks):
            if f - tr['rows'][-1][0] > max_gap:
                continue
            for d, (c, s, _) in enumerate(sq):
                iou = square_iou(tr['c'], tr['s'], c, s)
                if iou >= min_iou:
                    cand.append((-iou, k, d))
        cand.sort()
        used_k, used_d = set(), set()
        for _, k, d in cand:
            if k in used_k or d in used_d:
                continue
            used_k.add(k)
            used_d.add(d)
            tracks[k]['rows'].append((f, d, sq[d][2]))
            tracks[k]['c'], tracks[k]['s'] = sq[d][0], sq[d][1]
        for d, (c, s, cf) in enumerate(sq):
            if d not in used_d:
                tracks.append({'rows': [(f, d, cf)], 'c': c, 's': s})
    start, frame, det, conf = [0], [], [], []
    for tr in tracks:
        seen = {r[0]: r for r in tr['rows']}
        for f in range(tr['rows'][0][0], tr['rows'][-1][0] + 1):
            r = seen.get(f, (f, -1, 0.0))
            frame.append(f)
            det.append(r[1])
            conf.append(r[2])
        start.append(len(frame))
    return TrackSet(start, frame, det, conf, len(boxes))


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
