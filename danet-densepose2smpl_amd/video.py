"""Video demo: the frames of a clip plus person boxes per frame in, the frames with every person's mesh drawn in place out, the people
followed across frames (tracks.associate), their boxes and rows smoothed along each track (tracks.smooth, tracks.smooth_para;
DESIGN.md 4b'-track "the track rule") and the frames in which a person has no box filled in.

    demo = VideoDemo(model_or_engine, smpl, batch, fitter=None)
    rendered, people, summary = demo(frames, boxes, keypoints=None)

A VideoDemo wraps a scene.SceneDemo and calls its stages; the scene demo itself is what it was.  The whole clip is one call: every
row of every track is on the device at once.  Not here: video decoding, a person detector, online or causal filtering, clips that do
not fit on the device.  There is no CPU path."""
import numpy as np
import torch

from . import tracks as tr
from .scene import SceneDemo, person_cameras, unpack_frames
from .smpl import from_para


class VideoDemo(object):
    """VideoDemo(model_or_engine, smpl, batch, fitter=None, smooth=True, rounds=1, shared_shape=True, max_gap=5, min_iou=0.3,
    gap_conf=0., lam=tracks.DEFAULT_LAM, box_lam=tracks.BOX_LAM, **scene_kw): the first three and `fitter` as scene.SceneDemo takes
    them.  `rounds` times the rows are fitted from their current values (where there is a fitter) and then smoothed: the fitters
    take the start row both as initialisation and as prior, so the alternation is a proximal one.  gap_conf: the weight of a gap
    row's own prediction in the smoother (0: the row is filled from its neighbours alone).  With smooth = False nothing is smoothed
    (gap rows still get an interpolated box), and a clip without gap rows comes out as SceneDemo draws it, bit for bit."""

    def __init__(self, model_or_engine, smpl, batch, fitter=None, smooth=True, rounds=1, shared_shape=True, max_gap=5, min_iou=0.3,
                 gap_conf=0., lam=tr.DEFAULT_LAM, box_lam=tr.BOX_LAM, **scene_kw):
        self.scene = SceneDemo(model_or_engine, smpl, batch, fitter=fitter, **scene_kw)
        self.smooth, self.rounds, self.shared_shape = bool(smooth), int(rounds), bool(shared_shape)
        self.max_gap, self.min_iou, self.gap_conf = int(max_gap), float(min_iou), float(gap_conf)
        self.lam, self.box_lam = tuple(tuple(p) for p in lam), tuple(box_lam)
        if self.rounds < 1 or not (np.isfinite(self.gap_conf) and 0.0 <= self.gap_conf <= 1.0):
            raise ValueError('VideoDemo: rounds %d (>= 1), gap_conf %r (in [0, 1])' % (self.rounds, gap_conf))
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
                b = boxes[ts.frame[n]][ts.det[n]]
                c = np.asarray(b[0], np.float64).reshape(2)
                raw[n] = (c[0], c[1], np.log(float(b[1])))
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
                per_frame[ts.frame[n]].append((sm[n, :2].astype(np.float64), float(np.exp(np.float64(sm[n, 2])))))
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

    def __call__(self, frames, boxes, keypoints=None):
        """-> (rendered frames, people: SceneDemo's dict per frame plus 'track_id' [k], 'observed' [k] and 'para_raw' [k,229] (the
        network's rows), summary: 'tracks', 'rows', 'gap_rows', 'accel_raw' and 'accel' (the mean acceleration of the SMPL joints over
        all tracks' interior rows before and after), 'accel_raw_tracks' / 'accel_tracks' [K])."""
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
        iuv = None
        if P and sc.dense:
            para, iuv = sc.infer(plan, return_iuv=True)
        else:
            para = sc.infer(plan) if P else torch.zeros(0, 229, device=dev)
        para_raw = para
        fitting = sc.fitter is not None and (sc.dense or keypoints is not None)
        fitted = None
        kps = self.person_keypoints(ts, keypoints) if (fitting and keypoints is not None) else None
        for _ in range(self.rounds):
            if fitting:
                fitted = (para, None)
                if P:
                    para_fit, info = sc.fit(para, plan, kps, iuv)
                    fitted, para = (para, info), para_fit
            if not self.smooth or not P:
                break
            rows, _ = tr.smooth_para(para[to_rows], ts_para, self.lam, self.shared_shape)
            para = rows[to_people]
        summary = {'tracks': ts.K, 'rows': ts.N, 'gap_rows': int((ts.det < 0).sum())}
        if P:
            a0, cnt = tr.accel(self.joints(para_raw)[to_rows], ts)
            a1, _ = tr.accel(self.joints(para)[to_rows], ts)
            a0, a1, cnt = a0.cpu().numpy(), a1.cpu().numpy(), cnt.cpu().numpy().astype(np.float64)
        else:
            a0 = a1 = cnt = np.zeros(ts.K)
        w = cnt / cnt.sum() if cnt.sum() > 0 else cnt
        summary.update({'accel_raw': float((a0 * w).sum()), 'accel': float((a1 * w).sum()), 'accel_raw_tracks': a0, 'accel_tracks': a1})
        verts = sc.vertices(para) if P else None
        aux = sc.render(para, plan, return_aux=True, vertices=verts)
        rendered = unpack_frames(aux[0].cpu().numpy(), plan['offsets'], plan['shapes'])
        para_h, raw_h = para.cpu().numpy(), para_raw.cpu().numpy()
        verts_h = verts.cpu().numpy() if P else np.zeros((0, 0, 3), np.float32)
        if P:
            k = person_cameras(para_h[:, 0:3], plan['tinv'], plan['shapes'], plan['person_frame'], sc.res, sc.focal, sc.focal_full)
        track_p, obs_p = ts.track[ts.person_row], ts.det[ts.person_row] >= 0
        people = []
        for n in range(plan['N']):
            m = plan['person_frame'] == n
            people.append({'para': para_h[m], 'cam': para_h[m, 0:3], 'cam_t_full': k['cam_t_full'][m] if P else np.zeros((0, 3)),
                           'focal_full': k['focal_full'][m] if P else np.zeros(0), 'center': plan['center'][m], 'scale': plan['scale'][m],
                           'vertices': verts_h[m], 'track_id': track_p[m], 'observed': obs_p[m], 'para_raw': raw_h[m]})
        if fitted is not None:
            init = fitted[0].cpu().numpy()
            if P:
                hist, it = fitted[1]['history'].cpu().numpy(), fitted[1]['best_iter'].cpu().numpy()
                loss = np.stack([hist[:, 0], hist[np.arange(P), it]], 1)
            else:
                loss, it = np.zeros((0, 2), np.float32), np.zeros(0, np.int32)
            for n in range(plan['N']):
                m = plan['person_frame'] == n
                people[n].update({'para_init': init[m], 'fit_loss': loss[m], 'fit_iter': it[m]})
        self.last = {'tracks': ts, 'plan': plan, 'render_aux': aux, 'boxes_raw': boxes_raw, 'boxes': boxes_s,
                     'para_raw': raw_h[ts.row_person] if P else raw_h, 'para': para_h[ts.row_person] if P else para_h}
        return rendered, people, summary
