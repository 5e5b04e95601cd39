"""The frames of a clip plus person boxes per frame in, the frames with every person's mesh drawn in place out -- the people followed
across frames, their boxes and SMPL rows smoothed along each track, and a person whose box is missing in a frame filled in
(video.VideoDemo, DESIGN.md 4b'-track "the track rule").  Writes <name>_scene.png per frame and ONE tracks.npz: the TrackSet arrays
(track_start, frame, det, conf, person_row, row_person), para_raw and para [N,229] (the network's rows and the final ones, track-major),
boxes_raw and boxes [N,3] (cx, cy, log scale before and after the box smoother), accel_raw and accel [K] (the mean acceleration of
the SMPL joints per track before and after).

  python tools/demo_video.py --frames_dir DIR --out_dir DIR --boxes FILE.json [--keypoints_dir DIR] [--fit | --fit_iuv] [--rounds R]
                             [--no_smooth] [--engine] [--batch N] [--checkpoint FILE] [--cfg YAML] [--fit_iters N]
                             [--stream [--lag L] [--box_lag L] [--slots S] [--reid [--max_absence F] [--id_texture_size T] [--gallery G]]]
                             [--link [--max_absence F] [--id_texture_size T]]

With --link (DESIGN.md 4b'-link "the identity rule") the tracks of one person are linked into an identity by body shape and fused
texture, every identity gets one shape, tracks.npz gains identity [K], links [L,2] and link_cost [L], and the JSON line the two counts
and the stage's milliseconds per frame; it needs finished tracks, so --stream --link is refused.  With --stream --reid (DESIGN.md
4b'-reid "the causal identity rule") a track's identity is decided at its first drawn frame against the finished tracks of the last
--max_absence frames, of which at most --gallery wait, and never revised; tracks.npz gains the same three arrays and the JSON line
`reid`, the two counts and the stage's milliseconds per frame.  --reid without --stream is refused: a whole clip has --link.

Frames are taken in name order; the input conventions are those of tools/demo_scene.py: .npy arrays always (uint8 [H,W,3]), .jpg / .png
if PIL is installed; --boxes maps a frame's file name to a list of [x, y, w, h] or [x, y, w, h, confidence]; --keypoints_dir holds
<name>_keypoints.json in OpenPose's layout, and with it the boxes come from the keypoints (so --fit, which needs it, is refused with
--boxes, as in the scene tool: there is no rule for matching boxes to the people of the keypoint files).  The whole clip is one call: it must fit on the
device.  With --stream (video.StreamDemo, DESIGN.md 4b'-stream "the stream rule") the frames are read one at a time and never held
together: every frame is drawn box_lag + lag frames after it was read, from the offline rule on what its tracks have seen by then, and
its <name>_scene.png is written as it comes out; the JSON line adds delay_frames and max_frames_held.  There is no video decoder and no
person detector here.  Last line: one JSON object with the counts and the
milliseconds per frame of every stage (host clock around a device synchronisation, one run: the clip is processed once)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from danet_densepose2smpl_amd.train_vis import write_png       # noqa: E402
from demo_scene import boxes_of, keypoints_of, load_frame       # noqa: E402


def frame_boxes(name, frame, box_table, keypoints_dir):
    """demo_scene.boxes_of, with a fifth number of a --boxes entry as the box's confidence."""
    from danet_densepose2smpl_amd import scene
    if box_table is None:
        return boxes_of(name, frame, None, keypoints_dir)
    out = []
    for b in box_table.get(name, box_table.get(os.path.splitext(name)[0], [])):
        c, s = scene.boxes_from_xywh(b[:4])
        out.append((c, s, float(b[4])) if len(b) > 4 else (c, s))
    return out


def stream(a, demo, names, box_table, with_kp):
    """The --stream mode: a frame is loaded, pushed and forgotten; what comes out is written at once.  -> the JSON line's dict."""
    import torch
    demo.timing = True
    written = 0

    def write(done):
        for n, img, _ in done:
            write_png(os.path.join(a.out_dir, os.path.splitext(names[n])[0] + '_scene.png'), img)
        return len(done)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in names:
        frame = load_frame(os.path.join(a.frames_dir, n))
        written += write(demo.push(frame, frame_boxes(n, frame, box_table, a.keypoints_dir), keypoints_of(n, a.keypoints_dir) if with_kp else None))
    rest, summary = demo.flush()
    written += write(rest)
    torch.cuda.synchronize()
    demo.ms['total'] = (time.perf_counter() - t0) * 1e3
    extra = {'identity': demo.identity, 'links': demo.links, 'link_cost': demo.link_cost} if demo.reid else {}
    np.savez(os.path.join(a.out_dir, 'tracks.npz'), para_raw=demo.para_raw, para=demo.para, boxes_raw=demo.boxes_raw, boxes=demo.boxes,
             accel_raw=summary['accel_raw_tracks'], accel=summary['accel_tracks'], **extra, **demo.tracks.arrays())
    print('Video demo results (%d frames, %d tracks, %d rows) have been saved in %s.' % (written, summary['tracks'], summary['rows'], a.out_dir))
    res = {'tool': 'demo_video', 'stream': True, 'frames': written, 'tracks': summary['tracks'], 'rows': summary['rows'],
           'gap_rows': summary['gap_rows'], 'accel_raw': summary['accel_raw'], 'accel': summary['accel'], 'batch': a.batch,
           'engine': bool(a.engine), 'smooth': not a.no_smooth, 'fit': 'keypoints' if a.fit else ('iuv' if a.fit_iuv else None),
           'lag': demo.lag, 'box_lag': demo.box_lag, 'max_gap': demo.max_gap, 'delay_frames': demo.lag + demo.box_lag,
           'max_frames_held': demo.max_held, 'ms_per_frame': {k: round(v / max(written, 1), 4) for k, v in demo.ms.items()}}
    if demo.reid:
        res.update({'reid': True, 'identities': summary['identities'], 'links': summary['links'], 'max_absence': demo.reid_kw['max_absence'],
                    'id_texture_size': demo.id_texture_size, 'gallery': demo.gallery})
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description='DaNet video demo: tracked, smoothed meshes drawn into the frames of a clip')
    ap.add_argument('--cfg', dest='cfg_file', default=None)
    ap.add_argument('--checkpoint', default=None)
    ap.add_argument('--frames_dir', required=True)
    ap.add_argument('--out_dir', default='./output')
    ap.add_argument('--boxes', default=None, help='JSON: frame name -> list of [x, y, w, h] or [x, y, w, h, confidence]')
    ap.add_argument('--keypoints_dir', default=None)
    ap.add_argument('--fit', action='store_true', help='refine every row against the keypoints of --keypoints_dir in every round')
    ap.add_argument('--fit_iuv', action='store_true', help='refine every row on the predicted IUV image in every round')
    ap.add_argument('--fit_iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=1, help='fit-then-smooth rounds')
    ap.add_argument('--no_smooth', action='store_true')
    ap.add_argument('--engine', action='store_true')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--stream', action='store_true', help='one frame at a time: online tracks and the fixed-lag smoother')
    ap.add_argument('--lag', type=int, default=8, help='--stream: rows behind the newest at which a row is drawn')
    ap.add_argument('--box_lag', type=int, default=8, help='--stream: the same for the boxes; tracks bridge gaps of up to min(5, box_lag) frames')
    ap.add_argument('--slots', type=int, default=32, help='--stream: tracks alive at once')
    ap.add_argument('--link', action='store_true', help='link the tracks of one person into an identity by shape and fused texture')
    ap.add_argument('--reid', action='store_true', help='--stream: decide every track\'s identity at its first drawn frame, causally')
    ap.add_argument('--max_absence', type=int, default=None, help='--link / --reid: frames a person may be away and keep their identity')
    ap.add_argument('--id_texture_size', type=int, default=None, help='--link / --reid: texels per side of a chart of the skin descriptor')
    ap.add_argument('--gallery', type=int, default=None, help='--reid: finished tracks that may wait for a successor at once')
    a = ap.parse_args(argv)
    if a.reid and not a.stream:
        raise SystemExit('--reid belongs to --stream: it decides identities while the clip is still coming in; a whole clip has --link')
    if a.gallery is not None and not a.reid:
        raise SystemExit('--gallery belongs to --reid')
    if a.stream and a.link:
        from danet_densepose2smpl_amd.video import NO_STREAM_LINK
        raise SystemExit('--stream --link: ' + NO_STREAM_LINK)
    if not (a.link or a.reid) and (a.max_absence is not None or a.id_texture_size is not None):
        raise SystemExit('--max_absence and --id_texture_size belong to --link or --reid')
    if a.stream and a.rounds != 1:
        raise SystemExit('--stream has no --rounds: the fit / smooth alternation needs whole tracks')
    if a.fit and a.fit_iuv:
        raise SystemExit('--fit and --fit_iuv: one of the two (--fit_iuv --keypoints_dir DIR fits both terms)')
    if (a.fit or (a.fit_iuv and a.keypoints_dir)) and a.boxes:
        raise SystemExit('keypoints cannot be combined with --boxes: there is no rule here for matching boxes to the people of the keypoint files')
    if a.fit and not a.keypoints_dir:
        raise SystemExit('--fit needs --keypoints_dir')
    if not a.boxes and not a.keypoints_dir:
        raise SystemExit('--boxes or --keypoints_dir: a clip needs person boxes per frame')
    if a.fit_iters < 1 or a.rounds < 1:
        raise SystemExit('--fit_iters %d --rounds %d' % (a.fit_iters, a.rounds))

    import torch
    from danet_densepose2smpl_amd import checkpoint, scene, video
    from danet_densepose2smpl_amd.config import cfg_from_file
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    if not torch.cuda.is_available():
        raise SystemExit('tools/demo_video.py needs a GPU (there is no CPU path)')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    names = sorted(n for n in os.listdir(a.frames_dir) if n.lower().endswith(('.npy', '.jpg', '.jpeg', '.png')) and not n.endswith('_scene.png'))
    if not names:
        raise SystemExit('no .npy / .jpg / .png frames in %s' % a.frames_dir)
    box_table = json.load(open(a.boxes)) if a.boxes else None
    os.makedirs(a.out_dir, exist_ok=True)

    torch.manual_seed(0)
    model = DaNet(default_options(a.batch), None, pretrained=False)
    if a.checkpoint:
        checkpoint.load_pretrained(model, a.checkpoint)
    model = model.cuda().eval()
    smpl = model.iuv2smpl.smpl
    engine = model.inference_engine(a.batch) if a.engine else None
    if a.stream:
        reid_kw = {}
        if a.reid:
            reid_kw = {'reid': True, 'max_absence': a.max_absence}
            reid_kw.update({k: v for k, v in (('id_texture_size', a.id_texture_size), ('gallery', a.gallery)) if v is not None})
        try:
            demo = video.StreamDemo(engine if engine is not None else model, smpl, a.batch, smooth=not a.no_smooth, lag=a.lag, box_lag=a.box_lag,
                                    slots=a.slots, max_gap=min(5, a.box_lag) if a.box_lag >= 1 else 5, **reid_kw)
        except ValueError as e:
            if not a.reid:
                raise
            raise SystemExit('--reid: %s' % e)
    else:
        link_kw = {}
        if a.link:
            from danet_densepose2smpl_amd import tracks as trk
            link_kw = {'link': True, 'max_absence': a.max_absence, 'id_texture_size': trk.ID_TEXTURE_SIZE if a.id_texture_size is None else a.id_texture_size}
        try:
            demo = video.VideoDemo(engine if engine is not None else model, smpl, a.batch, smooth=not a.no_smooth, rounds=a.rounds, **link_kw)
        except ValueError as e:
            if not a.link:
                raise
            raise SystemExit('--link: %s' % e)
    n0 = (3 * a.fit_iters) // 10
    stages = ((n0, 'cam+orient'), (a.fit_iters - n0, 'all'))
    if a.fit:
        from danet_densepose2smpl_amd.kp_fit import KeypointFitter
        demo.scene.fitter = KeypointFitter(smpl, stages=stages, focal=demo.scene.focal, res=demo.scene.res)
    if a.fit_iuv:
        from danet_densepose2smpl_amd.dense_fit import DenseFitter
        demo.scene.fitter = DenseFitter(smpl, stages=stages, focal=demo.scene.focal, res=demo.scene.res)
    with_kp = a.fit or (a.fit_iuv and a.keypoints_dir is not None)
    if a.stream:
        res = stream(a, demo, names, box_table, with_kp)
        print(json.dumps(res), flush=True)
        if engine is not None:
            engine.close()
        return 0

    frames = [load_frame(os.path.join(a.frames_dir, n)) for n in names]
    boxes = [frame_boxes(n, f, box_table, a.keypoints_dir) for n, f in zip(names, frames)]
    keypoints = [keypoints_of(n, a.keypoints_dir) for n in names] if with_kp else None

    # the stages once by hand for the clock; the results come from the one call below
    ms = {}
    timed = functools.partial(scene.timed, ms)
    from danet_densepose2smpl_amd import tracks as tr
    ts = timed('associate', lambda: tr.associate(boxes, demo.max_gap, demo.min_iou))
    _, _, _, per_frame = timed('boxes', lambda: demo.track_boxes(boxes))
    plan = timed('prepare', lambda: demo.scene.prepare(frames, per_frame))
    if plan['P']:
        para = timed('infer', lambda: demo.scene.infer(plan))
        rows = para[torch.from_numpy(ts.row_person).to(para.device)]
        smoothed, _ = timed('smooth', lambda: tr.smooth_para(rows, ts, demo.lam, demo.shared_shape))
        if a.link:
            def link_stage():
                res = demo.link_tracks(smoothed, ts, plan)
                return tr.share_shape(smoothed, ts, res['identity']) if demo.shared_shape else res
            timed('link', link_stage)
        timed('render', lambda: demo.scene.render(para, plan))
    rendered, people, summary = timed('total', lambda: demo(frames, boxes, keypoints))
    for n, img in zip(names, rendered):
        write_png(os.path.join(a.out_dir, os.path.splitext(n)[0] + '_scene.png'), img)
    last = demo.last
    extra = {k: last[k] for k in ('identity', 'links', 'link_cost')} if a.link else {}
    np.savez(os.path.join(a.out_dir, 'tracks.npz'), para_raw=last['para_raw'], para=last['para'], boxes_raw=last['boxes_raw'], boxes=last['boxes'],
             accel_raw=summary['accel_raw_tracks'], accel=summary['accel_tracks'], **extra, **last['tracks'].arrays())
    print('Video demo results (%d frames, %d tracks, %d rows) have been saved in %s.' % (len(names), summary['tracks'], summary['rows'], a.out_dir))
    res = {'tool': 'demo_video', 'frames': len(frames), 'tracks': summary['tracks'], 'rows': summary['rows'], 'gap_rows': summary['gap_rows'],
           'accel_raw': summary['accel_raw'], 'accel': summary['accel'], 'batch': a.batch, 'engine': bool(a.engine), 'smooth': not a.no_smooth,
           'rounds': a.rounds, 'fit': 'keypoints' if a.fit else ('iuv' if a.fit_iuv else None),
           'ms_per_frame': {k: round(v / len(frames), 4) for k, v in ms.items()}}
    if a.link:
        res.update({'link': True, 'identities': summary['identities'], 'links': summary['links'], 'max_absence': demo.link_kw['max_absence'],
                    'id_texture_size': demo.id_texture_size})
    print(json.dumps(res), flush=True)
    if engine is not None:
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
