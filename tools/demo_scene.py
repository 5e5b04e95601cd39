"""Uncropped photographs plus person boxes in, the same photographs with every predicted mesh drawn in place out: per image one
<name>_scene.png (people in front occlude people behind) and one <name>_people.npz (para, cam, cam_t_full, focal_full, center,
scale, vertices of every person); with --obj one <name>_person<k>.obj per person; with --obj --texture instead one textured
triple per person, <name>_<k>.obj + <name>_<k>.mtl + <name>_<k>_texture.png: the person's crop unwrapped to the 24 DensePose charts
through the crop camera (texture.TextureAtlas, texture.write_textured_obj).  The scene picture is the same either way.

  python tools/demo_scene.py --img_dir DIR --out_dir DIR [--boxes FILE.json] [--keypoints_dir DIR] [--checkpoint FILE] [--cfg YAML]
                             [--engine] [--batch N] [--obj [--texture [--texture_size T]]] [--fit | --fit_iuv [--fit_iters N]]

Boxes: --boxes maps an image's file name to a list of [x, y, w, h]; --keypoints_dir holds <name>_keypoints.json in OpenPose's layout
(one person per people[] entry, pose_keypoints_2d = x, y, confidence, ...); with neither, the whole image is one box.  There is no
person detector here.  --fit (needs --keypoints_dir; refused with --boxes, there is no rule here for matching boxes to people) refines
every person's predicted row against the person's BODY_25 keypoints before it is drawn (kp_fit.KeypointFitter, DESIGN.md "fit rule";
--fit_iters N iterations, 30 % of them on camera and global orientation alone); the _people.npz then also holds para_init, fit_loss
(initial and final energy) and fit_iter.  --fit_iuv refines every person on the network's own decoded IUV image instead
(dense_fit.DenseFitter, DESIGN.md "the dense fit rule"): it needs no keypoints, and with --keypoints_dir (again not with --boxes) both
terms are fitted together; the _people.npz gains the same three arrays.  Images: .npy arrays always (uint8 [H,W,3]); .jpg / .png if PIL is installed.  Without --checkpoint the model
has seeded random weights and the synthetic SMPL / DensePose tables, so the tool runs on a clean checkout.  The PNG files are written
by train_vis.write_png.  Last line: one JSON object with the milliseconds per frame of the three device stages (crop: ops.batch_crop;
infer: the network; render: SMPL forward, shading and ops.scene_render) on the last group of frames, HIP events, the median and
p10..p90 of 20 repetitions after 3 warm-up rounds."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from danet_densepose2smpl_amd.train_vis import write_png       # noqa: E402

GROUP = 8           # frames per SceneDemo call


def load_frame(path):
    """-> uint8 [H,W,3]."""
    if path.lower().endswith('.npy'):
        a = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise SystemExit('%s: reading .jpg / .png needs PIL, which is not installed; pass .npy arrays' % path)
        a = np.asarray(Image.open(path).convert('RGB'))
    if a.ndim == 3 and a.shape[0] == 3 and a.shape[2] != 3:
        a = np.transpose(a, (1, 2, 0))
    if a.ndim != 3 or a.shape[2] != 3:
        raise SystemExit('%s: image of shape %s, expected [H,W,3]' % (path, a.shape))
    if a.dtype != np.uint8:
        a = np.rint(np.clip(a.astype(np.float32), 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.ascontiguousarray(a)


def boxes_of(name, frame, box_table, keypoints_dir):
    from danet_densepose2smpl_amd import scene
    stem = os.path.splitext(name)[0]
    if box_table is not None:
        return [scene.boxes_from_xywh(b) for b in box_table.get(name, box_table.get(stem, []))]
    if keypoints_dir is not None:
        path = os.path.join(keypoints_dir, stem + '_keypoints.json')
        if not os.path.exists(path):
            return []
        out = []
        for person in json.load(open(path)).get('people', []):
            kps = np.asarray(person['pose_keypoints_2d'], np.float64).reshape(-1, 3)
            if (kps[:, 2] > 0.2).any():
                out.append(scene.boxes_from_keypoints(kps))
        return out
    return [scene.whole_image_box(frame.shape)]


def keypoints_of(name, keypoints_dir):
    """The BODY_25 arrays [25,3] of the people boxes_of makes boxes for, in the same order."""
    path = os.path.join(keypoints_dir, os.path.splitext(name)[0] + '_keypoints.json')
    if not os.path.exists(path):
        return []
    kps = [np.asarray(person['pose_keypoints_2d'], np.float64).reshape(-1, 3) for person in json.load(open(path)).get('people', [])]
    for k in kps:
        if k.shape != (25, 3):
            raise SystemExit('%s: --fit needs BODY_25 keypoints (25 rows), got %d' % (path, k.shape[0]))
    return [k for k in kps if (k[:, 2] > 0.2).any()]


def _stats(ts, n):
    ts = np.asarray(ts) / n
    return {'ms_per_frame': round(float(np.median(ts)), 4), 'p10': round(float(np.percentile(ts, 10)), 4), 'p90': round(float(np.percentile(ts, 90)), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description='DaNet scene demo: meshes drawn into uncropped photographs')
    ap.add_argument('--cfg', dest='cfg_file', default=None, help='YAML config (default: the built-in defaults)')
    ap.add_argument('--checkpoint', default=None, help='checkpoint in the reference\'s layout (default: seeded random weights)')
    ap.add_argument('--img_dir', required=True)
    ap.add_argument('--out_dir', default='./output')
    ap.add_argument('--boxes', default=None, help='JSON: image name -> list of [x, y, w, h]')
    ap.add_argument('--keypoints_dir', default=None, help='folder of <name>_keypoints.json (OpenPose)')
    ap.add_argument('--engine', action='store_true', help='run the BatchNorm-folded InferenceEngine instead of infer_net')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--obj', action='store_true', help='also write one .obj per person')
    ap.add_argument('--texture', action='store_true', help='with --obj: textured .obj + .mtl + _texture.png per person')
    ap.add_argument('--texture_size', type=int, default=64, help='texels per side of a chart')
    ap.add_argument('--reps', type=int, default=20, help='timed repetitions of the three stages (0: no timing)')
    ap.add_argument('--fit', action='store_true', help='refine every person against the keypoints of --keypoints_dir before drawing')
    ap.add_argument('--fit_iuv', action='store_true', help='refine every person on the predicted IUV image before drawing (and on the '
                    'keypoints of --keypoints_dir, if given)')
    ap.add_argument('--fit_iters', type=int, default=100, help='with --fit / --fit_iuv: iterations of the fit')
    a = ap.parse_args(argv)
    if a.fit and a.fit_iuv:
        raise SystemExit('--fit and --fit_iuv: one of the two (--fit_iuv --keypoints_dir DIR fits both terms)')
    if a.fit_iuv and a.keypoints_dir and a.boxes:
        raise SystemExit('--fit_iuv with --keypoints_dir cannot be combined with --boxes: there is no rule here for matching boxes to the '
                         'people of the keypoint files')
    if a.fit_iuv and a.fit_iters < 1:
        raise SystemExit('--fit_iters %d' % a.fit_iters)
    if a.fit and a.boxes:
        raise SystemExit('--fit cannot be combined with --boxes: there is no rule here for matching boxes to the people of the keypoint files')
    if a.fit and not a.keypoints_dir:
        raise SystemExit('--fit needs --keypoints_dir')
    if a.fit and a.fit_iters < 1:
        raise SystemExit('--fit_iters %d' % a.fit_iters)

    import torch
    from danet_densepose2smpl_amd import checkpoint, constants, scene, texture
    from danet_densepose2smpl_amd.config import cfg_from_file
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    if not torch.cuda.is_available():
        raise SystemExit('tools/demo_scene.py needs a GPU (there is no CPU path)')
    if a.texture and not a.obj:
        raise SystemExit('--texture needs --obj')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    names = sorted(n for n in os.listdir(a.img_dir) if n.lower().endswith(('.npy', '.jpg', '.jpeg', '.png')) and not n.endswith(('_scene.png', '_texture.png')))
    if not names:
        raise SystemExit('no .npy / .jpg / .png images in %s' % a.img_dir)
    box_table = json.load(open(a.boxes)) if a.boxes else None
    os.makedirs(a.out_dir, exist_ok=True)

    torch.manual_seed(0)
    model = DaNet(default_options(a.batch), None, pretrained=False)
    if a.checkpoint:
        checkpoint.load_pretrained(model, a.checkpoint)
    model = model.cuda().eval()
    smpl = model.iuv2smpl.smpl
    engine = model.inference_engine(a.batch) if a.engine else None
    demo = scene.SceneDemo(engine if engine is not None else model, smpl, a.batch)
    if a.fit:
        from danet_densepose2smpl_amd.kp_fit import KeypointFitter
        n0 = (3 * a.fit_iters) // 10
        demo.fitter = KeypointFitter(smpl, stages=((n0, 'cam+orient'), (a.fit_iters - n0, 'all')), focal=demo.focal, res=demo.res)
    if a.fit_iuv:
        from danet_densepose2smpl_amd.dense_fit import DenseFitter
        n0 = (3 * a.fit_iters) // 10
        demo.fitter = DenseFitter(smpl, stages=((n0, 'cam+orient'), (a.fit_iters - n0, 'all')), focal=demo.focal, res=demo.res)
    with_kp = a.fit or (a.fit_iuv and a.keypoints_dir is not None)
    tex = texture.TextureAtlas(size=a.texture_size, focal_length=demo.focal) if a.texture else None

    last, people_total = None, 0
    for i in range(0, len(names), GROUP):
        group = names[i:i + GROUP]
        frames = [load_frame(os.path.join(a.img_dir, n)) for n in group]
        boxes = [boxes_of(n, f, box_table, a.keypoints_dir) for n, f in zip(group, frames)]
        rendered, people = demo(frames, boxes, [keypoints_of(n, a.keypoints_dir) for n in group] if with_kp else None)
        sheets = None
        if tex is not None and any(boxes):                          # every person's crop, de-normalised, through the crop camera
            mean, std = (torch.tensor(c, device=demo.device).view(1, 3, 1, 1) for c in (constants.IMG_NORM_MEAN, constants.IMG_NORM_STD))
            crops = (demo.crops(demo.prepare(frames, boxes)) * std + mean).clamp(0.0, 1.0)
            dev = lambda key: torch.from_numpy(np.concatenate([p[key] for p in people]).astype(np.float32)).to(demo.device)   # noqa: E731
            atlas = tex.unwrap(crops, dev('vertices'), dev('cam'))
            sheets = np.rint(tex.sheet(atlas).permute(0, 2, 3, 1).clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)
        person = 0
        for n, img, ppl in zip(group, rendered, people):
            stem = os.path.splitext(n)[0]
            write_png(os.path.join(a.out_dir, stem + '_scene.png'), img)
            np.savez(os.path.join(a.out_dir, stem + '_people.npz'), **ppl)
            people_total += ppl['para'].shape[0]
            if a.obj:
                for k in range(ppl['vertices'].shape[0]):
                    if tex is None:
                        scene.write_obj(os.path.join(a.out_dir, '%s_person%d.obj' % (stem, k)), ppl['vertices'][k], smpl.faces)
                    else:
                        write_png(os.path.join(a.out_dir, '%s_%d_texture.png' % (stem, k)), sheets[person + k])
                        texture.write_textured_obj(os.path.join(a.out_dir, '%s_%d.obj' % (stem, k)), ppl['vertices'][k], tex.tables,
                                                   '%s_%d_texture.png' % (stem, k))
            person += ppl['vertices'].shape[0]
        if any(boxes):
            last = (frames, boxes)
    print('Scene demo results (%d frames, %d people) have been saved in %s.' % (len(names), people_total, a.out_dir))

    if a.reps > 0 and last is not None:
        frames, boxes = last
        plan = demo.prepare(frames, boxes)
        crops = demo.crops(plan)
        para = demo.infer(plan, crops)
        stages = {'crop': lambda: demo.crops(plan), 'infer': lambda: demo.infer(plan, crops), 'render': lambda: demo.render(para, plan)}
        for _ in range(3):
            for f in stages.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in stages}
        for _ in range(a.reps):
            for k, f in stages.items():                            # alternately: drifts hit all stages alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        res = {'tool': 'demo_scene', 'frames': len(frames), 'shapes': [list(f.shape[:2]) for f in frames], 'people': plan['P'], 'batch': a.batch,
               'engine': bool(a.engine), 'res': demo.res, 'vertices': int(smpl.faces.max()) + 1, 'reps': a.reps}
        res.update({k: _stats(v, len(frames)) for k, v in times.items()})
        print(json.dumps(res), flush=True)
    if engine is not None:
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
