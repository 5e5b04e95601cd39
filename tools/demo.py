"""A folder of images in, one <name>_result.png per image out (/root/reference/demo.py): input | decoded global IUV | the 24
decoded partial IUV maps | IUV rendering of the predicted mesh over the input | with --mesh: shaded mesh over the input |
shaded mesh turned by 90 degrees | with --texture: the mesh wearing the photograph's own colours, turned by 90 and by 180 degrees,
plus one <name>_texture.png, the 4 x 6 sheet of the 24 DensePose charts the photograph was unwrapped to (texture.TextureAtlas).
With --fuse all images of the folder are views of ONE person: one atlas, fused_texture.png, drawn in every strip.

  python tools/demo.py --img_dir DIR --out_dir DIR [--checkpoint FILE] [--cfg YAML] [--mesh] [--engine] [--batch N]
                       [--texture [--fuse] [--texture_size T]] [--fit_iuv [--fit_iters N]]

--fit_iuv refines every predicted row on the network's own decoded global IUV image before anything is drawn (dense_fit.DenseFitter,
DESIGN.md "the dense fit rule", the training camera): the mesh panels, the IUV rendering and the textures come from the fitted row;
the decoded IUV panels stay the network's.

Images: .npy arrays always ([S,S,3] or [3,S,S], uint8 or float in [0,1]); .jpg / .png if PIL is installed.  They must be square
at DANET.INIMG_SIZE (cropping is augment.py's job).  Without --checkpoint the model has seeded random weights and the synthetic
SMPL / DensePose tables, so the tool runs on a clean checkout.  The PNG files are written by train_vis.write_png (zlib + struct).
Last line: one JSON object with the milliseconds per image of the panel stage (demo.result_panels, HIP) beside the same panels
assembled from tensor ops (panels_torch below), 20 alternating repetitions, median and p10..p90; with --texture also the texel map,
the unwrap and one draw (texture_map_hip, texture_unwrap_hip, texture_draw_hip)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from danet_densepose2smpl_amd.train_vis import write_png       # noqa: E402  (the writer the training sheets share)


def to_uint8(x):
    """float [0,1] -> uint8, round half to even (numpy.rint)."""
    return np.rint(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)


def load_image(path, S):
    """-> float32 [3,S,S] in [0,1]."""
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
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] != S or a.shape[1] != S:
        raise SystemExit('%s: image of shape %s; this tool takes images already cropped to %d x %d x 3 (DANET.INIMG_SIZE; '
                         'cropping is augment.py\'s job)' % (path, a.shape, S, S))
    a = a.astype(np.float32) / 255.0 if a.dtype == np.uint8 else a.astype(np.float32)
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def panels_torch(images, planes):
    """The strip of demo.result_panels from the same decoded / rendered planes, with tensor ops (demo.py:115-177)."""
    import torch
    import torch.nn.functional as F
    B, _, S, _ = images.shape
    hm = planes['glob'].shape[-1]
    up = lambda t: F.interpolate(t, size=(S, S), mode='bilinear', align_corners=False)
    glob = up(planes['glob'])
    grid = planes['part'].view(B, 4, 6, 3, hm, hm).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 4 * hm, 6 * hm)
    riuv = up(planes['riuv'])
    over = torch.where(riuv > 0, riuv, images)
    strip = [images, glob, grid, over]
    alpha = [torch.ones(B, 1, S, t.shape[-1], device=images.device) for t in strip]
    if planes.get('mesh') is not None:
        strip += [planes['mesh'], planes['side']]
        alpha += [torch.ones(B, 1, S, S, device=images.device), planes['side_alpha'].unsqueeze(1)]
    rgba = torch.cat([torch.cat(strip, dim=3), torch.cat(alpha, dim=3)], dim=1)
    return rgba.clamp(0.0, 1.0).permute(0, 2, 3, 1).contiguous()


def _stats(ts, B):
    ts = np.asarray(ts) / B
    return {'ms_per_img': round(float(np.median(ts)), 4), 'p10': round(float(np.percentile(ts, 10)), 4), 'p90': round(float(np.percentile(ts, 90)), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description='DaNet demo: result panels for a folder of images')
    ap.add_argument('--cfg', dest='cfg_file', default=None, help='YAML config (default: the built-in defaults)')
    ap.add_argument('--checkpoint', default=None, help='checkpoint in the reference\'s layout (default: seeded random weights)')
    ap.add_argument('--img_dir', required=True)
    ap.add_argument('--out_dir', default='./output')
    ap.add_argument('--mesh', action='store_true', help='add the two shaded-mesh panels (the reference\'s --use_opendr)')
    ap.add_argument('--texture', action='store_true', help='add the two textured-mesh panels and write the texture sheets')
    ap.add_argument('--fuse', action='store_true', help='with --texture: all images are views of one person, one fused atlas')
    ap.add_argument('--texture_size', type=int, default=64, help='texels per side of a chart')
    ap.add_argument('--engine', action='store_true', help='run the BatchNorm-folded InferenceEngine instead of infer_net')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--reps', type=int, default=20, help='timed repetitions of the panel stage (0: no timing)')
    ap.add_argument('--fit_iuv', action='store_true', help='refine every row on the predicted IUV image before drawing')
    ap.add_argument('--fit_iters', type=int, default=100, help='with --fit_iuv: iterations of the fit')
    a = ap.parse_args(argv)
    if a.fit_iuv and a.fit_iters < 1:
        raise SystemExit('--fit_iters %d' % a.fit_iters)

    import torch
    from danet_densepose2smpl_amd import checkpoint, demo
    from danet_densepose2smpl_amd.config import cfg, cfg_from_file
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    from danet_densepose2smpl_amd.texture import TextureAtlas
    from danet_densepose2smpl_amd.trainer import default_options
    if not torch.cuda.is_available():
        raise SystemExit('tools/demo.py needs a GPU (there is no CPU path)')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    S = cfg.DANET.INIMG_SIZE
    names = sorted(n for n in os.listdir(a.img_dir) if n.lower().endswith(('.npy', '.jpg', '.jpeg', '.png')) and not n.endswith(('_result.png', '_texture.png')))
    if not names:
        raise SystemExit('no .npy / .jpg / .png images in %s' % a.img_dir)
    imgs = [load_image(os.path.join(a.img_dir, n), S) for n in names]
    os.makedirs(a.out_dir, exist_ok=True)

    torch.manual_seed(0)
    model = DaNet(default_options(a.batch), None, pretrained=False)
    if a.checkpoint:
        checkpoint.load_pretrained(model, a.checkpoint)
    model = model.cuda().eval()
    smpl = model.iuv2smpl.smpl
    mesh_renderer = MeshRenderer(smpl.faces, img_res=S) if a.mesh else None
    engine = model.inference_engine(a.batch, mesh=True) if a.engine else None
    if a.fuse and not a.texture:
        raise SystemExit('--fuse needs --texture')
    tex = TextureAtlas(size=a.texture_size) if a.texture else None
    fitter = None
    if a.fit_iuv:
        from danet_densepose2smpl_amd import iuvmap
        from danet_densepose2smpl_amd.dense_fit import DenseFitter
        n0 = (3 * a.fit_iters) // 10
        fitter = DenseFitter(smpl, stages=((n0, 'cam+orient'), (a.fit_iters - n0, 'all')), res=S)
    sheet_png = lambda atlas: to_uint8(tex.sheet(atlas).permute(0, 2, 3, 1).cpu().numpy())           # noqa: E731

    def batches():
        for i in range(0, len(imgs), a.batch):
            chunk = imgs[i:i + a.batch]
            n = len(chunk)
            chunk = chunk + [chunk[-1]] * (a.batch - n)            # a short last batch is padded, its extra strips dropped
            image = torch.from_numpy(np.stack(chunk)).cuda()
            out = engine(image) if engine is not None else model.infer_net(image)
            if fitter is not None:                                 # the fitted row replaces the network's; its vertices are made anew
                vis = out['visualization']['iuv_pred']
                iuv = iuvmap.iuv_map2img(vis[0], vis[1], vis[2], vis[3] if len(vis) > 3 else None)
                out = dict(out, para=fitter.fit(out['para'].detach().float(), iuv))
                out.pop('vertices', None)
            yield i, n, image, out

    texture = tex
    if a.fuse:                                                     # a first pass: every image is a view of the one person
        views = [(image[:n], ) + tuple(t[:n].clone() for t in demo.mesh_of(out, smpl)) for _, n, image, out in batches()]
        fused = tex.unwrap(*(torch.cat(t, 0) for t in zip(*views)), view_offsets=[0, len(imgs)])
        write_png(os.path.join(a.out_dir, 'fused_texture.png'), sheet_png(fused)[0])
        texture = (tex, fused)
    last = None
    for i, n, image, out in batches():
        strip, planes = demo.result_panels(out, image, smpl, model.iuv_renderer, mesh_renderer, return_planes=True, texture=texture)
        arr = to_uint8(strip.cpu().numpy())
        sheets = sheet_png(planes['atlas']) if a.texture and not a.fuse else None
        for k in range(n):
            stem = os.path.join(a.out_dir, os.path.splitext(names[i + k])[0])
            write_png(stem + '_result.png', arr[k])
            if sheets is not None:
                write_png(stem + '_texture.png', sheets[k])
        last = (out, image)
    print('Demo results have been saved in {}.'.format(a.out_dir))

    if a.reps > 0:
        out, image = last
        hip = lambda: demo.result_panels(out, image, smpl, model.iuv_renderer, mesh_renderer)
        _, planes = demo.result_panels(out, image, smpl, model.iuv_renderer, mesh_renderer, return_planes=True)
        variants = {'panels_hip': hip, 'compose_hip': lambda: demo.ops.demo_compose(image, planes['glob'], planes['part'], planes['riuv'],
                                                                                  planes['mesh'], planes['side'], planes['side_alpha']),
                    'compose_tensor_ops': lambda: panels_torch(image, planes)}
        if tex is not None:
            import math
            verts, cam = demo.mesh_of(out, smpl)
            atlas = tex.unwrap(image, verts, cam)
            d = tex._dev(image.device)
            variants.update({'texture_map_hip': lambda: demo.ops.texture_map(d['uv'], d['faces'], d['part_off'], d['part_faces'], tex.size),
                             'texture_unwrap_hip': lambda: tex.unwrap(image, verts, cam),
                             'texture_draw_hip': lambda: tex.render(verts, cam, atlas, None, rot_y=math.radians(90), img_res=S)})
        for _ in range(3):
            for f in variants.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, f in variants.items():                          # alternately: drifts hit all variants alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        res = {'tool': 'demo', 'B': a.batch, 'S': S, 'mesh': bool(a.mesh), 'reps': a.reps}
        if tex is not None:
            res['texture_size'] = tex.size
        res.update({k: _stats(v, a.batch) for k, v in times.items()})
        print(json.dumps(res), flush=True)
    if engine is not None:
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
