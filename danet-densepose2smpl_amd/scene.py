"""Scene demo: uncropped photographs plus person boxes in, the same photographs with every predicted mesh drawn in place out.

    demo = SceneDemo(model_or_engine, smpl, batch)
    rendered, people = demo(frames, boxes)

`frames` is a list of uint8 [H,W,3] arrays of any sizes, `boxes` a list per frame of (center [2], scale) in the box convention of
every dataset here (scale = box size / 200; boxes_from_xywh / boxes_from_keypoints make them, whole_image_box is the frame
itself).  Per person the frame is cropped on the device (datasets.crop_params + ops.batch_crop, rot = 0, no flip, no noise), the
network runs in chunks of `batch`, and the stage from `para` to the rendered bytes -- SMPL forward, ops.mesh_shade_vertices,
ops.scene_render -- is a straight chain of launches that captures under torch.cuda.graph (SceneDemo.render).  The people of a
frame share one depth buffer: whoever is in front occludes (DESIGN.md "scene rule", and the camera formulas beside it).

There is no CPU path: the ops raise on CPU tensors like every other op of the package."""
import numpy as np
import torch

from . import constants, datasets, iuvmap, ops
from ._lib import GPU_ONLY
from .dense_fit import DenseFitter
from .renderer import ALBEDO, MeshRenderer
from .smpl import from_para


# ---- boxes -----------------------------------------------------------------------------------------------------------------------
def boxes_from_xywh(boxes, rescale=1.2):
    """[x, y, w, h] (or [n,4]) -> (center [2] or [n,2], scale): center = (x + w / 2, y + h / 2), scale = rescale * max(w, h) / 200."""
    b = np.asarray(boxes, np.float64)
    if b.shape[-1] != 4:
        raise ValueError('boxes_from_xywh: [x, y, w, h] expected, got shape %s' % (b.shape,))
    center = b[..., :2] + b[..., 2:] / 2.0
    scale = rescale * np.maximum(b[..., 2], b[..., 3]) / 200.0
    return center, (float(scale) if scale.ndim == 0 else scale)


def boxes_from_keypoints(kps, thresh=0.2, rescale=1.2):
    """kps [K,3] (x, y, confidence) -> (center [2], scale) of the tight box of the keypoints with confidence > thresh."""
    k = np.asarray(kps, np.float64).reshape(-1, 3)
    v = k[k[:, 2] > thresh, :2]
    if v.shape[0] == 0:
        raise ValueError('boxes_from_keypoints: no keypoint with confidence > %g' % thresh)
    lo, hi = v.min(0), v.max(0)
    return (lo + hi) / 2.0, float(rescale * (hi - lo).max() / 200.0)


def whole_image_box(shape):
    """The box of a whole image of shape (rows, cols, ...): center = ((W-1)/2, (H-1)/2), scale = max(H, W) / 200."""
    H, W = int(shape[0]), int(shape[1])
    return np.array([(W - 1) / 2.0, (H - 1) / 2.0]), max(H, W) / 200.0


def box_row(box):
    """A box (center [2], scale, ..) -> the row a box smoother works on: (cx, cy, log scale), float32 [3]."""
    c = np.asarray(box[0], np.float64).reshape(2)
    return np.array((c[0], c[1], np.log(float(box[1]))), np.float32)


def row_box(row):
    """The inverse of box_row for a float32 row: (center [2] float64, scale = exp in float64)."""
    return row[:2].astype(np.float64), float(np.exp(np.float64(row[2])))


def timed(ms, key, f):
    """f() between two device synchronisations; its milliseconds on the host clock are added to ms[key]."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    ms[key] = ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
    return r


def fit_record(fitted, P):
    """fitted = (the start rows [P,229], the fit's info dict or None where P = 0) -> (init [P,229], loss [P,2] f32: E at the start
    and at the best iterate, it [P] int32: the best iterate), on the host."""
    init = fitted[0].cpu().numpy()
    if not P:
        return init, np.zeros((0, 2), np.float32), np.zeros(0, np.int32)
    hist, it = fitted[1]['history'].cpu().numpy(), fitted[1]['best_iter'].cpu().numpy()
    return init, np.stack([hist[:, 0], hist[np.arange(P), it]], 1), it


def fit_columns(fitted, P):
    """The people-dict columns of a fit ({} without one): 'para_init', 'fit_loss', 'fit_iter'."""
    return {} if fitted is None else dict(zip(('para_init', 'fit_loss', 'fit_iter'), fit_record(fitted, P)))


def split_people(people, plan):
    """One dict over all people of a plan -> one dict per frame, every column split by plan['person_frame']."""
    return [{k: v[m] for k, v in people.items()} for m in (plan['person_frame'] == n for n in range(plan['N']))]


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def person_cameras(cam, tinv, frame_shapes, person_frame, res, focal=5000., focal_full=None):
    """The per-person arguments of ops.scene_render, in float64 on the host (the scene cameras).

    cam [P,3] = (s, tx, ty) as the network predicts it for the res x res crop; tinv [P,2,3] (or [P,3,3]) the inverse crop transform
    at rot = 0 (datasets.crop_transforms), crop pixel indices -> frame pixel indices; frame_shapes [N,2] (rows, cols); person_frame
    [P].  -> dict of float64 arrays: 'proj' [P,6], 'cam_t' [P,3], 'dscale' [P], 'cam_t_full' [P,3], and 'focal_full' [P].

    With fx = focal res / 224 and tz = 2 focal / (res s + 1e-9) a point projects to the crop index (fx x_n + c, fx y_n + c), c =
    res / 2 - 0.5; `proj` is tinv applied to that.  The person's own focal in frame pixels is F_p = fx tinv[0,0] (= fx 200 scale /
    res), the common one F0 = focal_full (default: the diagonal of the person's frame), dscale = F0 / F_p, and cam_t_full is the
    translation that puts the person, seen through ONE camera of focal F0 centred on the frame, where `proj` puts it."""
    cam = np.asarray(cam, np.float64).reshape(-1, 3)
    P = cam.shape[0]
    tinv = np.asarray(tinv, np.float64).reshape(P, -1, 3)[:, :2]
    shapes = np.asarray(frame_shapes, np.float64).reshape(-1, 2)
    pf = np.asarray(person_frame, np.int64).reshape(P)
    res = float(res)
    fx = focal * res / 224.0
    c = res / 2.0 - 0.5
    tz = 2.0 * focal / (res * cam[:, 0] + 1e-9)
    proj = np.empty((P, 6), np.float64)
    for r in range(2):
        proj[:, 3 * r + 0] = tinv[:, r, 0] * fx
        proj[:, 3 * r + 1] = tinv[:, r, 1] * fx
        proj[:, 3 * r + 2] = tinv[:, r, 0] * c + tinv[:, r, 1] * c + tinv[:, r, 2]
    H, W = shapes[pf, 0], shapes[pf, 1]
    Fp = fx * tinv[:, 0, 0]
    F0 = np.sqrt(H * H + W * W) if focal_full is None else np.broadcast_to(np.asarray(focal_full, np.float64), (P,)).copy()
    dscale = F0 / Fp
    tzf = tz * dscale
    cam_t = np.stack([cam[:, 1], cam[:, 2], tz], 1)
    cam_t_full = np.stack([cam[:, 1] + (proj[:, 2] - (W - 1) / 2.0) * tzf / F0, cam[:, 2] + (proj[:, 5] - (H - 1) / 2.0) * tzf / F0, tzf], 1)
    return {'proj': proj, 'cam_t': cam_t, 'dscale': dscale, 'cam_t_full': cam_t_full, 'focal_full': F0}


def keypoints_to_crop(kps_frame, t, res):
    """Keypoints in frame pixels -> normalised crop coordinates, the keypoint convention of the fit rule: kps_frame
    [..,K,3] (x, y, confidence), `t` [..,3,3] (or [..,2,3]) the forward crop transform of datasets.crop_transforms, frame pixel
    indices -> crop pixel indices.  With c = res / 2 - 0.5 the result is ((t (x, y, 1) - c) / (res / 2), confidence): person_cameras'
    `proj` of a point (x_n, y_n) comes back as 2 focal / 224 (x_n, y_n).  float64 on the host."""
    k = np.asarray(kps_frame, np.float64)
    t = np.asarray(t, np.float64)[..., :2, :]
    res = float(res)
    c = res / 2.0 - 0.5
    out = k.copy()
    for r in range(2):
        out[..., r] = (t[..., None, r, 0] * k[..., 0] + t[..., None, r, 1] * k[..., 1] + t[..., None, r, 2] - c) / (res / 2.0)
    return out


def write_obj(path, vertices, faces):
    """A Wavefront .obj: one `v x y z` line per vertex (9 significant digits: a float32 survives), one `f a b c` line per face
    (1-based)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    with open(path, 'w') as fh:
        for x in v:
            fh.write('v %.9g %.9g %.9g\n' % (x[0], x[1], x[2]))
        for t in f:
            fh.write('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1))


def pack_frames(frames):
    """A list of uint8 [H,W,3] arrays -> (src uint8 [n + 16], offsets int64 [N+1], shapes int32 [N,2]): batch_crop's layout with
    whole frames (16 spare bytes at the end, as datasets.crop_params leaves)."""
    N = len(frames)
    offsets, shapes = np.zeros(N + 1, np.int64), np.zeros((N, 2), np.int32)
    for n, f in enumerate(frames):
        f = np.asarray(f)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError('frame %d: a non-empty uint8 [H,W,3] array expected, got %s %s' % (n, f.dtype, f.shape))
        shapes[n] = f.shape[:2]
        offsets[n + 1] = offsets[n] + f.size
    src = np.zeros(int(offsets[-1]) + 16, np.uint8)
    for n, f in enumerate(frames):
        src[offsets[n]:offsets[n + 1]] = np.ascontiguousarray(f).reshape(-1)
    return src, offsets, shapes


def unpack_frames(buf, offsets, shapes):
    """The inverse of pack_frames for a host uint8 buffer: a list of [H,W,3] arrays (copies)."""
    return [np.array(buf[int(offsets[n]):int(offsets[n + 1])]).reshape(int(shapes[n][0]), int(shapes[n][1]), 3) for n in range(len(shapes))]


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
class SceneDemo(object):
    """SceneDemo(model_or_engine, smpl, batch): a DaNet in eval mode on the GPU (its infer_net runs) or an InferenceEngine built at
    batch size `batch`; `smpl` the SMPL layer of the model (model.iuv2smpl.smpl).

    With a dense_fit.DenseFitter as `fitter` the rows are refined on the network's own decoded IUV image (DESIGN.md "the dense fit
    rule"), with no keypoints at all or with both terms where keypoints are given; the people dicts gain the same keys.
    With `fitter` (a kp_fit.KeypointFitter over the same SMPL layer) and `keypoints` -- per frame one [49,3] (or BODY_25 [25,3]) array
    per box, frame pixels and confidences -- the network's rows are refined against the keypoints before they are drawn (DESIGN.md
    "fit rule", scene kappa = 2 focal / 224); every people dict then also holds 'para_init' [k,229], 'fit_loss' [k,2] (initial and final
    E) and 'fit_iter' [k].  Without either, every output is what it is without the fitter.

    __call__(frames, boxes) -> (rendered frames: list of uint8 [H,W,3], people: one dict per frame with 'para' [k,229], 'cam' [k,3],
    'cam_t_full' [k,3], 'focal_full' [k], 'center' [k,2], 'scale' [k] and 'vertices' [k,V,3], k the number of boxes of the frame).
    The three stages are methods of their own: prepare (host: packing, crop and camera parameters; device: uploads), infer (crops and
    the network -> para [P,229]) and render (para -> the rendered bytes; capturable for fixed shapes)."""

    def __init__(self, model_or_engine, smpl, batch, res=None, focal=constants.FOCAL_LENGTH, focal_full=None, fitter=None):
        from .config import cfg
        from .inference import InferenceEngine
        self.engine = model_or_engine if isinstance(model_or_engine, InferenceEngine) else None
        self.model = None if self.engine is not None else model_or_engine
        self.smpl, self.batch = smpl, int(batch)
        self.res = int(res if res is not None else (self.engine.img_size if self.engine is not None else cfg.DANET.INIMG_SIZE))
        self.focal, self.focal_full = float(focal), focal_full
        self.device = self.engine.device if self.engine is not None else next(self.model.parameters()).device
        if self.device.type != 'cuda':
            raise RuntimeError(GPU_ONLY % ('SceneDemo model', self.device))
        if self.batch < 1:
            raise ValueError('SceneDemo: batch %d' % self.batch)
        self.mesh = MeshRenderer(smpl.faces, focal_length=self.focal, img_res=self.res)      # its face tables and lights
        self.fitter = fitter

    @property
    def dense(self):
        """True where the fitter works on the predicted IUV image: no keypoints needed."""
        return isinstance(self.fitter, DenseFitter)

    def prepare(self, frames, boxes):
        """Everything that does not depend on the network's answer.  -> plan (a dict): the packed frames and the per-person crop and
        camera arguments on the device, and their host copies."""
        if len(frames) != len(boxes) or not frames:
            raise ValueError('SceneDemo: %d frames, %d box lists' % (len(frames), len(boxes)))
        src, offsets, shapes = pack_frames(frames)
        pf = np.array([n for n, bs in enumerate(boxes) for _ in bs], np.int32)
        P = pf.size
        center = np.array([np.asarray(b[0], np.float64).reshape(2) for bs in boxes for b in bs], np.float64).reshape(P, 2)
        scale = np.array([float(b[1]) for bs in boxes for b in bs], np.float64).reshape(P)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)            # noqa: E731
        plan = {'P': P, 'N': len(frames), 'person_frame': pf, 'offsets': offsets, 'shapes': shapes, 'center': center, 'scale': scale,
                'd_src': dev(src), 'd_offsets': dev(offsets), 'd_shapes': dev(shapes), 'd_person_frame': dev(pf)}
        if P:
            if not (np.isfinite(center).all() and np.isfinite(scale).all() and (scale > 0).all()):
                raise ValueError('SceneDemo: a box with a non-finite center or a scale that is not positive')
            zeros = np.zeros(P)
            cp = datasets.crop_params([frames[n] for n in pf], center, scale, zeros, zeros, np.ones((P, 3)), self.res)
            _, tinv = datasets.crop_transforms(center, scale, zeros, self.res)
            plan['tinv'] = tinv
            plan['crop'] = (dev(cp['src']), dev(cp['offsets']), dev(cp['geom'][0]), dev(cp['geom'][1]), dev(cp['params']))
            k = person_cameras(np.tile([1., 0., 0.], (P, 1)), tinv, shapes, pf, self.res, self.focal, self.focal_full)    # (proj and dscale do not depend on cam)
            plan['d_proj'], plan['d_dscale'] = dev(k['proj'].astype(np.float32)), dev(k['dscale'].astype(np.float32))
        return plan

    def crops(self, plan):
        """The res x res network inputs of the plan's people [P,3,res,res] f32 (ImageNet-normalised, as the training input)."""
        return ops.batch_crop(*plan['crop'], self.res)

    def infer(self, plan, crops=None, return_iuv=False):
        """-> para [P,229] f32: the network on the crops in chunks of `batch`, a short last chunk padded with its last crop.
        return_iuv: -> (para, the decoded global IUV image of every person [P,3,S,S] f32, iuvmap.iuv_map2img of the prediction)."""
        crops = self.crops(plan) if crops is None else crops
        paras, iuvs = [], []
        for i in range(0, plan['P'], self.batch):
            chunk = crops[i:i + self.batch]
            n = chunk.shape[0]
            if n < self.batch:
                chunk = torch.cat([chunk, chunk[-1:].expand(self.batch - n, -1, -1, -1)], 0)
            out = self.engine(chunk.contiguous()) if self.engine is not None else self.model.infer_net(chunk.contiguous())
            paras.append(out['para'][:n].detach().clone())                 # (the engine's buffers live until its next call)
            if return_iuv:
                vis = out['visualization']['iuv_pred']
                iuvs.append(iuvmap.iuv_map2img(vis[0], vis[1], vis[2], vis[3] if len(vis) > 3 else None)[:n].detach().clone())
        return (torch.cat(paras, 0), torch.cat(iuvs, 0)) if return_iuv else torch.cat(paras, 0)

    def crop_keypoints(self, plan, keypoints):
        """Per frame one [49,3] or [25,3] array per box (frame pixels) -> [P,49,3] f32 on the device, normalised crop coordinates."""
        from .kp_fit import openpose_to_j49
        if len(keypoints) != plan['N'] or [len(k) for k in keypoints] != np.bincount(plan['person_frame'], minlength=plan['N']).tolist():
            raise ValueError('SceneDemo: keypoints must hold one array per box of every frame')
        flat = [np.asarray(k, np.float64) for ks in keypoints for k in ks]
        flat = np.stack([openpose_to_j49(k).astype(np.float64) if k.shape == (25, 3) else k for k in flat]).reshape(plan['P'], 49, 3)
        t, _ = datasets.crop_transforms(plan['center'], plan['scale'], np.zeros(plan['P']), self.res)
        return torch.from_numpy(keypoints_to_crop(flat, t, self.res).astype(np.float32)).to(self.device)

    def fit(self, para, plan, keypoints, iuv=None):
        """para [P,229] refined against the plan's people's keypoints -> (para_fit, info), the scene camera's kappa = 2 focal / 224.
        With a DenseFitter: against `iuv` (infer's decoded IUV images), and the keypoints too where there are some (or None)."""
        if self.fitter.res != self.res or self.fitter.focal != self.focal:
            raise ValueError('SceneDemo: the fitter was built for res %g, focal %g; the demo runs at res %d, focal %g'
                             % (self.fitter.res, self.fitter.focal, self.res, self.focal))
        kappa = 2.0 * self.focal / 224.0
        if self.dense:
            kp = None if keypoints is None else self.crop_keypoints(plan, keypoints)
            return self.fitter.fit(para, iuv, keypoints=kp, return_history=True, kappa=kappa)
        return self.fitter.fit(para, self.crop_keypoints(plan, keypoints), return_history=True, kappa=kappa)

    def vertices(self, para):
        return from_para(self.smpl, para).vertices.detach()

    def render(self, para, plan, return_aux=False, vertices=None):
        """para [P,229] -> the rendered frames as one packed uint8 tensor in the plan's layout (with return_aux: also ids and depth
        per frame pixel).  SMPL forward, mesh_shade_vertices, three element-wise ops for cam_t = (tx, ty, 2 focal / (res s + 1e-9)) and
        scene_render: no synchronisation and no allocation by data, so for fixed shapes the call captures under torch.cuda.graph."""
        P = plan['P']
        host = (plan['person_frame'], plan['offsets'], plan['shapes'])
        if P == 0:
            z = torch.zeros(0, 1, 3, device=self.device)
            f2 = torch.zeros(1, 3, dtype=torch.int32, device=self.device)
            return ops.scene_render(z, z, f2, z.view(0, 3), torch.zeros(0, 6, device=self.device), z.view(0)[:0], plan['d_person_frame'],
                                    plan['d_src'], plan['d_offsets'], plan['d_shapes'], return_aux=return_aux, host=host)
        verts = self.vertices(para) if vertices is None else vertices
        V = verts.shape[1]
        t = self.mesh.tables(self.device, V)
        ws, _ = ops.mesh_shade_vertices(verts, t.faces, t.csr_off, t.csr_face, self.mesh.lights, 0., ALBEDO)
        rverts, vcol = ops.mesh_shade_views(ws, P, V)
        cam = para[:, 0:3].detach().float()
        cam_t = torch.stack([cam[:, 1], cam[:, 2], (2.0 * self.focal) / (self.res * cam[:, 0] + 1e-9)], 1)
        return ops.scene_render(rverts, vcol, t.faces2, cam_t, plan['d_proj'], plan['d_dscale'], plan['d_person_frame'], plan['d_src'],
                                plan['d_offsets'], plan['d_shapes'], return_aux=return_aux, host=host)

    def infer_stage(self, plan):
        """-> (para [P,229], the decoded IUV images where the fitter is a dense one, else None); nothing runs for P = 0."""
        if plan['P'] and self.dense:
            return self.infer(plan, return_iuv=True)
        return (self.infer(plan) if plan['P'] else torch.zeros(0, 229, device=self.device)), None

    def fit_stage(self, para, plan, keypoints, iuv):
        """-> (fitted, para): where there is a fitter and something to fit to, fitted = (the start rows, the fit's info; None for
        P = 0) and para the fitted rows; else (None, para as it came)."""
        if self.fitter is None or not (self.dense or keypoints is not None):
            return None, para
        if not plan['P']:
            return (para, None), para
        para_fit, info = self.fit(para, plan, keypoints, iuv)
        return (para, info), para_fit

    def people(self, para_h, verts_h, plan, **columns):
        """One dict over all P people of the plan from the rows and vertices on the host, plus further per-person columns."""
        P = plan['P']
        if P:
            k = person_cameras(para_h[:, 0:3], plan['tinv'], plan['shapes'], plan['person_frame'], self.res, self.focal, self.focal_full)
        return dict({'para': para_h, 'cam': para_h[:, 0:3], 'cam_t_full': k['cam_t_full'] if P else np.zeros((0, 3)),
                     'focal_full': k['focal_full'] if P else np.zeros(0), 'center': plan['center'], 'scale': plan['scale'], 'vertices': verts_h},
                    **columns)

    def __call__(self, frames, boxes, keypoints=None):
        plan = self.prepare(frames, boxes)
        P = plan['P']
        para, iuv = self.infer_stage(plan)
        fitted, para = self.fit_stage(para, plan, keypoints, iuv)
        verts = self.vertices(para) if P else None
        out = self.render(para, plan, vertices=verts)
        rendered = unpack_frames(out.cpu().numpy(), plan['offsets'], plan['shapes'])
        para_h = para.cpu().numpy()
        verts_h = verts.cpu().numpy() if P else np.zeros((0, 0, 3), np.float32)
        return rendered, split_people(self.people(para_h, verts_h, plan, **fit_columns(fitted, P)), plan)
