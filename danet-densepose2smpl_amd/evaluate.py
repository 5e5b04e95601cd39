"""The evaluation pipeline of the reference's eval.py: MPJPE / reconstruction error (Human3.6M P1 / P2, 3DPW, MPI-INF-3DHP) and
the LSP mask / part accuracy and F1, with the scoring on the device (csrc/eval_ops.hip).

  Evaluator        per-batch scoring: SMPL forward, ops.pose_eval (one launch), with eval_pve ops.vertex_eval (one launch: the PVE rule
                   of DESIGN.md 4c), for 'lsp' PartRenderer + ops.seg_confusion (one launch).  Errors and counters stay on the
                   device; summary() makes the one host copy.
  run_evaluation   the reference's loop and signature around a DaNet (infer_net) or an InferenceEngine.
  EvalDataset      an annotation .npz of the reference's layout (datasets/base_dataset.py, is_train=False) + image files.
  uncrop_geometry  the host side of the uncrop rule: paste rectangle and nearest-neighbour index tables that replace
                   utils/imutils.uncrop -- no image at the original resolution is ever written.

There is no CPU path: the ops raise on CPU tensors like every other op of the package.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import augment, constants, ops
from ._lib import GPU_ONLY, require_gpu
from .smpl import from_para

POSE_DATASETS = ('h36m-p1', 'h36m-p2', '3dpw', 'mpi-inf-3dhp')
DATASETS = POSE_DATASETS + ('lsp',)


def dataset_plan(dataset_name):
    """eval.py:128-140,187-199: what is scored for a dataset, with which joint mappers and from which ground truth."""
    if dataset_name not in DATASETS:
        raise ValueError('unknown evaluation dataset %r (one of %s)' % (dataset_name, ', '.join(DATASETS)))
    mpi = dataset_name == 'mpi-inf-3dhp'
    return {'eval_pose': dataset_name in POSE_DATASETS, 'eval_masks': dataset_name == 'lsp', 'eval_parts': dataset_name == 'lsp',
            'joint_mapper_h36m': list(constants.H36M_TO_J17 if mpi else constants.H36M_TO_J14),
            'joint_mapper_gt': list(constants.J24_TO_J17 if mpi else constants.J24_TO_J14),
            'gt_source': 'vertices' if dataset_name == '3dpw' else ('joints' if dataset_name in POSE_DATASETS else None),
            'per_action': dataset_name == 'h36m-p2'}


# ---- the uncrop rule -----------------------------------------------------------------------------------------------------------
_NEAREST = {}


def nearest_table(n_in, n_out):
    """Source index of each of n_out output pixels when PIL resizes n_in pixels with resample=NEAREST (what scipy.misc.imresize
    (interp='nearest') of utils/imutils.py:111 was): a running sum in double precision, a = n_in / n_out, x = a / 2, src[d] =
    int(x), x += a.  (The closed form floor((2 d + 1) n_in / (2 n_out)) differs from PIL at exact ties.)"""
    key = (int(n_in), int(n_out))
    t = _NEAREST.get(key)
    if t is None:
        if key[1] <= 0:
            raise ValueError('nearest_table: %d output pixels' % key[1])
        a = key[0] / key[1]
        steps = np.full(key[1], a, dtype=np.float64)
        steps[0] = 0.5 * a
        t = np.minimum(np.cumsum(steps).astype(np.int32), key[0] - 1)       # (numpy accumulates in order: the same running sum)
        t.setflags(write=False)
        if len(_NEAREST) < 4096:
            _NEAREST[key] = t
    return t


def uncrop_geometry(center, scale, orig_shape, res=constants.IMG_RES):
    """utils/imutils.py:89-113 without the image: for each sample the rectangle (y0, y1, x0, x1) of the original image the resized
    crop is pasted into, and for its rows / columns the row / column of the res x res rendering they show.
    center [B,2], scale [B], orig_shape [B,2] (rows, cols) -> list of (rect, row_table, col_table); rect = None when the crop misses
    the image."""
    center = np.asarray(center, dtype=np.float64).reshape(-1, 2)
    B = center.shape[0]
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    orig_shape = np.asarray(orig_shape).reshape(B, 2)
    corners = np.zeros((B, 2, 2), dtype=np.int64)                                   # ul, br as (x, y)
    for b in range(B):
        # augment.get_transform / transform for one unrotated sample in numpy, operation by operation as the reference: the
        # corners sit at exact ties of the truncation (centre - 100 scale), where one different rounding (torch divides a scalar by a
        # tensor as scalar * reciprocal; another inverse) moves the rectangle by a pixel
        h = 200 * scale[b]
        t = np.zeros((3, 3))
        t[0, 0] = float(res) / h
        t[1, 1] = float(res) / h
        t[0, 2] = res * (-float(center[b, 0]) / h + .5)
        t[1, 2] = res * (-float(center[b, 1]) / h + .5)
        t[2, 2] = 1
        tinv = np.linalg.inv(t)
        for k, p in enumerate((1., res + 1.)):
            corners[b, k] = np.dot(tinv, np.array([p - 1, p - 1, 1.]))[:2].astype(int) + 1 - 1
    out = []
    for b in range(B):
        (ulx, uly), (brx, bry) = corners[b]
        H, W = int(orig_shape[b, 0]), int(orig_shape[b, 1])
        ch, cw = int(bry - uly), int(brx - ulx)
        if ch <= 0 or cw <= 0:
            raise ValueError('uncrop_geometry: sample %d has an empty crop (%d x %d); scale %g' % (b, ch, cw, scale[b]))
        y0, y1 = max(0, uly), min(H, bry)
        x0, x1 = max(0, ulx), min(W, brx)
        if y1 <= y0 or x1 <= x0:
            out.append((None, None, None))
            continue
        rows = nearest_table(res, ch)[y0 - uly:y1 - uly]
        cols = nearest_table(res, cw)[x0 - ulx:x1 - ulx]
        out.append(((int(y0), int(y1), int(x0), int(x1)), rows, cols))
    return out


def pack_labels(gt_masks, gt_parts, center, scale, res=constants.IMG_RES, device=None):
    """The arguments of ops.seg_confusion for a batch: label images (lists of uint8 [H,W] arrays; one of the two lists may be None)
    packed into flat buffers, their offsets and shapes, the paste rectangles and index tables.  -> dict of tensors (+ 'max_pixels')."""
    imgs = gt_masks if gt_masks is not None else gt_parts
    B = len(imgs)
    shapes = np.array([im.shape[:2] for im in imgs], dtype=np.int32).reshape(B, 2)
    for lst in (gt_masks, gt_parts):
        if lst is not None and (len(lst) != B or any(tuple(l.shape[:2]) != tuple(s) or l.ndim != 2 for l, s in zip(lst, shapes))):
            raise ValueError('pack_labels: the mask and part label images of a sample must be [H,W] and share one size')
    sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
    offsets = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    geo = uncrop_geometry(center, scale, shapes, res)
    rects = np.zeros((B, 6), dtype=np.int32)
    tabs, pos = [], 0
    for b, (rect, rows, cols) in enumerate(geo):
        if rect is None:
            rects[b] = (0, 0, 0, 0, 0, 0)
            continue
        rects[b] = rect + (pos, pos + len(rows))
        tabs += [rows, cols]
        pos += len(rows) + len(cols)
    tables = np.concatenate(tabs).astype(np.int32) if tabs else np.zeros(1, dtype=np.int32)
    flat = lambda lst: None if lst is None else np.concatenate([np.ascontiguousarray(l, dtype=np.uint8).reshape(-1) for l in lst])
    to = lambda a: None if a is None else (torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device, non_blocking=True))
    return {'gt_mask': to(flat(gt_masks)), 'gt_parts': to(flat(gt_parts)), 'offsets': to(offsets), 'shapes': to(shapes), 'rects': to(rects),
            'tables': to(tables), 'max_pixels': int(sizes.max())}


# ---- scoring ---------------------------------------------------------------------------------------------------------------------
def h36m_action(imgname):
    """eval.py:152: the action of a Human3.6M image name (S9_Directions_1.54138969_000001.jpg -> Directions)."""
    return str(imgname).split('/')[-1].split('.')[0].split('_')[1]


def _f1(tp, fp, fn):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float((2. * tp / (2. * tp + fp + fn)).mean())                  # (a class that never occurs gives nan, as in eval.py)


class Evaluator(object):
    """Scores batches of predictions for one evaluation dataset.

    Evaluator(dataset_name, J_regressor [17,V], smpl_neutral, smpl_male=None, smpl_female=None, part_renderer=None, eval_pve=False)
    update(batch, para) -- batch: the dict run_evaluation's loader yields (device tensors 'pose', 'betas', 'gender', 'pose_3d',
    'center', 'scale'; for 'lsp' the host lists 'gt_mask' / 'gt_parts'; 'imgname'), para [B,229] = (camera 3, betas 10, 24 rotation
    matrices).  Enqueues only; nothing is read back.  summary() -> dict with the quantities eval.py prints.
    eval_pve (the reference's dead --eval_pve; 'lsp' ignores it): the per-vertex error PVE and its Procrustes-aligned form PA-PVE
     against the ground-truth mesh -- for '3dpw' the gendered mesh pose_eval is scored against, else the neutral
    model's mesh of the batch's pose and betas (eval.py:146), where a sample counts iff batch['has_smpl'] is 1 (absent: all).
    summary() then carries pve / pa_pve (mm, float64 means over the counted samples), pve_per_sample / pa_pve_per_sample and
    pve_num_samples; with no counted sample the four metric keys are absent."""

    def __init__(self, dataset_name, J_regressor, smpl_neutral, smpl_male=None, smpl_female=None, part_renderer=None, eval_pve=False):
        self.dataset_name = dataset_name
        self.plan = dataset_plan(dataset_name)
        self.smpl_neutral, self.smpl_male, self.smpl_female = smpl_neutral, smpl_male, smpl_female
        if self.plan['gt_source'] == 'vertices' and (smpl_male is None or smpl_female is None):
            raise ValueError("'3dpw' takes its ground truth from the male / female SMPL models: pass smpl_male and smpl_female")
        if self.plan['eval_masks'] and part_renderer is None:
            raise ValueError("'lsp' needs a PartRenderer")
        self.part_renderer = part_renderer
        self.device = smpl_neutral.v_template.device
        if self.device.type != 'cuda':
            raise RuntimeError(GPU_ONLY % ('Evaluator SMPL model', self.device))
        self.J_regressor = torch.as_tensor(J_regressor).float().contiguous().to(self.device)
        self.counters = torch.zeros(ops.SEG_COUNTERS, dtype=torch.int64, device=self.device)
        self._mpjpe, self._recon, self._j17, self._pose, self._betas, self._cam, self._names = [], [], [], [], [], [], []
        self.eval_pve = bool(eval_pve) and self.plan['eval_pose']
        self._pve, self._pa_pve, self._pve_on = [], [], []

    def update(self, batch, para):
        require_gpu(para, 'Evaluator.update')
        B = para.shape[0]
        cam = para[:, 0:3].clone()                                                 # (an engine's `para` is a static buffer)
        betas = para[:, 3:13].clone()
        with torch.no_grad():
            verts = from_para(self.smpl_neutral, para).vertices
            self._pose.append(ops.rotmat_to_angle_axis(para[:, 13:]).view(B, 72))   # eval.py:175-181
            self._betas.append(betas)
            self._cam.append(cam)
            self._names += [str(n) for n in batch.get('imgname', [''] * B)]
            if self.plan['eval_pose']:
                if self.plan['gt_source'] == 'joints':
                    gt = batch['pose_3d'].to(self.device)[:, self.plan['joint_mapper_gt'], :-1].contiguous()
                    e, r, j17 = ops.pose_eval(verts, self.J_regressor, self.plan['joint_mapper_h36m'], gt_keypoints_3d=gt)
                    if self.eval_pve:
                        gp, gb = batch['pose'].to(self.device), batch['betas'].to(self.device)
                        gv = self.smpl_neutral(global_orient=gp[:, :3], body_pose=gp[:, 3:], betas=gb).vertices        # eval.py:146
                        has = batch.get('has_smpl')
                        counted = torch.ones(B, dtype=torch.bool, device=self.device) if has is None else torch.as_tensor(has).to(self.device).view(B) > 0
                else:
                    gp, gb = batch['pose'].to(self.device), batch['betas'].to(self.device)
                    vm = self.smpl_male(global_orient=gp[:, :3], body_pose=gp[:, 3:], betas=gb).vertices
                    vf = self.smpl_female(global_orient=gp[:, :3], body_pose=gp[:, 3:], betas=gb).vertices
                    gv = torch.where((batch['gender'].to(self.device) == 1).view(B, 1, 1), vf, vm)
                    e, r, j17 = ops.pose_eval(verts, self.J_regressor, self.plan['joint_mapper_h36m'], gt_vertices=gv)
                    counted = torch.ones(B, dtype=torch.bool, device=self.device)
                if self.eval_pve:
                    pve, pa = ops.vertex_eval(verts, gv, self.J_regressor[0])
                    self._pve.append(pve)
                    self._pa_pve.append(pa)
                    self._pve_on.append(counted)
                self._mpjpe.append(e)
                self._recon.append(r)
                self._j17.append(j17)
            if self.plan['eval_masks'] or self.plan['eval_parts']:
                mask, parts = self.part_renderer(verts, cam)
                lab = batch.get('labels')
                if lab is None:
                    lab = pack_labels(batch['gt_mask'], batch['gt_parts'], _host(batch['center']), _host(batch['scale']),
                                      self.part_renderer.render_res, self.device)
                ops.seg_confusion(mask, parts, lab['gt_mask'], lab['gt_parts'], lab['offsets'], lab['shapes'], lab['rects'], lab['tables'],
                                  lab['max_pixels'], self.counters)

    def summary(self):
        cat = lambda lst, shape: (torch.cat(lst).double().cpu().numpy() if lst else np.zeros(shape))
        out = {'dataset': self.dataset_name, 'num_samples': len(self._names)}
        c = self.counters.cpu().numpy()
        res = {'pose': cat(self._pose, (0, 72)), 'betas': cat(self._betas, (0, 10)), 'camera': cat(self._cam, (0, 3)),
               'pred_joints': cat(self._j17, (len(self._names), 17, 3))}
        out['results'] = res
        if self.plan['eval_pose']:
            mp, re = cat(self._mpjpe, (0,)), cat(self._recon, (0,))
            out.update(mpjpe=float(1000 * mp.mean()), recon_err=float(1000 * re.mean()), mpjpe_per_sample=mp, recon_err_per_sample=re)
            if self.plan['per_action']:                                            # eval.py:302-316
                acts = {}
                for i, n in enumerate(self._names):
                    acts.setdefault(h36m_action(n), []).append(i)
                out['actions'] = {a: {'mpjpe': float(mp[ix].mean() * 1000.), 'recon_err': float(re[ix].mean() * 1000.)} for a, ix in acts.items()}
            if self.eval_pve:
                on = torch.cat(self._pve_on).cpu().numpy() if self._pve_on else np.zeros(0, bool)
                out['pve_num_samples'] = int(on.sum())
                if on.any():
                    pv, pa = cat(self._pve, (0,))[on], cat(self._pa_pve, (0,))[on]
                    out.update(pve=float(1000 * pv.mean()), pa_pve=float(1000 * pa.mean()), pve_per_sample=pv, pa_pve_per_sample=pa)
        if self.plan['eval_masks']:
            S = ops.SEG
            tp, fp, fn = (c[S[k]:S[k] + 2].astype(np.float64) for k in ('tp', 'fp', 'fn'))
            out.update(accuracy=float(c[S['accuracy']]) / max(int(c[S['pixel_count']]), 1), f1=_f1(tp, fp, fn))
        if self.plan['eval_parts']:
            S = ops.SEG
            tp, fp, fn = (c[S[k]:S[k] + 7].astype(np.float64) for k in ('parts_tp', 'parts_fp', 'parts_fn'))
            out.update(parts_accuracy=float(c[S['parts_accuracy']]) / max(int(c[S['parts_pixel_count']]), 1), parts_f1=_f1(tp, fp, fn))
        if self.plan['eval_masks'] or self.plan['eval_parts']:
            out['counters'] = {k: (c[i:i + (2 if k in ('tp', 'fp', 'fn') else 7)].copy() if k.endswith(('tp', 'fp', 'fn')) else int(c[i]))
                               for k, i in ops.SEG.items()}
        return out


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def print_summary(s, header='*** Final Results ***'):
    """eval.py:287-316."""
    print(header)
    if 'mpjpe' in s:
        print('MPJPE: ' + str(s['mpjpe']))
        print('Reconstruction Error: ' + str(s['recon_err']))
        if 'pve' in s:
            print('PVE: ' + str(s['pve']))
            print('PA-PVE: ' + str(s['pa_pve']))
        print()
    if 'accuracy' in s:
        print('Accuracy: ', s['accuracy'])
        print('F1: ', s['f1'])
        print()
    if 'parts_accuracy' in s:
        print('Parts Accuracy: ', s['parts_accuracy'])
        print('Parts F1 (BG): ', s['parts_f1'])
        print()
    if 'actions' in s:
        print(['action err'] + [str(v['recon_err']) for v in s['actions'].values()] + list(s['actions']))


# ---- data ------------------------------------------------------------------------------------------------------------------------
def read_array(path, gray=False):
    """.npy always; .png / .jpg when PIL can be imported (the rule of tools/demo.py)."""
    if path.lower().endswith('.npy'):
        return np.load(path)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError('%s: reading .jpg / .png needs PIL, which is not installed; convert the files to .npy arrays' % path)
    return np.asarray(Image.open(path).convert('L' if gray else 'RGB'))


class EvalDataset(object):
    """datasets/base_dataset.py with is_train=False (no augmentation): `annot` is the .npz of the reference's layout (imgname, center,
    scale and, where the dataset has them, pose, shape, S, gender, maskname, partname), `img_dir` holds the images and `label_dir` (the
    reference's 'upi-s1h' folder) the LSP label images.  An item carries the UNCROPPED image (uint8 [H,W,3]); the crop is one batched
    resampling pass on the device (augment.rgb_processing) in `to_device`."""

    def __init__(self, annot, img_dir, dataset_name, label_dir=None, img_res=constants.IMG_RES):
        self.dataset = dataset_name
        self.img_dir, self.label_dir, self.img_res = img_dir, label_dir if label_dir is not None else img_dir, img_res
        d = np.load(annot, allow_pickle=True) if isinstance(annot, str) else annot
        self.imgname = [str(n) for n in d['imgname']]
        n = len(self.imgname)
        self.scale, self.center = np.asarray(d['scale'], np.float64).reshape(n), np.asarray(d['center'], np.float64).reshape(n, 2)
        has = lambda k: k in (d.files if hasattr(d, 'files') else d)
        self.pose = np.asarray(d['pose'], np.float64) if has('pose') and has('shape') else np.zeros((n, 72))
        self.betas = np.asarray(d['shape'], np.float64) if has('pose') and has('shape') else np.zeros((n, 10))
        self.pose_3d = np.asarray(d['S'], np.float64) if has('S') else np.zeros((n, 24, 4))
        self.gender = (np.array([0 if str(g) == 'm' else 1 for g in d['gender']], np.int32) if has('gender') else -np.ones(n, np.int32))
        self.has_smpl = np.asarray(d['has_smpl'], np.float32).reshape(n) if has('has_smpl') else np.ones(n, np.float32)
        self.maskname = [str(m) for m in d['maskname']] if has('maskname') else None
        self.partname = [str(m) for m in d['partname']] if has('partname') else None

    def __len__(self):
        return len(self.imgname)

    def __getitem__(self, i):
        img = read_array(os.path.join(self.img_dir, self.imgname[i]))
        if img.ndim == 2:
            img = np.repeat(img[:, :, None], 3, 2)
        item = {'img_raw': np.ascontiguousarray(img[:, :, :3]), 'orig_shape': np.array(img.shape[:2]), 'imgname': os.path.join(self.img_dir, self.imgname[i]),
                'center': self.center[i].astype(np.float32), 'scale': float(self.scale[i]), 'pose': self.pose[i].astype(np.float32),
                'betas': self.betas[i].astype(np.float32), 'pose_3d': self.pose_3d[i].astype(np.float32), 'gender': self.gender[i],
                'has_smpl': self.has_smpl[i], 'sample_index': i, 'maskname': self.maskname[i] if self.maskname else '', 'partname': self.partname[i] if self.partname else ''}
        if self.dataset == 'lsp':
            item['gt_mask'] = np.ascontiguousarray(read_array(os.path.join(self.label_dir, item['maskname']), gray=True), dtype=np.uint8)
            item['gt_parts'] = np.ascontiguousarray(read_array(os.path.join(self.label_dir, item['partname']), gray=True), dtype=np.uint8)
        return item


def collate(items):
    """A list of EvalDataset items -> one host batch: stacked arrays, the images zero-padded to the batch's largest size (the crop
    samples zeros outside an image anyway), the label images as lists."""
    B = len(items)
    H, W = max(it['img_raw'].shape[0] for it in items), max(it['img_raw'].shape[1] for it in items)
    raw = np.zeros((B, H, W, 3), dtype=np.uint8)
    for b, it in enumerate(items):
        raw[b, :it['img_raw'].shape[0], :it['img_raw'].shape[1]] = it['img_raw']
    batch = {'img_raw': raw}
    for k in ('center', 'scale', 'pose', 'betas', 'pose_3d', 'gender', 'orig_shape', 'sample_index'):
        batch[k] = np.stack([np.asarray(it[k]) for it in items])
    if 'has_smpl' in items[0]:
        batch['has_smpl'] = np.stack([np.asarray(it['has_smpl'], np.float32) for it in items])
    for k in ('imgname', 'maskname', 'partname'):
        batch[k] = [it[k] for it in items]
    if 'gt_mask' in items[0]:
        batch['gt_mask'], batch['gt_parts'] = [it['gt_mask'] for it in items], [it['gt_parts'] for it in items]
    return batch


def to_device(batch, device, img_res=constants.IMG_RES):
    """Uploads a collated batch and crops its images: adds 'img' [B,3,res,res] (normalised, base_dataset.py:248-251 with no
    augmentation) and, for 'lsp', 'labels' (pack_labels)."""
    out = dict(batch)
    for k in ('center', 'scale', 'pose', 'betas', 'pose_3d', 'gender') + (('has_smpl',) if 'has_smpl' in batch else ()):
        out[k] = torch.from_numpy(np.ascontiguousarray(batch[k])).to(device, non_blocking=True)
    raw = torch.from_numpy(batch['img_raw']).to(device, non_blocking=True).permute(0, 3, 1, 2).float()
    B = raw.shape[0]
    out['img'] = augment.rgb_processing(raw, out['center'].double(), out['scale'].double(), torch.zeros(B, device=device), torch.zeros(B, device=device),
                                        torch.ones(B, 3, device=device), res=img_res).float().contiguous()
    if 'gt_mask' in batch:
        out['labels'] = pack_labels(batch['gt_mask'], batch['gt_parts'], batch['center'], batch['scale'], constants.IMG_RES, device)
    del out['img_raw']
    return out


def iterate_batches(dataset, batch_size, shuffle=False, num_workers=0, seed=0):
    """Collated host batches in order (or a seeded permutation).  `num_workers` read ahead in THREADS (at most 8; decoding and numpy
    release the interpreter lock): a process that holds a GPU context does not fork."""
    order = np.random.default_rng(seed).permutation(len(dataset)) if shuffle else np.arange(len(dataset))
    chunks = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    load = lambda idx: collate([dataset[int(i)] for i in idx])
    workers = max(0, min(int(num_workers), 8))
    if workers == 0:
        for c in chunks:
            yield load(c)
        return
    with ThreadPoolExecutor(max_workers=workers) as ex:
        pending = [ex.submit(load, c) for c in chunks[:workers]]
        for k in range(len(chunks)):
            if k + workers < len(chunks):
                pending.append(ex.submit(load, chunks[k + workers]))
            yield pending[k].result()
            pending[k] = None


# ---- synthetic stand-ins for the licence-gated files -------------------------------------------------------------------------------
def synthetic_h36m_regressor(num_verts=6890, seed=0):
    """A stand-in for J_regressor_h36m.npy: 17 rows of 32 non-negative weights each that sum to 1."""
    rng = np.random.default_rng(seed)
    J = np.zeros((17, num_verts), dtype=np.float32)
    for j in range(17):
        idx = rng.choice(num_verts, 32, replace=False)
        w = rng.random(32)
        J[j, idx] = (w / w.sum()).astype(np.float32)
    return J


def synthetic_part_renderer(faces, seed=0, render_res=constants.IMG_RES):
    """A PartRenderer on stand-ins for the reference's vertex_texture.npy / cube_parts.npy: each face a colour in the middle of a
    cube cell, the cell's part 1..6 by the face's index."""
    from .renderer import PartRenderer
    faces = np.asarray(faces).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    F = faces.shape[0]
    cell = rng.integers(0, 100, (F, 3))
    cube = np.zeros((100, 100, 100), dtype=np.float32)
    cube[cell[:, 0], cell[:, 1], cell[:, 2]] = 1 + (np.arange(F) * 6 // F)            # (the later face wins a shared cell)
    tex = (cell.astype(np.float32) + 0.5) / 100.0
    return PartRenderer(faces, tex, cube, render_res=render_res)


def write_synthetic_dataset(root, dataset_name, n=8, seed=0):
    """A small dataset of the reference's layout under `root` (images and label images as .npy): -> path of its annotation .npz.
    Images of different, non-square sizes; crops that overhang the image; LSP label images with every class and some 255."""
    dataset_plan(dataset_name)
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    acts = ['Directions', 'Eating', 'Walking']
    names, masks, parts = [], [], []
    center, scale = np.zeros((n, 2)), np.zeros(n)
    for i in range(n):
        H, W = int(rng.integers(150, 330)), int(rng.integers(150, 330))
        name = 'S9_%s_1.54138969_%06d.npy' % (acts[i % len(acts)], i + 1) if dataset_name.startswith('h36m') else 'im%04d.npy' % (i + 1)
        np.save(os.path.join(root, name), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        names.append(name)
        center[i] = (W / 2 + rng.uniform(-0.3, 0.3) * W, H / 2 + rng.uniform(-0.3, 0.3) * H)
        scale[i] = rng.uniform(0.5, 1.6) * max(H, W) / 200.
        if dataset_name == 'lsp':
            yy, xx = np.mgrid[0:H, 0:W]
            p = ((xx * 7 // W + yy * 3 // H) % 7).astype(np.uint8)
            p[(np.abs(xx - center[i, 0]) > W / 3) | (np.abs(yy - center[i, 1]) > H / 3)] = 0
            p[rng.random((H, W)) < 0.02] = 255
            m = ((p > 0) & (p != 255)).astype(np.uint8) * 255
            np.save(os.path.join(root, 'im%04d_mask.npy' % (i + 1)), m)
            np.save(os.path.join(root, 'im%04d_parts.npy' % (i + 1)), p)
            masks.append('im%04d_mask.npy' % (i + 1))
            parts.append('im%04d_parts.npy' % (i + 1))
    S = np.concatenate([rng.normal(0, 0.3, (n, 24, 3)), np.ones((n, 24, 1))], axis=2)
    S[:, :, :3] -= S[:, [14], :3]
    arrs = {'imgname': np.array(names), 'center': center, 'scale': scale, 'pose': rng.normal(0, 0.2, (n, 72)),
            'shape': np.clip(rng.normal(0, 1, (n, 10)), -3, 3), 'S': S, 'gender': np.array(['m' if i % 2 == 0 else 'f' for i in range(n)])}
    if dataset_name == 'lsp':
        arrs.update(maskname=np.array(masks), partname=np.array(parts))
    path = os.path.join(root, '%s_test.npz' % dataset_name.replace('-', '_'))
    np.savez(path, **arrs)
    return path


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def eval_target(model):
    """-> (callable image -> dict with 'para', the DaNet behind it, its device); a model on the CPU is refused."""
    if hasattr(model, 'infer_net'):
        infer, net = model.infer_net, model
    elif hasattr(model, 'model') and hasattr(model.model, 'iuv2smpl') and callable(model):
        infer, net = model, model.model                                            # an InferenceEngine
    else:
        raise TypeError('run_evaluation: model must be a DaNet or an InferenceEngine, got %s' % type(model).__name__)
    device = next(net.parameters()).device
    if device.type != 'cuda':
        raise RuntimeError(GPU_ONLY % ('run_evaluation model', device))
    return infer, net, device


def eval_batches(dataset, device, result_file, batch_size, img_res, num_workers, shuffle):
    """The loop's batches on the device; in dataset order when a result file is written (eval.py:81-83, eval_coco.py:61-63)."""
    for host in iterate_batches(dataset, batch_size, shuffle and result_file is None, num_workers):
        yield to_device(host, device, img_res)


def val_due(step_count, test_steps):
    """base_trainer.py:89-91: validation follows the steps with step_count % test_steps == 0; never for test_steps 0 / None."""
    return bool(test_steps) and int(test_steps) > 0 and int(step_count) > 0 and int(step_count) % int(test_steps) == 0


def run_evaluation(model, dataset_name, dataset, result_file, batch_size=32, img_res=224, num_workers=32, shuffle=False, log_freq=50,
                   options=None, verbose=True):
    """eval.py:57-316.  `model`: a DaNet in eval mode (infer_net is called) or an InferenceEngine.  `options` may carry what the
    reference reads from its path_config: J_regressor ([17,6890] array or .npy path), smpl_male / smpl_female (SMPL modules),
    part_renderer; what is missing is a seeded synthetic stand-in (the male / female models fall back to the neutral one).
    options.eval_pve adds the per-vertex errors (Evaluator).  Prints the reference's lines (verbose=False: nothing, for use inside
    Trainer.fit) and returns the summary dict; with `result_file` writes pred_joints, pose, betas, camera."""
    plan = dataset_plan(dataset_name)
    infer, net, device = eval_target(model)
    opt = lambda k: getattr(options, k, None) if options is not None else None
    smpl = net.iuv2smpl.smpl
    Jr = opt('J_regressor')
    if isinstance(Jr, str):
        Jr = np.load(Jr)
    if Jr is None:
        Jr = synthetic_h36m_regressor(smpl.v_template.shape[0])
    renderer = opt('part_renderer')
    if plan['eval_masks'] and renderer is None:
        renderer = synthetic_part_renderer(smpl.faces)
    ev = Evaluator(dataset_name, Jr, smpl, opt('smpl_male') or smpl, opt('smpl_female') or smpl, renderer, eval_pve=bool(opt('eval_pve')))
    for step, batch in enumerate(eval_batches(dataset, device, result_file, batch_size, img_res, num_workers, shuffle)):
        out = infer(batch['img'])
        ev.update(batch, out['para'])
        if verbose and log_freq and step % log_freq == log_freq - 1:
            print_summary(ev.summary(), 'step %d' % (step + 1))
    s = ev.summary()
    if result_file is not None:
        r = s['results']
        np.savez(result_file, pred_joints=r['pred_joints'], pose=r['pose'], betas=r['betas'], camera=r['camera'])
    if verbose:
        print_summary(s)
    return s
