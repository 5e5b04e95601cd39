"""COCO 2D keypoint AP / AR of the reference's eval_coco.py, with the back-projection and the per-image matching on the device
(csrc/coco_ops.hip) and the protocol of pycocotools.COCOeval written down as a rule (DESIGN.md 4c "the COCO keypoint rule":
pycocotools is absent here and unpinned).

  CocoKeypointGT       person_keypoints_*.json -> the ground truth packed by image, images in ascending id.
  CocoEvaluator        update(batch, para): SMPL forward + ops.coco_keypoints, enqueued only.  summary(): one host copy, the
                       evaluation order, ops.coco_oks_match (one launch for the dataset), the accumulation in fp64 numpy.
  accumulate           flags + counts -> precision [10,101,3], recall [10,3] and the ten numbers.
  write_results        the results json of _coco_keypoint_results_one_category_kernel.
  run_evaluation       the reference's loop and signature around a DaNet (infer_net) or an InferenceEngine.
  write_synthetic_coco a small val2014-shaped set for machines without the data.

Evaluation order (the tie rule).  eval_coco.py gives every keypoint and every box the score 1, so after the rescoring of
coco_keypoint_dataset.py:326-338 EVERY detection scores 1.0 and the order of the detections is decided by stable sorting alone:
images in ascending image id, within an image the order of the samples.  With more detections than ground truths in an image that
order decides which detection is the true positive, and with more than 20 which are dropped.

There is no CPU path: the ops raise on CPU tensors like every other op of the package.
"""
import json
import os

import numpy as np
import torch

from . import constants, ops
from ._lib import GPU_ONLY, require_gpu
from .evaluate import EvalDataset, eval_batches, eval_target, iterate_batches, to_device     # noqa: F401  (re-exported)
from .smpl import from_para

STAT_NAMES = ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']     # coco_keypoint_dataset.py:438
IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
MAX_DETS = ops.COCO_MAX_DETS
EPS = float(np.spacing(1))


def image_id(imgname):
    """coco_keypoint_dataset.py:312: COCO_val2014_000000000785.jpg -> 785."""
    return int(str(imgname)[-16:-4])


class CocoKeypointGT(object):
    """The ground truth of a person_keypoints_*.json (a path or the loaded dict), category 1 only, packed by image: image_ids [I]
    ascending (EVERY image of the file, also those without annotation or detection), offsets [I+1], kpts [M,17,3], area [M], bbox
    [M,4] (all float64, as the file holds them), iscrowd [M] and ignore [M] = iscrowd or num_keypoints == 0 (uint8), ann_ids [M].
    Within an image the annotations keep the order of the file."""

    def __init__(self, json_path_or_dict):
        d = json_path_or_dict
        if not isinstance(d, dict):
            with open(d) as f:
                d = json.load(f)
        self.image_ids = np.array(sorted(set(int(im['id']) for im in d['images'])), dtype=np.int64)
        index = {int(i): k for k, i in enumerate(self.image_ids)}
        per_image = [[] for _ in self.image_ids]
        for a in d.get('annotations', []):
            if int(a.get('category_id', 1)) != 1:
                continue
            if int(a['image_id']) not in index:
                raise ValueError('annotation %s names image %s, which the file does not list' % (a.get('id'), a['image_id']))
            per_image[index[int(a['image_id'])]].append(a)
        anns = [a for lst in per_image for a in lst]
        M = len(anns)
        self.offsets = np.zeros(len(per_image) + 1, dtype=np.int64)
        np.cumsum([len(lst) for lst in per_image], out=self.offsets[1:])
        self.kpts = np.array([a['keypoints'] for a in anns], dtype=np.float64).reshape(M, 17, 3)
        self.area = np.array([a['area'] for a in anns], dtype=np.float64).reshape(M)
        self.bbox = np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(M, 4)
        self.iscrowd = np.array([1 if a.get('iscrowd', 0) else 0 for a in anns], dtype=np.uint8).reshape(M)
        nk = np.array([a['num_keypoints'] if 'num_keypoints' in a else int((np.asarray(a['keypoints'])[2::3] > 0).sum()) for a in anns],
                      dtype=np.int64).reshape(M)
        self.ignore = ((self.iscrowd > 0) | (nk == 0)).astype(np.uint8)
        self.ann_ids = np.array([a.get('id', -1) for a in anns], dtype=np.int64).reshape(M)

    def __len__(self):
        return len(self.image_ids)

    def image_index(self, ids):
        """Position of each image id in image_ids; an id the annotation file does not list is an error (as in COCO.loadRes)."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        pos = np.searchsorted(self.image_ids, ids)
        bad = (pos >= len(self.image_ids)) | (self.image_ids[np.minimum(pos, len(self.image_ids) - 1)] != ids)
        if bad.any():
            raise ValueError('detections name image %d, which the annotation file does not list' % ids[bad][0])
        return pos

    def to(self, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return {'gt_kpts': t(self.kpts), 'gt_area': t(self.area), 'gt_bbox': t(self.bbox), 'gt_ignore': t(self.ignore),
                'gt_iscrowd': t(self.iscrowd), 'gt_offsets': t(self.offsets)}


def detection_area(kpts):
    """COCO.loadRes for keypoints: (max x - min x) * (max y - min y) over the 17 keypoints, in float64.  kpts [N,17,2+]."""
    k = np.asarray(kpts, dtype=np.float64)
    return (k[:, :, 0].max(1) - k[:, :, 0].min(1)) * (k[:, :, 1].max(1) - k[:, :, 1].min(1))


def evaluation_order(image_ids, gt):
    """The tie rule: the samples (in the order they were seen) sorted by image id, stably -> (order [N], dt_offsets [I+1] over
    gt.image_ids)."""
    pos = gt.image_index(image_ids)
    order = np.argsort(pos, kind='stable')
    offsets = np.zeros(len(gt) + 1, dtype=np.int64)
    np.cumsum(np.bincount(pos, minlength=len(gt)), out=offsets[1:])
    return order, offsets


def _mean(x):
    x = x[x > -1]
    return float(x.mean()) if x.size else -1.0


def accumulate(dt_match, dt_ignore, gt_count, scores=None):
    """COCOeval.accumulate + summarize for one category and maxDets = 20.  dt_match / dt_ignore [N,3] integer words (bit t =
    threshold t, column = area range) of the detections in evaluation order, gt_count [I,3]; scores [N] (default: all equal, the
    reference's case).  -> dict: 'precision' [10,101,3], 'recall' [10,3] (-1 where a range has no ground truth), 'stats' [10]."""
    dt_match, dt_ignore = np.asarray(dt_match).astype(np.int64).reshape(-1, 3), np.asarray(dt_ignore).astype(np.int64).reshape(-1, 3)
    gt_count = np.asarray(gt_count).astype(np.int64).reshape(-1, 3)
    N, T, R, A = dt_match.shape[0], len(IOU_THRS), len(REC_THRS), len(AREA_RANGES)
    order = np.arange(N) if scores is None else np.argsort(-np.asarray(scores, dtype=np.float64), kind='mergesort')
    precision, recall = -np.ones((T, R, A)), -np.ones((T, A))
    bit = np.arange(T)[:, None]
    for a in range(A):
        npig = int(gt_count[:, a].sum())
        if npig == 0:
            continue
        m = ((dt_match[order, a][None, :] >> bit) & 1).astype(bool)
        ig = ((dt_ignore[order, a][None, :] >> bit) & 1).astype(bool)
        tps = np.cumsum(m & ~ig, axis=1).astype(np.float64)
        fps = np.cumsum(~m & ~ig, axis=1).astype(np.float64)
        for t in range(T):
            tp, fp = tps[t], fps[t]
            rc = tp / npig
            pr = tp / (fp + tp + EPS)
            recall[t, a] = rc[-1] if N else 0.0
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            inds = np.searchsorted(rc, REC_THRS, side='left')
            q = np.zeros(R)
            ok = inds < N
            q[ok] = pr[inds[ok]]
            precision[t, :, a] = q
    stats = [_mean(precision[:, :, 0]), _mean(precision[0, :, 0]), _mean(precision[5, :, 0]), _mean(precision[:, :, 1]), _mean(precision[:, :, 2]),
             _mean(recall[:, 0]), _mean(recall[0, 0:1]), _mean(recall[5, 0:1]), _mean(recall[:, 1]), _mean(recall[:, 2])]
    return {'precision': precision, 'recall': recall, 'stats': np.array(stats, dtype=np.float64)}


def result_records(preds, image_ids, center, scale):
    """_coco_keypoint_results_one_category_kernel: one record per detection, grouped by image in the order the images were first
    seen: image_id, category_id, keypoints[51] = (x, y, 1) x 17, score, center, scale (the reference's scale_ = (scale, scale))."""
    preds = np.asarray(preds, dtype=np.float32).reshape(-1, 17, 2)
    groups = {}
    for i, im in enumerate(image_ids):
        groups.setdefault(int(im), []).append(i)
    out = []
    for im, idx in groups.items():
        for i in idx:
            k = np.concatenate([preds[i].astype(np.float64), np.ones((17, 1))], axis=1).reshape(-1)
            out.append({'image_id': im, 'category_id': 1, 'keypoints': [float(v) for v in k], 'score': 1.0,
                        'center': [float(v) for v in np.asarray(center[i]).reshape(2)], 'scale': [float(scale[i]), float(scale[i])]})
    return out


def write_results(path, preds, image_ids, center, scale):
    """coco_keypoint_dataset.py:367-393: the results json (sort_keys, indent 4).  -> the records."""
    rec = result_records(preds, image_ids, center, scale)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(rec, f, sort_keys=True, indent=4)
    return rec


class CocoEvaluator(object):
    """Scores batches of predictions against a CocoKeypointGT.

    CocoEvaluator(gt, smpl_neutral, img_res=224, focal_length=5000.)
    update(batch, para) -- batch: the dict run_evaluation's loader yields (device tensors 'center', 'scale'; 'imgname'), para [B,229]
    = (camera 3, betas 10, 24 rotation matrices).  Enqueues the SMPL forward and ops.coco_keypoints; nothing is read back.
    summary() -> dict: 'names', 'values', 'name_value' (ordered), 'precision', 'recall', 'order' and the flags 'dt_match' / 'dt_ignore'
    (detections in evaluation order) / 'gt_count' as the kernel wrote them, 'results' (preds in the order seen, ...)."""

    def __init__(self, gt, smpl_neutral, img_res=constants.IMG_RES, focal_length=constants.FOCAL_LENGTH):
        self.gt = gt if isinstance(gt, CocoKeypointGT) else CocoKeypointGT(gt)
        self.smpl = smpl_neutral
        self.device = smpl_neutral.v_template.device
        if self.device.type != 'cuda':
            raise RuntimeError(GPU_ONLY % ('CocoEvaluator SMPL model', self.device))
        self.img_res, self.focal_length = int(img_res), float(focal_length)
        self._preds, self._para, self._center, self._scale, self._names = [], [], [], [], []

    def update(self, batch, para):
        require_gpu(para, 'CocoEvaluator.update')
        B = para.shape[0]
        para = para.detach().clone()                                               # (an engine's `para` is a static buffer)
        center, scale = batch['center'].to(self.device), batch['scale'].to(self.device).reshape(B)
        with torch.no_grad():
            preds = ops.coco_keypoints(from_para(self.smpl, para).joints, para[:, 0:3].contiguous(), center, scale, self.img_res, self.focal_length)
        self._preds.append(preds)
        self._para.append(para)
        self._center.append(center)
        self._scale.append(scale)
        self._names += [str(n) for n in batch['imgname']]
        return preds

    def summary(self):
        n = len(self._names)
        cat = lambda lst, shape: (torch.cat(lst).double().cpu().numpy() if lst else np.zeros(shape))
        preds = torch.cat(self._preds) if n else torch.zeros(0, 17, 2, device=self.device)
        preds_h = preds.cpu().numpy()                                              # the one host copy the protocol needs
        ids = np.array([image_id(x) for x in self._names], dtype=np.int64)
        order, dt_offsets = evaluation_order(ids, self.gt)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        area = detection_area(preds_h)
        g = self.gt.to(self.device)
        dm, di, gc = ops.coco_oks_match(preds[dev(order)].contiguous(), dev(area[order]), dev(dt_offsets), g['gt_kpts'], g['gt_area'], g['gt_bbox'],
                                        g['gt_ignore'], g['gt_iscrowd'], g['gt_offsets'])
        dm, di, gc = dm.cpu().numpy(), di.cpu().numpy(), gc.cpu().numpy()
        acc = accumulate(dm, di, gc)
        para = cat(self._para, (0, 229))
        values = [float(v) for v in acc['stats']]
        return {'names': list(STAT_NAMES), 'values': values, 'name_value': dict(zip(STAT_NAMES, values)), 'num_samples': n,
                'precision': acc['precision'], 'recall': acc['recall'], 'order': order, 'dt_match': dm, 'dt_ignore': di, 'gt_count': gc,
                'results': {'preds': preds_h, 'image_ids': ids, 'imgname': list(self._names), 'center': cat(self._center, (0, 2)),
                            'scale': cat(self._scale, (0,)), 'camera': para[:, 0:3], 'betas': para[:, 3:13], 'rotmat': para[:, 13:]}}


def _table_row(cells):
    return '| ' + ' | '.join(cells) + ' |'


def print_name_value(name_value, arch):
    """The markdown table eval_coco.py prints: a header row 'Arch' + the names, a rule, and the values to three decimals under the
    architecture's name (a name longer than 15 characters is cut to its first 8 and '...')."""
    label = arch if len(arch) <= 15 else arch[:8] + '...'
    print(_table_row(['Arch'] + [str(k) for k in name_value]))
    print('|---' * (len(name_value) + 1) + '|')
    print(_table_row([label] + ['%.3f' % v for v in name_value.values()]))


def run_evaluation(model, dataset, result_file, batch_size=32, img_res=224, num_workers=32, shuffle=False, options=None):
    """eval_coco.py:46-173.  `model`: a DaNet in eval mode (infer_net is called) or an InferenceEngine; `dataset`: an EvalDataset of
    val2014 crops (imgname / center / scale).  `options` carries keypoint_json (path, dict or CocoKeypointGT: required), and may carry
    regressor ('danet'; 'hmr' is refused) and output_dir (the results json goes to <output_dir>/results/, as in the reference).
    Prints the reference's markdown table and returns the ordered name -> value dict; with `result_file` writes the reference's .npz
    (pred_joints, pose, betas, camera) plus preds and image_ids."""
    opt = lambda k, default=None: getattr(options, k, default) if options is not None else default
    regressor = opt('regressor', 'danet') or 'danet'
    if regressor == 'hmr':
        raise NotImplementedError("regressor 'hmr': there is no HMR regressor in this package (DESIGN.md section 8); use 'danet'")
    if regressor != 'danet':
        raise ValueError("unknown regressor %r ('danet')" % (regressor,))
    infer, net, device = eval_target(model)
    gt = opt('keypoint_json')
    if gt is None:
        raise ValueError('run_evaluation: options.keypoint_json (the person_keypoints_*.json of the images) is required')
    ev = CocoEvaluator(gt, net.iuv2smpl.smpl, img_res)
    print('dataset length: {}'.format(len(dataset)))
    for batch in eval_batches(dataset, device, result_file, batch_size, img_res, num_workers, shuffle):
        ev.update(batch, infer(batch['img'])['para'])
    s = ev.summary()
    r = s['results']
    if opt('output_dir'):
        write_results(os.path.join(opt('output_dir'), 'results', 'keypoints_val2014_results_%s.json' % regressor), r['preds'], r['image_ids'],
                      r['center'], r['scale'])
    print_name_value(s['name_value'], regressor)
    if result_file is not None:
        n = s['num_samples']
        pose = ops.rotmat_to_angle_axis(torch.from_numpy(r['rotmat']).float().to(device).view(-1, 3, 3)).view(n, 72).double().cpu().numpy() \
            if n else np.zeros((0, 72))
        # (the reference allocates pred_joints and never fills it: zeros)
        np.savez(result_file, pred_joints=np.zeros((n, 17, 3)), pose=pose, betas=r['betas'], camera=r['camera'], preds=r['preds'],
                 image_ids=r['image_ids'])
    return dict(s['name_value'])


# ---- a synthetic stand-in for val2014 ------------------------------------------------------------------------------------------------
def write_synthetic_coco(root, n=8, seed=0):
    """A small val2014-shaped set under `root`: images as .npy, the annotation .npz of EvalDataset (imgname, center, scale) with `n`
    samples, and person_keypoints_val2014.json.  -> (annotation path, json path).  The json holds several persons per image, a crowd
    annotation, a zero-keypoint annotation, an image without samples, a non-person annotation and areas on both sides of 32^2 and
    96^2 (two of them exactly on the boundaries).  The samples are the persons with keypoints, as in the reference's COCODataset;
    a person's keypoints sit where a centred, upright body would project into its crop, so a model that predicts one scores above 0."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    # a coarse upright body in crop coordinates ([-0.5, 0.5]^2), COCO joint order
    body = np.array([[0, -.38], [.03, -.40], [-.03, -.40], [.06, -.38], [-.06, -.38], [.12, -.25], [-.12, -.25], [.17, -.10], [-.17, -.10],
                     [.18, .03], [-.18, .03], [.08, .02], [-.08, .02], [.09, .22], [-.09, .22], [.09, .42], [-.09, .42]])
    sizes = [40.0, 150.0, 24.0, 260.0, 32.0, 96.0, 70.0, 200.0]                      # person heights in pixels: small, medium, large
    images, anns, names, centers, scales = [], [], [], [], []
    ann_id, k, img = 1, 0, 0
    while k < n or img < 3:
        img += 1
        iid = 17 * img + 3
        H, W = int(rng.integers(240, 400)), int(rng.integers(240, 400))
        name = 'COCO_val2014_%012d.npy' % iid
        np.save(os.path.join(root, name), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        images.append({'id': iid, 'file_name': name[:-4] + '.jpg', 'height': H, 'width': W})
        if img == 2:
            continue                                                                # an image without annotation and without samples
        persons = 1 + img % 3
        for p in range(persons):
            if k >= n:
                break
            h = sizes[k % len(sizes)] * float(rng.uniform(0.9, 1.1)) if k >= len(sizes) else sizes[k]
            c = np.array([rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H])
            kp = np.concatenate([np.rint(c + body * h / 0.84 + rng.normal(0, 0.01 * h, (17, 2))), np.full((17, 1), 2.0)], axis=1)
            kp[rng.random(17) < 0.2, 2] = 1
            if k % 5 == 4:
                kp[int(rng.integers(0, 17))] = 0                                    # an unlabelled joint
            x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
            bw, bh = float(x1 - x0), float(y1 - y0)
            area = {4: 32.0 ** 2, 5: 96.0 ** 2}.get(k, round(0.55 * bw * bh, 4))     # (two areas exactly on the range boundaries)
            anns.append({'id': ann_id, 'image_id': iid, 'category_id': 1, 'iscrowd': 0, 'num_keypoints': int((kp[:, 2] > 0).sum()),
                         'keypoints': [float(v) for v in kp.reshape(-1)], 'area': area, 'bbox': [float(x0), float(y0), bw, bh]})
            ann_id += 1
            names.append(name)
            centers.append([x0 + bw / 2, y0 + bh / 2])
            scales.append(max(bw, bh) * 1.2 / 200.0)
            k += 1
        if img == 1:                                                                # a crowd region and a person without keypoints
            anns.append({'id': ann_id, 'image_id': iid, 'category_id': 1, 'iscrowd': 1, 'num_keypoints': 0, 'keypoints': [0.0] * 51,
                         'area': float(W * H) / 4, 'bbox': [0.0, 0.0, W / 2.0, H / 2.0]})
            anns.append({'id': ann_id + 1, 'image_id': iid, 'category_id': 1, 'iscrowd': 0, 'num_keypoints': 0, 'keypoints': [0.0] * 51,
                         'area': 900.0, 'bbox': [W - 40.0, H - 50.0, 30.0, 40.0]})
            anns.append({'id': ann_id + 2, 'image_id': iid, 'category_id': 2, 'iscrowd': 0, 'num_keypoints': 0, 'keypoints': [0.0] * 51,
                         'area': 400.0, 'bbox': [5.0, 5.0, 20.0, 20.0]})
            ann_id += 3
    # the samples are stored out of image order (the loop sorts them back: the tie rule)
    perm = rng.permutation(len(names))
    annot = os.path.join(root, 'coco_val2014_test.npz')
    np.savez(annot, imgname=np.array(names)[perm], center=np.array(centers, dtype=np.float64).reshape(-1, 2)[perm],
             scale=np.array(scales, dtype=np.float64)[perm])
    jpath = os.path.join(root, 'person_keypoints_val2014.json')
    with open(jpath, 'w') as f:
        json.dump({'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}, f)
    return annot, jpath
