"""The training input pipeline: the reference's datasets/base_dataset.py (is_train=True), datasets/mixed_dataset.py and
utils/data_loader.py, with the augmentation itself on the device (csrc/input_ops.hip).

  TrainDataset       an annotation .npz of the reference's layout + images.  An item carries the RAW uint8 image, the
                     un-augmented labels (float64, as they lie in the file) and the augmentation parameters.
  MixedDataset       the partition arithmetic of mixed_dataset.py:25-51 over TrainDatasets.
  CheckpointSampler  the epoch's permutation, `dataset_perm` and the resume rule of utils/data_loader.py.
  TrainLoader        batches read ahead by THREADS (at most 8: a process that holds a GPU context does not fork), collated by
                     `collate`: every image's footprint rectangle packed into one uint8 buffer, every float label into one block.
  to_device          the upload (pinned memory, the current stream) and the two ops: -> the `input_batch` of Trainer.prepare_batch.

Every random draw of a sample -- MixedDataset's pick, augment.augm_params -- comes from
numpy.random.default_rng([seed, epoch, position in the epoch's permutation]): a resumed run draws what the uninterrupted run would have.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import augment, constants, dp_utils, ops
from ._lib import GPU_ONLY
from .evaluate import read_array

TRAIN_SETS = {'h36m_dp': ['h36m', 'dp_coco'],
              'h36m_coco_itw': ['h36m', 'lsp-orig', 'mpii', 'lspet', 'coco', 'mpi-inf-3dhp']}
DP_KEYS_F32 = ('body_uv_ann_weights', 'body_uv_X_points', 'body_uv_Y_points', 'body_uv_Ind_points', 'body_uv_I_points',
               'body_uv_U_points', 'body_uv_V_points', 'body_uv_point_weights')
LABEL_BLOCK = (('crop_params', 10), ('xform', 6), ('rot_flip', 2), ('keypoints', 147), ('smpl_2dkps', 72), ('pose_3d', 96), ('pose', 72))


def _opt(options, name, default):
    v = getattr(options, name, None) if options is not None else None
    return default if v is None else v


def sample_rng(seed, epoch, position):
    return np.random.default_rng([int(seed), int(epoch), int(position)])


class TrainDataset(object):
    """base_dataset.py:28-113 with is_train=True: `annot` is the annotation .npz (a path or a mapping), `img_dir` holds the images
    (.npy always, .png / .jpg with PIL).  options: noise_factor 0.4, rot_factor 30, scale_factor 0.25, heatmap_size 56, img_res 224,
    dp_symmetry (a dp_utils.DensePoseSymmetry or the path of UV_symmetry_transforms.mat; default: the synthetic stand-in tables)."""

    def __init__(self, options, dataset, annot, img_dir, ignore_3d=False, use_augmentation=True):
        self.options, self.dataset, self.img_dir, self.is_train = options, dataset, img_dir, True
        self.dataset_dict = {dataset: 0}
        self.use_augmentation = use_augmentation
        d = np.load(annot, allow_pickle=True) if isinstance(annot, str) else annot
        has = lambda k: k in (d.files if hasattr(d, 'files') else d)            # noqa: E731
        self.imgname = [str(n) for n in d['imgname']]
        n = len(self.imgname)
        self.maskname = [str(m) for m in d['maskname']] if has('maskname') else None
        self.partname = [str(m) for m in d['partname']] if has('partname') else None
        self.scale, self.center = np.asarray(d['scale'], np.float64).reshape(n), np.asarray(d['center'], np.float64).reshape(n, 2)
        if has('pose') and has('shape'):
            self.pose, self.betas = np.asarray(d['pose'], np.float64), np.asarray(d['shape'], np.float64)
            self.has_smpl = np.asarray(d['has_smpl'], np.float32) if has('has_smpl') else np.ones(n, np.float32)
        else:
            self.pose, self.betas, self.has_smpl = np.zeros((n, 72)), np.zeros((n, 10)), np.zeros(n, np.float32)
        if ignore_3d:
            self.has_smpl = np.zeros(n, np.float32)
        self.has_smpl_2dkps = int(has('smpl_2dkps'))
        self.smpl_2dkps = np.asarray(d['smpl_2dkps'], np.float64) if self.has_smpl_2dkps else None
        self.dp_annot = d['dp_annot'] if has('dp_annot') else None
        self.has_dp = np.ones(n, np.float32) if self.dp_annot is not None else np.zeros(n, np.float32)
        self.has_pose_3d = int(has('S') and not ignore_3d)
        self.pose_3d = np.asarray(d['S'], np.float64) if has('S') else None
        kp_gt = np.asarray(d['part'], np.float64) if has('part') else np.zeros((n, 24, 3))
        kp_op = np.asarray(d['openpose'], np.float64) if has('openpose') else np.zeros((n, 25, 3))
        self.keypoints = np.concatenate([kp_op, kp_gt], axis=1)
        self.gender = (np.array([0 if str(g) == 'm' else 1 for g in d['gender']]).astype(np.int32) if has('gender')
                       else -np.ones(n).astype(np.int32))
        self.length = n
        self._symmetry = None

    def __len__(self):
        return self.length

    def symmetry(self):
        if self._symmetry is None:
            s = _opt(self.options, 'dp_symmetry', None)
            if s is None:
                u, v = dp_utils.synthetic_symmetry_tables()
                s = {'U_transforms': u, 'V_transforms': v}
            self._symmetry = s if callable(s) else dp_utils.DensePoseSymmetry(s)
        return self._symmetry

    def get(self, index, rng=None):
        """base_dataset.py:201-300 up to the augmentation itself, which the device does for the batch."""
        o = self.options
        flip, pn, rot, sc = augment.augm_params(1, self.use_augmentation, _opt(o, 'noise_factor', 0.4), _opt(o, 'rot_factor', 30.),
                                                _opt(o, 'scale_factor', 0.25), rng)
        flip, pn, rot, sc = int(flip[0]), pn[0], float(rot[0]), float(sc[0])
        if self.has_dp[index]:
            rot = 0.
        center, scale = self.center[index].copy(), float(sc * self.scale[index])
        path = os.path.join(self.img_dir, self.imgname[index])
        img = read_array(path)
        if img.ndim == 2:
            img = np.repeat(img[:, :, None], 3, 2)
        img = np.ascontiguousarray(img[:, :, :3], dtype=np.uint8)
        hm = int(_opt(o, 'heatmap_size', 56))
        if self.has_dp[index]:
            dp_dict = dp_utils.dp_annot_process(self.dp_annot[index], hm, int(_opt(o, 'img_res', constants.IMG_RES)), center.tolist(), scale, flip,
                                                self.symmetry() if flip else None)
        else:
            dp_dict = dp_utils.empty_dp_dict(hm)
        smpl_on = bool(self.has_smpl[index])
        return {'img_raw': img, 'dp_dict': dp_dict, 'imgname': path,
                'pose': self.pose[index].copy() if smpl_on else np.zeros(72), 'betas': (self.betas[index] if smpl_on else np.zeros(10)).astype(np.float32),
                'smpl_2dkps': self.smpl_2dkps[index].copy() if self.has_smpl_2dkps else np.zeros((24, 3)), 'has_smpl_2dkps': self.has_smpl_2dkps,
                'pose_3d': self.pose_3d[index].copy() if self.has_pose_3d else np.zeros((24, 4)), 'keypoints': self.keypoints[index].copy(),
                'has_dp': self.has_dp[index], 'has_smpl': self.has_smpl[index], 'has_pose_3d': self.has_pose_3d,
                'scale': scale, 'center': center.astype(np.float32), 'orig_shape': np.array(img.shape[:2]), 'is_flipped': flip,
                'rot_angle': np.float32(rot), '_rot': rot, '_center': center, 'pn': np.asarray(pn, np.float64), 'gender': self.gender[index], 'sample_index': index,
                'dataset_name': self.dataset, 'maskname': self.maskname[index] if self.maskname else '',
                'partname': self.partname[index] if self.partname else ''}

    __getitem__ = get


def mixed_partition(train_data, lengths):
    """mixed_dataset.py:25-45: the cumulative pick probabilities of the datasets of `train_data`, whose sizes are `lengths`."""
    lengths = [int(l) for l in lengths]
    if train_data == 'h36m_dp':
        length_itw = sum(lengths[1:])
        part = [0.5, 0.5 * lengths[1] / length_itw]
    elif train_data == 'h36m_coco_itw':
        length_itw = sum(lengths[1:-1])                                        # 30 % H36M - 60 % in the wild - 10 % MPI-INF
        part = [.3] + [.6 * l / length_itw for l in lengths[1:5]] + [0.1]
    else:
        raise ValueError('unknown train_data %r (one of %s)' % (train_data, ', '.join(TRAIN_SETS)))
    return np.array(part).cumsum()


class MixedDataset(object):
    """mixed_dataset.py: `datasets` are the TrainDatasets of options.train_data in the order of TRAIN_SETS[train_data]."""

    def __init__(self, options, datasets):
        self.options, self.train_data = options, options.train_data
        if self.train_data not in TRAIN_SETS:
            raise ValueError('unknown train_data %r (one of %s)' % (self.train_data, ', '.join(TRAIN_SETS)))
        self.dataset_list = list(TRAIN_SETS[self.train_data])
        if [ds.dataset for ds in datasets] != self.dataset_list:
            raise ValueError('MixedDataset(%r) takes the datasets %s in this order, got %s' % (self.train_data, self.dataset_list, [ds.dataset for ds in datasets]))
        self.dataset_dict = {n: i for i, n in enumerate(self.dataset_list)}
        self.datasets = list(datasets)
        self.dataset_length = {n: len(ds) for n, ds in zip(self.dataset_list, self.datasets)}
        self.length = max(len(ds) for ds in self.datasets)
        self.partition = mixed_partition(self.train_data, [len(ds) for ds in self.datasets])

    def __len__(self):
        return self.length

    def get(self, index, rng=None):
        rng = np.random.default_rng() if rng is None else rng
        p = rng.random()
        for i in range(len(self.datasets)):
            if p <= self.partition[i] or i == len(self.datasets) - 1:
                return self.datasets[i].get(index % len(self.datasets[i]), rng)

    __getitem__ = get


class CheckpointSampler(object):
    """utils/data_loader.py:6-38: the order of one epoch.  `dataset_perm` is the whole epoch's order (what a checkpoint stores),
    `perm` what is left of it: resumed from checkpoint = {'dataset_perm', 'batch_size', 'batch_idx'} the tail after batch_idx batches.
    A fresh epoch's order is numpy.random.default_rng([seed, epoch]).permutation(n).  (The reference's RandomSampler draws two
    different permutations for `dataset_perm` and `perm`, so its resumed run does not continue the interrupted one; here they are one.)"""

    def __init__(self, n, checkpoint=None, shuffle=True, seed=0, epoch=0):
        if checkpoint is not None and checkpoint.get('dataset_perm') is not None:
            self.dataset_perm = [int(i) for i in checkpoint['dataset_perm']]
            self.start = int(checkpoint['batch_size']) * int(checkpoint['batch_idx'])
        else:
            self.dataset_perm = np.random.default_rng([int(seed), int(epoch)]).permutation(n).tolist() if shuffle else list(range(n))
            self.start = 0
        self.perm = self.dataset_perm[self.start:]

    def __iter__(self):
        return iter(self.perm)

    def __len__(self):
        return len(self.perm)


# ---- collation -------------------------------------------------------------------------------------------------------------------
def crop_transforms(center, scale, rot, res):
    """(t [B,3,3], its inverse [B,3,3]) of augment.get_transform(center, scale, [res, res], rot) in float64 on the host."""
    t = augment.get_transform(torch.as_tensor(np.asarray(center, np.float64)).reshape(-1, 2), torch.as_tensor(np.asarray(scale, np.float64)).reshape(-1),
                              [res, res], torch.as_tensor(np.asarray(rot, np.float64)).reshape(-1))
    return t.numpy(), torch.linalg.inv(t).numpy()


def footprint(tinv, shape, res):
    """The rectangle (x0, y0, x1, y1; x1, y1 exclusive) of an image of `shape` = (rows, cols) that holds every bilinear tap of the
    res x res crop with inverse transform `tinv`: the integer box of the crop's four corners, grown by one pixel, clipped."""
    c = np.array([[0., 0., 1.], [res - 1., 0., 1.], [0., res - 1., 1.], [res - 1., res - 1., 1.]])
    p = c @ np.asarray(tinv, np.float64)[:2].T                                   # [4,2] (x, y)
    H, W = int(shape[0]), int(shape[1])
    if not np.isfinite(p).all():
        return 0, 0, W, H
    lo, hi = np.floor(p.min(0)) - 1, np.ceil(p.max(0)) + 2                       # taps floor(s), floor(s) + 1; one pixel of margin
    x0, y0 = int(np.clip(lo[0], 0, W)), int(np.clip(lo[1], 0, H))
    x1, y1 = int(np.clip(hi[0], 0, W)), int(np.clip(hi[1], 0, H))
    if x1 <= x0 or y1 <= y0:
        return 0, 0, 0, 0
    return x0, y0, x1, y1


def crop_params(images, center, scale, rot, flip, pn, res, whole=False):
    """The host-side arguments of ops.batch_crop for a list of uint8 [H,W,3] images: dict with 'src' (uint8 [n]), 'offsets' (int64
    [B+1]), 'geom' (int32 [2,B,2]: shapes, origins), 'params' (float64 [B,10]) and 'xform' (float64 [B,6], the forward transform).
    whole=True packs the whole images (origin 0) instead of the footprint rectangles."""
    B = len(images)
    t, tinv = crop_transforms(center, scale, rot, res)
    geom = np.zeros((2, B, 2), np.int32)
    parts, offsets = [], np.zeros(B + 1, np.int64)
    for b, im in enumerate(images):
        x0, y0, x1, y1 = (0, 0, im.shape[1], im.shape[0]) if whole else footprint(tinv[b], im.shape[:2], res)
        geom[0, b], geom[1, b] = (y1 - y0, x1 - x0), (x0, y0)
        parts.append(np.ascontiguousarray(im[y0:y1, x0:x1, :3], dtype=np.uint8).reshape(-1))
        offsets[b + 1] = offsets[b] + parts[-1].size
    src = np.zeros(int(offsets[-1]) + 16, np.uint8)                              # (never empty: a batch may see nothing of its images)
    if offsets[-1]:
        np.concatenate(parts, out=src[:int(offsets[-1])])
    params = np.concatenate([tinv[:, :2].reshape(B, 6), np.asarray(flip, np.float64).reshape(B, 1), np.asarray(pn, np.float64).reshape(B, 3)], axis=1)
    return {'src': src, 'offsets': offsets, 'geom': geom, 'params': np.ascontiguousarray(params), 'xform': np.ascontiguousarray(t[:, :2].reshape(B, 6))}


def collate(items, res=constants.IMG_RES):
    """A list of TrainDataset items -> one host batch: 'src' / 'offsets' / 'geom' (crop_params: footprint rectangles only), 'labels'
    (ONE float64 block, the sections of LABEL_BLOCK one after the other, each [B, n]), 'flags' (float32 [4,B]: has_smpl, has_pose_3d,
    has_dp, has_iuv_dataset), 'betas' (float32 [B,10]), 'dp_f32' (the eight float32 DensePose blobs, one after the other) and
    'dp_labels' (int32 [B,S*S]), and the host-side values of the reference's batch."""
    B = len(items)
    col = lambda k, dt=np.float64: np.stack([np.asarray(it[k], dt) for it in items])        # noqa: E731
    rot, flip = col('_rot'), col('is_flipped')                  # (the unrounded values: 'rot_angle' / 'center' are float32, as the reference's)
    cp = crop_params([it['img_raw'] for it in items], col('_center'), col('scale'), rot, flip, col('pn'), res)
    sections = {'crop_params': cp['params'], 'xform': cp['xform'], 'rot_flip': np.stack([rot, flip], 1), 'keypoints': col('keypoints'),
                'smpl_2dkps': col('smpl_2dkps'), 'pose_3d': col('pose_3d'), 'pose': col('pose')}
    labels = np.concatenate([sections[k].reshape(B, n).reshape(-1) for k, n in LABEL_BLOCK])
    names = [it['dataset_name'] for it in items]
    flags = np.stack([col('has_smpl', np.float32), col('has_pose_3d', np.float32), col('has_dp', np.float32),
                      np.array([n != 'dp_coco' for n in names], np.float32)])
    dp = [it['dp_dict'] for it in items]
    return {'src': cp['src'], 'offsets': cp['offsets'], 'geom': cp['geom'], 'labels': labels, 'flags': flags, 'betas': col('betas', np.float32),
            'dp_f32': np.concatenate([np.stack([np.asarray(d[k], np.float32) for d in dp]).reshape(-1) for k in DP_KEYS_F32]),
            'dp_sizes': [int(np.asarray(dp[0][k]).size) for k in DP_KEYS_F32],
            'dp_labels': np.stack([np.asarray(d['body_uv_ann_labels'], np.int32) for d in dp]), 'dp_active': bool(flags[2].any()),
            'batch_size': B, 'res': int(res), 'dataset_name': names, 'imgname': [it['imgname'] for it in items],
            'sample_index': col('sample_index', np.int64), 'rot_angle': rot.astype(np.float32), 'is_flipped': flip.astype(np.int64),
            'scale': col('scale', np.float32), 'center': col('center', np.float32), 'orig_shape': col('orig_shape', np.int64),
            'gender': col('gender', np.int32), 'pn': col('pn')}


_PINNED = {}


def _upload(a, device):
    """A host array -> device tensor on the current stream, through pinned memory (a ring of staging buffers per dtype, each reused only
    after the copy that read it has finished; eight deep, so that the wait is for a copy of an earlier batch)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if device.type != 'cuda':
        raise RuntimeError(GPU_ONLY % ('upload device', device))
    slot = _PINNED.setdefault((t.dtype, device.index), {'bufs': [None] * 8, 'events': [None] * 8, 'turn': 0})
    k = slot['turn']
    slot['turn'] = (k + 1) % 8
    if slot['events'][k] is not None:
        slot['events'][k].synchronize()
    n = t.numel()
    if slot['bufs'][k] is None or slot['bufs'][k].numel() < n:
        slot['bufs'][k] = torch.empty(max(n, 1) * 5 // 4 + 64, dtype=t.dtype).pin_memory()
    stage = slot['bufs'][k][:n]
    stage.copy_(t.reshape(-1))
    out = stage.to(device, non_blocking=True).view(t.shape)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    slot['events'][k] = ev
    return out


def to_device(batch, device, res=None):
    """Uploads a collated batch (five copies: pixels, offsets, geometry, the label block, the flags; plus betas and the two DensePose
    blocks) and runs ops.batch_crop and ops.label_augment on the current stream -> exactly the `input_batch` Trainer.prepare_batch takes,
    plus dataset_name, sample_index, rot_angle, is_flipped (what FitsDict is asked with) and has_iuv_dataset."""
    device = torch.device(device)
    B, res = batch['batch_size'], int(res or batch['res'])
    src, offsets, geom = _upload(batch['src'], device), _upload(batch['offsets'], device), _upload(batch['geom'], device)
    lab, flags = _upload(batch['labels'], device), _upload(batch['flags'], device)
    sec, at = {}, 0
    for k, n in LABEL_BLOCK:
        sec[k] = lab[at:at + B * n].view(B, n)
        at += B * n
    img = ops.batch_crop(src, offsets, geom[0], geom[1], sec['crop_params'], res)
    aug = ops.label_augment(sec['rot_flip'], sec['xform'], sec['keypoints'].view(B, 49, 3), sec['smpl_2dkps'].view(B, 24, 3),
                            sec['pose_3d'].view(B, 24, 4), sec['pose'], res=res)
    dpf, dp, at = _upload(batch['dp_f32'], device), {}, 0
    for k, n in zip(DP_KEYS_F32, batch['dp_sizes']):
        dp[k] = dpf[at:at + B * n].view(B, n)
        at += B * n
    dp['body_uv_ann_labels'] = _upload(batch['dp_labels'], device)
    dp['dp_active'] = bool(batch['dp_active'])
    return {'img': img, 'keypoints': aug['keypoints'], 'smpl_2dkps': aug['smpl_2dkps'], 'pose_3d': aug['pose_3d'], 'pose': aug['pose'],
            'betas': _upload(batch['betas'], device), 'has_smpl': flags[0], 'has_pose_3d': flags[1], 'has_dp': flags[2], 'has_iuv_dataset': flags[3],
            'dp_dict': dp, 'dataset_name': list(batch['dataset_name']), 'sample_index': _upload(batch['sample_index'], device),
            'rot_angle': sec['rot_flip'][:, 0].float(), 'is_flipped': sec['rot_flip'][:, 1] != 0, 'imgname': list(batch['imgname']),
            'scale': batch['scale'], 'center': batch['center'], 'orig_shape': batch['orig_shape'], 'gender': batch['gender'],
            'uploaded_bytes': int(sum(batch[k].nbytes for k in ('src', 'offsets', 'geom', 'labels', 'flags', 'betas', 'dp_f32', 'dp_labels', 'sample_index')))}


class TrainLoader(object):
    """utils/data_loader.py CheckpointDataLoader (drop_last=True): collated host batches of one epoch in the sampler's order."""

    def __init__(self, dataset, checkpoint=None, batch_size=1, shuffle=True, num_workers=0, seed=0, epoch=0, res=constants.IMG_RES):
        self.dataset, self.batch_size, self.seed, self.epoch, self.res = dataset, int(batch_size), int(seed), int(epoch), int(res)
        self.sampler = CheckpointSampler(len(dataset), checkpoint, shuffle, seed, epoch)
        self.checkpoint_batch_idx = int(checkpoint['batch_idx']) if checkpoint is not None and checkpoint.get('dataset_perm') is not None else 0
        self.workers = max(0, min(int(num_workers), 8))

    def __len__(self):
        return len(self.sampler) // self.batch_size

    def load(self, k):
        """Batch k of what is left of the epoch."""
        bs, s = self.batch_size, self.sampler
        items = [self.dataset.get(int(s.perm[k * bs + j]), sample_rng(self.seed, self.epoch, s.start + k * bs + j)) for j in range(bs)]
        return collate(items, self.res)

    def __iter__(self):
        n, w = len(self), self.workers
        if w == 0:
            for k in range(n):
                yield self.load(k)
            return
        with ThreadPoolExecutor(max_workers=w) as ex:
            pending = [ex.submit(self.load, k) for k in range(min(w, n))]
            for k in range(n):
                if k + w < n:
                    pending.append(ex.submit(self.load, k + w))
                yield pending[k].result()
                pending[k] = None


# ---- a synthetic training set -------------------------------------------------------------------------------------------------------
def write_synthetic_train_set(root, n_h36m=6, n_dp=6, seed=0):
    """A small 'h36m_dp' training set of the reference's layout under `root`: -> {'annot': {name: .npz}, 'img_dir': {name: dir},
    'final_fits_dir', 'static_fits_dir'}.  Images (.npy) of different non-square sizes, crops that overhang the image; the 'dp_coco'
    part has dp_annot (decoded label images, see dp_utils.dp_annot_process) and smpl_2dkps but no SMPL parameters."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    fits, static = os.path.join(root, 'final_fits'), os.path.join(root, 'static_fits')
    os.makedirs(fits, exist_ok=True)
    os.makedirs(static, exist_ok=True)
    out = {'annot': {}, 'img_dir': {}, 'final_fits_dir': fits, 'static_fits_dir': static}
    for name, n in (('h36m', n_h36m), ('dp_coco', n_dp)):
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        names, center, scale, shapes = [], np.zeros((n, 2)), np.zeros(n), []
        for i in range(n):
            H, W = int(rng.integers(150, 330)), int(rng.integers(150, 330))
            np.save(os.path.join(d, 'im%04d.npy' % i), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            names.append('im%04d.npy' % i)
            shapes.append((H, W))
            center[i] = (W / 2 + rng.uniform(-0.3, 0.3) * W, H / 2 + rng.uniform(-0.3, 0.3) * H)
            scale[i] = rng.uniform(0.5, 1.6) * max(H, W) / 200.
        box = lambda i: (center[i, 0] - 100 * scale[i], center[i, 1] - 100 * scale[i], 200 * scale[i])       # noqa: E731
        kp = np.zeros((n, 24, 3))
        for i in range(n):
            x, y, s = box(i)
            kp[i, :, 0], kp[i, :, 1], kp[i, :, 2] = x + rng.uniform(0.1, 0.9, 24) * s, y + rng.uniform(0.1, 0.9, 24) * s, (rng.random(24) > 0.2)
        arrs = {'imgname': np.array(names), 'center': center, 'scale': scale, 'part': kp}
        pose, betas = rng.normal(0, 0.2, (n, 72)), np.clip(rng.normal(0, 1, (n, 10)), -3, 3)
        if name == 'h36m':
            S = np.concatenate([rng.normal(0, 0.3, (n, 24, 3)), np.ones((n, 24, 1))], axis=2)
            S[:, :, :3] -= S[:, [14], :3]
            arrs.update(pose=pose, shape=betas, S=S, gender=np.array(['m' if i % 2 == 0 else 'f' for i in range(n)]))
            np.save(os.path.join(fits, 'h36m.npy'), np.concatenate([pose, betas], 1).astype(np.float32))
        else:
            sk = kp.copy()
            sk[:, :, 2] = rng.random((n, 24)) > 0.25
            ann = np.empty(n, dtype=object)
            for i in range(n):
                x, y, s = box(i)
                npts = int(rng.integers(40, 150))
                yy, xx = np.mgrid[0:256, 0:256]
                lab = ((xx * 5 // 256 + yy * 3 // 256) % 15).astype(np.uint8)
                ann[i] = {'bbox': [float(x + 0.1 * s), float(y + 0.1 * s), float(0.8 * s), float(0.8 * s)], 'dp_Ilabel': lab,
                          'dp_I': rng.integers(1, 25, npts).astype(np.float64).tolist(), 'dp_U': rng.random(npts).tolist(),
                          'dp_V': rng.random(npts).tolist(), 'dp_x': rng.uniform(0, 255, npts).tolist(), 'dp_y': rng.uniform(0, 255, npts).tolist()}
            arrs.update(smpl_2dkps=sk, dp_annot=ann)
            np.savez(os.path.join(fits, 'dp_coco.npz'), pose=rng.normal(0, 0.2, (n, 72)).astype(np.float32),
                     betas=np.clip(rng.normal(0, 1, (n, 10)), -3, 3).astype(np.float32), valid_fit=(rng.random(n) > 0.3))
        path = os.path.join(root, '%s_train.npz' % name)
        np.savez(path, **arrs)
        out['annot'][name], out['img_dir'][name] = path, d
    return out


def synthetic_mixed_dataset(options, root, n_h36m=6, n_dp=6, seed=0):
    """write_synthetic_train_set + the MixedDataset over it ('h36m_dp') -> (dataset, the paths dict)."""
    paths = write_synthetic_train_set(root, n_h36m, n_dp, seed)
    sets = [TrainDataset(options, n, paths['annot'][n], paths['img_dir'][n], ignore_3d=bool(_opt(options, 'ignore_3d', False)))
            for n in TRAIN_SETS['h36m_dp']]
    return MixedDataset(options, sets), paths
