"""Host side of the training input pipeline (danet_densepose2smpl_amd/datasets.py, fits_dict.py): dataset fields and fall-backs,
the MixedDataset partition, the resumable order, the fits file rules and the footprint rectangle.  No GPU."""
import os

import numpy as np
import pytest
import torch

from danet_densepose2smpl_amd import augment, datasets
from danet_densepose2smpl_amd.fits_dict import FitsDict

DP_SHAPES = {'body_uv_ann_labels': ((3136,), np.int32), 'body_uv_ann_weights': ((3136,), np.float32), 'body_uv_X_points': ((196,), np.float32),
             'body_uv_Y_points': ((196,), np.float32), 'body_uv_Ind_points': ((196,), np.float32), 'body_uv_I_points': ((196,), np.float32),
             'body_uv_U_points': ((4900,), np.float32), 'body_uv_V_points': ((4900,), np.float32), 'body_uv_point_weights': ((4900,), np.float32)}
# base_dataset.py:201-300: 'img' is the raw image here (the crop is the device's), 'pn' and the unrounded '_rot' / '_center' travel with it
ITEM_KEYS = {'img_raw', 'dp_dict', 'pose', 'betas', 'imgname', 'smpl_2dkps', 'has_smpl_2dkps', 'pose_3d', 'keypoints', 'has_dp', 'has_smpl',
             'has_pose_3d', 'scale', 'center', 'orig_shape', 'is_flipped', 'rot_angle', 'gender', 'sample_index', 'dataset_name', 'maskname',
             'partname', 'pn', '_rot', '_center'}


def _write(tmp_path, n=5, drop=(), seed=0):
    rng = np.random.default_rng(seed)
    names = []
    for i in range(n):
        np.save(str(tmp_path / ('a%d.npy' % i)), rng.integers(0, 256, (20 + i, 31 - i, 3), dtype=np.uint8))
        names.append('a%d.npy' % i)
    arrs = {'imgname': np.array(names), 'center': rng.uniform(5, 20, (n, 2)), 'scale': rng.uniform(0.05, 0.2, n), 'pose': rng.normal(0, 0.2, (n, 72)),
            'shape': rng.normal(0, 1, (n, 10)), 'S': rng.normal(0, 1, (n, 24, 4)), 'part': rng.uniform(0, 30, (n, 24, 3)),
            'openpose': rng.uniform(0, 30, (n, 25, 3)), 'gender': np.array(['m', 'f'] * n)[:n]}
    for k in drop:
        del arrs[k]
    path = str(tmp_path / 'annot.npz')
    np.savez(path, **arrs)
    return path, arrs


def test_dataset_item_keys_dtypes_shapes_and_fallbacks(tmp_path):
    path, arrs = _write(tmp_path)
    ds = datasets.TrainDataset(None, 'h36m', path, str(tmp_path))
    assert len(ds) == 5 and ds.dataset_dict == {'h36m': 0}
    it = ds.get(3, np.random.default_rng(1))
    assert set(it) == ITEM_KEYS
    assert it['img_raw'].dtype == np.uint8 and it['img_raw'].shape == (23, 28, 3) and tuple(it['orig_shape']) == (23, 28)
    assert it['pose'].shape == (72,) and it['betas'].shape == (10,) and it['betas'].dtype == np.float32
    assert it['keypoints'].shape == (49, 3) and it['pose_3d'].shape == (24, 4) and it['smpl_2dkps'].shape == (24, 3)
    np.testing.assert_array_equal(it['keypoints'], np.concatenate([arrs['openpose'][3], arrs['part'][3]]))        # un-augmented
    np.testing.assert_array_equal(it['pose'], arrs['pose'][3])
    np.testing.assert_array_equal(it['pose_3d'], arrs['S'][3])
    assert (it['smpl_2dkps'] == 0).all() and it['has_smpl_2dkps'] == 0
    assert it['has_smpl'] == 1 and it['has_pose_3d'] == 1 and it['has_dp'] == 0 and it['gender'] == 1 and it['sample_index'] == 3
    assert it['center'].dtype == np.float32 and isinstance(it['scale'], float) and it['rot_angle'].dtype == np.float32
    assert it['dataset_name'] == 'h36m' and it['maskname'] == '' and it['partname'] == '' and it['imgname'].endswith('a3.npy')
    for k, (shp, dt) in DP_SHAPES.items():
        assert it['dp_dict'][k].shape == shp and it['dp_dict'][k].dtype == dt and not it['dp_dict'][k].any()
    # the augmentation parameters are augment.augm_params' draw from the generator the item was asked with
    flip, pn, rot, sc = augment.augm_params(1, True, rng=np.random.default_rng(1))
    assert it['is_flipped'] == flip[0] and it['_rot'] == rot[0] and it['scale'] == float(sc[0] * arrs['scale'][3])
    np.testing.assert_array_equal(it['pn'], pn[0])
    # fall-backs of base_dataset.py:59-111
    (tmp_path / 'b').mkdir()
    p2, _ = _write(tmp_path, drop=('pose', 'S', 'openpose', 'gender'))
    it = datasets.TrainDataset(None, 'lspet', p2, str(tmp_path)).get(0, np.random.default_rng(2))
    assert it['has_smpl'] == 0 and it['has_pose_3d'] == 0 and not it['pose'].any() and not it['betas'].any() and not it['pose_3d'].any()
    assert not it['keypoints'][:25].any() and it['keypoints'][25:].any() and it['gender'] == -1
    p3, _ = _write(tmp_path)
    it = datasets.TrainDataset(None, 'h36m', p3, str(tmp_path), ignore_3d=True).get(0, np.random.default_rng(2))
    assert it['has_smpl'] == 0 and it['has_pose_3d'] == 0 and not it['pose'].any() and not it['pose_3d'].any()
    it = datasets.TrainDataset(None, 'h36m', p3, str(tmp_path), use_augmentation=False).get(0)
    assert it['is_flipped'] == 0 and it['_rot'] == 0 and (it['pn'] == 1).all()


def test_dp_samples_have_no_rotation_and_real_blobs(tmp_path):
    paths = datasets.write_synthetic_train_set(str(tmp_path), 2, 4, seed=3)
    ds = datasets.TrainDataset(None, 'dp_coco', paths['annot']['dp_coco'], paths['img_dir']['dp_coco'])
    flips = set()
    for i in range(4):
        it = ds.get(i, np.random.default_rng(i))
        flips.add(it['is_flipped'])
        assert it['has_dp'] == 1 and it['rot_angle'] == 0 and it['has_smpl'] == 0 and it['has_smpl_2dkps'] == 1
        for k, (shp, dt) in DP_SHAPES.items():
            assert it['dp_dict'][k].shape == shp and it['dp_dict'][k].dtype == dt
        assert it['dp_dict']['body_uv_ann_weights'].all()
    assert flips == {0, 1}


class _Len(object):
    def __init__(self, name, n):
        self.dataset, self.n = name, n

    def __len__(self):
        return self.n

    def get(self, i, rng=None):
        return (self.dataset, i)


def test_mixed_partition_is_the_reference_formula():
    class O(object):
        train_data = 'h36m_coco_itw'
    lens = [312188, 1000, 14810, 9428, 28344, 96507]
    md = datasets.MixedDataset(O, [_Len(n, l) for n, l in zip(datasets.TRAIN_SETS['h36m_coco_itw'], lens)])
    itw = sum(lens[1:-1])
    want = np.array([.3, .6 * lens[1] / itw, .6 * lens[2] / itw, .6 * lens[3] / itw, .6 * lens[4] / itw, 0.1]).cumsum()
    np.testing.assert_array_equal(md.partition, want)
    assert len(md) == max(lens) and md.dataset_dict['coco'] == 4 and md.dataset_length['mpii'] == 14810
    O.train_data = 'h36m_dp'
    md = datasets.MixedDataset(O, [_Len('h36m', 7), _Len('dp_coco', 3)])
    np.testing.assert_array_equal(md.partition, np.array([0.5, 0.5 * 3 / 3]).cumsum())
    rng = np.random.default_rng(5)
    p = np.random.default_rng(5).random()
    assert md.get(5, rng) == (('h36m', 5) if p <= 0.5 else ('dp_coco', 5 % 3))
    with pytest.raises(ValueError):
        datasets.MixedDataset(O, [_Len('dp_coco', 3), _Len('h36m', 7)])


def test_resumed_sampler_yields_the_tail_and_the_same_parameters(tmp_path):
    class O(object):
        train_data = 'h36m_dp'
    ds, _ = datasets.synthetic_mixed_dataset(O, str(tmp_path), 7, 5, seed=1)
    full = datasets.TrainLoader(ds, batch_size=2, seed=4, epoch=2)
    assert sorted(full.sampler.dataset_perm) == list(range(7)) and len(full) == 3 and full.checkpoint_batch_idx == 0
    assert full.sampler.dataset_perm != datasets.TrainLoader(ds, batch_size=2, seed=4, epoch=3).sampler.dataset_perm
    ck = {'dataset_perm': full.sampler.dataset_perm, 'batch_size': 2, 'batch_idx': 1}
    tail = datasets.TrainLoader(ds, checkpoint=ck, batch_size=2, seed=4, epoch=2, num_workers=2)
    assert tail.sampler.perm == full.sampler.dataset_perm[2:] and tail.checkpoint_batch_idx == 1 and len(tail) == 2
    a, b = list(full)[1:], list(tail)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x['dataset_name'] == y['dataset_name'] and x['imgname'] == y['imgname']
        for k in ('src', 'offsets', 'geom', 'labels', 'flags', 'betas', 'dp_f32', 'dp_labels', 'sample_index', 'pn'):
            np.testing.assert_array_equal(x[k], y[k])
    # sequential order
    assert datasets.CheckpointSampler(4, shuffle=False).perm == [0, 1, 2, 3]


def test_fits_dict_file_rules(tmp_path):
    final, static = tmp_path / 'final', tmp_path / 'static'
    final.mkdir()
    static.mkdir()
    rng = np.random.default_rng(0)
    h = rng.normal(size=(4, 82)).astype(np.float32)
    np.save(str(final / 'h36m.npy'), h)
    pose, betas, valid = rng.normal(size=(3, 72)).astype(np.float32), rng.normal(size=(3, 10)).astype(np.float32), np.array([1, 0, 1], bool)
    np.savez(str(final / 'coco.npz'), pose=pose, betas=betas, valid_fit=valid)
    st = rng.normal(size=(5, 82)).astype(np.float32)
    np.save(str(static / 'mpii_fits.npy'), st)
    t, v = FitsDict.read('h36m', str(final), str(static))
    np.testing.assert_array_equal(t, h)
    assert v.dtype == np.uint8 and v.all()
    t, v = FitsDict.read('coco', str(final), str(static))
    np.testing.assert_array_equal(t, np.concatenate([pose, betas], 1))
    np.testing.assert_array_equal(v, valid.astype(np.uint8))
    t, v = FitsDict.read('mpii', str(final), str(static))                       # no final fits: the static ones
    np.testing.assert_array_equal(t, st)
    assert not v.any()
    with pytest.raises(IOError):
        FitsDict.read('lspet', str(final), str(static))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        FitsDict(None, None, str(final), str(static), 'cpu')


@pytest.mark.gpu
def test_fits_dict_round_trips_through_save(tmp_path):
    class O(object):
        train_data, checkpoint_dir = 'h36m_dp', str(tmp_path / 'ck')
    ds, paths = datasets.synthetic_mixed_dataset(O, str(tmp_path), 3, 4, seed=2)
    fd = FitsDict(O, ds, paths['final_fits_dir'], paths['static_fits_dir'], 'cuda')
    fd.save()
    for name in ('h36m', 'dp_coco'):
        want, _ = FitsDict.read(name, paths['final_fits_dir'], paths['static_fits_dir'])
        np.testing.assert_array_equal(np.load(os.path.join(O.checkpoint_dir, name + '_fits.npy')), want)
    again = FitsDict(O, ds, str(tmp_path / 'nothing'), O.checkpoint_dir, 'cuda')            # what was saved reads as static fits
    assert torch.equal(again.table, fd.table)


def _taps(tinv, res):
    v, u = np.mgrid[0:res, 0:res].astype(np.float64)
    sx = tinv[0, 0] * u + tinv[0, 1] * v + tinv[0, 2]
    sy = tinv[1, 0] * u + tinv[1, 1] * v + tinv[1, 2]
    return np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)


@pytest.mark.parametrize('res', [16, 32])
def test_footprint_contains_every_tap(res):
    """Brute force over the shapes of tests/test_gpu_input_ops.py: every tap of every output pixel that lies inside the image lies
    inside the rectangle."""
    rng = np.random.default_rng(res)
    n_inside = 0
    for (H, W) in ((1, 1), (7, 5), (33, 64), (64, 33), (50, 50)):
        for rot in (0., 30., -47.5, 90., 180.):
            for _ in range(4):
                center = np.array([rng.uniform(-0.2, 1.2) * W, rng.uniform(-0.2, 1.2) * H])
                scale = rng.uniform(0.3, 1.5) * max(H, W) / 200.
                _, tinv = datasets.crop_transforms(center[None], [scale], [rot], res)
                x0, y0, x1, y1 = datasets.footprint(tinv[0], (H, W), res)
                assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
                fx, fy = _taps(tinv[0], res)
                for dx in (0, 1):
                    for dy in (0, 1):
                        x, y = fx + dx, fy + dy
                        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                        n_inside += int(inside.sum())
                        assert ((x[inside] >= x0) & (x[inside] < x1) & (y[inside] >= y0) & (y[inside] < y1)).all(), (H, W, rot, center, scale)
    assert n_inside > 1000
    # a crop that misses its image: nothing is packed
    _, tinv = datasets.crop_transforms(np.array([[500., 500.]]), [0.1], [30.], res)
    assert datasets.footprint(tinv[0], (50, 50), res) == (0, 0, 0, 0)
    # ... and the rectangle is proportional to the crop, not to the photograph
    _, tinv = datasets.crop_transforms(np.array([[500., 400.]]), [0.5], [0.], res)
    x0, y0, x1, y1 = datasets.footprint(tinv[0], (1000, 1000), res)
    assert (x1 - x0) <= 104 and (y1 - y0) <= 104
