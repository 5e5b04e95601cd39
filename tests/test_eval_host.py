"""Host side of the evaluation pipeline (danet_densepose2smpl_amd/evaluate.py), no GPU: the uncrop rule against golden g25 (the
reference's utils.imutils.uncrop on PIL), the counting oracle against counts taken from the golden uncropped images, the dataset
reader, the dataset-name dispatch, the no-CPU-path rule and the ABI."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_oracle as eo    # noqa: E402


def _g25():
    g = golden('g25_eval')
    off = g['offsets']
    N = len(off) - 1
    shp = g['orig_shape']
    cut = lambda k: [g[k][off[i]:off[i + 1]].reshape(shp[i]) for i in range(N)]
    return g, N, {k: cut(k) for k in ('un_mask', 'un_parts', 'gt_mask', 'gt_parts')}


def test_g25_has_the_cases_the_rule_is_pinned_on():
    g, N, im = _g25()
    assert N >= 8
    r, shp, crop = g['rects'], g['orig_shape'], g['crop_shape']
    clipped = [(r[:, 2] == 0) & (r[:, 3] - r[:, 2] < crop[:, 1]), (r[:, 3] == shp[:, 1]) & (r[:, 3] - r[:, 2] < crop[:, 1]),
               (r[:, 0] == 0) & (r[:, 1] - r[:, 0] < crop[:, 0]), (r[:, 1] == shp[:, 0]) & (r[:, 1] - r[:, 0] < crop[:, 0])]
    assert all(c.any() for c in clipped)                              # each of the four borders is overhung somewhere
    assert (crop.max(1) > 224).any() and (crop.max(1) < 224).any() and (shp[:, 0] != shp[:, 1]).any()
    assert all(set(np.unique(p)) == set(range(7)) for p in g['parts'])
    assert all((p == 255).any() for p in im['gt_parts'])


def test_index_tables_and_paste_rectangles_reproduce_uncrop_exactly():
    from danet_densepose2smpl_amd import evaluate
    g, N, im = _g25()
    geo = evaluate.uncrop_geometry(g['center'], g['scale'], g['orig_shape'], 224)
    for i in range(N):
        rect, rows, cols = geo[i]
        assert tuple(rect) == tuple(int(v) for v in g['rects'][i])
        assert len(rows) == rect[1] - rect[0] and len(cols) == rect[3] - rect[2]
        assert rows.min() >= 0 and rows.max() < 224 and cols.min() >= 0 and cols.max() < 224
        np.testing.assert_array_equal(eo.uncrop_lookup(g['mask'][i] > 0, geo[i], g['orig_shape'][i]), im['un_mask'][i] > 0)
        np.testing.assert_array_equal(eo.uncrop_lookup(g['parts'][i], geo[i], g['orig_shape'][i]), im['un_parts'][i])
    # one sample at a time gives the same geometry as the batch
    one = evaluate.uncrop_geometry(g['center'][3], g['scale'][3], g['orig_shape'][3], 224)[0]
    assert one[0] == geo[3][0] and (one[1] == geo[3][1]).all() and (one[2] == geo[3][2]).all()


def test_nearest_table_is_the_running_sum():
    from danet_densepose2smpl_amd import evaluate
    for n in (20, 120, 180, 223, 224, 225, 260, 400, 699):
        a = 224 / n
        x, want = 0.5 * a, []
        for _ in range(n):
            want.append(int(x))
            x += a
        np.testing.assert_array_equal(evaluate.nearest_table(224, n), want)
    closed = lambda n: np.floor((2 * np.arange(n) + 1) * 224 / (2 * n)).astype(int)
    assert any((closed(n) != evaluate.nearest_table(224, n)).any() for n in range(20, 700))      # the closed form is another rule
    with pytest.raises(ValueError):
        evaluate.nearest_table(224, 0)


def test_oracle_counts_equal_counts_on_the_golden_uncropped_images():
    from danet_densepose2smpl_amd import evaluate
    g, N, im = _g25()
    want = np.zeros(eo.SEG_COUNTERS, np.int64)
    for i in range(N):
        want += eo.seg_counts(im['un_mask'][i] > 0, im['gt_mask'][i] > 0, im['un_parts'][i], im['gt_parts'][i])
    got = eo.score_batch(g['mask'].astype(np.float32), g['parts'].astype(np.int64), im['gt_mask'], im['gt_parts'], g['center'], g['scale'],
                         evaluate.uncrop_geometry)
    np.testing.assert_array_equal(got, want)
    S = eo.SEG
    px = int((g['orig_shape'][:, 0] * g['orig_shape'][:, 1]).sum())
    assert got[S['pixel_count']] == px and got[S['parts_pixel_count']] == px
    # every mask pixel falls in exactly one cell of each class's table; tp + fn of a class = its label pixels
    assert got[S['tp']] + got[S['fp']] + got[S['fn']] + got[S['tp'] + 1] == px
    lab = np.concatenate([p.reshape(-1) for p in im['gt_parts']])
    for c in range(7):
        assert got[S['parts_tp'] + c] + got[S['parts_fn'] + c] == (lab == c).sum()
    assert (got[S['parts_tp']:S['parts_tp'] + 7] > 0).all() and got[S['parts_accuracy']] > 0
    # pack_labels lays the same batch out for the kernel
    pk = evaluate.pack_labels(im['gt_mask'], im['gt_parts'], g['center'], g['scale'], 224)
    np.testing.assert_array_equal(pk['offsets'].numpy(), g['offsets'])
    np.testing.assert_array_equal(pk['gt_parts'].numpy(), g['gt_parts'])
    np.testing.assert_array_equal(pk['rects'].numpy()[:, :4], g['rects'])
    r = pk['rects'].numpy()
    assert pk['tables'].numel() == (r[:, 1] - r[:, 0] + r[:, 3] - r[:, 2]).sum() and pk['max_pixels'] == int((g['orig_shape'][:, 0] * g['orig_shape'][:, 1]).max())


def test_eval_dataset_round_trip(tmp_path):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), 'lsp', n=5, seed=3)
    d = np.load(path)
    assert set(('imgname', 'center', 'scale', 'pose', 'shape', 'S', 'gender', 'maskname', 'partname')) <= set(d.files)
    ds = evaluate.EvalDataset(path, str(tmp_path), 'lsp')
    assert len(ds) == 5
    it = ds[2]
    raw = np.load(os.path.join(str(tmp_path), str(d['imgname'][2])))
    np.testing.assert_array_equal(it['img_raw'], raw)
    np.testing.assert_array_equal(it['orig_shape'], raw.shape[:2])
    np.testing.assert_array_equal(it['gt_parts'], np.load(os.path.join(str(tmp_path), str(d['partname'][2]))))
    assert it['gt_mask'].dtype == np.uint8 and it['gt_mask'].shape == raw.shape[:2] and (it['gt_parts'] == 255).any()
    np.testing.assert_allclose(it['pose'], d['pose'][2].astype(np.float32))
    np.testing.assert_allclose(it['betas'], d['shape'][2].astype(np.float32))
    assert it['gender'] == 0 and ds[1]['gender'] == 1 and it['pose_3d'].shape == (24, 4) and it['scale'] == float(d['scale'][2])
    batches = list(evaluate.iterate_batches(ds, 2, num_workers=2))
    assert [len(b['imgname']) for b in batches] == [2, 2, 1]
    b0 = batches[0]
    assert b0['img_raw'].shape[0] == 2 and b0['img_raw'].shape[1:3] == tuple(np.maximum(ds[0]['orig_shape'], ds[1]['orig_shape']))
    np.testing.assert_array_equal(b0['img_raw'][1, :ds[1]['orig_shape'][0], :ds[1]['orig_shape'][1]], ds[1]['img_raw'])
    assert len(b0['gt_mask']) == 2 and b0['sample_index'].tolist() == [0, 1]
    same = list(evaluate.iterate_batches(ds, 2, num_workers=0))
    assert all((a['img_raw'] == b['img_raw']).all() for a, b in zip(batches, same))
    # a pose dataset has no label images and names that carry the action
    p2 = evaluate.write_synthetic_dataset(str(tmp_path / 'h'), 'h36m-p2', n=4, seed=1)
    dp = evaluate.EvalDataset(p2, str(tmp_path / 'h'), 'h36m-p2')
    assert 'gt_mask' not in dp[0] and evaluate.h36m_action(dp[1]['imgname']) == 'Eating'


def test_dataset_name_dispatch():
    from danet_densepose2smpl_amd import evaluate, constants
    for name in ('h36m-p1', 'h36m-p2'):
        p = evaluate.dataset_plan(name)
        assert p['eval_pose'] and not p['eval_masks'] and not p['eval_parts'] and p['gt_source'] == 'joints'
        assert p['joint_mapper_h36m'] == constants.H36M_TO_J14 and p['joint_mapper_gt'] == constants.J24_TO_J14
        assert p['per_action'] == (name == 'h36m-p2')
    p = evaluate.dataset_plan('3dpw')
    assert p['eval_pose'] and p['gt_source'] == 'vertices' and len(p['joint_mapper_h36m']) == 14
    p = evaluate.dataset_plan('mpi-inf-3dhp')
    assert p['joint_mapper_h36m'] == constants.H36M_TO_J17 and p['joint_mapper_gt'] == constants.J24_TO_J17 and p['gt_source'] == 'joints'
    p = evaluate.dataset_plan('lsp')
    assert not p['eval_pose'] and p['eval_masks'] and p['eval_parts'] and p['gt_source'] is None
    with pytest.raises(ValueError, match='unknown evaluation dataset'):
        evaluate.dataset_plan('coco')
    assert evaluate.h36m_action('/data/h36m/S9_Directions_1.54138969_000001.jpg') == 'Directions'


def test_axis_angle_oracle_properties():
    rng = np.random.default_rng(0)
    ax = rng.normal(size=(200, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    aa = ax * rng.uniform(0, np.pi, (200, 1))
    back = eo.rotmat_to_angle_axis(eo.rodrigues(aa))
    np.testing.assert_allclose(back, aa, atol=1e-9)
    np.testing.assert_array_equal(eo.rotmat_to_angle_axis(np.eye(3)), np.zeros((1, 3)))
    for k in range(3):
        R = -np.eye(3)
        R[k, k] = 1
        np.testing.assert_allclose(eo.rotmat_to_angle_axis(R)[0], np.pi * np.eye(3)[k], atol=1e-15)


def test_ops_and_run_evaluation_refuse_cpu_tensors():
    from danet_densepose2smpl_amd import evaluate, geometry, ops
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        geometry.rotmat_to_angle_axis(torch.eye(3)[None])
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.pose_eval(torch.zeros(1, 30, 3), torch.zeros(17, 30), list(range(14)), gt_keypoints_3d=torch.zeros(1, 14, 3))
    z = torch.zeros(1, 224, 224)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.seg_confusion(z, z.long(), torch.zeros(4, dtype=torch.uint8), None, torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32),
                          torch.zeros(1, 6, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 4, torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match='exactly one'):
        ops.pose_eval(torch.zeros(1, 30, 3), torch.zeros(17, 30), list(range(14)))

    class _Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def infer_net(self, image):
            raise AssertionError('never reached')
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        evaluate.run_evaluation(_Net(), 'h36m-p1', [], None)
    with pytest.raises(TypeError, match='DaNet or an InferenceEngine'):
        evaluate.run_evaluation(object(), 'h36m-p1', [], None)
    from danet_densepose2smpl_amd.smpl import SMPL
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        evaluate.Evaluator('h36m-p1', np.zeros((17, 6890), np.float32), SMPL())


def test_abi_has_the_eval_symbols():
    import __graft_entry__ as g
    g.build()
    from danet_densepose2smpl_amd import _lib
    lib = _lib.lib()
    for n in ('danet_pose_eval', 'danet_seg_confusion', 'danet_rotmat_to_angle_axis'):
        assert n in _lib.exported_symbols() and hasattr(lib, n)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'danet_hip.h')).read()
    for k, v in eo.SEG.items():
        name = {'accuracy': 'ACC', 'pixel_count': 'PIXELS', 'parts_accuracy': 'PARTS_ACC', 'parts_pixel_count': 'PARTS_PIXELS'}.get(k, k.upper())
        assert '#define DANET_SEG_%s %d\n' % (name, v) in hdr
    from danet_densepose2smpl_amd import ops
    assert ops.SEG == eo.SEG and ops.SEG_COUNTERS == eo.SEG_COUNTERS == 32
