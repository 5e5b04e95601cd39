"""Host side of the COCO keypoint evaluation (danet_densepose2smpl_amd/evaluate_coco.py), no GPU: the oracle of tests/coco_oracle.py
against known answers, the package's accumulation against the oracle's, the tie rule, the results json, the ground-truth packing,
the no-CPU-path rule and the ABI."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_oracle as co    # noqa: E402


def _person(rng, cx, cy, h, ann_id, image_id, area=None, **kw):
    """An annotation with 17 labelled keypoints spread over a box of height h around (cx, cy)."""
    kp = np.concatenate([np.array([cx, cy]) + (rng.random((17, 2)) - 0.5) * np.array([0.5 * h, h]), np.full((17, 1), 2.0)], axis=1)
    x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
    a = {'id': ann_id, 'image_id': image_id, 'category_id': 1, 'iscrowd': 0, 'num_keypoints': 17, 'keypoints': [float(v) for v in kp.reshape(-1)],
         'area': float(0.5 * (x1 - x0) * (y1 - y0)) if area is None else float(area), 'bbox': [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]}
    a.update(kw)
    return a


def _name(image_id):
    return '/data/val2014/COCO_val2014_%012d.jpg' % image_id


def _three_range_set(seed=0):
    """Four images; persons with areas in the small, medium and large range; one image without a person."""
    rng = np.random.default_rng(seed)
    images = [{'id': i} for i in (9, 4, 30, 12)]
    anns = [_person(rng, 100, 120, 40, 1, 4), _person(rng, 300, 200, 150, 2, 4), _person(rng, 200, 200, 300, 3, 9),
            _person(rng, 150, 150, 120, 4, 30), _person(rng, 350, 250, 280, 5, 30), _person(rng, 50, 60, 30, 6, 30)]
    areas = [a['area'] for a in anns]
    assert min(areas) < 32 ** 2 and any(32 ** 2 < a < 96 ** 2 for a in areas) and max(areas) > 96 ** 2
    return {'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}


def _through_the_package(preds, names, coco):
    """The same evaluation with the package's host code around the oracle's matching: CocoKeypointGT packs the ground truth,
    evaluation_order orders the detections, detection_area measures them, accumulate produces the numbers."""
    from danet_densepose2smpl_amd import evaluate_coco as ec
    gt = ec.CocoKeypointGT(coco)
    preds = np.asarray(preds, np.float64).reshape(-1, 17, 2)
    order, offs = ec.evaluation_order([ec.image_id(n) for n in names], gt)
    dm, di, gc = co.match_dataset(preds[order], ec.detection_area(preds[order]), offs, gt.kpts, gt.area, gt.bbox, gt.ignore, gt.iscrowd, gt.offsets)
    return ec.accumulate(dm, di, gc)['stats'], gc


def test_detections_equal_to_the_ground_truth_score_one():
    coco = _three_range_set()
    preds = np.array([a['keypoints'] for a in coco['annotations']]).reshape(-1, 17, 3)[:, :, :2]
    names = [_name(a['image_id']) for a in coco['annotations']]
    stats, dm, di, gc = co.evaluate_json(preds, names, coco)
    # (tp / (tp + eps) is one ulp below 1)
    np.testing.assert_allclose(stats, np.ones(10), rtol=0, atol=1e-12)
    assert (dm[:, 0] == 0x3ff).all() and gc.sum(0).tolist() == [6, 2, 2]
    got, gc2 = _through_the_package(preds, names, coco)
    np.testing.assert_allclose(got, np.ones(10), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(gc2, gc)


def test_detections_far_away_score_zero():
    coco = _three_range_set()
    preds = np.array([a['keypoints'] for a in coco['annotations']]).reshape(-1, 17, 3)[:, :, :2] + 10000.0
    names = [_name(a['image_id']) for a in coco['annotations']]
    stats, dm, di, gc = co.evaluate_json(preds, names, coco)
    assert (dm == 0).all()
    np.testing.assert_array_equal(stats, np.zeros(10))
    np.testing.assert_array_equal(_through_the_package(preds, names, coco)[0], np.zeros(10))


def _hand_case():
    """One image, two ground truths A and B with ONE labelled joint each (the nose, sigma 0.026) and area 5000, so that
    OKS = exp(-d^2 / (2 * (2 * 0.026)^2 * 5000)) = exp(-d^2 / 27.04) for a detection whose nose is d pixels from the ground truth's.
    Three detections: `miss` (far from both: OKS 0), `a` with OKS(A) = 0.92, `b` with OKS(B) = 0.62."""
    def gt(ann_id, x, y):
        kp = np.zeros((17, 3))
        kp[0] = (x, y, 2)
        return {'id': ann_id, 'image_id': 7, 'category_id': 1, 'iscrowd': 0, 'num_keypoints': 1, 'keypoints': [float(v) for v in kp.reshape(-1)],
                'area': 5000.0, 'bbox': [x - 30.0, y - 50.0, 60.0, 100.0]}
    coco = {'images': [{'id': 7}], 'annotations': [gt(1, 100.0, 100.0), gt(2, 400.0, 300.0)], 'categories': [{'id': 1}]}
    d = lambda o: np.sqrt(-np.log(o) * 27.04)

    def det(x, y):                                                           # the other joints do not count; spread them for the area
        k = np.zeros((17, 2))
        k[:] = (x, y)
        k[16] = (x + 60, y + 90)
        return k
    dets = {'miss': det(250.0, 600.0), 'a': det(100.0 + d(0.92), 100.0), 'b': det(400.0, 300.0 - d(0.62))}
    return coco, dets


def test_hand_computed_case_and_the_tie_rule():
    """All scores are equal, so the sample order is the evaluation order.

    Order (miss, a, b) at threshold 0.5: FP, TP, TP; two ground truths.  tp = 0 1 2, fp = 1 1 1, recall = 0 .5 1, precision =
    0 1/2 2/3, made non-increasing from the right: 2/3 2/3 2/3.  Every recall point reads 2/3: AP .5 = 2/3, AR .5 = 1.
    At 0.75 only `a` (0.92) matches: FP, TP, FP; tp = 0 1 1, fp = 1 1 2, recall = 0 .5 .5, precision 0 1/2 1/3 -> 1/2 1/2 1/3.  The 51
    recall points 0 .. 0.5 read 1/2, the 50 above read 0: AP .75 = 25.5 / 101, AR .75 = 1/2.
    Order (a, b, miss) at 0.5: TP, TP, FP; precision 1 1 2/3, recall .5 1 1: every recall point reads 1: AP .5 = 1."""
    coco, dets = _hand_case()
    m = co.oks_matrix([dets['miss'], dets['a'], dets['b']], np.array([a['keypoints'] for a in coco['annotations']]).reshape(2, 17, 3),
                      [5000.0, 5000.0], [a['bbox'] for a in coco['annotations']])
    np.testing.assert_allclose(m, [[0, 0], [0.92, 0], [0, 0.62]], atol=1e-12)
    names = [_name(7)] * 3
    stats, dm, di, gc = co.evaluate_json(np.array([dets['miss'], dets['a'], dets['b']]), names, coco)
    assert dm[:, 0].tolist() == [0, 0x1ff, 0x7] and (di[:, 0] == 0).all() and gc[0].tolist() == [2, 2, 0]
    np.testing.assert_allclose(stats[1], 2.0 / 3.0, rtol=1e-12)
    np.testing.assert_allclose(stats[2], 25.5 / 101, rtol=1e-12)
    np.testing.assert_allclose(stats[6:8], [1.0, 0.5], rtol=1e-12)
    assert stats[4] == -1 and stats[9] == -1                                 # no ground truth in the large range
    permuted, _, _, _ = co.evaluate_json(np.array([dets['a'], dets['b'], dets['miss']]), names, coco)
    np.testing.assert_allclose(permuted[1], 1.0, atol=1e-12)
    assert abs(permuted[1] - stats[1]) > 0.3 and abs(permuted[0] - stats[0]) > 0.05

    # the package builds the documented order: images ascending, the samples of an image in the order they were seen
    from danet_densepose2smpl_amd import evaluate_coco as ec
    coco2 = {'images': coco['images'] + [{'id': 3}, {'id': 5}], 'annotations': coco['annotations'], 'categories': coco['categories']}
    gt = ec.CocoKeypointGT(coco2)
    assert gt.image_ids.tolist() == [3, 5, 7] and gt.offsets.tolist() == [0, 0, 0, 2]
    far = dets['miss'] + 1000.0
    seen = [(7, dets['miss']), (5, far), (7, dets['a']), (3, far), (7, dets['b']), (5, far)]
    ids = [ec.image_id(_name(i)) for i, _ in seen]
    order, offs = ec.evaluation_order(ids, gt)
    assert order.tolist() == [3, 1, 5, 0, 2, 4] and offs.tolist() == [0, 1, 3, 6]
    preds = np.array([p for _, p in seen])
    dm2, di2, gc2 = co.match_dataset(preds[order], ec.detection_area(preds[order]), offs, gt.kpts, gt.area, gt.bbox, gt.ignore, gt.iscrowd, gt.offsets)
    got = ec.accumulate(dm2, di2, gc2)['stats']
    want, _, _, _ = co.evaluate_json(preds, [_name(i) for i in ids], coco2)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[1], 1.0 / 3.0, rtol=1e-12)               # three more false positives, all before image 7: 2 / (2 + 4)
    with pytest.raises(ValueError, match='does not list'):
        ec.evaluation_order([8], gt)


def test_no_ground_truth_in_a_range_gives_minus_one():
    from danet_densepose2smpl_amd import evaluate_coco as ec
    rng = np.random.default_rng(1)
    coco = {'images': [{'id': 1}], 'annotations': [_person(rng, 100, 100, 50, 1, 1, area=3000.0)], 'categories': [{'id': 1}]}
    preds = np.array(coco['annotations'][0]['keypoints']).reshape(1, 17, 3)[:, :, :2]
    stats, dm, di, gc = co.evaluate_json(preds, [_name(1)], coco)
    assert stats[4] == -1 and stats[9] == -1 and abs(stats[3] - 1) < 1e-12 and abs(stats[0] - 1) < 1e-12
    empty = {'images': [{'id': 1}], 'annotations': [], 'categories': [{'id': 1}]}
    stats, _, _, _ = co.evaluate_json(preds, [_name(1)], empty)
    np.testing.assert_array_equal(stats, -np.ones(10))
    np.testing.assert_array_equal(ec.accumulate(np.zeros((1, 3), int), np.zeros((1, 3), int), np.zeros((1, 3), int))['stats'], -np.ones(10))
    # ground truth without any detection: recall 0, precision 0
    stats, _, _, _ = co.evaluate_json(np.zeros((0, 17, 2)), [], coco)
    assert stats[0] == 0 and stats[5] == 0 and stats[3] == 0 and stats[4] == -1
    np.testing.assert_array_equal(ec.accumulate(np.zeros((0, 3), int), np.zeros((0, 3), int), np.array([[1, 1, 0]]))['stats'], stats)


def test_areas_on_the_boundaries_are_inside_both_ranges():
    rng = np.random.default_rng(2)
    for area, want in ((32.0 ** 2, [1, 1, 0]), (96.0 ** 2, [1, 1, 1]), (32.0 ** 2 - 1e-9, [1, 0, 0]), (96.0 ** 2 + 1e-9, [1, 0, 1])):
        a = _person(rng, 100, 100, 80, 1, 1, area=area)
        g = np.array(a['keypoints']).reshape(1, 17, 3)
        dm, di, gc = co.match_image(g[:, :, :2], [area], g, [area], [a['bbox']], [False], [False])
        assert gc.tolist() == want
        assert dm[0].tolist() == [0x3ff] * 3 and di[0].tolist() == [0x3ff * (1 - w) for w in want]
        # the same ground truth through the package's json reader keeps its area to the last bit, and the numbers follow the counts
        coco = {'images': [{'id': 1}], 'annotations': [json.loads(json.dumps(a))], 'categories': [{'id': 1}]}
        stats, gc2 = _through_the_package(g[:, :, :2], [_name(1)], coco)
        assert gc2[0].tolist() == want
        np.testing.assert_allclose(stats[[0, 3, 4]], [1 if w else -1 for w in want], rtol=0, atol=1e-12)
    # an unmatched detection is ignored by its OWN area, with the same closed ends
    g = np.zeros((0, 17, 3))
    d = np.zeros((1, 17, 2))
    for area, want in ((32.0 ** 2, [0, 0, 0x3ff]), (96.0 ** 2, [0, 0, 0]), (10.0, [0, 0x3ff, 0x3ff])):
        dm, di, gc = co.match_image(d, [area], g, [], [], [], [])
        assert di[0].tolist() == want and (dm == 0).all()


def test_package_accumulation_equals_the_oracle_on_random_flags():
    from danet_densepose2smpl_amd import evaluate_coco as ec
    rng = np.random.default_rng(3)
    for n, images in ((0, 2), (1, 1), (37, 5), (200, 40)):
        dm, di = rng.integers(0, 1024, (n, 3)), rng.integers(0, 1024, (n, 3)) & rng.integers(0, 1024, (n, 3))
        gc = rng.integers(0, 4, (images, 3))
        gc[:, 2] = 0 if n == 37 else gc[:, 2]
        p, r, s = co.accumulate(dm, di, gc)
        got = ec.accumulate(dm, di, gc)
        np.testing.assert_allclose(got['precision'], p, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got['recall'], r, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got['stats'], s, rtol=0, atol=1e-12)
    assert ec.STAT_NAMES == co.NAMES == ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
    # equal scores keep the order; other scores sort stably, descending
    dm, di, gc = rng.integers(0, 1024, (30, 3)), np.zeros((30, 3), int), np.array([[9, 5, 4]])
    sc = rng.integers(0, 3, 30).astype(float)
    o = np.argsort(-sc, kind='stable')
    np.testing.assert_array_equal(ec.accumulate(dm, di, gc, scores=sc)['stats'], ec.accumulate(dm[o], di[o], gc)['stats'])


def test_results_json_layout(tmp_path):
    from danet_densepose2smpl_amd import evaluate_coco as ec
    rng = np.random.default_rng(4)
    preds = rng.random((5, 17, 2)).astype(np.float32) * 300
    ids = [12, 3, 12, 7, 3]
    center, scale = rng.random((5, 2)) * 100, rng.random(5) + 0.5
    path = str(tmp_path / 'out' / 'results' / 'keypoints_val2014_results_danet.json')
    ec.write_results(path, preds, ids, center, scale)
    rec = json.load(open(path))
    assert [r['image_id'] for r in rec] == [12, 12, 3, 3, 7]                 # grouped by image, images as first seen
    src = [0, 2, 1, 4, 3]
    for r, i in zip(rec, src):
        assert sorted(r) == ['category_id', 'center', 'image_id', 'keypoints', 'scale', 'score']
        assert r['category_id'] == 1 and r['score'] == 1.0 and len(r['keypoints']) == 51
        k = np.array(r['keypoints']).reshape(17, 3)
        np.testing.assert_array_equal(k[:, :2], preds[i].astype(np.float64))
        assert (k[:, 2] == 1).all()
        np.testing.assert_allclose(r['center'], center[i])
        np.testing.assert_allclose(r['scale'], [scale[i], scale[i]])


def test_ground_truth_packing_of_the_synthetic_set(tmp_path):
    from danet_densepose2smpl_amd import evaluate_coco as ec, evaluate
    annot, jpath = ec.write_synthetic_coco(str(tmp_path), n=10, seed=5)
    coco = json.load(open(jpath))
    gt = ec.CocoKeypointGT(jpath)
    ids, per = co.pack_json(coco)
    assert gt.image_ids.tolist() == ids and len(gt) == len(coco['images']) >= 4
    assert np.diff(gt.offsets).tolist() == [len(per[i]) for i in ids]
    flat = [a for i in ids for a in per[i]]
    assert gt.ann_ids.tolist() == [a['id'] for a in flat] and all(a['category_id'] == 1 for a in flat)
    assert any(a['category_id'] != 1 for a in coco['annotations'])           # ... one of which was dropped
    np.testing.assert_array_equal(gt.kpts.reshape(-1, 51), np.array([a['keypoints'] for a in flat]))
    np.testing.assert_array_equal(gt.area, [a['area'] for a in flat])
    np.testing.assert_array_equal(gt.bbox, np.array([a['bbox'] for a in flat]))
    np.testing.assert_array_equal(gt.iscrowd, [a['iscrowd'] for a in flat])
    np.testing.assert_array_equal(gt.ignore, [int(bool(a['iscrowd']) or a['num_keypoints'] == 0) for a in flat])
    # what the set must contain
    d = np.load(annot)
    assert len(d['imgname']) == 10
    sample_ids = [ec.image_id(n) for n in d['imgname']]
    assert max(np.bincount(sample_ids)) >= 2                                   # several persons per image
    assert set(ids) - set(sample_ids)                                          # an image without samples
    assert gt.iscrowd.sum() >= 1 and ((gt.iscrowd == 0) & (gt.ignore == 1)).sum() >= 1
    assert (gt.area < 32 ** 2).any() and ((gt.area > 32 ** 2) & (gt.area < 96 ** 2)).any() and (gt.area > 96 ** 2).any()
    assert (gt.area == 32 ** 2).any() and (gt.area == 96 ** 2).any()
    assert sample_ids != sorted(sample_ids)                                    # stored out of image order
    ds = evaluate.EvalDataset(annot, str(tmp_path), 'coco')
    it = ds[0]
    assert it['img_raw'].ndim == 3 and ec.image_id(it['imgname']) == sample_ids[0] and it['scale'] == float(d['scale'][0])
    assert ec.EvalDataset is evaluate.EvalDataset


def test_constants():
    from danet_densepose2smpl_amd import constants
    assert constants.J24_TO_JCOCO == [19, 20, 21, 22, 23, 9, 8, 10, 7, 11, 6, 3, 2, 4, 1, 5, 0]
    np.testing.assert_array_equal(np.array(constants.COCO_SIGMAS), co.SIGMAS)


def test_cpu_tensors_and_hmr_are_refused():
    from danet_densepose2smpl_amd import evaluate_coco as ec, ops
    from danet_densepose2smpl_amd.smpl import SMPL
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.coco_keypoints(torch.zeros(2, 49, 3), torch.ones(2, 3), torch.zeros(2, 2), torch.ones(2))
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.coco_oks_match(torch.zeros(1, 17, 2), z(1), z(2, dt=torch.int64), z(1, 17, 3), z(1), z(1, 4), z(1, dt=torch.uint8), z(1, dt=torch.uint8),
                           z(2, dt=torch.int64))
    coco = _three_range_set()
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ec.CocoEvaluator(coco, SMPL())

    class _Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def infer_net(self, image):
            raise AssertionError('never reached')
    opts = types.SimpleNamespace(regressor='danet', keypoint_json=coco)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ec.run_evaluation(_Net(), [], None, options=opts)
    with pytest.raises(TypeError, match='DaNet or an InferenceEngine'):
        ec.run_evaluation(object(), [], None, options=opts)
    with pytest.raises(NotImplementedError, match='no HMR'):
        ec.run_evaluation(_Net(), [], None, options=types.SimpleNamespace(regressor='hmr', keypoint_json=coco))


def test_abi_has_the_coco_symbols():
    import __graft_entry__ as g
    g.build()
    from danet_densepose2smpl_amd import _lib, ops
    lib = _lib.lib()
    for n in ('danet_coco_keypoints', 'danet_coco_oks_match'):
        assert n in _lib.exported_symbols() and hasattr(lib, n)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'danet_hip.h')).read()
    assert '#define DANET_COCO_MAX_DETS %d\n' % ops.COCO_MAX_DETS in hdr and '#define DANET_COCO_MAX_GT %d\n' % ops.COCO_MAX_GT in hdr
    assert ops.COCO_MAX_DETS == co.MAX_DETS == 20 and ops.COCO_MAX_GT == 256
    # the declared-symbol equality of test_abi.py holds with the two new entries
    import test_abi
    test_abi.test_library_exports_every_declared_symbol()
