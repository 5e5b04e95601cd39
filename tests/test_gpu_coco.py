"""The COCO keypoint evaluation on the device (csrc/coco_ops.hip, danet_densepose2smpl_amd/evaluate_coco.py): coco_keypoints against
the reference chain (golden g26), coco_oks_match against the numpy oracle of tests/coco_oracle.py with flags and counts exactly
equal, run_evaluation end to end on the synthetic set (eagerly and through the InferenceEngine), and CocoEvaluator.update under
graph capture."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import golden, record
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_oracle as co    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- coco_keypoints ------------------------------------------------------------------------------------------------------------------

def test_coco_keypoints_against_golden_g26():
    """Tolerance: 4 x the reference chain's own float32-vs-float64 distance, as recorded in the golden (4.5e-5 px: the chain's affine
    runs in double, so its floor is the float32 rounding of a coordinate of up to 900 px).  The measured distance is printed and recorded."""
    from danet_densepose2smpl_amd import ops
    g = golden('g26_coco')
    floor = float(g['floor_px'])
    assert 1e-6 < floor < 1e-3 and g['preds'].dtype == np.float64
    assert g['scale'].min() <= 0.4 and g['scale'].max() >= 3.0 and (g['preds'] < 0).any()       # crops that overhang the image
    out = ops.coco_keypoints(_t(g['joints']), _t(g['camera']), _t(g['center']), _t(g['scale']), int(g['img_res']), float(g['focal_length']))
    assert out.shape == (8, 17, 2) and out.dtype == torch.float32
    d = float(np.abs(out.cpu().numpy().astype(np.float64) - g['preds']).max())
    print('coco_keypoints vs g26: max |d| = %.3e px, floor_px = %.3e, ratio %.2f' % (d, floor, d / floor))
    record('coco_keypoints_vs_g26', {'max_abs_px': d, 'floor_px': floor})
    assert d <= 4 * floor, (d, floor)
    # `out=` is written in place; a float64 scale (what the loader hands over) is taken
    buf = torch.zeros(8, 17, 2, device=DEV)
    assert ops.coco_keypoints(_t(g['joints']), _t(g['camera']), _t(g['center']), _t(g['scale'].astype(np.float64)), 224, 5000., out=buf) is buf
    assert torch.equal(buf, out)


# ---- coco_oks_match ------------------------------------------------------------------------------------------------------------------

def _gt(rng, cx, cy, h, vis=True):
    kp = np.concatenate([np.array([cx, cy]) + (rng.random((17, 2)) - 0.5) * np.array([0.5 * h, h]), np.full((17, 1), 2.0)], axis=1)
    kp[rng.random(17) < 0.25, 2] = 0
    kp[0, 2] = 2
    x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
    if not vis:
        kp[:] = 0
    return kp, float(0.5 * (x1 - x0) * (y1 - y0)), [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]


def _det_near(rng, kp, area, f):
    """A detection whose joints are off by about f standard deviations of the similarity's Gaussian: OKS around 1 / (1 + f^2)."""
    return kp[:, :2] + rng.normal(size=(17, 2)) * (f * np.sqrt(area) * 2 * co.SIGMAS)[:, None]


def _det_at(kp, area, oks):
    """A detection with exactly this similarity to the ground truth: every joint moved in x by the distance that gives it."""
    d = kp[:, :2].copy()
    d[:, 0] += np.sqrt(-np.log(oks) * 2 * co.VARS * area)
    return d


def _cases(seed):
    """-> list of images, each (dets [D,17,2], gt list of (kp, area, bbox, ignore, crowd))."""
    rng = np.random.default_rng(seed)
    images = []
    person = lambda h, **kw: dict(zip(('kp', 'area', 'bbox'), _gt(rng, rng.uniform(100, 500), rng.uniform(100, 400), h)), ignore=0, crowd=0, **kw)

    def mixed(G, D, heights=(30, 60, 150, 300)):
        gts = [person(float(rng.choice(heights)) * rng.uniform(0.8, 1.2)) for _ in range(G)]
        for k, g in enumerate(gts):
            if k % 7 == 3:
                g['crowd'] = g['ignore'] = 1
            elif k % 5 == 2:
                g['ignore'] = 1                                                  # (stands for num_keypoints == 0 with stale keypoints)
        dets = []
        for _ in range(D):
            g = gts[int(rng.integers(0, G))]
            dets.append(_det_near(rng, g['kp'], g['area'], rng.uniform(0.1, 1.5)) if rng.random() < 0.85 else rng.uniform(0, 600, (17, 2)))
        return np.array(dets).reshape(-1, 17, 2), gts
    images.append((np.zeros((0, 17, 2)), mixed(3, 0)[1]))                         # 0: no detection
    images.append((rng.uniform(0, 600, (2, 17, 2)), []))                          # 1: no ground truth
    images.append(mixed(5, 23))                                                   # 2: truncation to 20
    images.append(mixed(40, 12))                                                  # 3: G = 40, crowd and ignored interleaved
    # 4: ground truths without a labelled joint (the box rule): a detection inside the doubled box and one outside it; the crowd one
    # takes both detections that fall inside it (5)
    kp0, area0, bb0 = _gt(rng, 300, 250, 120, vis=False)
    nokp = {'kp': kp0, 'area': area0, 'bbox': bb0, 'ignore': 1, 'crowd': 0}
    crowd = {'kp': np.zeros((17, 3)), 'area': 20000.0, 'bbox': [900.0, 900.0, 100.0, 100.0], 'ignore': 1, 'crowd': 1}
    inside = np.array([bb0[0], bb0[1]]) + rng.random((17, 2)) * np.array([bb0[2], bb0[3]])
    outside = inside + np.array([4.0 * bb0[2], 0.0])
    in_crowd = lambda: 900.0 + rng.random((17, 2)) * 100.0
    images.append((np.array([outside, inside, in_crowd(), in_crowd(), inside + 1.0]), [nokp, crowd, person(80.0)]))
    # 6: the best ground truth (0.97) is ignored, a worse one (0.72) that is not ignored passes the thresholds up to 0.70
    a = person(150.0)
    b = dict(a, kp=a['kp'].copy(), ignore=1)
    d = _det_at(a['kp'], a['area'], 0.72)
    b['kp'][:, :2] = _det_at(np.concatenate([d, a['kp'][:, 2:]], axis=1), a['area'], 0.97)
    images.append((np.array([d]), [a, b]))
    # 7: areas exactly on the boundaries, ground truths and (unmatched) detections
    g1, g2 = person(60.0), person(200.0)
    g1['area'], g2['area'] = 32.0 ** 2, 96.0 ** 2
    box = lambda s: np.array([[1000.0, 1000.0]] * 16 + [[1000.0 + s, 1000.0 + s]])
    images.append((np.array([box(32.0), box(96.0), _det_near(rng, g1['kp'], g1['area'], 0.5), _det_near(rng, g2['kp'], g2['area'], 0.5)]), [g1, g2]))
    images.append(mixed(1, 3))                                                    # 8
    images.append(mixed(7, 9))                                                    # 9
    images.append(mixed(64, 20, heights=(40, 120)))                               # 10
    images.append(mixed(256, 21, heights=(25, 50, 110)))                          # 11: the largest supported G
    return images


def _pack(images):
    dk = np.concatenate([d for d, _ in images]).astype(np.float32)
    doff = np.cumsum([0] + [len(d) for d, _ in images]).astype(np.int64)
    gts = [g for _, gl in images for g in gl]
    goff = np.cumsum([0] + [len(gl) for _, gl in images]).astype(np.int64)
    pk = {'dt_kpts': dk, 'dt_area': (dk[:, :, 0].astype(np.float64).max(1) - dk[:, :, 0].astype(np.float64).min(1)) *
          (dk[:, :, 1].astype(np.float64).max(1) - dk[:, :, 1].astype(np.float64).min(1)), 'dt_offsets': doff,
          'gt_kpts': np.array([g['kp'] for g in gts], np.float64).reshape(-1, 17, 3), 'gt_area': np.array([g['area'] for g in gts], np.float64),
          'gt_bbox': np.array([g['bbox'] for g in gts], np.float64).reshape(-1, 4), 'gt_ignore': np.array([g['ignore'] for g in gts], np.uint8),
          'gt_iscrowd': np.array([g['crowd'] for g in gts], np.uint8), 'gt_offsets': goff}
    return pk


KEYS = ('dt_kpts', 'dt_area', 'dt_offsets', 'gt_kpts', 'gt_area', 'gt_bbox', 'gt_ignore', 'gt_iscrowd', 'gt_offsets')


@pytest.fixture(scope='module')
def match_cases():
    """The packed case set and the oracle's answer.  A condition on the INPUTS, not a tolerance: no oracle similarity lies within
    1e-6 of a threshold (reseeded until that holds), so that a last-bit difference of exp cannot flip a flag."""
    for seed in range(100, 120):
        pk = _pack(_cases(seed))
        gap = co.nearest_threshold_gap(pk['dt_kpts'], pk['dt_offsets'], pk['gt_kpts'], pk['gt_area'], pk['gt_bbox'], pk['gt_offsets'])
        if gap > 1e-6:
            break
    assert gap > 1e-6, gap
    want = co.match_dataset(*[pk[k] for k in KEYS])
    return pk, want, seed, gap


def _cases_do_what_they_are_for(pk, dm, di, gc):
    """Checked on the ORACLE's answer (no device involved)."""
    off, goff = pk['dt_offsets'], pk['gt_offsets']
    assert np.diff(off).tolist()[:4] == [0, 2, 23, 12] and np.diff(goff).tolist()[:4] == [3, 0, 5, 40] and np.diff(goff).max() == 256
    # the cases do what they are there for (checked on the oracle's answer)
    assert (di[off[2] + 20:off[3]] == 0x3ff).all() and (dm[off[2] + 20:off[3]] == 0).all()                        # truncation
    i4 = off[4]
    assert dm[i4, 0] == 0 and dm[i4 + 1, 0] == 0x3ff and di[i4 + 1, 0] == 0x3ff                                   # outside / inside the doubled box
    assert dm[i4 + 2, 0] == 0x3ff and dm[i4 + 3, 0] == 0x3ff and di[i4 + 2, 0] == di[i4 + 3, 0] == 0x3ff         # the crowd region, twice
    assert dm[i4 + 4, 0] == 0                                                                                     # ... the plain ignored one only once
    assert dm[off[5], 0] == 0x3ff and di[off[5], 0] == 0x3e0                      # up to 0.70 the plain one, above it the ignored one
    assert di[off[6], :].tolist() == [0, 0, 0x3ff] and di[off[6] + 1, :].tolist() == [0, 0, 0] and gc[6].tolist() == [2, 2, 1]


def test_oks_match_equals_the_oracle_exactly(match_cases):
    from danet_densepose2smpl_amd import ops
    pk, (dm, di, gc), seed, gap = match_cases
    _cases_do_what_they_are_for(pk, dm, di, gc)
    got = ops.coco_oks_match(*[_t(pk[k]) for k in KEYS])
    gm, gi, gn = (x.cpu().numpy() for x in got)
    print('oks_match: seed %d, nearest |OKS - threshold| = %.2e, %d detections, %d ground truths; flags differing: match %d ignore %d'
          % (seed, gap, len(dm), len(pk['gt_area']), int((gm != dm).sum()), int((gi != di).sum())))
    np.testing.assert_array_equal(gn, gc)
    np.testing.assert_array_equal(gm, dm)
    np.testing.assert_array_equal(gi, di)
    assert got[2].dtype == torch.int32 and gm.max() <= 0x3ff


def test_oks_match_refuses_more_than_256_ground_truths_without_launching(match_cases):
    from danet_densepose2smpl_amd import ops, _lib
    rng = np.random.default_rng(7)
    gts = [dict(zip(('kp', 'area', 'bbox'), _gt(rng, 300, 300, 100)), ignore=0, crowd=0) for _ in range(257)]
    pk = _pack([(rng.uniform(0, 600, (2, 17, 2)), gts)])
    with pytest.raises(RuntimeError, match='257 ground truths.*at most 256'):
        ops.coco_oks_match(*[_t(pk[k]) for k in KEYS])
    # the C entry itself: an error status, the message, and the outputs untouched
    L = _lib.lib()
    t = {k: _t(pk[k]) for k in KEYS}
    dm = torch.full((2, 3), 0x5a5a, dtype=torch.int16, device=DEV)
    di, gc = dm.clone(), torch.full((1, 3), -7, dtype=torch.int32, device=DEV)
    rc = L.danet_coco_oks_match(t['dt_kpts'].data_ptr(), t['dt_area'].data_ptr(), t['dt_offsets'].data_ptr(), 2, t['gt_kpts'].data_ptr(),
                                t['gt_area'].data_ptr(), t['gt_bbox'].data_ptr(), t['gt_ignore'].data_ptr(), t['gt_iscrowd'].data_ptr(),
                                t['gt_offsets'].data_ptr(), 257, 1, 257, dm.data_ptr(), di.data_ptr(), gc.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'at most 256' in L.danet_last_error()
    assert (dm == 0x5a5a).all() and (di == 0x5a5a).all() and (gc == -7).all()
    with pytest.raises(ValueError, match='ascend'):
        ops.coco_oks_match(*[_t(pk[k]) if k != 'dt_offsets' else _t(np.array([0, 3])) for k in KEYS])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(4), None, pretrained=False).cuda().eval()


def test_run_evaluation_end_to_end_eager_and_engine(model, tmp_path, capsys):
    from danet_densepose2smpl_amd import evaluate_coco as ec, geometry
    n, bs = 8, 4
    annot, jpath = ec.write_synthetic_coco(str(tmp_path), n=n, seed=21)
    ds = ec.EvalDataset(annot, str(tmp_path), 'coco')
    coco = json.load(open(jpath))
    opts = types.SimpleNamespace(regressor='danet', keypoint_json=jpath, output_dir=str(tmp_path / 'out'))
    ra, rb = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    va = ec.run_evaluation(model, ds, ra, batch_size=bs, num_workers=2, options=opts)
    printed = capsys.readouterr().out
    assert '| Arch | AP | Ap .5 | AP .75 | AP (M) | AP (L) | AR | AR .5 | AR .75 | AR (M) | AR (L) |' in printed and '| danet | ' in printed
    eng = model.inference_engine(bs)
    try:
        vb = ec.run_evaluation(eng, ds, rb, batch_size=bs, num_workers=0, options=opts)
    finally:
        eng.close()
    names = [os.path.join(str(tmp_path), x) for x in np.load(annot)['imgname']]
    outs = []
    for path, values in ((ra, va), (rb, vb)):
        out = np.load(path)
        assert set(out.files) == {'pred_joints', 'pose', 'betas', 'camera', 'preds', 'image_ids'}
        assert out['preds'].shape == (n, 17, 2) and out['pose'].shape == (n, 72) and out['camera'].shape == (n, 3) and np.isfinite(out['preds']).all()
        assert out['image_ids'].tolist() == [ec.image_id(x) for x in names]
        want, dm, di, gc = co.evaluate_json(out['preds'], names, coco)
        assert list(values) == ec.STAT_NAMES
        print('end to end', path[-5:], [round(v, 4) for v in values.values()], 'oracle', np.round(want, 4).tolist())
        np.testing.assert_allclose(list(values.values()), want, rtol=0, atol=1e-12)
        assert gc.sum(0)[0] == sum(1 for a in coco['annotations'] if a['category_id'] == 1 and not a['iscrowd'] and a['num_keypoints'] > 0)
        outs.append(out)
    rec = json.load(open(str(tmp_path / 'out' / 'results' / 'keypoints_val2014_results_danet.json')))
    assert len(rec) == n and len(rec[0]['keypoints']) == 51
    # eager against the engine: the parity bound tests/test_gpu_infer.py holds the two to, on everything `para` holds
    a, b = outs
    d = max(float(np.abs(a[k] - b[k]).max()) for k in ('betas', 'camera'))
    Ra = geometry.batch_rodrigues(_t(a['pose'].astype(np.float32).reshape(-1, 3)))
    Rb = geometry.batch_rodrigues(_t(b['pose'].astype(np.float32).reshape(-1, 3)))
    d = max(d, float((Ra - Rb).abs().max()))
    dp = float(np.abs(a['preds'] - b['preds']).max())
    print('coco eager vs engine: max abs over para %.3e, over preds %.3e px' % (d, dp))
    record('coco_engine_vs_infer_net', {'para_max_abs': d, 'preds_max_abs_px': dp})
    assert d < 5e-4, d


def test_summary_on_predictions_that_match(tmp_path):
    """CocoEvaluator.summary() on predictions derived from the ground truth of the synthetic set (whose samples are stored out of image
    order): per sample the keypoints of its own person moved to a similarity of 1, 0.92, 0.77 or 0.62, plus a repeat of the first
    sample (a false positive behind the true one).  The flags of summary() are the oracle's, the numbers too, and they are not zero."""
    from danet_densepose2smpl_amd import assets, evaluate_coco as ec
    from danet_densepose2smpl_amd.smpl import SMPL
    annot, jpath = ec.write_synthetic_coco(str(tmp_path), n=10, seed=33)
    coco = json.load(open(jpath))
    d = np.load(annot)
    names = [os.path.join(str(tmp_path), str(x)) for x in d['imgname']]
    preds = []
    for i, name in enumerate(names):
        mine = [a for a in coco['annotations'] if a['image_id'] == ec.image_id(name) and a['category_id'] == 1 and a['num_keypoints'] > 0
                and np.allclose([a['bbox'][0] + a['bbox'][2] / 2, a['bbox'][1] + a['bbox'][3] / 2], d['center'][i])]
        assert len(mine) == 1
        kp = np.array(mine[0]['keypoints']).reshape(17, 3)
        preds.append(kp[:, :2] if i % 4 == 0 else _det_at(kp, mine[0]['area'], (0.92, 0.77, 0.62)[i % 4 - 1]))
    preds, names = np.array(preds + preds[:1], np.float32), names + names[:1]
    want, dm, di, gc = co.evaluate_json(preds, names, coco)
    ev = ec.CocoEvaluator(jpath, SMPL(assets.make_synthetic_smpl(0)).to(DEV))
    n = len(names)
    for lo, hi in ((0, 4), (4, n)):                                              # two "batches", as update() would have left them
        ev._preds.append(_t(preds[lo:hi]))
        ev._para.append(torch.zeros(hi - lo, 229, device=DEV))
        ev._center.append(torch.zeros(hi - lo, 2, device=DEV))
        ev._scale.append(torch.ones(hi - lo, device=DEV))
    ev._names += names
    s = ev.summary()
    ids = [ec.image_id(x) for x in names]
    assert ids != sorted(ids) and s['order'].tolist() == sorted(range(n), key=lambda k: (ids[k], k))
    np.testing.assert_array_equal(s['dt_match'], dm)
    np.testing.assert_array_equal(s['dt_ignore'], di)
    np.testing.assert_array_equal(s['gt_count'], gc)
    print('summary on matching predictions', [round(v, 4) for v in s['values']])
    np.testing.assert_allclose(s['values'], want, rtol=0, atol=1e-12)
    v = s['name_value']
    assert 0.3 < v['AP'] < 1 and v['Ap .5'] > v['AP .75'] > 0 and 0.3 < v['AR'] < 1 and v['AR .5'] > 0.99
    assert (dm[:, 0] == 0x3ff).any() and (dm[:, 0] == 0x7).any() and (dm[:, 0] == 0).sum() >= 1      # full, partial, the repeat


def test_evaluator_update_under_graph_capture():
    from danet_densepose2smpl_amd import assets, evaluate_coco as ec, ops
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL(assets.make_synthetic_smpl(0)).to(DEV)
    coco = {'images': [{'id': 5}], 'annotations': [], 'categories': [{'id': 1}]}
    B = 4

    def inputs(seed):
        rng = np.random.default_rng(seed)
        rot = ops.rodrigues_smplx(_t(rng.normal(0, 0.2, (B * 24, 3)).astype(np.float32))).view(B, 216)
        cam = _t(np.stack([rng.uniform(0.6, 1.2, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.2, 0.2, B)], 1).astype(np.float32))
        para = torch.cat([cam, _t(rng.normal(0, 1, (B, 10)).astype(np.float32)), rot], dim=1).contiguous()
        return para, _t(rng.uniform(50, 400, (B, 2)).astype(np.float32)), _t(rng.uniform(0.5, 2.5, B).astype(np.float32))
    para, center, scale = inputs(1)
    batch = {'center': center, 'scale': scale, 'imgname': ['COCO_val2014_%012d.jpg' % 5] * B}
    ev = ec.CocoEvaluator(coco, smpl)
    eager = ev.update(batch, para).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update(batch, para)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                                       # (the stream of the warm-up: its SMPL ticket buffer exists)
        out = ev.update(batch, para)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    p2, c2, s2 = inputs(2)                                                       # new inputs through the same static buffers
    para.copy_(p2); center.copy_(c2); scale.copy_(s2)
    g.replay()
    torch.cuda.synchronize()
    want = ec.CocoEvaluator(coco, smpl).update({'center': c2, 'scale': s2, 'imgname': batch['imgname']}, p2)
    assert torch.equal(out, want) and not torch.equal(out, eager)
    assert len(ev._names) == 3 * B
