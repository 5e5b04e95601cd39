"""The evaluation pipeline on the device (csrc/eval_ops.hip, danet_densepose2smpl_amd/evaluate.py): the three scoring ops against
the goldens and the numpy oracles of tests/eval_oracle.py, and run_evaluation end to end against a loop assembled here from
metrics.pose_errors, PartRenderer and the counting oracle."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, record
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_oracle as eo    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H36M_TO_J14 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- (a) pose_eval ---------------------------------------------------------------------------------------------------------------

def _g13_as_vertices():
    """Golden g13 holds mapped, centred joints.  As a mesh: vertex 0 = the origin (the pelvis), vertex 1 + k = joint k, and a
    regressor whose row `mapper[k]` picks vertex 1 + k and whose row 0 picks vertex 0 -- the op then sees exactly g13's joints."""
    g = golden('g13_eval_metrics')
    pred, gt = g['pred'].astype(np.float32), g['gt'].astype(np.float32)
    B, J = pred.shape[:2]
    verts = np.concatenate([np.zeros((B, 1, 3), np.float32), pred], 1)
    Jr = np.zeros((17, J + 1), np.float32)
    Jr[0, 0] = 1
    for k, m in enumerate(H36M_TO_J14):
        Jr[m, 1 + k] = 1
    return g, verts, Jr, gt


def test_pose_eval_against_golden_g13_reflection_included():
    from danet_densepose2smpl_amd import ops
    g, verts, Jr, gt = _g13_as_vertices()
    # the golden set contains a sample whose unconstrained optimum is a reflection (the det = -1 correction is exercised)
    X1, X2 = g['pred'] - g['pred'].mean(1, keepdims=True), g['gt'] - g['gt'].mean(1, keepdims=True)
    dets = [np.linalg.det(np.linalg.svd(a.T @ b)[0] @ np.linalg.svd(a.T @ b)[2]) for a, b in zip(X1.astype(np.float64), X2.astype(np.float64))]
    assert min(dets) < 0 < max(dets)
    e, r, j17 = ops.pose_eval(_t(verts), _t(Jr), H36M_TO_J14, gt_keypoints_3d=_t(gt))
    assert e.is_cuda and e.shape == (verts.shape[0],) and j17.shape == (verts.shape[0], 17, 3)
    print('g13 mpjpe', e.cpu().numpy(), g['mpjpe'], 'recon', r.cpu().numpy(), g['recon'])
    np.testing.assert_allclose(e.cpu().numpy(), g['mpjpe'], rtol=1e-5)
    np.testing.assert_allclose(r.cpu().numpy(), g['recon'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(j17.cpu().numpy()[:, H36M_TO_J14], g['pred'], atol=1e-5)


def _fixture(B=5, V=300, seed=5):
    """The inputs of test_gpu_f4.test_pose_evaluation_block_on_device."""
    rng = np.random.default_rng(seed)
    Jr = rng.random((17, V)).astype(np.float32)
    Jr /= Jr.sum(1, keepdims=True)
    pv, gv = rng.normal(size=(B, V, 3)).astype(np.float32), rng.normal(size=(B, V, 3)).astype(np.float32)
    return Jr, pv, gv


@pytest.mark.parametrize('B,V', [(5, 300), (32, 6890), (1, 257)])
def test_pose_eval_against_pose_errors_both_ground_truth_forms(B, V):
    from danet_densepose2smpl_amd import metrics, ops
    Jr, pv, gv = _fixture(B, V)
    j = np.einsum('jv,bvk->bjk', Jr.astype(np.float64), pv.astype(np.float64))
    for mapper in (H36M_TO_J14, H36M_TO_J14 + [0, 7, 9]):
        e0, r0, j0 = metrics.pose_errors(_t(pv), _t(Jr), mapper, gt_vertices=_t(gv))
        e, r, j17 = ops.pose_eval(_t(pv), _t(Jr), mapper, gt_vertices=_t(gv))
        print('vertices form', B, V, len(mapper), float((e - e0).abs().max()), float((r - r0).abs().max()), float(np.abs(j17.cpu().numpy() - j).max()))
        np.testing.assert_allclose(j17.cpu().numpy(), j, atol=1e-5)
        np.testing.assert_allclose(e.cpu().numpy(), e0.cpu().numpy(), rtol=1e-5)
        np.testing.assert_allclose(r.cpu().numpy(), r0.cpu().numpy(), rtol=1e-4, atol=1e-6)
        # given joints: the ground truth of the other form, handed over already mapped and centred
        g17 = metrics.regress_joints(_t(gv), _t(Jr))
        gk = (g17[:, mapper] - g17[:, [0]]).contiguous()
        e1, r1, _ = metrics.pose_errors(_t(pv), _t(Jr), mapper, gt_keypoints_3d=gk)
        e2, r2, _ = ops.pose_eval(_t(pv), _t(Jr), mapper, gt_keypoints_3d=gk)
        np.testing.assert_allclose(e2.cpu().numpy(), e1.cpu().numpy(), rtol=1e-5)
        np.testing.assert_allclose(r2.cpu().numpy(), r1.cpu().numpy(), rtol=1e-4, atol=1e-6)
    if B == 5:                                                   # test_gpu_f4's own expectations
        pj = (j[:, H36M_TO_J14] - j[:, [0]]).astype(np.float32)
        g = np.einsum('jv,bvk->bjk', Jr, gv)
        gj = g[:, H36M_TO_J14] - g[:, [0]]
        e, r, _ = ops.pose_eval(_t(pv), _t(Jr), H36M_TO_J14, gt_vertices=_t(gv))
        np.testing.assert_allclose(e.cpu().numpy(), np.sqrt(((pj - gj) ** 2).sum(-1)).mean(-1), rtol=1e-5)
        rc = metrics.reconstruction_error(torch.from_numpy(pj), torch.from_numpy(gj)).numpy()
        np.testing.assert_allclose(r.cpu().numpy(), rc, rtol=1e-4, atol=1e-6)


def test_pose_eval_under_graph_replay():
    from danet_densepose2smpl_amd import ops
    Jr, pv, gv = _fixture(8, 6890, seed=9)
    sv, sg, sJ = _t(pv), _t(gv), _t(Jr)
    eager = [t.clone() for t in ops.pose_eval(sv, sJ, H36M_TO_J14, gt_vertices=sg)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.pose_eval(sv, sJ, H36M_TO_J14, gt_vertices=sg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.pose_eval(sv, sJ, H36M_TO_J14, gt_vertices=sg)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    _, pv2, gv2 = _fixture(8, 6890, seed=10)                     # new inputs through the same static buffers
    sv.copy_(_t(pv2))
    sg.copy_(_t(gv2))
    g.replay()
    torch.cuda.synchronize()
    want = ops.pose_eval(_t(pv2), sJ, H36M_TO_J14, gt_vertices=_t(gv2))
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    with pytest.raises(RuntimeError, match='joint_mapper'):
        ops.pose_eval(sv, sJ, [0, 1, 17], gt_vertices=sg)


# ---- (b) seg_confusion -------------------------------------------------------------------------------------------------------------

def _g25():
    g = golden('g25_eval')
    off, shp = g['offsets'], g['orig_shape']
    N = len(off) - 1
    cut = lambda k: [g[k][off[i]:off[i + 1]].reshape(shp[i]) for i in range(N)]
    return g, N, cut('gt_mask'), cut('gt_parts')


def _run_seg(g, idx, gm, gp, counters):
    from danet_densepose2smpl_amd import evaluate, ops
    pk = evaluate.pack_labels([gm[i] for i in idx], [gp[i] for i in idx], g['center'][idx], g['scale'][idx], 224, DEV)
    return ops.seg_confusion(_t(g['mask'][idx].astype(np.float32)), _t(g['parts'][idx].astype(np.int64)), pk['gt_mask'], pk['gt_parts'],
                             pk['offsets'], pk['shapes'], pk['rects'], pk['tables'], pk['max_pixels'], counters)


def _oracle(g, idx, gm, gp):
    from danet_densepose2smpl_amd import evaluate
    return eo.score_batch(g['mask'][idx].astype(np.float32), g['parts'][idx].astype(np.int64), [gm[i] for i in idx], [gp[i] for i in idx],
                          g['center'][idx], g['scale'][idx], evaluate.uncrop_geometry)


def test_seg_confusion_equals_the_oracle_on_g25():
    g, N, gm, gp = _g25()
    zeros = lambda: torch.zeros(32, dtype=torch.int64, device=DEV)
    everything = list(range(N))
    whole = _run_seg(g, everything, gm, gp, zeros()).cpu().numpy()
    np.testing.assert_array_equal(whole, _oracle(g, everything, gm, gp))
    assert whole[31] == 0
    for i in range(N):                                           # B = 1, every case
        np.testing.assert_array_equal(_run_seg(g, [i], gm, gp, zeros()).cpu().numpy(), _oracle(g, [i], gm, gp))
    acc = zeros()                                                # accumulated over two calls into the same counters
    _run_seg(g, everything[:4], gm, gp, acc)
    _run_seg(g, everything[4:], gm, gp, acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), whole)
    np.testing.assert_array_equal(_run_seg(g, everything, gm, gp, zeros()).cpu().numpy(), whole)           # a second run: identical
    # one kind of label image only: the other half of the counters stays zero
    from danet_densepose2smpl_amd import evaluate, ops
    pk = evaluate.pack_labels(gm, None, g['center'], g['scale'], 224, DEV)
    only = ops.seg_confusion(_t(g['mask'].astype(np.float32)), _t(g['parts'].astype(np.int64)), pk['gt_mask'], None, pk['offsets'], pk['shapes'],
                             pk['rects'], pk['tables'], pk['max_pixels'], zeros()).cpu().numpy()
    np.testing.assert_array_equal(only[:8], whole[:8])
    assert (only[8:] == 0).all()


# ---- (c) rotmat_to_angle_axis ------------------------------------------------------------------------------------------------------

def _rotations(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return eo.rodrigues(ax * rng.uniform(lo, hi, (n, 1))).astype(np.float32)


def test_rotmat_to_angle_axis_inverts_batch_rodrigues():
    from danet_densepose2smpl_amd import geometry
    R = _rotations(4096, 0.0, np.pi - 0.05, 1)
    aa = geometry.rotmat_to_angle_axis(_t(R))
    assert aa.shape == (4096, 3) and aa.dtype == torch.float32
    back = geometry.batch_rodrigues(aa).cpu().numpy()
    err = float(np.abs(back - R).max())
    print('round trip max abs', err)
    assert err < 1e-4, err                                       # the project's fp32 bar for rotation round trips
    ang = np.linalg.norm(aa.cpu().numpy().astype(np.float64), axis=1)
    assert ang.max() <= np.pi * (1 + 2.0 ** -22)                 # [0, pi] to an fp32 rounding of the three components
    np.testing.assert_allclose(aa.cpu().numpy(), eo.rotmat_to_angle_axis(R), atol=2e-5)
    assert torch.equal(geometry.rotmat_to_angle_axis(torch.eye(3, device=DEV)[None]), torch.zeros(1, 3, device=DEV))
    for k in range(3):
        Rk = -np.eye(3, dtype=np.float32)
        Rk[k, k] = 1
        got = geometry.rotmat_to_angle_axis(_t(Rk[None])).cpu().numpy()[0]
        np.testing.assert_allclose(got, np.float32(np.pi) * np.eye(3, dtype=np.float32)[k], atol=1e-6)
    # [B,24,3,3] comes back as [B*24,3]
    assert geometry.rotmat_to_angle_axis(_t(R[:48].reshape(2, 24, 3, 3))).shape == (48, 3)


def test_rotmat_to_angle_axis_near_pi():
    """Closer to pi than 0.05 no bar follows from the formats alone.  The bar is measured: the oracle in fp32 against itself in fp64
    on the same matrices, compared as rotations (the sign of a half-turn's axis is free); the device may take twice that.
    Measured: oracle 4.8e-7."""
    from danet_densepose2smpl_amd import geometry
    R = np.concatenate([_rotations(2048, np.pi - 0.05, np.pi, 2), _rotations(512, np.pi - 1e-3, np.pi, 3)])
    a64 = eo.rotmat_to_angle_axis(R.astype(np.float64), np.float64)
    a32 = eo.rotmat_to_angle_axis(R, np.float32)
    oracle_err = float(np.abs(eo.rodrigues(a32) - eo.rodrigues(a64)).max())
    aa = geometry.rotmat_to_angle_axis(_t(R)).cpu().numpy()
    dev_err = float(np.abs(eo.rodrigues(aa) - eo.rodrigues(a64)).max())
    print('near pi: oracle fp32 vs fp64', oracle_err, 'device vs fp64', dev_err)
    record('rotmat_to_angle_axis_near_pi', {'oracle_fp32_vs_fp64': oracle_err, 'device_vs_fp64': dev_err})
    assert np.linalg.norm(aa.astype(np.float64), axis=1).max() <= np.pi * (1 + 2.0 ** -22)
    assert dev_err <= 2 * oracle_err, (dev_err, oracle_err)


# ---- end to end --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(4), None, pretrained=False).cuda().eval()


def _reference_loop(model, name, ds, batch_size, Jr, renderer):
    """The evaluation assembled from the pieces the project had before: infer_net, the SMPL layer, metrics.pose_errors, PartRenderer
    and the per-sample host loop of the counting oracle."""
    from danet_densepose2smpl_amd import evaluate, metrics
    plan = evaluate.dataset_plan(name)
    smpl = model.iuv2smpl.smpl
    mp, re, j17s, paras = [], [], [], []
    counts = np.zeros(32, np.int64)
    for host in evaluate.iterate_batches(ds, batch_size):
        b = evaluate.to_device(host, torch.device(DEV))
        para = model.infer_net(b['img'])['para'].clone()
        paras.append(para.cpu().numpy())
        rot = para[:, 13:].reshape(-1, 24, 3, 3)
        verts = smpl(betas=para[:, 3:13].contiguous(), body_pose=rot[:, 1:], global_orient=rot[:, :1], pose2rot=False).vertices
        if name == 'lsp':
            mask, parts = renderer(verts, para[:, :3].contiguous())
            counts += eo.score_batch(mask.cpu().numpy(), parts.cpu().numpy(), host['gt_mask'], host['gt_parts'], host['center'], host['scale'],
                                     evaluate.uncrop_geometry)
            continue
        if name == '3dpw':                                       # (no gendered synthetic models: both are the neutral one)
            gv = smpl(global_orient=b['pose'][:, :3], body_pose=b['pose'][:, 3:], betas=b['betas']).vertices
            e, r, j = metrics.pose_errors(verts, _t(Jr), plan['joint_mapper_h36m'], gt_vertices=gv)
        else:
            gt = b['pose_3d'][:, plan['joint_mapper_gt'], :-1]
            e, r, j = metrics.pose_errors(verts, _t(Jr), plan['joint_mapper_h36m'], gt_keypoints_3d=gt)
        mp.append(e.cpu().numpy()); re.append(r.cpu().numpy()); j17s.append(j.cpu().numpy())
    cat = lambda l: np.concatenate(l) if l else None
    return cat(mp), cat(re), cat(j17s), np.concatenate(paras), counts


@pytest.mark.parametrize('name', ['h36m-p1', '3dpw', 'lsp'])
def test_run_evaluation_end_to_end(model, name, tmp_path, capsys):
    from danet_densepose2smpl_amd import evaluate, geometry
    n, bs = 6, 4                                                 # a full and a short batch
    path = evaluate.write_synthetic_dataset(str(tmp_path), name, n=n, seed=11)
    ds = evaluate.EvalDataset(path, str(tmp_path), name)
    smpl = model.iuv2smpl.smpl
    Jr = evaluate.synthetic_h36m_regressor(smpl.v_template.shape[0])
    renderer = evaluate.synthetic_part_renderer(smpl.faces)
    result = str(tmp_path / 'result.npz')
    s = evaluate.run_evaluation(model, name, ds, result, batch_size=bs, num_workers=2, log_freq=1)
    printed = capsys.readouterr().out
    assert '*** Final Results ***' in printed
    mp, re, j17, paras, counts = _reference_loop(model, name, ds, bs, Jr, renderer)
    out = np.load(result)
    assert set(out.files) == {'pred_joints', 'pose', 'betas', 'camera'}
    assert out['pred_joints'].shape == (n, 17, 3) and out['pose'].shape == (n, 72) and out['betas'].shape == (n, 10) and out['camera'].shape == (n, 3)
    np.testing.assert_array_equal(out['betas'].astype(np.float32), paras[:, 3:13])
    np.testing.assert_array_equal(out['camera'].astype(np.float32), paras[:, :3])
    back = geometry.batch_rodrigues(_t(out['pose'].astype(np.float32).reshape(-1, 3))).cpu().numpy()
    assert np.abs(back - paras[:, 13:].reshape(-1, 3, 3)).max() < 1e-4
    if name == 'lsp':
        for k, i in eo.SEG.items():
            w = 2 if k in ('tp', 'fp', 'fn') else (7 if k.startswith('parts_') and k[6:] in ('tp', 'fp', 'fn') else 1)
            np.testing.assert_array_equal(np.atleast_1d(s['counters'][k]), counts[i:i + w])
        assert counts[eo.SEG['pixel_count']] == sum(int(np.prod(ds[i]['orig_shape'])) for i in range(n))
        assert s['accuracy'] == counts[6] / counts[7] and s['parts_accuracy'] == counts[29] / counts[30]
        tp, fp, fn = counts[8:15].astype(float), counts[15:22].astype(float), counts[22:29].astype(float)
        with np.errstate(invalid='ignore', divide='ignore'):
            np.testing.assert_allclose(s['parts_f1'], (2 * tp / (2 * tp + fp + fn)).mean(), rtol=1e-12, equal_nan=True)
        assert 'Parts Accuracy' in printed and (out['pred_joints'] == 0).all()
        assert counts[eo.SEG['tp'] + 1] > 0                    # the synthetic meshes do land on the synthetic people
    else:
        np.testing.assert_allclose(s['mpjpe_per_sample'], mp, rtol=1e-5)
        np.testing.assert_allclose(s['recon_err_per_sample'], re, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(out['pred_joints'], j17, atol=1e-5)
        np.testing.assert_allclose(s['mpjpe'], 1000 * mp.astype(np.float64).mean(), rtol=1e-5)
        np.testing.assert_allclose(s['recon_err'], 1000 * re.astype(np.float64).mean(), rtol=1e-4)
        assert 'MPJPE: ' in printed and 'Reconstruction Error: ' in printed


def test_per_action_tables_for_h36m_p2(model, tmp_path):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), 'h36m-p2', n=6, seed=12)
    ds = evaluate.EvalDataset(path, str(tmp_path), 'h36m-p2')
    s = evaluate.run_evaluation(model, 'h36m-p2', ds, None, batch_size=4, num_workers=0)
    assert list(s['actions']) == ['Directions', 'Eating', 'Walking']
    for k, a in enumerate(s['actions']):
        ix = [i for i in range(6) if i % 3 == k]
        np.testing.assert_allclose(s['actions'][a]['mpjpe'], 1000 * s['mpjpe_per_sample'][ix].mean(), rtol=1e-12)
        np.testing.assert_allclose(s['actions'][a]['recon_err'], 1000 * s['recon_err_per_sample'][ix].mean(), rtol=1e-12)


def test_engine_and_danet_agree_as_model(model, tmp_path):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), 'h36m-p1', n=8, seed=13)
    ds = evaluate.EvalDataset(path, str(tmp_path), 'h36m-p1')
    ra, rb = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    evaluate.run_evaluation(model, 'h36m-p1', ds, ra, batch_size=4, num_workers=0)
    eng = model.inference_engine(4)
    try:
        evaluate.run_evaluation(eng, 'h36m-p1', ds, rb, batch_size=4, num_workers=0)
    finally:
        eng.close()
    a, b = np.load(ra), np.load(rb)
    d = max(float(np.abs(a[k] - b[k]).max()) for k in ('betas', 'camera'))
    from danet_densepose2smpl_amd import geometry
    Ra = geometry.batch_rodrigues(_t(a['pose'].astype(np.float32).reshape(-1, 3)))
    Rb = geometry.batch_rodrigues(_t(b['pose'].astype(np.float32).reshape(-1, 3)))
    d = max(d, float((Ra - Rb).abs().max()))
    print('engine vs infer_net as model: max abs over para', d)
    record('eval_engine_vs_infer_net', {'para_max_abs': d})
    assert d < 5e-4, d                                           # the bound test_gpu_infer.py holds the two to
