"""Trainer.fit on the synthetic 'h36m_dp' set (6 + 6 samples, batch 4): log, pre-training switch, checkpoint, bit-exact resume of
the inputs, the batch against the pieces the project had before, and the DensePose branch."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _options(root, **kw):
    from danet_densepose2smpl_amd.config import cfg
    o = types.SimpleNamespace(batch_size=4, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp', num_epochs=3, pretr_step=1,
                              checkpoint_steps=2, summary_steps=1, num_workers=2, seed=3, shuffle_train=True, time_to_run=None, resume=None,
                              pretrained_checkpoint=None, log_dir=os.path.join(root, 'log'), checkpoint_dir=os.path.join(root, 'ck'),
                              heatmap_size=cfg.DANET.HEATMAP_SIZE, img_res=cfg.DANET.INIMG_SIZE)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _trainer(o):
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    torch.manual_seed(0)
    return Trainer(o)


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """Three steps of fit (one batch per epoch: 6 // 4), every step's in_dict and losses kept."""
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    from danet_densepose2smpl_amd.trainer import Trainer
    root = str(tmp_path_factory.mktemp('fit'))
    o = _options(root)
    ds, paths = datasets.synthetic_mixed_dataset(o, os.path.join(root, 'data'), 6, 6, seed=5)
    tr = _trainer(o)
    fits = FitsDict(o, ds, paths['final_fits_dir'], paths['static_fits_dir'], tr.device)
    steps = []
    n = tr.fit(ds, fits, o, on_step=lambda s, d, l: steps.append((s, Trainer._clone_batch(d), {k: float(v.detach()) for k, v in l.items()})))
    torch.cuda.synchronize()
    return types.SimpleNamespace(o=o, ds=ds, paths=paths, trainer=tr, fits=fits, steps=steps, n=n, root=root)


def test_fit_logs_switches_out_of_pretraining_and_checkpoints(run):
    assert run.n == 3 and [s for s, _, _ in run.steps] == [1, 2, 3] and run.trainer.step_count == 3
    lines = [json.loads(l) for l in open(os.path.join(run.o.log_dir, 'train_log.jsonl'))]
    assert [l['step'] for l in lines] == [1, 2, 3] and [l['epoch'] for l in lines] == [0, 1, 2]
    for l in lines:
        vals = [v for k, v in l.items() if k.startswith('loss_')]
        assert len(vals) >= 5 and np.isfinite(vals).all()
    regr = {'loss_smpl_pose', 'loss_smpl_betas', 'loss_smpl_verts', 'loss_keypoints_2d', 'loss_keypoints_3d', 'loss_cam'}
    assert not (regr & set(lines[0])) and regr <= set(lines[1]) and regr <= set(lines[2])
    assert 'loss_loss_U' in lines[0] and 'loss_loss_Udp' in lines[0]      # ('loss_{}'.format(key), as train/trainer.py:221)
    assert [d['pretrain_mode'] for _, d, _ in run.steps] == [True, False, False]
    assert sorted(os.listdir(run.o.checkpoint_dir)) == ['step_00000002.pt']
    ck = torch.load(os.path.join(run.o.checkpoint_dir, 'step_00000002.pt'), weights_only=True)
    assert ck['total_step_count'] == 2 and ck['epoch'] == 1 and ck['batch_idx'] == 1 and ck['batch_size'] == 4
    assert sorted(ck['dataset_perm']) == list(range(6))


def _same(a, b, path=''):
    assert set(a) == set(b), path
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), path + k
        elif isinstance(a[k], dict):
            _same(a[k], b[k], path + k + '.')
        else:
            assert a[k] == b[k], path + k


def test_resumed_run_builds_the_same_inputs_bit_for_bit(run):
    """The inputs, not the losses: those are not bit-stable (tools/noise_probe.py)."""
    from danet_densepose2smpl_amd.trainer import Trainer
    o = _options(run.root, resume=os.path.join(run.o.checkpoint_dir, 'step_00000002.pt'), log_dir=os.path.join(run.root, 'log2'),
                 checkpoint_dir=os.path.join(run.root, 'ck2'))
    tr = _trainer(o)
    steps = []
    n = tr.fit(run.ds, run.fits, o, on_step=lambda s, d, l: steps.append((s, Trainer._clone_batch(d))))
    torch.cuda.synchronize()
    assert n == 1 and steps[0][0] == 3 and tr.step_count == 3
    _same(steps[0][1], run.steps[2][1])
    # the resumed parameters are the checkpoint's: the first resumed step starts from where the uninterrupted run's third did
    assert [json.loads(l)['step'] for l in open(os.path.join(o.log_dir, 'train_log.jsonl'))] == [3]


def _ulp(got, want, what, ulps=1):
    got, want = got.cpu().numpy(), want.cpu().numpy().astype(np.float32)
    assert got.shape == want.shape, what
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want))).all(), what


def test_batch_equals_the_pieces_the_project_had_before(run):
    """One batch through datasets.collate / to_device / FitsDict / prepare_batch against augment.rgb_processing, the three
    *_processing functions and prepare_batch on the same samples and parameters."""
    from danet_densepose2smpl_amd import augment, constants, datasets
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    tr, ds = run.trainer, run.ds
    items = [ds.get(i, datasets.sample_rng(9, 0, i)) for i in range(4)]
    assert {it['dataset_name'] for it in items} == {'h36m', 'dp_coco'}
    new = tr.build_in_dict(datasets.collate(items, 224), run.fits, 'h36m_dp')
    torch.cuda.synchronize()
    B = 4
    col = lambda k: torch.from_numpy(np.stack([np.asarray(it[k], np.float64) for it in items]))          # noqa: E731
    center, scale, rot, flip, pn = col('_center'), col('scale'), col('_rot'), col('is_flipped'), col('pn')
    H, W = max(it['img_raw'].shape[0] for it in items), max(it['img_raw'].shape[1] for it in items)
    raw = np.zeros((B, H, W, 3), np.uint8)                                     # evaluate.collate's layout
    for b, it in enumerate(items):
        raw[b, :it['img_raw'].shape[0], :it['img_raw'].shape[1]] = it['img_raw']
    raw = torch.from_numpy(raw).permute(0, 3, 1, 2)
    want64 = augment.rgb_processing(raw.double(), center, scale, rot, flip, pn, res=224)
    d = lambda t: t.to(DEV)                                                    # noqa: E731
    old_img = augment.rgb_processing(d(raw).float(), d(center), d(scale), d(rot), d(flip), d(pn), res=224).float()
    e_new = float((new['img'].double().cpu() - want64).abs().max())
    e_old = float((old_img.double().cpu() - want64).abs().max())
    print('in_dict img: e_new %.3e e_old %.3e' % (e_new, e_old))
    assert e_new <= 2 * e_old, (e_new, e_old)
    kp = augment.j2d_processing(col('keypoints'), center, scale, rot, flip)
    sk = augment.j2d_processing(col('smpl_2dkps'), center, scale, rot, torch.zeros(B)).numpy()
    sk[sk[:, :, 2] == 0] = 0
    fl = sk[:, constants.SMPL_JOINTS_FLIP_PERM].copy()
    fl[:, :, 0] = -fl[:, :, 0]
    sk = torch.from_numpy(np.where(flip.numpy().reshape(B, 1, 1) > 0, fl, sk))
    names = [it['dataset_name'] for it in items]
    stored = np.stack([FitsDict.read(n, run.paths['final_fits_dir'], run.paths['static_fits_dir'])[0][it['sample_index']] for n, it in zip(names, items)])
    rot32 = rot.float().double()                                               # the fits are asked with the batch's float32 rot_angle
    old_batch = {'img': old_img, 'keypoints': d(kp), 'pose': d(augment.pose_processing(col('pose'), rot, flip)), 'betas': d(col('betas').float()),
                 'pose_3d': d(augment.j3d_processing(col('pose_3d'), rot, flip)), 'has_smpl': d(col('has_smpl').float()),
                 'has_pose_3d': d(col('has_pose_3d').float()), 'has_dp': d(col('has_dp').float()), 'smpl_2dkps': d(sk.float()),
                 'has_iuv_dataset': d(torch.tensor([n != 'dp_coco' for n in names]).float()),
                 'dp_dict': {k: d(torch.from_numpy(np.stack([it['dp_dict'][k] for it in items]))) for k in items[0]['dp_dict']}}
    old_batch['valid_fit'] = old_batch['has_smpl'] > 0
    with tr._on_stream():
        old = tr.prepare_batch(old_batch, d(augment.pose_processing(torch.from_numpy(stored[:, :72]), rot32, flip)), d(torch.from_numpy(stored[:, 72:])))
    torch.cuda.synchronize()
    assert set(new) == set(old) and set(new['dp_dict']) == set(old['dp_dict'])
    for k in ('keypoints', 'pose_3d', 'opt_pose', 'opt_betas', 'has_pose_3d', 'valid_fit', 'has_iuv', 'has_dp'):
        _ulp(new[k], old[k], k)
    for k in ('target_smpl_kps', 'target_verts', 'target_cam'):               # through two SMPL forwards and a least-squares solve
        np.testing.assert_allclose(new[k].cpu().numpy(), old[k].cpu().numpy(), atol=1e-4, rtol=1e-4, err_msg=k)
    for k, v in old['dp_dict'].items():
        if torch.is_tensor(v):
            assert torch.equal(new['dp_dict'][k], v) and new['dp_dict'][k].dtype == v.dtype, k
    assert new['dp_dict']['dp_active'] is True and new['pretrain_mode'] is False and new['vis_on'] is False


def test_dp_coco_sample_reaches_the_has_dp_losses(run):
    with_dp = [(d, l) for _, d, l in run.steps if d['dp_dict']['dp_active']]
    assert with_dp, 'no batch of the run held a dp_coco sample'
    for d, l in with_dp:
        assert float(d['has_dp'].sum()) > 0 and float(d['dp_dict']['body_uv_ann_weights'].sum()) > 0
        assert all(np.isfinite(l[k]) for k in ('loss_Udp', 'loss_Vdp', 'loss_IndexUVdp', 'loss_segAnndp'))
        assert l['loss_IndexUVdp'] > 0 and l['loss_segAnndp'] > 0
    for _, d, l in run.steps:
        if not d['dp_dict']['dp_active']:
            assert l['loss_IndexUVdp'] == 0 and float(d['has_dp'].sum()) == 0
