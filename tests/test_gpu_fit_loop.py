"""The in-loop fit on the GPU (csrc/fit_loop.hip, fit_loop.py, Trainer.fit with options.run_smplify; DESIGN.md 4d "the refresh rule")
against the float64 oracle of fit_loop_oracle.py.

The bound of the stored values is the project's form: compared as rotation matrices (the axis is ill-conditioned near pi, the matrix is
not),

    max |kernel - f64|  <=  4 * max |composed - f64|  +  8 * 2^-23 * max |f64|           (maxima over the batch)

where `composed` is the path the package had before: ops.rotmat_to_angle_axis (fp32) followed by FitsDict.__setitem__.  The measured
ratios are printed and recorded (conftest.record)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import fit_loop_oracle as fo
import kp_fit_oracle as ko
from conftest import record

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
GRID = [(rot, flip) for rot in (0.0, 37.5, -180.0) for flip in (0, 1)]
SHORT = 8


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _stub_fits(table, valid):
    """A FitsDict over one dataset 'x' whose table is given (device tensors)."""
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    f = FitsDict.__new__(FitsDict)
    f.device = table.device
    f.base, f.length = {'x': 0}, {'x': table.shape[0]}
    f.table, f.valid = table, valid
    return f


@pytest.fixture(scope='module')
def ctx(smpl_model):
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL(smpl_model).cuda()
    return {'smpl': smpl, 'fitter': KeypointFitter(smpl), 'm64': ko.model_tensors(smpl_model)}


# ------------------------------------------------------------------------------------------------------------------ (a)
def test_decisions_are_exact():
    from danet_densepose2smpl_amd import fit_loop
    c = fo.decision_case()
    table, valid = _cu(c.table), _cu(c.valid, np.uint8)
    upd = fit_loop.accept(_cu(c.para), _cu(c.e_new), _cu(c.e_old), _cu(c.status_fit, np.int32), _cu(c.status_eval, np.int32), _cu(c.has_smpl),
                          _cu(c.rows, np.int64), _cu(c.rot_flip, np.float64), _cu(c.kp), table, valid, float(c.tau))
    torch.cuda.synchronize()
    upd, table, valid = upd.cpu().numpy(), table.cpu().numpy(), valid.cpu().numpy()
    e_upd, e_table, e_valid = fo.decide(c.para, c.e_new, c.e_old, c.status_fit, c.status_eval, c.has_smpl, c.rows, c.rot_flip, c.kp, c.table, c.valid, c.tau)
    print('updated %s' % dict(zip(c.names, upd.tolist())), flush=True)
    assert upd.dtype == np.int32 and upd.tolist() == e_upd.tolist() == c.expect.tolist()
    hit = sorted(set(c.rows[e_upd > 0].tolist()))
    keep = np.setdiff1d(np.arange(c.table.shape[0]), hit)
    assert np.array_equal(table[keep].view(np.uint32), c.table[keep].view(np.uint32))            # bit for bit
    assert np.array_equal(valid[keep], c.valid[keep])
    assert np.array_equal(valid, e_valid) and valid[[0, 39]].tolist() == [1, 0]                  # one on each side of tau * sum c^2
    assert np.array_equal(table[hit][:, 72:], e_table[hit][:, 72:])
    got, want = ko.rodrigues(table[hit][:, :72].reshape(-1, 24, 3)), ko.rodrigues(e_table[hit][:, :72].reshape(-1, 24, 3))
    # the stored fp32 pose is the oracle's rounded once: half an ulp of a component below 4 is 2^-22 = 2 EPS32, on three components a
    # matrix moves by at most sqrt(3) * 2 EPS32 = 3.5 EPS32; 16 leaves room for a differently rounded last place (the bound against the
    # composed path is test_stored_values')
    assert np.abs(got - want).max() <= 16 * EPS32


def test_a_row_outside_the_table_is_never_written():
    from danet_densepose2smpl_amd import fit_loop
    c = fo.decision_case()
    rows = c.rows.copy()
    rows[0], rows[12] = 40, -1
    table, valid = _cu(c.table), _cu(c.valid, np.uint8)
    guard = torch.cat([table, torch.full((2, 82), 7.0, device='cuda')])                           # what lies behind the table
    upd = fit_loop.accept(_cu(c.para), _cu(c.e_new), _cu(c.e_old), _cu(c.status_fit, np.int32), _cu(c.status_eval, np.int32), _cu(c.has_smpl),
                          _cu(rows, np.int64), _cu(c.rot_flip, np.float64), _cu(c.kp), guard[:40], valid, float(c.tau))
    torch.cuda.synchronize()
    e_upd, e_table, e_valid = fo.decide(c.para, c.e_new, c.e_old, c.status_fit, c.status_eval, c.has_smpl, rows, c.rot_flip, c.kp, c.table, c.valid, c.tau)
    assert upd.cpu().numpy().tolist() == e_upd.tolist() and e_upd[0] == 0 and e_upd[12] == 0
    assert (guard[40:] == 7.0).all() and np.array_equal(valid.cpu().numpy(), e_valid)
    keep = np.setdiff1d(np.arange(40), c.rows[e_upd > 0])
    assert np.array_equal(guard[:40].cpu().numpy()[keep].view(np.uint32), c.table[keep].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ (b), (c)
def stored_case(B, seed):
    """B fitted rows with rotations rodrigues(0.2 randn), one joint at the identity and one at angle pi - 1e-3 (the global orientation
    among them as b runs), the augmentation grid cycling over the samples, distinct table rows."""
    rng = np.random.default_rng(seed)
    pose = rng.normal(0, 0.2, (B, 24, 3))
    for b in range(B):
        axis = rng.normal(0, 1, 3)
        pose[b, b % 24] = axis / np.linalg.norm(axis) * (np.pi - 1e-3)
        pose[b, (b + 5) % 24] = 0.0
    para = ko.make_para(B, seed + 1).astype(np.float64)
    para[:, 13:] = ko.rodrigues(pose).reshape(B, 216)
    para = para.astype(np.float32)
    grid = [GRID[(b + seed) % len(GRID)] for b in range(B)]
    rot_flip = np.array(grid, np.float64)
    N = B + 7
    rows = rng.permutation(N)[:B].astype(np.int64)
    table = rng.normal(0, 0.3, (N, 82)).astype(np.float32)
    return types.SimpleNamespace(B=B, N=N, para=para, rot_flip=rot_flip, rows=rows, table=table, valid=np.zeros(N, np.uint8),
                                 kp=np.ones((B, 49, 3), np.float32))


def _store(c):
    """-> (table after the kernel, table after the composed path, the two FitsDict stubs), every sample accepted."""
    from danet_densepose2smpl_amd import fit_loop, ops
    B = c.B
    dev_para = _cu(c.para)
    fk = _stub_fits(_cu(c.table), _cu(c.valid, np.uint8))
    upd = fit_loop.accept(dev_para, _cu(np.full(B, 0.1)), _cu(np.full(B, 1.0)), _cu(np.zeros(B), np.int32), _cu(np.zeros(B), np.int32),
                          _cu(np.zeros(B)), _cu(c.rows, np.int64), _cu(c.rot_flip, np.float64), _cu(c.kp), fk.table, fk.valid, 0.002)
    assert upd.cpu().numpy().tolist() == [1] * B
    fc = _stub_fits(_cu(c.table), _cu(c.valid, np.uint8))
    aa = ops.rotmat_to_angle_axis(dev_para[:, 13:].reshape(B * 24, 3, 3)).view(B, 72)
    fc[(['x'] * B, c.rows, c.rot_flip[:, 0], c.rot_flip[:, 1], np.ones(B))] = (aa, dev_para[:, 3:13])
    torch.cuda.synchronize()
    return fk, fc


def _mats(pose):
    return ko.rodrigues(np.asarray(pose, np.float64).reshape(-1, 24, 3))


@pytest.mark.parametrize('B', [1, 65])
def test_stored_values(B):
    worst = None
    for seed in (range(len(GRID)) if B == 1 else (0,)):                       # B = 1: every cell of the grid, one launch each
        c = stored_case(B, seed)
        fk, fc = _store(c)
        want = np.stack([fo.stored_row(c.para[b], c.rot_flip[b, 0], c.rot_flip[b, 1] != 0) for b in range(B)])
        got, comp = fk.table.cpu().numpy()[c.rows], fc.table.cpu().numpy()[c.rows]
        assert np.array_equal(got[:, 72:].view(np.uint32), c.para[:, 3:13].view(np.uint32))      # betas bit for bit
        R64 = _mats(want[:, :72])
        err, err_c = np.abs(_mats(got[:, :72]) - R64).max(), np.abs(_mats(comp[:, :72]) - R64).max()
        bound = 4.0 * err_c + 8.0 * EPS32 * np.abs(R64).max()
        print('stored values B=%d seed=%d (rot, flip of sample 0: %s): kernel %.3g composed %.3g ratio %.3g bound %.3g'
              % (B, seed, c.rot_flip[0].tolist(), err, err_c, err / max(err_c, 1e-300), bound), flush=True)
        record('fit_loop_stored_values_B%d_seed%d' % (B, seed), {'err': float(err), 'err_composed': float(err_c), 'bound': float(bound)})
        assert err <= bound
        rest = np.setdiff1d(np.arange(c.N), c.rows)
        assert np.array_equal(fk.table.cpu().numpy()[rest].view(np.uint32), c.table[rest].view(np.uint32))
        worst = max(worst or 0.0, err / max(err_c, 1e-300))
    print('stored values B=%d: largest kernel / composed ratio %.3g' % (B, worst), flush=True)


def test_round_trip_returns_the_fitted_rotations():
    c = stored_case(65, 0)
    fk, fc = _store(c)
    key = (['x'] * c.B, c.rows, c.rot_flip[:, 0], c.rot_flip[:, 1])
    pose_k, betas_k = fk[key]
    pose_c, _ = fc[key]
    torch.cuda.synchronize()
    R64 = c.para[:, 13:].astype(np.float64).reshape(c.B, 24, 3, 3)
    err, err_c = np.abs(_mats(pose_k.cpu().numpy()) - R64).max(), np.abs(_mats(pose_c.cpu().numpy()) - R64).max()
    bound = 4.0 * err_c + 8.0 * EPS32 * np.abs(R64).max()
    print('round trip: kernel %.3g composed %.3g ratio %.3g bound %.3g' % (err, err_c, err / max(err_c, 1e-300), bound), flush=True)
    record('fit_loop_round_trip', {'err': float(err), 'err_composed': float(err_c), 'bound': float(bound)})
    assert err <= bound
    assert np.array_equal(betas_k.cpu().numpy().view(np.uint32), c.para[:, 3:13].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ (d)
def _in_dict(para_label, kp):
    """The label rows [B,229] as the in_dict of a step carries them (augmented frame)."""
    from danet_densepose2smpl_amd import ops
    B = para_label.shape[0]
    return {'keypoints': kp, 'target_cam': para_label[:, :3].contiguous(), 'opt_betas': para_label[:, 3:13].contiguous(),
            'opt_pose': ops.rotmat_to_angle_axis(para_label[:, 13:].reshape(B * 24, 3, 3)).view(B, 72)}


def test_refresh_end_to_end_on_the_recovery_case(ctx):
    from danet_densepose2smpl_amd.fit_loop import InLoopFit
    init, kp, _ = ko.recovery_case(ctx['m64'])
    init, kp = np.concatenate([init, init]), np.concatenate([kp, kp])                # four samples, the second pair with ground truth
    B, N = 4, 11
    has_smpl = np.array([0, 0, 1, 1], np.float32)
    rows = np.array([9, 2, 5, 0], np.int64)
    rot_flip = np.array([[37.5, 1], [0, 0], [-180, 0], [12, 1]], np.float64)
    rng = np.random.default_rng(1)
    table0, valid0 = rng.normal(0, 0.3, (N, 82)).astype(np.float32), np.zeros(N, np.uint8)
    fits = _stub_fits(_cu(table0), _cu(valid0, np.uint8))
    loop = InLoopFit(ctx['smpl'], fits, fitter=ctx['fitter'])
    dinit, dkp = _cu(init), _cu(kp)
    st = loop.refresh(dinit, _in_dict(dinit, dkp), _cu(rows, np.int64), _cu(rot_flip, np.float64), _cu(has_smpl))
    torch.cuda.synchronize()
    upd, e_old, e_new = st['updated'].cpu().numpy(), st['e_old'].cpu().numpy(), st['e_new'].cpu().numpy()
    print('refresh: updated %s e_old %s e_new %s ratio %s' % (upd.tolist(), e_old.tolist(), e_new.tolist(), (e_new / e_old).tolist()), flush=True)
    assert st['eligible'].cpu().numpy().tolist() == [True, True, False, False]
    assert upd.tolist() == [1, 1, 0, 0]                                               # every eligible row, no other
    table, valid = fits.table.cpu().numpy(), fits.valid.cpu().numpy()
    rest = np.setdiff1d(np.arange(N), rows[:2])
    assert np.array_equal(table[rest].view(np.uint32), table0[rest].view(np.uint32)) and np.array_equal(valid[rest], valid0[rest])
    assert valid[rows[:2]].tolist() == [int(float(e) < float(np.float32(loop.tau)) * 49.0) for e in e_new[:2]]
    # the rows read back through the fetch, with the fit's camera, score below the stored label on the same keypoints
    pose, betas = fits[(['x'] * 2, rows[:2], rot_flip[:2, 0], rot_flip[:2, 1])]
    para_fit = ctx['fitter'].fit(dinit[:2], dkp[:2])
    from danet_densepose2smpl_amd import ops
    back = torch.cat([para_fit[:, :3], betas, ops.batch_rodrigues(pose).view(2, 216)], dim=1)
    assert torch.equal(betas, para_fit[:, 3:13])
    _, ev = ctx['fitter'].fit(back, dkp[:2], return_history=True, stages=())
    e_back = ev['history'][:, 0].cpu().numpy()
    print('refresh: E of the rows read back %s (E_new %s, E_old %s)' % (e_back.tolist(), e_new[:2].tolist(), e_old[:2].tolist()), flush=True)
    record('fit_loop_refresh_recovery', {'e_old': e_old.tolist(), 'e_new': e_new.tolist(), 'e_back': e_back.tolist()})
    assert (ev['status'].cpu().numpy() == 0).all() and (e_back < e_old[:2]).all()


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_refresh_is_reproducible_capturable_and_a_batch_is_its_rows(ctx):
    from danet_densepose2smpl_amd.fit_loop import InLoopFit
    B, N = 5, 9
    star = ko.make_para(B, 31)
    init, kp = _cu(ko.perturb(star, 32, pose_sigma=0.1, shift=0.03, scale=1.05)), _cu(ko.keypoints_of(ctx['m64'], star))
    rng = np.random.default_rng(2)
    table0, valid0 = _cu(rng.normal(0, 0.3, (N, 82))), _cu(np.zeros(N), np.uint8)
    rows = _cu(np.array([4, 0, 8, 3, 6]), np.int64)
    rot_flip = _cu(np.array([GRID[b] for b in range(B)]), np.float64)
    has_smpl = _cu(np.zeros(B))
    in_dict = _in_dict(init, kp)

    def run(sel=slice(None)):
        fits = _stub_fits(table0.clone(), valid0.clone())
        loop = InLoopFit(ctx['smpl'], fits, fitter=ctx['fitter'], iters=SHORT)
        st = loop.refresh(init[sel], {k: v[sel] for k, v in in_dict.items()}, rows[sel], rot_flip[sel], has_smpl[sel])
        return fits, st
    f1, s1 = run()
    f2, s2 = run()
    torch.cuda.synchronize()
    assert int(s1['updated'].sum()) == B                                           # eight steps already halve the energy
    assert torch.equal(f1.table, f2.table) and torch.equal(f1.valid, f2.valid) and torch.equal(s1['updated'], s2['updated'])
    assert torch.equal(s1['e_new'], s2['e_new']) and not torch.equal(f1.table, table0)
    # five batches of one
    fits = _stub_fits(table0.clone(), valid0.clone())
    loop = InLoopFit(ctx['smpl'], fits, fitter=ctx['fitter'], iters=SHORT)
    for b in range(B):
        sel = slice(b, b + 1)
        loop.refresh(init[sel], {k: v[sel] for k, v in in_dict.items()}, rows[sel], rot_flip[sel], has_smpl[sel])
    assert torch.equal(fits.table, f1.table) and torch.equal(fits.valid, f1.valid)
    # captured and replayed
    fits = _stub_fits(table0.clone(), valid0.clone())
    loop = InLoopFit(ctx['smpl'], fits, fitter=ctx['fitter'], iters=SHORT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            loop.refresh(init, in_dict, rows, rot_flip, has_smpl)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = loop.refresh(init, in_dict, rows, rot_flip, has_smpl)
    for _ in range(2):
        fits.table.copy_(table0)
        fits.valid.copy_(valid0)
        st['updated'].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(fits.table, f1.table) and torch.equal(fits.valid, f1.valid) and torch.equal(st['updated'], s1['updated'])
        assert torch.equal(st['e_new'], s1['e_new']) and torch.equal(st['e_old'], s1['e_old'])
    del g


# ------------------------------------------------------------------------------------------------------------------ (f)
IN_DICT_KEYS = {'img', 'opt_pose', 'opt_betas', 'keypoints', 'pose_3d', 'has_pose_3d', 'valid_fit', 'has_iuv', 'has_dp', 'target_smpl_kps',
                'target_verts', 'target_cam', 'vis_on', 'pretrain_mode', 'dp_dict'}
FIT_KEYS = {'fit_eligible', 'fit_updated', 'fit_e_old', 'fit_e_new'}


def _options(root, tag, **kw):
    from danet_densepose2smpl_amd.config import cfg
    o = types.SimpleNamespace(batch_size=4, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp', num_epochs=4, pretr_step=1,
                              checkpoint_steps=2, summary_steps=1, num_workers=2, seed=3, shuffle_train=True, time_to_run=None, resume=None,
                              pretrained_checkpoint=None, log_dir=os.path.join(root, 'log_' + tag), checkpoint_dir=os.path.join(root, 'ck_' + tag),
                              heatmap_size=cfg.DANET.HEATMAP_SIZE, img_res=cfg.DANET.INIMG_SIZE, graph=False)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.config import reset_cfg
    reset_cfg()
    root = str(tmp_path_factory.mktemp('fitloop'))
    ds, paths = datasets.synthetic_mixed_dataset(_options(root, 'data'), os.path.join(root, 'data'), 6, 6, seed=5)
    return types.SimpleNamespace(root=root, ds=ds, paths=paths)


def _fit(world, tag, **kw):
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    o = _options(world.root, tag, **kw)
    fits = FitsDict(o, world.ds, world.paths['final_fits_dir'], world.paths['static_fits_dir'], torch.device('cuda'))
    r = types.SimpleNamespace(o=o, fits=fits, table0=fits.table.clone(), valid0=fits.valid.clone(), keys=[], pretrain=[])
    torch.manual_seed(0)
    tr = Trainer(o)

    def on_step(s, d, l):
        r.keys.append(set(d))
        r.pretrain.append(d['pretrain_mode'])
    r.n = tr.fit(world.ds, fits, o, on_step=on_step)
    torch.cuda.synchronize()
    r.stats = dict(tr.fit_stats)
    r.log = [json.loads(ln) for ln in open(os.path.join(o.log_dir, 'train_log.jsonl'))]
    tr.drop_graph()
    return r


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_trainer_fit_refreshes_the_table(world, graph):
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    r = _fit(world, 'on_graph' if graph else 'on_eager', run_smplify=True, graph=graph)
    assert r.n == 4 and r.pretrain == [True, False, False, False]
    assert r.stats == ({'eager_steps': 3, 'replayed_steps': 1, 'captures': 1} if graph else {'eager_steps': 4, 'replayed_steps': 0, 'captures': 0})
    assert all(k == IN_DICT_KEYS | {'fit_rows', 'fit_rot_flip', 'fit_has_smpl'} for k in r.keys)
    fits = r.fits
    h, dp = (slice(fits.base[n], fits.base[n] + fits.length[n]) for n in ('h36m', 'dp_coco'))
    assert torch.equal(fits.table[h], r.table0[h]) and torch.equal(fits.valid[h], r.valid0[h])
    assert [l['step'] for l in r.log] == [1, 2, 3, 4]
    assert not (FIT_KEYS & set(r.log[0]))                                           # the pretrain step
    print('fit_* lines: %s' % [{k: l[k] for k in sorted(FIT_KEYS)} for l in r.log[1:]], flush=True)
    for l in r.log[1:]:
        assert FIT_KEYS <= set(l) and 0 <= l['fit_updated'] <= l['fit_eligible'] <= 4
        if l['fit_eligible'] == 0:
            assert l['fit_e_old'] is None and l['fit_e_new'] is None
    changed = int((fits.table[dp] != r.table0[dp]).any(dim=1).sum())
    assert changed <= sum(l['fit_updated'] for l in r.log[1:])
    flags = int((fits.valid[dp] != r.valid0[dp]).sum())
    assert flags <= sum(l['fit_updated'] for l in r.log[1:])
    # the newest state lies beside the checkpoints and a fresh store reads it back
    names = sorted(os.listdir(r.o.checkpoint_dir))
    assert {'h36m_fits.npy', 'h36m_valid_fit.npy', 'dp_coco_fits.npy', 'dp_coco_valid_fit.npy', 'step_00000002.pt', 'step_00000004.pt'} <= set(names)
    fresh = FitsDict(r.o, world.ds, world.paths['final_fits_dir'], world.paths['static_fits_dir'], torch.device('cuda'))
    assert fresh.load_state(r.o.checkpoint_dir) == ['dp_coco', 'h36m']
    assert torch.equal(fresh.table, fits.table) and torch.equal(fresh.valid, fits.valid)


def test_trainer_fit_with_the_option_off_is_the_parents(world):
    r = _fit(world, 'off')
    assert r.n == 4 and all(k == IN_DICT_KEYS for k in r.keys)
    assert torch.equal(r.fits.table, r.table0) and torch.equal(r.fits.valid, r.valid0)
    assert all(not (FIT_KEYS & set(l)) for l in r.log) and len(r.log) == 4
    assert not [n for n in os.listdir(r.o.checkpoint_dir) if n.endswith('.npy')]
