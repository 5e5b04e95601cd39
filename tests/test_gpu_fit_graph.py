"""Trainer.fit with options.graph on the synthetic 'h36m_dp' set (6 + 6 samples, batch 4, pretr_step 3, eight one-batch epochs): two
eager steps and one capture per pretrain_mode phase, replays from there on -- against an eager fit from the same seed."""
import json
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DP = ('loss_Udp', 'loss_Vdp', 'loss_IndexUVdp', 'loss_segAnndp')
IUV_SENTINEL = 'img2iuv.iuv_est.conv1.weight'


def _options(root, tag, **kw):
    from danet_densepose2smpl_amd.config import cfg
    o = types.SimpleNamespace(batch_size=4, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp', num_epochs=8, pretr_step=3,
                              checkpoint_steps=10000, summary_steps=1, num_workers=2, seed=3, shuffle_train=True, time_to_run=None, resume=None,
                              pretrained_checkpoint=None, log_dir=os.path.join(root, 'log_' + tag), checkpoint_dir=os.path.join(root, 'ck_' + tag),
                              heatmap_size=cfg.DANET.HEATMAP_SIZE, img_res=cfg.DANET.INIMG_SIZE, graph=False)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _fit(world, tag, **kw):
    """One fit from the module's seed -> everything the tests look at, per step."""
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    cfg_from_dict({'SOLVER.STEPS': [0, 6]})                     # the step-LR decay lands on step 7 (step_count == 6 when it begins)
    o = _options(world.root, tag, **kw)
    torch.manual_seed(0)
    tr = Trainer(o)
    reg = next(p for _, p in tr.model.iuv2smpl.named_parameters() if p.requires_grad and p.ndim == 4)
    iuv = dict(tr.model.named_parameters())[IUV_SENTINEL]
    r = types.SimpleNamespace(o=o, trainer=tr, steps=[], in_dicts=[], losses=[], lr=[], iuv=[iuv.detach().clone()], reg=[reg.detach().clone()])

    def on_step(s, d, l):
        r.steps.append(s)
        r.in_dicts.append(Trainer._clone_batch(d))
        r.losses.append({k: float(v.detach()) for k, v in l.items()})
        r.lr.append(float(tr.optimizer.param_groups[0]['lr']))
        r.iuv.append(iuv.detach().clone())
        r.reg.append(reg.detach().clone())
    r.n = tr.fit(world.ds, world.fits, o, on_step=on_step)
    torch.cuda.synchronize()
    r.stats = dict(tr.fit_stats)
    r.log = [json.loads(ln) for ln in open(os.path.join(o.log_dir, 'train_log.jsonl'))]
    tr.drop_graph()
    r.trainer = None
    return r


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    reset_cfg()
    root = str(tmp_path_factory.mktemp('fitgraph'))
    o = _options(root, 'data')
    ds, paths = datasets.synthetic_mixed_dataset(o, os.path.join(root, 'data'), 6, 6, seed=5)
    fits = FitsDict(o, ds, paths['final_fits_dir'], paths['static_fits_dir'], torch.device('cuda'))
    return types.SimpleNamespace(root=root, ds=ds, paths=paths, fits=fits)


@pytest.fixture(scope='module')
def eager(world):
    return _fit(world, 'eager')


@pytest.fixture(scope='module')
def eager2(world):
    """The same eager run again, up to the first replayed step: the run-to-run spread of the losses."""
    return _fit(world, 'eager2', num_epochs=3)


@pytest.fixture(scope='module')
def graphed(world):
    return _fit(world, 'graph', graph=True, checkpoint_steps=6)


def _same(a, b, path=''):
    assert set(a) == set(b), path
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), path + k
        elif isinstance(a[k], dict):
            _same(a[k], b[k], path + k + '.')
        else:
            assert a[k] == b[k], path + k


def test_fit_stats_count_eager_steps_replays_and_captures(eager, graphed):
    assert graphed.n == 8 and graphed.steps == list(range(1, 9))
    assert graphed.stats == {'eager_steps': 4, 'replayed_steps': 4, 'captures': 2}
    assert eager.n == 8 and eager.stats == {'eager_steps': 8, 'replayed_steps': 0, 'captures': 0}


def test_both_runs_see_the_same_inputs_bit_for_bit(eager, graphed):
    for a, b in zip(eager.in_dicts, graphed.in_dicts):
        _same(a, b)


def test_pretrain_mode_switches_after_pretr_step(eager, graphed):
    for r in (eager, graphed):
        assert [d['pretrain_mode'] for d in r.in_dicts] == [True] * 3 + [False] * 5


def test_log_lines_have_the_eager_runs_keys(eager, graphed):
    assert [l['step'] for l in graphed.log] == list(range(1, 9))
    for a, b in zip(eager.log, graphed.log):
        assert set(a) == set(b), a['step']
    for a, b in zip(eager.losses, graphed.losses):
        assert set(a) == set(b)


def test_first_eager_and_first_replayed_step_agree_with_the_eager_run(eager, eager2, graphed):
    """Steps 1 and 3: every loss within three times the spread of two eager runs from the same seed (floor: 1e-6 relative); losses are
    not bit-stable in this project (tools/noise_probe.py)."""
    bad = []
    for s in (1, 3):
        e1, e2, g = eager.losses[s - 1], eager2.losses[s - 1], graphed.losses[s - 1]
        for k in e1:
            spread = max(abs(e1[k] - e2[k]), 1e-6 * abs(e1[k]))
            print('step %d %-22s eager %.8g eager2 %.8g graphed %.8g spread %.3e diff %.3e' % (s, k, e1[k], e2[k], g[k], spread, abs(g[k] - e1[k])))
            if not abs(g[k] - e1[k]) <= 3 * spread:
                bad.append((s, k, e1[k], e2[k], g[k]))
    assert not bad, bad


def test_replayed_steps_update_the_weights_their_phase_trains(graphed):
    changed = lambda seq, s: not torch.equal(seq[s], seq[s - 1])          # noqa: E731  (seq[s]: after step s; seq[0]: initial)
    for s in (3, 6, 7, 8):
        assert changed(graphed.iuv, s), s
    for s in (6, 7, 8):
        assert changed(graphed.reg, s), s
    assert not changed(graphed.reg, 3)                                    # the pretrain-mode graph leaves the regressor alone


def test_lr_decay_on_a_replayed_step_reaches_the_captured_adam(graphed):
    from danet_densepose2smpl_amd.config import cfg
    assert graphed.lr[5] == pytest.approx(cfg.SOLVER.BASE_LR, rel=1e-6)
    assert graphed.lr[7] == pytest.approx(cfg.SOLVER.GAMMA * graphed.lr[5], rel=1e-6)
    # ... and the replayed Adam used it: eight steps in, |m^ / sqrt(v^)| <= 1.04 (Cauchy-Schwarz over the eight gradients with
    # betas 0.9 / 0.999), so an update is at most 1.04 lr -- an Adam still at the undecayed rate would step 1 / GAMMA times as far
    step8 = float((graphed.iuv[8] - graphed.iuv[7]).abs().max())
    step6 = float((graphed.iuv[6] - graphed.iuv[5]).abs().max())
    print('max update step 6 %.3e (lr %.3e), step 8 %.3e (lr %.3e)' % (step6, graphed.lr[5], step8, graphed.lr[7]))
    assert 0 < step8 <= 2 * graphed.lr[7] < step6


def test_resume_inside_phase_two_starts_with_two_eager_steps(world, graphed):
    ck = os.path.join(graphed.o.checkpoint_dir, 'step_00000006.pt')
    assert os.path.isfile(ck)
    r = _fit(world, 'resume', graph=True, resume=ck)
    assert r.n == 2 and r.steps == [7, 8]
    assert r.stats == {'eager_steps': 2, 'replayed_steps': 0, 'captures': 0}
    for a, b in zip(r.in_dicts, graphed.in_dicts[6:8]):
        _same(a, b)


def test_run_without_densepose_datasets_captures_the_four_zero_losses(world, monkeypatch):
    """The synthetic writer produces 'h36m_dp' sets only: TRAIN_SETS is patched so that the run's datasets name no 'dp_coco'."""
    from danet_densepose2smpl_amd import datasets
    monkeypatch.setitem(datasets.TRAIN_SETS, 'h36m_dp', ['h36m', 'coco'])
    r = _fit(world, 'nodp', graph=True, pretr_step=0, num_epochs=3)
    assert r.stats == {'eager_steps': 2, 'replayed_steps': 1, 'captures': 1}
    assert all(r.losses[2][k] == 0.0 for k in DP)
    assert r.losses[2]['loss_IndexUV'] > 0
