"""Validation inside Trainer.fit (options.test_steps, Trainer.test) on the synthetic 'h36m_dp' set of tests/test_gpu_fit_graph.py (6 + 6
samples, batch 4, pretr_step 3, eight one-batch epochs) with a synthetic 'h36m-p2' validation set of 8 samples, test_steps 4,
checkpoint_steps 4 and eval_pve: the run with validation must be the run without it, eagerly and with graph replay, and the logged numbers
must be those of the weights the checkpoint of that step holds."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
VAL_KEYS = {'val_dataset', 'val_num_samples', 'val_mpjpe', 'val_recon_err', 'val_pve', 'val_pa_pve'}
METRICS = ('mpjpe', 'recon_err', 'pve', 'pa_pve')


def _options(root, tag, **kw):
    from danet_densepose2smpl_amd.config import cfg
    o = types.SimpleNamespace(batch_size=4, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp', num_epochs=8, pretr_step=3,
                              checkpoint_steps=4, summary_steps=1, num_workers=2, seed=3, shuffle_train=True, time_to_run=None, resume=None,
                              pretrained_checkpoint=None, log_dir=os.path.join(root, 'log_' + tag), checkpoint_dir=os.path.join(root, 'ck_' + tag),
                              heatmap_size=cfg.DANET.HEATMAP_SIZE, img_res=cfg.DANET.INIMG_SIZE, graph=False, eval_pve=True)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _fit(world, tag, validate, **kw):
    """One fit from the module's seed -> everything the tests look at, per step."""
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    kw.setdefault('test_steps', 4 if validate else 0)
    o = _options(world.root, tag, **kw)
    torch.manual_seed(0)
    tr = Trainer(o)
    r = types.SimpleNamespace(o=o, steps=[], in_dicts=[], losses=[], modes=[])

    def on_step(s, d, l):
        r.steps.append(s)
        r.in_dicts.append(Trainer._clone_batch(d))
        r.losses.append({k: float(v.detach()) for k, v in l.items()})
        r.modes.append(tr.model.training)
    r.n = tr.fit(world.ds, world.fits, o, on_step=on_step, val=world.val if validate else None)
    torch.cuda.synchronize()
    r.stats = dict(tr.fit_stats)
    r.training_after = tr.model.training
    r.step_count = tr.step_count
    r.log = [json.loads(ln) for ln in open(os.path.join(o.log_dir, 'train_log.jsonl'))]
    tr.drop_graph()
    return r


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from danet_densepose2smpl_amd import datasets, evaluate
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    reset_cfg()
    root = str(tmp_path_factory.mktemp('fitval'))
    o = _options(root, 'data')
    ds, paths = datasets.synthetic_mixed_dataset(o, os.path.join(root, 'data'), 6, 6, seed=5)
    fits = FitsDict(o, ds, paths['final_fits_dir'], paths['static_fits_dir'], torch.device('cuda'))
    vroot = os.path.join(root, 'val')
    val = ('h36m-p2', evaluate.EvalDataset(evaluate.write_synthetic_dataset(vroot, 'h36m-p2', n=8, seed=7), vroot, 'h36m-p2'))
    return types.SimpleNamespace(root=root, ds=ds, paths=paths, fits=fits, val=val)


@pytest.fixture(scope='module')
def plain(world):
    return _fit(world, 'plain', False)


@pytest.fixture(scope='module')
def plain2(world):
    """The same run again: the run-to-run spread of the losses."""
    return _fit(world, 'plain2', False)


@pytest.fixture(scope='module')
def eager_val(world):
    return _fit(world, 'eager_val', True)


@pytest.fixture(scope='module')
def graph_val(world):
    return _fit(world, 'graph_val', True, graph=True)


@pytest.fixture(scope='module')
def graph_val_every(world):
    """Validation after EVERY step of a graphed run: the validations after steps 7 and 8 both follow a replayed optimizer step of one
    capture, the case in which an operand packed for the first would still pass for current at the second."""
    return _fit(world, 'graph_val_every', True, graph=True, test_steps=1, checkpoint_steps=8)


def _same(a, b, path=''):
    assert set(a) == set(b), path
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), path + k
        elif isinstance(a[k], dict):
            _same(a[k], b[k], path + k + '.')
        else:
            assert a[k] == b[k], path + k


def test_log_has_val_keys_exactly_at_steps_4_and_8(plain, eager_val, graph_val):
    assert [l['step'] for l in plain.log] == list(range(1, 9)) and not any(k.startswith('val_') for l in plain.log for k in l)
    for r in (eager_val, graph_val):
        assert [l['step'] for l in r.log] == list(range(1, 9))
        for a, b in zip(plain.log, r.log):
            extra = set(b) - set(a)
            assert set(a) <= set(b) and extra == (VAL_KEYS if b['step'] in (4, 8) else set()), (b['step'], extra)
        for l in (r.log[3], r.log[7]):
            assert l['val_dataset'] == 'h36m-p2' and l['val_num_samples'] == 8
            assert all(np.isfinite(l['val_' + k]) and l['val_' + k] > 0 for k in METRICS)
            print('step', l['step'], {k: l[k] for k in sorted(VAL_KEYS)})


def test_runs_with_and_without_validation_see_the_same_inputs_bit_for_bit(plain, eager_val, graph_val):
    for r in (eager_val, graph_val):
        assert r.n == 8 and r.steps == list(range(1, 9)) and r.step_count == 8
        for a, b in zip(plain.in_dicts, r.in_dicts):
            _same(a, b)


def test_fit_stats_are_those_of_the_runs_without_validation(plain, eager_val, graph_val):
    assert plain.stats == eager_val.stats == {'eager_steps': 8, 'replayed_steps': 0, 'captures': 0}
    assert graph_val.stats == {'eager_steps': 4, 'replayed_steps': 4, 'captures': 2}            # (tests/test_gpu_fit_graph.py, no validation)


def test_losses_stay_within_the_spread_of_two_plain_runs(plain, plain2, eager_val, graph_val):
    """Every loss within three times the spread of two plain runs from the same seed (floor: 1e-6 relative), the criterion of
    test_gpu_fit_graph.test_first_eager_and_first_replayed_step_agree_with_the_eager_run: all 8 steps of the eager run with
    validation (steps 5 - 8 follow the validation after step 4), steps 1 and 3 of the graphed one."""
    bad = []
    for r, name, steps in ((eager_val, 'eager', range(1, 9)), (graph_val, 'graphed', (1, 3))):
        for s in steps:
            e1, e2, g = plain.losses[s - 1], plain2.losses[s - 1], r.losses[s - 1]
            assert set(e1) == set(g)
            for k in e1:
                spread = max(abs(e1[k] - e2[k]), 1e-6 * abs(e1[k]))
                if not abs(g[k] - e1[k]) <= 3 * spread or s in (1, 5, 8):
                    print('%s step %d %-22s plain %.8g plain2 %.8g validated %.8g spread %.3e diff %.3e' % (name, s, k, e1[k], e2[k], g[k], spread, abs(g[k] - e1[k])))
                if not abs(g[k] - e1[k]) <= 3 * spread:
                    bad.append((name, s, k, e1[k], e2[k], g[k]))
    assert not bad, bad


def test_model_is_back_in_training_mode(eager_val, graph_val):
    for r in (eager_val, graph_val):
        assert all(r.modes) and r.training_after


def _fresh(world, r, step, tag):
    """The val_* numbers logged at `step` against run_evaluation on a fresh model loaded from that step's checkpoint.  Tolerance: three
    times the spread of two identical run_evaluation calls on one model, measured here; floor rtol 1e-5."""
    from danet_densepose2smpl_amd import checkpoint, evaluate
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    ck = os.path.join(r.o.checkpoint_dir, 'step_%08d.pt' % step)
    assert os.path.isfile(ck)
    reset_cfg()
    torch.manual_seed(1)
    model = DaNet(r.o, None, pretrained=False).cuda()
    checkpoint.load_pretrained(model, ck, trusted=True)
    model.eval()
    run = lambda: evaluate.run_evaluation(model, world.val[0], world.val[1], None, batch_size=4, num_workers=2, log_freq=0, options=r.o, verbose=False)
    a, b = run(), run()
    logged = r.log[step - 1]
    assert logged['step'] == step and logged['val_num_samples'] == a['num_samples'] == 8
    for k in METRICS:
        tol = max(3 * abs(a[k] - b[k]), 1e-5 * abs(a[k]))
        print('%s step %d %-10s logged %.9g fresh %.9g / %.9g tol %.3e diff %.3e' % (tag, step, k, logged['val_' + k], a[k], b[k], tol, abs(logged['val_' + k] - a[k])))
        assert abs(logged['val_' + k] - a[k]) <= tol, (k, logged['val_' + k], a[k], b[k])


@pytest.mark.parametrize('mode', ['eager', 'graph'])
@pytest.mark.parametrize('step', [4, 8])
def test_logged_numbers_are_those_of_the_checkpointed_weights(world, eager_val, graph_val, mode, step):
    """Freshness: a stale packed weight (the bank of the captured step holds the weights BEFORE the replayed optimizer step) shows
    here.  Step 4 is the first, eager step of the second phase, step 8 a replayed one."""
    r = eager_val if mode == 'eager' else graph_val
    _fresh(world, r, step, mode)
    # ... and the model moved between the two validations: step 8's numbers are not step 4's
    assert any(r.log[7]['val_' + k] != r.log[3]['val_' + k] for k in METRICS)


def test_validation_after_every_replayed_step_is_fresh_too(world, plain, graph_val_every):
    r = graph_val_every
    assert r.stats == {'eager_steps': 4, 'replayed_steps': 4, 'captures': 2} and all(r.modes) and r.training_after
    assert all(VAL_KEYS <= set(l) for l in r.log) and [l['step'] for l in r.log] == list(range(1, 9))
    for a, b in zip(plain.in_dicts, r.in_dicts):
        _same(a, b)
    _fresh(world, r, 8, 'graph, validation after every step')
    assert any(r.log[7]['val_' + k] != r.log[6]['val_' + k] for k in METRICS)


def test_direct_test_call_leaves_batchnorm_statistics_and_mode_alone(world):
    from danet_densepose2smpl_amd import nn as dnn
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    o = _options(world.root, 'direct')
    torch.manual_seed(0)
    tr = Trainer(o)
    bn = next(m for m in tr.model.modules() if isinstance(m, dnn.BatchNorm2d) and m.track_running_stats)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.1)
        bn.num_batches_tracked.fill_(5)
    mean0, count0 = bn.running_mean.clone(), bn.num_batches_tracked.clone()
    sd0 = {k: v.clone() for k, v in tr.model.state_dict().items()}
    tr.model.train()
    out = tr.test(world.val)
    assert set(out) == VAL_KEYS and out['val_num_samples'] == 8 and tr.model.training and tr.step_count == 0
    assert torch.equal(bn.running_mean, mean0) and torch.equal(bn.num_batches_tracked, count0)
    assert all(torch.equal(v, sd0[k]) for k, v in tr.model.state_dict().items())
    tr.model.eval()
    o.eval_pve = False
    out2 = tr.test(world.val, o)
    assert set(out2) == VAL_KEYS - {'val_pve', 'val_pa_pve'} and not tr.model.training
    assert out2['val_mpjpe'] == out['val_mpjpe']                                                  # (infer_net is bit-stable, tests/test_gpu_infer.py)
