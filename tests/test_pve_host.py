"""Host-side checks of the validation / PVE feature: the numpy oracle of the PVE rule (tests/mesh_eval_oracle.py) against golden g27
(the reference's reconstruction_error on float64), the test_steps schedule, the new options' defaults and fit's argument check."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import golden
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_eval_oracle as mo    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G27_CASES = ['v6890', 'v257', 'v255', 'v256', 'v4', 'mirror', 'similarity', 'coplanar', 'identical']


def test_g27_holds_every_case_of_the_rule():
    g = golden('g27_pve')
    assert [str(c) for c in g['cases']] == G27_CASES
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g27_pve.npz')) < 512 * 1024
    for c in G27_CASES:
        p, t, w = g[c + '_pred'], g[c + '_gt'], g[c + '_pelvis_row']
        assert p.dtype == t.dtype == w.dtype == np.float32 and p.shape == t.shape and w.shape == (p.shape[1],)
        assert g[c + '_pve'].dtype == np.float64 and g[c + '_pve'].shape == g[c + '_pa_pve'].shape == (p.shape[0],)
        assert abs(float(w.astype(np.float64).sum()) - 1) < 1e-6 and (w >= 0).all()
    assert g['v6890_pred'].shape == (2, 6890, 3)
    # what the cases are there for
    assert (g['similarity_pa_pve'] < 1e-6).all() and (g['similarity_pve'] > 0.1).all()
    assert (g['identical_pve'] == 0).all() and (g['identical_pa_pve'] < 1e-12).all()
    X1 = g['mirror_pred'].astype(np.float64) - g['mirror_pred'].astype(np.float64).mean(1, keepdims=True)
    X2 = g['mirror_gt'].astype(np.float64) - g['mirror_gt'].astype(np.float64).mean(1, keepdims=True)
    for a, b in zip(X1, X2):
        U, _, Vh = np.linalg.svd(a.T @ b)
        assert np.linalg.det(U @ Vh) < 0                                  # the unconstrained optimum is a reflection
    cp = g['coplanar_pred'].astype(np.float64)
    sv = np.linalg.svd(cp[0] - cp[0].mean(0), compute_uv=False)
    assert sv[2] < 1e-6 * sv[1]                                           # rank 2 (to the float32 rounding of the stored points)


@pytest.mark.parametrize('case', G27_CASES)
def test_oracle_against_g27(case):
    g = golden('g27_pve')
    pve, pa = mo.vertex_errors(g[case + '_pred'], g[case + '_gt'], g[case + '_pelvis_row'])
    print(case, 'pve', pve, g[case + '_pve'], 'pa_pve', pa, g[case + '_pa_pve'])
    # the zero cases (identical: both; similarity: PA-PVE ~ 1e-7, the float32 rounding of the stored points) get an absolute bound
    np.testing.assert_allclose(pve, g[case + '_pve'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(pa, g[case + '_pa_pve'], rtol=1e-9, atol=1e-12)


def test_oracle_is_invariant_where_the_rule_says_so():
    rng = np.random.default_rng(0)
    p, t = rng.normal(size=(2, 40, 3)), rng.normal(size=(2, 40, 3))
    w = rng.random(40)
    w /= w.sum()
    pve, pa = mo.vertex_errors(p, t, w)
    pve2, pa2 = mo.vertex_errors(p + np.array([5.0, -2.0, 1.0]), t - 3.0, w)                  # each mesh is centred at its own pelvis
    np.testing.assert_allclose(pve2, pve, rtol=1e-12)
    np.testing.assert_allclose(pa2, pa, rtol=1e-10)
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    np.testing.assert_allclose(mo.vertex_errors(2.5 * p @ R.T, t, w)[1], pa, rtol=1e-10)      # PA-PVE ignores a similarity transform
    scale, Rr, _ = mo.similarity_transform(p[0], p[0] * np.array([-1.0, 1, 1]))
    assert abs(np.linalg.det(Rr) - 1) < 1e-12


def test_val_due_schedule():
    from danet_densepose2smpl_amd.evaluate import val_due
    steps = range(0, 13)
    assert [s for s in steps if val_due(s, 0)] == [] and [s for s in steps if val_due(s, None)] == []
    assert [s for s in steps if val_due(s, 4)] == [4, 8, 12]                                  # base_trainer.py:90, never before a step ran
    assert [s for s in steps if val_due(s, 1)] == list(range(1, 13))
    assert [s for s in steps if val_due(s, 1000)] == []


def test_train_tool_defaults_keep_todays_behaviour():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train as train_tool
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    a = train_tool.build_parser().parse_args(['--name', 'x'])
    assert a.test_steps == 0 and a.eval_pve is False and a.val_dataset == 'h36m-p2' and a.val_annot is None and a.val_img_dir is None
    assert a.vis_interval == 0 and a.graph is False
    b = train_tool.build_parser().parse_args(['--name', 'x', '--test_steps', '4', '--eval_pve', '--val_dataset', '3dpw'])
    assert b.test_steps == 4 and b.eval_pve is True and b.val_dataset == '3dpw'
    with pytest.raises(SystemExit):
        train_tool.build_parser().parse_args(['--name', 'x', '--val_dataset', 'coco'])


def test_fit_refuses_test_steps_without_a_validation_set(tmp_path):
    """The check comes before anything of the run is touched: no model, no data and no log directory are needed to see it."""
    from danet_densepose2smpl_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    o = types.SimpleNamespace(batch_size=4, test_steps=4, log_dir=str(tmp_path / 'log'), checkpoint_dir=str(tmp_path / 'ck'))
    with pytest.raises(ValueError, match='test_steps'):
        tr.fit(None, None, o)
    assert not os.path.exists(o.log_dir)


def test_evaluator_and_loop_take_the_new_keywords():
    import inspect
    from danet_densepose2smpl_amd import evaluate, ops
    from danet_densepose2smpl_amd.trainer import Trainer
    assert inspect.signature(evaluate.Evaluator.__init__).parameters['eval_pve'].default is False
    assert inspect.signature(evaluate.run_evaluation).parameters['verbose'].default is True
    assert inspect.signature(Trainer.fit).parameters['val'].default is None
    assert callable(Trainer.test) and callable(ops.vertex_eval)


def test_vertex_eval_refuses_cpu_tensors_like_its_neighbours():
    import torch
    from danet_densepose2smpl_amd import ops
    with pytest.raises(RuntimeError, match='run on the GPU only'):
        ops.vertex_eval(torch.zeros(1, 30, 3), torch.zeros(1, 30, 3), torch.zeros(30))


def test_eval_dataset_passes_has_smpl_through(tmp_path):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), 'h36m-p2', n=3, seed=1)
    ds = evaluate.EvalDataset(path, str(tmp_path), 'h36m-p2')
    assert [float(ds[i]['has_smpl']) for i in range(3)] == [1.0, 1.0, 1.0]                   # the file has no such key: all ones
    d = dict(np.load(path, allow_pickle=True))
    d['has_smpl'] = np.array([1, 0, 1])
    ds = evaluate.EvalDataset(d, str(tmp_path), 'h36m-p2')
    batch = evaluate.collate([ds[i] for i in range(3)])
    assert batch['has_smpl'].tolist() == [1.0, 0.0, 1.0]


def test_print_summary_prints_the_two_lines_only_with_the_keys(capsys):
    from danet_densepose2smpl_amd import evaluate
    s = {'mpjpe': 1.0, 'recon_err': 2.0}
    evaluate.print_summary(s)
    plain = capsys.readouterr().out
    assert 'PVE' not in plain
    evaluate.print_summary({**s, 'pve': 3.0, 'pa_pve': 4.0, 'pve_num_samples': 2})
    out = capsys.readouterr().out
    assert out == plain.replace('Reconstruction Error: 2.0\n', 'Reconstruction Error: 2.0\nPVE: 3.0\nPA-PVE: 4.0\n')
