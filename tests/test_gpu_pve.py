"""The per-vertex error on the device (csrc/eval_ops.hip vertex_eval_kernel): ops.vertex_eval against golden g27 (the reference's
reconstruction_error in float64) and the numpy oracle of tests/mesh_eval_oracle.py, under graph replay, and inside Evaluator /
run_evaluation (eval_pve).  Tolerances are those the pose_eval tests hold (tests/test_gpu_eval.py:50-51)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import golden, record
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_eval_oracle as mo    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G27_CASES = ['v6890', 'v257', 'v255', 'v256', 'v4', 'mirror', 'similarity', 'coplanar', 'identical']
PVE_TOL = dict(rtol=1e-5)
PA_TOL = dict(rtol=1e-4, atol=1e-6)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _random(B, V, seed):
    rng = np.random.default_rng(seed)
    p = (rng.normal(0, 1, (B, V, 3)) * [0.25, 0.5, 0.15] + rng.normal(0, 0.3, (B, 1, 3))).astype(np.float32)
    g = (p + rng.normal(0, 0.06, p.shape) + rng.normal(0, 0.05, (B, 1, 3))).astype(np.float32)
    w = rng.random(V)
    return p, g, (w / w.sum()).astype(np.float32)


@pytest.mark.parametrize('case', G27_CASES)
def test_vertex_eval_against_golden_g27(case):
    from danet_densepose2smpl_amd import ops
    g = golden('g27_pve')
    pve, pa = ops.vertex_eval(_t(g[case + '_pred']), _t(g[case + '_gt']), _t(g[case + '_pelvis_row']))
    B = g[case + '_pred'].shape[0]
    assert pve.is_cuda and pve.dtype == pa.dtype == torch.float32 and pve.shape == pa.shape == (B,)
    pve, pa = pve.cpu().numpy().astype(np.float64), pa.cpu().numpy().astype(np.float64)
    print(case, 'pve', pve, g[case + '_pve'], 'pa_pve', pa, g[case + '_pa_pve'])
    record('vertex_eval_g27_' + case, {'pve_abs': float(np.abs(pve - g[case + '_pve']).max()), 'pa_pve_abs': float(np.abs(pa - g[case + '_pa_pve']).max())})
    np.testing.assert_allclose(pve, g[case + '_pve'], **PVE_TOL)
    np.testing.assert_allclose(pa, g[case + '_pa_pve'], **PA_TOL)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('V', [4, 255, 256, 257, 6890])
def test_vertex_eval_against_the_oracle(B, V):
    from danet_densepose2smpl_amd import ops
    p, g, w = _random(B, V, seed=100 * B + V)
    e_pve, e_pa = mo.vertex_errors(p, g, w)
    pve, pa = ops.vertex_eval(_t(p), _t(g), _t(w))
    pve, pa = pve.cpu().numpy().astype(np.float64), pa.cpu().numpy().astype(np.float64)
    print('B', B, 'V', V, 'pve rel', np.abs(pve / e_pve - 1).max(), 'pa_pve rel', np.abs(pa / e_pa - 1).max())
    np.testing.assert_allclose(pve, e_pve, **PVE_TOL)
    np.testing.assert_allclose(pa, e_pa, **PA_TOL)


def test_vertex_eval_takes_other_dtypes_and_strides():
    from danet_densepose2smpl_amd import ops
    p, g, w = _random(2, 300, seed=7)
    want = ops.vertex_eval(_t(p), _t(g), _t(w))
    wide = torch.zeros(2, 300, 6, device=DEV, dtype=torch.float64)
    wide[:, :, ::2] = _t(p).double()
    got = ops.vertex_eval(wide[:, :, ::2], _t(g).double(), _t(np.stack([w, w], 1))[:, 0])
    assert all(torch.equal(a, b) for a, b in zip(want, got))


def test_vertex_eval_under_graph_replay():
    from danet_densepose2smpl_amd import ops
    p, g, w = _random(8, 6890, seed=9)
    sp, sg, sw = _t(p), _t(g), _t(w)
    eager = [t.clone() for t in ops.vertex_eval(sp, sg, sw)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.vertex_eval(sp, sg, sw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.vertex_eval(sp, sg, sw)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    p2, g2, _ = _random(8, 6890, seed=10)                        # new inputs through the same static buffers
    sp.copy_(_t(p2))
    sg.copy_(_t(g2))
    graph.replay()
    torch.cuda.synchronize()
    want = ops.vertex_eval(_t(p2), _t(g2), sw)
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    assert not torch.equal(out[0], eager[0])


def test_vertex_eval_refuses_cpu_tensors_and_empty_sizes():
    from danet_densepose2smpl_amd import ops
    p, g, w = _random(2, 8, seed=1)
    with pytest.raises(RuntimeError, match='run on the GPU only'):
        ops.vertex_eval(torch.from_numpy(p), _t(g), _t(w))
    with pytest.raises(RuntimeError, match='run on the GPU only'):
        ops.vertex_eval(_t(p), _t(g), torch.from_numpy(w))
    with pytest.raises(RuntimeError, match='vertex_eval: bad sizes B=0'):
        ops.vertex_eval(torch.zeros(0, 8, 3, device=DEV), torch.zeros(0, 8, 3, device=DEV), _t(w))
    with pytest.raises(RuntimeError, match='vertex_eval: bad sizes B=2 V=0'):
        ops.vertex_eval(torch.zeros(2, 0, 3, device=DEV), torch.zeros(2, 0, 3, device=DEV), torch.zeros(0, device=DEV))
    with pytest.raises(ValueError, match='vertex_eval'):
        ops.vertex_eval(_t(p), _t(g[:, :7]), _t(w))
    # the C entry point itself: null pointers and sizes, nothing launched
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    out = torch.zeros(2, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert L.danet_vertex_eval(_t(p).data_ptr(), None, _t(w).data_ptr(), 2, 8, out.data_ptr(), out.data_ptr(), s) < 0
    assert b'null pointer' in L.danet_last_error()
    assert L.danet_vertex_eval(_t(p).data_ptr(), _t(g).data_ptr(), _t(w).data_ptr(), -1, 8, out.data_ptr(), out.data_ptr(), s) < 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


# ---- Evaluator / run_evaluation ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(4), None, pretrained=False).cuda().eval()


@pytest.fixture
def spy(monkeypatch):
    """Records what the evaluator hands to ops.vertex_eval: the vertices it used."""
    from danet_densepose2smpl_amd import evaluate
    calls, real = [], evaluate.ops.vertex_eval

    def vertex_eval(pred, gt, row):
        calls.append((pred.detach().clone(), gt.detach().clone(), row.detach().clone()))
        return real(pred, gt, row)
    monkeypatch.setattr(evaluate.ops, 'vertex_eval', vertex_eval)
    return calls


def _oracle_of(calls):
    pve, pa = zip(*[mo.vertex_errors(p.cpu().numpy(), g.cpu().numpy(), w.cpu().numpy()) for p, g, w in calls])
    return np.concatenate(pve), np.concatenate(pa)


@pytest.mark.parametrize('name', ['3dpw', 'h36m-p2'])
def test_run_evaluation_with_eval_pve(model, name, tmp_path, capsys, spy):
    from danet_densepose2smpl_amd import evaluate
    n = 6                                                         # a full and a short batch
    path = evaluate.write_synthetic_dataset(str(tmp_path), name, n=n, seed=21)
    ds = evaluate.EvalDataset(path, str(tmp_path), name)
    s = evaluate.run_evaluation(model, name, ds, None, batch_size=4, num_workers=0, log_freq=0, options=types.SimpleNamespace(eval_pve=True))
    printed = capsys.readouterr().out
    V = model.iuv2smpl.smpl.v_template.shape[0]
    assert len(spy) == 2 and [c[0].shape[0] for c in spy] == [4, 2] and spy[0][0].shape[1:] == (V, 3)
    Jr = evaluate.synthetic_h36m_regressor(V)
    assert all(np.array_equal(c[2].cpu().numpy(), Jr[0]) for c in spy)        # the pelvis row of the regressor pose_eval uses
    e_pve, e_pa = _oracle_of(spy)
    assert s['pve_num_samples'] == n and s['pve_per_sample'].shape == s['pa_pve_per_sample'].shape == (n,)
    assert s['pve_per_sample'].dtype == np.float64
    print(name, 'pve', s['pve'], 'pa_pve', s['pa_pve'], 'mpjpe', s['mpjpe'])
    np.testing.assert_allclose(s['pve_per_sample'], e_pve, **PVE_TOL)
    np.testing.assert_allclose(s['pa_pve_per_sample'], e_pa, **PA_TOL)
    assert s['pve'] == float(1000 * s['pve_per_sample'].mean()) and s['pa_pve'] == float(1000 * s['pa_pve_per_sample'].mean())
    lines = printed.splitlines()
    k = lines.index('Reconstruction Error: ' + str(s['recon_err']))
    assert lines[k + 1] == 'PVE: ' + str(s['pve']) and lines[k + 2] == 'PA-PVE: ' + str(s['pa_pve'])
    if name == '3dpw':                                            # the mesh pose_eval was scored against, built once
        b = evaluate.to_device(next(evaluate.iterate_batches(ds, 4)), torch.device(DEV))
        smpl = model.iuv2smpl.smpl
        gv = smpl(global_orient=b['pose'][:, :3], body_pose=b['pose'][:, 3:], betas=b['betas']).vertices
        assert torch.equal(spy[0][1], gv)


def test_has_smpl_zeros_are_not_counted(model, tmp_path, spy):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), 'h36m-p2', n=6, seed=22)
    d = dict(np.load(path, allow_pickle=True))
    on = np.array([1, 0, 1, 1, 0, 1])
    d['has_smpl'] = on
    ds = evaluate.EvalDataset(d, str(tmp_path), 'h36m-p2')
    s = evaluate.run_evaluation(model, 'h36m-p2', ds, None, batch_size=4, num_workers=0, options=types.SimpleNamespace(eval_pve=True), verbose=False)
    e_pve, e_pa = _oracle_of(spy)
    assert s['pve_num_samples'] == 4 and s['num_samples'] == 6 and s['mpjpe_per_sample'].shape == (6,)
    np.testing.assert_allclose(s['pve_per_sample'], e_pve[on > 0], **PVE_TOL)
    np.testing.assert_allclose(s['pa_pve_per_sample'], e_pa[on > 0], **PA_TOL)
    np.testing.assert_allclose(s['pve'], 1000 * e_pve[on > 0].mean(), **PVE_TOL)
    d['has_smpl'] = np.zeros(6)
    s = evaluate.run_evaluation(model, 'h36m-p2', evaluate.EvalDataset(d, str(tmp_path), 'h36m-p2'), None, batch_size=4, num_workers=0,
                                options=types.SimpleNamespace(eval_pve=True), verbose=False)
    assert s['pve_num_samples'] == 0 and not {'pve', 'pa_pve', 'pve_per_sample', 'pa_pve_per_sample'} & set(s)


@pytest.mark.parametrize('name', ['h36m-p2', 'lsp'])
def test_eval_pve_off_changes_nothing(model, name, tmp_path, capsys, spy):
    from danet_densepose2smpl_amd import evaluate
    path = evaluate.write_synthetic_dataset(str(tmp_path), name, n=4, seed=23)
    ds = evaluate.EvalDataset(path, str(tmp_path), name)
    ra, rb = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    a = evaluate.run_evaluation(model, name, ds, ra, batch_size=4, num_workers=0, log_freq=1)                   # never heard of the option
    out_a = capsys.readouterr().out
    b = evaluate.run_evaluation(model, name, ds, rb, batch_size=4, num_workers=0, log_freq=1, options=types.SimpleNamespace(eval_pve=False))
    out_b = capsys.readouterr().out
    assert list(a.keys()) == list(b.keys()) and not any(k.startswith(('pve', 'pa_pve')) for k in b)
    assert out_a == out_b and 'PVE' not in out_b and '*** Final Results ***' in out_b
    fa, fb = np.load(ra), np.load(rb)
    assert fa.files == fb.files and all(fa[k].tobytes() == fb[k].tobytes() and fa[k].dtype == fb[k].dtype for k in fa.files)
    if name == 'lsp':                                             # 'lsp' ignores the switch
        c = evaluate.run_evaluation(model, name, ds, None, batch_size=4, num_workers=0, log_freq=1, options=types.SimpleNamespace(eval_pve=True))
        assert list(c.keys()) == list(a.keys()) and capsys.readouterr().out == out_a
    assert spy == []
    evaluate.run_evaluation(model, name, ds, None, batch_size=4, num_workers=0, verbose=False)
    assert capsys.readouterr().out == ''
