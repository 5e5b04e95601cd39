"""CPU-side checks of the in-loop fit (DESIGN.md 4d "the refresh rule"): the float64 oracle of the accept step against itself, the
host pieces of fit_loop.py / fits_dict.py / tools/train.py, and the C boundary."""
import os
import re
import types

import numpy as np
import pytest
import torch

import fit_loop_oracle as fo
import kp_fit_oracle as ko
from conftest import ROOT


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rot', [0.0, 37.5, -180.0])
@pytest.mark.parametrize('flip', [0, 1])
def test_oracle_inverse_undoes_forward(rot, flip):
    rng = np.random.default_rng(11)
    for _ in range(4):
        pose = rng.normal(0, 0.4, 72)
        back = fo.inverse(fo.forward(pose, rot, flip), rot, flip)
        assert np.abs(ko.rodrigues(back.reshape(24, 3)) - ko.rodrigues(pose.reshape(24, 3))).max() <= 1e-12
        assert np.abs(back - pose).max() <= 1e-12


def test_oracle_axis_angle_inverts_rodrigues():
    rng = np.random.default_rng(5)
    aa = rng.normal(0, 0.6, (50, 3))
    aa[0] = 0.0
    aa[1] = np.array([0.6, -0.48, 0.64]) * (np.pi - 1e-3)
    assert np.abs(ko.rodrigues(fo.rotmat_to_aa(ko.rodrigues(aa))) - ko.rodrigues(aa)).max() <= 1e-12
    assert np.abs(fo.rotmat_to_aa(ko.rodrigues(aa)) - aa)[2:].max() <= 1e-12


def test_oracle_decision_table():
    c = fo.decision_case()
    upd, table, valid = fo.decide(c.para, c.e_new, c.e_old, c.status_fit, c.status_eval, c.has_smpl, c.rows, c.rot_flip, c.kp, c.table, c.valid, c.tau)
    assert upd.tolist() == c.expect.tolist(), dict(zip(c.names, upd.tolist()))
    hit = sorted(set(c.rows[upd > 0].tolist()))
    assert hit == [0, 3, 9, 21, 39]
    keep = np.setdiff1d(np.arange(c.table.shape[0]), hit)
    assert np.array_equal(table[keep].view(np.uint32), c.table[keep].view(np.uint32)) and np.array_equal(valid[keep], c.valid[keep])
    assert valid[[3, 9, 21, 0, 39]].tolist() == [1, 1, 0, 1, 0]                        # 0.05, 0.05, 0.2, 0.0979 | 0.0981 against 0.098
    b = c.names.index('dup_b')
    assert np.array_equal(table[21], fo.stored_row(c.para[b], c.rot_flip[b, 0], c.rot_flip[b, 1] != 0).astype(np.float32))
    assert np.array_equal(table[21, 72:], c.para[b, 3:13])
    # a row outside the table is never written
    rows = c.rows.copy()
    rows[0] = 40
    upd2, _, _ = fo.decide(c.para, c.e_new, c.e_old, c.status_fit, c.status_eval, c.has_smpl, rows, c.rot_flip, c.kp, c.table, c.valid, c.tau)
    assert upd2[0] == 0 and upd2[1:].tolist() == c.expect[1:].tolist()


# ---- the host side of the package -----------------------------------------------------------------------------------------------------
def test_refresh_refuses_cpu_tensors_before_the_library_loads(monkeypatch):
    from danet_densepose2smpl_amd import _lib, fit_loop

    def no_lib():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_lib)
    loop = fit_loop.InLoopFit(types.SimpleNamespace(), types.SimpleNamespace(table=torch.zeros(4, 82), valid=torch.zeros(4, dtype=torch.uint8)),
                              fitter=types.SimpleNamespace(sigma=0.1))
    B = 2
    in_dict = {'keypoints': torch.zeros(B, 49, 3), 'target_cam': torch.ones(B, 3), 'opt_betas': torch.zeros(B, 10), 'opt_pose': torch.zeros(B, 72)}
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        loop.refresh(torch.zeros(B, 229), in_dict, torch.zeros(B, dtype=torch.int64), torch.zeros(B, 2, dtype=torch.float64), torch.zeros(B))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        fit_loop.accept(torch.zeros(B, 229), torch.zeros(B), torch.zeros(B), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32),
                        torch.zeros(B), torch.zeros(B, dtype=torch.int64), torch.zeros(B, 2, dtype=torch.float64), torch.zeros(B, 49, 3),
                        torch.zeros(4, 82), torch.zeros(4, dtype=torch.uint8), 0.002)


def test_header_declares_and_lib_binds_the_accept_call():
    import ctypes
    from danet_densepose2smpl_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'danet_hip.h')).read()
    assert re.search(r'\bint\s+danet_fits_accept\s*\(\s*const\s+struct\s+danet_fits_accept_args\s*\*', src)
    assert 'danet_fits_accept' in _lib.exported_symbols()
    body = re.search(r'struct\s+danet_fits_accept_args\s*\{(.*?)\};', src, flags=re.S).group(1)
    declared = re.findall(r'[\s*]([A-Za-z_][A-Za-z0-9_]*)\s*[;,]', body)
    assert declared == [f[0] for f in _lib.FitsAcceptArgs._fields_]
    assert ctypes.sizeof(_lib.FitsAcceptArgs) == 12 * 8 + 8 + 4 + 4 + 4 + 4       # 12 pointers, N, B, NB, tau, tail padding
    assert 'fit_loop.hip' in open(os.path.join(ROOT, 'danet-densepose2smpl_amd', 'csrc', 'build.py')).read()


def test_iterations_map_to_stages():
    from danet_densepose2smpl_amd import fit_loop, kp_fit
    assert fit_loop.stages_for(None) is None
    assert fit_loop.stages_for(100) == kp_fit.DEFAULT_STAGES
    assert fit_loop.stages_for(10) == ((3, 'cam+orient'), (7, 'all'))
    assert fit_loop.stages_for(1) == ((0, 'cam+orient'), (1, 'all'))
    assert fit_loop.stages_for(0) == ((0, 'cam+orient'), (0, 'all'))
    for n in (0, 1, 2, 3, 7, 50, 100):
        st = fit_loop.stages_for(n)
        assert sum(k for k, _ in st) == n and st[0][0] == round(0.3 * n)
        assert kp_fit.parse_stages(st) == ([st[0][0], st[1][0]], [3, 15])
    for bad in (-1, 2.5):
        with pytest.raises(ValueError):
            fit_loop.stages_for(bad)
    assert fit_loop.default_tau(0.1) == pytest.approx(0.002, rel=1e-12)
    s2 = 0.1 ** 2
    assert fit_loop.default_tau(0.1) == pytest.approx(s2 * (s2 / 4) / (s2 + s2 / 4), rel=1e-12)          # rho((sigma / 2)^2)
    loop = fit_loop.InLoopFit(None, None, fitter=types.SimpleNamespace(sigma=0.2), iters=10)
    assert loop.tau == pytest.approx(0.008) and loop.stages == ((3, 'cam+orient'), (7, 'all'))
    assert fit_loop.InLoopFit(None, None, fitter=types.SimpleNamespace(sigma=0.2), tau=0.5).tau == 0.5


def test_train_tool_knows_the_three_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location('danet_tools_train', os.path.join(ROOT, 'tools', 'train.py'))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    ap = train.build_parser()
    a = ap.parse_args(['--name', 'x'])
    assert a.run_smplify is False and a.smplify_threshold is None and a.num_smplify_iters == 100
    a = ap.parse_args(['--name', 'x', '--run_smplify', '--smplify_threshold', '0.01', '--num_smplify_iters', '20'])
    assert a.run_smplify is True and a.smplify_threshold == 0.01 and a.num_smplify_iters == 20


def _stub_fits(n_a=5, n_b=3, seed=0):
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    rng = np.random.default_rng(seed)
    f = FitsDict.__new__(FitsDict)
    f.base, f.length = {'h36m': 0, 'dp_coco': n_a}, {'h36m': n_a, 'dp_coco': n_b}
    f.table = torch.from_numpy(rng.normal(0, 1, (n_a + n_b, 82)).astype(np.float32))
    f.valid = torch.from_numpy(rng.integers(0, 2, n_a + n_b).astype(np.uint8))
    f.device = torch.device('cpu')
    return f


def test_fits_state_round_trip_and_shape_check(tmp_path):
    a = _stub_fits(seed=1)
    d = str(tmp_path / 'ck')
    a.save_state(d)
    assert sorted(os.listdir(d)) == ['dp_coco_fits.npy', 'dp_coco_valid_fit.npy', 'h36m_fits.npy', 'h36m_valid_fit.npy']
    assert np.load(os.path.join(d, 'dp_coco_valid_fit.npy')).dtype == np.uint8
    b = _stub_fits(seed=2)
    assert not torch.equal(a.table, b.table)
    assert b.load_state(d) == ['dp_coco', 'h36m']
    assert torch.equal(a.table, b.table) and torch.equal(a.valid, b.valid)
    # a dataset with one of its two files missing keeps what it held
    os.remove(os.path.join(d, 'h36m_valid_fit.npy'))
    c = _stub_fits(seed=3)
    before = c.table.clone()
    assert c.load_state(d) == ['dp_coco']
    assert torch.equal(c.table[:5], before[:5]) and torch.equal(c.table[5:], a.table[5:]) and torch.equal(c.valid[5:], a.valid[5:])
    assert _stub_fits(seed=3).load_state(str(tmp_path / 'nothing_here')) == []
    # another shape: raises, and nothing is changed
    other = _stub_fits(n_a=5, n_b=4, seed=4)
    before_t, before_v = other.table.clone(), other.valid.clone()
    a.save_state(d)
    with pytest.raises(ValueError, match='dp_coco'):
        other.load_state(d)
    assert torch.equal(other.table, before_t) and torch.equal(other.valid, before_v)


def test_fit_refuses_run_smplify_with_more_than_one_rank():
    from danet_densepose2smpl_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.distributed = True
    o = types.SimpleNamespace(run_smplify=True, batch_size=4)
    with pytest.raises(RuntimeError, match='each rank holds its own'):
        tr.fit(None, None, o)
