"""REFINE_STRATEGY 'lstm' / 'lstm_direct' on the host: the predictor's state dict against the reference's (g21 fixtures), the
inference engine's fold plan, the configurations that stay refused, and the fp64 chain oracle (tests/lstm_oracle.py) against the
reference's own intermediate results."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
from make_golden import formula_tensor    # noqa: E402
from lstm_oracle import CHAINS, NAMES, lstm_tree_ref, make_lstms    # noqa: E402

SMPL_PARENTS = [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
SMPL_CHILDREN = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 10, 11, 15, 16, 17, 15, 18, 19, 20, 21, 22, 23, 22, 23]


def _model(strategy, **extra):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    try:
        cfg_from_dict(dict({'DANET.REFINE_STRATEGY': strategy}, **extra))
        return DaNet(default_options(2), None, pretrained=False)
    finally:
        reset_cfg()


def _predictor(model):
    from danet_densepose2smpl_amd.smpl_regressor import DecomposedPredictor
    return [m for m in model.modules() if isinstance(m, DecomposedPredictor)][0]


def formula_lstms(dtype=torch.float64):
    """The five LSTMs of stack 0 with the fixtures' formula parameters (tests/golden/make_golden.py formula_tensor)."""
    params = []
    for k in range(5):
        p = {}
        for sfx in ('', '_reverse'):
            for n, shape in zip(NAMES, ((512, 128), (512, 128), (512,), (512,))):
                p[n + sfx] = formula_tensor('limb_lstm.0.%d.%s%s' % (k, n, sfx), shape)
        params.append(p)
    return make_lstms(params, dtype)


@pytest.mark.parametrize('strategy,n_params', [('lstm', 39938365), ('lstm_direct', 34271165)])
def test_state_dict_matches_the_reference(strategy, n_params):
    pred = _predictor(_model(strategy))
    assert pred.refine_strategy == strategy
    sd = pred.state_dict()
    g = golden('g21_predictor_%s_train' % strategy)
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(g['sd_keys'], g['sd_shapes'])}
    got = {k: tuple(t.shape) for k, t in sd.items()}
    assert got == want
    assert sum(p.numel() for p in pred.parameters()) == n_params
    assert not any(k.startswith(('refine_gcn', 'r2p_gcn', 'p2r_gcn', 'edge_importance', 'A', 'I_n', 'r2p_A', 'p2r_A')) for k in sd)
    for k in range(5):
        assert 'limb_lstm.0.%d.weight_hh_l0_reverse' % k in sd


@pytest.mark.parametrize('regressor,n_total', [('hrnet', 343), ('resnet', 107)])
@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
def test_fold_plan_counts(regressor, n_total, strategy):
    from danet_densepose2smpl_amd.inference import fold_plan
    plan = fold_plan(_model(strategy, **{'DANET.IUV_REGRESSOR': regressor}))
    assert plan.unfolded == [] and plan.skipped == []
    extra = 24 * 2 + 2 if strategy == 'lstm' else 0
    assert len(plan) == n_total + extra
    assert sum('.rot2pos.' in p.bn_name for p in plan.pairs) == (48 if strategy == 'lstm' else 0)
    assert sum('.pos2rot.' in p.bn_name for p in plan.pairs) == (2 if strategy == 'lstm' else 0)


def test_refused_configurations():
    with pytest.raises(NotImplementedError, match='157'):
        _model('gcn_direct')
    for strategy in ('lstm', 'lstm_direct'):
        with pytest.raises(NotImplementedError, match='STACK_NUM'):
            _model(strategy, **{'DANET.REFINEMENT.STACK_NUM': 2})


def test_chain_table_matches_the_op():
    from danet_densepose2smpl_amd.lstm_tree import CHAINS as OP_CHAINS
    assert [c for c, _ in OP_CHAINS] == list(CHAINS)
    assert [k for _, k in OP_CHAINS] == [0, 0, 1, 2, 3, 4]


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_oracle_reproduces_the_reference_lstm_direct(mode):
    """lstm_direct: the input of pose_regressors[1] IS pos' = refine(rot_feats)."""
    g = golden('g21_predictor_lstm_direct_%s' % mode)
    rot = torch.from_numpy(g['rot_feats']).double()
    with torch.no_grad():
        ref = lstm_tree_ref(rot, formula_lstms())
    want = torch.from_numpy(g['prehead']).double()
    err = (ref - want).abs().max().item()
    assert err < 1e-5, err
    # not degenerate: the LSTM's share of pos' is far from zero
    assert (want - torch.cat([rot, rot], 2)).norm() / want.norm() > 0.2


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_reference_tri_layout(mode):
    """lstm: tri[j] = cat(pos'[P[j]], pos'[j], pos'[Ch[j]]) -- the gather the port's pos2rot input repeats."""
    tri = torch.from_numpy(golden('g21_predictor_lstm_%s' % mode)['tri']).double()
    mid = tri[:, :, 256:512]
    assert torch.equal(tri[:, :, :256], mid[:, SMPL_PARENTS])
    assert torch.equal(tri[:, :, 512:], mid[:, SMPL_CHILDREN])


@pytest.mark.parametrize('strategy', ['lstm', 'lstm_direct'])
def test_reference_layout_checkpoint_loads(strategy, tmp_path):
    """A checkpoint in the reference's layout ({'model': state dict}, keys as g21 lists them under the regressor's prefix) loads
    through checkpoint.load_pretrained with nothing missing or unexpected in the predictor."""
    from danet_densepose2smpl_amd.checkpoint import load_pretrained
    model = _model(strategy)
    prefix = [n for n, m in model.named_modules() if m is _predictor(model)][0] + '.'
    g = golden('g21_predictor_%s_train' % strategy)
    sd = {}
    for k, s in zip(g['sd_keys'], g['sd_shapes']):
        shape = tuple(int(v) for v in s if v >= 0)
        k = str(k)
        sd[prefix + k] = formula_tensor(k, shape) if not k.endswith('num_batches_tracked') else torch.zeros((), dtype=torch.long)
    path = str(tmp_path / 'ref.pth')
    torch.save({'model': sd}, path)
    missing, unexpected = load_pretrained(model, path)
    assert not unexpected
    assert not [k for k in missing if k.startswith(prefix)]
    got = model.state_dict()
    key = prefix + 'limb_lstm.0.2.weight_hh_l0_reverse'
    assert torch.equal(got[key], sd[key])
