"""DANET.INPUT_MODE 'iuv_gt' without a GPU: the module layout and state dict, which configurations are refused and why, the crop-ratio
pickle round trip, the tap-by-tap fp64 oracle of the crops' theta gradient against torch's autograd, and the estimator's tensor-op
formulation against the reference's own results (g23, fp64)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import part_gt_oracle as orc    # noqa: E402


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(dict({'DANET.IUV_REGRESSOR': 'resnet', 'DANET.INIMG_SIZE': 64, 'DANET.HEATMAP_SIZE': 16}, **kw))


@pytest.fixture(autouse=True)
def _reset():
    yield
    from danet_densepose2smpl_amd.config import reset_cfg
    reset_cfg()


def _danet(mode):
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    _cfg(**{'DANET.INPUT_MODE': mode})
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False)


def test_state_dict_keys():
    gt, dflt = _danet('iuv_gt').state_dict(), _danet('iuv').state_dict()
    assert not any(k.startswith('img2iuv.iuv_est') for k in gt)
    want = {k for k in dflt if not k.startswith('img2iuv.')} | {'img2iuv.learned_ratio', 'img2iuv.learned_offset'}
    assert set(gt) == want
    # the names equal the default model's: an 'iuv_gt' checkpoint sets a default model's ratio buffers with strict=False
    m = _danet('iuv')
    sd = {k: v.clone() for k, v in gt.items()}
    sd['img2iuv.learned_ratio'] = torch.full((24,), 0.7)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert torch.equal(m.img2iuv.learned_ratio, torch.full((24,), 0.7))


def test_ratio_parameters_only_in_iuv_gt():
    est = _danet('iuv_gt').img2iuv
    names = dict(est.named_parameters())
    assert set(names) == {'learned_ratio', 'learned_offset'}
    assert isinstance(est.learned_ratio, torch.nn.Parameter) and isinstance(est.learned_offset, torch.nn.Parameter)
    est = _danet('iuv').img2iuv
    assert 'learned_ratio' in dict(est.named_buffers()) and 'learned_ratio' not in dict(est.named_parameters())


@pytest.mark.parametrize('mode,why', [('feat', 'KeyError'), ('iuv_feat', 'KeyError'), ('iuv_gt_feat', 'KeyError'), ('seg', 'KeyError'),
                                      ('rgb', 'never assigned')])
def test_refused_input_modes(mode, why):
    with pytest.raises(NotImplementedError, match=why):
        _danet(mode)


def test_refused_iuv_gt_global_predictor():
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    _cfg(**{'DANET.INPUT_MODE': 'iuv_gt', 'DANET.DECOMPOSED': False})
    with pytest.raises(NotImplementedError, match='joint_rotation'):
        DaNet(default_options(2), None, pretrained=False)


def test_refused_inference_engine():
    from danet_densepose2smpl_amd.inference import InferenceEngine
    m = _danet('iuv_gt').eval()
    with pytest.raises(NotImplementedError, match='infer_net'):
        InferenceEngine(m, 2)


def test_save_load_learned_ratio(tmp_path):
    from danet_densepose2smpl_amd.iuv_estimator import save_learned_ratio, load_learned_ratio
    m = _danet('iuv_gt')
    ratio, offset = orc_ratio()
    with torch.no_grad():
        m.img2iuv.learned_ratio.copy_(ratio)
        m.img2iuv.learned_offset.copy_(offset)
    p = str(tmp_path / 'learned_ratio.pkl')
    save_learned_ratio(m, p)
    with open(p, 'rb') as f:
        d = pickle.load(f)
    assert set(d) == {'ratio', 'offset'} and d['ratio'].dtype == np.float32 and d['offset'].dtype == np.float32
    r, o = load_learned_ratio(p)
    assert np.array_equal(r, ratio.numpy()) and np.array_equal(o, offset.numpy())     # raw values: the negative entries survive
    save_learned_ratio(m.img2iuv, p)
    assert np.array_equal(load_learned_ratio(p)[0], ratio.numpy())
    # ... and a default model built from that file uses them
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    _cfg()
    est = IUV_Estimator(pretrained=False, learned_ratio_path=p)
    assert torch.equal(est.learned_ratio, ratio) and torch.equal(est.learned_offset, offset)


def orc_ratio():
    sys.path.insert(0, GOLDEN)
    from make_golden_iuvgt import ratio_offset
    return ratio_offset()


@pytest.mark.parametrize('align', [0, 1])
def test_oracle_dtheta_matches_torch_autograd(align):
    """The tap-by-tap d theta of tests/part_gt_oracle.py (what the HIP backward implements) equals fp64 autograd through
    affine_grid / grid_sample, all six entries; pixels whose coordinate is within 1e-4 of an integer get no upstream gradient (the
    bilinear gradient jumps there)."""
    B, H, W = 2, 20, 24
    img = orc.make_image(B, H, W, 5).double()
    th = orc.make_thetas(B, 6)
    sel = np.array(__import__('danet_densepose2smpl_amd.iuv_estimator', fromlist=['x']).DP2SMPL_MAPPING)
    keep = (torch.rand(B, 24, 7, generator=torch.Generator().manual_seed(7)) > 0.3).double()
    keep[..., 0] = 1
    g = torch.randn(B, 24, 21, H, W, generator=torch.Generator().manual_seed(8)).double()
    g = g * torch.from_numpy(~orc.tie_mask(th, H, W, align)).unsqueeze(2)
    t64 = th.double().requires_grad_(True)
    out = orc.torch_reference(img, t64, sel, keep, bool(align))
    (out.reshape(B, 24, 21, H, W) * g).sum().backward()
    for b in range(B):
        d, T, _ = orc.dtheta_sample(img[b].numpy(), th[b].numpy(), sel, g[b].numpy(), keep[b].numpy(), align, emulate_fp32=False)
        ref = t64.grad[b].numpy()
        assert np.abs(d - ref).max() <= 1e-11 * (1 + T.max()), (np.abs(d - ref).max(), T.max())
        assert np.abs(ref[:, 0, 1]).max() > 0 and np.abs(ref[:, 1, 0]).max() > 0


def test_oracle_forward_matches_torch():
    B, H, W = 2, 16, 16
    img = orc.make_image(B, H, W, 1).double()
    th = orc.make_thetas(B, 2)
    from danet_densepose2smpl_amd.iuv_estimator import DP2SMPL_MAPPING
    out = orc.torch_reference(img, th.double(), DP2SMPL_MAPPING, None, True).reshape(B, 24, 21, H, W).numpy()
    for b in range(B):
        v, _ = orc.forward_sample(img[b].numpy(), th[b].numpy(), DP2SMPL_MAPPING, None, 1, emulate_fp32=False)
        assert np.abs(v - out[b]).max() < 1e-12


@pytest.mark.parametrize('which', ['train', 'eval'])
def test_estimator_fallback_matches_reference_fp64(which):
    """The tensor-op formulation of IUV_Estimator 'iuv_gt' (CPU, fp64): thetas and the crops against the reference's fp64 run (g23)."""
    sys.path.insert(0, GOLDEN)
    from make_golden import g19_inputs
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    g = golden('g23_iuvgt_%s' % which)
    _cfg(**{'DANET.INPUT_MODE': 'iuv_gt', 'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.STN_CENTER_JITTER': 0.,
            'DANET.STN_SCALE_JITTER': 0., 'DANET.PARTDROP_RATE': 0.})
    est = IUV_Estimator(pretrained=False).double().train(which == 'train')
    with torch.no_grad():
        est.learned_ratio.copy_(torch.from_numpy(g['ratio']))
        est.learned_offset.copy_(torch.from_numpy(g['offset']))
    _, gt, kps = g19_inputs(4, 64)
    th = []
    ap = est.affine_para
    est.affine_para = lambda c, h=None: th.append(ap(c, h)) or th[-1]
    rd = est(None, gt.double(), kps.double())
    assert rd['losses'] == {}
    theta = th[0][0]
    assert np.abs(theta.detach().numpy() - g['theta64']).max() <= 1e-7 * np.abs(g['theta64']).max()
    part = rd['part_iuv_gt'].detach()[:, ::3, :, :, ::4, ::4].numpy()
    assert part.shape == g['part_iuv_gt'].shape
    assert np.abs(part - g['part_iuv_gt']).max() <= 1e-6
    if which == 'train':
        # the ReLU-clamped ratio / offset (negative in the fixture) get exactly zero gradient through the crops
        part_full = rd['part_iuv_gt']
        (part_full * torch.cos(torch.arange(part_full.numel(), dtype=torch.float64).view_as(part_full))).sum().backward()
        rz = g['relu_zero']
        assert est.learned_ratio.grad[int(rz[0])] == 0 and est.learned_offset.grad[int(rz[1])] == 0
        assert (est.learned_ratio.grad != 0).sum() >= 20
