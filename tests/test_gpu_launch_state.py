"""Launch state that used to be written out at every site: the side-stream fork / join with its barrier window (nn.SideBranch) and the
per-device opt-in for more than 64 KB of dynamic LDS (csrc/capi.hip raise_dynamic_lds).

Which test covers which refinement arm of DecomposedPredictor._refine END TO END (through forward, against the reference's values):
the LSTM strategies -- tests/test_gpu_refine_lstm.py (g21 'lstm' / 'lstm_direct', train and eval; g22 the train pass); the fused graph
tail -- tests/test_gpu_fp32.py (g20 train pass at the benched size, g9 train); the tensor-op graph tail -- tests/test_gpu_fp32.py (g9
eval) and tests/test_gpu_iuv_gt.py.  None of them gives both inputs a gradient, so none of them forks: the comparison of the forked
forward with the unforked one below runs every arm both ways."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(kw)


def _predictor(strategy='gcn'):
    from danet_densepose2smpl_amd.smpl_regressor import DecomposedPredictor
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.REFINE_STRATEGY': strategy})
    torch.manual_seed(3)
    pose6 = torch.tensor([1., 0., 0., 1., 0., 0.]).repeat(24).unsqueeze(0)
    return DecomposedPredictor(None, (torch.tensor([[0.9, 0., 0.]]), torch.zeros(1, 10), pose6), pretrained=False).cuda().train()


def _inputs():
    g = torch.Generator().manual_seed(5)
    return (torch.randn(2, 75, 64, 64, generator=g).cuda().requires_grad_(True),
            torch.randn(2, 24, 3, 7, 64, 64, generator=g).cuda().requires_grad_(True))


def test_side_stream_window_closes_when_the_forward_raises():
    """An exception between the regressor's fork and its join (here: limb_reslayer) leaves nn.SIDE_LIVE, the barrier budget and the
    current stream as they were; the next forward + backward opens and closes the window as usual."""
    from danet_densepose2smpl_amd import conv, nn as dnn, smpl_regressor as sr
    net = _predictor()
    dnn.ONEPASS_STREAM = None
    assert dnn.SIDE_LIVE == 0
    iuv, part = _inputs()
    cur = torch.cuda.current_stream()

    def boom(*a, **k):
        raise RuntimeError('limb_reslayer failed')
    keep = net.limb_reslayer.forward
    net.limb_reslayer.forward = boom
    try:
        with pytest.raises(RuntimeError, match='limb_reslayer failed'):
            net(iuv, part)
    finally:
        net.limb_reslayer.forward = keep
    assert dnn.SIDE_LIVE == 0
    assert dnn.onepass_budget() == dnn.ONEPASS_MAX_BLOCKS
    assert torch.cuda.current_stream() == cur
    seen = []
    hook = net.limb_net[3].layer1[0].bn1.register_full_backward_hook(lambda m, gi, go: seen.append(dnn.SIDE_LIVE))
    rd = net(iuv, part)
    assert dnn.SIDE_LIVE == 0                                   # the forward window is closed at the join
    (rd['para'].float().sum() + sum(t.float().sum() for t in rd['joint_position'])).backward()
    hook.remove()
    assert seen == [1] if sr.BODY_STREAM else seen == [0]       # limb_net's backward ran inside the window
    assert dnn.SIDE_LIVE == 0 and iuv.grad is not None and part.grad is not None
    conv.flush_wgrads()
    torch.cuda.synchronize()
    assert not dnn.onepass_error()


def test_onepass_recover_clears_the_side_stream_window():
    from danet_densepose2smpl_amd import nn as dnn
    keep = dnn.ONEPASS
    dnn.SIDE_LIVE = 1
    try:
        assert dnn.onepass_recover(force=True)
        assert dnn.SIDE_LIVE == 0
    finally:
        dnn.SIDE_LIVE = 0
        dnn.ONEPASS = keep


@pytest.mark.parametrize('arm', ['gcn_fused', 'gcn_tensor_ops', 'lstm', 'lstm_direct'])
def test_forked_forward_equals_the_unforked_one(arm):
    """rd['para'] (and the intermediate heads) with body_net on its side stream == with everything on one stream, bit for bit, for
    every arm of the refinement: the fork moves launches between streams and changes none of them."""
    from danet_densepose2smpl_amd import conv, gcn_tail, smpl_regressor as sr
    net = _predictor('gcn' if arm.startswith('gcn') else arm)
    iuv, part = _inputs()
    keep = sr.BODY_STREAM, gcn_tail.GCN_TAIL
    outs = []
    try:
        gcn_tail.GCN_TAIL = arm != 'gcn_tensor_ops'
        for on in (True, False):
            sr.BODY_STREAM = on
            before = conv.FUSION['gcn_tail']
            rd = net(iuv, part)
            assert conv.FUSION['gcn_tail'] - before == (1 if arm == 'gcn_fused' else 0)
            outs.append([rd['para']] + list(rd['joint_rotation']) + list(rd.get('joint_position', [])))
        torch.cuda.synchronize()
    finally:
        sr.BODY_STREAM, gcn_tail.GCN_TAIL = keep
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.isfinite(outs[0][0].float()).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs a second GPU')
def test_lds_opt_in_follows_the_current_device():
    """conv3x3a_kernel<16> asks for Geo<16>::LDS = 129536 bytes of dynamic LDS (csrc/conv3x3a.hip: 2 * 41472 staging + 32768 exchange +
    512 tables + 10752 offsets + 512 + 2048 statistics), above the 64 KB a kernel gets without the opt-in, and has no grid barrier.
    The smallest problem it takes: 64 -> 64 channels, 16 x 16 maps, 256 tiles = B 256.  One process runs it on cuda:0 and then on
    cuda:1: the second device needs its own opt-in.  Bound: the one tests/test_gpu_conv.py holds this kernel's forward to (1e-2 of
    the reference's scale against F.conv2d in fp32 on the bf16-rounded operands)."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    B, C, H, W = 256, 64, 16, 16
    assert _lib.lib().danet_conv3x3a_ok(B, H, W, C, C, 3, 3, 1, 1, 1, 1) == 1
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    w = (torch.randn(C, C, 3, 3, generator=g) / np.sqrt(9 * C / 4)).bfloat16().float()
    ys = []
    for d in (0, 1):
        with torch.cuda.device(d), torch.no_grad():
            y = dconv.conv2d(dconv.nhwc_bf16(x.cuda(d)), w.cuda(d), None, 1, 1)
            torch.cuda.synchronize(d)
            ys.append(y.float().cpu())
    ref = F.conv2d(x.float(), w, None, 1, 1)
    scale = ref.abs().max().item()
    assert (ys[0] - ref).abs().max().item() <= 1e-2 * scale
    assert (ys[1] - ref).abs().max().item() <= 1e-2 * scale
