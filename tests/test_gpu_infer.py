"""The BatchNorm-folded, graph-captured inference engine (danet_densepose2smpl_amd/inference.py) on the device: its new conv epilogues
against fp64 within a derived rounding bound (tests/conv_bound.py), parity with the reference (golden g17) and with DaNet.infer_net on both backbones, graph replay, refresh / stale, and
that it leaves the model alone.  Measured errors go to record(); the tolerances are set from those measurements."""
import os
import sys
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN, record
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_bound import U_BF16, reference, bound, check    # noqa: E402
from make_golden import formula_input    # noqa: E402
from test_gpu_f2 import _reference_layout_checkpoint, GRAPH_BUFFERS    # noqa: E402

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(kw)


# ---- the new epilogues, against fp64 on the bf16-rounded operands (tests/conv_bound.py) -----------------------------------------

def _operands(B, Cin, Cout, H, W, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(k * k * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda() * 0.5
    return x, w, b


def _check(y, x, w, b, res, relu, stride, pad, what, idx=None):
    """y (at batch items idx) against the fp64 [relu](conv(x, bf16(w)) + b [+ res]) on the operands the kernel consumed, within
    tests/conv_bound.py's rounding bound and per-channel mean check -- a bound that is itself checked to be below the 1e-2 of max|ref|
    these tests used to allow."""
    if idx is not None:
        y, x, res = y[idx], x[idx], None if res is None else res[idx]
    ref = reference(x, w.bfloat16(), b, res, relu, stride, pad)
    scale = ref.r.abs().max().item()
    assert bound(ref, U_BF16)[0].max().item() < 1e-2 * scale, what
    elem, mean = check(y, ref, U_BF16, what)
    return {'elem': elem, 'chan_mean': mean, 'rel': (y.double() - ref.r).abs().max().item() / scale}


def _stem_case(B, Cin, relu, bias_shift, seed):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    assert L.danet_conv_stem_ok(B, 64, 64, Cin, 32, 32, 64, 7, 7, 2, 3, 1, 1) == 1
    x, w, b = _operands(B, Cin, 64, 64, 64, 7, seed)
    b = b + bias_shift
    wp = dconv.pack_weight(w, 1, 0, 16)
    y = dconv._empty_nhwc(B, 64, 32, 32, torch.bfloat16, x.device)
    dconv.check(L.danet_conv_stem_forward_epi(dconv.ptr(x.permute(0, 2, 3, 1)), dconv.ptr(wp), dconv.ptr(b), dconv.ptr(y.permute(0, 2, 3, 1)),
                                              B, 64, 64, Cin, 32, 32, 64, int(relu), dconv.stream()), 'stem epi')
    idx = torch.linspace(0, B - 1, min(B, 48)).long().cuda()
    m = _check(y, x, w, b, None, relu, 2, 3, ('stem', B, Cin, relu), idx)
    record('infer_stem_epilogue', dict(m, B=B, Cin=Cin, relu=relu, bias_shift=bias_shift))
    if relu:
        assert (y >= 0).all()
    if bias_shift:
        assert (y < 0).float().mean().item() > 0.5


@pytest.mark.parametrize('relu', [True, False])
def test_stem_bias_relu_epilogue(relu):
    """conv_stem_bias_kernel at the regressor's limb stem: 768 crops, 64 -> 64 channels, 64 x 64, 7x7 / stride 2."""
    _stem_case(768, 64, relu, 0., 1)


@pytest.mark.parametrize('B,Cin', [(64, 64), (96, 32), (70, 16)])
@pytest.mark.parametrize('relu,bias_shift', [(True, 0.), (False, 0.), (False, -1.5)])
def test_stem_bias_epilogue_at_the_plain_kernel_shapes(B, Cin, relu, bias_shift):
    """The same at the shapes the plain stem kernel is tested at (test_gpu_conv.py: odd tile counts per workgroup, 16- and 32-channel
    slabs); bias_shift < 0: no ReLU and most outputs negative."""
    _stem_case(B, Cin, relu, bias_shift, B + Cin)


@pytest.mark.parametrize('B,Cin', [(768, 64)])
def test_stem_bias_epilogue_negative_outputs(B, Cin):
    """The regressor's limb stem without ReLU and with a bias that makes most outputs negative."""
    _stem_case(B, Cin, False, -1.5, 1)


def _c3a_case(B, H, W, with_res, relu, res_scale, seed):
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    assert L.danet_conv3x3a_ok(B, H, W, 64, 64, 3, 3, 1, 1, 1, 1) == 1
    x, w, b = _operands(B, 64, 64, H, W, 3, seed)
    res = (torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(3)) * res_scale).bfloat16().cuda() \
        .contiguous(memory_format=torch.channels_last)
    wp = dconv.pack_weight(w, 1, 0, 16)
    y = dconv._empty_nhwc(B, 64, H, W, torch.bfloat16, x.device)
    dconv.check(L.danet_conv3x3a_forward_epi(dconv.ptr(x.permute(0, 2, 3, 1)), dconv.ptr(wp), dconv.ptr(b),
                                             dconv.ptr(res.permute(0, 2, 3, 1)) if with_res else None, dconv.ptr(y.permute(0, 2, 3, 1)),
                                             B, H, W, int(relu), dconv.stream()), 'c3a epi')
    idx = torch.linspace(0, B - 1, min(B, 64)).long().cuda()
    m = _check(y, x, w, b, res if with_res else None, relu, 1, 1, ('conv3x3a', B, H, W, with_res, relu, res_scale), idx)
    record('infer_c3a_epilogue', dict(m, B=B, H=H, W=W, res=with_res, relu=relu, res_scale=res_scale))


@pytest.mark.parametrize('with_res', [False, True])
def test_conv3x3a_bias_addend_relu_epilogue(with_res):
    """conv3x3a_bias_kernel at the regressor's layer1 BasicBlocks: 768 x 16 x 16, 64 -> 64 channels (conv1 -> bn1 -> relu and
    conv2 -> bn2 -> + identity -> relu)."""
    _c3a_case(768, 16, 16, with_res, True, 1., 2)


@pytest.mark.parametrize('B,H,W,with_res,relu,res_scale', [
    shape + flags for shape in [(768, 16, 16), (32, 64, 64), (300, 16, 16), (20, 64, 64), (140, 32, 16)]
    for flags in [(False, True, 1.), (True, True, 1.), (True, True, 8.), (True, False, 8.)]
    if not (shape[0] == 768 and flags[2] == 1.)])          # (those two are test_conv3x3a_bias_addend_relu_epilogue)
def test_conv3x3a_bias_epilogue_shapes_and_large_addend(B, H, W, with_res, relu, res_scale):
    """The same at the shapes the plain kernel is tested at (test_gpu_conv.py: 16- and 64-wide maps, several strips per image);
    res_scale = 8: an addend much larger than the convolution, so that adding it in the wrong place (after the ReLU, or rounded
    separately) shows."""
    _c3a_case(B, H, W, with_res, relu, res_scale, B + H)


def _multi(specs, B, seed):
    """specs: (Cin, Cout, H, k, stride, relu, with_res) -> the ConvJobEpi set, its outputs and each job's operands for _check."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    jobs = (_lib.ConvJobEpi * len(specs))()
    keep, ops, ys = [], [], []
    for i, (Cin, Cout, H, k, st, relu, with_res) in enumerate(specs):
        x, w, b = _operands(B, Cin, Cout, H, H, k, seed + i)
        OH = (H + 2 * (k // 2) - k) // st + 1
        res = torch.randn(B, Cout, OH, OH, generator=torch.Generator().manual_seed(seed + 50 + i)).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last) if with_res else None
        wp = dconv.pack_weight(w, 1, 0)
        y = dconv._empty_nhwc(B, Cout, OH, OH, torch.bfloat16, x.device)
        dconv.stream_tables(x.device)
        j = jobs[i].j
        j.x, j.wp, j.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
        j.addend = None if res is None else res.data_ptr()
        (j.B, j.H, j.W, j.Cin, j.OH, j.OW, j.Cout, j.R, j.S, j.stride, j.pad, j.dil, j.groups, j.transposed, j.bn_gate) = \
            (B, H, H, Cin, OH, OH, Cout, k, k, st, k // 2, 1, 1, 0, 0)
        jobs[i].bias, jobs[i].relu = b.data_ptr(), int(relu)
        ops.append((x, w, b, res, relu, st, k // 2))
        ys.append(y)
        keep += [x, w, b, res, wp]
    return jobs, ys, ops, keep


_LEVEL = [(48, 48, 64, 3, 1), (96, 96, 32, 3, 1), (192, 192, 16, 3, 1), (384, 384, 8, 3, 1)]
_POINTWISE = [(48, 48, 32, 1, 1), (96, 96, 16, 1, 1), (192, 192, 8, 1, 1), (48, 96, 32, 1, 1), (96, 48, 16, 1, 1)]
_MULTI_SETS = {
    # (B, specs, the kernel danet_conv_forward_multi_epi_kernel must pick: 3 streamed 3x3, 2 LDS-tile 3x3, 1 gather, None: either)
    'hrnet_level_conv1': (32, [s + (True, False) for s in _LEVEL], 3),
    'hrnet_level_conv2': (32, [s + (True, True) for s in _LEVEL], 3),
    'fuse_stage': (32, [(48, 48, 64, 3, 2, True, False), (96, 96, 32, 3, 2, True, False), (48, 96, 64, 3, 2, False, False),
                        (96, 192, 32, 3, 2, False, False)], None),
    # mixed ReLU flags, addend and no-addend jobs in one launch: on the 3x3 kernels and on the gather kernel
    'mixed_level': (32, [s + f for s, f in zip(_LEVEL, [(True, True), (False, False), (False, True), (True, False)])], None),
    'mixed_pointwise': (32, [s + f for s, f in zip(_POINTWISE, [(True, True), (False, False), (True, False), (False, True), (True, True)])], 1),
    # a demo batch size
    'hrnet_level_conv2_b3': (3, [s + (True, True) for s in _LEVEL], None),
    'mixed_pointwise_b3': (3, [s + f for s, f in zip(_POINTWISE, [(True, True), (False, False), (True, False), (False, True), (True, True)])], 1),
}


@pytest.mark.parametrize('kind', list(_MULTI_SETS))
def test_multi_problem_epilogue_sets(kind):
    """danet_conv_forward_multi_epi on the sets the engine launches: a four-branch HRNet-W48 block level at B = 32, 256^2 (conv1 with
    ReLU; conv2 with the identity addend and ReLU) and a fuse stage (strided 3x3 exchange paths, with and without ReLU); sets that mix
    ReLU flags and addend / no-addend jobs on the 3x3 and the gather kernels; the same at B = 3."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    B, specs, kernel = _MULTI_SETS[kind]
    jobs, ys, ops, keep = _multi(specs, B, 10)
    n = len(specs)
    ok = L.danet_conv_forward_multi_epi_ok(ctypes.addressof(jobs), n)
    if kind.startswith('hrnet') and B == 32:
        # the branch levels run on the streamed 3x3 kernel, in one launch
        assert ok == 2
    if kernel is not None:
        assert L.danet_conv_forward_multi_epi_kernel(ctypes.addressof(jobs), n) == kernel
    sets = [list(range(n))] if ok else [[0, 1], [2, 3]]
    assert ok or kind == 'fuse_stage', kind
    for s in sets:
        arr = (_lib.ConvJobEpi * len(s))(*[jobs[k] for k in s])
        assert L.danet_conv_forward_multi_epi_ok(ctypes.addressof(arr), len(s))
        dconv.check(L.danet_conv_forward_multi_epi(ctypes.addressof(arr), len(s), dconv.stream()), 'multi epi')
    ms = [_check(y, *op, what=(kind, i)) for i, (y, op) in enumerate(zip(ys, ops))]
    record('infer_multi_epilogue', {'kind': kind, 'B': B, 'elem': [m['elem'] for m in ms], 'chan_mean': [m['chan_mean'] for m in ms],
                                    'rel': [m['rel'] for m in ms]})
    # a missing job list is refused, not dereferenced
    assert L.danet_conv_forward_multi_epi_ok(None, n) == 0


def test_multi_problem_epilogue_refuses_an_unsupported_set():
    """Five pointwise jobs (too many for the 3x3 kernels) whose channel-block counts differ (48 vs 64 output channels): no kernel
    takes the set, the predicate says so and the launch is refused before anything runs."""
    from danet_densepose2smpl_amd import conv as dconv, _lib
    L = _lib.lib()
    specs = [(48, 48, 32, 1, 1, True, False), (64, 64, 32, 1, 1, True, False), (48, 48, 16, 1, 1, False, True), (64, 64, 16, 1, 1, False, False),
             (48, 48, 8, 1, 1, True, False)]
    jobs, ys, ops, keep = _multi(specs, 4, 30)
    assert L.danet_conv_nt(48) != L.danet_conv_nt(64)
    assert L.danet_conv_forward_multi_epi_ok(ctypes.addressof(jobs), len(specs)) == 0
    assert L.danet_conv_forward_multi_epi_kernel(ctypes.addressof(jobs), len(specs)) == 0
    assert L.danet_conv_forward_multi_epi(ctypes.addressof(jobs), len(specs), dconv.stream()) != 0
    # each equal-count subset is taken
    for s in ([0, 2, 4], [1, 3]):
        arr = (_lib.ConvJobEpi * len(s))(*[jobs[k] for k in s])
        assert L.danet_conv_forward_multi_epi_ok(ctypes.addressof(arr), len(s)) == 1
# ---- the engine against the reference (golden g17: reference inference at 128^2, B = 2) ------------------------------------------

@pytest.fixture(scope='module')
def loaded(tmp_path_factory):
    _cfg(**{'DANET.INIMG_SIZE': 128, 'DANET.HEATMAP_SIZE': 32, 'DANET.STN_CENTER_JITTER': 0., 'DANET.STN_SCALE_JITTER': 0.,
            'DANET.PARTDROP_RATE': 0.})
    from danet_densepose2smpl_amd import checkpoint
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    g = golden('g17_infer')
    torch.manual_seed(123)
    model = DaNet(default_options(2), None, pretrained=False)
    shapes = {k: (tuple(v.shape), v.dtype) for k, v in model.state_dict().items()}
    path = str(tmp_path_factory.mktemp('infer') / 'danet_model_formula.pt')
    _reference_layout_checkpoint(path, shapes, g)
    checkpoint.load_pretrained(model, path)
    return model.cuda().eval(), g


def _rel(a, ref):
    ref = np.asarray(ref, np.float32)
    a = a.detach().float().cpu().numpy()
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-6))


def test_engine_fp32_and_bf16_match_the_reference(loaded):
    from danet_densepose2smpl_amd import conv
    from danet_densepose2smpl_amd.inference import InferenceEngine
    model, g = loaded
    img = formula_input('g17.img', (2, 3, 128, 128), -2.0, 2.0).cuda()
    eng = InferenceEngine(model, 2, 128)
    with conv.precision('fp32'):
        rd = eng(img)
        est = eng._shadow.img2iuv(img)
    errs = {}
    for a, k in zip(est['uvia_pred'], ('u_raw', None, 'index_raw', 'ann_raw')):
        if k:
            errs[k] = _rel(a, g[k])
    errs['part_iuv_pred'] = _rel(est['part_iuv_pred'][:, ::6], g['part_iuv_pred'])
    errs['stn_kps_pred'] = float(np.abs(est['stn_kps_pred'].cpu().numpy() - g['stn_kps_pred']).max())
    errs['para'] = float(np.abs(rd['para'].cpu().numpy() - g['para']).max())
    rb = eng(img)['para']                                        # bf16, graph replay
    errs['para_bf16'] = float(np.abs(rb.cpu().numpy() - g['para']).max())
    record('infer_engine_vs_reference_g17', errs)
    assert max(errs[k] for k in ('u_raw', 'index_raw', 'ann_raw', 'part_iuv_pred')) < 2e-5, errs
    assert errs['stn_kps_pred'] < 2e-6 and errs['para'] < 5e-6, errs
    assert torch.isfinite(rb).all() and errs['para_bf16'] < 5e-3, errs
    eng.close()


# ---- the engine against infer_net on both backbones at their benchmark sizes ---------------------------------------------------------

def _model(regressor, B):
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.IUV_REGRESSOR': regressor})
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    torch.manual_seed(0)
    model = DaNet(default_options(B), None, pretrained=False)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                        # non-trivial eval statistics, so that the folding matters
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.weight.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return model.cuda().eval()


def _decided_index_agrees(model, eng, img, idx_engine, idx_ref):
    """test_gpu_f2's rule: the cleaned part index agrees wherever the eager logits' top two are further apart than 4x the measured
    distance of the engine's raw index logits from infer_net's."""
    with torch.no_grad():
        raw = model.img2iuv(img)['uvia_pred'][2].float()
        raw_e = eng._shadow.img2iuv(img)['uvia_pred'][2].float()
    err = ((raw_e - raw).abs().max() / raw.abs().max()).item()
    top = raw.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 4 * err * raw.abs().max()
    agree = idx_engine.argmax(1) == idx_ref.argmax(1)
    return float(decided.float().mean()), bool(agree[decided].all()), int((~agree & decided).sum()), err


@pytest.mark.parametrize('regressor,B', [('resnet', 16), ('hrnet', 32)])
def test_engine_matches_infer_net_graph_replay_and_leaves_the_model_alone(regressor, B):
    from danet_densepose2smpl_amd import conv
    model = _model(regressor, B)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(2)
    img = torch.randn(B, 3, 256, 256, generator=g).cuda()
    img2 = torch.randn(B, 3, 256, 256, generator=g).cuda()
    ref = model.infer_net(img)
    eng = model.inference_engine(B)
    conv.TRACE = []
    try:
        eager = eng.eager(img)
        trace = list(conv.TRACE)
    finally:
        conv.TRACE = None
    # plan coverage: no BatchNorm launch at all, every folded pair ran as a convolution with its epilogue
    assert not [t for t in trace if t[0].startswith('bn')], trace[:3]
    assert eng.launches['conv_multi_epi'] > 0 if regressor == 'hrnet' else True
    eager = {'para': eager['para'].clone(), 'idx': eager['visualization']['iuv_pred'][2].clone()}
    out = eng(img)
    # graph replay == the engine run eagerly, bit for bit; a second image through the same static input as well
    assert torch.equal(out['para'], eager['para']) and torch.equal(out['visualization']['iuv_pred'][2], eager['idx'])
    d = (out['para'] - ref['para']).abs().max().item()
    frac, agree, flips, raw_err = _decided_index_agrees(model, eng, img, out['visualization']['iuv_pred'][2], ref['visualization']['iuv_pred'][2])
    eager2 = eng.eager(img2)['para'].clone()
    assert torch.equal(eng(img2)['para'], eager2)
    record('infer_engine_vs_infer_net', {'regressor': regressor, 'B': B, 'para_max_abs': d, 'decided': frac, 'flips': flips, 'index_raw_rel': raw_err,
                                         'launches': dict(eng.launches)})
    # bf16 rounding of w * s (and one rounding of the conv + bias + residual + ReLU result instead of two) rather than of w and of
    # the conv output: a few bf16 ulps per layer.  Measured 1.6e-5 (C2) and 2.1e-5 (HRNet-W48) -- infer_net's own distance to the fp32
    # reference is 2.5e-4 (test_gpu_f2); the bound is 25x the worst measurement
    assert d < 5e-4, d
    # (seeded random weights leave the index logits close together: measured 8.6 % of the HRNet pixels and all C2 pixels are
    # decided at 4x the measured raw distance, 2.2e-2 / 3.7e-3 -- on all of them the engine's cleaned index equals infer_net's)
    assert agree and frac > 0.04, (frac, flips, raw_err)
    # the model is untouched: state bit-identical, infer_net bit-identical
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items())
    assert torch.equal(model.infer_net(img)['para'], ref['para'])
    eng.close()


def test_engine_mesh_refresh_and_stale():
    from danet_densepose2smpl_amd.inference import InferenceEngine
    B = 32
    model = _model('hrnet', B)
    img = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(4)).cuda()
    eng = InferenceEngine(model, B, mesh=True)
    out = eng(img)
    para = out['para']
    rot = para[:, 13:].reshape(B, 24, 3, 3)
    sm = model.iuv2smpl.smpl(betas=para[:, 3:13], body_pose=rot[:, 1:], global_orient=rot[:, :1], pose2rot=False)
    assert torch.equal(out['vertices'], sm.vertices) and torch.equal(out['joints'], sm.joints)
    assert not eng.stale()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd['img2iuv.iuv_est.layer1.0.bn2.running_var'] *= 1.5
    key = [k for k in sd if k.startswith('iuv2smpl.') and k.endswith('conv1.weight') and 'limb' in k][0]
    sd[key] = sd[key] * 0.9
    model.load_state_dict(sd)
    assert eng.stale()
    eng.refresh()
    assert not eng.stale()
    new = InferenceEngine(model, B, graph=False, mesh=True).eager(img)
    out = eng(img)
    assert torch.equal(out['para'], new['para']) and torch.equal(out['vertices'], new['vertices'])
    eng.close()


def test_engine_preconditions():
    from danet_densepose2smpl_amd.inference import InferenceEngine
    _cfg(**{'DANET.INIMG_SIZE': 128, 'DANET.HEATMAP_SIZE': 32})
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    model = DaNet(default_options(2), None, pretrained=False)
    with pytest.raises(ValueError, match='inference mode'):
        InferenceEngine(model.cuda().train(), 2)
    with pytest.raises(ValueError, match='GPU'):
        InferenceEngine(model.cpu().eval(), 2)
