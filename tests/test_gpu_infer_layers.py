"""Every convolution launch of the inference engine (danet_densepose2smpl_amd/inference.py) against an fp64 evaluation of the same
operation on the exact operands the kernel consumed, layer by layer, within the rounding bound of tests/conv_bound.py -- on both
backbones at batch sizes on both sides of each epilogue kernel's batch threshold -- plus graph replay at small batch sizes.

The engine is instrumented from here (monkeypatch on _FoldedConv.run and inference._run_multi): each folded launch is checked right after
it returns, its path read off the change of engine.launches, and the per-path worst ratios and the path census go to record()."""
import collections
import os
import sys

import pytest
import torch

from conftest import record
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_bound import U_BF16, U_F32, reference, check    # noqa: E402
from test_gpu_infer import _model    # noqa: E402

pytestmark = pytest.mark.gpu

BIG_B = 1024        # a batch size past every kernel's batch threshold: what a layer's geometry alone would allow


def _items(n, B):
    """Batch items of a layer with n items to check in an engine run at batch size B: all of them up to B = 3, else the first, a middle
    one and the last (the tile tails live there)."""
    return list(range(n)) if B <= 3 else sorted({0, n // 2, n - 1})


class LayerCheck(object):
    """Wraps the engine's launch points (install); checks every folded launch once, right after it ran."""

    def __init__(self, eng, B, fp32):
        from danet_densepose2smpl_amd import _lib, conv
        self.eng, self.B, self.fp32 = eng, B, fp32
        self.L, self.conv = _lib.lib(), conv
        self.u = U_F32 if fp32 else U_BF16
        self.census = collections.Counter()
        self.worst = {}                        # path -> [worst elementwise ratio, worst per-channel mean ratio]
        self.seen = set()                      # ids of the folded convs checked
        self.multi = None                      # ids of the convs a running _run_multi handed back to run()

    # -- what a launch was
    def _path(self, delta, res, relu):
        if self.fp32:
            return 'f32_transposed' if delta.get('_t') else ('f32_sum_relu' if res is not None or relu else 'f32_conv')
        keys = {k for k, v in delta.items() if v}
        if keys in ({'conv_transposed'}, {'conv_stem_bias'}, {'conv3x3a_bias'}):
            return keys.pop()
        if keys == {'conv'}:
            return 'conv' if res is None else 'conv_addend'
        if keys == {'conv', 'sum_relu'}:
            return 'conv_sum_relu'
        raise AssertionError('a folded launch with an unknown launch pattern: %s' % dict(delta))

    def _geometry(self, fc, x, path):
        """census flags: padded widths, groups, and layers the stem / conv3x3a epilogue kernels would take at a larger batch."""
        if fc.transposed:
            return
        g = fc.groups
        if (-(fc.out_channels // g)) % 8:
            self.census['padn'] += 1
        if x.shape[1] != fc.in_channels or (g == 1 and fc.in_channels % 8):
            self.census['padc'] += 1
        if g > 1:
            self.census['grouped'] += 1
        B, Cin, H, W = x.shape
        Cin_p = Cin + (-Cin) % 8 if g == 1 else Cin
        OH, OW = self.conv.conv_out_size(H, fc.R, fc.stride, fc.pad, fc.dil), self.conv.conv_out_size(W, fc.S, fc.stride, fc.pad, fc.dil)
        if self.fp32 or (-(fc.out_channels // g)) % 8:
            return
        stem = self.L.danet_conv_stem_ok(BIG_B, H, W, Cin_p, OH, OW, fc.out_channels, fc.R, fc.S, fc.stride, fc.pad, fc.dil, g)
        c3a = W in self.conv.C3A_WIDTHS and self.L.danet_conv3x3a_ok(BIG_B, H, W, Cin_p, fc.out_channels, fc.R, fc.S, fc.stride, fc.pad,
                                                                      fc.dil, g)
        if stem and path != 'conv_stem_bias':
            self.census['fallback_stem'] += 1
        if c3a and path not in ('conv3x3a_bias', 'conv_stem_bias'):
            self.census['fallback_conv3x3a'] += 1

    # -- the check
    def check(self, fc, x, res, relu, y, path):
        self.census[path] += 1
        self.seen.add(id(fc))
        self._geometry(fc, x, path)
        idx = _items(x.shape[0], self.B)
        sel = torch.tensor(idx, device=x.device)
        xi = x.index_select(0, sel)
        ri = None if res is None else res.index_select(0, sel)
        if self.fp32:
            xq, wq, rq = xi.float(), fc.w, ri
            if not fc.transposed:
                xq = xq[:, :fc.in_channels]
        else:
            xq = xi.bfloat16() if fc.transposed else xi[:, :fc.in_channels].bfloat16()      # the padded channels are zeros
            wq, rq = fc.w.bfloat16(), None if ri is None else ri.bfloat16()
        ref = reference(xq, wq, fc.b, rq, relu, fc.stride, fc.pad, fc.dil, fc.groups, fc.transposed, fc.outpad)
        rounded_conv = self.fp32 or path == 'conv_sum_relu' or (path == 'conv_transposed' and res is not None)
        what = (path, fc.pair.conv_name, tuple(x.shape), tuple(y.shape))
        elem, mean = check(y.index_select(0, sel), ref, self.u, what, rounded_conv=rounded_conv)
        w = self.worst.setdefault(path, [0.0, 0.0])
        w[0], w[1] = max(w[0], elem), max(w[1], mean)

    # -- the instrumented launch points
    def install(self, monkeypatch):
        from danet_densepose2smpl_amd import inference
        orig_run, orig_multi = inference._FoldedConv.run, inference._run_multi
        me = self

        def run(fc, x, res, relu):
            before = collections.Counter(me.eng.launches)
            y = orig_run(fc, x, res, relu)
            delta = collections.Counter(me.eng.launches)
            delta.subtract(before)
            if me.fp32 and fc.transposed:
                delta['_t'] = 1
            if me.multi is not None:
                me.multi.add(id(fc))
            me.check(fc, x, res, relu, y, me._path(delta, res, relu))
            return y

        def run_multi(engine, items):
            outer, me.multi = me.multi, set()
            try:
                before = engine.launches['conv_multi_epi']
                out = orig_multi(engine, items)
                handed_back = me.multi
            finally:
                me.multi = outer
            if not me.fp32:
                me.census['fallback_multi'] += sum(id(it[0]) in handed_back for it in items) if len(items) > 1 else 0
                assert (engine.launches['conv_multi_epi'] > before) == any(id(it[0]) not in handed_back for it in items)
            for (fc, x, res, relu), y in zip(items, out):
                if id(fc) not in handed_back:
                    me.check(fc, x, res, relu, y, 'conv_multi_epi')
            return out

        monkeypatch.setattr(inference._FoldedConv, 'run', run)
        monkeypatch.setattr(inference, '_run_multi', run_multi)


def _image(B, seed):
    return torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(seed)).cuda()


# per case: the paths that must run (> 0) and must not (== 0) -- from the kernels' _ok predicates at the regressor's crop counts
# (24 B crops; stem epilogue: >= 64 crops, B >= 3; conv3x3a epilogue on the 16 x 16 maps: >= 256 crops, B >= 11).  The body regressor's
# stem sees B crops and stays on the generic kernel at every size here.  Together with test_engine_fallback_paths_match_fp64 (the two
# paths these networks never take at these sizes: a multi-problem set split and handed back, a rounded conv + sum / ReLU) every launch
# path runs, and each epilogue kernel both runs and falls back.
def _expected(regressor, B):
    run = {'conv', 'conv_addend', 'padc', 'grouped'}
    none = set()
    run |= {'conv_stem_bias'} if B >= 3 else {'fallback_stem'}
    none |= set() if B >= 3 else {'conv_stem_bias'}
    run |= {'conv3x3a_bias'} if B >= 11 else {'fallback_conv3x3a'}
    none |= set() if B >= 11 else {'conv3x3a_bias'}
    run |= {'conv_multi_epi', 'padn'} if regressor == 'hrnet' else {'conv_transposed'}
    return run, none


@pytest.mark.parametrize('regressor,B', [('hrnet', 1), ('hrnet', 3), ('hrnet', 32), ('resnet', 1), ('resnet', 3), ('resnet', 16)])
def test_every_engine_launch_matches_fp64(regressor, B, monkeypatch):
    """bf16 engine (eager): every folded launch within the single-rounding bound (two roundings where the conv is rounded before a
    separate sum / ReLU launch) and the per-channel mean check."""
    model = _model(regressor, B)
    eng = model.inference_engine(B)
    chk = LayerCheck(eng, B, fp32=False)
    chk.install(monkeypatch)
    out = eng.eager(_image(B, 5))
    torch.cuda.synchronize()
    assert torch.isfinite(out['para']).all()
    census = dict(chk.census)
    record('infer_layers_fp64', {'regressor': regressor, 'B': B, 'precision': 'bf16', 'worst': chk.worst, 'census': census})
    assert chk.seen == {id(f) for f in eng.folded}, (len(chk.seen), len(eng.folded))
    run, none = _expected(regressor, B)
    assert all(census.get(k, 0) > 0 for k in run), (sorted(run), census)
    assert all(census.get(k, 0) == 0 for k in none), (sorted(none), census)
    eng.close()


def test_engine_fallback_paths_match_fp64(monkeypatch):
    """The engine's fallbacks that HRNet-W48 / ResNet-50 do not reach at 256^2, on the engine's own folded layers (HRNet, B = 3):
    _run_multi with a set no kernel takes whole (pointwise jobs of two channel-block counts: split by count, the single job handed back
    to run()), and a residual on output-channel-padded layers (the heat-map head's 12-wide Bottleneck: conv rounded, then sum / ReLU)."""
    from danet_densepose2smpl_amd import inference, _lib
    L = _lib.lib()
    B, H = 3, 16
    model = _model('hrnet', B)
    eng = model.inference_engine(B)
    chk = LayerCheck(eng, B, fp32=False)
    chk.install(monkeypatch)
    g = torch.Generator().manual_seed(11)
    act = lambda C: torch.randn(B, C, H, H, generator=g).cuda()
    by_nt = {}
    for f in eng.folded:
        if not f.transposed and f.R == 1 and f.stride == 1 and f.groups == 1 and f.in_channels % 8 == 0 and f.out_channels % 8 == 0:
            by_nt.setdefault(int(L.danet_conv_nt(f.out_channels)), []).append(f)
    pairs = [v for v in by_nt.values() if len(v) >= 2]
    assert pairs and len(by_nt) >= 2, {k: len(v) for k, v in by_nt.items()}
    a0, a1 = pairs[0][:2]
    b0 = next(v[0] for v in by_nt.values() if v is not pairs[0])
    items = [(a0, act(a0.in_channels), None, True), (b0, act(b0.in_channels), act(b0.out_channels), False),
             (a1, act(a1.in_channels), act(a1.out_channels), True)]
    before = eng.launches['conv_multi_epi']
    out = inference._run_multi(eng, items)
    assert eng.launches['conv_multi_epi'] == before + 1 and len(out) == 3
    assert chk.census['conv_multi_epi'] == 2 and chk.census['fallback_multi'] == 1, dict(chk.census)
    head = [f for f in eng.folded if '.predict_hm.' in f.pair.conv_name and f.out_channels % 8]
    assert head
    for f in head:
        f.run(act(f.in_channels), act(f.out_channels), True)
    torch.cuda.synchronize()
    census = dict(chk.census)
    record('infer_layers_fp64_fallbacks', {'worst': chk.worst, 'census': census})
    assert census.get('conv_sum_relu', 0) == len(head) and census.get('padn', 0) == len(head), census
    eng.close()


@pytest.mark.parametrize('regressor', ['hrnet', 'resnet'])
def test_fp32_mode_every_launch_matches_fp64(regressor, monkeypatch):
    """The fp32 verification mode (_run_f32: the fp32 kernels with the folded bias, then the sum / ReLU kernel) at B = 3."""
    from danet_densepose2smpl_amd import conv
    B = 3
    model = _model(regressor, B)
    eng = model.inference_engine(B)
    chk = LayerCheck(eng, B, fp32=True)
    chk.install(monkeypatch)
    with conv.precision('fp32'):
        out = eng.eager(_image(B, 6))
    torch.cuda.synchronize()
    assert torch.isfinite(out['para']).all()
    census = dict(chk.census)
    record('infer_layers_fp64', {'regressor': regressor, 'B': B, 'precision': 'fp32', 'worst': chk.worst, 'census': census})
    assert chk.seen == {id(f) for f in eng.folded}, (len(chk.seen), len(eng.folded))
    assert census.get('f32_conv', 0) > 0 and census.get('f32_sum_relu', 0) > 0, census
    assert (census.get('f32_transposed', 0) > 0) == (regressor == 'resnet'), census
    eng.close()


@pytest.mark.parametrize('regressor,B', [('hrnet', 1), ('hrnet', 3), ('resnet', 1), ('resnet', 3)])
def test_graph_replay_at_small_batch_sizes(regressor, B):
    """Graph replay == the engine run eagerly, bit for bit, on two images through the same static input; para within infer_net's
    5e-4 (tests/test_gpu_infer.py); the model untouched."""
    model = _model(regressor, B)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    eng = model.inference_engine(B)
    for seed in (7, 8):
        img = _image(B, seed)
        ref = model.infer_net(img)['para'].clone()
        eager = eng.eager(img)
        e_para, e_idx = eager['para'].clone(), eager['visualization']['iuv_pred'][2].clone()
        out = eng(img)
        assert eng._graph is not None
        assert torch.equal(out['para'], e_para) and torch.equal(out['visualization']['iuv_pred'][2], e_idx), seed
        d = (out['para'] - ref).abs().max().item()
        record('infer_graph_small_batch', {'regressor': regressor, 'B': B, 'seed': seed, 'para_max_abs': d})
        assert d < 5e-4, d
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items())
    eng.close()
