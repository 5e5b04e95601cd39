"""BatchNorm-folded, graph-captured inference (the frozen-model form of DaNet.infer_net, danet.py:61-131).

In eval mode every BatchNorm2d is an affine map per channel, so it folds into the convolution in front of it:

    s  = gamma / sqrt(running_var + eps)          (fp64, stored in the weight's dtype)
    w' = w * s                                    (per output channel: dim 0, or dim 1 of a ConvTranspose2d weight)
    b' = beta + (bias - running_mean) * s

and `conv -> bn [-> + residual] [-> relu]` becomes ONE convolution launch whose epilogue adds the bias, the residual and applies the
ReLU (y = bf16(relu(acc + b'[c] + residual)), rounded once): danet_conv_forward, danet_conv_forward_multi_epi (HRNet branch levels and
fuse stages in lockstep), danet_conv_stem_forward_epi (the regressors' 7x7 stems) and danet_conv3x3a_forward_epi (their layer1 blocks).

InferenceEngine never modifies the model.  It runs the model's own forward code on a *shadow* module tree: shallow copies of the
containers (sharing every parameter and buffer) in which each folded convolution is replaced by a `_FoldedConv` holding the engine's
folded, packed weights and each folded BatchNorm by a `_FoldedBN` that launches that convolution with the BatchNorm call's own residual
and ReLU arguments; HighResolutionModules run their branches and exchange paths in lockstep.  Everything that is not a
convolution + BatchNorm (soft-argmax, STN, heads, part cleaning, GCN, rot6d) is the model's code unchanged.
"""
import collections
import copy
import ctypes

import torch
import torch.nn as tnn

from . import _lib
from . import conv as _conv
from .conv import ptr, nptr, check, stream, conv_out_size, nhwc_bf16, _empty_nhwc
from . import nn as _nn

__all__ = ['fold_conv_bn', 'fold_plan', 'FoldPlan', 'InferenceEngine']


# ---------------------------------------------------------------------------------------------------------------------------------
# folding (pure torch: CPU or GPU tensors)

def fold_conv_bn(weight, bias, bn, transposed=False):
    """(w', b') of `bn(conv(x))` with `bn` in eval mode: w' = w * s per output channel, b' = beta + (bias - running_mean) * s,
    s = gamma / sqrt(running_var + eps) computed in fp64.  Output channel: dim 0 of a Conv2d weight (grouped ones included),
    dim 1 of a ConvTranspose2d weight (groups = 1).  New tensors in the weight's dtype; nothing of the inputs is modified."""
    dt = weight.dtype
    var = bn.running_var.detach().double()
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(var)
    s = gamma / torch.sqrt(var + bn.eps)
    w = weight.detach().double()
    shape = [1] * w.dim()
    shape[1 if transposed else 0] = -1
    w2 = (w * s.view(shape)).to(dt)
    b0 = bias.detach().double() if bias is not None else torch.zeros_like(var)
    b2 = (beta + (b0 - bn.running_mean.detach().double()) * s).to(dt)
    return w2.contiguous(), b2.contiguous()


FoldPair = collections.namedtuple('FoldPair', 'conv_name conv bn_name bn transposed')


class FoldPlan(object):
    """pairs: FoldPair per folded BatchNorm; unfolded: names of BatchNorm2d modules the forward calls that have no pair; skipped:
    names of BatchNorm2d modules the forward never calls (the reference allocates them: smpl_regressor.py rot2pos / pos2rot)."""

    def __init__(self, pairs, unfolded, skipped):
        self.pairs, self.unfolded, self.skipped = pairs, unfolded, skipped

    def __len__(self):
        return len(self.pairs)


def fold_plan(model):
    """Pair every BatchNorm2d of `model` with the convolution that feeds it (host only, no kernels)."""
    from .resnet import ConvBN, BasicBlock, Bottleneck, PoseResNet, SmplResNet
    from .hrnet import PoseHighResolutionNet
    from .smpl_regressor import _StemNet, _MlpBnRelu, DecomposedPredictor
    names = {id(m): n for n, m in model.named_modules()}
    pairs, skip = [], set()

    def add(c, b, transposed=False):
        pairs.append(FoldPair(names[id(c)], c, names[id(b)], b, transposed))

    for _, m in model.named_modules():
        if isinstance(m, DecomposedPredictor):
            if m.refine_strategy == 'gcn':
                for unused in (m.rot2pos, m.pos2rot):                 # allocated, never called (smpl_regressor.py)
                    skip.update(id(u) for u in unused.modules())
        elif isinstance(m, (ConvBN, _StemNet)):
            add(m._modules['0'], m._modules['1'])
        elif isinstance(m, _MlpBnRelu):                               # REFINE_STRATEGY 'lstm': rot2pos / pos2rot
            add(m._modules['0'], m._modules['1']); add(m._modules['3'], m._modules['4'])
        elif isinstance(m, BasicBlock):
            add(m.conv1, m.bn1); add(m.conv2, m.bn2)
        elif isinstance(m, Bottleneck):
            add(m.conv1, m.bn1); add(m.conv2, m.bn2); add(m.conv3, m.bn3)
        elif isinstance(m, PoseHighResolutionNet):
            add(m.conv1, m.bn1); add(m.conv2, m.bn2)
        elif isinstance(m, (PoseResNet, SmplResNet)):
            add(m.conv1, m.bn1)
            if isinstance(m, PoseResNet):
                mods = list(m.deconv_layers)
                for i in range(0, len(mods), 3):
                    add(mods[i], mods[i + 1], transposed=True)
    paired = {id(p.bn) for p in pairs}
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, tnn.BatchNorm2d)]
    unfolded = [n for n, m in bns if id(m) not in paired and id(m) not in skip]
    skipped = [n for n, m in bns if id(m) in skip]
    return FoldPlan(pairs, unfolded, skipped)


# ---------------------------------------------------------------------------------------------------------------------------------
# the folded layers

class _Pending(object):
    """What a _FoldedConv returns: the launch waits for the _FoldedBN call that follows, which brings the residual and the ReLU flag."""
    __slots__ = ('conv', 'x')

    def __init__(self, conv, x):
        self.conv, self.x = conv, x


class _FoldedBN(tnn.Module):
    def forward(self, x, res=None, relu=False, link=None):
        if not isinstance(x, _Pending):
            raise RuntimeError('folded BatchNorm called on a tensor that its folded convolution did not produce')
        return x.conv.run(x.x, res, bool(relu))


class _FoldedConv(tnn.Module):
    """conv + folded BatchNorm: fp32 folded weight / bias (self.w, self.b), bf16 packings made on first use per input width."""

    def __init__(self, engine, pair):
        super().__init__()
        c = pair.conv
        self.engine, self.pair, self.transposed = engine, pair, pair.transposed
        self.stride, self.pad, self.dil, self.groups = c.stride[0], c.padding[0], c.dilation[0], c.groups
        self.outpad = c.output_padding[0] if pair.transposed else 0
        self.R, self.S = c.kernel_size
        self.w, self.b = fold_conv_bn(c.weight, c.bias, pair.bn, pair.transposed)
        self.packs = {}            # (mode key) -> (bf16 buffer, recipe for refresh)
        self.in_channels = c.in_channels
        self.out_channels = c.out_channels

    def forward(self, x, link=None):
        return _Pending(self, x)

    # -- refolding in place (InferenceEngine.refresh): same tensors, same packed buffers
    def refold(self):
        c = self.pair.conv
        w, b = fold_conv_bn(c.weight, c.bias, self.pair.bn, self.transposed)
        self.w.copy_(w)
        self.b.copy_(b)
        for key, (buf, recipe) in self.packs.items():
            self._pack_into(buf, *recipe)

    def _pack_into(self, buf, src, bpad, bias_src, Cout, Cin_g, mode, chunk):
        src_now = src()
        L = _lib.lib()
        check(L.danet_conv_pack_weights_padded(ptr(src_now), ptr(buf), Cout, Cin_g, self.R, self.S, self.groups if not self.transposed else 1, mode,
                                               chunk, src_now.shape[0] // (self.groups if not self.transposed else 1), src_now.shape[1], stream()),
              'danet_conv_pack_weights')
        if bpad is not None:
            bpad.zero_()
            bs = bias_src()
            if self.groups > 1 and bpad.numel() != bs.numel():
                bpad.view(self.groups, -1)[:, :bs.numel() // self.groups].copy_(bs.view(self.groups, -1))
            else:
                bpad[:bs.numel()].copy_(bs)

    def _packed(self, key, Cout, Cin_g, mode, chunk):
        """(bf16 packed weight at widths (Cout, Cin_g), fp32 bias padded to Cout); made once, refreshed in place."""
        hit = self.packs.get(key)
        if hit is None:
            L = _lib.lib()
            g = self.groups if not self.transposed else 1
            n = L.danet_conv_packed_elems(Cout // g, Cin_g, self.R, self.S, g, mode, chunk)
            buf = torch.empty(n, dtype=torch.bfloat16, device=self.w.device)
            bpad = torch.zeros((Cout + 3) // 4 * 4, dtype=torch.float32, device=self.w.device)
            # (a transposed layer: its [Cin, Cout, R, S] weight in the data-gradient packing of the gather kernel, as deconv.py runs it)
            recipe = (lambda: self.w, bpad, lambda: self.b, Cout, Cin_g, mode, chunk)
            self._pack_into(buf, *recipe)
            hit = self.packs[key] = (buf, recipe)
        return hit[0], hit[1][1]

    def run(self, x, res, relu):
        if _conv.fp32_mode():
            return self._run_f32(x, res, relu)
        return self._run_bf16(x, res, relu)

    def _run_f32(self, x, res, relu):
        """The fp32 verification mode: the existing fp32 kernels with the folded bias, then the HIP sum / ReLU kernel."""
        from .deconv import ConvTranspose2dF32Function
        if self.transposed:
            y = ConvTranspose2dF32Function.apply(x, self.w, self.b, self.stride, self.pad, self.outpad)
        else:
            if x.shape[1] != self.w.shape[1] * self.groups:
                x = x[:, :self.w.shape[1] * self.groups]
            y = _conv.Conv2dF32Function.apply(x, self.w, self.b, self.stride, self.pad, self.dil, self.groups)
        if res is not None:
            return _nn.sum_relu([y, res], [0, 0], relu)
        return _nn.sum_relu([y], [0], True) if relu else y

    def _widths(self, x):
        """(x as the kernels take it, padc, padn, Cout padded, Cin_g padded) by conv.channel_padding, the rule conv2d pads by."""
        Cout, Cin_w = self.w.shape[0], self.w.shape[1]
        padc, pad_x, padn = _conv.channel_padding(x.shape[1], Cin_w, Cout, self.groups)
        if pad_x:
            x = _conv._pad_channels_nhwc(x)
        return nhwc_bf16(x), padc, padn, self.groups * (Cout // self.groups + padn), Cin_w + padc

    def _run_bf16(self, x, res, relu):
        L = _lib.lib()
        if self.transposed:
            x = nhwc_bf16(x)
            B, Cin, H, W = x.shape
            Cout = self.w.shape[1]
            OH, OW = (H - 1) * self.stride - 2 * self.pad + self.R + self.outpad, (W - 1) * self.stride - 2 * self.pad + self.S + self.outpad
            wp, b = self._packed('t', Cin, Cout, 1, 0)
            y = _conv._conv_fwd_raw(x, wp, b, B, H, W, Cin, OH, OW, Cout, self.R, self.S, self.stride, self.pad, 1, 1, True, relu and res is None,
                                    False)
            self.engine.launches['conv_transposed'] += 1
            return y if res is None else _nn.sum_relu([y, res], [0, 0], relu)
        x, padc, padn, Cout_p, Cin_gp = self._widths(x)
        B, Cin, H, W = x.shape
        g = self.groups
        OH, OW = conv_out_size(H, self.R, self.stride, self.pad, self.dil), conv_out_size(W, self.S, self.stride, self.pad, self.dil)
        y = None
        if res is None and not padn and L.danet_conv_stem_ok(B, H, W, Cin, OH, OW, Cout_p, self.R, self.S, self.stride, self.pad, self.dil, g):
            wp, b = self._packed(('s', padc), Cout_p, Cin_gp, 0, 16)
            y = _empty_nhwc(B, Cout_p, OH, OW, torch.bfloat16, x.device)
            check(L.danet_conv_stem_forward_epi(nptr(x), ptr(wp), ptr(b), nptr(y), B, H, W, Cin, OH, OW, Cout_p,
                                                int(relu), stream()), 'danet_conv_stem_forward_epi')
            self.engine.launches['conv_stem_bias'] += 1
            return y
        if not padn and W in _conv.C3A_WIDTHS and L.danet_conv3x3a_ok(B, H, W, Cin, Cout_p, self.R, self.S, self.stride, self.pad, self.dil, g):
            wp, b = self._packed(('a', padc), Cout_p, Cin_gp, 0, 16)
            y = _empty_nhwc(B, Cout_p, OH, OW, torch.bfloat16, x.device)
            add = None if res is None else nhwc_bf16(res)
            check(L.danet_conv3x3a_forward_epi(nptr(x), ptr(wp), ptr(b), nptr(add),
                                               nptr(y), B, H, W, int(relu), stream()), 'danet_conv3x3a_forward_epi')
            self.engine.launches['conv3x3a_bias'] += 1
            return y
        wp, b = self._packed(('g', padc), Cout_p, Cin_gp, 0, 0)
        kid = L.danet_conv_forward_kernel(B, H, W, Cin, OH, OW, Cout_p, self.R, self.S, self.stride, self.pad, self.dil, g, 0, 0)
        fuse_res = res is not None and not padn and kid % 10 in (1, 2, 3) and tuple(res.shape) == (B, Cout_p, OH, OW)
        add = nhwc_bf16(res) if fuse_res else None
        y = _conv._conv_fwd_raw(x, wp, b, B, H, W, Cin, OH, OW, Cout_p, self.R, self.S, self.stride, self.pad, self.dil, g, False,
                                relu and (res is None or fuse_res), False, addend=add)
        self.engine.launches['conv'] += 1
        if padn:
            y = _conv._crop_group_padding(y, g, Cout_p // g - padn, padn)
        if res is not None and not fuse_res:
            self.engine.launches['sum_relu'] += 1
            y = _nn.sum_relu([y, res], [0, 0], relu)
        return y

    # -- a lockstep job (danet_conv_forward_multi_epi): None when this layer does not run on the multi-problem kernels as it is
    def job(self, job, x, res, relu):
        if self.transposed or _conv.fp32_mode():
            return None
        x, padc, padn, Cout_p, Cin_gp = self._widths(x)
        if padc or padn or x.shape[1] % 8:
            return None
        B, Cin, H, W = x.shape
        OH, OW = conv_out_size(H, self.R, self.stride, self.pad, self.dil), conv_out_size(W, self.S, self.stride, self.pad, self.dil)
        if res is not None and tuple(res.shape) != (B, Cout_p, OH, OW):
            return None
        wp, b = self._packed(('g', 0), Cout_p, Cin_gp, 0, 0)
        y = _empty_nhwc(B, Cout_p, OH, OW, torch.bfloat16, x.device)
        add = None if res is None else nhwc_bf16(res)
        _conv._conv_job(job.j, x, wp, y, (B, H, W, Cin, OH, OW, Cout_p, self.R, self.S, self.stride, self.pad, self.dil, self.groups), False, addend=add)
        job.bias, job.relu = b.data_ptr(), int(relu)
        return (y, x, wp, b, add)          # (keeps the operands alive until the launch is queued)


def _run_multi(engine, items):
    """[conv.run(x, res, relu) for (conv, x, res, relu) in items] with as few danet_conv_forward_multi_epi launches as qualify: the whole
    set, else the subsets of equal danet_conv_nt (the kernels' channel-block count), else layer by layer."""
    L = _lib.lib()
    out = [None] * len(items)
    if not _conv.fp32_mode() and len(items) > 1:
        jobs = (_lib.ConvJobEpi * len(items))()
        keep = [it[0].job(jobs[k], it[1], it[2], it[3]) for k, it in enumerate(items)]
        todo = [k for k in range(len(items)) if keep[k] is not None]
        sets = [todo]
        if len(todo) > 1:
            arr = (_lib.ConvJobEpi * len(todo))(*[jobs[k] for k in todo])
            if len(todo) > 12 or not L.danet_conv_forward_multi_epi_ok(ctypes.addressof(arr), len(todo)):
                by = collections.OrderedDict()
                for k in todo:
                    by.setdefault(int(L.danet_conv_nt(jobs[k].j.Cout // jobs[k].j.groups)), []).append(k)
                sets = list(by.values())
        for s in sets:
            for g0 in range(0, len(s), 12):
                sub = s[g0:g0 + 12]
                if len(sub) < 2:
                    continue
                arr = (_lib.ConvJobEpi * len(sub))(*[jobs[k] for k in sub])
                if not L.danet_conv_forward_multi_epi_ok(ctypes.addressof(arr), len(sub)):
                    continue
                check(L.danet_conv_forward_multi_epi(ctypes.addressof(arr), len(sub), stream()), 'danet_conv_forward_multi_epi')
                engine.launches['conv_multi_epi'] += 1
                engine.launches['conv_multi_epi_problems'] += len(sub)
                for k in sub:
                    out[k] = keep[k][0]
    for k, (c, x, res, relu) in enumerate(items):
        if out[k] is None:
            out[k] = c.run(x, res, relu)
    return out


def _folded_hr_forward(self, x):
    """HighResolutionModule.forward in eval mode on folded layers: the branches advance one BasicBlock level at a time (conv1 of every
    branch in one launch, conv2 + identity + ReLU in one), the exchange paths one stage at a time, then the fuse sums in one launch."""
    from .resnet import BasicBlock
    eng = self._engine
    if self.num_branches == 1:
        return [self.branches[0](x[0])]
    lock = all(len(br) == len(self.branches[0]) and all(isinstance(b, BasicBlock) and b.downsample is None for b in br) for br in self.branches)
    if lock:
        xs = list(x[:self.num_branches])
        for k in range(len(self.branches[0])):
            blocks = [br[k] for br in self.branches]
            h = _run_multi(eng, [(b.conv1, v, None, True) for b, v in zip(blocks, xs)])
            xs = _run_multi(eng, [(b.conv2, v, r, True) for b, v, r in zip(blocks, h, xs)])
    else:
        xs = [self.branches[i](x[i]) for i in range(self.num_branches)]
    nout = len(self.fuse_layers)
    paths = {}
    for i in range(nout):
        for j in range(self.num_branches):
            if j != i:
                m = self.fuse_layers[i][j]
                paths[(i, j)] = [m] if '0' in m._modules and isinstance(m._modules['0'], _FoldedConv) else list(m._modules.values())
    cur = {key: xs[key[1]] for key in paths}
    for k in range(max(len(st) for st in paths.values())):
        keys = [key for key, st in paths.items() if len(st) > k]
        keys.sort(key=lambda key: (paths[key][k]._modules['0'].out_channels % 48 == 0, paths[key][k]._modules['0'].out_channels))
        h = _run_multi(eng, [(paths[key][k]._modules['0'], cur[key], None, bool(paths[key][k].relu)) for key in keys])
        for key, v in zip(keys, h):
            cur[key] = v
    groups = []
    for i in range(nout):
        terms = [xs[j] if j == i else cur[(i, j)] for j in range(self.num_branches)]
        shifts = [j - i if j > i else 0 for j in range(self.num_branches)]
        groups.append((terms, shifts))
    return _nn.sum_relu_multi(groups, relu=True)


def _folded_bottleneck_forward(self, x):
    """Bottleneck.forward on folded layers (every width, the padded-width heat-map block included: _FoldedConv pads as conv2d does)."""
    residual = x if self.downsample is None else self.downsample(x)
    out = self.bn1(self.conv1(x), relu=True)
    out = self.bn2(self.conv2(out), relu=True)
    return self.bn3(self.conv3(out), res=residual, relu=True)


# ---------------------------------------------------------------------------------------------------------------------------------

class InferenceEngine(object):
    """Folded, graph-captured DaNet.infer_net.

    engine = InferenceEngine(model, batch_size, img_size=None, graph=True, mesh=False); out = engine(image)

    `out` has infer_net's keys ('para' [B, 229], 'visualization' with 'iuv_pred', 'part_iuv_pred' and what smpl_infer_net adds), plus
    'vertices' / 'joints' (model.iuv2smpl.smpl on 'para') with mesh=True.  With graph=True the first call at (batch_size, 3, H, W)
    warms up twice and captures the whole inference as one graph; later calls copy the image in and replay.  THE RETURNED TENSORS ARE THE
    ENGINE'S STATIC BUFFERS: they stay valid until the next call (clone what must outlive it).  Other shapes, and the fp32 verification
    mode (conv.precision('fp32')), run the same folded layers eagerly.  The model is never modified; after load_state_dict (or any other
    in-place change of a folded parameter / running statistic) stale() turns True and refresh() refolds and repacks into the same buffers,
    so a captured graph stays valid.  close() releases the graph and its memory pool."""

    def __init__(self, model, batch_size, img_size=None, graph=True, mesh=False):
        if getattr(model.img2iuv, 'input_mode', 'iuv') == 'iuv_gt':
            raise NotImplementedError("InferenceEngine folds the IUV backbone's BatchNorms and captures image -> para; DANET.INPUT_MODE "
                                      "'iuv_gt' has no backbone and takes (image, iuv_image_gt, smpl_kps_gt): use DaNet.infer_net")
        if model.training:
            raise ValueError('You should call this function only on inference.'
                             'Set the network in inference mode by net.eval().')
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise ValueError('InferenceEngine needs the model on a GPU (got %s)' % dev)
        from .config import cfg
        self.model, self.device = model, dev
        self.batch_size = int(batch_size)
        self.img_size = int(img_size if img_size is not None else cfg.DANET.INIMG_SIZE)
        self.use_graph, self.mesh = bool(graph), bool(mesh)
        self.launches = collections.Counter()
        self.plan = fold_plan(model)
        if self.plan.unfolded:
            raise RuntimeError('BatchNorms without a convolution to fold into: %s' % self.plan.unfolded[:5])
        self.folded = [_FoldedConv(self, p) for p in self.plan.pairs]
        self._shadow = self._build_shadow()
        self._versions = self._source_versions()
        self._graph = self._pool = self._static_in = self._static_out = None

    # -- the shadow tree
    def _build_shadow(self):
        from .hrnet import HighResolutionModule
        from .resnet import Bottleneck
        repl = {}
        for f in self.folded:
            repl[id(f.pair.conv)] = f
            repl[id(f.pair.bn)] = _FoldedBN()
        need = set()
        for m in self.model.modules():
            if isinstance(m, (HighResolutionModule, Bottleneck)) or any(id(c) in repl for c in m.children()):
                need.add(id(m))
        changed = True
        while changed:                                  # every ancestor of a replaced module is copied too
            changed = False
            for m in self.model.modules():
                if id(m) not in need and any(id(c) in need for c in m.children()):
                    need.add(id(m))
                    changed = True
        memo = {}

        def shadow(m):
            if id(m) in repl:
                return repl[id(m)]
            if id(m) not in need:
                return m
            if id(m) in memo:
                return memo[id(m)]
            s = copy.copy(m)
            memo[id(m)] = s
            s._modules = collections.OrderedDict((k, None if c is None else shadow(c)) for k, c in m._modules.items())
            if isinstance(m, HighResolutionModule):
                s._engine = self
                s.forward = _folded_hr_forward.__get__(s)
            elif isinstance(m, Bottleneck):
                s.forward = _folded_bottleneck_forward.__get__(s)
            return s
        return shadow(self.model)

    # -- staleness / refolding
    def _source_versions(self):
        vs = []
        for p in self.plan.pairs:
            for t in (p.conv.weight, p.conv.bias, p.bn.weight, p.bn.bias, p.bn.running_mean, p.bn.running_var):
                vs.append(None if t is None else t._version)
        return vs

    def stale(self):
        """True when a folded parameter or running statistic changed in place since the last fold (load_state_dict, an optimizer step)."""
        return self._source_versions() != self._versions

    def refresh(self):
        """Refold and repack into the engine's existing buffers (a captured graph stays valid)."""
        with torch.no_grad():
            for f in self.folded:
                f.refold()
        self._versions = self._source_versions()

    # -- running
    def _forward(self, image):
        with torch.no_grad():
            rd = self._shadow.infer_net(image)
            if self.mesh:
                para = rd['para']
                B = para.shape[0]
                rot = para[:, 13:].reshape(B, 24, 3, 3)
                out = self.model.iuv2smpl.smpl(betas=para[:, 3:13], body_pose=rot[:, 1:], global_orient=rot[:, :1], pose2rot=False)
                rd['vertices'], rd['joints'] = out.vertices, out.joints
            return rd

    def eager(self, image):
        """The folded forward without the graph (any shape)."""
        return self._forward(image)

    def __call__(self, image):
        static_shape = (self.batch_size, 3, self.img_size, self.img_size)
        if not self.use_graph or _conv.fp32_mode() or tuple(image.shape) != static_shape:
            return self._forward(image)
        if self._graph is None:
            self._capture(image)
        self._static_in.copy_(image)
        self._graph.replay()
        return self._static_out

    def _capture(self, image, warmup=2):
        self._static_in = image.detach().clone()
        side = _nn.SideBranch(torch.cuda.Stream(device=self.device))
        with side.fork():
            for _ in range(warmup):
                self._forward(self._static_in)
        side.join()
        torch.cuda.synchronize(self.device)
        self._pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._pool):
            self._static_out = self._forward(self._static_in)
        torch.cuda.synchronize(self.device)
        self._graph = g

    def close(self):
        """Release the captured graph, its static buffers and its memory pool."""
        self._graph = self._static_out = self._static_in = self._pool = None
        torch.cuda.empty_cache()
