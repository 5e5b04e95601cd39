"""The LSTM tree refinement of REFINE_STRATEGY 'lstm' / 'lstm_direct' as one op (csrc/lstm_tree.hip;
/root/reference/models/danet/smpl_regressor.py:742-822).

`lstm_tree(pos, lstms)` maps pos [B,24,128] to cat(pos, pos) + the bidirectional LSTM outputs along the six chains of the SMPL
tree, [B,24,256]: two launches forward, three backward.  `LimbLSTM` holds the parameters of one
nn.LSTM(128, 128, batch_first=True, bidirectional=True) under nn.LSTM's names, so state dicts and checkpoints of the reference
load unchanged; it has no forward of its own (nothing here runs torch's LSTM, i.e. MIOpen).
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, stream, f32c as _f32, require_gpu

# the chains (joints, LSTM index) in the reference's order (limb_branch_lstm, smpl_regressor.py:470-476); c1..c3 start from c0's
# final state.  The kernel holds the same table (csrc/lstm_tree.hip kJoint / kLstm).
CHAINS = [((0, 3, 6, 9), 0), ((12, 15), 0), ((9, 13, 16, 18, 20, 22), 1), ((9, 14, 17, 19, 21, 23), 2),
          ((0, 1, 4, 7, 10), 3), ((0, 2, 5, 8, 11), 4)]
NUM_LSTMS = 5


class LimbLSTM(nn.Module):
    """The parameters of nn.LSTM(input_size, hidden_size, num_layers=1, batch_first=True, bidirectional=True): weight_ih_l0,
    weight_hh_l0, bias_ih_l0, bias_hh_l0 and their `_reverse` twins, initialised as nn.LSTM does (U(-1/sqrt(H), 1/sqrt(H)))."""

    def __init__(self, input_size=128, hidden_size=128):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        for sfx in ('', '_reverse'):
            self.register_parameter('weight_ih_l0' + sfx, nn.Parameter(torch.empty(4 * hidden_size, input_size)))
            self.register_parameter('weight_hh_l0' + sfx, nn.Parameter(torch.empty(4 * hidden_size, hidden_size)))
            self.register_parameter('bias_ih_l0' + sfx, nn.Parameter(torch.empty(4 * hidden_size)))
            self.register_parameter('bias_hh_l0' + sfx, nn.Parameter(torch.empty(4 * hidden_size)))
        self.reset_parameters()

    def reset_parameters(self):
        s = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -s, s)

    def flat(self):
        """[w_ih, w_hh, b_ih, b_hh] of the forward direction, then of the reverse direction."""
        return [self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                self.weight_ih_l0_reverse, self.weight_hh_l0_reverse, self.bias_ih_l0_reverse, self.bias_hh_l0_reverse]

    def forward(self, *args):
        raise RuntimeError('LimbLSTM runs only inside lstm_tree() (csrc/lstm_tree.hip)')


def _fill_params(a, ps, grads=False):
    """ps: 40 tensors, LSTM-major, then direction, then (w_ih, w_hh, b_ih, b_hh)."""
    names = ('g_w_ih', 'g_w_hh', 'g_b_ih', 'g_b_hh') if grads else ('w_ih', 'w_hh', 'b_ih', 'b_hh')
    for k in range(NUM_LSTMS):
        for d in range(2):
            for m, n in enumerate(names):
                getattr(a, n)[k][d] = ps[k * 8 + d * 4 + m].data_ptr()


class LstmTreeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, *params):
        L = _lib.lib()
        B = pos.shape[0]
        if pos.dim() != 3 or tuple(pos.shape[1:]) != (24, 128) or len(params) != 8 * NUM_LSTMS:
            raise ValueError('lstm_tree: pos must be [B,24,128] with 5 LSTMs of 128 units (got %s)' % (tuple(pos.shape),))
        if not L.danet_lstm_tree_ok(B):
            raise ValueError('lstm_tree: unsupported batch %d' % B)
        x = _f32(pos)
        require_gpu(x, 'lstm_tree')
        ps = [_f32(p) for p in params]
        ws = torch.empty(L.danet_lstm_tree_ws_floats(B), dtype=torch.float32, device=x.device)
        out = torch.empty(B, 24, 256, dtype=torch.float32, device=x.device)
        a = _lib.LstmTreeArgs()
        a.pos, a.out, a.ws, a.B = x.data_ptr(), out.data_ptr(), ws.data_ptr(), B
        _fill_params(a, ps)
        check(L.danet_lstm_tree_forward(ctypes.addressof(a), stream()), 'danet_lstm_tree_forward')
        ctx.save_for_backward(x, ws, *ps)
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    def backward(ctx, g_out):
        L = _lib.lib()
        x, ws = ctx.saved_tensors[:2]
        ps = list(ctx.saved_tensors[2:])
        B = x.shape[0]
        go = _f32(g_out)
        g_pos = torch.empty_like(x)
        gp = [torch.empty_like(p) for p in ps]
        scratch = torch.empty(L.danet_lstm_tree_scratch_floats(B), dtype=torch.float32, device=x.device)
        a = _lib.LstmTreeArgs()
        a.pos, a.ws, a.g_out, a.scratch, a.g_pos, a.B = x.data_ptr(), ws.data_ptr(), go.data_ptr(), scratch.data_ptr(), g_pos.data_ptr(), B
        _fill_params(a, ps)
        _fill_params(a, gp, grads=True)
        check(L.danet_lstm_tree_backward(ctypes.addressof(a), stream()), 'danet_lstm_tree_backward')
        return (g_pos,) + tuple(g.view(s) for g, s in zip(gp, ctx.shapes))


def lstm_tree(pos, lstms):
    """pos [B,24,128] -> cat(pos, pos) + LSTM tree outputs [B,24,256] (fp32); lstms: the five LimbLSTM modules of one stack."""
    lstms = list(lstms)
    if len(lstms) != NUM_LSTMS:
        raise ValueError('lstm_tree: expects %d LSTMs, got %d' % (NUM_LSTMS, len(lstms)))
    params = [p for m in lstms for p in m.flat()]
    return LstmTreeFunction.apply(pos, *params)
