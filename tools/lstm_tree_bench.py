"""Times the LSTM tree op (csrc/lstm_tree.hip) at one batch size: forward alone and forward + backward, each captured as a graph
and replayed (median of CUDA-event timings).  python tools/lstm_tree_bench.py [B] [reps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(graph, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main(B=32, reps=50):
    import __graft_entry__ as g
    g.build()
    from danet_densepose2smpl_amd.lstm_tree import LimbLSTM, lstm_tree
    torch.manual_seed(0)
    mods = [LimbLSTM().cuda() for _ in range(5)]
    pos = torch.randn(B, 24, 128, device='cuda', requires_grad=True)
    gout = torch.randn(B, 24, 256, device='cuda')
    for _ in range(3):
        lstm_tree(pos, mods).backward(gout)
    torch.cuda.synchronize()
    gf = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gf):
        with torch.no_grad():
            lstm_tree(pos, mods)
    gb = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gb):
        lstm_tree(pos, mods).backward(gout)
    for gr in (gf, gb):
        gr.replay()
    torch.cuda.synchronize()
    f, fb = _time(gf, reps), _time(gb, reps)
    print('lstm_tree B=%d: forward %.1f us (2 launches), forward+backward %.1f us (5 launches), backward ~%.1f us' % (B, f, fb, fb - f))


if __name__ == '__main__':
    main(*[int(a) for a in sys.argv[1:3]])
