"""Times DANET.INPUT_MODE 'iuv_gt': the train step at B = 32, 256^2 images / 64^2 maps (eager, and replay of the captured step), and the
ground-truth crop op (csrc/part_gt.hip) alone in each direction (median of CUDA-event timings) and forward + backward replayed from a graph.
python tools/iuv_gt_bench.py [steps] [reps]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def bench_op(B=32, H=64, reps=50):
    """Each direction's launch timed with events on the current stream (eager, after warm-up), then forward + backward captured
    together in one graph after a side-stream warm-up (as Trainer.capture does) and replayed."""
    from danet_densepose2smpl_amd import _lib, part_ops
    from danet_densepose2smpl_amd._lib import ptr, check, stream
    from danet_densepose2smpl_amd.iuv_estimator import DP2SMPL_MAPPING
    g = torch.Generator().manual_seed(0)
    part = torch.randint(0, 25, (B, H // 4, H // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    img = torch.cat([(part.float() / 24).unsqueeze(1), torch.rand(B, 2, H, H, generator=g)], 1).cuda().contiguous()
    th = torch.zeros(B, 24, 2, 3)
    th[..., 0, 0] = th[..., 1, 1] = 0.2 + 0.6 * torch.rand(B, 24, generator=g)
    th[..., :, 2] = torch.rand(B, 24, 2, generator=g) - 0.5
    th = th.cuda().contiguous()
    sel = torch.tensor(DP2SMPL_MAPPING, dtype=torch.int32).cuda()
    keep = torch.ones(B, 24, 7).cuda()
    keep25 = torch.ones(B, 25).cuda()
    x24 = torch.empty(B * 24, H, H, 24, dtype=torch.bfloat16, device='cuda')
    body = torch.empty(B, H, H, 80, dtype=torch.bfloat16, device='cuda')
    g24 = torch.randn(B * 24, H, H, 24, generator=g).to(torch.bfloat16).cuda()
    dth = torch.empty(B, 24, 2, 3, device='cuda')
    L = _lib.lib()

    def fwd(with_body=True):
        check(L.danet_part_gt_forward(ptr(img), ptr(th), ptr(sel), ptr(keep), ptr(keep25), B, H, H, 1, ptr(x24),
                                      ptr(body) if with_body else None, stream()), 'danet_part_gt_forward')

    def bwd():
        check(L.danet_part_gt_backward(ptr(img), ptr(th), ptr(sel), ptr(keep), ptr(g24), B, H, H, 1, ptr(dth), stream()),
              'danet_part_gt_backward')

    for fn in (fwd, bwd):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    f, f_nobody, b = _time(fwd, reps), _time(lambda: fwd(False), reps), _time(bwd, reps)
    mb = B * 24 * H * H * 48 / 1e6
    print('part_gt B=%d %dx%d eager: forward %.1f us (x24 %.0f MB + body %.0f MB written; x24 alone %.1f us), backward %.1f us (g24 %.0f MB read)'
          % (B, H, H, f, mb, B * H * H * 160 / 1e6, f_nobody, b, mb), flush=True)
    # forward + backward of the autograd op, captured together
    tg = th.clone().requires_grad_(True)
    gin = g24.permute(0, 3, 1, 2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xx, _ = part_ops.part_gt(img, tg, sel, keep, keep25, True, body=True)
            xx.backward(gin)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xx, _ = part_ops.part_gt(img, tg, sel, keep, keep25, True, body=True)
        xx.backward(gin)
    graph.replay()
    torch.cuda.synchronize()
    fb = _time(graph.replay, reps)
    print('part_gt B=%d %dx%d graph replay: forward + backward (with the gradient accumulation into theta.grad) %.1f us' % (B, H, H, fb),
          flush=True)
    del graph
    return f, b, fb


def bench_step(B=32, steps=20):
    from danet_densepose2smpl_amd.config import cfg_from_dict
    cfg_from_dict({'DANET.INPUT_MODE': 'iuv_gt', 'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64})
    from danet_densepose2smpl_amd.trainer import Trainer, synthetic_in_dict, default_options
    dev = torch.device('cuda')
    torch.manual_seed(0)
    tr = Trainer(default_options(B), device=dev, distributed=False)
    batch = synthetic_in_dict(tr.model, B, dev, seed=1)
    for _ in range(3):
        tr.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(batch)
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / steps * 1e3
    tr.capture(batch, warmup=2)
    for _ in range(3):
        tr.train_step_graphed()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step_graphed()
    torch.cuda.synchronize()
    graph = (time.perf_counter() - t0) / steps * 1e3
    print("iuv_gt train step B=%d 256^2 / 64^2: eager %.2f ms, graph replay %.2f ms" % (B, eager, graph), flush=True)
    return eager, graph


def main(steps=20, reps=50):
    import __graft_entry__ as g
    g.build()
    bench_op(reps=reps)
    bench_step(steps=steps)


if __name__ == '__main__':
    main(*[int(a) for a in sys.argv[1:3]])
