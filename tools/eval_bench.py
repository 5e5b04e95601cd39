"""Timings of the evaluation pipeline at B = 32 (one JSON line each):

  pose      ops.pose_eval (one launch) against metrics.pose_errors (tensor ops, fp64 torch.linalg.svd) on the same inputs
  pve       ops.vertex_eval (one launch: PVE and PA-PVE over all V vertices) beside ops.pose_eval with ground-truth vertices
  seg       ops.seg_confusion (one launch, label upload included) against the per-sample host loop of tests/eval_oracle.py
            including its device -> host copies of the rendered mask / part images
  loop      images/s of evaluate.run_evaluation for 'h36m-p1' and 'lsp' on a synthetic dataset with an InferenceEngine

  python tools/eval_bench.py [--what pose,pve,seg,loop] [--reps 30] [--images 128]

Variants alternate inside one repetition loop (a drift hits both alike); device work is timed with events on the stream, the host
loop with the wall clock around a synchronize; medians with p10 / p90 after 5 warm-up rounds."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _stats(ts):
    ts = np.asarray(ts)
    return {'median_ms': round(float(np.median(ts)), 4), 'p10': round(float(np.percentile(ts, 10)), 4), 'p90': round(float(np.percentile(ts, 90)), 4)}


def _alternate(variants, reps, warmup=5):
    import torch
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            times[k].append(max(e0.elapsed_time(e1), wall) if k.endswith('_host') else e0.elapsed_time(e1))
    return {k: _stats(v) for k, v in times.items()}


def bench_pose(reps, B=32, V=6890):
    import torch
    from danet_densepose2smpl_amd import constants, metrics, ops
    g = torch.Generator().manual_seed(0)
    Jr = torch.rand(17, V, generator=g)
    Jr = (Jr / Jr.sum(1, keepdim=True)).cuda()
    pv, gv = torch.randn(B, V, 3, generator=g).cuda(), torch.randn(B, V, 3, generator=g).cuda()
    gk = torch.randn(B, 14, 3, generator=g).cuda()
    m = constants.H36M_TO_J14
    res = _alternate({'pose_eval_joints': lambda: ops.pose_eval(pv, Jr, m, gt_keypoints_3d=gk),
                      'pose_errors_joints': lambda: metrics.pose_errors(pv, Jr, m, gt_keypoints_3d=gk),
                      'pose_eval_vertices': lambda: ops.pose_eval(pv, Jr, m, gt_vertices=gv),
                      'pose_errors_vertices': lambda: metrics.pose_errors(pv, Jr, m, gt_vertices=gv)}, reps)
    res.update(tool='eval_bench', what='pose', B=B, V=V, reps=reps)
    return res


def bench_pve(reps, B=32, V=6890):
    import torch
    from danet_densepose2smpl_amd import constants, ops
    g = torch.Generator().manual_seed(0)
    Jr = torch.rand(17, V, generator=g)
    Jr = (Jr / Jr.sum(1, keepdim=True)).cuda()
    pv = torch.randn(B, V, 3, generator=g).cuda()
    gv = pv + 0.06 * torch.randn(B, V, 3, generator=g).cuda()
    row = Jr[0].contiguous()
    res = _alternate({'vertex_eval': lambda: ops.vertex_eval(pv, gv, row),
                      'pose_eval_vertices': lambda: ops.pose_eval(pv, Jr, constants.H36M_TO_J14, gt_vertices=gv)}, reps)
    res.update(tool='eval_bench', what='pve', B=B, V=V, reps=reps)
    return res


def bench_seg(reps, B=32):
    import torch
    import eval_oracle as eo
    from danet_densepose2smpl_amd import evaluate, ops
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:224, 0:224]
    parts = np.stack([np.where((xx - 112) ** 2 + (yy - 112) ** 2 < (60 + b) ** 2, 1 + (xx // 16 + yy // 16 + b) % 6, 0) for b in range(B)]).astype(np.int64)
    mask = (parts > 0).astype(np.float32)
    shapes = [(int(rng.integers(200, 480)), int(rng.integers(200, 480))) for _ in range(B)]
    gp = [rng.integers(0, 7, s).astype(np.uint8) for s in shapes]
    for p in gp:
        p[rng.random(p.shape) < 0.02] = 255
    gm = [((p > 0) & (p != 255)).astype(np.uint8) * 255 for p in gp]
    center = np.array([[s[1] / 2, s[0] / 2] for s in shapes]) + rng.uniform(-30, 30, (B, 2))
    scale = np.array([max(s) / 200. for s in shapes]) * rng.uniform(0.6, 1.2, B)
    dm, dp = torch.from_numpy(mask).cuda(), torch.from_numpy(parts).cuda()
    counters = torch.zeros(32, dtype=torch.int64, device='cuda')

    def hip():
        pk = evaluate.pack_labels(gm, gp, center, scale, 224, 'cuda')
        ops.seg_confusion(dm, dp, pk['gt_mask'], pk['gt_parts'], pk['offsets'], pk['shapes'], pk['rects'], pk['tables'], pk['max_pixels'], counters)
    pk = evaluate.pack_labels(gm, gp, center, scale, 224, 'cuda')

    def hip_kernel():
        ops.seg_confusion(dm, dp, pk['gt_mask'], pk['gt_parts'], pk['offsets'], pk['shapes'], pk['rects'], pk['tables'], pk['max_pixels'], counters)

    def host():
        eo.score_batch(dm.cpu().numpy(), dp.cpu().numpy(), gm, gp, center, scale, evaluate.uncrop_geometry)
    counters.zero_()
    hip_kernel()
    assert (counters.cpu().numpy() == eo.score_batch(mask, parts, gm, gp, center, scale, evaluate.uncrop_geometry)).all()
    res = _alternate({'seg_confusion_with_upload_host': hip, 'seg_confusion_kernel': hip_kernel, 'oracle_loop_host': host}, reps)
    res.update(tool='eval_bench', what='seg', B=B, label_pixels=int(sum(s[0] * s[1] for s in shapes)), reps=reps)
    return res


def bench_loop(images, B=32):
    import torch
    from danet_densepose2smpl_amd import evaluate
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    torch.manual_seed(0)
    model = DaNet(default_options(B), None, pretrained=False).cuda().eval()
    eng = model.inference_engine(B)
    out = {'tool': 'eval_bench', 'what': 'loop', 'B': B, 'images': images}
    with tempfile.TemporaryDirectory() as root:
        for name in ('h36m-p1', 'lsp'):
            d = os.path.join(root, name)
            ds = evaluate.EvalDataset(evaluate.write_synthetic_dataset(d, name, n=images, seed=0), d, name)
            ts = []
            for rep in range(4):                                  # the first pass captures the graph and fills the table cache
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                evaluate.run_evaluation(eng, name, ds, None, batch_size=B, num_workers=8, log_freq=0)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            out[name] = {'images_per_s': round(images / float(np.median(ts[1:])), 1), 'passes_s': [round(t, 3) for t in ts]}
    eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='pose,pve,seg,loop')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--images', type=int, default=128)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/eval_bench.py needs a GPU')
    for w in a.what.split(','):
        res = {'pose': lambda: bench_pose(a.reps), 'pve': lambda: bench_pve(a.reps), 'seg': lambda: bench_seg(a.reps), 'loop': lambda: bench_loop(a.images)}[w]()
        print(json.dumps(res), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
