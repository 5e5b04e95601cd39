"""Inference throughput of DaNet: model.infer_net against the BatchNorm-folded engine (inference.py) run eagerly and replayed from its
graph, alternately in one process, warmed up, on seeded inputs.  One JSON line per configuration: ms per batch and img/s (median and
the spread p10..p90 over the timed repetitions of each variant) and the max |para| difference between infer_net and the replay.

  python tools/infer_bench.py [--config c2|hrnet|all] [--reps 20] [--warmup 3]
  C2:    ResNet-50 backbone, B = 16, 256^2 (BASELINE config C2)
  hrnet: HRNet-W48 backbone, B = 32, 256^2
Kernel statistics: run it once more under `rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py ...` (its own step)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {'c2': ('resnet', 16), 'hrnet': ('hrnet', 32)}


def _stats(ts, B):
    ts = np.asarray(ts)
    med = float(np.median(ts))
    return {'ms': round(med, 3), 'ms_p10': round(float(np.percentile(ts, 10)), 3), 'ms_p90': round(float(np.percentile(ts, 90)), 3),
            'img_s': round(B * 1000.0 / med, 1)}


def run(name, reps, warmup):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    regressor, B = CONFIGS[name]
    reset_cfg()
    cfg_from_dict({'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.IUV_REGRESSOR': regressor})
    torch.manual_seed(0)
    model = DaNet(default_options(B), None, pretrained=False).cuda().eval()
    img = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    eng = model.inference_engine(B)
    variants = {'infer_net': lambda: model.infer_net(img), 'engine_eager': lambda: eng.eager(img), 'engine_graph': lambda: eng(img)}
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():                  # alternately: drifts of clock / temperature hit all three alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    ref = model.infer_net(img)['para']
    diff = float((eng(img)['para'] - ref).abs().max())
    out = {'config': name, 'backbone': regressor, 'B': B, 'size': 256, 'reps': reps}
    out.update({k: _stats(v, B) for k, v in times.items()})
    out['speedup_graph_vs_infer_net'] = round(out['infer_net']['ms'] / out['engine_graph']['ms'], 3)
    out['para_max_abs_diff'] = diff
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='all', choices=['all'] + sorted(CONFIGS))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    for name in (sorted(CONFIGS) if a.config == 'all' else [a.config]):
        print(json.dumps(run(name, a.reps, a.warmup)), flush=True)


if __name__ == '__main__':
    main()
