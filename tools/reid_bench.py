"""The online descriptor of the causal identity rule (DESIGN.md 4b'-reid) against the exact alternative the project had before it:

  step      tracks.StreamDescriptor.step for S tracks, one new observed row each: one launch on the running sums, whatever the tracks'
            length (`step` is the whole call on a given depth plane: the checks, two small uploads and the launch;
            `step_with_depth` adds the rasteriser's three launches for the S new rows, which is what a frame costs in
            video.StreamDemo; `step_replay` is the launch alone, captured once under torch.cuda.graph and replayed)
  unwrap    texture.TextureAtlas.unwrap over every track's whole observed prefix of L rows (the rasteriser over S L views, then one
            launch that loops over them): what the same descriptor costs without the running sums, at L = 16 and 256

  python tools/reid_bench.py [--slots 8,32] [--sizes 8,16] [--prefix 16,256] [--reps 20] [--warmup 3] [--out FILE.jsonl]

The synthetic SMPL body and DensePose topology, crops of 224 x 224, noise images (the time does not depend on the colours).  Times
are HIP events around one call, the ways alternating inside every repetition; reported are the median and p10 / p90 in milliseconds.
The two ways give the same bits (tests/test_gpu_reid.py); nothing is compared here and there is no threshold.  One JSON line per (S, T),
appended to --out as well."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 224


def _timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(v, digits=4):
    v = np.asarray(v)
    return {'median': round(float(np.median(v)), digits), 'p10': round(float(np.percentile(v, 10)), digits),
            'p90': round(float(np.percentile(v, 90)), digits), 'unit': 'ms'}


def bodies(smpl, S, seed=5):
    """S rows (cam, betas, rotations) and their meshes: people in the middle of their crops, turned about the vertical."""
    import torch
    from danet_densepose2smpl_amd import ops
    from danet_densepose2smpl_amd.smpl import from_para
    g = torch.Generator().manual_seed(seed)
    aa = 0.2 * torch.randn(S, 24, 3, generator=g)
    aa[:, 0] = torch.stack([torch.zeros(S), 6.28 * torch.rand(S, generator=g), torch.zeros(S)], 1)
    R = ops.rodrigues_smplx(aa.view(-1, 3).cuda()).view(S, 216)
    cam = torch.tensor([[0.9, 0.0, 0.0]]).repeat(S, 1)
    para = torch.cat([cam.cuda(), torch.randn(S, 10, generator=g).clamp(-3, 3).cuda(), R], 1).contiguous()
    return para, from_para(smpl, para).vertices.detach().contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description='online descriptor: one step on the running sums against the unwrap of the whole prefix')
    ap.add_argument('--slots', default='8,32')
    ap.add_argument('--sizes', default='8,16')
    ap.add_argument('--prefix', default='16,256')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/reid_bench.py needs a GPU (there is no CPU path)')
    from danet_densepose2smpl_amd import tracks
    from danet_densepose2smpl_amd.smpl import SMPL
    from danet_densepose2smpl_amd.texture import TextureAtlas
    smpl = SMPL().cuda()
    prefixes = [int(v) for v in a.prefix.split(',')]
    for S in [int(v) for v in a.slots.split(',')]:
        para, verts = bodies(smpl, S)
        cam = para[:, 0:3].contiguous()
        images = torch.rand(S, 3, H, H, device='cuda')
        conf = torch.ones(S, device='cuda')
        slot, observed = np.arange(S, dtype=np.int32), np.ones(S, np.int32)
        for T in [int(v) for v in a.sizes.split(',')]:
            tex = TextureAtlas(size=T)
            sd = tracks.StreamDescriptor(S, 1, tex)
            depth = sd.depth_planes(verts, cam, H)
            ways = {'step': lambda: sd.step(images, verts, cam, depth, para, conf, slot, observed),
                    'step_with_depth': lambda: sd.step(images, verts, cam, sd.depth_planes(verts, cam, H), para, conf, slot, observed)}
            graph = torch.cuda.CUDAGraph()                                    # (the two steps above have warmed the launch up)
            for f in list(ways.values()):
                f()
            torch.cuda.synchronize()
            sd.commands(slot, observed)
            with torch.cuda.graph(graph):
                sd.launch(images, verts, cam, depth, para, conf)
            ways['step_replay'] = graph.replay
            for L in prefixes:                                               # track-major views: track k owns views k L .. (k + 1) L - 1
                idx = torch.arange(S, device='cuda').repeat_interleave(L)
                vi, vv, vc = torch.rand(S * L, 3, H, H, device='cuda'), verts[idx].contiguous(), cam[idx].contiguous()
                off = np.arange(S + 1, dtype=np.int32) * L
                ways['unwrap_%d' % L] = (lambda vi=vi, vv=vv, vc=vc, off=off: tex.unwrap(vi, vv, vc, view_offsets=off))
            for _ in range(a.warmup):
                for f in ways.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in ways}
            for _ in range(a.reps):
                for k, f in ways.items():
                    times[k].append(_timed(f))
            sd.read(slot, 1 + slot)
            line = {'tool': 'reid_bench', 'S': S, 'T': T, 'texels': 24 * T * T, 'H': H, 'reps': a.reps, 'warmup': a.warmup,
                    'state_bytes': int(sd.state_bytes), 'observed_texels': float((sd.desc_atlas[1:, ..., 3] > 0).float().mean())}
            line.update({k: _stats(v) for k, v in times.items()})
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                with open(a.out, 'a') as fh:
                    fh.write(text + '\n')
            del ways, times, graph
            torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
