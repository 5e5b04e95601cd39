"""Times tracks.affinity (csrc/track_link.hip, one launch, one wave per pair) against the same four numbers per pair composed from
torch broadcasts in float64: the two atlases of every pair gathered to [C, texels, 4], the masks, the weighted sums and the shape
term, in chunks of 1 024 pairs.  K = 32 and 128 tracks of 20 frames with first frames uniform in [0, 600), T = 8 and 16, every
time-admissible pair at max_absence = 150.  HIP events around one whole call, 20 repetitions after 3 warm-ups, the two ways
alternating; median and p10 / p90 in ms and the largest relative difference between the two ways, one JSON line per (K, T), appended
to --out (default profiles/track_link_bench.jsonl).  There is no threshold on these numbers: there is nothing before the op to
compare with.

  python tools/link_bench.py [--out FILE] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W_MIN = 1e-3
CHUNK = 1024


def make_case(K, T, seed, device):
    """-> (shape [K,10], atlas [K,24,T,T,4] on the device, TrackSet): a third of the texels of every track unseen."""
    import torch
    from danet_densepose2smpl_amd import tracks
    rng = np.random.default_rng(seed)
    L = 20
    first = np.sort(rng.integers(0, 600, K))
    ts = tracks.TrackSet(np.arange(K + 1) * L, (first[:, None] + np.arange(L)[None]).reshape(-1), np.zeros(K * L, np.int32),
                         np.ones(K * L, np.float32), int(first.max()) + L)
    w = np.where(rng.uniform(size=(K, 24, T, T)) < 1 / 3, 0.0, rng.uniform(0.01, 3.0, (K, 24, T, T)))
    atlas = np.concatenate([rng.uniform(0, 1, (K, 24, T, T, 3)), w[..., None]], -1).astype(np.float32)
    shape = rng.normal(0, 1, (K, 10)).astype(np.float32)
    return torch.from_numpy(shape).to(device), torch.from_numpy(atlas).to(device), ts


def composed(shape, atlas, pairs):
    """The pair distance of DESIGN.md 4b'-link from torch broadcasts, float64 inside, fp32 out: no host read."""
    import torch
    K = atlas.shape[0]
    flat = atlas.view(K, -1, 4)
    out = []
    for i in range(0, pairs.shape[0], CHUNK):
        a, b = pairs[i:i + CHUNK, 0].long(), pairs[i:i + CHUNK, 1].long()
        ta, tb = flat[a].double(), flat[b].double()
        ia, ib = ta[..., 3] > W_MIN, tb[..., 3] > W_MIN
        both = ia & ib
        m = torch.where(both, ta[..., 3].clamp(max=1.0) * tb[..., 3].clamp(max=1.0), torch.zeros_like(ta[..., 3]))
        d = torch.where(both.unsqueeze(-1), ta[..., :3] - tb[..., :3], torch.zeros_like(ta[..., :3]))
        S, n, u = m.sum(1), both.sum(1).double(), (ia | ib).sum(1).double()
        d_app = torch.where(n > 0, (m * (d * d).sum(-1)).sum(1) / (3.0 * S.clamp(min=1e-300)), torch.zeros_like(S))
        overlap = torch.where(u > 0, n / u.clamp(min=1.0), torch.zeros_like(u))
        ds = shape[a].double() - shape[b].double()
        out.append(torch.stack([(ds * ds).sum(1) / 10.0, d_app, overlap, S], 1).float())
    return torch.cat(out, 0)


def main(argv=None):
    profiles = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles')
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(profiles, 'track_link_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args(argv)
    import torch
    from danet_densepose2smpl_amd import tracks
    if not torch.cuda.is_available():
        raise SystemExit('tools/link_bench.py needs a GPU')
    dev = torch.device('cuda', 0)
    for K in (32, 128):
        for T in (8, 16):
            shape, atlas, ts = make_case(K, T, 1000 * K + T, dev)
            ps = tracks.PairSet(tracks.candidates(ts, 150), K)
            d_pairs = ps.device(dev)
            ways = {'composed': lambda: composed(shape, atlas, d_pairs), 'op': lambda: tracks.affinity(shape, atlas, ps)}
            x, y = ways['op']().double(), ways['composed']().double()
            rel = float(((x - y).abs() / y.abs().clamp(min=1e-30)).max())
            for _ in range(a.warmup):
                for f in ways.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in ways}
            for _ in range(a.reps):
                for k, f in ways.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1))
            res = {'tool': 'link_bench', 'K': K, 'T': T, 'texels': 24 * T * T, 'pairs': ps.C, 'reps': a.reps, 'warmup': a.warmup,
                   'max_rel_diff': rel, 'atlas_mb_read': round(2 * ps.C * 24 * T * T * 16 / 1e6, 2)}
            for k, v in times.items():
                res[k] = {'median_ms': round(float(np.median(v)), 4), 'p10': round(float(np.percentile(v, 10)), 4), 'p90': round(float(np.percentile(v, 90)), 4)}
            line = json.dumps(res)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
