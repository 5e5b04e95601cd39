"""Times tracks.smooth_para (csrc/track_ops.hip, three launches) against the same solve composed in torch: per track and lam group a
dense float64 torch.linalg.solve of the pentadiagonal system, the s clamp, the shared shape, and the 6D map by
geometry.rot6d_to_rotmat.  K = 8 tracks of T = 64 and 256 rows, a tenth of the interior rows gap rows.  HIP events around one whole
call, 20 repetitions after 3 warm-ups, the two ways alternating; median and p10 / p90 in ms, one JSON line per T, appended to --out
(default profiles/track_smooth_bench.jsonl).  There is no threshold on these numbers: the op is a dependent chain of T steps, latency-
bound by construction, and nothing before it to compare with.

  python tools/track_bench.py [--out FILE] [--reps 20] [--warmup 3]

With --stream: one para-form step of tracks.StreamSmoother (csrc/track_stream.hip, one launch: every slot takes a row and emits the row
`lag` behind) at S in {8, 32} slots and lag in {8, 32}, against the two ways to a streaming estimate without it: tracks.smooth_para
re-run on every slot's whole prefix of T = 256 rows (exact), and re-run on a window of the last lag + 16 rows (not exact).  The same
protocol; the step's commands are uploaded outside the events, as a captured pipeline would have them.  Appended to
profiles/track_stream_bench.jsonl.

  python tools/track_bench.py --stream [--out FILE] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = 1e-6


def make_rows(K, T, seed, device):
    """-> (para [K T,229] f32 on the device, TrackSet): random walks in the 157 unknowns, matrices by the 6D map."""
    import torch
    from danet_densepose2smpl_amd import geometry, tracks
    g = torch.Generator().manual_seed(seed)
    N = K * T
    eye6 = torch.tensor([1., 0., 0., 1., 0., 0.])
    x6 = eye6 + torch.cumsum(torch.randn(K, T, 24, 6, generator=g) * 0.02, 1) + torch.randn(K, T, 24, 6, generator=g) * 0.05
    cam = torch.tensor([0.9, 0., 0.]) + torch.randn(K, T, 3, generator=g) * 0.02
    betas = torch.randn(K, 1, 10, generator=g) + torch.randn(K, T, 10, generator=g) * 0.3
    R = geometry.rot6d_to_rotmat(x6.reshape(-1, 6).to(device)).view(N, 216)
    para = torch.cat([cam.reshape(N, 3).to(device), betas.reshape(N, 10).to(device), R], 1).contiguous()
    rng = np.random.default_rng(seed)
    conf = np.ones((K, T), np.float32)
    conf[:, 1:-1][rng.uniform(size=(K, T - 2)) < 0.1] = 0.0
    ts = tracks.TrackSet(np.arange(K + 1) * T, np.tile(np.arange(T), K), np.where(conf.reshape(-1) > 0, 0, -1), conf.reshape(-1), T)
    return para, ts


def stencils(T, device):
    import torch
    Dv = torch.zeros(T - 1, T, dtype=torch.float64, device=device)
    r = torch.arange(T - 1, device=device)
    Dv[r, r], Dv[r, r + 1] = -1.0, 1.0
    Da = torch.zeros(T - 2, T, dtype=torch.float64, device=device)
    r = torch.arange(T - 2, device=device)
    Da[r, r], Da[r, r + 1], Da[r, r + 2] = 1.0, -2.0, 1.0
    return Dv.T @ Dv, Da.T @ Da


def composed(para, conf, K, T, lam, VV, AA):
    """The track rule of DESIGN.md 4b'-track in torch, all tracks batched (they have one length here): no host read."""
    import torch
    from danet_densepose2smpl_amd import geometry
    N = K * T
    R = para[:, 13:].view(N, 24, 3, 3)
    ch = torch.cat([para[:, :13], R[:, :, :, :2].reshape(N, 144)], 1).double().view(K, T, 157)
    c = conf.double().view(K, T)
    obs = (c > 0).unsqueeze(-1)
    mean = (torch.where(obs, ch, torch.zeros_like(ch)) * c.unsqueeze(-1)).sum(1, keepdim=True) / c.sum(1).view(K, 1, 1)
    y = torch.where(obs, ch, mean)
    w = c + EPS
    out = torch.empty_like(ch)
    for g, sl in enumerate((slice(0, 3), slice(3, 13), slice(13, 157))):
        A = torch.diag_embed(w) + lam[g][0] * VV + lam[g][1] * AA
        out[:, :, sl] = torch.linalg.solve(A, w.unsqueeze(-1) * y[:, :, sl])
    big = torch.full_like(ch[:, :, 0], float('inf'))
    lo = torch.where(obs[:, :, 0], ch[:, :, 0], big).amin(1, keepdim=True)
    hi = torch.where(obs[:, :, 0], ch[:, :, 0], -big).amax(1, keepdim=True)
    out[:, :, 0] = torch.minimum(torch.maximum(out[:, :, 0], lo), hi)
    out[:, :, 3:13] = mean[:, :, 3:13]
    o32 = out.float().view(N, 157)
    return torch.cat([o32[:, :13], geometry.rot6d_to_rotmat(o32[:, 13:].reshape(-1, 6)).view(N, 216)], 1)


def measure(ways, reps, warmup, before=None):
    """HIP events around one call of each way, the ways alternating; `before(k)` runs outside the events.  -> {way: [ms]}"""
    import torch
    times = {k: [] for k in ways}
    for i in range(warmup + reps):
        for k, f in ways.items():
            if before is not None:
                before(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return times


def stream_bench(a, dev):
    import torch
    from danet_densepose2smpl_amd import tracks
    T = 256
    for S in (8, 32):
        para, ts = make_rows(S, T, T + S, dev)
        rows = para.view(S, T, 229)
        conf = ts.conf.reshape(S, T)
        for lag in (8, 32):
            sm = tracks.StreamSmoother(S, lag, para=True)
            one = np.ones(S, np.int64)
            for t in range(T):                                                 # the prefix goes in, a row per step
                out, _ = sm.step(one, rows[:, t:t + 1].contiguous(), conf[:, t:t + 1], np.full(S, max(t - lag, 0)))
            exact, _ = tracks.smooth_para(para, ts)
            diff = float((out - exact.view(S, T, 229)[:, T - 1 - lag]).abs().max())
            W = lag + 16
            win = rows[:, T - W:].reshape(S * W, 229).contiguous()
            cw = conf[:, T - W:].copy()
            cw[:, 0] = np.maximum(cw[:, 0], 1.0)
            tw = tracks.TrackSet(np.arange(S + 1) * W, np.tile(np.arange(W), S), np.where(cw.reshape(-1) > 0, 0, -1), cw.reshape(-1), W)
            tw.device(dev)
            step_rows = rows[:, T - 1:T].contiguous()
            state = {'t': T}

            def before(k):
                if k == 'op':                                                  # the next row's commands: checked and uploaded outside the events
                    sm.commands(one, conf[:, T - 1:T], np.full(S, state['t'] - lag))
                    state['t'] += 1
            ways = {'op': lambda: sm.launch(step_rows), 'prefix': lambda: tracks.smooth_para(para, ts)[0],
                    'window': lambda: tracks.smooth_para(win, tw)[0]}
            times = measure(ways, a.reps, a.warmup, before)
            res = {'tool': 'track_bench', 'mode': 'stream', 'S': S, 'lag': lag, 'T': T, 'window': W, 'reps': a.reps, 'warmup': a.warmup,
                   'max_abs_diff_to_offline': diff}
            for k, v in times.items():
                res[k] = {'median_ms': round(float(np.median(v)), 4), 'p10': round(float(np.percentile(v, 10)), 4), 'p90': round(float(np.percentile(v, 90)), 4)}
            line = json.dumps(res)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    return 0


def main(argv=None):
    profiles = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles')
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--stream', action='store_true', help='time one step of the stream smoother instead')
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(profiles, 'track_stream_bench.jsonl' if a.stream else 'track_smooth_bench.jsonl')
    import torch
    from danet_densepose2smpl_amd import tracks
    if not torch.cuda.is_available():
        raise SystemExit('tools/track_bench.py needs a GPU')
    dev = torch.device('cuda', 0)
    if a.stream:
        return stream_bench(a, dev)
    K = 8
    for T in (64, 256):
        para, ts = make_rows(K, T, T, dev)
        _, d_conf = ts.device(dev)
        VV, AA = stencils(T, dev)
        lam = tracks.DEFAULT_LAM
        ways = {'composed': lambda: composed(para, d_conf, K, T, lam, VV, AA), 'op': lambda: tracks.smooth_para(para, ts, lam)[0]}
        diff = float((ways['op']() - ways['composed']()).abs().max())
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
        res = {'tool': 'track_bench', 'K': K, 'T': T, 'rows': K * T, 'gap_rows': int((ts.det < 0).sum()), 'reps': a.reps, 'warmup': a.warmup,
               'max_abs_diff': diff}
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
