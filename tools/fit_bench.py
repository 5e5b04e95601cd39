"""Steady-state step time of Trainer.fit, eager and with options.graph, and the DensePose point-loss branch alone (HIP op against
the tensor-op form).

  python tools/fit_bench.py [--steps N] [--batch_size B] [--samples K] [--modes dp,eager,graph,vis] [--vis_interval K] [--run_smplify]
                            [--out FILE]

A synthetic 'h36m_dp' set (K + K samples, written to a scratch directory from a seed) is trained on at 256 x 256 with batch B, one
process.  Each fit runs N steps after its warm-up (graphed: two eager steps and the capture; eager: three steps); the step time is the
difference of host timestamps taken in on_step after a device synchronise, so it holds the loader, build_in_dict and the step.
build_in_dict alone is timed the same way.  The DensePose branch (forward + backward at B x 64 x 64) is timed with device events:
median of 50 after 10 warm-up rounds.  --vis_interval K is passed on to the fits (a graphed fit then runs every step with the frozen
vis_on = True); their step times are then reported separately for the steps that end in a visualisation.  Mode 'vis' times
Trainer.visualize alone on one eager step's output: sheets built (device events), the copy to the host, the PNG encoding.
--run_smplify switches the refresh stage of the fits on (options.run_smplify: the in-loop keypoint fit after every step).  Last line: one JSON object.  Nothing outside the repository is read."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ms):
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'n': len(ms)}


def fit_times(torch, train_ds, paths, a, graph, root):
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    from danet_densepose2smpl_amd.trainer import Trainer
    warm = 3
    per_epoch = max(1, len(train_ds) // a.batch_size)
    tag = 'graph' if graph else 'eager'
    o = types.SimpleNamespace(batch_size=a.batch_size, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp',
                              num_epochs=-(-(a.steps + warm) // per_epoch), pretr_step=0, checkpoint_steps=10 ** 9, summary_steps=10 ** 9, num_workers=8,
                              seed=3, shuffle_train=True, time_to_run=None, resume=None, pretrained_checkpoint=None, graph=graph,
                              vis_interval=a.vis_interval, run_smplify=a.run_smplify,
                              log_dir=os.path.join(root, 'log_' + tag), checkpoint_dir=os.path.join(root, 'ck_' + tag))
    torch.manual_seed(0)
    tr = Trainer(o)
    fits = FitsDict(o, train_ds, paths['final_fits_dir'], paths['static_fits_dir'], tr.device)
    stamps = []

    def on_step(step, in_dict, losses):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    tr.fit(train_ds, fits, o, on_step=on_step)
    from danet_densepose2smpl_amd.train_vis import vis_due
    steps = list(zip(range(warm + 1, len(stamps) + 1), stamps[warm - 1:-1], stamps[warm:]))      # the steps after the warm-up (and the capture)
    ms = [(b - t) * 1e3 for n, t, b in steps if not vis_due(n, a.vis_interval)]
    out = dict(_stats(ms), **getattr(tr, 'fit_stats', {}))
    if a.vis_interval:
        out['vis_steps'] = _stats([(b - t) * 1e3 for n, t, b in steps if vis_due(n, a.vis_interval)])
    if graph:
        # build_in_dict alone, on batches of the same loader: what a replayed step cannot shed
        loader = datasets.TrainLoader(train_ds, checkpoint=None, batch_size=a.batch_size, shuffle=True, num_workers=8, seed=3, epoch=0, res=256)
        t = []
        for host in loader:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.build_in_dict(host, fits, 'h36m_dp')
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        out['build_in_dict'] = _stats(t[1:] or t)
        tr.drop_graph()
    return out


def vis_times(torch, train_ds, paths, a, root, rounds=10):
    """Trainer.visualize on the output of one eager step with vis_on: device time of the sheets, host time of sheets + copy, PNG encoding."""
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    from danet_densepose2smpl_amd.trainer import Trainer
    o = types.SimpleNamespace(batch_size=a.batch_size, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp')
    torch.manual_seed(0)
    tr = Trainer(o)
    fits = FitsDict(o, train_ds, paths['final_fits_dir'], paths['static_fits_dir'], tr.device)
    loader = datasets.TrainLoader(train_ds, checkpoint=None, batch_size=a.batch_size, shuffle=True, num_workers=8, seed=3, epoch=0, res=256)
    in_dict = tr.build_in_dict(next(iter(loader)), fits, 'h36m_dp', vis_on=True)
    output, losses = tr.train_step(in_dict)
    dev, copy, png = [], [], []
    for r in range(rounds + 2):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        sheets = tr.visualize(in_dict, output, losses)
        e1.record()
        tags = [t for t in sheets if t not in tr.VIS_SCALARS]
        host = torch.cat([sheets[t].reshape(-1) for t in tags]).cpu()
        t1 = time.perf_counter()
        for t in tags:
            tr.write_sheets(os.path.join(root, 'vis_bench'), {t: sheets[t]})
        t2 = time.perf_counter()
        if r >= 2:
            dev.append(e0.elapsed_time(e1))
            copy.append((t1 - t0) * 1e3)
            png.append((t2 - t1) * 1e3)
    return {'sheets_device': _stats(dev), 'sheets_and_copy_host': _stats(copy), 'png_encode_and_write': _stats(png),
            'sheet_bytes': int(host.numel()), 'tags': tags}


def dp_branch_times(torch, B, S=64, rounds=50, warmup=10):
    from danet_densepose2smpl_amd import iuv_ops
    from danet_densepose2smpl_amd.iuv_estimator import IUV_Estimator
    g = torch.Generator().manual_seed(1)
    dev = 'cuda'
    bases = [torch.zeros(B, S, S, ld, device=dev) for ld in (32, 32, 32, 16)]
    for t, n in zip(bases, (25, 25, 25, 15)):
        t[..., :n] = torch.randn(B, S, S, n, generator=g).to(dev)
    bases = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in bases]
    I = torch.randint(0, 25, (B, 196), generator=g)
    I[:, 150:] = 0
    wts = torch.nn.functional.one_hot(I, 25).permute(0, 2, 1).float() * (I > 0).float().unsqueeze(1)
    dp = {'body_uv_X_points': torch.rand(B, 196, generator=g) * (S - 1), 'body_uv_Y_points': torch.rand(B, 196, generator=g) * (S - 1),
          'body_uv_I_points': I.float(), 'body_uv_U_points': (torch.rand(B, 25, 196, generator=g) * wts).reshape(B, 4900),
          'body_uv_V_points': (torch.rand(B, 25, 196, generator=g) * wts).reshape(B, 4900), 'body_uv_point_weights': wts.reshape(B, 4900),
          'body_uv_ann_labels': torch.randint(0, 15, (B, S * S), generator=g).to(torch.int32)}
    dp = {k: v.to(dev) for k, v in dp.items()}
    has_dp = (torch.arange(B) % 2 == 0).float().to(dev)

    def hip():
        return iuv_ops.dp_point_losses(*bases, dp, has_dp, True)

    def tensor_ops():
        return IUV_Estimator.dp_uvia_losses(bases[0][:, :25], bases[1][:, :25], bases[2][:, :25], bases[3][:, :15], dp, has_dp, True)
    out = {}
    for name, fn in (('hip_op', hip), ('tensor_ops', tensor_ops), ('hip_op_again', hip), ('tensor_ops_again', tensor_ops)):      # alternating: the spread
        ms = []
        for r in range(warmup + rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.autograd.grad(sum(l.sum() for l in fn()), bases)
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms.append(e0.elapsed_time(e1))
        out[name] = _stats(ms)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description='Trainer.fit step time, eager and graphed')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--samples', type=int, default=64, help='synthetic samples per dataset')
    ap.add_argument('--out', default=None)
    ap.add_argument('--modes', default='dp,eager,graph', help="what to time: 'dp' (the DensePose branch alone), 'eager' / 'graph' (fit), 'vis' (Trainer.visualize)")
    ap.add_argument('--vis_interval', type=int, default=0, help='options.vis_interval of the fits (0: no visualisation)')
    ap.add_argument('--run_smplify', action='store_true', help='options.run_smplify of the fits: the in-loop keypoint fit after every step')
    a = ap.parse_args(argv)
    import torch
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.config import cfg_from_dict, reset_cfg
    if not torch.cuda.is_available():
        raise SystemExit('tools/fit_bench.py needs a GPU (there is no CPU path)')
    reset_cfg()
    cfg_from_dict({'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64})
    modes = a.modes.split(',')
    res = {'batch_size': a.batch_size, 'steps': a.steps, 'vis_interval': a.vis_interval, 'run_smplify': a.run_smplify}
    if 'dp' in modes:
        res['dp_branch'] = dp_branch_times(torch, a.batch_size)
    if 'eager' in modes or 'graph' in modes or 'vis' in modes:
        with tempfile.TemporaryDirectory() as root:
            o = types.SimpleNamespace(batch_size=a.batch_size, train_data='h36m_dp', heatmap_size=64, img_res=256)
            train_ds, paths = datasets.synthetic_mixed_dataset(o, os.path.join(root, 'data'), a.samples, a.samples, seed=5)
            for mode in modes:
                if mode in ('eager', 'graph'):
                    res['fit_' + mode] = fit_times(torch, train_ds, paths, a, mode == 'graph', root)
                if mode == 'vis':
                    res['visualize'] = vis_times(torch, train_ds, paths, a, root)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
