"""The dense fit rule (DESIGN.md "the dense fit rule") run two ways on rendered synthetic bodies at P = 1, 8 and 32 people, dense term
only, default stages (100 iterations, 101 energy evaluations), S = 56, G = 4:

  replay    composed from the existing ops -- ops.rot6d_to_rotmat, the SMPL layer (full LBS, autograd), the landmark points gathered
            from its vertices, projection, energy and Adam in torch -- with ONE iteration captured under torch.cuda.graph and
            replayed 100 times (tools/kpfit_bench.py's composition with the dense term added; the gate is the op's)
  op        dense_fit.DenseFitter.fit on the observations: one launch

  python tools/densefit_bench.py [--people 1,8,32] [--reps 20] [--warmup 3] [--out FILE.jsonl]

Times are HIP events around a whole fit, the two ways alternating inside every repetition; reported are the median and p10 / p90 in
milliseconds, the per-iteration time (median / 100) in microseconds, the support size and the landmark count, the largest
difference of the final energies between the ways, and the observation kernel alone (DenseFitter.landmarks on the [P,3,56,56]
images, microseconds).  There is no threshold.  One JSON line per P, appended to --out as well."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

S_IMG = 56


def rendered_inputs(smpl, P, seed=7):
    """P rows (cam, betas, rotations), the IUV images of their bodies under the rule's camera, and a perturbed start (pose noise of
    0.08 rad, camera shift 0.03, scale 1.05: the dense recovery case's)."""
    import torch
    from danet_densepose2smpl_amd import assets, constants, ops
    from danet_densepose2smpl_amd.smpl import from_para
    g = torch.Generator().manual_seed(seed)
    betas = torch.randn(P, 10, generator=g).clamp(-3, 3)
    R = ops.rodrigues_smplx((0.2 * torch.randn(P * 24, 3, generator=g)).cuda()).view(P, 216)
    cam = torch.stack([0.6 + 0.5 * torch.rand(P, generator=g), 0.2 * torch.rand(P, generator=g) - 0.1, 0.2 * torch.rand(P, generator=g) - 0.1], 1)
    star = torch.cat([cam.cuda(), betas.cuda(), R], 1).contiguous()
    vm, faces, tex = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in assets.densepose_render_tables(assets.make_synthetic_densepose(None, 0)))
    iuv = ops.iuv_raster(from_para(smpl, star).vertices.detach(), star[:, :3].contiguous(), vm, faces, tex, constants.FOCAL_LENGTH,
                         constants.IMG_RES, S_IMG)
    noise = ops.rodrigues_smplx((0.08 * torch.randn(P * 24, 3, generator=g)).cuda()).view(P, 24, 3, 3)
    init = star.clone()
    init[:, 13:] = (star[:, 13:].view(P, 24, 3, 3) @ noise).reshape(P, 216)
    init[:, 0] *= 1.05
    init[:, 1:3] += 0.03
    return init.contiguous(), iuv


def composed(fitter, para, obs, gate):
    """kpfit_bench.Composed with the dense term: the landmark points from the SMPL layer's vertices, the gate held."""
    import torch
    from kpfit_bench import Composed
    h = fitter.host_tables()
    vert = torch.from_numpy(h['lm_vert']).cuda()
    w = torch.from_numpy(h['lm_w'].astype(np.float32)).cuda()
    wl = fitter.w_dense * (gate.float() * obs[..., 2]) ** 2
    P = para.shape[0]

    class Dense(Composed):
        def energy(self, x):
            f = self.f
            R = self.ops.rot6d_to_rotmat(x[:, 13:].reshape(-1, 6)).view(P, 24, 3, 3)
            v = f.smpl(betas=x[:, 3:13].contiguous(), body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False, rotmats=R).vertices
            c = v[:, vert]                                            # [P,M,3,3]
            pts = w[None, :, 0, None] * c[:, :, 0] + w[None, :, 1, None] * c[:, :, 1] + w[None, :, 2, None] * c[:, :, 2]
            tz = 2.0 * f.focal / (f.res * x[:, 0] + 1e-9)
            D = pts[..., 2] + tz[:, None]
            e = f.kappa * (pts[..., :2] + x[:, None, 1:3]) / D[..., None] - obs[..., :2]
            r2 = (e * e).sum(-1)
            s2 = f.sigma_dense ** 2
            data = torch.where(~(D <= 1e-6), wl * (s2 * r2 / (s2 + r2)), torch.zeros_like(r2)).sum(1)
            dR = ((R - self.R0) ** 2).sum((-1, -2))
            return data + f.w_orient * dR[:, 0] + f.w_pose * dR[:, 1:].sum(1) + f.w_shape * ((x[:, 3:13] - self.x0[:, 3:13]) ** 2).sum(1)
    return Dense(fitter, para, None)


def _timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(v, scale=1.0, digits=4):
    v = np.asarray(v) * scale
    return {'median': round(float(np.median(v)), digits), 'p10': round(float(np.percentile(v, 10)), digits), 'p90': round(float(np.percentile(v, 90)), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser(description='dense fit: composed and replayed against the one-launch op')
    ap.add_argument('--people', default='1,8,32')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/densefit_bench.py needs a GPU (there is no CPU path)')
    from danet_densepose2smpl_amd.dense_fit import DenseFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL().cuda()
    fitter = DenseFitter(smpl)
    t = fitter.tables(torch.device('cuda', torch.cuda.current_device()))
    for P in [int(p) for p in a.people.split(',')]:
        init, iuv = rendered_inputs(smpl, P)
        obs = fitter.landmarks(iuv)
        _, info = fitter.fit(init, obs=obs, return_history=True)
        comp = composed(fitter, init, obs, info['gate'])
        comp.capture()
        ways = {'replay': lambda: comp.run(True), 'op': lambda: fitter.fit(init, obs=obs, return_history=True)[1]['history'],
                'landmarks': lambda: fitter.landmarks(iuv)}
        final = {}
        for _ in range(a.warmup):
            for k, f in ways.items():
                r = f()
                if k != 'landmarks':
                    final[k] = r[:, -1].clone()
        torch.cuda.synchronize()
        times = {k: [] for k in ways}
        for _ in range(a.reps):
            for k, f in ways.items():
                times[k].append(_timed(f))
        T = fitter.iterations
        line = {'tool': 'densefit_bench', 'P': P, 'iterations': T, 'support': int(t['S']), 'support_padded': int(t['Sp']), 'landmarks': int(t['M']),
                'grid': fitter.grid, 'S': S_IMG, 'reps': a.reps, 'warmup': a.warmup, 'observed': float((obs[..., 2] > 0).float().mean()),
                'E0': [round(float(v), 6) for v in info['history'][:, 0].cpu()[:4]], 'ET_op': [round(float(v), 6) for v in final['op'].cpu()[:4]],
                'ET_max_diff_op_vs_replay': float((final['op'] - final['replay']).abs().max())}
        for k in ('replay', 'op'):
            line[k] = dict(_stats(times[k]), unit='ms', us_per_iteration=round(float(np.median(times[k])) * 1000.0 / T, 2))
        line['landmarks_kernel'] = dict(_stats(times['landmarks'], 1000.0, 2), unit='us')
        line['op_faster_than_replay'] = bool(line['op']['median'] < line['replay']['median'])
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
