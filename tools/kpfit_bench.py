"""The keypoint fit rule (DESIGN.md "fit rule") run three ways on the synthetic recovery case at P = 1, 8 and 32 people, default stages
(100 iterations, 101 energy evaluations):

  eager     composed from the existing ops -- ops.rot6d_to_rotmat, the SMPL layer (full LBS, autograd), projection, energy and Adam in
            torch -- run eagerly, one iteration after the other
  replay    the same composition with ONE iteration captured under torch.cuda.graph and replayed 100 times (the step count, the group
            mask and the history index are device tensors)
  op        kp_fit.KeypointFitter.fit: one launch

  python tools/kpfit_bench.py [--people 1,8,32] [--reps 20] [--warmup 3]

Times are HIP events around a whole fit, the three ways alternating inside every repetition; reported are the median and p10 / p90
in milliseconds, the per-iteration time (median / 100) in microseconds, the support size, and the largest difference of the final
energies between the ways (the composition sums in another order; the values agree to single precision).  One JSON line per P."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recovery_inputs(smpl, P, seed=7):
    """P rows (cam, betas, rotations), their keypoints through the SMPL layer and the rule's camera, and a perturbed start."""
    import torch
    from danet_densepose2smpl_amd import constants, ops
    from danet_densepose2smpl_amd.smpl import from_para
    g = torch.Generator().manual_seed(seed)
    betas = torch.randn(P, 10, generator=g).clamp(-3, 3)
    R = ops.rodrigues_smplx((0.2 * torch.randn(P * 24, 3, generator=g)).cuda()).view(P, 216)
    cam = torch.stack([0.6 + 0.5 * torch.rand(P, generator=g), 0.2 * torch.rand(P, generator=g) - 0.1, 0.2 * torch.rand(P, generator=g) - 0.1], 1)
    star = torch.cat([cam.cuda(), betas.cuda(), R], 1)
    j = from_para(smpl, star).joints
    kappa = 2.0 * constants.FOCAL_LENGTH / constants.IMG_RES
    tz = 2.0 * constants.FOCAL_LENGTH / (constants.IMG_RES * star[:, 0] + 1e-9)
    uv = kappa * (j[..., :2] + star[:, None, 1:3]) / (j[..., 2:3] + tz[:, None, None])
    kp = torch.cat([uv, torch.ones(P, 49, 1, device='cuda')], 2).contiguous()
    noise = ops.rodrigues_smplx((0.15 * torch.randn(P * 24, 3, generator=g)).cuda()).view(P, 24, 3, 3)
    init = star.clone()
    init[:, 13:] = (star[:, 13:].view(P, 24, 3, 3) @ noise).reshape(P, 216)
    init[:, 0] *= 1.1
    init[:, 1:3] += 0.05
    return init.contiguous(), kp


class Composed(object):
    """The rule from the existing ops.  One object serves the eager and the replayed run."""

    def __init__(self, fitter, para, kp):
        import torch
        from danet_densepose2smpl_amd import ops
        self.torch, self.ops, self.f, self.kp = torch, ops, fitter, kp
        P = para.shape[0]
        R = para[:, 13:].view(P, 24, 3, 3)
        self.x0 = torch.cat([para[:, :13], R[..., :2].reshape(P, 144)], 1).contiguous()
        with torch.no_grad():
            self.R0 = ops.rot6d_to_rotmat(self.x0[:, 13:].reshape(-1, 6)).view(P, 24, 3, 3)
        self.T = fitter.iterations
        groups = torch.tensor([1] * 3 + [8] * 10 + [2] * 6 + [4] * 138, device='cuda')
        from danet_densepose2smpl_amd.kp_fit import parse_stages
        self.iters, masks = parse_stages(fitter.stages)
        self.masks = [((groups & m) != 0).float()[None] for m in masks]
        self.x = self.x0.clone().requires_grad_(True)
        z = lambda *s: torch.zeros(*s, device='cuda')            # noqa: E731
        self.mom, self.var, self.step, self.mask = z(P, 157), z(P, 157), z(1), z(1, 157)
        self.hist, self.iti = z(P, self.T + 1), torch.zeros(1, dtype=torch.long, device='cuda')
        self.bestE, self.xbest = z(P), self.x0.clone()

    def energy(self, x):
        torch, f = self.torch, self.f
        P = x.shape[0]
        R = self.ops.rot6d_to_rotmat(x[:, 13:].reshape(-1, 6)).view(P, 24, 3, 3)
        j = f.smpl(betas=x[:, 3:13].contiguous(), body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False, rotmats=R).joints
        tz = 2.0 * f.focal / (f.res * x[:, 0] + 1e-9)
        D = j[..., 2] + tz[:, None]
        e = f.kappa * (j[..., :2] + x[:, None, 1:3]) / D[..., None] - self.kp[..., :2]
        r2 = (e * e).sum(-1)
        s2 = f.sigma ** 2
        data = torch.where(~(D <= 1e-6), self.kp[..., 2] ** 2 * (s2 * r2 / (s2 + r2)), torch.zeros_like(r2)).sum(1)
        dR = ((R - self.R0) ** 2).sum((-1, -2))
        return data + f.w_orient * dR[:, 0] + f.w_pose * dR[:, 1:].sum(1) + f.w_shape * ((x[:, 3:13] - self.x0[:, 3:13]) ** 2).sum(1)

    def reset(self):
        with self.torch.no_grad():
            self.x.copy_(self.x0)
            self.xbest.copy_(self.x0)
            self.iti.zero_()
            self.bestE.fill_(float('inf'))

    def stage(self, k):
        with self.torch.no_grad():
            self.mom.zero_()
            self.var.zero_()
            self.step.zero_()
            self.mask.copy_(self.masks[k])

    def record(self, E):
        torch = self.torch
        self.hist.index_copy_(1, self.iti, E.detach()[:, None])
        better = E.detach() < self.bestE
        self.bestE.copy_(torch.where(better, E.detach(), self.bestE))
        self.xbest.copy_(torch.where(better[:, None], self.x.detach(), self.xbest))
        self.iti.add_(1)

    def iteration(self):
        torch, f = self.torch, self.f
        E = self.energy(self.x)
        (g,) = torch.autograd.grad(E.sum(), self.x)
        with torch.no_grad():
            self.record(E)
            self.step.add_(1)
            g = g * self.mask
            self.mom.mul_(0.9).add_(g, alpha=0.1)
            self.var.mul_(0.999).addcmul_(g, g, value=0.001)
            mh, vh = self.mom / (1 - torch.pow(0.9, self.step)), self.var / (1 - torch.pow(0.999, self.step))
            self.x.sub_(self.mask * f.lr * mh / (vh.sqrt() + 1e-8))
            self.x[:, 0].copy_(torch.maximum(self.x[:, 0], 0.1 * self.x0[:, 0]))

    def final(self):
        with self.torch.no_grad():
            self.record(self.energy(self.x))

    def capture(self):
        torch = self.torch
        self.reset()
        self.stage(0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self.iteration()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):             # (the warmed stream: per-stream state of the ops exists already)
            self.iteration()

    def run(self, replay):
        self.reset()
        for k, n in enumerate(self.iters):
            self.stage(k)
            for _ in range(n):
                if replay:
                    self.graph.replay()
                else:
                    self.iteration()
        self.final()
        return self.hist


def main(argv=None):
    ap = argparse.ArgumentParser(description='keypoint fit: composed eager, composed replayed, one-launch op')
    ap.add_argument('--people', default='1,8,32')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/kpfit_bench.py needs a GPU (there is no CPU path)')
    from danet_densepose2smpl_amd.kp_fit import KeypointFitter
    from danet_densepose2smpl_amd.smpl import SMPL
    smpl = SMPL().cuda()
    fitter = KeypointFitter(smpl)
    S = fitter.tables(torch.device('cuda', torch.cuda.current_device()))['S']
    for P in [int(p) for p in a.people.split(',')]:
        init, kp = recovery_inputs(smpl, P)
        comp = Composed(fitter, init, kp)
        comp.capture()
        ways = {'eager': lambda: comp.run(False), 'replay': lambda: comp.run(True),
                'op': lambda: fitter.fit(init, kp, return_history=True)[1]['history']}
        final = {}
        for _ in range(a.warmup):
            for k, f in ways.items():
                final[k] = f()[:, -1].clone()
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
        T = fitter.iterations
        line = {'tool': 'kpfit_bench', 'P': P, 'iterations': T, 'support': int(S), 'reps': a.reps, 'warmup': a.warmup,
                'E0': [round(float(v), 6) for v in comp.hist[:, 0].cpu()[:4]], 'ET_op': [round(float(v), 6) for v in final['op'].cpu()[:4]],
                'ET_max_diff_vs_eager': {k: float((final[k] - final['eager']).abs().max()) for k in ('replay', 'op')}}
        for k, v in times.items():
            v = np.asarray(v)
            line[k] = {'ms': round(float(np.median(v)), 4), 'p10': round(float(np.percentile(v, 10)), 4), 'p90': round(float(np.percentile(v, 90)), 4),
                       'us_per_iteration': round(float(np.median(v)) * 1000.0 / T, 2)}
        line['op_faster_than_replay'] = bool(line['op']['ms'] < line['replay']['ms'])
        print(json.dumps(line), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
