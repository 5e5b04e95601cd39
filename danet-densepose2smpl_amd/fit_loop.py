"""Fit in the loop (DESIGN.md 4d "the refresh rule"): after a training step the regressor's prediction is refined on the batch's 2D
keypoints and, where the fit explains them better than the stored pseudo-label, replaces that label in FitsDict's table.

    loop = InLoopFit(smpl, fits_dict)                                   # tau = sigma^2 / 5, the fitter's default stages
    stats = loop.refresh(output['para'], in_dict, rows, rot_flip, has_smpl)
    # stats: 'updated' int32 [B], 'e_old' / 'e_new' f32 [B] (data energies on the batch's keypoints), 'eligible' bool [B]

Three launches of the library and a few tensor ops, all on the current stream: the fit (kp_fit.KeypointFitter.fit), one T = 0 call
of the same fitter on the 2B rows [para_fit; para_old] for the two data energies, and danet_fits_accept (csrc/fit_loop.hip), which
decides and writes the table and its valid flags.  Nothing is synchronised, no allocation is sized by data, the call can be captured
under torch.cuda.graph.  There is no CPU path."""
import ctypes

import torch

from . import _lib, ops
from ._lib import check, ptr, require_gpu, stream
from .kp_fit import KeypointFitter
from .ops import _f32, _typed


def stages_for(iters):
    """num_smplify_iters -> the fitter's stages: None the fitter's own default, n -> ((round(0.3 n), 'cam+orient'), (n - round(0.3 n),
    'all')) (100 is the default ((30, ..), (70, ..)); round is Python's: halves go to the even number)."""
    if iters is None:
        return None
    n = int(iters)
    if n != iters or n < 0:
        raise ValueError('InLoopFit: %r iterations' % (iters,))
    first = int(round(0.3 * n))
    return ((first, 'cam+orient'), (n - first, 'all'))


def default_tau(sigma):
    """sigma^2 / 5 = rho((sigma / 2)^2): a mean residual of half the outlier scale per unit of squared confidence.  A convention of this
    project; what it admits on real data is unpinned."""
    return float(sigma) ** 2 / 5.0


class InLoopFit(object):
    """InLoopFit(smpl, fits_dict, fitter=None, tau=None, iters=None): `smpl` the SMPL layer, `fits_dict` the FitsDict whose table is
    refreshed, `fitter` a kp_fit.KeypointFitter (default: one with the defaults of DESIGN.md and kappa = 2 f / res, the training
    convention), `tau` the valid-fit threshold (options.smplify_threshold; default default_tau(fitter.sigma)), `iters` the number of
    fit iterations (options.num_smplify_iters; None: the fitter's default stages)."""

    def __init__(self, smpl, fits_dict, fitter=None, tau=None, iters=None):
        self.smpl, self.fits_dict = smpl, fits_dict
        self.fitter = KeypointFitter(smpl) if fitter is None else fitter
        self.tau = default_tau(self.fitter.sigma) if tau is None else float(tau)
        self.stages = stages_for(iters)

    @torch.no_grad()
    def refresh(self, para, in_dict, rows, rot_flip, has_smpl):
        """para [B,229]: the prediction of the step (output['para']); in_dict: the step's, of which 'keypoints' [B,49,3], 'target_cam'
        [B,3], 'opt_betas' [B,10] and 'opt_pose' [B,72] are read -- the label as the step saw it, in the augmented frame; rows int64 [B]:
        the table rows (FitsDict.rows); rot_flip float64 [B,2]: (degrees, flip) of each sample's augmentation; has_smpl [B]: rows with
        ground truth are never touched.  Updates fits_dict.table / fits_dict.valid in place under the refresh rule.
        -> {'updated' int32 [B], 'e_old' [B], 'e_new' [B], 'eligible' bool [B]}, device tensors."""
        require_gpu(para, 'InLoopFit.refresh')
        p0 = _f32(para, (None, 229), 'InLoopFit.refresh: para')
        B = p0.shape[0]
        if B < 1:
            raise ValueError('InLoopFit.refresh: an empty batch')
        kp = _f32(in_dict['keypoints'], (B, 49, 3), 'InLoopFit.refresh: keypoints')
        cam = _f32(in_dict['target_cam'], (B, 3), 'InLoopFit.refresh: target_cam')
        betas = _f32(in_dict['opt_betas'], (B, 10), 'InLoopFit.refresh: opt_betas')
        pose = _f32(in_dict['opt_pose'], (B, 72), 'InLoopFit.refresh: opt_pose')
        hs = _f32(has_smpl, (B,), 'InLoopFit.refresh: has_smpl')
        rw = _typed(rows, torch.int64, (B,), 'InLoopFit.refresh: rows')
        rf = _typed(rot_flip, torch.float64, (B, 2), 'InLoopFit.refresh: rot_flip')
        table, valid = self.fits_dict.table, self.fits_dict.valid
        if any(t.device != p0.device for t in (kp, cam, betas, pose)):
            raise ValueError('InLoopFit.refresh: the prediction and the batch must be on one device')
        para_old = torch.cat([cam, betas, ops.batch_rodrigues(pose).view(B, 216)], dim=1)
        para_fit, fit = self.fitter.fit(p0, kp, return_history=True, stages=self.stages)
        _, ev = self.fitter.fit(torch.cat([para_fit, para_old]), torch.cat([kp, kp]), return_history=True, stages=())
        energy = ev['history'].view(2 * B)                       # (T = 0: the priors are exactly zero, both are data terms)
        e_new, e_old = energy[:B], energy[B:]
        updated = accept(para_fit, e_new, e_old, fit['status'], ev['status'][:B], hs, rw, rf, kp, table, valid, self.tau)
        return {'updated': updated, 'e_old': e_old, 'e_new': e_new, 'eligible': hs == 0}


def accept(para_fit, e_new, e_old, status_fit, status_eval, has_smpl, rows, rot_flip, keypoints, table, valid, tau):
    """danet_fits_accept on given energies and status words (refresh's last launch alone; the tests set the energies by hand):
    updates table [N,82] f32 / valid [N] u8 in place -> updated int32 [B]."""
    require_gpu(para_fit, 'fit_loop.accept')
    pf = _f32(para_fit, (None, 229), 'fit_loop.accept: para_fit')
    B = pf.shape[0]
    if B < 1:
        raise ValueError('fit_loop.accept: an empty batch')
    N = table.shape[0] if torch.is_tensor(table) and table.dim() == 2 else 0
    ts = {'para_fit': pf, 'e_new': _f32(e_new, (B,), 'fit_loop.accept: e_new'), 'e_old': _f32(e_old, (B,), 'fit_loop.accept: e_old'),
          'status_fit': _typed(status_fit, torch.int32, (B,), 'fit_loop.accept: status_fit'),
          'status_eval': _typed(status_eval, torch.int32, (B,), 'fit_loop.accept: status_eval'),
          'has_smpl': _f32(has_smpl, (B,), 'fit_loop.accept: has_smpl'), 'rows': _typed(rows, torch.int64, (B,), 'fit_loop.accept: rows'),
          'rot_flip': _typed(rot_flip, torch.float64, (B, 2), 'fit_loop.accept: rot_flip'),
          'kp': _f32(keypoints, (B, 49, 3), 'fit_loop.accept: keypoints'), 'table': _typed(table, torch.float32, (N, 82), 'fit_loop.accept: table'),
          'valid': _typed(valid, torch.uint8, (N,), 'fit_loop.accept: valid')}
    if any(t.device != pf.device for t in ts.values()):
        raise ValueError('fit_loop.accept: every tensor must be on one device')
    ts['updated'] = torch.empty(B, device=pf.device, dtype=torch.int32)
    a = _lib.FitsAcceptArgs()
    for k, t in ts.items():
        setattr(a, k, ptr(t))
    a.N, a.B, a.NB, a.tau = N, B, 10, float(tau)
    check(_lib.lib().danet_fits_accept(ctypes.addressof(a), stream()), 'danet_fits_accept')
    return ts['updated']
