"""Fit SMPL parameter rows to 2D keypoints (DESIGN.md "fit rule"): the step after the regression.

    fitter = KeypointFitter(smpl)
    para_fit = fitter.fit(para, keypoints)                                   # [P,229], [P,49,3] (u, v, confidence) -> [P,229]
    para_fit, info = fitter.fit(para, keypoints, return_history=True)        # info: history [P,T+1], best_iter [P], status [P]

The regression is the initialisation and the prior; the whole fit of all P people is ONE launch (csrc/kp_fit.hip, one workgroup
per person, every iteration inside the kernel).  The kernel reads the SMPL tables restricted to the support set -- the landmark
vertices and the vertices J_regressor_extra touches --, built once by fit_tables (in float64) and cached on the fitter per device;
nothing is registered on the SMPL layer.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib, constants
from ._lib import check, ptr, require_gpu, stream
from .ops import _f32, _typed

GROUPS = {'cam': 1, 'orient': 2, 'body': 4, 'shape': 8, 'all': 15}
DEFAULT_STAGES = ((30, 'cam+orient'), (70, 'all'))
TILE = 128          # the kernel's vertex tile: every vertex axis of the tables is zero-padded to a multiple of it
NKP = 224           # padded feature axis of basisT (207 pose features + up to 16 betas)
# BODY_25 rows are the first 25 of the 49 joints, in the same order (constants.JOINT_MAP_49)
NUM_OPENPOSE = 25


def group_mask(groups):
    """'cam+orient', 'all', or an iterable of group names -> the kernel's bit mask."""
    names = groups.split('+') if isinstance(groups, str) else list(groups)
    mask = 0
    for n in names:
        if n not in GROUPS:
            raise ValueError('keypoint fit: unknown parameter group %r (one of %s)' % (n, ', '.join(GROUPS)))
        mask |= GROUPS[n]
    return mask


def parse_stages(stages):
    """((iterations, groups), ...) -> ([iterations], [masks]); at most four stages."""
    iters, masks = [], []
    for st in stages:
        n, g = st
        if int(n) != n or n < 0:
            raise ValueError('keypoint fit: a stage of %r iterations' % (n,))
        iters.append(int(n))
        masks.append(group_mask(g))
    if len(iters) > 4:
        raise ValueError('keypoint fit: %d stages, at most 4' % len(iters))
    return iters, masks


def fit_tables(smpl, extra_verts=None):
    """The support sub-tables of an SMPL layer, as float64 / int32 numpy arrays (the layout csrc/kp_fit.hip reads, include/danet_hip.h):
    'support' [S] the vertex indices (ascending), 'S', 'Sp' (S padded to the tile), 'v_template' [Sp*3], 'basis' [207+NB, Sp*3]
    (posedirs rows, then shapedirs transposed), 'basisT' [Sp*3, 224], 'weights' [Sp,24], 'jx' [NE,Sp], 'lm' [NL] (position of each
    landmark vertex in the support) and 'jmap' [49].  Padding is zero.  extra_verts: further mesh vertices for the support (the
    dense fit's landmark corners)."""
    g = lambda n: getattr(smpl, n).detach().cpu().numpy()           # noqa: E731
    jx_full = g('J_regressor_extra').astype(np.float64)             # [NE,V]
    lmv = g('landmark_verts').astype(np.int64)
    V = g('v_template').shape[0]
    NB = smpl.num_betas
    support = np.union1d(lmv, np.nonzero((jx_full != 0).any(0))[0]).astype(np.int64)
    if extra_verts is not None:
        support = np.union1d(support, np.asarray(extra_verts, np.int64).reshape(-1))
    S = support.size
    Sp = -(-S // TILE) * TILE
    coords = (support[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
    NK = 207 + NB
    if NK > NKP - 1:
        raise ValueError('fit_tables: %d betas' % NB)
    vt = np.zeros(Sp * 3)
    vt[:S * 3] = g('v_template').astype(np.float64).reshape(-1)[coords]
    basis = np.zeros((NK, Sp * 3))
    basis[:207, :S * 3] = g('posedirs').astype(np.float64)[:, coords]
    basis[207:, :S * 3] = g('shapedirs').astype(np.float64).reshape(V * 3, NB)[coords].T
    basisT = np.zeros((Sp * 3, NKP))
    basisT[:, :NK] = basis.T
    weights = np.zeros((Sp, 24))
    weights[:S] = g('lbs_weights').astype(np.float64)[support]
    jx = np.zeros((jx_full.shape[0], Sp))
    jx[:, :S] = jx_full[:, support]
    lm = np.searchsorted(support, lmv).astype(np.int32)
    return {'support': support, 'S': int(S), 'Sp': int(Sp), 'NB': int(NB), 'v_template': vt, 'basis': basis, 'basisT': basisT,
            'weights': weights, 'jx': jx, 'lm': lm, 'jmap': np.asarray(constants.JOINT_MAP_49, np.int32)}


def openpose_to_j49(pose_keypoints_2d):
    """OpenPose BODY_25 keypoints ([25,3], [n,25,3] or the flat list of a JSON file: x, y, confidence) -> [.., 49, 3] float32 with the
    25 rows first and the other 24 joints at confidence 0."""
    k = np.asarray(pose_keypoints_2d, np.float32)
    if k.ndim == 1:
        k = k.reshape(-1, 3)
    if k.shape[-2:] != (NUM_OPENPOSE, 3):
        raise ValueError('openpose_to_j49: BODY_25 keypoints [25,3] expected, got shape %s' % (k.shape,))
    out = np.zeros(k.shape[:-2] + (49, 3), np.float32)
    out[..., :NUM_OPENPOSE, :] = k
    return out


class KeypointFitter(object):
    """KeypointFitter(smpl, stages=, lr=, sigma=, w_pose=, w_orient=, w_shape=, focal=, res=, kappa=None): `smpl` the SMPL layer (on the
    GPU when fit is called).  kappa None: 2 focal / res, the training convention; the scene demo passes 2 focal / 224.  The defaults
    are those of DESIGN.md, chosen on the synthetic recovery case."""

    def __init__(self, smpl, stages=DEFAULT_STAGES, lr=0.02, sigma=0.1, w_pose=0.005, w_orient=0.005, w_shape=0.002,
                 focal=constants.FOCAL_LENGTH, res=constants.IMG_RES, kappa=None):
        self.smpl = smpl
        self.stages = tuple((int(n), g) for n, g in stages)
        parse_stages(self.stages)
        self.lr, self.sigma = float(lr), float(sigma)
        self.w_pose, self.w_orient, self.w_shape = float(w_pose), float(w_orient), float(w_shape)
        self.focal, self.res = float(focal), float(res)
        self.kappa = 2.0 * self.focal / self.res if kappa is None else float(kappa)
        self._host = None
        self._dev = {}

    @property
    def iterations(self):
        return sum(n for n, _ in self.stages)

    def tables(self, device):
        """The sub-tables on `device` (fp32 / int32), built once and cached per device."""
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._dev.get(key)
        if t is None:
            if self._host is None:
                self._host = fit_tables(self.smpl)
            h = self._host
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)          # noqa: E731
            t = {k: up(h[k], np.float32) for k in ('v_template', 'basis', 'basisT', 'weights', 'jx')}
            t.update({k: up(h[k], np.int32) for k in ('lm', 'jmap')})
            t.update({k: h[k] for k in ('S', 'Sp', 'NB')})
            self._dev[key] = t
        return t

    def fit(self, para, keypoints, return_history=False, return_grad=False, stages=None, kappa=None):
        """para [P,229], keypoints [P,49,3] on the GPU -> para_fit [P,229]; with return_history / return_grad also a dict with 'history'
        [P,T+1], 'best_iter' [P], 'status' [P] (and 'grad' [P,157], dE/dx at x_0).  No synchronisation, no allocation by data.  The arguments
        go through the rules of ops.py (_f32, _typed) and then to danet_kp_fit, one launch."""
        require_gpu(para, 'KeypointFitter.fit')
        require_gpu(keypoints, 'KeypointFitter.fit: keypoints')
        tables = self.tables(para.device)
        stages = self.stages if stages is None else stages
        kappa = self.kappa if kappa is None else kappa
        S, Sp, NB = int(tables['S']), int(tables['Sp']), int(tables['NB'])
        p = _f32(para, (None, 3 + NB + 216), 'KeypointFitter.fit: para')
        P = p.shape[0]
        if P < 1:
            raise ValueError('KeypointFitter.fit: an empty batch')
        kp = _f32(keypoints, (P, 49, 3), 'KeypointFitter.fit: keypoints')
        dev = p.device
        NL, NE = tables['lm'].numel(), tables['jx'].shape[0]
        NK = 207 + NB
        vt = _typed(tables['v_template'], torch.float32, (Sp * 3,), 'KeypointFitter.fit: v_template')
        basis = _typed(tables['basis'], torch.float32, (NK, Sp * 3), 'KeypointFitter.fit: basis')
        basisT = _typed(tables['basisT'], torch.float32, (Sp * 3, NKP), 'KeypointFitter.fit: basisT')
        wts = _typed(tables['weights'], torch.float32, (Sp, 24), 'KeypointFitter.fit: weights')
        jx = _typed(tables['jx'], torch.float32, (NE, Sp), 'KeypointFitter.fit: jx')
        lm = _typed(tables['lm'], torch.int32, (NL,), 'KeypointFitter.fit: lm')
        jmap = _typed(tables['jmap'], torch.int32, (49,), 'KeypointFitter.fit: jmap')
        Jt = _typed(self.smpl.J_template, torch.float32, (24, 3), 'KeypointFitter.fit: J_template')
        Jd = _typed(self.smpl.J_shapedirs, torch.float32, (72, NB), 'KeypointFitter.fit: J_shapedirs')
        par = _typed(self.smpl.parents, torch.int32, (24,), 'KeypointFitter.fit: parents')
        if any(t.device != dev for t in (kp, vt, basis, basisT, wts, jx, lm, jmap, Jt, Jd, par)):
            raise ValueError('KeypointFitter.fit: para, keypoints, the SMPL layer and the tables must be on one device')
        iters, masks = parse_stages(stages)
        T = sum(iters)
        L = _lib.lib()
        a = _lib.KpFitArgs()
        para_fit = torch.empty_like(p)
        history = torch.empty(P, T + 1, device=dev, dtype=torch.float32)
        best_iter = torch.empty(P, device=dev, dtype=torch.int32)
        status = torch.empty(P, device=dev, dtype=torch.int32)
        grad = torch.empty(P, 3 + NB + 144, device=dev, dtype=torch.float32) if return_grad else None
        nws = L.danet_kp_fit_ws_floats(P, Sp)
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        for k, t in (('para', p), ('kp', kp), ('J_template', Jt), ('J_shapedirs', Jd), ('parents', par), ('v_template', vt), ('basis', basis),
                     ('basisT', basisT), ('weights', wts), ('jx', jx if NE else None), ('lm', lm if NL else None), ('jmap', jmap), ('ws', ws),
                     ('para_fit', para_fit), ('history', history), ('best_iter', best_iter), ('status', status), ('grad0', grad)):
            setattr(a, k, ptr(t))
        for i, (n, m) in enumerate(zip(iters, masks)):
            a.stage_iters[i], a.stage_mask[i] = n, m
        a.P, a.NB, a.S, a.Sp, a.NL, a.NE, a.nstages, a.T = P, NB, S, Sp, NL, NE, len(iters), T
        a.focal, a.res, a.kappa, a.sigma = self.focal, self.res, float(kappa), self.sigma
        a.w_orient, a.w_pose, a.w_shape, a.lr = self.w_orient, self.w_pose, self.w_shape, self.lr
        check(L.danet_kp_fit(ctypes.addressof(a), nws, stream()), 'danet_kp_fit')
        if not (return_history or return_grad):
            return para_fit
        info = {'history': history, 'best_iter': best_iter, 'status': status}
        if return_grad:
            info['grad'] = grad
        return para_fit, info
