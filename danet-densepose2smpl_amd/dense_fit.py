"""Fit SMPL parameter rows to the predicted IUV image (DESIGN.md "the dense fit rule"), alone or together with 2D keypoints.

    fitter = DenseFitter(smpl, densepose=None, smpl_model=model_dict)        # the synthetic topology; or densepose = the UV_Processed dict
    obs = fitter.landmarks(iuv_image)                                         # [P,3,S,S] -> [P,M,3] (x, y, confidence)
    para_fit = fitter.fit(para, iuv_image)                                    # two launches
    para_fit, info = fitter.fit(para, obs=obs, keypoints=kp, return_history=True)   # one launch; info also holds 'gate', 'obs'

The landmarks are the mapped texels of the texture rule's texel map at T = grid (texture.TextureAtlas.texel_map, one launch per
device, copied to the host once); dense_tables turns them into the tables csrc/dense_fit.hip reads, in float64.  Everything else is
the keypoint fit (kp_fit.py): the same unknowns, priors, staged Adam, best iterate, status, history.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib, constants
from ._lib import check, ptr, require_gpu, stream
from .kp_fit import DEFAULT_STAGES, NKP, fit_tables, parse_stages
from .ops import _f32, _typed

PARTS = 24
GRID_MIN, GRID_MAX = 2, 6
W_MIN = 1e-3


def landmark_cells(face):
    """face [24,G,G] int (-1: unmapped) -> cell [M,3] int32 = (part 1..24, i, j) of the mapped texels in raster order."""
    face = np.asarray(face)
    p, i, j = np.nonzero(face >= 0)
    return np.stack([p + 1, i, j], 1).astype(np.int32)


def dense_tables(smpl, atlas_tables, face, bary):
    """The tables of the dense fit on the host, float64 / int32: kp_fit.fit_tables' dict over the support enlarged by the landmark
    corners, plus 'G', 'M', 'cell' [M,3] (part, i, j), 'lm_vert' [M,3] the corners' mesh vertices in the face's own order,
    'lm_corner' [M,3] their positions in the support, 'lm_w' [M,3] = (w0, w1, 1 - w0 - w1) from bary, and the inverse CSR
    ('csr_off' [Sp+1], 'csr_lm' [3M], 'csr_w' [3M]: per support vertex its (landmark, weight) pairs, ascending landmark)."""
    face, bary = np.asarray(face), np.asarray(bary)
    G = face.shape[-1]
    if face.shape != (PARTS, G, G) or bary.shape != (PARTS, G, G, 2) or not GRID_MIN <= G <= GRID_MAX:
        raise ValueError('dense_tables: a texel map [24,G,G] / [24,G,G,2] with G in %d..%d expected, got %s / %s' % (GRID_MIN, GRID_MAX, face.shape, bary.shape))
    cell = landmark_cells(face)
    M = cell.shape[0]
    if M < 1:
        raise ValueError('dense_tables: the texel map has no mapped texel')
    f = face[cell[:, 0] - 1, cell[:, 1], cell[:, 2]].astype(np.int64)
    b = bary[cell[:, 0] - 1, cell[:, 1], cell[:, 2]].astype(np.float64)
    lm_vert = np.asarray(atlas_tables['vert_mapping'], np.int64)[np.asarray(atlas_tables['faces'], np.int64)[f]]        # [M,3]
    lm_w = np.stack([b[:, 0], b[:, 1], 1.0 - b[:, 0] - b[:, 1]], 1)
    t = fit_tables(smpl, extra_verts=lm_vert)
    corner = np.searchsorted(t['support'], lm_vert).astype(np.int32)
    # vertex -> (landmark, weight): a stable sort by vertex of the (landmark, corner) pairs in ascending landmark order
    flat_v, flat_l, flat_w = corner.reshape(-1).astype(np.int64), np.repeat(np.arange(M), 3), lm_w.reshape(-1)
    order = np.argsort(flat_v, kind='stable')
    off = np.zeros(t['Sp'] + 1, np.int64)
    np.cumsum(np.bincount(flat_v, minlength=t['Sp']), out=off[1:])
    t.update({'G': int(G), 'M': int(M), 'cell': cell, 'lm_vert': lm_vert, 'lm_corner': corner, 'lm_w': lm_w, 'csr_off': off.astype(np.int32),
              'csr_lm': flat_l[order].astype(np.int32), 'csr_w': flat_w[order]})
    return t


class DenseFitter(object):
    """DenseFitter(smpl, densepose=None, grid=4, smpl_model=None, stages=, lr=, sigma=, w_pose=, w_orient=, w_shape=, focal=, res=,
    kappa=None, w_dense=, sigma_dense=, tau=None, min_cos=): `smpl` the SMPL layer; `densepose` the UV_Processed dict, or None for
    the seeded synthetic topology of `smpl_model` (as texture.TextureAtlas).  tau None: 1 / (4 grid).  The other hyper-parameters are
    KeypointFitter's; the defaults of the dense term are those of DESIGN.md, chosen on the dense recovery case."""

    def __init__(self, smpl, densepose=None, grid=4, smpl_model=None, stages=DEFAULT_STAGES, lr=0.02, sigma=0.1, w_pose=0.005,
                 w_orient=0.005, w_shape=0.002, focal=constants.FOCAL_LENGTH, res=constants.IMG_RES, kappa=None,
                 w_dense=0.25, sigma_dense=0.05, tau=None, min_cos=0.1):
        from .texture import TextureAtlas
        if int(grid) != grid or not GRID_MIN <= int(grid) <= GRID_MAX:
            raise ValueError('DenseFitter: grid %r (an integer in %d..%d)' % (grid, GRID_MIN, GRID_MAX))
        self.smpl, self.grid = smpl, int(grid)
        self.stages = tuple((int(n), g) for n, g in stages)
        parse_stages(self.stages)
        self.lr, self.sigma = float(lr), float(sigma)
        self.w_pose, self.w_orient, self.w_shape = float(w_pose), float(w_orient), float(w_shape)
        self.focal, self.res = float(focal), float(res)
        self.kappa = 2.0 * self.focal / self.res if kappa is None else float(kappa)
        self.w_dense, self.sigma_dense, self.min_cos = float(w_dense), float(sigma_dense), float(min_cos)
        self.tau = 1.0 / (4.0 * self.grid) if tau is None else float(tau)
        if not (self.sigma > 0 and self.sigma_dense > 0 and self.tau > 0 and self.w_dense >= 0):
            raise ValueError('DenseFitter: sigma, sigma_dense and tau must be positive, w_dense not negative')
        self.atlas = TextureAtlas(densepose, smpl_model, size=self.grid, focal_length=self.focal)
        self._host = None
        self._dev = {}

    @property
    def iterations(self):
        return sum(n for n, _ in self.stages)

    def host_tables(self, device=None):
        """dense_tables' dict, built at the first call (the texel map is made on `device` and copied to the host, once)."""
        if self._host is None:
            if device is None:
                device = torch.device('cuda', torch.cuda.current_device())
            face, bary = self.atlas.texel_map(device)
            self._host = dense_tables(self.smpl, self.atlas.tables, face.cpu().numpy(), bary.cpu().numpy())
        return self._host

    def tables(self, device):
        """The tables on `device` (fp32 / int32), built once and cached per device."""
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._dev.get(key)
        if t is None:
            h = self.host_tables(device)
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)          # noqa: E731
            t = {k: up(h[k], np.float32) for k in ('v_template', 'basis', 'basisT', 'weights', 'jx', 'lm_w', 'csr_w')}
            t.update({k: up(h[k], np.int32) for k in ('lm', 'jmap', 'cell', 'lm_corner', 'csr_off', 'csr_lm')})
            t.update({k: h[k] for k in ('S', 'Sp', 'NB', 'M', 'G')})
            self._dev[key] = t
        return t

    def landmarks(self, iuv_image, return_weight=False):
        """iuv_image [P,3,S,S] on the GPU (plane 0 part / 24, planes 1, 2 U and V: what iuvmap.iuv_map2img and the rasteriser give)
        -> obs [P,M,3] f32 = (x, y, c) in the fit's image coordinates; with return_weight also W [P,M], the summed weight.  One
        launch, no synchronisation."""
        require_gpu(iuv_image, 'DenseFitter.landmarks')
        img = _f32(iuv_image, (None, 3, None, None), 'DenseFitter.landmarks: iuv_image')
        P, S = img.shape[0], img.shape[2]
        if P < 1 or S < 1 or img.shape[3] != S:
            raise ValueError('DenseFitter.landmarks: a non-empty batch of square images [P,3,S,S] expected, got %s' % (tuple(img.shape),))
        t = self.tables(img.device)
        M, G = int(t['M']), int(t['G'])
        cell = _typed(t['cell'], torch.int32, (M, 3), 'DenseFitter.landmarks: cell')
        obs = torch.empty(P, M, 3, device=img.device, dtype=torch.float32)
        W = torch.empty(P, M, device=img.device, dtype=torch.float32) if return_weight else None
        check(_lib.lib().danet_dense_landmarks(ptr(img), ptr(cell), P, M, S, G, self.tau, W_MIN, ptr(obs), ptr(W), stream()),
              'danet_dense_landmarks')
        return (obs, W) if return_weight else obs

    def fit(self, para, iuv_image=None, keypoints=None, obs=None, return_history=False, return_grad=False, stages=None, kappa=None):
        """para [P,229] on the GPU, and iuv_image [P,3,S,S] or obs [P,M,3] (exactly one of the two), optionally keypoints [P,49,3]
        -> para_fit [P,229]; with return_history / return_grad also a dict with 'history' [P,T+1], 'best_iter' [P], 'status' [P],
        'gate' [P,M] int32, 'obs' [P,M,3] (and 'grad' [P,157], dE/dx at x_0).  Two launches with an image, one with obs; no
        synchronisation, no allocation by data."""
        if (iuv_image is None) == (obs is None):
            raise ValueError('DenseFitter.fit: exactly one of iuv_image and obs')
        parse_stages(self.stages if stages is None else stages)
        require_gpu(para, 'DenseFitter.fit')
        require_gpu(iuv_image if obs is None else obs, 'DenseFitter.fit: ' + ('iuv_image' if obs is None else 'obs'))
        if keypoints is not None:
            require_gpu(keypoints, 'DenseFitter.fit: keypoints')
        tables = self.tables(para.device)
        stages = self.stages if stages is None else stages
        kappa = self.kappa if kappa is None else kappa
        S, Sp, NB, M = int(tables['S']), int(tables['Sp']), int(tables['NB']), int(tables['M'])
        p = _f32(para, (None, 3 + NB + 216), 'DenseFitter.fit: para')
        P = p.shape[0]
        if P < 1:
            raise ValueError('DenseFitter.fit: an empty batch')
        dev = p.device
        iters, masks = parse_stages(stages)
        if obs is None:
            img = _f32(iuv_image, (P, 3, None, None), 'DenseFitter.fit: iuv_image')
            if img.device != dev:
                raise ValueError('DenseFitter.fit: para and iuv_image must be on one device')
            ob = self.landmarks(img)
        else:
            ob = _f32(obs, (P, M, 3), 'DenseFitter.fit: obs')
        kp = torch.zeros(P, 49, 3, device=dev, dtype=torch.float32) if keypoints is None else _f32(keypoints, (P, 49, 3), 'DenseFitter.fit: keypoints')
        NL, NE = tables['lm'].numel(), tables['jx'].shape[0]
        NK = 207 + NB
        vt = _typed(tables['v_template'], torch.float32, (Sp * 3,), 'DenseFitter.fit: v_template')
        basis = _typed(tables['basis'], torch.float32, (NK, Sp * 3), 'DenseFitter.fit: basis')
        basisT = _typed(tables['basisT'], torch.float32, (Sp * 3, NKP), 'DenseFitter.fit: basisT')
        wts = _typed(tables['weights'], torch.float32, (Sp, 24), 'DenseFitter.fit: weights')
        jx = _typed(tables['jx'], torch.float32, (NE, Sp), 'DenseFitter.fit: jx')
        lm = _typed(tables['lm'], torch.int32, (NL,), 'DenseFitter.fit: lm')
        jmap = _typed(tables['jmap'], torch.int32, (49,), 'DenseFitter.fit: jmap')
        corner = _typed(tables['lm_corner'], torch.int32, (M, 3), 'DenseFitter.fit: lm_corner')
        lmw = _typed(tables['lm_w'], torch.float32, (M, 3), 'DenseFitter.fit: lm_w')
        coff = _typed(tables['csr_off'], torch.int32, (Sp + 1,), 'DenseFitter.fit: csr_off')
        clm = _typed(tables['csr_lm'], torch.int32, (3 * M,), 'DenseFitter.fit: csr_lm')
        cw = _typed(tables['csr_w'], torch.float32, (3 * M,), 'DenseFitter.fit: csr_w')
        Jt = _typed(self.smpl.J_template, torch.float32, (24, 3), 'DenseFitter.fit: J_template')
        Jd = _typed(self.smpl.J_shapedirs, torch.float32, (72, NB), 'DenseFitter.fit: J_shapedirs')
        par = _typed(self.smpl.parents, torch.int32, (24,), 'DenseFitter.fit: parents')
        if any(t.device != dev for t in (kp, ob, vt, basis, basisT, wts, jx, lm, jmap, corner, lmw, coff, clm, cw, Jt, Jd, par)):
            raise ValueError('DenseFitter.fit: para, the observations, the SMPL layer and the tables must be on one device')
        T = sum(iters)
        L = _lib.lib()
        a = _lib.DenseFitArgs()
        para_fit = torch.empty_like(p)
        history = torch.empty(P, T + 1, device=dev, dtype=torch.float32)
        best_iter = torch.empty(P, device=dev, dtype=torch.int32)
        status = torch.empty(P, device=dev, dtype=torch.int32)
        gate = torch.empty(P, M, device=dev, dtype=torch.int32)
        grad = torch.empty(P, 3 + NB + 144, device=dev, dtype=torch.float32) if return_grad else None
        nws = L.danet_dense_fit_ws_floats(P, Sp)
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        for k, t in (('para', p), ('kp', kp), ('J_template', Jt), ('J_shapedirs', Jd), ('parents', par), ('v_template', vt), ('basis', basis),
                     ('basisT', basisT), ('weights', wts), ('jx', jx if NE else None), ('lm', lm if NL else None), ('jmap', jmap), ('ws', ws),
                     ('para_fit', para_fit), ('history', history), ('best_iter', best_iter), ('status', status), ('grad0', grad),
                     ('lm_corner', corner), ('lm_w', lmw), ('csr_off', coff), ('csr_lm', clm), ('csr_w', cw), ('obs', ob), ('gate', gate)):
            setattr(a, k, ptr(t))
        for i, (n, m) in enumerate(zip(iters, masks)):
            a.stage_iters[i], a.stage_mask[i] = n, m
        a.P, a.NB, a.S, a.Sp, a.NL, a.NE, a.nstages, a.T, a.M = P, NB, S, Sp, NL, NE, len(iters), T, M
        a.focal, a.res, a.kappa, a.sigma = self.focal, self.res, float(kappa), self.sigma
        a.w_orient, a.w_pose, a.w_shape, a.lr = self.w_orient, self.w_pose, self.w_shape, self.lr
        a.w_dense, a.sigma_dense, a.min_cos = self.w_dense, self.sigma_dense, self.min_cos
        check(L.danet_dense_fit(ctypes.addressof(a), nws, stream()), 'danet_dense_fit')
        if not (return_history or return_grad):
            return para_fit
        info = {'history': history, 'best_iter': best_iter, 'status': status, 'gate': gate, 'obs': ob}
        if return_grad:
            info['grad'] = grad
        return para_fit, info
