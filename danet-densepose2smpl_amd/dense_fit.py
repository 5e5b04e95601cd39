"""Fit SMPL parameter rows to the predicted IUV image (DESIGN.md "the dense fit rule"), alone or together with 2D keypoints.

    fitter = DenseFitter(smpl, densepose=None, smpl_model=model_dict)        # the synthetic topology; or densepose = the UV_Processed dict
    obs = fitter.landmarks(iuv_image)                                         # [P,3,S,S] -> [P,M,3] (x, y, confidence)
    para_fit = fitter.fit(para, iuv_image)                                    # two launches
    para_fit, info = fitter.fit(para, obs=obs, keypoints=kp, return_history=True)   # one launch; info also holds 'gate', 'obs'

The landmarks are the mapped texels of the texture rule's texel map at T = grid (texture.TextureAtlas.texel_map, one launch per
device, copied to the host once); dense_tables turns them into the tables csrc/dense_fit.hip reads, in float64.  Everything else is
the keypoint fit (kp_fit.py): the same unknowns, priors, staged Adam, best iterate, status, history.  There is no CPU path."""
import numpy as np
import torch

from . import _lib, constants
from ._lib import check, ptr, require_gpu, stream
from .kp_fit import DEFAULT_STAGES, KeypointFitter, fit_tables, parse_stages
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


class DenseFitter(KeypointFitter):
    """DenseFitter(smpl, densepose=None, grid=4, smpl_model=None, stages=, lr=, sigma=, w_pose=, w_orient=, w_shape=, focal=, res=,
    kappa=None, w_dense=, sigma_dense=, tau=None, min_cos=): `smpl` the SMPL layer; `densepose` the UV_Processed dict, or None for
    the seeded synthetic topology of `smpl_model` (as texture.TextureAtlas).  tau None: 1 / (4 grid).  The other hyper-parameters are
    KeypointFitter's, and so is everything the two fits share; the defaults of the dense term are those of DESIGN.md, chosen on the
    dense recovery case."""
    ARGS, ENTRY = 'DenseFitArgs', 'danet_dense_fit'
    F32_KEYS = KeypointFitter.F32_KEYS + ('lm_w', 'csr_w')
    I32_KEYS = KeypointFitter.I32_KEYS + ('cell', 'lm_corner', 'csr_off', 'csr_lm')
    HOST_KEYS = KeypointFitter.HOST_KEYS + ('M', 'G')
    FLOATS = KeypointFitter.FLOATS + ('w_dense', 'sigma_dense', 'min_cos')
    ONE_DEVICE = 'para, the observations, the SMPL layer and the tables'

    def __init__(self, smpl, densepose=None, grid=4, smpl_model=None, stages=DEFAULT_STAGES, lr=0.02, sigma=0.1, w_pose=0.005,
                 w_orient=0.005, w_shape=0.002, focal=constants.FOCAL_LENGTH, res=constants.IMG_RES, kappa=None,
                 w_dense=0.25, sigma_dense=0.05, tau=None, min_cos=0.1):
        from .texture import TextureAtlas
        if int(grid) != grid or not GRID_MIN <= int(grid) <= GRID_MAX:
            raise ValueError('DenseFitter: grid %r (an integer in %d..%d)' % (grid, GRID_MIN, GRID_MAX))
        self.grid = int(grid)
        KeypointFitter.__init__(self, smpl, stages, lr, sigma, w_pose, w_orient, w_shape, focal, res, kappa)
        self.w_dense, self.sigma_dense, self.min_cos = float(w_dense), float(sigma_dense), float(min_cos)
        self.tau = 1.0 / (4.0 * self.grid) if tau is None else float(tau)
        if not (self.sigma > 0 and self.sigma_dense > 0 and self.tau > 0 and self.w_dense >= 0):
            raise ValueError('DenseFitter: sigma, sigma_dense and tau must be positive, w_dense not negative')
        self.atlas = TextureAtlas(densepose, smpl_model, size=self.grid, focal_length=self.focal)

    def host_tables(self, device=None):
        """dense_tables' dict, built at the first call (the texel map is made on `device` and copied to the host, once)."""
        if self._host is None:
            if device is None:
                device = torch.device('cuda', torch.cuda.current_device())
            face, bary = self.atlas.texel_map(device)
            self._host = dense_tables(self.smpl, self.atlas.tables, face.cpu().numpy(), bary.cpu().numpy())
        return self._host

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

    def _table_shapes(self, t):
        Sp, M = int(t['Sp']), int(t['M'])
        return KeypointFitter._table_shapes(self, t) + (
            ('lm_corner', torch.int32, (M, 3)), ('lm_w', torch.float32, (M, 3)), ('csr_off', torch.int32, (Sp + 1,)),
            ('csr_lm', torch.int32, (3 * M,)), ('csr_w', torch.float32, (3 * M,)))

    def _own(self, P, tables, dev):
        M = int(tables['M'])
        return {'M': M}, {'gate': torch.empty(P, M, device=dev, dtype=torch.int32)}

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
        tables, p = self._rows(para)
        P, dev = p.shape[0], p.device
        if obs is None:
            img = _f32(iuv_image, (P, 3, None, None), 'DenseFitter.fit: iuv_image')
            if img.device != dev:
                raise ValueError('DenseFitter.fit: para and iuv_image must be on one device')
            ob = self.landmarks(img)
        else:
            ob = _f32(obs, (P, int(tables['M']), 3), 'DenseFitter.fit: obs')
        kp = torch.zeros(P, 49, 3, device=dev, dtype=torch.float32) if keypoints is None else _f32(keypoints, (P, 49, 3), 'DenseFitter.fit: keypoints')
        return self._fit(tables, p, kp, {'obs': ob}, stages, kappa, return_history, return_grad)
