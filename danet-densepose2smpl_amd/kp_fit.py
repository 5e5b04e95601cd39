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
from .ops import _f32, _per_device, _typed

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


def fill_args(a, pointers, sizes, stages, floats):
    """Every field a fit's argument struct (_lib.KpFitArgs, _lib.DenseFitArgs) holds, by name: `pointers` {field: device address or
    None}, `sizes` {field: int}, `stages` parse_stages' two lists, `floats` {field: float}; nstages and T come from the stages."""
    for k, v in pointers.items():
        setattr(a, k, v)
    for i, (n, m) in enumerate(zip(*stages)):
        a.stage_iters[i], a.stage_mask[i] = n, m
    for k, v in dict(sizes, nstages=len(stages[0]), T=sum(stages[0]), **floats).items():
        setattr(a, k, v)
    return a


class KeypointFitter(object):
    """KeypointFitter(smpl, stages=, lr=, sigma=, w_pose=, w_orient=, w_shape=, focal=, res=, kappa=None): `smpl` the SMPL layer (on the
    GPU when fit is called).  kappa None: 2 focal / res, the training convention; the scene demo passes 2 focal / 224.  The defaults
    are those of DESIGN.md, chosen on the synthetic recovery case.  dense_fit.DenseFitter is this class with its own tables, struct
    and entry point: what the two fits share is stated here."""
    ARGS, ENTRY = 'KpFitArgs', 'danet_kp_fit'
    F32_KEYS, I32_KEYS, HOST_KEYS = ('v_template', 'basis', 'basisT', 'weights', 'jx'), ('lm', 'jmap'), ('S', 'Sp', 'NB')
    FLOATS = ('focal', 'res', 'sigma', 'w_orient', 'w_pose', 'w_shape', 'lr')
    ONE_DEVICE = 'para, keypoints, the SMPL layer and the tables'

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

    def host_tables(self, device=None):
        """fit_tables' dict, built at the first call."""
        if self._host is None:
            self._host = fit_tables(self.smpl)
        return self._host

    def tables(self, device):
        """The sub-tables on `device` (fp32 / int32), built once and cached per device."""
        def make():
            h = self.host_tables(device)
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)          # noqa: E731
            t = {k: up(h[k], np.float32) for k in self.F32_KEYS}
            t.update({k: up(h[k], np.int32) for k in self.I32_KEYS})
            t.update({k: h[k] for k in self.HOST_KEYS})
            return t
        return _per_device(self._dev, device, make)

    def _table_shapes(self, t):
        """(key, dtype, shape) of every device table the kernel reads, in the order they are checked."""
        Sp, NB = int(t['Sp']), int(t['NB'])
        return (('v_template', torch.float32, (Sp * 3,)), ('basis', torch.float32, (207 + NB, Sp * 3)), ('basisT', torch.float32, (Sp * 3, NKP)),
                ('weights', torch.float32, (Sp, 24)), ('jx', torch.float32, (t['jx'].shape[0], Sp)), ('lm', torch.int32, (t['lm'].numel(),)),
                ('jmap', torch.int32, (49,)))

    def _rows(self, para):
        """-> (the tables on para's device, para as [P,229] f32, P >= 1)."""
        what = type(self).__name__ + '.fit'
        tables = self.tables(para.device)
        p = _f32(para, (None, 3 + int(tables['NB']) + 216), what + ': para')
        if p.shape[0] < 1:
            raise ValueError(what + ': an empty batch')
        return tables, p

    def _own(self, P, tables, dev):
        """-> (a subclass's own sizes {field: int}, its own output tensors {field: tensor}, which join the info dict)."""
        return {}, {}

    def _fit(self, tables, p, kp, own, stages, kappa, return_history, return_grad):
        """The fit of the rows p [P,229] to kp [P,49,3] (both fp32 on the GPU) and to `own`, a subclass's further inputs {field: tensor}
        (they join the info dict): the table checks, the one-device check, the outputs and the workspace, the struct, ONE launch."""
        what = type(self).__name__ + '.fit'
        P, dev, NB = p.shape[0], p.device, int(tables['NB'])
        held = {k: _typed(tables[k], dt, shape, '%s: %s' % (what, k)) for k, dt, shape in self._table_shapes(tables)}
        held['J_template'] = _typed(self.smpl.J_template, torch.float32, (24, 3), what + ': J_template')
        held['J_shapedirs'] = _typed(self.smpl.J_shapedirs, torch.float32, (72, NB), what + ': J_shapedirs')
        held['parents'] = _typed(self.smpl.parents, torch.int32, (24,), what + ': parents')
        if any(t.device != dev for t in [kp] + list(own.values()) + list(held.values())):
            raise ValueError('%s: %s must be on one device' % (what, self.ONE_DEVICE))
        parsed = parse_stages(self.stages if stages is None else stages)
        L = _lib.lib()
        out = {'para_fit': torch.empty_like(p), 'history': torch.empty(P, sum(parsed[0]) + 1, device=dev, dtype=torch.float32),
               'best_iter': torch.empty(P, device=dev, dtype=torch.int32), 'status': torch.empty(P, device=dev, dtype=torch.int32)}
        sizes, more = self._own(P, tables, dev)
        out.update(more)
        grad = torch.empty(P, 3 + NB + 144, device=dev, dtype=torch.float32) if return_grad else None
        nws = getattr(L, self.ENTRY + '_ws_floats')(P, int(tables['Sp']))
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        NL, NE = held['lm'].numel(), held['jx'].shape[0]
        tensors = dict(held, para=p, kp=kp, ws=ws, grad0=grad, jx=held['jx'] if NE else None, lm=held['lm'] if NL else None, **own, **out)
        floats = dict({k: getattr(self, k) for k in self.FLOATS}, kappa=float(self.kappa if kappa is None else kappa))
        a = fill_args(getattr(_lib, self.ARGS)(), {k: ptr(t) for k, t in tensors.items()},
                      dict(sizes, P=P, NB=NB, S=int(tables['S']), Sp=int(tables['Sp']), NL=NL, NE=NE), parsed, floats)
        check(getattr(L, self.ENTRY)(ctypes.addressof(a), nws, stream()), self.ENTRY)
        para_fit = out.pop('para_fit')
        if not (return_history or return_grad):
            return para_fit
        info = dict(out, **own)
        if return_grad:
            info['grad'] = grad
        return para_fit, info

    def fit(self, para, keypoints, return_history=False, return_grad=False, stages=None, kappa=None):
        """para [P,229], keypoints [P,49,3] on the GPU -> para_fit [P,229]; with return_history / return_grad also a dict with 'history'
        [P,T+1], 'best_iter' [P], 'status' [P] (and 'grad' [P,157], dE/dx at x_0).  No synchronisation, no allocation by data.  The arguments
        go through the rules of ops.py (_f32, _typed) and then to danet_kp_fit, one launch."""
        require_gpu(para, 'KeypointFitter.fit')
        require_gpu(keypoints, 'KeypointFitter.fit: keypoints')
        tables, p = self._rows(para)
        kp = _f32(keypoints, (p.shape[0], 49, 3), 'KeypointFitter.fit: keypoints')
        return self._fit(tables, p, kp, {}, stages, kappa, return_history, return_grad)
