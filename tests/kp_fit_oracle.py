"""The fit rule (DESIGN.md "fit rule") restated in torch on the CPU over the full, dense SMPL model dict: its own few-line LBS, the
energy, autograd for the gradient, the staged Adam loop and best-iterate selection.  `dtype` float64 is the reference; the same
code in float32 measures what single precision alone costs (the GPU tests bound the kernel by a multiple of that).  Also here: the
54 joints from kp_fit.fit_tables' sub-tables in numpy float64, and the shared test cases."""
import numpy as np
import torch

GROUPS = {'cam': 1, 'orient': 2, 'body': 4, 'shape': 8, 'all': 15}
JOINT_MAP_49 = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27]
DEFAULTS = dict(lr=0.02, sigma=0.1, w_pose=0.005, w_orient=0.005, w_shape=0.002, focal=5000., res=224., kappa=None)
DEFAULT_STAGES = ((30, 'cam+orient'), (70, 'all'))


def _mask(groups):
    names = groups.split('+') if isinstance(groups, str) else list(groups)
    m = 0
    for n in names:
        m |= GROUPS[n]
    return m


def model_tensors(model, dtype=torch.float64):
    V = np.asarray(model['v_template']).shape[0]
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)        # noqa: E731
    return {'V': V, 'v_template': t(model['v_template']).reshape(V * 3),
            'shapedirs': t(np.asarray(model['shapedirs']).reshape(V * 3, -1)), 'posedirs': t(model['posedirs']),
            'J_regressor': t(model['J_regressor']), 'lbs_weights': t(model['lbs_weights']),
            'J_regressor_extra': t(model['J_regressor_extra']), 'parents': [int(p) for p in np.asarray(model['parents'])],
            'landmark_verts': torch.as_tensor(np.asarray(model['landmark_verts'], np.int64))}


def as_tensors(model, dtype):
    """A model dict (numpy) or model_tensors' result of any dtype -> model_tensors' layout in `dtype`."""
    if 'V' not in model:
        return model_tensors(model, dtype)
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in model.items()}


def rot6d_to_rotmat(a):
    """a [...,3,2] -> R [...,3,3] (columns b1, b2, b1 x b2)."""
    a1, a2 = a[..., 0], a[..., 1]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -1)


def joints54(m, betas, R):
    """betas [P,NB], R [P,24,3,3] -> [P,54,3]: the posed joints, the landmark vertices, the regressed extra joints."""
    P, V = betas.shape[0], m['V']
    v_shaped = m['v_template'] + betas @ m['shapedirs'].T
    J = torch.einsum('jv,pvk->pjk', m['J_regressor'], v_shaped.view(P, V, 3))
    eye = torch.eye(3, dtype=betas.dtype)
    v_posed = (v_shaped + (R[:, 1:] - eye).reshape(P, 207) @ m['posedirs']).view(P, V, 3)
    Rg, Jp = [None] * 24, [None] * 24
    for i, pa in enumerate(m['parents']):
        if pa < 0:
            Rg[i], Jp[i] = R[:, i], J[:, i]
        else:
            Rg[i] = Rg[pa] @ R[:, i]
            Jp[i] = Jp[pa] + (Rg[pa] @ (J[:, i] - J[:, pa]).unsqueeze(-1)).squeeze(-1)
    Rg, Jp = torch.stack(Rg, 1), torch.stack(Jp, 1)
    tt = Jp - (Rg @ J.unsqueeze(-1)).squeeze(-1)
    T = torch.einsum('vj,pjrc->pvrc', m['lbs_weights'], Rg)
    verts = (T @ v_posed.unsqueeze(-1)).squeeze(-1) + torch.einsum('vj,pjr->pvr', m['lbs_weights'], tt)
    return torch.cat([Jp, verts[:, m['landmark_verts']], torch.einsum('ev,pvk->pek', m['J_regressor_extra'], verts)], 1)


def joints49(m, betas, R):
    return joints54(m, betas, R)[:, JOINT_MAP_49]


def project(j, cam, focal, res, kappa):
    """-> (uv [P,K,2], D [P,K])."""
    tz = 2.0 * focal / (res * cam[:, 0] + 1e-9)
    D = j[..., 2] + tz[:, None]
    uv = kappa * (j[..., :2] + cam[:, None, 1:3]) / D[..., None]
    return uv, D


def unpack(para):
    """para [P,229] -> x [P,157] = (cam, betas, the first two columns of every rotation, [3,2] row-major)."""
    P = para.shape[0]
    R = para[:, 13:].reshape(P, 24, 3, 3)
    return torch.cat([para[:, :13], R[..., :2].reshape(P, 144)], 1)


def energy(m, x, x0, R0, kp, c):
    """E [P] of x [P,157]; x0 the initial x and R0 = rot6d_to_rotmat(a(x0)) carry the priors."""
    P = x.shape[0]
    R = rot6d_to_rotmat(x[:, 13:].reshape(P, 24, 3, 2))
    j = joints49(m, x[:, 3:13], R)
    uv, D = project(j, x[:, :3], c['focal'], c['res'], c['kappa'])
    ok = ~(D <= 1e-6)                     # (a NaN depth is not skipped: the energy is NaN, status 1)
    e = uv - kp[..., :2]
    r2 = (e * e).sum(-1)
    s2 = c['sigma'] ** 2
    rho = s2 * r2 / (s2 + r2)
    data = torch.where(ok, kp[..., 2] ** 2 * rho, torch.zeros_like(rho)).sum(1)
    dR = ((R - R0) ** 2).sum((-1, -2))
    return data + c['w_orient'] * dR[:, 0] + c['w_pose'] * dR[:, 1:].sum(1) + c['w_shape'] * ((x[:, 3:13] - x0[:, 3:13]) ** 2).sum(1)


def fit(model, para, kp, stages=DEFAULT_STAGES, dtype=torch.float64, **kw):
    """-> dict of numpy arrays: para_fit [P,229], history [P,T+1], best_iter [P], status [P], grad [P,157] (dE/dx at x_0)."""
    c = dict(DEFAULTS)
    c.update(kw)
    if c['kappa'] is None:
        c['kappa'] = 2.0 * c['focal'] / c['res']
    m = as_tensors(model, dtype)
    para = torch.as_tensor(np.asarray(para)).to(dtype)
    kp = torch.as_tensor(np.asarray(kp)).to(dtype)
    P = para.shape[0]
    x0 = unpack(para)
    R0 = rot6d_to_rotmat(x0[:, 13:].reshape(P, 24, 3, 2))
    group = torch.tensor([1] * 3 + [8] * 10 + [2] * 6 + [4] * 138)
    x = x0.clone()
    T = sum(int(n) for n, _ in stages)
    history = torch.full((P, T + 1), float('nan'), dtype=dtype)
    best_iter = torch.zeros(P, dtype=torch.int64)
    bestE = torch.zeros(P, dtype=dtype)
    xbest = x0.clone()
    status = torch.zeros(P, dtype=torch.bool)
    grad0 = torch.zeros_like(x0)
    i = 0
    for n, groups in list(stages) + [(1, None)]:
        mom, var = torch.zeros_like(x), torch.zeros_like(x)
        for k in range(int(n)):
            xv = x.clone().requires_grad_(True)
            E = energy(m, xv, x0, R0, kp, c)
            Ed = E.detach()
            if i == 0:
                status = ~torch.isfinite(Ed)
                history[:, 0] = Ed
            else:
                history[~status, i] = Ed[~status]
            better = torch.isfinite(Ed) & ((Ed < bestE) if i else torch.ones(P, dtype=torch.bool)) & ~status
            bestE = torch.where(better, Ed, bestE)
            best_iter[better] = i
            xbest[better] = x[better]
            if groups is None and i > 0:
                break
            g = torch.autograd.grad(E.sum(), xv)[0]
            g = torch.where(status[:, None], torch.zeros_like(g), g)
            if i == 0:
                grad0 = g.clone()
            if groups is None:
                break
            on = ((group & _mask(groups)) != 0).to(dtype)[None]
            mom = torch.where(on > 0, 0.9 * mom + 0.1 * g, mom)
            var = torch.where(on > 0, 0.999 * var + 0.001 * g * g, var)
            mh, vh = mom / (1 - 0.9 ** (k + 1)), var / (1 - 0.999 ** (k + 1))
            step = torch.where(on > 0, c['lr'] * mh / (vh.sqrt() + 1e-8), torch.zeros_like(x))
            xn = x - step
            xn[:, 0] = torch.maximum(xn[:, 0], 0.1 * x0[:, 0])
            x = torch.where(status[:, None], x, xn)
            i += 1
    Rb = rot6d_to_rotmat(xbest[:, 13:].reshape(P, 24, 3, 2)).reshape(P, 216)
    fitted = torch.cat([xbest[:, :13], Rb], 1)
    keep = (status | (best_iter == 0))[:, None]
    para_fit = torch.where(keep, para, fitted)
    return {'para_fit': para_fit.numpy(), 'history': history.numpy(), 'best_iter': best_iter.numpy().astype(np.int32),
            'status': status.numpy().astype(np.int32), 'grad': grad0.numpy()}


# ---- the 54 joints from the support sub-tables (numpy float64) -------------------------------------------------------------------
def _chain(J, R, parents):
    P = R.shape[0]
    Rg, Jp = np.zeros((P, 24, 3, 3)), np.zeros((P, 24, 3))
    for i, pa in enumerate(parents):
        if pa < 0:
            Rg[:, i], Jp[:, i] = R[:, i], J[:, i]
        else:
            Rg[:, i] = Rg[:, pa] @ R[:, i]
            Jp[:, i] = Jp[:, pa] + np.einsum('prc,pc->pr', Rg[:, pa], J[:, i] - J[:, pa])
    return Rg, Jp


def joints54_from_tables(t, J_template, J_shapedirs, parents, betas, R):
    """What csrc/kp_fit.hip computes, from kp_fit.fit_tables' dict `t` and the layer's folded joint regression, in float64."""
    betas, R = np.asarray(betas, np.float64), np.asarray(R, np.float64)
    P, Sp = betas.shape[0], t['Sp']
    J = (np.asarray(J_template, np.float64).reshape(72) + betas @ np.asarray(J_shapedirs, np.float64).T).reshape(P, 24, 3)
    Rg, Jp = _chain(J, R, [int(p) for p in parents])
    f = np.concatenate([(R[:, 1:] - np.eye(3)).reshape(P, 207), betas], 1)
    v_posed = (t['v_template'][None] + f @ t['basis']).reshape(P, Sp, 3)
    tt = Jp - np.einsum('pjrc,pjc->pjr', Rg, J)
    T = np.einsum('vj,pjrc->pvrc', t['weights'], Rg)
    verts = np.einsum('pvrc,pvc->pvr', T, v_posed) + np.einsum('vj,pjr->pvr', t['weights'], tt)
    return np.concatenate([Jp, verts[:, t['lm']], np.einsum('ev,pvk->pek', t['jx'], verts)], 1)


# ---- shared cases ----------------------------------------------------------------------------------------------------------------
def rodrigues(pose):
    """axis-angle [P,24,3] float64 -> rotation matrices [P,24,3,3]."""
    pose = np.asarray(pose, np.float64)
    th = np.linalg.norm(pose, axis=-1, keepdims=True)
    k = pose / np.maximum(th, 1e-12)
    K = np.zeros(pose.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    th = th[..., None]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_para(P, seed, pose_sigma=0.2, s=None):
    """-> para [P,229] float32 (orthonormal to float32 rounding): betas ~ N(0,1) clipped, pose ~ N(0, pose_sigma^2), s in [0.6, 1.1]."""
    rng = np.random.default_rng(seed)
    betas = np.clip(rng.normal(0, 1, (P, 10)), -3, 3)
    R = rodrigues(rng.normal(0, pose_sigma, (P, 24, 3)))
    cam = np.stack([rng.uniform(0.6, 1.1, P) if s is None else np.broadcast_to(np.asarray(s, np.float64), (P,)),
                    rng.uniform(-0.1, 0.1, P), rng.uniform(-0.1, 0.1, P)], 1)
    return np.concatenate([cam, betas, R.reshape(P, 216)], 1).astype(np.float32)


def keypoints_of(model, para, conf=1.0, **kw):
    """The 49 joints of para projected by the rule's camera -> [P,49,3] float32 with confidence `conf`."""
    c = dict(DEFAULTS)
    c.update(kw)
    if c['kappa'] is None:
        c['kappa'] = 2.0 * c['focal'] / c['res']
    m = as_tensors(model, torch.float64)
    p = torch.as_tensor(np.asarray(para, np.float64))
    P = p.shape[0]
    j = joints49(m, p[:, 3:13], p[:, 13:].reshape(P, 24, 3, 3))
    uv, _ = project(j, p[:, :3], c['focal'], c['res'], c['kappa'])
    return np.concatenate([uv.numpy(), np.full((P, 49, 1), conf)], 2).astype(np.float32)


def perturb(para, seed, pose_sigma=0.15, shift=0.05, scale=1.1):
    """para with pose noise (a rotation of ~pose_sigma rad right-multiplied on every joint), a camera shift and a scale factor."""
    rng = np.random.default_rng(seed)
    p = np.asarray(para, np.float64).copy()
    P = p.shape[0]
    R = p[:, 13:].reshape(P, 24, 3, 3) @ rodrigues(rng.normal(0, pose_sigma, (P, 24, 3)))
    p[:, 13:] = R.reshape(P, 216)
    p[:, 0] *= scale
    p[:, 1:3] += shift * rng.choice([-1.0, 1.0], (P, 2))
    return p.astype(np.float32)


def edge_case(model, P, seed):
    """The energy / gradient case of the GPU tests: P people; keypoints from a perturbed copy of each row.
    Row 0: confidences in [0,1] with zeros among them, one keypoint far away (saturates rho).  Row 1 (P > 1): small s.
    Row 2 (P > 2): s so large that tz is ~0.1 and joints with Z < -tz fall behind the Z + tz guard."""
    rng = np.random.default_rng(seed + 100)
    para = make_para(P, seed).astype(np.float64)
    if P > 1:
        para[1, 0] = 0.05
    if P > 2:
        para[2, 0] = 2 * 5000. / (224. * 0.1)
    para = para.astype(np.float32)
    target = perturb(para, seed + 1, pose_sigma=0.1, shift=0.02, scale=1.0)
    kp = keypoints_of(model, target)
    kp[:, :, 2] = rng.uniform(0.0, 1.0, (P, 49))
    kp[:, rng.choice(49, 8, replace=False), 2] = 0.0
    kp[0, 3, 0] += 5.0
    kp[0, 3, 2] = 0.9
    if P > 2:           # (projections of joints near the camera plane are huge or not finite: keep the targets finite and moderate)
        kp[2, :, :2] = np.clip(np.nan_to_num(kp[2, :, :2], nan=0.0, posinf=3.0, neginf=-3.0), -3.0, 3.0)
    return para, kp


def recovery_case(model):
    """The synthetic recovery case: keypoints (confidence 1) made from para* through the SMPL layer and the projection; the start is
    para* with pose noise of 0.15 rad on every joint, a camera shift of 0.05 and a scale factor of 1.1.  -> (init, kp, para*)."""
    star = make_para(2, 7)
    return perturb(star, 8), keypoints_of(model, star), star


def spread_model(model, seed=5, per_joint=230):
    """The model dict with J_regressor_extra rows spread over about 2000 vertices (9 rows of `per_joint` random vertices each)."""
    rng = np.random.default_rng(seed)
    V = np.asarray(model['v_template']).shape[0]
    out = dict(model)
    jx = np.zeros((9, V))
    for e in range(9):
        idx = rng.choice(V, per_joint, replace=False)
        w = rng.uniform(0.2, 1.0, per_joint)
        jx[e, idx] = w / w.sum()
    out['J_regressor_extra'] = jx.astype(np.float32)
    return out


def model_from_layer(smpl):
    """The model dict of an SMPL layer's own (float32) buffers: what the kernel's tables were cut from."""
    g = lambda n: getattr(smpl, n).detach().cpu().numpy()           # noqa: E731
    V = g('v_template').shape[0]
    return {'v_template': g('v_template'), 'shapedirs': g('shapedirs').reshape(V, 3, -1), 'posedirs': g('posedirs'), 'J_regressor': g('J_regressor'),
            'lbs_weights': g('lbs_weights'), 'parents': g('parents'), 'J_regressor_extra': g('J_regressor_extra'),
            'landmark_verts': g('landmark_verts'), 'faces': smpl.faces}
