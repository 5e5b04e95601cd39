"""The track rule (DESIGN.md 4b'-track) restated in float64 numpy: association is tracks.associate itself (host code, tested by known
answers); here are the smoother, solved two ways, the para rows, the acceleration measure and the synthetic recovery case.

The smoothing system of one track is A x = b with A = diag(c + EPS) + lam_vel Dv'Dv + lam_acc Da'Da (Dv the first, Da the second
difference) and b = (c + EPS) y, y the input where c > 0 and the weighted mean elsewhere.  solve_dense builds A and calls
numpy.linalg.solve; solve_banded is the banded L D L^T of csrc/track_ops.hip, operation by operation.  Neither is the code under
test; their difference is the oracle's own error and enters the bounds of tests/test_gpu_tracks.py."""
import numpy as np

EPS = 1e-6
NB = 10
GROUPS = (slice(0, 3), slice(3, 13), slice(13, 157))           # cam, betas, rotations: the channels of each lam pair
DEFAULT_LAM = ((0.0, 3.0), (0.0, 10.0), (0.0, 10.0))          # tracks.DEFAULT_LAM, restated


def system(c, lam_vel, lam_acc):
    """The dense [T,T] matrix of one track."""
    T = len(c)
    A = np.diag(np.asarray(c, np.float64) + EPS)
    if T >= 2:
        Dv = np.zeros((T - 1, T))
        Dv[np.arange(T - 1), np.arange(T - 1)] = -1.0
        Dv[np.arange(T - 1), np.arange(1, T)] = 1.0
        A += lam_vel * Dv.T @ Dv
    if T >= 3:
        Da = np.zeros((T - 2, T))
        r = np.arange(T - 2)
        Da[r, r], Da[r, r + 1], Da[r, r + 2] = 1.0, -2.0, 1.0
        A += lam_acc * Da.T @ Da
    return A


def targets(y, c):
    """y [T,C], c [T] -> (the right-hand side's y with the weighted mean in the rows c = 0, sum c).  The sums run in ascending t;
    rows with c = 0 are never read."""
    y = np.asarray(y, np.float64)
    c = np.asarray(c, np.float64)
    sc, sy = 0.0, np.zeros(y.shape[1])
    for t in range(len(c)):
        if c[t] > 0:
            sc += c[t]
            sy = sy + c[t] * y[t]
    if sc == 0:
        return None, 0.0
    mean = sy / sc
    return np.where(c[:, None] > 0, y, mean[None]), sc


def solve_dense(y, c, lam_vel, lam_acc):
    """One track: y [T,C] -> x [T,C] float64 (y itself where sum c = 0)."""
    yy, sc = targets(y, c)
    if sc == 0:
        return np.asarray(y, np.float64).copy()
    w = np.asarray(c, np.float64) + EPS
    with np.errstate(invalid='ignore'):
        bad = ~np.isfinite(yy).all(0)
        x = np.linalg.solve(system(c, lam_vel, lam_acc), w[:, None] * np.where(bad[None], 0.0, yy))
    x[:, bad] = np.nan
    return x


def factor(c, lam_vel, lam_acc):
    """(l1, l2, D) [T] each: A = L D L', L unit lower triangular with sub-diagonals l1, l2.  The operations of track_factor_kernel."""
    T = len(c)
    lv, la = float(lam_vel), float(lam_acc)
    l1, l2, D = np.zeros(T), np.zeros(T), np.zeros(T)
    Dm1 = Dm2 = l1m1 = 0.0
    for t in range(T):
        w = float(c[t]) + EPS
        nv = (1.0 if t in (0, T - 1) else 2.0) if T >= 2 else 0.0
        na = (1.0 if t + 1 <= T - 2 else 0.0) + (4.0 if 1 <= t <= T - 2 else 0.0) + (1.0 if t - 1 >= 1 else 0.0)
        d = (w + lv * nv) + la * (na if T >= 3 else 0.0)
        L1 = L2 = 0.0
        if t >= 2:
            L2 = la / Dm2
        if t >= 1:
            u = t - 1
            ne = (1.0 if 1 <= u <= T - 2 else 0.0) + (1.0 if 1 <= u + 1 <= T - 2 else 0.0)
            e = -lv - 2.0 * la * ne
            L1 = (e - (L2 * Dm2) * l1m1) / Dm1
        Dt = (d - (L1 * L1) * Dm1) - (L2 * L2) * Dm2
        l1[t], l2[t], D[t] = L1, L2, Dt
        Dm2, Dm1, l1m1 = Dm1, Dt, L1
    return l1, l2, D


def solve_banded(y, c, lam_vel, lam_acc):
    """As solve_dense, by the banded factor: forward in ascending t, back substitution in descending t."""
    yy, sc = targets(y, c)
    if sc == 0:
        return np.asarray(y, np.float64).copy()
    T = len(c)
    l1, l2, D = factor(c, lam_vel, lam_acc)
    w = np.asarray(c, np.float64) + EPS
    z = np.zeros_like(yy)
    x = np.zeros_like(yy)
    with np.errstate(invalid='ignore'):
        for t in range(T):
            z[t] = (w[t] * yy[t] - l1[t] * (z[t - 1] if t >= 1 else 0.0)) - l2[t] * (z[t - 2] if t >= 2 else 0.0)
        for t in range(T - 1, -1, -1):
            x[t] = (z[t] / D[t] - (l1[t + 1] * x[t + 1] if t + 1 < T else 0.0)) - (l2[t + 2] * x[t + 2] if t + 2 < T else 0.0)
    return x


def smooth(values, conf, track_start, lam_vel, lam_acc, solver=solve_banded):
    """values [N,C] -> (x [N,C] float64, status [K])."""
    v = np.asarray(values, np.float64)
    out = np.empty_like(v)
    K = len(track_start) - 1
    status = np.zeros(K, np.int32)
    for k in range(K):
        s, e = int(track_start[k]), int(track_start[k + 1])
        c = np.asarray(conf[s:e], np.float64)
        status[k] = 0 if c.sum() > 0 else 1
        out[s:e] = solver(v[s:e], c, lam_vel, lam_acc)
    return out, status


def solver_gap(values, conf, track_start, lam_vel, lam_acc):
    """max |dense - banded| per track [K] (finite entries), the oracle's own error."""
    a, _ = smooth(values, conf, track_start, lam_vel, lam_acc, solve_dense)
    b, _ = smooth(values, conf, track_start, lam_vel, lam_acc, solve_banded)
    d = np.abs(a - b)
    d[~np.isfinite(d)] = 0.0
    return np.array([d[track_start[k]:track_start[k + 1]].max() if track_start[k + 1] > track_start[k] else 0.0 for k in range(len(track_start) - 1)])


# ---- para rows -------------------------------------------------------------------------------------------------------------------
def para_to_channels(para):
    """[N,229] -> [N,157]: cam, betas, and per joint the [3,2] row-major view of the matrix' first two columns."""
    p = np.asarray(para)
    R = p[:, 13:].reshape(-1, 24, 3, 3)
    return np.concatenate([p[:, :13], R[:, :, :, :2].reshape(-1, 144)], 1)


def rot6d(x6, dtype):
    """[M,6] ([3,2] row-major) -> [M,3,3] by Gram-Schmidt in `dtype`, the operations of csrc/rot6d.h."""
    x = np.asarray(x6, dtype).reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    tiny = dtype(1e-12)
    n1 = np.maximum(np.sqrt((a1[:, 0] * a1[:, 0] + a1[:, 1] * a1[:, 1]) + a1[:, 2] * a1[:, 2]), tiny)
    b1 = a1 / n1[:, None]
    d = (b1[:, 0] * a2[:, 0] + b1[:, 1] * a2[:, 1]) + b1[:, 2] * a2[:, 2]
    u = a2 - d[:, None] * b1
    n2 = np.maximum(np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]), tiny)
    b2 = u / n2[:, None]
    b3 = np.stack([b1[:, 1] * b2[:, 2] - b1[:, 2] * b2[:, 1], b1[:, 2] * b2[:, 0] - b1[:, 0] * b2[:, 2],
                   b1[:, 0] * b2[:, 1] - b1[:, 1] * b2[:, 0]], 1)
    return np.stack([b1, b2, b3], 2).astype(dtype)


def smooth_para(para, conf, track_start, lam=DEFAULT_LAM, shared_shape=True, solver=solve_banded):
    """para [N,229] -> dict: 'ch' [N,157] float64 the smoothed channels before rounding (s clamped, betas shared), 'para64' [N,229]
    with the 6D map in float64 on them, 'para32' the float32 variant: the channels rounded to fp32, then Gram-Schmidt in float32;
    'status' [K]; 'a1' / 'u' [N,24] the norms of the first column and of the orthogonalised second (the map's conditioning)."""
    para = np.asarray(para)
    ch_in = para_to_channels(para).astype(np.float64)
    N, K = para.shape[0], len(track_start) - 1
    ch = np.empty((N, 157))
    status = None
    for g, sl in enumerate(GROUPS):
        ch[:, sl], status = smooth(ch_in[:, sl], conf, track_start, lam[g][0], lam[g][1], solver)
    ch32 = ch.astype(np.float32)
    for k in range(K):
        s, e = int(track_start[k]), int(track_start[k + 1])
        if status[k]:
            continue
        c = np.asarray(conf[s:e], np.float64)
        obs = c > 0
        lo, hi = ch_in[s:e, 0][obs].min(), ch_in[s:e, 0][obs].max()
        ch[s:e, 0] = np.clip(ch[s:e, 0], lo, hi)
        ch32[s:e, 0] = np.clip(ch32[s:e, 0], np.float32(lo), np.float32(hi))
        if shared_shape:
            sc, sy = 0.0, np.zeros(10)
            for t in np.nonzero(obs)[0]:
                sc += c[t]
                sy = sy + c[t] * ch_in[s + t, 3:13]
            mean = sy / sc
            ch[s:e, 3:13] = mean[None]
            ch32[s:e, 3:13] = mean.astype(np.float32)[None]
    out64 = np.concatenate([ch[:, :13], rot6d(ch[:, 13:].reshape(-1, 6), np.float64).reshape(N, 216)], 1)
    out32 = np.concatenate([ch32[:, :13], rot6d(ch32[:, 13:].reshape(-1, 6), np.float32).reshape(N, 216)], 1).astype(np.float32)
    x = ch[:, 13:].reshape(N, 24, 3, 2)
    a1n = np.linalg.norm(x[..., 0], axis=-1)
    b1 = x[..., 0] / np.maximum(a1n, 1e-300)[..., None]
    un = np.linalg.norm(x[..., 1] - (b1 * x[..., 1]).sum(-1, keepdims=True) * b1, axis=-1)
    for k in range(K):
        if status[k]:
            s, e = int(track_start[k]), int(track_start[k + 1])
            out64[s:e], out32[s:e] = para[s:e], para[s:e]
            a1n[s:e], un[s:e] = 1.0, 1.0
    return {'ch': ch, 'para64': out64, 'para32': out32, 'status': status, 'a1': a1n, 'u': un}


# ---- acceleration ----------------------------------------------------------------------------------------------------------------
def accel(joints, track_start, joints_ref=None):
    """joints [N,J,3] -> (accel [K] float64, count [K])."""
    x = np.asarray(joints, np.float64)
    if joints_ref is not None:
        x = x - np.asarray(joints_ref, np.float64)
    K = len(track_start) - 1
    a, n = np.zeros(K), np.zeros(K, np.int32)
    for k in range(K):
        s, e = int(track_start[k]), int(track_start[k + 1])
        if e - s >= 3:
            d = np.linalg.norm((x[s + 2:e] - 2.0 * x[s + 1:e - 1]) + x[s:e - 2], axis=-1)
            a[k], n[k] = d.mean(), d.size
    return a, n


# ---- the recovery case -----------------------------------------------------------------------------------------------------------
def recovery_case(seed=0, lengths=(24, 40, 17), keys=3, pose_noise=0.06, cam_noise=0.02, shape_noise=0.3, drop=0.15):
    """Smooth ground-truth tracks and their noisy, partly dropped observation.

    Per track: rot6d key poses (identity columns plus N(0, 0.25)) interpolated linearly between `keys` key frames and renormalised by
    the 6D map; a camera (s, tx, ty) moving along a sine; one shape.  Observation: the 6D columns plus N(0, pose_noise), the camera
    plus N(0, cam_noise) (s: a fifth of it), the shape plus N(0, shape_noise), per frame; a fraction `drop` of the interior frames has
    conf 0 and NaN rows (they must never be read).  -> dict: 'track_start', 'conf' [N] f32, 'gt' [N,229] float64, 'obs' [N,229] f32, and
    'obs_full' [N,229] f32: the observation before the frames were dropped, the baseline the smoothed rows are compared with (it knows
    more than the smoother is shown)."""
    rng = np.random.default_rng(seed)
    ts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    N = int(ts[-1])
    gt, obs, conf = np.zeros((N, 229)), np.zeros((N, 229), np.float32), np.ones(N, np.float32)
    eye6 = np.array([1., 0., 0., 1., 0., 0.])
    for k, T in enumerate(lengths):
        s = int(ts[k])
        key = eye6[None, None] + rng.normal(0, 0.25, (keys, 24, 6))
        pos = np.linspace(0, keys - 1, T)
        i0 = np.minimum(pos.astype(int), keys - 2)
        f = (pos - i0)[:, None, None]
        x6 = (1 - f) * key[i0] + f * key[i0 + 1]
        R = rot6d(x6.reshape(-1, 6), np.float64).reshape(T, 24, 3, 3)
        tt = np.linspace(0, 1, T)
        ph = rng.uniform(0, 2 * np.pi, 3)
        cam = np.stack([0.9 + 0.1 * np.sin(2 * np.pi * tt + ph[0]), 0.2 * np.sin(2 * np.pi * tt + ph[1]), 0.15 * np.cos(2 * np.pi * tt + ph[2])], 1)
        betas = rng.normal(0, 1, 10)
        gt[s:s + T] = np.concatenate([cam, np.tile(betas, (T, 1)), R.reshape(T, 216)], 1)
        n6 = R[:, :, :, :2].reshape(T, 24, 6) + rng.normal(0, pose_noise, (T, 24, 6))
        ncam = cam + rng.normal(0, cam_noise, (T, 3)) * np.array([0.2, 1.0, 1.0])
        nb = betas[None] + rng.normal(0, shape_noise, (T, 10))
        obs[s:s + T] = np.concatenate([ncam, nb, rot6d(n6.reshape(-1, 6), np.float64).reshape(T, 216)], 1).astype(np.float32)
        gone = 1 + np.nonzero(rng.uniform(size=T - 2) < drop)[0]
        conf[s + gone] = 0.0
    full = obs.copy()
    obs[conf == 0] = np.nan
    return {'track_start': ts, 'conf': conf, 'gt': gt, 'obs': obs, 'obs_full': full}


def toy_joints(para):
    """A stand-in for the SMPL joints that needs no model: joint j of a row = R_j applied to a fixed offset, chained by a running sum
    along j, scaled by (1 + 0.05 betas_0), plus (tx, ty, 0).  [N,229] -> [N,24,3] float64; smooth in every unknown, which is all the
    recovery case asks of it."""
    p = np.asarray(para, np.float64)
    R = p[:, 13:].reshape(-1, 24, 3, 3)
    off = np.array([0.05, 0.1, 0.02])
    J = np.cumsum(R @ off, axis=1) * (1.0 + 0.05 * p[:, 3])[:, None, None]
    J[:, :, 0] += p[:, 1:2]
    J[:, :, 1] += p[:, 2:3]
    return J


def joint_error(para, gt, track_start):
    """Mean joint distance per track [K] between toy_joints of two row sets."""
    d = np.linalg.norm(toy_joints(para) - toy_joints(gt), axis=-1).mean(1)
    return np.array([d[track_start[k]:track_start[k + 1]].mean() for k in range(len(track_start) - 1)])


# ---- the cases of tests/test_gpu_tracks.py (tests/test_tracks_host.py checks the oracle's own error on every one of them) ---------
LAMS = ((0.0, 0.0), (1.0, 0.0), (0.0, 10.0), (0.5, 100.0))
CONF_KINDS = ('ones', 'ends', 'mid', 'single', 'zero')
LENGTHS = (1, 2, 3, 4, 5, 6, 257)
WIDTHS = (1, 63, 64, 65, 157)
FIVE = ((1, 'ones'), (2, 'ones'), (5, 'mid'), (64, 'zero'), (257, 'ends'))       # K = 5 tracks in one launch


def case_seed(C, i):
    return 100 * C + i


def make_conf(kind, T, rng):
    """Row weights of one track: all ones; zeros at both ends; a gap in the middle; a single observed row; all zero."""
    c = rng.uniform(0.2, 1.0, T).astype(np.float32)
    if kind == 'ones':
        c[:] = 1.0
    elif kind == 'ends':
        c[0] = c[-1] = 0.0
    elif kind == 'mid':
        c[T // 3:(2 * T) // 3] = 0.0
    elif kind == 'single':
        keep = c[T // 2]
        c[:] = 0.0
        c[T // 2] = keep
    elif kind == 'zero':
        c[:] = 0.0
    return c


def make_case(lengths, C, kind, seed, nan_gaps=True):
    """-> (values [N,C] f32, conf [N] f32, track_start).  Rows with conf 0 of a track that has an observed row hold NaN: they must
    never be read."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    N = int(start[-1])
    v = (rng.normal(0, 1, (N, C)) * rng.uniform(0.1, 3.0, C) + rng.normal(0, 2, C)).astype(np.float32)
    conf = np.concatenate([make_conf(kind, T, rng) for T in lengths])
    if nan_gaps:
        for k in range(len(lengths)):
            s, e = start[k], start[k + 1]
            if conf[s:e].sum() > 0:
                v[s:e][conf[s:e] == 0] = np.nan
    return v, conf, start


def para_case():
    """The recovery case plus three short tracks: T = 1, T = 2 and one of three rows without any weight.  -> (para [N,229] f32,
    conf [N] f32, track_start, the recovery case's dict)."""
    rc = recovery_case()
    extra = recovery_case(seed=9, lengths=(3, 4, 5))
    rows = extra['obs_full'][[0, 3, 4, 7, 8, 9]]
    conf = np.concatenate([rc['conf'], [0.7], [1.0, 0.4], [0.0, 0.0, 0.0]]).astype(np.float32)
    para = np.concatenate([rc['obs'], rows]).astype(np.float32)
    start = np.concatenate([rc['track_start'], rc['track_start'][-1] + np.array([1, 3, 6])]).astype(np.int32)
    return para, conf, start, rc
