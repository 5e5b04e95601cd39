"""The refresh rule's accept step (DESIGN.md 4d "the refresh rule") restated in numpy float64: rotation matrix -> axis-angle, the pose
augmentation and its undo, the row a fitted sample would store, and the decision over a batch (eligibility, the energy test, the betas
bound, finiteness, duplicates, the valid flag).  Nothing here imports the package."""
import types

import numpy as np

from kp_fit_oracle import make_para, rodrigues

SMPL_FLIP = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]


def rotmat_to_aa(R):
    """[...,3,3] float64 -> axis-angle [...,3] with the angle in [0, pi] (through the quaternion of the largest pivot)."""
    R = np.asarray(R, np.float64)
    out = np.zeros(R.shape[:-2] + (3,))
    for idx in np.ndindex(*R.shape[:-2]):
        m = R[idx]
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = 2 * np.sqrt(tr + 1)
            q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
            s = 2 * np.sqrt(1 + m[0, 0] - m[1, 1] - m[2, 2])
            q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
        elif m[1, 1] >= m[2, 2]:
            s = 2 * np.sqrt(1 + m[1, 1] - m[0, 0] - m[2, 2])
            q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
        else:
            s = 2 * np.sqrt(1 + m[2, 2] - m[0, 0] - m[1, 1])
            q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
        q = np.asarray(q)
        if q[0] < 0:
            q = -q
        sn = np.linalg.norm(q[1:])
        out[idx] = q[1:] * (2 / q[0] if sn < 1e-6 else 2 * np.arctan2(sn, q[0]) / sn)
    return out


def rotate_pose(pose, rot):
    """pose [72] axis-angle, rot in degrees: the global orientation turned by -rot about the camera axis (augment.rot_aa)."""
    pose = np.asarray(pose, np.float64).copy()
    rad = -float(rot) * np.pi / 180
    Rz = np.array([[np.cos(rad), -np.sin(rad), 0], [np.sin(rad), np.cos(rad), 0], [0, 0, 1]])
    pose[:3] = rotmat_to_aa(Rz @ rodrigues(pose[:3]))
    return pose


def flip_pose(pose, flip):
    pose = np.asarray(pose, np.float64)
    if not flip:
        return pose.copy()
    out = pose.reshape(24, 3)[SMPL_FLIP].copy()
    out[:, 1:] *= -1
    return out.reshape(72)


def forward(pose, rot, flip):
    """What a fetch applies: flip_pose(rotate_pose(pose, rot), flip)."""
    return flip_pose(rotate_pose(pose, rot), flip)


def inverse(pose, rot, flip):
    """What an update applies: rotate_pose(flip_pose(pose, flip), -rot)."""
    return rotate_pose(flip_pose(pose, flip), -float(rot))


def stored_row(para_row, rot, flip):
    """A fitted row [229] -> the 82 float64 values the table would take."""
    p = np.asarray(para_row, np.float64)
    aa = rotmat_to_aa(p[13:].reshape(24, 3, 3)).reshape(72)
    return np.concatenate([inverse(aa, rot, flip), p[3:13]])


def decide(para_fit, e_new, e_old, status_fit, status_eval, has_smpl, rows, rot_flip, kp, table, valid, tau):
    """-> (updated int32 [B], table', valid'): the accept rule over one batch.  para_fit [B,229], energies [B] (float32 values), rows [B],
    rot_flip [B,2], kp [B,49,3], table [N,82] float32, valid [N] uint8, tau a float32 value."""
    para_fit, kp = np.asarray(para_fit), np.asarray(kp, np.float64)
    e_new, e_old = np.asarray(e_new, np.float64), np.asarray(e_old, np.float64)
    B, N = para_fit.shape[0], table.shape[0]
    cand = np.zeros((B, 82), np.float32)
    accept = np.zeros(B, bool)
    with np.errstate(all='ignore'):
        for b in range(B):
            cand[b] = stored_row(para_fit[b], rot_flip[b][0], rot_flip[b][1] != 0).astype(np.float32)
            accept[b] = (has_smpl[b] == 0 and 0 <= rows[b] < N and status_fit[b] == 0 and status_eval[b] == 0 and np.isfinite(e_new[b])
                         and not (e_old[b] <= e_new[b]) and bool((np.abs(cand[b, 72:]) <= 3).all()) and bool(np.isfinite(cand[b]).all()))
    updated = np.zeros(B, np.int32)
    table, valid = np.array(table, np.float32), np.array(valid, np.uint8)
    for b in range(B):
        if not accept[b]:
            continue
        rivals = [c for c in range(B) if c != b and accept[c] and rows[c] == rows[b]]
        if any(e_new[c] < e_new[b] or (e_new[c] == e_new[b] and c < b) for c in rivals):
            continue
        updated[b] = 1
        table[rows[b]] = cand[b]
        valid[rows[b]] = 1 if e_new[b] < float(np.float32(tau)) * (kp[b, :, 2] ** 2).sum() else 0
    return updated, table, valid


# ---- shared cases ----------------------------------------------------------------------------------------------------------------
def decision_case(N=40, seed=3):
    """The hand-set batch of the decision test, shared with tests/test_gpu_fit_loop.py: one sample per listed case.  tau = 0.002 and
    confidences of 1 put the valid-flag bar at 0.098."""
    rng = np.random.default_rng(seed)
    names = ['accept', 'worse', 'equal', 'old_nan', 'new_nan', 'status_fit', 'status_eval', 'has_smpl', 'beta', 'dup_a', 'dup_b', 'dup_c',
             'other_row_valid', 'other_row_invalid']
    B = len(names)
    para = make_para(B, seed).astype(np.float32)
    e_new = np.full(B, 0.05, np.float32)
    e_old = np.full(B, 0.5, np.float32)
    status_fit, status_eval = np.zeros(B, np.int32), np.zeros(B, np.int32)
    has_smpl = np.zeros(B, np.float32)
    rows = np.array([3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 21, 21, 0, 39], np.int64)
    i = names.index
    e_new[i('worse')], e_old[i('worse')] = 0.6, 0.5
    e_new[i('equal')] = e_old[i('equal')] = 0.25
    e_old[i('old_nan')] = np.nan
    e_new[i('new_nan')] = np.nan
    status_fit[i('status_fit')] = 1
    status_eval[i('status_eval')] = 1
    has_smpl[i('has_smpl')] = 1
    para[i('beta'), 3 + 4] = 3.5
    e_new[i('dup_a')], e_new[i('dup_b')], e_new[i('dup_c')] = 0.3, 0.2, 0.2
    e_new[i('other_row_valid')], e_new[i('other_row_invalid')] = 0.0979, 0.0981
    rot_flip = np.stack([rng.choice([0.0, 37.5, -180.0, 12.0], B), rng.integers(0, 2, B).astype(np.float64)], 1)
    kp = rng.uniform(-1, 1, (B, 49, 3)).astype(np.float32)
    kp[:, :, 2] = 1.0
    table = rng.normal(0, 0.3, (N, 82)).astype(np.float32)
    valid = rng.integers(0, 2, N).astype(np.uint8)
    valid[[3, 0]], valid[[9, 39]] = 0, 1
    expect = {'accept': 1, 'worse': 0, 'equal': 0, 'old_nan': 1, 'new_nan': 0, 'status_fit': 0, 'status_eval': 0, 'has_smpl': 0, 'beta': 0,
              'dup_a': 0, 'dup_b': 1, 'dup_c': 0, 'other_row_valid': 1, 'other_row_invalid': 1}
    return types.SimpleNamespace(names=names, para=para, e_new=e_new, e_old=e_old, status_fit=status_fit, status_eval=status_eval,
                                 has_smpl=has_smpl, rows=rows, rot_flip=rot_flip, kp=kp, table=table, valid=valid, tau=np.float32(0.002),
                                 expect=np.array([expect[n] for n in names], np.int32))
