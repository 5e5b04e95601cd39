"""Generates tests/golden/g27_pve.npz by IMPORTING the reference's utils.pose_utils.reconstruction_error (reduction=None) for the
Procrustes-aligned per-vertex error, beside the pelvis-centred mean vertex distance of the PVE rule in float64.  The
inputs are stored as float32 and cast up before either is evaluated, so the expected values belong to exactly the stored numbers.

Cases (B = 2, seeded): V = 6890 with meshes about 0.1 m apart; V = 257, 255, 256 (around one stride of the kernel's 256 lanes) and
V = 4; GT = the mirror image of the prediction (the det < 0 branch); GT = a known similarity transform of the prediction (scale 1.3, 70
degrees, a 5 m shift: PA-PVE ~ 0, PVE large); all vertices of the prediction coplanar (K of rank 2); GT identical to the prediction.
No collinear and no single-point sets: the reference divides by var1 = 0 there or LAPACK picks an arbitrary basis.
Re-run:  python tests/golden/make_golden_pve.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref_env, save   # noqa: E402


def pelvis_row(rng, V):
    """A stand-in for row 0 of J_regressor_h36m.npy: up to 32 non-negative weights that sum to 1."""
    n = min(32, V)
    w = np.zeros(V, np.float32)
    r = rng.random(n)
    w[rng.choice(V, n, replace=False)] = (r / r.sum()).astype(np.float32)
    return w


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def body(rng, B, V):
    """Points of a person-sized cloud around a root somewhere in the camera frame."""
    return rng.normal(0, 1, (B, V, 3)) * np.array([0.25, 0.5, 0.15]) + rng.normal(0, 0.3, (B, 1, 3))


def cases():
    rng = np.random.default_rng(27)
    out = {}
    for name, V in (('v6890', 6890), ('v257', 257), ('v255', 255), ('v256', 256), ('v4', 4)):
        p = body(rng, 2, V)
        out[name] = (p, p @ rotation(rng.normal(size=3), 8.0).T + rng.normal(0, 0.06, p.shape) + rng.normal(0, 0.05, (2, 1, 3)))
    p = body(rng, 2, 300)
    out['mirror'] = (p, p * np.array([-1.0, 1.0, 1.0]))
    p = body(rng, 2, 300)
    out['similarity'] = (p, 1.3 * p @ rotation([0.3, 1.0, -0.2], 70.0).T + np.array([3.0, -4.0, 0.0]))       # |shift| = 5 m
    p = body(rng, 2, 257)
    p[:, :, 2] = 0.0
    p = p @ rotation([1.0, 0.4, 0.2], 25.0).T                                                                   # a tilted plane
    out['coplanar'] = (p, p @ rotation([0.1, 1.0, 0.3], 40.0).T + rng.normal(0, 0.05, p.shape))
    p = body(rng, 2, 300)
    out['identical'] = (p, p.copy())
    return rng, out


def main():
    ref_env()
    from utils.pose_utils import reconstruction_error
    rng, cs = cases()
    arrs = {'cases': np.array(list(cs))}
    for name, (p, g) in cs.items():
        p32, g32 = p.astype(np.float32), g.astype(np.float32)
        w32 = pelvis_row(rng, p.shape[1])
        P, G, w = p32.astype(np.float64), g32.astype(np.float64), w32.astype(np.float64)
        pa = reconstruction_error(P, G, reduction=None)
        pel_p, pel_g = np.einsum('v,bvk->bk', w, P)[:, None], np.einsum('v,bvk->bk', w, G)[:, None]
        pve = np.sqrt((((P - pel_p) - (G - pel_g)) ** 2).sum(-1)).mean(-1)
        print('%-11s V %5d  pve %s  pa_pve %s' % (name, p.shape[1], pve, pa))
        arrs.update({name + '_pred': p32, name + '_gt': g32, name + '_pelvis_row': w32, name + '_pve': pve, name + '_pa_pve': pa})
    save('g27_pve', **arrs)


if __name__ == '__main__':
    main()
