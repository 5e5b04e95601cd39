"""Generates tests/golden/g26_coco.npz by IMPORTING the reference (only possible where the reference checkout exists): lines 114-145
of its eval_coco.py -- J24_TO_JCOCO, the weak-perspective camera as a translation, utils.geometry.perspective_projection,
+ img_res / 2, utils.transforms.transform_preds -- on 8 seeded samples.  The file holds inputs and expected outputs only.

cv2 is absent; the one function the chain needs, getAffineTransform, is plugged in as an exact three-point solve in double (the
restatement approach of g15 / g25).  Two runs: the chain as the reference runs it (float32 tensors, float32 corner points, a float32
result array) and the same chain in float64 throughout.  `preds` is the float64 run; `floor_px` is the largest distance of the
float32 run from it, in pixels: the reference chain's own rounding floor.

Re-run:  python tests/golden/make_golden_coco.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden    # noqa: E402

IMG_RES = 224


def _cv2_stub():
    cv2 = types.ModuleType('cv2')

    def getAffineTransform(src, dst):
        src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
        A = np.concatenate([src, np.ones((3, 1))], axis=1)
        return np.linalg.solve(A, dst).T                                     # [2,3]: dst = M (x, y, 1)
    cv2.getAffineTransform = getAffineTransform
    return cv2


class _Numpy64(object):
    """numpy with float32 spelled float64: lets get_affine_transform build its corner points in double."""
    float32 = np.float64

    def __getattr__(self, k):
        return getattr(np, k)


def back_project(joints, camera, center, scale, dtype, tables, project, transforms):
    """The COCO keypoint back-projection for a batch, with the reference's own two functions doing the arithmetic:
    `project` = utils.geometry.perspective_projection, `transforms.transform_preds` the inverse crop affine.  dtype torch.float32
    runs them as the reference does; torch.float64 runs every step in double."""
    double = dtype == torch.float64
    B = joints.shape[0]
    j49, cam = torch.as_tensor(joints, dtype=dtype), torch.as_tensor(camera, dtype=dtype)
    pick = [49 - 24 + k for k in tables.J24_TO_JCOCO]                           # the COCO joints among the last 24
    s, tx, ty = cam.unbind(dim=1)
    t = torch.stack((tx, ty, 2 * tables.FOCAL_LENGTH / (IMG_RES * s + 1e-9)), dim=1)
    identity = torch.eye(3, dtype=dtype).repeat(B, 1, 1)
    torch.set_default_dtype(dtype)                                             # (the projection allocates its intrinsics in the default dtype)
    try:
        crop_px = project(j49[:, pick], identity, t, tables.FOCAL_LENGTH, torch.zeros(B, 2, dtype=dtype)) + IMG_RES / 2.
    finally:
        torch.set_default_dtype(torch.float32)
    crop_px = crop_px.numpy()
    out = np.empty_like(crop_px)                                               # (float32 in the reference's run: its result array is)
    numpy_of_transforms = transforms.np
    if double:
        transforms.np = _Numpy64()
    try:
        for b in range(B):
            out[b] = transforms.transform_preds(crop_px[b], center[b], np.array([scale[b], scale[b]]), [IMG_RES, IMG_RES])
    finally:
        transforms.np = numpy_of_transforms
    return out


def g26_coco():
    sys.modules['cv2'] = _cv2_stub()
    make_golden.ref_env()
    import constants
    from utils.geometry import perspective_projection
    from utils import transforms
    rng = np.random.default_rng(26)
    B = 8
    joints = (rng.normal(0, 0.35, (B, 49, 3)) * np.array([1.0, 1.6, 0.4])).astype(np.float32)
    camera = np.stack([rng.uniform(0.5, 1.3, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B)], axis=1).astype(np.float32)
    scale = np.array([0.4, 0.55, 0.8, 1.0, 1.37, 1.9, 2.5, 3.0], np.float32)
    # crop centres near the borders of a 640 x 480 image (and one outside it)
    center = np.array([[3.5, 2.25], [636.0, 5.0], [10.0, 470.5], [630.25, 476.0], [320.0, 0.5], [0.0, 240.0], [655.0, 250.0], [321.7, 239.4]], np.float32)
    args = (constants, perspective_projection, transforms)
    p32 = back_project(joints, camera, center, scale, torch.float32, *args)
    p64 = back_project(joints, camera, center.astype(np.float64), scale.astype(np.float64), torch.float64, *args)
    assert p32.dtype == np.float32 and p64.dtype == np.float64 and p64.shape == (B, 17, 2)
    floor = float(np.abs(p32.astype(np.float64) - p64).max())
    print('floor_px', floor, 'range', p64.min(), p64.max())
    make_golden.save('g26_coco', joints=joints, camera=camera, center=center, scale=scale, img_res=np.int64(IMG_RES),
                     focal_length=np.float64(constants.FOCAL_LENGTH), preds=p64, preds_f32=p32, floor_px=np.float64(floor))


if __name__ == '__main__':
    g26_coco()
