"""Generates tests/golden/g25_eval.npz by IMPORTING the reference's utils.imutils.uncrop (like make_golden.py) with PIL plugged in
where scipy.misc.imresize was: modern scipy no longer has it, and it was a wrapper around PIL -- bytescale to uint8 unless the
array already is uint8, Image.resize((cols, rows), resample=NEAREST), back to an array.  The way g15 plugs restatements in for cv2
and pycocotools.

Cases: (centre, scale, orig_shape) triples whose paste rectangle lies inside the image, overhangs each of its four borders and
all four at once, a crop larger and one smaller than 224, non-square originals.  The rendered mask / part images are synthetic
(all 7 classes), the label images contain 255.  For every case the generator ASSERTS that this project's running-sum rule
(evaluate.uncrop_geometry) reproduces uncrop's output on every pixel, for the float mask and for the uint8 part image.
Re-run:  python tests/golden/make_golden_eval.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import ref_env, save   # noqa: E402
import eval_oracle as eo                 # noqa: E402

RES = 224
# (centre x, centre y, scale, rows, cols)
CASES = [
    (160.0, 120.0, 0.90, 240, 320),      # inside, crop 180 < 224
    (30.0, 120.0, 0.80, 240, 320),       # overhangs the left border
    (300.0, 110.0, 0.85, 240, 320),      # right
    (150.0, 25.0, 0.70, 240, 320),       # top
    (170.0, 230.0, 0.75, 240, 320),      # bottom
    (100.0, 130.0, 2.00, 260, 200),      # crop 400 > 224 and larger than the image: all four borders
    (90.5, 140.25, 0.60, 300, 150),      # crop 120 < 224, tall image
    (75.0, 150.0, 1.30, 300, 150),       # crop 260 > 224, tall image, left / right overhang
    (201.3, 77.7, 1.12, 160, 400),       # crop = 224, wide image
    (133.37, 99.91, 1.037, 201, 273),    # odd sizes, fractional everything
    (350.0, 40.0, 1.55, 180, 360),       # corner: top and right
]


def pil_imresize(arr, size, interp='bilinear', mode=None):
    """scipy.misc.imresize for 2-D arrays and a (rows, cols) size, on PIL."""
    from PIL import Image
    assert interp == 'nearest' and mode is None and arr.ndim == 2
    data = np.asarray(arr)
    if data.dtype != np.uint8:                                    # scipy.misc.bytescale with its defaults
        cmin, cmax = data.min(), data.max()
        cscale = cmax - cmin
        if cscale == 0:
            cscale = 1
        data = ((data - cmin) * (255.0 / cscale)).clip(0, 255) + 0.5
        data = data.astype(np.uint8)
    im = Image.fromarray(data, mode='L')
    return np.asarray(im.resize((int(size[1]), int(size[0])), resample=Image.NEAREST))


def rendered(rng):
    """A synthetic [224,224] part image with all 7 classes in fine structure (every row and column carries information), and
    its mask."""
    yy, xx = np.mgrid[0:RES, 0:RES]
    parts = ((xx * 3 + yy * 5 + (xx * yy) // 7) % 7).astype(np.uint8)
    blob = ((xx - rng.uniform(80, 140)) ** 2 / rng.uniform(50, 100) ** 2 + (yy - rng.uniform(80, 140)) ** 2 / rng.uniform(60, 110) ** 2) < 1
    parts = np.where(blob, np.maximum(parts, 1), 0).astype(np.uint8)
    parts[::17, ::13] = 0
    return (parts > 0).astype(np.float32), parts


def labels(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    p = ((xx // 9 + yy // 11) % 7).astype(np.uint8)
    p[((xx - W / 2) ** 2 / (W / 2.5) ** 2 + (yy - H / 2) ** 2 / (H / 2.2) ** 2) > 1] = 0
    p[(xx % 23 == 0) & (yy % 5 < 2)] = 255
    p[rng.integers(0, H, 40), rng.integers(0, W, 40)] = 255
    m = (((p > 0) & (p != 255)) | ((xx + yy) % 41 == 0)).astype(np.uint8) * 255
    return m, p


def main():
    import PIL
    ref_env()
    import scipy.misc
    scipy.misc.imresize = pil_imresize
    import utils.imutils as im
    from danet_densepose2smpl_amd import evaluate
    rng = np.random.default_rng(25)
    N = len(CASES)
    center = np.array([[c[0], c[1]] for c in CASES])
    scale = np.array([c[2] for c in CASES])
    shapes = np.array([[c[3], c[4]] for c in CASES], dtype=np.int64)
    mask = np.zeros((N, RES, RES), np.float32)
    parts = np.zeros((N, RES, RES), np.uint8)
    flat = {k: [] for k in ('un_mask', 'un_parts', 'gt_mask', 'gt_parts')}
    geo = evaluate.uncrop_geometry(center, scale, shapes, RES)
    rects = np.zeros((N, 4), np.int64)
    crop = np.zeros((N, 2), np.int64)
    for i in range(N):
        mask[i], parts[i] = rendered(rng)
        assert set(np.unique(parts[i])) == set(range(7))
        um = im.uncrop(mask[i], center[i], scale[i], shapes[i])
        up = im.uncrop(parts[i], center[i], scale[i], shapes[i])
        assert um.shape == tuple(shapes[i]) and um.dtype == np.uint8 and up.dtype == np.uint8
        ours_m = eo.uncrop_lookup(mask[i] > 0, geo[i], shapes[i])
        ours_p = eo.uncrop_lookup(parts[i], geo[i], shapes[i])
        bad = int(((um > 0) != ours_m).sum()) + int((up != ours_p).sum())
        assert bad == 0, 'case %d: the running-sum rule differs from uncrop on %d pixels' % (i, bad)
        assert geo[i][0] is not None
        rects[i] = geo[i][0]
        ul = np.array(im.transform([1, 1], center[i], scale[i], [RES, RES], invert=1)) - 1
        br = np.array(im.transform([RES + 1, RES + 1], center[i], scale[i], [RES, RES], invert=1)) - 1
        crop[i] = (br[1] - ul[1], br[0] - ul[0])
        gm, gp = labels(rng, *shapes[i])
        assert (gp == 255).any()
        for k, a in (('un_mask', um), ('un_parts', up), ('gt_mask', gm), ('gt_parts', gp)):
            flat[k].append(np.ascontiguousarray(a, dtype=np.uint8).reshape(-1))
    H, W = shapes[:, 0], shapes[:, 1]
    over = np.stack([rects[:, 2] == 0, rects[:, 3] == W, rects[:, 0] == 0, rects[:, 1] == H], 1) & \
        np.stack([(rects[:, 3] - rects[:, 2]) < crop[:, 1]] * 2 + [(rects[:, 1] - rects[:, 0]) < crop[:, 0]] * 2, 1)
    assert over.any(0).all(), 'a border is never overhung: %s' % over.any(0)
    assert (crop.max(1) > RES).any() and (crop.max(1) < RES).any() and (H != W).any()
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(H * W, out=offsets[1:])
    save('g25_eval', center=center, scale=scale, orig_shape=shapes, mask=mask.astype(np.uint8), parts=parts, offsets=offsets, rects=rects,
         crop_shape=crop, pil_version=np.array(PIL.__version__), **{k: np.concatenate(v) for k, v in flat.items()})


if __name__ == '__main__':
    main()
