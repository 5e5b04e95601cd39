"""numpy oracles of the evaluation pipeline, in this project's own words.

  seg_counts / score_batch   the counting of the reference's eval.py:228-266 on images at the original resolution
  uncrop_lookup              the uncropped image from a paste rectangle and two index tables (DESIGN.md "uncrop rule")
  rotmat_to_angle_axis       DESIGN.md "axis-angle rule" in a chosen precision;  rodrigues: its inverse in fp64
"""
import numpy as np

SEG = {'tp': 0, 'fp': 2, 'fn': 4, 'accuracy': 6, 'pixel_count': 7, 'parts_tp': 8, 'parts_fp': 15, 'parts_fn': 22,
       'parts_accuracy': 29, 'parts_pixel_count': 30}
SEG_COUNTERS = 32


def seg_counts(pred_mask, gt_mask, pred_parts, gt_parts):
    """One sample at the original resolution: pred_mask / gt_mask boolean, pred_parts / gt_parts uint8 -> int64 [32]."""
    c = np.zeros(SEG_COUNTERS, dtype=np.int64)
    if gt_mask is not None:
        c[SEG['accuracy']] = (gt_mask == pred_mask).sum()
        c[SEG['pixel_count']] = gt_mask.size
        for k in range(2):
            g, p = gt_mask == k, pred_mask == k
            c[SEG['tp'] + k] = (g & p).sum()
            c[SEG['fp'] + k] = (~g & p).sum()
            c[SEG['fn'] + k] = (g & ~p).sum()
    if gt_parts is not None:
        ignore = gt_parts == 255
        for k in range(7):
            g = gt_parts == k
            p = (pred_parts == k) & ~ignore                   # a pixel labelled 255 never counts as predicted
            c[SEG['parts_tp'] + k] = (g & p).sum()
            c[SEG['parts_fp'] + k] = (~g & p).sum()
            c[SEG['parts_fn'] + k] = (g & ~p).sum()
        g0, p0 = np.where(ignore, 0, gt_parts), np.where(pred_parts == 255, 0, pred_parts)
        c[SEG['parts_accuracy']] = (g0 == p0).sum()
        c[SEG['parts_pixel_count']] = gt_parts.size
    return c


def uncrop_lookup(img, geometry, orig_shape):
    """img [R,R] -> uint8-free copy at orig_shape: zeros, and inside the paste rectangle img[rows][:, cols]."""
    out = np.zeros(tuple(int(s) for s in orig_shape), dtype=img.dtype)
    rect, rows, cols = geometry
    if rect is not None:
        y0, y1, x0, x1 = rect
        out[y0:y1, x0:x1] = img[np.asarray(rows)][:, np.asarray(cols)]
    return out


def score_batch(mask, parts, gt_masks, gt_parts, center, scale, uncrop_geometry):
    """mask [B,R,R] float, parts [B,R,R] int (what PartRenderer returns, on the host), label images as lists -> int64 [32]; the
    per-sample host loop of eval.py:228-266 with `uncrop_geometry` (evaluate.uncrop_geometry) in the place of imutils.uncrop."""
    B = mask.shape[0]
    shapes = [(gt_masks if gt_masks is not None else gt_parts)[b].shape for b in range(B)]
    geo = uncrop_geometry(center, scale, np.asarray(shapes), mask.shape[-1])
    total = np.zeros(SEG_COUNTERS, dtype=np.int64)
    for b in range(B):
        pm = uncrop_lookup(np.asarray(mask[b]) > 0, geo[b], shapes[b])
        pp = uncrop_lookup(np.asarray(parts[b]).astype(np.uint8), geo[b], shapes[b])
        total += seg_counts(pm, None if gt_masks is None else np.asarray(gt_masks[b]) > 0, pp, None if gt_parts is None else np.asarray(gt_parts[b]))
    return total


def rotmat_to_angle_axis(R, dtype=np.float64):
    """[N,3,3] -> [N,3] by DESIGN.md's axis-angle rule, every operation in `dtype`."""
    R = np.asarray(R, dtype=dtype).reshape(-1, 3, 3)
    out = np.zeros((R.shape[0], 3), dtype=dtype)
    one, two, quarter = dtype(1), dtype(2), dtype(0.25)
    for i, m in enumerate(R):
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = two * np.sqrt(tr + one)
            q = [quarter * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
            s = two * np.sqrt(one + m[0, 0] - m[1, 1] - m[2, 2])
            q = [(m[2, 1] - m[1, 2]) / s, quarter * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
        elif m[1, 1] >= m[2, 2]:
            s = two * np.sqrt(one + m[1, 1] - m[0, 0] - m[2, 2])
            q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, quarter * s, (m[1, 2] + m[2, 1]) / s]
        else:
            s = two * np.sqrt(one + m[2, 2] - m[0, 0] - m[1, 1])
            q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, quarter * s]
        w, x, y, z = (dtype(v) for v in q)
        if w < 0:
            w, x, y, z = -w, -x, -y, -z
        sn = np.sqrt(x * x + y * y + z * z)
        k = two / w if sn < dtype(1e-6) else two * np.arctan2(sn, w) / sn
        out[i] = (x * k, y * k, z * k)
    return out


def rodrigues(aa):
    """[N,3] axis-angle -> [N,3,3] in fp64 (R = I + sin K + (1 - cos) K K)."""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((aa.shape[0], 3, 3))
    for i, v in enumerate(aa):
        th = np.linalg.norm(v)
        if th < 1e-300:
            out[i] = np.eye(3)
            continue
        k = v / th
        K = np.array([[0., -k[2], k[1]], [k[2], 0., -k[0]], [-k[1], k[0], 0.]])
        out[i] = np.eye(3) + np.sin(th) * K + (1. - np.cos(th)) * (K @ K)
    return out
