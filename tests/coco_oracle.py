"""A plain numpy restatement of the COCO keypoint rule, per-image Python loops in float64.  Test infrastructure:
written from the rule, not from the package's code, and never imported by it.

  oks(d, g, area, bbox)                      one object keypoint similarity
  match_image(...)                           the greedy matching of one image for the three area ranges -> flag words, counts
  match_dataset(...)                         the same over packed arrays (the layout ops.coco_oks_match takes)
  accumulate(dt_match, dt_ignore, gt_count)  precision [10,101,3], recall [10,3], the ten numbers
  evaluate_json(preds, imgnames, coco)       everything from predictions in sample order + the annotation dict
"""
import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
VARS = (SIGMAS * 2) ** 2
THRS = np.linspace(.5, 0.95, 10)
RECS = np.linspace(.0, 1.00, 101)
RANGES = [(0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
MAX_DETS = 20
EPS = 2.220446049250313e-16
NAMES = ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']


def oks(d, g, area, bbox):
    """d [17,2] detection, g [17,3] ground truth (x, y, v), its area and bbox (x, y, w, h)."""
    d, g = np.asarray(d, np.float64), np.asarray(g, np.float64)
    vis = g[:, 2] > 0
    k1 = int(vis.sum())
    total, count = 0.0, 0
    for j in range(17):
        if k1 > 0:
            if not vis[j]:
                continue
            dx, dy = d[j, 0] - g[j, 0], d[j, 1] - g[j, 1]
        else:
            x0, x1 = bbox[0] - bbox[2], bbox[0] + bbox[2] * 2
            y0, y1 = bbox[1] - bbox[3], bbox[1] + bbox[3] * 2
            dx = max(0.0, x0 - d[j, 0]) + max(0.0, d[j, 0] - x1)
            dy = max(0.0, y0 - d[j, 1]) + max(0.0, d[j, 1] - y1)
        e = (dx ** 2 + dy ** 2) / VARS[j] / (float(area) + EPS) / 2
        total += np.exp(-e)
        count += 1
    return total / count


def oks_matrix(dts, gts, areas, bboxes):
    D, G = min(len(dts), MAX_DETS), len(gts)
    m = np.zeros((D, G))
    for i in range(D):
        for k in range(G):
            m[i, k] = oks(dts[i], gts[k], areas[k], bboxes[k])
    return m


def match_image(dts, dt_area, gts, gt_area, gt_bbox, gt_ignore, gt_iscrowd):
    """-> dt_match [D,3], dt_ignore [D,3] (bit t = threshold t; a detection past the first 20: 0 and 0x3ff), gt_count [3]."""
    D, G = len(dts), len(gts)
    keep = min(D, MAX_DETS)
    m = oks_matrix(dts, gts, gt_area, gt_bbox)
    dt_match, dt_ign = np.zeros((D, 3), np.int64), np.zeros((D, 3), np.int64)
    dt_ign[keep:] = (1 << 10) - 1
    counts = np.zeros(3, np.int64)
    for a, (lo, hi) in enumerate(RANGES):
        ig = [bool(gt_ignore[k]) or gt_area[k] < lo or gt_area[k] > hi for k in range(G)]
        order = [k for k in range(G) if not ig[k]] + [k for k in range(G) if ig[k]]
        counts[a] = sum(1 for k in range(G) if not ig[k])
        for t, thr in enumerate(THRS):
            taken = [False] * G
            for i in range(keep):
                best, hit = min(thr, 1 - 1e-10), None
                for k in order:
                    if taken[k] and not gt_iscrowd[k]:
                        continue
                    if hit is not None and not ig[hit] and ig[k]:
                        break
                    if m[i, k] < best:
                        continue
                    best, hit = m[i, k], k
                if hit is None:
                    if dt_area[i] < lo or dt_area[i] > hi:
                        dt_ign[i, a] |= 1 << t
                    continue
                taken[hit] = True
                dt_match[i, a] |= 1 << t
                if ig[hit]:
                    dt_ign[i, a] |= 1 << t
    return dt_match, dt_ign, counts


def match_dataset(dt_kpts, dt_area, dt_offsets, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd, gt_offsets):
    I = len(dt_offsets) - 1
    dm, di, gc = np.zeros((len(dt_kpts), 3), np.int64), np.zeros((len(dt_kpts), 3), np.int64), np.zeros((I, 3), np.int64)
    for i in range(I):
        d0, d1, g0, g1 = dt_offsets[i], dt_offsets[i + 1], gt_offsets[i], gt_offsets[i + 1]
        dm[d0:d1], di[d0:d1], gc[i] = match_image(dt_kpts[d0:d1], dt_area[d0:d1], gt_kpts[g0:g1], gt_area[g0:g1], gt_bbox[g0:g1],
                                                  gt_ignore[g0:g1], gt_iscrowd[g0:g1])
    return dm, di, gc


def nearest_threshold_gap(dt_kpts, dt_offsets, gt_kpts, gt_area, gt_bbox, gt_offsets):
    """The smallest |OKS - threshold| over every pair the matching looks at."""
    gap = np.inf
    for i in range(len(dt_offsets) - 1):
        d0, d1, g0, g1 = dt_offsets[i], dt_offsets[i + 1], gt_offsets[i], gt_offsets[i + 1]
        m = oks_matrix(dt_kpts[d0:d1], gt_kpts[g0:g1], gt_area[g0:g1], gt_bbox[g0:g1])
        if m.size:
            gap = min(gap, float(np.abs(m[:, :, None] - THRS[None, None, :]).min()))
    return gap


def accumulate(dt_match, dt_ignore, gt_count):
    """Detections in evaluation order with equal scores (the stable sort keeps the order)."""
    N = len(dt_match)
    precision, recall = -np.ones((10, 101, 3)), -np.ones((10, 3))
    for a in range(3):
        npig = int(np.sum(gt_count[:, a])) if len(gt_count) else 0
        if npig == 0:
            continue
        for t in range(10):
            tp, fp, tps, fps = 0, 0, [], []
            for i in range(N):
                if not (dt_ignore[i][a] >> t) & 1:
                    if (dt_match[i][a] >> t) & 1:
                        tp += 1
                    else:
                        fp += 1
                tps.append(tp)
                fps.append(fp)
            rc = [x / npig for x in tps]
            pr = [x / (y + x + EPS) for x, y in zip(tps, fps)]
            recall[t, a] = rc[-1] if N else 0
            for i in range(N - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            for r, rec in enumerate(RECS):
                k = 0
                while k < N and rc[k] < rec:
                    k += 1
                precision[t, r, a] = pr[k] if k < N else 0.0
    mean = lambda x: float(np.mean(x[x > -1])) if (x > -1).any() else -1.0
    stats = [mean(precision[:, :, 0]), mean(precision[0, :, 0]), mean(precision[5, :, 0]), mean(precision[:, :, 1]), mean(precision[:, :, 2]),
             mean(recall[:, 0]), mean(recall[0:1, 0]), mean(recall[5:6, 0]), mean(recall[:, 1]), mean(recall[:, 2])]
    return precision, recall, np.array(stats)


def pack_json(coco):
    """The annotation dict -> (image ids ascending, per-image lists of the category-1 annotations in file order)."""
    ids = sorted(set(int(im['id']) for im in coco['images']))
    per = {i: [] for i in ids}
    for a in coco['annotations']:
        if a['category_id'] == 1:
            per[int(a['image_id'])].append(a)
    return ids, per


def evaluate_json(preds, imgnames, coco):
    """preds [n,17,2] and imgnames in SAMPLE order -> the ten numbers (and the flags, for inspection)."""
    preds = np.asarray(preds, np.float64)
    ids, per = pack_json(coco)
    sample_img = [int(str(n)[-16:-4]) for n in imgnames]
    dm, di, gc = [], [], []
    for i in ids:
        mine = [k for k in range(len(sample_img)) if sample_img[k] == i]                 # the order of the samples
        d = preds[np.array(mine, dtype=np.int64)].reshape(-1, 17, 2)
        da = [(p[:, 0].max() - p[:, 0].min()) * (p[:, 1].max() - p[:, 1].min()) for p in d]
        anns = per[i]
        g = np.array([a['keypoints'] for a in anns], np.float64).reshape(-1, 17, 3)
        ign = [bool(a['iscrowd']) or a['num_keypoints'] == 0 for a in anns]
        m, ig, c = match_image(d, da, g, [a['area'] for a in anns], [a['bbox'] for a in anns], ign, [bool(a['iscrowd']) for a in anns])
        dm.append(m); di.append(ig); gc.append(c)
    dm, di = np.concatenate(dm) if dm else np.zeros((0, 3), np.int64), np.concatenate(di) if di else np.zeros((0, 3), np.int64)
    precision, recall, stats = accumulate(dm, di, np.array(gc).reshape(-1, 3))
    return stats, dm, di, np.array(gc).reshape(-1, 3)
