"""The identity rule (DESIGN.md 4b'-link) restated in float64 numpy, written from the section and not from the kernel: the shape
descriptor and the views of the skin descriptor, the pair distance, the linking and the one shape per identity -- and the synthetic
recovery case on which the defaults were chosen.  The skin descriptor's atlas itself is the texture rule's (DESIGN.md 4b''), which has
its own oracle; here it is an input."""
import numpy as np

import track_oracle as to

W_MIN = 1e-3
PARTS = 24
DEFAULTS = {'max_absence': 150, 'sigma_s': 0.3, 'sigma_a': 0.15, 'min_overlap': 0.1, 'no_app': 0.5}     # tracks.LINK_DEFAULTS, restated


# ---- descriptors -------------------------------------------------------------------------------------------------------------------
def weighted_mean(x, c):
    """sum c x / sum c over the rows in the order given, rows with c = 0 never read; (None, 0) where sum c = 0."""
    sc, sy = 0.0, np.zeros(np.asarray(x).shape[1])
    for t in range(len(c)):
        if c[t] > 0:
            sc += float(c[t])
            sy = sy + float(c[t]) * np.asarray(x[t], np.float64)
    return (sy / sc if sc > 0 else None), sc


def shape_descriptors(para, conf, track_start):
    """para [N,229], conf [N] -> (shape [K,10] float64 (zeros where a track has no weight), status [K])."""
    K = len(track_start) - 1
    out, status = np.zeros((K, 10)), np.zeros(K, np.int32)
    for k in range(K):
        s, e = int(track_start[k]), int(track_start[k + 1])
        m, sc = weighted_mean(np.asarray(para)[s:e, 3:13], conf[s:e])
        if sc > 0:
            out[k] = m
        else:
            status[k] = 1
    return out, status


def observed_views(det, track_start):
    """The rows the skin descriptor draws: (rows: the observed rows, track-major and ascending in t; view_offsets [K+1])."""
    det = np.asarray(det)
    rows = np.nonzero(det >= 0)[0]
    counts = [int((det[track_start[k]:track_start[k + 1]] >= 0).sum()) for k in range(len(track_start) - 1)]
    return rows.astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ---- the pair distance ---------------------------------------------------------------------------------------------------------------
def pair_distance(shape, atlas, pairs):
    """shape [K,10], atlas [K,24,T,T,4], pairs [C,2] -> [C,4] float64 = (d_shape, d_app, overlap, S), not rounded."""
    shape = np.asarray(shape, np.float64)
    atlas = np.asarray(atlas)
    out = np.zeros((len(pairs), 4))
    for c, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        d = shape[a] - shape[b]
        out[c, 0] = float((d * d).sum()) / 10.0
        ta = atlas[a].reshape(-1, 4).astype(np.float64)
        tb = atlas[b].reshape(-1, 4).astype(np.float64)
        wa, wb = ta[:, 3], tb[:, 3]
        with np.errstate(invalid='ignore'):
            ia, ib = wa > W_MIN, wb > W_MIN
        both = ia & ib
        m = np.minimum(1.0, wa[both]) * np.minimum(1.0, wb[both])
        S, n, u = float(m.sum()), int(both.sum()), int((ia | ib).sum())
        if n > 0:
            diff = ta[both, :3] - tb[both, :3]                              # (the colours of the other texels are never read)
            out[c, 1] = float((m * (diff * diff).sum(1)).sum()) / (3.0 * S)
        out[c, 2] = n / u if u > 0 else 0.0
        out[c, 3] = S
    return out


def near_w_min(atlas, rel=1e-6):
    """Whether any texel weight lies within `rel` relative of w_min (such a pair is outside every comparison)."""
    w = np.asarray(atlas, np.float64)[..., 3]
    with np.errstate(invalid='ignore'):
        return bool((np.abs(w - W_MIN) <= rel * W_MIN).any())


# ---- linking -------------------------------------------------------------------------------------------------------------------------
def spans(track_start, frame):
    ts = np.asarray(track_start)
    return np.asarray(frame)[ts[:-1]].astype(np.int64), np.asarray(frame)[ts[1:] - 1].astype(np.int64)


def candidates(track_start, frame, max_absence):
    first, last = spans(track_start, frame)
    K = len(first)
    return np.array([(a, b) for a in range(K) for b in range(K) if 1 <= first[b] - last[a] <= max_absence], np.int32).reshape(-1, 2)


def link(track_start, frame, dist, pairs, max_absence, sigma_s, sigma_a, min_overlap, no_app):
    """-> dict: identity [K], links [L,2], link_cost [L], cost [C] (inf outside the time window)."""
    first, last = spans(track_start, frame)
    K = len(first)
    cand = []
    cost = np.full(len(pairs), np.inf)
    for c, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        if not 1 <= first[b] - last[a] <= max_absence:
            continue
        d_shape, d_app, overlap = (float(v) for v in dist[c][:3])
        cost[c] = d_shape / sigma_s ** 2 + (d_app / sigma_a ** 2 if overlap >= min_overlap else no_app)
        if cost[c] <= 1.0:
            cand.append((cost[c], int(a), int(b)))
    cand.sort()
    succ, pred, links, link_cost = {}, {}, [], []
    for cst, a, b in cand:
        if a in succ or b in pred:
            continue
        succ[a], pred[b] = b, a
        links.append((a, b))
        link_cost.append(cst)
    identity = np.full(K, -1, np.int32)
    n = 0
    for k in range(K):
        if k in pred:
            continue
        j = k
        identity[j] = n
        while j in succ:
            j = succ[j]
            identity[j] = n
        n += 1
    return {'identity': identity, 'links': np.array(links, np.int32).reshape(-1, 2), 'link_cost': np.array(link_cost, np.float64), 'cost': cost}


# ---- one shape per identity --------------------------------------------------------------------------------------------------------
def share_shape(para, conf, track_start, identity):
    """para [N,229] f32 -> (rows [N,229] f32 with every identity's betas replaced by its weighted mean, rounded once; mean [G,10]
    float64; status [G]).  The order inside an identity is ascending (track id, t); a weightless identity keeps its rows."""
    para = np.asarray(para, np.float32)
    out = para.copy()
    G = int(np.max(identity)) + 1 if len(identity) else 0
    mean, status = np.zeros((G, 10)), np.zeros(G, np.int32)
    for g in range(G):
        rows = np.concatenate([np.arange(track_start[k], track_start[k + 1]) for k in range(len(identity)) if identity[k] == g])
        m, sc = weighted_mean(para[rows, 3:13], np.asarray(conf)[rows])
        if sc > 0:
            mean[g] = m
            out[rows, 3:13] = m.astype(np.float32)[None]
        else:
            status[g] = 1
    return out, mean, status


# ---- the recovery case ---------------------------------------------------------------------------------------------------------------
VIEWS = (('front', 'back', 'both'), ('both', 'front', 'front'), ('back', 'both', 'front'), ('front', 'front', 'back'))


def recovery_case(seed=0, T=8, max_absence=150, shape_noise=0.3, texel_noise=0.05):
    """Four people, each seen as three tracklets of 17 to 40 rows.  The first absence of everyone lies inside max_absence (70 to 140
    frames, so that the first and the third tracklet of a person are never candidates); the second absence lies inside for people 1
    and 3 and beyond (160 to 220 frames) for people 0 and 2.  One shape per person, N(0, 1); people 0 and 1 share a shape and differ
    only in colour, people 2 and 3 share their colours and differ only in shape.  The rows of a tracklet are
    track_oracle.recovery_case's (noisy cam and rotations, N(0, shape_noise) on the shape per row, 15 % of the interior rows dropped:
    gap rows with conf 0 and NaN values).  Skin: one base colour per person and chart, uniform in [0.1, 0.9], plus N(0, texel_noise)
    per texel and tracklet, clipped to [0, 1]; a tracklet sees the front half of the charts (0 .. 11), the back half or both, weights
    uniform in [0.2, 3]; texels it does not see have weight 0 and NaN colours.  Tracks are numbered by their first frame.

    -> dict: track_start, frame, det, conf, para [N,229] f32, atlas [K,24,T,T,4] f32, person [K], order [K] (the tracklet's place in
    its person's sequence), true_links: the set of (a, b) consecutive tracklets of one person whose absence is within max_absence,
    far_links: those beyond it."""
    rng = np.random.default_rng(seed)
    shapes = rng.normal(0, 1, (4, 10))
    shapes[1] = shapes[0]
    colours = rng.uniform(0.1, 0.9, (4, PARTS, 3))
    colours[3] = colours[2]
    tracklets = []
    for p in range(4):
        lengths = rng.integers(17, 41, 3)
        absences = [int(rng.integers(70, 141)), int(rng.integers(160, 221) if p in (0, 2) else rng.integers(70, 141))]
        rc = to.recovery_case(seed=100 * seed + 10 + p, lengths=tuple(int(n) for n in lengths), shape_noise=shape_noise)
        start = int(rng.integers(0, 40))
        for i in range(3):
            s, e = int(rc['track_start'][i]), int(rc['track_start'][i + 1])
            rows, conf = rc['obs'][s:e].copy(), rc['conf'][s:e].copy()
            betas = (shapes[p][None] + rng.normal(0, shape_noise, (e - s, 10))).astype(np.float32)
            rows[:, 3:13] = np.where(conf[:, None] > 0, betas, np.nan)
            view = VIEWS[p][i]
            seen = np.zeros(PARTS, bool)
            seen[:12] = view in ('front', 'both')
            seen[12:] = view in ('back', 'both')
            atlas = np.full((PARTS, T, T, 4), np.nan, np.float32)
            atlas[..., 3] = 0.0
            rgb = np.clip(colours[p][:, None, None, :] + rng.normal(0, texel_noise, (PARTS, T, T, 3)), 0.0, 1.0)
            atlas[seen, :, :, :3] = rgb[seen].astype(np.float32)
            atlas[seen, :, :, 3] = rng.uniform(0.2, 3.0, (int(seen.sum()), T, T)).astype(np.float32)
            tracklets.append({'person': p, 'order': i, 'first': start, 'rows': rows, 'conf': conf, 'atlas': atlas})
            start += (e - s) + (absences[i] - 1 if i < 2 else 0)
    tracklets.sort(key=lambda t: (t['first'], t['person']))
    track_start = np.concatenate([[0], np.cumsum([len(t['conf']) for t in tracklets])]).astype(np.int32)
    frame = np.concatenate([t['first'] + np.arange(len(t['conf'])) for t in tracklets]).astype(np.int32)
    conf = np.concatenate([t['conf'] for t in tracklets]).astype(np.float32)
    person = np.array([t['person'] for t in tracklets], np.int32)
    order = np.array([t['order'] for t in tracklets], np.int32)
    first, last = spans(track_start, frame)
    true_links, far_links = set(), set()
    for a in range(len(tracklets)):
        for b in range(len(tracklets)):
            if person[a] == person[b] and order[b] == order[a] + 1:
                (true_links if first[b] - last[a] <= max_absence else far_links).add((a, b))
    return {'track_start': track_start, 'frame': frame, 'det': np.where(conf > 0, 0, -1).astype(np.int32), 'conf': conf,
            'para': np.concatenate([t['rows'] for t in tracklets]).astype(np.float32), 'atlas': np.stack([t['atlas'] for t in tracklets]),
            'person': person, 'order': order, 'true_links': true_links, 'far_links': far_links, 'n_frames': int(frame.max()) + 1}


def score(links, case):
    """-> (found, wrong, missed) of a link list against the case's true links."""
    got = set((int(a), int(b)) for a, b in links)
    return len(got & case['true_links']), len(got - case['true_links']), len(case['true_links'] - got)


def solve_case(case, **kw):
    """The whole rule on a recovery case in float64 (descriptors rounded to fp32 once, distances rounded to fp32 once, as the rule
    says) -> link's dict plus 'dist' and 'pairs'."""
    par = dict(DEFAULTS, **kw)
    shape, _ = shape_descriptors(case['para'], case['conf'], case['track_start'])
    shape = shape.astype(np.float32)
    pairs = candidates(case['track_start'], case['frame'], par['max_absence'])
    dist = pair_distance(shape, case['atlas'], pairs).astype(np.float32)
    res = link(case['track_start'], case['frame'], dist, pairs, **par)
    res.update({'dist': dist, 'pairs': pairs, 'shape': shape})
    return res
