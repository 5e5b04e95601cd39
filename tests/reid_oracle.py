"""The causal identity rule (DESIGN.md 4b'-reid) restated in float64 numpy, written from the section and not from the kernel or the
product's host code: the head of a newborn track, the gallery of finished tracks with its two evictions, the decision taken once per
drawn frame, and the carry arithmetic of "one shape per identity" -- and the recovery case on which the online defaults were chosen.
The pair distance, the cost and the weighted mean are the identity rule's (tests/link_oracle.py); they are used here, not restated.

The skin of the recovery case.  link_oracle.recovery_case gives every tracklet one fused atlas.  Here that atlas is spread over the
tracklet's rows: every observed row contributes an equal share of a texel's weight and the texel's colour, so the running sums after
m of the tracklet's n observed rows are (m / n) w (r, g, b, 1), and the head's atlas is the tracklet's colours with the weights
scaled by m / n (rounded to float32 once, as a descriptor is).  Gap rows contribute nothing to the skin."""
import numpy as np

import link_oracle as lo

DEFAULTS = {'max_absence': 150, 'sigma_s': 0.4, 'sigma_a': 0.2, 'min_overlap': 0.1, 'no_app': 0.5}      # tracks.REID_DEFAULTS, restated
LAG = 8                                                                                                  # video.STREAM_LAG, restated


# ---- the shape sums --------------------------------------------------------------------------------------------------------------------
def shape_sums(betas, conf):
    """(sum_y [10], sum_c) over the rows in the order given: sum_c += c, sum_y += c * beta, rows with c = 0 never read."""
    sy, sc = np.zeros(10), 0.0
    for t in range(len(conf)):
        if conf[t] > 0:
            sc = sc + float(conf[t])
            sy = sy + float(conf[t]) * np.asarray(betas[t], np.float64)
    return sy, sc


def shape_of(sy, sc):
    """The shape descriptor of the sums, rounded to float32 once; zeros where there is no weight."""
    return (sy / sc).astype(np.float32) if sc > 0 else np.zeros(10, np.float32)


def carried_shape(carry, sy, sc):
    """The betas an emitted row of a linked track gets: (carry_y + sum_y) / (carry_c + sum_c), rounded once; None without weight."""
    den = carry[10] + sc
    return ((carry[:10] + sy) / den).astype(np.float32) if den > 0 else None


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def solve(first, last, final, head, sums, gallery=None, **kw):
    """first, last [K]: the spans of the tracks, numbered by (first frame, id).  final(k) / head(k) -> (shape [10] f32, atlas
    [24,T,T,4] f32): the descriptor of the finished track and of its head.  sums [K,11] float64: the finished track's own
    (sum_y, sum_c).  gallery: the number of entries the gallery may hold (None: no limit and no eviction by absence: nothing ever
    leaves but by a successor).  -> dict: identity [K], links [L,2] and link_cost [L] in acceptance order, carry [K,11] and tot
    [K,11] float64, dist {(a, b): [4] f32}, peak (the most entries the gallery held)."""
    par = dict(DEFAULTS, **kw)
    K = len(first)
    A = par['max_absence']
    identity = np.full(K, -1, np.int32)
    carry, tot = np.zeros((K, 11)), np.zeros((K, 11))
    links, link_cost, dist_of = [], [], {}
    entries = []                                                             # the gallery: track ids
    n, peak = 0, 0
    for d in range(int(np.min(first)), int(np.max(last)) + 1):
        if gallery is not None:
            entries = [a for a in entries if d - last[a] <= A]                # such an entry can never be a candidate again
        born = [b for b in range(K) if first[b] == d]
        cand = [a for a in entries if 1 <= d - last[a] <= A]
        scored = []
        if born and cand:
            pairs = [(a, b) for a in sorted(cand) for b in born]
            shape = np.stack([final(a)[0] for a in range(K)])                 # (only the rows of `cand` and `born` are read below)
            atlas = np.stack([final(a)[1] for a in range(K)])
            for b in born:
                shape[b], atlas[b] = head(b)
            dist = lo.pair_distance(shape, atlas, np.array(pairs)).astype(np.float32)
            for (a, b), row in zip(pairs, dist):
                dist_of[(a, b)] = row
                d_shape, d_app, overlap = (float(v) for v in row[:3])
                cost = d_shape / par['sigma_s'] ** 2 + (d_app / par['sigma_a'] ** 2 if overlap >= par['min_overlap'] else par['no_app'])
                if cost <= 1.0:
                    scored.append((cost, a, b))
        scored.sort()
        succ, pred = set(), {}
        for cost, a, b in scored:
            if a in succ or b in pred:
                continue
            succ.add(a)
            pred[b] = a
            links.append((a, b))
            link_cost.append(cost)
        for b in born:
            if b in pred:
                identity[b] = identity[pred[b]]
                carry[b] = tot[pred[b]]
                entries.remove(pred[b])                                      # it has its successor
            else:
                identity[b] = n
                n += 1
        for a in range(K):
            if last[a] == d:                                                 # its last row is drawn: the track enters the gallery
                tot[a] = carry[a] + sums[a]
                entries.append(a)
        peak = max(peak, len(entries))
        if gallery is not None and len(entries) > gallery:
            raise RuntimeError('the gallery holds %d entries, %d allowed' % (len(entries), gallery))
    return {'identity': identity, 'links': np.array(links, np.int32).reshape(-1, 2), 'link_cost': np.array(link_cost, np.float64),
            'carry': carry, 'tot': tot, 'dist': dist_of, 'peak': peak}


# ---- the recovery case -----------------------------------------------------------------------------------------------------------------
def recovery_case(seed=0, **kw):
    """link_oracle.recovery_case plus what the causal rule needs of it: first, last [K], and per track the rows' betas and conf."""
    case = lo.recovery_case(seed, **kw)
    case['first'], case['last'] = lo.spans(case['track_start'], case['frame'])
    return case


def head_rows(case, k, rows):
    """The rows of track k's head: its first `rows` rows (None: all of them)."""
    s, e = int(case['track_start'][k]), int(case['track_start'][k + 1])
    return s, e if rows is None else min(e, s + rows)


def descriptor(case, k, rows=None):
    """The descriptor of the first `rows` rows of track k (None: the finished track) -> (shape [10] f32, atlas [24,T,T,4] f32, sums
    [11] f64).  The skin follows the model of the header: the weights scaled by the head's share of the observed rows."""
    s, e = head_rows(case, k, rows)
    full = int(case['track_start'][k + 1])
    sy, sc = shape_sums(case['para'][s:e, 3:13], case['conf'][s:e])
    share = float((case['det'][s:e] >= 0).sum()) / float((case['det'][s:full] >= 0).sum())
    atlas = case['atlas'][k].copy()
    atlas[..., 3] = (atlas[..., 3].astype(np.float64) * share).astype(np.float32)
    return shape_of(sy, sc), atlas, np.concatenate([sy, [sc]])


def solve_case(case, rows=LAG + 1, gallery=None, **kw):
    """The causal rule on a recovery case with heads of `rows` rows (None: unbounded heads, the whole track)."""
    K = len(case['first'])
    final = [descriptor(case, k) for k in range(K)]
    heads = [descriptor(case, k, rows) for k in range(K)]
    return solve(case['first'], case['last'], lambda k: final[k][:2], lambda k: heads[k][:2], np.stack([f[2] for f in final]), gallery, **kw)


SWEEP = [dict(sigma_s=s, sigma_a=a, no_app=n) for s in (0.3, 0.4, 0.5) for a in (0.15, 0.2, 0.3) for n in (0.5, 0.75)]


def sweep(seeds=(0, 1, 2), rows=(LAG + 1, 5), settings=SWEEP):
    """-> [(setting, {rows: (found, wrong, missed) summed over the seeds})] for every setting of the table of DESIGN.md 4b'-reid."""
    cases = [recovery_case(s) for s in seeds]
    out = []
    for kw in settings:
        res = {}
        for r in rows:
            res[r] = tuple(int(v) for v in np.sum([lo.score(solve_case(c, r, **kw)['links'], c) for c in cases], 0))
        out.append((kw, res))
    return out
