"""The scene rule of DESIGN.md restated in numpy (float64 by default; float32 on request, to measure what the number format alone
costs), independent of csrc/scene_ops.hip: a loop over the faces in id order with the pixels of a face's candidate range as
arrays, and a strict `<` so that an exact tie stays with the smaller id.

render(...) returns, per frame, besides what the op returns (out, ids, depth):
  edge   (a) the smallest distance, in pixels, from the pixel centre to an edge LINE of any face whose candidate range holds the
             pixel (+inf where there is none) -- a coverage decision within rounding of an edge is not the rule's to make;
  gap    (b) the relative gap (d2 - d1) / d1 between the two smallest depths at the pixel (+inf with fewer than two);
  level  (c) the unrounded colour level clamp01(v) * 255 of the winning face (NaN where nothing is drawn).
The scenes of tests/test_scene_host.py and tests/test_gpu_scene.py are built here too, so that both files see the same inputs."""
import numpy as np

NEAR = 0.1
EDGE_EPS = 1e-3          # pixels
GAP_EPS = 1e-5           # relative
# The colour margin of tests/test_gpu_scene.py, in levels of 255: 4 x the largest difference between this oracle in float32 and in
# float64 on main_scene (colour_delta below: 4 x 1.2217e-3 = 4.887e-3), rounded up.  Neither run is the code under test;
# tests/test_scene_host.py recomputes it.
DELTA = 0.005


def project(verts, cam_t, proj, dt=np.float64):
    """[P,V,3] -> (col, row, z) [P,V] each, the operations of scene_project_kernel in `dt`."""
    v, t, q = (np.asarray(a).astype(dt) for a in (verts, cam_t, proj))
    with np.errstate(all='ignore'):
        z = v[..., 2] + t[:, None, 2]
        xn = (v[..., 0] + t[:, None, 0]) / z
        yn = (v[..., 1] + t[:, None, 1]) / z
        col = (q[:, None, 0] * xn + q[:, None, 1] * yn) + q[:, None, 2]
        row = (q[:, None, 3] * xn + q[:, None, 4] * yn) + q[:, None, 5]
    return col, row, z


def _clamp01(x):
    return np.minimum(np.maximum(x, x.dtype.type(0)), x.dtype.type(1))


def render(verts, vcol, faces2, cam_t, proj, dscale, person_frame, frames, dt=np.float64):
    """-> list (one dict per frame) of out uint8 [H,W,3], ids int32 [H,W], depth `dt` [H,W], edge f64 [H,W], gap f64 [H,W],
    level `dt` [H,W,3]."""
    faces2 = np.asarray(faces2).astype(np.int64).reshape(-1, 3)
    F2 = faces2.shape[0]
    vcol = np.asarray(vcol).astype(dt)
    ds = np.asarray(dscale).astype(dt).reshape(-1)
    col, row, z = project(verts, cam_t, proj, dt)
    pf = np.asarray(person_frame).reshape(-1)
    res = []
    slack = dt(0.01)
    for n, frame in enumerate(frames):
        H, W = frame.shape[:2]
        best = np.full((H, W), np.inf, dt)
        second = np.full((H, W), np.inf, dt)
        ids = np.full((H, W), -1, np.int64)
        edge = np.full((H, W), np.inf, np.float64)
        for p in np.nonzero(pf == n)[0]:
            X, Y, Z = col[p][faces2], row[p][faces2], z[p][faces2]                       # [F2,3]
            with np.errstate(all='ignore'):
                ok = (Z > dt(NEAR)).all(1) & np.isfinite(X).all(1) & np.isfinite(Y).all(1) & np.isfinite(Z).all(1) & np.isfinite(ds[p])
                area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
                ok &= (area > 0) & np.isfinite(area)
            for f in np.nonzero(ok)[0]:
                x0, x1, x2 = X[f]
                y0, y1, y2 = Y[f]
                z0, z1, z2 = Z[f]
                c0 = max(int(np.ceil(min(x0, x1, x2) - slack)), 0)
                c1 = min(int(np.floor(max(x0, x1, x2) + slack)), W - 1)
                r0 = max(int(np.ceil(min(y0, y1, y2) - slack)), 0)
                r1 = min(int(np.floor(max(y0, y1, y2) + slack)), H - 1)
                if c0 > c1 or r0 > r1:
                    continue
                yp, xp = np.meshgrid(np.arange(r0, r1 + 1).astype(dt), np.arange(c0, c1 + 1).astype(dt), indexing='ij')
                e0 = (x1 - xp) * (y2 - yp) - (y1 - yp) * (x2 - xp)
                e1 = (x2 - xp) * (y0 - yp) - (y2 - yp) * (x0 - xp)
                e2 = (x0 - xp) * (y1 - yp) - (y0 - yp) * (x1 - xp)
                sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
                l0 = np.hypot(float(x2) - float(x1), float(y2) - float(y1))
                l1 = np.hypot(float(x0) - float(x2), float(y0) - float(y2))
                l2 = np.hypot(float(x1) - float(x0), float(y1) - float(y0))
                with np.errstate(all='ignore'):
                    dist = np.minimum(np.minimum(np.abs(e0.astype(np.float64)) / l0, np.abs(e1.astype(np.float64)) / l1), np.abs(e2.astype(np.float64)) / l2)
                    edge[sl] = np.fmin(edge[sl], dist)
                    inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
                    if not inside.any():
                        continue
                    a = area[f]
                    w0, w1, w2 = e0 / a, e1 / a, e2 / a
                    zp = dt(1) / (w0 / z0 + w1 / z1 + w2 / z2)
                    d = zp * ds[p]
                    valid = inside & (d > 0) & (d < np.inf)
                b, s = best[sl], second[sl]
                better = valid & (d < b)
                second[sl] = np.where(better, b, np.where(valid, np.minimum(s, d), s))
                best[sl] = np.where(better, d, b)
                ids[sl] = np.where(better, p * F2 + f, ids[sl])
        out = np.array(frame, dtype=np.uint8, copy=True)
        level = np.full((H, W, 3), np.nan, dt)
        rr, cc = np.nonzero(ids >= 0)
        if rr.size:
            pid, fid = ids[rr, cc] // F2, ids[rr, cc] % F2
            tri = faces2[fid]                                                            # [n,3]
            xp, yp = cc.astype(dt), rr.astype(dt)
            xs = [col[pid, tri[:, k]] - xp for k in range(3)]
            ys = [row[pid, tri[:, k]] - yp for k in range(3)]
            zs = [z[pid, tri[:, k]] for k in range(3)]
            w0 = xs[1] * ys[2] - ys[1] * xs[2]
            w1 = xs[2] * ys[0] - ys[2] * xs[0]
            w2 = xs[0] * ys[1] - ys[0] * xs[1]
            with np.errstate(all='ignore'):
                a = w0 + w1 + w2
                w0, w1, w2 = _clamp01(w0 / a), _clamp01(w1 / a), _clamp01(w2 / a)
                ws = w0 + w1 + w2
                bad = ~(ws > 0)
                w0, w1, w2, ws = (np.where(bad, dt(k), x) for k, x in ((1, w0), (1, w1), (1, w2), (3, ws)))
                w0, w1, w2 = w0 / ws, w1 / ws, w2 / ws
                p0, p1, p2 = w0 / zs[0], w1 / zs[1], w2 / zs[2]
                ps = p0 + p1 + p2
                for ch in range(3):
                    v = (p0 * vcol[pid, tri[:, 0], ch] + p1 * vcol[pid, tri[:, 1], ch] + p2 * vcol[pid, tri[:, 2], ch]) / ps
                    level[rr, cc, ch] = _clamp01(v) * dt(255)
            out[rr, cc] = np.rint(level[rr, cc]).astype(np.uint8)                        # half to even
        with np.errstate(all='ignore'):
            gap = np.where(np.isfinite(second), (second.astype(np.float64) - best.astype(np.float64)) / best.astype(np.float64), np.inf)
        res.append({'out': out, 'ids': ids.astype(np.int32), 'depth': best, 'edge': edge, 'gap': gap, 'level': level})
    return res


def uncertain(r):
    """The pixels of one frame's result whose winner the rule does not decide within rounding: (a) < 1e-3 pixels or (b) < 1e-5."""
    return (r['edge'] < EDGE_EPS) | (r['gap'] < GAP_EPS)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def icosahedron():
    """12 vertices on the unit sphere, 20 faces."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    v /= np.linalg.norm(v[0])
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return v, f


def both_windings(f):
    return np.concatenate([f, f[:, ::-1]], 0).astype(np.int32).copy()


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


RES, FOCAL = 224, 500.0        # a short focal: the depth relief of a body is a quarter of its distance, so depths interleave
MAIN_SEED = 20
FRAME_SHAPES = ((37, 53), (64, 40), (16, 16))


def make_people(seed, boxes, cams, frame_shapes, person_frame, radius=0.5):
    """Icosahedra of `radius`, each turned at random and coloured at random in [0, 1.2] (so that the clamp is used), behind the
    cameras person_cameras makes of `boxes` (center, scale) and `cams` (s, tx, ty).  Everything the op takes, as float32."""
    from danet_densepose2smpl_amd import datasets, scene
    rng = np.random.default_rng(seed)
    ico, f = icosahedron()
    P = len(boxes)
    verts = np.stack([radius * ico @ _rotation(rng).T for _ in range(P)])
    vcol = rng.uniform(0.0, 1.2, (P, 12, 3))
    center = np.array([b[0] for b in boxes], np.float64).reshape(P, 2)
    scale = np.array([b[1] for b in boxes], np.float64).reshape(P)
    _, tinv = datasets.crop_transforms(center, scale, np.zeros(P), RES)
    k = scene.person_cameras(np.asarray(cams, np.float64), tinv, frame_shapes, person_frame, RES, focal=FOCAL)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    return {'verts': f32(verts), 'vcol': f32(vcol), 'faces2': both_windings(f), 'cam_t': f32(k['cam_t']), 'proj': f32(k['proj']),
            'dscale': f32(k['dscale']), 'person_frame': np.asarray(person_frame, np.int32)}


def make_frames(seed, shapes=FRAME_SHAPES):
    rng = np.random.default_rng(seed + 1000)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


def main_scene(seed=MAIN_SEED):
    """Test 1: three frames of 37 x 53, 64 x 40 and 16 x 16 (rows x cols; odd sizes, so byte offsets are no multiples of 4).  Frame
    0: two people whose boxes overlap at the same s * scale, so that their depth ranges interleave, and one whose 80-pixel box,
    larger than the frame, hangs over the top-left corner (it is nearer, and covers part of the first); frame 1: one person from an [x, y, w, h] box; frame 2: nobody."""
    from danet_densepose2smpl_amd import scene
    boxes = [(np.array([22.0, 18.0]), 0.17), (np.array([31.0, 20.0]), 0.17), (np.array([2.0, 3.0]), 0.40),
             scene.boxes_from_xywh([6.0, 10.0, 25.0, 40.0])]
    cams = [(1.0, 0.03, -0.02), (1.0, -0.05, 0.04), (0.7, 0.2, 0.15), (0.9, 0.0, 0.05)]
    people = make_people(seed, boxes, cams, FRAME_SHAPES, [0, 0, 0, 1])
    return people, make_frames(seed)


def run(people, frames, dt=np.float64, keep=None):
    """render() on a make_people dict (optionally only the people `keep`, a list of indices)."""
    k = np.arange(people['verts'].shape[0]) if keep is None else np.asarray(keep)
    return render(people['verts'][k], people['vcol'][k], people['faces2'], people['cam_t'][k], people['proj'][k], people['dscale'][k],
                  people['person_frame'][k], frames, dt)


def colour_delta(people, frames):
    """4 x the largest difference of the unrounded levels between the rule in float32 and in float64, over the pixels both runs give
    to the same face and neither flags: what the number format alone costs on these inputs, with a factor for the device's freedom to
    differ from numpy's float32 in the last place of each step."""
    a, b = run(people, frames, np.float64), run(people, frames, np.float32)
    m = 0.0
    for ra, rb in zip(a, b):
        same = (ra['ids'] == rb['ids']) & (ra['ids'] >= 0) & ~uncertain(ra)
        if same.any():
            m = max(m, float(np.abs(ra['level'][same] - rb['level'][same].astype(np.float64)).max()))
    return 4.0 * m


SKIP_KINDS = ('zero_area', 'behind', 'nan', 'outside')
SKIP_SEED = 31


def skip_scene(kind, seed=SKIP_SEED):
    """Test 2: one 37 x 53 frame with the two overlapping people of main_scene and one thing that must draw nothing.
    zero_area: two more faces (0, 0, 1) and (1, 0, 0) at the end of the table; behind: the nearest vertex of person 0 put at Z + tz
    = 0.05; nan: its x is NaN; outside: person 1's box lies wholly outside the frame.  -> (people, frames, dead) with dead(ids) ->
    the mask of pixels that name something that must not be drawn."""
    boxes = [(np.array([22.0, 18.0]), 0.17), (np.array([31.0, 20.0]), 0.17)]
    if kind == 'outside':
        boxes[1] = (np.array([-100.0, -90.0]), 0.17)
    people = make_people(seed, boxes, [(1.0, 0.03, -0.02), (1.0, -0.05, 0.04)], FRAME_SHAPES[:1], [0, 0])
    F2 = 40
    if kind == 'zero_area':
        people['faces2'] = np.concatenate([people['faces2'], np.array([[0, 0, 1], [1, 0, 0]], np.int32)], 0)
        F2 = 42
        dead = lambda ids: (ids >= 0) & (ids % F2 >= 40)                                  # noqa: E731
    elif kind in ('behind', 'nan'):
        k = int(np.argmin(people['verts'][0, :, 2]))
        if kind == 'behind':
            people['verts'][0, k, 2] = np.float32(0.05) - people['cam_t'][0, 2]
        else:
            people['verts'][0, k, 0] = np.nan
        hit = (people['faces2'] == k).any(1)
        dead = lambda ids: (ids >= 0) & (ids < F2) & hit[np.maximum(ids, 0) % F2]         # noqa: E731
    elif kind == 'outside':
        dead = lambda ids: ids >= F2                                                      # noqa: E731
    else:
        raise ValueError(kind)
    return people, make_frames(seed, FRAME_SHAPES[:1]), dead
