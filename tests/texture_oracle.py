"""TEST INFRASTRUCTURE: a numpy restatement of the texture rule (DESIGN.md "texture rule"; csrc/texture_ops.hip), operation by
operation, with a dtype switch: float64 is the oracle, float32 repeats the device's arithmetic and gives the rounding bound.  The
texel map is always computed in double (that is the rule).  The depth and face-index planes come from oracle.raster_forward.

Also here: the test topology (an icosahedron, the smallest body that can go wrong), the scenes the GPU tests use, `uncertain`
(texels and pixels whose decisions a rounding could flip) and `bounds()`, the two tolerances the GPU tests share."""
import functools
import math

import numpy as np

import oracle

FOCAL = 5000.0
H = 64                    # image size of every scene
PARTS = 24
EPS = 1e-3                # the margin of `uncertain`


# ---- the topology ------------------------------------------------------------------------------------------------------------------
def ico_mesh(radius=0.8):
    """-> vertices [12,3] f32, faces [20,3] (outward winding)."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    v *= radius / np.linalg.norm(v[0])
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    return v.astype(np.float32), f


CHART_A = ((1, 1), (7, 1), (1, 15))             # sixteenths
CHART_B = ((15, 15), (9, 15), (15, 1))
DIAG_A = ((1, 1), (15, 1), (1, 15))             # parts 9: two faces sharing the diagonal u + v = 1
DIAG_B = ((15, 15), (1, 15), (15, 1))


def ico_densepose():
    """The DensePose dict of the test topology: 60 DensePose vertices (three per face), parts 1..9 two faces each on disjoint
    chart triangles, part 10 two faces sharing the chart's diagonal, parts 11..24 empty."""
    _, f = ico_mesh()
    uv = np.zeros((60, 2))
    part = np.zeros(20, np.int64)
    for k in range(20):
        part[k] = k // 2 + 1
        tri = (DIAG_A, DIAG_B)[k % 2] if k >= 18 else (CHART_A, CHART_B)[k % 2]
        uv[3 * k:3 * k + 3] = np.array(tri, np.float64) / 16.0
    return {'All_vertices': (f.reshape(-1) + 1).astype(np.uint32), 'All_Faces': (np.arange(60).reshape(20, 3) + 1).astype(np.uint32),
            'All_FaceIndices': part.astype(np.uint8), 'All_U_norm': uv[:, 0].copy(), 'All_V_norm': uv[:, 1].copy()}


def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def smooth_image():
    """Two linear ramps and one low-frequency product of sines, [3,H,H] f32."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(H, dtype=np.float64), indexing='ij')
    return np.stack([x / (H - 1), y / (H - 1), 0.5 + 0.5 * np.sin(2 * np.pi * x / H) * np.sin(2 * np.pi * 1.5 * y / H)]).astype(np.float32)


VIEWS = ((0.31, 0.17, 0.05), (0.22, 1.05, -0.11), (-0.4, 2.3, 0.2), (0.1, -0.9, 0.33))        # body rotations (x, y, z), radians
CAMS = ((3.0, 0.85, 0.85), (3.1, 0.84, 0.87), (2.9, 0.86, 0.83), (3.0, 0.2, 0.85))          # the last pushes the body out of the frame


def scene(name):
    """-> dict(images [N,3,H,H], vertices [N,12,3], cam [N,3] f32, view_off).  'main': two views of one person; 'three': view_off
    [0,2,3]; 'edge': a view that leaves the frame, a person without views, a third person; 'round': one view of the smooth image."""
    v, _ = ico_mesh()
    which, off = {'main': ((0, 1), [0, 2]), 'three': ((0, 1, 2), [0, 2, 3]), 'edge': ((3, 2), [0, 1, 1, 2]), 'round': ((0,), [0, 1])}[name]
    rng = np.random.default_rng(7)
    imgs = rng.random((4, 3, H, H)).astype(np.float32)
    images = np.stack([smooth_image() if name == 'round' else imgs[k] for k in which])
    verts = np.stack([(v.astype(np.float64) @ rot_xyz(*VIEWS[k]).T).astype(np.float32) for k in which])
    cam = np.array([CAMS[k] for k in which], np.float32)
    return {'images': images, 'vertices': verts, 'cam': cam, 'view_off': off}


# ---- step 1: the map ---------------------------------------------------------------------------------------------------------------
def texture_map(tables, T):
    """-> face [24,T,T] int32 (-1: none), bary [24,T,T,2] f32.  Double arithmetic from the f32 UV table, in the written order."""
    uv = tables['uv'].astype(np.float64)
    faces, off, pf = tables['faces'], tables['part_off'], tables['part_faces']
    face = np.full((PARTS, T * T), -1, np.int32)
    bary = np.zeros((PARTS, T * T, 2), np.float32)
    t = np.arange(T * T)
    u = (((t % T).astype(np.float64) + 0.5) / float(T))[:, None]
    v = (((t // T).astype(np.float64) + 0.5) / float(T))[:, None]
    for p in range(PARTS):
        fs = pf[off[p]:off[p + 1]]
        if fs.size == 0:
            continue
        a, b, c = (uv[faces[fs, k]] for k in range(3))
        au, av, bu, bv, cu, cv = a[None, :, 0], a[None, :, 1], b[None, :, 0], b[None, :, 1], c[None, :, 0], c[None, :, 1]
        e0 = (bu - u) * (cv - v) - (bv - v) * (cu - u)
        e1 = (cu - u) * (av - v) - (cv - v) * (au - u)
        e2 = (au - u) * (bv - v) - (av - v) * (bu - u)
        area = e0 + e1 + e2
        ok = (area != 0.0) & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))
        hit = ok.any(1)
        first = ok.argmax(1)                                   # the lowest index among the faces that hold the texel
        rows = np.nonzero(hit)[0]
        face[p, rows] = fs[first[rows]]
        with np.errstate(all='ignore'):
            bary[p, rows, 0] = (e0[rows, first[rows]] / area[rows, first[rows]]).astype(np.float32)
            bary[p, rows, 1] = (e1[rows, first[rows]] / area[rows, first[rows]]).astype(np.float32)
    return face.reshape(PARTS, T, T), bary.reshape(PARTS, T, T, 2)


# ---- the camera of raster_project_kernel -----------------------------------------------------------------------------------------------
def _camera(dt, focal, orig, s):
    fx, cx = dt(focal), dt(orig) / dt(2)
    if orig != 224:
        sc = dt(orig) / dt(224)
        fx, cx = fx * sc, cx * sc
    tz = (dt(2) * dt(focal)) / (dt(orig) * s + dt(1e-9))
    return fx, cx, tz


def depth_planes(tables, vertices, cam, S):
    """The rasteriser's (face index, depth) planes of the DensePose faces at orig = out_size = S."""
    tex = np.zeros((tables['faces'].shape[0], 3), np.float32)
    _, fidx, depth = oracle.raster_forward(vertices, cam, tables['vert_mapping'], tables['faces'], tex, FOCAL, float(S), S)
    return fidx, depth


# ---- step 2: the unwrap ------------------------------------------------------------------------------------------------------------
def texture_unwrap(tables, map_face, map_bary, images, vertices, cam, view_off, dtype=np.float64, depth_tol=0.02, min_cos=0.1, depth=None):
    """-> atlas [P,24,T,T,4] dtype, aux: per view the quantities `uncertain` looks at (NaN where the texel has no face)."""
    dt = np.dtype(dtype).type
    N, Hh = images.shape[0], images.shape[2]
    T = map_face.shape[-1]
    ntex = PARTS * T * T
    if depth is None:
        depth = depth_planes(tables, vertices, cam, Hh)[1] if N else np.zeros((0, Hh, Hh), np.float32)
    mf = map_face.reshape(-1)
    has = mf >= 0
    f = np.where(has, mf, 0)
    w0, w1 = map_bary.reshape(-1, 2)[:, 0].astype(dtype), map_bary.reshape(-1, 2)[:, 1].astype(dtype)
    w2 = dt(1) - w0 - w1
    idx = tables['vert_mapping'][tables['faces'][f]]                                   # [ntex,3] mesh vertices
    P = len(view_off) - 1
    atlas = np.zeros((P, ntex, 4), dtype)
    aux = {k: np.full((N, ntex), np.nan) for k in ('r', 'c', 'z', 'd', 'cos')}
    tol, mc, orig = dt(depth_tol), dt(min_cos), dt(Hh)
    for p in range(P):
        sc = np.zeros((ntex, 3), dtype)
        sw = np.zeros(ntex, dtype)
        for n in range(view_off[p], view_off[p + 1]):
            vb = vertices[n].astype(dtype)
            s, tx, ty = (dt(x) for x in cam[n].astype(dtype))
            fx, cx, tz = _camera(dt, FOCAL, Hh, s)
            A, B, C = vb[idx[:, 0]], vb[idx[:, 1]], vb[idx[:, 2]]
            X = w0 * A[:, 0] + w1 * B[:, 0] + w2 * C[:, 0]
            Y = w0 * A[:, 1] + w1 * B[:, 1] + w2 * C[:, 1]
            Z = w0 * A[:, 2] + w1 * B[:, 2] + w2 * C[:, 2]
            px, py, pz = X + tx, Y + ty, Z + tz
            zz = pz + dt(1e-9)
            x, y = px / zz, py / zz
            c = fx * x + cx - dt(0.5)
            r = fx * y + cx - dt(0.5)
            rn, cn = np.floor(r + dt(0.5)), np.floor(c + dt(0.5))
            inside = (rn >= 0) & (rn < orig) & (cn >= 0) & (cn < orig)
            ri, ci = np.where(inside, rn, 0).astype(np.int64), np.where(inside, cn, 0).astype(np.int64)
            d = np.where(inside, depth[n][ri, ci], np.float32(np.inf)).astype(dtype)
            vis = has & inside & (d < np.inf) & (pz <= d + tol)
            t0 = np.stack([A[:, 0] + tx, A[:, 1] + ty, A[:, 2] + tz], 1)
            e1 = np.stack([(B[:, 0] + tx) - t0[:, 0], (B[:, 1] + ty) - t0[:, 1], (B[:, 2] + tz) - t0[:, 2]], 1)
            e2 = np.stack([(C[:, 0] + tx) - t0[:, 0], (C[:, 1] + ty) - t0[:, 1], (C[:, 2] + tz) - t0[:, 2]], 1)
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            nl = np.sqrt(nx * nx + ny * ny + nz * nz)
            pl = np.sqrt(px * px + py * py + pz * pz)
            good = (nl > 0) & (pl > 0)
            with np.errstate(all='ignore'):
                cs = (dt(0) - (nx * px + ny * py + nz * pz)) / (nl * pl)
            vis &= good & (cs > mc)
            rf, cf = np.floor(r), np.floor(c)
            lr, lc = r - rf, c - cf
            r0, r1 = np.clip(rf.astype(np.int64), 0, Hh - 1), np.clip(rf.astype(np.int64) + 1, 0, Hh - 1)
            c0, c1 = np.clip(cf.astype(np.int64), 0, Hh - 1), np.clip(cf.astype(np.int64) + 1, 0, Hh - 1)
            for ch in range(3):
                pln = images[n, ch].astype(dtype)
                top = (dt(1) - lc) * pln[r0, c0] + lc * pln[r0, c1]
                bot = (dt(1) - lc) * pln[r1, c0] + lc * pln[r1, c1]
                col = (dt(1) - lr) * top + lr * bot
                sc[:, ch] = np.where(vis, sc[:, ch] + cs * col, sc[:, ch])
            sw = np.where(vis, sw + cs, sw)
            for k, a in (('r', r), ('c', c), ('z', pz), ('d', d), ('cos', cs)):
                aux[k][n] = np.where(has, a.astype(np.float64), np.nan)
        seen = sw > 0
        with np.errstate(all='ignore'):
            atlas[p, :, :3] = np.where(seen[:, None], sc / sw[:, None], dt(0))
        atlas[p, :, 3] = np.where(seen, sw, dt(0))
    return atlas.reshape(P, PARTS, T, T, 4), aux


def uncertain(aux, view_off, depth_tol=0.02, min_cos=0.1):
    """-> [P,ntex] bool: a texel one of whose decisions, in any view of its person, lies within EPS of flipping: r + 0.5 or c + 0.5
    of an integer (the nearest pixel), z of depth + depth_tol, cos of min_cos."""
    P = len(view_off) - 1
    out = np.zeros((P, aux['r'].shape[1]), bool)
    for p in range(P):
        for n in range(view_off[p], view_off[p + 1]):
            with np.errstate(invalid='ignore'):
                near = lambda a: np.abs(a - np.rint(a)) < EPS            # noqa: E731
                u = near(aux['r'][n] + 0.5) | near(aux['c'][n] + 0.5)
                u |= np.abs(aux['z'][n] - (aux['d'][n] + depth_tol)) < EPS
                u |= np.abs(aux['cos'][n] - min_cos) < EPS
            out[p] |= u
    return out


# ---- step 3: the draw --------------------------------------------------------------------------------------------------------------
def rotate_y(vertices, rot_y):
    """mesh_shade_vertex_kernel's rotation: f32, x' = x c - z s, z' = x s + z c with c, s rounded to f32."""
    c, s = np.float32(math.cos(rot_y)), np.float32(math.sin(rot_y))
    v = vertices.astype(np.float32)
    return np.stack([v[..., 0] * c - v[..., 2] * s, v[..., 1], v[..., 0] * s + v[..., 2] * c], -1)


def texture_render(tables, rverts, cam, fidx, atlas, atlas_index, images=None, fill=(0.5, 0.5, 0.5), dtype=np.float64):
    """rverts: the ROTATED vertices [N,NV,3] f32, fidx [N,S,S] the rasteriser's plane, atlas [P,24,T,T,4] f32.
    -> rgb [N,3,S,S] dtype, alpha [N,S,S], den [N,S,S] (the valid-tap denominator; NaN where nothing is drawn),
    taps [N,S,S,4] (flat texel index part * T * T + i * T + j of the four taps, -1 where nothing is drawn)."""
    dt = np.dtype(dtype).type
    N, S = fidx.shape[0], fidx.shape[-1]
    T = atlas.shape[2]
    uv = tables['uv'].astype(dtype)
    rgb = np.zeros((N, 3, S, S), dtype)
    alpha = np.zeros((N, S, S), np.float32)
    den_o = np.full((N, S, S), np.nan)
    taps_o = np.full((N, S, S, 4), -1, np.int64)
    Sf = dt(S)
    for b in range(N):
        rr, cc = np.nonzero(fidx[b] >= 0)
        if images is not None:
            rgb[b] = images[b].astype(dtype)
        if rr.size == 0:
            continue
        f = fidx[b][rr, cc]
        s, tx, ty = (dt(x) for x in cam[b].astype(dtype))
        fx, cx, tz = _camera(dt, FOCAL, S, s)
        half = Sf / dt(2)
        xp = (dt(2) * cc.astype(dtype) + dt(1) - Sf) / Sf
        yp = (Sf - dt(1) - dt(2) * rr.astype(dtype)) / Sf
        X = (xp * half + half - cx) / fx
        Y = (Sf - half - cx - yp * half) / fx
        dv = tables['faces'][f]                                                        # [n,3] DensePose vertices
        vb = rverts[b].astype(dtype)[tables['vert_mapping'][dv]]                       # [n,3,3]
        z = [vb[:, k, 2] + tz for k in range(3)]
        xs = [(vb[:, k, 0] + tx) / (z[k] + dt(1e-9)) - X for k in range(3)]
        ys = [(vb[:, k, 1] + ty) / (z[k] + dt(1e-9)) - Y for k in range(3)]
        w = [xs[1] * ys[2] - ys[1] * xs[2], xs[2] * ys[0] - ys[2] * xs[0], xs[0] * ys[1] - ys[0] * xs[1]]
        area = w[0] + w[1] + w[2]
        with np.errstate(all='ignore'):
            w = [np.clip(wk / area, dt(0), dt(1)) for wk in w]
            ws = w[0] + w[1] + w[2]
            bad = ~(ws > 0)
            w = [np.where(bad, dt(1), wk) for wk in w]
            ws = np.where(bad, dt(3), ws)
            w = [wk / ws for wk in w]
            pk = [w[k] / z[k] for k in range(3)]
            ps = pk[0] + pk[1] + pk[2]
            u = (pk[0] * uv[dv[:, 0], 0] + pk[1] * uv[dv[:, 1], 0] + pk[2] * uv[dv[:, 2], 0]) / ps
            v = (pk[0] * uv[dv[:, 0], 1] + pk[1] * uv[dv[:, 1], 1] + pk[2] * uv[dv[:, 2], 1]) / ps
        x, y = u * dt(T) - dt(0.5), v * dt(T) - dt(0.5)
        xf, yf = np.floor(x), np.floor(y)
        lx, ly = x - xf, y - yf
        j0, j1 = np.clip(xf, 0, T - 1).astype(np.int64), np.clip(xf + 1, 0, T - 1).astype(np.int64)
        i0, i1 = np.clip(yf, 0, T - 1).astype(np.int64), np.clip(yf + 1, 0, T - 1).astype(np.int64)
        part = tables['face_part'][f].astype(np.int64)
        chart = atlas[atlas_index[b]].reshape(PARTS * T * T, 4)
        ti = [part * T * T + i0 * T + j0, part * T * T + i0 * T + j1, part * T * T + i1 * T + j0, part * T * T + i1 * T + j1]
        tb = [(dt(1) - ly) * (dt(1) - lx), (dt(1) - ly) * lx, ly * (dt(1) - lx), ly * lx]
        num = np.zeros((f.size, 3), dtype)
        den = np.zeros(f.size, dtype)
        for q in range(4):
            tex = chart[ti[q]]
            ok = tex[:, 3] > 0
            for ch in range(3):
                num[:, ch] = np.where(ok, num[:, ch] + tb[q] * tex[:, ch].astype(dtype), num[:, ch])
            den = np.where(ok, den + tb[q], den)
        seen = den > 0
        with np.errstate(all='ignore'):
            for ch in range(3):
                rgb[b, ch][rr, cc] = np.where(seen, num[:, ch] / den, dt(np.float32(fill[ch])))
        alpha[b][rr, cc] = 1.0
        den_o[b][rr, cc] = den
        taps_o[b][rr, cc] = np.stack(ti, 1)
    return rgb, alpha, den_o, taps_o


# ---- the bounds the GPU tests share --------------------------------------------------------------------------------------------------
def tables():
    from danet_densepose2smpl_amd import texture
    return texture.atlas_tables(ico_densepose())


T_MAIN = 16


def unwrap_scene(name, dtype, T=T_MAIN):
    tb = tables()
    sc = scene(name)
    mf, mb = texture_map(tb, T)
    atlas, aux = texture_unwrap(tb, mf, mb, sc['images'], sc['vertices'], sc['cam'], sc['view_off'], dtype)
    return sc, mf, atlas, aux


def draw_scene(atlas32, sc, view, rot_y, dtype, images=None, atlas_index=0):
    """Draw view `view` of scene `sc` turned by rot_y with person `atlas_index`'s atlas."""
    tb = tables()
    rv = rotate_y(sc['vertices'][view:view + 1], rot_y)
    cam = sc['cam'][view:view + 1]
    fidx, _ = depth_planes(tb, rv, cam, H)
    out = texture_render(tb, rv, cam, fidx, atlas32, [atlas_index], None if images is None else images[view:view + 1], dtype=dtype)
    return out + (fidx,)


@functools.lru_cache(maxsize=None)
def bounds():
    """-> dict: DELTA (4 x the largest float32-vs-float64 difference of the oracle on the main scene over certain texels and pixels),
    ROUND (1.5 x the oracle's largest round-trip error), and the figures they come from."""
    sc, mf, a64, aux = unwrap_scene('main', np.float64)
    _, _, a32, _ = unwrap_scene('main', np.float32)
    unc = uncertain(aux, sc['view_off']).reshape(a64.shape[:4])
    cert = ~unc & (mf >= 0)[None]
    seen64, seen32 = a64[..., 3] > 0, a32[..., 3] > 0
    flips = int((cert & (seen64 != seen32)).sum())
    both = cert & seen64 & seen32
    d_col = float(np.abs(a64[..., :3] - a32[..., :3].astype(np.float64))[both].max())
    d_w = float((np.abs(a64[..., 3] - a32[..., 3].astype(np.float64)) / np.where(both, a64[..., 3], 1.0))[both].max())
    d_draw = 0.0
    at = a64.astype(np.float32)
    for rot in (0.0, math.radians(90)):
        r64, _, den, _, _ = draw_scene(at, sc, 0, rot, np.float64)
        r32, _, _, _, _ = draw_scene(at, sc, 0, rot, np.float32)
        ok = den >= EPS                                                     # (NaN where nothing is drawn: False)
        d_draw = max(d_draw, float(np.abs(r64 - r32.astype(np.float64))[:, :, ok[0]].max()))
    # round trip: the smooth image through one view and back
    rs, rmf, ra, _ = unwrap_scene('round', np.float64)
    rgb, _, _, taps, fidx = draw_scene(ra.astype(np.float32), rs, 0, 0.0, np.float64)
    mask = round_trip_mask(ra, rmf, taps, fidx)
    err = float(np.abs(rgb[0] - rs['images'][0].astype(np.float64))[:, mask[0]].max())
    return {'DELTA': 4.0 * max(d_col, d_draw), 'ROUND': 1.5 * err, 'd_col': d_col, 'd_w': d_w, 'd_draw': d_draw, 'flips': flips,
            'round_err': err, 'round_pixels': int(mask.sum())}


def round_trip_mask(atlas, map_face, taps, fidx):
    """[N,S,S] bool: pixels whose four taps are all observed and mapped to the pixel's own face."""
    w = atlas[0, ..., 3].reshape(-1)
    mf = map_face.reshape(-1)
    t = np.where(taps >= 0, taps, 0)
    return (fidx >= 0) & (w[t] > 0).all(-1) & (mf[t] == fidx[..., None]).all(-1)
