"""Independent restatements for the visualisation ops (csrc/vis_ops.hip), in numpy: iuv_map2img, the shading rule of DESIGN.md
in double precision, a PNG decoder by hand, and the seeded inputs of golden g24 (the fixture stores their check sums and the
reference's outputs; the inputs come from numpy's frozen RandomState stream, so nothing large is committed)."""
import struct
import zlib

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- g24 inputs
def g24_global_inputs():
    """Case (a): raw global predictions, B = 4, 64 x 64, K = 25 and a 15-channel Ann, seeded normal values."""
    rs = np.random.RandomState(2401)
    U, V, I = (rs.standard_normal((4, 25, 64, 64)).astype(np.float32) for _ in range(3))
    A = rs.standard_normal((4, 15, 64, 64)).astype(np.float32)
    return U, V, I, A


def g24_part_inputs():
    """Case (c): the 24 partial maps, B = 2, K = 7, 32 x 32."""
    rs = np.random.RandomState(2403)
    return rs.standard_normal((2, 24, 3, 7, 32, 32)).astype(np.float32)


def crc(*arrays):
    """Check sum of the VALUES (a negative zero counts as zero)."""
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(np.asarray(a) + 0.0).tobytes(), c)
    return np.int64(c)


# ---------------------------------------------------------------------------------------------------------------- iuv_map2img
def iuv_map2img(U, V, I, A=None, ind_mapping=None):
    """[B,K,H,W] arrays -> [B,3,H,W] float32: the arg-max index (first maximum), gated by the Ann arg-max, scaled; U, V taken
    at that index."""
    K = I.shape[1]
    idx = np.argmax(I, axis=1)
    if A is not None:
        idx = idx * (np.argmax(A, axis=1) > 0)
    if ind_mapping is None:
        p0 = idx.astype(np.float32) / np.float32(K - 1)
    else:
        assert ind_mapping[0] == 0 and len(ind_mapping) == K
        p0 = np.array([m * (1. / 24.) for m in ind_mapping], dtype=np.float64).astype(np.float32)[idx]
    u = np.take_along_axis(U, idx[:, None], axis=1)[:, 0] * (idx >= 1)
    v = np.take_along_axis(V, idx[:, None], axis=1)[:, 0] * (idx >= 1)
    return np.stack([p0, u.astype(np.float32), v.astype(np.float32)], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- shading
def rotate_y(points, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.dot(points, np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]]))


LIGHTS = [((-200., -100., -100.), 1.0), ((800., 10., 300.), 1.0), ((-500., 500., 1000.), 0.7)]


def vertex_colors(verts, faces, color=None):
    """verts [V,3] float64 (already rotated), faces [F,3] -> [V,3]: area-weighted normals, three Lambertian point lights."""
    v = np.asarray(verts, np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    col = np.zeros_like(v)
    for pos, c in LIGHTS:
        lp = rotate_y(np.array(pos), np.radians(120.))
        d = lp[None] - v
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        lam = np.maximum(0.0, (n * d).sum(1))
        cc = np.full(3, c) if color is None else np.broadcast_to(np.asarray(color, np.float64), (3,))
        col += 0.9 * cc[None] * lam[:, None]
    return col


def shade(verts, cam, faces, fidx, images=None, rot_y=0., focal=5000., res=224, color=None):
    """fp64 shaded view given the device's face-index plane fidx [B,R,R] (indices into faces + reversed faces).
    verts [B,V,3] float32, cam [B,3] float32 -> (rgb [B,3,R,R], alpha [B,R,R]) float64."""
    B, R = fidx.shape[0], res
    faces = np.asarray(faces).astype(np.int64)
    f2 = np.concatenate([faces, faces[:, ::-1]], 0)
    fx = focal * (R / 224.) if R != 224 else focal
    cx = (R / 2.) * (R / 224.) if R != 224 else R / 2.
    rgb = np.zeros((B, 3, R, R)) if images is None else np.asarray(images, np.float64).copy()
    alpha = np.zeros((B, R, R))
    rows, cols = np.meshgrid(np.arange(R), np.arange(R), indexing='ij')
    xp = (2. * cols + 1. - R) / R
    yp = (R - 1. - 2. * rows) / R
    for b in range(B):
        c32, s32 = np.float32(np.cos(rot_y)), np.float32(np.sin(rot_y))
        v32 = np.asarray(verts[b], np.float32)
        # the rotation is part of the input side of the rule: one binary32 operation each, as the kernel states it
        v = np.stack([v32[:, 0] * c32 - v32[:, 2] * s32, v32[:, 1], v32[:, 0] * s32 + v32[:, 2] * c32], 1).astype(np.float64)
        col = vertex_colors(v, faces, color)
        s, tx, ty = (np.float64(x) for x in cam[b])
        tz = 2. * focal / (R * s + 1e-9)
        p = v + np.array([tx, ty, tz])
        z = p[:, 2]
        u = 2. * (fx * p[:, 0] / (z + 1e-9) + cx - R / 2.) / R
        w = 2. * ((R - (fx * p[:, 1] / (z + 1e-9) + cx)) - R / 2.) / R
        m = fidx[b] >= 0
        tri = f2[fidx[b][m]]
        X, Y = xp[m], yp[m]
        x0, x1, x2 = (u[tri[:, k]] - X for k in range(3))
        y0, y1, y2 = (w[tri[:, k]] - Y for k in range(3))
        e = np.stack([x1 * y2 - y1 * x2, x2 * y0 - y2 * x0, x0 * y1 - y0 * x1], 1)
        bw = np.clip(e / e.sum(1, keepdims=True), 0., 1.)
        bw = bw / bw.sum(1, keepdims=True)
        pw = bw / z[tri]
        pw = pw / pw.sum(1, keepdims=True)
        pix = np.clip((pw[:, :, None] * col[tri]).sum(1), 0., 1.)
        for ch in range(3):
            rgb[b, ch][m] = pix[:, ch]
        alpha[b][m] = 1.
    return rgb, alpha


# ---------------------------------------------------------------------------------------------------------------- PNG
def png_decode(data):
    """8-bit RGB / RGBA, non-interlaced PNG bytes -> uint8 [H,W,C]; every filter type."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, typ = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(typ + body) & 0xffffffff), typ
        if typ == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif typ == b'IDAT':
            idat += body
        pos += 12 + n
    W, H, depth, ctype, comp, filt, inter = hdr
    assert depth == 8 and ctype in (2, 6) and (comp, filt, inter) == (0, 0, 0), hdr
    C = 3 if ctype == 2 else 4
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * C)
    out = np.zeros((H, W * C), np.int64)
    for y in range(H):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(W * C, np.int64)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) & 255
        else:
            for x in range(W * C):
                a = out[y, x - C] if x >= C else 0
                c = up[x - C] if x >= C else 0
                b = up[x]
                if f == 1:
                    pr = a
                elif f == 3:
                    pr = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pr = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                out[y, x] = (line[x] + pr) & 255
    return out.astype(np.uint8).reshape(H, W, C)
