"""numpy restatement of the sheet rule, the overlay and the marker rule of DESIGN.md 4e (training visualisation), written from
those rules.  The yardstick of tests/test_gpu_train_vis.py; every float operation is one float32 operation in the order the
rule names it."""
import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 3, 1, 1)


def grid_size(n, H, W, nrow, padding):
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def denormalize(x):
    return (x.astype(np.float32) * STD + MEAN).astype(np.float32)


def overlay(images, iuv):
    """img[up(iuv) > 0] = up(iuv)[up(iuv) > 0], up = nearest by the integer factor H / h; per element."""
    H, h = images.shape[-1], iuv.shape[-1]
    if H % h:
        raise ValueError('the factor %d / %d is not an integer' % (H, h))
    up = np.repeat(np.repeat(iuv.astype(np.float32), H // h, axis=2), H // h, axis=3)
    out = images.astype(np.float32).copy()
    out[up > 0] = up[up > 0]
    return out


def normalize(x):
    """(x - lo) / (hi - lo + 1e-5) clamped to [0, 1]; lo, hi over the whole batch."""
    x = x.astype(np.float32)
    lo, hi = x.min(), x.max()
    den = np.float32(np.float32(hi - lo) + np.float32(1e-5))
    return np.clip((x - lo) / den, np.float32(0), np.float32(1)).astype(np.float32)


def make_grid(t, nrow=8, padding=2, pad_value=0.):
    """[B,C,H,W] (C = 1 or 3) -> [3,Hs,Ws] float32."""
    t = np.asarray(t, np.float32)
    B, C, H, W = t.shape
    if C == 1:
        t = np.repeat(t, 3, axis=1)
    xmaps = min(nrow, B)
    Hs, Ws = grid_size(B, H, W, nrow, padding)
    sheet = np.full((3, Hs, Ws), pad_value, np.float32)
    for k in range(B):
        r, c = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        sheet[:, r:r + H, c:c + W] = t[k]
    return sheet


def pair_grid(a, b):
    both = np.stack([np.asarray(a, np.float32), np.asarray(b, np.float32)], axis=1).reshape((-1,) + tuple(a.shape[1:]))
    return make_grid(both, nrow=2, padding=2, pad_value=0.)


def marker_pixels(B, H, W, joints, vis=None, nrow=8, padding=1):
    """{(y, x): joint index j} of the markers on the sheet of B tiles of H x W, the later (tile, joint) winning."""
    xmaps = min(nrow, B)
    Hs, Ws = grid_size(B, H, W, nrow, padding)
    joints = np.asarray(joints, np.float32)
    out = {}
    for k in range(B):
        ox, oy = (k % xmaps) * (W + padding) + padding, (k // xmaps) * (H + padding) + padding
        for j in range(joints.shape[1]):
            if vis is not None and float(np.asarray(vis).reshape(B, -1)[k, j]) == 0:
                continue
            fx, fy = np.float32(ox) + joints[k, j, 0], np.float32(oy) + joints[k, j, 1]
            if not (np.isfinite(fx) and np.isfinite(fy)):
                continue
            cx, cy = int(fx), int(fy)                                # truncation toward zero
            for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
                x, y = cx + dx, cy + dy
                if 0 <= x < Ws and 0 <= y < Hs:
                    out[(y, x)] = j
    return out


def draw_joints(sheet, B, H, W, joints, vis=None, nrow=8, padding=1):
    """-> a copy of the [3,Hs,Ws] sheet with the markers: even joints (0, 1, 0), odd joints (1, 0, 0)."""
    out = np.array(sheet, np.float32, copy=True)
    for (y, x), j in marker_pixels(B, H, W, joints, vis, nrow, padding).items():
        out[:, y, x] = (1, 0, 0) if j % 2 else (0, 1, 0)
    return out


def to_uint8(sheet):
    """mul(255).clamp(0, 255).byte(): truncation."""
    return np.clip(np.asarray(sheet, np.float32) * np.float32(255), 0, 255).astype(np.uint8)


def png_decode(data):
    """An 8-bit RGB / RGBA, non-interlaced PNG whose lines all have filter type 0 -> uint8 [H,W,C] (zlib + struct)."""
    import struct
    import zlib
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, idat, head = 8, b'', None
    while at < len(data):
        n, typ = struct.unpack('>I', data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(typ + body) & 0xffffffff
        if typ == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif typ == b'IDAT':
            idat += body
        at += 12 + n
    W, H, depth, colour, _, _, interlace = head
    assert depth == 8 and colour in (2, 6) and interlace == 0
    C = 3 if colour == 2 else 4
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * C)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, C).copy()
