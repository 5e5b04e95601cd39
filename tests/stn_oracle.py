"""The joint-centric part gather (csrc/stn.hip) restated in numpy float64 from the definition of affine_grid + grid_sample
(bilinear, zero padding, both align_corners modes), for the tests: forward, its exact transpose, and the candidate sums the
backward's error bound needs.  Layouts are the kernels': x [B,H,W,C], theta [B,P,2,3], y [B,OH,OW,P*C] with channel p*C + c.

Definition.  Output pixel o of n has the normalised coordinate
    align_corners:      -1 + 2 o / (n - 1)        (0 when n == 1)
    otherwise:          (2 o + 1) / n - 1
the grid point is theta . (xn, yn, 1), and a normalised g maps to the pixel coordinate
    align_corners:      (g + 1) / 2 * (size - 1)
    otherwise:          ((g + 1) * size - 1) / 2
x along W, y along H.  The sample is the bilinear mix of the four pixels around it; a pixel outside the map counts as 0.

Thetas are taken as the float32 values the kernel sees and widened; every coordinate after that is float64."""
import numpy as np


def _norm(n, align):
    o = np.arange(n, dtype=np.float64)
    if align:
        return -1.0 + 2.0 * o / (n - 1) if n > 1 else np.zeros(1)
    return (2.0 * o + 1.0) / n - 1.0


def _unnorm(g, size, align):
    return (g + 1.0) / 2.0 * (size - 1) if align else ((g + 1.0) * size - 1.0) / 2.0


def coords(theta, H, W, OH, OW, align):
    """Sample positions (ix along W, iy along H) in pixels, each [B,P,OH,OW] float64."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    xn = _norm(OW, align)[None, None, None, :]
    yn = _norm(OH, align)[None, None, :, None]
    t = th[:, :, :, :, None, None]
    gx = t[:, :, 0, 0] * xn + t[:, :, 0, 1] * yn + t[:, :, 0, 2]
    gy = t[:, :, 1, 0] * xn + t[:, :, 1, 1] * yn + t[:, :, 1, 2]
    return _unnorm(gx, W, align), _unnorm(gy, H, align)


def _taps(ix, iy, H, W):
    """The four corners of every sample: (yy, xx, weight); a corner outside the map gets weight 0 and clipped indices."""
    x0, y0 = np.floor(ix), np.floor(iy)
    fx, fy = ix - x0, iy - y0
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            yy, xx = y0 + dy, x0 + dx
            inside = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            yield (np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, W - 1).astype(np.int64), np.where(inside, wy * wx, 0.0))


def forward(x, theta, OH, OW, align):
    """x [B,H,W,C], theta [B,P,2,3] (any 2 x 3 matrices, shear included) -> y [B,OH,OW,P*C] float64."""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    P = np.asarray(theta).shape[1]
    ix, iy = coords(theta, H, W, OH, OW, align)
    y = np.zeros((B, P, OH, OW, C))
    bi = np.arange(B)[:, None, None, None]
    for yy, xx, w in _taps(ix, iy, H, W):
        y += w[..., None] * x[bi, yy, xx]
    return np.ascontiguousarray(y.transpose(0, 2, 3, 1, 4)).reshape(B, OH, OW, P * C)


def backward(gy, theta, H, W, align):
    """gy [B,OH,OW,P*C] -> dx [B,H,W,C]: the transpose of forward(), as a scatter-add in float64."""
    gy = np.asarray(gy, dtype=np.float64)
    B, OH, OW, PC = gy.shape
    P = np.asarray(theta).shape[1]
    C = PC // P
    ix, iy = coords(theta, H, W, OH, OW, align)
    g = gy.reshape(B, OH * OW, P, C)
    dx = np.zeros((B, H * W, C))
    for yy, xx, w in _taps(ix, iy, H, W):
        flat = (yy * W + xx).reshape(B, P, OH * OW)
        w = w.reshape(B, P, OH * OW)
        for b in range(B):
            for p in range(P):
                np.add.at(dx[b], flat[b, p], w[b, p][:, None] * g[b, :, p])
    return dx.reshape(B, H, W, C)


def candidates(absgy, theta, H, W, align, delta):
    """T [B,H,W,C]: the sum of absgy over every (p, oh, ow) whose sample position lies within 1 + delta of the pixel on both
    axes (indicator weights): everything a coordinate error of delta can move into or inside a pixel's tent."""
    g = np.asarray(absgy, dtype=np.float64)
    B, OH, OW, PC = g.shape
    P = np.asarray(theta).shape[1]
    C = PC // P
    ix, iy = coords(theta, H, W, OH, OW, align)
    g = g.reshape(B, OH * OW, P, C)
    T = np.zeros((B, H * W, C))
    ws, hs = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    for b in range(B):
        for p in range(P):
            ax = np.abs(ix[b, p].reshape(-1, 1) - ws) <= 1.0 + delta          # [n, W]
            ay = np.abs(iy[b, p].reshape(-1, 1) - hs) <= 1.0 + delta          # [n, H]
            near = (ay[:, :, None] & ax[:, None, :]).reshape(-1, H * W).astype(np.float64)
            T[b] += near.T @ g[b, :, p]
    return T.reshape(B, H, W, C)


# ---------------------------------------------------------------------------------------------------------------- the cases
# (B, P, C, H, W, OH, OW): each exists for the branch of csrc/stn.hip it reaches
SHAPES = {
    'pc1': (2, 1, 8, 12, 20, 12, 20),          # PC == 1 (dq = 256, dr = 0), H != W
    'pc288': (2, 24, 96, 8, 8, 8, 8),          # PC = 288 > 256 (dq == 0)
    'out_hw': (3, 5, 48, 16, 16, 8, 24),       # out_hw differs on both axes, CV = 6, row length not a multiple of 256
    'oh1': (2, 3, 16, 9, 7, 1, 5),             # OH == 1: zero slope, norm_coord with n = 1
    'ow1': (2, 3, 16, 9, 7, 5, 1),             # OW == 1
    'lanes': (1, 2, 256, 3, 33, 3, 33),        # backward W * CV = 1056 > 1024: the lanes loop
    'idle': (2, 3, 40, 6, 13, 6, 13),          # 65 items, 128 threads: idle lanes
    'prod': (2, 24, 48, 32, 32, 32, 32),       # the production geometry at a quarter of its size
}
KINDS = ('random', 'flipped', 'sx0_inside', 'sx0_outside', 'tiny', 'large', 'far', 'identity')
EMPTY_KINDS = ('sx0_outside', 'far')           # no sample touches the map: y and the part's share of dx are exact zeros


def thetas(B, P, seed, phase=0):
    """Axis-aligned thetas [B,P,2,3] float32, a different one for every (b, p), and the kind of each: slot b * P + p takes
    KINDS[(slot + phase) % 8].  Every |centre| + |scale| <= 8."""
    rs = np.random.RandomState(seed)
    th = np.zeros((B, P, 2, 3), dtype=np.float64)
    kinds = []
    for b in range(B):
        for p in range(P):
            k = KINDS[(b * P + p + phase) % len(KINDS)]
            sx, sy = rs.uniform(0.05, 1.0, 2)
            cx, cy = rs.uniform(-0.8, 0.8, 2)
            sgn = 1.0 if rs.rand() < 0.5 else -1.0
            if k == 'flipped':
                sx, sy = -sx, sy * sgn
            elif k == 'sx0_inside':
                sx = 0.0
            elif k == 'sx0_outside':
                sx, cx = 0.0, sgn * rs.uniform(1.5, 2.0)
            elif k == 'tiny':
                sx = sy = 1e-4
            elif k == 'large':
                sx = sy = 3.0
                cx, cy = cx * 0.5, cy * 0.5
            elif k == 'far':
                if sgn > 0:
                    cx = 5.0
                else:
                    cy = 5.0
            elif k == 'identity':
                sx = sy = 1.0
                cx = cy = 0.0
            th[b, p] = [[sx, 0.0, cx], [0.0, sy, cy]]
            kinds.append(k)
    return th.astype(np.float32), np.array(kinds).reshape(B, P)


def sheared_thetas(B, P, seed):
    """General 2 x 3 thetas (th[0][1], th[1][0] != 0) for the forward, which implements them."""
    rs = np.random.RandomState(seed)
    th = rs.uniform(-1.0, 1.0, (B, P, 2, 3))
    th[:, :, :, 2] *= 0.8
    th[:, :, 0, 1] = np.where(np.abs(th[:, :, 0, 1]) < 0.1, 0.3, th[:, :, 0, 1])
    th[:, :, 1, 0] = np.where(np.abs(th[:, :, 1, 0]) < 0.1, -0.3, th[:, :, 1, 0])
    return th.astype(np.float32)
