"""fp64 oracle of the 'iuv_gt' ground-truth part crops (csrc/part_gt.hip): part_iuv_simp + affine_grid + grid_sample (bilinear, zero
padding) of the 3-channel IUV image, and the gradient with respect to theta, written out tap by tap.

`coords(..., emulate_fp32=True)` reproduces the kernel's sampling coordinates bit for bit (sample_coord: every operation rounded to
fp32 on its own, no FMA); with emulate_fp32=False they are exact fp64 values, as torch's fp64 autograd computes them."""
import numpy as np
import torch

NJ, NC = 24, 7


def coords(theta, H, W, align, emulate_fp32):
    """theta [N,2,3] (fp32 values) -> xn [W], yn [H], ix, iy [N,H,W] (fp64 arrays holding fp32 values when emulate_fp32)."""
    th = np.asarray(theta, np.float32).reshape(-1, 6)
    if emulate_fp32:
        f = np.float32
        ow, oh = np.arange(W, dtype=f), np.arange(H, dtype=f)
        if align:
            xn = (f(-1) + (f(2) * ow) / f(W - 1)) if W > 1 else np.zeros(W, f)
            yn = (f(-1) + (f(2) * oh) / f(H - 1)) if H > 1 else np.zeros(H, f)
        else:
            xn = (f(2) * ow + f(1)) / f(W) - f(1)
            yn = (f(2) * oh + f(1)) / f(H) - f(1)
        t = [th[:, k].reshape(-1, 1, 1) for k in range(6)]
        X, Y = xn.reshape(1, 1, W), yn.reshape(1, H, 1)
        gx = (t[0] * X + t[1] * Y) + t[2]
        gy = (t[3] * X + t[4] * Y) + t[5]
        if align:
            ix, iy = (gx + f(1)) * f(0.5) * f(W - 1), (gy + f(1)) * f(0.5) * f(H - 1)
        else:
            ix, iy = ((gx + f(1)) * f(W) - f(1)) * f(0.5), ((gy + f(1)) * f(H) - f(1)) * f(0.5)
        return xn.astype(np.float64), yn.astype(np.float64), ix.astype(np.float64), iy.astype(np.float64)
    th = th.astype(np.float64)
    ow, oh = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    if align:
        xn, yn = -1 + 2 * ow / max(W - 1, 1), -1 + 2 * oh / max(H - 1, 1)
    else:
        xn, yn = (2 * ow + 1) / W - 1, (2 * oh + 1) / H - 1
    t = [th[:, k].reshape(-1, 1, 1) for k in range(6)]
    X, Y = xn.reshape(1, 1, W), yn.reshape(1, H, 1)
    gx, gy = t[0] * X + t[1] * Y + t[2], t[3] * X + t[4] * Y + t[5]
    if align:
        return xn, yn, (gx + 1) * 0.5 * (W - 1), (gy + 1) * 0.5 * (H - 1)
    return xn, yn, ((gx + 1) * W - 1) * 0.5, ((gy + 1) * H - 1) * 0.5


def simp_source(img, sel):
    """img [3,H,W] of one sample, sel [24,6] -> src [24,21,H,W] fp64 (part_iuv_simp: U | V | I of the 7 classes per joint)."""
    img = np.asarray(img, np.float64)
    part = np.clip(np.rint(img[0] * 24), 0, 24).astype(np.int64)
    sel = np.asarray(sel)
    src = np.zeros((NJ, 21) + part.shape)
    for j in range(NJ):
        anyp = np.zeros(part.shape, bool)
        for c in range(6):
            m = part == sel[j, c]
            anyp |= m
            src[j, 1 + c] = m * img[1]
            src[j, NC + 1 + c] = m * img[2]
            src[j, 2 * NC + 1 + c] = m
        src[j, 2 * NC] = ~anyp
    return src


def _taps(ix, iy, H, W):
    x0, y0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            wx = wx1 if dx else 1 - wx1
            wy = wy1 if dy else 1 - wy1
            idx = np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)
            out.append((ok, wx, wy, dx, dy, idx))
    return out


def forward_sample(img, theta_b, sel, keep_b=None, align=1, emulate_fp32=True):
    """One sample: img [3,H,W], theta_b [24,2,3], keep_b [24,7] or None -> (value [24,21,H,W], S [24,21,H,W] = sum over taps of
    |weight * source|, the scale of the fp32 rounding of the kernel's accumulation)."""
    H, W = img.shape[-2:]
    src = simp_source(img, sel).reshape(NJ, 21, H * W)
    _, _, ix, iy = coords(theta_b, H, W, align, emulate_fp32)
    val = np.zeros((NJ, 21, H, W))
    S = np.zeros_like(val)
    for ok, wx, wy, dx, dy, idx in _taps(ix, iy, H, W):
        w = np.where(ok, wx * wy, 0.0)                                              # [24,H,W]
        s = np.take_along_axis(src, idx.reshape(NJ, 1, H * W).repeat(21, 1), 2).reshape(NJ, 21, H, W)
        val += w[:, None] * s
        S += np.abs(w[:, None] * s)
    if keep_b is not None:
        k = np.repeat(np.asarray(keep_b, np.float64)[:, None, :], 3, 1).reshape(NJ, 21, 1, 1)
        val, S = val * k, S * np.abs(k)
    return val, S


def dtheta_sample(img, theta_b, sel, g, keep_b=None, align=1, emulate_fp32=False):
    """d theta [24,2,3] of sum(g * x24[..., :21]) for one sample, g [24,21,H,W] (fp64); also the per-entry magnitude sums the rounding
    bound needs: T [24,6] = sum over pixels of |term|, A [24,H,W] = sum over taps and channels of |k g src| (the size of gix / giy)."""
    H, W = img.shape[-2:]
    src = simp_source(img, sel).reshape(NJ, 21, H * W)
    xn, yn, ix, iy = coords(theta_b, H, W, align, emulate_fp32)
    g = np.asarray(g, np.float64)
    if keep_b is not None:
        g = g * np.repeat(np.asarray(keep_b, np.float64)[:, None, :], 3, 1).reshape(NJ, 21, 1, 1)
    gix = np.zeros((NJ, H, W))
    giy = np.zeros_like(gix)
    A = np.zeros_like(gix)
    for ok, wx, wy, dx, dy, idx in _taps(ix, iy, H, W):
        s = np.take_along_axis(src, idx.reshape(NJ, 1, H * W).repeat(21, 1), 2).reshape(NJ, 21, H, W)
        st = np.where(ok, (g * s).sum(1), 0.0)
        A += np.where(ok, np.abs(g * s).sum(1), 0.0)
        gix += (wy if dx else -wy) * st
        giy += (wx if dy else -wx) * st
    mx = 0.5 * (W - 1) if align else 0.5 * W
    my = 0.5 * (H - 1) if align else 0.5 * H
    ggx, ggy = gix * mx, giy * my
    X, Y = xn.reshape(1, 1, W), yn.reshape(1, H, 1)
    terms = [ggx * X, ggx * Y, ggx, ggy * X, ggy * Y, ggy]
    d = np.stack([t.sum((1, 2)) for t in terms], 1)
    T = np.stack([np.abs(t).sum((1, 2)) for t in terms], 1)
    return d.reshape(NJ, 2, 3), T, A * max(mx, my)


def torch_reference(img, theta, sel, keep=None, align=True):
    """The tensor-op statement (iuv_estimator.py:64-89) in whatever dtype the inputs have: [B,24,3,7,H,W], differentiable in theta."""
    import torch.nn.functional as F
    B, _, H, W = img.shape
    part = torch.round(img[:, 0] * 24).long().clamp(0, 24)
    I = F.one_hot(part, 25).permute(0, 3, 1, 2).to(img.dtype)
    U, V = I * img[:, 1:2], I * img[:, 2:3]
    s = torch.as_tensor(np.asarray(sel), dtype=torch.long)
    Us, Vs, Is = U[:, s], V[:, s], I[:, s]
    z = torch.zeros_like(Us[:, :, :1])
    bg = (Is.sum(2, keepdim=True) < 0.5).to(img.dtype)
    simp = torch.stack([torch.cat([z, Us], 2), torch.cat([z, Vs], 2), torch.cat([bg, Is], 2)], 2).reshape(B * NJ, 21, H, W)
    grid = F.affine_grid(theta.reshape(B * NJ, 2, 3), [B * NJ, 21, H, W], align_corners=align)
    out = F.grid_sample(simp, grid, mode='bilinear', padding_mode='zeros', align_corners=align).reshape(B, NJ, 3, NC, H, W)
    if keep is not None:
        out = out * keep.reshape(B, NJ, 1, NC, 1, 1)
    return out


def make_thetas(B, seed, general=True, outside=True):
    """Random crop thetas [B,24,2,3] fp32: scales 0.15..1.3, centres within +-0.95 (crops reach outside the image), and with `general`
    small off-diagonal terms so that all six entries matter."""
    g = torch.Generator().manual_seed(seed)
    s = 0.15 + 1.15 * torch.rand(B, NJ, generator=g)
    c = (torch.rand(B, NJ, 2, generator=g) * 2 - 1) * (0.95 if outside else 0.4)
    th = torch.zeros(B, NJ, 2, 3)
    th[..., 0, 0] = s * (1 + 0.2 * (torch.rand(B, NJ, generator=g) - 0.5))
    th[..., 1, 1] = s
    th[..., :, 2] = c
    if general:
        th[..., 0, 1] = 0.3 * (torch.rand(B, NJ, generator=g) - 0.5) * s
        th[..., 1, 0] = 0.3 * (torch.rand(B, NJ, generator=g) - 0.5) * s
    return th


def make_image(B, H, W, seed):
    """IUV image [B,3,H,W]: 4x4 blobs of one part id (0..24), U / V in [0,1) on the foreground."""
    g = torch.Generator().manual_seed(seed)
    part = torch.randint(0, 25, (B, (H + 3) // 4, (W + 3) // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W]
    part[:, :3] = 0
    uv = torch.rand(B, 2, H, W, generator=g) * (part > 0).unsqueeze(1)
    return torch.cat([(part.float() / 24).unsqueeze(1), uv], 1)


def tie_mask(theta, H, W, align, tol=1e-4):
    """[B,24,H,W] bool: pixels whose exact sampling coordinate lies within tol of an integer (where the bilinear gradient jumps)."""
    B = theta.shape[0]
    _, _, ix, iy = coords(theta.reshape(-1, 2, 3).numpy(), H, W, align, False)
    near = lambda v: np.abs(v - np.rint(v)) < tol          # noqa: E731
    return (near(ix) | near(iy)).reshape(B, NJ, H, W)
