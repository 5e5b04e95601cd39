"""Wrappers over the C ABI (include/danet_hip.h): the SMPL forward and the rotation conversions as torch.autograd.Functions, and the
forward-only ops -- rasteriser, decode and shading, sheets and markers, pose / vertex / segmentation / COCO scoring, crop and label
augmentation, scene and texture.  Every entry refuses a CPU tensor before the library is loaded; the argument rules are stated once."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr, check, stream, require_gpu, f32c as _f32c, dev_tensor as _dev_tensor


# ---- argument rules ------------------------------------------------------------------------------------------------------------
def _shape(t, shape, what):
    """`t` unless its shape misses the pattern `shape` (None matches any extent; shape None: anything goes)."""
    if shape is not None and (t.dim() != len(shape) or any(e is not None and e != g for e, g in zip(shape, t.shape))):
        raise ValueError('%s: shape %s, expected [%s]' % (what, tuple(t.shape), ','.join('*' if e is None else str(e) for e in shape)))
    return t


def _f32(t, shape, what, optional=False):
    """A GPU tensor of any dtype and strides -> its detached, contiguous fp32 form, of the shape pattern `shape`."""
    if t is None and optional:
        return None
    return _shape(_f32c(_dev_tensor(t, what)), shape, what)


def _typed(t, dtype, shape, what):
    """A GPU tensor that already has the dtype, shape and contiguity the kernel reads: nothing is converted."""
    t = _dev_tensor(t, what)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous %s %s tensor, got %s %s' % (what, dtype, tuple(shape), t.dtype, tuple(t.shape)))
    return t


def _out(out, dtype, shape, device, what):
    """`out` itself (checked), or a new tensor."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    _typed(out, dtype, shape, what)
    return out


def _packed_u8(src, what):
    s = _dev_tensor(src, what)
    if s.dtype != torch.uint8 or s.dim() != 1 or s.numel() == 0:
        raise ValueError('%s: one packed, non-empty uint8 buffer expected' % what)
    return s


def _strided(tensors, what, rank, slots):
    """Sources the kernel reads through their strides (nothing is copied): -> (the tensors in ONE dtype, fp32 unless all are bf16;
    their strides as c_int64[slots * rank], zero-padded; the dtype flag, 0 = fp32, 1 = bf16)."""
    ts = [_dev_tensor(t, what) for t in tensors]
    dt = ts[0].dtype
    if dt not in (torch.float32, torch.bfloat16) or any(t.dtype != dt for t in ts):
        ts, dt = [t.to(torch.float32) for t in ts], torch.float32
    if any(t.dim() != rank for t in ts):
        raise ValueError('%s: sources of rank %d expected, got %s' % (what, rank, [tuple(t.shape) for t in ts]))
    strides = [st for t in ts for st in t.stride()]
    return ts, (ctypes.c_int64 * (slots * rank))(*(strides + [0] * (slots * rank - len(strides)))), 0 if dt == torch.float32 else 1


def _draw_buffers(images, N, S, device, what):
    """What a draw over optional background images [N,3,S,S] takes: (the images in fp32 or None, new rgb [N,3,S,S], alpha [N,S,S])."""
    return (_f32(images, (N, 3, S, S), what + ': images', optional=True), torch.empty(N, 3, S, S, device=device, dtype=torch.float32),
            torch.empty(N, S, S, device=device, dtype=torch.float32))


def _ascending(off, n, what, integers=False):
    """A host array of offsets that ascend (not strictly) from 0 to n; `integers`: a float array is refused too."""
    off = np.asarray(off).reshape(-1)
    if off.size < 2 or (integers and not np.issubdtype(off.dtype, np.integer)) or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError('%s must ascend from 0 to %d%s, got %s' % (what, n, ' in integers' if integers else '', off.tolist()))
    return off


def _host_i32(a):
    """A host array as the `const int32_t*` argument of an entry point (the pointer keeps the array alive)."""
    return np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _int(v, what, name, low=None, high=None):
    """`v` as an int where it is a whole number (3, 3.0, np.int64(3)) inside [low, high]; a bool is refused."""
    if isinstance(v, bool) or int(v) != v or (low is not None and v < low) or (high is not None and v > high):
        bound = '' if low is None and high is None else ' >= %d' % low if high is None else ' <= %d' % high if low is None \
            else ' in %d..%d' % (low, high)
        raise ValueError('%s: %s %r (an integer%s)' % (what, name, v, bound))
    return int(v)


def _device_key(device):
    """(type, index) of a device; a CUDA device without an index is the current one, any other device never asks torch.cuda."""
    device = torch.device(device)
    return device.type, torch.cuda.current_device() if device.index is None and device.type == 'cuda' else device.index


def _per_device(cache, device, make):
    """cache[_device_key(device)], made by make() at the first call and kept: no upload inside a captured region afterwards."""
    key = _device_key(device)
    if key not in cache:
        cache[key] = make()
    return cache[key]


def _host_i64(a):
    return np.ascontiguousarray(a, np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _workspace(nbytes, device, dtype=torch.int64, spare=1):
    """At least `nbytes` of scratch in whole elements of `dtype`, plus `spare` elements."""
    return torch.empty(-(-nbytes // dtype.itemsize) + spare, device=device, dtype=dtype)


LBS_ONE_LAUNCH = True       # the SMPL forward as one kernel launch (csrc/smpl_lbs.hip smpl_fused_fwd_kernel); False: prep -> main -> finalize
_LBS_TICKETS = {}
SMPL_BWD_FUSED = bool(int(os.environ.get('DANET_LBS_BWD_FUSED', '0')))    # the SMPL backward as ONE launch (smpl_fused_bwd_kernel); default: three launches (faster)


def lbs_ticket(device, words):
    """The fused forward's arrival counters: zeroed once, then owned (and reset) by the launches on ONE stream -- a buffer
    per (device, stream), so launches that could overlap never share one."""
    if not LBS_ONE_LAUNCH or device.type != 'cuda':          # (CPU tensors: the C-ABI call below refuses them)
        return None
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    t = _LBS_TICKETS.get(key)
    if t is None or t.numel() < words:
        with torch.cuda.device(key[0]):
            t = _LBS_TICKETS[key] = torch.zeros(max(1024, int(words)), dtype=torch.int32, device=device)
    return t


class SmplLbsFunction(torch.autograd.Function):
    """(betas [B,NB], rotmats [B,24,3,3], model buffers) -> (vertices [B,V,3], joints54 [B,54,3]).
    Gradients flow to betas and rotmats (/root/reference/models/danet/smpl_regressor.py:176)."""

    @staticmethod
    def forward(ctx, betas, rotmats, m):
        require_gpu(betas, 'smpl_lbs')
        L = _lib.lib()
        betas_c, rot_c = _f32c(betas), _f32c(rotmats).view(-1, 24, 3, 3)
        B, NB = betas_c.shape
        V = m.v_template.shape[0]
        NL, NE = m.landmark_verts.numel(), m.J_regressor_extra.shape[0]
        dev = betas_c.device
        need_grad = betas.requires_grad or rotmats.requires_grad
        verts = torch.empty(B, V, 3, device=dev, dtype=torch.float32)
        j54 = torch.empty(B, 24 + NL + NE, 3, device=dev, dtype=torch.float32)
        cbuf = torch.empty(L.danet_smpl_lbs_ctx_floats(B), device=dev, dtype=torch.float32)
        vposed = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if need_grad else None
        nws = L.danet_smpl_lbs_fwd_ws_floats(B, V, NE)
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        ticket = lbs_ticket(dev, L.danet_smpl_lbs_ticket_words(B))
        check(L.danet_smpl_lbs_forward(
            ptr(betas_c), ptr(rot_c), B, ptr(m.v_template), ptr(m.shapedirs), ptr(m.posedirs),
            ptr(m.J_template), ptr(m.J_shapedirs), ptr(m.lbs_weights), ptr(m.parents),
            ptr(m.J_regressor_extra), ptr(m.landmark_verts), V, NB, NL, NE,
            ptr(verts), ptr(j54), ptr(cbuf), ptr(vposed), ptr(ws), nws, ptr(ticket), stream()), 'danet_smpl_lbs_forward')
        if need_grad:
            ctx.m = m
            ctx.save_for_backward(betas_c, rot_c, cbuf, vposed)
        return verts, j54

    @staticmethod
    def backward(ctx, g_verts, g_j54):
        L = _lib.lib()
        m = ctx.m
        betas_c, rot_c, cbuf, vposed = ctx.saved_tensors
        B, NB = betas_c.shape
        V = m.v_template.shape[0]
        NL, NE = m.landmark_verts.numel(), m.J_regressor_extra.shape[0]
        dev = betas_c.device
        gv = None if g_verts is None else _f32c(g_verts)
        gj = None if g_j54 is None else _f32c(g_j54)
        g_betas = torch.empty(B, NB, device=dev, dtype=torch.float32)
        g_rot = torch.empty(B, 24, 3, 3, device=dev, dtype=torch.float32)
        nws = L.danet_smpl_lbs_bwd_ws_floats(B, V, NB)
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        # Three launches by default (126 us at B = 32 against 150 for the one-launch form, bench.py roofline_extra of round 5; neutral in
        # the step).  SMPL_BWD_FUSED: ONE launch when the grid fits the co-residency budget; the barrier state is the one-pass BatchNorm
        # backward's (same stream, never concurrent; its error word guards the optimizer step inside a Trainer -- outside one nothing
        # reads it, which is why the one-launch form is opt-in)
        from . import nn as _nn, conv as _conv
        bar = _nn._onepass_bar(dev) if SMPL_BWD_FUSED else None
        if bar is not None and L.danet_smpl_lbs_backward_fused_ok(B, V, _nn.onepass_budget(dev)):
            _conv.FUSION['smpl_bwd_fused'] += 1
        else:
            bar = None
        check(L.danet_smpl_lbs_backward(
            ptr(betas_c), ptr(rot_c), B, ptr(m.shapedirs), ptr(m.posedirs), ptr(m.J_shapedirs),
            ptr(m.lbs_weights), ptr(m.parents), ptr(m.J_regressor_extra), ptr(m.landmark_verts),
            V, NB, NL, NE, ptr(cbuf), ptr(vposed), ptr(gv), ptr(gj), ptr(g_betas), ptr(g_rot),
            ptr(ws), nws, ptr(bar), int(_nn.onepass_budget(dev)), stream()), 'danet_smpl_lbs_backward')
        return g_betas, g_rot, None


class SmplJointsFunction(torch.autograd.Function):
    """joints54 [B,54,3] -> (joints49 = j54[:, map49], joints_J19 = joints49[:, -24:][:, map19], smpl_joints = j54[:, :24]) in one launch,
    and their three gradients back into one (/root/reference/models/smpl.py:31-37: three index ops, their scatters and two accumulations)."""

    @staticmethod
    def forward(ctx, j54, map49, map19):
        require_gpu(j54, 'smpl_joints')
        L = _lib.lib()
        j = _f32c(j54)
        B, NJ = j.shape[0], j.shape[1]
        N49, N19 = map49.numel(), map19.numel()
        j49 = torch.empty(B, N49, 3, device=j.device, dtype=torch.float32)
        j19 = torch.empty(B, N19, 3, device=j.device, dtype=torch.float32)
        j24 = torch.empty(B, 24, 3, device=j.device, dtype=torch.float32)
        check(L.danet_smpl_joints_forward(ptr(j), ptr(map49), ptr(map19), B, NJ, N49, N19, ptr(j49), ptr(j19), ptr(j24), stream()), 'danet_smpl_joints_forward')
        ctx.maps = (map49, map19, B, NJ, N49, N19)
        ctx.set_materialize_grads(False)
        return j49, j19, j24

    @staticmethod
    def backward(ctx, g49, g19, g24):
        L = _lib.lib()
        map49, map19, B, NJ, N49, N19 = ctx.maps
        if g49 is None and g19 is None and g24 is None:
            return None, None, None
        f = lambda g: None if g is None else _f32c(g)      # noqa: E731
        g49, g19, g24 = f(g49), f(g19), f(g24)
        g54 = torch.empty(B, NJ, 3, device=map49.device, dtype=torch.float32)
        check(L.danet_smpl_joints_backward(ptr(g49), ptr(g19), ptr(g24), ptr(map49), ptr(map19), B, NJ, N49, N19, ptr(g54), stream()), 'danet_smpl_joints_backward')
        return g54, None, None


def smpl_joints(j54, map49, map19):
    return SmplJointsFunction.apply(j54, map49, map19)


def smpl_lbs(betas, rotmats, model):
    return SmplLbsFunction.apply(betas, rotmats, model)


def iuv_raster(verts, cam, vert_mapping, faces, tex, focal, orig, out_size, return_aux=False):
    """Forward-only (labels are rendered from detached meshes, danet.py:163-165)."""
    require_gpu(verts, 'iuv_raster')
    L = _lib.lib()
    v, c = _f32c(verts), _f32c(cam)
    B, NV = v.shape[0], v.shape[1]
    S = int(out_size)
    out = torch.empty(B, 3, S, S, device=v.device, dtype=torch.float32)
    fidx = torch.empty(B, S, S, device=v.device, dtype=torch.int32) if return_aux else None
    depth = torch.empty(B, S, S, device=v.device, dtype=torch.float32) if return_aux else None
    nws = L.danet_iuv_raster_ws_bytes(B, vert_mapping.numel(), S)
    ws = _workspace(nws, v.device)
    check(L.danet_iuv_raster_forward(ptr(v), ptr(c), B, NV, ptr(vert_mapping), vert_mapping.numel(),
                                     ptr(faces), ptr(tex), faces.shape[0], float(focal), float(orig), S,
                                     ptr(out), ptr(fidx), ptr(depth), ptr(ws), nws, stream()), 'danet_iuv_raster_forward')
    return (out, fidx, depth) if return_aux else out


def iuv_map2img(U, V, I, A=None, table=None):
    """The decode kernel behind iuvmap.iuv_map2img / part_iuv_map2img (csrc/vis_ops.hip), one launch.  U, V, I: [N,K,H,W] or
    [B,J,K,H,W] fp32 / bf16 with any strides (they are passed on, nothing is copied); A: [N,KA,H,W] or None; table: device
    [J,K] f32 or None.  -> [N,3,H,W] / [B,J,3,H,W] f32."""
    srcs = [t for t in (U, V, I, A) if t is not None]
    for t in srcs:
        require_gpu(t, 'iuv_map2img')
    five = srcs[0].dim() == 5
    ts, strides, bf16 = _strided(srcs if five else [t.unsqueeze(1) for t in srcs], 'iuv_map2img', 5, 4)
    for t in ts[1:3]:
        _shape(t, tuple(ts[0].shape), 'iuv_map2img: V / Index (as U)')
    NB, J, K, H, W = ts[0].shape
    KA = 0 if A is None else _shape(ts[3], (NB, J, None, H, W), 'iuv_map2img: AnnIndex').shape[2]
    if table is not None:
        _typed(table, torch.float32, (J, K), 'iuv_map2img: table')
    out = torch.empty(NB * J, 3, H, W, device=ts[0].device, dtype=torch.float32)
    check(_lib.lib().danet_iuv_map2img_forward(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), None if A is None else ts[3].data_ptr(),
                                               strides, NB, J, K, KA, H, W, bf16, ptr(table), ptr(out), stream()), 'danet_iuv_map2img_forward')
    return out.view(NB, J, 3, H, W) if five else out


def mesh_shade_views(ws, B, V):
    """The two halves of mesh_shade_vertices' workspace as views: (rotated vertices [B,V,3], vertex colours [B,V,3])."""
    n = B * V * 3
    return ws[:n].view(B, V, 3), ws[n:2 * n].view(B, V, 3)


def mesh_shade_vertices(verts, faces, csr_off, csr_face, lights, rot_y=0., albedo=0.9):
    """verts [B,V,3] -> workspace holding the vertices multiplied by rotateY(rot_y) and their colours (DESIGN.md shading rule);
    `lights`: 18 host floats (3 positions, 3 colours).  Returns (ws, rotated vertices [B,V,3] -- a view of ws)."""
    v = _f32(verts, (None, None, 3), 'mesh_shade: verts')
    B, V = v.shape[0], v.shape[1]
    L = _lib.lib()
    nws = L.danet_mesh_shade_ws_bytes(B, V)
    ws = _workspace(nws, v.device, torch.float32, spare=0)                  # (also the result: exactly the two halves)
    lt = (ctypes.c_float * 18)(*[float(x) for x in lights])
    check(L.danet_mesh_shade_vertices(ptr(v), B, V, ptr(faces), faces.shape[0], ptr(csr_off), ptr(csr_face), lt,
                                      float(math.cos(rot_y)), float(math.sin(rot_y)), float(albedo), ptr(ws), nws, stream()),
          'danet_mesh_shade_vertices')
    return ws, mesh_shade_views(ws, B, V)[0]


def mesh_shade_pixels(ws, cam, V, faces2, fidx, images, focal, orig):
    """The colours of mesh_shade_vertices mixed over the rasteriser's face-index plane fidx [B,S,S] -> (rgb [B,3,S,S], alpha [B,S,S])."""
    c = _f32(cam, None, 'mesh_shade: cam')
    B, S = fidx.shape[0], fidx.shape[-1]
    img, rgb, alpha = _draw_buffers(images, B, S, c.device, 'mesh_shade')
    check(_lib.lib().danet_mesh_shade_pixels(ptr(ws), ptr(c), B, V, ptr(faces2), faces2.shape[0], ptr(fidx), ptr(img), float(focal), float(orig), S,
                                             ptr(rgb), ptr(alpha), stream()), 'danet_mesh_shade_pixels')
    return rgb, alpha


def demo_compose(images, glob, part, riuv, mesh=None, side=None, side_alpha=None):
    """The result panels of demo.py:115-177 in one launch -> [B, S, 4.5 S (6.5 S with the mesh panels), 4] f32 RGBA."""
    img = _f32(images, (None, 3, None, None), 'demo_compose: images')
    B, _, S, _ = img.shape
    hm = S // 4
    if img.shape[3] != S or 4 * hm != S:
        raise ValueError('demo_compose: images %s, expected square with a side of four heat-maps' % (tuple(img.shape),))
    three = [mesh, side, side_alpha]
    if any(t is None for t in three) != all(t is None for t in three):
        raise ValueError('demo_compose: the two mesh panels come together')
    opt = mesh is None
    planes = [_f32(glob, (B, 3, hm, hm), 'demo_compose: glob'), _f32(part, (B, 24, 3, hm, hm), 'demo_compose: part'),
              _f32(riuv, (B, 3, hm, hm), 'demo_compose: riuv'), _f32(mesh, (B, 3, S, S), 'demo_compose: mesh', opt),
              _f32(side, (B, 3, S, S), 'demo_compose: side', opt), _f32(side_alpha, (B, S, S), 'demo_compose: side_alpha', opt)]
    out = torch.empty(B, S, (9 if opt else 13) * S // 2, 4, device=img.device, dtype=torch.float32)
    check(_lib.lib().danet_demo_compose(ptr(img), *[ptr(t) for t in planes], B, S, hm, ptr(out), stream()), 'danet_demo_compose')
    return out


def vis_grid_size(N, H, W, nrow, padding):
    """The sheet rule's size for N tiles of H x W -> (Hs, Ws)."""
    xmaps = min(int(nrow), int(N))
    ymaps = -(-int(N) // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def vis_grid(a, b=None, nrow=8, padding=2, pad_value=0., denormalize=False, overlay=None, lohi=None):
    """The sheet rule (csrc/train_vis.hip), one launch: a [B,C,H,W] fp32 / bf16 with any strides (C = 1 or 3), b a
    second source of the same shape whose tiles are interleaved with a's, overlay [B,3,h,w] laid over the tiles where > 0, lohi a
    2-float device buffer (min, max) that switches the normalisation on.  -> [3,Hs,Ws] f32."""
    ts, strides, bf16 = _strided([a] if b is None else [a, b], 'vis_grid', 4, 2)
    B, C, H, W = ts[0].shape
    if b is not None:
        _shape(ts[1], (B, C, H, W), 'vis_grid: b')
    ov = _f32(overlay, (B, 3, None, None), 'vis_grid: overlay', optional=True)
    oh, ow = (0, 0) if ov is None else (ov.shape[2], ov.shape[3])
    lh = None if lohi is None else _shape(_f32(lohi, None, 'vis_grid: lohi').reshape(-1), (2,), 'vis_grid: lohi (min, max)')
    flags = (1 if denormalize else 0) | (2 if lh is not None else 0)
    Hs, Ws = vis_grid_size(B * len(ts), H, W, nrow, padding)
    out = torch.empty(3, Hs, Ws, device=ts[0].device, dtype=torch.float32)
    check(_lib.lib().danet_vis_grid(ts[0].data_ptr(), None if b is None else ts[1].data_ptr(), strides, bf16,
                                    B, C, H, W, int(nrow), int(padding), float(pad_value), flags, ptr(ov), oh, ow, ptr(lh), ptr(out), stream()),
          'danet_vis_grid')
    return out


def vis_joints(sheet, joints, vis, B, H, W, nrow=8, padding=2):
    """The marker rule (csrc/train_vis.hip), one launch, IN PLACE on sheet [3,Hs,Ws] f32 (contiguous) as vis_grid made
    it from B tiles of H x W: joints [B,J,>=2] f32 (x, y relative to the tile), vis [B,J] / [B,J,1] f32 or None (all visible)."""
    sh = _dev_tensor(sheet, 'vis_joints')
    if sh.dtype != torch.float32 or sh.dim() != 3 or sh.shape[0] != 3 or not sh.is_contiguous():
        raise ValueError('vis_joints: a contiguous [3,Hs,Ws] f32 sheet expected, got %s %s' % (sh.dtype, tuple(sh.shape)))
    j = _shape(_dev_tensor(joints, 'vis_joints').to(torch.float32), (B, None, None), 'vis_joints: joints')      # (read through its strides)
    if j.shape[2] < 2:
        raise ValueError('vis_joints: joints %s, expected [B,J,>=2]' % (tuple(j.shape),))
    J = j.shape[1]
    v, vs = None, None
    if vis is not None:
        v = _shape(_dev_tensor(vis, 'vis_joints').to(torch.float32).reshape(vis.shape[0], -1), (B, J), 'vis_joints: visibility')
        vs = (ctypes.c_int64 * 2)(*v.stride())
    check(_lib.lib().danet_vis_joints(sh.data_ptr(), sh.shape[1], sh.shape[2], j.data_ptr(), (ctypes.c_int64 * 3)(*j.stride()),
                                      None if v is None else v.data_ptr(), vs, B, J, H, W, int(nrow), int(padding), stream()), 'danet_vis_joints')
    return sheet


def _rodrigues(theta, which):
    require_gpu(theta, which)
    if theta.requires_grad:
        raise RuntimeError('%s is forward-only (the reference only applies it to labels)' % which)
    th = _f32c(theta).view(-1, 3)
    R = torch.empty(th.shape[0], 3, 3, device=th.device, dtype=torch.float32)
    check(getattr(_lib.lib(), which)(ptr(th), th.shape[0], ptr(R), stream()), which)
    return R


def batch_rodrigues(theta):
    """/root/reference/utils/geometry.py:9-23."""
    return _rodrigues(theta, 'danet_batch_rodrigues')


def rodrigues_smplx(theta):
    return _rodrigues(theta, 'danet_rodrigues_smplx')


class Rot6dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        require_gpu(x, 'rot6d_to_rotmat')
        L = _lib.lib()
        xc = _f32c(x).view(-1, 6)
        R = torch.empty(xc.shape[0], 3, 3, device=xc.device, dtype=torch.float32)
        check(L.danet_rot6d_to_rotmat_forward(ptr(xc), xc.shape[0], ptr(R), stream()), 'danet_rot6d_to_rotmat_forward')
        ctx.save_for_backward(xc)
        ctx.in_shape = x.shape
        return R

    @staticmethod
    def backward(ctx, gR):
        L = _lib.lib()
        (xc,) = ctx.saved_tensors
        g = _f32c(gR)
        gx = torch.empty_like(xc)
        check(L.danet_rot6d_to_rotmat_backward(ptr(xc), ptr(g), xc.shape[0], ptr(gx), stream()), 'danet_rot6d_to_rotmat_backward')
        return gx.view(ctx.in_shape)


def rot6d_to_rotmat(x):
    """/root/reference/utils/geometry.py:47-61."""
    return Rot6dFunction.apply(x)


def rotmat_to_angle_axis(R):
    """[..., 3, 3] rotation matrices -> [N, 3] axis-angle vectors with the angle in [0, pi] (DESIGN.md "axis-angle rule"): the inverse
    of batch_rodrigues, where eval.py:175-178 calls tgm.rotation_matrix_to_angle_axis.  Forward only."""
    Rc = _f32(R, None, 'rotmat_to_angle_axis').view(-1, 3, 3)
    aa = torch.empty(Rc.shape[0], 3, device=Rc.device, dtype=torch.float32)
    check(_lib.lib().danet_rotmat_to_angle_axis(ptr(Rc), Rc.shape[0], ptr(aa), stream()), 'danet_rotmat_to_angle_axis')
    return aa


def pose_eval(pred_vertices, J_regressor, joint_mapper, gt_keypoints_3d=None, gt_vertices=None):
    """metrics.pose_errors as ONE launch (csrc/eval_ops.hip): pred_vertices [B,V,3], J_regressor [17,V], joint_mapper 3..17 ints
    (host), exactly one of gt_keypoints_3d [B,J,3] / gt_vertices [B,V,3] -> (mpjpe [B], recon_err [B], pred_joints17 [B,17,3]).
    Allocates its three outputs and nothing else; capturable under torch.cuda.graph."""
    if (gt_keypoints_3d is None) == (gt_vertices is None):
        raise ValueError('pose_eval: give exactly one of gt_keypoints_3d / gt_vertices')
    v = _f32(pred_vertices, (None, None, 3), 'pose_eval: pred_vertices')
    B, V = v.shape[0], v.shape[1]
    Jr = _f32(J_regressor, (17, V), 'pose_eval: J_regressor')
    mapper = [int(m) for m in joint_mapper]
    J = len(mapper)
    gv = _f32(gt_vertices, (B, V, 3), 'pose_eval: gt_vertices', optional=True)
    gk = _f32(gt_keypoints_3d, (B, J, 3), 'pose_eval: gt_keypoints_3d', optional=True)
    e, r = (torch.empty(B, device=v.device, dtype=torch.float32) for _ in range(2))
    j17 = torch.empty(B, 17, 3, device=v.device, dtype=torch.float32)
    check(_lib.lib().danet_pose_eval(ptr(v), ptr(Jr), _host_i32(mapper), J, ptr(gk), ptr(gv), B, V, ptr(e), ptr(r), ptr(j17), stream()),
          'danet_pose_eval')
    return e, r, j17


def vertex_eval(pred_vertices, gt_vertices, pelvis_row):
    """The PVE rule of DESIGN.md 4c as ONE launch (csrc/eval_ops.hip): pred_vertices, gt_vertices [B,V,3], pelvis_row [V] (row 0 of the
    H36M joint regressor) -> (pve [B], pa_pve [B]) in metres: the mean vertex distance of the two meshes, each centred at its own
    pelvis, and the mean distance after the Procrustes alignment of the V raw points.  Allocates its two outputs and nothing else;
    capturable under torch.cuda.graph."""
    v = _f32(pred_vertices, (None, None, 3), 'vertex_eval: pred_vertices')
    B, V = v.shape[0], v.shape[1]
    g = _f32(gt_vertices, (B, V, 3), 'vertex_eval: gt_vertices')
    w = _f32(pelvis_row, (V,), 'vertex_eval: pelvis_row')
    pve, pa = (torch.empty(B, device=v.device, dtype=torch.float32) for _ in range(2))
    check(_lib.lib().danet_vertex_eval(ptr(v), ptr(g), ptr(w), B, V, ptr(pve), ptr(pa), stream()), 'danet_vertex_eval')
    return pve, pa


SEG_COUNTERS = 32
SEG = {'tp': 0, 'fp': 2, 'fn': 4, 'accuracy': 6, 'pixel_count': 7, 'parts_tp': 8, 'parts_fp': 15, 'parts_fn': 22,
       'parts_accuracy': 29, 'parts_pixel_count': 30}              # include/danet_hip.h DANET_SEG_*


def seg_confusion(mask, parts, gt_mask, gt_parts, offsets, shapes, rects, tables, max_pixels, counters):
    """The LSP mask / part scoring of eval.py:222-266 for a batch in ONE launch, ADDED to `counters` (int64 [32] on the device, layout
    SEG).  mask [B,R,R] f32 and parts [B,R,R] int64 as PartRenderer returns them; gt_mask / gt_parts packed uint8 label images (either
    may be None); offsets int64 [B+1], shapes int32 [B,2], rects int32 [B,6], tables int32 [T]: evaluate.pack_labels builds them."""
    m = _dev_tensor(mask, 'seg_confusion')
    p = _dev_tensor(parts, 'seg_confusion')
    B, R = m.shape[0], m.shape[-1]
    if m.dtype != torch.float32 or p.dtype != torch.int64 or tuple(m.shape) != (B, R, R) or tuple(p.shape) != (B, R, R):
        raise ValueError('seg_confusion: mask %s %s, parts %s %s (expected f32 / int64 [B,R,R])' % (m.dtype, tuple(m.shape), p.dtype, tuple(p.shape)))
    labels = [t for t in (gt_mask, gt_parts) if t is not None]
    if not labels or any(t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != labels[0].numel() for t in labels):
        raise ValueError('seg_confusion: the label images come as packed uint8 buffers of one length')
    for t, dt, shp, what in ((offsets, torch.int64, (B + 1,), 'offsets'), (shapes, torch.int32, (B, 2), 'shapes'), (rects, torch.int32, (B, 6), 'rects'),
                             (counters, torch.int64, (SEG_COUNTERS,), 'counters')):
        if t.dtype != dt or tuple(t.shape) != shp:
            raise ValueError('seg_confusion: %s must be %s %s, got %s %s' % (what, dt, shp, t.dtype, tuple(t.shape)))
    if tables.dtype != torch.int32 or tables.dim() != 1:
        raise ValueError('seg_confusion: tables must be a flat int32 tensor')
    check(_lib.lib().danet_seg_confusion(ptr(m), ptr(p), ptr(gt_mask), ptr(gt_parts), labels[0].numel(), ptr(offsets), ptr(shapes),
                                         ptr(rects), ptr(tables), tables.numel(), B, R, int(max_pixels), ptr(counters), stream()),
          'danet_seg_confusion')
    return counters


COCO_MAX_DETS, COCO_MAX_GT = 20, 256                                   # include/danet_hip.h DANET_COCO_*


def coco_keypoints(joints, camera, center, scale, img_res=224, focal_length=5000., out=None):
    """eval_coco.py:114-145 for a batch in ONE launch (csrc/coco_ops.hip): joints [B,49,3] as the SMPL layer returns them, camera
    [B,3] = (s, tx, ty), center [B,2] and scale [B] of the crop -> the 17 COCO keypoints [B,17,2] f32 in pixels of the original
    image (`out`, or a new tensor -- the op's only allocation).  Capturable under torch.cuda.graph."""
    j = _f32(joints, (None, 49, 3), 'coco_keypoints: joints')
    B = j.shape[0]
    cam = _f32(camera, (B, 3), 'coco_keypoints: camera')
    c = _f32(center, (B, 2), 'coco_keypoints: center')
    s = _shape(_f32(scale, None, 'coco_keypoints: scale').reshape(-1), (B,), 'coco_keypoints: scale')
    out = _out(out, torch.float32, (B, 17, 2), j.device, 'coco_keypoints: out')
    check(_lib.lib().danet_coco_keypoints(ptr(j), ptr(cam), ptr(c), ptr(s), B, int(img_res), float(focal_length), ptr(out), stream()),
          'danet_coco_keypoints')
    return out


def coco_oks_match(dt_kpts, dt_area, dt_offsets, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd, gt_offsets):
    """The per-image part of the COCO keypoint rule for a whole dataset in ONE launch, one workgroup per image
    (csrc/coco_ops.hip).  Detections packed by image in evaluation order: dt_kpts [N,17,2] f32, dt_area [N] f64, dt_offsets int64
    [I+1]; ground truth packed by image: gt_kpts [M,17,3] f64, gt_area [M] f64, gt_bbox [M,4] f64, gt_ignore / gt_iscrowd [M] uint8,
    gt_offsets int64 [I+1].  -> (dt_match [N,3], dt_ignore [N,3]) as int32 holding the kernel's 16-bit words (bit t = threshold
    0.5 + 0.05 t; columns = area ranges all, medium, large) and gt_count [I,3] int32.  The offsets are read back and checked on the
    host (this op belongs to summary(), which copies to the host anyway); more than COCO_MAX_GT ground truths in an image is an error."""
    dk = _dev_tensor(dt_kpts, 'coco_oks_match')
    N, I = dk.shape[0], dt_offsets.numel() - 1
    M = gt_kpts.shape[0]
    for t, dt, shp, name in ((dk, torch.float32, (N, 17, 2), 'dt_kpts'), (dt_area, torch.float64, (N,), 'dt_area'),
                             (gt_kpts, torch.float64, (M, 17, 3), 'gt_kpts'), (gt_area, torch.float64, (M,), 'gt_area'),
                             (gt_bbox, torch.float64, (M, 4), 'gt_bbox'), (gt_ignore, torch.uint8, (M,), 'gt_ignore'),
                             (gt_iscrowd, torch.uint8, (M,), 'gt_iscrowd'), (dt_offsets, torch.int64, (I + 1,), 'dt_offsets'),
                             (gt_offsets, torch.int64, (I + 1,), 'gt_offsets')):
        _typed(t, dt, shp, 'coco_oks_match: ' + name)
    if I < 1:
        raise ValueError('coco_oks_match: no images')
    _ascending(dt_offsets.cpu().numpy(), N, 'coco_oks_match: dt_offsets')
    max_gt = int(np.diff(_ascending(gt_offsets.cpu().numpy(), M, 'coco_oks_match: gt_offsets')).max())
    # the kernel stores 16-bit words; torch has no arithmetic on uint16, so the buffers are int16 and widened after the launch
    dm, di = (torch.empty(N, 3, device=dk.device, dtype=torch.int16) for _ in range(2))
    gc = torch.empty(I, 3, device=dk.device, dtype=torch.int32)
    check(_lib.lib().danet_coco_oks_match(ptr(dk), ptr(dt_area), ptr(dt_offsets), N, ptr(gt_kpts), ptr(gt_area), ptr(gt_bbox), ptr(gt_ignore),
                                          ptr(gt_iscrowd), ptr(gt_offsets), M, I, max_gt, ptr(dm), ptr(di), ptr(gc), stream()),
          'danet_coco_oks_match')
    return dm.int() & 0xffff, di.int() & 0xffff, gc


def batch_crop(src, offsets, shapes, origin, params, res, out=None):
    """augment.rgb_processing for a batch in ONE launch (csrc/input_ops.hip): src packed uint8 HWC pixels (flat), offsets int64 [B+1]
    (bytes), shapes int32 [B,2] (rows, cols of what is packed per sample), origin int32 [B,2] (x0, y0 of that rectangle in its image),
    params float64 [B,10] = (inverse crop transform: 6, flip, pn: 3) -> [B,3,res,res] f32 (`out`, or a new tensor -- the op's only
    allocation).  datasets.crop_params builds the arguments."""
    s = _packed_u8(src, 'batch_crop: src')
    B = offsets.numel() - 1
    _typed(offsets, torch.int64, (B + 1,), 'batch_crop: offsets')
    _typed(shapes, torch.int32, (B, 2), 'batch_crop: shapes')
    _typed(origin, torch.int32, (B, 2), 'batch_crop: origin')
    _typed(params, torch.float64, (B, 10), 'batch_crop: params')
    res = int(res)
    out = _out(out, torch.float32, (B, 3, res, res), s.device, 'batch_crop: out')
    check(_lib.lib().danet_batch_crop(ptr(s), s.numel(), ptr(offsets), ptr(shapes), ptr(origin), ptr(params), B, res, ptr(out), stream()),
          'danet_batch_crop')
    return out


def label_augment(rot_flip, xform=None, keypoints=None, smpl_2dkps=None, pose_3d=None, pose=None, fits=None, res=224, inverse=False):
    """The label transforms of a batch in ONE launch (csrc/input_ops.hip): rot_flip float64 [B,2] (degrees, flip), xform float64 [B,6]
    (crop transform, for the 2D inputs), float64 keypoints [B,49,3] / smpl_2dkps [B,24,3] / pose_3d [B,24,4] / pose [B,72], float32 fits
    [B,82].  -> dict of f32 tensors under the inputs' names; `fits` gives 'fits_pose' [B,72] and 'fits_betas' [B,10].  inverse: the pose
    transforms undone (FitsDict.__setitem__)."""
    B = rot_flip.shape[0]
    rf = _typed(rot_flip, torch.float64, (B, 2), 'label_augment: rot_flip')
    dev = rf.device
    xf = None if xform is None else _typed(xform, torch.float64, (B, 6), 'label_augment: xform')
    if (keypoints is not None or smpl_2dkps is not None) and xf is None:
        raise ValueError('label_augment: 2D keypoints need the crop transform')
    spec = (('keypoints', keypoints, torch.float64, (B, 49, 3)), ('smpl_2dkps', smpl_2dkps, torch.float64, (B, 24, 3)),
            ('pose_3d', pose_3d, torch.float64, (B, 24, 4)), ('pose', pose, torch.float64, (B, 72)), ('fits', fits, torch.float32, (B, 82)))
    ins, outs = [], {}
    for name, t, dt, shp in spec:
        ins.append(None if t is None else _typed(t, dt, shp, 'label_augment: ' + name))
        if t is not None and name != 'fits':
            outs[name] = torch.empty(shp, device=dev, dtype=torch.float32)
    if fits is not None:
        outs['fits_pose'] = torch.empty(B, 72, device=dev, dtype=torch.float32)
        outs['fits_betas'] = torch.empty(B, 10, device=dev, dtype=torch.float32)
    if not outs:
        raise ValueError('label_augment: nothing to do')
    o = lambda k: ptr(outs.get(k))           # noqa: E731
    check(_lib.lib().danet_label_augment(ptr(xf), ptr(rf), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), B, int(res),
                                         int(bool(inverse)), o('keypoints'), o('smpl_2dkps'), o('pose_3d'), o('pose'), o('fits_pose'),
                                         o('fits_betas'), stream()), 'danet_label_augment')
    return outs


def scene_render(verts, vcol, faces2, cam_t, proj, dscale, person_frame, src, offsets, shapes, return_aux=False, out=None, host=None):
    """The scene rule of DESIGN.md in three launches (csrc/scene_ops.hip): the shaded meshes of P people drawn into the N frames they
    were found in, the people of a frame sharing one depth buffer.  verts / vcol [P,V,3] f32: the two halves of mesh_shade_vertices'
    workspace; faces2 [F2,3] int32 (both windings); cam_t [P,3], proj [P,6], dscale [P] f32 (scene.person_cameras builds them);
    person_frame [P] int32, non-decreasing; src / offsets int64 [N+1] / shapes int32 [N,2]: batch_crop's packed uint8 HWC frames.
    -> out (uint8, the size and layout of src; `out`, or a new tensor), with return_aux also ids (int32 per frame pixel, person * F2
    + face or -1) and depth (f32 per frame pixel, +inf where empty).  `host`: (person_frame, offsets, shapes) as host arrays, which
    the entry point checks before it launches; without it they are read back from the device (a synchronisation: pass it to capture
    the call under torch.cuda.graph)."""
    s = _packed_u8(src, 'scene_render: src')
    v = _f32(verts, (None, None, 3), 'scene_render: verts')
    P, V = v.shape[0], v.shape[1]
    c = _f32(vcol, (P, V, 3), 'scene_render: vcol')
    N = offsets.numel() - 1
    F2 = faces2.shape[0]
    _typed(faces2, torch.int32, (F2, 3), 'scene_render: faces2')
    ct, pj = _f32(cam_t, (P, 3), 'scene_render: cam_t'), _f32(proj, (P, 6), 'scene_render: proj')
    ds = _shape(_f32(dscale, None, 'scene_render: dscale').reshape(-1), (P,), 'scene_render: dscale')
    _typed(person_frame, torch.int32, (P,), 'scene_render: person_frame')
    _typed(offsets, torch.int64, (N + 1,), 'scene_render: offsets')
    _typed(shapes, torch.int32, (N, 2), 'scene_render: shapes')
    if host is None:
        host = (person_frame.cpu().numpy(), offsets.cpu().numpy(), shapes.cpu().numpy())
    hp, ho, hs = (np.asarray(a) for a in host)
    if hp.size != P or ho.size != N + 1 or hs.size != 2 * N:
        raise ValueError('scene_render: host copies of %d, %d, %d elements for P = %d, N = %d' % (hp.size, ho.size, hs.size, P, N))
    npix = max(int(ho[-1]) - int(ho[0]), 0) // 3 if N > 0 else 0
    out = _out(out, torch.uint8, tuple(s.shape), s.device, 'scene_render: out')
    ids = torch.empty(npix, device=s.device, dtype=torch.int32) if return_aux else None
    depth = torch.empty(npix, device=s.device, dtype=torch.float32) if return_aux else None
    L = _lib.lib()
    nws = L.danet_scene_render_ws_bytes(P, V, npix)
    ws = _workspace(nws, s.device)
    check(L.danet_scene_render(ptr(v), ptr(c), P, V, ptr(faces2), F2, ptr(ct), ptr(pj), ptr(ds), ptr(person_frame), ptr(s), s.numel(),
                               ptr(offsets), ptr(shapes), N, _host_i32(hp), _host_i64(ho), _host_i32(hs),
                               ptr(out), ptr(ids), ptr(depth), ptr(ws), nws, stream()), 'danet_scene_render')
    return (out, ids, depth) if return_aux else out


# ---- texture atlases (csrc/texture_ops.hip; DESIGN.md "texture rule") ----------------------------------------------------------
_TEXTURE_INTS = {}


def _texture_ints(host, device):
    """A small host int32 array on `device`, uploaded once per value (an upload cannot be captured under torch.cuda.graph) and kept
    for the life of the process: a captured graph holds its address."""
    key = (str(device), host.tobytes())
    if key not in _TEXTURE_INTS:
        _TEXTURE_INTS[key] = torch.from_numpy(host.copy()).to(device)
    return _TEXTURE_INTS[key]


def texture_view_offsets(view_off, N):
    """The views of person p are view_off[p] .. view_off[p+1] - 1; None: one view per person.  -> host int32 [P+1], checked."""
    off = np.arange(N + 1, dtype=np.int32) if view_off is None else view_off
    return np.ascontiguousarray(_ascending(off, N, 'texture_unwrap: view_off', integers=True), np.int32)


def texture_atlas_index(atlas_index, N, P):
    """Which person's atlas a drawn view uses; None: view n uses atlas n.  -> host int32 [N], checked."""
    idx = np.arange(N, dtype=np.int32) if atlas_index is None else np.asarray(atlas_index).reshape(-1)
    if idx.size != N or not np.issubdtype(idx.dtype, np.integer) or (idx < 0).any() or (idx >= P).any():
        raise ValueError('texture_render: atlas_index must hold %d integers in [0, %d), got %s' % (N, P, idx.tolist()))
    return np.ascontiguousarray(idx, np.int32)


def _texture_size(T):
    if int(T) != T or int(T) < 2 or int(T) > 4096:
        raise ValueError('texture: chart size T = %s (an integer in [2, 4096])' % (T,))
    return int(T)


def texture_map(uv, faces, part_off, part_faces, T):
    """The texel -> surface map of the texture rule, one launch: uv [NDV,2] f32, faces [F,3] int32 over the DensePose vertices,
    the faces of the 24 parts as a CSR (part_off [25], part_faces [F] int32, ascending within a part) -> (face [24,T,T] int32, -1
    where no face holds the texel centre; bary [24,T,T,2] f32)."""
    uv = _dev_tensor(uv, 'texture_map')
    T = _texture_size(T)
    NDV, F = uv.shape[0], faces.shape[0]
    _typed(uv, torch.float32, (NDV, 2), 'texture_map: uv')
    _typed(faces, torch.int32, (F, 3), 'texture_map: faces')
    _typed(part_off, torch.int32, (25,), 'texture_map: part_off')
    _typed(part_faces, torch.int32, (F,), 'texture_map: part_faces')
    face = torch.empty(24, T, T, device=uv.device, dtype=torch.int32)
    bary = torch.empty(24, T, T, 2, device=uv.device, dtype=torch.float32)
    check(_lib.lib().danet_texture_map(ptr(uv), NDV, ptr(faces), F, ptr(part_off), ptr(part_faces), T, ptr(face), ptr(bary), stream()),
          'danet_texture_map')
    return face, bary


def texture_views(images, vertices, cam, what, optional=False):
    """The per-view arguments both texture ops share, checked and in fp32: images [N,3,H,H] (`optional`: or None), vertices
    [N,NV,3], cam [N,3].  TextureAtlas calls it before its first launch; the ops call it again (no copy the second time)."""
    v = _f32(vertices, (None, None, 3), what + ': vertices')
    N = v.shape[0]
    img = _f32(images, (N, 3, None, None), what + ': images', optional=optional)
    if img is not None and img.shape[2] != img.shape[3]:
        raise ValueError('%s: images %s, expected square [N,3,H,H]' % (what, tuple(img.shape)))
    return img, v, _f32(cam, (N, 3), what + ': cam')


def texture_atlas(atlas, what='texture_render'):
    """atlas [P,24,T,T,4] f32, contiguous, P >= 1 -> (atlas, P, T)."""
    if not torch.is_tensor(atlas) or atlas.dim() != 5 or atlas.shape[0] < 1 or atlas.shape[2] != atlas.shape[3]:
        raise ValueError('%s: atlas %s, expected [P,24,T,T,4]' % (what, tuple(getattr(atlas, 'shape', ())) or type(atlas).__name__))
    P, T = atlas.shape[0], _texture_size(atlas.shape[2])
    return _typed(atlas, torch.float32, (P, 24, T, T, 4), what + ': atlas'), P, T


def texture_unwrap(images, vertices, cam, depth, view_off, vert_mapping, faces, map_face, map_bary, focal, depth_tol=0.02, min_cos=0.1):
    """Photographs -> atlas [P,24,T,T,4] f32 (r, g, b, summed weight), one launch.  images [N,3,H,H] f32, vertices [N,NV,3], cam
    [N,3], depth [N,H,H] (iuv_raster's depth plane of `faces` at orig = out_size = H), view_off: HOST integers [P+1] (None: one view
    per person), vert_mapping [NDV] / faces [F,3] int32, map_face / map_bary: texture_map's."""
    img, v, c = texture_views(images, vertices, cam, 'texture_unwrap')
    N, H = img.shape[0], img.shape[2]
    d = _f32(depth, (N, H, H), 'texture_unwrap: depth')
    off = texture_view_offsets(view_off, N)
    P = off.size - 1
    T = _texture_size(map_face.shape[-1])
    NDV, F = vert_mapping.numel(), faces.shape[0]
    _typed(vert_mapping, torch.int32, (NDV,), 'texture_unwrap: vert_mapping')
    _typed(faces, torch.int32, (F, 3), 'texture_unwrap: faces')
    _typed(map_face, torch.int32, (24, T, T), 'texture_unwrap: map_face')
    _typed(map_bary, torch.float32, (24, T, T, 2), 'texture_unwrap: map_bary')
    atlas = torch.empty(P, 24, T, T, 4, device=img.device, dtype=torch.float32)
    check(_lib.lib().danet_texture_unwrap(ptr(img), ptr(v), ptr(c), ptr(d), N, v.shape[1], H, ptr(_texture_ints(off, img.device)),
                                          _host_i32(off), P, ptr(vert_mapping), NDV, ptr(faces), F, ptr(map_face), ptr(map_bary), T,
                                          float(focal), float(depth_tol), float(min_cos), ptr(atlas), stream()), 'danet_texture_unwrap')
    return atlas


def texture_render(rverts, cam, vert_mapping, faces, uv, face_part, fidx, atlas, atlas_index=None, images=None, focal=5000.,
                   fill=(0.5, 0.5, 0.5)):
    """The textured draw, one launch: rverts [N,NV,3] (already rotated), cam [N,3], fidx [N,S,S] int32 (iuv_raster's face-index
    plane of `faces` at orig = out_size = S), atlas [P,24,T,T,4], atlas_index: HOST integers [N] in [0, P) (None: view n draws
    atlas n), images [N,3,S,S] or None -> (rgb [N,3,S,S], alpha [N,S,S])."""
    _, v, c = texture_views(None, rverts, cam, 'texture_render', optional=True)
    at, P, T = texture_atlas(atlas)
    N, S = v.shape[0], fidx.shape[-1]
    _typed(fidx, torch.int32, (N, S, S), 'texture_render: fidx')
    idx = texture_atlas_index(atlas_index, N, P)
    NDV, F = vert_mapping.numel(), faces.shape[0]
    _typed(vert_mapping, torch.int32, (NDV,), 'texture_render: vert_mapping')
    _typed(faces, torch.int32, (F, 3), 'texture_render: faces')
    _typed(uv, torch.float32, (NDV, 2), 'texture_render: uv')
    _typed(face_part, torch.int32, (F,), 'texture_render: face_part')
    img, rgb, alpha = _draw_buffers(images, N, S, v.device, 'texture_render')
    fl = (ctypes.c_float * 3)(*[float(x) for x in fill])
    check(_lib.lib().danet_texture_render(ptr(v), ptr(c), N, v.shape[1], ptr(vert_mapping), NDV, ptr(faces), F, ptr(uv), ptr(face_part),
                                          ptr(fidx), ptr(at), P, T, ptr(_texture_ints(idx, v.device)), _host_i32(idx), ptr(img),
                                          float(focal), S, fl, ptr(rgb), ptr(alpha), stream()), 'danet_texture_render')
    return rgb, alpha
