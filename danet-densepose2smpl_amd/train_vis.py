"""Image sheets of the training visualisation (/root/reference/train/trainer.py:250-305, utils/vis.py:359-405,
utils/renderer.py:39-50) on the device: the sheet rule and the marker rule of DESIGN.md 4e as two HIP kernels
(csrc/train_vis.hip), the PNG writer the demo shares, and the step schedule of base_trainer.py:73,81-83.

torchvision and cv2 are absent: make_grid here is the sheet rule, draw_joints the marker rule, both specified by this project.
Nothing allocates by data and nothing synchronises: every function but write_png captures under torch.cuda.graph."""
import struct
import zlib

import numpy as np

_CONSTANTS = {}


def vis_due(step_count, vis_interval):
    """Is the step that raised the trainer's counter to `step_count` a visualisation step?  (base_trainer.py:81: the counter is
    tested after the increment, `(step_count - 1) % vis_interval == 0`; None / 0 = never.)"""
    return bool(vis_interval) and int(vis_interval) > 0 and (int(step_count) - 1) % int(vis_interval) == 0


def grid_size(n, H, W, nrow=8, padding=2):
    """(Hs, Ws) of the sheet of n tiles of H x W."""
    from . import ops
    return ops.vis_grid_size(n, H, W, nrow, padding)


def make_grid(tensor, nrow=8, padding=2, pad_value=0., normalize=False, denormalize=False):
    """The sheet rule: tensor [B,C,H,W] (C = 1 or 3, fp32 / bf16, any strides) -> [3,Hs,Ws] f32, one launch.  denormalize:
    x * std + mean with the ImageNet constants first.  normalize: (x - lo) / (hi - lo + 1e-5) clamped to [0, 1] with the min / max
    of the whole batch (after the de-normalisation, if any); they come from one torch.aminmax call and stay on the device."""
    from . import ops
    lohi = None
    if normalize:
        import torch
        x = tensor.detach().to(torch.float32)
        lohi = torch.stack(torch.aminmax(denormalized(x) if denormalize else x))
    return ops.vis_grid(tensor, None, nrow, padding, pad_value, denormalize=denormalize, lohi=lohi)


def overlay_grid(images, iuv, nrow=8, padding=1, pad_value=1., denormalize=True):
    """trainer.py:270-274 in one launch: the (ImageNet-normalised) images de-normalised, iuv [B,3,h,w] nearest-upsampled by the
    integer factor H / h laid over them per element where it is > 0, then the sheet."""
    from . import ops
    return ops.vis_grid(images, None, nrow, padding, pad_value, denormalize=denormalize, overlay=iuv)


def pair_grid(a, b):
    """utils/renderer.py:39-50 (visualize_tb): the sheet of a0, b0, a1, b1, ... with nrow 2, padding 2, pad 0."""
    from . import ops
    return ops.vis_grid(a, b, 2, 2, 0.)


def draw_joints(sheet, joints, vis=None, tile=None, nrow=8, padding=1):
    """The marker rule, in place on the fp32 sheet [3,Hs,Ws] in [0,1] (to_uint8 afterwards gives the reference's 0 / 255): joints
    [B,J,>=2] in tile pixels, vis [B,J] / [B,J,1] or None = all visible, tile = (H, W) of the sheet's tiles (the sheet must be
    the sheet rule's for B such tiles with this nrow and padding).  -> sheet."""
    from . import ops
    H, W = tile
    return ops.vis_joints(sheet, joints, vis, joints.shape[0], int(H), int(W), nrow, padding)


def joints_grid(images, joints, vis=None, nrow=8, padding=1, pad_value=1., denormalize=True):
    """vis_batch_image_with_joints (utils/vis.py:359-405) without the joint numbers: the images (de-normalised first, as
    trainer.py:251-253 hands them over), normalised by their batch min / max, on a sheet, with the markers on top."""
    sheet = make_grid(images, nrow, padding, pad_value, normalize=True, denormalize=denormalize)
    return draw_joints(sheet, joints, vis, images.shape[-2:], nrow, padding)


def denormalized(images):
    """trainer.py:251-253 as tensor ops (two roundings, as the kernel's x * std + mean)."""
    import torch
    key = str(images.device)
    if key not in _CONSTANTS:                     # (made once per device: an upload has no place in a capture)
        _CONSTANTS[key] = tuple(torch.tensor(c, device=images.device).reshape(1, 3, 1, 1) for c in ((0.229, 0.224, 0.225), (0.485, 0.456, 0.406)))
    std, mean = _CONSTANTS[key]
    return images.to(torch.float32) * std + mean


def to_uint8(sheet):
    """float -> uint8 as utils/vis.py:368: mul(255).clamp(0, 255).byte(), i.e. truncation."""
    return sheet.mul(255).clamp(0, 255).byte()


def write_png(path, arr):
    """uint8 array [H,W,3] (RGB) or [H,W,4] (RGBA) -> an 8-bit, non-interlaced PNG file (filter type 0 on every line).  A tensor
    is a sheet [3,H,W] as to_uint8 returns it: copied to the host and turned to [H,W,3] first."""
    if hasattr(arr, 'detach'):
        arr = np.transpose(arr.detach().cpu().numpy(), (1, 2, 0)) if arr.dim() == 3 else arr.detach().cpu().numpy()
    arr = np.ascontiguousarray(arr)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] not in (3, 4):
        raise ValueError('write_png: uint8 [H,W,3|4] expected, got %s %s' % (arr.dtype, arr.shape))
    H, W, C = arr.shape
    raw = np.concatenate([np.zeros((H, 1), np.uint8), arr.reshape(H, W * C)], 1).tobytes()

    def chunk(typ, body):
        return struct.pack('>I', len(body)) + typ + body + struct.pack('>I', zlib.crc32(typ + body) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2 if C == 3 else 6, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))
