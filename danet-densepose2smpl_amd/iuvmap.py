"""IUV map glue (/root/reference/utils/iuvmap.py:6-38, 103-147) as a handful of tensor ops
instead of ~100 threshold/min launches; integer-exact one-hot planes.  iuv_map2img (iuvmap.py:41-100), the decode for
display, is one HIP launch (csrc/vis_ops.hip)."""
import numpy as np
import torch
import torch.nn.functional as F

INDEX2MASK = [[0], [1, 2], [3], [4], [5], [6], [7, 9], [8, 10], [11, 13], [12, 14], [15, 17], [16, 18],
              [19, 21], [20, 22], [23, 24]]
_MERGE = {}


def _onehot(x):
    idx = torch.argmax(x, dim=1)
    return F.one_hot(idx, x.shape[1]).permute(0, 3, 1, 2).to(torch.float32)


def iuvmap_clean(U_uv, V_uv, Index_UV, AnnIndex=None):
    """argmax -> exact one-hot, U/V masked by it (gradient flows to U,V only), iuvmap.py:6-38."""
    I = _onehot(Index_UV)
    A = None if AnnIndex is None else _onehot(AnnIndex)
    return I * U_uv.float(), I * V_uv.float(), I, A


def _merge_matrix(device):
    key = str(device)
    if key not in _MERGE:
        m = torch.zeros(15, 25)
        for i, grp in enumerate(INDEX2MASK):
            m[i, grp] = 1
        _MERGE[key] = m.to(device)
    return _MERGE[key]


def iuv_img2map(uvimages):
    """3-channel IUV image -> U,V,Index [B,25,H,W] + Ann [B,15,H,W] (iuvmap.py:103-147, uv_rois=None)."""
    part = torch.round(uvimages[:, 0] * 24).long().clamp_(0, 24)
    I = F.one_hot(part, 25).permute(0, 3, 1, 2).to(torch.float32)
    U = I * uvimages[:, 1:2]
    V = I * uvimages[:, 2:3]
    A = torch.einsum('ac,bchw->bahw', _merge_matrix(uvimages.device), I)
    return U, V, I, A


_TABLES = {}


def mapping_table(rows, device):
    """[J,K] f32 device table of plane-0 values, float32(ind_mapping[k] * (1. / 24.)) with the product in double -- how the
    reference's assignment `output[0][output[0] == ind] = ind_mapping[ind] * (1. / 24.)` rounds them.  That in-place loop
    cannot chain as long as ind_mapping[0] == 0 (no later value is an integer a later `ind` could match), which is required."""
    rows = tuple(tuple(int(m) for m in r) for r in rows)
    if any(r[0] != 0 for r in rows):
        raise ValueError('iuv_map2img: ind_mapping[0] must be 0 (the reference loop re-maps its own results otherwise)')
    key = (str(device), rows)
    if key not in _TABLES:
        tab = np.array([[np.float32(m * (1. / 24.)) for m in r] for r in rows], dtype=np.float32)
        _TABLES[key] = torch.from_numpy(tab).to(device)
    return _TABLES[key]


def iuv_map2img(U_uv, V_uv, Index_UV, AnnIndex=None, uv_rois=None, ind_mapping=None):
    """U, V, Index [B,K,H,W] (+ Ann [B,KA,H,W]) -> IUV image [B,3,H,W] f32 (iuvmap.py:41-100): plane 0 the arg-max index (zeroed
    where the Ann arg-max is 0) over K - 1, or ind_mapping[index] / 24; planes 1, 2 the U, V of that channel.  fp32 or bf16,
    any strides.  Forward only, GPU only."""
    from . import ops
    if uv_rois is not None:
        raise NotImplementedError('iuv_map2img(uv_rois=...): a Detectron leftover that no caller of the reference passes')
    table = None
    if ind_mapping is not None:
        if len(ind_mapping) != Index_UV.shape[1]:
            raise ValueError('iuv_map2img: ind_mapping has %d entries for %d index channels' % (len(ind_mapping), Index_UV.shape[1]))
        table = mapping_table([ind_mapping], Index_UV.device)
    return ops.iuv_map2img(U_uv, V_uv, Index_UV, AnnIndex, table)


def part_iuv_map2img(part_iuv_map, dp2smpl_mapping=None):
    """The 24 iuv_map2img calls of demo.py:131-141 as ONE launch: [B,24,3,K,H,W] -> [B,24,3,H,W]; K = 7 decodes joint i with
    ind_mapping = [0] + dp2smpl_mapping[i], K = 25 without a mapping."""
    from . import ops
    if part_iuv_map.dim() != 6 or part_iuv_map.shape[2] != 3:
        raise ValueError('part_iuv_map2img: expected [B,J,3,K,H,W], got %s' % (tuple(part_iuv_map.shape),))
    J, K = part_iuv_map.shape[1], part_iuv_map.shape[3]
    table = None
    if K != 25:
        if dp2smpl_mapping is None or len(dp2smpl_mapping) != J or any(len(r) != K - 1 for r in dp2smpl_mapping):
            raise ValueError('part_iuv_map2img: K = %d needs dp2smpl_mapping with %d rows of %d parts' % (K, J, K - 1))
        table = mapping_table([[0] + list(r) for r in dp2smpl_mapping], part_iuv_map.device)
    return ops.iuv_map2img(part_iuv_map[:, :, 0], part_iuv_map[:, :, 1], part_iuv_map[:, :, 2], None, table)
