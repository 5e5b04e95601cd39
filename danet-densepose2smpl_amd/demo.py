"""The result panels of /root/reference/demo.py:115-177 on the device.

result_panels(out, images, smpl, iuv_renderer, mesh_renderer=None, texture=None) turns what DaNet.infer_net or InferenceEngine.__call__
returned into one RGBA strip per image: input | decoded global IUV | the 24 decoded partial IUV maps (4 x 6) | IUV rendering of
the predicted mesh over the input | (with a MeshRenderer) shaded mesh over the input | shaded mesh turned by 90 degrees | (with a
texture.TextureAtlas) the mesh wearing the input's own colours, turned by 90 and by 180 degrees.

Launches of this package per batch with the mesh panels: 2 decodes (iuvmap.iuv_map2img, part_iuv_map2img), 3 x 3 of the
rasteriser (IUV render, two mesh views), 2 x 2 shading, 1 compose (+ the SMPL layer when `out` carries no vertices); the texture
panels add one unwrap (3 + 1 launches), two draws (1 + 3 + 1 each) and the tensor ops that join them to the strip.  Nothing
allocates by data and nothing synchronises: the whole call captures under torch.cuda.graph."""
import math

import torch

from . import iuvmap, ops
from ._lib import require_gpu
from .iuv_estimator import DP2SMPL_MAPPING
from .smpl import from_para


def mesh_of(out, smpl):
    """-> (vertices [B,V,3], cam [B,3]) of a result dict: the engine's vertices, or the SMPL layer on `para` (demo.py:148)."""
    para = out['para']
    verts = out.get('vertices')
    if verts is None:
        verts = from_para(smpl, para).vertices
    return verts.detach(), para[:, 0:3].contiguous()


def result_panels(out, images, smpl, iuv_renderer, mesh_renderer=None, dp2smpl_mapping=DP2SMPL_MAPPING, return_planes=False, texture=None):
    """out: infer_net's / the engine's dict; images [B,3,S,S] in [0,1] -> [B, S, 4.5 S, 4] f32 RGBA (6.5 S wide with a mesh
    renderer).  Alpha is 1 except in the last panel, where it is the mesh's coverage.  return_planes: also the dict of the planes
    the strip was composed from (glob, part, riuv, mesh, side, side_alpha).  texture: a TextureAtlas (or a pair (TextureAtlas,
    atlas [1 or B,24,T,T,4]) to draw an atlas made elsewhere, e.g. fused from several views): the strip grows by 2 S, the body
    textured from the images and turned by 90 and by 180 degrees, alpha = coverage; the columns before are unchanged."""
    require_gpu(images, 'result_panels')
    B, _, S, _ = images.shape
    vis = out['visualization']
    u, v, idx = vis['iuv_pred'][:3]
    ann = vis['iuv_pred'][3] if len(vis['iuv_pred']) > 3 else None
    hm = idx.shape[-1]
    assert 4 * hm == S, 'the part grid (4 rows of heat-map size %d) must be as tall as the image (%d)' % (hm, S)
    if iuv_renderer.out_size != hm:
        raise ValueError('result_panels: the IUV renderer draws %d pixels, the heat-maps have %d' % (iuv_renderer.out_size, hm))
    if mesh_renderer is not None and mesh_renderer.img_res != S:
        raise ValueError('result_panels: the mesh renderer draws %d pixels, the images have %d' % (mesh_renderer.img_res, S))
    glob = iuvmap.iuv_map2img(u, v, idx, ann)
    part = iuvmap.part_iuv_map2img(vis['part_iuv_pred'], dp2smpl_mapping)
    verts, cam = mesh_of(out, smpl)
    riuv = iuv_renderer.verts2uvimg(verts, cam)
    mesh = side = side_alpha = None
    if mesh_renderer is not None:
        mesh, _ = mesh_renderer(verts, cam, images)
        side, side_alpha = mesh_renderer(verts, cam, None, rot_y=math.radians(90))
    panels = ops.demo_compose(images, glob, part, riuv, mesh, side, side_alpha)
    planes = {'glob': glob, 'part': part, 'riuv': riuv, 'mesh': mesh, 'side': side, 'side_alpha': side_alpha}
    if texture is not None:
        tex, atlas = texture if isinstance(texture, tuple) else (texture, None)
        if atlas is None:
            atlas = tex.unwrap(images, verts, cam)
        index = [0] * B if atlas.shape[0] == 1 else None
        turned = []
        for deg in (90, 180):
            rgb, alpha = tex.render(verts, cam, atlas, None, rot_y=math.radians(deg), atlas_index=index, img_res=S)
            planes['tex%d' % deg], planes['tex%d_alpha' % deg] = rgb, alpha
            turned.append(torch.cat([rgb, alpha.unsqueeze(1)], 1).clamp(0.0, 1.0).permute(0, 2, 3, 1))
        planes['atlas'] = atlas
        panels = torch.cat([panels] + turned, 2)
    if return_planes:
        return panels, planes
    return panels
