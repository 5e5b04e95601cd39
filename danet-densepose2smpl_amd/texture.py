"""Texture atlases over the 24 DensePose charts (DESIGN.md "texture rule"; csrc/texture_ops.hip): photographs are unwrapped to
the charts through the predicted mesh, several views of one person are fused by their facing cosine, and the textured mesh is
drawn back from any side or exported as a Wavefront .obj with a texture sheet.

    tex = TextureAtlas(densepose=None, smpl_model=None, size=64)
    atlas = tex.unwrap(images, vertices, cam)                     # [P,24,T,T,4]: r, g, b, summed weight
    rgb, alpha = tex.render(vertices, cam, atlas, rot_y=math.radians(90))
    write_png(path, to_uint8(tex.sheet(atlas)[0]))                # 4 x 6 charts, the grid of the part panels

Launches of this package: unwrap = 3 of the rasteriser (the depth plane) + 1; render = 1 rotation + 3 of the rasteriser + 1;
the texel map is one launch per device, made at the first call.  Nothing allocates by data and nothing synchronises, so after
one warm-up call both capture under torch.cuda.graph."""
import os

import numpy as np
import torch

from . import assets, ops
from .renderer import DeviceTables, plain_tables, upload

PARTS = 24
SHEET_ROWS, SHEET_COLS = 4, 6


def atlas_tables(densepose):
    """The host tables of the texture rule from a DensePose dict (the one assets.densepose_render_tables takes): vert_mapping
    [NDV] int32, faces [F,3] int32 over the DensePose vertices, uv [NDV,2] f32 = (All_U_norm, All_V_norm), face_part [F] int32 =
    All_FaceIndices - 1, and the faces of every part in ascending index as a CSR (part_off [25], part_faces [F] int32)."""
    vm, faces, _ = assets.densepose_render_tables(densepose)
    ndv = vm.shape[0]
    uv = np.stack([np.asarray(densepose['All_U_norm'], np.float64).reshape(-1), np.asarray(densepose['All_V_norm'], np.float64).reshape(-1)], 1)
    part = np.asarray(densepose['All_FaceIndices']).reshape(-1).astype(np.int64) - 1
    if uv.shape[0] != ndv or part.shape[0] != faces.shape[0]:
        raise ValueError('atlas_tables: %d vertices with %d UV pairs, %d faces with %d part indices' % (ndv, uv.shape[0], faces.shape[0], part.shape[0]))
    if faces.size == 0 or faces.min() < 0 or faces.max() >= ndv or vm.min() < 0 or part.min() < 0 or part.max() >= PARTS:
        raise ValueError('atlas_tables: a face names a vertex outside [0, %d), a negative mesh vertex or a part outside 1..%d' % (ndv, PARTS))
    order = np.argsort(part, kind='stable')                     # stable: ascending face index within a part
    off = np.zeros(PARTS + 1, np.int64)
    np.cumsum(np.bincount(part, minlength=PARTS), out=off[1:])
    return {'vert_mapping': vm.astype(np.int32), 'faces': np.ascontiguousarray(faces, np.int32), 'uv': np.ascontiguousarray(uv, np.float32),
            'face_part': part.astype(np.int32), 'part_off': off.astype(np.int32), 'part_faces': order.astype(np.int32)}


def corner_vt(tables):
    """The sheet coordinates of every face corner [F,3,2]: vt = ((col + U) / 6, 1 - (row + V) / 4) with the face's part at row
    part // 6, column part % 6 of the sheet (the image's top row is vt = 1)."""
    uv = tables['uv'].astype(np.float64)[tables['faces']]                      # [F,3,2]
    part = tables['face_part'].astype(np.int64)[:, None]
    return np.stack([(part % SHEET_COLS + uv[..., 0]) / SHEET_COLS, 1.0 - (part // SHEET_COLS + uv[..., 1]) / SHEET_ROWS], -1)


def write_textured_obj(path, vertices, atlas_tables, texture_name):
    """A Wavefront .obj with its .mtl beside it: one `v` line per mesh vertex, three `vt` lines per face (one per corner, so a
    vertex on a chart seam gets the coordinates of each chart), faces as `f a/ta b/tb c/tc` (1-based) over the mesh vertices.
    The .mtl names `texture_name` (TextureAtlas.sheet written as an image) as map_Kd."""
    t = atlas_tables
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = t['vert_mapping'].astype(np.int64)[t['faces']]
    if f.max() >= v.shape[0]:
        raise ValueError('write_textured_obj: the topology names vertex %d of %d' % (int(f.max()), v.shape[0]))
    vt = corner_vt(t).reshape(-1, 2)
    stem = os.path.splitext(path)[0]
    with open(stem + '.mtl', 'w') as fh:
        fh.write('newmtl skin\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n' % texture_name)
    with open(path, 'w') as fh:
        fh.write('mtllib %s\nusemtl skin\n' % os.path.basename(stem + '.mtl'))
        for x in v:
            fh.write('v %.9g %.9g %.9g\n' % (x[0], x[1], x[2]))
        for x in vt:
            fh.write('vt %.9g %.9g\n' % (x[0], x[1]))
        for k, c in enumerate(f):
            fh.write('f %d/%d %d/%d %d/%d\n' % (c[0] + 1, 3 * k + 1, c[1] + 1, 3 * k + 2, c[2] + 1, 3 * k + 3))


class TextureAtlas(object):
    """TextureAtlas(densepose=None, smpl_model=None, size=64, focal_length=5000.): `densepose` a dict with the UV_Processed.mat
    fields, or None for the seeded synthetic topology (as IUV_Renderer); `size` the side T of a chart in texels."""

    def __init__(self, densepose=None, smpl_model=None, size=64, focal_length=5000.):
        self.size = ops._texture_size(size)
        self.focal_length = float(focal_length)
        if densepose is None:
            densepose = assets.make_synthetic_densepose(smpl_model, 0)
        self.tables = atlas_tables(densepose)
        self.num_verts = int(self.tables['vert_mapping'].max()) + 1           # the mesh must have at least this many vertices
        self._cache = DeviceTables()

    def _dev(self, device):
        """The tables and the texel map on `device`, made once."""
        def build():
            d = {k: upload(a, device) for k, a in self.tables.items()}
            d['tex'] = plain_tables(None, d['faces'].shape[0], device)[1]                    # (the rasteriser's colours are not used)
            d['no_faces'] = torch.zeros(1, 3, dtype=torch.int32, device=device)
            d['csr_face'] = torch.zeros(1, dtype=torch.int32, device=device)
            d['map_face'], d['map_bary'] = ops.texture_map(d['uv'], d['faces'], d['part_off'], d['part_faces'], self.size)
            return d
        return self._cache.tables(str(device), build)

    def texel_map(self, device):
        """-> (face [24,T,T] int32, bary [24,T,T,2] f32) on `device`."""
        d = self._dev(device)
        return d['map_face'], d['map_bary']

    def _check_mesh(self, what, vertices):
        if vertices.shape[1] < self.num_verts:
            raise ValueError('%s: vertices %s (the topology names %d mesh vertices)' % (what, tuple(vertices.shape), self.num_verts))

    def unwrap(self, images, vertices, cam, view_offsets=None, depth_tol=0.02, min_cos=0.1):
        """images [N,3,H,H] in [0,1], vertices [N,NV,3], cam [N,3] (s, tx, ty) -> atlas [P,24,T,T,4].  view_offsets: host integers
        [P+1], the views of person p being view_offsets[p] .. view_offsets[p+1] - 1 (None: every view is a person of its own).  A
        texel no view observes, and every texel of a person without views, is 0."""
        img, v, c = ops.texture_views(images, vertices, cam, 'texture_unwrap')             # (every refusal comes before the first launch)
        self._check_mesh('texture unwrap', v)
        N, H = img.shape[0], img.shape[2]
        off = ops.texture_view_offsets(view_offsets, N)
        d = self._dev(v.device)
        if N:
            _, _, depth = ops.iuv_raster(v, c, d['vert_mapping'], d['faces'], d['tex'], self.focal_length, H, H, return_aux=True)
        else:
            depth = torch.empty(0, H, H, device=v.device, dtype=torch.float32)
        return ops.texture_unwrap(img, v, c, depth, off, d['vert_mapping'], d['faces'], d['map_face'], d['map_bary'],
                                  self.focal_length, depth_tol, min_cos)

    def render(self, vertices, cam, atlas, images=None, rot_y=0., atlas_index=None, fill=(0.5, 0.5, 0.5), img_res=None):
        """vertices [N,NV,3], cam [N,3], atlas [P,24,T,T,4] -> (rgb [N,3,S,S], alpha [N,S,S]); S is the images' size, without
        images `img_res` (default 224).  rot_y (radians) turns the body as MeshRenderer does; atlas_index: host integers [N]
        naming the person whose atlas a view draws (None: view n draws atlas n); a pixel whose chart region nothing was
        unwrapped to is `fill`; a pixel no face covers is the image's (or 0) with alpha 0."""
        img, v, c = ops.texture_views(images, vertices, cam, 'texture_render', optional=True)
        self._check_mesh('texture render', v)
        N, NV = v.shape[0], v.shape[1]
        _, P, T = ops.texture_atlas(atlas)
        if T != self.size:
            raise ValueError('texture render: atlas %s, expected [P,%d,%d,%d,4]' % (tuple(atlas.shape), PARTS, self.size, self.size))
        idx = ops.texture_atlas_index(atlas_index, N, P)
        S = int(img.shape[2] if img is not None else (224 if img_res is None else img_res))
        d = self._dev(v.device)
        csr_off = self._cache.tables((str(v.device), NV), lambda: torch.zeros(NV + 1, dtype=torch.int32, device=v.device))
        # the rotation is MeshRenderer's vertex launch with an empty vertex -> face table (its colours are not used)
        _, rverts = ops.mesh_shade_vertices(v, d['no_faces'], csr_off, d['csr_face'], (0.,) * 18, rot_y, 0.)
        _, fidx, _ = ops.iuv_raster(rverts, c, d['vert_mapping'], d['faces'], d['tex'], self.focal_length, S, S, return_aux=True)
        return ops.texture_render(rverts, c, d['vert_mapping'], d['faces'], d['uv'], d['face_part'], fidx, atlas, idx, img,
                                  self.focal_length, fill)

    def sheet(self, atlas):
        """atlas [P,24,T,T,4] -> [P,3,4T,6T]: the colours of part k at row k // 6, column k % 6 (the grid of the part panels)."""
        P, T = atlas.shape[0], self.size
        if tuple(atlas.shape[1:]) != (PARTS, T, T, 4):
            raise ValueError('texture sheet: atlas %s, expected [P,%d,%d,%d,4]' % (tuple(atlas.shape), PARTS, T, T))
        return atlas[..., :3].reshape(P, SHEET_ROWS, SHEET_COLS, T, T, 3).permute(0, 5, 1, 3, 2, 4).reshape(P, 3, SHEET_ROWS * T, SHEET_COLS * T)
