"""IUV_Renderer with the reference's call signature (/root/reference/utils/renderer.py:202-298).
The rasterisation (neural_renderer in the reference) is the HIP kernel of csrc/iuv_raster.hip.  MeshRenderer is the shaded
view of /root/reference/utils/renderer.py:125-199 (opendr there) on the same rasteriser plus csrc/vis_ops.hip."""
from collections import namedtuple

import numpy as np
import torch

from . import assets, ops
from ._lib import require_gpu


class DeviceTables(dict):
    """What a renderer uploads once: tables(key, build) -> build(), made at the first call with `key` (the device, as a string,
    plus any extra such as the vertex count) and kept."""

    def tables(self, key, build):
        if key not in self:
            self[key] = build()
        return self[key]


def upload(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def fill_back(faces):
    """Every face also with the opposite winding, [F,3] -> [2F,3] int32 (the rasteriser culls faces of non-positive signed area)."""
    faces = np.asarray(faces).reshape(-1, 3)
    return np.concatenate([faces, faces[:, ::-1]], 0).astype(np.int32)


def plain_tables(num_verts, num_faces, device):
    """What the rasteriser takes where a mesh is drawn as it is and only coverage, face index and depth are read: (the identity
    vertex mapping [num_verts] int32, a zero colour per face [num_faces,3] f32); a count of None leaves that half out (None)."""
    return (None if num_verts is None else torch.arange(num_verts, dtype=torch.int32, device=device),
            None if num_faces is None else torch.zeros(num_faces, 3, dtype=torch.float32, device=device))


class IUV_Renderer(object):
    def __init__(self, orig_size=224, out_size=56, focal_length=5000., densepose=None, smpl_model=None):
        """densepose: dict with the UV_Processed.mat fields (assets.load_densepose_mat), or None for
        the seeded synthetic topology."""
        self.orig_size = orig_size
        self.out_size = out_size
        self.focal_length = focal_length
        K = np.array([[focal_length, 0., orig_size / 2.], [0., focal_length, orig_size / 2.], [0., 0., 1.]])
        if orig_size != 224:                     # renderer.py:219-224: all four entries are scaled
            sc = orig_size / float(224)
            K[0, 0] *= sc; K[1, 1] *= sc; K[0, 2] *= sc; K[1, 2] *= sc
        self.K = torch.FloatTensor(K[None, :, :])
        self.R = torch.FloatTensor(np.eye(3)[None, :, :])
        self.t = torch.FloatTensor(np.array([0, 0, 5])[None, None, :])
        if densepose is None:
            densepose = assets.make_synthetic_densepose(smpl_model, 0)
        vm, faces, tex = assets.densepose_render_tables(densepose)
        self.vert_mapping = torch.from_numpy(vm.astype(np.int64))
        self.faces = torch.from_numpy(faces[None, :, :])
        self.textures = torch.from_numpy(tex[None, :, None, None, None, :])
        self._np = (vm, faces, tex)
        self._cache = DeviceTables()

    def _dev(self, device):
        return self._cache.tables(str(device), lambda: tuple(upload(a, device) for a in self._np))

    def verts2uvimg(self, verts, cam, return_aux=False):
        """verts [B,6890,3], cam [B,3] (s,x,y) -> IUV image [B,3,out,out]."""
        vm, faces, tex = self._dev(verts.device)
        return ops.iuv_raster(verts, cam, vm, faces, tex, self.focal_length, self.orig_size, self.out_size,
                              return_aux=return_aux)

    def camera_matrix(self, cam):
        """renderer.py:280-298."""
        B = cam.size(0)
        K = self.K.repeat(B, 1, 1).to(cam.device)
        R = self.R.repeat(B, 1, 1).to(cam.device)
        t = torch.stack([cam[:, 1], cam[:, 2], 2 * self.focal_length / (self.orig_size * cam[:, 0] + 1e-9)], dim=-1)
        return K, R, t.unsqueeze(1)


class PartRenderer(object):
    """Silhouette mask and body-part segmentation of a posed SMPL mesh, the call signature of
    /root/reference/utils/part_utils.py:8-53 (used by the LSP mask / part evaluation, eval.py:218-246).

    The reference renders per-face colours with neural_renderer (fill_back on, no anti-aliasing, ambient light only) and
    looks the part id of a pixel up as cube_parts[floor(100 * rgb)].  Here the HIP rasteriser (csrc/iuv_raster.hip, the
    kernel behind IUV_Renderer) draws the same flat per-face colours -- both windings of every face, which is what
    fill_back means -- and the lookup is one gather.  `faces` [F,3] int (the SMPL topology), `textures` the
    VERTEX_TEXTURE_FILE array ([1,F,t,t,t,3] or [F,3]; flat per face), `cube_parts` the CUBE_PARTS_FILE table."""

    def __init__(self, faces, textures, cube_parts, focal_length=5000., render_res=224):
        self.focal_length = focal_length
        self.render_res = render_res
        faces = np.asarray(faces).astype(np.int32).reshape(-1, 3)
        tex = np.asarray(textures, dtype=np.float32)
        tex = tex.reshape(tex.shape[-5], -1, 3)[:, 0, :] if tex.ndim >= 5 else tex.reshape(-1, 3)
        if tex.shape[0] != faces.shape[0]:
            raise ValueError('textures: %d faces, topology: %d' % (tex.shape[0], faces.shape[0]))
        self.faces = torch.from_numpy(faces)
        self.textures = torch.from_numpy(tex)
        self.cube_parts = torch.as_tensor(np.asarray(cube_parts), dtype=torch.float32)
        self._np = (fill_back(faces), np.concatenate([tex, tex], 0))
        self._cache = DeviceTables()

    def _dev(self, device, nv):
        f2, t2 = self._np
        return self._cache.tables((str(device), nv), lambda: (plain_tables(nv, None, device)[0], upload(f2, device), upload(t2, device),
                                                         self.cube_parts.to(device)))

    def get_parts(self, parts, mask):
        """part_utils.py:27-35: rendered colours [B,3,H,W] + mask [B,H,W] -> part indices [B,H,W] (long)."""
        bn, c, h, w = parts.shape
        cube = self.cube_parts.to(parts.device)
        idx = torch.floor(100 * parts.permute(0, 2, 3, 1).contiguous().view(-1, 3)).long()
        out = cube[idx[:, 0], idx[:, 1], idx[:, 2], None] * mask.reshape(-1, 1)
        return out.view(bn, h, w).long()

    def __call__(self, vertices, camera):
        """vertices [B,V,3], camera [B,3] (s, tx, ty) -> (mask [B,H,W] float, parts [B,H,W] long)."""
        vm, faces, tex, _ = self._dev(vertices.device, vertices.shape[1])
        rgb, fidx, _ = ops.iuv_raster(vertices, camera, vm, faces, tex, self.focal_length, self.render_res, self.render_res,
                                      return_aux=True)
        mask = (fidx >= 0).to(torch.float32)
        return mask, self.get_parts(rgb, mask)


def rotateY(points, angle):
    """renderer.py:97-104: row vectors times the rotation about y, in double."""
    ry = np.array([[np.cos(angle), 0., np.sin(angle)], [0., 1., 0.], [-np.sin(angle), 0., np.cos(angle)]])
    return np.dot(points, ry)


def vertex_face_csr(faces, num_verts):
    """Vertex -> incident-faces table in CSR form: (offsets [V+1] int32, face ids [3F] int32), the faces of a vertex in
    ascending face order (a face that names a vertex twice is listed twice)."""
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= num_verts):
        raise ValueError('faces name vertex %d of %d' % (int(faces.max()), num_verts))
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind='stable')                 # stable: ascending face index within a vertex
    off = np.zeros(num_verts + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=num_verts), out=off[1:])
    return off.astype(np.int32), (order // 3).astype(np.int32)


LIGHT_POSITIONS = ((-200., -100., -100.), (800., 10., 300.), (-500., 500., 1000.))      # renderer.py:160-184, before rotateY(120 deg)
LIGHT_COLORS = ((1., 1., 1.), (1., 1., 1.), (.7, .7, .7))
ALBEDO = 0.9
# MeshRenderer.tables: identity vertex mapping, faces, fill_back(faces), vertex_face_csr's two arrays, the rasteriser's unused colours
MeshTables = namedtuple('MeshTables', ['vert_mapping', 'faces', 'faces2', 'csr_off', 'csr_face', 'tex'])


class MeshRenderer(object):
    """Shaded view of a mesh over an image: `opendr_render.render` (/root/reference/utils/renderer.py:125-199) under the
    shading rule of DESIGN.md (opendr is absent; what it does beyond that rule is unpinned).

    MeshRenderer(faces, focal_length=5000., img_res=224, color=None)
    __call__(vertices [B,V,3], cam [B,3] (s, tx, ty), images=None | [B,3,R,R], rot_y=0.) -> (rgb [B,3,R,R] in [0,1], alpha [B,R,R])

    Coverage and depth are the HIP rasteriser's with both windings of every face (PartRenderer's mask, bit for bit); the
    colours are two launches of csrc/vis_ops.hip.  `rot_y` (radians) multiplies the vertices by rotateY first (the side view)."""

    def __init__(self, faces, focal_length=5000., img_res=224, color=None):
        self.focal_length = focal_length
        self.img_res = int(img_res)
        faces = np.asarray(faces).astype(np.int32).reshape(-1, 3)
        self.faces = torch.from_numpy(faces.copy())
        cols = LIGHT_COLORS if color is None else (tuple(float(c) for c in np.broadcast_to(np.asarray(color, dtype=np.float64), (3,))),) * 3
        pos = [rotateY(np.array(p), np.radians(120)) for p in LIGHT_POSITIONS]
        self.lights = [float(x) for p in pos for x in p] + [float(x) for c in cols for x in c]
        self._faces_np = faces
        self._cache = DeviceTables()

    def tables(self, device, nv):
        """-> MeshTables on `device` for a mesh of `nv` vertices, made once."""
        def build():
            f = self._faces_np
            off, inc = vertex_face_csr(f, nv)
            vm, tex = plain_tables(nv, 2 * f.shape[0], device)
            return MeshTables(vm, upload(f, device), upload(fill_back(f), device), upload(off, device), upload(inc, device), tex)
        return self._cache.tables((str(device), nv), build)

    def __call__(self, vertices, cam, images=None, rot_y=0.):
        require_gpu(vertices, 'MeshRenderer')
        R = self.img_res
        t = self.tables(vertices.device, vertices.shape[1])
        ws, rverts = ops.mesh_shade_vertices(vertices, t.faces, t.csr_off, t.csr_face, self.lights, rot_y, ALBEDO)
        _, fidx, _ = ops.iuv_raster(rverts, cam, t.vert_mapping, t.faces2, t.tex, self.focal_length, R, R, return_aux=True)
        return ops.mesh_shade_pixels(ws, cam, vertices.shape[1], t.faces2, fidx, images, self.focal_length, R)
