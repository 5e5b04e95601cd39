"""Hand-over rules between the host wrappers of the drawing ops (ops.py) and their kernels that no other file asserts, at the smallest
shapes that can go wrong.  Every comparison is bit-equal: both sides run the same kernel on the same values, and bf16 -> fp32 is exact."""
import numpy as np
import pytest
import torch

import texture_oracle as to

pytestmark = pytest.mark.gpu

S = 16                                                                  # render size everywhere in this file


@pytest.fixture(scope='module')
def octa():
    """A closed mesh with outward winding, 6 vertices and 8 faces, in two poses: (faces [8,3] int32, vertices [2,6,3], cam [2,3]).
    At 16 pixels a unit of length is 16 * 16 * s / 448 pixels: s = 12 and 14 make bodies of about four pixels' radius.  The
    rasteriser's principal point at this size is 8 * 16 / 224 pixels (all four entries of K are scaled, as in the reference) and
    its y axis points up, so (tx, ty) near (1.5, 1.1) and (0.5, 0.9) put one body in each half of the frame."""
    v = 0.6 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    verts = np.stack([v @ to.rot_xyz(0.3, 0.5, 0.1).T, 0.8 * v @ to.rot_xyz(-0.4, 2.0, 0.7).T]).astype(np.float32)
    cam = np.array([[12., 1.5, 1.1], [14., 0.5, 0.9]], np.float32)
    return faces, torch.from_numpy(verts).cuda(), torch.from_numpy(cam).cuda()


def test_strided_bf16_sources_equal_their_contiguous_fp32_copies():
    from danet_densepose2smpl_amd import ops
    g = torch.Generator('cuda').manual_seed(11)
    big = [torch.randn(2, 8, 5, 12, device='cuda', generator=g).to(torch.bfloat16) for _ in range(3)]
    cut = [b[:, 2:5, :, 3:10] for b in big]                             # [N=2,K=3,H=5,W=7]: the channel and the width axis are cut
    assert all(t.shape == (2, 3, 5, 7) and not t.is_contiguous() for t in cut)
    wide = [t.float().contiguous() for t in cut]
    got = ops.iuv_map2img(*cut)
    assert got.shape == (2, 3, 5, 7) and got.dtype == torch.float32 and torch.equal(got, ops.iuv_map2img(*wide))
    assert len(got[:, 0].unique()) == 3                                 # every index occurs: the decode read all three sources
    sheet = ops.vis_grid(cut[0], cut[1], nrow=3, padding=1)
    assert sheet.shape == (3,) + ops.vis_grid_size(4, 5, 7, 3, 1) and torch.equal(sheet, ops.vis_grid(wide[0], wide[1], nrow=3, padding=1))
    assert torch.equal(ops.vis_grid(cut[2]), ops.vis_grid(wide[2])) and float(sheet.abs().max()) > 0


def test_mesh_alpha_is_the_part_mask_on_a_closed_mesh(octa):
    from danet_densepose2smpl_amd.renderer import MeshRenderer, PartRenderer
    faces, v, c = octa
    mask, _ = PartRenderer(faces, np.full((8, 3), 0.005, np.float32), np.zeros((100, 100, 100), np.float32), render_res=S)(v, c)
    _, alpha = MeshRenderer(faces, img_res=S)(v, c)
    assert torch.equal(alpha > 0, mask > 0) and torch.equal(alpha, mask)
    assert all(10 < int(m.sum()) < S * S - 10 for m in mask)            # a body and a background in both views


def test_mesh_shade_views_hand_scene_render_the_colours(octa):
    from danet_densepose2smpl_amd import datasets, ops, scene
    from danet_densepose2smpl_amd.renderer import ALBEDO, MeshRenderer, vertex_face_csr
    faces, v, _ = octa
    c = np.array([[12., 0.45, -0.1], [14., -0.45, 0.2]])                # (the scene cameras centre the crop at 7.5: one body in each half)
    cu = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    off, inc = vertex_face_csr(faces, 6)
    faces2 = cu(np.concatenate([faces, faces[:, ::-1]]), np.int32)      # both windings
    ws, rverts = ops.mesh_shade_vertices(v, cu(faces, np.int32), cu(off, np.int32), cu(inc, np.int32), MeshRenderer(faces, img_res=S).lights, 0., ALBEDO)
    first, vcol = ops.mesh_shade_views(ws, 2, 6)
    raw = ws[2 * 6 * 3:].view(2, 6, 3)                                  # the layout of csrc/vis_ops.hip: rotated vertices, then colours
    assert first.data_ptr() == rverts.data_ptr() == ws.data_ptr() and torch.equal(first, rverts) and torch.equal(vcol, raw)
    assert vcol.data_ptr() == raw.data_ptr() and float(vcol.min()) >= 0 and float(vcol.max()) > 0.1
    # one 16 x 16 frame whose box is the frame, two people in it
    _, tinv = datasets.crop_transforms(np.full((2, 2), S / 2.), np.full(2, S / 200.), np.zeros(2), S)
    k = scene.person_cameras(c, tinv, [[S, S]], [0, 0], S)
    src, off, shp = scene.pack_frames([np.random.default_rng(3).integers(0, 256, (S, S, 3), dtype=np.uint8)])
    args = (faces2, cu(k['cam_t'], np.float32), cu(k['proj'], np.float32), cu(k['dscale'], np.float32), cu([0, 0], np.int32),
            cu(src, np.uint8), cu(off, np.int64), cu(shp, np.int32))
    a = ops.scene_render(rverts, vcol, *args, return_aux=True)
    b = ops.scene_render(rverts, raw.clone(), *args, return_aux=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ids = a[1]
    assert set((ids[ids >= 0] // 16).unique().tolist()) == {0, 1} and bool((ids < 0).any())       # both people and some background


def _check_background(draw, images):
    rgb, alpha = draw(images)
    rgb0, alpha0 = draw(None)
    un = (alpha == 0).unsqueeze(1).expand_as(rgb)
    assert torch.equal(alpha0, alpha) and bool(un.any()) and not bool(un.all())
    assert torch.equal(rgb[un], images[un]) and not bool(rgb0[un].any()) and torch.equal(rgb0[~un], rgb[~un])


def test_uncovered_pixels_are_the_image_or_zero(octa):
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    from danet_densepose2smpl_amd.texture import TextureAtlas
    images = 0.25 + 0.5 * torch.rand(2, 3, S, S, device='cuda', generator=torch.Generator('cuda').manual_seed(5))      # (never 0)
    faces, v, c = octa
    rend = MeshRenderer(faces, img_res=S)
    _check_background(lambda img: rend(v, c, img), images)
    ico, _ = to.ico_mesh()
    vi = torch.from_numpy(np.stack([ico @ to.rot_xyz(*r).T.astype(np.float32) for r in to.VIEWS[:2]])).cuda()
    tex = TextureAtlas(densepose=to.ico_densepose(), size=8)
    atlas = tex.unwrap(images, vi, c)
    _check_background(lambda img: tex.render(vi, c, atlas, img, rot_y=0.4, img_res=S), images)
