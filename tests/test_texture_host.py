"""CPU side of the texture atlas: known answers that pin the restatement of tests/texture_oracle.py itself, the two bounds the
GPU tests use (made from the oracle alone), the host tables, the .obj writer and the sheet.

Measured on the oracle (texture_oracle.bounds()): float32 vs float64 on the main scene, certain texels and pixels only: unwrap
colours 6.0e-6, weights 4.2e-6 relative, no visibility flip, draw colours 1.2e-4 -> DELTA = 4 x 1.2e-4 = 4.8e-4.  (The scenes
hold noise images: a unit of colour per pixel and per texel multiplies every rounding of a coordinate, and near unobserved texels
the valid-tap ratio of the draw divides by a denominator as small as 1e-3.)  Round trip of the smooth image over 579 pixels:
0.0186 -> bound 1.5 x = 0.0279.  The uncertain share of mapped texels is 0.6 % .. 1.7 % on every scene (cap: 5 %)."""
import math

import numpy as np
import pytest
import torch

import texture_oracle as to


@pytest.fixture(scope='module')
def tb():
    return to.tables()


# ---- known answers -----------------------------------------------------------------------------------------------------------------
def test_tables_and_csr(tb):
    assert tb['vert_mapping'].shape == (60,) and tb['faces'].shape == (20, 3) and tb['uv'].dtype == np.float32
    assert tb['face_part'].tolist() == [k // 2 for k in range(20)]
    assert tb['part_off'].tolist() == [min(2 * p, 20) for p in range(25)]
    assert tb['part_faces'].tolist() == list(range(20))
    from danet_densepose2smpl_amd import assets, texture
    full = texture.atlas_tables(assets.make_synthetic_densepose(None, 0))
    for p in range(24):                                              # ascending face index within every part
        fs = full['part_faces'][full['part_off'][p]:full['part_off'][p + 1]]
        assert (np.diff(fs) > 0).all() and (full['face_part'][fs] == p).all()
    assert full['part_off'][24] == 13774
    dp = to.ico_densepose()
    dp['All_FaceIndices'] = dp['All_FaceIndices'] + 20
    with pytest.raises(ValueError, match='part'):
        texture.atlas_tables(dp)


def test_map_covers_the_expected_texels_and_the_tie_goes_to_the_lower_face(tb):
    T = 16
    face, bary = to.texture_map(tb, T)
    # chart triangle A (1,1) (7,1) (1,15) sixteenths: texel centres (j + 0.5, i + 0.5) with 14 (x - 1) + 6 (y - 1) <= 84 inside
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    x, y = j + 0.5, i + 0.5
    in_a = (x >= 1) & (y >= 1) & (14 * (x - 1) + 6 * (y - 1) <= 84)
    in_b = (x <= 15) & (y <= 15) & (14 * (15 - x) + 6 * (15 - y) <= 84)
    assert not (in_a & in_b).any()
    for p in range(9):
        assert np.array_equal(face[p] == 2 * p, in_a) and np.array_equal(face[p] == 2 * p + 1, in_b)
        assert ((face[p] == -1) == ~(in_a | in_b)).all()
    lower = (x + y <= 16) & (x >= 1) & (y >= 1)
    upper = (x + y > 16) & (x <= 15) & (y <= 15)
    assert (x + y == 16).sum() == 16                                 # the exact tie: texel centres on the shared diagonal
    assert np.array_equal(face[9] == 18, lower) and np.array_equal(face[9] == 19, upper)
    assert (face[10:] == -1).all()
    # barycentrics of a known texel of face 0: (x, y) = (1.5, 1.5) -> w0 = 1 - 0.5/6 - 0.5/14, w1 = 0.5/6
    assert bary[0, 1, 1].tolist() == [np.float32(1 - 0.5 / 6 - 0.5 / 14), np.float32(0.5 / 6)]


def _one_view(images, name='round', min_cos=0.1, cam=None, dtype=np.float64):
    sc = to.scene(name)
    mf, mb = to.texture_map(to.tables(), 16)
    cams = sc['cam'][:1] if cam is None else np.array([cam], np.float32)
    return mf, to.texture_unwrap(to.tables(), mf, mb, images, sc['vertices'][:1], cams, [0, 1], dtype, min_cos=min_cos)


def test_constant_image_gives_its_colour_on_every_observed_texel(tb):
    col = np.array([0.25, 0.5, 0.75], np.float32)
    img = np.broadcast_to(col[None, :, None, None], (1, 3, to.H, to.H)).copy()
    mf, (atlas, aux) = _one_view(img)
    seen = atlas[0, ..., 3] > 0
    assert seen.sum() > 300 and not seen[mf < 0].any()
    assert np.abs(atlas[0][seen][:, :3] - col.astype(np.float64)).max() < 1e-15
    assert (atlas[0][~seen] == 0).all()
    # the weight is the cosine of that view
    assert np.allclose(atlas[0, ..., 3].reshape(-1)[seen.reshape(-1)], aux['cos'][0][seen.reshape(-1)], rtol=0, atol=0)


def test_two_views_give_the_cosine_weighted_mean(tb):
    sc = to.scene('main')
    cols = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]], np.float32)
    img = np.broadcast_to(cols[:, :, None, None], (2, 3, to.H, to.H)).copy()
    mf, mb = to.texture_map(tb, 16)
    fused, _ = to.texture_unwrap(tb, mf, mb, img, sc['vertices'], sc['cam'], [0, 2])
    single, _ = to.texture_unwrap(tb, mf, mb, img, sc['vertices'], sc['cam'], [0, 1, 2])
    w0, w1 = single[0, ..., 3], single[1, ..., 3]
    in_both = (w0 > 0) & (w1 > 0)
    assert in_both.sum() > 50
    want = (w0[..., None] * cols[0].astype(np.float64) + w1[..., None] * cols[1].astype(np.float64)) / np.where(w0 + w1 > 0, w0 + w1, 1.0)[..., None]
    assert np.abs(fused[0, ..., :3] - want)[in_both].max() < 1e-15
    assert np.array_equal(fused[0, ..., 3], w0 + w1)
    only0 = (w0 > 0) & ~(w1 > 0)
    assert only0.sum() > 50 and np.array_equal(fused[0][only0], single[0][only0])


def test_hidden_averted_and_outside_texels_are_unobserved(tb):
    img = np.ones((1, 3, to.H, to.H), np.float32)
    mf, (atlas, aux) = _one_view(img)
    seen = (atlas[0, ..., 3] > 0).reshape(-1)
    cos, z, d = aux['cos'][0], aux['z'][0], aux['d'][0]
    mapped = (mf >= 0).reshape(-1)
    away = mapped & (cos <= 0.1)
    assert away.sum() > 300 and not seen[away].any()                  # facing away (the far half of the body)
    behind = mapped & np.isfinite(d) & (z > d + 0.02)
    assert behind.sum() > 100 and not seen[behind].any()              # behind a nearer face
    with_min = _one_view(img, min_cos=-2.0)[1][0]
    assert not (with_min[0, ..., 3].reshape(-1) > 0)[behind].any()    # ... whatever the facing rule says
    # a camera that pushes the body out of the frame: fewer observed texels, none whose nearest pixel is outside
    mf, (out, aux2) = _one_view(img, cam=to.CAMS[3])
    seen2 = (out[0, ..., 3] > 0).reshape(-1)
    outside = mapped & ((np.floor(aux2['c'][0] + 0.5) < 0) | (np.floor(aux2['c'][0] + 0.5) >= to.H))
    assert outside.sum() > 50 and not seen2[outside].any() and 0 < seen2.sum() < seen.sum()


def test_rasteriser_draws_the_faces_whose_cosine_is_positive(tb):
    """The orientation of the rule: (T1 - T0) x (T2 - T0) against -P is positive on the faces the rasteriser draws."""
    sc = to.scene('main')
    fidx, _ = to.depth_planes(tb, sc['vertices'], sc['cam'], to.H)
    mf, mb = to.texture_map(tb, 16)
    _, aux = to.texture_unwrap(tb, mf, mb, sc['images'], sc['vertices'], sc['cam'], [0, 2])
    for n in range(2):
        drawn = np.unique(fidx[n][fidx[n] >= 0])
        assert drawn.size >= 8
        for f in drawn:
            assert (aux['cos'][n][(mf == f).reshape(-1)] > 0).all()


# ---- conditions and bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['main', 'three', 'edge', 'round'])
def test_uncertain_share_is_at_most_five_percent(name):
    for T in (16, 12):
        sc, mf, _, aux = to.unwrap_scene(name, np.float64, T)
        unc = to.uncertain(aux, sc['view_off'])
        mapped = (mf >= 0).reshape(-1)
        share = (unc & mapped[None]).sum(1) / mapped.sum()
        print(name, T, share)
        assert (share <= 0.05).all()


def test_bounds_come_from_the_oracle_alone():
    b = to.bounds()
    print(b)
    assert b['flips'] == 0                                            # no visibility flip between float32 and float64 on certain texels
    assert b['DELTA'] == 4.0 * max(b['d_col'], b['d_draw']) and 0 < b['DELTA'] < 2e-3
    assert b['d_w'] < 1e-5                                            # the weight bound of the GPU tests leaves room for float32
    assert b['ROUND'] == 1.5 * b['round_err'] and b['round_pixels'] > 300 and 0.005 < b['ROUND'] < 0.05


def test_draw_known_answers(tb):
    """A constant atlas draws its colour; an empty atlas draws `fill`; uncovered pixels are the background, alpha the coverage."""
    sc = to.scene('round')
    atlas = np.zeros((1, 24, 16, 16, 4), np.float32)
    atlas[..., :3] = (0.2, 0.4, 0.6)
    atlas[..., 3] = 1.0
    rgb, alpha, den, _, fidx = to.draw_scene(atlas, sc, 0, math.radians(90), np.float64, sc['images'])
    cov = fidx[0] >= 0
    assert np.array_equal(alpha[0] > 0, cov) and cov.sum() > 500
    assert np.abs(rgb[0][:, cov] - np.array([0.2, 0.4, 0.6], np.float32).astype(np.float64)[:, None]).max() < 1e-15
    assert np.array_equal(rgb[0][:, ~cov], sc['images'][0][:, ~cov].astype(np.float64))
    assert np.abs(den[0][cov] - 1.0).max() < 1e-12
    rgb, _, den, _, _ = to.draw_scene(np.zeros_like(atlas), sc, 0, math.radians(90), np.float64)
    assert (rgb[0][:, cov] == 0.5).all() and (den[0][cov] == 0).all() and (rgb[0][:, ~cov] == 0).all()


# ---- the writer and the sheet ------------------------------------------------------------------------------------------------------
def _parse_obj(path):
    v, vt, f, mtl = [], [], [], None
    for line in open(path):
        k = line.split()
        if not k:
            continue
        if k[0] == 'v':
            v.append([float(x) for x in k[1:]])
        elif k[0] == 'vt':
            vt.append([float(x) for x in k[1:]])
        elif k[0] == 'f':
            f.append([[int(i) for i in c.split('/')] for c in k[1:]])
        elif k[0] == 'mtllib':
            mtl = k[1]
    return np.array(v), np.array(vt), np.array(f), mtl


def test_textured_obj_round_trips(tmp_path, tb):
    from danet_densepose2smpl_amd.texture import write_textured_obj
    verts, faces = to.ico_mesh()
    path = str(tmp_path / 'body.obj')
    write_textured_obj(path, verts, tb, 'body_texture.png')
    v, vt, f, mtl = _parse_obj(path)
    assert v.shape == (12, 3) and vt.shape == (60, 2) and f.shape == (20, 3, 2) and mtl == 'body.mtl'
    assert np.array_equal(v.astype(np.float32), verts)
    assert np.array_equal(f[..., 0] - 1, faces) and np.array_equal(f[..., 1] - 1, np.arange(60).reshape(20, 3))
    # corner 1 of face 15 (part 7: row 1, column 1; chart B, corner (9/16, 15/16))
    assert np.allclose(vt[15 * 3 + 1], [(1 + 9 / 16) / 6, 1 - (1 + 15 / 16) / 4], rtol=0, atol=1e-9)
    assert (vt >= 0).all() and (vt <= 1).all()
    text = open(str(tmp_path / 'body.mtl')).read()
    assert 'map_Kd body_texture.png' in text and 'newmtl skin' in text
    assert 'usemtl skin' in open(path).read()


def test_sheet_puts_part_k_at_row_k_div_6_column_k_mod_6():
    from danet_densepose2smpl_amd.texture import TextureAtlas
    T = 4
    tex = TextureAtlas(densepose=to.ico_densepose(), size=T)
    atlas = torch.arange(2 * 24 * T * T * 4, dtype=torch.float32).view(2, 24, T, T, 4)
    sheet = tex.sheet(atlas)
    assert sheet.shape == (2, 3, 4 * T, 6 * T)
    for k in (0, 5, 6, 17, 23):
        r, c = k // 6, k % 6
        assert torch.equal(sheet[:, :, r * T:(r + 1) * T, c * T:(c + 1) * T], atlas[:, k, :, :, :3].permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match='chart size'):
        TextureAtlas(densepose=to.ico_densepose(), size=1)


def test_host_checks_need_no_device():
    from danet_densepose2smpl_amd import ops
    assert ops.texture_view_offsets(None, 3).tolist() == [0, 1, 2, 3]
    assert ops.texture_view_offsets([0, 2, 2, 3], 3).tolist() == [0, 2, 2, 3]
    for bad in ([0, 1], [1, 3], [0, 2, 1, 3], [0.0, 3.0]):
        with pytest.raises(ValueError, match='view_off'):
            ops.texture_view_offsets(bad, 3)
    assert ops.texture_atlas_index(None, 2, 2).tolist() == [0, 1]
    for bad in ([0, 2], [-1, 0], [0]):
        with pytest.raises(ValueError, match='atlas_index'):
            ops.texture_atlas_index(bad, 2, 2)
    from danet_densepose2smpl_amd.texture import TextureAtlas
    tex = TextureAtlas(densepose=to.ico_densepose(), size=8)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        tex.unwrap(torch.zeros(1, 3, 64, 64), torch.zeros(1, 12, 3), torch.ones(1, 3))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        tex.render(torch.zeros(1, 12, 3), torch.ones(1, 3), torch.zeros(1, 24, 8, 8, 4))
