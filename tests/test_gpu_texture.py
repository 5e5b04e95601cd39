"""The texture atlas on the device (csrc/texture_ops.hip) against the restatement of tests/texture_oracle.py.

Bounds.  Map: face and barycentrics bit-equal (double arithmetic in the written order on both sides).  Unwrap and draw: on texels
and pixels that are not `uncertain`, the observed flag is equal, the weight is within relative 1e-5 and colours are within DELTA =
4 x the oracle's own float32-vs-float64 difference (texture_oracle.bounds(); test_texture_host.py asserts how it is made; measured
4.8e-4 -- the scenes hold noise images, a unit of colour per pixel and per texel, and the valid-tap ratio of the draw amplifies a
rounding of the bilinear weights near unobserved texels).  Round trip: 1.5 x the oracle's largest error, 0.028.  Alpha, the
background, the fill regions, the empty person and the replays are exact."""
import math

import numpy as np
import pytest
import torch

import texture_oracle as to

pytestmark = pytest.mark.gpu

W_REL = 1e-5


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def ico():
    from danet_densepose2smpl_amd.texture import TextureAtlas
    return TextureAtlas(densepose=to.ico_densepose(), size=to.T_MAIN)


def _scene_cu(sc):
    return _cu(sc['images']), _cu(sc['vertices']), _cu(sc['cam'])


# ------------------------------------------------------------------------------------------------------------------ 1. map
def _check_map(tex, tables, T):
    face, bary = tex.texel_map(torch.device('cuda:0'))
    rf, rb = to.texture_map(tables, T)
    assert np.array_equal(face.cpu().numpy(), rf)
    assert np.array_equal(bary.cpu().numpy().view(np.uint32), rb.view(np.uint32))
    return rf


@pytest.mark.parametrize('T', [16, 12])
def test_map_bit_equal_with_tie_and_empty_parts(T):
    from danet_densepose2smpl_amd.texture import TextureAtlas
    tex = TextureAtlas(densepose=to.ico_densepose(), size=T)
    rf = _check_map(tex, tex.tables, T)
    assert (rf[10:] == -1).all() and (rf[:10] >= 0).any(axis=(1, 2)).all()
    if T == 16:
        diag = rf[9][np.arange(16), 15 - np.arange(16)]                  # texel centres on u + v = 1: both faces hold them
        assert (diag[1:15] == 18).all() and diag[0] == diag[15] == -1    # (the two end texels lie outside the chart triangles)


def test_map_full_size_topology(smpl_model):
    from danet_densepose2smpl_amd.texture import TextureAtlas
    tex = TextureAtlas(smpl_model=smpl_model, size=32)
    assert tex.tables['faces'].shape == (13774, 3) and tex.tables['uv'].shape == (7829, 2)
    rf = _check_map(tex, tex.tables, 32)
    assert (rf >= 0).mean() > 0.1


# ------------------------------------------------------------------------------------------------------------------ 2, 3. unwrap
def _check_unwrap(ico, name):
    sc, mf, ref, aux = to.unwrap_scene(name, np.float64)
    img, v, c = _scene_cu(sc)
    atlas = ico.unwrap(img, v, c, view_offsets=sc['view_off'])
    got = atlas.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    cert = ~to.uncertain(aux, sc['view_off']).reshape(ref.shape[:4]) & (mf >= 0)[None]
    seen_r, seen_g = ref[..., 3] > 0, got[..., 3] > 0
    assert np.array_equal(seen_r[cert], seen_g[cert])
    assert not seen_g[:, mf < 0].any() and (got[~seen_g] == 0).all()
    both = cert & seen_r
    d_w = (np.abs(got[..., 3] - ref[..., 3]) / np.where(both, ref[..., 3], 1.0))[both].max()
    d_c = np.abs(got[..., :3] - ref[..., :3])[both].max()
    print('unwrap %s: %d certain observed texels, weight rel %.3g, colour %.3g (DELTA %.3g)' % (name, both.sum(), d_w, d_c, to.bounds()['DELTA']))
    assert d_w <= W_REL
    assert d_c <= to.bounds()['DELTA']
    return sc, atlas, both


@pytest.mark.parametrize('name', ['main', 'three'])
def test_unwrap_vs_oracle(ico, name):
    _, _, both = _check_unwrap(ico, name)
    assert both.sum() > 200


def test_unwrap_out_of_frame_view_and_person_without_views(ico):
    sc, atlas, both = _check_unwrap(ico, 'edge')
    assert atlas.shape[0] == 3 and not atlas[1].any()
    assert both[0].sum() > 50 and both[2].sum() > 50


# ------------------------------------------------------------------------------------------------------------------ 4. draw
@pytest.fixture(scope='module')
def main_atlas():
    sc, mf, ref, _ = to.unwrap_scene('main', np.float64)
    return sc, ref.astype(np.float32)


def _robustly_unseen(atlas32, taps):
    """Pixels all of whose taps, and the ring of texels around them, are unobserved: `fill` whatever the roundings."""
    T = atlas32.shape[2]
    w = atlas32[0, ..., 3]                                               # [24,T,T]
    t = np.where(taps[..., 0] >= 0, taps[..., 0], 0)
    part, i0, j0 = t // (T * T), (t // T) % T, t % T
    out = taps[..., 0] >= 0
    for di in range(-1, 3):
        for dj in range(-1, 3):
            out &= w[part, np.clip(i0 + di, 0, T - 1), np.clip(j0 + dj, 0, T - 1)] == 0
    return out


@pytest.mark.parametrize('background', [False, True])
@pytest.mark.parametrize('deg', [0, 90])
def test_draw_vs_oracle(ico, main_atlas, deg, background):
    sc, at = main_atlas
    rot = math.radians(deg)
    images = sc['images'] if background else None
    ref, _, den, taps, fidx = to.draw_scene(at, sc, 0, rot, np.float64, images)
    img, v, c = _scene_cu(sc)
    fill = (0.25, 0.5, 0.75)
    rgb, alpha = ico.render(v[:1], c[:1], _cu(at), img[:1] if background else None, rot_y=rot, fill=fill, img_res=to.H)
    rgb, alpha = rgb.cpu().numpy(), alpha.cpu().numpy()
    covered = fidx >= 0
    assert covered.sum() > 500
    assert np.array_equal(alpha, covered.astype(np.float32))
    bg = sc['images'][:1] if background else np.zeros_like(rgb)
    assert np.array_equal(rgb[:, :, ~covered[0]], bg[:, :, ~covered[0]])
    unseen = _robustly_unseen(at, taps)
    for ch in range(3):
        assert (rgb[:, ch][unseen] == np.float32(fill[ch])).all()
    certain = den >= to.EPS
    d = np.abs(rgb.astype(np.float64) - ref)[:, :, certain[0]].max()
    print('draw %d deg: %d covered, %d certain, %d robustly unseen, colour %.3g (DELTA %.3g)' % (deg, covered.sum(), certain.sum(), unseen.sum(), d, to.bounds()['DELTA']))
    assert certain.sum() > 200
    if deg == 90:
        assert unseen.sum() > 20                                         # the side no view saw
    assert d <= to.bounds()['DELTA']


# ------------------------------------------------------------------------------------------------------------------ 5. round trip
def test_round_trip_on_the_device(ico):
    sc, mf, ref, _ = to.unwrap_scene('round', np.float64)
    img, v, c = _scene_cu(sc)
    atlas = ico.unwrap(img, v, c)
    rgb, _ = ico.render(v, c, atlas, None, img_res=to.H)
    _, _, _, taps, fidx = to.draw_scene(ref.astype(np.float32), sc, 0, 0.0, np.float64)
    mask = to.round_trip_mask(ref, mf, taps, fidx)
    err = np.abs(rgb.cpu().numpy().astype(np.float64)[0] - sc['images'][0].astype(np.float64))[:, mask[0]].max()
    print('round trip: %d pixels, error %.4g (bound %.4g)' % (mask.sum(), err, to.bounds()['ROUND']))
    assert mask.sum() > 300
    assert err <= to.bounds()['ROUND']


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_runs_equal_and_graph_replay(ico):
    sc = to.scene('main')
    img, v, c = _scene_cu(sc)

    def f():
        atlas = ico.unwrap(img, v, c, view_offsets=sc['view_off'])
        rgb, alpha = ico.render(v, c, atlas, img, rot_y=math.radians(90), atlas_index=[0, 0])
        return atlas, rgb, alpha
    eager = [t.clone() for t in f()]
    for a, b in zip(eager, f()):
        assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = f()
    for _ in range(2):
        for t in static:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, static):
            assert torch.equal(a, b)
    del g


# ------------------------------------------------------------------------------------------------------------------ 7. panels
def test_result_panels_texture_appends_two_panels():
    from danet_densepose2smpl_amd import demo
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    from danet_densepose2smpl_amd.texture import TextureAtlas
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    cfg_from_dict({'DANET.INIMG_SIZE': 64, 'DANET.HEATMAP_SIZE': 16})
    try:
        S, B = 64, 2
        torch.manual_seed(0)
        model = DaNet(default_options(B), None, pretrained=False).cuda().eval()
        images = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
        smpl = model.iuv2smpl.smpl
        mr = MeshRenderer(smpl.faces, img_res=S)
        tex = TextureAtlas(size=16)
        out = model.infer_net(images)
        for rend in (mr, None):
            plain = demo.result_panels(out, images, smpl, model.iuv_renderer, rend)
            strip, planes = demo.result_panels(out, images, smpl, model.iuv_renderer, rend, return_planes=True, texture=tex)
            W = plain.shape[2]
            assert strip.shape == (B, S, W + 2 * S, 4)
            assert torch.equal(strip[:, :, :W], plain)
            assert torch.equal(strip[:, :, W:W + S, 3], planes['tex90_alpha']) and torch.equal(strip[:, :, W + S:, 3], planes['tex180_alpha'])
            assert torch.equal(strip[:, :, W + S:, :3], planes['tex180'].clamp(0, 1).permute(0, 2, 3, 1))
        # an atlas made elsewhere: one per image gives the same strip; one for all draws person 0's colours on every body
        assert torch.equal(demo.result_panels(out, images, smpl, model.iuv_renderer, None, texture=(tex, planes['atlas'])), strip)
        fused = demo.result_panels(out, images, smpl, model.iuv_renderer, None, texture=(tex, planes['atlas'][:1].contiguous()))
        assert torch.equal(fused[:1], strip[:1]) and torch.equal(fused[1:, :, :W], strip[1:, :, :W])
        # the stage captures
        f = lambda: demo.result_panels(out, images, smpl, model.iuv_renderer, mr, texture=tex)           # noqa: E731
        eager = f().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                f()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static = f()
        static.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)
        del g
    finally:
        reset_cfg()


# ------------------------------------------------------------------------------------------------------------------ 8. errors
def test_errors_are_raised_before_any_launch(ico):
    from danet_densepose2smpl_amd import ops
    from danet_densepose2smpl_amd.texture import TextureAtlas
    sc = to.scene('main')
    img, v, c = _scene_cu(sc)
    atlas = ico.unwrap(img, v, c)
    with pytest.raises(ValueError, match='chart size'):
        TextureAtlas(densepose=to.ico_densepose(), size=1)
    d = ico._dev(v.device)
    with pytest.raises(ValueError, match='chart size'):
        ops.texture_map(d['uv'], d['faces'], d['part_off'], d['part_faces'], 1)
    with pytest.raises(ValueError, match='square'):
        ico.unwrap(img[:, :, :, :32].contiguous(), v, c)
    for bad in ([0, 1], [1, 2], [0, 2, 1, 2], [0, 3], [0]):
        with pytest.raises(ValueError, match='view_off'):
            ico.unwrap(img, v, c, view_offsets=bad)
    for bad in ([0, 2], [-1, 0], [0]):
        with pytest.raises(ValueError, match='atlas_index'):
            ico.render(v, c, atlas, atlas_index=bad, img_res=to.H)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ico.unwrap(img.cpu(), v.cpu(), c.cpu())
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ico.render(v.cpu(), c.cpu(), atlas.cpu())
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.texture_map(d['uv'].cpu(), d['faces'].cpu(), d['part_off'].cpu(), d['part_faces'].cpu(), 16)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.texture_unwrap(img.cpu(), v, c, torch.zeros(2, 64, 64).cuda(), None, d['vert_mapping'], d['faces'], d['map_face'], d['map_bary'], 5000.)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.texture_render(v.cpu(), c, d['vert_mapping'], d['faces'], d['uv'], d['face_part'], torch.zeros(2, 64, 64, dtype=torch.int32).cuda(), atlas)
