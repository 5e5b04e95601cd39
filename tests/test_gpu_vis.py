"""The demo pipeline on the device (csrc/vis_ops.hip): IUV decode against the REFERENCE's outputs (golden g24, exact), the shaded
mesh view against known answers and the fp64 restatement of tests/vis_oracle.py, the result panels against an assembly from
tensor ops, graph capture, and tools/demo.py end to end.

Bounds.  Decode: exact equality -- planes 1 / 2 are copies, plane 0 is one correctly rounded division or a table entry.
Shading vs fp64: 1 / 255 on EVERY covered pixel, one level of the 8-bit file the tool writes (a bound from the output format).
Panels: exact, except the two resized panels: there both sides evaluate h0 (w0 a + w1 b) + h1 (w0 c + w1 d) on values in [0, 1]
with exact weights (the scale is 4: the weights are multiples of 1/8), and the device side does so without fusing (this file's
translation unit is compiled with -ffp-contract=off), so they differ by at most the roundings a fused evaluation saves: two
products (half an ulp of 1 each at most) in each of the two brackets and one in the outer sum, and the same again in the other
order of evaluation -- 4 * 2^-24 is taken as the bound.  The measured figures go through conftest.record."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT, golden, rand_pose_shape, record
import vis_oracle as vo

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from danet_densepose2smpl_amd.config import reset_cfg, cfg_from_dict
    reset_cfg()
    cfg_from_dict(kw)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------ decode
def test_map2img_global_exact_vs_reference():
    from danet_densepose2smpl_amd import iuvmap
    g = golden('g24_vis')
    U, V, I, A = (_cu(a) for a in vo.g24_global_inputs())
    np.testing.assert_array_equal(iuvmap.iuv_map2img(U, V, I, A).cpu().numpy(), g['raw'])
    cU, cV, cI, cA = iuvmap.iuvmap_clean(U, V, I, A)
    assert vo.crc(*(t.cpu().numpy() for t in (cU, cV, cI, cA))) == g['clean_crc']
    np.testing.assert_array_equal(iuvmap.iuv_map2img(cU, cV, cI, cA).cpu().numpy(), g['clean_ann'])
    np.testing.assert_array_equal(iuvmap.iuv_map2img(cU, cV, cI).cpu().numpy(), g['clean'])
    np.testing.assert_array_equal(iuvmap.iuv_map2img(cU, cV, cI, None).cpu().numpy(), g['clean'])
    # any strides: the same values behind a channels-last layout and behind a sliced parent
    np.testing.assert_array_equal(iuvmap.iuv_map2img(*(t.contiguous(memory_format=torch.channels_last) for t in (U, V, I, A))).cpu().numpy(), g['raw'])
    big = torch.randn(4, 90, 64, 70, device='cuda')
    big[:, 5:30, :, 3:67], big[:, 30:55, :, 3:67], big[:, 55:80, :, 3:67] = U, V, I
    np.testing.assert_array_equal(iuvmap.iuv_map2img(big[:, 5:30, :, 3:67], big[:, 30:55, :, 3:67], big[:, 55:80, :, 3:67], A).cpu().numpy(), g['raw'])


def test_map2img_mapping_and_tie_rule():
    from danet_densepose2smpl_amd import iuvmap
    I = torch.zeros(1, 7, 2, 2, device='cuda')
    I[0, 2, 0, 0] = I[0, 5, 0, 0] = 3.0                               # tie between 2 and 5 -> 2
    I[0, :, 0, 1] = -1.0                                              # all equal -> 0
    I[0, 6, 1, 0] = 1.0
    I[0, 1, 1, 1] = float('nan')                                      # a NaN is the maximum (torch.argmax)
    U = torch.arange(28, dtype=torch.float32, device='cuda').view(1, 7, 2, 2) + 1
    out = iuvmap.iuv_map2img(U, -U, I).cpu().numpy()
    ref = torch.argmax(I.cpu(), dim=1).numpy()
    np.testing.assert_array_equal(ref[0], [[2, 0], [6, 1]])
    np.testing.assert_array_equal(out[0, 0], ref[0].astype(np.float32) / np.float32(6))
    np.testing.assert_array_equal(out[0, 1], [[U[0, 2, 0, 0].item(), 0.], [U[0, 6, 1, 0].item(), U[0, 1, 1, 1].item()]])
    np.testing.assert_array_equal(out[0, 2], -out[0, 1])
    mapping = [0, 3, 4, 24, 9, 10, 23]
    outm = iuvmap.iuv_map2img(U, -U, I, ind_mapping=mapping).cpu().numpy()
    want = np.array([np.float32(m * (1. / 24.)) for m in mapping], np.float32)[ref[0]]
    np.testing.assert_array_equal(outm[0, 0], want)
    np.testing.assert_array_equal(outm[0, 1:], out[0, 1:])
    np.testing.assert_array_equal(outm, vo.iuv_map2img(U.cpu().numpy(), -U.cpu().numpy(), np.nan_to_num(I.cpu().numpy(), nan=9.), None, mapping))


def test_map2img_bf16_equals_widened():
    from danet_densepose2smpl_amd import iuvmap
    U, V, I, A = (_cu(a).to(torch.bfloat16) for a in vo.g24_global_inputs())
    got = iuvmap.iuv_map2img(U, V, I, A)
    assert got.dtype == torch.float32
    assert torch.equal(got, iuvmap.iuv_map2img(U.float(), V.float(), I.float(), A.float()))
    np.testing.assert_array_equal(got.cpu().numpy(), vo.iuv_map2img(*(t.float().cpu().numpy() for t in (U, V, I, A))))
    # mixed dtypes are widened by the wrapper
    assert torch.equal(got, iuvmap.iuv_map2img(U.float(), V, I, A))


def test_map2img_part_one_launch_equals_24_calls_and_reference():
    from danet_densepose2smpl_amd import iuvmap, part_ops
    from danet_densepose2smpl_amd.iuv_estimator import DP2SMPL_MAPPING
    g = golden('g24_vis')
    P = _cu(vo.g24_part_inputs())
    B = P.shape[0]
    one = iuvmap.part_iuv_map2img(P, DP2SMPL_MAPPING)
    assert one.shape == (B, 24, 3, 32, 32)
    np.testing.assert_array_equal(one.cpu().numpy(), g['part'])
    single = torch.stack([iuvmap.iuv_map2img(P[:, i, 0], P[:, i, 1], P[:, i, 2], ind_mapping=[0] + list(DP2SMPL_MAPPING[i])) for i in range(24)], 1)
    assert torch.equal(one, single)
    # the strided [B,24,3,7,H,W] view of the channel-padded buffer the training path produces, fp32 and bf16 NHWC
    x24 = torch.zeros(B * 24, 24, 32, 32, device='cuda')
    x24[:, :21] = P.reshape(B * 24, 21, 32, 32)
    view = part_ops.padded_part_view(x24)
    assert not view.is_contiguous()
    assert torch.equal(iuvmap.part_iuv_map2img(view, DP2SMPL_MAPPING), one)
    xb = x24.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    vb = part_ops.padded_part_view(xb)
    assert torch.equal(iuvmap.part_iuv_map2img(vb, DP2SMPL_MAPPING), iuvmap.part_iuv_map2img(vb.float().contiguous(), DP2SMPL_MAPPING))
    # K = 25: no mapping
    P25 = torch.randn(1, 24, 3, 25, 8, 8, device='cuda', generator=torch.Generator('cuda').manual_seed(3))
    got = iuvmap.part_iuv_map2img(P25)
    for i in (0, 11, 23):
        np.testing.assert_array_equal(got[:, i].cpu().numpy(), vo.iuv_map2img(*(P25[:, i, k].cpu().numpy() for k in range(3))))


# ------------------------------------------------------------------------------------------------------------------ mesh
def _scene(smpl_model, B, seed):
    betas, pose = rand_pose_shape(B, seed, pose_sigma=0.35)
    verts, _ = oracle.lbs_forward(smpl_model, betas, pose, False, np.float32)
    rng = np.random.default_rng(seed)
    cam = np.stack([rng.uniform(0.6, 1.1, B), rng.uniform(-.1, .1, B), rng.uniform(-.1, .1, B)], 1).astype(np.float32)
    return verts.astype(np.float32), cam


def test_mesh_single_triangle_known_answer():
    """A fronto-parallel triangle at z = 0, camera s = 1 at 224 (one unit = 112 pixels).  With the order (0,0)-(0,1)-(1,0) its
    normal is (0,0,-1), towards the camera: lit by the lights with z < 0, i.e. the first (colour 1) and the third (0.7); with
    the opposite order the normal is (0,0,1): lit by the second alone.  n . normalise(L - v) = -+(L_z - v_z) / |L - v|."""
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    tri = np.array([[-0.3, -0.3, 0.], [-0.3, 0.5, 0.], [0.5, -0.3, 0.]], np.float32)
    verts = np.stack([tri, tri[[0, 2, 1]]])
    cam = np.array([[1., 0., 0.]] * 2, np.float32)
    L = [vo.rotate_y(np.array(p), np.radians(120.)) for p, _ in vo.LIGHTS]
    lam = lambda v, l, sign: max(0., sign * (L[l][2] - v[2]) / np.linalg.norm(L[l] - v))
    col = np.array([[0.9 * (1. * lam(v, 0, -1) + 1. * lam(v, 1, -1) + .7 * lam(v, 2, -1)) for v in tri.astype(np.float64)],
                    [0.9 * (1. * lam(v, 0, +1) + 1. * lam(v, 1, +1) + .7 * lam(v, 2, +1)) for v in tri.astype(np.float64)]])
    assert abs(col[0].mean() - 0.933) < 2e-3 and abs(col[1].mean() - 0.572) < 2e-3       # the arithmetic of the docstring, by hand
    rgb, alpha = MeshRenderer(np.array([[0, 1, 2]]), img_res=224)(_cu(verts), _cu(cam))
    rgb, alpha = rgb.cpu().numpy(), alpha.cpu().numpy()
    # coverage: pixel centres inside the projected triangle (x right, y down; 112 px per unit about the centre 112)
    r, c = np.meshgrid(np.arange(224) + 0.5, np.arange(224) + 0.5, indexing='ij')
    x, y = (c - 112.) / 112., (r - 112.) / 112.
    inside = (x > -0.3 + 1e-3) & (y > -0.3 + 1e-3) & (x + y < 0.2 - 1e-3)
    outside = (x < -0.3 - 1e-3) | (y < -0.3 - 1e-3) | (x + y > 0.2 + 1e-3)
    for b in range(2):
        assert (alpha[b][inside] == 1).all() and (alpha[b][outside] == 0).all() and inside.sum() > 3500      # (0.8 * 112)^2 / 2 = 4014 pixels, less the margin
        assert (rgb[b][:, outside] == 0).all()
        px = rgb[b][:, inside]
        assert (px[0] == px[1]).all() and (px[0] == px[2]).all()                       # white lights: grey
        assert px.min() >= col[b].min() - 1e-5 and px.max() <= col[b].max() + 1e-5     # a convex mix of the vertex colours
    # the mix itself: affine in the pixel position for a fronto-parallel face
    w1, w2 = (y[inside] + 0.3) / 0.8, (x[inside] + 0.3) / 0.8
    want = (1 - w1 - w2) * col[0, 0] + w1 * col[0, 1] + w2 * col[0, 2]
    assert np.abs(rgb[0, 0][inside] - want).max() < 1e-5
    # a colour for all three lights
    rgbc, _ = MeshRenderer(np.array([[0, 1, 2]]), img_res=224, color=(0.2, 0.5, 1.0))(_cu(verts[:1]), _cu(cam[:1]))
    k = 0.9 * sum(lam(tri[0].astype(np.float64), l, -1) for l in range(3))
    np.testing.assert_allclose(rgbc[0, :, 112 - 20, 112 - 20].cpu().numpy(), np.clip(k * np.array([0.2, 0.5, 1.0]), 0, 1), atol=5e-3)


@pytest.fixture(scope='module')
def mesh32(smpl_model):
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    verts, cam = _scene(smpl_model, 32, 4242)
    faces = np.asarray(smpl_model['faces']).astype(np.int32)
    return MeshRenderer(faces, img_res=224), faces, verts, cam


def test_mesh_alpha_is_part_renderer_mask_and_background_untouched(mesh32):
    from danet_densepose2smpl_amd.renderer import PartRenderer
    rend, faces, verts, cam = mesh32
    F = faces.shape[0]
    pr = PartRenderer(faces, np.full((F, 3), 0.005, np.float32), np.zeros((100, 100, 100), np.float32), render_res=224)
    v, c = _cu(verts), _cu(cam)
    mask, _ = pr(v, c)
    images = torch.rand(32, 3, 224, 224, device='cuda', generator=torch.Generator('cuda').manual_seed(5))
    rgb, alpha = rend(v, c, images)
    assert torch.equal(alpha, mask) and 0.03 < float(alpha.mean()) < 0.6
    un = (alpha == 0).unsqueeze(1).expand_as(rgb)
    assert torch.equal(rgb[un], images[un])
    rgb0, alpha0 = rend(v, c)
    assert torch.equal(alpha0, alpha) and (rgb0[un] == 0).all()
    cov = ~un
    assert torch.equal(rgb0[cov], rgb[cov]) and float(rgb0.min()) >= 0 and float(rgb0.max()) <= 1
    # two runs: bit-identical (no atomics in the shading; the rasteriser's depth test is an order-independent minimum)
    rgb2, alpha2 = rend(v, c, images)
    assert torch.equal(rgb2, rgb) and torch.equal(alpha2, alpha)


def test_mesh_rot_y_equals_rotated_vertices(mesh32):
    rend, faces, verts, cam = mesh32
    v, c = _cu(verts[:8]), _cu(cam[:8])
    a = math.radians(90)
    cs, sn = float(np.float32(math.cos(a))), float(np.float32(math.sin(a)))
    vr = torch.stack([v[..., 0] * cs - v[..., 2] * sn, v[..., 1], v[..., 0] * sn + v[..., 2] * cs], -1)     # one binary32 operation each
    rgb_a, alpha_a = rend(v, c, rot_y=a)
    rgb_b, alpha_b = rend(vr, c)
    assert torch.equal(alpha_a, alpha_b) and torch.equal(rgb_a, rgb_b)
    assert not torch.equal(alpha_a, rend(v, c)[1])


def test_mesh_vs_fp64_oracle_every_covered_pixel(mesh32, smpl_model):
    """Bound 1 / 255 on every covered pixel.  Measured on the MI355X (32 poses, 224 x 224): front view max 1.1e-4 (p99.9 5.9e-6,
    mean 1.9e-7, 253 114 covered pixels), side view max 4.2e-5 (195 319 pixels); profiles/vis_parity_measured.jsonl."""
    from danet_densepose2smpl_amd import ops
    rend, faces, verts, cam = mesh32
    v, c = _cu(verts), _cu(cam)
    images = torch.rand(32, 3, 224, 224, device='cuda', generator=torch.Generator('cuda').manual_seed(6))
    meas = {}
    for name, rot, img in (('front', 0., images), ('side', math.radians(90), None)):
        rgb, alpha = rend(v, c, img, rot_y=rot)
        vm, f, f2, off, inc, tex = rend.tables(v.device, v.shape[1])
        _, rverts = ops.mesh_shade_vertices(v, f, off, inc, rend.lights, rot)
        _, fidx, _ = ops.iuv_raster(rverts, c, vm, f2, tex, 5000., 224, 224, return_aux=True)
        fidx = fidx.cpu().numpy()
        assert np.array_equal(fidx >= 0, alpha.cpu().numpy() > 0)
        want, _ = vo.shade(verts, cam, faces, fidx, None if img is None else img.cpu().numpy(), rot_y=rot, res=224)
        d = np.abs(rgb.cpu().numpy().astype(np.float64) - want)
        cov = np.broadcast_to((fidx >= 0)[:, None], d.shape)
        dc = d[cov]
        meas[name] = {'max': float(dc.max()), 'p99.9': float(np.percentile(dc, 99.9)), 'mean': float(dc.mean()), 'covered': int((fidx >= 0).sum())}
        print('mesh vs fp64 (%s):' % name, meas[name], flush=True)
    record('vis_mesh_shade_vs_fp64', meas)
    for name in meas:
        assert meas[name]['covered'] > 32 * 1500
        assert meas[name]['max'] <= 1.0 / 255.0, meas


# ------------------------------------------------------------------------------------------------------------------ panels
def _panels_from_planes(images, planes):
    """demo.py:115-177 with tensor ops, from the same decoded / rendered planes."""
    import torch.nn.functional as F
    B, _, S, _ = images.shape
    hm = planes['glob'].shape[-1]
    glob = F.interpolate(planes['glob'], size=(S, S), mode='bilinear', align_corners=False)
    rows = [torch.cat([planes['part'][:, r * 6 + k] for k in range(6)], dim=3) for r in range(4)]        # make_grid(nrow=6, padding=0)
    grid = torch.cat(rows, dim=2)
    riuv = F.interpolate(planes['riuv'], size=(S, S), mode='bilinear', align_corners=False)
    over = images.clone()
    over[riuv > 0] = riuv[riuv > 0]
    one = lambda w: torch.ones(B, 1, S, w, device=images.device)
    strips = [torch.cat([images, one(S)], 1), torch.cat([glob, one(S)], 1), torch.cat([grid, one(6 * hm)], 1), torch.cat([over, one(S)], 1)]
    if planes['mesh'] is not None:
        strips += [torch.cat([planes['mesh'], one(S)], 1), torch.cat([planes['side'], planes['side_alpha'].unsqueeze(1)], 1)]
    vis = torch.cat(strips, dim=3)
    vis[vis < 0.0] = 0.0
    vis[vis > 1.0] = 1.0
    return vis.permute(0, 2, 3, 1).contiguous()


RESIZE_BOUND = 4 * 2.0 ** -24


def _check_panels(strip, images, planes, S, tag):
    want = _panels_from_planes(images, planes)
    assert strip.shape == want.shape and strip.dtype == torch.float32
    wide = planes['mesh'] is not None
    assert strip.shape[1:] == (S, (13 if wide else 9) * S // 2, 4)
    resized = [(S, 2 * S), (7 * S // 2, 9 * S // 2)]
    exact = [(0, S), (2 * S, 7 * S // 2)] + ([(9 * S // 2, 13 * S // 2)] if wide else [])
    for a, b in exact:
        assert torch.equal(strip[:, :, a:b], want[:, :, a:b]), (tag, a, b)
    d = max(float((strip[:, :, a:b] - want[:, :, a:b]).abs().max()) for a, b in resized)
    print('panels %s: resized panels max |diff| = %.3e (bound %.3e)' % (tag, d, RESIZE_BOUND), flush=True)
    record('vis_panels_resize_vs_interpolate_' + tag, {'max_abs': d, 'bound': RESIZE_BOUND})
    assert d <= RESIZE_BOUND, (tag, d)
    assert (strip[..., 3][:, :, :9 * S // 2] == 1).all()
    # the overlay's choice (render > 0) is made on values that may differ in the last place only where the render is not 0:
    # where the tensor-op overlay took the image, the kernel did too
    return d


@pytest.fixture(scope='module')
def c2():
    """BASELINE config C2's model (ResNet-50 backbone, 256 x 256), seeded weights, B = 4."""
    _cfg(**{'DANET.INIMG_SIZE': 256, 'DANET.HEATMAP_SIZE': 64, 'DANET.IUV_REGRESSOR': 'resnet'})
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    from danet_densepose2smpl_amd.trainer import default_options
    torch.manual_seed(0)
    model = DaNet(default_options(4), None, pretrained=False).cuda().eval()
    images = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    return model, images, MeshRenderer(model.iuv2smpl.smpl.faces, img_res=256)


def test_panels_infer_net_equal_tensor_op_assembly(c2):
    from danet_densepose2smpl_amd import demo
    model, images, mr = c2
    out = model.infer_net(images)
    smpl = model.iuv2smpl.smpl
    for tag, rend in (('mesh', mr), ('plain', None)):
        strip, planes = demo.result_panels(out, images, smpl, model.iuv_renderer, rend, return_planes=True)
        _check_panels(strip, images, planes, 256, 'infer_net_' + tag)
        assert torch.equal(strip, demo.result_panels(out, images, smpl, model.iuv_renderer, rend))
    # the planes are what the public ops give on the same inputs
    from danet_densepose2smpl_amd import iuvmap
    strip, planes = demo.result_panels(out, images, smpl, model.iuv_renderer, mr, return_planes=True)
    assert torch.equal(planes['glob'], iuvmap.iuv_map2img(*out['visualization']['iuv_pred']))
    assert float(planes['side_alpha'].mean()) > 0.005 and torch.equal(strip[..., 3][:, :, 11 * 256 // 2:], planes['side_alpha'])
    with pytest.raises(ValueError, match='mesh renderer'):
        from danet_densepose2smpl_amd.renderer import MeshRenderer
        demo.result_panels(out, images, smpl, model.iuv_renderer, MeshRenderer(smpl.faces, img_res=224))
    with pytest.raises(ValueError, match='IUV renderer'):
        from danet_densepose2smpl_amd.renderer import IUV_Renderer
        demo.result_panels(out, images, smpl, IUV_Renderer(256, 56, smpl_model=None), mr)


def test_panels_engine_mesh_output_and_graph_capture(c2):
    from danet_densepose2smpl_amd import demo
    model, images, mr = c2
    smpl = model.iuv2smpl.smpl
    eng = model.inference_engine(4, mesh=True)
    try:
        out = eng(images)
        assert 'vertices' in out
        strip, planes = demo.result_panels(out, images, smpl, model.iuv_renderer, mr, return_planes=True)
        _check_panels(strip, images, planes, 256, 'engine_mesh')
        eager = strip.clone()
        # capture: two warm-up calls on a side stream, as inference.py does
        f = lambda: demo.result_panels(out, images, smpl, model.iuv_renderer, mr)
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
            static.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(static, eager)
        del g
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ tool
def test_tool_writes_png_panels(tmp_path):
    rng = np.random.default_rng(11)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    imgs = {'a': rng.random((224, 224, 3)).astype(np.float32), 'b': rng.integers(0, 256, (224, 224, 3)).astype(np.uint8)}
    for k, a in imgs.items():
        np.save(str(src / (k + '.npy')), a)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'demo.py'), '--img_dir', str(src), '--out_dir', str(dst), '--mesh', '--batch', '2',
                        '--reps', '2'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout[-600:], flush=True)
    assert 'panels_hip' in r.stdout
    for k, a in imgs.items():
        png = vo.png_decode(open(str(dst / (k + '_result.png')), 'rb').read())
        assert png.shape == (224, 224 * 13 // 2, 4)
        first = np.rint(a.astype(np.float32) / 255.0 * 255.0).astype(np.uint8) if a.dtype == np.uint8 else np.rint(np.clip(a, 0, 1) * np.float32(255.0)).astype(np.uint8)
        np.testing.assert_array_equal(png[:, :224, :3], first)
        assert (png[:, :224 * 9 // 2, 3] == 255).all()
