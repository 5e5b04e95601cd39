"""The scene rasteriser (csrc/scene_ops.hip) and the scene demo (scene.py) on the device, against the float64 restatement of the
scene rule in tests/scene_oracle.py.

Shapes: the smallest that can go wrong -- icosahedra (12 vertices, 20 faces, both windings) in frames of 37 x 53, 64 x 40 and 16 x 16
pixels.  Every projected coordinate stays within +-256 pixels (tests/test_scene_host.py checks it), where an fp32 ulp is 3e-5
pixels; the chain from a vertex to an edge function is about six operations, so device and oracle coordinates differ by less than
2e-4 pixels.  A pixel is UNCERTAIN when (a) its centre is within 1e-3 pixels of an edge line of a candidate face or (b) its two
smallest depths are within a relative 1e-5; test_scene_host.py asserts on the CPU that this is at most 5 % of the covered pixels of
the scenes used here.

Bounds.  ids: exact on every other pixel.  depth: relative 1e-5.  out: per covered, certain pixel, with the margin DELTA = 0.005
levels of 255 -- four times the largest difference between the oracle run in float32 and in float64 on main_scene (1.22e-3;
test_scene_host.py recomputes it; neither run is the code under test): where the oracle's unrounded level is farther than DELTA
from a half-integer the byte must be equal, elsewhere it may differ by 1.  Uncovered pixels equal the source bytes."""
import ctypes
import re

import numpy as np
import pytest
import torch

import scene_oracle as so
from scene_oracle import DELTA

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_args(people, frames):
    from danet_densepose2smpl_amd import scene
    src, off, shp = scene.pack_frames(frames)
    t = {k: _cu(v) for k, v in people.items()}
    t.update(src=_cu(src), offsets=_cu(off), shapes=_cu(shp))
    return t, (src, off, shp)


def _call(t, **kw):
    from danet_densepose2smpl_amd import ops
    return ops.scene_render(t['verts'], t['vcol'], t['faces2'], t['cam_t'], t['proj'], t['dscale'], t['person_frame'], t['src'], t['offsets'],
                            t['shapes'], **kw)


def gpu_render(people, frames):
    """-> (list per frame of {'out', 'ids', 'depth'} as numpy arrays, the raw (out, ids, depth) tensors)."""
    from danet_densepose2smpl_amd import scene
    t, (src, off, shp) = _device_args(people, frames)
    out, ids, depth = _call(t, return_aux=True)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.shape == t['src'].shape and ids.dtype == torch.int32 and depth.dtype == torch.float32
    o, i, d = out.cpu().numpy(), ids.cpu().numpy(), depth.cpu().numpy()
    assert np.array_equal(o[off[-1]:], src[off[-1]:])                                    # the spare bytes after the last frame are copied too
    res = []
    for n, (f, of) in enumerate(zip(scene.unpack_frames(o, off, shp), off)):
        H, W = shp[n]
        a = int(of) // 3
        res.append({'out': f, 'ids': i[a:a + H * W].reshape(H, W), 'depth': d[a:a + H * W].reshape(H, W)})
    return res, (out, ids, depth)


def check_against_oracle(got, ref, frames, tag):
    """The bounds of this file's docstring for every frame; prints what it measured before it asserts."""
    for n, (g, r, f) in enumerate(zip(got, ref, frames)):
        unc = so.uncertain(r)
        sure = ~unc
        cov = (r['ids'] >= 0) & sure
        wrong = int((g['ids'][sure] != r['ids'][sure]).sum())
        rel = float(np.max(np.abs(g['depth'][cov].astype(np.float64) - r['depth'][cov]) / r['depth'][cov])) if cov.any() else 0.0
        lv = r['level'][cov]                                                             # [n,3]
        gb, rb = g['out'][cov].astype(np.int64), r['out'][cov].astype(np.int64)
        off_half = np.abs(lv - np.floor(lv) - 0.5)
        strict = off_half > DELTA
        bad_strict = int((gb != rb)[strict].sum())
        bad_loose = int((np.abs(gb - rb) > 1).sum())
        lvl_err = float(np.abs(gb - lv).max()) if cov.any() else 0.0
        unt = (g['ids'] < 0) & sure
        print('%s frame %d: covered+certain %d, uncertain %d, ids wrong %d, depth max rel %.3e, bytes != (strict) %d of %d, |diff| > 1 %d, '
              'max |byte - level| %.4f' % (tag, n, int(cov.sum()), int(unc.sum()), wrong, rel, bad_strict, int(strict.sum()), bad_loose, lvl_err), flush=True)
        assert wrong == 0
        assert np.isinf(g['depth'][(r['ids'] < 0) & sure]).all() and (g['depth'][(r['ids'] < 0) & sure] > 0).all()
        assert rel <= 1e-5
        assert bad_strict == 0 and bad_loose == 0
        assert np.array_equal(g['out'][unt], f[unt])


# ------------------------------------------------------------------------------------------------------------------ 1
def test_scene_render_against_the_oracle():
    people, frames = so.main_scene()
    ref = so.run(people, frames)
    got, _ = gpu_render(people, frames)
    check_against_oracle(got, ref, frames, 'main')
    assert (got[0]['ids'] >= 0).sum() > 400 and (got[1]['ids'] >= 0).sum() > 200
    assert np.array_equal(got[2]['out'], frames[2]) and (got[2]['ids'] == -1).all() and np.isinf(got[2]['depth']).all()
    # without the optional planes: the same bytes
    t, _ = _device_args(people, frames)
    _, (out, _, _) = gpu_render(people, frames)
    assert torch.equal(_call(t), out)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('kind', so.SKIP_KINDS)
def test_scene_render_skips(kind):
    people, frames, dead = so.skip_scene(kind)
    ref = so.run(people, frames)
    got, _ = gpu_render(people, frames)                                                  # (returns: DANET_OK)
    assert not dead(got[0]['ids']).any()
    assert (got[0]['ids'] >= 0).sum() > 150
    check_against_oracle(got, ref, frames, kind)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_scene_render_exact_tie_goes_to_the_smaller_id():
    people, frames = so.main_scene()
    two = {k: (v if k == 'faces2' else np.ascontiguousarray(v[[0, 0]])) for k, v in people.items()}
    got, _ = gpu_render(two, frames[:1])
    one, _ = gpu_render({k: (v if k == 'faces2' else np.ascontiguousarray(v[[0]])) for k, v in people.items()}, frames[:1])
    cov = got[0]['ids'] >= 0
    assert cov.sum() > 150 and (got[0]['ids'][cov] < 40).all()
    for k in ('out', 'ids', 'depth'):
        assert np.array_equal(got[0][k], one[0][k])


# ------------------------------------------------------------------------------------------------------------------ 4
def test_scene_render_is_independent_of_order():
    people, frames = so.main_scene()
    a, _ = gpu_render(people, frames)
    b, _ = gpu_render(people, frames)
    perm = np.array([2, 1, 0, 3])                                                        # frame 0's people in reverse order
    rev = {k: (v if k == 'faces2' else np.ascontiguousarray(v[perm])) for k, v in people.items()}
    c, _ = gpu_render(rev, frames)
    F2 = people['faces2'].shape[0]
    for n in range(len(frames)):
        for k in ('out', 'ids', 'depth'):
            assert np.array_equal(a[n][k], b[n][k]), (n, k)
        ids = c[n]['ids']
        back = np.where(ids >= 0, perm[np.maximum(ids, 0) // F2] * F2 + np.maximum(ids, 0) % F2, -1)
        assert np.array_equal(back, a[n]['ids']) and np.array_equal(c[n]['out'], a[n]['out'])
        assert np.array_equal(c[n]['depth'].view(np.uint32), a[n]['depth'].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 5
def test_scene_coverage_equals_mesh_renderer_at_224(smpl_model):
    """One person, a 224 x 224 frame, the synthetic SMPL mesh and the box that IS the frame: the crop transform sends source index c
    to crop index c * res / h + res / 2 - center * res / h, so the identity has h = 224 and center = (112, 112) (whole_image_box's
    centre (W - 1) / 2 is the frame seen half a pixel off, and the mesh follows it there)."""
    from danet_densepose2smpl_amd import datasets, ops, scene
    from danet_densepose2smpl_amd.renderer import ALBEDO, MeshRenderer
    faces = np.asarray(smpl_model['faces']).astype(np.int32)
    verts = np.asarray(smpl_model['v_template'], np.float32)[None]
    cam = np.array([[0.9, 0.02, -0.03]], np.float32)
    rend = MeshRenderer(faces, img_res=224)
    v, c = _cu(verts), _cu(cam)
    _, alpha = rend(v, c)
    _, tinv = datasets.crop_transforms(np.array([[112., 112.]]), np.array([1.12]), np.zeros(1), 224)
    assert np.abs(tinv[0] - np.eye(3)).max() < 1e-12
    k = scene.person_cameras(cam.astype(np.float64), tinv, [[224, 224]], [0], 224)
    _, f, f2, off, inc, _ = rend.tables(v.device, verts.shape[1])
    ws, rverts = ops.mesh_shade_vertices(v, f, off, inc, rend.lights, 0., ALBEDO)
    V = verts.shape[1]
    vcol = ws[V * 3:].view(1, V, 3)
    people = {'verts': rverts.cpu().numpy(), 'vcol': vcol.cpu().numpy(), 'faces2': f2.cpu().numpy(), 'cam_t': k['cam_t'].astype(np.float32),
              'proj': k['proj'].astype(np.float32), 'dscale': k['dscale'].astype(np.float32), 'person_frame': np.zeros(1, np.int32)}
    frames = so.make_frames(7, ((224, 224),))
    got, _ = gpu_render(people, frames)
    ref = so.run(people, frames)
    sure = ~(ref[0]['edge'] < so.EDGE_EPS)
    a = alpha[0].cpu().numpy() > 0
    print('224: covered %d, flagged by (a) %d, disagree %d' % (int(a.sum()), int((~sure).sum()), int(((got[0]['ids'] >= 0) != a)[sure].sum())), flush=True)
    assert a.sum() > 1500 and (~sure).sum() < 0.05 * a.sum()
    assert np.array_equal((got[0]['ids'] >= 0)[sure], a[sure])
    assert np.array_equal((ref[0]['ids'] >= 0)[sure], a[sure])


# ------------------------------------------------------------------------------------------------------------------ 6
def _raw(L, t, host, out, P=None, F2=None):
    from danet_densepose2smpl_amd._lib import ptr, stream
    hp, ho, hs = host
    P0, V = t['verts'].shape[:2]
    N = hs.shape[0]
    nws = 1 << 20
    ws = torch.empty(nws // 8, dtype=torch.int64, device='cuda')
    rc = L.danet_scene_render(ptr(t['verts']), ptr(t['vcol']), P0 if P is None else P, V, ptr(t['faces2']), t['faces2'].shape[0] if F2 is None else F2,
                              ptr(t['cam_t']), ptr(t['proj']), ptr(t['dscale']), ptr(t['person_frame']), ptr(t['src']), t['src'].numel(),
                              ptr(t['offsets']), ptr(t['shapes']), N, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              ho.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), hs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              ptr(out), None, None, ptr(ws), nws, stream())
    return rc, (L.danet_last_error() or b'').decode()


def test_scene_render_argument_checks_launch_nothing():
    from danet_densepose2smpl_amd import _lib
    L = _lib.lib()
    people, frames = so.main_scene()
    t, (src, off, shp) = _device_args(people, frames)
    out = torch.full_like(t['src'], 7)
    pf = people['person_frame']
    rc, msg = _raw(L, t, (pf, off, shp), out)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7).all())                                        # the call itself is good
    out.fill_(7)
    bad_off = off.copy()
    bad_off[1] += 3
    short = off.copy()
    short[-1] += 3 * 16 * 16                                                            # frame 2 twice as large as its shape says
    cases = [('person_frame decreases', dict(host=(np.array([0, 1, 0, 1], np.int32), off, shp))),
             ('person_frame.*outside', dict(host=(np.array([0, 0, 0, 3], np.int32), off, shp))),
             ('person_frame.*outside', dict(host=(np.array([-1, 0, 0, 1], np.int32), off, shp))),
             ('does not fit the 31-bit id', dict(host=(np.tile(pf, 2), off, shp), P=8, F2=1 << 28)),
             ('do not hold', dict(host=(pf, bad_off, shp))),
             ('do not hold', dict(host=(pf, short, shp))),
             ('do not hold', dict(host=(pf, off, shp[:, ::-1].copy() + np.array([[0, 1]], np.int32))))]
    for pat, kw in cases:
        host = kw.pop('host')
        rc, msg = _raw(L, t, host, out, **kw)
        assert rc != 0, pat
        assert re.search(pat, msg), (pat, msg)
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                        # nothing was launched
    # the wrapper reads the three index arrays back and raises
    t2 = dict(t, person_frame=_cu(np.array([0, 1, 0, 1], np.int32)))
    with pytest.raises(RuntimeError, match='person_frame decreases'):
        _call(t2)
    with pytest.raises(RuntimeError, match='do not hold'):
        _call(dict(t, offsets=_cu(bad_off)))


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.fixture(scope='module')
def demo_model():
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    reset_cfg()
    torch.manual_seed(0)
    return DaNet(default_options(2), None, pretrained=False).cuda().eval()


def test_scene_demo_end_to_end_and_graph_replay(demo_model):
    from danet_densepose2smpl_amd import scene
    model = demo_model
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (96, 80, 3)).astype(np.uint8), rng.integers(0, 256, (50, 70, 3)).astype(np.uint8)]
    boxes = [[scene.boxes_from_xywh([5., 8., 50., 70.]), scene.boxes_from_xywh([30., 20., 45., 60.])], []]
    demo = scene.SceneDemo(model, model.iuv2smpl.smpl, 2)
    rendered, people = demo(frames, boxes)
    assert [r.shape for r in rendered] == [f.shape for f in frames] and all(r.dtype == np.uint8 for r in rendered)
    assert np.array_equal(rendered[1], frames[1])                                        # nobody in it
    assert people[0]['para'].shape == (2, 229) and people[1]['para'].shape == (0, 229)
    assert people[0]['vertices'].shape[0] == 2 and people[0]['cam_t_full'].shape == (2, 3) and people[0]['scale'].shape == (2,)
    # the stages by hand
    plan = demo.prepare(frames, boxes)
    crops = demo.crops(plan)
    assert crops.shape == (2, 3, demo.res, demo.res)
    para = model.infer_net(crops)['para']
    assert np.array_equal(people[0]['para'], para.cpu().numpy())                         # bit-equal
    para = para.clone()
    out, ids, _ = demo.render(para, plan, return_aux=True)
    torch.cuda.synchronize()
    o, i = out.cpu().numpy(), ids.cpu().numpy()
    n0 = 96 * 80
    assert np.array_equal(o[:n0 * 3].reshape(96, 80, 3), rendered[0])
    empty = i[:n0].reshape(96, 80) < 0
    print('end to end: %d of %d pixels of frame 0 drawn, cam %s' % (int((~empty).sum()), n0, people[0]['cam'].tolist()), flush=True)
    assert np.array_equal(rendered[0][empty], frames[0][empty]) and (i[n0:] == -1).all()
    assert (~empty).any()
    # the stage from para to the bytes under graph replay
    eager = demo.render(para, plan).clone()
    assert torch.equal(eager, out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            demo.render(para, plan)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = demo.render(para, plan)
    for _ in range(2):
        static.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)
    del g


# ------------------------------------------------------------------------------------------------------------------ tool
def test_tool_writes_scenes_people_and_objs(tmp_path):
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    import vis_oracle as vo
    rng = np.random.default_rng(12)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    imgs = {'a': rng.integers(0, 256, (60, 90, 3)).astype(np.uint8), 'b': rng.integers(0, 256, (48, 40, 3)).astype(np.uint8)}
    for k, a in imgs.items():
        np.save(str(src / (k + '.npy')), a)
    (tmp_path / 'boxes.json').write_text(json.dumps({'a.npy': [[5, 4, 40, 50], [40, 10, 45, 45]], 'b.npy': []}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'demo_scene.py'), '--img_dir', str(src), '--out_dir', str(dst), '--boxes',
                        str(tmp_path / 'boxes.json'), '--batch', '2', '--obj', '--reps', '2'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().split('\n')[-1])
    print(line, flush=True)
    assert line['tool'] == 'demo_scene' and line['people'] == 2 and all(line[k]['ms_per_frame'] > 0 for k in ('crop', 'infer', 'render'))
    a = vo.png_decode(open(str(dst / 'a_scene.png'), 'rb').read())
    b = vo.png_decode(open(str(dst / 'b_scene.png'), 'rb').read())
    assert a.shape == (60, 90, 3) and np.array_equal(b, imgs['b'])                       # nobody in b: byte for byte
    changed = (a != imgs['a']).any(2)
    assert 0 < changed.sum() < 60 * 90
    pa, pb = np.load(str(dst / 'a_people.npz')), np.load(str(dst / 'b_people.npz'))
    assert pa['para'].shape == (2, 229) and pa['vertices'].shape[0] == 2 and pa['cam_t_full'].shape == (2, 3) and pb['para'].shape == (0, 229)
    assert pa['center'].tolist() == [[25., 29.], [62.5, 32.5]] and np.allclose(pa['scale'], [0.3, 0.27])
    objs = sorted(n for n in os.listdir(str(dst)) if n.endswith('.obj'))
    assert objs == ['a_person0.obj', 'a_person1.obj']
    first = open(str(dst / 'a_person0.obj')).readline().split()
    assert first[0] == 'v' and np.array_equal(np.array([float(x) for x in first[1:]], np.float64).astype(np.float32), pa['vertices'][0, 0])
