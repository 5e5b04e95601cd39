"""Host side of the forward-only ops (ops.py) and their callers: the argument rules, each stated once as a helper, the device-table
helpers of renderer.py, smpl.from_para, evaluate.eval_target, and the GPU-only error of every entry -- everything that decides before
a kernel runs.  No GPU and no built library needed."""
import ctypes

import numpy as np
import pytest
import torch

f32, bf16 = torch.float32, torch.bfloat16


@pytest.fixture
def ops(monkeypatch):
    """ops with the GPU check switched off, so that the shape / dtype rules behind it can be driven with CPU tensors."""
    from danet_densepose2smpl_amd import _lib, ops
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, what: None)
    monkeypatch.setattr(ops, 'require_gpu', lambda t, what: None)
    return ops


def test_f32_converts_and_matches_the_pattern(ops):
    t = torch.arange(24, dtype=torch.float64).view(2, 3, 4).permute(0, 2, 1).requires_grad_()
    got = ops._f32(t, (2, None, 3), 'op: arg')
    assert got.dtype == f32 and got.is_contiguous() and not got.requires_grad and torch.equal(got, t.detach().float())
    assert ops._f32(t, None, 'op: arg').shape == (2, 4, 3)
    assert ops._f32(t, (None, None, None), 'op: arg').shape == (2, 4, 3)
    assert ops._f32(torch.zeros(0, 5), (None, 5), 'op: arg').shape == (0, 5)
    for bad in ((2, 4), (2, 4, 3, 1), (2, None, 4), (3, None, None)):              # rank below, rank above, two wrong extents
        with pytest.raises(ValueError, match=r'^op: arg: shape \(2, 4, 3\), expected \[') as e:
            ops._f32(t, bad, 'op: arg')
        assert ','.join('*' if b is None else str(b) for b in bad) in str(e.value)
    assert ops._f32(None, (2, 3), 'op: arg', optional=True) is None
    with pytest.raises((AttributeError, RuntimeError)):                           # None where it is not allowed is no silent NULL
        ops._f32(None, (2, 3), 'op: arg')


def test_typed_converts_nothing(ops):
    t = torch.zeros(2, 3, dtype=torch.int32)
    assert ops._typed(t, torch.int32, (2, 3), 'op: arg').data_ptr() == t.data_ptr()
    for bad in (t.long(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32).t(), torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(ValueError, match='^op: arg must be a contiguous torch.int32'):
            ops._typed(bad, torch.int32, (2, 3), 'op: arg')


def test_out_is_the_given_tensor_or_a_new_one(ops):
    new = ops._out(None, f32, (2, 17, 2), torch.device('cpu'), 'op: out')
    assert new.dtype == f32 and new.shape == (2, 17, 2) and new.is_contiguous()
    assert ops._out(new, f32, (2, 17, 2), torch.device('cpu'), 'op: out') is new            # the caller's own tensor, not a detached alias
    for bad in (new.double(), torch.zeros(2, 17, 3), torch.zeros(2, 2, 17).transpose(1, 2)):          # dtype, shape, strides
        with pytest.raises(ValueError, match='^op: out must be a contiguous'):
            ops._out(bad, f32, (2, 17, 2), torch.device('cpu'), 'op: out')


def test_packed_u8(ops):
    buf = torch.zeros(7, dtype=torch.uint8)
    assert ops._packed_u8(buf, 'op: src').data_ptr() == buf.data_ptr()
    for bad in (torch.zeros(0, dtype=torch.uint8), torch.zeros(7, dtype=torch.int8), torch.zeros(7, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='^op: src: one packed, non-empty uint8 buffer'):
            ops._packed_u8(bad, 'op: src')


def test_ascending(ops):
    got = ops._ascending([0, 2, 2, 5], 5, 'op: offsets')
    assert isinstance(got, np.ndarray) and got.tolist() == [0, 2, 2, 5]
    assert ops._ascending(np.array([0., 5.]), 5, 'op: offsets').tolist() == [0., 5.]      # (the COCO path compares values only)
    for bad in ([1, 2, 5], [0, 2, 4], [0, 3, 2, 5], [0]):                                 # start, end, a decrease, no interval
        with pytest.raises(ValueError, match='^op: offsets must ascend from 0 to 5'):
            ops._ascending(bad, 5, 'op: offsets')
    with pytest.raises(ValueError, match='view_off must ascend.*integers'):
        ops._ascending(np.array([0., 5.]), 5, 'texture_unwrap: view_off', integers=True)
    assert ops.texture_view_offsets([0, 2, 5], 5).dtype == np.int32


def test_strided_unifies_the_dtype_and_pads_the_strides(ops):
    big = torch.zeros(2, 6, 5, 9)
    a, b = big[:, 1:4, :, 1:8], big[:, 3:6, :, 2:9]
    ts, strides, flag = ops._strided([a.to(bf16), b], 'op', 4, 2)                         # mixed: fp32
    assert [t.dtype for t in ts] == [f32, f32] and flag == 0
    ts, strides, flag = ops._strided([a.to(bf16)[:, :, :, ::2], b.to(bf16)[:, :, :, ::2]], 'op', 4, 2)   # all bf16: kept, nothing copied
    assert [t.dtype for t in ts] == [bf16, bf16] and flag == 1 and not ts[0].is_contiguous()
    assert isinstance(strides, ctypes.c_int64 * 8) and list(strides) == list(ts[0].stride()) + list(ts[1].stride())
    ts, strides, flag = ops._strided([a], 'op', 4, 2)
    assert flag == 0 and ts[0].data_ptr() == a.data_ptr() and list(strides) == list(a.stride()) + [0] * 4
    five = torch.zeros(2, 3, 4, 5, 6, dtype=torch.float64)
    ts, strides, flag = ops._strided([five, five, five], 'op', 5, 4)                      # neither fp32 nor bf16: fp32
    assert ts[0].dtype == f32 and flag == 0 and len(strides) == 20 and list(strides)[15:] == [0] * 5
    with pytest.raises(ValueError, match='^op: sources of rank 4'):
        ops._strided([a, five], 'op', 4, 2)


def test_host_pointers_and_workspace(ops):
    p = ops._host_i32([3, 1, 2])
    assert isinstance(p, ctypes.POINTER(ctypes.c_int32)) and [p[i] for i in range(3)] == [3, 1, 2]
    q = ops._host_i64(np.array([[1, 2], [3, 1 << 40]])[:, 1])                             # a strided view: copied, kept alive by the pointer
    assert isinstance(q, ctypes.POINTER(ctypes.c_int64)) and [q[0], q[1]] == [2, 1 << 40]
    for n in (0, 1, 8, 12, 4097):
        ws = ops._workspace(n, torch.device('cpu'))
        assert ws.dtype == torch.int64 and ws.numel() * 8 >= (n // 8 + 1) * 8 >= (n + 7) // 8 * 8      # the largest rounding any site had
    ws = ops._workspace(2 * 2 * 3 * 3 * 4, torch.device('cpu'), f32, spare=0)               # mesh_shade_vertices: exactly its two halves
    assert ws.dtype == f32 and ws.numel() == 36 and ops._workspace(13, torch.device('cpu'), f32, spare=0).numel() == 4


def test_mesh_shade_views_are_the_two_halves(ops):
    B, V = 2, 3
    ws = torch.arange(2 * B * V * 3, dtype=f32)
    rverts, vcol = ops.mesh_shade_views(ws, B, V)
    assert rverts.shape == vcol.shape == (B, V, 3)
    assert rverts.data_ptr() == ws.data_ptr() and vcol.data_ptr() == ws.data_ptr() + 4 * B * V * 3
    assert torch.equal(rverts.reshape(-1), ws[:18]) and torch.equal(vcol.reshape(-1), ws[18:])
    vcol[1, 2, 0] = -1.0                                                                  # views, not copies
    assert ws[18 + 15] == -1.0


def test_fill_back_and_plain_tables():
    from danet_densepose2smpl_amd import renderer
    f2 = renderer.fill_back([[0, 1, 2], [2, 1, 3]])
    assert f2.dtype == np.int32 and f2.flags['C_CONTIGUOUS'] and f2.tolist() == [[0, 1, 2], [2, 1, 3], [2, 1, 0], [3, 1, 2]]
    vm, tex = renderer.plain_tables(5, 4, torch.device('cpu'))
    assert vm.dtype == torch.int32 and vm.tolist() == [0, 1, 2, 3, 4] and tex.dtype == f32 and tex.shape == (4, 3) and not tex.any()
    assert renderer.plain_tables(None, 4, torch.device('cpu'))[0] is None and renderer.plain_tables(5, None, torch.device('cpu'))[1] is None
    made = []
    cache = renderer.DeviceTables()
    build = lambda: made.append(1) or object()                                            # noqa: E731
    a = cache.tables(('cpu', 5), build)
    assert cache.tables(('cpu', 5), build) is a and cache.tables(('cpu', 6), build) is not a and len(made) == 2
    r = renderer.MeshRenderer(np.array([[0, 1, 2], [2, 1, 3]]))
    t = r.tables(torch.device('cpu'), 4)
    assert r.tables(torch.device('cpu'), 4) is t and t._fields == ('vert_mapping', 'faces', 'faces2', 'csr_off', 'csr_face', 'tex')
    assert t.faces2.tolist() == f2.tolist() and t.tex.shape == (4, 3) and t.csr_off.tolist() == [0, 1, 3, 5, 6]


def test_every_entry_refuses_cpu_tensors_before_the_library_is_loaded(monkeypatch):
    from danet_densepose2smpl_amd import _lib, ops
    from danet_densepose2smpl_amd.smpl import SMPL

    def no_library():
        raise AssertionError('the library was asked for before the CPU tensor was refused')
    monkeypatch.setattr(_lib, 'lib', no_library)
    B, V, S = 2, 12, 16
    z = torch.zeros
    i32, i64, u8, f64 = torch.int32, torch.int64, torch.uint8, torch.float64
    verts, cam, faces = z(B, V, 3), torch.ones(B, 3), z(20, 3, dtype=i32)
    images, fidx = z(B, 3, S, S), z(B, S, S, dtype=i32)
    src, off, shp = z(64, dtype=u8), z(B + 1, dtype=i64), z(B, 2, dtype=i32)
    smpl = SMPL()
    calls = {
        'smpl_lbs': lambda: ops.smpl_lbs(z(B, 10), z(B, 24, 3, 3), smpl),
        'smpl_joints': lambda: ops.smpl_joints(z(B, 54, 3), smpl.joint_map, smpl.j24_to_j19),
        'iuv_raster': lambda: ops.iuv_raster(verts, cam, z(V, dtype=i32), faces, z(20, 3), 5000., S, S),
        'iuv_map2img': lambda: ops.iuv_map2img(z(B, 25, S, S), z(B, 25, S, S), z(B, 25, S, S)),
        'mesh_shade_vertices': lambda: ops.mesh_shade_vertices(verts, faces, z(V + 1, dtype=i32), z(60, dtype=i32), (0.,) * 18),
        'mesh_shade_pixels': lambda: ops.mesh_shade_pixels(z(2 * B * V * 3), cam, V, faces, fidx, images, 5000., S),
        'demo_compose': lambda: ops.demo_compose(images, z(B, 3, 4, 4), z(B, 24, 3, 4, 4), z(B, 3, 4, 4)),
        'vis_grid': lambda: ops.vis_grid(images),
        'vis_joints': lambda: ops.vis_joints(z(3, 20, 38), z(B, 5, 2), None, B, S, S),
        'batch_rodrigues': lambda: ops.batch_rodrigues(z(B, 3)),
        'rodrigues_smplx': lambda: ops.rodrigues_smplx(z(B, 3)),
        'rot6d_to_rotmat': lambda: ops.rot6d_to_rotmat(z(B, 6)),
        'rotmat_to_angle_axis': lambda: ops.rotmat_to_angle_axis(z(B, 3, 3)),
        'pose_eval': lambda: ops.pose_eval(verts, z(17, V), list(range(14)), gt_vertices=verts),
        'vertex_eval': lambda: ops.vertex_eval(verts, verts, z(V)),
        'seg_confusion': lambda: ops.seg_confusion(z(B, S, S), z(B, S, S, dtype=i64), src, None, off, shp, z(B, 6, dtype=i32), z(4, dtype=i32), 4,
                                                   z(32, dtype=i64)),
        'coco_keypoints': lambda: ops.coco_keypoints(z(B, 49, 3), cam, z(B, 2), torch.ones(B)),
        'coco_oks_match': lambda: ops.coco_oks_match(z(B, 17, 2), z(B, dtype=f64), off, z(1, 17, 3, dtype=f64), z(1, dtype=f64), z(1, 4, dtype=f64),
                                                     z(1, dtype=u8), z(1, dtype=u8), off),
        'batch_crop': lambda: ops.batch_crop(src, off, shp, shp, z(B, 10, dtype=f64), S),
        'label_augment': lambda: ops.label_augment(z(B, 2, dtype=f64), pose=z(B, 72, dtype=f64)),
        'scene_render': lambda: ops.scene_render(verts, verts, faces, z(B, 3), z(B, 6), torch.ones(B), z(B, dtype=i32), src, off, shp,
                                                 host=(np.zeros(B), np.zeros(B + 1), np.zeros((B, 2)))),
        'texture_map': lambda: ops.texture_map(z(V, 2), faces, z(25, dtype=i32), z(20, dtype=i32), 8),
        'texture_unwrap': lambda: ops.texture_unwrap(images, verts, cam, z(B, S, S), None, z(V, dtype=i32), faces, z(24, 8, 8, dtype=i32),
                                                     z(24, 8, 8, 2), 5000.),
        'texture_render': lambda: ops.texture_render(verts, cam, z(V, dtype=i32), faces, z(V, 2), z(20, dtype=i32), fidx, z(1, 24, 8, 8, 4)),
        'texture_views': lambda: ops.texture_views(images, verts, cam, 'texture_unwrap'),
        'texture_atlas': lambda: ops.texture_atlas(z(1, 24, 8, 8, 4)),
    }
    public = {n for n, f in vars(ops).items() if callable(f) and not n.startswith('_') and getattr(f, '__module__', None) == ops.__name__
              and not isinstance(f, type)}
    host_only = {'lbs_ticket', 'vis_grid_size', 'mesh_shade_views', 'texture_view_offsets', 'texture_atlas_index'}    # take no device tensor
    assert public - host_only == set(calls), public - host_only ^ set(calls)
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=r'GPU only \(.*got a cpu tensor\); there is no CPU path'):
            call()


def test_from_para_splits_the_row_once():
    from danet_densepose2smpl_amd import smpl
    seen = {}

    def layer(**kw):
        seen.update(kw, grad=torch.is_grad_enabled())
        return 'output'
    B = 3
    para = torch.arange(B * 229, dtype=f32).view(B, 229).requires_grad_()
    assert smpl.from_para(layer, para) == 'output'
    assert set(seen) == {'betas', 'body_pose', 'global_orient', 'pose2rot', 'grad'} and seen['pose2rot'] is False and seen['grad'] is False
    assert torch.equal(seen['betas'], para[:, 3:13]) and seen['betas'].is_contiguous()
    rot = para[:, 13:].reshape(B, 24, 3, 3)
    assert seen['global_orient'].shape == (B, 1, 3, 3) and torch.equal(seen['global_orient'], rot[:, :1])
    assert seen['body_pose'].shape == (B, 23, 3, 3) and torch.equal(seen['body_pose'], rot[:, 1:])
    assert seen['global_orient'].data_ptr() + 36 == seen['body_pose'].data_ptr()          # slices of ONE [B,24,3,3] tensor


def test_eval_target():
    from danet_densepose2smpl_amd import evaluate

    class _Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.iuv2smpl = None

        def infer_net(self, image):
            raise AssertionError('never reached')

    class _Engine(object):
        def __init__(self, net):
            self.model = net

        def __call__(self, image):
            raise AssertionError('never reached')
    with pytest.raises(RuntimeError, match=r'GPU only \(run_evaluation model: got a cpu tensor\)'):
        evaluate.eval_target(_Net())
    with pytest.raises(RuntimeError, match='GPU only'):
        evaluate.eval_target(_Engine(_Net()))
    for bad in (object(), _Engine(object())):
        with pytest.raises(TypeError, match='DaNet or an InferenceEngine'):
            evaluate.eval_target(bad)
    # the three parts: the device is read off the first parameter, which a stand-in can claim to be on the GPU
    net, cuda = _Net(), torch.device('cuda', 0)
    net.parameters = lambda: iter([type('P', (), {'device': cuda})()])
    infer, got, device = evaluate.eval_target(net)
    assert infer == net.infer_net and got is net and device == cuda
    eng = _Engine(net)
    infer, got, device = evaluate.eval_target(eng)
    assert infer is eng and got is net and device == cuda


def test_eval_batches_keep_the_dataset_order_for_a_result_file(monkeypatch):
    from danet_densepose2smpl_amd import evaluate
    seen = []
    monkeypatch.setattr(evaluate, 'iterate_batches', lambda dataset, batch_size, shuffle, num_workers: seen.append(shuffle) or iter([{'k': 1}]))
    monkeypatch.setattr(evaluate, 'to_device', lambda host, device, img_res: (host, device, img_res))
    for result_file, shuffle, want in ((None, True, True), (None, False, False), ('r.npz', True, False), ('r.npz', False, False)):
        assert list(evaluate.eval_batches([], 'dev', result_file, 4, 224, 0, shuffle)) == [({'k': 1}, 'dev', 224)]
        assert seen.pop() is want


def test_int_rule_accepts_whole_numbers_and_names_what_it_refuses():
    from danet_densepose2smpl_amd import ops
    for v in (3, 3.0, np.int64(3)):
        got = ops._int(v, 'op', 'n', 1, 5)
        assert got == 3 and type(got) is int
    assert ops._int(-7, 'op', 'n') == -7 and ops._int(0, 'op', 'n', 0) == 0 and ops._int(5, 'op', 'n', None, 5) == 5
    for bad, bound in ((True, r'in 1\.\.5'), (2.5, r'in 1\.\.5'), (0, r'in 1\.\.5'), (6, r'in 1\.\.5')):
        with pytest.raises(ValueError, match=r'^op: n %s \(an integer %s\)$' % (repr(bad).replace('.', r'\.'), bound)):
            ops._int(bad, 'op', 'n', 1, 5)
    with pytest.raises(ValueError, match=r'^op: n 0 \(an integer >= 1\)$'):
        ops._int(0, 'op', 'n', 1)
    with pytest.raises(ValueError, match=r'^op: n 6 \(an integer <= 5\)$'):
        ops._int(6, 'op', 'n', high=5)
    with pytest.raises(ValueError, match=r'^op: n False \(an integer\)$'):
        ops._int(False, 'op', 'n')


def test_per_device_cache_makes_once_and_leaves_torch_cuda_alone_for_a_cpu_device(monkeypatch):
    from danet_densepose2smpl_amd import ops

    def no_cuda():
        raise AssertionError('torch.cuda.current_device was asked about a CPU device')
    monkeypatch.setattr(torch.cuda, 'current_device', no_cuda)
    cache, made = {}, []

    def make():
        made.append(object())
        return made[-1]
    first = ops._per_device(cache, torch.device('cpu'), make)
    assert ops._per_device(cache, torch.device('cpu'), make) is first and len(made) == 1 and list(cache) == [('cpu', None)]
    assert ops._device_key(torch.device('cuda', 3)) == ('cuda', 3) and ops._device_key('cpu') == ('cpu', None)
    # an index-less CUDA device is the current one
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 2)
    assert ops._device_key(torch.device('cuda')) == ('cuda', 2)
    second = ops._per_device(cache, torch.device('cuda'), make)
    assert ops._per_device(cache, torch.device('cuda', 2), make) is second and second is not first and len(made) == 2
