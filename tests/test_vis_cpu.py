"""Host-side checks of the demo pipeline (no GPU): the numpy restatement of iuv_map2img against the REFERENCE's outputs (golden
g24, tests/golden/make_golden_vis.py), the tool's PNG writer against a decoder written by hand, the vertex -> face table, and the
refusals (CPU tensors, uv_rois, a mapping that the reference's in-place loop would chain)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import vis_oracle as vo


def _tool():
    spec = importlib.util.spec_from_file_location('danet_demo_tool', os.path.join(ROOT, 'tools', 'demo.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_oracle_map2img_equals_reference_exactly():
    from danet_densepose2smpl_amd import iuvmap
    from danet_densepose2smpl_amd.iuv_estimator import DP2SMPL_MAPPING
    g = golden('g24_vis')
    U, V, I, A = vo.g24_global_inputs()
    assert vo.crc(U, V, I, A) == g['in_crc']                         # the seeded stream is the one the reference saw
    np.testing.assert_array_equal(vo.iuv_map2img(U, V, I, A), g['raw'])
    cU, cV, cI, cA = (t.numpy() for t in iuvmap.iuvmap_clean(*(torch.from_numpy(a) for a in (U, V, I, A))))
    assert vo.crc(cU, cV, cI, cA) == g['clean_crc']
    np.testing.assert_array_equal(vo.iuv_map2img(cU, cV, cI, cA), g['clean_ann'])
    np.testing.assert_array_equal(vo.iuv_map2img(cU, cV, cI), g['clean'])
    assert not np.array_equal(g['clean'], g['clean_ann'])            # the Ann gate does something on this input
    P = vo.g24_part_inputs()
    assert vo.crc(P) == g['part_crc']
    assert g['dp2smpl_mapping'].tolist() == [list(r) for r in DP2SMPL_MAPPING]
    for i in range(24):
        got = vo.iuv_map2img(P[:, i, 0], P[:, i, 1], P[:, i, 2], None, [0] + list(DP2SMPL_MAPPING[i]))
        np.testing.assert_array_equal(got, g['part'][:, i])


def test_oracle_tie_rule_lowest_index_wins():
    I = np.zeros((1, 5, 2, 2), np.float32)
    I[0, 2, 0, 0] = I[0, 4, 0, 0] = 3.0                              # tie between 2 and 4 -> 2
    I[0, :, 0, 1] = -1.0                                             # all equal -> 0
    U = np.arange(20, dtype=np.float32).reshape(1, 5, 2, 2) + 1
    out = vo.iuv_map2img(U, -U, I)
    assert out[0, 0, 0, 0] == np.float32(2) / np.float32(4) and out[0, 1, 0, 0] == U[0, 2, 0, 0] and out[0, 2, 0, 0] == -U[0, 2, 0, 0]
    assert (out[0, :, 0, 1] == 0).all()


@pytest.mark.parametrize('C', [3, 4])
def test_png_writer_round_trip(tmp_path, C):
    tool = _tool()
    rng = np.random.default_rng(C)
    arr = rng.integers(0, 256, (13, 29, C)).astype(np.uint8)
    arr[0, 0] = 0
    arr[-1, -1] = 255
    p = str(tmp_path / 'x.png')
    tool.write_png(p, arr)
    np.testing.assert_array_equal(vo.png_decode(open(p, 'rb').read()), arr)
    with pytest.raises(ValueError):
        tool.write_png(p, arr.astype(np.float32))


def test_png_decoder_knows_the_filters():
    """The decoder is the yardstick of the writer, so it is checked on lines filtered by hand (types 1..4)."""
    import struct
    import zlib
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 4, 3)).astype(np.int64)
    flat = img.reshape(5, 12)
    lines = []
    for y in range(5):
        f = y                                                        # filter type = row number (0..4)
        up = flat[y - 1] if y else np.zeros(12, np.int64)
        left = np.concatenate([np.zeros(3, np.int64), flat[y, :-3]])
        ul = np.concatenate([np.zeros(3, np.int64), up[:-3]])
        if f == 0:
            pr = np.zeros(12, np.int64)
        elif f == 1:
            pr = left
        elif f == 2:
            pr = up
        elif f == 3:
            pr = (left + up) // 2
        else:
            pa, pb, pc = np.abs(up - ul), np.abs(left - ul), np.abs(left + up - 2 * ul)
            pr = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        lines.append(bytes([f]) + ((flat[y] - pr) & 255).astype(np.uint8).tobytes())
    ch = lambda t, b: struct.pack('>I', len(b)) + t + b + struct.pack('>I', zlib.crc32(t + b) & 0xffffffff)
    data = b'\x89PNG\r\n\x1a\n' + ch(b'IHDR', struct.pack('>IIBBBBB', 4, 5, 8, 2, 0, 0, 0)) + ch(b'IDAT', zlib.compress(b''.join(lines))) + ch(b'IEND', b'')
    np.testing.assert_array_equal(vo.png_decode(data), img.astype(np.uint8))


def test_vertex_face_table_lists_every_face_three_times(smpl_model):
    from danet_densepose2smpl_amd.renderer import vertex_face_csr
    faces = np.asarray(smpl_model['faces']).astype(np.int64)
    V = int(np.asarray(smpl_model['v_template']).shape[0])
    off, inc = vertex_face_csr(faces, V)
    assert off.dtype == np.int32 and inc.dtype == np.int32 and off.shape == (V + 1,) and inc.shape == (3 * faces.shape[0],)
    assert off[0] == 0 and off[-1] == inc.size and (np.diff(off) >= 0).all()
    np.testing.assert_array_equal(np.bincount(inc, minlength=faces.shape[0]), np.full(faces.shape[0], 3))
    for v in list(range(0, V, 97)) + [V - 1]:
        mine = inc[off[v]:off[v + 1]]
        assert (np.diff(mine) > 0).all()                             # table order = ascending face index
        np.testing.assert_array_equal(mine, np.nonzero((faces == v).any(1))[0])
    with pytest.raises(ValueError):
        vertex_face_csr(faces, V - 1)


def test_vis_ops_refuse_cpu_tensors():
    from danet_densepose2smpl_amd import demo, iuvmap, ops
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    z = torch.zeros(1, 25, 4, 4)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        iuvmap.iuv_map2img(z, z, z)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        iuvmap.iuv_map2img(z[:, :7], z[:, :7], z[:, :7], ind_mapping=[0, 1, 2, 3, 4, 5, 6])
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        iuvmap.part_iuv_map2img(torch.zeros(1, 24, 3, 25, 4, 4))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        MeshRenderer(np.array([[0, 1, 2]]), img_res=8)(torch.zeros(1, 3, 3), torch.ones(1, 3))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.demo_compose(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 2, 2), torch.zeros(1, 24, 3, 2, 2), torch.zeros(1, 3, 2, 2))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        demo.result_panels({}, torch.zeros(1, 3, 8, 8), None, None)


def test_map2img_refusals():
    from danet_densepose2smpl_amd import iuvmap
    z = torch.zeros(1, 7, 4, 4)
    with pytest.raises(NotImplementedError, match='Detectron'):
        iuvmap.iuv_map2img(z, z, z, uv_rois=[[0, 0, 0, 4, 4]])
    with pytest.raises(ValueError, match=r'ind_mapping\[0\]'):
        iuvmap.iuv_map2img(z, z, z, ind_mapping=[24, 1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match='entries'):
        iuvmap.iuv_map2img(z, z, z, ind_mapping=[0, 1, 2])
    with pytest.raises(ValueError, match='dp2smpl_mapping'):
        iuvmap.part_iuv_map2img(torch.zeros(1, 24, 3, 7, 4, 4))


def test_workspace_query_and_lights():
    from danet_densepose2smpl_amd import _lib
    from danet_densepose2smpl_amd.renderer import MeshRenderer
    assert _lib.lib().danet_mesh_shade_ws_bytes(4, 6890) == 2 * 4 * 6890 * 3 * 4
    r = MeshRenderer(np.array([[0, 1, 2]]), img_res=8)
    want = [x for (p, _) in vo.LIGHTS for x in vo.rotate_y(np.array(p), np.radians(120.))] + [1.] * 6 + [.7] * 3
    np.testing.assert_allclose(r.lights, want, rtol=0, atol=1e-9)
    assert MeshRenderer(np.array([[0, 1, 2]]), color=(0.2, 0.4, 0.6)).lights[9:] == [0.2, 0.4, 0.6] * 3
