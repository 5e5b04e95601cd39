"""Host-side checks of the training visualisation (no GPU): known answers for the numpy oracle of the sheet rule and the marker
rule, the shared PNG writer's round trip, the visualisation schedule, and build_in_dict's default."""
import inspect

import numpy as np
import pytest
import torch

import train_vis_oracle as tvo


def test_oracle_sheet_worked_out_by_hand():
    """[3,1,2,2], nrow 2, padding 1, pad 1: 7 x 7, tiles at (1,1), (1,4), (4,1); the fourth cell is all pad."""
    t = np.arange(12, dtype=np.float32).reshape(3, 1, 2, 2) * 0.01
    s = tvo.make_grid(t, nrow=2, padding=1, pad_value=1.)
    assert s.shape == (3, 7, 7) and tvo.grid_size(3, 2, 2, 2, 1) == (7, 7)
    want = np.ones((7, 7), np.float32)
    want[1:3, 1:3] = t[0, 0]
    want[1:3, 4:6] = t[1, 0]
    want[4:6, 1:3] = t[2, 0]
    for c in range(3):                                               # C = 1 is replicated
        np.testing.assert_array_equal(s[c], want)
    assert (s[:, 4:6, 4:6] == 1).all()
    assert tvo.grid_size(9, 32, 32, 8, 2) == (2 * 34 + 2, 8 * 34 + 2) and tvo.grid_size(1, 32, 32, 8, 0) == (32, 32)


def test_oracle_pair_grid_interleaves():
    a, b = np.full((2, 3, 1, 1), 0.25, np.float32), np.full((2, 3, 1, 1), 0.75, np.float32)
    a[1], b[1] = 0.3, 0.8
    s = tvo.pair_grid(a, b)
    assert s.shape == (3, 2 * 3 + 2, 2 * 3 + 2)
    assert s[0, 2, 2] == np.float32(0.25) and s[0, 2, 5] == np.float32(0.75) and s[0, 5, 2] == np.float32(0.3) and s[0, 5, 5] == np.float32(0.8)
    assert s[0, 0, 0] == 0 and s[0, 3, 3] == 0


def test_oracle_overlay_is_per_element_and_refuses_a_fraction():
    img = np.full((1, 3, 4, 4), 0.5, np.float32)
    iuv = np.zeros((1, 3, 2, 2), np.float32)
    iuv[0, 0, 0, 0], iuv[0, 1, 0, 0], iuv[0, 2, 1, 1] = 0.0, 0.7, -0.2
    out = tvo.overlay(img, iuv)
    assert (out[0, 0, :2, :2] == 0.5).all() and (out[0, 1, :2, :2] == np.float32(0.7)).all()      # same pixel, channel by channel
    assert (out[0, 2, 2:, 2:] == 0.5).all()                                                    # a negative value is not laid over
    with pytest.raises(ValueError):
        tvo.overlay(np.zeros((1, 3, 32, 32), np.float32), np.zeros((1, 3, 12, 12), np.float32))


def test_oracle_normalize_of_a_constant_batch_is_zero():
    assert (tvo.normalize(np.full((2, 3, 2, 2), 0.37, np.float32)) == 0).all()
    x = np.array([0., 1., 3.], np.float32).reshape(1, 1, 1, 3)
    np.testing.assert_allclose(tvo.normalize(x).ravel(), [0, 1 / 3.00001, 3 / 3.00001], rtol=1e-6)


def test_oracle_marker_parity_truncation_clipping_overlap():
    # joints 0 and 1 of one 8 x 8 tile, padding 1: even green, odd red
    j = np.array([[[3., 3.], [6., 6.]]], np.float32)
    s = tvo.draw_joints(np.full((3, 10, 10), 0.5, np.float32), 1, 8, 8, j)
    assert tuple(s[:, 4, 4]) == (0, 1, 0) and tuple(s[:, 7, 7]) == (1, 0, 0)
    assert sorted(tvo.marker_pixels(1, 8, 8, j[:, :1])) == [(3, 4), (4, 3), (4, 4), (4, 5), (5, 4)]
    assert int((s != 0.5).any(axis=0).sum()) == 10
    # (2.9, -0.5) -> (2, 0): truncation toward zero, not floor (padding 0: the tile's corner is the sheet's)
    px = tvo.marker_pixels(1, 8, 8, np.array([[[2.9, -0.5]]], np.float32), padding=0)
    assert sorted(px) == [(0, 1), (0, 2), (0, 3), (1, 2)]
    # a plus at the sheet's corner keeps 3 pixels
    assert sorted(tvo.marker_pixels(1, 8, 8, np.array([[[0., 0.]]], np.float32), padding=0)) == [(0, 0), (0, 1), (1, 0)]
    # overlap: the higher index wins
    px = tvo.marker_pixels(1, 8, 8, np.array([[[3., 3.], [4., 3.]]], np.float32), padding=0)
    assert px[(3, 3)] == 1 and px[(3, 4)] == 1 and px[(3, 2)] == 0 and px[(2, 3)] == 0
    # the later tile wins over an earlier tile's joint that lands in it; NaN, inf and visibility 0 are skipped
    jj = np.array([[[np.nan, 1.], [9., 0.]], [[0., 0.], [np.inf, 2.]]], np.float32)
    px = tvo.marker_pixels(2, 8, 8, jj, padding=1)
    assert len(px) == 5 and all(v == 0 for v in px.values()) and px[(1, 10)] == 0
    assert tvo.marker_pixels(2, 8, 8, jj, vis=np.array([[1, 1], [0, 1]], np.float32), padding=1)[(1, 10)] == 1
    assert tvo.marker_pixels(2, 8, 8, jj, vis=np.array([[1, 0], [0, 1]], np.float32), padding=1) == {}


def test_oracle_to_uint8_truncates():
    np.testing.assert_array_equal(tvo.to_uint8(np.array([0., 0.999, 1., 1.5, -0.2, 0.5], np.float32)), [0, 254, 255, 255, 0, 127])


@pytest.mark.parametrize('as_tensor', [False, True])
def test_write_png_round_trip(tmp_path, as_tensor):
    from danet_densepose2smpl_amd import train_vis
    rng = np.random.default_rng(3)
    sheet = rng.integers(0, 256, (3, 11, 17)).astype(np.uint8)         # [3,Hs,Ws] as to_uint8 returns it
    p = str(tmp_path / 's.png')
    train_vis.write_png(p, torch.from_numpy(sheet) if as_tensor else np.transpose(sheet, (1, 2, 0)))
    np.testing.assert_array_equal(tvo.png_decode(open(p, 'rb').read()), np.transpose(sheet, (1, 2, 0)))
    with pytest.raises(ValueError):
        train_vis.write_png(p, sheet.astype(np.float32).transpose(1, 2, 0))


def test_to_uint8_is_the_reference_expression():
    from danet_densepose2smpl_amd import train_vis
    x = torch.tensor([0., 0.999, 1., 1.5, -0.2, 0.5])
    assert train_vis.to_uint8(x).tolist() == [0, 254, 255, 255, 0, 127]


def test_vis_schedule():
    from danet_densepose2smpl_amd.train_vis import vis_due
    steps = range(1, 11)
    assert [s for s in steps if vis_due(s, 0)] == [] and [s for s in steps if vis_due(s, None)] == []
    assert [s for s in steps if vis_due(s, 1)] == list(steps)
    assert [s for s in steps if vis_due(s, 3)] == [1, 4, 7, 10]


def test_build_in_dict_defaults_to_vis_off_and_ops_refuse_cpu_tensors():
    from danet_densepose2smpl_amd import train_vis
    from danet_densepose2smpl_amd.trainer import Trainer
    assert inspect.signature(Trainer.build_in_dict).parameters['vis_on'].default is False
    assert callable(Trainer.visualize)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        train_vis.make_grid(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        train_vis.draw_joints(torch.zeros(3, 6, 6), torch.zeros(1, 2, 2), None, (4, 4))
