"""The training visualisation on the GPU: the sheet kernels of csrc/train_vis.hip against the numpy oracle (train_vis_oracle.py:
the sheet rule, the overlay, the marker rule of DESIGN.md 4e), their capture under torch.cuda.graph, Trainer.visualize and the
vis_interval schedule of Trainer.fit, eager and graphed, on the synthetic 'h36m_dp' set of the train-loop tests (6 + 6 samples,
batch 4).

Bounds: copies, pad values, overlaid values and marker pixels are bit-exact.  De-normalised values: 2.4e-7 absolute (2 ulp of fp32
at 1.0, the output range; allows an FMA contraction of x * std + mean).  Normalised values: 1e-6 absolute (one subtraction and one
division at <= 1), hence at most 1 level after to_uint8's truncation."""
import json
import os
import types

import numpy as np
import pytest
import torch

import train_vis_oracle as tvo

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 32


def _np(t):
    return t.detach().to(torch.float32).cpu().numpy()


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _images(B, seed):
    """ImageNet-normalised images whose de-normalised values lie in [0, 1]."""
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed))
    return ((x - torch.tensor(tvo.MEAN)) / torch.tensor(tvo.STD)).to(DEV)


# ------------------------------------------------------------------------------------------------ the sheet rule
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,nrow,C,pad', [(3, 2, 3, 1), (3, 2, 1, 0), (9, 8, 1, 2), (9, 8, 3, 0), (1, 8, 3, 2), (1, 8, 1, 1)])
def test_grid_is_the_sheet_rule_bit_for_bit(dtype, B, nrow, C, pad):
    from danet_densepose2smpl_amd import train_vis as tv
    x = _rand((B, C, S, S), 7 * B + pad, dtype)
    got = tv.make_grid(x, nrow, pad, 0.25)
    want = tvo.make_grid(_np(x), nrow, pad, 0.25)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (3,) + tvo.grid_size(B, S, S, nrow, pad)
    np.testing.assert_array_equal(_np(got), want)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_grid_reads_a_non_contiguous_input(dtype):
    from danet_densepose2smpl_amd import train_vis as tv
    big = _rand((3, 2 * S + 1, S + 3, 5), 11, dtype)                  # [B, H', W', C']
    x = big.permute(0, 3, 1, 2)[:, 1:4, 1::2, 2:2 + S]                # [3,3,32,32]: channel stride 1, row stride 2 rows
    assert not x.is_contiguous() and tuple(x.shape) == (3, 3, S, S)
    np.testing.assert_array_equal(_np(tv.make_grid(x, 2, 1, 1.)), tvo.make_grid(_np(x), 2, 1, 1.))


def test_pair_grid_interleaves_the_two_sources():
    from danet_densepose2smpl_amd import train_vis as tv
    a, b = _rand((2, 3, S, S), 21), _rand((2, 3, S, S), 22)
    got = tv.pair_grid(a, b)
    want = tvo.pair_grid(_np(a), _np(b))
    assert tuple(got.shape) == (3, 2 * (S + 2) + 2, 2 * (S + 2) + 2)
    np.testing.assert_array_equal(_np(got), want)
    np.testing.assert_array_equal(want[:, 2:2 + S, 2 + S + 2:2 + S + 2 + S], _np(b[0]))       # b0 right of a0
    assert (want[:, :2] == 0).all()


# ------------------------------------------------------------------------------------------------ overlay, de-normalise
def _iuv(B, h, seed):
    g = torch.Generator().manual_seed(seed)
    iuv = torch.rand(B, 3, h, h, generator=g) * (torch.rand(B, 3, h, h, generator=g) > 0.5)
    iuv[0, 0, 1, 1], iuv[0, 1, 1, 1], iuv[0, 2, 1, 1] = 0., 0.6, 0.3        # zero in one plane, positive in the others: per channel
    iuv[1, 0, 2, 3], iuv[1, 1, 2, 3] = -0.4, 0.2                             # a negative value is not laid over
    return iuv.to(DEV)


@pytest.mark.parametrize('h', [8, 16])
def test_overlay_grid(h):
    from danet_densepose2smpl_amd import train_vis as tv
    B = 3
    img, iuv = _images(B, h), _iuv(B, h, 100 + h)
    got = _np(tv.overlay_grid(img, iuv))
    dn = tvo.denormalize(_np(img))
    want = tvo.make_grid(tvo.overlay(dn, _np(iuv)), 8, 1, 1.)
    up = np.repeat(np.repeat(_np(iuv), S // h, 2), S // h, 3)
    laid = tvo.make_grid(np.where(up > 0, 1., 0.), 8, 1, 0.) > 0             # where the sheet shows an overlaid value
    tile = tvo.make_grid(np.ones_like(dn), 8, 1, 0.) > 0
    assert laid.any() and (tile & ~laid).any() and got.shape == want.shape
    np.testing.assert_array_equal(got[laid], want[laid])
    np.testing.assert_array_equal(got[~tile], want[~tile])
    err = float(np.abs(got - want)[tile & ~laid].max())
    print('overlay_grid h=%d: max |de-normalised - oracle| = %.3e' % (h, err))
    assert err <= 2.4e-7
    f = S // h                                                              # the per-channel case of sample 0, low-res pixel (1, 1)
    y, x = 1 + f, 1 + f
    assert abs(got[0, y, x] - dn[0, 0, f, f]) <= 2.4e-7 and got[1, y, x] == np.float32(0.6) and got[2, y, x] == np.float32(0.3)


def test_overlay_with_a_fractional_factor_is_refused():
    from danet_densepose2smpl_amd import train_vis as tv
    with pytest.raises(RuntimeError, match='integer factor'):
        tv.overlay_grid(_images(2, 1), torch.zeros(2, 3, 12, 12, device=DEV))


# ------------------------------------------------------------------------------------------------ normalise
def test_normalised_grid():
    from danet_densepose2smpl_amd import train_vis as tv
    x = _rand((3, 3, S, S), 31)
    got = _np(tv.make_grid(x, 8, 1, 1., normalize=True))
    want = tvo.make_grid(tvo.normalize(_np(x)), 8, 1, 1.)
    err = float(np.abs(got - want).max())
    print('normalised grid: max |got - oracle| = %.3e' % err)
    assert err <= 1e-6 and got.min() == 0.0 and got.max() <= 1.0
    const = _np(tv.make_grid(torch.full((2, 3, S, S), 0.37, device=DEV), 8, 1, 1., normalize=True))
    assert np.isfinite(const).all()
    np.testing.assert_array_equal(const, tvo.make_grid(np.zeros((2, 3, S, S), np.float32), 8, 1, 1.))     # hi == lo: 0, not NaN


# ------------------------------------------------------------------------------------------------ the marker rule
def _joints(B=3, J=24):
    j = torch.rand(B, J, 2, generator=torch.Generator().manual_seed(5)) * 26 + 3          # inside the tile
    j[0, 0] = torch.tensor([5.5, 6.2])
    j[0, 1] = torch.tensor([0., 31.9])                       # on the tile border
    j[0, 2] = torch.tensor([31., 0.])
    j[0, 3] = torch.tensor([40., 10.])                       # inside the neighbouring tile
    j[0, 4] = torch.tensor([-0.5, 2.9])                      # truncation toward zero
    j[0, 5] = torch.tensor([-5., -3.])                       # negative: off the sheet
    j[1, 6] = torch.tensor([1000., 1000.])                   # beyond the sheet
    j[1, 7] = torch.tensor([1e12, 3.])
    j[1, 8] = torch.tensor([float('nan'), 4.])
    j[1, 9] = torch.tensor([4., float('inf')])
    j[1, 10] = torch.tensor([float('-inf'), float('nan')])
    j[2, 12] = j[2, 13] = torch.tensor([12.3, 12.9])         # coincident: the higher index wins
    j[2, 14] = torch.tensor([13.1, 12.2])                    # overlapping its neighbours
    j[2, 15] = torch.tensor([31.5, 31.5])                    # tile 2's last pixel: the plus reaches the sheet's pad frame
    j[2, 16] = torch.tensor([-40., 20.])                     # left of the sheet: clipped
    return j


@pytest.mark.parametrize('with_vis', [False, True])
def test_markers(with_vis):
    from danet_densepose2smpl_amd import train_vis as tv
    B, J, nrow, pad = 3, 24, 2, 1
    img, joints = _images(B, 41), _joints(B, J)
    vis = None
    if with_vis:
        vis = torch.ones(B, J, 1)
        vis[0, 0] = vis[2, 13] = vis[1, 20] = 0
    Hs, Ws = tvo.grid_size(B, S, S, nrow, pad)
    buf = torch.full((Ws + 3 * Hs * Ws + Ws,), 7.0, device=DEV)                 # a canary row before and after the sheet
    sheet = buf[Ws:Ws + 3 * Hs * Ws].view(3, Hs, Ws)
    sheet.copy_(tv.make_grid(img, nrow, pad, 1., normalize=True, denormalize=True))
    before = _np(sheet)
    out = tv.draw_joints(sheet, joints.to(DEV), None if vis is None else vis.to(DEV), (S, S), nrow, pad)
    assert out.data_ptr() == sheet.data_ptr()
    got = _np(sheet)
    assert (_np(buf[:Ws]) == 7.0).all() and (_np(buf[-Ws:]) == 7.0).all()
    px = tvo.marker_pixels(B, S, S, joints.numpy(), None if vis is None else vis.numpy(), nrow, pad)
    mask = np.zeros((Hs, Ws), bool)
    for (y, x) in px:
        mask[y, x] = True
    assert mask.sum() == len(px) > 5 * 40
    want = tvo.draw_joints(before, B, S, S, joints.numpy(), None if vis is None else vis.numpy(), nrow, pad)
    np.testing.assert_array_equal(got[:, mask], want[:, mask])
    np.testing.assert_array_equal(got[:, ~mask], before[:, ~mask])              # nothing but marker pixels changes
    # against the oracle's own sheet, after to_uint8: markers exact, the normalised rest within one level
    osheet = tvo.draw_joints(tvo.make_grid(tvo.normalize(tvo.denormalize(_np(img))), nrow, pad, 1.), B, S, S, joints.numpy(),
                             None if vis is None else vis.numpy(), nrow, pad)
    g8, o8 = tv.to_uint8(sheet).cpu().numpy().astype(np.int32), tvo.to_uint8(osheet).astype(np.int32)
    np.testing.assert_array_equal(g8[:, mask], o8[:, mask])
    assert set(np.unique(g8[:, mask])) <= {0, 255}
    lev = int(np.abs(g8 - o8).max())
    print('markers: max level difference off the markers = %d' % lev)
    assert lev <= 1
    # the cases, spelled out (33-pixel cells: tile 0's corner is (1, 1), tile 1's (34, 1), tile 2's (1, 34); px is keyed (y, x))
    assert px[(11, 41)] == 3 and tuple(got[:, 11, 41]) == (1, 0, 0)                  # (40, 10) of tile 0 lands inside tile 1: odd, red
    assert px[(3, 0)] == 4 and (3, 1) in px and tuple(got[:, 3, 0]) == (0, 1, 0)      # (-0.5, 2.9): int(0.5), int(3.9); (3, -1) is clipped
    assert px[(32, 1)] == 1 and px[(33, 1)] == 1                                     # (0, 31.9) on tile 0's border reaches the padding row
    assert px[(65, 32)] == 15 and (66, 32) in px and (65, 33) in px                  # tile 2's last pixel reaches the sheet's pad frame
    assert px[(45, 13)] == (12 if with_vis else 13)                                  # coincident 12 / 13: the higher visible index wins
    assert tuple(got[:, 45, 13]) == ((0, 1, 0) if with_vis else (1, 0, 0))
    assert px[(46, 13)] == 14                                                        # ... and joint 14's plus covers their centre
    if with_vis:
        assert (7, 6) not in px or px[(7, 6)] != 0                                   # joint 0 of tile 0 (5.5, 6.2) is hidden
    else:
        assert px[(7, 6)] == 0


# ------------------------------------------------------------------------------------------------ capture
def test_sheets_capture_and_replay_equals_eager():
    from danet_densepose2smpl_amd import train_vis as tv
    B = 3
    img, iuv, joints = _images(B, 51), _iuv(B, 8, 52), _joints(B).to(DEV)

    def sheets():
        return tv.to_uint8(tv.overlay_grid(img, iuv)), tv.to_uint8(tv.joints_grid(img, joints)), tv.pair_grid(img, img)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sheets()                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = sheets()
    for seed in (61, 62):
        img.copy_(_images(B, seed))
        iuv.copy_(_iuv(B, 8, seed + 10))
        joints.copy_(_joints(B).to(DEV) + float(seed - 60))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, sheets()):
            assert torch.equal(got, want)
    assert not torch.equal(static[0], torch.zeros_like(static[0]))


# ------------------------------------------------------------------------------------------------ Trainer.visualize, Trainer.fit
SHEET_TAGS = ('opt_shape', 'pred_shape', 'pred_uv', 'gt_uv', 'part_uvi_pred', 'skps_hm_pred', 'skps_hm_pred_soft', 'stn_centers_gt',
              'stn_centers_pred')


def _options(root, tag, **kw):
    from danet_densepose2smpl_amd.config import cfg
    o = types.SimpleNamespace(batch_size=4, openpose_train_weight=0., gt_train_weight=1., train_data='h36m_dp', num_epochs=3, pretr_step=1,
                              checkpoint_steps=10000, summary_steps=1, num_workers=2, seed=3, shuffle_train=True, time_to_run=None, resume=None,
                              pretrained_checkpoint=None, log_dir=os.path.join(root, 'log_' + tag), checkpoint_dir=os.path.join(root, 'ck_' + tag),
                              heatmap_size=cfg.DANET.HEATMAP_SIZE, img_res=cfg.DANET.INIMG_SIZE, graph=False)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from danet_densepose2smpl_amd import datasets
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    reset_cfg()
    root = str(tmp_path_factory.mktemp('trainvis'))
    o = _options(root, 'data')
    ds, paths = datasets.synthetic_mixed_dataset(o, os.path.join(root, 'data'), 6, 6, seed=5)
    fits = FitsDict(o, ds, paths['final_fits_dir'], paths['static_fits_dir'], torch.device('cuda'))
    return types.SimpleNamespace(root=root, ds=ds, paths=paths, fits=fits)


def _fit(world, tag, unset=(), **kw):
    """One fit from the module's seed; every visualize() result is kept as it was returned (cloned: a replayed step's sources are
    overwritten by the next replay)."""
    from danet_densepose2smpl_amd.config import reset_cfg
    from danet_densepose2smpl_amd.trainer import Trainer
    reset_cfg()
    o = _options(world.root, tag, **kw)
    for k in unset:
        delattr(o, k)
    torch.manual_seed(0)
    tr = Trainer(o)
    r = types.SimpleNamespace(o=o, steps=[], losses=[], vis_on=[], kps=[], seen={}, trainer=tr)
    inner = tr.visualize

    def visualize(in_dict, output, losses=None):
        kps = in_dict['target_smpl_kps'].clone()
        out = inner(in_dict, output, losses)
        assert torch.equal(kps, in_dict['target_smpl_kps'])                   # the caller's tensor is not scaled in place
        r.seen[tr.step_count] = ({k: v.clone() for k, v in out.items()}, bool(in_dict['pretrain_mode']), in_dict, output)
        return out
    tr.visualize = visualize

    def on_step(s, d, l):
        r.steps.append(s)
        r.vis_on.append(d['vis_on'])
        r.losses.append({k: float(v.detach()) for k, v in l.items()})
    r.n = tr.fit(world.ds, world.fits, o, on_step=on_step)
    torch.cuda.synchronize()
    r.stats = dict(tr.fit_stats)
    r.log = [json.loads(ln) for ln in open(os.path.join(o.log_dir, 'train_log.jsonl'))]
    return r


@pytest.fixture(scope='module')
def eager_vis(world):
    return _fit(world, 'eager_vis', vis_interval=2)


def _sheet_dirs(o):
    d = os.path.join(o.log_dir, 'vis')
    return sorted(os.listdir(d)) if os.path.isdir(d) else None


def test_visualize_returns_the_reference_tags_as_uint8_sheets(eager_vis):
    from danet_densepose2smpl_amd import iuvmap, train_vis as tv
    from danet_densepose2smpl_amd.config import cfg
    R, hm, B = cfg.DANET.INIMG_SIZE, cfg.DANET.HEATMAP_SIZE, 4
    assert sorted(eager_vis.seen) == [1, 3]
    for step, pretrain in ((1, True), (3, False)):
        sheets, was_pretrain, in_dict, output = eager_vis.seen[step]
        assert was_pretrain == pretrain
        want = {'opt_shape': tvo.grid_size(2 * B, R, R, 2, 2), 'pred_uv': tvo.grid_size(B, R, R, 8, 1), 'gt_uv': tvo.grid_size(B, R, R, 8, 1),
                'skps_hm_pred': tvo.grid_size(B, hm, hm, 8, 1), 'skps_hm_pred_soft': tvo.grid_size(B, hm, hm, 8, 1),
                'stn_centers_gt': tvo.grid_size(B, R, R, 8, 1), 'stn_centers_pred': tvo.grid_size(B, R, R, 8, 1)}
        if not pretrain:
            want.update({'pred_shape': tvo.grid_size(2 * B, R, R, 2, 2), 'part_uvi_pred': tvo.grid_size(24, hm, hm, 8, 1)})
        scalars = {'index_fg'} | (set() if pretrain else {'p_index_fg'})
        assert set(sheets) == set(want) | scalars, (step, sorted(sheets))
        assert 'part_uvi_gt' not in sheets                                      # the fused path does not materialise part_iuv_gt
        for tag, hw in want.items():
            assert tag in SHEET_TAGS and sheets[tag].dtype == torch.uint8 and sheets[tag].is_cuda and tuple(sheets[tag].shape) == (3,) + hw, tag
        for k in scalars:
            assert sheets[k].dim() == 0 and 0.0 <= float(sheets[k]) <= 1.0
    # pred_uv recomputed from the last step's state (its in_dict and output are still alive: the run was eager)
    sheets, _, in_dict, output = eager_vis.seen[3]
    again = tv.to_uint8(tv.overlay_grid(in_dict['img'], iuvmap.iuv_map2img(*output['visualization']['iuv_pred'])))
    assert torch.equal(sheets['pred_uv'], again)
    assert len(torch.unique(sheets['pred_uv'])) > 2 and len(torch.unique(sheets['opt_shape'])) > 2


def test_eager_fit_writes_sheets_on_the_schedule(eager_vis):
    r = eager_vis
    assert r.n == 3 and r.steps == [1, 2, 3] and r.vis_on == [True, False, True]
    assert _sheet_dirs(r.o) == ['step_00000001', 'step_00000003']
    for step in (1, 3):
        sheets = r.seen[step][0]
        folder = os.path.join(r.o.log_dir, 'vis', 'step_%08d' % step)
        tags = sorted(t for t in sheets if sheets[t].dim() == 3)
        assert sorted(os.listdir(folder)) == [t + '.png' for t in tags]
        for t in tags:
            png = tvo.png_decode(open(os.path.join(folder, t + '.png'), 'rb').read())
            np.testing.assert_array_equal(png, sheets[t].cpu().numpy().transpose(1, 2, 0))
    by_step = {l['step']: l for l in r.log}
    assert sorted(by_step) == [1, 2, 3]
    for step in (1, 3):
        assert 0.0 <= by_step[step]['index_fg'] <= 1.0
        assert by_step[step]['index_fg'] == float(r.seen[step][0]['index_fg'])
    assert 0.0 <= by_step[3]['p_index_fg'] <= 1.0 and 'p_index_fg' not in by_step[1] and 'index_fg' not in by_step[2]


def test_vis_interval_zero_is_the_run_without_the_option(world):
    """vis_interval = 0 against a run whose options carry no vis_interval at all: no vis directory, vis_on never set, and the losses
    of the three steps equal bit for bit."""
    off = _fit(world, 'off', vis_interval=0)
    unset = _fit(world, 'unset')
    assert not hasattr(unset.o, 'vis_interval')
    for r in (off, unset):
        assert r.n == 3 and _sheet_dirs(r.o) is None and r.vis_on == [False] * 3 and not r.seen
        assert all('index_fg' not in l for l in r.log)
    for s, (a, b) in enumerate(zip(off.losses, unset.losses), 1):
        for k in a:
            print('step %d %-22s vis_interval=0 %.9g unset %.9g' % (s, k, a[k], b[k]))
    assert off.losses == unset.losses


def test_graphed_fit_reads_live_static_outputs(world):
    """4 steps, vis_interval 3: sheets after step 1 (eager) and step 4 (replayed); the counts of the run without visualisation.
    summary_steps 100: step 4 is off the summary schedule and gets a log line of its own."""
    kw = dict(graph=True, pretr_step=0, num_epochs=4, summary_steps=100)
    vis = _fit(world, 'graph_vis', vis_interval=3, **kw)
    vis.trainer.drop_graph()
    plain = _fit(world, 'graph_plain', **kw)
    plain.trainer.drop_graph()
    assert vis.n == plain.n == 4
    assert vis.stats == plain.stats == {'eager_steps': 2, 'replayed_steps': 2, 'captures': 1}
    assert vis.vis_on == [True] * 4 and plain.vis_on == [False] * 4             # the switch is frozen into the capture
    assert _sheet_dirs(vis.o) == ['step_00000001', 'step_00000004'] and _sheet_dirs(plain.o) is None
    assert sorted(vis.seen) == [1, 4]
    first, last = vis.seen[1][0]['pred_uv'], vis.seen[4][0]['pred_uv']
    assert len(torch.unique(last)) > 2 and not torch.equal(first, last)
    png = tvo.png_decode(open(os.path.join(vis.o.log_dir, 'vis', 'step_00000004', 'pred_uv.png'), 'rb').read())
    np.testing.assert_array_equal(png, last.cpu().numpy().transpose(1, 2, 0))
    assert set(vis.seen[4][0]) == set(vis.seen[1][0])
    assert [l['step'] for l in vis.log] == [1, 4] and [l['step'] for l in plain.log] == [1]
    assert 'loss_tatal' in vis.log[0] and 0.0 <= vis.log[0]['index_fg'] <= 1.0
    assert set(vis.log[1]) == {'step', 'epoch', 'batch_idx', 'index_fg', 'p_index_fg'} and 0.0 <= vis.log[1]['index_fg'] <= 1.0
