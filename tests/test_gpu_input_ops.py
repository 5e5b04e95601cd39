"""The two input ops of the training pipeline (csrc/input_ops.hip) and the device FitsDict against augment.py on the CPU in float64.

Oracle of the crop: augment.rgb_processing on the batch as evaluate.collate lays it out -- every image zero-padded to the batch's
largest size (64 x 64 here), which is what "a tap outside the image contributes zero" means for images of different sizes."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import record
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_oracle as eo    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROTS = (0., 30., -47.5, 90., 180.)
SIZES = ((1, 1), (7, 5), (33, 64), (64, 33), (50, 50), (50, 50))           # (rows, cols); the last sample's crop misses its image
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
_CACHE = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _crop_case(res, rnd):
    """Inputs of round `rnd` (the rotations, flips and noise ends move over the samples from round to round) and the float64 oracle,
    computed once."""
    key = (res, rnd)
    if key not in _CACHE:
        from danet_densepose2smpl_amd import augment
        rng = np.random.default_rng(100 * res + rnd)
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
        B = len(imgs)
        center = np.array([[rng.uniform(-0.1, 1.1) * w, rng.uniform(-0.1, 1.1) * h] for h, w in SIZES])
        scale = np.array([rng.uniform(0.4, 1.3) * max(h, w, 4) / 200. for h, w in SIZES])
        center[-1], scale[-1] = (400., -300.), 0.2
        rot = np.array([ROTS[(b + rnd) % 5] for b in range(B)])
        flip = np.array([(b + rnd) % 2 for b in range(B)])
        pn = np.array([[0.6, 1.4, 1.0][(b + rnd + c) % 3] for b in range(B) for c in range(3)]).reshape(B, 3)
        pn[(rnd + 1) % B], pn[(rnd + 3) % B] = 0.6, 1.4                        # both ends of the range on all three channels
        pad = np.zeros((B, 64, 64, 3), np.uint8)
        for b, im in enumerate(imgs):
            pad[b, :im.shape[0], :im.shape[1]] = im
        pad = torch.from_numpy(pad).permute(0, 3, 1, 2)
        args = [torch.from_numpy(a) for a in (center, scale, rot, flip, pn)]
        want = augment.rgb_processing(pad.double(), *args, res=res).numpy()
        _CACHE[key] = (imgs, center, scale, rot, flip, pn, pad, want)
    return _CACHE[key]


def _run_crop(imgs, center, scale, rot, flip, pn, res, whole=False):
    from danet_densepose2smpl_amd import datasets, ops
    cp = datasets.crop_params(imgs, center, scale, rot, flip, pn, res, whole=whole)
    geom = _t(cp['geom'])
    return ops.batch_crop(_t(cp['src']), _t(cp['offsets']), geom[0], geom[1], _t(cp['params']), res), cp


@pytest.mark.parametrize('res', [16, 32])
def test_batch_crop_against_rgb_processing_in_float64(res):
    """e_new <= 2 e_old: e_new the op's largest distance from the float64 oracle, e_old that of the float32 device path
    (augment.rgb_processing on the GPU, what evaluate.to_device runs).  Measured on MI355X: e_new 1.19e-7 at both sizes, e_old 2.57e-5 (res 16) and 3.19e-5 (res 32)."""
    from danet_densepose2smpl_amd import augment
    e_new = e_old = 0.0
    clamped = 0
    for rnd in range(5):
        imgs, center, scale, rot, flip, pn, pad, want = _crop_case(res, rnd)
        got, _ = _run_crop(imgs, center, scale, rot, flip, pn, res)
        assert got.shape == (6, 3, res, res) and got.dtype == torch.float32
        old = augment.rgb_processing(pad.to(DEV).float(), _t(center), _t(scale), _t(rot), _t(flip), _t(pn), res=res)
        e_new = max(e_new, float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()))
        e_old = max(e_old, float(np.abs(old.cpu().numpy().astype(np.float64) - want).max()))
        # the sample whose crop misses its image: -mean / std everywhere
        blank = np.broadcast_to((-MEAN / STD).astype(np.float32).reshape(3, 1, 1), (3, res, res))
        np.testing.assert_array_equal(got[-1].cpu().numpy(), blank)
        clamped += int((want[:-1] == ((1 - MEAN) / STD).reshape(1, 3, 1, 1)).sum())
        assert np.abs(want[:-1] - (-MEAN / STD).reshape(1, 3, 1, 1)).max() > 1          # the others do see their images
    print('batch_crop res %d: e_new %.3e e_old %.3e clamped pixels %d' % (res, e_new, e_old, clamped))
    record('batch_crop_vs_fp64_res%d' % res, {'e_new': e_new, 'e_old': e_old})
    assert clamped > 0                                                        # the clamp fires
    assert e_new <= 2 * e_old, (e_new, e_old)


@pytest.mark.parametrize('res', [16, 32])
def test_batch_crop_identity_transform_known_answer(res):
    """center = (res/2, res/2), scale = res/200, rot = 0: the transform is the identity, the output the source through flip, noise and
    normalisation -- to one float32 rounding."""
    rng = np.random.default_rng(res)
    B = 4
    imgs = [rng.integers(0, 256, (res, res, 3), dtype=np.uint8) for _ in range(B)]
    flip = np.array([0, 1, 0, 1])
    pn = rng.uniform(0.6, 1.4, (B, 3))
    got, _ = _run_crop(imgs, np.full((B, 2), res / 2.), np.full(B, res / 200.), np.zeros(B), flip, pn, res)
    for b in range(B):
        x = imgs[b].astype(np.float64).transpose(2, 0, 1)
        if flip[b]:
            x = x[:, :, ::-1]
        want = ((np.clip(x * pn[b].reshape(3, 1, 1), 0., 255.) / 255.) - MEAN.reshape(3, 1, 1)) / STD.reshape(3, 1, 1)
        g = got[b].cpu().numpy()
        assert (np.abs(g.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


def test_batch_crop_footprint_packing_is_bit_identical_to_whole_images():
    rng = np.random.default_rng(7)
    res = 32
    for rnd in range(5):
        imgs, center, scale, rot, flip, pn, _, _ = _crop_case(res, rnd)
        big = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)                         # a crop much smaller than its photograph
        imgs = imgs + [big]
        center, scale = np.concatenate([center, [[150., 90.]]]), np.concatenate([scale, [0.25]])
        rot, flip, pn = np.concatenate([rot, [ROTS[rnd]]]), np.concatenate([flip, [rnd % 2]]), np.concatenate([pn, [[1.2, 0.7, 1.0]]])
        a, cpa = _run_crop(imgs, center, scale, rot, flip, pn, res)
        b, cpb = _run_crop(imgs, center, scale, rot, flip, pn, res, whole=True)
        assert torch.equal(a, b)
        assert cpa['src'].size < cpb['src'].size / 3 and (cpa['geom'][1, -1] > 0).all()
        assert (cpa['geom'][0, 5] == 0).all()                                             # the crop that misses its image packs nothing


def test_batch_crop_under_graph_replay():
    from danet_densepose2smpl_amd import datasets, ops
    res = 32
    imgs, center, scale, rot, flip, pn, _, _ = _crop_case(res, 0)
    cp = datasets.crop_params(imgs, center, scale, rot, flip, pn, res, whole=True)
    src, off, geom, par = _t(cp['src']), _t(cp['offsets']), _t(cp['geom']), _t(cp['params'])
    out = torch.empty(6, 3, res, res, device=DEV)
    eager = ops.batch_crop(src, off, geom[0], geom[1], par, res).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.batch_crop(src, off, geom[0], geom[1], par, res, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.batch_crop(src, off, geom[0], geom[1], par, res, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    imgs2, center2, scale2, rot2, flip2, pn2, _, _ = _crop_case(res, 3)       # same sizes: new contents through the same buffers
    cp2 = datasets.crop_params(imgs2, center2, scale2, rot2, flip2, pn2, res, whole=True)
    src.copy_(_t(cp2['src']))
    par.copy_(_t(cp2['params']))
    g.replay()
    torch.cuda.synchronize()
    geom2 = _t(cp2['geom'])
    want = ops.batch_crop(_t(cp2['src']), _t(cp2['offsets']), geom2[0], geom2[1], _t(cp2['params']), res)
    assert torch.equal(out, want) and not torch.equal(out, eager)
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.batch_crop(src.cpu(), off, geom[0], geom[1], par, res)


# ---- label_augment -------------------------------------------------------------------------------------------------------------
def _ulp_equal(got, want64, what):
    """Equal after rounding both to float32, up to one float32 ulp."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > np.spacing(np.abs(want))
    assert not bad.any(), (what, got[bad][:4], want[bad][:4])


def _orientations(rng, rot, lo, hi):
    """Global orientations whose rotation by `rot` (augment.rot_aa) has its angle in [lo, hi]: drawn until it has."""
    from danet_densepose2smpl_amd import augment
    out = np.zeros((len(rot), 3))
    for b, r in enumerate(rot):
        while True:
            ax = rng.normal(size=3)
            aa = ax / np.linalg.norm(ax) * rng.uniform(0.05, np.pi)
            ang = float(augment.rot_aa(torch.from_numpy(aa[None]), torch.tensor([r])).norm())
            if lo <= ang <= hi:
                out[b] = aa
                break
    return out


def _label_case():
    rng = np.random.default_rng(2024)
    B, res = 7, 224
    rot = np.array([0., 30., -47.5, 90., 180., 0., -12.25])
    flip = np.array([0, 1, 0, 1, 1, 0, 1])
    center, scale = rng.uniform(80, 240, (B, 2)), rng.uniform(0.6, 1.8, B)
    kp = np.concatenate([rng.uniform(0, 320, (B, 49, 2)), (rng.random((B, 49, 1)) > 0.3).astype(np.float64)], -1)
    sk = np.concatenate([rng.uniform(0, 320, (B, 24, 2)), (rng.random((B, 24, 1)) > 0.4).astype(np.float64)], -1)
    S = rng.normal(0, 0.4, (B, 24, 4))
    pose = rng.normal(0, 0.3, (B, 72))
    pose[:, :3] = _orientations(rng, rot, 0.2, np.pi - 0.2)
    return B, res, rot, flip, center, scale, kp, sk, S, pose


def test_label_augment_against_augment_on_the_cpu():
    from danet_densepose2smpl_amd import augment, constants, datasets, ops
    B, res, rot, flip, center, scale, kp, sk, S, pose = _label_case()
    tc = lambda a: torch.from_numpy(np.asarray(a))          # noqa: E731
    # the oracle alone: coordinates within 1e-6 of an integer before the truncation are left out; they are at most 1 %
    t = augment.get_transform(tc(center), tc(scale), [res, res], tc(rot))
    hom = lambda p: torch.cat([tc(p[..., :2] + 1) - 1, torch.ones(B, p.shape[1], 1, dtype=torch.float64)], -1)       # noqa: E731
    near = []
    for p in (kp, sk):
        pre = torch.einsum('bij,bnj->bni', t, hom(p))[..., :2].numpy()
        near.append(np.abs(pre - np.rint(pre)) < 1e-6)
    assert sum(int(n.sum()) for n in near) <= 0.01 * sum(n.size for n in near)
    want_kp = augment.j2d_processing(tc(kp), tc(center), tc(scale), tc(rot), tc(flip), res).numpy()
    w = augment.j2d_processing(tc(sk), tc(center), tc(scale), tc(rot), torch.zeros(B), res).numpy()            # base_dataset.py:258-263
    w[w[:, :, 2] == 0] = 0
    fl = w[:, constants.SMPL_JOINTS_FLIP_PERM].copy()
    fl[:, :, 0] = -fl[:, :, 0]
    want_sk = np.where(flip.reshape(B, 1, 1) > 0, fl, w)
    want_S = augment.j3d_processing(tc(S), tc(rot), tc(flip)).numpy()
    want_pose = augment.pose_processing(tc(pose), tc(rot), tc(flip)).numpy()
    xf, _ = datasets.crop_transforms(center, scale, rot, res)
    out = ops.label_augment(_t(np.stack([rot, flip.astype(np.float64)], 1)), _t(xf[:, :2].reshape(B, 6)), _t(kp), _t(sk), _t(S), _t(pose), res=res)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert set(got) == {'keypoints', 'smpl_2dkps', 'pose_3d', 'pose'}
    # (a flipped row's coordinates come from row perm[j]: the mask of left-out coordinates moves with them)
    keep_kp = ~np.where(flip.reshape(B, 1, 1) > 0, near[0][:, constants.J49_FLIP_PERM], near[0])
    keep_sk = ~np.where(flip.reshape(B, 1, 1) > 0, near[1][:, constants.SMPL_JOINTS_FLIP_PERM], near[1])
    for g, wnt, keep, what in ((got['keypoints'], want_kp, keep_kp, 'keypoints'), (got['smpl_2dkps'], want_sk, keep_sk, 'smpl_2dkps')):
        _ulp_equal(g[..., 2], wnt[..., 2], what + ' confidence')
        _ulp_equal(g[..., :2][keep], wnt[..., :2][keep], what)
    zero = got['smpl_2dkps'][..., 2] == 0
    assert zero.any() and (got['smpl_2dkps'][zero] == 0).all()                       # rows of confidence 0 are zeroed
    _ulp_equal(got['pose_3d'], want_S, 'pose_3d')
    _ulp_equal(got['pose'], want_pose, 'pose')
    # only what was asked for is computed
    assert set(ops.label_augment(_t(np.stack([rot, flip.astype(np.float64)], 1)), pose=_t(pose))) == {'pose'}
    with pytest.raises(ValueError):
        ops.label_augment(_t(np.stack([rot, flip.astype(np.float64)], 1)), keypoints=_t(kp))
    with pytest.raises(RuntimeError, match='GPU only|no CPU'):
        ops.label_augment(torch.zeros(B, 2, dtype=torch.float64), pose=_t(pose))


def test_label_augment_orientation_near_pi_as_rotations():
    """Rotated angles within 0.05 of pi, compared as rotation matrices at the bar of tests/test_gpu_eval.py's near-pi test: twice the
    distance of the numpy oracle in float32 from itself in float64 on the same matrices."""
    from danet_densepose2smpl_amd import ops
    rng = np.random.default_rng(11)
    B = 256
    rot = rng.uniform(-60, 60, B)
    rad = -rot * np.pi / 180
    Rz = np.zeros((B, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(rad), -np.sin(rad), np.sin(rad), np.cos(rad), 1
    ax = rng.normal(size=(B, 3))
    target = eo.rodrigues(ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.uniform(np.pi - 0.05, np.pi, (B, 1)))     # Rz R
    aa = eo.rotmat_to_angle_axis(np.einsum('bji,bjk->bik', Rz, target), np.float64)
    pose = np.concatenate([aa, rng.normal(0, 0.2, (B, 69))], 1)
    a64 = eo.rotmat_to_angle_axis(target, np.float64)
    a32 = eo.rotmat_to_angle_axis(target.astype(np.float32), np.float32)
    oracle_err = float(np.abs(eo.rodrigues(a32) - eo.rodrigues(a64)).max())
    got = ops.label_augment(_t(np.stack([rot, np.zeros(B)], 1)), pose=_t(pose))['pose'].cpu().numpy()
    dev_err = float(np.abs(eo.rodrigues(got[:, :3]) - eo.rodrigues(a64)).max())
    print('label_augment near pi: oracle fp32 vs fp64', oracle_err, 'device vs fp64', dev_err)
    record('label_augment_near_pi', {'oracle_fp32_vs_fp64': oracle_err, 'device_vs_fp64': dev_err})
    assert np.linalg.norm(got[:, :3].astype(np.float64), axis=1).max() <= np.pi * (1 + 2.0 ** -22)
    assert dev_err <= 2 * oracle_err, (dev_err, oracle_err)
    np.testing.assert_array_equal(got[:, 3:], pose[:, 3:].astype(np.float32))


# ---- FitsDict --------------------------------------------------------------------------------------------------------------------
def test_fits_dict_fetch_update_and_untouched_rows(tmp_path):
    from danet_densepose2smpl_amd import augment, datasets
    from danet_densepose2smpl_amd.fits_dict import FitsDict

    class O(object):
        train_data, checkpoint_dir = 'h36m_dp', str(tmp_path / 'ck')
    ds, paths = datasets.synthetic_mixed_dataset(O, str(tmp_path), 5, 6, seed=4)
    fd = FitsDict(O, ds, paths['final_fits_dir'], paths['static_fits_dir'], DEV)
    names = ['h36m', 'dp_coco', 'dp_coco', 'h36m', 'dp_coco', 'h36m', 'h36m']
    ind = torch.tensor([4, 0, 5, 1, 2, 0, 3])
    rot = torch.tensor([0., 30., -47.5, 12., 0., -25., 55.])
    flip = torch.tensor([0, 1, 0, 1, 1, 0, 1])
    stored = {n: FitsDict.read(n, paths['final_fits_dir'], paths['static_fits_dir']) for n in ('h36m', 'dp_coco')}
    rows = np.stack([stored[n][0][int(i)] for n, i in zip(names, ind)])
    before = fd.table.clone()
    pose, betas = fd[(names, ind.to(DEV), rot.to(DEV), flip.to(DEV))]
    assert pose.is_cuda and pose.shape == (7, 72) and betas.shape == (7, 10)
    want = augment.pose_processing(torch.from_numpy(rows[:, :72]), rot.double(), flip).numpy()
    _ulp_equal(pose.cpu().numpy(), want, 'fits pose')
    np.testing.assert_array_equal(betas.cpu().numpy(), rows[:, 72:])
    assert torch.equal(fd.table, before)
    valid = fd.get_vaild_state(names, ind).cpu().numpy()
    np.testing.assert_array_equal(valid, [stored[n][1][int(i)] for n, i in zip(names, ind)])
    # writing back what was fetched restores the rows; rows with update = False keep what they had, whatever is offered
    update = torch.tensor([1, 1, 0, 1, 0, 1, 1])
    offered = pose.clone()
    offered[update == 0] += 0.1
    fd[(names, ind, rot, flip, update)] = (offered, betas + (update == 0).float().view(-1, 1).to(DEV))
    after = fd.table.cpu().numpy()
    gi = fd.rows(names, ind).cpu().numpy()
    b = before.cpu().numpy()
    np.testing.assert_array_equal(after[gi[update.numpy() == 0]], b[gi[update.numpy() == 0]])
    others = np.setdiff1d(np.arange(len(b)), gi)
    np.testing.assert_array_equal(after[others], b[others])
    up = gi[update.numpy() == 1]
    np.testing.assert_array_equal(after[up, 72:], b[up, 72:])                                # betas exactly
    Ra, Rb = eo.rodrigues(after[up, :72].reshape(-1, 3).astype(np.float64)), eo.rodrigues(b[up, :72].reshape(-1, 3).astype(np.float64))
    err = float(np.abs(Ra - Rb).max())
    print('fits round trip, as rotations:', err)
    assert err <= 1e-5, err
