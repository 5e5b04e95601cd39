"""What the training step's input prologue costs on the device: B = 32 crops of 256 x 256 from 32 source images of about 1000 x 1000,
with rotation, flip and pixel noise, plus the label transforms.

  new   datasets.collate (footprint rectangles, one label block) + datasets.to_device (pinned upload, ops.batch_crop, ops.label_augment)
  old   evaluate.collate-style zero-padded uint8 batch, uploaded whole and expanded to float, augment.rgb_processing + the three
        augment.*_processing label transforms as torch ops on the device

One process, after warm-up, median of 50, HIP events around the device work (upload + kernels); the host-side collation is timed with
the wall clock beside it.  Last line: one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    import torch
    from danet_densepose2smpl_amd import augment, datasets, dp_utils
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    B, res, reps, warm = 32, 256, 50, 5
    items = []
    for b in range(B):
        H, W = int(rng.integers(900, 1100)), int(rng.integers(900, 1100))
        flip, pn, rot, sc = augment.augm_params(1, True, rng=rng)
        items.append({'img_raw': rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 'dp_dict': dp_utils.empty_dp_dict(56), 'imgname': '',
                      'pose': rng.normal(0, 0.2, 72), 'betas': rng.normal(0, 1, 10).astype(np.float32), 'smpl_2dkps': rng.uniform(0, 900, (24, 3)),
                      'pose_3d': rng.normal(0, 0.3, (24, 4)), 'keypoints': rng.uniform(0, 900, (49, 3)), 'has_dp': 0., 'has_smpl': 1., 'has_pose_3d': 1,
                      'scale': float(sc[0] * rng.uniform(1.5, 3.5)), 'center': np.zeros(2, np.float32), '_center': np.array([W / 2., H / 2.]) + rng.uniform(-80, 80, 2),
                      'orig_shape': np.array([H, W]), 'is_flipped': int(flip[0]), 'rot_angle': np.float32(rot[0]), '_rot': float(rot[0] if b % 2 else 17.5),
                      'pn': pn[0], 'gender': -1, 'sample_index': b, 'dataset_name': 'h36m'})
    col = lambda k: np.stack([np.asarray(it[k], np.float64) for it in items])           # noqa: E731

    def new_host():
        return datasets.collate(items, res)

    def new_dev(batch):
        return datasets.to_device(batch, dev, res)

    def old_host():
        H, W = max(it['img_raw'].shape[0] for it in items), max(it['img_raw'].shape[1] for it in items)
        raw = np.zeros((B, H, W, 3), np.uint8)
        for b, it in enumerate(items):
            raw[b, :it['img_raw'].shape[0], :it['img_raw'].shape[1]] = it['img_raw']
        return {'img_raw': raw, **{k: col(k) for k in ('_center', 'scale', '_rot', 'is_flipped', 'pn', 'keypoints', 'smpl_2dkps', 'pose_3d', 'pose')}}

    def old_dev(h):
        t = {k: torch.from_numpy(v).to(dev, non_blocking=True) for k, v in h.items()}
        raw = t['img_raw'].permute(0, 3, 1, 2).float()
        c, s, r, f = t['_center'], t['scale'], t['_rot'], t['is_flipped']
        img = augment.rgb_processing(raw, c, s, r, f, t['pn'], res=res).float().contiguous()
        kp = augment.j2d_processing(t['keypoints'], c, s, r, f, res)
        sk = augment.j2d_processing(t['smpl_2dkps'], c, s, r, torch.zeros_like(f), res)
        return img, kp, sk, augment.j3d_processing(t['pose_3d'], r, f), augment.pose_processing(t['pose'], r, f)

    out = {'B': B, 'res': res, 'reps': reps}
    for name, host, devf in (('new', new_host, new_dev), ('old', old_host, old_dev)):
        t_host, t_dev = [], []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            h = host()
            t1 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            devf(h)
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                t_host.append((t1 - t0) * 1e3)
                t_dev.append(a.elapsed_time(b))
        nbytes = sum(v.nbytes for v in h.values() if isinstance(v, np.ndarray))
        out[name] = {'device_ms_median': float(np.median(t_dev)), 'device_ms_min': float(np.min(t_dev)), 'host_collate_ms_median': float(np.median(t_host)),
                     'uploaded_bytes': int(nbytes)}
        print(name, out[name], flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
