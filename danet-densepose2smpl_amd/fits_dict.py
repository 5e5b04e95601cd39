"""The pseudo-label store of the reference's train/fits_dict.py on the device: per-dataset tables [N,82] (72 pose, 10 betas) and
valid-fit flags live in HBM as ONE table; a fetch is one gather and one launch of the label op (csrc/input_ops.hip), an update one
launch and one scatter.  Nothing of a fetch or an update passes through the host."""
import os

import numpy as np
import torch

from . import ops
from ._lib import GPU_ONLY


class FitsDict(object):
    """FitsDict(options, train_dataset, final_fits_dir, static_fits_dir, device).  File rules of fits_dict.py:23-43: for every dataset
    of train_dataset.dataset_dict, <final_fits_dir>/<ds>.npy for 'h36m' (ground truth: every fit valid), <ds>.npz with pose, betas,
    valid_fit otherwise; if that file is missing <static_fits_dir>/<ds>_fits.npy (no fit of it counts as valid).  save() writes
    <options.checkpoint_dir>/<ds>_fits.npy.  A run that refreshes the table (fit_loop.InLoopFit, options.run_smplify) keeps it with
    its valid flags through save_state / load_state."""

    def __init__(self, options, train_dataset, final_fits_dir, static_fits_dir, device):
        self.options, self.train_dataset, self.device = options, train_dataset, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(GPU_ONLY % ('FitsDict device', self.device))
        tables, valid, self.base, self.length = [], [], {}, {}
        at = 0
        for ds_name in train_dataset.dataset_dict:
            t, v = self.read(ds_name, final_fits_dir, static_fits_dir)
            self.base[ds_name], self.length[ds_name] = at, t.shape[0]
            at += t.shape[0]
            tables.append(t)
            valid.append(v)
        self.table = torch.from_numpy(np.concatenate(tables)).to(self.device)
        self.valid = torch.from_numpy(np.concatenate(valid)).to(self.device)

    @staticmethod
    def read(ds_name, final_fits_dir, static_fits_dir):
        """-> (float32 [N,82], uint8 [N])."""
        try:
            if ds_name == 'h36m':
                t = np.load(os.path.join(final_fits_dir, ds_name + '.npy'))
                v = np.ones(len(t), np.uint8)
            else:
                f = np.load(os.path.join(final_fits_dir, ds_name + '.npz'))
                t = np.concatenate([f['pose'], f['betas']], axis=1)
                v = np.asarray(f['valid_fit']).astype(np.uint8)
        except IOError:
            t = np.load(os.path.join(static_fits_dir, ds_name + '_fits.npy'))
            v = np.zeros(len(t), np.uint8)
        t = np.ascontiguousarray(t, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != 82 or v.shape != (t.shape[0],):
            raise ValueError('fits of %r: expected [N,82] parameters and [N] flags, got %s and %s' % (ds_name, t.shape, v.shape))
        return t, v

    @property
    def fits_dict(self):
        """{dataset: its [N,82] rows} (views of the one table)."""
        return {n: self.table[b:b + self.length[n]] for n, b in self.base.items()}

    @property
    def valid_fit_state(self):
        return {n: self.valid[b:b + self.length[n]] for n, b in self.base.items()}

    def save(self):
        os.makedirs(self.options.checkpoint_dir, exist_ok=True)
        for ds_name, rows in self.fits_dict.items():
            np.save(os.path.join(self.options.checkpoint_dir, ds_name + '_fits.npy'), rows.cpu().numpy())

    def save_state(self, directory):
        """The table AND its valid flags, for a run that refreshes them (DESIGN.md 4d "the refresh rule"): <directory>/<ds>_fits.npy
        as save() writes it, plus <ds>_valid_fit.npy (uint8 [N]).  Each call overwrites the last: only the newest state is kept."""
        os.makedirs(directory, exist_ok=True)
        flags = self.valid_fit_state
        for ds_name, rows in self.fits_dict.items():
            np.save(os.path.join(directory, ds_name + '_fits.npy'), rows.cpu().numpy())
            np.save(os.path.join(directory, ds_name + '_valid_fit.npy'), flags[ds_name].cpu().numpy())

    def load_state(self, directory):
        """What save_state wrote, back into the table in place: a dataset is read where BOTH its files exist (the others keep what
        the constructor read), a file of another shape raises ValueError before anything is changed.  -> the names read."""
        found = {}
        for ds_name, n in self.length.items():
            ft, fv = (os.path.join(directory, ds_name + s) for s in ('_fits.npy', '_valid_fit.npy'))
            if not (os.path.isfile(ft) and os.path.isfile(fv)):
                continue
            t, v = np.load(ft), np.load(fv)
            if t.shape != (n, 82) or v.shape != (n,):
                raise ValueError('fits state of %r in %s: expected [%d,82] parameters and [%d] flags, got %s and %s'
                                 % (ds_name, directory, n, n, t.shape, v.shape))
            found[ds_name] = (np.ascontiguousarray(t, dtype=np.float32), np.ascontiguousarray(v).astype(np.uint8))
        for ds_name, (t, v) in found.items():
            b = self.base[ds_name]
            self.table[b:b + t.shape[0]].copy_(torch.from_numpy(t))
            self.valid[b:b + v.shape[0]].copy_(torch.from_numpy(v))
        return sorted(found)

    def rows(self, dataset_name, ind):
        """Row numbers in the one table (device int64 [B]); the dataset names are host strings, the indices may be on either side."""
        base = torch.as_tensor(np.array([self.base[n] for n in dataset_name], np.int64)).to(self.device, non_blocking=True)
        return base + torch.as_tensor(ind).to(self.device, non_blocking=True).long().reshape(-1)

    def _rot_flip(self, rot, is_flipped):
        rot, flip = torch.as_tensor(rot).to(self.device), torch.as_tensor(is_flipped).to(self.device)
        return torch.stack([rot.double().reshape(-1), flip.double().reshape(-1)], dim=1).contiguous()

    def __getitem__(self, x):
        """(dataset_name, ind, rot, is_flipped) -> (pose [B,72], betas [B,10]) on the device:
        flip_pose(rotate_pose(stored pose, rot), is_flipped)."""
        dataset_name, ind, rot, is_flipped = x
        out = ops.label_augment(self._rot_flip(rot, is_flipped), fits=self.table.index_select(0, self.rows(dataset_name, ind)))
        return out['fits_pose'], out['fits_betas']

    def get_vaild_state(self, dataset_name, ind):
        return self.valid.index_select(0, self.rows(dataset_name, ind))

    def __setitem__(self, x, val):
        """(dataset_name, ind, rot, is_flipped, update), (pose, betas): rows with update[n] take
        rotate_pose(flip_pose(pose, is_flipped), -rot) and betas; the others stay."""
        dataset_name, ind, rot, is_flipped, update = x
        pose, betas = val
        rows = self.rows(dataset_name, ind)
        new = torch.cat([pose.to(self.device).float(), betas.to(self.device).float()], dim=1).contiguous()
        out = ops.label_augment(self._rot_flip(rot, is_flipped), fits=new, inverse=True)
        new = torch.cat([out['fits_pose'], out['fits_betas']], dim=1)
        keep = torch.as_tensor(update).to(self.device).reshape(-1, 1) > 0
        self.table.index_copy_(0, rows, torch.where(keep, new, self.table.index_select(0, rows)))
