"""Training step with the contract of the reference's Trainer.train_step
(/root/reference/train/trainer.py:117-244): ``train_step(in_dict) -> (output, losses)`` =
forward, sum of the loss dict (trainer.py:217-220), backward, Adam step (lr 1e-4, trainer.py:42-44).
The in_dict is the one the reference builds at trainer.py:184-212; `synthetic_in_dict` produces it
from seeded random labels.  `Trainer.fit` is the loop of base_trainer.py:53-106 over
datasets.py / fits_dict.py; TensorBoard's image summaries are PNG sheets here (Trainer.visualize, train_vis.py), its event files are out of scope."""
import types

import numpy as np
import contextlib
import os

import torch

from . import ops
from .config import cfg
from .danet import DaNet
from .distributed import GradStore
from .nn import SideBranch
from . import conv as _conv, hrnet, nn as _nn, segments
from .geometry import perspective_projection, label_prologue


DEFER_WGRAD = bool(int(os.environ.get('DANET_DEFER_WGRAD', '1')))
USE_FUSED_ADAM = bool(int(os.environ.get('DANET_FUSED_ADAM', '1')))
# Data-parallel steps run the backward pass in segments (segments.py) and release complete gradient buckets between them:
# all-reduces overlap the backward pass proper, issued by this thread in program order (eager and captured alike).
# DANET_SEGMENTS=0 switches the cuts off (every bucket after the backward pass: round 2's order); DANET_SEGMENTS=1 forces them
# on in a single-process trainer (tests, A/B timing).
SEGMENTS = os.environ.get('DANET_SEGMENTS', '')
# Experiment knob (round 5, OFF): one process launches the queued weight gradients of a finished backward segment on a SIDE stream while
# the next segment's data-gradient / BatchNorm chain continues on the step's stream -- the chain's kernels are latency-bound and leave
# most of the chip idle, the weight gradients need nothing from it.  Measured on MI355X inside the captured step (bench.py, one gpurun
# call): 27.9 ms without; with it 1 842 ms -- the one-pass BatchNorm backward's grid barrier needs all its workgroups resident at once
# and a chip-filling weight-gradient kernel beside it makes the barrier run into its spin bound --; with the two-kernel
# BatchNorm backward instead 28.86 ms against 28.47 without overlap, and 57 ms with the step's stream at high priority.  Graph
# branches do not buy concurrency on this stack: the step stays one stream.
WGRAD_OVERLAP = bool(int(os.environ.get('DANET_WGRAD_OVERLAP', '0')))
# Compute units the communication library may occupy while the backward pass runs (one workgroup per channel): the one-pass
# BatchNorm backward's grid barrier is sized to fit beside them (nn.ONEPASS_MAX_BLOCKS).  The limit is the LAUNCHER's to set --
# NCCL_MAX_NCHANNELS must be in the environment before the first collective creates the communicator: bench.py calls
# reserve_comm_channels() before init_process_group.  A Trainer never touches the environment: it reads the limit,
# and without one it does not know how many compute units the all-reduce kernels may take, so its data-parallel steps run the
# two-kernel BatchNorm backward (a warning says so).  Trade-off: 24 channels leave the all-reduce 24 of 256 compute units;
# DANET_COMM_CHANNELS chooses another number (tools/scale_sweep.sh sweeps it), NCCL_MAX_NCHANNELS set by hand wins.
COMM_CHANNELS = int(os.environ.get('DANET_COMM_CHANNELS', '24'))
# Buckets that complete together are flushed / copied / all-reduced as ONE run (GradStore.release_ready_group); 0: one bucket at a time (A-B)
GROUP_RELEASE = bool(int(os.environ.get('DANET_GROUP_RELEASE', '1')))


def reserve_comm_channels():
    """For LAUNCH scripts, before torch.distributed.init_process_group: export the channel limit (if none is set) and return the
    number of compute units kept free for collectives."""
    cur = os.environ.get('NCCL_MAX_NCHANNELS')
    if cur is None:
        os.environ['NCCL_MAX_NCHANNELS'] = str(COMM_CHANNELS)
        return COMM_CHANNELS
    return max(1, int(cur))


def comm_channel_limit():
    """The channel limit the environment names (what the communicator was, or will be, created with), or None."""
    cur = os.environ.get('NCCL_MAX_NCHANNELS')
    return None if cur is None else max(1, int(cur))


def default_options(batch_size=32):
    return types.SimpleNamespace(batch_size=batch_size, openpose_train_weight=0., gt_train_weight=1.)


def synthetic_in_dict(model, B, device, seed=1234, img_size=None, with_dp=False):
    """Seeded synthetic training batch with the reference's keys and shapes (trainer.py:184-212;
    datasets/base_dataset.py:228-298)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    S = img_size or cfg.DANET.INIMG_SIZE
    img = torch.randn(B, 3, S, S, generator=g).to(device)
    betas = torch.randn(B, 10, generator=g).clamp(-3, 3).to(device)
    pose = (torch.randn(B, 72, generator=g) * 0.2).to(device)
    cam = torch.stack([torch.rand(B, generator=g) * 0.5 + 0.6, torch.rand(B, generator=g) * 0.2 - 0.1,
                       torch.rand(B, generator=g) * 0.2 - 0.1], dim=1).to(device)
    smpl = model.iuv2smpl.smpl
    with torch.no_grad():
        out = smpl(betas=betas, body_pose=pose[:, 3:], global_orient=pose[:, :3])
        cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * 5000. / (S * cam[:, 0] + 1e-9)], dim=-1)
        zero_c = torch.zeros(B, 2, device=device)
        kp2d = perspective_projection(out.joints, None, cam_t, 5000., zero_c) / (S / 2.)
        conf = torch.cat([torch.zeros(B, 25, 1, device=device), torch.ones(B, 24, 1, device=device)], dim=1)
        keypoints = torch.cat([kp2d, conf], dim=-1)
        pose_3d = torch.cat([out.joints[:, 25:], torch.ones(B, 24, 1, device=device)], dim=-1)
        skps = perspective_projection(out.smpl_joints, None, cam_t, 5000., zero_c) / (S / 2.)
        target_smpl_kps = torch.cat([skps, torch.ones(B, 24, 1, device=device)], dim=-1)
    ones = torch.ones(B, device=device)
    extra = {}
    if with_dp:
        # the zero DensePose blobs every non-COCO sample carries (datasets/base_dataset.py:228-237); 'dp_active' is the
        # host-side twin of the reference's `torch.sum(has_dp) > 0` test
        Sh = S // 4
        z = lambda n: torch.zeros(B, n, device=device)      # noqa: E731
        extra['dp_dict'] = {'body_uv_ann_labels': torch.zeros(B, Sh * Sh, dtype=torch.int32, device=device),
                            'body_uv_ann_weights': z(Sh * Sh), 'body_uv_X_points': z(196), 'body_uv_Y_points': z(196),
                            'body_uv_Ind_points': z(196), 'body_uv_I_points': z(196), 'body_uv_U_points': z(4900),
                            'body_uv_V_points': z(4900), 'body_uv_point_weights': z(4900), 'dp_active': False}
    return {**extra, 'img': img, 'opt_pose': pose, 'opt_betas': betas, 'keypoints': keypoints, 'pose_3d': pose_3d,
            'has_pose_3d': ones.clone(), 'valid_fit': ones.clone(), 'has_iuv': ones.clone(), 'has_dp': torch.zeros(B, device=device),
            'target_smpl_kps': target_smpl_kps, 'target_verts': out.vertices.detach(), 'target_cam': cam,
            'vis_on': False, 'pretrain_mode': False}


class Trainer(object):
    """Single-process-per-GPU trainer.  Gradients live in one flat store (distributed.GradStore); with world_size > 1
    its buckets are all-reduced (RCCL) while the rest of the backward pass and the remaining weight gradients of the step
    are still being computed (segments.py)."""

    def __init__(self, options=None, model=None, device=None, lr=None, distributed=None, smpl_model=None, bucket_mb=None, grad_wire=None):
        self.options = options or default_options()
        self.device = device or torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        self.model = (model or DaNet(self.options, None, pretrained=False, smpl_model=smpl_model)).to(self.device)
        self.smpl = self.model.iuv2smpl.smpl
        on_gpu = self.device.type == 'cuda'
        lr0 = lr or cfg.SOLVER.BASE_LR
        if distributed is None:
            distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size() > 1
        self.distributed = bool(distributed)
        # a tensor learning rate keeps the manual step decay (trainer.py:120-128) effective under hipGraph replay
        params = [p for p in self.model.parameters() if p.requires_grad]
        self.params = params
        self.store = None
        if on_gpu and USE_FUSED_ADAM:
            from .optim import FusedAdam
            if bucket_mb is None:
                bucket_mb = float(os.environ.get('DANET_BUCKET_MB', '32'))
            wire = torch.bfloat16 if (grad_wire or os.environ.get('DANET_GRAD_WIRE', 'fp32')) == 'bf16' else torch.float32
            self.store = GradStore(params, bucket_mb=bucket_mb, device=self.device,
                                   world=torch.distributed.get_world_size() if self.distributed else 1,
                                   wire_dtype=wire if self.distributed else torch.float32)
            self.optimizer = FusedAdam(params, lr=lr0, grad_store=self.store)      # one HIP launch per step (csrc/adam.hip)
        else:
            if self.distributed:
                raise RuntimeError('data-parallel training needs the GPU path (FusedAdam + GradStore)')
            self.optimizer = torch.optim.Adam(params=params, lr=torch.tensor(lr0, device=self.device) if on_gpu else lr0,
                                              weight_decay=0, **({'capturable': True, 'fused': True} if on_gpu else {}))
        self.step_count = 0
        self.bank = None
        # Every step (eager or captured) runs on ONE dedicated stream: autograd pins each parameter's
        # gradient-accumulation node to the stream it was created on, and a node created on the default
        # stream would pull that (non-capturing) stream into a later hipGraph capture.
        self.stream = torch.cuda.Stream(device=self.device, priority=int(os.environ.get('DANET_MAIN_PRIORITY', '0'))) if on_gpu else None
        self.wgrad_stream = torch.cuda.Stream(device=self.device, priority=int(os.environ.get('DANET_WGRAD_PRIORITY', '0'))) if on_gpu else None
        self._held = []
        self.onepass_blocks = 0
        self.segmented = (self.distributed and SEGMENTS != '0') or SEGMENTS == '1'
        if on_gpu:
            _conv.ARENA.enable(self.device)
            _nn.confine_onepass(self.stream)        # the one-pass BatchNorm backward is confined to the step's own stream
            if isinstance(self.optimizer, torch.optim.Optimizer) is False:
                # a step whose one-pass BatchNorm backward timed out at its grid barrier is skipped by the Adam kernel itself
                self.optimizer.poison = _nn.onepass_poison(self.device)
                if self.distributed:
                    # ... and, since its gradients are in every rank's sums by then, by every other rank's as well: the word travels
                    # with the last gradient bucket (GradStore.stamp_poison) and the kernel tests the all-reduced sum
                    self.store.poison_src = self.optimizer.poison
                    self.optimizer.poison_sum = self.store.poison
            # workgroup budget of the one-pass BatchNorm backward in THIS trainer's steps (installed by _core for the duration of a
            # step): 0 = the whole device; data-parallel: all-reduce kernels of earlier buckets run beside the backward pass, so the grid
            # barrier must fit next to them -- 2 * (compute units - channel limit); -1 = no limit known: two-kernel path
            if os.environ.get('DANET_ONEPASS_BLOCKS'):            # experiment knob: an explicit budget
                self.onepass_blocks = int(os.environ['DANET_ONEPASS_BLOCKS'])
            elif self.distributed:
                ch = comm_channel_limit()
                if ch is None:
                    import warnings
                    warnings.warn('data-parallel Trainer without NCCL_MAX_NCHANNELS in the environment: the number of compute units the '
                                  'all-reduce kernels may occupy is unknown, so the one-pass BatchNorm backward (a grid barrier over 2 workgroups '
                                  'per compute unit) is off for this trainer; call trainer.reserve_comm_channels() before init_process_group')
                    self.onepass_blocks = -1
                else:
                    cus = torch.cuda.get_device_properties(self.device).multi_processor_count
                    self.onepass_blocks = max(2, 2 * (cus - ch))
        self._graph = None
        self._static = None
        self._reduce_in_graph = True
        if self.distributed:
            self.store.broadcast_parameters(self.model)

    @property
    def reducer(self):          # (name kept for callers of the first version)
        return self.store if self.distributed else None

    @torch.no_grad()
    def prepare_batch(self, input_batch, opt_pose=None, opt_betas=None, img_res=None, focal_length=5000.):
        """The reference's step prologue (train/trainer.py:134-212) on the device -- SURVEY.md 8 row f1.
        input_batch: img, keypoints [B,49,3] (normalised to [-1,1], confidence), pose [B,72], betas [B,10], pose_3d [B,24,4],
        has_smpl, has_pose_3d, has_dp, optional smpl_2dkps / dp_dict / has_iuv_dataset (the reference's
        `dataset_name != 'dp_coco'`) / valid_fit.  opt_pose / opt_betas: the pseudo-label fits (FitsDict in the
        reference; default: the ground truth).  Two SMPL forwards (HIP), one batched least-squares solve, no host
        round trip.  Returns the in_dict `train_step` takes."""
        dev = self.device
        res = img_res or cfg.DANET.INIMG_SIZE
        B = input_batch['img'].shape[0]
        gt_pose, gt_betas = input_batch['pose'].to(dev), input_batch['betas'].to(dev)
        has_smpl = input_batch['has_smpl'].to(dev) > 0
        opt_pose = gt_pose.clone() if opt_pose is None else opt_pose.to(dev).clone()
        opt_betas = gt_betas.clone() if opt_betas is None else opt_betas.to(dev).clone()
        opt_betas = torch.where((opt_betas.abs() > 3).any(dim=-1, keepdim=True), torch.zeros_like(opt_betas), opt_betas)
        opt_pose = torch.where(has_smpl.view(B, 1), gt_pose, opt_pose)
        opt_betas = torch.where(has_smpl.view(B, 1), gt_betas, opt_betas)
        opt = self.smpl(betas=opt_betas, body_pose=opt_pose[:, 3:], global_orient=opt_pose[:, :3])
        valid_fit = input_batch['valid_fit'].to(dev) > 0 if 'valid_fit' in input_batch else has_smpl
        has_iuv = valid_fit & (input_batch['has_iuv_dataset'].to(dev) > 0 if 'has_iuv_dataset' in input_batch
                               else torch.ones(B, dtype=torch.bool, device=dev))
        has_dp = input_batch.get('has_dp', torch.zeros(B, device=dev)).to(dev)
        kps, cam, _ = label_prologue(opt.joints, opt.smpl_joints, input_batch['keypoints'].to(dev), has_iuv, has_dp,
                                     input_batch.get('smpl_2dkps', None) if input_batch.get('smpl_2dkps', None) is None
                                     else input_batch['smpl_2dkps'].to(dev), focal_length, res)
        out = {'img': input_batch['img'].to(dev), 'opt_pose': opt_pose, 'opt_betas': opt_betas,
               'keypoints': input_batch['keypoints'].to(dev), 'pose_3d': input_batch['pose_3d'].to(dev),
               'has_pose_3d': input_batch['has_pose_3d'].to(dev).float(), 'valid_fit': valid_fit.float(),
               'has_iuv': has_iuv.float(), 'has_dp': has_dp.float(), 'target_smpl_kps': kps,
               'target_verts': opt.vertices.detach(), 'target_cam': cam,
               'vis_on': bool(input_batch.get('vis_on', False)), 'pretrain_mode': bool(input_batch.get('pretrain_mode', False))}
        if 'dp_dict' in input_batch:
            out['dp_dict'] = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in input_batch['dp_dict'].items()}
            out['dp_dict'].setdefault('dp_active', bool((has_dp > 0).any()))        # (one host read per batch, outside the step)
        return out

    ONEPASS_CHECK_EVERY = 64       # steps between looks at the one-pass BatchNorm's barrier error flag (one 4-byte read each)

    def check_onepass(self):
        """The one-pass BatchNorm backward (csrc/norm_act.hip) spins at a grid-wide barrier with a bound; a time-out -- a GPU
        shared with another process, a partitioned device -- leaves garbage gradients and a stale barrier.  The Adam kernel
        reads the barrier's error word and skips such a step on the device (csrc/adam.hip `poison`), so nothing is ever
        applied; this host-side check (every ONEPASS_CHECK_EVERY steps and before a checkpoint is written) is for reporting and
        recovery: the barrier is reset, the one-pass path switched off (two-kernel BatchNorm backward from here on), a
        captured graph dropped, and the caller told.  Data-parallel: the decision is taken from the all-reduced poison word
        (GradStore.poison: the error word is sticky, so the last step's sum tells whether ANY rank has timed out since the last
        check) -- every rank recovers and raises in the same call, none is left waiting in a collective."""
        if self.device.type != 'cuda':
            return
        elsewhere = bool(self.distributed and self.store is not None and self.store.poison_src is not None and float(self.store.poison) > 0)
        if _nn.onepass_recover(self.device, force=elsewhere):
            self._graph = None
            guarded = getattr(self.optimizer, 'poison', None) is not None
            raise RuntimeError('a one-pass BatchNorm launch timed out at its grid barrier' + (' on some rank' if elsewhere else '') +
                               ': gradients since then are invalid'
                               + (' -- the optimizer skipped those steps on every rank (device-side guard on the all-reduced error word), '
                                  'parameters and moments are intact. '
                                  if guarded else ' and were applied: resume from the last checkpoint. ') +
                               'The barrier was reset and the one-pass path switched off (nn.ONEPASS = False); capture() again if you '
                               'replay a graph')

    def save(self, path, epoch=0, batch_idx=0, batch_size=0, dataset_perm=None):
        """A training checkpoint in the reference's format (utils/saver.py:24-50): model, optimizer, bookkeeping with
        `total_step_count` = this trainer's step count."""
        from . import checkpoint
        self.check_onepass()
        return checkpoint.save_checkpoint(path, {'model': self.model}, {'optimizer': self.optimizer}, epoch=epoch, batch_idx=batch_idx,
                                          batch_size=batch_size, dataset_perm=dataset_perm, total_step_count=self.step_count)

    def resume(self, path, trusted=False):
        """Continue from a checkpoint (base_trainer.py:37-51): parameters, BatchNorm buffers, Adam moments and learning rate
        come from the file, and `step_count` -- which drives the step-LR decay -- from its `total_step_count`.  Works
        with a captured graph too: the tensors are updated in place and the weight repack is part of the graph.
        Returns the bookkeeping values (epoch, batch_idx, ...)."""
        from . import checkpoint
        book = checkpoint.load_checkpoint(path, {'model': self.model}, {'optimizer': self.optimizer},
                                          map_location=self.device, trusted=trusted)
        self.step_count = int(book.get('total_step_count') or 0)
        _conv._PACK_CACHE.clear()
        return book

    def _decay_lr(self):
        """manual step-LR decay (trainer.py:120-128)"""
        for i, s in enumerate(cfg.SOLVER.STEPS):
            if i > 0 and self.step_count == s:
                for group in self.optimizer.param_groups:
                    if torch.is_tensor(group['lr']):
                        group['lr'].mul_(cfg.SOLVER.GAMMA)
                    else:
                        group['lr'] *= cfg.SOLVER.GAMMA

    def _begin_step(self):
        """Per-step device housekeeping: zero the accumulator arena, repack all conv weights (one launch).
        The first GPU step records which packed weights the model asks for and builds the bank."""
        _conv.ARENA.begin_step()
        if self.device.type == 'cuda' and not os.environ.get('DANET_NO_BANK'):
            if self.bank is None:
                self.bank = _conv.WeightBank()
                self.bank.start_recording()
            elif self.bank.requests is not None:
                self.bank.build()
            self.bank.refresh()

    def _forget_bank(self):
        """The next step records and builds the weight bank anew (a phase that runs other modules)."""
        if self.bank is not None:
            self.bank.stop_recording()
        self.bank = None

    def _abandon_step(self):
        """What a step that was given up (a late gradient, a failed graph capture) leaves behind for the rerun: queued weight-gradient
        jobs that point at its tensors, pending collectives, gradients that point into an aborted pool.  (The step globals are put
        back by their scopes; the arena cursor and the weight bank are re-armed by the next step's _begin_step.)"""
        _conv.drop_wgrads()
        if self.store is not None:
            self.store.forget_pending()
        self.optimizer.zero_grad(set_to_none=True)

    @contextlib.contextmanager
    def _on_stream(self):
        side = SideBranch(self.stream)                  # (None on the CPU: everything stays where it is)
        with side.fork():
            yield
        side.join()

    def _core(self, batch, reduce=True, with_optimizer=True):
        """One optimisation step on the current stream: forward; backward with the weight gradients queued -- in segments
        when data-parallel (segments.py), releasing every complete gradient bucket between two segments: the bucket's
        weight-gradient launches, its small gradients copied into the store, its all-reduce (asynchronous, on the
        communication stream: the next segment's backward kernels overlap it); then the remaining buckets the same way; Adam
        waits for the last all-reduce.  Every global of another module that the step switches is held by that module's scope."""
        st = self.store
        reduce_now = bool(self.distributed and reduce)
        overlap = bool(WGRAD_OVERLAP and DEFER_WGRAD and st is not None and not self.distributed and self.wgrad_stream is not None)
        with _nn.onepass_blocks(self.onepass_blocks):
            self._begin_step()
            if st is not None:
                st.begin_step()
            # (the store is named from the forward pass on, which does not ask for it: ONE scope for the backward pass and the tail
            # flush, around the segment registry's, which ends before the tail so that the cut tensors are gone by then)
            with _conv.grad_store(st):
                with segments.recording((self.segmented or overlap) and st is not None):
                    with _nn.deferred_batch_counts():
                        out = self.model(batch)
                    losses = out['losses']
                    self.optimizer.zero_grad(set_to_none=True)
                    if st is not None:
                        st.backward_scope(True, early=reduce_now)
                    try:
                        with _conv.deferred_wgrads(DEFER_WGRAD):
                            if segments.level() > 0:
                                segments.backward(losses, (lambda k: st.release_ready_group(self._release_buckets)) if reduce_now else
                                                  ((lambda k: self._flush_on_side_stream()) if overlap else None))
                            else:
                                # (every loss is a 1-element tensor, models/danet/danet.py:359-364: views + one cat + one sum)
                                torch.cat([v.reshape(-1) for v in losses.values()]).sum().backward()
                    finally:
                        # close the store's scope behind a backward pass that raised as well; it may raise itself, on a late gradient
                        if st is not None:
                            try:
                                st.backward_scope(False)
                                st.stamp_poison()
                            except RuntimeError:
                                self._abandon_step()
                                raise
                if reduce_now:
                    if st.next_bucket() < len(st.buckets):                   # what the backward pass did not release, as one run
                        self._release_buckets(st.next_bucket(), len(st.buckets))
                elif overlap:                                                # segment by segment on the side stream, which joins the step's here
                    self._flush_on_side_stream()
                    torch.cuda.current_stream(self.device).wait_stream(self.wgrad_stream)
                    del self._held[:]
                # one process: no all-reduce to overlap with, so all queued weight gradients go out in the fewest, largest
                # multi-problem launches (-0.15 ms against 13 bucket-sized flushes); data-parallel: nothing left, every parameter
                # belongs to a bucket
                _conv.flush_wgrads()
                if reduce_now:
                    st.wait()
                elif st is not None:
                    st.collect()
            if with_optimizer:
                self.optimizer.step()
        return out, losses

    def _flush_on_side_stream(self):
        """Launch everything queued so far (conv.flush_wgrads) on the weight-gradient stream, ordered after the work already on
        the step's stream; the operands stay referenced (self._held) until the streams join at the end of the backward pass."""
        cur = torch.cuda.current_stream(self.device)
        self.wgrad_stream.wait_stream(cur)
        with torch.cuda.stream(self.wgrad_stream):
            _conv.flush_wgrads(hold=self._held)

    def _release_buckets(self, b0, b1):
        """The consecutive complete gradient buckets b0 .. b1 - 1 (GradStore.release_ready_group between two backward segments, or the
        tail): their queued weight gradients are launched in one flush (fewer, larger multi-problem launches), their other gradients
        copied into the store by one multi-tensor copy, and one all-reduce started over their contiguous slice of the store.
        DANET_GROUP_RELEASE=0: the same, bucket by bucket."""
        if not GROUP_RELEASE and b1 - b0 > 1:
            for bi in range(b0, b1):
                self._release_buckets(bi, bi + 1)
            return
        st = self.store
        run = range(b0, b1)
        with _conv.grad_store(st):
            _conv.flush_wgrads(bucket=run)
        st.collect(run)
        st.reduce_buckets(b0, b1)

    def _end_step(self):
        self.step_count += 1
        if self.step_count % self.ONEPASS_CHECK_EVERY == 0:
            self.check_onepass()

    def train_step(self, in_dict):
        self.model.train()
        self._decay_lr()
        with self._on_stream():
            out, losses = self._core(in_dict)
        self._end_step()
        return out, losses

    # ------------------------------------------------------------------------------------------
    # hipGraph execution: the ~2.4k kernel launches of one step are captured once and replayed, which
    # removes the host-side launch cost (the step is launch-bound in eager mode).
    @staticmethod
    def _clone_batch(d):
        return {k: (v.clone() if torch.is_tensor(v) else Trainer._clone_batch(v) if isinstance(v, dict) else v) for k, v in d.items()}

    def capture(self, in_dict, warmup=2, dp_active=True):
        """Capture the whole step -- forward, backward, the bucketed gradient all-reduces (N > 1) and Adam -- for batches
        shaped like `in_dict`.  The host-side switches of a batch are frozen into the graph: `pretrain_mode` / `vis_on`
        must not change between replays (checked by load_batch), and DensePose point supervision is captured as ACTIVE
        whenever the batch carries a `dp_dict` (its losses are masked by `has_dp` per sample, so batches without
        DensePose labels simply contribute zeros) -- unless dp_active is False: a run whose datasets hold no DensePose labels
        captures the four zero losses and none of the work.  warmup: eager steps on `in_dict` before the capture (real optimizer
        steps; 0 when the caller has just run eager steps of this kind itself, as Trainer.fit does).  If the communication
        library cannot be captured the all-reduces and the optimizer run right after each replay instead."""
        if self.device.type != 'cuda':
            raise RuntimeError('hipGraph capture needs a GPU')
        self.model.train()
        self._static = self._clone_batch(in_dict)
        if isinstance(self._static.get('dp_dict'), dict):
            self._static['dp_dict']['dp_active'] = bool(dp_active)
        with self._on_stream():
            for _ in range(warmup):
                self._core(self._static)
        torch.cuda.synchronize(self.device)
        if self.store is not None:
            self.store.quiesce()                  # no collective of the eager steps may still be on the watchdog's list (see there)
        if self.store is not None:
            self.store.prepare_capture(attempts=2 if self.distributed else 1)
        modes = (True,)
        if self.distributed:
            # collectives inside the graph need a backend whose calls are stream work (RCCL); any other backend (gloo: host-side
            # reductions on its own threads) cannot be captured -- and a capture that FAILS half-way is not something to rely on
            # recovering from: round 5 tried it with gloo, the step's stream stayed in capture mode after the failed capture and the
            # second capture_begin raised.  So the choice is made up front; the retry below remains for an RCCL capture that raises.
            backend = torch.distributed.get_backend(self.store.group) if torch.distributed.is_initialized() else ''
            modes = (True, False) if 'nccl' in str(backend) else (False,)
        for in_graph in modes:
            _conv._PACK_CACHE.clear()             # weight packing must be part of the captured work
            self.optimizer.zero_grad(set_to_none=True)
            graph = torch.cuda.CUDAGraph()
            _conv.FUSION.clear()
            try:
                # thread_local: the communication library's watchdog thread may poll events of earlier collectives while
                # this thread captures (the default, global mode turns that into a capture error)
                with hrnet.branch_streams(int(os.environ.get('DANET_BRANCH_STREAMS', '1'))), \
                        torch.cuda.graph(graph, stream=self.stream, capture_error_mode='thread_local' if self.distributed else 'global'):
                    self._static_out = self._core(self._static, reduce=in_graph, with_optimizer=in_graph)
                self._reduce_in_graph = in_graph
                self.fusion_counts = dict(_conv.FUSION)     # which attribute-carried fusions the captured step contains
                # the collectives the capture recorded, in issue order, and how many of them from inside the backward pass
                self.captured_collectives = (list(self.store.issued), self.store.issued_early) if (self.store is not None and in_graph) else ([], 0)
                break
            except RuntimeError:
                if not (in_graph and self.distributed):      # (only a capture that holds collectives has a fallback: reduce after the replay)
                    raise
                self._end_stray_capture()
                torch.cuda.synchronize(self.device)
                self._abandon_step()
        self._graph = graph
        return self

    @staticmethod
    def _loaded_hip_runtime():
        """The libamdhip64 THIS process already runs on (the copy torch loaded), by the path the loader mapped it from: dlopen of
        that path returns the same handle, where a bare soname could resolve to another installation's runtime and act on nothing."""
        import ctypes
        try:
            for ln in open('/proc/self/maps'):
                path = ln.rsplit(None, 1)[-1]
                if 'libamdhip64.so' in os.path.basename(path):
                    return ctypes.CDLL(path)
        except OSError:
            pass
        return None

    def _end_stray_capture(self):
        """A capture that raised may leave the step's stream in capture mode (observed: hipStreamCaptureStatusActive after
        torch.cuda.graph's own clean-up): end it through the runtime so that the next capture can begin.  Best effort, and it says
        so when it could not (torch's own capture bookkeeping is not reset either way: a failed capture is not recoverable in
        general, DESIGN 6 lesson 13 -- this only makes the NEXT error name the real state)."""
        import ctypes
        import warnings
        try:
            if not self.stream.is_capturing():
                return
            hip = self._loaded_hip_runtime()
            if hip is None:
                warnings.warn('trainer: the step stream is still capturing after a failed capture and the loaded HIP runtime was not found; '
                              'the next capture will fail')
                return
            g = ctypes.c_void_p()
            rc = hip.hipStreamEndCapture(ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(g))
            if g.value:
                hip.hipGraphDestroy(g)
            if rc != 0 or self.stream.is_capturing():
                warnings.warn('trainer: hipStreamEndCapture on the stray capture returned %d; the stream %s capturing' %
                              (rc, 'is still' if self.stream.is_capturing() else 'stopped'))
        except Exception as e:          # noqa: BLE001 -- nothing more to try; the second capture will report the state it finds
            warnings.warn('trainer: could not end the stray capture (%r)' % (e,))

    def drop_graph(self):
        """Forget the captured step: the graph with its memory pool, the static batch and the static outputs (tensors handed out by
        train_step_graphed die with them), and the packed-weight cache, whose entries may point into that pool."""
        self._graph = None
        self._static = None
        self._static_out = None
        _conv._PACK_CACHE.clear()

    def load_batch(self, in_dict):
        """Copy a new batch into the captured graph's static input tensors (nested dictionaries included)."""
        def rec(dst, src, path):
            for k, v in src.items():
                if torch.is_tensor(v):
                    dst[k].copy_(v, non_blocking=True)
                elif isinstance(v, dict):
                    rec(dst[k], v, path + k + '.')
                elif k != 'dp_active' and dst.get(k) != v:
                    raise ValueError('train_step_graphed: %s%s = %r differs from the captured %r; capture() again' % (path, k, v, dst.get(k)))
        rec(self._static, in_dict, '')

    def train_step_graphed(self, in_dict=None):
        if self._graph is None:
            raise RuntimeError('call capture(in_dict) first')
        if in_dict is not None:
            self.load_batch(in_dict)
        self._decay_lr()
        self._graph.replay()
        if not self._reduce_in_graph:
            with self._on_stream():
                self.store.reduce_all()
                self.optimizer.step()
        self._end_step()
        return self._static_out

    # ------------------------------------------------------------------------------------------
    # The training loop: base_trainer.py:53-106 around the step prologue of train/trainer.py:134-212.  Steps run eagerly unless
    # options.graph asks for captured steps: `pretrain_mode` and `dp_active` are host switches that a captured graph freezes, so a
    # graphed run holds one graph per pretrain_mode phase and decides dp_active once, from the datasets of the run (_fit_step).
    def build_in_dict(self, host_batch, fits_dict, train_data='h36m_dp', pretrain_mode=False, vis_on=False, run_smplify=None):
        """A collated loader batch (datasets.collate) -> the in_dict of train_step, all on the step's own stream: upload + the two
        input ops (datasets.to_device), the fits (fits_dict[...], one gather + the label op), valid_fit, prepare_batch.  vis_on: the
        step's output will be looked at (base_trainer.py:73; fit sets it on visualisation steps).  run_smplify (None:
        self.options.run_smplify, absent = off): the in_dict also carries what the refresh stage needs to find each sample's table
        row again -- 'fit_rows' int64 [B], 'fit_rot_flip' float64 [B,2] (degrees, flip: what the fetch was asked with) and
        'fit_has_smpl' [B]; off, the key set is unchanged."""
        from . import datasets
        with self._on_stream():
            batch = datasets.to_device(host_batch, self.device, cfg.DANET.INIMG_SIZE)
            opt_pose, opt_betas = fits_dict[(batch['dataset_name'], batch['sample_index'], batch['rot_angle'], batch['is_flipped'])]
            has_smpl = batch['has_smpl'] > 0
            if train_data == 'h36m_coco_itw':
                batch['valid_fit'] = (fits_dict.get_vaild_state(batch['dataset_name'], batch['sample_index']) > 0) | has_smpl
            else:
                batch['valid_fit'] = has_smpl
            batch['vis_on'] = bool(vis_on)
            batch['pretrain_mode'] = bool(pretrain_mode)
            in_dict = self.prepare_batch(batch, opt_pose, opt_betas)
            in_dict['dp_dict']['dp_active'] = bool(host_batch['dp_active'])
            if getattr(self.options, 'run_smplify', False) if run_smplify is None else run_smplify:
                in_dict['fit_rows'] = fits_dict.rows(batch['dataset_name'], batch['sample_index'])
                in_dict['fit_rot_flip'] = fits_dict._rot_flip(batch['rot_angle'], batch['is_flipped'])
                in_dict['fit_has_smpl'] = batch['has_smpl'].clone()
        return in_dict

    def refresh_fits(self, looper, in_dict, output):
        """The refresh stage of a step that has run (fit_loop.InLoopFit.refresh; DESIGN.md 4d "the refresh rule"), eagerly on the step's
        stream: in_dict as the step saw it (of a replayed step the graph's static batch) and the step's output, both read before the
        next step overwrites them.  The training output carries the predicted row in three pieces (output['prediction']: cam, shape,
        pose), which are put back together here; an output with 'para' is taken as it is.  -> refresh's device tensors; nothing is
        read on the host."""
        with self._on_stream():
            if 'para' in output:
                para = output['para'].detach()
            else:
                pred = output['prediction']
                para = torch.cat([pred['cam'].detach(), pred['shape'].detach(), pred['pose'].detach().reshape(-1, 216)], dim=1)
            return looper.refresh(para, in_dict, in_dict['fit_rows'], in_dict['fit_rot_flip'], in_dict['fit_has_smpl'])

    @staticmethod
    def fit_summary(stats):
        """refresh's tensors -> the four numbers of a summary line (ONE host read): fit_eligible and fit_updated are counts, fit_e_old
        and fit_e_new means over the eligible samples (None with none, or where the mean is not finite)."""
        el = stats['eligible']
        elf = el.to(torch.float64)
        zero = torch.zeros((), device=el.device, dtype=torch.float64)
        mean = lambda e: torch.where(el, e.to(torch.float64), zero).sum() / elf.sum().clamp(min=1)      # noqa: E731
        n, up, eo, en = torch.stack([elf.sum(), stats['updated'].to(torch.float64).sum(), mean(stats['e_old']), mean(stats['e_new'])]).tolist()
        ok = lambda v: float(v) if n > 0 and np.isfinite(v) else None                                # noqa: E731
        return {'fit_eligible': int(n), 'fit_updated': int(up), 'fit_e_old': ok(eo), 'fit_e_new': ok(en)}

    def _fit_step(self, in_dict):
        """One step of a graphed fit (see fit): eager for the first two steps of a pretrain_mode phase, a capture before the third,
        replays from there on.  -> (output, losses, in_dict as the step saw it): of a replayed step the graph's static tensors."""
        phase, done, dp_captured = self._fit_phase
        if phase != in_dict['pretrain_mode']:
            # a new phase runs other modules: drop the old graph, static batch and pool FIRST, and let the two eager steps record and
            # build the weight bank again (the bank of a pretrain-mode step holds none of the regressor's weights)
            self.drop_graph()
            self._forget_bank()
            phase, done = in_dict['pretrain_mode'], 0
        if done < 2:
            out, losses = self.train_step(in_dict)
            self.fit_stats['eager_steps'] += 1
        else:
            if self._graph is None:
                self.capture(in_dict, warmup=0, dp_active=dp_captured)
                self.fit_stats['captures'] += 1
            out, losses = self.train_step_graphed(in_dict)
            in_dict = self._static
            self.fit_stats['replayed_steps'] += 1
        self._fit_phase = (phase, done + 1, dp_captured)
        return out, losses, in_dict

    # ------------------------------------------------------------------------------------------
    # Training visualisation (train/trainer.py:250-305, models/danet/danet.py:210-235,334-350): image sheets as uint8 device
    # tensors, built by the two kernels of csrc/train_vis.hip from ops the demo already has.
    VIS_SCALARS = ('index_fg', 'p_index_fg')

    def _mesh_renderer(self, res):
        from .renderer import MeshRenderer
        cache = self.__dict__.setdefault('_mesh_renderers', {})
        if res not in cache:
            cache[res] = MeshRenderer(self.smpl.faces, img_res=res)
        return cache[res]

    @torch.no_grad()
    def visualize(self, in_dict, output, losses=None):
        """The sheets of a step that ran with `vis_on`, under the reference's tags -> {tag: uint8 [3,Hs,Ws] device tensor}, a sheet
        only where its source is present: opt_shape, pred_shape (label / predicted mesh beside the input, train_vis.pair_grid),
        pred_uv, gt_uv (decoded IUV over the input, overlay_grid), part_uvi_pred (sample 0's 24 decoded partial maps), part_uvi_gt
        (where the estimator materialises part_iuv_gt: not on the fused path), skps_hm_pred (max over the 24 heat-maps, clamped to
        1), skps_hm_pred_soft (sum of their spatial softmaxes), stn_centers_gt, stn_centers_pred (the STN centres marked on the
        input, joints_grid; all joints visible).  Plus the foreground fractions of the cleaned index maps (danet.py:218,336) as
        0-dim f32 device tensors: index_fg, and p_index_fg when the regressor ran.  Runs eagerly on the step's stream; reads its
        arguments only (target_smpl_kps and stn_kps_pred are not scaled in place, unlike trainer.py:281-282,293-294).  `losses` is
        accepted for the reference's signature and not used."""
        from . import iuvmap, train_vis as tv
        from .iuv_estimator import DP2SMPL_MAPPING
        vis = output.get('visualization', {})
        pred = output.get('prediction', {})
        pretrain = bool(in_dict.get('pretrain_mode', False))
        img = in_dict['img']
        S = img.shape[-1]
        sheets = {}
        with self._on_stream():
            if 'target_verts' in in_dict and 'target_cam' in in_dict and S == cfg.DANET.INIMG_SIZE:
                images = tv.denormalized(img)                          # (the renderer's background; the sheets de-normalise in their own launch)
                render = self._mesh_renderer(S)
                sheets['opt_shape'] = tv.pair_grid(images, render(in_dict['target_verts'].detach(), in_dict['target_cam'].detach(), images)[0])
                if not pretrain and 'vertices' in pred and 'cam' in pred:
                    sheets['pred_shape'] = tv.pair_grid(images, render(pred['vertices'].detach(), pred['cam'].detach(), images)[0])
            if 'iuv_pred' in vis:
                sheets['pred_uv'] = tv.overlay_grid(img, iuvmap.iuv_map2img(*vis['iuv_pred']))
                index = vis['iuv_pred'][2]
                sheets['index_fg'] = index[:, 1:].sum(dtype=torch.float32) / index[:, 0].numel()
            if 'gt_uv' in vis:
                sheets['gt_uv'] = tv.overlay_grid(img, vis['gt_uv'])
            if not pretrain and vis.get('part_iuv_pred') is not None:
                part = vis['part_iuv_pred']
                sheets['part_uvi_pred'] = tv.make_grid(iuvmap.part_iuv_map2img(part[:1], DP2SMPL_MAPPING)[0], padding=1, pad_value=1)
                sheets['p_index_fg'] = part[:, :, 2, 1:].sum(dtype=torch.float32) / part[:, :, 2, 0].numel()
            if vis.get('part_iuv_gt') is not None:
                sheets['part_uvi_gt'] = tv.make_grid(iuvmap.part_iuv_map2img(vis['part_iuv_gt'][:1], DP2SMPL_MAPPING)[0], padding=1, pad_value=1)
            if 'skps_hm_pred' in vis:
                hm = vis['skps_hm_pred'].to(torch.float32)
                sheets['skps_hm_pred'] = tv.make_grid(hm.amax(dim=1, keepdim=True).clamp(max=1.), padding=1, pad_value=1)
                soft = torch.softmax(hm.flatten(2), dim=2).reshape(hm.shape).sum(dim=1, keepdim=True)
                sheets['skps_hm_pred_soft'] = tv.make_grid(soft, padding=1, pad_value=1)
            for tag, kps in (('stn_centers_gt', in_dict.get('target_smpl_kps')), ('stn_centers_pred', vis.get('stn_kps_pred'))):
                if kps is not None:
                    sheets[tag] = tv.joints_grid(img, kps[:, :, :2].to(torch.float32) * (S / 2.) + S / 2.)
            for tag in sheets:
                if tag not in self.VIS_SCALARS:
                    sheets[tag] = tv.to_uint8(sheets[tag])
        return sheets

    def write_sheets(self, folder, sheets):
        """What visualize returned -> one <tag>.png per sheet under `folder` (ONE device-to-host copy for all of them) and the
        scalars as {name: float}."""
        from . import train_vis as tv
        tags = [t for t in sheets if t not in self.VIS_SCALARS]
        os.makedirs(folder, exist_ok=True)
        if tags:
            with self._on_stream():
                flat = torch.cat([sheets[t].reshape(-1) for t in tags] +
                                 [sheets[t].reshape(1).view(torch.uint8) for t in self.VIS_SCALARS if t in sheets])
            host = flat.cpu().numpy()
            at = 0
            for t in tags:
                n = sheets[t].numel()
                tv.write_png(os.path.join(folder, t + '.png'), host[at:at + n].reshape(tuple(sheets[t].shape)).transpose(1, 2, 0))
                at += n
            return {t: float(v) for t, v in zip([t for t in self.VIS_SCALARS if t in sheets], host[at:].view(np.float32))}
        return {t: float(sheets[t]) for t in self.VIS_SCALARS if t in sheets}

    # ------------------------------------------------------------------------------------------
    # Validation (train/base_trainer.py:89-91,121-122: `test` is declared and left empty there).
    def test(self, val, options=None):
        """Scores the model as it stands on a validation set: val = (dataset_name, dataset), an evaluate.EvalDataset or anything
        evaluate.iterate_batches takes.  Runs evaluate.run_evaluation(self.model, ..., verbose=False) in eval mode on the step's stream
        with options.batch_size (options: default self.options; eval_pve, num_workers, J_regressor, smpl_male / smpl_female and
        part_renderer are read from it) and puts the model back into the mode it found.  -> {'val_dataset', 'val_num_samples',
        'val_mpjpe', 'val_recon_err'[, 'val_pve', 'val_pa_pve']}; for 'lsp' the accuracy / F1 numbers under val_ names.
        Leaves the training run alone: eval mode updates no BatchNorm statistics and draws no random numbers, nothing of the
        optimizer, the loader or step_count is touched, and a captured graph with its static batch and pool is not either -- the
        loop runs eagerly between replays, like visualize.  The inference forward packs every conv weight afresh from the fp32
        parameters: the packed-weight cache is emptied before, because a replayed optimizer step changes the
        parameters without moving the version numbers the cache keys on, and again afterwards, so that no copy packed here can be
        taken for current at a later validation.  The bank the captured step reads is a buffer of its own and is not touched.
        With world_size > 1 rank 0 validates the whole set and the other ranks wait at the next step's collective; the
        validation set is not sharded."""
        from . import evaluate
        name, dataset = val
        o = options if options is not None else self.options
        if self.distributed and torch.distributed.get_rank() != 0:
            return {}
        was_training = self.model.training
        with _conv.fresh_packs():
            self.model.eval()
            try:
                with self._on_stream():
                    s = evaluate.run_evaluation(self.model, name, dataset, None, batch_size=int(getattr(o, 'batch_size', 32)),
                                                num_workers=int(getattr(o, 'num_workers', 0) or 0), log_freq=0, options=o, verbose=False)
            finally:
                self.model.train(was_training)
        out = {'val_dataset': name, 'val_num_samples': s['num_samples']}
        for k in ('mpjpe', 'recon_err', 'pve', 'pa_pve', 'accuracy', 'f1', 'parts_accuracy', 'parts_f1'):
            if k in s:
                out['val_' + k] = s[k]
        return out

    @staticmethod
    def latest_checkpoint(checkpoint_dir):
        names = sorted(n for n in os.listdir(checkpoint_dir) if n.startswith('step_') and n.endswith('.pt')) if os.path.isdir(checkpoint_dir) else []
        return os.path.join(checkpoint_dir, names[-1]) if names else None

    def fit(self, train_ds, fits_dict, options, on_step=None, val=None):
        """Trains on `train_ds` (a datasets.MixedDataset / TrainDataset) with the pseudo-label store `fits_dict`.  options:
        num_epochs, batch_size, checkpoint_steps, summary_steps, pretr_step, train_data, num_workers, time_to_run (seconds), seed,
        shuffle_train, log_dir, checkpoint_dir, resume (a checkpoint file, or True: the newest of checkpoint_dir), pretrained_checkpoint.
        Every summary_steps steps one JSON line with the losses goes to <log_dir>/train_log.jsonl; a checkpoint step_<n>.pt with
        epoch, batch_idx and dataset_perm is written every checkpoint_steps steps and when time_to_run is over.
        on_step(step_count, in_dict, losses), if given, is called after every step.  Returns the number of steps run.
        options.graph (default off): steps run as hipGraph replays.  A phase is a value of pretrain_mode; its first two steps run
        eagerly on their own batches (they build the weight bank and the allocator's state the capture needs, and they are real
        optimizer steps), the third step's in_dict is captured (no warm-up steps of the capture's own) and that step and every later
        one of the phase is a replay; when the phase changes the graph, its static batch and its pool are dropped first.  DensePose
        point supervision is captured as active iff 'dp_coco' is one of the run's datasets (TRAIN_SETS[train_data]), decided once per
        run.  A batch of another shape than the captured one raises (load_batch).  The `losses` of a replayed step are the graph's
        static output tensors: valid until the next step, which overwrites them -- copy what must outlive it.
        self.fit_stats = {'eager_steps', 'replayed_steps', 'captures'} counts this call's steps.
        options.vis_interval (absent, None or 0: off): a step with (step_count - 1) % vis_interval == 0 is followed by visualize();
        its sheets go to <log_dir>/vis/step_%08d/<tag>.png and index_fg / p_index_fg into the step's JSON line (a line of its own
        where the summary schedule has none).  Eager runs set `vis_on` on exactly those steps (base_trainer.py:73); a graphed run
        sets it on EVERY step, since the capture freezes the switch, and a replayed visualisation step reads the graph's static
        outputs before the next replay overwrites them.  visualize itself always runs eagerly, outside the graph.
        options.test_steps (absent, None or 0: off; the reference's default is 1000) with val = (dataset_name, dataset): every step
        with step_count % test_steps == 0 (base_trainer.py:90) is followed, after its checkpoint, by self.test(val, options); the
        val_* numbers go into the step's JSON line (a line of its own where the summary schedule has none).  test_steps > 0 without
        `val` raises ValueError before the first step.  Validation runs eagerly between replays and leaves the run alone (test).
        options.run_smplify (absent or False: off; DESIGN.md 4d "the refresh rule"): every step outside pretrain_mode is followed by
        refresh_fits -- the prediction is fitted to the batch's keypoints (options.num_smplify_iters iterations; None: the fitter's
        default) and replaces the stored pseudo-label where it explains them better; a refreshed row's valid flag follows
        options.smplify_threshold.  The step trains on what the table held when its batch was built; the refreshed label is seen at
        the sample's next visit.  Under options.graph the stage is a handful of eager launches after the replay, on the step's
        stream, reading the graph's static batch and output; it is not part of the graph.  Summary lines gain fit_eligible,
        fit_updated, fit_e_old, fit_e_new (fit_summary; the only host reads of the stage).  The table and its valid flags are
        written to checkpoint_dir (FitsDict.save_state) with every checkpoint and when fit returns, and read back from there on
        `resume`; only the newest state is kept, so resuming an older step_<n>.pt continues with the newest table.  With
        world_size > 1 the option raises before the first step: each rank holds its own table and nothing reconciles them."""
        import json
        import time
        from . import checkpoint, datasets, evaluate, train_vis
        opt = lambda k, d=None: d if getattr(options, k, None) is None else getattr(options, k)       # noqa: E731
        test_steps = int(opt('test_steps', 0))
        if test_steps > 0 and val is None:
            raise ValueError('fit: options.test_steps = %d needs a validation set: pass val=(dataset_name, dataset)' % test_steps)
        run_smplify = bool(opt('run_smplify', False))
        if run_smplify and self.distributed:
            raise RuntimeError('fit: options.run_smplify with world_size > 1: each rank holds its own FitsDict table and nothing reconciles them')
        bs, ckpt_dir, log_dir = int(options.batch_size), opt('checkpoint_dir', 'checkpoints'), opt('log_dir', 'logs')
        endtime = time.time() + float(opt('time_to_run', np.inf))
        book, epoch0 = None, 0
        resume = opt('resume', None)
        if resume:
            path = resume if isinstance(resume, str) else self.latest_checkpoint(ckpt_dir)
            if path is not None:
                book = self.resume(path, trusted=True)
                epoch0 = int(book.get('epoch') or 0)
            if run_smplify:
                fits_dict.load_state(ckpt_dir)
        elif opt('pretrained_checkpoint', None):
            checkpoint.load_pretrained(self.model, options.pretrained_checkpoint)
        os.makedirs(log_dir, exist_ok=True)
        ran = 0
        self.fit_stats = {'eager_steps': 0, 'replayed_steps': 0, 'captures': 0}
        graphed = bool(opt('graph', False))
        train_data = opt('train_data', 'h36m_dp')
        vis_interval = int(opt('vis_interval', 0))
        if graphed:
            if self.device.type != 'cuda':
                raise RuntimeError('options.graph needs a GPU')
            self.drop_graph()                                              # (a graph of an earlier run: its phase is unknown here)
            self._fit_phase = (None, 0, 'dp_coco' in datasets.TRAIN_SETS.get(train_data, ()))

        looper = None
        if run_smplify:
            from .fit_loop import InLoopFit
            looper = InLoopFit(self.smpl, fits_dict, tau=opt('smplify_threshold', None), iters=opt('num_smplify_iters', None))

        def save(epoch, batch_idx, perm):
            if run_smplify:
                fits_dict.save_state(ckpt_dir)
            return self.save(os.path.join(ckpt_dir, 'step_%08d.pt' % self.step_count), epoch=epoch, batch_idx=batch_idx, batch_size=bs, dataset_perm=perm)

        with open(os.path.join(log_dir, 'train_log.jsonl'), 'a') as log:
            for epoch in range(epoch0, int(options.num_epochs)):
                loader = datasets.TrainLoader(train_ds, checkpoint=book, batch_size=bs, shuffle=bool(opt('shuffle_train', True)),
                                              num_workers=int(opt('num_workers', 0)), seed=int(opt('seed', 0)), epoch=epoch, res=cfg.DANET.INIMG_SIZE)
                for step, host in enumerate(loader, loader.checkpoint_batch_idx):
                    if time.time() >= endtime:
                        save(epoch, step, loader.sampler.dataset_perm)       # (with the table's state, when it is refreshed)
                        return ran
                    count = self.step_count + 1                            # (base_trainer.py:70-74: the step about to run)
                    vis_on = vis_interval > 0 if graphed else train_vis.vis_due(count, vis_interval)
                    in_dict = self.build_in_dict(host, fits_dict, train_data, pretrain_mode=count <= int(opt('pretr_step', 0)), vis_on=vis_on,
                                                 run_smplify=run_smplify)
                    if graphed:
                        output, losses, seen = self._fit_step(in_dict)
                    else:
                        output, losses = self.train_step(in_dict)
                        seen = in_dict
                        self.fit_stats['eager_steps'] += 1
                    ran += 1
                    refreshed = None if looper is None or seen['pretrain_mode'] else self.refresh_fits(looper, seen, output)
                    line = None
                    if (self.step_count - 1) % int(opt('summary_steps', 100)) == 0:
                        vals = {'loss_' + k: float(v.detach()) for k, v in losses.items()}      # ('loss_{}'.format(key), train/trainer.py:221)
                        vals['loss_tatal'] = float(sum(vals.values()))
                        line = {'step': self.step_count, 'epoch': epoch, 'batch_idx': step, **vals}
                        if refreshed is not None:
                            line.update(self.fit_summary(refreshed))
                    if train_vis.vis_due(self.step_count, vis_interval):
                        line = line or {'step': self.step_count, 'epoch': epoch, 'batch_idx': step}
                        line.update(self.write_sheets(os.path.join(log_dir, 'vis', 'step_%08d' % self.step_count), self.visualize(seen, output, losses)))
                    due = evaluate.val_due(self.step_count, test_steps)
                    if line is not None and not due:
                        log.write(json.dumps(line) + '\n')
                        log.flush()
                    if on_step is not None:
                        on_step(self.step_count, in_dict, losses)
                    if self.step_count % int(opt('checkpoint_steps', 10000)) == 0:
                        save(epoch, step + 1, loader.sampler.dataset_perm)
                    if due:                                                # (base_trainer.py:89-91, after the checkpoint of the step)
                        line = line or {'step': self.step_count, 'epoch': epoch, 'batch_idx': step}
                        line.update(self.test(val, options))
                        log.write(json.dumps(line) + '\n')
                        log.flush()
                book = None                                                # (a checkpoint positions the first epoch only)
                if (epoch + 1) % 10 == 0:
                    save(epoch + 1, 0, None)
        if run_smplify:
            fits_dict.save_state(ckpt_dir)
        return ran
