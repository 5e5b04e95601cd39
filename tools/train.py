"""Train a DaNet model: the reference's train.py.

  python tools/train.py --name RUN [--data_root DIR] [--train_data h36m_dp|h36m_coco_itw] [--num_epochs N] [--batch_size B]
                        [--checkpoint_steps K] [--summary_steps K] [--pretr_step K] [--resume] [--pretrained_checkpoint FILE]
                        [--num_workers W] [--ignore_3d] [--time_to_run SECONDS] [--cfg YAML] [--log_dir DIR] [--graph]
                        [--vis_interval K] [--test_steps K [--val_dataset NAME] [--val_annot FILE.npz --val_img_dir DIR] [--eval_pve]]
                        [--run_smplify [--smplify_threshold TAU] [--num_smplify_iters N]]

--data_root holds, for every dataset <ds> of --train_data, <ds>_train.npz (the reference's annotation layout), the image folder <ds>/
and the fits folders final_fits/ and static_fits/.  Without it a small synthetic 'h36m_dp' set is written to a scratch directory and
trained on, so the tool runs on a machine with no data.  --graph runs the steps as hipGraph replays (Trainer.fit: two eager steps and
one capture per pretrain_mode phase).  --vis_interval K (default 0 = off; the reference's default is 1000) writes the image sheets of
Trainer.visualize to <log_dir>/<name>/vis/step_<n>/<tag>.png after every K-th step.  --test_steps K (default 0 = off; the reference's
default is 1000, and its test() is empty) runs the evaluation loop of tools/eval.py on --val_dataset (default h36m-p2) after every K-th
step and writes val_mpjpe, val_recon_err and, with --eval_pve, val_pve / val_pa_pve (mm) into that step's line of train_log.jsonl;
without --val_annot a small synthetic validation set is written to the run's scratch directory.  --run_smplify (default off) refreshes
the pseudo-labels inside training (DESIGN.md 4d "the refresh rule"): after every step outside pretrain_mode the prediction is fitted to
the batch's keypoints for --num_smplify_iters iterations (default 100) and replaces the stored fit where it explains them better; a
refreshed row counts as a valid fit when its data energy is below --smplify_threshold (default sigma^2 / 5 of the fitter) times the
summed squared confidences.  The table and its valid flags are kept beside the checkpoints and read back by --resume.  Logs (train_log.jsonl) and checkpoints
go to <log_dir>/<name>/.
Last line: one JSON object (steps run, last losses)."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(description='DaNet training')
    ap.add_argument('--name', required=True, help='name of the run')
    ap.add_argument('--data_root', default=None)
    ap.add_argument('--log_dir', default='logs')
    ap.add_argument('--num_epochs', type=int, default=30)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--checkpoint_steps', type=int, default=10000)
    ap.add_argument('--summary_steps', type=int, default=100)
    ap.add_argument('--pretr_step', type=int, default=0, help='steps that train the IUV estimator alone')
    ap.add_argument('--train_data', default='h36m_dp', choices=['h36m_dp', 'h36m_coco_itw'])
    ap.add_argument('--resume', action='store_true', help='continue from the newest checkpoint of the run')
    ap.add_argument('--pretrained_checkpoint', default=None)
    ap.add_argument('--num_workers', type=int, default=8, help='reader threads (at most 8)')
    ap.add_argument('--ignore_3d', action='store_true')
    ap.add_argument('--time_to_run', type=float, default=None, help='seconds; a checkpoint is written when they are over')
    ap.add_argument('--cfg', dest='cfg_file', default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--num_synthetic', type=int, default=32)
    ap.add_argument('--graph', action='store_true', help='replay captured steps (one hipGraph per pretrain_mode phase)')
    ap.add_argument('--vis_interval', type=int, default=0, help='steps between image sheets under <log_dir>/<name>/vis (0: none)')
    ap.add_argument('--test_steps', type=int, default=0, help='steps between validation runs (0: none)')
    ap.add_argument('--val_dataset', default='h36m-p2', choices=['h36m-p1', 'h36m-p2', 'lsp', '3dpw', 'mpi-inf-3dhp'])
    ap.add_argument('--val_annot', default=None, help='annotation .npz of the validation set (default: a synthetic one)')
    ap.add_argument('--val_img_dir', default=None)
    ap.add_argument('--eval_pve', action='store_true', help='validation also reports the per-vertex errors PVE / PA-PVE')
    ap.add_argument('--run_smplify', action='store_true', help='refresh the pseudo-labels from keypoint fits of the predictions (one process only)')
    ap.add_argument('--smplify_threshold', type=float, default=None,
                    help='a refreshed fit is valid below this data energy per unit of squared confidence (default: sigma^2 / 5)')
    ap.add_argument('--num_smplify_iters', type=int, default=100, help='iterations of the in-loop fit: 30 %% camera and orientation, then all')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)

    import torch
    from danet_densepose2smpl_amd import datasets, evaluate
    from danet_densepose2smpl_amd.config import cfg, cfg_from_file
    from danet_densepose2smpl_amd.fits_dict import FitsDict
    from danet_densepose2smpl_amd.trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit('tools/train.py needs a GPU (there is no CPU path)')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    run = os.path.join(a.log_dir, a.name)
    a.log_dir, a.checkpoint_dir = run, os.path.join(run, 'checkpoints')
    a.shuffle_train, a.heatmap_size, a.img_res = True, cfg.DANET.HEATMAP_SIZE, cfg.DANET.INIMG_SIZE
    a.openpose_train_weight, a.gt_train_weight = 0., 1.
    tmp = None
    if a.data_root is None:
        if a.train_data != 'h36m_dp':
            raise SystemExit("the synthetic training set is an 'h36m_dp' one; --train_data %s needs --data_root" % a.train_data)
        tmp = tempfile.TemporaryDirectory()
        train_ds, paths = datasets.synthetic_mixed_dataset(a, tmp.name, a.num_synthetic, a.num_synthetic, a.seed)
        fits_dirs = (paths['final_fits_dir'], paths['static_fits_dir'])
    else:
        sets = [datasets.TrainDataset(a, n, os.path.join(a.data_root, n + '_train.npz'), os.path.join(a.data_root, n), ignore_3d=a.ignore_3d)
                for n in datasets.TRAIN_SETS[a.train_data]]
        train_ds = datasets.MixedDataset(a, sets)
        fits_dirs = (os.path.join(a.data_root, 'final_fits'), os.path.join(a.data_root, 'static_fits'))
    val = None
    if a.test_steps > 0:
        if a.val_annot is None:
            if tmp is None:
                tmp = tempfile.TemporaryDirectory()
            a.val_img_dir = os.path.join(tmp.name, 'val')
            a.val_annot = evaluate.write_synthetic_dataset(a.val_img_dir, a.val_dataset, n=a.num_synthetic, seed=a.seed)
        elif a.val_img_dir is None:
            raise SystemExit('--val_annot needs --val_img_dir')
        val = (a.val_dataset, evaluate.EvalDataset(a.val_annot, a.val_img_dir, a.val_dataset))
    torch.manual_seed(a.seed)
    trainer = Trainer(a)
    fits = FitsDict(a, train_ds, fits_dirs[0], fits_dirs[1], trainer.device)
    last = {}

    def on_step(step, in_dict, losses):
        last.clear()
        last.update(step=step, **losses)         # (tensors: read once, after the last step -- no host read per step)
    steps = trainer.fit(train_ds, fits, a, on_step=on_step, val=val)
    last = {k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in last.items()}
    fits.save()
    print(json.dumps({'steps': steps, 'last': last}), flush=True)
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == '__main__':
    sys.exit(main())
