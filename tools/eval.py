"""Evaluate a DaNet model on 3D pose (MPJPE, reconstruction error) or on the LSP mask / part segmentation: the reference's eval.py.

  python tools/eval.py --dataset h36m-p2 [--checkpoint FILE] [--cfg YAML] [--annot FILE.npz --img_dir DIR [--label_dir DIR]]
                       [--batch_size N] [--result_file OUT.npz] [--log_freq K] [--engine] [--eval_pve]

--dataset: h36m-p1 | h36m-p2 | 3dpw | lsp | mpi-inf-3dhp.  --annot is the annotation .npz of the reference's layout; images and
label images are .npy arrays always, .png / .jpg if PIL is installed.  --joint_regressor (J_regressor_h36m.npy) and --smpl_dir
(SMPL_MALE / SMPL_FEMALE .pkl, for 3dpw) name the licence-gated files where they exist.  Without --checkpoint the model has seeded
random weights, and without --annot a small synthetic dataset is written to --scratch, so the tool runs on a machine with no data.
--eval_pve adds the per-vertex error over all mesh vertices, PVE and its Procrustes-aligned form PA-PVE in mm (the
reference declares the option and reads it nowhere).
Last line: one JSON object with the summary."""
import argparse
import json
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description='DaNet evaluation')
    ap.add_argument('--checkpoint', default=None, help='checkpoint in the reference\'s layout (default: seeded random weights)')
    ap.add_argument('--dataset', default='h36m-p2', choices=['h36m-p1', 'h36m-p2', 'lsp', '3dpw', 'mpi-inf-3dhp'])
    ap.add_argument('--log_freq', default=50, type=int)
    ap.add_argument('--batch_size', default=16, type=int)
    ap.add_argument('--shuffle', default=False, action='store_true')
    ap.add_argument('--num_workers', default=8, type=int, help='reader threads')
    ap.add_argument('--result_file', default=None, help='save pred_joints, pose, betas, camera to this .npz')
    ap.add_argument('--cfg', dest='cfg_file', default=None)
    ap.add_argument('--engine', action='store_true', help='run the BatchNorm-folded InferenceEngine instead of infer_net')
    ap.add_argument('--annot', default=None)
    ap.add_argument('--img_dir', default=None)
    ap.add_argument('--label_dir', default=None)
    ap.add_argument('--joint_regressor', default=None)
    ap.add_argument('--smpl_dir', default=None)
    ap.add_argument('--scratch', default=None, help='where the synthetic dataset goes (default: a temporary directory)')
    ap.add_argument('--num_synthetic', default=32, type=int)
    ap.add_argument('--eval_pve', default=False, action='store_true', help='evaluate PVE')
    a = ap.parse_args(argv)

    import torch
    from danet_densepose2smpl_amd import checkpoint, evaluate
    from danet_densepose2smpl_amd.config import cfg_from_file
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.smpl import SMPL
    from danet_densepose2smpl_amd.trainer import default_options
    if not torch.cuda.is_available():
        raise SystemExit('tools/eval.py needs a GPU (there is no CPU path)')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    tmp = None
    if a.annot is None:
        root = a.scratch
        if root is None:
            tmp = tempfile.TemporaryDirectory()
            root = tmp.name
        a.annot = evaluate.write_synthetic_dataset(root, a.dataset, n=a.num_synthetic, seed=0)
        a.img_dir = root
    elif a.img_dir is None:
        raise SystemExit('--annot needs --img_dir')
    dataset = evaluate.EvalDataset(a.annot, a.img_dir, a.dataset, a.label_dir)

    torch.manual_seed(0)
    model = DaNet(default_options(a.batch_size), None, pretrained=False)
    if a.checkpoint:
        checkpoint.load_pretrained(model, a.checkpoint)
    model = model.cuda().eval()
    options = types.SimpleNamespace(checkpoint=a.checkpoint, dataset=a.dataset, J_regressor=a.joint_regressor, eval_pve=a.eval_pve)
    if a.smpl_dir:
        options.smpl_male = SMPL(a.smpl_dir, gender='male').cuda()
        options.smpl_female = SMPL(a.smpl_dir, gender='female').cuda()
    runner = model.inference_engine(a.batch_size) if a.engine else model
    print(a.checkpoint, a.dataset)
    s = evaluate.run_evaluation(runner, a.dataset, dataset, a.result_file, batch_size=a.batch_size, shuffle=a.shuffle,
                                num_workers=a.num_workers, log_freq=a.log_freq, options=options)
    if a.engine:
        runner.close()
    keep = {k: v for k, v in s.items() if k in ('dataset', 'num_samples', 'mpjpe', 'recon_err', 'accuracy', 'f1', 'parts_accuracy', 'parts_f1', 'actions', 'pve', 'pa_pve', 'pve_num_samples')}
    print(json.dumps(keep), flush=True)
    if tmp is not None:
        tmp.cleanup()
    return 0


if __name__ == '__main__':
    sys.exit(main())
