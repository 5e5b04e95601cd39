"""Evaluate a DaNet model on COCO val2014 2D keypoints (AP / AR at OKS 0.50:0.95): the reference's eval_coco.py.

  python tools/eval_coco.py [--checkpoint FILE] [--cfg YAML] [--annot FILE.npz --keypoint_json FILE.json --img_dir DIR]
                            [--batch_size N] [--result_file OUT.npz] [--output_dir DIR] [--engine]

--annot is the annotation .npz of the reference's layout (imgname, center, scale: one row per person crop), --keypoint_json the
person_keypoints_val2014.json of the same images; images are .npy arrays always, .png / .jpg if PIL is installed.  Without
--checkpoint the model has seeded random weights, and without --annot a small synthetic set is written to --scratch, so the tool
runs on a machine with no data.  The results json goes to <output_dir>/results/.  Prints the reference's markdown table; last
line: one JSON object with the ten numbers."""
import argparse
import json
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description='DaNet COCO keypoint evaluation')
    ap.add_argument('--checkpoint', default=None, help='checkpoint in the reference\'s layout (default: seeded random weights)')
    ap.add_argument('--batch_size', default=16, type=int)
    ap.add_argument('--shuffle', default=False, action='store_true')
    ap.add_argument('--num_workers', default=8, type=int, help='reader threads')
    ap.add_argument('--result_file', default=None, help='save pred_joints, pose, betas, camera (and preds, image_ids) to this .npz')
    ap.add_argument('--regressor', default='danet', choices=['hmr', 'danet'], help="'hmr' is refused: there is no HMR regressor here")
    ap.add_argument('--output_dir', default='./output')
    ap.add_argument('--cfg', dest='cfg_file', default=None)
    ap.add_argument('--annot', default=None)
    ap.add_argument('--keypoint_json', default=None)
    ap.add_argument('--img_dir', default=None)
    ap.add_argument('--engine', action='store_true', help='run the BatchNorm-folded InferenceEngine instead of infer_net')
    ap.add_argument('--scratch', default=None, help='where the synthetic set goes (default: a temporary directory)')
    ap.add_argument('--num_synthetic', default=32, type=int)
    a = ap.parse_args(argv)

    import torch
    from danet_densepose2smpl_amd import checkpoint, evaluate_coco
    from danet_densepose2smpl_amd.config import cfg_from_file
    from danet_densepose2smpl_amd.danet import DaNet
    from danet_densepose2smpl_amd.trainer import default_options
    if a.regressor == 'hmr':
        raise SystemExit("--regressor hmr: there is no HMR regressor in this package; use 'danet'")
    if not torch.cuda.is_available():
        raise SystemExit('tools/eval_coco.py needs a GPU (there is no CPU path)')
    if a.cfg_file:
        cfg_from_file(a.cfg_file)
    tmp = runner = None
    try:
        if a.annot is None:
            root = a.scratch
            if root is None:
                tmp = tempfile.TemporaryDirectory()
                root = tmp.name
            a.annot, a.keypoint_json = evaluate_coco.write_synthetic_coco(root, n=a.num_synthetic, seed=0)
            a.img_dir = root
        elif a.img_dir is None or a.keypoint_json is None:
            raise SystemExit('--annot needs --img_dir and --keypoint_json')
        dataset = evaluate_coco.EvalDataset(a.annot, a.img_dir, 'coco')

        torch.manual_seed(0)
        model = DaNet(default_options(a.batch_size), None, pretrained=False)
        if a.checkpoint:
            checkpoint.load_pretrained(model, a.checkpoint)
        model = model.cuda().eval()
        options = types.SimpleNamespace(checkpoint=a.checkpoint, regressor=a.regressor, keypoint_json=a.keypoint_json, output_dir=a.output_dir)
        runner = model.inference_engine(a.batch_size) if a.engine else None
        values = evaluate_coco.run_evaluation(runner if a.engine else model, dataset, a.result_file, batch_size=a.batch_size, shuffle=a.shuffle,
                                              num_workers=a.num_workers, options=options)
        print(json.dumps(values), flush=True)
    finally:
        if runner is not None:
            runner.close()
        if tmp is not None:
            tmp.cleanup()
    return 0


if __name__ == '__main__':
    sys.exit(main())
