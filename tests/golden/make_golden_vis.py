"""Generates tests/golden/g24_vis.npz by IMPORTING the reference's utils.iuvmap.iuv_map2img (like make_golden.py, whose CPU shim
its `.cuda(device_id)` needs): (a) raw global predictions with Ann, (b) the same through the reference's iuvmap_clean with and
without Ann, (c) the 24 partial maps with ind_mapping = [0] + dp2smpl_mapping[i].  The inputs are the seeded streams of
tests/vis_oracle.py (numpy's frozen RandomState); the file holds their check sums and the reference's outputs.
Re-run:  python tests/golden/make_golden_vis.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import ref_env, save   # noqa: E402
import vis_oracle as vo                  # noqa: E402


def main():
    ref_env()
    from utils.iuvmap import iuv_map2img, iuvmap_clean
    from utils.smpl_utlis import smpl_structure
    U, V, I, A = (torch.from_numpy(a) for a in vo.g24_global_inputs())
    raw = iuv_map2img(U, V, I, A)
    cU, cV, cI, cA = iuvmap_clean(U, V, I, A)
    clean_ann = iuv_map2img(cU, cV, cI, cA)
    clean = iuv_map2img(cU, cV, cI)
    mapping = smpl_structure('dp2smpl_mapping')
    P = torch.from_numpy(vo.g24_part_inputs())
    part = torch.stack([torch.cat([iuv_map2img(P[b:b + 1, i, 0], P[b:b + 1, i, 1], P[b:b + 1, i, 2], ind_mapping=[0] + mapping[i])
                                   for i in range(24)], 0) for b in range(P.shape[0])], 0)
    save('g24_vis', in_crc=vo.crc(U.numpy(), V.numpy(), I.numpy(), A.numpy()), clean_crc=vo.crc(cU.numpy(), cV.numpy(), cI.numpy(), cA.numpy()),
         part_crc=vo.crc(P.numpy()), raw=raw, clean_ann=clean_ann, clean=clean, part=part, dp2smpl_mapping=np.asarray(mapping, dtype=np.int64))


if __name__ == '__main__':
    main()
