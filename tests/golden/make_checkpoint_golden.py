#!/usr/bin/env python3
"""The reference's trained checkpoints of two materials as plain arrays: ``reference_checkpoints.npz``.

Four ``state_dict``s, stored unchanged (fp32, the reference's own key names) under ``<case>/<file stem>/<key>``:
  chm_orange_rgb_disk/brdf_rectify_networkchm_orange_rgb     (NN_cond_pos_simpler, 32 x 3)
  chm_orange_rgb_disk/brdf_pretrain_networkchm_orange_rgb    (NN_cond_pretrain_disk_one)
  bsdf_3_spherical/brdf_rectify_network3                     (NN_cond_pos, 32 x 4)
  bsdf_3_spherical/brdf_pretrain_network3                    (NN_cond_pretrain_spherical_one)
tests/test_host_cpu.py loads them into the weight containers of bsdf_diffusion_sampling_amd/model.py and checks that
packing them yields exactly the shipped .bsdfw weights.

Usage:  python tests/golden/make_checkpoint_golden.py <reference checkout>/rendering/checkpoints_new
"""
import os
import sys

import numpy as np
import torch

FILES = ("chm_orange_rgb_disk/brdf_rectify_networkchm_orange_rgb", "chm_orange_rgb_disk/brdf_pretrain_networkchm_orange_rgb",
         "bsdf_3_spherical/brdf_rectify_network3", "bsdf_3_spherical/brdf_pretrain_network3")


def main():
    ckpt = sys.argv[1]
    out = {}
    for f in FILES:
        sd = torch.load(os.path.join(ckpt, f + ".pth"), map_location="cpu", weights_only=True)
        for k, v in sd.items():
            out[f"{f}/{k}"] = v.detach().cpu().numpy()
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_checkpoints.npz")
    np.savez_compressed(dst, **out)
    print(dst, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
