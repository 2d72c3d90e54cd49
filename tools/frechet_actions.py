#!/usr/bin/env python3
"""Frechet pose / motion distance of generated actions on the kg_frechet HIP kernels (metrics.frechet).

The file flags and the selection of tools/prdc_actions.py.  Real data is read through Feeder(norm=True), fake data (the
.npy / .pkl pair sample.py's outputs are saved as) through Feeder(norm=False); the first --per_class samples of every class
(10 for h36m, 60 otherwise) are selected as mmd_actions.py selects them and cropped to --t_size frames.  Every class is
scored on its own - pose: a point is one frame (dimension C*V); motion: the difference of two consecutive frames - and the
two class means are printed; --per_class_table adds one row per class.  --unconditional scores all selected samples as one
set.

    python tools/frechet_actions.py --data_real train_data.npy --labels_real train_label.pkl \\
        --data_fake gen_data.npy --labels_fake gen_label.pkl --t_size 64 --dataset h36m --per_class 100"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.metrics import frechet, select_reference_samples  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_real", type=str, required=True, help="path to real data")
    ap.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    ap.add_argument("--data_fake", type=str, required=True, help="path to fake data")
    ap.add_argument("--labels_fake", type=str, required=True, help="path to fake labels")
    ap.add_argument("--t_size", type=int, default=64, help="Temporal dimension")
    ap.add_argument("--dataset", type=str, default="h36m", help="dataset to evaluate")
    ap.add_argument("--per_class", type=int, default=100, help="samples of every class, of each set")
    ap.add_argument("--unconditional", action="store_true", help="score all selected samples as one set")
    ap.add_argument("--per_class_table", action="store_true", help="print one row per class")
    opt = ap.parse_args(argv)
    print(opt)

    real_f = Feeder(opt.data_real, opt.labels_real, norm=True, dataset=opt.dataset)     # normalised to [-1, 1]
    fake_f = Feeder(opt.data_fake, opt.labels_fake, norm=False, dataset=opt.dataset)    # already normalised
    classes = np.arange(10 if opt.dataset == "h36m" else 60)
    real, real_lab, _ = select_reference_samples(real_f, classes, opt.t_size, opt.per_class)
    fake, fake_lab, _ = select_reference_samples(fake_f, classes, opt.t_size, opt.per_class)
    print(real.shape, "real")
    print(fake.shape, "fake")
    dev = torch.device("cuda", torch.cuda.current_device())
    if opt.unconditional:
        real_lab = fake_lab = None
    out = frechet(torch.from_numpy(fake).to(dev), torch.from_numpy(real).to(dev), fake_lab, real_lab, mode="both")
    pose, motion = float(out["pose"]["mean"].cpu()), float(out["motion"]["mean"].cpu())
    if opt.per_class_table:
        print("class %12s %12s" % ("pose_fd", "motion_fd"))
        for c, (p, q) in enumerate(zip(out["pose"]["values"].cpu().tolist(), out["motion"]["values"].cpu().tolist())):
            print("%5d %12.6f %12.6f" % (c, p, q))
    print("pose_fd %.6f motion_fd %.6f" % (pose, motion))
    return pose, motion


if __name__ == "__main__":
    main()
