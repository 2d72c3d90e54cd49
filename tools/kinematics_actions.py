#!/usr/bin/env python3
"""Kinematic plausibility of generated actions on the kg_kin HIP kernels (metrics.kinematics): is this a body?

The file flags and the selection of tools/frechet_actions.py.  Real data is read through Feeder(norm=True), fake data (the
.npy / .pkl pair sample.py's outputs are saved as) through Feeder(norm=False); the descriptors do not depend on that scalar
normalisation.  The first --per_class samples of every class are selected as mmd_actions.py selects them and cropped to
--t_size frames.  Every sample gets six dimensionless descriptors (bone-length variation, left / right asymmetry, speed,
acceleration, jerk, share of still steps); per class and descriptor the score is the Wasserstein-1 distance between the real
and the generated values.  Printed: the six class means of W1 (smaller is better) and both sides' mean descriptors;
--per_class_table adds one row per class.  --unconditional scores all selected samples as one set.  On h36m (2-D
projections) bone_cv and asymmetry are not zero for real data either: read them against the real side's means.

    python tools/kinematics_actions.py --data_real train_data.npy --labels_real train_label.pkl \\
        --data_fake gen_data.npy --labels_fake gen_label.pkl --t_size 64 --dataset h36m --per_class 100"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.metrics import KIN_NAMES, kinematics, select_reference_samples  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_real", type=str, required=True, help="path to real data")
    ap.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    ap.add_argument("--data_fake", type=str, required=True, help="path to fake data")
    ap.add_argument("--labels_fake", type=str, required=True, help="path to fake labels")
    ap.add_argument("--t_size", type=int, default=64, help="Temporal dimension")
    ap.add_argument("--dataset", type=str, default="h36m", help="dataset to evaluate")
    ap.add_argument("--per_class", type=int, default=100, help="samples of every class, of each set")
    ap.add_argument("--still_eps", type=float, default=1e-3, help="a step shorter than still_eps mean bone lengths is still")
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
    out = kinematics(torch.from_numpy(fake).to(dev), torch.from_numpy(real).to(dev), fake_lab, real_lab,
                     dataset="h36m" if opt.dataset == "h36m" else "ntu", still_eps=opt.still_eps)
    out = {k: v.cpu() for k, v in out.items()}
    if opt.per_class_table:
        print("class " + " ".join("%12s" % ("w1_" + nm) for nm in KIN_NAMES))
        for c, row in enumerate(out["w1"].tolist()):
            print("%5d " % c + " ".join("%12.6g" % v for v in row))
    w1 = out["w1_mean"].tolist()
    for side in ("real", "fake"):
        print("mean_%s " % side + " ".join("%s %.6g" % (nm, v) for nm, v in zip(KIN_NAMES, out["mean_" + side].mean(0).tolist())))
    bad = (int(out["nonfinite"].sum()), int(out["degenerate_real"].sum() + out["degenerate"].sum()))
    if any(bad):
        print("samples with a non-finite descriptor: %d, with every bone of length zero: %d" % bad)
    print(" ".join("w1_%s %.6g" % (nm, v) for nm, v in zip(KIN_NAMES, w1)))
    return tuple(w1)


if __name__ == "__main__":
    main()
