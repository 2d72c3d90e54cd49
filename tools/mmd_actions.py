#!/usr/bin/env python3
"""MMD evaluation of generated actions: evaluation/mmd-actions.py of the reference on the kg_mmd HIP kernels.

Same flags as the reference script.  Real data is read through Feeder(norm=True), fake data (the .npy / .pkl pair
sample.py's outputs are saved as) through Feeder(norm=False); the first 100 samples of every class (10 for h36m, 60
otherwise) are selected as the script selects them, cropped to --t_size frames, and scored by calculate_mmd in one
kernel launch plus one finishing launch.  The run-directory bookkeeping of the reference script is left out; the
result is printed.

    python tools/mmd_actions.py --data_real train_data.npy --labels_real train_label.pkl \\
        --data_fake gen_data.npy --labels_fake gen_label.pkl --mmd_mode avg --t_size 64 --dataset h36m"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.metrics import calculate_mmd, select_reference_samples  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_real", type=str, required=True, help="path to real data")
    ap.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    ap.add_argument("--data_fake", type=str, required=True, help="path to fake data")
    ap.add_argument("--labels_fake", type=str, required=True, help="path to fake labels")
    ap.add_argument("--mmd_mode", type=str, default="avg", choices=["avg", "joint"],
                    help="avg for dynamics and joint for whole sequence")
    ap.add_argument("--t_size", type=int, default=64, help="Temporal dimension")
    ap.add_argument("--dataset", type=str, default="h36m", help="dataset to evaluate")
    opt = ap.parse_args(argv)
    print(opt)

    real_f = Feeder(opt.data_real, opt.labels_real, norm=True, dataset=opt.dataset)     # normalised to [-1, 1]
    fake_f = Feeder(opt.data_fake, opt.labels_fake, norm=False, dataset=opt.dataset)    # already normalised
    classes = np.arange(10 if opt.dataset == "h36m" else 60)
    real, real_lab, _ = select_reference_samples(real_f, classes, opt.t_size)
    fake, fake_lab, _ = select_reference_samples(fake_f, classes, opt.t_size)
    assert np.array_equal(real_lab, fake_lab)
    print(real.shape, "real")
    print(fake.shape)
    dev = torch.device("cuda", torch.cuda.current_device())
    result = calculate_mmd(torch.from_numpy(fake).to(dev), torch.from_numpy(real).to(dev), real_lab, opt.mmd_mode)
    print(result.item())
    return result.item()


if __name__ == "__main__":
    main()
