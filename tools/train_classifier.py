#!/usr/bin/env python3
"""Train the action classifier (kinetic_gan_amd.classifier.Classifier: the critic's six st_gcn blocks + a classification head)
on a skeleton dataset with ``kinetic_gan_amd.classify.ClassifierLoop`` - every iteration one hipGraph replay whose first launch
gathers the batch on the device.

Writes ``<out>/classifier_<n>.pth`` every ``--checkpoint_interval`` iterations and at the end - the module's state_dict plus a
``meta`` entry (dataset, in_channels, n_classes, t_size, latent, feat_dim and the Feeder's normalisation constants
(scale, shift)), what tools/classify_actions.py loads - and ``<out>/classifier_log.csv``: iteration, loss, batch accuracy and,
every ``--eval_interval`` iterations when a held-out set is given, its accuracy.

    python tools/train_classifier.py --data_path train_data.npy --label_path train_label.pkl --dataset ntu --t_size 64 \\
        --val_data_path val_data.npy --val_label_path val_label.pkl --out runs/classifier"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kinetic_gan_amd  # noqa: E402,F401
from kinetic_gan_amd.classifier import Classifier  # noqa: E402
from kinetic_gan_amd.classify import ClassifierLoop  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.train import norm_constants  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--data_path", type=str, required=True, help="path to data")
    p.add_argument("--label_path", type=str, required=True, help="path to label")
    p.add_argument("--dataset", type=str, default="ntu", help="dataset (graph): ntu or h36m")
    p.add_argument("--t_size", type=int, default=64, help="frames of a sample (the first t_size are kept)")
    p.add_argument("--batch_size", type=int, default=64, help="size of the batches")
    p.add_argument("--n_epochs", type=int, default=30, help="number of epochs of training")
    p.add_argument("--lr", type=float, default=1e-3, help="adam: learning rate")
    p.add_argument("--seed", type=int, default=0, help="seed of the initial weights and of the epoch permutations")
    p.add_argument("--feat_dim", type=int, default=64, help="width of the feature layer (at most 96)")
    p.add_argument("--latent", type=int, default=512, help="channels of the last st_gcn block")
    p.add_argument("--n_classes", type=int, default=0, help="number of classes (0: largest label + 1)")
    p.add_argument("--val_data_path", type=str, default=None, help="held-out data")
    p.add_argument("--val_label_path", type=str, default=None, help="labels of --val_data_path")
    p.add_argument("--eval_interval", type=int, default=500, help="iterations between held-out evaluations")
    p.add_argument("--checkpoint_interval", type=int, default=2000, help="iterations between checkpoints")
    p.add_argument("--out", type=str, default="runs/classifier", help="run directory")
    p.add_argument("--no-graph", action="store_true", help="run the iteration eagerly instead of replaying a hipGraph")
    return p.parse_args(argv)


def held_out(path, labels, dataset, t_size, scale, shift):
    """(x, y) of the held-out set, normalised with the TRAINING set's constants"""
    f = Feeder(path, labels, norm=False, dataset=dataset)
    raw = f.data[:, :, :t_size, :, 0] if dataset == "ntu" else f.data[:, :, :t_size]
    x = torch.from_numpy(np.array(raw, dtype=np.float32))      # (a copy: the memory map is read-only)
    return x * np.float32(scale) + np.float32(shift), torch.as_tensor(np.asarray(f.label, dtype=np.int64))


def main(argv=None):
    opt = parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_classifier.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    os.makedirs(opt.out, exist_ok=True)
    feeder = Feeder(opt.data_path, opt.label_path, dataset=opt.dataset)
    n_classes = opt.n_classes or int(np.max(feeder.label)) + 1
    t_size = min(opt.t_size, feeder.T)
    scale, shift = norm_constants(feeder)
    torch.manual_seed(opt.seed)
    clf = Classifier(feeder.C, n_classes, t_size, latent=opt.latent, feat_dim=opt.feat_dim, dataset=opt.dataset).to(dev)
    loop = ClassifierLoop(clf, feeder, opt.batch_size, t_size, seed=opt.seed, lr=opt.lr, use_graph=not opt.no_graph)
    meta = dict(dataset=opt.dataset, in_channels=feeder.C, n_classes=n_classes, t_size=t_size, latent=opt.latent,
                feat_dim=opt.feat_dim, scale=scale, shift=shift)
    val = None
    if opt.val_data_path:
        if not opt.val_label_path:
            raise SystemExit("--val_data_path needs --val_label_path")
        val = held_out(opt.val_data_path, opt.val_label_path, opt.dataset, t_size, scale, shift)
    print("dataset: %d samples, %d classes, %d batches per epoch (%.1f MB resident)" % (len(feeder), n_classes, loop.bpe,
                                                                                       loop.resident.nbytes / 1e6))

    def checkpoint(n):
        sd = {k: v.detach().cpu().clone() for k, v in clf.state_dict().items()}
        sd["meta"] = meta
        torch.save(sd, os.path.join(opt.out, "classifier_%d.pth" % n))

    held = {}
    total = opt.n_epochs * loop.bpe
    while loop.step_count < total:
        loop.step()
        n = loop.step_count
        if val is not None and (n % opt.eval_interval == 0 or n == total):
            held[n] = loop.evaluate(*val)["accuracy"]
            loss, acc = loop.losses()
            print("[Iteration %d/%d] [loss %f] [batch accuracy %.3f] [held-out accuracy %.4f]" % (n, total, loss[-1], acc[-1], held[n]))
        if opt.checkpoint_interval > 0 and n % opt.checkpoint_interval == 0 and n != total:
            checkpoint(n)
    checkpoint(loop.step_count)
    loss, acc = loop.losses()
    with open(os.path.join(opt.out, "classifier_log.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["iteration", "loss", "batch_accuracy", "held_out_accuracy"])
        for i, (a, b) in enumerate(zip(loss, acc)):
            w.writerow([i + 1, "%.8g" % a, "%.6g" % b, "%.6g" % held[i + 1] if (i + 1) in held else ""])
    print("final: loss %f, batch accuracy %.3f%s" % (loss[-1], acc[-1],
                                                      ", held-out accuracy %.4f" % held[max(held)] if held else ""))


if __name__ == "__main__":
    main()
