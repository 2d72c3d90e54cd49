#!/usr/bin/env python3
"""Recognition accuracy and feature Frechet distance of generated actions under a trained action classifier
(metrics.classifier_scores): the protocol of Action2Motion / ACTOR with a classifier trained on the user's own
data by tools/train_classifier.py.

The file pairs tools/generate.py writes and tools/mmd_actions.py reads.  Real data is normalised with the constants stored in
the checkpoint (the training set's); generated data is used as it is - the generator emits normalised samples.  Prints
``accuracy`` (generated samples against their conditioning labels), ``accuracy_real``, ``feature_fd`` (all generated against all
real features) and ``feature_fd_class_mean`` (per class on the first --per_class samples of every class); --per_class_table
adds one row per class.  With --diversity_pairs and --multimodality_pairs above 0 it also prints ``diversity`` /
``multimodality`` of the generated and of the real set (means of feature distances over fixed random pairs, --pair_seed)
and --per_class_table gains the per-class accuracy column.

    python tools/classify_actions.py --model runs/classifier/classifier_3000.pth --data_real train_data.npy \\
        --labels_real train_label.pkl --data_fake gen_data.npy --labels_fake gen_label.pkl --per_class 100"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.classifier import load_classifier  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.metrics import classifier_scores  # noqa: E402


def samples(feeder, t_size, scale=1.0, shift=0.0):
    raw = feeder.data[:, :, :t_size, :, 0] if feeder.dataset == "ntu" and feeder.data.ndim == 5 else feeder.data[:, :, :t_size]
    x = torch.from_numpy(np.array(raw, dtype=np.float32))      # (a copy: the memory map is read-only)
    return x * np.float32(scale) + np.float32(shift), np.asarray(feeder.label, dtype=np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", type=str, required=True, help="classifier_<n>.pth of tools/train_classifier.py")
    ap.add_argument("--data_real", type=str, required=True, help="path to real data")
    ap.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    ap.add_argument("--data_fake", type=str, required=True, help="path to fake data")
    ap.add_argument("--labels_fake", type=str, required=True, help="path to fake labels")
    ap.add_argument("--per_class", type=int, default=None, help="samples of every class for the per-class Frechet distance")
    ap.add_argument("--per_class_table", action="store_true", help="print one row per class")
    ap.add_argument("--batch", type=int, default=512, help="samples per classifier pass")
    ap.add_argument("--diversity_pairs", type=int, default=0,
                    help="pairs of the diversity score (0: off; Action2Motion uses 200); needs --multimodality_pairs")
    ap.add_argument("--multimodality_pairs", type=int, default=0,
                    help="pairs per class of the multimodality score (0: off; Action2Motion uses 20); needs --diversity_pairs")
    ap.add_argument("--pair_seed", type=int, default=0, help="seed of the pair tables (metrics.cls_pair_tables)")
    opt = ap.parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("tools/classify_actions.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    clf, meta = load_classifier(opt.model, dev)
    real_f = Feeder(opt.data_real, opt.labels_real, norm=False, dataset=meta["dataset"])
    fake_f = Feeder(opt.data_fake, opt.labels_fake, norm=False, dataset=meta["dataset"])
    real, real_lab = samples(real_f, meta["t_size"], meta["scale"], meta["shift"])       # the checkpoint's constants
    fake, fake_lab = samples(fake_f, meta["t_size"])                                      # already normalised
    print(tuple(real.shape), "real")
    print(tuple(fake.shape), "fake")
    # per class: the first --per_class samples of every class (default: as many as the smallest class of either set holds)
    counts = np.concatenate([np.bincount(l, minlength=meta["n_classes"]) for l in (real_lab, fake_lab)])
    per_class = opt.per_class if opt.per_class is not None else int(counts.min())
    class_fd = per_class >= 2
    if not class_fd:
        print("a class holds fewer than 2 samples: no per-class Frechet distance")
    pairs = opt.diversity_pairs > 0 or opt.multimodality_pairs > 0
    s = classifier_scores(clf, fake, fake_lab, real, real_lab, per_class=per_class, batch=opt.batch, class_fd=class_fd,
                          diversity_pairs=opt.diversity_pairs, multimodality_pairs=opt.multimodality_pairs, pair_seed=opt.pair_seed)
    fd = float(s["feature_fd"].cpu())
    fd_c = float(s["feature_fd_class_mean"].cpu()) if class_fd else float("nan")
    if opt.per_class_table and (class_fd or pairs):
        cols = [("feature_fd", s["feature_fd_per_class"].cpu().tolist())] if class_fd else []
        if pairs:
            cor, cnt = s["correct_per_class"].cpu().tolist(), s["count_per_class"].cpu().tolist()
            cols.append(("accuracy", [c / n if n else float("nan") for c, n in zip(cor, cnt)]))
        print("class" + "".join(" %12s" % name for name, _ in cols))
        for c in range(len(cols[0][1])):
            print("%5d" % c + "".join(" %12.6f" % v[c] for _, v in cols))
    print("accuracy %.6f accuracy_real %.6f feature_fd %.6f feature_fd_class_mean %.6f" % (s["accuracy"], s["accuracy_real"], fd, fd_c))
    if pairs:
        print("diversity %.6f diversity_real %.6f multimodality %.6f multimodality_real %.6f" % tuple(
            float(s[k].cpu()) for k in ("diversity", "diversity_real", "multimodality", "multimodality_real")))
    return s["accuracy"], s["accuracy_real"], fd, fd_c


if __name__ == "__main__":
    main()
