#!/usr/bin/env python3
"""Nearest training sample of every generated action and the memorisation scores built on it, on the kg_nn HIP kernels
(metrics.nearest / memorisation / nn_two_sample).

The file flags and the selection of tools/prdc_actions.py - real data through Feeder(norm=True), fake data (the .npy / .pkl
pair sample.py's outputs are saved as) through Feeder(norm=False), the first --per_class samples of every class cropped to
--t_size frames - plus the TRAINING set (--data_train / --labels_train, Feeder(norm=True)), which is put on the device whole
and searched in place.  Printed: authenticity and 1-NN label agreement of the generated samples against the training set,
the same two numbers for the selected real samples as queries (pass a set the generator never saw: what a perfect
generator scores) and the class means of the leave-one-out 1-NN two-sample test between the selected fake and real samples
(ideal 0.5; acc_fake -> 0 means copies).  --pairs_out writes one row (generated index, train index, d2) per generated
sample and each of its --k nearest training samples as a float64 .npy, for the visualisation scripts.
--classifier classifier_<n>.pth (tools/train_classifier.py; --classifier_batch samples per pass) also prints
feature_authenticity / feature_label_agreement and their real_ twins: the same scores in the classifier's feature space
(metrics.memorisation_features), all three sets going through Classifier.features in chunks; a checkpoint
trained on another dataset, shape or normalisation is refused.

    python tools/nearest_actions.py --data_real val_data.npy --labels_real val_label.pkl \\
        --data_fake gen_data.npy --labels_fake gen_label.pkl --data_train train_data.npy --labels_train train_label.pkl \\
        --t_size 64 --dataset ntu --k 5 --per_class 100 --pairs_out pairs.npy"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.classifier import check_classifier_meta, load_classifier  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.metrics import (NN_TWO_SAMPLE_NAMES, memorisation, memorisation_features, nearest,  # noqa: E402
                                     nn_two_sample, select_reference_samples)
from kinetic_gan_amd.train import ResidentDataset, norm_constants  # noqa: E402


def features(clf, x, batch, affine=None):
    """(n, F) features of the samples x (n, C, T, V) on the device, ``batch`` at a time; ``affine``: (scale, shift) of samples
    that are not normalised yet"""
    out = []
    with torch.no_grad():
        for lo in range(0, x.shape[0], batch):
            chunk = x[lo:lo + batch]
            if affine is not None:
                chunk = chunk * affine[0] + affine[1]
            out.append(clf.features(chunk))
    return torch.cat(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_real", type=str, required=True, help="path to real data")
    ap.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    ap.add_argument("--data_fake", type=str, required=True, help="path to fake data")
    ap.add_argument("--labels_fake", type=str, required=True, help="path to fake labels")
    ap.add_argument("--data_train", type=str, required=True, help="path to the training data the generator saw")
    ap.add_argument("--labels_train", type=str, required=True, help="path to the training labels")
    ap.add_argument("--t_size", type=int, default=64, help="Temporal dimension")
    ap.add_argument("--dataset", type=str, default="h36m", help="dataset to evaluate")
    ap.add_argument("--k", type=int, default=1, help="nearest training samples written to --pairs_out")
    ap.add_argument("--per_class", type=int, default=100, help="samples of every class, of each set")
    ap.add_argument("--pairs_out", type=str, default=None, help=".npy of (generated index, train index, d2) rows")
    ap.add_argument("--classifier", type=str, default=None,
                    help="classifier_<n>.pth of tools/train_classifier.py: also score in its feature space")
    ap.add_argument("--classifier_batch", type=int, default=512, help="samples per classifier pass")
    ap.add_argument("--method", type=str, default="exact", choices=["exact", "gram"],
                    help="gram: every search through kg_nn_gram, the matrix-core pre-filter with exact re-score - the same "
                         "scores and pairs (DESIGN.md 24); the certified / fallback row counts are printed")
    opt = ap.parse_args(argv)
    print(opt)

    real_f = Feeder(opt.data_real, opt.labels_real, norm=True, dataset=opt.dataset)     # normalised to [-1, 1]
    fake_f = Feeder(opt.data_fake, opt.labels_fake, norm=False, dataset=opt.dataset)    # already normalised
    train_f = Feeder(opt.data_train, opt.labels_train, norm=True, dataset=opt.dataset)
    classes = np.arange(10 if opt.dataset == "h36m" else 60)
    real, real_lab, _ = select_reference_samples(real_f, classes, opt.t_size, opt.per_class)
    fake, fake_lab, fake_index = select_reference_samples(fake_f, classes, opt.t_size, opt.per_class)
    print(real.shape, "real")
    print(fake.shape, "fake")
    dev = torch.device("cuda", torch.cuda.current_device())
    train = ResidentDataset(train_f, opt.t_size, dev)
    print(train.shape, "train")
    fake, real = torch.from_numpy(fake).to(dev), torch.from_numpy(real).to(dev)

    mem = memorisation(fake, fake_lab, train, heldout=real, labels_heldout=real_lab, method=opt.method)
    two = nn_two_sample(fake, real, fake_lab, real_lab, method=opt.method)
    if opt.method == "gram":
        print("kg_nn_gram rows (certified, fallback): fake -> train %d %d, real -> train %d %d, train -> train %d %d, two-sample %d %d"
              % (mem["certified"], mem["fallback"], mem["heldout_certified"], mem["heldout_fallback"], mem["train_loo_certified"],
                 mem["train_loo_fallback"], two["certified"].sum(), two["fallback"].sum()))
    scores = dict(authenticity=mem["authenticity"], label_agreement=mem["label_agreement"],
                  real_authenticity=mem["heldout_authenticity"], real_label_agreement=mem["heldout_label_agreement"])
    scores.update(zip(("nn_" + n for n in NN_TWO_SAMPLE_NAMES), two["mean"]))
    if opt.classifier:
        clf, meta = load_classifier(opt.classifier, dev)
        try:
            scale, shift = norm_constants(train_f)
            check_classifier_meta(meta, dict(dataset=opt.dataset, n_classes=len(classes), in_channels=train_f.C,
                                             t_size=train.t, scale=scale, shift=shift))
        except ValueError as e:
            raise SystemExit("--classifier %s: %s" % (opt.classifier, e))
        clf.eval()
        affine = None if (train.scale, train.shift) == (1.0, 0.0) else (train.scale, train.shift)
        feat = memorisation_features(features(clf, fake, opt.classifier_batch), fake_lab,
                                     features(clf, train.data, opt.classifier_batch, affine), train.labels,
                                     features(clf, real, opt.classifier_batch), real_lab, method=opt.method)
        scores.update(feature_authenticity=feat["authenticity"], feature_label_agreement=feat["label_agreement"],
                      real_feature_authenticity=feat["heldout_authenticity"],
                      real_feature_label_agreement=feat["heldout_label_agreement"])
    scores = {n: float(v) for n, v in scores.items()}
    if opt.pairs_out:
        near = nearest(fake, train, k=opt.k, method=opt.method)
        gen_index = np.repeat(fake_index, opt.k)            # the generated sample's index in its file
        pairs = np.stack([gen_index.astype(np.float64), near["index"].reshape(-1).double().cpu().numpy(),
                          near["d2"].reshape(-1).double().cpu().numpy()], axis=1)
        np.save(opt.pairs_out, pairs)
        print("%d pairs -> %s" % (pairs.shape[0], opt.pairs_out))
    print(" ".join("%s %.6f" % (n, v) for n, v in scores.items()))
    return scores


if __name__ == "__main__":
    main()
