#!/usr/bin/env python
"""The reference's training program (kinetic-gan.py) on ``kinetic_gan_amd.train.TrainLoop``: same flags, same progress
line, same outputs (``<out>/actions/<batches_done>.npy``, ``<out>/plot_loss.mat``, ``<out>/models/generator_<n>.pth`` /
``discriminator_<n>.pth``) - every iteration one hipGraph replay whose first launch draws the iteration's batch and
random inputs on the device.  Extra flags: ``--seed`` (shuffling and every random input), ``--resume FILE`` (a
``loop_state.pth`` written by an earlier run: continues it bit for bit), ``--no-graph`` (the same launches, eagerly),
``--out``, ``--log_interval``, ``--ema_decay D`` / ``--ema_warmup W`` (a moving average of the generator's weights, updated
inside the generator's Adam launch: also writes ``models/generator_ema_<n>.pth`` and ``actions_ema/<n>.npy``),
``--eval_interval N`` (every N iterations the generator - and its average - is scored with the MMD protocol on the device,
inside the loop: writes ``metrics.csv`` and ``models/generator_best.pth``, the weights of the best-scoring evaluation;
``--eval_pairs``, ``--eval_select``, ``--eval_trunc``, ``--eval_trunc_mode``, ``--eval_data_path`` / ``--eval_label_path``;
``--eval_prdc N`` also scores precision / recall / density / coverage on N samples per class with ``--eval_prdc_k`` neighbours:
eight more ``metrics.csv`` columns, and ``--eval_select`` may name one, e.g. ``ema/coverage``; ``--eval_frechet N`` also scores
the Frechet pose / motion distance on N samples per class, ``--eval_frechet_modes`` choosing between them: up to four more
columns, and ``--eval_select`` may name one, e.g. ``ema/motion_fd``; ``--eval_classifier classifier_<n>.pth`` with
``--eval_classifier_samples N`` also scores accuracy, feature Frechet distance, diversity and multimodality under a classifier
trained by tools/train_classifier.py on N samples per class - ``--eval_classifier_batch``, ``--eval_diversity_pairs``,
``--eval_multimodality_pairs``: eight more columns, and ``--eval_select`` may name ``<live|ema>/accuracy`` or
``<live|ema>/feature_fd``; a checkpoint trained on another dataset, shape or normalisation is refused;
``--eval_memorisation features`` (the --eval_classifier round's features) or ``--eval_memorisation raw`` with
``--eval_memorisation_samples P`` (and ``--eval_memorisation_method gram`` for the matrix-core pre-filter) also scores authenticity and label agreement against the training set on the device: four
more columns, ``--eval_select`` may name ``<live|ema>/label_agreement``; a dataset that is streamed - ``--max_resident_bytes``
or half the free device memory is too small for it - is refused at start-up; ``--eval_kinematics P`` also scores kinematic
plausibility on P samples per class - the W1 distance of bone-length variation, asymmetry, speed, acceleration, jerk and
stillness to the real samples', ``--eval_kinematics_still_eps`` the stillness threshold, DESIGN.md 26: twelve more columns,
and ``--eval_select`` may name one, e.g. ``ema/jerk``)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kinetic_gan_amd  # noqa: E402,F401
from kinetic_gan_amd.classifier import check_classifier_meta, load_classifier  # noqa: E402
from kinetic_gan_amd.discriminator import Discriminator  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.train import TrainLoop, norm_constants  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n_epochs", type=int, default=1200, help="number of epochs of training")
    p.add_argument("--batch_size", type=int, default=32, help="size of the batches")
    p.add_argument("--lr", type=float, default=0.0002, help="adam: learning rate")
    p.add_argument("--b1", type=float, default=0.5, help="adam: decay of first order momentum of gradient")
    p.add_argument("--b2", type=float, default=0.999, help="adam: decay of first order momentum of gradient")
    p.add_argument("--n_cpu", type=int, default=8, help="accepted for compatibility (batches are gathered on the device)")
    p.add_argument("--latent_dim", type=int, default=512, help="dimensionality of the latent space")
    p.add_argument("--mlp_dim", type=int, default=4, help="mapping network depth")
    p.add_argument("--n_classes", type=int, default=60, help="number of classes for dataset")
    p.add_argument("--t_size", type=int, default=64, help="size of each temporal dimension")
    p.add_argument("--v_size", type=int, default=25, help="size of each spatial dimension (vertices)")
    p.add_argument("--channels", type=int, default=3, help="number of channels (coordinates)")
    p.add_argument("--n_critic", type=int, default=5, help="number of training steps for discriminator per generator's iteration")
    p.add_argument("--lambda_gp", type=int, default=10, help="Loss weight for gradient penalty in WGAN-GP Loss")
    p.add_argument("--sample_interval", type=int, default=5000, help="interval between action sampling")
    p.add_argument("--checkpoint_interval", type=int, default=10000, help="interval between model saving")
    p.add_argument("--dataset", type=str, default="ntu", help="dataset")
    p.add_argument("--data_path", type=str, required=True, help="path to data")
    p.add_argument("--label_path", type=str, required=True, help="path to label")
    p.add_argument("--seed", type=int, default=0, help="seed of the epoch permutations and of every random input")
    p.add_argument("--resume", type=str, default=None, help="loop_state.pth of an earlier run to continue")
    p.add_argument("--no-graph", action="store_true", help="run the iteration eagerly instead of replaying hipGraphs")
    p.add_argument("--out", type=str, default="runs/kinetic-gan", help="run directory")
    p.add_argument("--log_interval", type=int, default=100, help="iterations between progress lines (one loss read each)")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="decay of an exponential moving average of the generator's weights (0 = off; e.g. 0.999)")
    p.add_argument("--ema_warmup", type=float, default=10.0,
                   help="ramp of the average's decay: min(ema_decay, (1 + s) / (ema_warmup + s)) at generator step s; 0 = no ramp")
    p.add_argument("--eval_interval", type=int, default=0,
                   help="iterations between evaluations inside the loop (0 = off): MMD of generated against real samples")
    p.add_argument("--eval_pairs", type=int, default=10, help="(fake, real) pairs per class of one evaluation")
    p.add_argument("--eval_select", type=str, default=None,
                   help="the score that picks the best weights, '<live|ema>/<avg|joint>' (default: ema/avg with --ema_decay, else live/avg); "
                        "with --eval_prdc also '<live|ema>/<precision|recall|density|coverage>' (larger is better); "
                        "with --eval_frechet also '<live|ema>/<pose_fd|motion_fd>' (smaller is better); "
                        "with --eval_classifier also '<live|ema>/accuracy' (larger is better) and '<live|ema>/feature_fd' "
                        "(smaller is better); "
                        "with --eval_kinematics also '<live|ema>/<bone_cv|asymmetry|speed|accel|jerk|still>' (smaller is better)")
    p.add_argument("--eval_prdc", type=int, default=0,
                   help="samples per class on which an evaluation also scores precision / recall / density / coverage (0 = off)")
    p.add_argument("--eval_prdc_k", type=int, default=5, help="neighbours of --eval_prdc")
    p.add_argument("--eval_frechet", type=int, default=0,
                   help="samples per class on which an evaluation also scores the Frechet pose / motion distance (0 = off)")
    p.add_argument("--eval_frechet_modes", type=str, nargs="+", default=["pose", "motion"], choices=["pose", "motion"],
                   help="the Frechet distances of --eval_frechet")
    p.add_argument("--eval_classifier", type=str, default=None,
                   help="classifier_<n>.pth of tools/train_classifier.py: an evaluation also scores accuracy, feature Frechet "
                        "distance, diversity and multimodality (needs --eval_classifier_samples)")
    p.add_argument("--eval_classifier_samples", type=int, default=0,
                   help="samples per class of the --eval_classifier scores (0 = off; e.g. 100)")
    p.add_argument("--eval_classifier_batch", type=int, default=512, help="samples per classifier pass of an evaluation")
    p.add_argument("--eval_diversity_pairs", type=int, default=200, help="pairs of the diversity score")
    p.add_argument("--eval_multimodality_pairs", type=int, default=20, help="pairs per class of the multimodality score")
    p.add_argument("--eval_memorisation", type=str, default=None, choices=["features", "raw"],
                   help="an evaluation also scores authenticity and label agreement against the training set: 'features' in the "
                        "--eval_classifier round's feature space (the per-interval form), 'raw' on the samples themselves "
                        "(needs --eval_memorisation_samples; at NTU one search of the whole training set per generator)")
    p.add_argument("--eval_memorisation_samples", type=int, default=0,
                   help="samples per class of --eval_memorisation raw")
    p.add_argument("--eval_memorisation_method", type=str, default="exact", choices=["exact", "gram"],
                   help="gram: the memorisation searches through kg_nn_gram, the matrix-core pre-filter with exact re-score "
                        "(the same columns, DESIGN.md 24)")
    p.add_argument("--eval_kinematics", type=int, default=0,
                   help="samples per class on which an evaluation also scores kinematic plausibility: the W1 distance of six "
                        "per-sample descriptors to the real samples' (0 = off; e.g. 100)")
    p.add_argument("--eval_kinematics_still_eps", type=float, default=1e-3,
                   help="a joint step shorter than this share of the sample's mean bone length counts as still")
    p.add_argument("--max_resident_bytes", type=int, default=None,
                   help="device memory the cropped dataset may take to stay resident (default: half of what is free); a larger "
                        "dataset is streamed")
    p.add_argument("--eval_trunc", type=float, default=None, help="truncation factor of the evaluation's samples")
    p.add_argument("--eval_trunc_mode", type=str, default="-", help="'-' none, 'z' or 'w' truncation of the evaluation's samples")
    p.add_argument("--eval_data_path", type=str, default=None, help="real samples of the evaluation (default: the training data)")
    p.add_argument("--eval_label_path", type=str, default=None, help="labels of --eval_data_path")
    return p.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("tools/train.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    os.makedirs(opt.out, exist_ok=True)
    with open(os.path.join(opt.out, "config.txt"), "w") as f:
        f.write(os.path.basename(__file__) + "|" + str(opt))
    torch.manual_seed(opt.seed)
    G = Generator(opt.latent_dim, opt.channels, opt.n_classes, opt.t_size, opt.mlp_dim, dataset=opt.dataset).to(dev)
    D = Discriminator(opt.channels, opt.n_classes, opt.t_size, opt.latent_dim, dataset=opt.dataset).to(dev)
    feeder = Feeder(opt.data_path, opt.label_path, dataset=opt.dataset)
    if feeder.V != opt.v_size or feeder.C != opt.channels:
        raise SystemExit("data is (C=%d, V=%d) but --channels %d --v_size %d" % (feeder.C, feeder.V, opt.channels, opt.v_size))
    eval_data = None
    if opt.eval_interval and opt.eval_data_path:
        if not opt.eval_label_path:
            raise SystemExit("--eval_data_path needs --eval_label_path")
        eval_data = Feeder(opt.eval_data_path, opt.eval_label_path, dataset=opt.dataset)
    clf = None
    if opt.eval_interval and opt.eval_classifier and opt.eval_classifier_samples:
        clf, meta = load_classifier(opt.eval_classifier, dev)
        try:
            for f in [feeder] + ([] if eval_data is None else [eval_data]):
                scale, shift = norm_constants(f)
                check_classifier_meta(meta, dict(dataset=opt.dataset, n_classes=opt.n_classes, in_channels=opt.channels,
                                                 t_size=min(opt.t_size, f.T), scale=scale, shift=shift))
        except ValueError as e:
            raise SystemExit("--eval_classifier %s: %s" % (opt.eval_classifier, e))
    try:
        loop = _make_loop(opt, G, D, feeder, eval_data, clf)
    except ValueError as e:
        if opt.eval_memorisation and "eval_memorisation" in str(e):
            raise SystemExit("--eval_memorisation %s: %s" % (opt.eval_memorisation, e))
        raise
    print("dataset: %d samples, %d batches per epoch, %s (%.1f MB cropped)" % (
        len(feeder), loop.bpe, "streamed" if loop.streaming else "resident on the device", loop.resident.nbytes / 1e6))
    if opt.resume:
        loop.load_state_dict(torch.load(opt.resume, weights_only=False))
        print("resumed at iteration %d (epoch %d)" % (loop.step_count, loop.epoch))
    loop.run(opt.n_epochs, opt.sample_interval, opt.checkpoint_interval, opt.out, log_interval=opt.log_interval,
             state_path=os.path.join(opt.out, "loop_state.pth"))


def _make_loop(opt, G, D, feeder, eval_data, clf):
    return TrainLoop(G, D, feeder, opt.batch_size, opt.t_size, n_critic=opt.n_critic, seed=opt.seed, lr=opt.lr, b1=opt.b1,
                     b2=opt.b2, lambda_gp=float(opt.lambda_gp), use_graph=not opt.no_graph,
                     ring_len=max(4096, opt.log_interval), ema_decay=opt.ema_decay or None, ema_warmup=opt.ema_warmup,
                     eval_interval=opt.eval_interval or None, eval_pairs=opt.eval_pairs, eval_select=opt.eval_select,
                     eval_trunc=opt.eval_trunc, eval_trunc_mode=opt.eval_trunc_mode, eval_data=eval_data,
                     eval_prdc=opt.eval_prdc, eval_prdc_k=opt.eval_prdc_k, eval_frechet=opt.eval_frechet,
                     eval_frechet_modes=tuple(opt.eval_frechet_modes), eval_classifier=clf,
                     eval_classifier_samples=opt.eval_classifier_samples, eval_classifier_batch=opt.eval_classifier_batch,
                     eval_diversity_pairs=opt.eval_diversity_pairs, eval_multimodality_pairs=opt.eval_multimodality_pairs,
                     eval_memorisation=opt.eval_memorisation, eval_memorisation_samples=opt.eval_memorisation_samples,
                     eval_memorisation_method=opt.eval_memorisation_method,
                     eval_kinematics=opt.eval_kinematics, eval_kinematics_still_eps=opt.eval_kinematics_still_eps,
                     max_resident_bytes=opt.max_resident_bytes)


if __name__ == "__main__":
    main()
