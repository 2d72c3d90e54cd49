#!/usr/bin/env python3
"""sha256 digests of what the replay loops compute, to compare two trees bit for bit on one GPU (record:
profiles/replay_refactor.log).  Toy Human3.6M shapes, synthetic data, fixed seeds, batch 4, 7 batches per epoch:
  * TrainLoop (n_critic 2, ema_decay 0.999, eval_interval 3, 2 pairs) for --steps iterations: flat parameters, moments, Adam
    counter, weight average and module buffers of G and D, both loss arrays, the evaluation record;
  * ClassifierLoop for --steps iterations: flat parameters, moments, Adam counter, loss and accuracy arrays;
  * three Sampler.next() rounds on the trained generator.
One line per digest, "<name> <sha256>".  ``<name>.all`` covers every iteration of this process, ``<name>.tail`` the last six: a
run resumed from --load at iteration 6 has the same lines as an uninterrupted one, the ``.all`` ones apart.
    python tools/replay_digest.py [--root TREE] [--steps 12] [--save STATE] [--load STATE]"""
import argparse
import hashlib
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package runs")
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--save", default=None, help="write both loops' state_dict() there after the last iteration")
ap.add_argument("--load", default=None, help="load both loops' state from there before the first iteration")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.classifier import Classifier  # noqa: E402
from kinetic_gan_amd.classify import ClassifierLoop  # noqa: E402
from kinetic_gan_amd.discriminator import Discriminator  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.sample import Sampler  # noqa: E402
from kinetic_gan_amd.train import TrainLoop  # noqa: E402

B, C, T_RAW, T, V, L, N, TAIL = 4, 2, 40, 32, 16, 10, 31, 6


def say(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        h.update(np.ascontiguousarray(a).tobytes())
    print("%-28s %s" % (name, h.hexdigest()), flush=True)


def say_flat(name, f):
    for k, t in (("flat", f.flat), ("exp_avg", f.exp_avg), ("exp_avg_sq", f.exp_avg_sq), ("adam_step", f.step)):
        say("%s.%s" % (name, k), t)


def say_losses(name, pair):
    for k, a in zip(("first", "second"), pair):
        say("%s.%s.all" % (name, k), a)
        say("%s.%s.tail" % (name, k), a[-TAIL:])


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    assert kinetic_gan_amd.__file__.startswith(os.path.abspath(opt.root)), kinetic_gan_amd.__file__
    state = torch.load(opt.load, weights_only=False) if opt.load else None
    rs = np.random.RandomState(3)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "x.npy"), rs.rand(N, C, T_RAW, V).astype(np.float32))
        with open(os.path.join(d, "y.pkl"), "wb") as f:
            pickle.dump((["s%d" % i for i in range(N)], [i % L for i in range(N)]), f)
        feeder = Feeder(os.path.join(d, "x.npy"), os.path.join(d, "y.pkl"), dataset="h36m", mmap=False)
    torch.manual_seed(1234)
    G = Generator(512, C, L, T, 4, dataset="h36m").to(dev)
    D = Discriminator(C, L, T, 512, dataset="h36m").to(dev)
    clf = Classifier(C, L, T, dataset="h36m").to(dev)

    loop = TrainLoop(G, D, feeder, B, T, n_critic=2, seed=5, ema_decay=0.999, eval_interval=3, eval_pairs=2)
    if state is not None:
        loop.load_state_dict(state["train"])
    for _ in range(opt.steps):
        loop.step()
    pair = loop.losses()
    print("# TrainLoop at iteration %d (epoch %d)" % (loop.step_count, loop.epoch))
    for name, f, m in (("train.G", loop.trainer.fG, G), ("train.D", loop.trainer.fD, D)):
        say_flat(name, f)
        say(name + ".buffers", *[b for _, b in m.named_buffers()])
    say("train.G.ema", loop.trainer.fG.ema)
    say_losses("train.losses", pair)
    rec = loop.evaluator.records()
    say("train.eval.records", rec["iteration"], rec["scores"], rec["improved"])
    say("train.eval.best", loop.evaluator.best_val, loop.evaluator.best_iter, loop.evaluator.snap_flat)

    cl = ClassifierLoop(clf, feeder, B, T, seed=6)
    if state is not None:
        cl.load_state_dict(state["classifier"])
    for _ in range(opt.steps):
        cl.step()
    print("# ClassifierLoop at iteration %d" % cl.step_count)
    say_flat("classifier", cl.flat)
    say_losses("classifier.losses", cl.losses())

    s = Sampler(G, qtd=2, seed=7)
    outs = [s.next()[0].clone() for _ in range(3)]
    say("sampler.rounds", *outs)
    if opt.save:
        torch.save({"train": loop.state_dict(), "classifier": cl.state_dict()}, opt.save)
        print("# state of iteration %d written to %s" % (loop.step_count, os.path.basename(opt.save)))


if __name__ == "__main__":
    main()
