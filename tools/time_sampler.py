#!/usr/bin/env python3
"""Speed of one generation round (record: profiles/sampler_time.log).

Three paths alternate round by round in one process, each round timed with device events after a warm-up of every shape:
  (a) ``sample_actions(..., keep_on_device=True)``: host-drawn latents, the stock mapping network for the truncation
      mean, BatchNorm folded per call, the autograd ops block by block;
  (b) ``Sampler(use_graph=False).next()``: the inference schedule, launched eagerly;
  (c) ``Sampler(use_graph=True).next()``: the same launches as one hipGraph replay.
Sizes are what a user runs: ntu with 10 samples per class (600 per round) with W-space truncation at 0.95 (the
reference's defaults) and without truncation, h36m with 10 per class (100 per round, W-space truncation).  Per size:
the median over ``--rounds`` rounds, ``--reps`` repetitions, and the spread between the repetitions' medians.
    python tools/time_sampler.py [--rounds 200] [--reps 3] [--log FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.sample import Sampler, sample_actions  # noqa: E402

SIZES = [("ntu", dict(latent=512, channels=3, n_classes=60, t_size=64), "w", 0.95),
         ("ntu", dict(latent=512, channels=3, n_classes=60, t_size=64), "-", None),
         ("h36m", dict(latent=512, channels=2, n_classes=10, t_size=32), "w", 0.95)]
QTD = 10


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", type=str, default=None)
    opt = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)
    say("time_sampler: %s, torch %s, rounds %d, reps %d" % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds, opt.reps))
    for ds, c, mode, trunc in SIZES:
        torch.manual_seed(1234)
        np.random.seed(1)
        G = Generator(c["latent"], c["channels"], c["n_classes"], c["t_size"], 4, dataset=ds).to(dev)
        with torch.no_grad():       # non-trivial running statistics and noise weights
            for name, b in G.named_buffers():
                if name.endswith("running_var"):
                    b.uniform_(0.5, 1.5)
                elif name.endswith("running_mean"):
                    b.uniform_(-0.2, 0.2)
            for blk in G.st_gcn_networks:
                blk.noise.weight.uniform_(-0.3, 0.3)
        eager = Sampler(G, qtd=QTD, seed=1, trunc=trunc, trunc_mode=mode, use_graph=False)
        replay = Sampler(G, qtd=QTD, seed=1, trunc=trunc, trunc_mode=mode, use_graph=True)
        paths = [("a sample_actions", lambda: sample_actions(G, c["n_classes"], c["latent"], gen_qtd=QTD, qtd=QTD, trunc=trunc,
                                                             trunc_mode=mode, keep_on_device=True)),
                 ("b Sampler eager", eager.next),
                 ("c Sampler replay", replay.next)]
        for _ in range(opt.warmup):
            for _, fn in paths:
                fn()
        torch.cuda.synchronize()
        meds = {name: [] for name, _ in paths}
        for rep in range(opt.reps):
            ts = {name: [] for name, _ in paths}
            for _ in range(opt.rounds):
                for name, fn in paths:
                    ts[name].append(timed(fn))
            for name in ts:
                meds[name].append(statistics.median(ts[name]))
        n = QTD * c["n_classes"]
        say("%s, %d samples per round, trunc_mode %r%s" % (ds, n, mode, "" if trunc is None else " at %.2f" % trunc))
        for name, _ in paths:
            m = meds[name]
            say("  (%s)  median ms per round, per repetition: %s | mean %.3f | spread %.3f (%.1f %%)" % (
                name, " ".join("%.3f" % v for v in m), statistics.mean(m), max(m) - min(m), 100 * (max(m) - min(m)) / statistics.mean(m)))
        a, b_, c_ = (statistics.mean(meds[name]) for name, _ in paths)
        worst = max(max(m) - min(m) for m in meds.values())
        say("  a / c = %.2f, a / b = %.2f, b / c = %.2f; a - c = %.3f ms against the largest spread %.3f ms" % (
            a / c_, a / b_, b_ / c_, a - c_, worst))
        del eager, replay
    if opt.log:
        with open(opt.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
