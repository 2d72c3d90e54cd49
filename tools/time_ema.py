#!/usr/bin/env python3
"""Cost of the generator weight average (record: profiles/ema_time.log).

NTU-60 shapes, 64 samples, a generator step in every iteration (n_critic = 1), a resident synthetic dataset of 64 batches -
the configuration of tools/time_train_loop.py.  Three captured loops alternate in one process, ``--rounds`` rounds each,
event-timed blocks of 10 replays, median ms per iteration over 30 blocks:

  (a) TrainLoop without a decay (the launches of a run without --ema_decay);
  (b) TrainLoop(ema_decay=0.999): the average rides on the generator's Adam launch (kg_adam_step_ema);
  (c) the loop of (a) with a stock ``ema.lerp_(flat, 1 - decay)`` captured behind the generator's Adam launch - the
      comparator only (no warm-up ramp), built here, not part of the package.

Reported: the median of the rounds' medians and the spread between rounds (max - min) per loop, (b) - (a) against (c) - (a),
and the optimiser launch alone in its forms (graphs of 20 launches on buffers of the NTU generator's flat length).
    python tools/time_ema.py [--rounds 3] [--log FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd.train import ResidentDataset, TrainLoop  # noqa: E402
from time_train_loop import BATCH, CFG, SyntheticFeeder, models, time_loop  # noqa: E402

DECAY = 0.999


def with_stock_lerp(loop):
    """comparator (c): a separate average moved by a stock lerp_ launch right behind the generator's Adam launch"""
    f = loop.trainer.fG
    ema = f.flat.detach().clone()
    inner = f.allreduce_and_step

    def stepped(*a, **k):
        inner(*a, **k)
        ema.lerp_(f.flat, 1.0 - DECAY)
    f.allreduce_and_step = stepped
    return ema


def time_launches(fn, reps=20, rounds=15):
    """us per launch of fn() from a graph of `reps` launches"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    feeder = SyntheticFeeder(64 * BATCH + 17, CFG["channels"], CFG["t_size"], CFG["v"], CFG["n_classes"])
    data = ResidentDataset(feeder, CFG["t_size"], dev)
    say("device %s; NTU-60 shapes, %d samples per iteration, a generator step in every iteration, %d resident samples" % (
        torch.cuda.get_device_name(0), BATCH, len(feeder)))
    loops = {}
    for name, kw in (("a", {}), ("b", dict(ema_decay=DECAY)), ("c", {})):
        G, D = models(dev)
        loops[name] = TrainLoop(G, D, data, BATCH, CFG["t_size"], n_critic=1, seed=0, **kw)
    stock = with_stock_lerp(loops["c"])
    for loop in loops.values():
        for _ in range(20):
            loop.step()
    label = {"a": "(a) no average", "b": "(b) average on the Adam launch", "c": "(c) stock lerp_ behind the Adam launch"}
    meds = {k: [] for k in loops}
    for r in range(args.rounds):
        for k, loop in loops.items():
            med, lo, hi, _ = time_loop(loop, blocks=30, per_block=10, warmup=5)
            meds[k].append(med)
            say("round %d %-40s median %.4f ms per iteration over 300 replays (blocks of 10: min %.4f, max %.4f)" % (
                r, label[k], med, lo, hi))
    for k, loop in loops.items():
        d, g = loop.losses()
        assert np.isfinite(d).all() and np.isfinite(g).all(), "the timed loop diverged"
    # the three loops started from the same weights and drew the same inputs (a sanity check, not a measurement)
    flat = {k: loop.trainer.fG.flat for k, loop in loops.items()}
    say("live generator weights after %d iterations: (b) == (a) %s, (c) == (a) %s; fused vs stock average (no ramp in the "
        "comparator) max |d| %.3e" % (loops["a"].step_count, torch.equal(flat["a"], flat["b"]), torch.equal(flat["a"], flat["c"]),
                                      (stock - loops["b"].trainer.fG.ema).abs().max().item()))
    m = {k: statistics.median(v) for k, v in meds.items()}
    sp = {k: max(v) - min(v) for k, v in meds.items()}
    for k in loops:
        say("%-40s %.4f ms per iteration (median of %d rounds), spread between rounds %.4f ms" % (label[k], m[k], args.rounds, sp[k]))
    say("(b) - (a) = %+.2f us; (c) - (a) = %+.2f us; larger spread of the two %.2f us: fused %s stock + spread" % (
        (m["b"] - m["a"]) * 1e3, (m["c"] - m["a"]) * 1e3, max(sp["b"], sp["c"]) * 1e3,
        "<=" if m["b"] - m["a"] <= m["c"] - m["a"] + max(sp["b"], sp["c"]) else ">"))
    # the optimiser launch alone
    f = loops["b"].trainer.fG
    n = f.flat.numel()
    p, g, mm, e = torch.randn(n, device=dev), torch.randn(n, device=dev), 0.1 * torch.randn(n, device=dev), torch.randn(n, device=dev)
    v = torch.rand(n, device=dev) * 0.01
    step = torch.full((1,), 100, dtype=torch.int32, device=dev)
    us_plain = time_launches(lambda: nv.adam_step(p, g, mm, v, 2e-4, 0.5, 0.999, 1e-8, step, 1.0, zero_grad=True))
    us_ema = time_launches(lambda: nv.adam_step_ema(p, g, mm, v, e, 2e-4, 0.5, 0.999, 1e-8, step, 1.0, True, DECAY, 10.0))
    us_lerp = time_launches(lambda: e.lerp_(p, 1.0 - DECAY))
    say("optimiser launch alone, %d parameters (graphs of 20): kg_adam_step_fused %.2f us (%.0f GB/s over 8 streams), "
        "kg_adam_step_ema %.2f us (%.0f GB/s over 10 streams), stock lerp_ %.2f us (%.0f GB/s over 3 streams); "
        "fused adds %.2f us, separate launch adds %.2f us" % (
            n, us_plain, 8 * 4 * n / us_plain / 1e3, us_ema, 10 * 4 * n / us_ema / 1e3, us_lerp, 3 * 4 * n / us_lerp / 1e3,
            us_ema - us_plain, us_lerp))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
