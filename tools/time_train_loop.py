#!/usr/bin/env python3
"""Speed of the training loop (record: profiles/train_loop_time.log).

  (i)   TrainLoop with a generator step in every iteration (n_critic = 1), NTU-60 shapes, 64 samples, a resident
        synthetic dataset of 64 batches: event-timed blocks of 10 replays, median ms per iteration over 30 blocks;
        next to ``ms_per_step`` of ``python bench.py --gpus 1 --steps 30 --warmup 5`` (the same iteration on constant
        inputs, drawn noise included) run as a child process in between - the two alternate three times on one box;
        also the loop over bench.py's own window (5 + 30 iterations on a host clock) and bench.py over 300 steps: the
        chip's clock settles lower in a one-second window than in a 0.1-second one;
  (ii)  kg_step_inputs alone (a graph of 20 launches): us per launch and GB/s of gathered data (read + written);
  (iii) n_critic = 5 (four of five replays are the critic-only graph);
  (iv)  the eager loop (use_graph=False), for contrast.
    python tools/time_train_loop.py [--rounds 3] [--no-bench] [--log FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd.discriminator import Discriminator  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.train import TrainLoop  # noqa: E402

CFG = dict(latent=512, channels=3, n_classes=60, t_size=64, mlp=4, v=25)
BATCH = 64


class SyntheticFeeder:
    """what TrainLoop reads of a Feeder, over an in-memory (N, C, T, V) array"""
    dataset, norm = "h36m", True          # (4-D layout; the models below are the NTU ones)

    def __init__(self, n, c, t, v, n_classes, seed=0):
        rng = np.random.RandomState(seed)
        self.data = (rng.rand(n, c, t, v) * 2 - 1).astype(np.float32)
        self.label = rng.randint(0, n_classes, n)
        self.N, self.C, self.T, self.V = self.data.shape
        self.max, self.min = self.data.max(), self.data.min()

    def __len__(self):
        return self.N


def models(dev):
    torch.manual_seed(1234)
    G = Generator(CFG["latent"], CFG["channels"], CFG["n_classes"], CFG["t_size"], CFG["mlp"], dataset="ntu")
    D = Discriminator(CFG["channels"], CFG["n_classes"], CFG["t_size"], CFG["latent"], dataset="ntu")
    return G.to(dev), D.to(dev)


def time_loop(loop, blocks, per_block, warmup):
    for _ in range(warmup):
        loop.step()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(blocks + 1)]
    evs[0].record()
    for b in range(blocks):
        for _ in range(per_block):
            loop.step()
        evs[b + 1].record()
    torch.cuda.synchronize()
    ms = [evs[b].elapsed_time(evs[b + 1]) / per_block for b in range(blocks)]
    return statistics.median(ms), min(ms), max(ms), ms


def time_loop_like_bench(loop, steps=30, warmup=5):
    """the loop timed the way bench.py times its step: a short window on a host clock around a synchronise"""
    import time
    for _ in range(warmup):
        loop.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loop.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_ms(steps=30):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def time_step_inputs(loop):
    def fn():
        nv.step_inputs(loop.step_dev, loop._ticket, loop.seed, loop.B, z=loop.z, alpha=loop.alpha, noise=loop.noise,
                       plane_len=loop.plane_len, gather=loop._gather)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    reps = 20
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    keep = loop.step_dev.clone()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1e3)
    loop.step_dev.copy_(keep)                 # the timed launches walked the counter: put the run back
    torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
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
    say("device %s; NTU-60 shapes, %d samples per iteration, %d resident samples (%d batches per epoch)" % (
        torch.cuda.get_device_name(0), BATCH, len(feeder), len(feeder) // BATCH))
    G, D = models(dev)
    loop = TrainLoop(G, D, feeder, BATCH, CFG["t_size"], n_critic=1, seed=0)
    assert not loop.streaming
    loop_ms, bench = [], []
    for _ in range(20):
        loop.step()
    for r in range(args.rounds):
        if not args.no_bench:
            bench.append(bench_ms())
        short = time_loop_like_bench(loop)
        med, lo, hi, series = time_loop(loop, blocks=30, per_block=10, warmup=5)
        loop_ms.append(med)
        say("round %d: bench.py ms_per_step %s | TrainLoop (G every iteration) median %.4f ms per iteration over 300 replays "
            "(blocks of 10: min %.4f, max %.4f); timed like bench.py (5 + 30 iterations, host clock) %.4f ms"
            % (r, "%.3f" % bench[-1] if bench else "-", med, lo, hi, short))
        say("         blocks in order: " + " ".join("%.3f" % v for v in series))
    d, g = loop.losses()
    assert np.isfinite(d).all() and np.isfinite(g).all(), "the timed loop diverged"
    lm = statistics.median(loop_ms)
    if bench:
        bm = statistics.median(bench)
        say("TrainLoop %.4f ms vs bench.py %.4f ms per iteration (medians of %d alternating rounds): %+.2f %% (acceptance: <= +2 %%)"
            % (lm, bm, args.rounds, (lm / bm - 1) * 100))
    if not args.no_bench:
        say("bench.py --steps 300 (the yardstick's own step over a window as long as the loop's): ms_per_step %.3f" % bench_ms(300))
    us = time_step_inputs(loop)
    gathered = 2 * BATCH * CFG["channels"] * CFG["t_size"] * CFG["v"] * 4
    say("kg_step_inputs alone: %.2f us per launch (graph of 20); gather %.2f MB read + written -> %.0f GB/s; %d random values"
        % (us, gathered / 1e6, gathered / (us * 1e-6) / 1e9, loop.z.numel() + loop.alpha.numel() + loop.noise.numel()))
    del loop
    G, D = models(dev)
    loop5 = TrainLoop(G, D, feeder, BATCH, CFG["t_size"], n_critic=5, seed=0)
    med, lo, hi, _ = time_loop(loop5, blocks=30, per_block=10, warmup=20)
    say("n_critic = 5: median %.4f ms per iteration over 300 replays (min %.4f, max %.4f)" % (med, lo, hi))
    del loop5
    G, D = models(dev)
    eager = TrainLoop(G, D, feeder, BATCH, CFG["t_size"], n_critic=1, seed=0, use_graph=False)
    med, lo, hi, _ = time_loop(eager, blocks=10, per_block=5, warmup=5)
    say("eager loop (use_graph=False, G every iteration): median %.3f ms per iteration over 50 iterations" % med)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
