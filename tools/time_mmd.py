#!/usr/bin/env python3
"""kg_mmd timing: event-timed median of repeated calls for
  (i)   the reference protocol (calculate_mmd over all classes, 14 bandwidths): H36M T = 32 / 1024 avg and joint, NTU 60
        classes T = 64 avg and joint;
  (ii)  sample sets of m = 1000 (mmd_sweep, 14 bandwidths): NTU avg (G = 64 frames, dim = 75), NTU joint (G = 1,
        dim = 4800), H36M T = 1024 joint (dim = 32768);
  (iii) for (ii), stock torch in fp32: torch.cdist + exp + sum per bandwidth and frame.
Per shape: median ms, GPU kernel launches of one call (torch.profiler), distance TFLOP/s counted as 3 m (m-1) dim 2 flop
per group for every form, and that as a fraction of the 157.3 TF fp32 peak.
    python tools/time_mmd.py [--reps 20] [--skip-torch]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import metrics  # noqa: E402

PEAK_TF = 157.3
BWS = metrics.DEFAULT_BANDWIDTHS


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:      # the profiler is a convenience here, the timing stands without it
        print("  (launch count unavailable: %s)" % e)
        return -1


def report(name, fn, flops, reps):
    ms = median_ms(fn, reps)
    n = launches(fn)
    tf = flops / (ms * 1e-3) / 1e12
    print("%-44s %9.3f ms  launches %5s  %7.2f TF/s  %5.1f %% of %.1f TF" % (name, ms, n, tf, 100 * tf / PEAK_TF, PEAK_TF),
          flush=True)


def torch_sweep(seq1, seq2, mode):
    """stock torch, fp32: per frame (avg) or once (joint), cdist + exp + off-diagonal sum per bandwidth"""
    n, L, D = seq1.shape
    if mode == "joint":
        xs, ys = seq1.reshape(1, n, L * D), seq2.reshape(1, n, L * D)
    else:
        xs, ys = seq1.transpose(0, 1), seq2.transpose(0, 1)          # (L, n, D): the frames batched
    dxx, dyy, dxy = (torch.cdist(a, b).pow(2) for a, b in ((xs, xs), (ys, ys), (xs, ys)))
    out = []
    for bw in BWS:
        h = (-dxx / bw).exp() + (-dyy / bw).exp() - 2 * (-dxy / bw).exp()
        s = (h.sum((1, 2)) - h.diagonal(dim1=1, dim2=2).sum(1)) / (n * (n - 1))
        out.append(s.sqrt().mean())
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    print("(i) reference protocol: calculate_mmd, %d bandwidths, one sample per class" % len(BWS))
    for name, K, C, T, V in (("H36M T=32", 10, 3, 32, 16), ("H36M T=1024", 10, 3, 1024, 16), ("NTU-60 T=64", 60, 3, 64, 25)):
        real = torch.rand((K * 100, C, T, V), device=dev, generator=g) * 2 - 1
        fake = real * 1.1 + 0.05
        lab = np.repeat(np.arange(K), 100)                  # the selection's layout: 100 per class, class by class
        for mode in ("avg", "joint"):
            flops = 3.0 * V * (V - 1) * C * T * 2 * K          # avg: T groups of dim C; joint: one of dim C*T
            report("%s %s (G=%d)" % (name, mode, K * (T if mode == "avg" else 1)),
                   lambda: metrics.calculate_mmd(fake, real, lab, mode), flops, args.reps)
    print("(ii) sample sets, m = 1000: mmd_sweep, %d bandwidths  /  (iii) stock torch fp32 (cdist + exp + sum)" % len(BWS))
    for name, L, D, mode in (("NTU avg (G=64, dim=75)", 64, 75, "avg"), ("NTU joint (G=1, dim=4800)", 64, 75, "joint"),
                             ("H36M T=1024 joint (G=1, dim=32768)", 1024, 32, "joint")):
        m = 1000
        x = torch.rand((m, L, D), device=dev, generator=g) * 2 - 1
        y = x * 1.1 + 0.05
        flops = 3.0 * m * (m - 1) * L * D * 2
        report("kg_mmd %s" % name, lambda: metrics.mmd_sweep(x, y, BWS, mode), flops, args.reps)
        if not args.skip_torch:
            report("torch  %s" % name, lambda: torch_sweep(x, y, mode), flops, max(3, args.reps // 4))


if __name__ == "__main__":
    main()
