#!/usr/bin/env python3
"""kg_prdc timing: one kg_prdc call (three launches) against a stock torch composition in fp32 -
torch.cdist of R x R, F x F and R x F batched over the classes, kthvalue for the radii, comparisons and reductions for
the counts - alternating in one process.  Per shape and side: the event-timed median of --calls calls, taken --reps
times; reported are the median of those medians and their spread (max - min), the GPU kernel launches of one call
(torch.profiler) and whether the two sides count the same.
Shapes: the NTU protocol (60 classes, 100 + 100 samples, D = 3*64*25 = 4800, k = 5), the H36M protocol (10 classes,
100 + 100, D = 2*64*16 = 2048) and one unconditional set of 4096 + 4096 samples at D = 4800 (--big-calls calls).
    python tools/time_prdc.py [--calls 200] [--reps 3] [--big-calls 20] [--log profiles/prdc_time.log]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native  # noqa: E402

_log = None


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def median_ms(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
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
        say("  (launch count unavailable: %s)" % e)
        return -1


def kernel_path(R, F, k):
    K, n, D = R.shape
    return _native.prdc(_native.PrdcView(R, R.stride(0), R.stride(1), 0), _native.PrdcView(F, F.stride(0), F.stride(1), 0),
                        n, F.shape[1], 1, D, K, k, want_mean=True)


def stock_path(R, F, k):
    """stock torch, fp32, every class at once: three cdist, kthvalue, comparisons, reductions"""
    K, n, _ = R.shape
    m = F.shape[1]
    drr, dff, drf = torch.cdist(R, R).pow(2), torch.cdist(F, F).pow(2), torch.cdist(R, F).pow(2)
    drr.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    dff.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    rr, rf = drr.kthvalue(k, dim=2).values, dff.kthvalue(k, dim=2).values
    P, Q = drf <= rr[:, :, None], drf <= rf[:, None, :]
    counts = torch.stack([P.any(1).sum(1), Q.any(2).sum(1), P.sum((1, 2)), P.any(2).sum(1)], 1)
    den = torch.tensor([m, n, k * m, n], dtype=torch.float64, device=R.device)
    values = (counts.double() / den).float()
    return dict(counts=counts, values=values, mean=values.mean(0))


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--big-calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if args.log:
        _log = open(args.log, "w")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    say("kg_prdc against stock torch (cdist / kthvalue / comparisons), fp32, k = 5; median of N calls x %d repetitions" % args.reps)
    for name, K, n, D, calls in (("NTU protocol  60 x (100 + 100) x 4800", 60, 100, 4800, args.calls),
                                 ("H36M protocol 10 x (100 + 100) x 2048", 10, 100, 2048, args.calls),
                                 ("unconditional  1 x (4096 + 4096) x 4800", 1, 4096, 4800, args.big_calls)):
        base = torch.randn((K, 1, D), device=dev, generator=g)
        R = base + 0.5 * torch.randn((K, n, D), device=dev, generator=g)
        F = base + 0.45 * torch.randn((K, n, D), device=dev, generator=g) + 0.02
        sides = (("kg_prdc", lambda: kernel_path(R, F, 5)), ("stock  ", lambda: stock_path(R, F, 5)))
        meds = {s: [] for s, _ in sides}
        for _ in range(args.reps):                      # alternating: kernel, stock, kernel, stock, ...
            for s, fn in sides:
                meds[s].append(median_ms(fn, calls))
        a, b = kernel_path(R, F, 5)["counts"].long(), stock_path(R, F, 5)["counts"].long()
        diff = (a - b).abs().max().item()
        say("%s  (N = %d)" % (name, calls))
        res = {}
        for s, fn in sides:
            med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
            res[s] = (med, spread)
            say("  %s %9.4f ms  spread %7.4f ms  medians %s  launches %3d" % (s, med, spread,
                                                                            " ".join("%.4f" % v for v in meds[s]), launches(fn)))
        gap, bar = res["stock  "][0] - res["kg_prdc"][0], max(res["kg_prdc"][1], res["stock  "][1])
        say("  stock - kg_prdc = %+.4f ms against the larger spread %.4f ms: kg_prdc is %s; largest count difference %d"
            % (gap, bar, "faster" if gap > bar else ("slower" if -gap > bar else "not separated"), diff))


if __name__ == "__main__":
    main()
