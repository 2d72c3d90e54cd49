#!/usr/bin/env python3
"""kg_frechet timing: one kg_frechet call (four launches) against a stock fp64 composition on the device -
mean, a centred matmul for the covariances and two torch.linalg.eigh batched over the classes (S_r, then sym(G^T S_f G)) -
alternating in one process.  Per shape and side: the event-timed median of --calls calls, taken --reps times; reported are
the median of those medians and their spread (max - min), the GPU kernel launches of one call (torch.profiler) and the
largest difference of the two sides' FD.
Shapes (pose; --motion for the frame differences): the NTU protocol (60 classes, 100 + 100 samples, T = 64, d = 75), the
H36M protocol (10 classes, 100 + 100, T = 64, d = 48) and one unconditional set of 6000 + 6000 samples at d = 75
(--big-calls calls, 200 as well unless told otherwise).
    python tools/time_frechet.py [--calls 200] [--reps 3] [--big-calls 200] [--motion] [--log profiles/frechet_time.log]"""
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
    try:                        # the profiler is a convenience here, the timing stands without it
        from torch.profiler import ProfilerActivity, profile
        prof = profile(activities=[ProfilerActivity.CUDA])
    except (ImportError, RuntimeError) as e:
        say("  (launch count unavailable: %s)" % e)
        return -1
    torch.cuda.synchronize()
    with prof as p:             # (an error raised by fn itself is an error of the run)
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def kernel_path(R, F, diff, ws):
    """R (K, n, C, T, V), F (K, m, C, T, V) fp32"""
    K, n, C, T, V = R.shape
    view = lambda x: _native.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))      # noqa: E731
    return _native.frechet(view(R), view(F), n, F.shape[1], T, diff, C, V, K, want_mean=True, ws=ws)


def stock_path(R, F, diff):
    """stock torch, fp64, every class at once: mean, centred matmul, eigh of S_r, eigh of sym(G^T S_f G)"""
    def mom(x):
        K, n, C, T, V = x.shape
        x = x.double()
        if diff:
            x = x[:, :, :, 1:] - x[:, :, :, :-1]
        p = x.permute(0, 1, 3, 2, 4).reshape(K, -1, C * V)
        mu = p.mean(1)
        c = p - mu[:, None, :]
        return mu, c.transpose(1, 2) @ c / (p.shape[1] - 1)

    mu_r, S_r = mom(R)
    mu_f, S_f = mom(F)
    l, V = torch.linalg.eigh(S_r)
    G = V * l.clamp_min(0).sqrt()[:, None, :]
    H = G.transpose(1, 2) @ S_f @ G
    e = torch.linalg.eigvalsh(0.5 * (H + H.transpose(1, 2)))
    T = e.clamp_min(0).sqrt().sum(1)
    tr = lambda S: S.diagonal(dim1=1, dim2=2).sum(1)     # noqa: E731
    values = ((mu_r - mu_f) ** 2).sum(1) + tr(S_r) + tr(S_f) - 2 * T
    return dict(values=values, mean=values.mean())


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--big-calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if args.log:
        _log = open(args.log, "w")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    diff = bool(args.motion)
    say("kg_frechet against stock torch (mean / centred matmul / 2 x linalg.eigh, fp64), %s; median of N calls x %d repetitions"
        % ("motion" if diff else "pose", args.reps))
    for name, K, n, C, T, V, calls in (("NTU protocol  60 x (100 + 100) x T 64, d 75", 60, 100, 3, 64, 25, args.calls),
                                       ("H36M protocol 10 x (100 + 100) x T 64, d 48", 10, 100, 3, 64, 16, args.calls),
                                       ("unconditional  1 x (6000 + 6000) x T 64, d 75", 1, 6000, 3, 64, 25, args.big_calls)):
        mix = torch.randn((K, 1, C, 1, V), device=dev, generator=g)
        R = 0.3 * (mix + torch.randn((K, n, C, T, V), device=dev, generator=g))
        F = 0.28 * (mix + torch.randn((K, n, C, T, V), device=dev, generator=g)) + 0.02
        ws = torch.empty(_native.frechet_workspace_bytes(n, n, T, diff, C, V, K) // 8, dtype=torch.float64, device=dev)
        sides = (("kg_frechet", lambda: kernel_path(R, F, diff, ws)), ("stock     ", lambda: stock_path(R, F, diff)))
        meds = {s: [] for s, _ in sides}
        for _ in range(args.reps):                      # alternating: kernel, stock, kernel, stock, ...
            for s, fn in sides:
                meds[s].append(median_ms(fn, calls))
        out = kernel_path(R, F, diff, ws)
        err = (out["values"] - stock_path(R, F, diff)["values"]).abs().max().item()
        say("%s  (N = %d)" % (name, calls))
        res = {}
        for s, fn in sides:
            med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
            res[s] = (med, spread)
            say("  %s %9.4f ms  spread %7.4f ms  medians %s  launches %3d" % (s, med, spread,
                                                                            " ".join("%.4f" % v for v in meds[s]), launches(fn)))
        gap, bar = res["stock     "][0] - res["kg_frechet"][0], max(res["kg_frechet"][1], res["stock     "][1])
        say("  stock - kg_frechet = %+.4f ms against the larger spread %.4f ms: kg_frechet is %s; largest FD difference %.3g; "
            "sweeps at most %d" % (gap, bar, "faster" if gap > bar else ("slower" if -gap > bar else "not separated"), err,
                                   int(out["sweeps"].max())))


if __name__ == "__main__":
    main()
