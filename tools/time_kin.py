#!/usr/bin/env python3
"""kg_kin timing: the kinematic scores of a real and a generated set - two kg_kin_desc launches and one
kg_kin_scores call (two launches) - against a stock fp64 composition on the device of the same scores (indexing, torch.diff,
torch.linalg.vector_norm, sort, cumsum), alternating in one process.  Per shape and side: the event-timed median of --calls
calls, taken --reps times; reported are the median of those medians and their spread (max - min), the GPU kernel launches of
one call (torch.profiler) and the largest difference of the two sides' W1.  As context: kg_kin_desc of one set and
kg_kin_scores on their own, and the input bytes of kg_kin_desc over its time.
Shapes: the NTU protocol (60 classes, 100 + 100 samples, T = 64, C 3, V 25), the H36M protocol (10 classes, 100 + 100, T = 64,
C 2, V 16) and one unconditional set of 6000 + 6000 NTU samples (--big-calls calls).
    python tools/time_kin.py [--calls 200] [--reps 3] [--big-calls 200] [--log profiles/kin_time.log]
``--sets G`` (record: profiles/eval_kinematics_time.log): instead of the above, ONE kg_kin_desc_sets launch over
G sets against G kg_kin_desc calls of the same build at the NTU and the H36M protocol shapes, alternating in the same way
(outputs and workspaces allocated outside the timed calls on both sides, the bits compared once).
    python tools/time_kin.py --sets 2 [--calls 200] [--reps 3] [--log FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native  # noqa: E402
from kinetic_gan_amd.graph import Graph_h36m, graph_ntu  # noqa: E402
from time_frechet import launches, median_ms  # noqa: E402
import time_frechet  # noqa: E402

STILL_EPS = 1e-3


def say(line):
    time_frechet.say(line)


def view(x):
    return _native.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))


def kernel_desc(x, bones, mirror):
    K, n, C, T, V = x.shape
    return _native.kin_desc(view(x), n, T, C, V, K, bones, mirror, STILL_EPS)[0]


def kernel_path(R, F, bones, mirror):
    return _native.kin_scores(kernel_desc(R, bones, mirror), [kernel_desc(F, bones, mirror)])


def stock_desc(x, bu, bv, ma, mb):
    """x (K, n, C, T, V) fp32 -> (K, n, 6) fp32, stock torch in fp64"""
    x = x.double()
    L = torch.linalg.vector_norm(x[..., bu] - x[..., bv], dim=2)                    # (K, n, T, B)
    mu = L.mean(2)
    sd = ((L - mu[:, :, None]) ** 2).mean(2).sqrt()
    s = L.mean((2, 3))
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    cv = torch.where(mu != 0, sd / mu, zero).mean(-1)
    den = 0.5 * (mu[..., ma] + mu[..., mb])
    asym = torch.where(den != 0, (mu[..., ma] - mu[..., mb]).abs() / den, zero).mean(-1)
    v1 = torch.linalg.vector_norm(torch.diff(x, dim=3), dim=2)                      # (K, n, T - 1, V)
    v2 = torch.linalg.vector_norm(torch.diff(x, n=2, dim=3), dim=2)
    v3 = torch.linalg.vector_norm(torch.diff(x, n=3, dim=3), dim=2)
    still = (v1 < STILL_EPS * s[:, :, None, None]).double().mean((2, 3))
    d = torch.stack([cv, asym, v1.mean((2, 3)) / s, v2.mean((2, 3)) / s, v3.mean((2, 3)) / s, still], -1)
    return torch.where((s == 0)[..., None], zero, d).float()


def stock_scores(dr, df):
    """(K, n, 6), (K, m, 6) fp32 -> w1 (K, 6), w1_mean (6,), means"""
    n, m = dr.shape[1], df.shape[1]
    zs, order = torch.cat([dr, df], 1).double().sort(dim=1)
    cr = (order < n).cumsum(1)
    cf = torch.arange(1, n + m + 1, device=dr.device)[None, :, None] - cr
    term = (cr * m - cf * n).abs()[:, :-1].double() * torch.diff(zs, dim=1)
    w1 = term.sum(1) / float(n * m)
    return dict(w1=w1, w1_mean=w1.mean(0), mean_real=dr.double().mean(1), mean_fake=df.double().mean(1))


def stock_path(R, F, tabs):
    return stock_scores(stock_desc(R, *tabs), stock_desc(F, *tabs))


def time_sets(args, dev, g):
    """kg_kin_desc_sets over args.sets sets against that many kg_kin_desc calls"""
    G = args.sets
    say("kg_kin_desc_sets over %d sets (ONE launch) against %d kg_kin_desc calls; median of %d calls x %d repetitions" % (
        G, G, args.calls, args.reps))
    for name, graph, K, n, C, T, V in (("NTU protocol  60 x 100 x T 64, C 3, V 25", graph_ntu, 60, 100, 3, 64, 25),
                                       ("H36M protocol 10 x 100 x T 64, C 2, V 16", Graph_h36m, 10, 100, 2, 64, 16)):
        bones, mirror = graph.bones, graph.mirror_bones
        xs = [make(K, n, C, T, V, dev, g, 1.0 / (1 + i)) for i in range(G)]
        views = [view(x) for x in xs]
        out = torch.zeros((G, K, n, 6), dtype=torch.float32, device=dev)
        ref = torch.zeros((G, K, n, 6), dtype=torch.float32, device=dev)
        ws = torch.zeros(_native.kin_desc_sets_workspace_bytes(G, n, T, C, V, K, bones, mirror) // 4, dtype=torch.float32, device=dev)

        def one_launch():
            return _native.kin_desc_sets(views, 0, 0, 0, 0, n, T, C, V, K, bones, mirror, STILL_EPS, out=out, ws=ws)

        def per_set():
            return [_native.kin_desc(views[i], n, T, C, V, K, bones, mirror, STILL_EPS, out=ref[i]) for i in range(G)]

        sides = (("desc_sets ", one_launch), ("desc x %d  " % G, per_set))
        meds = {s: [] for s, _ in sides}
        for _ in range(args.reps):                      # alternating: sets, per set, sets, per set, ...
            for s, fn in sides:
                meds[s].append(median_ms(fn, args.calls))
        deg = one_launch()[1]
        degs = torch.stack([d for _, d in per_set()])
        torch.cuda.synchronize()
        same = torch.equal(out.view(torch.int32), ref.view(torch.int32)) and torch.equal(deg, degs)
        say("%s  (N = %d)" % (name, args.calls))
        res = {}
        for s, fn in sides:
            med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
            res[s] = (med, spread)
            say("  %s %9.4f ms  spread %7.4f ms  medians %s  launches %3d" % (s, med, spread,
                                                                            " ".join("%.4f" % v for v in meds[s]), launches(fn)))
        (a, sa), (b, sb) = res[sides[0][0]], res[sides[1][0]]
        gap, bar = b - a, max(sa, sb)
        verdict = "faster by more than three spreads" if gap > 3 * bar else ("slower by more than three spreads" if -gap > 3 * bar
                                                                            else "not separated (within three spreads)")
        nbytes = 4.0 * G * K * n * C * T * V
        say("  per-set calls - one launch = %+.4f ms against the larger spread %.4f ms (three times: %.4f ms): kg_kin_desc_sets is %s; "
            "%.1f MB of input at %.3f TB/s; bits equal: %s" % (gap, bar, 3 * bar, verdict, nbytes / 1e6,
                                                              nbytes / (a * 1e-3) / 1e12, same))


def make(K, n, C, T, V, dev, g, scale):
    p0 = torch.randn((K, n, C, 1, V), device=dev, generator=g)
    own = torch.cumsum(0.02 * torch.randn((K, n, C, T, V), device=dev, generator=g), 3)
    shared = torch.cumsum(0.05 * torch.randn((K, n, C, T, 1), device=dev, generator=g), 3)
    return ((p0 + own + shared) * scale).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--big-calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log", type=str, default=None)
    ap.add_argument("--sets", type=int, default=0, help="time kg_kin_desc_sets over this many sets against as many kg_kin_desc calls")
    args = ap.parse_args()
    if args.log:
        time_frechet._log = open(args.log, "w")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if args.sets:
        return time_sets(args, dev, g)
    say("kg_kin_desc x 2 + kg_kin_scores against stock torch (index / diff / linalg.vector_norm / sort / cumsum, fp64); "
        "median of N calls x %d repetitions" % args.reps)
    for name, graph, K, n, C, T, V, calls in (("NTU protocol  60 x (100 + 100) x T 64, C 3, V 25", graph_ntu, 60, 100, 3, 64, 25, args.calls),
                                              ("H36M protocol 10 x (100 + 100) x T 64, C 2, V 16", Graph_h36m, 10, 100, 2, 64, 16, args.calls),
                                              ("unconditional  1 x (6000 + 6000) x T 64, C 3, V 25", graph_ntu, 1, 6000, 3, 64, 25, args.big_calls)):
        bones, mirror = graph.bones, graph.mirror_bones
        idx = lambda pairs, k: torch.tensor([p[k] for p in pairs], device=dev)       # noqa: E731
        tabs = (idx(bones, 0), idx(bones, 1), idx(mirror, 0), idx(mirror, 1))
        R, F = make(K, n, C, T, V, dev, g, 1.0), make(K, n, C, T, V, dev, g, 0.3)
        sides = (("kg_kin    ", lambda: kernel_path(R, F, bones, mirror)), ("stock     ", lambda: stock_path(R, F, tabs)))
        meds = {s: [] for s, _ in sides}
        for _ in range(args.reps):                      # alternating: kernel, stock, kernel, stock, ...
            for s, fn in sides:
                meds[s].append(median_ms(fn, calls))
        out, ref = kernel_path(R, F, bones, mirror), stock_path(R, F, tabs)
        err = (out["w1"][0] - ref["w1"]).abs().max().item()
        rel = ((out["w1"][0] - ref["w1"]).abs() / ref["w1"].abs().clamp_min(1e-300)).max().item()
        say("%s  (N = %d)" % (name, calls))
        res = {}
        for s, fn in sides:
            med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
            res[s] = (med, spread)
            say("  %s %9.4f ms  spread %7.4f ms  medians %s  launches %3d" % (s, med, spread,
                                                                            " ".join("%.4f" % v for v in meds[s]), launches(fn)))
        gap, bar = res["stock     "][0] - res["kg_kin    "][0], max(res["kg_kin    "][1], res["stock     "][1])
        verdict = "faster by more than three spreads" if gap > 3 * bar else ("faster" if gap > bar else
                                                                            ("slower" if -gap > bar else "not separated"))
        say("  stock - kg_kin = %+.4f ms against the larger spread %.4f ms (three times: %.4f ms): kg_kin is %s; largest W1 "
            "difference %.3g absolute, %.3g relative" % (gap, bar, 3 * bar, verdict, err, rel))
        dr, df = kernel_desc(R, bones, mirror), kernel_desc(F, bones, mirror)
        t_desc = median_ms(lambda: kernel_desc(R, bones, mirror), calls)
        t_sc = median_ms(lambda: _native.kin_scores(dr, [df]), calls)
        nbytes = 4.0 * K * n * C * T * V
        say("  context: kg_kin_desc of one set %.4f ms = %.1f MB of input at %.3f TB/s (call time, binding included); kg_kin_scores "
            "%.4f ms" % (t_desc, nbytes / 1e6, nbytes / (t_desc * 1e-3) / 1e12, t_sc))


if __name__ == "__main__":
    main()
