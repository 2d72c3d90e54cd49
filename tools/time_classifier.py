#!/usr/bin/env python3
"""Action-classifier timing, NTU shapes (3 x 64 x 25, 60 classes), 64 samples per iteration, one process:
  * one ClassifierLoop iteration, graph replay against the same launches eagerly (alternating windows of --iters iterations,
    host clock around a device synchronise), and the GPU kernel launches of one eager iteration (torch.profiler);
  * the head alone on h (64, 512, 4, 1): kg_cls_head_fwd + _bwd + _wgrad against a stock-op composition of the same head
    (mean, two F.linear, leaky_relu, cross_entropy and its autograd backward), event-timed medians;
  * metrics.classifier_scores on 6000 + 6000 samples resident on the device, chunks of 512.
Per figure: the median of --reps windows and their spread (max - min).  Needs a GPU; nothing here is an acceptance criterion.
    python tools/time_classifier.py [--iters 200] [--reps 3] [--log profiles/classifier_time.log]"""
import argparse
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd import metrics  # noqa: E402
from kinetic_gan_amd.classifier import Classifier  # noqa: E402
from kinetic_gan_amd.classify import ClassifierLoop  # noqa: E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402

_log = None


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def window_ms(fn, iters):
    """ms per call over a window of `iters` calls that ends in a synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_median_ms(fn, calls):
    for _ in range(5):
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
    with prof as p:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def report(name, vals, unit="ms"):
    say("%-58s %9.4f %s  (spread %.4f over %d)" % (name, statistics.median(vals), unit, max(vals) - min(vals), len(vals)))


def main(argv=None):
    global _log
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log", type=str, default=None)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_classifier.py needs a GPU")
    if opt.log:
        os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
        _log = open(opt.log, "w")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    say("# %s, B = 64, NTU shapes; iters %d, reps %d" % (torch.cuda.get_device_name(dev), opt.iters, opt.reps))
    B, C, T, V, L = 64, 3, 64, 25, 60
    rs = np.random.RandomState(0)

    # ---- the loop -------------------------------------------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as d:
        n = 1024
        np.save(os.path.join(d, "x.npy"), rs.randn(n, C, T, V, 1).astype(np.float32))
        with open(os.path.join(d, "y.pkl"), "wb") as f:
            pickle.dump((["s%d" % i for i in range(n)], rs.randint(0, L, n).tolist()), f)
        feeder = Feeder(os.path.join(d, "x.npy"), os.path.join(d, "y.pkl"), dataset="ntu", mmap=False)
        loops = {}
        for mode in ("replay", "eager"):
            torch.manual_seed(0)
            loops[mode] = ClassifierLoop(Classifier(C, L, T, dataset="ntu").to(dev), feeder, B, T, use_graph=mode == "replay")
            for _ in range(5):
                loops[mode].step()
    res = {"replay": [], "eager": []}
    for _ in range(opt.reps):
        for mode in ("replay", "eager"):
            res[mode].append(window_ms(loops[mode].step, opt.iters))
    report("ClassifierLoop iteration, graph replay", res["replay"])
    report("ClassifierLoop iteration, eager", res["eager"])
    say("GPU kernel launches of one eager iteration: %d" % launches(loops["eager"].step))

    # ---- the head alone ---------------------------------------------------------------------------------------------------
    Cl, Fd, Tp, Vp = 512, 64, 4, 1
    h = nv.new_plane(B, Cl, Tp, Vp, dev)
    h.copy_(torch.randn(B, Cl, Tp, Vp, device=dev))
    w1, b1 = torch.randn(Fd, Cl, device=dev) / 22.0, torch.zeros(Fd, device=dev)
    w2, b2 = torch.randn(L, Fd, device=dev) / 8.0, torch.zeros(L, device=dev)
    y = torch.randint(0, L, (B,), device=dev)
    one = torch.ones(1, device=dev)
    dws = [torch.zeros(p.numel(), device=dev) for p in (w1, b1, w2, b2)]

    def native():
        o = nv.cls_head_fwd(h, w1, b1, w2, b2, y)
        g, ws = nv.cls_head_bwd(one, h, w1, w2, y, o["feat"], o["logits"], masked=False)
        nv.cls_head_wgrad(ws, o["pooled"], o["feat"], L, *dws, accumulate=False)
        return o["loss"], g

    hs = h.detach().clone().requires_grad_()
    ps = [p.detach().clone().requires_grad_() for p in (w1, b1, w2, b2)]

    def stock():
        logits = F.linear(F.leaky_relu(F.linear(hs.mean(dim=(2, 3)), ps[0], ps[1]), 0.2), ps[2], ps[3])
        loss = F.cross_entropy(logits, y)
        grads = torch.autograd.grad(loss, [hs] + ps)
        return loss, grads[0]

    ln, gn = native()
    lt, gt = stock()
    say("head: native against stock loss %.3e, top gradient %.3e (relative to max)" % (
        abs(float(ln) - float(lt.detach())) / abs(float(lt.detach())), float((gn - gt).abs().max() / gt.abs().max())))
    hn, ht = [], []
    for _ in range(opt.reps):
        hn.append(event_median_ms(native, opt.iters))
        ht.append(event_median_ms(stock, opt.iters))
    report("head fwd + bwd + wgrad, kg_cls_head_* (%d launches)" % launches(native), hn)
    report("head fwd + bwd, stock ops (%d launches)" % launches(stock), ht)

    # ---- scoring ----------------------------------------------------------------------------------------------------------
    clf = loops["replay"].C
    n = 6000
    xg, xr = torch.randn(n, C, T, V, device=dev) * 0.3, torch.randn(n, C, T, V, device=dev) * 0.3
    yg = yr = np.repeat(np.arange(L), n // L)

    def score():
        s = metrics.classifier_scores(clf, xg, yg, xr, yr, per_class=n // L, batch=512)
        return float(s["feature_fd_class_mean"].cpu())

    score()
    sc = []
    for _ in range(opt.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score()
        torch.cuda.synchronize()
        sc.append((time.perf_counter() - t0) * 1e3)
    report("classifier_scores, 6000 + 6000 samples, chunks of 512", sc)


if __name__ == "__main__":
    main()
