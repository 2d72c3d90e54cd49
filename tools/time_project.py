#!/usr/bin/env python3
"""Projection timing: one iteration of project.Projector - synthesis, kg_proj_loss, the generator's backward
pass, kg_proj_step, step += 1 - as a hipGraph replay and eagerly, and the two new launches against a stock-op composition of
the same objective and step (fp32 torch: slices, differences, gathers, sums, where, Adam, keep-the-best), in isolation (eager:
only the tail, on a fixed generated batch) and inside the replay (the whole iteration captured with the stock tail instead).
Shapes: NTU (n = 64, T = 64, 60 classes, latent 512) and H36M (n = 64, T = 32, 10 classes).  Per side: the event-timed median of
--calls calls, taken --reps times in alternation; reported are the median of those medians, their spread (max - min) and the
GPU launches of one call (torch.profiler).  A difference counts only beyond three spreads.
    python tools/time_project.py [--calls 200] [--reps 3] [--log profiles/project_time.log]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.project import Projector  # noqa: E402
from kinetic_gan_amd.replay import capture_keeping  # noqa: E402
from time_frechet import launches, median_ms  # noqa: E402
import time_frechet  # noqa: E402

say = time_frechet.say


def stock_loss(x, y, m, ia, ic, lam):
    """the objective of kg_proj_loss in fp32 stock ops, differentiable in x: (n,) totals and the (n, 4) words"""
    C = x.shape[1]
    zero = x.new_zeros(())
    d = x - y
    on = m > 0
    Lp = torch.where(on[:, None], m[:, None] * d * d, zero).sum((1, 2, 3)) / (C * torch.where(on, m, zero).sum((1, 2))).clamp_min(1e-30)
    onv = on[:, :-1] & on[:, 1:]
    mv = torch.where(onv, m[:, :-1] * m[:, 1:], zero)
    e = d[:, :, 1:] - d[:, :, :-1]
    Lv = torch.where(onv[:, None], mv[:, None] * e * e, zero).sum((1, 2, 3)) / (C * mv.sum((1, 2))).clamp_min(1e-30)
    onb = (m[:, :, ia] > 0) & (m[:, :, ic] > 0)
    mb = torch.where(onb, m[:, :, ia] * m[:, :, ic], zero)
    sx = ((x[:, :, :, ia] - x[:, :, :, ic]) ** 2).sum(1)
    sy = ((y[:, :, :, ia] - y[:, :, :, ic]) ** 2).sum(1)
    df = torch.where(onb, sx - sy, zero)
    Lb = (mb * df * df).sum((1, 2)) / mb.sum((1, 2)).clamp_min(1e-30)
    L = (lam[0] * Lp + lam[1] * Lv) + lam[2] * Lb
    return L, torch.stack([L, Lp, Lv, Lb], 1)


def stock_step(p, gw, loss):
    """kg_proj_step in fp32 stock ops on the Projector's buffers; no host synchronisation"""
    w, S, D = p.w.detach(), p.steps, p.D
    b1, b2 = p.betas
    diff = w - p.wmean[p.labels]
    obj = loss[:, 0] + p.lambda_w * diff.pow(2).mean(1)
    ok = torch.isfinite(obj) & torch.isfinite(gw).all(1)
    better = ok & (obj < p.best_obj)
    p.best_obj.copy_(torch.where(better, obj, p.best_obj))
    p.best_loss.copy_(torch.where(better[:, None], loss, p.best_loss))
    p.best_w.copy_(torch.where(better[:, None], w, p.best_w))
    p.history.index_copy_(0, (p.step.long() - 1).clamp(0, S - 1), obj[None])
    p.nonfinite.add_((~ok).int())
    g = gw + (2.0 * p.lambda_w / D) * diff
    s = p.step.float()
    lr = torch.full_like(s, p.lr)
    if p.ramp_up > 0:
        lr = lr * (s / p.ramp_up).clamp_max(1.0)
    if p.ramp_down > 0:
        lr = lr * torch.where(s > S - p.ramp_down, 0.5 * (1.0 + torch.cos(math.pi * (s - (S - p.ramp_down)) / p.ramp_down)), torch.ones_like(s))
    am1 = b1 * p.am + (1 - b1) * g
    av1 = b2 * p.av + (1 - b2) * g * g
    up = (am1 / (1 - b1 ** s)) / ((av1 / (1 - b2 ** s)).sqrt() + p.eps)
    k = ok[:, None]
    p.am.copy_(torch.where(k, am1, p.am))
    p.av.copy_(torch.where(k, av1, p.av))
    w.copy_(torch.where(k, w - lr * up, w))


class StockProjector(Projector):
    """the same iteration with the stock-op tail: the objective's gradient comes out of autograd with the generator's"""

    def _iteration(self):
        with torch.enable_grad():
            x = self.G.synthesis(self.w, self.noise)
            L, words = stock_loss(x, self.target, self.mask, self._ia, self._ic, self.lambdas)
            gw, = torch.autograd.grad(L.sum(), self.w)
        stock_step(self, gw, words.detach())
        self.step.add_(1)


def report(name, sides, calls, reps):
    meds = {s: [] for s, _ in sides}
    for _ in range(reps):                               # alternating: a, b, a, b, ...
        for s, fn in sides:
            meds[s].append(median_ms(fn, calls))
    say("%s  (N = %d)" % (name, calls))
    res = {}
    for s, fn in sides:
        med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
        res[s] = (med, spread)
        say("  %-28s %9.4f ms  spread %7.4f ms  medians %s  launches %3d" % (s, med, spread, " ".join("%.4f" % v for v in meds[s]), launches(fn)))
    (a, sa), (b, sb) = res[sides[0][0]], res[sides[1][0]]
    gap, bar = b - a, max(sa, sb)
    verdict = "faster by more than three spreads" if gap > 3 * bar else ("slower by more than three spreads" if -gap > 3 * bar
                                                                        else "not separated (within three spreads)")
    say("  %s - %s = %+.4f ms against the larger spread %.4f ms (three times: %.4f ms): the first is %s" % (
        sides[1][0].strip(), sides[0][0].strip(), gap, bar, 3 * bar, verdict))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if args.log:
        time_frechet._log = open(args.log, "w")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    say("project.Projector: one iteration (synthesis, objective, backward, step); median of N calls x %d alternating repetitions" % args.reps)
    for name, ds, C, K, T, n in (("NTU  n 64, T 64, C 3, V 25, 60 classes", "ntu", 3, 60, 64, 64), ("H36M n 64, T 32, C 2, V 16, 10 classes", "h36m", 2, 10, 32, 64)):
        torch.manual_seed(0)
        G = Generator(512, C, K, T, 4, dataset=ds).to(dev)
        kw = dict(dataset=ds, steps=200, lr=1e-3, lambda_w=0.01, mean_size=100)
        g = torch.Generator(device=dev).manual_seed(1)
        V = G.graph.num_node[0]
        y = torch.rand((n, C, T, V), device=dev, generator=g) * 2 - 1
        labels = torch.arange(n) % K
        ours, stock = Projector(G, n, **kw), StockProjector(G, n, **kw)
        stock._ia = torch.tensor([b[0] for b in stock.bones], device=dev)
        stock._ic = torch.tensor([b[1] for b in stock.bones], device=dev)
        for p in (ours, stock):
            p._reset(y, labels, None, None)
        with ours._reading():
            graphs = {id(p): capture_keeping(p._iteration, p._state(), dev) for p in (ours, stock)}
            say("%s" % name)
            report("  whole iteration, replayed", (("kg_proj tail, replay", graphs[id(ours)].replay), ("stock tail, replay", graphs[id(stock)].replay)),
                   args.calls, args.reps)
            report("  whole iteration, eager", (("kg_proj tail, eager", ours._iteration), ("stock tail, eager", stock._iteration)), args.calls, args.reps)
            # the tail alone, on a fixed generated batch
            with torch.no_grad():
                x = G.synthesis(ours.w.detach(), ours.noise).detach()
            gw = torch.randn((n, ours.D), device=dev, generator=g) * 1e-3

            def tail_ours():
                nv.proj_loss(x, ours.target, ours.bones, ours.lambdas, mask=ours.mask, loss=ours.loss, gx=ours.gx)
                nv.proj_step(ours.w.detach(), ours.am, ours.av, gw, ours.wmean, ours.labels, ours.loss, ours.step, ours.best_obj, ours.best_loss,
                             ours.best_w, ours.nonfinite, ours.history, ours.steps, ours.lr, ours.betas[0], ours.betas[1], ours.eps, ours.lambda_w,
                             ours.ramp_up, ours.ramp_down)

            def tail_stock():
                xs = x.clone().requires_grad_(True)
                with torch.enable_grad():
                    L, words = stock_loss(xs, stock.target, stock.mask, stock._ia, stock._ic, stock.lambdas)
                    torch.autograd.grad(L.sum(), xs)
                stock_step(stock, gw, words.detach())

            report("  the tail alone, eager", (("kg_proj_loss + kg_proj_step", tail_ours), ("stock ops", tail_stock)), args.calls, args.reps)


if __name__ == "__main__":
    main()
