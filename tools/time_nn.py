#!/usr/bin/env python3
"""kg_nn timing: one kg_nn call (two launches) against a stock torch composition in fp32 - torch.cdist of
row chunks sized so that the distance matrix stays under 1 GB, squared, topk(k, largest=False) per chunk - alternating in
one process.  Per shape and side: the event-timed median of --calls calls, taken --reps times; reported are the median of
those medians and their spread (max - min), and how many queries the two sides give the same nearest index (the stock
side is the Gram form: near-copies cancel there).  The verdict per shape: kg_nn is "faster", "slower" or "not separated"
by more than the larger spread.
Shapes: the NTU shape (6000 generated x 40000 training sequences, D = 3*64*25 = 4800, k = 1 and 5), the H36M shape (1000 x
4000, D = 2*64*16 = 2048, k = 1 and 5) and one leave-one-out train -> train pass (40000 x 40000 x 4800, k = 1,
--big-calls calls).
``--method gram`` (record: profiles/nn_gram_time.log): a third side, one kg_nn_gram call (six launches: the
matrix-core pre-filter, exact re-score, fallback) with the base's norms given - kg_nn_norms, one launch, is timed on its own
since it is made once per base -, alternating with the other two; its bits are compared with kg_nn's, its stats (certified
rows, fallback rows) stand next to the times, and the verdict is kg_nn_gram against kg_nn by more than three times the larger
spread.
    python tools/time_nn.py [--calls 200] [--reps 3] [--big-calls 5] [--shapes ntu,h36m,train] [--method exact|gram]
                            [--log profiles/nn_time.log]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native  # noqa: E402

_log = None
MATRIX_BYTES = 10 ** 9


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def median_ms(fn, calls):
    for _ in range(2):
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


def kernel_path(q, b, k, exclude_self, ws):
    v = lambda x: _native.PrdcView(x, 0, x.stride(0), 0)      # noqa: E731
    return _native.nn(v(q), v(b), q.shape[0], b.shape[0], 1, q.shape[1], 1, k, exclude_self=exclude_self, ws=ws)


def gram_path(q, b, k, exclude_self, ws, norms):
    return _native.nn_gram([q], 0, q.stride(0), 0, _native.PrdcView(b, 0, b.stride(0), 0), q.shape[0], b.shape[0], 1, q.shape[1], 1, k,
                           exclude_self=exclude_self, ws=ws, base_norms=norms)


def stock_path(q, b, k, exclude_self):
    """stock torch, fp32: cdist (its Gram form at these sizes) and topk over row chunks of at most MATRIX_BYTES"""
    rows = max(1, MATRIX_BYTES // (4 * b.shape[0]))
    idx, d2 = [], []
    for lo in range(0, q.shape[0], rows):
        d = torch.cdist(q[lo:lo + rows], b).pow_(2)
        if exclude_self:
            n = d.shape[0]
            d[torch.arange(n, device=d.device), torch.arange(lo, lo + n, device=d.device)] = float("inf")
        t = d.topk(k, dim=1, largest=False)
        idx.append(t.indices)
        d2.append(t.values)
    return torch.cat(idx), torch.cat(d2)


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--big-calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", type=str, default="ntu,h36m,train")
    ap.add_argument("--method", type=str, default="exact", choices=["exact", "gram"],
                    help="gram: also time kg_nn_gram, the matrix-core pre-filter with exact re-score (DESIGN.md 24)")
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        _log = open(args.log, "a")        # (a run per group of shapes adds to one log)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    say("kg_nn against stock torch (chunked cdist / topk, matrix under 1 GB), fp32; median of N calls x %d repetitions" % args.reps)
    table = {"ntu": [("NTU shape    6000 x 40000 x 4800", 6000, 40000, 4800, k, False, args.calls) for k in (1, 5)],
             "h36m": [("H36M shape   1000 x  4000 x 2048", 1000, 4000, 2048, k, False, args.calls) for k in (1, 5)],
             "train": [("train->train 40000 x 40000 x 4800 leave-one-out", 40000, 40000, 4800, 1, True, args.big_calls)]}
    for key in args.shapes.split(","):
        for name, Q, N, D, k, excl, calls in table[key]:
            # a 4-dimensional latent mixed into D dimensions: neighbours at every scale, as in the tests
            mix = torch.randn((4, D), device=dev, generator=g) * (3 / D ** 0.5)
            b = torch.randn((N, 4), device=dev, generator=g) @ mix + 0.01 * torch.randn((N, D), device=dev, generator=g)
            q = b if excl else torch.randn((Q, 4), device=dev, generator=g) @ mix + 0.01 * torch.randn((Q, D), device=dev, generator=g)
            ws = torch.empty(_native.nn_workspace_bytes(Q, N, 1, D, 1, k, exclude_self=excl) // 4, dtype=torch.int32, device=dev)
            sides = (("kg_nn", lambda: kernel_path(q, b, k, excl, ws)), ("stock", lambda: stock_path(q, b, k, excl)))
            if args.method == "gram":
                bv = _native.PrdcView(b, 0, b.stride(0), 0)
                norms = _native.nn_norms(bv, N, 1, D, 1)
                gws = torch.empty(_native.nn_gram_workspace_bytes(1, Q, N, 1, D, 1, k, exclude_self=excl) // 4, dtype=torch.int32,
                                  device=dev)
                sides = (("kg_nn_gram", lambda: gram_path(q, b, k, excl, gws, norms)),) + sides
            meds = {s: [] for s, _ in sides}
            for _ in range(args.reps):                      # alternating: kernel, stock, kernel, stock, ...
                for s, fn in sides:
                    meds[s].append(median_ms(fn, calls))
            same = (kernel_path(q, b, k, excl, ws)[0][0, :, 0].long() == stock_path(q, b, k, excl)[0][:, 0]).sum().item()
            say("%s  k = %d  (N = %d)" % (name, k, calls))
            res = {}
            for s, _ in sides:
                med, spread = statistics.median(meds[s]), max(meds[s]) - min(meds[s])
                res[s] = (med, spread)
                say("  %s %10.3f ms  spread %8.3f ms  medians %s" % (s, med, spread, " ".join("%.3f" % v for v in meds[s])))
            if args.method == "gram":
                out, ref = gram_path(q, b, k, excl, gws, norms), kernel_path(q, b, k, excl, ws)
                bits = torch.equal(out[0][0], ref[0]) and torch.equal(out[1][0].view(torch.int32), ref[1].view(torch.int32))
                t_norms = median_ms(lambda: _native.nn_norms(bv, N, 1, D, 1), min(calls, 20))
                gap, bar = res["kg_nn"][0] - res["kg_nn_gram"][0], 3 * max(res["kg_nn"][1], res["kg_nn_gram"][1])
                say("  kg_nn - kg_nn_gram = %+.3f ms against 3 x the larger spread %.3f ms: kg_nn_gram is %s (%.2f x); stats (certified, "
                    "fallback) = %s; bits equal to kg_nn: %s; kg_nn_norms of the base (once): %.3f ms"
                    % (gap, bar, "faster" if gap > bar else ("slower" if -gap > bar else "not separated"),
                       res["kg_nn"][0] / res["kg_nn_gram"][0], out[2][0, 0].tolist(), bits, t_norms))
                del gws, norms
            gap, bar = res["stock"][0] - res["kg_nn"][0], max(res["kg_nn"][1], res["stock"][1])
            say("  stock - kg_nn = %+.3f ms against the larger spread %.3f ms: kg_nn is %s; same nearest index for %d of %d queries"
                % (gap, bar, "faster" if gap > bar else ("slower" if -gap > bar else "not separated"), same, Q))
            del q, b, ws


if __name__ == "__main__":
    main()
