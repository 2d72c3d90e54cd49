#!/usr/bin/env python3
"""Cost of scoring the generator inside the training loop (record: profiles/eval_time.log).

NTU-60 shapes, 64 samples per iteration, a generator step in every iteration (n_critic = 1), a resident synthetic dataset -
the configuration of tools/time_train_loop.py and tools/time_ema.py.  One evaluation: 60 classes x 10 pairs, the live and
the averaged generator, both modes (four scores).

  1. the evaluation replay alone: event-timed, median over ``--replays`` replays, ``--reps`` repetitions with their spread;
     next to it its parts timed the same way - one 600-sample Sampler round and kg_mmd per mode - whose sum
     (2 rounds + 2 x 2 kg_mmd) is the comparator for what the re-layout and the two new launches add;
  2. the loop with eval_interval = 100 against the loop without: two captured loops (both with the weight average)
     alternate in one process, ``--rounds`` rounds of 300 iterations (three evaluations each); the difference per iteration
     next to the spread between rounds.  The loop without IS the off path: its figure is the one to hold against
     tools/time_train_loop.py's.

``--only-eval N``: N evaluation replays and nothing else (the run to put under a kernel trace).
``--prdc N`` (record: profiles/eval_prdc_time.log): instead of the above, the cost of scoring precision / recall /
density / coverage on N samples per class inside an evaluation, at the NTU shapes (60 classes) and the H36M shapes (10 classes),
live + ema, k = 5:
  a. the PRDC part as a graph of its own - ONE kg_prdc_sets over both generators' rounds with the real radii cached - against
     the same part built from one kg_prdc call per generator, alternating in one process: median of ``--replays`` event-timed
     replays, ``--reps`` repetitions, spread = max - min of the medians; "faster" only if the gap exceeds the larger spread;
  b. the whole evaluation replay with and without PRDC, and the Sampler round of classes x N samples alone with the device
     memory it holds (``--eval-replays`` replays each).
``--frechet N`` (record: profiles/eval_frechet_time.log): instead of the above, the cost of scoring the Frechet
pose and motion distance on N samples per class inside an evaluation, at the NTU and the H36M shapes, live + ema.  ONE
evaluation replay three ways - with Frechet through kg_frechet_sets (the real side cached), with the same columns composed
from one kg_frechet call per generator and mode (the real moments and the Jacobi solve of S_R repeated every time), and
without Frechet - alternating in one process: ``--rounds`` rounds, each the median of ``--eval-replays`` event-timed replays
per variant; spread = max - min of the medians; "faster" only if the gap exceeds the larger spread.
``--classifier P`` (record: profiles/eval_classifier_time.log): instead of the above, the cost of scoring accuracy,
feature Frechet distance, diversity and multimodality under an action classifier (untrained weights: the cost does not depend
on them) on P samples per class inside an evaluation, at the NTU and the H36M shapes, live + ema.  ONE evaluation replay
three ways - with the classifier columns (one kg_frechet_sets + one kg_cls_scores for both generators, the real side cached),
with the same columns composed from one ``metrics.classifier_scores`` call per generator (eager: it reads the host), and
without them - alternating in one process as under ``--frechet``; then kg_cls_scores alone as a graph of its own.
``--memorisation {features,raw}`` (record: profiles/eval_memorisation_time.log): instead of the above, the cost of
the authenticity / label agreement columns on ``--memorisation-samples`` samples per class inside an evaluation, at the NTU
shapes (a synthetic training set of 40000 samples) and the H36M shapes (4000), live + ema.  The evaluation replay with and
without the two columns per generator (feature space: both with the classifier columns, whose round is scored; raw space: a
round of its own) alternating in one process as under ``--frechet``; the same columns composed from one
``metrics.memorisation_features`` / ``memorisation`` call per generator on rounds already drawn (eager: it reads the host; the
leave-one-out distances given); then, each a graph of its own, kg_nn_sets over both generators against two kg_nn calls -
"faster" only if the gap exceeds the larger spread - and kg_nn_scores alone.
``--kinematics P`` (record: profiles/eval_kinematics_time.log): instead of the above, the cost of the six kinematic
W1 columns per generator on P samples per class inside an evaluation, at the NTU and the H36M shapes, live + ema.  ONE
evaluation replay three ways - with the columns (one kg_kin_desc_sets + one kg_kin_scores for both generators, the real
descriptors cached), with the same columns composed from one ``metrics.kinematics_sets`` call per generator (a kg_kin_desc and a
kg_kin_scores each), and without them - alternating in one process as under ``--frechet``; a difference is called real only
when it exceeds three times the larger spread.
``--all P`` (record: profiles/eval_refactor_time.log): instead of the above, ONE Evaluator with every family on
and P samples per class everywhere (memorisation in ``--memorisation`` space, default raw), live + ema, at the NTU and the H36M
shapes: how long its construction takes and what it leaves allocated on the device, then its evaluation replay, ``--rounds``
rounds of ``--eval-replays`` replays with their spread, and a checksum of the recorded bits.
    python tools/time_eval.py [--rounds 3] [--prdc 100 | --frechet 100 | --classifier 100 | --memorisation features |
                               --kinematics 100 | --all 100] [--log FILE]"""
import argparse
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd import metrics  # noqa: E402
from kinetic_gan_amd.evaluate import Evaluator  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.replay import capture  # noqa: E402
from kinetic_gan_amd.sample import Sampler  # noqa: E402
from kinetic_gan_amd.train import ResidentDataset, TrainLoop  # noqa: E402
from time_train_loop import BATCH, CFG, SyntheticFeeder, models, time_loop  # noqa: E402

DECAY, PAIRS, INTERVAL = 0.999, 10, 100


def time_replays(graph, n):
    """ms of each of n replays (one event pair per replay)"""
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


PRDC_SHAPES = (("NTU", dict(latent=512, channels=3, n_classes=60, t_size=64, mlp=4, v=25, dataset="ntu")),
               ("H36M", dict(latent=512, channels=2, n_classes=10, t_size=64, mlp=4, v=16, dataset="h36m")))


def toy_setup(c, per_class, dev):
    """(generators, real, labels): two generators of different weights (no training needed here) and a random real set of
    ``per_class`` samples per class"""
    K = c["n_classes"]
    gens = {}
    for g, seed in (("live", 1234), ("ema", 4321)):
        torch.manual_seed(seed)
        gens[g] = Generator(c["latent"], c["channels"], K, c["t_size"], c["mlp"], dataset=c["dataset"]).to(dev)
    rng = np.random.RandomState(0)
    real = torch.as_tensor((rng.rand(K * per_class, c["channels"], c["t_size"], c["v"]) * 2 - 1).astype(np.float32))
    return gens, real, np.tile(np.arange(K), per_class)


def time_alternating(graphs, rounds, replays, say, line=None, after=None, each=None):
    """{label: the median ms of ``replays`` replays, per round}: the graphs alternate within every round.  ``line``: the log
    line of one measurement (label, round, median, replays, min, max); ``after(label)``: called after a graph's replays;
    ``each(round)``: called at the end of a round"""
    meds = {k: [] for k in graphs}
    for r in range(rounds):
        for k, g in graphs.items():
            ts = time_replays(g, replays)
            if after:
                after(k)
            meds[k].append(statistics.median(ts))
            if line:
                say(line % (k + ",", r, meds[k][-1], replays, min(ts), max(ts)))
        if each:
            each(r)
    return meds


def time_evaluations(ev, rounds, replays, say, line=None, each=None):
    """``time_alternating`` over the evaluation replays of {label: Evaluator}, captured here; the host mirrors of the counters
    the replays advance are kept"""
    for x in ev.values():
        if x._graph is None:
            x.evaluate()                 # (captures)
    torch.cuda.synchronize()

    def after(k):                        # (time_replays: one replay to warm up, then the timed ones)
        ev[k].n_evals += replays + 1
        for s in ev[k]._all_samplers():
            s.step_count += replays + 1

    return time_alternating({k: x._graph for k, x in ev.items()}, rounds, replays, say, line, after, each)


def summary(meds):
    """({label: median of its rounds}, {label: spread = max - min of its rounds})"""
    return {k: statistics.median(v) for k, v in meds.items()}, {k: max(v) - min(v) for k, v in meds.items()}


def verdict(gap, wide, what, times=1):
    """``what`` is faster / slower only when the gap exceeds ``times`` x the larger spread"""
    if abs(gap) <= times * wide:
        return "not separated" + (" (within three spreads)" if times == 3 else "")
    return "%s is %s" % (what, "faster" if gap > 0 else "slower") + (" by more than three spreads" if times == 3 else "")


def same_records(a, b):
    """whether two Evaluators recorded the same bits"""
    return np.array_equal(a.records()["scores"].view(np.uint32), b.records()["scores"].view(np.uint32))


def prdc_part(args, say, dev):
    """``--prdc N``: see the module docstring"""
    N, K5 = args.prdc, 5
    for name, c in PRDC_SHAPES:
        K = c["n_classes"]
        gens, real, labels = toy_setup(c, N, dev)
        say("%s shapes: %d classes x %d samples per class, D = %d, live + ema, k = %d" % (
            name, K, N, c["channels"] * c["t_size"] * c["v"], K5))
        # b. the Sampler round of K x N samples alone, and what it holds
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated(dev)
        smp = {g: Sampler(G, qtd=N, seed=0) for g, G in gens.items()}
        outs = {g: s.next()[0] for g, s in smp.items()}
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated(dev)
        t_round = statistics.median(time_replays(smp["live"]._graph, args.eval_replays))
        say("%s Sampler round of %d samples alone: %.4f ms (median of %d replays); the two Samplers hold %.1f MB of device memory" % (
            name, K * N, t_round, args.eval_replays, (m1 - m0) / 1e6))
        # a. the PRDC part: one kg_prdc_sets with cached radii against one kg_prdc per generator
        ev = {"on": Evaluator(gens, real, labels, pairs=PAIRS, seed=0, prdc_per_class=N, prdc_k=K5),
              "off": Evaluator(gens, real, labels, pairs=PAIRS, seed=0)}
        e = ev["on"]
        o = outs["live"]
        _, C, T, V = o.shape
        sn, sc = o.stride(0), o.stride(1)
        rv = e._prdc_rv._replace(so=T * V)
        fv = {g: nv.PrdcView(t, sn, K * sn, sc) for g, t in outs.items()}
        ws1 = torch.empty(nv.prdc_workspace_bytes(N, N, C, T * V, K, K5) // 4, dtype=torch.int32, device=dev)
        graphs = {"kg_prdc_sets, cached real radii": capture(lambda: nv.prdc_sets(
                      rv, list(outs.values()), sn, K * sn, sc, e.prdc_radii, N, N, C, T * V, K, K5, ws=e._prdc_ws)),
                  "kg_prdc per generator": capture(lambda: [nv.prdc(rv, v, N, N, C, T * V, K, K5, ws=ws1) for v in fv.values()])}
        m, sp = summary(time_alternating(graphs, args.reps, args.replays, say, name + " PRDC part, %-34s repetition %d: median "
                                         "%.4f ms over %d replays (min %.4f, max %.4f)"))
        a, b = list(graphs)
        gap, wide = m[b] - m[a], max(sp.values())
        say("%s PRDC part: %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f); gap %+.4f ms against the larger spread %.4f ms: %s" % (
            name, a, m[a], sp[a], b, m[b], sp[b], gap, wide, verdict(gap, wide, "kg_prdc_sets")))
        # b. the whole evaluation replay with and without PRDC
        em = time_evaluations(ev, args.reps, args.eval_replays, say)
        say("%s evaluation replay (%d pairs per class, avg and joint): without PRDC %.4f ms (spread %.4f), with PRDC %.4f ms "
            "(spread %.4f): %+.4f ms (median of %d repetitions of %d replays)" % (
                name, PAIRS, statistics.median(em["off"]), max(em["off"]) - min(em["off"]), statistics.median(em["on"]),
                max(em["on"]) - min(em["on"]), statistics.median(em["on"]) - statistics.median(em["off"]), args.reps, args.eval_replays))
        rec = e.records()
        say("%s last recorded scores: %s" % (name, ", ".join("%s %.4f" % (n, v) for n, v in zip(rec["names"], rec["scores"][-1]))))
        del ev, e, graphs, smp, outs, fv, gens
        torch.cuda.empty_cache()


class ComposedFrechetEvaluator(Evaluator):
    """the Frechet columns as they would be without kg_frechet_sets: per generator and mode one kg_frechet call against the
    real samples themselves, its fp64 mean rounded to the fp32 word the record reads (the same bits, more work)"""

    def _frechet_scores(self):
        K, P = self.n_classes, self.frechet_per_class
        outs = []
        for k in self.gens:
            s = self.frechet_samplers[k]
            s._round()
            outs.append(s._out)
        _, C, T, V = outs[0].shape
        sn, sc = nv._sn_sc(outs[0])
        D = C * T * V
        rv = nv.FrechetView(self.frechet_real, P * D, D, V, T * V if C > 1 else 0)
        if getattr(self, "_composed_ws", None) is None:
            self._composed_ws = torch.empty(nv.frechet_workspace_bytes(P, P, T, True, C, V, K) // 8 + nv.frechet_workspace_bytes(
                P, P, T, False, C, V, K) // 8, dtype=torch.float64, device=self.device)
        scores = []
        for o in outs:
            fv = nv.FrechetView(o, sn, K * sn, V, sc if C > 1 else 0)
            for f in self.frechet_modes:
                res = nv.frechet(rv, fv, P, P, T, f == "motion", C, V, K, want_mean=True, ws=self._composed_ws)
                scores.append(res["mean"].to(torch.float32).reshape(1))
        return scores


def frechet_part(args, say, dev):
    """``--frechet N``: see the module docstring"""
    N = args.frechet
    for name, c in PRDC_SHAPES:
        K = c["n_classes"]
        gens, real, labels = toy_setup(c, N, dev)
        say("%s shapes: %d classes x %d samples per class of %d frames, d = %d, live + ema, pose and motion" % (
            name, K, N, c["t_size"], c["channels"] * c["v"]))
        ev = {"kg_frechet_sets, cached real side": Evaluator(gens, real, labels, pairs=PAIRS, seed=0, frechet_per_class=N),
              "kg_frechet per generator and mode": ComposedFrechetEvaluator(gens, real, labels, pairs=PAIRS, seed=0, frechet_per_class=N),
              "without Frechet": Evaluator(gens, real, labels, pairs=PAIRS, seed=0)}
        m, sp = summary(time_evaluations(ev, args.rounds, args.eval_replays, say, name + " evaluation replay, %-36s round %d: "
                                         "median %.4f ms over %d replays (min %.4f, max %.4f)"))
        a, b, off = list(ev)
        gap, wide = m[b] - m[a], max(sp[a], sp[b])
        say("%s evaluation replay: %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f)" % (
            name, a, m[a], sp[a], b, m[b], sp[b], off, m[off], sp[off]))
        say("%s Frechet columns cost %+.4f ms through kg_frechet_sets, %+.4f ms composed; gap %+.4f ms against the larger spread "
            "%.4f ms: %s" % (name, m[a] - m[off], m[b] - m[off], gap, wide, verdict(gap, wide, "kg_frechet_sets")))
        ra = ev[a].records()
        say("%s the two routes record the same bits: %s; last scores: %s" % (
            name, same_records(ev[a], ev[b]),
            ", ".join("%s %.6g" % (n, v) for n, v in zip(ra["names"], ra["scores"][-1]))))
        del ev, gens
        torch.cuda.empty_cache()


class ComposedKinematicsEvaluator(Evaluator):
    """the kinematic columns as they would be without kg_kin_desc_sets: per generator one ``metrics.kinematics_sets`` call on its
    round (one kg_kin_desc launch and one kg_kin_scores call each) against the cached real descriptors - the same bits, two
    launches more per further generator"""

    def _kinematics_scores(self):
        K, P = self.n_classes, self.kinematics_per_class
        labels = np.tile(np.arange(K), P)        # the Sampler's label vector: row j*K + c has class c (read in place)
        words = []
        for s in self.kin_samplers.values():
            s._round()
            res = metrics.kinematics_sets([s._out], self._kin_real_desc, labels, bones=self.kinematics_bones,
                                          mirror=self.kinematics_mirror, still_eps=self.kinematics_still_eps)
            words += [res["scores"][0, i:i + 1] for i in range(nv.KIN_DESC)]
        return words


def kinematics_part(args, say, dev):
    """``--kinematics P``: see the module docstring"""
    P = args.kinematics
    for name, c in PRDC_SHAPES:
        K = c["n_classes"]
        gens, real, labels = toy_setup(c, P, dev)
        say("%s shapes: %d classes x %d samples per class of %d frames, C %d, V %d, live + ema, six W1 columns per generator" % (
            name, K, P, c["t_size"], c["channels"], c["v"]))
        kw = dict(pairs=PAIRS, seed=0, kinematics_per_class=P, kinematics_dataset=c["dataset"])
        ev = {"kg_kin_desc_sets, cached real side": Evaluator(gens, real, labels, **kw),
              "metrics.kinematics_sets per generator": ComposedKinematicsEvaluator(gens, real, labels, **kw),
              "without the kinematic columns": Evaluator(gens, real, labels, pairs=PAIRS, seed=0)}
        m, sp = summary(time_evaluations(ev, args.rounds, args.eval_replays, say, name + " evaluation replay, %-38s round %d: "
                                         "median %.4f ms over %d replays (min %.4f, max %.4f)"))
        a, b, off = list(ev)
        gap, wide = m[b] - m[a], max(sp[a], sp[b])
        say("%s evaluation replay: %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f)" % (
            name, a, m[a], sp[a], b, m[b], sp[b], off, m[off], sp[off]))
        say("%s kinematic columns cost %+.4f ms through kg_kin_desc_sets, %+.4f ms composed; gap %+.4f ms against the larger spread "
            "%.4f ms (three times: %.4f ms): %s" % (name, m[a] - m[off], m[b] - m[off], gap, wide, 3 * wide,
                                                    verdict(gap, wide, "kg_kin_desc_sets", times=3)))
        ra = ev[a].records()
        say("%s the two routes record the same bits: %s; last kinematic scores: %s" % (
            name, same_records(ev[a], ev[b]),
            ", ".join("%s %.6g" % (n, v) for n, v in zip(ra["names"][-12:], ra["scores"][-1][-12:]))))
        del ev, gens
        torch.cuda.empty_cache()


def time_calls(fn, n):
    """ms of each of n eager calls of fn, host synchronisations of its own included (wall clock around a device sync)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def classifier_part(args, say, dev):
    """``--classifier P``: see the module docstring"""
    from kinetic_gan_amd.classifier import Classifier
    P = args.classifier
    for name, c in PRDC_SHAPES:
        K = c["n_classes"]
        gens, real, labels = toy_setup(c, P, dev)
        torch.manual_seed(99)
        clf = Classifier(c["channels"], K, c["t_size"], dataset=c["dataset"]).to(dev)
        sd, sl = min(200, K * P), min(20, P)
        say("%s shapes: %d classes x %d samples per class of %d frames, feat_dim %d, %d diversity pairs, %d multimodality pairs "
            "per class, live + ema" % (name, K, P, c["t_size"], clf.feat_dim, sd, sl))
        on = Evaluator(gens, real, labels, pairs=PAIRS, seed=0, classifier=clf, classifier_per_class=P, diversity_pairs=sd,
                       multimodality_pairs=sl)
        off = Evaluator(gens, real, labels, pairs=PAIRS, seed=0)
        ev = {"with the classifier columns": on, "without them": off}
        # the same columns from one metrics.classifier_scores call per generator, on rounds already drawn
        smp = {g: Sampler(G, qtd=P, seed=0) for g, G in gens.items()}
        outs = {g: s.next()[0] for g, s in smp.items()}
        lab_real = np.repeat(np.arange(K), P)
        real_dev = torch.as_tensor(on._select_real(real, labels, P, "classes", c["t_size"])).to(dev)

        def composed():
            return [metrics.classifier_scores(clf, o, labels, real_dev, lab_real, class_fd=False, diversity_pairs=sd,
                                              multimodality_pairs=sl) for o in outs.values()]

        t_round = statistics.median(time_replays(smp["live"]._graph, args.eval_replays))
        eager = []

        def each(r):
            ts = time_calls(composed, max(3, args.eval_replays // 3))
            eager.append(statistics.median(ts))
            say("%s metrics.classifier_scores per generator (2 calls, eager, real side recomputed), round %d: median %.4f ms over %d "
                "calls (min %.4f, max %.4f)" % (name, r, eager[-1], len(ts), min(ts), max(ts)))

        em = time_evaluations(ev, args.rounds, args.eval_replays, say, name + " evaluation replay, %-30s round %d: median %.4f ms "
                              "over %d replays (min %.4f, max %.4f)", each)
        m, sp = summary(dict(em, composed=eager))
        a, b = list(ev)
        say("%s evaluation replay: %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f): the classifier columns cost %+.4f ms; "
            "two Sampler rounds of %d samples are %.4f ms of that" % (name, a, m[a], sp[a], b, m[b], sp[b], m[a] - m[b], K * P,
                                                                     2 * t_round))
        say("%s the same columns from metrics.classifier_scores, one call per generator, without the rounds: %.4f ms (spread %.4f)" % (
            name, m["composed"], sp["composed"]))
        # kg_cls_scores alone
        feats, preds = list(on._cls_feat.values()), list(on._cls_pred.values())
        g = capture(lambda: nv.cls_scores(feats, preds, on._cls_labels, *on._cls_tables, K))
        meds = [statistics.median(time_replays(g, args.replays)) for _ in range(args.reps)]
        say("%s kg_cls_scores alone (2 sets, N = %d, F = %d, %d pairs; two launches): %.4f ms (median of %d repetitions of %d replays, "
            "spread %.4f)" % (name, K * P, clf.feat_dim, sd + K * sl, statistics.median(meds), args.reps, args.replays,
                              max(meds) - min(meds)))
        rec = on.records()
        say("%s last recorded scores: %s" % (name, ", ".join("%s %.6g" % (n, v) for n, v in zip(rec["names"], rec["scores"][-1]))))
        del ev, on, off, gens, smp, outs, clf, g, composed, real_dev
        torch.cuda.empty_cache()


MEM_TRAIN = {"NTU": 40000, "H36M": 4000}       # synthetic training-set sizes (tools/time_nn.py)


def toy_train(c, n, dev):
    """(samples on the device, labels): a random training set of n samples"""
    g = torch.Generator(device=dev).manual_seed(7)
    return torch.rand((n, c["channels"], c["t_size"], c["v"]), device=dev, generator=g) * 2 - 1, np.arange(n) % c["n_classes"]


def memorisation_part(args, say, dev):
    """``--memorisation {features,raw}``: see the module docstring"""
    from kinetic_gan_amd.classifier import Classifier
    mode, P = args.memorisation, args.memorisation_samples
    for name, c in PRDC_SHAPES:
        K, Nt = c["n_classes"], MEM_TRAIN[name]
        gens, real, labels = toy_setup(c, P, dev)
        train, lab_t = toy_train(c, Nt, dev)
        base = {}
        if mode == "features":
            torch.manual_seed(99)
            clf = Classifier(c["channels"], K, c["t_size"], dataset=c["dataset"]).to(dev)
            base = dict(classifier=clf, classifier_per_class=P, diversity_pairs=min(200, K * P), multimodality_pairs=min(20, P))
            mem = dict(memorisation="features")
        else:
            mem = dict(memorisation="raw", memorisation_per_class=P)
        on = Evaluator(gens, real, labels, pairs=PAIRS, seed=0, memorisation_train=train, memorisation_train_labels=lab_t, **base, **mem)
        off = Evaluator(gens, real, labels, pairs=PAIRS, seed=0, **base)
        d_outer, d_inner = on._mem_dims
        say("%s shapes, %s space: %d classes x %d samples per class against %d training samples, D = %d, live + ema%s" % (
            name, mode, K, P, Nt, d_outer * d_inner, "; both replays hold the classifier columns" if base else ""))
        ev = {"with the memorisation columns": on, "without them": off}
        if args.memorisation_method == "gram":
            # (record: profiles/eval_memorisation_gram_time.log) the same columns through kg_nn_gram: three
            # replays alternate - exact search, pre-filter, no memorisation columns - and the recorded scores must agree
            gram = Evaluator(gens, real, labels, pairs=PAIRS, seed=0, memorisation_train=train, memorisation_train_labels=lab_t,
                             memorisation_method="gram", **base, **mem)
            ev = {"with the memorisation columns": on, "with them through kg_nn_gram": gram, "without them": off}
        line = name + " evaluation replay, %-32s round %d: median %.4f ms over %d replays (min %.4f, max %.4f)"
        if args.memorisation_method == "gram":
            m, sp = summary(time_evaluations(ev, args.rounds, args.eval_replays, say, line))
            a, b, c_ = list(ev)
            say("%s evaluation replay: exact %.4f ms (spread %.4f), kg_nn_gram %.4f ms (spread %.4f), without the columns %.4f ms "
                "(spread %.4f): the columns cost %+.4f ms exact, %+.4f ms through the pre-filter" % (
                    name, m[a], sp[a], m[b], sp[b], m[c_], sp[c_], m[a] - m[c_], m[b] - m[c_]))
            ra, rb = on.records(), gram.records()
            same = np.array_equal(np.asarray(ra["scores"][0]), np.asarray(rb["scores"][0]))
            say("%s first recorded row equal in every column: %s; stats (certified, fallback) per generator of the last replay: %s; "
                "leave-one-out distances equal: %s" % (name, same, gram.memorisation_stats[:, 0].tolist(),
                                                        bool(torch.equal(on._mem_loo, gram._mem_loo))))
            del ev, on, off, gram, gens, train
            torch.cuda.empty_cache()
            continue
        # the same columns from one metrics call per generator, on rounds already drawn
        smp = {g: Sampler(G, qtd=P, seed=0) for g, G in gens.items()}
        outs = {g: s.next()[0] for g, s in smp.items()}
        if mode == "features":
            feats = list(on._cls_feat.values())
            tf = on.memorisation_train_features

            def composed():
                return [metrics.memorisation_features(f, labels, tf, lab_t, train_loo=on._mem_loo) for f in feats]
        else:
            def composed():
                return [metrics.memorisation(o, labels, train, lab_t, train_loo=on._mem_loo) for o in outs.values()]

        eager = []

        def each(r):
            ts = time_calls(composed, max(3, args.eval_replays // 3))
            eager.append(statistics.median(ts))
            say("%s metrics.memorisation%s per generator (2 calls, eager, train_loo given), round %d: median %.4f ms over %d calls "
                "(min %.4f, max %.4f)" % (name, "_features" if mode == "features" else "", r, eager[-1], len(ts), min(ts), max(ts)))

        em = time_evaluations(ev, args.rounds, args.eval_replays, say, line, each)
        m, sp = summary(dict(em, composed=eager))
        a, b = list(ev)
        say("%s evaluation replay: %s %.4f ms (spread %.4f), %s %.4f ms (spread %.4f): the memorisation columns cost %+.4f ms" % (
            name, a, m[a], sp[a], b, m[b], sp[b], m[a] - m[b]))
        say("%s the same columns composed from one metrics call per generator, without the rounds: %.4f ms (spread %.4f)" % (
            name, m["composed"], sp["composed"]))
        # kg_nn_sets over both generators against two kg_nn calls, then kg_nn_scores alone: graphs of their own
        n = K * P
        if mode == "features":
            qs, (q_sc, q_sp, q_so) = feats, on._mem_q
        else:
            qs = list(outs.values())
            sn, sc = nv._sn_sc(qs[0])
            q_sc, q_sp, q_so = 0, sn, (0 if d_outer == 1 else sc)
        bv, ba = on._mem_bv, on._mem_ba
        ws1 = torch.empty(nv.nn_workspace_bytes(n, Nt, d_outer, d_inner, 1, 1) // 4, dtype=torch.int32, device=dev)
        graphs = {"kg_nn_sets, both generators": capture(lambda: nv.nn_sets(qs, q_sc, q_sp, q_so, bv, n, Nt, d_outer, d_inner, 1, 1,
                                                                            b_affine=ba, ws=on._mem_ws)),
                  "kg_nn per generator": capture(lambda: [nv.nn(nv.PrdcView(q, q_sc, q_sp, q_so), bv, n, Nt, d_outer, d_inner, 1, 1,
                                                                b_affine=ba, ws=ws1) for q in qs])}
        replays = args.replays if mode == "features" else args.eval_replays
        gm, gs = summary(time_alternating(graphs, args.reps, replays, say, name + " search, %-30s repetition %d: median %.4f ms "
                                          "over %d replays (min %.4f, max %.4f)"))
        a, b = list(graphs)
        gap, wide = gm[b] - gm[a], max(gs.values())
        split = lambda f, *x: f(*x) // (x[0] * 8) if f is nv.nn_workspace_bytes else f(*x) // (x[0] * x[1] * 8)      # noqa: E731
        say("%s search: %s %.4f ms (spread %.4f; %d chunks), %s %.4f ms (spread %.4f; %d chunks each); gap %+.4f ms against the larger "
            "spread %.4f ms: %s (two launches instead of four either way)" % (
                name, a, gm[a], gs[a], split(nv.nn_sets_workspace_bytes, 2, n, Nt, d_outer, d_inner, 1, 1), b, gm[b], gs[b],
                split(nv.nn_workspace_bytes, n, Nt, d_outer, d_inner, 1, 1), gap, wide, verdict(gap, wide, "kg_nn_sets")))
        idx, d2 = nv.nn_sets(qs, q_sc, q_sp, q_so, bv, n, Nt, d_outer, d_inner, 1, 1, b_affine=ba, ws=on._mem_ws)
        g = capture(lambda: nv.nn_scores(idx, d2, on._mem_qlab, on._mem_blab, on._mem_loo, K))
        sm = [statistics.median(time_replays(g, args.replays)) for _ in range(args.reps)]
        say("%s kg_nn_scores alone (2 sets, Q = %d, N = %d; one launch): %.4f ms (median of %d repetitions of %d replays, spread %.4f)" % (
            name, n, Nt, statistics.median(sm), args.reps, args.replays, max(sm) - min(sm)))
        rec = on.records()
        say("%s last recorded scores: %s; the real side's own: authenticity %.4f, label_agreement %.4f" % (
            name, ", ".join("%s %.6g" % (n_, v) for n_, v in zip(rec["names"][-4:], rec["scores"][-1][-4:])),
            float(on.memorisation_real["authenticity"]), float(on.memorisation_real["label_agreement"])))
        del ev, on, off, gens, smp, outs, graphs, g, composed, train, qs, bv, idx, d2, ws1
        torch.cuda.empty_cache()


def all_part(args, say, dev):
    """``--all P``: see the module docstring"""
    from kinetic_gan_amd.classifier import Classifier
    P, mode = args.all, args.memorisation or "raw"
    for name, c in PRDC_SHAPES:
        K, Nt = c["n_classes"], MEM_TRAIN[name]
        gens, real, labels = toy_setup(c, P, dev)
        train, lab_t = toy_train(c, Nt, dev)
        torch.manual_seed(99)
        clf = Classifier(c["channels"], K, c["t_size"], dataset=c["dataset"]).to(dev)
        kw = dict(prdc_per_class=P, prdc_k=5, frechet_per_class=P, classifier=clf, classifier_per_class=P,
                  diversity_pairs=min(200, K * P), multimodality_pairs=min(20, P), memorisation=mode, memorisation_train=train,
                  memorisation_train_labels=lab_t, memorisation_per_class=P if mode == "raw" else 0, kinematics_per_class=P,
                  kinematics_dataset=c["dataset"])
        torch.cuda.synchronize()
        m0, t0 = torch.cuda.memory_allocated(dev), time.perf_counter()
        ev = Evaluator(gens, real, labels, pairs=PAIRS, seed=0, **kw)
        torch.cuda.synchronize()
        t1, m1 = time.perf_counter(), torch.cuda.memory_allocated(dev)
        say("%s shapes: every family on, %d classes x %d samples per class everywhere, memorisation in %s space against %d training "
            "samples, live + ema: %d columns, %d Samplers" % (name, K, P, mode, Nt, len(ev.names), len(ev._all_samplers())))
        say("%s construction (real side a host tensor): %.1f ms; it leaves %.1f MB allocated on the device" % (
            name, (t1 - t0) * 1e3, (m1 - m0) / 1e6))
        em = time_evaluations({"every family on": ev}, args.rounds, args.eval_replays, say, name + " evaluation replay, %-18s round %d: "
                              "median %.4f ms over %d replays (min %.4f, max %.4f)")
        m, sp = summary(em)
        rec = ev.records()
        say("%s evaluation replay, every family on: %.4f ms (median of %d rounds), spread between rounds %.4f ms; crc32 of the %d "
            "recorded rows: %08x" % (name, m["every family on"], args.rounds, sp["every family on"], len(rec["scores"]),
                                     zlib.crc32(rec["scores"].tobytes())))
        del ev, gens, train, clf
        torch.cuda.empty_cache()


def write_log(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--only-eval", type=int, default=0, help="this many evaluation replays and nothing else (for a kernel trace)")
    ap.add_argument("--prdc", type=int, default=0, help="samples per class: time the PRDC part of an evaluation instead (DESIGN.md 17)")
    ap.add_argument("--frechet", type=int, default=0,
                    help="samples per class: time the Frechet part of an evaluation instead (DESIGN.md 19)")
    ap.add_argument("--classifier", type=int, default=0,
                    help="samples per class: time the classifier columns of an evaluation instead (DESIGN.md 21)")
    ap.add_argument("--memorisation", type=str, default=None, choices=["features", "raw"],
                    help="time the memorisation columns of an evaluation in that space instead (DESIGN.md 23)")
    ap.add_argument("--memorisation-samples", type=int, default=100, help="samples per class of --memorisation")
    ap.add_argument("--memorisation_method", type=str, default="exact", choices=["exact", "gram"],
                    help="gram: time the memorisation columns through kg_nn_gram against the exact search (DESIGN.md 24)")
    ap.add_argument("--kinematics", type=int, default=0,
                    help="samples per class: time the kinematic columns of an evaluation instead (DESIGN.md 26)")
    ap.add_argument("--all", type=int, default=0,
                    help="samples per class: construct and time ONE Evaluator with every family on instead (DESIGN.md 27)")
    ap.add_argument("--eval-replays", type=int, default=30,
                    help="replays of a whole evaluation / a Sampler round under --prdc and --frechet")
    ap.add_argument("--log", default=None, help="also write the lines to this file")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.all or args.prdc or args.frechet or args.classifier or args.memorisation or args.kinematics:
        say("device %s" % torch.cuda.get_device_name(0))
        if args.all:
            all_part(args, say, dev)
        elif args.kinematics:
            kinematics_part(args, say, dev)
        elif args.memorisation:
            memorisation_part(args, say, dev)
        elif args.prdc:
            prdc_part(args, say, dev)
        elif args.classifier:
            classifier_part(args, say, dev)
        else:
            frechet_part(args, say, dev)
        return write_log(args.log, lines)
    feeder = SyntheticFeeder(64 * BATCH + 17, CFG["channels"], CFG["t_size"], CFG["v"], CFG["n_classes"])
    data = ResidentDataset(feeder, CFG["t_size"], dev)
    say("device %s; NTU-60 shapes, %d samples per iteration, a generator step in every iteration, %d resident samples; "
        "evaluation: %d classes x %d pairs, live and ema, avg and joint" % (
            torch.cuda.get_device_name(0), BATCH, len(feeder), CFG["n_classes"], PAIRS))
    loops = {}
    for name, kw in (("off", {}), ("on", dict(eval_interval=INTERVAL, eval_pairs=PAIRS))):
        G, D = models(dev)
        loops[name] = TrainLoop(G, D, data, BATCH, CFG["t_size"], n_critic=1, seed=0, ema_decay=DECAY, **kw)
    ev = loops["on"].evaluator
    for loop in loops.values():
        for _ in range(20):
            loop.step()
    ev.evaluate()                            # (captures)
    torch.cuda.synchronize()
    if args.only_eval:
        for _ in range(args.only_eval):
            ev.evaluate()
        torch.cuda.synchronize()
        say("%d evaluation replays done; %d copy jobs, snapshot of %d parameters" % (args.only_eval, len(ev._jobs), ev.snap_flat.numel()))
        return
    # 1. the evaluation replay alone, and its parts
    meds = time_evaluations({"evaluation replay": ev}, args.reps, args.replays, say,
                            "%s repetition %d: median %.4f ms over %d replays (min %.4f, max %.4f)")["evaluation replay"]
    say("evaluation replay: %.4f ms (median of %d repetitions), spread between repetitions %.4f ms" % (
        statistics.median(meds), args.reps, max(meds) - min(meds)))
    smp = Sampler(loops["on"].G, qtd=PAIRS, seed=0)
    smp.next()
    t_round = statistics.median(time_replays(smp._graph, args.replays))
    out, _, _ = smp.next()
    nchw = out.contiguous()
    parts = {}
    for mode in ev.modes:
        g = capture(lambda: metrics.calculate_mmd(nchw, ev.real, ev._pair_labels, mode))
        parts[mode] = statistics.median(time_replays(g, args.replays))
    g = capture(lambda: nchw.copy_(out))
    t_copy = statistics.median(time_replays(g, args.replays))
    total = 2 * t_round + 2 * sum(parts.values())
    say("parts, each a graph of its own: Sampler round of %d samples %.4f ms; kg_mmd %s; re-layout copy_ %.4f ms" % (
        smp.n, t_round, ", ".join("%s %.4f ms" % kv for kv in parts.items()), t_copy))
    say("comparator 2 rounds + 2 x (%s) = %.4f ms; the evaluation replay is %+.4f ms against it (2 re-layouts, kg_eval_record, "
        "kg_copy_if over %d jobs / %.1f MB)" % (" + ".join(parts), total, statistics.median(meds) - total, len(ev._jobs),
                                               4 * ev.snap_flat.numel() / 1e6))
    # 2. the loop with evaluation against the loop without
    label = {"off": "loop without evaluation (the off path)", "on": "loop with eval_interval=%d" % INTERVAL}
    lm = {k: [] for k in loops}
    for r in range(args.rounds):
        for k, loop in loops.items():
            med, lo, hi, ms = time_loop(loop, blocks=30, per_block=10, warmup=5)
            lm[k].append(statistics.mean(ms))
            say("round %d %-42s mean %.4f ms per iteration over 300 replays (median of blocks of 10 %.4f, min %.4f, max %.4f)" % (
                r, label[k], lm[k][-1], med, lo, hi))
    for loop in loops.values():
        d, g_ = loop.losses()
        assert np.isfinite(d).all() and np.isfinite(g_).all(), "the timed loop diverged"
    m = {k: statistics.median(v) for k, v in lm.items()}
    sp = {k: max(v) - min(v) for k, v in lm.items()}
    for k in loops:
        say("%-42s %.4f ms per iteration (median of %d rounds), spread between rounds %.4f ms" % (label[k], m[k], args.rounds, sp[k]))
    say("on - off = %+.2f us per iteration (one evaluation per %d iterations: %.4f ms / %d = %.2f us expected); larger spread %.2f us" % (
        (m["on"] - m["off"]) * 1e3, INTERVAL, statistics.median(meds), INTERVAL, statistics.median(meds) / INTERVAL * 1e3,
        max(sp.values()) * 1e3))
    same = torch.equal(loops["on"].trainer.fG.flat, loops["off"].trainer.fG.flat)
    rec = ev.records()
    b = ev.best()
    say("generator weights of the two loops after %d iterations equal: %s; %d evaluations recorded, best %s %.6f at iteration %d" % (
        loops["on"].step_count, same, len(rec["iteration"]), ev.select, b["value"], b["iteration"]))
    write_log(args.log, lines)


if __name__ == "__main__":
    main()
